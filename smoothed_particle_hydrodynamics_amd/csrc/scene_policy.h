// Decisions of the scene renderer (scene_kernels.h, sph_hip_render_scene): where a pixel's ray meets the
// context's solids, what such a pixel is given, and the argument checks.  One set of inline functions
// for the device (k_scene_solids) and for g++ (tests/test_scene_cpu.py, against the numpy restatement
// tests/scene_emulation.py).  include/sph_hip.h states the contract operation by operation ("scene
// renderer"); all arithmetic is fp32, unfused, in the order written, with sqrtf, "/" and C99
// fminf / fmaxf only.  Pure C++17 without HIP.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/sph_hip.h"
#include "obstacle_policy.h"
#include "render_policy.h"

#define SCENE_FLAGS SPH_HIP_RENDER_VELOCITY

// One solid as the device reads it: the obstacle as it stands now, its velocity and its albedo.
struct SceneSolid {   // 72 bytes
   sph_hip_obstacle o;
   float vel[3];
   float alb[3];
};

// Why the arguments are refused, or nullptr.  (The context checks - FULL, whole grid - are the sampler's
// and come first; camera, params and size are render_check's.)
inline const char* scene_check(const sph_hip_camera* cam, const sph_hip_render_params* rp,
                               const sph_hip_scene_params* sp, const float* solid_albedo_rgb, int n_albedo,
                               int n_obstacles, int width, int height, int flags)
{
   if (!sp) return "null scene params";
   if (flags & ~SCENE_FLAGS) return "flag bits other than SPH_HIP_RENDER_VELOCITY";
   if (const char* why = render_check(cam, rp, width, height, flags)) return why;
   for (int c = 0; c < 3; c++)
      if (!isfinite(sp->albedo[c])) return "scene params must be finite";
   if (!isfinite(sp->ambient) || !isfinite(sp->diffuse)) return "scene params must be finite";
   if (n_albedo != 0 && n_albedo != n_obstacles) return "the albedo count must be 0 or the obstacle count";
   if (n_albedo > 0 && !solid_albedo_rgb) return "null albedo array";
   for (int i = 0; i < 3 * n_albedo; i++)
      if (!isfinite(solid_albedo_rgb[i])) return "a solid's albedo must be finite";
   return nullptr;
}

// device scratch this pass adds per row chunk: one int32 of solid_id per pixel, in a buffer of its own
inline long long scene_id_bytes(int width, int rows) { return round256((long long)width * rows * 4); }

// A solid's velocity at the motion clock tau: its motion's while the clamp of obstacle_motion_s lets
// tau through (start <= tau < stop: the shift grows during a step taken now), else 0.
inline void scene_motion_velocity(const sph_hip_obstacle_motion& m, float tau, float v[3])
{
   const bool on = obstacle_moves(m) && tau >= m.start && tau < m.stop;
   for (int c = 0; c < 3; c++) v[c] = on ? m.velocity[c] : 0.0f;
}

// The pixel's normalised direction, formed as the renderer forms it; false where len is 0 or not finite.
RENDER_HD inline bool scene_pixel_dir(const sph_hip_camera& cam, int width, int height, int px, int py, float d[3])
{
   const float a = (float)(2 * px + 1 - width) / (float)width;
   const float b = (float)(height - 2 * py - 1) / (float)height;
   float dc[3];
   for (int c = 0; c < 3; c++) dc[c] = (cam.forward[c] + a * cam.right[c]) + b * cam.up[c];
   const float len = sqrtf((dc[0] * dc[0] + dc[1] * dc[1]) + dc[2] * dc[2]);
   if (!(len > 0.0f) || !isfinite(len)) return false;
   for (int c = 0; c < 3; c++) d[c] = dc[c] / len;
   return true;
}

// one axis' slab, as the renderer's box: the lower and upper bound of the ray parameter
RENDER_HD inline void scene_slab(float eye, float d, float lo, float hi, float& tn, float& tf)
{
   const float inv = 1.0f / d;
   const float t0 = (lo - eye) * inv;
   const float t1 = (hi - eye) * inv;
   tn = fminf(t0, t1);
   tf = fmaxf(t0, t1);
}

// the entry parameter of an interval that starts at t0 >= 0 (a -0 becomes +0)
RENDER_HD inline float scene_entry(float t0) { return fmaxf(t0, 0.0f) + 0.0f; }

// the rules every kind shares, once [t0, t1] is known: false for a miss; inside: t = 0 and n = -d
RENDER_HD inline bool scene_interval(float t0, float t1, const float d[3], float& t, float n[3], bool& inside)
{
   if (!(t0 <= t1) || !(t1 >= 0.0f)) return false;
   inside = t0 < 0.0f;
   if (inside) {
      t = 0.0f;
      for (int c = 0; c < 3; c++) n[c] = -d[c];
   } else {
      t = scene_entry(t0);
   }
   return true;
}

RENDER_HD inline bool scene_hit_sphere(const sph_hip_obstacle& o, const float eye[3], const float d[3], float& t,
                                       float n[3])
{
   const float r = o.radius;
   const float ox = eye[0] - o.center[0], oy = eye[1] - o.center[1], oz = eye[2] - o.center[2];
   const float b = (ox * d[0] + oy * d[1]) + oz * d[2];
   const float c = ((ox * ox + oy * oy) + oz * oz) - r * r;
   const float disc = b * b - c;
   if (!(disc >= 0.0f)) return false;
   const float s = sqrtf(disc);
   const float t0 = -b - s, t1 = -b + s;
   bool inside;
   if (!scene_interval(t0, t1, d, t, n, inside)) return false;
   if (!inside)
      for (int a = 0; a < 3; a++) n[a] = ((eye[a] + t * d[a]) - o.center[a]) / r;
   return true;
}

RENDER_HD inline bool scene_hit_box(const sph_hip_obstacle& o, const float eye[3], const float d[3], float& t,
                                    float n[3])
{
   float nr[3], fr[3];
   for (int a = 0; a < 3; a++) scene_slab(eye[a], d[a], o.lo[a], o.hi[a], nr[a], fr[a]);
   const float t0 = fmaxf(fmaxf(nr[0], nr[1]), nr[2]);
   const float t1 = fminf(fminf(fr[0], fr[1]), fr[2]);
   bool inside;
   if (!scene_interval(t0, t1, d, t, n, inside)) return false;
   if (!inside) {
      const int ax = nr[0] == t0 ? 0 : nr[1] == t0 ? 1 : 2;   // the first axis that supplied t0
      const float da = ax == 0 ? d[0] : ax == 1 ? d[1] : d[2];
      const float s = da > 0.0f ? -1.0f : 1.0f;
      for (int a = 0; a < 3; a++) n[a] = a == ax ? s : 0.0f;
   }
   return true;
}

// the box cut by the plane n.x < off (n = center, off = radius): the box's interval narrowed by the plane's
RENDER_HD inline bool scene_hit_wedge(const sph_hip_obstacle& o, const float eye[3], const float d[3], float& t,
                                      float n[3])
{
   float nr[3], fr[3];
   for (int a = 0; a < 3; a++) scene_slab(eye[a], d[a], o.lo[a], o.hi[a], nr[a], fr[a]);
   const float b0 = fmaxf(fmaxf(nr[0], nr[1]), nr[2]);
   const float b1 = fminf(fminf(fr[0], fr[1]), fr[2]);
   const float g = obstacle_plane_dot(o, d);
   const float f = obstacle_plane_dot(o, eye) - o.radius;
   float near_p = -INFINITY, far_p = INFINITY;
   if (g < 0.0f) {
      near_p = (-f) / g;
   } else if (g > 0.0f) {
      far_p = (-f) / g;
   } else if (!(f < 0.0f)) {
      return false;
   }
   const float t0 = fmaxf(b0, near_p);
   const float t1 = fminf(b1, far_p);
   bool inside;
   if (!scene_interval(t0, t1, d, t, n, inside)) return false;
   if (!inside) {
      if (t0 == b0) {   // a box face wins a tie with the cut face
         const int ax = nr[0] == t0 ? 0 : nr[1] == t0 ? 1 : 2;
         const float da = ax == 0 ? d[0] : ax == 1 ? d[1] : d[2];
         const float s = da > 0.0f ? -1.0f : 1.0f;
         for (int a = 0; a < 3; a++) n[a] = a == ax ? s : 0.0f;
      } else {
         for (int a = 0; a < 3; a++) n[a] = o.center[a];
      }
   }
   return true;
}

// cylinder about axis A (a compile-time axis keeps every index into eye, d and n a constant)
template <int A>
RENDER_HD inline bool scene_hit_cylinder_axis(const sph_hip_obstacle& o, const float eye[3], const float d[3],
                                              float& t, float n[3])
{
   constexpr int U = (A + 1) % 3, W = (A + 2) % 3;
   const float r = o.radius;
   const float ou = eye[U] - o.center[U], ow = eye[W] - o.center[W];
   const float qa = d[U] * d[U] + d[W] * d[W];
   float s0, s1;
   if (qa == 0.0f) {   // parallel to the axis: everything, or nothing
      if (!(ou * ou + ow * ow < r * r)) return false;
      s0 = -INFINITY;
      s1 = INFINITY;
   } else {
      const float b = ou * d[U] + ow * d[W];
      const float c = (ou * ou + ow * ow) - r * r;
      const float disc = b * b - qa * c;
      if (!(disc >= 0.0f)) return false;
      const float s = sqrtf(disc);
      s0 = (-b - s) / qa;
      s1 = (-b + s) / qa;
   }
   float c0, c1;
   scene_slab(eye[A], d[A], o.lo[A], o.hi[A], c0, c1);
   const bool side = s0 >= c0;   // on equal bounds the side wins
   const float t0 = side ? s0 : c0;
   const float t1 = fminf(s1, c1);
   bool inside;
   if (!scene_interval(t0, t1, d, t, n, inside)) return false;
   if (!inside) {
      if (side) {
         n[U] = ((eye[U] + t * d[U]) - o.center[U]) / r;
         n[W] = ((eye[W] + t * d[W]) - o.center[W]) / r;
         n[A] = 0.0f;
      } else {
         n[U] = 0.0f;
         n[W] = 0.0f;
         n[A] = d[A] > 0.0f ? -1.0f : 1.0f;
      }
   }
   return true;
}

// Where the ray eye + t * d (d normalised) enters solid o, and the outward unit normal there.
RENDER_HD inline bool scene_hit(const sph_hip_obstacle& o, const float eye[3], const float d[3], float& t, float n[3])
{
   if (o.kind == SPH_HIP_OBSTACLE_SPHERE) return scene_hit_sphere(o, eye, d, t, n);
   if (o.kind == SPH_HIP_OBSTACLE_BOX) return scene_hit_box(o, eye, d, t, n);
   if (o.kind == SPH_HIP_OBSTACLE_WEDGE) return scene_hit_wedge(o, eye, d, t, n);
   if (o.axis == 0) return scene_hit_cylinder_axis<0>(o, eye, d, t, n);
   if (o.axis == 1) return scene_hit_cylinder_axis<1>(o, eye, d, t, n);
   return scene_hit_cylinder_axis<2>(o, eye, d, t, n);
}

// The nearest of the list's solids along the ray: list order, strict <, so the lower index wins a tie.
// `obstacle(i)` gives solid i (a plain list on the host, the LDS copy on the device).
template <class List>
RENDER_HD inline bool scene_nearest_of(const List& obstacle, int count, const float eye[3], const float d[3],
                                       float& t, float n[3], int& id)
{
   id = -1;
   t = INFINITY;
   for (int i = 0; i < count; i++) {
      float ti, ni[3];
      if (scene_hit(obstacle(i), eye, d, ti, ni) && ti < t) {
         t = ti;
         id = i;
         for (int c = 0; c < 3; c++) n[c] = ni[c];
      }
   }
   return id >= 0;
}

struct SceneObstacleList {
   const sph_hip_obstacle* list;
   RENDER_HD const sph_hip_obstacle& operator()(int i) const { return list[i]; }
};

RENDER_HD inline bool scene_nearest(const sph_hip_obstacle* list, int count, const float eye[3], const float d[3],
                                    float& t, float n[3], int& id)
{
   return scene_nearest_of(SceneObstacleList{list}, count, eye, d, t, n, id);
}

// Lambert shading of a solid pixel: the renderer's formula with the solid's albedo and the scene's
// ambient / diffuse; the light is the render params'.
RENDER_HD inline uint32_t scene_shade(const float n[3], const float light[3], const float albedo[3], float ambient,
                                      float diffuse)
{
   const float llen = sqrtf((light[0] * light[0] + light[1] * light[1]) + light[2] * light[2]);
   const float l[3] = {light[0] / llen, light[1] / llen, light[2] / llen};
   const float ndl = (n[0] * l[0] + n[1] * l[1]) + n[2] * l[2];
   const float w = ambient + diffuse * fmaxf(ndl, 0.0f);
   uint32_t rgba = 255u << 24;
   for (int c = 0; c < 3; c++) rgba |= (uint32_t)render_byte(albedo[c] * w) << (8 * c);
   return rgba;
}

// composite: the solid takes the pixel when it lies strictly in front of the fluid
RENDER_HD inline bool scene_in_front(float t_solid, float depth_fluid) { return t_solid < depth_fluid; }
