// Static analytic obstacles (include/sph_hip.h: sph_hip_set_obstacles): the argument checks and the
// per-particle collision response, one inline function for the device (k_integrate_obst,
// k_slab_pack_early_obst: common_kernels.h, slab_kernels.h) and for g++ (tests/test_obstacles_cpu.py,
// against the numpy restatement tests/obstacle_emulation.py).
// Pure C++17 without HIP; the translation units that use it are compiled with -ffp-contract=off.
//
// The contract, operation by operation.  All arithmetic is fp32, unfused, in the order written
// ("a + b + c" is (a + b) + c); sqrtf and "/" are correctly rounded.  Obstacle i of the list sees the
// v, q the obstacle before it left; p is never updated.
//   inputs     p: the particle's position before the step; v, q: its velocity and position after
//              the drift, the kick and the wall handling (apply_walls); dt = time_step; damping.
//   inside     (strict) sphere: d = q - center, (dx*dx + dy*dy) + dz*dz < r*r.
//              box: lo[a] < q[a] < hi[a] on every axis a.
//              cylinder (axis a, u = (a+1)%3, w = (a+2)%3): lo[a] < q[a] < hi[a] and
//              du*du + dw*dw < r*r with d = q - center.
//              wedge (the box cut by a plane: n = center, d = radius, axis ignored): the box's test and
//              (n0*q0 + n1*q1) + n2*q2 < d.  Every n.x below is formed like this one.
//              A particle that is not inside is left untouched, bit for bit.
//   entry      along the line p + v*s:
//              box: for every axis with v[a] != 0, t_a = ((v[a] > 0 ? lo[a] : hi[a]) - p[a]) / v[a]
//              and x_a = ((v[a] > 0 ? hi[a] : lo[a]) - p[a]) / v[a]; an axis with v[a] == 0 misses
//              unless lo[a] < p[a] < hi[a].  t = the largest t_a (ties: the lowest axis),
//              t_exit = the smallest x_a; n = -sign(v[a]) e_a of the axis that gave t.
//              sphere: d0 = p - center, A = (vx*vx + vy*vy) + vz*vz, B = (d0x*vx + d0y*vy) + d0z*vz,
//              C = ((d0x*d0x + d0y*d0y) + d0z*d0z) - r*r, D = B*B - A*C; the line misses unless
//              D > 0; s = sqrtf(D), t = (-B - s) / A, t_exit = (-B + s) / A;
//              n = (inter - center) / r per component.
//              cylinder: cap slab as the box on axis a (tc0, tc1; v[a] == 0: -inf, +inf when
//              lo[a] < p[a] < hi[a], else a miss); circle in (u, w): A = vu*vu + vw*vw,
//              B = d0u*vu + d0w*vw, C = (d0u*d0u + d0w*d0w) - r*r, D = B*B - A*C, a miss unless
//              D > 0, tr0 = (-B - s) / A, tr1 = (-B + s) / A with s = sqrtf(D) (A == 0: -inf, +inf
//              when d0u*d0u + d0w*d0w < r*r, else a miss).  t = the later of tc0 and tr0, the cap
//              on a tie; t_exit = the smaller of tc1 and tr1.  n: the cap's -sign(v[a]) e_a, or the
//              side's (inter_u - center_u) / r, (inter_w - center_w) / r with n_a = 0.
//              wedge: the box's three slabs with the box's ties give t, t_exit and the axis; then the
//              plane: g = n.v, f = (n.p) - d.  g == 0: a miss unless f < 0.  g < 0: s_pl = (-f) / g is an
//              entry candidate and replaces t only when s_pl > t (a box face wins a tie); otherwise
//              (g > 0) s_pl = (-f) / g is an exit candidate and replaces t_exit only when s_pl < t_exit.
//              n: the slab's -sign(v[a]) e_a, or the plane's n = center as stored.
//              The entry is valid only when p is not inside, v != 0, the line meets the obstacle
//              and 0 <= t < t_exit.
//   response   (a valid entry: SPH::applyBoundary, reference src/sph.cpp:1124-1148, as coded)
//              inter = p + v*t; dot = (v0*n0 + v1*n1) + v2*n2; refl = v - (n*dot)*2;
//              remaining = dt - t if dt - t > 0, else 0 (the wall lets it go negative);
//              v = refl; q = inter + refl*(remaining*damping), per component.
//   fallback   (no valid entry) q moves to the nearest surface point, n is the outward normal there:
//              sphere: d = q - center, len = sqrtf((dx*dx + dy*dy) + dz*dz), n = d / len per
//              component (len == 0: n = +x), q = center + n*r.
//              box: the face with the smallest distance q[a] - lo[a] (n = -e_a, q[a] = lo[a]) or
//              hi[a] - q[a] (n = +e_a, q[a] = hi[a]); ties: the lowest axis, lo before hi.
//              cylinder: candidates in the order lo cap (q[a] - lo[a]), hi cap (hi[a] - q[a]), side
//              (r - len, len = sqrtf(du*du + dw*dw)); the first smallest wins.  A cap sets q[a] to
//              its plane; the side sets q_u = center_u + n_u*r, q_w = center_w + n_w*r with
//              n = (du / len, dw / len) (len == 0: n = e_u).
//              wedge: the box's six candidates in the box's order, then the plane's dpl = d - n.q; the
//              first smallest wins.  A box face as the box; the plane sets q_c = q_c + n_c*dpl per
//              component with the normal n = center.
//              dot = (v0*n0 + v1*n1) + v2*n2, m = dot if dot < 0 else 0, v = v - n*(m*2) per
//              component: only an inward component is reflected, without damping.
// The result is not strictly inside the obstacle except by the rounding of the last formula applied
// (the sphere's and the side's q are rounded once per component from an exact surface point).
//
// Moving obstacles (include/sph_hip.h: sph_hip_set_obstacle_motion; k_integrate_obst_moving,
// k_integrate_loads_moving, k_slab_pack_early_obst_moving; tests/test_moving_obstacles_cpu.py against
// tests/moving_obstacle_emulation.py).  Entry i of the motion list belongs to obstacle i; tau is the
// context's motion clock, tau0 at the start of the step and tau1 = tau0 + dt at its end (fp32 add).
//   moves      any velocity[c] != 0.  An entry that does not move is used untouched and responds as
//              above (no "+ 0": a -0 field keeps its sign).
//   shift      s(tau) = (tau < start ? start : tau > stop ? stop : tau) - start;
//              D_c(tau) = velocity[c] * s(tau); the obstacle at tau is the list entry with D_c added to
//              center[c], lo[c] and hi[c] on all three axes, the unused fields included.  A wedge's
//              center holds its normal and stays untouched: lo[c] and hi[c] get D_c and
//              radius = radius + ((n0*D0 + n1*D1) + n2*D2).
//   response   D0 = D(tau0), D1 = D(tau1), o1 = the obstacle at tau1.  q not strictly inside o1: the
//              particle is untouched, bit for bit.  d_c = D1_c - D0_c.  All three d_c == 0 (not started,
//              stopped, dt == 0): the response above with o1; nothing is divided.  Otherwise
//              ue_c = d_c / dt, pr_c = p_c + d_c, w_c = v_c - ue_c; the response above with
//              (o1, pr, w, q); then v_c = w_c + ue_c.  This is the static response in the frame that
//              moves with the solid and coincides with the world at the end of the step: a solid moving
//              at u into a particle at rest leaves it at 2u along the normal.
// Obstacles act in list order, moving or not, each on the v, q the one before it left.
//
// Oriented and rotating obstacles: the contract only (tests/test_rotating_obstacles_cpu.py against
// tests/rotating_obstacle_emulation.py).  No entry point of include/sph_hip.h takes a rotation list and no
// kernel calls these functions yet - DESIGN.md section 20 says why - so sph_hip_obstacle_rotation is
// declared below, not in the public header.
// Entry i of the rotation list belongs to obstacle i.  a = axis, u = (a+1)%3, w = (a+2)%3.
//   posed      angle != 0 || rate != 0; rotates: rate != 0.  An entry that is not posed takes exactly the
//              turn above (static, or obstacle_turn with its motion): nothing is added to it or rotated by
//              zero.
//   angle      theta(tau) = angle + rate * s(tau), s the clamp above with the rotation's start and stop.
//   sincos     obstacle_sincos(theta, cs, sn): k = rintf(theta * 2/pi); r = ((theta - k*P1) - k*P2) - k*P3
//              (P1 + P2 + P3 = pi/2: P1 has 8 significant bits, P2 11, so both products are exact up to
//              |theta| = 8192); z = r*r; s = ((S3*z + S2)*z + S1), s = (s*z)*r + r;
//              c = ((C3*z + C2)*z + C1), c = ((c*z)*z - 0.5*z) + 1; quadrant k & 3 (two's complement):
//              0: (c, s), 1: (-s, c), 2: (-c, -s), 3: (s, -c) for (cs, sn).  No libm call: numpy float32
//              operations restate it exactly.
//   frames     to_body(cs, sn, x): y_a = x_a; du = x_u - pivot_u, dw = x_w - pivot_w;
//              y_u = pivot_u + (cs*du + sn*dw); y_w = pivot_w + (cs*dw - sn*du).
//              to_world(cs, sn, y): du, dw from y; x_u = pivot_u + (cs*du - sn*dw);
//              x_w = pivot_w + (sn*du + cs*dw).  vec_to_body / vec_to_world: the same without the pivot.
//   response   (cs0, sn0) at theta(tau0), (cs1, sn1) at theta(tau1), o the list entry as set.
//              q1 = to_body(1, q); q1 not strictly inside o: the particle is untouched, bit for bit.
//              p0 = to_body(0, p).  theta(tau1) == theta(tau0) (tilted at rest, not started, stopped,
//              dt == 0): w = vec_to_body(1, v); the response above with (o, p0, w, q1);
//              v = vec_to_world(1, w); q = to_world(1, q1); nothing is divided.  Otherwise
//              pc = to_world(1, p0) - where the solid's material point at p ends up -, d = pc - p,
//              ue = d / dt, wv = v - ue, w = vec_to_body(1, wv); the same response; wv = vec_to_world(1, w),
//              v = wv + ue, q = to_world(1, q1).  The static response in the frame fixed to the solid that
//              coincides with the world at the end of the step, with a per-particle displacement: a face
//              moving at omega * r into fluid at rest leaves it at 2 * omega * r along the normal.
//   excluded   a posed entry on an obstacle whose motion moves; posed entries and free bodies in one list.
//
// Motion paths (include/sph_hip.h: sph_hip_set_obstacle_paths; k_paths_eval, k_integrate_obst_path,
// k_integrate_loads_path; tests/test_paths_cpu.py against tests/path_emulation.py).  Path i belongs to
// obstacle i; count == 0: no path, otherwise its keys (t, d[3]) are keys[first .. first + count).
//   time       T = t[count-1]; u = tau - start; u < 0: u = 0.  cycle == 0: u > T: u = T.  cycle != 0:
//              if u >= T then k = floorf(u / T), u = u - k * T; after that u < 0: u = 0, u >= T: u = 0.
//              clamped: the first u was < 0, or cycle == 0 and it was > T.
//   segment    j: the largest index in [0, count-2] with t[j] <= u (t[0] == 0 <= u always).
//   shift      w = (u - t[j]) / (t[j+1] - t[j]); D_c(tau) = d[j][c] + w * (d[j+1][c] - d[j][c]): one
//              function, path_displacement, for the device's k_paths_eval and the host.  The obstacle
//              at tau is obstacle_shifted(o, D); an entry with a path is always shifted ("+ 0" included).
//   velocity   (d[j+1][c] - d[j][c]) / (t[j+1] - t[j]) of that segment, 0 while clamped.
//   turn       D0 = D(tau0), D1 = D(tau1) (PathShift, formed once per obstacle and step), o1 =
//              obstacle_shifted(o, D1), then obstacle_respond_moved(o1, D0, D1, ...) as it is; the return
//              value is "q strictly inside o1".  An entry without a path takes exactly the turn it takes
//              without paths: static, or obstacle_turn with its motion.
//   excluded   a path on an obstacle whose motion moves; any path in a list that holds a free body
//              (body_policy.h: path_body_check); slab contexts; rotations stay withdrawn.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/sph_hip.h"

#ifdef __HIPCC__
#define OBST_HD __host__ __device__
#else
#define OBST_HD
#endif

// Why a list is refused, or nullptr.  Every float field of every entry must be finite, the unused
// ones included.
inline const char* obstacle_check(const sph_hip_obstacle* list, int n)
{
   if (n < 0 || n > SPH_HIP_MAX_OBSTACLES) return "the obstacle count must be in [0, 64]";
   if (n > 0 && !list) return "null obstacle list";
   for (int i = 0; i < n; i++) {
      const sph_hip_obstacle& o = list[i];
      if (o.kind != SPH_HIP_OBSTACLE_SPHERE && o.kind != SPH_HIP_OBSTACLE_BOX && o.kind != SPH_HIP_OBSTACLE_CYLINDER &&
          o.kind != SPH_HIP_OBSTACLE_WEDGE)
         return "unknown obstacle kind";
      bool finite = isfinite(o.radius);
      for (int a = 0; a < 3; a++) finite = finite && isfinite(o.center[a]) && isfinite(o.lo[a]) && isfinite(o.hi[a]);
      if (!finite) return "obstacle fields must be finite";
      if (o.kind == SPH_HIP_OBSTACLE_SPHERE) {
         if (!(o.radius > 0.0f)) return "a sphere's radius must be > 0";
      } else if (o.kind == SPH_HIP_OBSTACLE_BOX) {
         for (int a = 0; a < 3; a++)
            if (!(o.lo[a] < o.hi[a])) return "a box needs lo < hi on every axis";
      } else if (o.kind == SPH_HIP_OBSTACLE_WEDGE) {
         for (int a = 0; a < 3; a++)
            if (!(o.lo[a] < o.hi[a])) return "a wedge needs lo < hi on every axis";
         const double n0 = o.center[0], n1 = o.center[1], n2 = o.center[2];
         if (!(fabs(((n0 * n0 + n1 * n1) + n2 * n2) - 1.0) <= 0x1p-20)) return "a wedge's normal must have unit length";
         bool some = false;   // a corner of the box on the solid's side of the plane
         for (int k = 0; k < 8; k++) {
            const double c0 = k & 1 ? o.hi[0] : o.lo[0], c1 = k & 2 ? o.hi[1] : o.lo[1], c2 = k & 4 ? o.hi[2] : o.lo[2];
            some = some || (n0 * c0 + n1 * c1) + n2 * c2 < (double)o.radius;
         }
         if (!some) return "a wedge's plane leaves nothing of its box";
      } else {
         if (o.axis < 0 || o.axis > 2) return "a cylinder's axis must be 0, 1 or 2";
         if (!(o.radius > 0.0f)) return "a cylinder's radius must be > 0";
         if (!(o.lo[o.axis] < o.hi[o.axis])) return "a cylinder needs lo < hi on its axis";
      }
   }
   return nullptr;
}

// n.x of a wedge's plane (n = center)
OBST_HD inline float obstacle_plane_dot(const sph_hip_obstacle& o, const float x[3])
{
   return (o.center[0] * x[0] + o.center[1] * x[1]) + o.center[2] * x[2];
}

OBST_HD inline bool obstacle_inside(const sph_hip_obstacle& o, const float x[3])
{
   if (o.kind == SPH_HIP_OBSTACLE_SPHERE) {
      const float dx = x[0] - o.center[0], dy = x[1] - o.center[1], dz = x[2] - o.center[2];
      return dx * dx + dy * dy + dz * dz < o.radius * o.radius;
   }
   if (o.kind == SPH_HIP_OBSTACLE_BOX)
      return o.lo[0] < x[0] && x[0] < o.hi[0] && o.lo[1] < x[1] && x[1] < o.hi[1] && o.lo[2] < x[2] &&
             x[2] < o.hi[2];
   if (o.kind == SPH_HIP_OBSTACLE_WEDGE)
      return o.lo[0] < x[0] && x[0] < o.hi[0] && o.lo[1] < x[1] && x[1] < o.hi[1] && o.lo[2] < x[2] &&
             x[2] < o.hi[2] && obstacle_plane_dot(o, x) < o.radius;
   const int a = o.axis, u = (a + 1) % 3, w = (a + 2) % 3;
   const float du = x[u] - o.center[u], dw = x[w] - o.center[w];
   return o.lo[a] < x[a] && x[a] < o.hi[a] && du * du + dw * dw < o.radius * o.radius;
}

// Slab of one axis for the line p + v*s: entry t0 and exit t1 (false: the line misses it).
OBST_HD inline bool obstacle_slab(float p, float v, float lo, float hi, float& t0, float& t1)
{
   if (v != 0.0f) {
      t0 = ((v > 0.0f ? lo : hi) - p) / v;
      t1 = ((v > 0.0f ? hi : lo) - p) / v;
      return true;
   }
   t0 = -INFINITY;
   t1 = INFINITY;
   return lo < p && p < hi;
}

// The response of one obstacle (see the contract above).
OBST_HD inline void obstacle_respond(const sph_hip_obstacle& o, const float p[3], float v[3], float q[3],
                                     float dt, float damping)
{
   if (!obstacle_inside(o, q)) return;
   const float r = o.radius;
   float n[3] = {0.0f, 0.0f, 0.0f};
   float t = 0.0f, t_exit = 0.0f;
   bool hit = !obstacle_inside(o, p) && (v[0] != 0.0f || v[1] != 0.0f || v[2] != 0.0f);
   const bool wedge = o.kind == SPH_HIP_OBSTACLE_WEDGE;
   int kind_n = -1;   // entry normal: axis 0..2 (slab), 3 (sphere), 4 (cylinder side), 5 (wedge plane)
   if (hit) {
      if (o.kind == SPH_HIP_OBSTACLE_BOX || wedge) {
         t = -INFINITY;
         t_exit = INFINITY;
         for (int a = 0; a < 3 && hit; a++) {
            float t0, t1;
            if (!obstacle_slab(p[a], v[a], o.lo[a], o.hi[a], t0, t1)) hit = false;
            if (v[a] != 0.0f && t0 > t) {
               t = t0;
               kind_n = a;
            }
            if (t1 < t_exit) t_exit = t1;
         }
         if (wedge && hit) {
            const float g = obstacle_plane_dot(o, v);
            const float f = obstacle_plane_dot(o, p) - r;
            if (g == 0.0f) {
               if (!(f < 0.0f)) hit = false;
            } else {
               const float s_pl = (-f) / g;
               if (g < 0.0f) {
                  if (s_pl > t) {
                     t = s_pl;
                     kind_n = 5;
                  }
               } else if (s_pl < t_exit) {
                  t_exit = s_pl;
               }
            }
         }
      } else if (o.kind == SPH_HIP_OBSTACLE_SPHERE) {
         const float d0x = p[0] - o.center[0], d0y = p[1] - o.center[1], d0z = p[2] - o.center[2];
         const float A = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
         const float B = d0x * v[0] + d0y * v[1] + d0z * v[2];
         const float C = (d0x * d0x + d0y * d0y + d0z * d0z) - r * r;
         const float D = B * B - A * C;
         if (D > 0.0f) {
            const float s = sqrtf(D);
            t = (-B - s) / A;
            t_exit = (-B + s) / A;
            kind_n = 3;
         } else {
            hit = false;
         }
      } else {
         const int a = o.axis, u = (a + 1) % 3, w = (a + 2) % 3;
         float tc0, tc1, tr0 = -INFINITY, tr1 = INFINITY;
         hit = obstacle_slab(p[a], v[a], o.lo[a], o.hi[a], tc0, tc1);
         const float d0u = p[u] - o.center[u], d0w = p[w] - o.center[w];
         const float A = v[u] * v[u] + v[w] * v[w];
         const float C = (d0u * d0u + d0w * d0w) - r * r;
         if (A > 0.0f) {
            const float B = d0u * v[u] + d0w * v[w];
            const float D = B * B - A * C;
            if (D > 0.0f) {
               const float s = sqrtf(D);
               tr0 = (-B - s) / A;
               tr1 = (-B + s) / A;
            } else {
               hit = false;
            }
         } else if (!(d0u * d0u + d0w * d0w < r * r)) {
            hit = false;
         }
         if (tc0 >= tr0) {
            t = tc0;
            kind_n = a;
         } else {
            t = tr0;
            kind_n = 4;
         }
         t_exit = tc1 < tr1 ? tc1 : tr1;
      }
      hit = hit && t >= 0.0f && t < t_exit;
   }
   if (hit) {
      float inter[3], refl[3];
      for (int c = 0; c < 3; c++) inter[c] = p[c] + v[c] * t;
      if (kind_n < 3) {
         n[kind_n] = v[kind_n] > 0.0f ? -1.0f : 1.0f;
      } else if (kind_n == 3) {
         for (int c = 0; c < 3; c++) n[c] = (inter[c] - o.center[c]) / r;
      } else if (kind_n == 5) {
         for (int c = 0; c < 3; c++) n[c] = o.center[c];
      } else {
         const int a = o.axis, u = (a + 1) % 3, w = (a + 2) % 3;
         n[u] = (inter[u] - o.center[u]) / r;
         n[w] = (inter[w] - o.center[w]) / r;
         n[a] = 0.0f;
      }
      const float dot = v[0] * n[0] + v[1] * n[1] + v[2] * n[2];
      for (int c = 0; c < 3; c++) refl[c] = v[c] - ((n[c] * dot) * 2.0f);
      const float rem = dt - t;
      const float remaining = rem > 0.0f ? rem : 0.0f;
      for (int c = 0; c < 3; c++) {
         v[c] = refl[c];
         q[c] = inter[c] + refl[c] * (remaining * damping);
      }
      return;
   }
   // fallback: nearest surface point
   if (o.kind == SPH_HIP_OBSTACLE_SPHERE) {
      const float dx = q[0] - o.center[0], dy = q[1] - o.center[1], dz = q[2] - o.center[2];
      const float len = sqrtf(dx * dx + dy * dy + dz * dz);
      if (len > 0.0f) {
         n[0] = dx / len;
         n[1] = dy / len;
         n[2] = dz / len;
      } else {
         n[0] = 1.0f;
      }
      for (int c = 0; c < 3; c++) q[c] = o.center[c] + n[c] * r;
   } else if (o.kind == SPH_HIP_OBSTACLE_BOX || wedge) {
      float best = INFINITY;
      int face = 0;
      for (int a = 0; a < 3; a++) {
         const float dlo = q[a] - o.lo[a], dhi = o.hi[a] - q[a];
         if (dlo < best) {
            best = dlo;
            face = 2 * a;
         }
         if (dhi < best) {
            best = dhi;
            face = 2 * a + 1;
         }
      }
      const float dpl = wedge ? r - obstacle_plane_dot(o, q) : INFINITY;
      const int a = face >> 1;
      if (dpl < best) {
         for (int c = 0; c < 3; c++) {
            n[c] = o.center[c];
            q[c] = q[c] + n[c] * dpl;
         }
      } else if (face & 1) {
         q[a] = o.hi[a];
         n[a] = 1.0f;
      } else {
         q[a] = o.lo[a];
         n[a] = -1.0f;
      }
   } else {
      const int a = o.axis, u = (a + 1) % 3, w = (a + 2) % 3;
      const float du = q[u] - o.center[u], dw = q[w] - o.center[w];
      const float len = sqrtf(du * du + dw * dw);
      const float dlo = q[a] - o.lo[a], dhi = o.hi[a] - q[a], dside = r - len;
      if (dlo <= dhi && dlo <= dside) {
         q[a] = o.lo[a];
         n[a] = -1.0f;
      } else if (dhi <= dside) {
         q[a] = o.hi[a];
         n[a] = 1.0f;
      } else {
         if (len > 0.0f) {
            n[u] = du / len;
            n[w] = dw / len;
         } else {
            n[u] = 1.0f;
         }
         q[u] = o.center[u] + n[u] * r;
         q[w] = o.center[w] + n[w] * r;
      }
   }
   const float dot = v[0] * n[0] + v[1] * n[1] + v[2] * n[2];
   const float m = dot < 0.0f ? dot : 0.0f;
   for (int c = 0; c < 3; c++) v[c] = v[c] - n[c] * (m * 2.0f);
}

// Every obstacle of a list, in order.
OBST_HD inline void obstacles_respond(const sph_hip_obstacle* list, int n, const float p[3], float v[3], float q[3],
                                      float dt, float damping)
{
   for (int i = 0; i < n; i++) obstacle_respond(list[i], p, v, q, dt, damping);
}

// ---- moving obstacles (the contract's second part) ------------------------------------------------

// Why a motion list for `n_obstacles` obstacles is refused, or nullptr.  n = 0 clears all motions.
inline const char* obstacle_motion_check(const sph_hip_obstacle_motion* list, int n, int n_obstacles)
{
   if (n != 0 && n != n_obstacles) return "the motion count must be 0 or the obstacle count";
   if (n > 0 && !list) return "null motion list";
   for (int i = 0; i < n; i++) {
      const sph_hip_obstacle_motion& m = list[i];
      if (!isfinite(m.velocity[0]) || !isfinite(m.velocity[1]) || !isfinite(m.velocity[2]))
         return "a motion's velocity must be finite";
      if (!isfinite(m.start) || !(m.start >= 0.0f)) return "a motion's start must be finite and >= 0";
      if (!(m.stop >= m.start)) return "a motion needs stop >= start";
   }
   return nullptr;
}

OBST_HD inline bool obstacle_moves(const sph_hip_obstacle_motion& m)
{
   return m.velocity[0] != 0.0f || m.velocity[1] != 0.0f || m.velocity[2] != 0.0f;
}

// how many entries of a motion list move
inline int obstacles_moving(const sph_hip_obstacle_motion* list, int n)
{
   int k = 0;
   for (int i = 0; i < n; i++) k += obstacle_moves(list[i]) ? 1 : 0;
   return k;
}

// the motion clock after a step of dt
inline float obstacle_clock_next(float tau, float dt) { return tau + dt; }

OBST_HD inline float obstacle_motion_s(const sph_hip_obstacle_motion& m, float tau)
{
   return (tau < m.start ? m.start : tau > m.stop ? m.stop : tau) - m.start;
}

OBST_HD inline void obstacle_displacement(const sph_hip_obstacle_motion& m, float tau, float D[3])
{
   const float s = obstacle_motion_s(m, tau);
   for (int c = 0; c < 3; c++) D[c] = m.velocity[c] * s;
}

OBST_HD inline sph_hip_obstacle obstacle_shifted(const sph_hip_obstacle& o, const float D[3])
{
   sph_hip_obstacle s = o;
   const bool wedge = o.kind == SPH_HIP_OBSTACLE_WEDGE;   // its center is a normal: the plane's offset moves
   for (int c = 0; c < 3; c++) {
      s.center[c] = wedge ? o.center[c] : o.center[c] + D[c];
      s.lo[c] = o.lo[c] + D[c];
      s.hi[c] = o.hi[c] + D[c];
   }
   if (wedge) s.radius = o.radius + obstacle_plane_dot(o, D);
   return s;
}

// the obstacle at tau: shifted when its motion moves it, untouched otherwise (m may be null)
OBST_HD inline sph_hip_obstacle obstacle_at(const sph_hip_obstacle& o, const sph_hip_obstacle_motion* m, float tau)
{
   if (!m || !obstacle_moves(*m)) return o;
   float D[3];
   obstacle_displacement(*m, tau, D);
   return obstacle_shifted(o, D);
}

// The response of one moving obstacle whose shifts at the start and the end of the step are D0 and D1,
// o1 being the obstacle at the end (one obstacle_respond call site for both branches of the contract).
OBST_HD inline void obstacle_respond_moved(const sph_hip_obstacle& o1, const float D0[3], const float D1[3],
                                           const float p[3], float v[3], float q[3], float dt, float damping)
{
   if (!obstacle_inside(o1, q)) return;
   const float d[3] = {D1[0] - D0[0], D1[1] - D0[1], D1[2] - D0[2]};
   const bool boost = d[0] != 0.0f || d[1] != 0.0f || d[2] != 0.0f;
   float ue[3] = {0.0f, 0.0f, 0.0f}, pr[3] = {p[0], p[1], p[2]}, w[3] = {v[0], v[1], v[2]};
   if (boost) {
      for (int c = 0; c < 3; c++) {
         ue[c] = d[c] / dt;
         pr[c] = p[c] + d[c];
         w[c] = v[c] - ue[c];
      }
   }
   obstacle_respond(o1, pr, w, q, dt, damping);
   for (int c = 0; c < 3; c++) v[c] = boost ? w[c] + ue[c] : w[c];
}

// One entry's turn in a list with motions: obstacle_respond for one that does not move,
// obstacle_respond_moved for one that does.  Returns whether q was strictly inside the obstacle as it
// stands at the end of the step (what the load recorder calls a response).
OBST_HD inline bool obstacle_turn(const sph_hip_obstacle& o, const sph_hip_obstacle_motion& m, const float p[3],
                                  float v[3], float q[3], float dt, float damping, float tau0, float tau1)
{
   if (!obstacle_moves(m)) {
      const bool in = obstacle_inside(o, q);
      obstacle_respond(o, p, v, q, dt, damping);
      return in;
   }
   float D0[3], D1[3];
   obstacle_displacement(m, tau0, D0);
   obstacle_displacement(m, tau1, D1);
   const sph_hip_obstacle o1 = obstacle_shifted(o, D1);
   const bool in = obstacle_inside(o1, q);
   obstacle_respond_moved(o1, D0, D1, p, v, q, dt, damping);
   return in;
}

// Every obstacle of a list with motions, in order.
OBST_HD inline void obstacles_respond_moving(const sph_hip_obstacle* list, const sph_hip_obstacle_motion* motion,
                                             int n, const float p[3], float v[3], float q[3], float dt,
                                             float damping, float tau0, float tau1)
{
   for (int i = 0; i < n; i++) obstacle_turn(list[i], motion[i], p, v, q, dt, damping, tau0, tau1);
}

// ---- oriented and rotating obstacles (the contract's third part) ------------------------------------

#define OBSTACLE_MAX_ANGLE 8192.0f

typedef struct sph_hip_obstacle_rotation {   /* field order is fixed: 32 bytes */
   int32_t axis;                    /* 0, 1 or 2: the coordinate axis the solid turns about */
   float pivot[3];                  /* a point on that axis (the component along `axis` is unused) */
   float angle;                     /* radians at the clock's start, right-handed about +axis */
   float rate;                      /* radians per unit of time_step while start <= tau <= stop */
   float start, stop;               /* on the motion clock; stop may be +INFINITY */
} sph_hip_obstacle_rotation;

OBST_HD inline bool obstacle_posed(const sph_hip_obstacle_rotation& r) { return r.angle != 0.0f || r.rate != 0.0f; }
OBST_HD inline bool obstacle_rotates(const sph_hip_obstacle_rotation& r) { return r.rate != 0.0f; }

// Why a rotation list for `n_obstacles` obstacles is refused, or nullptr.  n = 0 clears all rotations.
inline const char* obstacle_rotation_check(const sph_hip_obstacle_rotation* list, int n, int n_obstacles)
{
   if (n != 0 && n != n_obstacles) return "the rotation count must be 0 or the obstacle count";
   if (n > 0 && !list) return "null rotation list";
   for (int i = 0; i < n; i++) {
      const sph_hip_obstacle_rotation& r = list[i];
      if (r.axis < 0 || r.axis > 2) return "a rotation's axis must be 0, 1 or 2";
      if (!isfinite(r.pivot[0]) || !isfinite(r.pivot[1]) || !isfinite(r.pivot[2]))
         return "a rotation's pivot must be finite";
      if (!isfinite(r.angle) || !isfinite(r.rate)) return "a rotation's angle and rate must be finite";
      if (!isfinite(r.start) || !(r.start >= 0.0f)) return "a rotation's start must be finite and >= 0";
      if (!(r.stop >= r.start)) return "a rotation needs stop >= start";
      if (fabs((double)r.angle) > (double)OBSTACLE_MAX_ANGLE) return "a rotation's angle must stay within 8192 radians";
      if (isfinite(r.stop) &&
          fabs((double)r.angle) + fabs((double)r.rate) * ((double)r.stop - (double)r.start) > (double)OBSTACLE_MAX_ANGLE)
         return "a rotation's angle must stay within 8192 radians until its stop";
   }
   return nullptr;
}

// Why rotations and motions do not go together (either list may be empty), or nullptr: one function
// for both directions.
inline const char* obstacle_rotation_motion_check(const sph_hip_obstacle_rotation* rot, int n_rot,
                                                  const sph_hip_obstacle_motion* motion, int n_motion)
{
   for (int i = 0; i < n_rot && i < n_motion; i++)
      if (obstacle_posed(rot[i]) && obstacle_moves(motion[i])) return "a posed entry on an obstacle whose motion moves";
   return nullptr;
}

// how many entries of a rotation list are posed / rotate
inline int obstacles_posed(const sph_hip_obstacle_rotation* list, int n)
{
   int k = 0;
   for (int i = 0; i < n; i++) k += obstacle_posed(list[i]) ? 1 : 0;
   return k;
}
inline int obstacles_rotating(const sph_hip_obstacle_rotation* list, int n)
{
   int k = 0;
   for (int i = 0; i < n; i++) k += obstacle_rotates(list[i]) ? 1 : 0;
   return k;
}

OBST_HD inline float obstacle_theta(const sph_hip_obstacle_rotation& r, float tau)
{
   const float s = (tau < r.start ? r.start : tau > r.stop ? r.stop : tau) - r.start;
   const float turned = r.rate * s;
   return r.angle + turned;
}

// cos and sin of theta (see the contract: every operation is written out, one rounding each)
OBST_HD inline void obstacle_sincos(float theta, float& cs, float& sn)
{
   const float k = rintf(theta * 0.636619772367581343f);
   float r = theta - k * 1.5703125f;
   r = r - k * 4.837512969970703125e-4f;
   r = r - k * 7.54978995489188216e-8f;
   const float z = r * r;
   float s = -1.9515295891e-4f * z + 8.3321608736e-3f;
   s = s * z + -1.6666654611e-1f;
   s = (s * z) * r + r;
   float c = 2.443315711809948e-5f * z + -1.388731625493765e-3f;
   c = c * z + 4.166664568298827e-2f;
   c = (c * z) * z - 0.5f * z;
   c = c + 1.0f;
   const int q = (int)k & 3;
   cs = q == 0 ? c : q == 1 ? -s : q == 2 ? -c : s;
   sn = q == 0 ? s : q == 1 ? c : q == 2 ? -s : -c;
}

// One entry's pose for a step: the frame at the start (0) and at the end (1) of the step; still: the
// angle is the same at both.  24 bytes: formed once per obstacle and step, not once per particle.
struct ObstaclePose {
   float cs0, sn0, cs1, sn1;
   int32_t posed, still;
};

OBST_HD inline ObstaclePose obstacle_pose_of_step(const sph_hip_obstacle_rotation& r, float tau0, float tau1)
{
   ObstaclePose ps = {1.0f, 0.0f, 1.0f, 0.0f, 0, 1};
   if (!obstacle_posed(r)) return ps;
   const float t0 = obstacle_theta(r, tau0), t1 = obstacle_theta(r, tau1);
   obstacle_sincos(t0, ps.cs0, ps.sn0);
   obstacle_sincos(t1, ps.cs1, ps.sn1);
   ps.posed = 1;
   ps.still = t1 == t0 ? 1 : 0;
   return ps;
}

OBST_HD inline void obstacle_to_body(const sph_hip_obstacle_rotation& r, float cs, float sn, const float x[3], float y[3])
{
   const int a = r.axis, u = (a + 1) % 3, w = (a + 2) % 3;
   const float du = x[u] - r.pivot[u], dw = x[w] - r.pivot[w];
   y[a] = x[a];
   y[u] = r.pivot[u] + (cs * du + sn * dw);
   y[w] = r.pivot[w] + (cs * dw - sn * du);
}

OBST_HD inline void obstacle_to_world(const sph_hip_obstacle_rotation& r, float cs, float sn, const float y[3], float x[3])
{
   const int a = r.axis, u = (a + 1) % 3, w = (a + 2) % 3;
   const float du = y[u] - r.pivot[u], dw = y[w] - r.pivot[w];
   x[a] = y[a];
   x[u] = r.pivot[u] + (cs * du - sn * dw);
   x[w] = r.pivot[w] + (sn * du + cs * dw);
}

OBST_HD inline void obstacle_vec_to_body(const sph_hip_obstacle_rotation& r, float cs, float sn, const float x[3], float y[3])
{
   const int a = r.axis, u = (a + 1) % 3, w = (a + 2) % 3;
   const float xu = x[u], xw = x[w];
   y[a] = x[a];
   y[u] = cs * xu + sn * xw;
   y[w] = cs * xw - sn * xu;
}

OBST_HD inline void obstacle_vec_to_world(const sph_hip_obstacle_rotation& r, float cs, float sn, const float y[3], float x[3])
{
   const int a = r.axis, u = (a + 1) % 3, w = (a + 2) % 3;
   const float yu = y[u], yw = y[w];
   x[a] = y[a];
   x[u] = cs * yu - sn * yw;
   x[w] = sn * yu + cs * yw;
}

// A posed entry's turn with its pose of this step (one obstacle_respond call site for both branches of
// the contract).  Returns whether q was strictly inside the solid as it stands at the end of the step.
OBST_HD inline bool obstacle_turn_posed(const sph_hip_obstacle& o, const sph_hip_obstacle_rotation& r,
                                        const ObstaclePose& ps, const float p[3], float v[3], float q[3], float dt,
                                        float damping)
{
   float q1[3];
   obstacle_to_body(r, ps.cs1, ps.sn1, q, q1);
   if (!obstacle_inside(o, q1)) return false;
   float p0[3];
   obstacle_to_body(r, ps.cs0, ps.sn0, p, p0);
   const bool boost = !ps.still;
   float ue[3] = {0.0f, 0.0f, 0.0f}, wv[3] = {v[0], v[1], v[2]};
   if (boost) {
      float pc[3];
      obstacle_to_world(r, ps.cs1, ps.sn1, p0, pc);
      for (int c = 0; c < 3; c++) {
         const float d = pc[c] - p[c];
         ue[c] = d / dt;
         wv[c] = v[c] - ue[c];
      }
   }
   float w[3];
   obstacle_vec_to_body(r, ps.cs1, ps.sn1, wv, w);
   obstacle_respond(o, p0, w, q1, dt, damping);
   obstacle_vec_to_world(r, ps.cs1, ps.sn1, w, wv);
   for (int c = 0; c < 3; c++) v[c] = boost ? wv[c] + ue[c] : wv[c];
   obstacle_to_world(r, ps.cs1, ps.sn1, q1, q);
   return true;
}

// One entry's turn in a list with rotations: obstacle_turn_posed for a posed one, otherwise the turn of
// its motion (`motion` may be null: no motions set) or the static one.
OBST_HD inline bool obstacle_turn_any(const sph_hip_obstacle& o, const sph_hip_obstacle_motion* motion,
                                      const sph_hip_obstacle_rotation& r, const ObstaclePose& ps, const float p[3],
                                      float v[3], float q[3], float dt, float damping, float tau0, float tau1)
{
   if (ps.posed) return obstacle_turn_posed(o, r, ps, p, v, q, dt, damping);
   if (motion) return obstacle_turn(o, *motion, p, v, q, dt, damping, tau0, tau1);
   const bool in = obstacle_inside(o, q);
   obstacle_respond(o, p, v, q, dt, damping);
   return in;
}

// Every obstacle of a list with rotations, in order, with the poses of this step (`pose`: one per obstacle).
OBST_HD inline void obstacles_respond_posed(const sph_hip_obstacle* list, const sph_hip_obstacle_motion* motion,
                                            const sph_hip_obstacle_rotation* rot, const ObstaclePose* pose, int n,
                                            const float p[3], float v[3], float q[3], float dt, float damping,
                                            float tau0, float tau1)
{
   for (int i = 0; i < n; i++)
      obstacle_turn_any(list[i], motion ? motion + i : nullptr, rot[i], pose[i], p, v, q, dt, damping, tau0, tau1);
}

// ---- motion paths (the contract's fourth part) ------------------------------------------------------

OBST_HD inline bool path_is(const sph_hip_motion_path& P) { return P.count != 0; }

// how many entries of a path list have a path
inline int paths_count(const sph_hip_motion_path* paths, int n)
{
   int k = 0;
   for (int i = 0; i < n; i++) k += path_is(paths[i]) ? 1 : 0;
   return k;
}

// Why a path list for `n_obstacles` obstacles is refused, or nullptr.  n = 0 clears all paths.
inline const char* path_check(const sph_hip_motion_path* paths, int n, const sph_hip_motion_key* keys, int n_keys,
                              int n_obstacles)
{
   if (n != 0 && n != n_obstacles) return "the path count must be 0 or the obstacle count";
   if (n == 0) return nullptr;
   if (!paths) return "null path list";
   if (n_keys < 0 || n_keys > SPH_HIP_MAX_PATH_KEYS) return "the key count must be in [0, 16384]";
   if (n_keys > 0 && !keys) return "null key list";
   for (int i = 0; i < n; i++) {
      const sph_hip_motion_path& P = paths[i];
      if (P.count < 0) return "a path's key count must be >= 0";
      if (P.count == 1) return "a path needs at least two keys";
      if (P.count == 0) continue;
      if (P.first < 0 || P.first > n_keys || P.count > n_keys - P.first) return "a path's keys leave the key list";
      if (!isfinite(P.start) || !(P.start >= 0.0f)) return "a path's start must be finite and >= 0";
      const sph_hip_motion_key* k = keys + P.first;
      if (k[0].t != 0.0f) return "a path's first key must be at t = 0";
      for (int j = 0; j < P.count; j++) {
         if (!isfinite(k[j].t) || (j > 0 && !(k[j].t > k[j - 1].t)))
            return "a path's key times must be finite and strictly increasing";
         if (!isfinite(k[j].d[0]) || !isfinite(k[j].d[1]) || !isfinite(k[j].d[2]))
            return "a path's displacements must be finite";
      }
      if (P.cycle != 0)
         for (int c = 0; c < 3; c++)
            if (k[P.count - 1].d[c] != k[0].d[c]) return "a cyclic path must end at the displacement it begins with";
   }
   return nullptr;
}

// Why paths and motions do not go together (either list may be empty), or nullptr: one function for
// both directions.
inline const char* path_motion_check(const sph_hip_motion_path* paths, int n_paths, const sph_hip_obstacle_motion* motion,
                                     int n_motion)
{
   for (int i = 0; i < n_paths && i < n_motion; i++)
      if (path_is(paths[i]) && obstacle_moves(motion[i])) return "a path on an obstacle whose motion moves";
   return nullptr;
}

// Where tau falls on a path: the segment j (relative to the path's first key), the path time u, and
// whether u was clamped (before the start, or past the end of a path that does not cycle).
struct PathSegment {
   int j;
   float u;
   bool clamped;
};

OBST_HD inline PathSegment path_segment(const sph_hip_motion_path& P, const sph_hip_motion_key* keys, float tau)
{
   const sph_hip_motion_key* k = keys + P.first;
   const float T = k[P.count - 1].t;
   float u = tau - P.start;
   bool clamped = false;
   if (u < 0.0f) {
      u = 0.0f;
      clamped = true;
   }
   if (P.cycle == 0) {
      if (u > T) {
         u = T;
         clamped = true;
      }
   } else {
      if (u >= T) {
         const float turns = floorf(u / T);
         u = u - turns * T;
      }
      if (u < 0.0f) u = 0.0f;
      if (u >= T) u = 0.0f;
   }
   int lo = 0, hi = P.count - 2;   // the largest j with t[j] <= u
   while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (k[mid].t <= u) lo = mid;
      else hi = mid - 1;
   }
   const PathSegment s = {lo, u, clamped};
   return s;
}

// D(tau) of a path (path_is(P)): the one function the device's k_paths_eval and the host use.
OBST_HD inline void path_displacement(const sph_hip_motion_path& P, const sph_hip_motion_key* keys, float tau, float D[3])
{
   const PathSegment s = path_segment(P, keys, tau);
   const sph_hip_motion_key* k = keys + P.first + s.j;
   const float w = (s.u - k[0].t) / (k[1].t - k[0].t);
   for (int c = 0; c < 3; c++) D[c] = k[0].d[c] + w * (k[1].d[c] - k[0].d[c]);
}

// the velocity of the segment in force at tau, 0 while the path time is clamped
inline void path_velocity(const sph_hip_motion_path& P, const sph_hip_motion_key* keys, float tau, float v[3])
{
   const PathSegment s = path_segment(P, keys, tau);
   const sph_hip_motion_key* k = keys + P.first + s.j;
   for (int c = 0; c < 3; c++) v[c] = s.clamped ? 0.0f : (k[1].d[c] - k[0].d[c]) / (k[1].t - k[0].t);
}

// One entry's shifts for a step: 32 bytes, formed once per obstacle and step (k_paths_eval), read
// wave-uniformly by the integrate.
struct PathShift {
   float D0[3], D1[3];
   int32_t has_path, pad;
};

OBST_HD inline PathShift path_shift_of_step(const sph_hip_motion_path& P, const sph_hip_motion_key* keys, float tau0,
                                            float tau1)
{
   PathShift s = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, 0, 0};
   if (!path_is(P)) return s;
   path_displacement(P, keys, tau0, s.D0);
   path_displacement(P, keys, tau1, s.D1);
   s.has_path = 1;
   return s;
}

// k_paths_eval's lane loop, lane i = obstacle i (the host's restatement of the launch)
inline void paths_eval(const sph_hip_motion_path* paths, const sph_hip_motion_key* keys, int n, float tau0, float tau1,
                       PathShift* out)
{
   for (int i = 0; i < n; i++) out[i] = path_shift_of_step(paths[i], keys, tau0, tau1);
}

// the obstacle at tau in a list with paths: shifted along its path, otherwise obstacle_at with its motion
inline sph_hip_obstacle path_obstacle_at(const sph_hip_obstacle& o, const sph_hip_motion_path* P,
                                         const sph_hip_motion_key* keys, const sph_hip_obstacle_motion* m, float tau)
{
   if (!P || !path_is(*P)) return obstacle_at(o, m, tau);
   float D[3];
   path_displacement(*P, keys, tau, D);
   return obstacle_shifted(o, D);
}

// One entry's turn in a list with paths: the moved response with the shifts of `s` for an entry with a
// path, otherwise the turn of its motion (`motion` may be null: no motions set) or the static one.
// Returns whether q was strictly inside the obstacle as it stands at the end of the step.
OBST_HD inline bool obstacle_turn_path(const sph_hip_obstacle& o, const sph_hip_obstacle_motion* motion,
                                       const PathShift& s, const float p[3], float v[3], float q[3], float dt,
                                       float damping, float tau0, float tau1)
{
   // (obstacle_turn written out, so that the two shifted turns share one call site and the static ones
   // another: with a call site each the compiler kept o1 in scratch memory)
   float D0[3], D1[3];
   bool shifted = false;
   if (s.has_path) {
      for (int c = 0; c < 3; c++) {
         D0[c] = s.D0[c];
         D1[c] = s.D1[c];
      }
      shifted = true;
   } else if (motion && obstacle_moves(*motion)) {
      obstacle_displacement(*motion, tau0, D0);
      obstacle_displacement(*motion, tau1, D1);
      shifted = true;
   }
   if (shifted) {
      const sph_hip_obstacle o1 = obstacle_shifted(o, D1);
      const bool in = obstacle_inside(o1, q);
      obstacle_respond_moved(o1, D0, D1, p, v, q, dt, damping);
      return in;
   }
   const bool in = obstacle_inside(o, q);
   obstacle_respond(o, p, v, q, dt, damping);
   return in;
}

// Every obstacle of a list with paths, in order, with the shifts of this step (`shift`: one per obstacle).
OBST_HD inline void obstacles_respond_path(const sph_hip_obstacle* list, const sph_hip_obstacle_motion* motion,
                                           const PathShift* shift, int n, const float p[3], float v[3], float q[3],
                                           float dt, float damping, float tau0, float tau1)
{
   for (int i = 0; i < n; i++)
      obstacle_turn_path(list[i], motion ? motion + i : nullptr, shift[i], p, v, q, dt, damping, tau0, tau1);
}
