// Decisions of the scalar renderer (tint_kernels.h, sph_hip_render_scalars): the colour map, the shade, the
// column's accumulation, the scratch it adds and the argument checks.  One set of inline functions for the
// device (k_tint_surface, k_tint_column) and for g++ (tests/test_tint_cpu.py, against the numpy restatement
// tests/tint_emulation.py).  include/sph_hip.h states the contract operation by operation ("scalar
// renderer"); all arithmetic is fp32, unfused, in the order written, with sqrtf, "/" and C99 fminf / fmaxf
// only.  Pure C++17 without HIP.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/sph_hip.h"
#include "render_policy.h"
#include "scalar_policy.h"
#include "scene_policy.h"

#define TINT_FLAGS SPH_HIP_TINT_FLAT
#define TINT_TABLE_FLOATS (3 * SPH_HIP_TINT_MAX_COLORS)

// Why the arguments are refused, or nullptr.  (The context checks - FULL, whole grid - are the sampler's and
// come first.)  n_scalars: the rows of scalars the context carries.
inline const char* tint_check(const sph_hip_camera* cam, const sph_hip_render_params* rp,
                              const sph_hip_scene_params* sp, const float* solid_albedo_rgb, int n_albedo,
                              int n_obstacles, int n_scalars, const sph_hip_tint_params* tp, const float* table_rgb,
                              int width, int height, int flags)
{
   if (sp) {
      if (const char* why = scene_check(cam, rp, sp, solid_albedo_rgb, n_albedo, n_obstacles, width, height, flags))
         return why;
   } else {
      if (flags & ~SCENE_FLAGS) return "flag bits other than SPH_HIP_RENDER_VELOCITY";
      if (const char* why = render_check(cam, rp, width, height, flags)) return why;
      if (solid_albedo_rgb || n_albedo != 0) return "solid albedos without scene params";
   }
   if (const char* why = scalar_have_check(n_scalars)) return why;
   if (!tp || !table_rgb) return "null tint params or colour table";
   if (tp->channel < 0 || tp->channel >= SPH_HIP_SCALAR_CHANNELS) return "channel must be 0 .. 3";
   if (tp->mode != SPH_HIP_TINT_SURFACE && tp->mode != SPH_HIP_TINT_COLUMN) return "unknown tint mode";
   if (tp->flags & ~TINT_FLAGS) return "unknown tint flag bits";
   if (tp->n_colors < 2 || tp->n_colors > SPH_HIP_TINT_MAX_COLORS) return "n_colors must be in [2, 256]";
   if (!scalar_finite(tp->lo) || !scalar_finite(tp->hi)) return "tint range must be finite";
   if (!(tp->lo < tp->hi)) return "tint range needs lo < hi";
   for (int i = 0; i < 3 * tp->n_colors; i++)
      if (!scalar_finite(table_rgb[i])) return "a colour table entry that is not finite";
   return nullptr;
}

// device scratch this pass adds per row chunk: one float of `scalar` per pixel, in a buffer of its own
inline long long tint_scalar_bytes(int width, int rows) { return round256((long long)width * rows * 4); }

// The colour of a value: the table's rows interpolated between lo (row 0) and hi (the last row).  A NaN
// value lands on row 0 (fmaxf(NaN, 0) is 0).  t: 3 * n_colors floats.
RENDER_HD inline void tint_map(float v, float lo, float hi, int n_colors, const float* t, float col[3])
{
   float u = (v - lo) / (hi - lo);
   u = fminf(fmaxf(u, 0.0f), 1.0f);
   const float x = u * (float)(n_colors - 1);
   int i = (int)x;
   if (i > n_colors - 2) i = n_colors - 2;
   const float fr = x - (float)i;
   for (int c = 0; c < 3; c++) col[c] = t[3 * i + c] + fr * (t[3 * (i + 1) + c] - t[3 * i + c]);
}

// the renderer's Lambert weight of a stored normal (k_render_shade's formula)
RENDER_HD inline float tint_weight(const float n[3], const float light[3], float ambient, float diffuse)
{
   const float llen = sqrtf((light[0] * light[0] + light[1] * light[1]) + light[2] * light[2]);
   const float l[3] = {light[0] / llen, light[1] / llen, light[2] / llen};
   const float ndl = (n[0] * l[0] + n[1] * l[1]) + n[2] * l[2];
   return ambient + diffuse * fmaxf(ndl, 0.0f);
}

// the pixel: col * w per channel as the renderer's byte, alpha 255
RENDER_HD inline uint32_t tint_pixel(const float col[3], float w)
{
   uint32_t rgba = 255u << 24;
   for (int c = 0; c < 3; c++) rgba |= (uint32_t)render_byte(col[c] * w) << (8 * c);
   return rgba;
}

// one sample of the column into the running integral: inside is rho > iso, strictly (a NaN rho is outside)
RENDER_HD inline float tint_column_add(float A, float rho, float a, float iso, float step)
{
   return rho > iso ? A + scalar_shepard(a, rho) * step : A;
}
