// Decisions of the renderer (render_kernels.h, sph_hip_render) that need no GPU: the argument
// checks and the row chunks a frame is rendered in.
// Pure C++17 without HIP (tests/test_render_cpu.py compiles it with g++); the environment switch
// (SPH_HIP_RENDER_NOSKIP) is read by the caller at context creation.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/sph_hip.h"
#include "sample_policy.h"

#define RENDER_MAX_DIM 16384
#define RENDER_MAX_REFINE 30
#define RENDER_MAX_SAMPLES (1 << 24)   // (float)k stays exact
#define RENDER_FLAGS SPH_HIP_RENDER_VELOCITY

#ifdef __HIPCC__
#define RENDER_HD __host__ __device__
#else
#define RENDER_HD
#endif

// a shaded channel as a byte: (uint8_t)(fminf(fmaxf(v, 0), 1) * 255 + 0.5) - NaN gives 0
RENDER_HD inline uint8_t render_byte(float v) { return (uint8_t)(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f + 0.5f); }

// Why the arguments are refused, or nullptr.  (The context checks - FULL, whole grid - are the
// sampler's and come first.)
inline const char* render_check(const sph_hip_camera* cam, const sph_hip_render_params* rp, int width, int height,
                                int flags)
{
   if (!cam || !rp) return "null camera or render params";
   if (width < 1 || width > RENDER_MAX_DIM || height < 1 || height > RENDER_MAX_DIM)
      return "width and height must be in [1, 16384]";
   if (flags & ~RENDER_FLAGS) return "unknown flag bits";
   for (int a = 0; a < 3; a++)
      if (!isfinite(cam->eye[a]) || !isfinite(cam->forward[a]) || !isfinite(cam->right[a]) || !isfinite(cam->up[a]))
         return "camera fields must be finite";
   for (int a = 0; a < 3; a++)
      if (!isfinite(rp->box_lo[a]) || !isfinite(rp->box_hi[a]) || !isfinite(rp->light[a]) ||
          !isfinite(rp->albedo[a]))
         return "render params must be finite";
   if (!isfinite(rp->step) || !isfinite(rp->iso) || !isfinite(rp->grad_step) || !isfinite(rp->ambient) ||
       !isfinite(rp->diffuse))
      return "render params must be finite";
   if (!(rp->step > 0.0f)) return "step must be > 0";
   if (!(rp->grad_step > 0.0f)) return "grad_step must be > 0";
   if (!(rp->iso > 0.0f)) return "iso must be > 0";
   if (rp->refine < 0 || rp->refine > RENDER_MAX_REFINE) return "refine must be in [0, 30]";
   for (int a = 0; a < 3; a++)
      if (!(rp->box_lo[a] < rp->box_hi[a])) return "box_lo must be below box_hi on every axis";
   if (rp->light[0] == 0.0f && rp->light[1] == 0.0f && rp->light[2] == 0.0f) return "the light vector is zero";
   if (rp->max_samples < 1 || rp->max_samples > RENDER_MAX_SAMPLES) return "max_samples must be in [1, 2^24]";
   return nullptr;
}

// ---- row chunks -------------------------------------------------------------------------------------
// A frame is rendered in chunks of whole rows.  Device scratch per pixel of a chunk: rgba (4), depth
// (4), normal (12), velocity (12), first_inside (4) and the compacted hit list (4); each array is
// rounded up to 256 bytes, and 256 bytes more hold the hit counter.  A chunk's rows are a multiple of
// the 8-row pixel tile wherever the budget allows more than one tile row.
#define RENDER_TILE 8
#define RENDER_SCRATCH_BUDGET SAMPLE_SCRATCH_BUDGET   // the sampler's chunk budget (sample_policy.h)
#define RENDER_PIXEL_BYTES 40

inline long long render_scratch_bytes(int width, int rows)
{
   const long long px = (long long)width * rows;
   return round256(px * 4) * 4 + round256(px * 12) * 2 + 256;
}

// rows per chunk: the most whole tile rows within the budget (at least one row), never more than the frame
inline int render_chunk_rows(int width, int height)
{
   long long rows = (RENDER_SCRATCH_BUDGET - 256 - 6 * 256) / ((long long)width * RENDER_PIXEL_BYTES);
   if (rows >= RENDER_TILE) rows = rows / RENDER_TILE * RENDER_TILE;
   if (rows < 1) rows = 1;
   return rows < height ? (int)rows : height;
}
