// Scalar renderer: the frame's fluid pixels coloured by one carried channel (sph_hip_render_scalars;
// include/sph_hip.h states the contract, tint_policy.h holds its functions, and tests/test_gpu_tint.py pins
// the device to the numpy restatement tests/tint_emulation.py).
//
// Per row chunk the tint kernel runs behind k_render_shade and, where solids are drawn, behind
// k_scene_solids: one lane per entry of the chunk's hit list, which k_render_march leaves in the scratch
// until the next chunk.  The march appends each wave's hits as one run (the runs in the order its waves retire),
// so the list is per-wave runs of one 8 x 8 tile and most of a wave's lanes here are neighbouring pixels: they
// walk the same cells through L1 and read the same or adjacent rows of the colour table (identical LDS
// addresses broadcast).  A lane whose pixel a solid took (first_inside < 0) returns at once.
//   k_tint_surface   one walk of the channels at the pixel's hit point (sample_walk with ScalarSum: the scalar
//                    sampler's bits)
//   k_tint_column    the march from first_inside to the end of the box, a channel walk at every sample the
//                    occupancy map does not rule out; rays of a wave differ in length, the loop runs as long
//                    as the wave's longest
// The workgroup's first wave copies the table (at most 3072 bytes) to LDS: its row is a run-time index.
// No atomics; every local array is indexed by unrolled constants.
#pragma once

#include "render_kernels.h"
#include "scalar_kernels.h"
#include "tint_policy.h"

// what a tint launch needs besides the frame: the params and the device copy of the table
struct TintArgs {
   sph_hip_tint_params tp;
   const float* table;   // 3 * n_colors floats
};

// the accumulator's sum of the channel (a select per channel: no array indexed by a run-time number)
__device__ __forceinline__ float tint_channel(const ScalarSum& s, int channel)
{
   return channel == 0 ? s.a0 : channel == 1 ? s.a1 : channel == 2 ? s.a2 : s.a3;
}

// the table to LDS by the first wave; every lane of the workgroup reaches the barrier
__device__ __forceinline__ void tint_table_load(const TintArgs& T, float* lds)
{
   if (threadIdx.x < SPH_WAVE)
      for (int i = threadIdx.x; i < 3 * T.tp.n_colors; i += SPH_WAVE) lds[i] = T.table[i];
   __syncthreads();
}

// map, shade and store of one tinted pixel
template <bool FLAT>
__device__ __forceinline__ void tint_store(const RenderFrame& F, const TintArgs& T, const float* lds, int o, float v,
                                           const float* __restrict__ normal_in, uint32_t* __restrict__ rgba_out,
                                           float* __restrict__ scalar_out)
{
   float col[3];
   tint_map(v, T.tp.lo, T.tp.hi, T.tp.n_colors, lds, col);
   float w = 1.0f;
   if (!FLAT) {
      const float n[3] = {normal_in[3 * o + 0], normal_in[3 * o + 1], normal_in[3 * o + 2]};
      w = tint_weight(n, F.rp.light, F.rp.ambient, F.rp.diffuse);
   }
   rgba_out[o] = tint_pixel(col, w);
   scalar_out[o] = v;
}

// ---- SURFACE: one walk per listed hit ---------------------------------------------------------------------
template <bool UNIT_SCALE, bool FLAT>
__global__ void __launch_bounds__(RENDER_THREADS)
k_tint_surface(RenderFrame F, TintArgs T, const float4* __restrict__ posm, const float4* __restrict__ Ts,
               const uint32_t* __restrict__ cell_start, CellGrid g, PairConsts k, const int32_t* __restrict__ hits,
               const uint32_t* __restrict__ hit_count, const int32_t* __restrict__ first_in,
               const float* __restrict__ depth_in, const float* __restrict__ normal_in,
               uint32_t* __restrict__ rgba_out, float* __restrict__ scalar_out)
{
   __shared__ float lds[TINT_TABLE_FLOATS];
   const uint32_t count = *hit_count;
   if (blockIdx.x * blockDim.x >= count) return;   // (the whole workgroup)
   tint_table_load(T, lds);
   const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i >= count) return;
   const int o = hits[i];
   if (first_in[o] < 0) return;   // a solid took the pixel
   const int px = o % F.width, py = F.row0 + o / F.width;
   float d[3], tnear, tfar;
   render_ray(F, px, py, d, tnear, tfar);   // a listed pixel's ray hit the box
   const float t = depth_in[o];
   const float* eye = F.cam.eye;
   ScalarSum s;
   sample_walk<UNIT_SCALE>(eye[0] + t * d[0], eye[1] + t * d[1], eye[2] + t * d[2], posm, Ts, cell_start, g, k,
                                   s);
   const float v = scalar_shepard(tint_channel(s, T.tp.channel), s.rho);
   tint_store<FLAT>(F, T, lds, o, v, normal_in, rgba_out, scalar_out);
}

// ---- COLUMN: the march through the fluid, one lane per listed hit ---------------------------------------------
template <bool UNIT_SCALE, bool SKIP, bool FLAT>
__global__ void __launch_bounds__(RENDER_THREADS)
k_tint_column(RenderFrame F, TintArgs T, const float4* __restrict__ posm, const float4* __restrict__ Ts,
              const uint32_t* __restrict__ cell_start, CellGrid g, PairConsts k, const unsigned char* __restrict__ occ,
              const int32_t* __restrict__ hits, const uint32_t* __restrict__ hit_count,
              const int32_t* __restrict__ first_in, const float* __restrict__ normal_in,
              uint32_t* __restrict__ rgba_out, float* __restrict__ scalar_out)
{
   __shared__ float lds[TINT_TABLE_FLOATS];
   const uint32_t count = *hit_count;
   if (blockIdx.x * blockDim.x >= count) return;   // (the whole workgroup)
   tint_table_load(T, lds);
   const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i >= count) return;
   const int o = hits[i];
   const int first = first_in[o];
   if (first < 0) return;   // a solid took the pixel
   const int px = o % F.width, py = F.row0 + o / F.width;
   float d[3], tnear, tfar;
   render_ray(F, px, py, d, tnear, tfar);   // a listed pixel's ray hit the box
   const float* eye = F.cam.eye;
   const float step = F.rp.step, iso = F.rp.iso;
   const int channel = T.tp.channel;
   float A = 0.0f;
   for (int s = first; s < F.rp.max_samples; s++) {
      const float t = tnear + (float)s * step;
      if (!(t <= tfar)) break;
      const float x = eye[0] + t * d[0];
      const float y = eye[1] + t * d[1];
      const float z = eye[2] + t * d[2];
      if (SKIP) {
         // an unmarked cell: rho is exactly +0.  Whatever iso is, the walk would change no bit: inside, it would
         // add scalar_shepard(a, +0) * step = +0 to A, and A is never -0 (it starts at +0)
         int cx, cy, cz;
         probe_cell(g, x, y, z, cx, cy, cz);
         if (!occ[(cz * g.ny + cy) * g.nx + cx]) continue;
      }
      ScalarSum sum;
      sample_walk<UNIT_SCALE>(x, y, z, posm, Ts, cell_start, g, k, sum);
      A = tint_column_add(A, sum.rho, tint_channel(sum, channel), iso, step);
   }
   tint_store<FLAT>(F, T, lds, o, A, normal_in, rgba_out, scalar_out);
}
