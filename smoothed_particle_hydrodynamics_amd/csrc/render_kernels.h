// Renderer: a ray-marched image of the surface {f > iso} of the field sampler's density
// (sph_hip_render; include/sph_hip.h states the contract operation by operation, and
// tests/test_gpu_render.py pins the device to its numpy restatement, tests/render_emulation.py).
//
// Every f evaluation is sample_walk (sample_kernels.h), so the bits are the sampler's.  Per row chunk
// of the frame (render_policy.h):
//   k_render_march   one wave per 8 x 8 pixel tile (its lanes walk neighbouring cells through L1):
//                    ray, box, march to the first inside sample.  A miss writes its outputs at once;
//                    a hit writes first_inside and appends its pixel to a compacted hit list.
//   k_render_shade   one lane per listed hit, in full waves: bisection, the six gradient walks,
//                    the velocity walk, shading.  Without the compaction these refine + 6 (+ 1)
//                    walks would run under the march loop, where most lanes of a wave have left.
// Empty-space skip (default route): f at p sums the 27 cells around p's clamped cell, so where that
// block holds no particle f is exactly +0 - outside, since iso > 0.  k_render_occupancy marks each
// FULL cell whose block holds a particle, once per call after the cell build; a sample in an unmarked
// cell takes f = 0 without the nine row-range loads.  SPH_HIP_RENDER_NOSKIP=1 walks every sample.
#pragma once

#include "render_policy.h"
#include "sample_kernels.h"

#define RENDER_THREADS 256

// what a launch over one row chunk needs (camera and params as the caller gave them)
struct RenderFrame {
   sph_hip_camera cam;
   sph_hip_render_params rp;
   int width, height;   // the whole image
   int row0, rows;      // the chunk: image rows [row0, row0 + rows)
   int tiles_x;         // 8 x 8 tiles per tile row
};

// ---- occupancy: a byte per FULL cell, 1 where its (clamped) 27-cell block holds a particle ------------
__global__ void __launch_bounds__(RENDER_THREADS)
k_render_occupancy(const uint32_t* __restrict__ cell_start, CellGrid g, unsigned char* __restrict__ occ)
{
   const int c = blockIdx.x * blockDim.x + threadIdx.x;
   if (c >= g.ncells) return;
   const int cx = c % g.nx, cy = (c / g.nx) % g.ny, cz = c / (g.nx * g.ny);
   RowRanges r;
   row_ranges(g, cell_start, cx, cy, cz, r);
   bool any = false;
#pragma unroll
   for (int k = 0; k < 9; k++) any = any || r.e[k] > r.s[k];
   occ[c] = any ? 1 : 0;
}

// f(p): the sampler's density; +0 without a walk where the occupancy map says the block is empty
template <bool UNIT_SCALE, bool SKIP>
__device__ __forceinline__ float render_field(float x, float y, float z, const float4* __restrict__ posm,
                                              const uint32_t* __restrict__ cell_start, const CellGrid& g,
                                              const PairConsts& k, const unsigned char* __restrict__ occ)
{
   if (SKIP) {
      int cx, cy, cz;
      probe_cell(g, x, y, z, cx, cy, cz);
      if (!occ[(cz * g.ny + cy) * g.nx + cx]) return 0.0f;
   }
   SampleSum<false> s;
   sample_walk<UNIT_SCALE>(x, y, z, posm, nullptr, cell_start, g, k, s);
   return s.rho;
}

// The pixel's ray and its box interval; false for a miss (len 0 or not finite, or tnear > tfar / NaN).
__device__ __forceinline__ bool render_ray(const RenderFrame& F, int px, int py, float d[3], float& tnear,
                                           float& tfar)
{
   const float a = (float)(2 * px + 1 - F.width) / (float)F.width;
   const float b = (float)(F.height - 2 * py - 1) / (float)F.height;
   float dc[3];
#pragma unroll
   for (int c = 0; c < 3; c++) dc[c] = (F.cam.forward[c] + a * F.cam.right[c]) + b * F.cam.up[c];
   const float len = sqrtf((dc[0] * dc[0] + dc[1] * dc[1]) + dc[2] * dc[2]);
   if (!(len > 0.0f) || !isfinite(len)) return false;
   float nr[3], fr[3];
#pragma unroll
   for (int c = 0; c < 3; c++) {
      d[c] = dc[c] / len;
      const float inv = 1.0f / d[c];
      const float t0 = (F.rp.box_lo[c] - F.cam.eye[c]) * inv;
      const float t1 = (F.rp.box_hi[c] - F.cam.eye[c]) * inv;
      nr[c] = fminf(t0, t1);
      fr[c] = fmaxf(t0, t1);
   }
   tnear = fmaxf(fmaxf(fmaxf(nr[0], nr[1]), nr[2]), 0.0f);
   tfar = fminf(fminf(fr[0], fr[1]), fr[2]);
   return tnear <= tfar;
}

__device__ __forceinline__ uint32_t render_background(const RenderFrame& F)
{
   return (uint32_t)F.rp.background[0] | ((uint32_t)F.rp.background[1] << 8) |
          ((uint32_t)F.rp.background[2] << 16) | ((uint32_t)F.rp.background[3] << 24);
}

// ---- march: one wave per 8 x 8 tile of the chunk ---------------------------------------------------------
// Outputs are indexed by the pixel's place in the chunk, (py - row0) * width + px.
template <bool UNIT_SCALE, bool SKIP>
__global__ void __launch_bounds__(RENDER_THREADS)
k_render_march(RenderFrame F, const float4* __restrict__ posm, const uint32_t* __restrict__ cell_start, CellGrid g,
               PairConsts k, const unsigned char* __restrict__ occ, uint32_t* __restrict__ rgba_out,
               float* __restrict__ depth_out, float* __restrict__ normal_out, float* __restrict__ vel_out,
               int32_t* __restrict__ first_out, int32_t* __restrict__ hits, uint32_t* __restrict__ hit_count)
{
   const int lane = threadIdx.x % SPH_WAVE;
   const int tile = blockIdx.x * (RENDER_THREADS / SPH_WAVE) + threadIdx.x / SPH_WAVE;
   const int tx = tile % F.tiles_x, ty = tile / F.tiles_x;
   const int px = tx * RENDER_TILE + lane % RENDER_TILE;
   const int ly = ty * RENDER_TILE + lane / RENDER_TILE;
   const bool valid = px < F.width && ly < F.rows;
   int first = -1;
   if (valid) {
      float d[3], tnear, tfar;
      if (render_ray(F, px, F.row0 + ly, d, tnear, tfar)) {
         const float step = F.rp.step, iso = F.rp.iso;
         for (int s = 0; s < F.rp.max_samples; s++) {
            const float t = tnear + (float)s * step;
            if (!(t <= tfar)) break;
            const float x = F.cam.eye[0] + t * d[0];
            const float y = F.cam.eye[1] + t * d[1];
            const float z = F.cam.eye[2] + t * d[2];
            if (render_field<UNIT_SCALE, SKIP>(x, y, z, posm, cell_start, g, k, occ) > iso) {
               first = s;
               break;
            }
         }
      }
   }
   const int o = ly * F.width + px;
   if (valid) {
      first_out[o] = first;
      if (first < 0) {
         rgba_out[o] = render_background(F);
         depth_out[o] = __int_as_float(0x7f800000);
#pragma unroll
         for (int c = 0; c < 3; c++) {
            normal_out[3 * o + c] = 0.0f;
            vel_out[3 * o + c] = 0.0f;
         }
      }
   }
   // append the wave's hits to the list, one atomic per wave
   const bool hit = valid && first >= 0;
   const unsigned long long mask = __ballot(hit);
   if (mask == 0) return;
   uint32_t base = 0;
   if (lane == __ffsll((long long)mask) - 1) base = atomicAdd(hit_count, (uint32_t)__popcll(mask));
   base = __shfl(base, __ffsll((long long)mask) - 1);
   if (hit) hits[base + __popcll(mask & ((1ull << lane) - 1ull))] = o;
}

// ---- shade: one lane per listed hit ----------------------------------------------------------------------
template <bool UNIT_SCALE, bool SKIP, bool VEL>
__global__ void __launch_bounds__(RENDER_THREADS)
k_render_shade(RenderFrame F, const float4* __restrict__ posm, const float4* __restrict__ velp,
               const uint32_t* __restrict__ cell_start, CellGrid g, PairConsts k,
               const unsigned char* __restrict__ occ, const int32_t* __restrict__ hits,
               const uint32_t* __restrict__ hit_count, const int32_t* __restrict__ first_in,
               uint32_t* __restrict__ rgba_out, float* __restrict__ depth_out, float* __restrict__ normal_out,
               float* __restrict__ vel_out)
{
   const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i >= *hit_count) return;
   const int o = hits[i];
   const int px = o % F.width, py = F.row0 + o / F.width;
   float d[3], tnear, tfar;
   render_ray(F, px, py, d, tnear, tfar);   // a listed pixel's ray hit the box
   const int first = first_in[o];
   const float* eye = F.cam.eye;
   const float iso = F.rp.iso;
   // bisection between the last outside and the first inside sample
   float tb = tnear;
   if (first > 0) {
      float ta = tnear + (float)(first - 1) * F.rp.step;
      tb = tnear + (float)first * F.rp.step;
      for (int r = 0; r < F.rp.refine; r++) {
         const float tm = 0.5f * (ta + tb);
         const float f = render_field<UNIT_SCALE, SKIP>(eye[0] + tm * d[0], eye[1] + tm * d[1], eye[2] + tm * d[2],
                                                        posm, cell_start, g, k, occ);
         if (f > iso) tb = tm;
         else ta = tm;
      }
   }
   const float p[3] = {eye[0] + tb * d[0], eye[1] + tb * d[1], eye[2] + tb * d[2]};
   // normal: central differences, toward lower density
   const float gs = F.rp.grad_step, two = 2.0f * gs;
   float gr[3];
#pragma unroll 1
   for (int a = 0; a < 3; a++) {
      float q[3] = {p[0], p[1], p[2]};
      q[a] = p[a] + gs;
      const float fp = render_field<UNIT_SCALE, SKIP>(q[0], q[1], q[2], posm, cell_start, g, k, occ);
      q[a] = p[a] - gs;
      const float fm = render_field<UNIT_SCALE, SKIP>(q[0], q[1], q[2], posm, cell_start, g, k, occ);
      gr[a] = (fp - fm) / two;
   }
   const float glen = sqrtf((gr[0] * gr[0] + gr[1] * gr[1]) + gr[2] * gr[2]);
   const bool gok = glen > 0.0f && isfinite(glen);
   float n[3];
#pragma unroll
   for (int a = 0; a < 3; a++) n[a] = gok ? -(gr[a] / glen) : 0.0f;
   // shade
   const float* L = F.rp.light;
   const float llen = sqrtf((L[0] * L[0] + L[1] * L[1]) + L[2] * L[2]);
   const float l[3] = {L[0] / llen, L[1] / llen, L[2] / llen};
   const float ndl = (n[0] * l[0] + n[1] * l[1]) + n[2] * l[2];
   const float w = F.rp.ambient + F.rp.diffuse * fmaxf(ndl, 0.0f);
   uint32_t rgba = 255u << 24;
#pragma unroll
   for (int c = 0; c < 3; c++) rgba |= (uint32_t)render_byte(F.rp.albedo[c] * w) << (8 * c);
   rgba_out[o] = rgba;
   depth_out[o] = tb;
#pragma unroll
   for (int a = 0; a < 3; a++) normal_out[3 * o + a] = n[a];
   float v[3] = {0.0f, 0.0f, 0.0f};
   if (VEL) {
      int cx, cy, cz;
      probe_cell(g, p[0], p[1], p[2], cx, cy, cz);
      if (!SKIP || occ[(cz * g.ny + cy) * g.nx + cx]) {
         SampleSum<true> s;
         sample_walk<UNIT_SCALE>(p[0], p[1], p[2], posm, velp, cell_start, g, k, s);
         if (s.rho > 0.0f) {
            v[0] = s.vx / s.rho;
            v[1] = s.vy / s.rho;
            v[2] = s.vz / s.rho;
         }
      }
   }
#pragma unroll
   for (int a = 0; a < 3; a++) vel_out[3 * o + a] = v[a];
}
