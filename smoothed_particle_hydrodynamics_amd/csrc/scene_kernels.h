// Scene renderer: the context's solids drawn into the renderer's frame (sph_hip_render_scene;
// include/sph_hip.h states the contract, scene_policy.h holds its functions, and
// tests/test_gpu_scene_render.py pins the device to the numpy restatement tests/scene_emulation.py).
//
// k_scene_solids runs behind k_render_shade on each row chunk, one lane per chunk pixel in the march's
// layout - one wave per 8 x 8 pixel tile, so that a wave's rays meet the same solid and branch
// together.  The solids (at most 64 of 72 bytes: obstacle, velocity, albedo) come from a device buffer
// the host fills before the first chunk; the workgroup's first wave copies them to LDS once.  Each
// lane finds its ray's nearest solid analytically and, where that lies strictly in front of the fluid's
// depth, overwrites the pixel's outputs; solid_id is written for every pixel.  No atomics.
#pragma once

#include "render_kernels.h"
#include "scene_policy.h"

#define SCENE_SOLID_WORDS (int)(sizeof(SceneSolid) / sizeof(uint32_t))

// the LDS copy of the list, as scene_nearest_of reads it
struct SceneLdsList {
   const SceneSolid* s;
   __device__ const sph_hip_obstacle& operator()(int i) const { return s[i].o; }
};

// FILL: no fluid pass ran on this chunk (no particle is resident) - every pixel is written, a pixel no
// solid takes as the renderer's miss.
template <bool FILL>
__global__ void __launch_bounds__(RENDER_THREADS)
k_scene_solids(RenderFrame F, sph_hip_scene_params sp, const uint32_t* __restrict__ list, int n_solids, int vel,
               uint32_t* __restrict__ rgba_out, float* __restrict__ depth_out, float* __restrict__ normal_out,
               float* __restrict__ vel_out, int32_t* __restrict__ first_out, int32_t* __restrict__ id_out)
{
   __shared__ uint32_t lds[SPH_HIP_MAX_OBSTACLES * SCENE_SOLID_WORDS];
   if (threadIdx.x < SPH_WAVE)
      for (int i = threadIdx.x; i < n_solids * SCENE_SOLID_WORDS; i += SPH_WAVE) lds[i] = list[i];
   __syncthreads();
   const SceneSolid* solids = reinterpret_cast<const SceneSolid*>(lds);

   const int lane = threadIdx.x % SPH_WAVE;
   const int tile = blockIdx.x * (RENDER_THREADS / SPH_WAVE) + threadIdx.x / SPH_WAVE;
   const int tx = tile % F.tiles_x, ty = tile / F.tiles_x;
   const int px = tx * RENDER_TILE + lane % RENDER_TILE;
   const int ly = ty * RENDER_TILE + lane / RENDER_TILE;
   if (px >= F.width || ly >= F.rows) return;
   const int o = ly * F.width + px;

   float d[3], t = 0.0f, n[3] = {0.0f, 0.0f, 0.0f};
   int id = -1;
   if (scene_pixel_dir(F.cam, F.width, F.height, px, F.row0 + ly, d))
      scene_nearest_of(SceneLdsList{solids}, n_solids, F.cam.eye, d, t, n, id);
   const float fluid = FILL ? __int_as_float(0x7f800000) : depth_out[o];
   if (id >= 0 && !scene_in_front(t, fluid)) id = -1;
   id_out[o] = id;
   if (id >= 0) {
      const SceneSolid& s = solids[id];
      rgba_out[o] = scene_shade(n, F.rp.light, s.alb, sp.ambient, sp.diffuse);
      depth_out[o] = t;
      first_out[o] = -1;
#pragma unroll
      for (int c = 0; c < 3; c++) normal_out[3 * o + c] = n[c];
      if (vel) {
#pragma unroll
         for (int c = 0; c < 3; c++) vel_out[3 * o + c] = s.vel[c];
      }
   } else if (FILL) {
      rgba_out[o] = render_background(F);
      depth_out[o] = __int_as_float(0x7f800000);
      first_out[o] = -1;
#pragma unroll
      for (int c = 0; c < 3; c++) {
         normal_out[3 * o + c] = 0.0f;
         vel_out[3 * o + c] = 0.0f;
      }
   }
}
