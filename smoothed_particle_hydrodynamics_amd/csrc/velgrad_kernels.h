// Velocity gradients (include/sph_hip.h: velocity gradients; the contract and every check: velgrad_policy.h): one
// per-particle pair kernel outside the step, behind a cell build of the current state, and the copy of its rows into
// particle-id order for the getter.  No existing kernel changes, and a context that never asks launches neither.
//
// k_velgrad_particles is pair_walk_rows' walk (pair_walk.h), which is k_particle_density's (pressure_kernels.h), in a
// copy of its own - on the shared walk the compiler vectorised its fifteen sums differently, with two more vector
// registers (the pair walk): the nine cell rows of the particle's cell, itself skipped, the d2 < h2 test in
// front of the second gather.  It gathers posm[q] - 16 bytes, the mass in .w - for every candidate and velp[q] for members only.
// There is no neighbour-list route: by the time a caller can ask, the lists are those of the state before the last
// integrate, and the cell build in front of this pass has moved the particles they index.  The kernel uses no LDS,
// its fifteen accumulators are named scalars (VelgradSums), and no local is indexed by anything but unrolled
// constants, so nothing lives in scratch memory.  It writes its own two arrays only.
#pragma once

#include "cell_build.h"
#include "full_tiled.h"
#include "pair_math.h"
#include "velgrad_policy.h"

// One workgroup per 256 sorted particles of the live range, spread over the XCDs as the sums' workgroups are.  The
// constants arrive by value.  rowA[p] = (w_x, w_y, w_z, div), rowB[p] = (strain, Q, |w|, valid) by sorted slot.
template <bool UNIT_SCALE>
__global__ void __launch_bounds__(TILE_THREADS)
k_velgrad_particles(const float4* __restrict__ posm, const float4* __restrict__ velp, const uint32_t* __restrict__ cell_start,
                    const int32_t* __restrict__ meta, CellGrid g, PairConsts k, float4* __restrict__ rowA,
                    float4* __restrict__ rowB)
{
   const int begin = meta[META_SUM_BEGIN], end = meta[META_SUM_END];
   const int wg = xcd_workgroup(blockIdx.x, gridDim.x);
   const int p = begin + wg * TILE_THREADS + (int)threadIdx.x;
   if (p >= end) return;

   const float4 pi = posm[p];
   const float4 vi = velp[p];
   int cx, cy, cz;
   cell_of(g, pi.x, pi.y, pi.z, cx, cy, cz);
   RowRanges r;
   row_ranges(g, cell_start, cx, cy, cz, r);
   VelgradSums s = velgrad_zero();
#pragma unroll 1
   for (int row = 0; row < 9; row++) {
      uint32_t b, e;
      row_range(r, row, b, e);
      for (uint32_t q = b; q < e; q++) {
         if (q == (uint32_t)p) continue;
         const float4 pj = posm[q];
         float dx, dy, dz;
         const float d2 = dist2(pi.x, pi.y, pi.z, pj.x, pj.y, pj.z, dx, dy, dz);
         if (d2 < k.h2) {
            const float4 vj = velp[q];
            float d = sqrt_rn(d2);
            if (!UNIT_SCALE) d *= k.sim_scale;
            const float w = density_term<UNIT_SCALE>(k, pj.w, d);
            velgrad_pair(s, w, dx, dy, dz, vi.x - vj.x, vi.y - vj.y, vi.z - vj.z, k.sim_scale, UNIT_SCALE);
         }
      }
   }
   const VelgradRows o = velgrad_finish(s);
   rowA[p] = make_float4(o.wx, o.wy, o.wz, o.div);
   rowB[p] = make_float4(o.strain, o.q, o.wmag, o.valid);
}

// One lane per sorted slot of the live range: both rows to the particle's id, the id from velp[p].w.  An id outside
// the n_rows rows of the output (a dead entry) copies nothing, as k_scalars_stage reads nothing for it.
__global__ void __launch_bounds__(256)
k_velgrad_unsort(const float4* __restrict__ velp, const int32_t* __restrict__ meta, const float4* __restrict__ rowA,
                 const float4* __restrict__ rowB, int n_rows, float4* __restrict__ outA, float4* __restrict__ outB)
{
   const int p = meta[META_SUM_BEGIN] + blockIdx.x * blockDim.x + threadIdx.x;
   if (p >= meta[META_SUM_END]) return;
   const uint32_t id = __float_as_uint(velp[p].w);
   if (id >= (uint32_t)n_rows) return;
   outA[id] = rowA[p];
   outB[id] = rowB[p];
}
