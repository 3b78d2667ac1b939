// XSPH velocity smoothing (include/sph_hip.h: xsph; the contract and every check: xsph_policy.h; the decision:
// launch_policy.h, step_launches_xsph): two kernels between a step's acceleration pass and its integrate, behind
// cohesion's and in front of buoyancy's.  No existing kernel changes: the integrate of the context, whichever form
// launch_integrate picks, runs behind them from the velocities they leave.
//
// k_xsph_stage is k_scalars_stage's shape (scalar_kernels.h): one lane per live sorted slot writes R[p] = {v, 1/rho}.
// k_xsph_apply is one of the consumers of the neighbour lists the density pass left for the acceleration pass: the
// walk, on either route, is pair_walk.h's.  It gathers posm[q] and R[q] - 32 bytes per neighbour, no division per
// pair - and never another particle's velp; it writes its own velp[p] only.  So nothing races, and every sum reads
// S_k's velocities (Jacobi, not Gauss-Seidel).
//
// Nothing between the density pass and these kernels writes what they read: posm[cur], ncount, nlist,
// nlist_overflow and tile_desc are written by the cell build and the density kernels only, rho by the density
// kernels only, and velp[cur] of an unfused step by nothing in front of buoyancy (xsph, "The premise").
#pragma once

#include "pair_walk.h"
#include "xsph_policy.h"

static_assert(sizeof(XsphRow) == sizeof(float4), "a staged row is one float4");

__device__ __forceinline__ XsphRow xsph_row_of(const float4& v) { return XsphRow{v.x, v.y, v.z, v.w}; }

// ---- stage: one lane per sorted particle --------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_xsph_stage(const float4* __restrict__ velp, const float* __restrict__ rho, const int32_t* __restrict__ meta,
             float4* __restrict__ R)
{
   const int p = meta[META_SUM_BEGIN] + blockIdx.x * blockDim.x + threadIdx.x;
   if (p >= meta[META_SUM_END]) return;
   const float4 v = velp[p];
   const XsphRow r = xsph_stage(v.x, v.y, v.z, rho[p]);
   R[p] = make_float4(r.x, r.y, r.z, r.w);
}

// ---- the pass: one workgroup per 256 sorted particles ----------------------------------------------------------
// the pass's accumulator (pair_walk.h): the weight of a pair is the density pass's own pair term, formed as
// cohesion's is
struct XsphPairs {
   const PairConsts& k;
   const float4* __restrict__ R;
   XsphRow Ri;
   XsphSum s;

   using Payload = float4;   // R: the staged row of sorted particle q (k_xsph_stage)
   template <class Index>
   __device__ __forceinline__ Payload gather(Index q) const { return R[q]; }

   template <bool UNIT_SCALE>
   __device__ __forceinline__ void add(const float4& pi, const float4& pj, const float4& rj)
   {
      float dx, dy, dz;
      float d = sqrt_rn(dist2(pi.x, pi.y, pi.z, pj.x, pj.y, pj.z, dx, dy, dz));
      if (!UNIT_SCALE) d *= k.sim_scale;
      const float w = density_term<UNIT_SCALE>(k, pj.w, d);
      xsph_pair(s, w, Ri, xsph_row_of(rj));
   }
};

// One workgroup per 256 sorted particles of the live range.  tiled: the context's density pass wrote lists and
// flags (else nlist, nlist_overflow, desc are not read).  eps and the constants arrive by value: a later setter
// does not reach the steps already queued.
template <bool UNIT_SCALE, bool WIDE>
__global__ void __launch_bounds__(TILE_THREADS)
k_xsph_apply(const float4* __restrict__ posm, const float4* __restrict__ R, const int32_t* __restrict__ ncount,
             const uint32_t* __restrict__ cell_start, const int32_t* __restrict__ meta, CellGrid g, PairConsts k, float eps,
             const TileDesc* __restrict__ desc, const uint32_t* __restrict__ nlist,
             const uint32_t* __restrict__ nlist_overflow, int list_cap, int tiled, float4* __restrict__ velp)
{
   __shared__ TileDesc sd;
   const PairLane w = pair_workgroup(meta, tiled, 0, nlist_overflow, desc, sd);
   if (!w.live) return;
   const int p = w.p;

   const float4 pi = posm[p];
   XsphPairs pairs = {k, R, xsph_row_of(R[p]), {0.0f, 0.0f, 0.0f}};
   pair_walk<UNIT_SCALE, WIDE>(w, sd, ncount, nlist, list_cap, g, cell_start, k.h2, pi, posm, pairs);

   const XsphSum dv = xsph_change(eps, pairs.s);
   if (!xsph_acts(dv)) return;
   float4 v = velp[p];   // (.w, the id, is stored back as it was read)
   xsph_apply(dv, v.x, v.y, v.z);
   velp[p] = v;
}
