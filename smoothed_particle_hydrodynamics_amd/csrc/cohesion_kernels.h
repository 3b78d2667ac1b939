// Cohesion (include/sph_hip.h: cohesion; the contract and every check: cohesion_policy.h; the decision:
// launch_policy.h, step_launches_cohesion): one kernel between a step's acceleration pass and its integrate, in
// front of buoyancy's.  No existing kernel changes: the integrate of the context, whichever form launch_integrate
// picks, runs behind it from the rows it leaves.
//
// k_cohesion_apply is one of the consumers of the neighbour lists the density pass left for the acceleration pass:
// the walk, on either route, is pair_walk.h's.  It gathers posm[q] only - 16 bytes per neighbour, the mass in .w, no
// payload - and reads and writes its own acc[p] only, so nothing races.
//
// One kernel is enough because nothing between the density pass and the integrate of an unfused step writes what
// it reads: posm[cur], ncount, nlist, nlist_overflow and tile_desc are written by the cell build and the density
// kernels only (cohesion, "The premise"), and k_full_accel_lists / k_full_accel take them all const.
#pragma once

#include "cohesion_policy.h"
#include "pair_walk.h"

// the pass's accumulator (pair_walk.h): the weight of a pair is the density pass's own pair term
struct CohesionPairs {
   const PairConsts& k;
   CohesionSum s;

   struct Payload {};
   template <class Index>
   __device__ __forceinline__ Payload gather(Index) const { return Payload{}; }

   template <bool UNIT_SCALE>
   __device__ __forceinline__ void add(const float4& pi, const float4& pj, const Payload&)
   {
      float dx, dy, dz;
      float d = sqrt_rn(dist2(pi.x, pi.y, pi.z, pj.x, pj.y, pj.z, dx, dy, dz));
      if (!UNIT_SCALE) d *= k.sim_scale;
      const float w = density_term<UNIT_SCALE>(k, pj.w, d);
      cohesion_pair(s, w, dx, dy, dz, k.sim_scale, UNIT_SCALE);
   }
};

// One workgroup per 256 sorted particles of the live range.  tiled: the context's density pass wrote lists and
// flags (else nlist, nlist_overflow, desc are not read).  gamma and the constants arrive by value: a later setter
// does not reach the steps already queued.
template <bool UNIT_SCALE, bool WIDE>
__global__ void __launch_bounds__(TILE_THREADS)
k_cohesion_apply(const float4* __restrict__ posm, const int32_t* __restrict__ ncount, const uint32_t* __restrict__ cell_start,
                 const int32_t* __restrict__ meta, CellGrid g, PairConsts k, float gamma, const TileDesc* __restrict__ desc,
                 const uint32_t* __restrict__ nlist, const uint32_t* __restrict__ nlist_overflow, int list_cap, int tiled,
                 float4* __restrict__ acc)
{
   __shared__ TileDesc sd;
   const PairLane w = pair_workgroup(meta, tiled, 0, nlist_overflow, desc, sd);
   if (!w.live) return;
   const int p = w.p;

   const float4 pi = posm[p];
   CohesionPairs pairs = {k, {0.0f, 0.0f, 0.0f}};
   pair_walk<UNIT_SCALE, WIDE>(w, sd, ncount, nlist, list_cap, g, cell_start, k.h2, pi, posm, pairs);

   const CohesionSum c = cohesion_accel(gamma, pairs.s);
   if (!cohesion_acts(c)) return;
   float4 a = acc[p];
   cohesion_apply(c, k.cfl_limit, k.cfl_limit2, a.x, a.y, a.z);
   acc[p] = a;
}
