// Implicit viscous stress (include/sph_hip.h: implicit viscous stress; the contract and every check:
// viscous_implicit_policy.h): the Jacobi sweeps of a context whose viscous setting carries a sweep count, in the place
// of k_viscous_apply - behind k_viscous_stage, which is launched unchanged, behind cohesion's kernel and in front of
// XSPH's and buoyancy's.  No existing kernel changes.
//
// k_viscous_sweep is one more consumer of the neighbour lists the density pass left for the acceleration pass, and
// its walk, on either route, is pair_walk.h's: with the shared walk every instantiation keeps the project's resource
// condition (implicit viscous stress has the figures), so it needs no copy of its own.  The payload is
// ScalarPairs' two-stream shape: the row Xa[q] of the sweep before and, with a law, M[q] - 32 bytes per neighbour
// behind posm[q], 36 with a law.  A sweep reads its own velp[p] and gathers nothing else of another particle; it
// writes its own Xb[p] (not LAST) or its own velp[p] (LAST).  Xa and Xb are different row sets (the ping-pong of
// viscous_implicit_policy.h), so nothing races and every sweep is Jacobi.  The only LDS is the kernel's copy of its
// TileDesc, and every local array is indexed by unrolled constants (none lives in scratch memory).
//
// Nothing between the density pass and these kernels writes what they read: posm[cur], ncount, nlist,
// nlist_overflow and tile_desc are written by the cell build and the density kernels only, M by k_viscous_stage
// only, velp[cur] of an unfused step by nothing in front of the last sweep, and each row set by the stage or the
// sweep before only.
#pragma once

#include "pair_walk.h"
#include "viscous_implicit_policy.h"
#include "viscous_kernels.h"

// the pass's accumulator (pair_walk.h)
template <bool LAW>
struct ViscousSweepPairs {
   const PairConsts& k;
   float mu;
   const float4* __restrict__ X;
   const float* __restrict__ M;
   float v0x, v0y, v0z, Vi, Mi;
   ViscousImplicitSum s;

   struct Payload {
      float4 x;   // Xa: the row of sorted particle q the sweep before left (k_viscous_stage for the first)
      float m;    // M: its staged viscosity (a law only)
   };
   template <class Index>
   __device__ __forceinline__ Payload gather(Index q) const { return Payload{X[q], LAW ? M[q] : 0.0f}; }

   template <bool UNIT_SCALE>
   __device__ __forceinline__ void add(const float4& pi, const float4& pj, const Payload& j)
   {
      float dx, dy, dz;
      float d = sqrt_rn(dist2(pi.x, pi.y, pi.z, pj.x, pj.y, pj.z, dx, dy, dz));
      if (!UNIT_SCALE) d *= k.sim_scale;
      viscous_implicit_pair(s, viscous_pair_mu(LAW, mu, Mi, j.m), d, k.hscaled, k.kernel3, v0x, v0y, v0z, Vi,
                            viscous_row_of(j.x));
   }
};

// One workgroup per 256 sorted particles of the live range.  tiled: the context's density pass wrote lists and
// flags (else nlist, nlist_overflow, desc are not read).  LAW: M is read (else it is not and may be null).  A sweep
// that is not LAST reads the particle's velocity from vel (velp[cur]) and writes its row to out (Xb); the LAST one
// reads and writes out (velp[cur]) and is handed no vel: the one pointer the kernel writes is the one it reads its
// own slot of.  mu and the constants arrive by value: a later setter does not reach the steps already queued.
template <bool UNIT_SCALE, bool WIDE, bool LAW, bool LAST>
__global__ void __launch_bounds__(TILE_THREADS)
k_viscous_sweep(const float4* __restrict__ posm, const float4* __restrict__ vel, const float4* __restrict__ Xa,
                const float* __restrict__ M, const int32_t* __restrict__ ncount, const uint32_t* __restrict__ cell_start,
                const int32_t* __restrict__ meta, CellGrid g, PairConsts k, float mu, const TileDesc* __restrict__ desc,
                const uint32_t* __restrict__ nlist, const uint32_t* __restrict__ nlist_overflow, int list_cap, int tiled,
                float4* __restrict__ out)
{
   __shared__ TileDesc sd;
   const PairLane w = pair_workgroup(meta, tiled, 0, nlist_overflow, desc, sd);
   if (!w.live) return;
   const int p = w.p;

   const float4 pi = posm[p];
   const float4 v = LAST ? out[p] : vel[p];   // (.w, the id, is stored back as it was read)
   const float Vi = Xa[p].w;
   ViscousSweepPairs<LAW> pairs = {k, mu, Xa, M, v.x, v.y, v.z, Vi, LAW ? M[p] : 0.0f, {0.0f, 0.0f, 0.0f, 0.0f}};
   pair_walk<UNIT_SCALE, WIDE>(w, sd, ncount, nlist, list_cap, g, cell_start, k.h2, pi, posm, pairs);

   const float den = viscous_implicit_den(pairs.s, pi.w, k.dt);
   const ViscousSum dv = viscous_implicit_change(pairs.s, den, k.dt);
   const bool acts = viscous_implicit_acts(Vi, pi.w, den, dv);
   if (LAST) {
      if (acts) out[p] = make_float4(v.x + dv.x, v.y + dv.y, v.z + dv.z, v.w);
   } else {
      const ViscousRow r = viscous_implicit_row(acts, v.x, v.y, v.z, dv, Vi);
      out[p] = make_float4(r.x, r.y, r.z, r.w);
   }
}
