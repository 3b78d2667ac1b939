// Viscous stress (include/sph_hip.h: viscous stress; the contract and every check: viscous_policy.h; the decision:
// launch_policy.h, step_launches_viscous): two kernels between a step's acceleration pass and its integrate, behind
// cohesion's and in front of XSPH's and buoyancy's.  No existing kernel changes: the integrate of the context,
// whichever form launch_integrate picks, runs behind them from the rows they leave.
//
// k_viscous_stage is k_xsph_stage's shape (xsph_kernels.h): one lane per live sorted slot writes R[p] = {v, m / rho}
// and, with a law, M[p] = mu * factor(Ts[p].c).  k_viscous_apply is a consumer of the neighbour lists the density pass
// left for the acceleration pass, and its walk is pair_walk.h's - in a copy of its own: on the shared walk the compiler
// allotted its instantiations 100 and 114 vector registers for 102 and 112 and packed the pair arithmetic of two of
// them differently (the pair walk), and a pass moves there only with the registers and the arithmetic it
// has.  A fix to pair_walk.h's workgroup step, list walk or row walk is to be made here too.  It gathers posm[q] and
// R[q] - 32 bytes per neighbour in two streams - and with a law M[q], 36 bytes in three; it reads and writes its own
// acc[p] only.  So nothing races, and every sum reads S_k's velocities.  The only LDS is its copy of its TileDesc,
// and every local array is indexed by unrolled constants (none lives in scratch memory).
//
// Nothing between the density pass and these kernels writes what they read: posm[cur], ncount, nlist,
// nlist_overflow and tile_desc are written by the cell build and the density kernels only, rho by the density
// kernels only, Ts by the scalar pass's stage only, velp[cur] of an unfused step by nothing in front of XSPH, and R
// and M by k_viscous_stage only (viscous stress, "The premise").
#pragma once

#include "cell_build.h"
#include "full_tiled.h"
#include "neighbor_lists.h"
#include "pair_math.h"
#include "viscous_policy.h"

static_assert(sizeof(ViscousRow) == sizeof(float4), "a staged row is one float4");

__device__ __forceinline__ ViscousRow viscous_row_of(const float4& v) { return ViscousRow{v.x, v.y, v.z, v.w}; }

// ---- stage: one lane per sorted particle --------------------------------------------------------------------
// LAW: Ts and M are read and written (else they are not touched and may be null); mu and the law arrive by value
template <bool LAW>
__global__ void __launch_bounds__(256)
k_viscous_stage(const float4* __restrict__ velp, const float4* __restrict__ posm, const float* __restrict__ rho,
                const int32_t* __restrict__ meta, const float4* __restrict__ Ts, float mu, sph_hip_viscosity_law law,
                float4* __restrict__ R, float* __restrict__ M)
{
   const int p = meta[META_SUM_BEGIN] + blockIdx.x * blockDim.x + threadIdx.x;
   if (p >= meta[META_SUM_END]) return;
   const float4 v = velp[p];
   const ViscousRow r = viscous_stage(v.x, v.y, v.z, posm[p].w, rho[p]);
   R[p] = make_float4(r.x, r.y, r.z, r.w);
   if (LAW) {
      const float4 t = Ts[p];
      M[p] = viscous_stage_mu(mu, law, viscous_channel(law.channel, t.x, t.y, t.z, t.w));
   }
}

// ---- the pass: one workgroup per 256 sorted particles ----------------------------------------------------------
// one neighbour into the sum
template <bool UNIT_SCALE, bool LAW>
__device__ __forceinline__ void viscous_add(const PairConsts& k, float mu, const float4& pi, const ViscousRow& Ri, float Mi,
                                            const float4& pj, const float4& rj, float mj, ViscousSum& s)
{
   float dx, dy, dz;
   float d = sqrt_rn(dist2(pi.x, pi.y, pi.z, pj.x, pj.y, pj.z, dx, dy, dz));
   if (!UNIT_SCALE) d *= k.sim_scale;
   viscous_pair(s, viscous_pair_mu(LAW, mu, Mi, mj), d, k.hscaled, k.kernel3, Ri, viscous_row_of(rj));
}

// the list walk of one lane (pair_walk_lists' loop, pair_walk.h: one 16-byte load per eight entries)
template <bool UNIT_SCALE, bool WIDE, bool LAW>
__device__ __forceinline__ void viscous_from_lists(int cnt, const ListReader& lr, const TileDesc& d, const PairConsts& k,
                                                   float mu, const float4& pi, const ViscousRow& Ri, float Mi,
                                                   const float4* __restrict__ posm, const float4* __restrict__ R,
                                                   const float* __restrict__ M, ViscousSum& s)
{
   const int lastb = cnt > 0 ? (cnt - 1) >> 3 : 0;
   uint4 blk = lr.block(0);
   for (int j0 = 0; j0 < cnt; j0 += 8) {
      uint32_t entry[8];
      list_block_entries(blk, entry);
      blk = lr.block(min((j0 >> 3) + 1, lastb));
      float4 pj[8], rj[8];
      float mj[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
         const uint32_t e = j0 + u < cnt ? entry[u] : entry[0];      // (entry 0 of a block in use is a neighbour)
         const int q = ListEntry<WIDE>::tile(e) - ListEntry<WIDE>::shift(d, e);
         pj[u] = posm[q];
         rj[u] = R[q];
         mj[u] = LAW ? M[q] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < 8; u++)
         if (j0 + u < cnt) viscous_add<UNIT_SCALE, LAW>(k, mu, pi, Ri, Mi, pj[u], rj[u], mj[u], s);
   }
}

// the row walk of one lane (pair_walk_rows', pair_walk.h)
template <bool UNIT_SCALE, bool LAW>
__device__ __forceinline__ void viscous_from_rows(int p, const CellGrid& g, const uint32_t* __restrict__ cell_start,
                                                  const PairConsts& k, float mu, const float4& pi, const ViscousRow& Ri,
                                                  float Mi, const float4* __restrict__ posm, const float4* __restrict__ R,
                                                  const float* __restrict__ M, ViscousSum& s)
{
   int cx, cy, cz;
   cell_of(g, pi.x, pi.y, pi.z, cx, cy, cz);
   RowRanges r;
   row_ranges(g, cell_start, cx, cy, cz, r);
#pragma unroll 1
   for (int row = 0; row < 9; row++) {
      uint32_t b, e;
      row_range(r, row, b, e);
      for (uint32_t q = b; q < e; q++) {
         if (q == (uint32_t)p) continue;
         const float4 pj = posm[q];
         float dx, dy, dz;
         const float d2 = dist2(pi.x, pi.y, pi.z, pj.x, pj.y, pj.z, dx, dy, dz);
         if (d2 < k.h2) viscous_add<UNIT_SCALE, LAW>(k, mu, pi, Ri, Mi, pj, R[q], LAW ? M[q] : 0.0f, s);
      }
   }
}

// One workgroup per 256 sorted particles of the live range.  tiled: the context's density pass wrote lists and
// flags (else nlist, nlist_overflow, desc are not read).  LAW: M is read (else it is not and may be null).  mu and
// the constants arrive by value: a later setter does not reach the steps already queued.
template <bool UNIT_SCALE, bool WIDE, bool LAW>
__global__ void __launch_bounds__(TILE_THREADS)
k_viscous_apply(const float4* __restrict__ posm, const float4* __restrict__ R, const float* __restrict__ M,
                const int32_t* __restrict__ ncount, const uint32_t* __restrict__ cell_start,
                const int32_t* __restrict__ meta, CellGrid g, PairConsts k, float mu, const TileDesc* __restrict__ desc,
                const uint32_t* __restrict__ nlist, const uint32_t* __restrict__ nlist_overflow, int list_cap, int tiled,
                float4* __restrict__ acc)
{
   __shared__ TileDesc sd;
   const int begin = meta[META_SUM_BEGIN], end = meta[META_SUM_END];
   const int tid = threadIdx.x;
   const int wg = xcd_workgroup(blockIdx.x, gridDim.x);
   const int p0 = begin + wg * TILE_THREADS;
   if (p0 >= end) return;   // (the whole workgroup)
   const int p = p0 + tid;
   const bool live = p < end;
   // (workgroup-uniform: the barrier inside tile_desc_load is reached by every lane or by none)
   const uint32_t flag = tiled ? nlist_overflow[wg] : LISTS_NONE;
   const int wg_route = scalar_workgroup_route(tiled != 0, false, flag);
   if (wg_route == SCALAR_ROUTE_LISTS) tile_desc_load(desc, wg, sd);
   if (!live) return;

   const float4 pi = posm[p];
   const ViscousRow Ri = viscous_row_of(R[p]);
   const float Mi = LAW ? M[p] : 0.0f;
   ViscousSum s = {0.0f, 0.0f, 0.0f};
   int lane_route = SCALAR_ROUTE_ROWS;
   if (wg_route == SCALAR_ROUTE_LISTS) {
      const int cnt = ncount[p];
      const ListReader lr(nlist, wg, list_cap, tid);
      const uint32_t first_word = (flag == LISTS_SOME && cnt > 0) ? (lr.no_list() ? NLIST_NO_LIST : 0u) : 0u;
      lane_route = scalar_lane_route(wg_route, flag, cnt, first_word);
      if (lane_route == SCALAR_ROUTE_LISTS)
         viscous_from_lists<UNIT_SCALE, WIDE, LAW>(cnt, lr, sd, k, mu, pi, Ri, Mi, posm, R, M, s);
   }
   if (lane_route == SCALAR_ROUTE_ROWS) viscous_from_rows<UNIT_SCALE, LAW>(p, g, cell_start, k, mu, pi, Ri, Mi, posm, R, M, s);

   const ViscousSum c = viscous_accel(s, pi.w);
   if (!viscous_acts(Ri.w, pi.w, c)) return;
   float4 a = acc[p];
   viscous_apply(c, k.cfl_limit, k.cfl_limit2, a.x, a.y, a.z);
   acc[p] = a;
}
