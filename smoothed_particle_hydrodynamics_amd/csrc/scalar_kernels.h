// Carried scalars (include/sph_hip.h: carried scalars; the contract and every check: scalar_policy.h; the
// routes: launch_policy.h): the stage that brings the scalars to the sorted slots, the pass that advances
// them, and the channel sums of the sampler's walk (with them the sampler's own kernels are the point and
// lattice samplers of the channels: sample_kernels.h).
//
// The scalars live by particle ID (T[id], the id in velp.w) and never ride through the cell build.  A step
// stages Ts[p] = T[id(p)] and Vs[p] = m / rho for the sorted slots of its state S_k (k_scalars_stage), then
// k_scalars_step - a third consumer of the neighbour lists the density pass left for the acceleration pass -
// sums over every particle's neighbours and writes T[id(p)] in place: it reads Ts and Vs only, so nothing
// races.  A lane takes its list a block of eight entries per trip, the next block requested before this one's
// gathers (accel_from_lists' loop: full_tiled.h); a workgroup or a lane without a list walks the nine cell
// rows as k_particle_density does.  Same pairs, same order, same arithmetic: same bits.  No kernel here
// writes anything of the particle state; the only LDS is the step kernel's copy of its TileDesc, and every
// local array is indexed by unrolled constants (none lives in scratch memory).
#pragma once

#include "cell_build.h"
#include "full_tiled.h"
#include "neighbor_lists.h"
#include "sample_kernels.h"
#include "scalar_policy.h"

static_assert(SCALAR_FLAG_LISTS_NONE == LISTS_NONE && SCALAR_FLAG_LISTS_SOME == LISTS_SOME &&
                 SCALAR_WORD_NO_LIST == NLIST_NO_LIST,
              "launch_policy.h restates the list flags of neighbor_lists.h");
static_assert(sizeof(Scalar4) == sizeof(float4), "a particle's channels are one float4");

__device__ __forceinline__ Scalar4 scalar4_of(const float4& v) { return Scalar4{v.x, v.y, v.z, v.w}; }
__device__ __forceinline__ float4 float4_of(const Scalar4& v) { return make_float4(v.c0, v.c1, v.c2, v.c3); }

// ---- stage: one lane per sorted particle --------------------------------------------------------------------
// Ts[p] = T[id(p)] (zeros for an id outside the rows: a dead entry), and with rho the volumes Vs[p] (the
// samplers pass rho = Vs = nullptr: they need the channels only).
__global__ void __launch_bounds__(256)
k_scalars_stage(const float4* __restrict__ posm, const float4* __restrict__ velp, const float* __restrict__ rho,
                const int32_t* __restrict__ meta, const float4* __restrict__ T, int n_rows, float4* __restrict__ Ts,
                float* __restrict__ Vs)
{
   const int p = meta[META_SUM_BEGIN] + blockIdx.x * blockDim.x + threadIdx.x;
   if (p >= meta[META_SUM_END]) return;
   const uint32_t id = __float_as_uint(velp[p].w);
   Ts[p] = id < (uint32_t)n_rows ? T[id] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
   if (Vs) Vs[p] = scalar_volume(posm[p].w, rho[p]);
}

// ---- the pass: one workgroup per 256 sorted particles ----------------------------------------------------------
// one neighbour's operands into the sums
template <bool UNIT_SCALE>
__device__ __forceinline__ void scalars_add(const ScalarStep& st, const float4& pi, const Scalar4& Ti, const float4& pj,
                                            const float4& tj, float vj, Scalar4& s)
{
   float dx, dy, dz;
   float d = sqrt_rn(dist2(pi.x, pi.y, pi.z, pj.x, pj.y, pj.z, dx, dy, dz));
   if (!UNIT_SCALE) d *= st.sim_scale;
   scalar_pair(s, Ti, scalar4_of(tj), vj, d, st.hscaled, st.kernel3);
}

// the list walk of one lane (accel_from_lists' tolerance-mode loop: one 16-byte load per eight entries)
template <bool UNIT_SCALE, bool WIDE>
__device__ __forceinline__ void scalars_from_lists(int cnt, const ListReader& lr, const TileDesc& d, const ScalarStep& st,
                                                   const float4& pi, const Scalar4& Ti, const float4* __restrict__ posm,
                                                   const float4* __restrict__ Ts, const float* __restrict__ Vs, Scalar4& s)
{
   const int lastb = cnt > 0 ? (cnt - 1) >> 3 : 0;
   uint4 blk = lr.block(0);
   for (int j0 = 0; j0 < cnt; j0 += 8) {
      uint32_t entry[8];
      list_block_entries(blk, entry);
      blk = lr.block(min((j0 >> 3) + 1, lastb));
      float4 pj[8], tj[8];
      float vj[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
         const uint32_t e = j0 + u < cnt ? entry[u] : entry[0];      // (entry 0 of a block in use is a neighbour)
         const int q = ListEntry<WIDE>::tile(e) - ListEntry<WIDE>::shift(d, e);
         pj[u] = posm[q];
         tj[u] = Ts[q];
         vj[u] = Vs[q];
      }
#pragma unroll
      for (int u = 0; u < 8; u++)
         if (j0 + u < cnt) scalars_add<UNIT_SCALE>(st, pi, Ti, pj[u], tj[u], vj[u], s);
   }
}

// the row walk of one lane (k_particle_density's: pressure_kernels.h)
template <bool UNIT_SCALE>
__device__ __forceinline__ void scalars_from_rows(int p, const CellGrid& g, const uint32_t* __restrict__ cell_start, float h2,
                                                  const ScalarStep& st, const float4& pi, const Scalar4& Ti,
                                                  const float4* __restrict__ posm, const float4* __restrict__ Ts,
                                                  const float* __restrict__ Vs, Scalar4& s)
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
         if (d2 < h2) scalars_add<UNIT_SCALE>(st, pi, Ti, pj, Ts[q], Vs[q], s);
      }
   }
}

// tiled: the context's density pass wrote lists and flags (else nlist, nlist_overflow, desc are not read);
// force_rows: every workgroup walks the rows (launch_policy.h: scalar_workgroup_route)
template <bool UNIT_SCALE, bool WIDE>
__global__ void __launch_bounds__(TILE_THREADS)
k_scalars_step(const float4* __restrict__ posm, const float4* __restrict__ velp, const float4* __restrict__ Ts,
               const float* __restrict__ Vs, const int32_t* __restrict__ ncount, const uint32_t* __restrict__ cell_start,
               const int32_t* __restrict__ meta, CellGrid g, float h2, ScalarStep st, const TileDesc* __restrict__ desc,
               const uint32_t* __restrict__ nlist, const uint32_t* __restrict__ nlist_overflow, int list_cap, int tiled,
               int force_rows, float4* __restrict__ T, int n_rows)
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
   const int wg_route = scalar_workgroup_route(tiled != 0, force_rows != 0, flag);
   if (wg_route == SCALAR_ROUTE_LISTS) tile_desc_load(desc, wg, sd);
   if (!live) return;

   const float4 pi = posm[p];
   const Scalar4 Ti = scalar4_of(Ts[p]);
   Scalar4 s = {0.0f, 0.0f, 0.0f, 0.0f};
   int lane_route = SCALAR_ROUTE_ROWS;
   if (wg_route == SCALAR_ROUTE_LISTS) {
      const int cnt = ncount[p];
      const ListReader lr(nlist, wg, list_cap, tid);
      const uint32_t first_word = (flag == LISTS_SOME && cnt > 0) ? (lr.no_list() ? NLIST_NO_LIST : 0u) : 0u;
      lane_route = scalar_lane_route(wg_route, flag, cnt, first_word);
      if (lane_route == SCALAR_ROUTE_LISTS) scalars_from_lists<UNIT_SCALE, WIDE>(cnt, lr, sd, st, pi, Ti, posm, Ts, Vs, s);
   }
   if (lane_route == SCALAR_ROUTE_ROWS) scalars_from_rows<UNIT_SCALE>(p, g, cell_start, h2, st, pi, Ti, posm, Ts, Vs, s);

   const Scalar4 out = scalar_finish(Ti, s, st, pi.x, pi.y, pi.z);
   const uint32_t id = __float_as_uint(velp[p].w);
   if (id < (uint32_t)n_rows) T[id] = float4_of(out);
}

// ---- the channel sums of the sampler's walk (sample_kernels.h) -------------------------------------------------
// accumulator of one probe: the sampler's rho and count, and a_c = sum of t_j * T_j,c
struct ScalarSum {
   float rho = 0.0f, a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
   int count = 0;

   using Payload = float4;   // Ts: the channels of sorted particle q (k_scalars_stage)
   struct Out {
      float4* chan;
      float* rho;
      int32_t* cnt;
   };

   template <bool UNIT_SCALE>
   __device__ __forceinline__ void member(const PairConsts& k, float d2, float m, const float4* __restrict__ Ts,
                                          uint32_t q)
   {
      add<UNIT_SCALE>(k, d2, m, Ts[q]);
   }

   template <bool UNIT_SCALE>
   __device__ __forceinline__ void add(const PairConsts& k, float d2, float m, const float4& tj)
   {
      float d = sqrt_rn(d2);   // (as SampleSum::add: sample_kernels.h)
      if (!UNIT_SCALE) d *= k.sim_scale;
      const float t = density_term<UNIT_SCALE>(k, m, d);
      rho += t;
      a0 += t * tj.x;
      a1 += t * tj.y;
      a2 += t * tj.z;
      a3 += t * tj.w;
      count++;
   }

   __device__ __forceinline__ void store(int o, const Out& out) const
   {
      out.chan[o] = make_float4(scalar_shepard(a0, rho), scalar_shepard(a1, rho), scalar_shepard(a2, rho),
                                scalar_shepard(a3, rho));
      out.rho[o] = rho;
      out.cnt[o] = count;
   }
};
