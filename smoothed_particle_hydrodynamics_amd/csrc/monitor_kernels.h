// Step monitor (include/sph_hip.h: step monitor; the contract and every check: monitor_policy.h; the grid:
// launch_policy.h, monitor_grid): three kernels on the steps that fill a row of a recording, none on any other
// step.  No existing kernel changes, and nothing here writes anything of the particle state.
//
// k_monitor_particles runs behind the step's integrate on either route (the fused acceleration pass stores acc[p]
// too: full_tiled.h) and streams the state the step produced - posm[cur], velp[cur] - with the step's acc, rho and
// ncount, 72 bytes per slot, and T by id where the context carries scalars.  A bounded grid strides over the live
// range the integrate itself took (META_OWN_BEGIN .. META_OWN_END); a lane reduces in registers, a wave by
// shuffles (an int64 as two halves), a workgroup through LDS, and every workgroup stores ONE partial row.  The row
// takes no atomics: six contended atomics per workgroup are what full_tiled.h measured away.
//
// k_monitor_pairs is k_cohesion_apply's skeleton (cohesion_kernels.h) - a fifth consumer of the neighbour lists the
// density pass left - directly behind the scalar pass, on contexts that carry scalars: S_p, the factor of
// dt * kappa in the pass's convexity condition.  It gathers posm[q] and Vs[q] and writes one partial per workgroup.
// Nothing between the density pass and this launch writes its inputs: posm[cur], ncount, nlist, nlist_overflow and
// tile_desc are written by the cell build and the density kernels only (cohesion, "The premise"), Vs by
// k_scalars_stage only, and k_scalars_step - the one launch between the stage and this one - takes them all const
// and writes T alone (scalar_kernels.h).
//
// k_monitor_finish, one workgroup, folds both partial arrays into the step's row, whose address is a kernel
// argument: queued steps stay queued.  Every local array is indexed by unrolled constants (none lives in scratch
// memory).
#pragma once

#include "cell_build.h"
#include "full_tiled.h"
#include "launch_policy.h"
#include "monitor_policy.h"
#include "neighbor_lists.h"
#include "pair_math.h"
#include "scalar_kernels.h"

static_assert(MONITOR_THREADS % SPH_WAVE == 0, "a monitor workgroup is whole waves");
#define MONITOR_WAVES (MONITOR_THREADS / SPH_WAVE)

// ---- reductions ------------------------------------------------------------------------------------------------
// what the lane `mask` away holds
__device__ __forceinline__ MonitorAcc monitor_shuffled(const MonitorAcc& a, int mask)
{
   MonitorAcc b;
#pragma unroll
   for (int i = 0; i < MON_SUMS; i++) {
      const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)((unsigned long long)a.sum[i] & 0xffffffffull), mask);
      const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)((unsigned long long)a.sum[i] >> 32), mask);
      b.sum[i] = (long long)(((unsigned long long)hi << 32) | (unsigned long long)lo);
   }
#pragma unroll
   for (int i = 0; i < MON_ADDS; i++) b.add[i] = __shfl_xor(a.add[i], mask);
#pragma unroll
   for (int i = 0; i < MON_MAXS; i++) b.mx[i] = (uint32_t)__shfl_xor((int)a.mx[i], mask);
#pragma unroll
   for (int i = 0; i < MON_MINS; i++) b.mn[i] = (uint32_t)__shfl_xor((int)a.mn[i], mask);
   return b;
}

// every lane's a folded over the workgroup: the result in thread 0 (called by all MONITOR_THREADS threads)
__device__ __forceinline__ void monitor_block_fold(MonitorAcc& a)
{
   __shared__ MonitorAcc s_wave[MONITOR_WAVES];
#pragma unroll
   for (int mask = SPH_WAVE / 2; mask > 0; mask >>= 1) monitor_merge(a, monitor_shuffled(a, mask));
   const int tid = threadIdx.x;
   if ((tid & (SPH_WAVE - 1)) == 0) s_wave[tid / SPH_WAVE] = a;
   __syncthreads();
   if (tid == 0) {
#pragma unroll
      for (int w = 1; w < MONITOR_WAVES; w++) monitor_merge(a, s_wave[w]);
   }
}

__device__ __forceinline__ void monitor_pair_block_fold(MonitorPairAcc& a)
{
   __shared__ MonitorPairAcc s_wave[MONITOR_WAVES];
#pragma unroll
   for (int mask = SPH_WAVE / 2; mask > 0; mask >>= 1) {
      MonitorPairAcc b;
      b.s_key = (uint32_t)__shfl_xor((int)a.s_key, mask);
      b.pair_bad = __shfl_xor(a.pair_bad, mask);
      monitor_pair_merge(a, b);
   }
   const int tid = threadIdx.x;
   if ((tid & (SPH_WAVE - 1)) == 0) s_wave[tid / SPH_WAVE] = a;
   __syncthreads();
   if (tid == 0) {
#pragma unroll
      for (int w = 1; w < MONITOR_WAVES; w++) monitor_pair_merge(a, s_wave[w]);
   }
}

// ---- the particles: a bounded grid that strides over the live slots -----------------------------------------------
// T == nullptr: the context carries no scalars.  part[gridDim.x]: one partial row per workgroup.
__global__ void __launch_bounds__(MONITOR_THREADS)
k_monitor_particles(const float4* __restrict__ posm, const float4* __restrict__ velp, const float4* __restrict__ acc,
                    const float* __restrict__ rho, const int32_t* __restrict__ ncount, const int32_t* __restrict__ meta,
                    const float4* __restrict__ T, int n_rows, int quantum_log2, MonitorAcc* __restrict__ part)
{
   MonitorAcc a;
   monitor_clear(a);
   const double scale = load_scale(quantum_log2);
   const long long end = meta[META_OWN_END];
   const long long stride = (long long)gridDim.x * MONITOR_THREADS;
   for (long long p = (long long)meta[META_OWN_BEGIN] + (long long)blockIdx.x * MONITOR_THREADS + threadIdx.x; p < end;
        p += stride) {
      const float4 x = posm[p], v = velp[p], f = acc[p];
      const uint32_t id = __float_as_uint(v.w);
      const bool good = monitor_particle(a, x.x, x.y, x.z, x.w, v.x, v.y, v.z, id, f.x, f.y, f.z, rho[p], ncount[p], scale);
      if (T && good && id < (uint32_t)n_rows) monitor_scalars(a, scalar4_of(T[id]));
   }
   monitor_block_fold(a);
   if (threadIdx.x == 0) part[blockIdx.x] = a;
}

// ---- the pairs: one workgroup per 256 sorted particles --------------------------------------------------------------
// one neighbour's operands into S_p (scalars_add's distance)
template <bool UNIT_SCALE>
__device__ __forceinline__ void monitor_add(const PairConsts& k, const float4& pi, const float4& pj, float vj, float& S)
{
   float dx, dy, dz;
   float d = sqrt_rn(dist2(pi.x, pi.y, pi.z, pj.x, pj.y, pj.z, dx, dy, dz));
   if (!UNIT_SCALE) d *= k.sim_scale;
   monitor_pair(S, vj, d, k.hscaled, k.kernel3);
}

// the list walk of one lane (scalars_from_lists' loop: one 16-byte load per eight entries)
template <bool UNIT_SCALE, bool WIDE>
__device__ __forceinline__ void monitor_from_lists(int cnt, const ListReader& lr, const TileDesc& d, const PairConsts& k,
                                                   const float4& pi, const float4* __restrict__ posm,
                                                   const float* __restrict__ Vs, float& S)
{
   const int lastb = cnt > 0 ? (cnt - 1) >> 3 : 0;
   uint4 blk = lr.block(0);
   for (int j0 = 0; j0 < cnt; j0 += 8) {
      uint32_t entry[8];
      list_block_entries(blk, entry);
      blk = lr.block(min((j0 >> 3) + 1, lastb));
      float4 pj[8];
      float vj[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
         const uint32_t e = j0 + u < cnt ? entry[u] : entry[0];      // (entry 0 of a block in use is a neighbour)
         const int q = ListEntry<WIDE>::tile(e) - ListEntry<WIDE>::shift(d, e);
         pj[u] = posm[q];
         vj[u] = Vs[q];
      }
#pragma unroll
      for (int u = 0; u < 8; u++)
         if (j0 + u < cnt) monitor_add<UNIT_SCALE>(k, pi, pj[u], vj[u], S);
   }
}

// the row walk of one lane (k_particle_density's: pressure_kernels.h)
template <bool UNIT_SCALE>
__device__ __forceinline__ void monitor_from_rows(int p, const CellGrid& g, const uint32_t* __restrict__ cell_start,
                                                  const PairConsts& k, const float4& pi, const float4* __restrict__ posm,
                                                  const float* __restrict__ Vs, float& S)
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
         if (d2 < k.h2) monitor_add<UNIT_SCALE>(k, pi, pj, Vs[q], S);
      }
   }
}

// tiled, force_rows: the scalar pass's own route switches (k_scalars_step).  Every workgroup of the grid stores its
// partial part[blockIdx.x] - one past the live range an empty one - so nothing returns before the fold.
template <bool UNIT_SCALE, bool WIDE>
__global__ void __launch_bounds__(TILE_THREADS)
k_monitor_pairs(const float4* __restrict__ posm, const float* __restrict__ Vs, const int32_t* __restrict__ ncount,
                const uint32_t* __restrict__ cell_start, const int32_t* __restrict__ meta, CellGrid g, PairConsts k,
                const TileDesc* __restrict__ desc, const uint32_t* __restrict__ nlist,
                const uint32_t* __restrict__ nlist_overflow, int list_cap, int tiled, int force_rows,
                MonitorPairAcc* __restrict__ part)
{
   static_assert(TILE_THREADS == MONITOR_THREADS, "the pair pass folds with the monitor's workgroup size");
   __shared__ TileDesc sd;
   const int begin = meta[META_SUM_BEGIN], end = meta[META_SUM_END];
   const int tid = threadIdx.x;
   const int wg = xcd_workgroup(blockIdx.x, gridDim.x);
   const int p0 = begin + wg * TILE_THREADS;
   const bool any = p0 < end;   // (the whole workgroup)
   const int p = p0 + tid;
   const bool live = p < end;
   // (workgroup-uniform: the barrier inside tile_desc_load is reached by every lane or by none)
   const uint32_t flag = (tiled && any) ? nlist_overflow[wg] : LISTS_NONE;
   const int wg_route = scalar_workgroup_route(tiled != 0, force_rows != 0, flag);
   if (any && wg_route == SCALAR_ROUTE_LISTS) tile_desc_load(desc, wg, sd);

   MonitorPairAcc a;
   monitor_pair_clear(a);
   if (live) {
      const float4 pi = posm[p];
      float S = 0.0f;
      int lane_route = SCALAR_ROUTE_ROWS;
      if (wg_route == SCALAR_ROUTE_LISTS) {
         const int cnt = ncount[p];
         const ListReader lr(nlist, wg, list_cap, tid);
         const uint32_t first_word = (flag == LISTS_SOME && cnt > 0) ? (lr.no_list() ? NLIST_NO_LIST : 0u) : 0u;
         lane_route = scalar_lane_route(wg_route, flag, cnt, first_word);
         if (lane_route == SCALAR_ROUTE_LISTS) monitor_from_lists<UNIT_SCALE, WIDE>(cnt, lr, sd, k, pi, posm, Vs, S);
      }
      if (lane_route == SCALAR_ROUTE_ROWS) monitor_from_rows<UNIT_SCALE>(p, g, cell_start, k, pi, posm, Vs, S);
      monitor_pair_offer(a, S);
   }
   monitor_pair_block_fold(a);
   if (tid == 0) part[blockIdx.x] = a;
}

// ---- the fold: one workgroup ------------------------------------------------------------------------------------
// n_pair == 0: the pair pass did not run (flags bit 1 stays clear).  Closes the step's recorded launches.
__global__ void __launch_bounds__(MONITOR_THREADS)
k_monitor_finish(const MonitorAcc* __restrict__ part, int n_part, const MonitorPairAcc* __restrict__ pair_part, int n_pair,
                 int have_scalars, sph_hip_monitor_row* __restrict__ row)
{
   MonitorAcc a;
   monitor_clear(a);
   for (int b = threadIdx.x; b < n_part; b += MONITOR_THREADS) monitor_merge(a, part[b]);
   MonitorPairAcc pa;
   monitor_pair_clear(pa);
   for (int b = threadIdx.x; b < n_pair; b += MONITOR_THREADS) monitor_pair_merge(pa, pair_part[b]);
   monitor_block_fold(a);
   monitor_pair_block_fold(pa);
   if (threadIdx.x == 0) *row = monitor_row_of(a, have_scalars != 0, n_pair > 0, pa);
}
