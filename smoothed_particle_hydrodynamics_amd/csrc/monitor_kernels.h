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
// k_monitor_pairs is one of the consumers of the neighbour lists the density pass left - the walk, on either route,
// is pair_walk.h's - directly behind the scalar pass, on contexts that carry scalars: S_p, the factor of
// dt * kappa in the pass's convexity condition.  It gathers posm[q] and Vs[q], 20 bytes per neighbour in two
// streams, and writes one partial per workgroup.
// Nothing between the density pass and this launch writes its inputs: posm[cur], ncount, nlist, nlist_overflow and
// tile_desc are written by the cell build and the density kernels only (cohesion, "The premise"), Vs by
// k_scalars_stage only, and k_scalars_step - the one launch between the stage and this one - takes them all const
// and writes T alone (scalar_kernels.h).
//
// k_monitor_finish, one workgroup, folds both partial arrays into the step's row, whose address is a kernel
// argument: queued steps stay queued.  Every local array is indexed by unrolled constants (none lives in scratch
// memory).
#pragma once

#include "monitor_policy.h"
#include "pair_walk.h"
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
// the pass's accumulator (pair_walk.h): S_p, by the scalar pass's distance
struct MonitorPairs {
   const PairConsts& k;
   const float* __restrict__ Vs;
   float S;

   using Payload = float;   // Vs: the volume of sorted particle q (k_scalars_stage)
   template <class Index>
   __device__ __forceinline__ Payload gather(Index q) const { return Vs[q]; }

   template <bool UNIT_SCALE>
   __device__ __forceinline__ void add(const float4& pi, const float4& pj, float vj)
   {
      float dx, dy, dz;
      float d = sqrt_rn(dist2(pi.x, pi.y, pi.z, pj.x, pj.y, pj.z, dx, dy, dz));
      if (!UNIT_SCALE) d *= k.sim_scale;
      monitor_pair(S, vj, d, k.hscaled, k.kernel3);
   }
};

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
   const PairLane w = pair_workgroup(meta, tiled, force_rows, nlist_overflow, desc, sd);

   MonitorPairAcc a;
   monitor_pair_clear(a);
   if (w.live) {
      const float4 pi = posm[w.p];
      MonitorPairs pairs = {k, Vs, 0.0f};
      pair_walk<UNIT_SCALE, WIDE>(w, sd, ncount, nlist, list_cap, g, cell_start, k.h2, pi, posm, pairs);
      monitor_pair_offer(a, pairs.S);
   }
   monitor_pair_block_fold(a);
   if (w.tid == 0) part[blockIdx.x] = a;
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
