// Tracers (include/sph_hip.h: sph_hip_set_tracers; the contract and every decision: tracer_policy.h):
// the advance of every tracer inside the step, and the counting sort that keeps the slots in cell order.
//
// Device state: the tracers sit in slots.  xi[slot] = {x, y, z, id bits}, cnt[slot] = {wet_steps, dry_steps}.
// The id is the tracer's row in the caller's array: read-backs and the record rows are by id, so the slot
// order never shows.  The advance reads positions, masses and velocities of the sorted state the step's cell
// build has just produced (posm, velp, cell_start) and writes tracer state only.
#pragma once

#include "cell_build.h"
#include "sample_kernels.h"
#include "tracer_policy.h"

// the sampler's walk with velocity as tracer_advance's `sample`
template <bool UNIT_SCALE>
struct TracerSampler {
   const float4* __restrict__ posm;
   const float4* __restrict__ velp;
   const uint32_t* __restrict__ cell_start;
   const CellGrid& g;
   const PairConsts& k;
   int have_particles;

   __device__ __forceinline__ int operator()(float px, float py, float pz, float& ux, float& uy, float& uz) const
   {
      SampleSum<true> s;
      if (have_particles) sample_walk<UNIT_SCALE>(px, py, pz, posm, velp, cell_start, g, k, s);
      // SampleSum::store's normalisation
      const bool pos = s.rho > 0.0f;
      ux = pos ? s.vx / s.rho : 0.0f;
      uy = pos ? s.vy / s.rho : 0.0f;
      uz = pos ? s.vz / s.rho : 0.0f;
      return s.count;
   }
};

// One lane per slot, no LDS.  record_row: this step's row of the recording (3 floats per tracer, by id),
// or null.
template <bool UNIT_SCALE>
__global__ void __launch_bounds__(256)
k_tracers_advance(float4* __restrict__ xi, int2* __restrict__ cnt, int n, const float4* __restrict__ posm,
                  const float4* __restrict__ velp, const uint32_t* __restrict__ cell_start, CellGrid g, PairConsts k,
                  TracerStep st, float* __restrict__ record_row)
{
   const int s = blockIdx.x * blockDim.x + threadIdx.x;
   if (s >= n) return;
   const float4 t = xi[s];
   const int2 c0 = cnt[s];
   int32_t wet = c0.x, dry = c0.y;
   float x0 = t.x, x1 = t.y, x2 = t.z;
   const TracerSampler<UNIT_SCALE> sample = {posm, velp, cell_start, g, k, st.have_particles};
   tracer_advance(x0, x1, x2, wet, dry, st, sample);
   xi[s] = make_float4(x0, x1, x2, t.w);
   cnt[s] = make_int2(wet, dry);
   if (record_row) {
      const uint32_t id = __float_as_uint(t.w);
      if (id < (uint32_t)n) {
         record_row[3 * (size_t)id + 0] = x0;
         record_row[3 * (size_t)id + 1] = x1;
         record_row[3 * (size_t)id + 2] = x2;
      }
   }
}

// ---- counting sort of the slots by FULL cell id ---------------------------------------------------------
// 1. cell of every slot (the cell build's clamped cell_coord: always a real cell of a whole grid) and its
//    arrival rank in that cell from the counting atomic; 2. k_scan_reduce (cell_build.h) and
//    k_tracer_scan: the counts become exclusive starts in place; 3. the slots move to start + rank in the
//    other pair of arrays.  The order inside a cell is the atomics' and may differ from run to run.
__global__ void __launch_bounds__(256)
k_tracer_hash(const float4* __restrict__ xi, int n, CellGrid g, uint32_t* __restrict__ cell_count,
              uint32_t* __restrict__ key, uint32_t* __restrict__ rank)
{
   const int s = blockIdx.x * blockDim.x + threadIdx.x;
   if (s >= n) return;
   const float4 t = xi[s];
   int cx, cy, cz;
   probe_cell(g, t.x, t.y, t.z, cx, cy, cz);
   const uint32_t c = (uint32_t)((cz * g.ny + cy) * g.nx + cx);
   key[s] = c;
   rank[s] = atomicAdd(&cell_count[c], 1u);
}

// part[tile] = the tile's total (k_scan_reduce); count[0..ncells) -> exclusive prefix sums, in place
__global__ void __launch_bounds__(SCAN_THREADS)
k_tracer_scan(uint32_t* __restrict__ count, int ncells, const uint32_t* __restrict__ part)
{
   const int base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
   uint32_t before = 0;
   for (int t = threadIdx.x; t < (int)blockIdx.x; t += SCAN_THREADS) before += part[t];
   uint32_t carry;
   block_exclusive_scan(before, &carry);
   if (part[blockIdx.x] == 0u) return;   // (uniform) a tile without tracers: nothing reads its starts
   uint32_t v[SCAN_ITEMS];
   uint32_t sum = 0;
#pragma unroll
   for (int j = 0; j < SCAN_ITEMS; j++) {
      v[j] = base + j < ncells ? count[base + j] : 0u;
      sum += v[j];
   }
   uint32_t total;
   uint32_t run = carry + block_exclusive_scan(sum, &total);
#pragma unroll
   for (int j = 0; j < SCAN_ITEMS; j++) {
      if (base + j < ncells && v[j] != 0u) count[base + j] = run;
      run += v[j];
   }
}

__global__ void __launch_bounds__(256)
k_tracer_scatter(const float4* __restrict__ xi, const int2* __restrict__ cnt, int n, const uint32_t* __restrict__ key,
                 const uint32_t* __restrict__ rank, const uint32_t* __restrict__ start, float4* __restrict__ xi_out,
                 int2* __restrict__ cnt_out)
{
   const int s = blockIdx.x * blockDim.x + threadIdx.x;
   if (s >= n) return;
   const uint32_t d = start[key[s]] + rank[s];
   if (d >= (uint32_t)n) return;   // (cannot happen: the counts add up to n)
   xi_out[d] = xi[s];
   cnt_out[d] = cnt[s];
}
