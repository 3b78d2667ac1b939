// Pressure readings (include/sph_hip.h: pressure readings; the contract and every decision: gauge_policy.h):
// the particle densities of the current sorted state, the pressure sums of the sampler's walk (with them the
// sampler's own kernels are the point and lattice samplers of the pressure: sample_kernels.h) and the wave
// that reads the pressure gauges.
//
// k_particle_density is density_untiled's walk (full_kernels.h) writing the density alone, into a buffer of
// the context's own: none of rho, velB, auxc, ncount, the lists or the tile statistics is touched.  A
// pressure probe is sample_walk (sample_kernels.h) with PressureSum: one more load per MEMBER, the member's
// density; it forms P_j from it and adds t_j * P_j.  No kernel here uses LDS, and no local array goes to a
// function by pointer (RowRanges is selected from: row_range, full_kernels.h).
#pragma once

#include "cell_build.h"
#include "sample_kernels.h"
#include "gauge_policy.h"

// ---- the densities of the current state: one lane per sorted particle -------------------------------------
template <bool UNIT_SCALE>
__global__ void __launch_bounds__(256)
k_particle_density(const float4* __restrict__ posm, const uint32_t* __restrict__ cell_start,
                   const int32_t* __restrict__ meta, CellGrid g, PairConsts k, float* __restrict__ rho_out)
{
   const int p = meta[META_SUM_BEGIN] + blockIdx.x * blockDim.x + threadIdx.x;
   if (p >= meta[META_SUM_END]) return;
   const float4 pi = posm[p];
   int cx, cy, cz;
   cell_of(g, pi.x, pi.y, pi.z, cx, cy, cz);
   RowRanges r;
   row_ranges(g, cell_start, cx, cy, cz, r);
   float density = 0.0f;
#pragma unroll 1
   for (int row = 0; row < 9; row++) {
      uint32_t s, e;
      row_range(r, row, s, e);
      for (uint32_t q = s; q < e; q++) {
         if (q == (uint32_t)p) continue;
         const float4 pj = posm[q];
         float dx, dy, dz;
         const float d2 = dist2(pi.x, pi.y, pi.z, pj.x, pj.y, pj.z, dx, dy, dz);
         if (d2 < k.h2) {
            float d = sqrtf(d2);
            if (!UNIT_SCALE) d *= k.sim_scale;
            density_accumulate<UNIT_SCALE>(k, pj.w, d, density);
         }
      }
   }
   rho_out[p] = density;
}

// ---- the pressure sums of the sampler's walk ---------------------------------------------------------------
// accumulator of one probe: the sampler's rho and count, and pw = sum of t_j * P_j
struct PressureSum {
   float rho = 0.0f, pw = 0.0f;
   int count = 0;

   using Payload = float;   // prho: the density of sorted particle q
   struct Out {
      float* prs;
      float* rho;
      int32_t* cnt;
   };

   template <bool UNIT_SCALE>
   __device__ __forceinline__ void member(const PairConsts& k, float d2, float m, const float* __restrict__ prho,
                                          uint32_t q)
   {
      add<UNIT_SCALE>(k, d2, m, prho[q]);
   }

   template <bool UNIT_SCALE>
   __device__ __forceinline__ void add(const PairConsts& k, float d2, float m, float rho_j)
   {
      float d = sqrt_rn(d2);   // (as SampleSum::add: sample_kernels.h)
      if (!UNIT_SCALE) d *= k.sim_scale;
      const float t = density_term<UNIT_SCALE>(k, m, d);
      rho += t;
      pw += t * gauge_particle_pressure(rho_j, k.rho0, k.stiffness);
      count++;
   }

   __device__ __forceinline__ void store(int o, const Out& out) const
   {
      out.prs[o] = gauge_pressure_quotient(pw, rho);
      out.rho[o] = rho;
      out.cnt[o] = count;
   }
};

// ---- the pressure gauges: one wave per gauge, as k_gauges_read ---------------------------------------------
// prho: the densities of the state in sorted order - the density pass's own inside a step, the context's
// buffer (k_particle_density) elsewhere.  A gauge of a field kind is k_gauges_read's: nothing walked or stored.
template <bool UNIT_SCALE>
__global__ void __launch_bounds__(256)
k_gauges_pressure(const sph_hip_gauge* __restrict__ gauges, int n_gauges, const float4* __restrict__ posm,
                  const float* __restrict__ prho, const uint32_t* __restrict__ cell_start, CellGrid g, PairConsts k,
                  int have_particles, sph_hip_gauge_reading* __restrict__ out)
{
   static_assert(SPH_WAVE == GAUGE_WAVE, "gauge_policy.h counts in waves of 64");
   const int lane = threadIdx.x % SPH_WAVE;
   const int gi = blockIdx.x * GAUGES_PER_BLOCK + threadIdx.x / SPH_WAVE;
   if (gi >= n_gauges) return;   // (the whole wave)
   const sph_hip_gauge G = gauges[gi];
   if (gauge_read_by(G.kind) != GAUGE_LAUNCH_PRESSURE) return;   // (the whole wave)
   const int probes = gauge_pressure_probes(G);
   const int trips = gauge_trips(probes);

   int n = 0;
   float a = 0.0f, r = 0.0f;
   float l_rho = 0.0f, l_pw = 0.0f;   // the sums of the lane's last walk: a point's only one
   int l_count = 0;
#pragma unroll 1
   for (int trip = 0; trip < trips; trip++) {
      const int q = trip * SPH_WAVE + lane;
      const bool has = q < probes;
      float px, py, pz;
      gauge_probe(G, q, px, py, pz);
      PressureSum s;
      if (has && have_particles) sample_walk<UNIT_SCALE>(px, py, pz, posm, prho, cell_start, g, k, s);
      l_rho = s.rho;
      l_pw = s.pw;
      l_count = s.count;
      const bool wet = has && gauge_wet(s.rho, G.iso);
      n = gauge_count_wet(n, __ballot(wet));
      gauge_patch_add(wet, s.rho, s.pw, a, r);
   }

   sph_hip_gauge_reading rd;
   if (G.kind == SPH_HIP_GAUGE_PRESSURE_PATCH) {
#pragma unroll
      for (int d = 1; d < SPH_WAVE; d <<= 1) {
         a = a + __shfl_xor(a, d, SPH_WAVE);
         r = r + __shfl_xor(r, d, SPH_WAVE);
      }
      rd = gauge_patch_reading(G, n, a, r);
   } else {
      rd = gauge_pressure_reading(l_rho, l_pw, l_count);
   }
   if (lane == 0) out[gi] = rd;
}
