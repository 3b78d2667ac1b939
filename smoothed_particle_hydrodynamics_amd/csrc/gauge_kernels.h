// Gauges (include/sph_hip.h: sph_hip_set_gauges; the contract and every decision: gauge_policy.h): the
// evaluation of every gauge in the sorted state a cell build has just produced.
//
// One wave per gauge, four gauges per workgroup, no LDS.  Lane l walks the probes l, l + 64, ... of its gauge,
// one trip of the wave each; a column makes one more trip in which lanes 0 and 1 walk its topmost wet probe and
// the one above it again (a walk's result has one possible set of bits), so the whole kernel has one call
// site of sample_walk.  Every branch on the gauge's kind and every trip count is the same in all 64 lanes.
// Reads positions, masses and velocities of the state (posm, velp, cell_start); writes one reading per gauge
// of a field kind.  A gauge of a pressure kind is k_gauges_pressure's (pressure_kernels.h): its wave returns at
// once, nothing walked and nothing stored.
#pragma once

#include "cell_build.h"
#include "sample_kernels.h"
#include "gauge_policy.h"

#define GAUGES_PER_BLOCK (256 / SPH_WAVE)

template <bool UNIT_SCALE>
__global__ void __launch_bounds__(256)
k_gauges_read(const sph_hip_gauge* __restrict__ gauges, int n_gauges, const float4* __restrict__ posm,
              const float4* __restrict__ velp, const uint32_t* __restrict__ cell_start, CellGrid g, PairConsts k,
              int have_particles, sph_hip_gauge_reading* __restrict__ out)
{
   static_assert(SPH_WAVE == GAUGE_WAVE, "gauge_policy.h counts in waves of 64");
   const int lane = threadIdx.x % SPH_WAVE;
   const int gi = blockIdx.x * GAUGES_PER_BLOCK + threadIdx.x / SPH_WAVE;
   if (gi >= n_gauges) return;   // (the whole wave)
   const sph_hip_gauge G = gauges[gi];
   if (gauge_read_by(G.kind) != GAUGE_LAUNCH_FIELD) return;   // (the whole wave) k_gauges_pressure's: nothing walked or stored
   const int probes = gauge_field_probes(G);
   const int trips = gauge_trips(probes);
   const bool column = G.kind == SPH_HIP_GAUGE_COLUMN;
   const int all_trips = trips + (column ? 1 : 0);

   int n = 0, top = -1;
   float a = 0.0f, r = 0.0f;
   // the sums of the lane's last walk: a point's only one; a column's second look at its top
   float l_rho = 0.0f, l_vx = 0.0f, l_vy = 0.0f, l_vz = 0.0f;
   int l_count = 0;
#pragma unroll 1
   for (int trip = 0; trip < all_trips; trip++) {
      const bool again = trip == trips;
      const int q = again ? gauge_column_again(top) + lane : trip * SPH_WAVE + lane;
      const bool has = q < probes && (!again || lane < 2);
      float px, py, pz;
      gauge_probe(G, q, px, py, pz);
      SampleSum<true> s;
      if (has && have_particles) sample_walk<UNIT_SCALE>(px, py, pz, posm, velp, cell_start, g, k, s);
      l_rho = s.rho;
      l_vx = s.vx;
      l_vy = s.vy;
      l_vz = s.vz;
      l_count = s.count;
      if (!again) {
         const unsigned long long wet = __ballot(has && gauge_wet(s.rho, G.iso));
         n = gauge_count_wet(n, wet);
         top = gauge_top_wet(top, wet, trip);
         const float va = gauge_pick(s.vx, s.vy, s.vz, G.axis);
         a = has ? a + va : a;
         r = has ? r + s.rho : r;
      }
   }

   sph_hip_gauge_reading rd;
   if (column) {
      const float f0 = __shfl(l_rho, 0, SPH_WAVE), f1 = __shfl(l_rho, 1, SPH_WAVE);
      rd = gauge_column_reading(G, n, top, f0, f1);
   } else if (G.kind == SPH_HIP_GAUGE_SECTION) {
#pragma unroll
      for (int d = 1; d < SPH_WAVE; d <<= 1) {
         a = a + __shfl_xor(a, d, SPH_WAVE);
         r = r + __shfl_xor(r, d, SPH_WAVE);
      }
      rd = gauge_section_reading(G, n, a, r);
   } else {
      rd = gauge_point_reading(l_rho, l_vx, l_vy, l_vz, l_count);
   }
   if (lane == 0) out[gi] = rd;
}
