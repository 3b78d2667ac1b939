// Pressure readings (include/sph_hip.h: pressure readings; the contract and every decision: gauge_policy.h):
// the particle densities of the current sorted state, the pressure form of the sampler's walk, the point and
// lattice samplers of the pressure and the wave that reads the pressure gauges.
//
// k_particle_density is density_untiled's walk (full_kernels.h) writing the density alone, into a buffer of
// the context's own: none of rho, velB, auxc, ncount, the lists or the tile statistics is touched.  The
// pressure walk is sample_walk's (sample_kernels.h) with one more load per MEMBER, the member's density; it
// forms P_j from it and adds t_j * P_j.  No kernel here uses LDS, and no local array goes to a function by
// pointer (RowRanges is selected from, as in sample_walk).
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
      const uint32_t s = row == 0 ? r.s[0] : row == 1 ? r.s[1] : row == 2 ? r.s[2] : row == 3 ? r.s[3]
                       : row == 4 ? r.s[4] : row == 5 ? r.s[5] : row == 6 ? r.s[6] : row == 7 ? r.s[7] : r.s[8];
      const uint32_t e = row == 0 ? r.e[0] : row == 1 ? r.e[1] : row == 2 ? r.e[2] : row == 3 ? r.e[3]
                       : row == 4 ? r.e[4] : row == 5 ? r.e[5] : row == 6 ? r.e[6] : row == 7 ? r.e[7] : r.e[8];
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

// ---- the pressure form of the sampler's walk ---------------------------------------------------------------
// accumulator of one probe: the sampler's rho and count, and pw = sum of t_j * P_j
struct PressureSum {
   float rho = 0.0f, pw = 0.0f;
   int count = 0;

   template <bool UNIT_SCALE>
   __device__ __forceinline__ void add(const PairConsts& k, float d2, float m, float rho_j)
   {
      float d = sqrt_rn(d2);   // (SampleSum::add)
      if (!UNIT_SCALE) d *= k.sim_scale;
      const float t = density_term<UNIT_SCALE>(k, m, d);
      rho += t;
      pw += t * gauge_particle_pressure(rho_j, k.rho0, k.stiffness);
      count++;
   }

   __device__ __forceinline__ void store(int o, float* __restrict__ prs_out, float* __restrict__ rho_out,
                                         int32_t* __restrict__ cnt_out) const
   {
      prs_out[o] = gauge_pressure_quotient(pw, rho);
      rho_out[o] = rho;
      cnt_out[o] = count;
   }
};

// one probe, candidates read from global memory; prho[q]: the density of sorted particle q, read for members
template <bool UNIT_SCALE>
__device__ __forceinline__ void sample_walk_pressure(float px, float py, float pz, const float4* __restrict__ posm,
                                                     const float* __restrict__ prho,
                                                     const uint32_t* __restrict__ cell_start, const CellGrid& g,
                                                     const PairConsts& k, PressureSum& s)
{
   int cx, cy, cz;
   probe_cell(g, px, py, pz, cx, cy, cz);
   RowRanges r;
   row_ranges(g, cell_start, cx, cy, cz, r);
#pragma unroll 1
   for (int row = 0; row < 9; row++) {
      const uint32_t b = row == 0 ? r.s[0] : row == 1 ? r.s[1] : row == 2 ? r.s[2] : row == 3 ? r.s[3]
                       : row == 4 ? r.s[4] : row == 5 ? r.s[5] : row == 6 ? r.s[6] : row == 7 ? r.s[7] : r.s[8];
      const uint32_t e = row == 0 ? r.e[0] : row == 1 ? r.e[1] : row == 2 ? r.e[2] : row == 3 ? r.e[3]
                       : row == 4 ? r.e[4] : row == 5 ? r.e[5] : row == 6 ? r.e[6] : row == 7 ? r.e[7] : r.e[8];
      for (uint32_t q = b; q < e; q++) {
         const float4 pj = posm[q];
         float dx, dy, dz;
         const float d2 = dist2(px, py, pz, pj.x, pj.y, pj.z, dx, dy, dz);
         if (d2 < k.h2) s.template add<UNIT_SCALE>(k, d2, pj.w, prho[q]);
      }
   }
}

// ---- point probes: one lane per probe ----------------------------------------------------------------------
template <bool UNIT_SCALE>
__global__ void __launch_bounds__(256)
k_sample_pressure_points(const float* __restrict__ xyz, int n, const float4* __restrict__ posm,
                         const float* __restrict__ prho, const uint32_t* __restrict__ cell_start, CellGrid g,
                         PairConsts k, float* __restrict__ prs_out, float* __restrict__ rho_out,
                         int32_t* __restrict__ cnt_out)
{
   const int p = blockIdx.x * blockDim.x + threadIdx.x;
   if (p >= n) return;
   PressureSum s;
   sample_walk_pressure<UNIT_SCALE>(xyz[3 * p + 0], xyz[3 * p + 1], xyz[3 * p + 2], posm, prho, cell_start, g, k, s);
   s.store(p, prs_out, rho_out, cnt_out);
}

// ---- lattice probes: one workgroup per brick, every lane walks per probe (k_sample_lattice<.., false>) -----
template <bool UNIT_SCALE>
__global__ void __launch_bounds__(SAMPLE_THREADS)
k_sample_pressure_lattice(SampleLattice L, const float4* __restrict__ posm, const float* __restrict__ prho,
                          const uint32_t* __restrict__ cell_start, CellGrid g, PairConsts k,
                          float* __restrict__ prs_out, float* __restrict__ rho_out, int32_t* __restrict__ cnt_out)
{
   const int t = threadIdx.x;
   const int b = blockIdx.x;
   const int bx = b % L.bricks_x, by = (b / L.bricks_x) % L.bricks_y, bz = b / (L.bricks_x * L.bricks_y);
   const int il = bx * L.bx + t % L.bx;
   const int jl = by * L.by + (t / L.bx) % L.by;
   const int kl = bz * L.bz + t / (L.bx * L.by);
   if (!(il < L.ex && jl < L.ey && kl < L.ez)) return;
   const float px = L.ox + (float)(L.i0 + il) * L.sx;
   const float py = L.oy + (float)(L.j0 + jl) * L.sy;
   const float pz = L.oz + (float)(L.k0 + kl) * L.sz;
   const int o = (kl * L.ey + jl) * L.ex + il;
   PressureSum s;
   sample_walk_pressure<UNIT_SCALE>(px, py, pz, posm, prho, cell_start, g, k, s);
   s.store(o, prs_out, rho_out, cnt_out);
}

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
      if (has && have_particles) sample_walk_pressure<UNIT_SCALE>(px, py, pz, posm, prho, cell_start, g, k, s);
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
