// Carried scalars (include/sph_hip.h: carried scalars; the contract and every check: scalar_policy.h; the
// routes: launch_policy.h): the stage that brings the scalars to the sorted slots, the pass that advances
// them, and the channel sums of the sampler's walk (with them the sampler's own kernels are the point and
// lattice samplers of the channels: sample_kernels.h).
//
// The scalars live by particle ID (T[id], the id in velp.w) and never ride through the cell build.  A step
// stages Ts[p] = T[id(p)] and Vs[p] = m / rho for the sorted slots of its state S_k (k_scalars_stage), then
// k_scalars_step - one of the consumers of the neighbour lists the density pass left for the acceleration pass -
// sums over every particle's neighbours and writes T[id(p)] in place: it reads Ts and Vs only, so nothing
// races.  The walk, on either route, is pair_walk.h's; it gathers posm[q], Ts[q] and Vs[q], 36 bytes per
// neighbour in three streams.  No kernel here writes anything of the particle state.
#pragma once

#include "pair_walk.h"
#include "sample_kernels.h"
#include "scalar_policy.h"

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
// the pass's accumulator (pair_walk.h)
struct ScalarPairs {
   const ScalarStep& st;
   const float4* __restrict__ Ts;
   const float* __restrict__ Vs;
   Scalar4 Ti;
   Scalar4 s;

   struct Payload {
      float4 t;   // Ts: the channels of sorted particle q (k_scalars_stage)
      float v;    // Vs: its volume
   };
   template <class Index>
   __device__ __forceinline__ Payload gather(Index q) const { return Payload{Ts[q], Vs[q]}; }

   template <bool UNIT_SCALE>
   __device__ __forceinline__ void add(const float4& pi, const float4& pj, const Payload& j)
   {
      float dx, dy, dz;
      float d = sqrt_rn(dist2(pi.x, pi.y, pi.z, pj.x, pj.y, pj.z, dx, dy, dz));
      if (!UNIT_SCALE) d *= st.sim_scale;
      scalar_pair(s, Ti, scalar4_of(j.t), j.v, d, st.hscaled, st.kernel3);
   }
};

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
   const PairLane w = pair_workgroup(meta, tiled, force_rows, nlist_overflow, desc, sd);
   if (!w.live) return;
   const int p = w.p;

   const float4 pi = posm[p];
   ScalarPairs pairs = {st, Ts, Vs, scalar4_of(Ts[p]), {0.0f, 0.0f, 0.0f, 0.0f}};
   pair_walk<UNIT_SCALE, WIDE>(w, sd, ncount, nlist, list_cap, g, cell_start, h2, pi, posm, pairs);

   const Scalar4 out = scalar_finish(pairs.Ti, pairs.s, st, pi.x, pi.y, pi.z);
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
