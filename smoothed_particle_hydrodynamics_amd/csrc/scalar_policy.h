// Carried scalars (include/sph_hip.h: sph_hip_set_scalars): four channels per particle - a temperature, a dye
// concentration, a salinity - that move with the fluid and diffuse between neighbours.  The arithmetic of one
// step, the sources and every argument check: one set of inline functions for the device (scalar_kernels.h)
// and for g++ (tests/test_scalars_cpu.py, against the numpy restatement tests/scalar_emulation.py).
// Pure C++17 without HIP; the translation units that use it are compiled with -ffp-contract=off.
//
// The contract.  All arithmetic is fp32, unfused, in the order written.
//   storage   T[id] = {T0, T1, T2, T3}, one row per particle ID (the upload row, velp.w), never per sorted
//             slot: the cell build re-sorts the state every step and the scalars do not move.
//   volume    V_j = rho_j > 0 ? m_j / rho_j : 0 (scalar_volume): one correctly rounded division, rho_j the
//             density pass's value in the step's state S_k
//   pairs     j runs over i's neighbours in S_k - (dx*dx + dy*dy) + dz*dz < h2 with (dx, dy, dz) = r_i - r_j,
//             i itself excluded: the acceleration pass's pairs - in canonical order (ascending FULL cell id,
//             then ascending sorted index: the order of k_particle_density and of the neighbour lists)
//   distance  d = sqrt(d2), correctly rounded, times sim_scale unless the context runs at unit scale
//             (scalar_distance): the distance accel_from_lists forms
//   weight    w_j = V_j * (kernel3 * (hscaled - d)) (scalar_weight): the reference's viscosity Laplacian
//             L(d) = kernel3 * (hscaled - d), formed first, times the volume
//   sum       s_c = 0.0f; for every j in order with V_j != 0: s_c = s_c + (T_j,c - T_i,c) * w_j (scalar_pair).  A
//             neighbour with V_j == 0 - every neighbour whose rho_j is not > 0 - is skipped by selection, whatever
//             its channels hold.
//   update    kappa[c] > 0: T_i,c' = T_i,c + (dt * kappa[c]) * s_c; else T_i,c' = T_i,c by selection - the bits
//             are kept, -0.0f and all (scalar_update)
//   sources   after the update, in list order: where r_i (of S_k) is STRICTLY inside the box,
//             lo_a < r_a < hi_a on every axis, HOLD sets T_i,channel = value and ADD sets
//             T_i,channel = T_i,channel + value * dt (scalar_apply_source)
// Every T_j, T_i and V_j is of S_k and of the scalars as they stood before the step (the device stages them by
// sorted slot first): the scheme is explicit.  Per channel the update is a convex combination of T_i and its
// neighbours' values while dt * kappa[c] * sum_j w_j <= 1; nothing polices that condition.  The coupling is one
// way: no particle changes by a bit.  FULL and FULL_FAST share the arithmetic (their densities agree).
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/sph_hip.h"

#ifdef __HIPCC__
#define SCALAR_HD __host__ __device__
#define SCALAR_INLINE __attribute__((always_inline))
#else
#define SCALAR_HD
#define SCALAR_INLINE
#endif

// finite: not NaN, not +-inf (a comparison, the same on the device and under g++)
SCALAR_HD inline bool scalar_finite(float v) { return fabsf(v) <= 3.402823466e38f; }

// the four channels of one particle (components written out: no array indexed by a channel number, which
// on the device would live in scratch memory)
struct Scalar4 {
   float c0, c1, c2, c3;
};

// what the arithmetic of a step needs besides the state: by value in the kernel's arguments
struct ScalarStep {
   float hscaled, kernel3, sim_scale, dt;
   float kappa[SPH_HIP_SCALAR_CHANNELS];
   int n_sources;
   sph_hip_scalar_source sources[SPH_HIP_MAX_SCALAR_SOURCES];
};

SCALAR_HD SCALAR_INLINE inline float scalar_volume(float m, float rho) { return rho > 0.0f ? m / rho : 0.0f; }

// (the device takes the same root with sqrt_rn: sph_device.h)
inline float scalar_distance(float d2, float sim_scale, bool unit_scale)
{
   float d = sqrtf(d2);
   if (!unit_scale) d *= sim_scale;
   return d;
}

SCALAR_HD SCALAR_INLINE inline float scalar_weight(float V, float d, float hscaled, float kernel3)
{
   const float L = kernel3 * (hscaled - d);
   return V * L;
}

// one neighbour into the running sums
SCALAR_HD SCALAR_INLINE inline void scalar_pair(Scalar4& s, const Scalar4& Ti, const Scalar4& Tj, float V, float d,
                                                float hscaled, float kernel3)
{
   const float w = scalar_weight(V, d, hscaled, kernel3);
   const bool on = V != 0.0f;
   s.c0 = on ? s.c0 + (Tj.c0 - Ti.c0) * w : s.c0;
   s.c1 = on ? s.c1 + (Tj.c1 - Ti.c1) * w : s.c1;
   s.c2 = on ? s.c2 + (Tj.c2 - Ti.c2) * w : s.c2;
   s.c3 = on ? s.c3 + (Tj.c3 - Ti.c3) * w : s.c3;
}

SCALAR_HD SCALAR_INLINE inline float scalar_update_channel(float T, float s, float dt, float kappa)
{
   return kappa > 0.0f ? T + (dt * kappa) * s : T;
}

SCALAR_HD SCALAR_INLINE inline Scalar4 scalar_update(const Scalar4& Ti, const Scalar4& s, float dt, const float (&kappa)[4])
{
   Scalar4 r;
   r.c0 = scalar_update_channel(Ti.c0, s.c0, dt, kappa[0]);
   r.c1 = scalar_update_channel(Ti.c1, s.c1, dt, kappa[1]);
   r.c2 = scalar_update_channel(Ti.c2, s.c2, dt, kappa[2]);
   r.c3 = scalar_update_channel(Ti.c3, s.c3, dt, kappa[3]);
   return r;
}

// strictly inside: a particle on a face is outside (NaN compares false: outside)
SCALAR_HD SCALAR_INLINE inline bool scalar_source_holds(const sph_hip_scalar_source& q, float x, float y, float z)
{
   return x > q.lo[0] && x < q.hi[0] && y > q.lo[1] && y < q.hi[1] && z > q.lo[2] && z < q.hi[2];
}

SCALAR_HD SCALAR_INLINE inline void scalar_apply_source(Scalar4& T, const sph_hip_scalar_source& q, float x, float y, float z,
                                                        float dt)
{
   if (!scalar_source_holds(q, x, y, z)) return;
   const float add = q.value * dt;
   const bool hold = q.kind == SPH_HIP_SCALAR_HOLD;
   const float v0 = hold ? q.value : T.c0 + add;
   const float v1 = hold ? q.value : T.c1 + add;
   const float v2 = hold ? q.value : T.c2 + add;
   const float v3 = hold ? q.value : T.c3 + add;
   T.c0 = q.channel == 0 ? v0 : T.c0;
   T.c1 = q.channel == 1 ? v1 : T.c1;
   T.c2 = q.channel == 2 ? v2 : T.c2;
   T.c3 = q.channel == 3 ? v3 : T.c3;
}

// the end of a particle's step: the update, then the sources in list order
SCALAR_HD SCALAR_INLINE inline Scalar4 scalar_finish(const Scalar4& Ti, const Scalar4& s, const ScalarStep& st, float x, float y,
                                                     float z)
{
   Scalar4 r = scalar_update(Ti, s, st.dt, st.kappa);
   for (int q = 0; q < st.n_sources; q++) scalar_apply_source(r, st.sources[q], x, y, z, st.dt);
   return r;
}

// the sampler's normalisation of a channel sum (SampleSum::store's rule for the velocity)
SCALAR_HD SCALAR_INLINE inline float scalar_shepard(float a, float rho) { return rho > 0.0f ? a / rho : 0.0f; }

// ---- checks ---------------------------------------------------------------------------------------------
// Why a context cannot carry scalars (REF and slab contexts are refused by the sampler's own check first), or
// nullptr.  ports_set: an emitter or a sink is set; ids_changed: ports have changed the particle set since the
// last upload (an emitter would need a scalar value per layer: not done).
inline const char* scalar_context_check(bool ports_set, bool ids_changed)
{
   if (ports_set) return "a context with ports cannot carry scalars";
   if (ids_changed) return "ports have changed the particle set: upload first";
   return nullptr;
}

// sph_hip_set_ports on a context that carries scalars
inline const char* scalar_ports_check(int n_scalars, int n_emitters, int n_sinks)
{
   if (n_scalars > 0 && (n_emitters > 0 || n_sinks > 0)) return "a context that carries scalars cannot have ports";
   return nullptr;
}

// Why a set of values is refused, or nullptr.  values4 == nullptr or n == 0 switches the scalars off and is
// never refused here.  live: the context's particle count.
inline const char* scalar_set_check(int n, const float* values4, const float* kappa4, int live)
{
   if (n < 0) return "negative count";
   if (!values4 || n == 0) return nullptr;
   if (n != live) return "n must equal the particle count";
   if (!kappa4) return "null diffusivity array";
   for (int c = 0; c < SPH_HIP_SCALAR_CHANNELS; c++)
      if (!(scalar_finite(kappa4[c]) && kappa4[c] >= 0.0f)) return "a diffusivity that is not finite and >= 0";
   for (long long i = 0; i < (long long)SPH_HIP_SCALAR_CHANNELS * n; i++)
      if (!scalar_finite(values4[i])) return "a value that is not finite";
   return nullptr;
}

inline const char* scalar_source_check(const sph_hip_scalar_source* list, int n)
{
   if (n < 0) return "negative count";
   if (n > SPH_HIP_MAX_SCALAR_SOURCES) return "more than SPH_HIP_MAX_SCALAR_SOURCES sources";
   if (n > 0 && !list) return "null source list";
   for (int i = 0; i < n; i++) {
      const sph_hip_scalar_source& q = list[i];
      if (q.channel < 0 || q.channel >= SPH_HIP_SCALAR_CHANNELS) return "channel must be 0 .. 3";
      if (q.kind != SPH_HIP_SCALAR_HOLD && q.kind != SPH_HIP_SCALAR_ADD) return "unknown source kind";
      for (int a = 0; a < 3; a++) {
         if (!(scalar_finite(q.lo[a]) && scalar_finite(q.hi[a]))) return "a box that is not finite";
         if (!(q.lo[a] < q.hi[a])) return "lo must be < hi on every axis";
      }
      if (!scalar_finite(q.value)) return "a value that is not finite";
   }
   return nullptr;
}

// a call that needs scalars on a context that carries none (never set, switched off, or dropped by an upload)
inline const char* scalar_have_check(int n_scalars) { return n_scalars > 0 ? nullptr : "the context carries no scalars"; }

inline const char* scalar_range_check(int first, int n, int have)
{
   if (first < 0 || n < 0 || (long long)first + n > have) return "the range leaves what the context holds";
   return nullptr;
}
