// Viscous stress (include/sph_hip.h: sph_hip_set_viscous_stress): a pairwise, momentum-conserving viscous force of a
// stated dynamic viscosity mu, a_i = (1 / rho_i) * sum_j mu_ij (m_j / rho_j) (v_j - v_i) L(d_ij) - the reference's
// viscous term with the density's inverse, no rescale inside the loop, and a symmetric pair viscosity - constant, or a
// function of a carried channel through a table of keys (a law): lava that stiffens as it cools, oil that thins as it
// warms.  The arithmetic of one particle and every check: one set of inline functions for the device
// (viscous_kernels.h) and for g++ (tests/test_viscous_cpu.py, against the numpy restatement
// tests/viscous_emulation.py).  Pure C++17 without HIP; the translation units that use it are compiled with
// -ffp-contract=off.
//
// The contract.  All arithmetic is fp32, unfused, in the order written.  For particle i of the step's state S_k:
//   setting   mu finite and >= 0; 0 and -0 are "off" by bits.  An optional law: a channel c in 0..3 and K keys,
//             2 <= K <= SPH_HIP_MAX_VISCOSITY_KEYS, key values x_0 < ... < x_{K-1} finite and strictly ascending,
//             key factors f_k finite and >= 0.  Each condition has its own check function and its own text.
//   law       factor(x): !(x > x_0) gives f_0 (NaN and -inf too); x >= x_{K-1} gives f_{K-1}; else, with
//             x_k <= x < x_{k+1}, u = (x - x_k) / (x_{k+1} - x_k) and f = f_k + u * (f_{k+1} - f_k)
//             (viscous_factor).  The key loop is written out over the 16 slots with selections: no array is indexed
//             by a run-time number.
//   stage     every live sorted slot p: R[p] = {v.x, v.y, v.z, V_p}, v = velp[cur][p], V_p = scalar_volume(m_p,
//             rho[p]) - m / rho, 0 where rho is not > 0 (viscous_stage).  With a law also M[p] = mu *
//             factor(Ts[p].c), Ts the channel row the step's scalar pass staged: the channels as they stood before
//             this step, what buoyancy reads (viscous_stage_mu).
//   members   cohesion's exactly: j with d2 = (dx*dx + dy*dy) + dz*dz < h2, (dx, dy, dz) = r_i - r_j, i itself
//             excluded, in canonical order (ascending FULL cell id, then ascending sorted index); d = sqrt(d2),
//             correctly rounded, times sim_scale unless the context runs at unit scale
//   pair      L = kernel3 * (hscaled - d): the reference's own viscosity Laplacian, no extra rule for d > hscaled
//             (as scalar_weight); m_ij = 0.5f * (M_i + M_j) with a law, else mu; g = (m_ij * (V_i * V_j)) * L.
//             A member with V_j == 0 is skipped by selection, whatever its row holds.  s = s + g * (R_j.xyz -
//             R_i.xyz) per component from 0.0f (viscous_pair).  Every factor of g is symmetric in i and j by bits
//             and the velocity difference is an exact negation: the force addend of (i, j) is the bitwise negation
//             of (j, i)'s for any masses, and momentum is conserved pair by pair.
//   accel     c = s / m_i per component: three correctly rounded divisions per particle, none per pair
//             (viscous_accel)
//   guard     V_i == 0, m_i not > 0, c zero in all three components, or c not finite in any: the particle is left
//             alone and nothing is stored (viscous_acts: cohesion_acts' rule behind the two operand tests).  A
//             uniform velocity field stores nothing.
//   apply     a' = clamp(a + c) stored to acc[p], clamp as cohesion_apply uses it (buoyancy_clamp).  The velocity
//             is not touched.
// In a step: acceleration pass, cohesion, viscous stress, XSPH, buoyancy, integrate.  The stage reads velp[cur] before
// XSPH writes it, so every sum reads S_k's velocities.  FULL and FULL_FAST share the arithmetic: the pass reads
// nothing the two modes form differently, except the acc it adds to.
//
// Range.  The scheme is explicit: a particle's velocity stays a convex combination of itself and its neighbours'
// while N_i = dt * (1 / m_i) * sum_j m_ij V_i V_j L <= 1.  NOTHING polices this on the device or in the setter: a
// caller that asks for a mu beyond it gets a step that amplifies velocity differences.  The restatement returns N_i.
#pragma once

#include "cohesion_policy.h"

// the staged row of one sorted slot: the velocity and the volume
struct ViscousRow {
   float x, y, z, w;
};

// the running sum of one particle (components written out: no array, which on the device could live in
// scratch memory)
struct ViscousSum {
   float x, y, z;
};

// ---- the law ----------------------------------------------------------------------------------------------
// one segment of the table: taken where the segment exists (k + 1 < K) and x_k <= x < x_{k+1}; `above` is x > x_0
SCALAR_HD SCALAR_INLINE inline float viscous_segment(float x, bool above, int K, int k, float xk, float xk1, float fk,
                                                     float fk1, float f)
{
   const bool in = above && k + 1 < K && x >= xk && x < xk1;
   const float u = (x - xk) / (xk1 - xk);
   const float t = fk + u * (fk1 - fk);
   return in ? t : f;
}

// the last key: x >= x_{K-1}
SCALAR_HD SCALAR_INLINE inline float viscous_last(float x, bool above, int K, int k, float xk, float fk, float f)
{
   return (above && k == K - 1 && x >= xk) ? fk : f;
}

#define VISCOUS_SEGMENT(k) \
   f = viscous_segment(x, above, K, k, law.value[k], law.value[k + 1], law.factor[k], law.factor[k + 1], f)
#define VISCOUS_LAST(k) f = viscous_last(x, above, K, k, law.value[k], law.factor[k], f)

SCALAR_HD SCALAR_INLINE inline float viscous_factor(const sph_hip_viscosity_law& law, float x)
{
   static_assert(SPH_HIP_MAX_VISCOSITY_KEYS == 16, "the key loop is written out over 16 slots");
   const int K = law.n_keys;
   const bool above = x > law.value[0];
   float f = law.factor[0];
   VISCOUS_SEGMENT(0); VISCOUS_SEGMENT(1); VISCOUS_SEGMENT(2); VISCOUS_SEGMENT(3);
   VISCOUS_SEGMENT(4); VISCOUS_SEGMENT(5); VISCOUS_SEGMENT(6); VISCOUS_SEGMENT(7);
   VISCOUS_SEGMENT(8); VISCOUS_SEGMENT(9); VISCOUS_SEGMENT(10); VISCOUS_SEGMENT(11);
   VISCOUS_SEGMENT(12); VISCOUS_SEGMENT(13); VISCOUS_SEGMENT(14);
   VISCOUS_LAST(1); VISCOUS_LAST(2); VISCOUS_LAST(3); VISCOUS_LAST(4); VISCOUS_LAST(5);
   VISCOUS_LAST(6); VISCOUS_LAST(7); VISCOUS_LAST(8); VISCOUS_LAST(9); VISCOUS_LAST(10);
   VISCOUS_LAST(11); VISCOUS_LAST(12); VISCOUS_LAST(13); VISCOUS_LAST(14); VISCOUS_LAST(15);
   return f;
}

#undef VISCOUS_SEGMENT
#undef VISCOUS_LAST

// the law's channel of a staged row, by selection
SCALAR_HD SCALAR_INLINE inline float viscous_channel(int c, float t0, float t1, float t2, float t3)
{
   return c == 0 ? t0 : c == 1 ? t1 : c == 2 ? t2 : t3;
}

// ---- the arithmetic of a step ---------------------------------------------------------------------------------
SCALAR_HD SCALAR_INLINE inline ViscousRow viscous_stage(float vx, float vy, float vz, float m, float rho)
{
   return ViscousRow{vx, vy, vz, scalar_volume(m, rho)};
}

// M[p] of a context with a law: x = the law's channel of the slot's staged row
SCALAR_HD SCALAR_INLINE inline float viscous_stage_mu(float mu, const sph_hip_viscosity_law& law, float x)
{
   return mu * viscous_factor(law, x);
}

// the pair viscosity: the mean of the two staged ones with a law, else the setting
SCALAR_HD SCALAR_INLINE inline float viscous_pair_mu(bool law, float mu, float Mi, float Mj)
{
   return law ? 0.5f * (Mi + Mj) : mu;
}

// one member into the sum: m_ij = the pair viscosity, d = the scaled distance
SCALAR_HD SCALAR_INLINE inline void viscous_pair(ViscousSum& s, float m_ij, float d, float hscaled, float kernel3,
                                                 const ViscousRow& Ri, const ViscousRow& Rj)
{
   const float L = kernel3 * (hscaled - d);
   const float g = (m_ij * (Ri.w * Rj.w)) * L;
   const bool on = Rj.w != 0.0f;
   const float tx = g * (Rj.x - Ri.x), ty = g * (Rj.y - Ri.y), tz = g * (Rj.z - Ri.z);
   s.x = on ? s.x + tx : s.x;
   s.y = on ? s.y + ty : s.y;
   s.z = on ? s.z + tz : s.z;
}

SCALAR_HD SCALAR_INLINE inline ViscousSum viscous_accel(const ViscousSum& s, float m)
{
   return ViscousSum{s.x / m, s.y / m, s.z / m};
}

// whether the particle is touched at all: its own volume and mass, then cohesion_acts' rule
SCALAR_HD SCALAR_INLINE inline bool viscous_acts(float Vi, float m, const ViscousSum& c)
{
   return Vi != 0.0f && m > 0.0f && cohesion_acts(CohesionSum{c.x, c.y, c.z});
}

// One particle with the viscous acceleration c: a (acc[p].xyz) in place.  The caller has asked viscous_acts.
SCALAR_HD SCALAR_INLINE inline void viscous_apply(const ViscousSum& c, float cfl_limit, float cfl_limit2, float& ax, float& ay,
                                                  float& az)
{
   cohesion_apply(CohesionSum{c.x, c.y, c.z}, cfl_limit, cfl_limit2, ax, ay, az);
}

// ---- checks ---------------------------------------------------------------------------------------------
// whether a mu switches the term off (-0.0f too)
inline bool viscous_is_off(float mu) { return mu == 0.0f; }

// Why sph_hip_set_viscous_stress refuses a mu, or nullptr
inline const char* viscous_mu_finite_check(float mu) { return scalar_finite(mu) ? nullptr : "a viscosity that is not finite"; }
inline const char* viscous_mu_sign_check(float mu) { return mu >= 0.0f ? nullptr : "a negative viscosity"; }

// Why it refuses a law, or nullptr: one function per condition
inline const char* viscous_law_channel_check(const sph_hip_viscosity_law& law)
{
   return (law.channel >= 0 && law.channel < SPH_HIP_SCALAR_CHANNELS) ? nullptr : "a law channel outside 0..3";
}

inline const char* viscous_law_keys_check(const sph_hip_viscosity_law& law)
{
   return (law.n_keys >= 2 && law.n_keys <= SPH_HIP_MAX_VISCOSITY_KEYS) ? nullptr : "a law with fewer than 2 or more than 16 keys";
}

// (behind viscous_law_keys_check: n_keys is in range)
inline const char* viscous_law_values_finite_check(const sph_hip_viscosity_law& law)
{
   for (int k = 0; k < law.n_keys; k++)
      if (!scalar_finite(law.value[k])) return "a key value that is not finite";
   return nullptr;
}

inline const char* viscous_law_ascending_check(const sph_hip_viscosity_law& law)
{
   for (int k = 0; k + 1 < law.n_keys; k++)
      if (!(law.value[k] < law.value[k + 1])) return "key values that are not strictly ascending";
   return nullptr;
}

inline const char* viscous_law_factors_finite_check(const sph_hip_viscosity_law& law)
{
   for (int k = 0; k < law.n_keys; k++)
      if (!scalar_finite(law.factor[k])) return "a key factor that is not finite";
   return nullptr;
}

inline const char* viscous_law_factors_sign_check(const sph_hip_viscosity_law& law)
{
   for (int k = 0; k < law.n_keys; k++)
      if (!(law.factor[k] >= 0.0f)) return "a negative key factor";
   return nullptr;
}

// all of them in the order above
inline const char* viscous_law_check(const sph_hip_viscosity_law& law)
{
   if (const char* why = viscous_law_channel_check(law)) return why;
   if (const char* why = viscous_law_keys_check(law)) return why;
   if (const char* why = viscous_law_values_finite_check(law)) return why;
   if (const char* why = viscous_law_ascending_check(law)) return why;
   if (const char* why = viscous_law_factors_finite_check(law)) return why;
   return viscous_law_factors_sign_check(law);
}

// a law reads the channels the scalar pass stages
inline const char* viscous_law_scalars_check(int n_scalars)
{
   return n_scalars > 0 ? nullptr : "a viscosity law on a context without scalars";
}

// Why a context cannot have the term, or nullptr: the kernel walks the FULL-mode cell rows and neighbour lists of a
// context that holds the whole grid.  full_mode: FULL or FULL_FAST; whole_grid: every plane, never exchanged.
inline const char* viscous_mode_check(bool full_mode) { return full_mode ? nullptr : "FULL and FULL_FAST contexts only"; }

inline const char* viscous_slab_check(bool whole_grid)
{
   return whole_grid ? nullptr : "slab contexts (with neighbours, or that have exchanged) cannot have viscous stress";
}

// sph_hip_set_viscous_stress on a context with ports (an emitter or a sink is set) ...
inline const char* viscous_ports_set_check(bool ports_set)
{
   return ports_set ? "a context with ports cannot have viscous stress" : nullptr;
}

// ... and sph_hip_set_ports on a context with the term
inline const char* viscous_ports_check(bool have_viscous, int n_emitters, int n_sinks)
{
   if (have_viscous && (n_emitters > 0 || n_sinks > 0)) return "a context with viscous stress cannot have ports";
   return nullptr;
}

// the law a context without one reports, and a law with its unused slots cleared (what the context keeps)
inline sph_hip_viscosity_law viscous_law_clean(const sph_hip_viscosity_law* law)
{
   sph_hip_viscosity_law out = {};
   if (!law) return out;
   out.channel = law->channel;
   out.n_keys = law->n_keys;
   for (int k = 0; k < SPH_HIP_MAX_VISCOSITY_KEYS; k++) {
      out.value[k] = k < law->n_keys ? law->value[k] : 0.0f;
      out.factor[k] = k < law->n_keys ? law->factor[k] : 0.0f;
   }
   return out;
}
