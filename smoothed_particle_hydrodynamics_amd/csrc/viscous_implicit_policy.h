// Implicit viscous stress (include/sph_hip.h: sph_hip_set_viscous_implicit): the viscous term of viscous_policy.h
// taken by backward Euler, m_i (v_i' - v_i) = dt * sum_j g_ij (v_j' - v_i'), solved by a fixed number of Jacobi
// sweeps on the device.  A mode of the viscous setting: mu and the law are sph_hip_set_viscous_stress's, the stage is
// k_viscous_stage's, the members, their order, the distance and the pair weight g are the explicit pass's.  The
// arithmetic of one particle in one sweep and every check: one set of inline functions for the device
// (viscous_implicit_kernels.h) and for g++ (tests/test_viscous_implicit_cpu.py, against the numpy restatement
// tests/viscous_implicit_emulation.py).  Pure C++17 without HIP; the translation units that use it are compiled with
// -ffp-contract=off.
//
// The contract.  All arithmetic is fp32, unfused, in the order written.
//   setting   sweeps in 0..SPH_HIP_MAX_VISCOUS_SWEEPS.  0 is the explicit term of viscous_policy.h by bits.  The
//             count takes effect only while mu != 0; an upload drops it with the rest of the viscous setting.
//   stage     viscous_policy.h's: X0[p] = R[p] = {v, V_p} and, with a law, M[p].
//   sweep     for sorted slot p, from the rows Xa of the sweep before (X0 for the first): v0 = velp[cur][p].xyz - the
//             particle's own velocity as the step found it, in every sweep - m = posm[p].w, Vi = Xa[p].w, Mi = M[p].
//             Members, their order and d: the explicit pass's.  L = kernel3 * (hscaled - d); g = (m_ij * (Vi * Vj))
//             * L with viscous_pair_mu - viscous_pair's bits; on = Vj != 0.  From s = {0, 0, 0} and D = 0.0f, by
//             selection: s.c = on ? s.c + g * (Xj.c - v0.c) : s.c;  D = on ? D + g : D  (viscous_implicit_pair).
//   change    den = m + dt * D;  dv.c = (dt * s.c) / den: one product and one correctly rounded division per
//             component, none per pair (viscous_implicit_change).  dt is PairConsts::dt, by value.
//   guard     acts = Vi != 0 && m > 0 && den > 0 && cohesion_acts(dv) (viscous_implicit_acts)
//   store     a sweep that is not the last: Xb[p] = {acts ? v0 + dv : v0, Vi} (viscous_implicit_row).  The last:
//             velp[cur][p].xyz = v0 + dv where acts, .w kept; else nothing is stored.
// The formula is (m v0 + dt sum g x_j) / (m + dt sum g), written about v0: a uniform velocity field has exact zero
// differences, stores nothing and keeps its bits.  With one sweep, s is the explicit pass's s bit for bit (X0's rows
// are the velocities v0 is read from).  The pass never reads or writes acc, so FULL and FULL_FAST give the same
// velocities by bits, and no clamp applies (cfl_limit is an acceleration rule, as in XSPH).
//
// Range.  While every g >= 0, each iterate is a convex combination of the particle's own velocity and its
// neighbours' iterates, with weights m / den and dt g / den, for ANY dt and mu >= 0: no component leaves the range of
// the step's velocities by more than rounding, whatever N_i = dt * D / m is.  g >= 0 holds where L >= 0, that is
// where no member stands beyond hscaled - not under DESIGN.md's SHELL parameters, where the convexity claim is not
// made (den > 0 is still guarded).  Two costs.  Convergence is slow where N >> 1: the error contracts like
// N / (1 + N) per sweep, K sweeps reach K neighbour rings, and an under-swept solve acts like a smaller mu.  And a
// truncated solve is not momentum-conserving pair by pair: the defect sum_i m_i (x_i - v0_i) equals the sum of the
// residuals m (x - v0) - dt sum g (x_j - x_i); it falls with the sweeps and vanishes at convergence.  On
// shear_layer(3000, 0.5), momentum 749.5: at 5 times the bulk's explicit limit (N 5.9 in the bulk, 44 at the rim) the
// defect is 1.07 after 2 sweeps and 0.064 after 16, at 50 times 1.85 and 1.79, at a tenth 1.4e-3 and 1e-6 (DESIGN.md:
// implicit viscous stress, with the whole table).
//
// The buffers.  The sweeps ping-pong between viscous_R (row set 0, what the stage writes) and viscous_R2 (row set
// 1): sweep k of K (0-based) reads set k & 1 and, unless it is the last, writes set 1 - (k & 1).  K sweeps take
// K + 1 launches, the stage included, and set 1 is needed from K = 2 on.
#pragma once

#include "viscous_policy.h"

// the running sums of one particle in one sweep
struct ViscousImplicitSum {
   float x, y, z, D;
};

// one member into the sums: m_ij = the pair viscosity, d = the scaled distance, v0 = the particle's own velocity,
// Vi its volume, Xj the neighbour's row of the sweep before
SCALAR_HD SCALAR_INLINE inline void viscous_implicit_pair(ViscousImplicitSum& s, float m_ij, float d, float hscaled,
                                                          float kernel3, float v0x, float v0y, float v0z, float Vi,
                                                          const ViscousRow& Xj)
{
   const float L = kernel3 * (hscaled - d);
   const float g = (m_ij * (Vi * Xj.w)) * L;
   const bool on = Xj.w != 0.0f;
   const float tx = g * (Xj.x - v0x), ty = g * (Xj.y - v0y), tz = g * (Xj.z - v0z);
   s.x = on ? s.x + tx : s.x;
   s.y = on ? s.y + ty : s.y;
   s.z = on ? s.z + tz : s.z;
   s.D = on ? s.D + g : s.D;
}

// den = m + dt * D
SCALAR_HD SCALAR_INLINE inline float viscous_implicit_den(const ViscousImplicitSum& s, float m, float dt)
{
   return m + dt * s.D;
}

// dv = (dt * s) / den per component
SCALAR_HD SCALAR_INLINE inline ViscousSum viscous_implicit_change(const ViscousImplicitSum& s, float den, float dt)
{
   return ViscousSum{(dt * s.x) / den, (dt * s.y) / den, (dt * s.z) / den};
}

// whether the sweep moves the particle at all
SCALAR_HD SCALAR_INLINE inline bool viscous_implicit_acts(float Vi, float m, float den, const ViscousSum& dv)
{
   return Vi != 0.0f && m > 0.0f && den > 0.0f && cohesion_acts(CohesionSum{dv.x, dv.y, dv.z});
}

// the row a sweep that is not the last leaves
SCALAR_HD SCALAR_INLINE inline ViscousRow viscous_implicit_row(bool acts, float v0x, float v0y, float v0z, const ViscousSum& dv,
                                                               float Vi)
{
   return ViscousRow{acts ? v0x + dv.x : v0x, acts ? v0y + dv.y : v0y, acts ? v0z + dv.z : v0z, Vi};
}

// ---- the ping-pong --------------------------------------------------------------------------------------------
// sweep k of K, 0-based: the row set it reads, and the one it writes (-1: the last sweep, which writes velp)
inline int viscous_implicit_source(int k) { return k & 1; }
inline int viscous_implicit_target(int k, int K) { return k + 1 >= K ? -1 : 1 - (k & 1); }
// whether K sweeps need the second row set at all, and the launches of K sweeps (the stage included)
inline bool viscous_implicit_needs_second(int K) { return K >= 2; }
inline int viscous_implicit_launches(int K) { return K > 0 ? K + 1 : 0; }

// ---- checks ---------------------------------------------------------------------------------------------
// whether a count selects the explicit term
inline bool viscous_implicit_is_off(int sweeps) { return sweeps == 0; }

// Why sph_hip_set_viscous_implicit refuses, or nullptr: one function per condition
inline const char* viscous_implicit_sweeps_check(int sweeps)
{
   static_assert(SPH_HIP_MAX_VISCOUS_SWEEPS == 64, "the refusal names the range");
   return (sweeps >= 0 && sweeps <= SPH_HIP_MAX_VISCOUS_SWEEPS) ? nullptr : "a sweep count outside 0..64";
}

inline const char* viscous_implicit_mode_check(bool full_mode)
{
   return full_mode ? nullptr : "FULL and FULL_FAST contexts only";
}

inline const char* viscous_implicit_slab_check(bool whole_grid)
{
   return whole_grid ? nullptr : "slab contexts (with neighbours, or that have exchanged) cannot have an implicit viscous solver";
}

// sph_hip_set_viscous_implicit on a context with ports (an emitter or a sink is set) ...
inline const char* viscous_implicit_ports_set_check(bool ports_set)
{
   return ports_set ? "a context with ports cannot have an implicit viscous solver" : nullptr;
}

// ... and sph_hip_set_ports on a context with the mode
inline const char* viscous_implicit_ports_check(int sweeps, int n_emitters, int n_sinks)
{
   if (sweeps > 0 && (n_emitters > 0 || n_sinks > 0)) return "a context with an implicit viscous solver cannot have ports";
   return nullptr;
}
