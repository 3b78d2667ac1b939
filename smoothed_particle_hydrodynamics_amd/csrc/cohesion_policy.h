// Cohesion (include/sph_hip.h: sph_hip_set_cohesion): a pairwise surface tension after Becker and Teschner (2007),
// a_i = -gamma * sum_j m_j W(d_ij) (x_i - x_j), with the density pass's own pair term for m_j W.  Inside the fluid
// the neighbours stand on every side and the terms cancel; at a free surface they all stand on one side and pull
// the particle inward.  The pair terms of (i, j) and (j, i) are each other's negation, so momentum is conserved.
// The arithmetic of one particle and every check: one set of inline functions for the device (cohesion_kernels.h)
// and for g++ (tests/test_cohesion_cpu.py, against the numpy restatement tests/cohesion_emulation.py).  Pure C++17
// without HIP; the translation units that use it are compiled with -ffp-contract=off.
//
// The contract.  All arithmetic is fp32, unfused, in the order written.  For particle i of the step's state S_k:
//   members   j with d2 = (dx*dx + dy*dy) + dz*dz < h2, (dx, dy, dz) = r_i - r_j, i itself excluded: the
//             acceleration pass's pairs, in canonical order (ascending FULL cell id, then ascending sorted index)
//   weight    w_j = t_j, the density pass's pair term m_j * (kernel1 * (hscaled2 - d*d)^3) of d = sqrt(d2),
//             correctly rounded, times sim_scale unless the context runs at unit scale.  It is density_term of
//             pair_math.h, which only the device compiles: the kernel calls it and hands w_j to cohesion_pair, and
//             its rule for d > hscaled comes with it - such a member adds w_j = +0.0f times its separation.
//   sum       s = 0.0f per component; for every member in order s = s + w_j * r, r the separation (dx, dy, dz),
//             times sim_scale first unless unit scale; a multiplication and an addition (cohesion_pair)
//   cohesive  c = (-gamma) * s per component (cohesion_accel)
//   guard     c == 0 in all three components, or not finite in any: the particle is left alone by selection and
//             nothing is stored (cohesion_acts).  gamma = 0 is "off" by bits, and an untouched particle keeps
//             its -0.0f's and whatever else its row holds.
//   apply     a' = clamp(a + c), a what the acceleration pass left in acc[p] and clamp accel_end's rule as
//             buoyancy_policy.h restates it (buoyancy_clamp: the one function).  a' is stored to acc[p]; the
//             velocity is not touched: cohesion is an ordinary acceleration, not a weight.
// FULL and FULL_FAST share the arithmetic: nothing here reads what the two modes form differently.  In a step
// cohesion stands behind the acceleration pass and in front of buoyancy, whose a is what cohesion left.
#pragma once

#include "buoyancy_policy.h"

// the running sum of one particle (components written out: no array, which on the device could live in
// scratch memory)
struct CohesionSum {
   float x, y, z;
};

// one member into the sum: w = its weight, (dx, dy, dz) = r_i - r_j
SCALAR_HD SCALAR_INLINE inline void cohesion_pair(CohesionSum& s, float w, float dx, float dy, float dz, float sim_scale,
                                                  bool unit_scale)
{
   const float rx = unit_scale ? dx : dx * sim_scale;
   const float ry = unit_scale ? dy : dy * sim_scale;
   const float rz = unit_scale ? dz : dz * sim_scale;
   const float tx = w * rx, ty = w * ry, tz = w * rz;
   s.x = s.x + tx;
   s.y = s.y + ty;
   s.z = s.z + tz;
}

SCALAR_HD SCALAR_INLINE inline CohesionSum cohesion_accel(float gamma, const CohesionSum& s)
{
   const float m = -gamma;
   return CohesionSum{m * s.x, m * s.y, m * s.z};
}

// whether the particle is touched at all (NaN != 0 is true, so the finite test is what stops it)
SCALAR_HD SCALAR_INLINE inline bool cohesion_acts(const CohesionSum& c)
{
   const bool some = c.x != 0.0f || c.y != 0.0f || c.z != 0.0f;
   return some && scalar_finite(c.x) && scalar_finite(c.y) && scalar_finite(c.z);
}

// One particle with the cohesive acceleration c: a (acc[p].xyz) in place.  The caller has asked cohesion_acts.
SCALAR_HD SCALAR_INLINE inline void cohesion_apply(const CohesionSum& c, float cfl_limit, float cfl_limit2, float& ax, float& ay,
                                                   float& az)
{
   ax = ax + c.x;
   ay = ay + c.y;
   az = az + c.z;
   buoyancy_clamp(ax, ay, az, cfl_limit, cfl_limit2);
}

// ---- checks ---------------------------------------------------------------------------------------------
// whether a gamma switches cohesion off (-0.0f too); a negative gamma is a repulsion and is allowed
inline bool cohesion_is_off(float gamma) { return gamma == 0.0f; }

// Why sph_hip_set_cohesion refuses a gamma, or nullptr
inline const char* cohesion_gamma_check(float gamma)
{
   return scalar_finite(gamma) ? nullptr : "a gamma that is not finite";
}

// Why a context cannot have cohesion, or nullptr: the kernel walks the FULL-mode cell rows and neighbour lists of
// a context that holds the whole grid.  full_mode: FULL or FULL_FAST; whole_grid: every plane, never exchanged.
inline const char* cohesion_context_check(bool full_mode, bool whole_grid)
{
   if (!full_mode) return "FULL and FULL_FAST contexts only";
   if (!whole_grid) return "slab contexts (with neighbours, or that have exchanged) cannot have cohesion";
   return nullptr;
}

// sph_hip_set_cohesion on a context with ports (an emitter or a sink is set) ...
inline const char* cohesion_ports_set_check(bool ports_set)
{
   return ports_set ? "a context with ports cannot have cohesion" : nullptr;
}

// ... and sph_hip_set_ports on a context with cohesion
inline const char* cohesion_ports_check(bool have_cohesion, int n_emitters, int n_sinks)
{
   if (have_cohesion && (n_emitters > 0 || n_sinks > 0)) return "a context with cohesion cannot have ports";
   return nullptr;
}
