// XSPH (include/sph_hip.h: sph_hip_set_xsph): Monaghan's velocity smoothing (1989).  Each step every particle's
// velocity is drawn towards a kernel-weighted mean of its neighbours' velocities,
// v_i' = v_i + eps * sum_j g_ij (v_j - v_i): particle-scale velocity noise decays, a uniform motion and - with equal
// masses - the total momentum stay as they are.  The arithmetic of one particle and every check: one set of inline
// functions for the device (xsph_kernels.h) and for g++ (tests/test_xsph_cpu.py, against the numpy restatement
// tests/xsph_emulation.py).  Pure C++17 without HIP; the translation units that use it are compiled with
// -ffp-contract=off.
//
// The contract.  All arithmetic is fp32, unfused, in the order written.  For particle i of the step's state S_k - with
// one exception: in a context that takes its viscous stress implicitly (viscous_implicit_policy.h) the velocities the
// stage reads are the ones the last viscous sweep of this step left, not S_k's; positions, masses and densities are
// S_k's in either case:
//   stage     every live sorted slot p: R[p] = {v.x, v.y, v.z, 1.0f / rho[p]}, v = velp[cur][p], rho what this
//             step's density pass left; one correctly rounded division (xsph_stage)
//   members   cohesion's exactly: j with d2 = (dx*dx + dy*dy) + dz*dz < h2, (dx, dy, dz) = r_i - r_j, i itself
//             excluded, in canonical order (ascending FULL cell id, then ascending sorted index)
//   weight    g_ij = w_j * (0.5f * (R_i.w + R_j.w)), w_j the density pass's pair term m_j * (kernel1 *
//             (hscaled2 - d*d)^3) of d = sqrt(d2), correctly rounded, times sim_scale unless the context runs at unit
//             scale.  w_j is density_term of pair_math.h, which only the device compiles: the kernel forms it as
//             cohesion's add does and hands it to xsph_pair, and its rule for d > hscaled comes with it - such a member
//             has w_j = +0.0f.  This is Monaghan's 2 m_j W / (rho_i + rho_j) with the arithmetic mean of the inverse
//             densities in place of the inverse of their mean: symmetric in i and j for equal masses, and no
//             division per pair.
//   sum       s = 0.0f per component; for every member in order s.x = s.x + g_ij * (R_j.x - R_i.x), likewise y
//             and z: a subtraction, a multiplication and an addition (xsph_pair)
//   change    dv = eps * s per component (xsph_change)
//   guard     dv == 0 in all three components, or not finite in any: the particle is left alone by selection and
//             nothing is stored (xsph_acts: cohesion_acts' rule).  eps = 0 is "off" by bits; a particle without a
//             neighbour and a uniform velocity field keep their bits.
//   apply     v' = v + dv, stored to velp[cur][p].xyz; .w (the id) keeps its bits (xsph_apply).  No clamp - the
//             acceleration's cfl_limit rule is not a velocity rule - and acc is not touched.
// FULL and FULL_FAST share the arithmetic: nothing here reads what the two modes form differently (positions,
// masses, velocities, member sets, order and densities are the same bits in both).  In a step the pass stands behind
// the acceleration pass and cohesion, in front of buoyancy, whose b*dt is added to the smoothed velocity.
//
// The smoothing is a convex combination of v_i and its neighbours' velocities while eps * sum_j g_ij <= 1; nothing
// polices that sum, the setter keeps eps inside Monaghan's [0, 1].
#pragma once

#include "cohesion_policy.h"

// the staged row of one sorted slot: the velocity and the inverse density
struct XsphRow {
   float x, y, z, w;
};

// the running sum of one particle (components written out: no array, which on the device could live in
// scratch memory)
struct XsphSum {
   float x, y, z;
};

SCALAR_HD SCALAR_INLINE inline XsphRow xsph_stage(float vx, float vy, float vz, float rho)
{
   return XsphRow{vx, vy, vz, 1.0f / rho};
}

// one member into the sum: w = the density pass's pair term of the member
SCALAR_HD SCALAR_INLINE inline void xsph_pair(XsphSum& s, float w, const XsphRow& Ri, const XsphRow& Rj)
{
   const float g = w * (0.5f * (Ri.w + Rj.w));
   const float tx = g * (Rj.x - Ri.x), ty = g * (Rj.y - Ri.y), tz = g * (Rj.z - Ri.z);
   s.x = s.x + tx;
   s.y = s.y + ty;
   s.z = s.z + tz;
}

SCALAR_HD SCALAR_INLINE inline XsphSum xsph_change(float eps, const XsphSum& s)
{
   return XsphSum{eps * s.x, eps * s.y, eps * s.z};
}

// whether the particle is touched at all: cohesion_acts' rule
SCALAR_HD SCALAR_INLINE inline bool xsph_acts(const XsphSum& dv)
{
   return cohesion_acts(CohesionSum{dv.x, dv.y, dv.z});
}

// One particle with the change dv: v (velp[p].xyz) in place.  The caller has asked xsph_acts.
SCALAR_HD SCALAR_INLINE inline void xsph_apply(const XsphSum& dv, float& vx, float& vy, float& vz)
{
   vx = vx + dv.x;
   vy = vy + dv.y;
   vz = vz + dv.z;
}

// ---- checks ---------------------------------------------------------------------------------------------
// whether an eps switches the smoothing off (-0.0f too)
inline bool xsph_is_off(float eps) { return eps == 0.0f; }

// Why sph_hip_set_xsph refuses an eps, or nullptr: Monaghan's range
inline const char* xsph_eps_check(float eps)
{
   if (!scalar_finite(eps)) return "an eps that is not finite";
   if (!(eps >= 0.0f && eps <= 1.0f)) return "an eps outside [0, 1]";
   return nullptr;
}

// Why a context cannot have the smoothing, or nullptr: the kernel walks the FULL-mode cell rows and neighbour lists
// of a context that holds the whole grid.  full_mode: FULL or FULL_FAST; whole_grid: every plane, never exchanged.
inline const char* xsph_context_check(bool full_mode, bool whole_grid)
{
   if (!full_mode) return "FULL and FULL_FAST contexts only";
   if (!whole_grid) return "slab contexts (with neighbours, or that have exchanged) cannot have velocity smoothing";
   return nullptr;
}

// sph_hip_set_xsph on a context with ports (an emitter or a sink is set) ...
inline const char* xsph_ports_set_check(bool ports_set)
{
   return ports_set ? "a context with ports cannot have velocity smoothing" : nullptr;
}

// ... and sph_hip_set_ports on a context with the smoothing
inline const char* xsph_ports_check(bool have_xsph, int n_emitters, int n_sinks)
{
   if (have_xsph && (n_emitters > 0 || n_sinks > 0)) return "a context with velocity smoothing cannot have ports";
   return nullptr;
}
