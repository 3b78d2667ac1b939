// Buoyancy (include/sph_hip.h: sph_hip_set_buoyancy): the carried scalars of scalar_policy.h change a particle's
// weight - warm water rises, salt water sinks.  The arithmetic of one particle and the argument check: one set of
// inline functions for the device (buoyancy_kernels.h) and for g++ (tests/test_buoyancy_cpu.py, against the numpy
// restatement tests/buoyancy_emulation.py).  Pure C++17 without HIP; the translation units that use it are compiled
// with -ffp-contract=off.
//
// The contract.  All arithmetic is fp32, unfused, in the order written.  For particle i of the step's state S_k,
// T_i is the step's staged row Ts[p]: the channels as they stood BEFORE this step's scalar update.
//   excess    s = 0.0f; for c = 0 .. 3: s = s + beta[c] * (T_i,c - reference[c]) (buoyancy_excess)
//   buoyant   b = (-s) * gravity, per component (buoyancy_accel).  With gravity pointing down a positive beta lifts
//             warm fluid, a negative one - a salinity - sinks it.
//   guard     s == 0, or s not finite: the particle is left alone by selection, neither of its rows is stored
//             (buoyancy_acts).  A diffusing channel can go NaN next to the spray (scalar_policy.h: stability): such
//             a particle keeps its own weight, and an untouched particle keeps its -0.0f's.
//   accel     a' = clamp(a + b), a what the acceleration pass left in acc[p] - already clamped by accel_end - and
//             clamp accel_end's own rule restated: dot = (ax*ax + ay*ay) + az*az; where dot > cfl_limit2 every
//             component is multiplied by cfl_limit / sqrt(dot), root and quotient correctly rounded
//             (buoyancy_clamp).  a' is stored to acc[p]: the acceleration read-back shows the total.
//   velocity  v' = v + b * dt, stored to velp[p].xyz; the id word velp[p].w keeps its bits.
// The step's unchanged integrate kernel then runs from (x, v', a').
//
// Why two terms.  The integrate gives a particle's acceleration HALF a time step of velocity, vh = v + a*dt/2, and
// gravity a WHOLE time step more, nv = vh + ag*dt (reference src/sph.cpp:937-1022): gravity acts on the velocity
// through both, 3/2 g*dt a step - the g inside a (accel_end adds it) and ag.  A force that is to change a
// particle's weight by the factor 1 - s must enter both ways: a + b gives vh its b*dt/2, v + b*dt stands in for the
// term the integrate adds for ag, together 3/2 b*dt = -s * 3/2 g*dt.  For a particle with s = 1 and a = gravity:
// a' = g + (-g) = 0 exactly, vh = v' = v - g*dt, nv = (v - g*dt) + g*dt.
// The position sees b*dt one step early: x' = x + vh * dt with vh = v' + a'*dt/2 already holds the whole b*dt of
// v', where gravity's own ag*dt enters the velocity behind the position and moves it only with the next step.  The
// offset is the size of one step's velocity change (b*dt*dt in position) and constant over a run; it is not
// corrected: integrate_particle_hooked stays as it is.
#pragma once

#include "scalar_policy.h"

// s of one particle, in channel order
SCALAR_HD SCALAR_INLINE inline float buoyancy_excess(const sph_hip_buoyancy& b, const Scalar4& T)
{
   float s = 0.0f;
   s = s + b.beta[0] * (T.c0 - b.reference[0]);
   s = s + b.beta[1] * (T.c1 - b.reference[1]);
   s = s + b.beta[2] * (T.c2 - b.reference[2]);
   s = s + b.beta[3] * (T.c3 - b.reference[3]);
   return s;
}

// whether the particle is touched at all (NaN != 0 is true, so the finite test is what stops it)
SCALAR_HD SCALAR_INLINE inline bool buoyancy_acts(float s) { return s != 0.0f && scalar_finite(s); }

// accel_end's clamp (pair_math.h), on the three components of a
SCALAR_HD SCALAR_INLINE inline void buoyancy_clamp(float& ax, float& ay, float& az, float cfl_limit, float cfl_limit2)
{
   const float dot = (ax * ax) + (ay * ay) + (az * az);
   if (dot > cfl_limit2) {
      const float length = sqrtf(dot);
      const float scale = cfl_limit / length;
      ax *= scale;
      ay *= scale;
      az *= scale;
   }
}

// One particle with excess s: a (acc[p].xyz) and v (velp[p].xyz) in place.  The caller has asked buoyancy_acts.
SCALAR_HD SCALAR_INLINE inline void buoyancy_apply(const sph_hip_buoyancy& b, float s, float dt, float cfl_limit, float cfl_limit2,
                                                   float& ax, float& ay, float& az, float& vx, float& vy, float& vz)
{
   const float m = -s;
   const float bx = m * b.gravity[0], by = m * b.gravity[1], bz = m * b.gravity[2];
   ax = ax + bx;
   ay = ay + by;
   az = az + bz;
   buoyancy_clamp(ax, ay, az, cfl_limit, cfl_limit2);
   vx = vx + bx * dt;
   vy = vy + by * dt;
   vz = vz + bz * dt;
}

// ---- checks ---------------------------------------------------------------------------------------------
// whether a setting switches buoyancy off: none given, or every beta zero (-0.0f too)
inline bool buoyancy_is_off(const sph_hip_buoyancy* b)
{
   if (!b) return true;
   for (int c = 0; c < SPH_HIP_SCALAR_CHANNELS; c++)
      if (b->beta[c] != 0.0f) return false;
   return true;
}

// Why sph_hip_set_buoyancy refuses, or nullptr.  A setting that switches buoyancy off is never refused.
inline const char* buoyancy_set_check(const sph_hip_buoyancy* b, int n_scalars)
{
   if (!b) return nullptr;
   for (int c = 0; c < SPH_HIP_SCALAR_CHANNELS; c++)
      if (!scalar_finite(b->beta[c])) return "a beta that is not finite";
   if (buoyancy_is_off(b)) return nullptr;
   if (const char* why = scalar_have_check(n_scalars)) return why;
   for (int c = 0; c < SPH_HIP_SCALAR_CHANNELS; c++)
      if (!scalar_finite(b->reference[c])) return "a reference that is not finite";
   for (int a = 0; a < 3; a++)
      if (!scalar_finite(b->gravity[a])) return "a gravity that is not finite";
   return nullptr;
}
