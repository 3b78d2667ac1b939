// Free bodies (include/sph_hip.h: sph_hip_set_bodies): obstacles that the fluid's own loads set in
// motion.  The argument checks, the per-step advance of a body and its turn inside integrate - one set of
// inline functions for the device (k_bodies_advance, k_integrate_bodies: common_kernels.h) and for g++
// (tests/test_bodies_cpu.py, against the numpy restatement tests/body_emulation.py).
// Pure C++17 without HIP; the translation units that use it are compiled with -ffp-contract=off.
//
// The contract.  All arithmetic is fp32, unfused, in the order written.  Body i belongs to obstacle i;
// an entry with mass == 0 is not a body: it is never advanced and takes the turn it always took.
//   state      BodyState per obstacle: D (the displacement at the end of the last enqueued step), Dprev
//              (at its start), V, and the int64 counters skipped and steps.  body_initial: all zero,
//              except V_c = velocity[c] on the free components.
//   advance    once per step, before that step's integrate, from the row the previous integrate filled
//              (null in the first step after the bodies were set: a zero impulse), e the quantum in force:
//              Dprev = D; for each free component c
//                 J = (float)((double)impulse_q[6 + i][c] * 2^e)
//                 V_c = V_c + J / mass
//                 V_c = V_c + accel_c * dt
//                 D_c = D_c + V_c * dt
//                 D_c < travel_lo[c]: D_c = travel_lo[c], V_c = 0
//                 D_c > travel_hi[c]: D_c = travel_hi[c], V_c = 0
//              a component that is not free keeps V_c = 0 and D_c = 0: nothing is added to it;
//              skipped += skipped[6 + i] of that row; steps += 1.
//   turn       obstacle_respond_moved(obstacle_shifted(o, D), Dprev, D, p, v, q, dt, damping)
//              (obstacle_policy.h); the loads record it exactly as load_obstacles_respond_moving records a
//              moving entry: when q is strictly inside the obstacle as it stands at the end of the step,
//              with the world velocities before and after the turn.
//   lag        The coupling is explicit, with a lag of one step: the impulse received in step k changes
//              the velocity used in step k + 1.  The response treats the solid as infinitely heavy within
//              a step, so a body much lighter than the fluid that touches it in one step gets more
//              impulse than it can absorb and oscillates.  Scenes use bodies several times heavier than
//              the fluid they displace.
//   quantum    the advance must read the impulse in the quantum it was summed with, and a recording must
//              not change the rounding of the impulse a body consumes ("a recording changes no
//              particle"): body_refuses_recording and recording_refuses_bodies.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/sph_hip.h"
#include "load_policy.h"
#include "obstacle_policy.h"

// device state of one obstacle's body: 56 bytes, the int64 words 8-byte aligned
struct BodyState {
   float D[3];
   float Dprev[3];
   float V[3];
   float unused;
   long long skipped;
   long long steps;
};

OBST_HD inline bool body_is(const sph_hip_body& b) { return b.mass != 0.0f; }

// how many entries of a body list are bodies
inline int bodies_count(const sph_hip_body* list, int n)
{
   int k = 0;
   for (int i = 0; i < n; i++) k += body_is(list[i]) ? 1 : 0;
   return k;
}

// Why a body list for `n_obstacles` obstacles under `motion` (n_motion = 0 or n_obstacles entries) is
// refused, or nullptr.  n = 0 clears all bodies.
inline const char* body_check(const sph_hip_body* list, int n, int n_obstacles, const sph_hip_obstacle_motion* motion,
                              int n_motion, int quantum_log2)
{
   if (n != 0 && n != n_obstacles) return "the body count must be 0 or the obstacle count";
   if (n > 0 && !list) return "null body list";
   if (quantum_log2 < LOAD_QUANTUM_MIN || quantum_log2 > LOAD_QUANTUM_MAX) return "quantum_log2 must be in [-64, 32]";
   for (int i = 0; i < n; i++) {
      const sph_hip_body& b = list[i];
      if (!body_is(b)) continue;
      if (!isfinite(b.mass) || !(b.mass > 0.0f)) return "a body's mass must be finite and > 0";
      for (int c = 0; c < 3; c++) {
         if (!isfinite(b.velocity[c])) return "a body's velocity must be finite";
         if (!isfinite(b.accel[c])) return "a body's accel must be finite";
         if (!(b.travel_lo[c] <= 0.0f) || !(b.travel_hi[c] >= 0.0f)) return "a body needs travel_lo <= 0 <= travel_hi";
      }
      if (b.free_axes & ~7u) return "a body's free_axes uses bits 0..2 only";
      if (i < n_motion && motion && obstacle_moves(motion[i])) return "a body on an obstacle whose motion moves";
   }
   return nullptr;
}

// Why a motion list is refused by the bodies in force (sph_hip_set_obstacle_motion), or nullptr.
inline const char* body_motion_check(const sph_hip_obstacle_motion* motion, int n_motion, const sph_hip_body* bodies,
                                     int n_bodies)
{
   for (int i = 0; i < n_motion && i < n_bodies; i++)
      if (body_is(bodies[i]) && obstacle_moves(motion[i])) return "a motion that moves on an obstacle that is a body";
   return nullptr;
}

// Why rotations and bodies do not go together (either list may be empty), or nullptr: posed entries and
// bodies exclude each other within one list, so that k_integrate_bodies never meets a posed entry (one
// function for both directions).
inline const char* body_rotation_check(const sph_hip_obstacle_rotation* rot, int n_rot, const sph_hip_body* bodies,
                                       int n_bodies)
{
   for (int i = 0; i < n_rot && i < n_bodies; i++)
      if (obstacle_posed(rot[i]) && body_is(bodies[i])) return "a posed entry on an obstacle that is a body";
   if (obstacles_posed(rot, n_rot) > 0 && bodies_count(bodies, n_bodies) > 0)
      return "posed entries and bodies in one obstacle list";
   return nullptr;
}

// Why paths and bodies do not go together (either list may be empty), or nullptr: a list with a path holds
// no body, so that k_integrate_bodies never meets a path and the path kernels never a body (one function
// for both directions).
inline const char* path_body_check(const sph_hip_motion_path* paths, int n_paths, const sph_hip_body* bodies,
                                   int n_bodies)
{
   if (paths_count(paths, n_paths) > 0 && bodies_count(bodies, n_bodies) > 0)
      return "paths and free bodies in one obstacle list (paths beside bodies are not built)";
   return nullptr;
}

// The quantum rule, both directions.  n_bodies: bodies in force with quantum body_quantum_log2.
inline const char* body_refuses_recording(int n_bodies, int body_quantum_log2, int rows, int quantum_log2)
{
   if (n_bodies > 0 && rows > 0 && quantum_log2 != body_quantum_log2)
      return "bodies are set with another quantum_log2";
   return nullptr;
}

// rows_left: rows of the recording in force (quantum recording_quantum_log2) not yet filled
inline const char* recording_refuses_bodies(int rows_left, int recording_quantum_log2, int n_bodies, int quantum_log2)
{
   if (n_bodies > 0 && rows_left > 0 && quantum_log2 != recording_quantum_log2)
      return "a recording with another quantum_log2 has rows left";
   return nullptr;
}

inline BodyState body_initial(const sph_hip_body& b)
{
   BodyState s = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, 0.0f, 0, 0};
   if (body_is(b))
      for (int c = 0; c < 3; c++)
         if (b.free_axes >> c & 1u) s.V[c] = b.velocity[c];
   return s;
}

// One advance of body i (see the contract): `row` is the LOAD_ROW_WORDS int64 of the row the previous
// integrate filled, or null.
OBST_HD inline void body_advance(const sph_hip_body& b, BodyState& s, const long long* row, int i, int quantum_log2,
                                 float dt)
{
   if (!body_is(b)) return;
   for (int c = 0; c < 3; c++) s.Dprev[c] = s.D[c];
   for (int c = 0; c < 3; c++) {
      if (!(b.free_axes >> c & 1u)) continue;
      const long long q = row ? row[3 * (6 + i) + c] : 0;
      const float J = (float)ldexp((double)q, quantum_log2);
      float V = s.V[c] + J / b.mass;
      V = V + b.accel[c] * dt;
      float D = s.D[c] + V * dt;
      if (D < b.travel_lo[c]) {
         D = b.travel_lo[c];
         V = 0.0f;
      }
      if (D > b.travel_hi[c]) {
         D = b.travel_hi[c];
         V = 0.0f;
      }
      s.V[c] = V;
      s.D[c] = D;
   }
   if (row) s.skipped += row[LOAD_ROW_SKIPPED + 6 + i];
   s.steps += 1;
}

// A body's turn inside integrate.  Returns whether q was strictly inside the obstacle as it stands at
// the end of the step (what the load recorder calls a response).
OBST_HD inline bool body_turn(const sph_hip_obstacle& o, const BodyState& s, const float p[3], float v[3], float q[3],
                              float dt, float damping)
{
   const sph_hip_obstacle o1 = obstacle_shifted(o, s.D);
   const bool in = obstacle_inside(o1, q);
   obstacle_respond_moved(o1, s.Dprev, s.D, p, v, q, dt, damping);
   return in;
}

// load_obstacles_respond_moving (load_policy.h) for a list with bodies: each entry takes the body turn
// (body_turn, written out: the shifts come from its state), the obstacle_turn of its motion (motion may be
// null: no motions set), or the static turn.  The two shifted turns share one call site.
template <class Rec>
OBST_HD inline void body_obstacles_respond(const sph_hip_obstacle* list, const sph_hip_obstacle_motion* motion,
                                           const sph_hip_body* bodies, const BodyState* state, int n, const float p[3],
                                           float v[3], float q[3], float dt, float damping, float tau0, float tau1,
                                           float m, const Rec& rec)
{
   for (int i = 0; i < n; i++) {
      const float vb[3] = {v[0], v[1], v[2]};
      float D0[3], D1[3];
      bool shifted = false;
      if (body_is(bodies[i])) {
         for (int c = 0; c < 3; c++) {
            D0[c] = state[i].Dprev[c];
            D1[c] = state[i].D[c];
         }
         shifted = true;
      } else if (motion && obstacle_moves(motion[i])) {
         obstacle_displacement(motion[i], tau0, D0);
         obstacle_displacement(motion[i], tau1, D1);
         shifted = true;
      }
      bool in;
      if (shifted) {
         const sph_hip_obstacle o1 = obstacle_shifted(list[i], D1);
         in = obstacle_inside(o1, q);
         obstacle_respond_moved(o1, D0, D1, p, v, q, dt, damping);
      } else {
         in = obstacle_inside(list[i], q);
         obstacle_respond(list[i], p, v, q, dt, damping);
      }
      rec(6 + i, in, m, vb, v);
   }
}
