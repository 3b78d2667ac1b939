// Loads on walls and obstacles (include/sph_hip.h: sph_hip_record_loads): what one collision response
// adds to a solid's row, and the wall and obstacle responses with a recorder called at every solid's
// turn - one set of inline functions for the device (k_integrate_loads: common_kernels.h) and for g++
// (tests/test_loads_cpu.py, against the numpy restatement tests/load_emulation.py).
// Pure C++17 without HIP; the translation units that use it are compiled with -ffp-contract=off.
//
// The contract.
//   solids     column s of a row: 0..5 the domain walls x-lo, x-hi, y-lo, y-hi, z-lo, z-hi (the branch
//              order of handleBoundaryConditions, reference src/sph.cpp:1025-1121), 6 + i obstacle i of
//              the list.  A row has SPH_HIP_LOAD_SOLIDS columns.
//   response   one applyBoundary call for a wall (new position < 0 / > max on that axis), or one
//              obstacle_respond call in which obstacle_inside(o, q) held at that obstacle's turn (the
//              fallback that leaves the velocity alone included).  vb: the velocity just before the
//              call, va: just after, m: the particle's mass.
//   term       j_c = m * (vb_c - va_c) per component, fp32, unfused: the impulse given to the solid;
//              s_c = (double)j_c * 2^(-e), e = quantum_log2 (exact: a power of two times an fp32);
//              if the three s_c are finite and |s_c| < 2^38: impulse[s][c] += llrint(s_c) (ties to
//              even), count[s] += 1; otherwise nothing is added and skipped[s] += 1.
// Every accumulator is an int64: the sum does not depend on the order of the terms.  2^38 per term times
// 2^24 responses on one solid in one step stays below 2^62.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/sph_hip.h"
#include "obstacle_policy.h"

#define LOAD_QUANTUM_DEFAULT (-24)
#define LOAD_QUANTUM_MIN (-64)
#define LOAD_QUANTUM_MAX 32
#define LOAD_TERM_LIMIT 274877906944.0   // 2^38

// int64 words of one row in device memory: impulse[SOLIDS][3], then count[SOLIDS], then skipped[SOLIDS]
#define LOAD_ROW_WORDS (5 * SPH_HIP_LOAD_SOLIDS)
#define LOAD_ROW_COUNT (3 * SPH_HIP_LOAD_SOLIDS)
#define LOAD_ROW_SKIPPED (4 * SPH_HIP_LOAD_SOLIDS)

// Why a recording is refused, or nullptr.
inline const char* load_check(int rows, int quantum_log2)
{
   if (rows < 0) return "rows must be >= 0";
   if (quantum_log2 < LOAD_QUANTUM_MIN || quantum_log2 > LOAD_QUANTUM_MAX) return "quantum_log2 must be in [-64, 32]";
   return nullptr;
}

// Why rows [first_row, first_row + n_rows) of a recording of `rows` rows are refused, or nullptr.
inline const char* load_range_check(int first_row, int n_rows, int rows)
{
   if (first_row < 0 || n_rows < 0) return "first_row and n_rows must be >= 0";
   if (first_row > rows || n_rows > rows - first_row) return "the range leaves the allocated rows";
   return nullptr;
}

// 2^(-quantum_log2)
OBST_HD inline double load_scale(int quantum_log2) { return ldexp(1.0, -quantum_log2); }

// The term of one response in quanta; false (q untouched): the response is skipped.
OBST_HD inline bool load_term(float m, const float vb[3], const float va[3], double scale, long long q[3])
{
   double s[3];
   bool ok = true;
   for (int c = 0; c < 3; c++) {
      const float d = vb[c] - va[c];
      const float j = m * d;
      s[c] = (double)j * scale;
      ok = ok && isfinite(s[c]) && fabs(s[c]) < LOAD_TERM_LIMIT;
   }
   if (!ok) return false;
   for (int c = 0; c < 3; c++) q[c] = llrint(s[c]);
   return true;
}

// SPH::handleBoundaryConditions / applyBoundary (reference src/sph.cpp:1025-1148): x, then y, then z;
// reflect at a wall with unit normal along the axis, continue for the rest of the step scaled by
// mDamping (the reference's vec3 operators are component-wise fp32 operations).  rec(solid, hit, m, vb,
// va) is called for BOTH walls of every axis, hit or not: a device recorder votes across the wave.  With
// LoadNoRecorder it is the plain wall response, which every hooked integrate uses; handle_boundaries of
// common_kernels.h computes the same operation for operation for the kernels without a hook.
template <class Rec>
OBST_HD inline void load_walls_respond(const float maxv[3], float damping, const float pos[3], float nv[3],
                                       float dt, float np[3], float m, const Rec& rec)
{
   for (int axis = 0; axis < 3; axis++) {
      const bool lo = np[axis] < 0.0f;
      const bool hi = !lo && np[axis] > maxv[axis];
      const float vb[3] = {nv[0], nv[1], nv[2]};
      if (lo || hi) {
         const float dist = lo ? -pos[axis] / nv[axis] : (maxv[axis] - pos[axis]) / nv[axis];
         float normal[3] = {0.0f, 0.0f, 0.0f};
         normal[axis] = lo ? 1.0f : -1.0f;
         float inter[3], refl[3];
         for (int c = 0; c < 3; c++) inter[c] = pos[c] + (nv[c] * dist);
         const float dot = nv[0] * normal[0] + nv[1] * normal[1] + nv[2] * normal[2];
         for (int c = 0; c < 3; c++) refl[c] = nv[c] - ((normal[c] * dot) * 2.0f);
         const float remaining = dt - dist;
         for (int c = 0; c < 3; c++) {
            nv[c] = refl[c];
            np[c] = inter[c] + refl[c] * (remaining * damping);
         }
      }
      rec(2 * axis, lo, m, vb, nv);
      rec(2 * axis + 1, hi, m, vb, nv);
   }
}

struct LoadNoRecorder { OBST_HD void operator()(int, bool, float, const float*, const float*) const {} };

// obstacles_respond (obstacle_policy.h) with rec called at every obstacle's turn.
template <class Rec>
OBST_HD inline void load_obstacles_respond(const sph_hip_obstacle* list, int n, const float p[3], float v[3],
                                           float q[3], float dt, float damping, float m, const Rec& rec)
{
   for (int i = 0; i < n; i++) {
      const bool in = obstacle_inside(list[i], q);
      const float vb[3] = {v[0], v[1], v[2]};
      obstacle_respond(list[i], p, v, q, dt, damping);
      rec(6 + i, in, m, vb, v);
   }
}

// obstacles_respond_moving (obstacle_policy.h) with rec called at every obstacle's turn: a moving entry's
// turn is recorded when q is inside the obstacle as it stands at the end of the step, vb and va being
// the world velocities before and after that turn.
template <class Rec>
OBST_HD inline void load_obstacles_respond_moving(const sph_hip_obstacle* list, const sph_hip_obstacle_motion* motion,
                                                  int n, const float p[3], float v[3], float q[3], float dt,
                                                  float damping, float tau0, float tau1, float m, const Rec& rec)
{
   for (int i = 0; i < n; i++) {
      const float vb[3] = {v[0], v[1], v[2]};
      const bool in = obstacle_turn(list[i], motion[i], p, v, q, dt, damping, tau0, tau1);
      rec(6 + i, in, m, vb, v);
   }
}

// obstacles_respond_posed (obstacle_policy.h) with rec called at every obstacle's turn: a posed entry's
// turn is recorded when q, taken to the solid's frame at the end of the step, is inside it, vb and va
// being the world velocities before and after that turn.  Column, quantum and skip rules are unchanged.
template <class Rec>
OBST_HD inline void load_obstacles_respond_posed(const sph_hip_obstacle* list, const sph_hip_obstacle_motion* motion,
                                                 const sph_hip_obstacle_rotation* rot, const ObstaclePose* pose, int n,
                                                 const float p[3], float v[3], float q[3], float dt, float damping,
                                                 float tau0, float tau1, float m, const Rec& rec)
{
   for (int i = 0; i < n; i++) {
      const float vb[3] = {v[0], v[1], v[2]};
      const bool in = obstacle_turn_any(list[i], motion ? motion + i : nullptr, rot[i], pose[i], p, v, q, dt, damping,
                                        tau0, tau1);
      rec(6 + i, in, m, vb, v);
   }
}

// A recorder that adds term by term into one row (LOAD_ROW_WORDS int64): what the device's wave
// reductions and atomic adds sum to.
struct LoadRowAdder {
   long long* row;
   double scale;
   void operator()(int s, bool hit, float m, const float* vb, const float* va) const
   {
      if (!hit) return;
      long long q[3];
      if (load_term(m, vb, va, scale, q)) {
         for (int c = 0; c < 3; c++) row[3 * s + c] += q[c];
         row[LOAD_ROW_COUNT + s] += 1;
      } else {
         row[LOAD_ROW_SKIPPED + s] += 1;
      }
   }
};

// obstacles_respond_path (obstacle_policy.h) with rec called at every obstacle's turn: an entry with a path
// is recorded as a moving entry is - q inside the obstacle as it stands at the end of the step, vb and va
// the world velocities before and after that turn.
template <class Rec>
OBST_HD inline void load_obstacles_respond_path(const sph_hip_obstacle* list, const sph_hip_obstacle_motion* motion,
                                                const PathShift* shift, int n, const float p[3], float v[3],
                                                float q[3], float dt, float damping, float tau0, float tau1,
                                                float m, const Rec& rec)
{
   for (int i = 0; i < n; i++) {
      const float vb[3] = {v[0], v[1], v[2]};
      const bool in = obstacle_turn_path(list[i], motion ? motion + i : nullptr, shift[i], p, v, q, dt, damping, tau0,
                                         tau1);
      rec(6 + i, in, m, vb, v);
   }
}
