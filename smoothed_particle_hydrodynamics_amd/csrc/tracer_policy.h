// Tracers (include/sph_hip.h: sph_hip_set_tracers): massless markers the fluid carries.  The argument
// checks, the arithmetic of one advance, the re-sort cadence and the record bookkeeping - one set of inline
// functions for the device (k_tracers_advance: tracer_kernels.h) and for g++ (tests/test_tracers_cpu.py,
// against the numpy restatement tests/tracer_emulation.py).
// Pure C++17 without HIP; the translation units that use it are compiled with -ffp-contract=off.
//
// The contract.  All arithmetic is fp32, unfused, in the order written.  sample(S, p) is the field
// sampler's walk at p over the state S with velocity (sample_kernels.h: sample_walk and SampleSum::store's
// normalisation): the Shepard velocity u and the member count c.  A tracer moves as a particle does: the
// integrate displaces a particle by vh * (dt * sim_scale_inv) (common_kernels.h: pos_dt), so the advance uses
// that same displacement step pos_dt = dt * sim_scale_inv - one fp32 product, formed once on the host when
// the step is enqueued (launch.h: launch_tracers); at unit scale it is dt itself.  One advance of a tracer at
// x, in the state S_k the step's cell build has just sorted:
//   1  (u1, c1) = sample(S_k, x)
//   2  c1 == 0: the tracer is dry this step - x unchanged, dry_steps += 1, done
//   3  half = 0.5f * pos_dt; xm_c = x_c + u1_c * half; (u2, c2) = sample(S_k, xm); u = c2 > 0 ? u2 : u1
//   4  y_c = x_c + u_c * pos_dt; any y_c not finite: dry, as in 2
//   5  apply_walls: y_c < 0 -> y_c = 0; y_c > max_c -> y_c = max_c (a clamp: a marker has no momentum)
//   6  x = y; wet_steps += 1
// The midpoint rule in the velocity field frozen at the start of the step.
#pragma once

#include <math.h>
#include <stdint.h>

#include "sample_policy.h"

#ifdef __HIPCC__
#define TRACER_HD __host__ __device__
#define TRACER_INLINE __attribute__((always_inline))
#else
#define TRACER_HD
#define TRACER_INLINE
#endif

// finite: not NaN, not +-inf (a comparison, the same on the device and under g++)
TRACER_HD inline bool tracer_finite(float v) { return fabsf(v) <= 3.402823466e38f; }

// what one advance needs besides the state: by value in the kernel's arguments
struct TracerStep {
   float pos_dt;         // dt * sim_scale_inv: the integrate's displacement step
   int apply_walls;
   float maxv[3];
   int have_particles;   // 0: nothing resident, every tracer is dry (the cell arrays may be stale)
};

// The move of one advance (the contract above); returns whether the tracer was wet.  sample(px, py, pz, ux, uy, uz) fills the Shepard velocity at p and returns
// the member count; both probes go through the one call site of the two-trip loop.
template <class Sample>
TRACER_HD TRACER_INLINE inline bool tracer_move(float& x0, float& x1, float& x2, const TracerStep& st, const Sample& sample)
{
   // (components written out, no local array: every value stays in a register on the device)
   float p0 = x0, p1 = x1, p2 = x2;
   float u0 = 0.0f, u1 = 0.0f, u2 = 0.0f;
   for (int trip = 0; trip < 2; trip++) {
      float t0, t1, t2;
      const int c = sample(p0, p1, p2, t0, t1, t2);
      if (trip == 0) {
         if (c == 0) return false;
         const float half = 0.5f * st.pos_dt;
         u0 = t0;
         u1 = t1;
         u2 = t2;
         p0 = x0 + t0 * half;
         p1 = x1 + t1 * half;
         p2 = x2 + t2 * half;
      } else if (c > 0) {
         u0 = t0;
         u1 = t1;
         u2 = t2;
      }
   }
   float y0 = x0 + u0 * st.pos_dt, y1 = x1 + u1 * st.pos_dt, y2 = x2 + u2 * st.pos_dt;
   if (!(tracer_finite(y0) && tracer_finite(y1) && tracer_finite(y2))) return false;
   if (st.apply_walls) {
      if (y0 < 0.0f) y0 = 0.0f;
      if (y0 > st.maxv[0]) y0 = st.maxv[0];
      if (y1 < 0.0f) y1 = 0.0f;
      if (y1 > st.maxv[1]) y1 = st.maxv[1];
      if (y2 < 0.0f) y2 = 0.0f;
      if (y2 > st.maxv[2]) y2 = st.maxv[2];
   }
   x0 = y0;
   x1 = y1;
   x2 = y2;
   return true;
}

// tracer_move and the two counters (both written whichever way it went: no store through a chosen address)
template <class Sample>
TRACER_HD TRACER_INLINE inline void tracer_advance(float& x0, float& x1, float& x2, int32_t& wet_steps, int32_t& dry_steps,
                                                   const TracerStep& st, const Sample& sample)
{
   const bool wet = tracer_move(x0, x1, x2, st, sample);
   wet_steps = wet_steps + (wet ? 1 : 0);
   dry_steps = dry_steps + (wet ? 0 : 1);
}

// Why a tracer set is refused, or nullptr.
inline const char* tracer_check(int n, const float* xyz)
{
   if (n < 0) return "negative count";
   if (n > 0 && !xyz) return "null coordinate array";
   for (long long i = 0; i < 3ll * n; i++)
      if (!tracer_finite(xyz[i])) return "a coordinate that is not finite";
   return nullptr;
}

// ---- locality: the slots re-sorted by FULL cell id ------------------------------------------------
// The device keeps the tracers in slots, each carrying its id; no result depends on the slot order.  A
// counting sort over the grid's cells puts tracers of one cell next to each other, so that the lanes of a
// wave walk the same cell rows (profiles/sample_cost.txt: 0.17 ns per coherent probe, 2.36 ns unordered).
// Measured on the 4M dam column (profiles/tracer_cost.txt): see TRACER_SORT_DEFAULT.
#define TRACER_RESORT_EVERY 16
// below this many tracers the advance is a handful of workgroups and the sort's four launches cost more
// than they can save
#define TRACER_SORT_MIN_COUNT 4096
#define TRACER_SORT_DEFAULT 1

// SPH_HIP_TRACER_SORT as read at context creation: unset (-1), 0 = never, n = every n steps
inline int tracer_sort_switch(const char* env)
{
   if (!env || !env[0]) return -1;
   int v = 0;
   for (const char* p = env; *p; p++) {
      if (*p < '0' || *p > '9') return -1;
      if (v < 100000000) v = v * 10 + (*p - '0');
   }
   return v;
}

// steps between two sorts; 0 = never
inline int tracer_resort_every(int sort_switch = -1) { return sort_switch >= 0 ? sort_switch : TRACER_RESORT_EVERY; }

// whether a set of `count` tracers is kept sorted at all (sph_hip_set_tracers sorts once when it is)
inline bool tracer_use_sort(int count, int sort_switch = -1)
{
   if (count < 2) return false;
   if (sort_switch >= 0) return sort_switch > 0;
   return TRACER_SORT_DEFAULT != 0 && count >= TRACER_SORT_MIN_COUNT;
}

// whether the advance about to be enqueued sorts first: steps_since = advances since the last sort
inline bool tracer_sort_due(int count, int sort_switch, long long steps_since)
{
   return tracer_use_sort(count, sort_switch) && steps_since >= tracer_resort_every(sort_switch);
}

// ---- recording ---------------------------------------------------------------------------------------
// rows x count x 3 floats on the device, within the scratch budget the sampler, the extractor and the
// renderer are sized to (sample_policy.h: SAMPLE_SCRATCH_BUDGET, 64 MiB)
inline long long tracer_record_bytes(int rows, int count) { return (long long)rows * count * 3 * (long long)sizeof(float); }

inline const char* tracer_record_check(int rows, int every, int count)
{
   if (rows < 0) return "rows must be >= 0";
   if (every < 1) return "every must be >= 1";
   if (tracer_record_bytes(rows, count) > SAMPLE_SCRATCH_BUDGET) return "the rows exceed the 64 MiB scratch budget";
   return nullptr;
}

// Steps are numbered 1, 2, ... from the call of sph_hip_record_tracers.  Step s fills row (s - 1) / every
// when every divides s - 1 and that row exists, else none (-1): the next step is recorded, then every
// every-th.  Row r holds the positions after step tracer_record_step(r, every).
inline int tracer_record_row(long long step, int every, int rows)
{
   if (step < 1 || (step - 1) % every != 0) return -1;
   const long long r = (step - 1) / every;
   return r < rows ? (int)r : -1;
}

inline int tracer_record_step(int row, int every) { return 1 + row * every; }

inline const char* tracer_range_check(int first, int n, int have)
{
   if (first < 0 || n < 0 || (long long)first + n > have) return "the range leaves what the context holds";
   return nullptr;
}
