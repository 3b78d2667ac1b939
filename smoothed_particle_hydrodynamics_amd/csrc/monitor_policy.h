// Step monitor (include/sph_hip.h: step monitor): what one particle adds to a step's row, how two partial rows
// fold, the row a fold ends in and every argument check - one set of inline functions for the device
// (monitor_kernels.h) and for g++ (tests/test_monitor_cpu.py, against the numpy restatement
// tests/monitor_emulation.py).  Pure C++17 without HIP; the translation units that use it are compiled with
// -ffp-contract=off.
//
// The contract.  All arithmetic is fp32, unfused, in the order written.  For every live sorted slot p of a step -
// its density rho, neighbour count and final acceleration a (behind cohesion and buoyancy), and the position x,
// velocity v, mass m, id and carried channels the step PRODUCED:
//   live      every slot visited adds 1
//   bad       x, y, z of x, v and a, or rho, not finite (scalar_finite), or rho < 0: bad += 1, the id is offered to
//             bad_id_min (the smallest wins; 0xffffffff: none), and the particle takes part in nothing below
//   ranges    v2 = (vx*vx + vy*vy) + vz*vz, a2 likewise; v2_max, a2_max, rho_max, rho_min, ncount_max;
//             lone += 1 where ncount == 0
//   key       floats are compared by monitor_key: bits | 0x80000000 for a clear sign bit, ~bits for a set one - an
//             unsigned integer that rises with the value, -0.0f below +0.0f; the winner's bits do not depend on the
//             order of comparison.  A maximum over nothing is key 0, a minimum over nothing key 0xffffffff (the
//             keys of two NaN patterns, which are never offered); both decode to +0.0f.
//   sums      the terms m*vx, m*vy, m*vz, (0.5f*m)*v2 and m, each widened to double, times 2^-quantum_log2
//             (load_scale: exact); if all five are finite and below 2^38 (LOAD_TERM_LIMIT) in magnitude each goes
//             through llrint into its int64 sum, else none does and skipped += 1: load_policy.h's rule
//   scalars   (a context that carries some, an id inside their rows) per channel c: a finite T_c is offered to
//             scalar_min[c] and scalar_max[c]; scalar_bad += 1 where any of the four is not finite
// and, from the pair pass (every live slot of the step's state S_k: it runs in front of the acceleration pass and
// knows nothing of `bad`):
//   S_p       0.0f, then for every member j of p in canonical order with V_j != 0: S_p = S_p + scalar_weight(V_j, d,
//             hscaled, kernel3), d as the scalar pass forms it, V_j the step's staged volume (monitor_pair)
//   s_max     the maximum of the finite S_p by the key; pair_bad counts the others
// Everything is a maximum, a minimum, a count or an integer sum: partial rows fold in any order to the same bits
// (monitor_merge), and so does a row whatever route the context takes.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/sph_hip.h"
#include "load_policy.h"
#include "scalar_policy.h"

static_assert(sizeof(sph_hip_monitor_row) == 128, "sph_hip_monitor_row is ABI: 128 bytes");

#define MONITOR_NO_ID 0xffffffffu
#define MONITOR_KEY_NO_MAX 0u
#define MONITOR_KEY_NO_MIN 0xffffffffu

// the slots of a partial row
#define MON_SUMS 5   // momentum x, y, z; kinetic; mass
#define MON_ADDS 5
#define MON_ADD_LIVE 0
#define MON_ADD_BAD 1
#define MON_ADD_SKIPPED 2
#define MON_ADD_LONE 3
#define MON_ADD_SCALAR_BAD 4
#define MON_MAXS 8   // unsigned maxima: the neighbour count, then keys
#define MON_MAX_NCOUNT 0
#define MON_MAX_V2 1
#define MON_MAX_A2 2
#define MON_MAX_RHO 3
#define MON_MAX_SCALAR 4   // .. 7
#define MON_MINS 6   // unsigned minima: the bad id, then keys
#define MON_MIN_BAD_ID 0
#define MON_MIN_RHO 1
#define MON_MIN_SCALAR 2   // .. 5

// What a lane, a wave, a workgroup and the whole grid have seen: one layout for all of them.  (On the device
// every index into these arrays is an unrolled constant: they live in registers.)
struct MonitorAcc {
   long long sum[MON_SUMS];
   int32_t add[MON_ADDS];
   uint32_t mx[MON_MAXS];
   uint32_t mn[MON_MINS];
};

// what a workgroup of the pair pass has seen
struct MonitorPairAcc {
   uint32_t s_key;     // key of the largest finite S_p
   int32_t pair_bad;
};

SCALAR_HD SCALAR_INLINE inline uint32_t monitor_bits(float v)
{
   uint32_t b;
   memcpy(&b, &v, sizeof(b));
   return b;
}

SCALAR_HD SCALAR_INLINE inline float monitor_float(uint32_t b)
{
   float v;
   memcpy(&v, &b, sizeof(v));
   return v;
}

SCALAR_HD SCALAR_INLINE inline uint32_t monitor_key(float v)
{
   const uint32_t b = monitor_bits(v);
   return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

SCALAR_HD SCALAR_INLINE inline float monitor_unkey(uint32_t k)
{
   return monitor_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// the float of a folded maximum / minimum: +0.0f where nothing was offered
SCALAR_HD SCALAR_INLINE inline float monitor_max_value(uint32_t k) { return k == MONITOR_KEY_NO_MAX ? 0.0f : monitor_unkey(k); }
SCALAR_HD SCALAR_INLINE inline float monitor_min_value(uint32_t k) { return k == MONITOR_KEY_NO_MIN ? 0.0f : monitor_unkey(k); }

SCALAR_HD SCALAR_INLINE inline uint32_t monitor_umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
SCALAR_HD SCALAR_INLINE inline uint32_t monitor_umin(uint32_t a, uint32_t b) { return a < b ? a : b; }

SCALAR_HD SCALAR_INLINE inline void monitor_clear(MonitorAcc& a)
{
   for (int i = 0; i < MON_SUMS; i++) a.sum[i] = 0;
   for (int i = 0; i < MON_ADDS; i++) a.add[i] = 0;
   for (int i = 0; i < MON_MAXS; i++) a.mx[i] = MONITOR_KEY_NO_MAX;
   for (int i = 0; i < MON_MINS; i++) a.mn[i] = MONITOR_KEY_NO_MIN;
}

// b into a: every slot's own operation, all of them commutative and associative
SCALAR_HD SCALAR_INLINE inline void monitor_merge(MonitorAcc& a, const MonitorAcc& b)
{
   for (int i = 0; i < MON_SUMS; i++) a.sum[i] += b.sum[i];
   for (int i = 0; i < MON_ADDS; i++) a.add[i] += b.add[i];
   for (int i = 0; i < MON_MAXS; i++) a.mx[i] = monitor_umax(a.mx[i], b.mx[i]);
   for (int i = 0; i < MON_MINS; i++) a.mn[i] = monitor_umin(a.mn[i], b.mn[i]);
}

SCALAR_HD SCALAR_INLINE inline void monitor_pair_clear(MonitorPairAcc& a)
{
   a.s_key = MONITOR_KEY_NO_MAX;
   a.pair_bad = 0;
}

SCALAR_HD SCALAR_INLINE inline void monitor_pair_merge(MonitorPairAcc& a, const MonitorPairAcc& b)
{
   a.s_key = monitor_umax(a.s_key, b.s_key);
   a.pair_bad += b.pair_bad;
}

SCALAR_HD SCALAR_INLINE inline bool monitor_is_bad(float px, float py, float pz, float vx, float vy, float vz, float ax,
                                                   float ay, float az, float rho)
{
   const bool finite = scalar_finite(px) && scalar_finite(py) && scalar_finite(pz) && scalar_finite(vx) &&
                       scalar_finite(vy) && scalar_finite(vz) && scalar_finite(ax) && scalar_finite(ay) &&
                       scalar_finite(az) && scalar_finite(rho);
   return !finite || rho < 0.0f;
}

SCALAR_HD SCALAR_INLINE inline float monitor_square(float x, float y, float z) { return (x * x + y * y) + z * z; }

// The five scaled terms of a particle in quanta; false (q untouched): the particle is skipped.
SCALAR_HD SCALAR_INLINE inline bool monitor_terms(float m, float vx, float vy, float vz, float v2, double scale,
                                                  long long q[MON_SUMS])
{
   const float hm = 0.5f * m;
   const float t[MON_SUMS] = {m * vx, m * vy, m * vz, hm * v2, m};
   double s[MON_SUMS];
   bool ok = true;
   for (int c = 0; c < MON_SUMS; c++) {
      s[c] = (double)t[c] * scale;
      ok = ok && isfinite(s[c]) && fabs(s[c]) < LOAD_TERM_LIMIT;
   }
   if (!ok) return false;
   for (int c = 0; c < MON_SUMS; c++) q[c] = llrint(s[c]);
   return true;
}

// One live slot into a.  Returns whether the particle is good (its channels are then offered by monitor_scalars).
SCALAR_HD SCALAR_INLINE inline bool monitor_particle(MonitorAcc& a, float px, float py, float pz, float m, float vx, float vy,
                                                     float vz, uint32_t id, float ax, float ay, float az, float rho,
                                                     int32_t ncount, double scale)
{
   a.add[MON_ADD_LIVE] += 1;
   if (monitor_is_bad(px, py, pz, vx, vy, vz, ax, ay, az, rho)) {
      a.add[MON_ADD_BAD] += 1;
      a.mn[MON_MIN_BAD_ID] = monitor_umin(a.mn[MON_MIN_BAD_ID], id);
      return false;
   }
   const float v2 = monitor_square(vx, vy, vz);
   const float a2 = monitor_square(ax, ay, az);
   a.mx[MON_MAX_V2] = monitor_umax(a.mx[MON_MAX_V2], monitor_key(v2));
   a.mx[MON_MAX_A2] = monitor_umax(a.mx[MON_MAX_A2], monitor_key(a2));
   const uint32_t rk = monitor_key(rho);
   a.mx[MON_MAX_RHO] = monitor_umax(a.mx[MON_MAX_RHO], rk);
   a.mn[MON_MIN_RHO] = monitor_umin(a.mn[MON_MIN_RHO], rk);
   a.mx[MON_MAX_NCOUNT] = monitor_umax(a.mx[MON_MAX_NCOUNT], (uint32_t)(ncount > 0 ? ncount : 0));
   a.add[MON_ADD_LONE] += ncount == 0 ? 1 : 0;
   long long q[MON_SUMS];
   if (monitor_terms(m, vx, vy, vz, v2, scale, q)) {
      for (int c = 0; c < MON_SUMS; c++) a.sum[c] += q[c];
   } else {
      a.add[MON_ADD_SKIPPED] += 1;
   }
   return true;
}

SCALAR_HD SCALAR_INLINE inline void monitor_channel(MonitorAcc& a, int c, float T)
{
   if (!scalar_finite(T)) return;
   const uint32_t k = monitor_key(T);
   a.mx[MON_MAX_SCALAR + c] = monitor_umax(a.mx[MON_MAX_SCALAR + c], k);
   a.mn[MON_MIN_SCALAR + c] = monitor_umin(a.mn[MON_MIN_SCALAR + c], k);
}

// the channels of a good particle
SCALAR_HD SCALAR_INLINE inline void monitor_scalars(MonitorAcc& a, const Scalar4& T)
{
   monitor_channel(a, 0, T.c0);
   monitor_channel(a, 1, T.c1);
   monitor_channel(a, 2, T.c2);
   monitor_channel(a, 3, T.c3);
   const bool finite = scalar_finite(T.c0) && scalar_finite(T.c1) && scalar_finite(T.c2) && scalar_finite(T.c3);
   a.add[MON_ADD_SCALAR_BAD] += finite ? 0 : 1;
}

// one member into S_p (scalar_pair's selection and weight)
SCALAR_HD SCALAR_INLINE inline void monitor_pair(float& S, float V, float d, float hscaled, float kernel3)
{
   const float w = scalar_weight(V, d, hscaled, kernel3);
   S = V != 0.0f ? S + w : S;
}

// a particle's finished S_p into the pair pass's accumulator
SCALAR_HD SCALAR_INLINE inline void monitor_pair_offer(MonitorPairAcc& a, float S)
{
   if (scalar_finite(S)) a.s_key = monitor_umax(a.s_key, monitor_key(S));
   else a.pair_bad += 1;
}

// The row of a folded step.  have_scalars: the step advanced carried scalars (flags bit 0); have_pairs: the pair
// pass ran and `pairs` is its fold (flags bit 1).  Fields that are not valid hold zeros.
SCALAR_HD SCALAR_INLINE inline sph_hip_monitor_row monitor_row_of(const MonitorAcc& a, bool have_scalars, bool have_pairs,
                                                                  const MonitorPairAcc& pairs)
{
   sph_hip_monitor_row r;
   r.momentum[0] = a.sum[0];
   r.momentum[1] = a.sum[1];
   r.momentum[2] = a.sum[2];
   r.kinetic = a.sum[3];
   r.mass = a.sum[4];
   r.live = a.add[MON_ADD_LIVE];
   r.bad = a.add[MON_ADD_BAD];
   r.skipped = a.add[MON_ADD_SKIPPED];
   r.lone = a.add[MON_ADD_LONE];
   r.ncount_max = (int32_t)a.mx[MON_MAX_NCOUNT];
   r.scalar_bad = have_scalars ? a.add[MON_ADD_SCALAR_BAD] : 0;
   r.pair_bad = have_pairs ? pairs.pair_bad : 0;
   r.bad_id_min = a.mn[MON_MIN_BAD_ID];
   r.v2_max = monitor_max_value(a.mx[MON_MAX_V2]);
   r.a2_max = monitor_max_value(a.mx[MON_MAX_A2]);
   r.rho_max = monitor_max_value(a.mx[MON_MAX_RHO]);
   r.rho_min = monitor_min_value(a.mn[MON_MIN_RHO]);
   r.s_max = have_pairs ? monitor_max_value(pairs.s_key) : 0.0f;
   for (int c = 0; c < 4; c++) {
      r.scalar_min[c] = have_scalars ? monitor_min_value(a.mn[MON_MIN_SCALAR + c]) : 0.0f;
      r.scalar_max[c] = have_scalars ? monitor_max_value(a.mx[MON_MAX_SCALAR + c]) : 0.0f;
   }
   r.flags = (have_scalars ? SPH_HIP_MONITOR_SCALARS_VALID : 0u) | (have_pairs ? SPH_HIP_MONITOR_DIFFUSION_VALID : 0u);
   return r;
}

// ---- the recording -----------------------------------------------------------------------------------------
// Steps are numbered 1, 2, ... from the call of sph_hip_record_monitor.  Step s fills row (s - 1) / every when every
// divides s - 1 and that row exists, else none (-1); the row describes step monitor_record_step(row, every).
inline int monitor_record_row(long long step, int every, int rows)
{
   if (step < 1 || (step - 1) % every != 0) return -1;
   const long long r = (step - 1) / every;
   return r < rows ? (int)r : -1;
}

inline int monitor_record_step(int row, int every) { return row * every + 1; }

// ---- checks: each refusal its own function with its own text ---------------------------------------------------
inline const char* monitor_rows_check(int rows) { return rows < 0 ? "rows must be >= 0" : nullptr; }
inline const char* monitor_every_check(int every) { return every < 1 ? "every must be >= 1" : nullptr; }
// (load_check's range: the quantum rule is load_policy.h's)
inline const char* monitor_quantum_check(int quantum_log2) { return load_check(0, quantum_log2); }

// Why a context cannot keep a recording, or nullptr: the kernels read the FULL-mode arrays of a context that holds
// the whole grid.  full_mode: FULL or FULL_FAST; whole_grid: every plane, never exchanged.
inline const char* monitor_mode_check(bool full_mode) { return full_mode ? nullptr : "FULL and FULL_FAST contexts only"; }
inline const char* monitor_slab_check(bool whole_grid)
{
   return whole_grid ? nullptr : "slab contexts (with neighbours, or that have exchanged) cannot keep a step monitor";
}
// sph_hip_record_monitor on a context with ports (an emitter or a sink is set) ...
inline const char* monitor_ports_set_check(bool ports_set)
{
   return ports_set ? "a context with ports cannot keep a step monitor" : nullptr;
}
// ... sph_hip_set_ports on a context with a recording ...
inline const char* monitor_ports_check(int rows, int n_emitters, int n_sinks)
{
   if (rows > 0 && (n_emitters > 0 || n_sinks > 0)) return "a context with a step monitor cannot have ports";
   return nullptr;
}
// ... and the slab exchange on one
inline const char* monitor_exchange_check(int rows)
{
   return rows > 0 ? "a context with a step monitor (sph_hip_record_monitor) cannot exchange with neighbouring slabs" : nullptr;
}

// Why rows [first_row, first_row + n_rows) of `filled` filled rows are refused, or nullptr.
inline const char* monitor_range_check(int first_row, int n_rows, int filled)
{
   if (first_row < 0 || n_rows < 0 || (long long)first_row + n_rows > filled) return "the range leaves the rows filled so far";
   return nullptr;
}
