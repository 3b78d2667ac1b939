// Gauges (include/sph_hip.h: sph_hip_set_gauges): fixed instruments that read the field inside the step.
// The argument checks, the probe points, the arithmetic of every reading and the record bookkeeping - one set
// of inline functions for the device (k_gauges_read: gauge_kernels.h) and for g++ (tests/test_gauges_cpu.py,
// against the numpy restatement tests/gauge_emulation.py).
// Pure C++17 without HIP; the translation units that use it are compiled with -ffp-contract=off.
//
// The contract.  All arithmetic is fp32, unfused, in the order written.  walk(S, p) is the field sampler's
// walk at p over the state S with velocity (sample_kernels.h: sample_walk<UNIT_SCALE, true>): the raw sums
// rho, vx, vy, vz and count of SampleSum<true>, before any normalisation.  One wave of 64 lanes evaluates a
// gauge; lane l takes the probes q = l, l + 64, l + 128, ... in that order (one trip of the wave each).
//   probes   COLUMN   q = k: the base with coordinate `axis` replaced by origin[axis] + (float)k * spacing[0]
//            SECTION  q = j * nu + i: the corner with the first other axis at origin[u] + (float)i * spacing[0]
//                     and the second at origin[v] + (float)j * spacing[1] (u < v, the axes that are not `axis`)
//            POINT    the origin
//   wet      a probe is wet when rho > iso (strictly; a NaN density is dry)
//   POINT    v = {rho, vx / rho, vy / rho, vz / rho} (0 for rho <= 0: SampleSum::store), n = count, k = 0
//   COLUMN   n = wet probes, k = the largest wet index or -1, v[1] = (float)n * spacing[0];
//            p_k = origin[axis] + (float)k * spacing[0];
//            k == -1:    v[0] = origin[axis], v[2] = 0, v[3] = rho_0
//            k == m - 1: v[0] = p_k, v[2] = rho_k, v[3] = 0
//            otherwise   fa = rho_k, fb = rho_(k+1), t = (iso - fa) / (fb - fa), t = fminf(fmaxf(t, 0), 1)
//                        (a NaN t becomes 0: the extractor's rule), v[0] = p_k + t * (p_(k+1) - p_k),
//                        v[2] = fa, v[3] = fb
//   SECTION  every lane keeps a = r = 0.0f and, for its probes in order, a = a + (the raw velocity sum of the
//            normal axis), r = r + rho; a lane without a probe in a trip adds nothing.  The 64 lane values are
//            summed by the butterfly x = x + x[lane ^ d], d = 1, 2, 4, 8, 16, 32; area = spacing[0] *
//            spacing[1]; v = {a_sum * area, (float)n * area, r_sum, 0}, n = wet probes, k = 0
// With no particle resident every walk gives zeros.
//
// The pressure kinds (PRESSURE = 4, PRESSURE_PATCH = 5; 3 stays refused as an unknown kind).  rho_j is the FULL
// density pass's density of particle j in the state S (the particle itself excluded, canonical order,
// density_untiled's arithmetic: the same bits in FULL and FULL_FAST and on every route), and
//   P_j      = (rho_j - rho0) * stiffness: gauge_particle_pressure, the first line of neighbor_terms, with the
//            context's constants at the time of the call or at the time the step is enqueued; not clamped
//   pwalk(S, p): the sampler's members and terms t_j at p (a particle at p included) and, beside rho and count,
//            pw = sum of t_j * P_j in canonical order (sample_walk with PressureSum: pressure_kernels.h)
//   pressure = rho > 0 ? pw / rho : 0: gauge_pressure_quotient, the Shepard normalisation of the velocity.  A
//            probe at a wall has half its support empty; the quotient is what makes that reading a pressure.
//   PRESSURE        one probe at the origin: v = {pressure, rho, pw, 0}, n = count, k = 0
//   PRESSURE_PATCH  SECTION's rectangle of probes, lane l taking probes l, l + 64, ...; every lane keeps
//            a = r = 0.0f and, for its WET probes in order, a = a + pressure (the quotient of that probe),
//            r = r + rho; a dry or missing probe adds nothing.  The 64 lane values are summed by SECTION's
//            butterfly; area = spacing[0] * spacing[1]; v = {a_sum * area (the force along the normal),
//            (float)n * area (the wetted area), n > 0 ? a_sum / (float)n : 0 (the mean pressure), r_sum},
//            n = wet probes, k = 0
// The field kinds are read by k_gauges_read and the pressure kinds by k_gauges_pressure (gauge_read_by); a
// kernel walks and stores nothing for a gauge of the other family (gauge_field_probes, gauge_pressure_probes).
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/sph_hip.h"
#include "sample_policy.h"

#ifdef __HIPCC__
#define GAUGE_HD __host__ __device__
#define GAUGE_INLINE __attribute__((always_inline))
#else
#define GAUGE_HD
#define GAUGE_INLINE
#endif

#define GAUGE_WAVE 64

// finite: not NaN, not +-inf (a comparison, the same on the device and under g++)
GAUGE_HD inline bool gauge_finite(float v) { return fabsf(v) <= 3.402823466e38f; }

// component `axis` of three values (a select, not an index: the values stay in registers on the device)
GAUGE_HD GAUGE_INLINE inline float gauge_pick(float a0, float a1, float a2, int axis)
{
   return axis == 0 ? a0 : axis == 1 ? a1 : a2;
}

// the pressure kinds: read by k_gauges_pressure, with the particle densities of the state
GAUGE_HD GAUGE_INLINE inline bool gauge_is_pressure(int kind)
{
   return kind == SPH_HIP_GAUGE_PRESSURE || kind == SPH_HIP_GAUGE_PRESSURE_PATCH;
}

// the kinds whose probes are SECTION's rectangle
GAUGE_HD GAUGE_INLINE inline bool gauge_is_rectangle(int kind)
{
   return kind == SPH_HIP_GAUGE_SECTION || kind == SPH_HIP_GAUGE_PRESSURE_PATCH;
}

// probes of one gauge (checked: at most SPH_HIP_MAX_GAUGE_PROBES)
GAUGE_HD GAUGE_INLINE inline int gauge_probes(const sph_hip_gauge& g)
{
   return g.kind == SPH_HIP_GAUGE_COLUMN ? g.count[0] : gauge_is_rectangle(g.kind) ? g.count[0] * g.count[1] : 1;
}

// which launch reads a gauge: the field kinds by k_gauges_read, the pressure kinds by k_gauges_pressure
#define GAUGE_LAUNCH_FIELD 0
#define GAUGE_LAUNCH_PRESSURE 1
GAUGE_HD GAUGE_INLINE inline int gauge_read_by(int kind) { return gauge_is_pressure(kind) ? GAUGE_LAUNCH_PRESSURE : GAUGE_LAUNCH_FIELD; }

// the probes a kernel walks for a gauge: none for a gauge the other kernel reads (and then it stores nothing)
GAUGE_HD GAUGE_INLINE inline int gauge_field_probes(const sph_hip_gauge& g)
{
   return gauge_read_by(g.kind) == GAUGE_LAUNCH_FIELD ? gauge_probes(g) : 0;
}

GAUGE_HD GAUGE_INLINE inline int gauge_pressure_probes(const sph_hip_gauge& g)
{
   return gauge_read_by(g.kind) == GAUGE_LAUNCH_PRESSURE ? gauge_probes(g) : 0;
}

// how many gauges of a (checked) set each launch reads: out[GAUGE_LAUNCH_FIELD], out[GAUGE_LAUNCH_PRESSURE]
inline void gauge_set_counts(const sph_hip_gauge* list, int n, int out[2])
{
   out[0] = out[1] = 0;
   for (int i = 0; i < n; i++) out[gauge_read_by(list[i].kind)]++;
}

// whether a set holds a pressure kind
inline bool gauge_set_has_pressure(const sph_hip_gauge* list, int n)
{
   int c[2];
   gauge_set_counts(list, n, c);
   return c[GAUGE_LAUNCH_PRESSURE] > 0;
}

// trips of the wave over a gauge's probes
GAUGE_HD GAUGE_INLINE inline int gauge_trips(int probes) { return (probes + GAUGE_WAVE - 1) / GAUGE_WAVE; }

// coordinate of a column's probe k along its axis
GAUGE_HD GAUGE_INLINE inline float gauge_column_coord(const sph_hip_gauge& g, int k)
{
   return gauge_pick(g.origin[0], g.origin[1], g.origin[2], g.axis) + (float)k * g.spacing[0];
}

// probe q of a gauge
GAUGE_HD GAUGE_INLINE inline void gauge_probe(const sph_hip_gauge& g, int q, float& px, float& py, float& pz)
{
   px = g.origin[0];
   py = g.origin[1];
   pz = g.origin[2];
   if (g.kind == SPH_HIP_GAUGE_COLUMN) {
      const float c = gauge_column_coord(g, q);
      px = g.axis == 0 ? c : px;
      py = g.axis == 1 ? c : py;
      pz = g.axis == 2 ? c : pz;
   } else if (gauge_is_rectangle(g.kind)) {
      const int i = q % g.count[0], j = q / g.count[0];
      // the other two axes in ascending order: (1, 2), (0, 2), (0, 1)
      const float cu = (g.axis == 0 ? g.origin[1] : g.origin[0]) + (float)i * g.spacing[0];
      const float cv = (g.axis == 2 ? g.origin[1] : g.origin[2]) + (float)j * g.spacing[1];
      px = g.axis == 0 ? px : cu;
      py = g.axis == 0 ? cu : g.axis == 1 ? py : cv;
      pz = g.axis == 2 ? pz : cv;
   }
}

GAUGE_HD GAUGE_INLINE inline bool gauge_wet(float rho, float iso) { return rho > iso; }

// What one trip adds to a gauge's wet count and topmost wet probe: mask holds the wet lanes of trip `trip`
// (bit l = probe trip * 64 + l).  The same value in every lane.
GAUGE_HD GAUGE_INLINE inline int gauge_count_wet(int n, unsigned long long mask) { return n + __builtin_popcountll(mask); }

GAUGE_HD GAUGE_INLINE inline int gauge_top_wet(int top, unsigned long long mask, int trip)
{
   return mask ? trip * GAUGE_WAVE + (63 - __builtin_clzll(mask)) : top;
}

// which two probes a column walks again once its top k is known: first and first + 1 (where the column has it)
GAUGE_HD GAUGE_INLINE inline int gauge_column_again(int k) { return k < 0 ? 0 : k; }

// ---- readings ---------------------------------------------------------------------------------------
GAUGE_HD GAUGE_INLINE inline sph_hip_gauge_reading gauge_point_reading(float rho, float vx, float vy, float vz, int count)
{
   // SampleSum::store's normalisation
   const bool pos = rho > 0.0f;
   sph_hip_gauge_reading r;
   r.v[0] = rho;
   r.v[1] = pos ? vx / rho : 0.0f;
   r.v[2] = pos ? vy / rho : 0.0f;
   r.v[3] = pos ? vz / rho : 0.0f;
   r.n = count;
   r.k = 0;
   return r;
}

// n wet probes, the topmost k; f0 = rho of probe gauge_column_again(k), f1 = rho of the one above it (unused
// where the column has none)
GAUGE_HD GAUGE_INLINE inline sph_hip_gauge_reading gauge_column_reading(const sph_hip_gauge& g, int n, int k, float f0, float f1)
{
   sph_hip_gauge_reading r;
   r.n = n;
   r.k = k;
   r.v[1] = (float)n * g.spacing[0];
   const int m = g.count[0];
   if (k < 0) {
      r.v[0] = gauge_pick(g.origin[0], g.origin[1], g.origin[2], g.axis);
      r.v[2] = 0.0f;
      r.v[3] = f0;
   } else if (k == m - 1) {
      r.v[0] = gauge_column_coord(g, k);
      r.v[2] = f0;
      r.v[3] = 0.0f;
   } else {
      const float pk = gauge_column_coord(g, k), pk1 = gauge_column_coord(g, k + 1);
      float t = (g.iso - f0) / (f1 - f0);
      t = fminf(fmaxf(t, 0.0f), 1.0f);
      r.v[0] = pk + t * (pk1 - pk);
      r.v[2] = f0;
      r.v[3] = f1;
   }
   return r;
}

// a_sum, r_sum: the butterfly sums of the lanes' accumulators
GAUGE_HD GAUGE_INLINE inline sph_hip_gauge_reading gauge_section_reading(const sph_hip_gauge& g, int n, float a_sum, float r_sum)
{
   const float area = g.spacing[0] * g.spacing[1];
   sph_hip_gauge_reading r;
   r.v[0] = a_sum * area;
   r.v[1] = (float)n * area;
   r.v[2] = r_sum;
   r.v[3] = 0.0f;
   r.n = n;
   r.k = 0;
   return r;
}

// the pressure of a particle of density rho_j: the first line of neighbor_terms (pair_math.h); not clamped
GAUGE_HD GAUGE_INLINE inline float gauge_particle_pressure(float rho_j, float rho0, float stiffness)
{
   return (rho_j - rho0) * stiffness;
}

// Shepard normalisation of a probe's pressure sum (SampleSum::store's rule for the velocity)
GAUGE_HD GAUGE_INLINE inline float gauge_pressure_quotient(float pw, float rho) { return rho > 0.0f ? pw / rho : 0.0f; }

// rho, pw, count: the raw sums of the probe's pressure walk
GAUGE_HD GAUGE_INLINE inline sph_hip_gauge_reading gauge_pressure_reading(float rho, float pw, int count)
{
   sph_hip_gauge_reading r;
   r.v[0] = gauge_pressure_quotient(pw, rho);
   r.v[1] = rho;
   r.v[2] = pw;
   r.v[3] = 0.0f;
   r.n = count;
   r.k = 0;
   return r;
}

// what a probe adds to its lane's accumulators of a patch: its pressure and its density when wet, nothing when
// dry or missing
GAUGE_HD GAUGE_INLINE inline void gauge_patch_add(bool wet, float rho, float pw, float& a, float& r)
{
   const float pr = gauge_pressure_quotient(pw, rho);
   a = wet ? a + pr : a;
   r = wet ? r + rho : r;
}

// n wet probes; a_sum, r_sum: the butterfly sums of the lanes' accumulators
GAUGE_HD GAUGE_INLINE inline sph_hip_gauge_reading gauge_patch_reading(const sph_hip_gauge& g, int n, float a_sum, float r_sum)
{
   const float area = g.spacing[0] * g.spacing[1];
   sph_hip_gauge_reading r;
   r.v[0] = a_sum * area;
   r.v[1] = (float)n * area;
   r.v[2] = n > 0 ? a_sum / (float)n : 0.0f;
   r.v[3] = r_sum;
   r.n = n;
   r.k = 0;
   return r;
}

// ---- checks ---------------------------------------------------------------------------------------------
// Why a gauge set is refused, or nullptr.
inline const char* gauge_check(const sph_hip_gauge* list, int n)
{
   if (n < 0) return "negative count";
   if (n > SPH_HIP_MAX_GAUGES) return "more than SPH_HIP_MAX_GAUGES gauges";
   if (n > 0 && !list) return "null gauge list";
   for (int i = 0; i < n; i++) {
      const sph_hip_gauge& g = list[i];
      if (g.kind != SPH_HIP_GAUGE_POINT && g.kind != SPH_HIP_GAUGE_COLUMN && g.kind != SPH_HIP_GAUGE_SECTION &&
          !gauge_is_pressure(g.kind))
         return "unknown gauge kind";
      if (g.axis < 0 || g.axis > 2) return "axis must be 0, 1 or 2";
      if (!(gauge_finite(g.origin[0]) && gauge_finite(g.origin[1]) && gauge_finite(g.origin[2]) &&
            gauge_finite(g.spacing[0]) && gauge_finite(g.spacing[1]) && gauge_finite(g.iso)))
         return "a field that is not finite";
      if (g.kind == SPH_HIP_GAUGE_POINT || g.kind == SPH_HIP_GAUGE_PRESSURE) continue;
      const int used = g.kind == SPH_HIP_GAUGE_COLUMN ? 1 : 2;
      long long probes = 1;
      for (int a = 0; a < used; a++) {
         if (!(g.spacing[a] > 0.0f)) return "spacing must be > 0";
         if (g.count[a] < 1) return "count must be >= 1";
         probes *= g.count[a];
      }
      if (probes > SPH_HIP_MAX_GAUGE_PROBES) return "more than SPH_HIP_MAX_GAUGE_PROBES probes in one gauge";
      if (!(g.iso > 0.0f)) return g.kind == SPH_HIP_GAUGE_PRESSURE_PATCH ? "a pressure patch's iso must be > 0" : "iso must be > 0";
   }
   return nullptr;
}

// ---- recording ---------------------------------------------------------------------------------------
// rows x gauges readings on the device, within the scratch budget the sampler, the extractor and the renderer
// are sized to (sample_policy.h: SAMPLE_SCRATCH_BUDGET, 64 MiB)
inline long long gauge_record_bytes(int rows, int gauges)
{
   return (long long)rows * gauges * (long long)sizeof(sph_hip_gauge_reading);
}

inline const char* gauge_record_check(int rows, int every, int gauges)
{
   if (rows < 0) return "rows must be >= 0";
   if (every < 1) return "every must be >= 1";
   if (gauge_record_bytes(rows, gauges) > SAMPLE_SCRATCH_BUDGET) return "the rows exceed the 64 MiB scratch budget";
   if (rows > 0 && gauges == 0) return "no gauges are set";
   return nullptr;
}

// Steps are numbered 1, 2, ... from the call of sph_hip_record_gauges.  Step s reads the gauges in the state
// it starts from and fills row (s - 1) / every when every divides s - 1 and that row exists, else none (-1):
// the tracers' rule.  Row r is the state after gauge_record_steps_done(r, every) steps: row 0 the state at the
// call.
inline int gauge_record_row(long long step, int every, int rows)
{
   if (step < 1 || (step - 1) % every != 0) return -1;
   const long long r = (step - 1) / every;
   return r < rows ? (int)r : -1;
}

inline int gauge_record_steps_done(int row, int every) { return row * every; }

inline const char* gauge_range_check(int first, int n, int have)
{
   if (first < 0 || n < 0 || (long long)first + n > have) return "the range leaves the rows filled so far";
   return nullptr;
}
