// Ports (include/sph_hip.h: sph_hip_set_ports): inflow emitters and outflow sinks, a particle count that
// changes while the steps stay queued.  The argument checks, the firing schedule, the lattice points, the ids
// and the sink test - one set of inline functions for the device (k_ports_apply: port_kernels.h), the host
// (launch.h) and g++ (tests/test_ports_cpu.py, against the numpy restatement tests/port_emulation.py).
// Pure C++17 without HIP; the translation units that use it are compiled with -ffp-contract=off.
//
// The contract.  All arithmetic is fp32, unfused, in the order written.
//   emitter  a = axis, u = (a + 1) % 3, w = (a + 2) % 3 (the convention of the oriented obstacles).  Point k
//            of a layer: i = k % nu, j = k / nu, x_a = origin[a], x_u = origin[u] + (float)i * spacing,
//            x_w = origin[w] + (float)j * spacing - one multiply and one add each.  Every point enters with
//            the emitter's velocity and mass.
//   firing   emitter e fires in port step s iff s >= first && (s - first) % every == 0 && (layers < 0 ||
//            fired_e < layers).  s counts the steps of sph_hip_step / sph_hip_run since the ports were set or
//            the state was uploaded, from 0.
//   ids      the context keeps next_id (host, uint32): an upload sets it to n, an upload with ids to the
//            largest id + 1.  A step's firing emitters take ids in list order: id_base_e = next_id + the
//            points of the firing emitters before e, point k gets id_base_e + k.  A step whose ids would
//            reach 0xffffffff (the dead id) is refused.
//   sink     caught iff lo_c <= x_c && x_c < hi_c on all three axes: NaN is never caught.  A particle in
//            several sinks counts for the lowest index.
//   order    within a step, before its cell build: the sinks look at the entries [0, n_live) the last build
//            left (moved by the last integrate) and write the dead id into the caught entries' id word; then
//            the firing emitters' points are appended at n_live + offset; then meta[META_N_IN] = n_live + m.
//            So a layer is never caught in the step it enters, and it takes part in that whole step: build,
//            sums, integrate.  Sinks act at the START of a step: whatever stands inside a sink after the last
//            step of a run is still there.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/sph_hip.h"

#ifdef __HIPCC__
#define PORT_HD __host__ __device__
#define PORT_INLINE __attribute__((always_inline))
#else
#define PORT_HD
#define PORT_INLINE
#endif

#define PORT_DEAD_ID 0xffffffffu   // SPH_DEAD_ID (sph_device.h)

// The cell grid a context holds, as plain values (sph_device.h: CellGrid).
struct PortGrid {
   int nx, ny, nz_global;   // cells of the whole grid
   float inv;               // cells per unit length
   int z0, nz;              // planes held: [z0, z0 + nz)
};

// What one step's k_ports_apply appends, by value in its kernel arguments: the n emitters that fire, in list
// order, the offset of each one's layer behind n_live, its first id; m = points in all.
struct PortFiring {
   int n, m;
   int emitter[SPH_HIP_MAX_EMITTERS];
   int offset[SPH_HIP_MAX_EMITTERS];
   uint32_t id_base[SPH_HIP_MAX_EMITTERS];
};

// finite: not NaN, not +-inf (a comparison, the same on the device and under g++)
PORT_HD inline bool port_finite(float v) { return fabsf(v) <= 3.402823466e38f; }

// points of one layer (checked: 1 .. SPH_HIP_MAX_EMITTER_POINTS)
PORT_HD PORT_INLINE inline int port_points(const sph_hip_emitter& e) { return e.count[0] * e.count[1]; }

// point k of a layer
PORT_HD PORT_INLINE inline void port_point(const sph_hip_emitter& e, int k, float& x, float& y, float& z)
{
   const int i = k % e.count[0], j = k / e.count[0];
   const int a = e.axis;
   // origin[u] and origin[w] as selects (the values stay in registers on the device)
   const float ou = a == 0 ? e.origin[1] : a == 1 ? e.origin[2] : e.origin[0];
   const float ow = a == 0 ? e.origin[2] : a == 1 ? e.origin[0] : e.origin[1];
   const float oa = a == 0 ? e.origin[0] : a == 1 ? e.origin[1] : e.origin[2];
   const float cu = ou + (float)i * e.spacing;
   const float cw = ow + (float)j * e.spacing;
   x = a == 0 ? oa : a == 1 ? cw : cu;
   y = a == 0 ? cu : a == 1 ? oa : cw;
   z = a == 0 ? cw : a == 1 ? cu : oa;
}

// whether the emitter fires in port step s, having fired `fired` times
PORT_HD PORT_INLINE inline bool port_fires(const sph_hip_emitter& e, long long s, long long fired)
{
   return s >= e.first && (s - e.first) % e.every == 0 && (e.layers < 0 || fired < e.layers);
}

// whether a sink catches a position
PORT_HD PORT_INLINE inline bool port_caught(const sph_hip_sink& k, float x, float y, float z)
{
   return k.lo[0] <= x && x < k.hi[0] && k.lo[1] <= y && y < k.hi[1] && k.lo[2] <= z && z < k.hi[2];
}

// the sink a position counts for: the lowest index that catches it, or -1
PORT_HD PORT_INLINE inline int port_first_sink(const sph_hip_sink* sinks, int ns, float x, float y, float z)
{
   int hit = -1;
   for (int s = ns - 1; s >= 0; s--) hit = port_caught(sinks[s], x, y, z) ? s : hit;
   return hit;
}

// The firing table of port step s: which emitters fire, where their layers go, their ids.
inline PortFiring port_plan(const sph_hip_emitter* emitters, int ne, long long s, const long long* fired,
                            uint32_t next_id)
{
   PortFiring f = {};
   for (int e = 0; e < ne; e++) {
      if (!port_fires(emitters[e], s, fired[e])) continue;
      f.emitter[f.n] = e;
      f.offset[f.n] = f.m;
      f.id_base[f.n] = next_id + (uint32_t)f.m;
      f.m += port_points(emitters[e]);
      f.n++;
   }
   return f;
}

// whether m new ids from next_id on stay below the dead id
inline bool port_ids_fit(uint32_t next_id, int m) { return (uint64_t)next_id + (uint64_t)m <= (uint64_t)PORT_DEAD_ID; }

// The cell coordinate the build gives x along an axis of n cells (sph_device.h: cell_coord) BEFORE its clamp,
// or -1 where the clamp would have to move it (outside the grid, or not finite).
inline int port_cell_unclamped(float x, float inv, int n)
{
   const float fl = floorf(x * inv);
   return (fl >= 0.0f && fl < (float)n) ? (int)fl : -1;
}

// whether the build's cell_of places a position in a real cell of the planes held, without clamping it
inline bool port_in_real_cell(const PortGrid& g, float x, float y, float z)
{
   const int cz = port_cell_unclamped(z, g.inv, g.nz_global);
   return port_cell_unclamped(x, g.inv, g.nx) >= 0 && port_cell_unclamped(y, g.inv, g.ny) >= 0 && cz >= g.z0 &&
          cz < g.z0 + g.nz;
}

// ---- the uniform-mass rule --------------------------------------------------------------------------------
// A context whose resident particles all have one mass skips the mass gather in its density and acceleration
// passes (launch.h: uniform_mass).  With emitters that stays right only while every emitter's mass equals the
// resident one IN BITS (memcmp, not ==: -0.0f and +0.0f differ, a NaN equals itself).
struct PortMassRule {
   int uniform;     // the flag after the rule
   int known;       // whether `mass` is the mass of everything resident
   float mass;      // the resident mass
};

inline bool port_same_bits(float a, float b) { return memcmp(&a, &b, sizeof(float)) == 0; }

// uniform, known, mass: the flag the upload left, whether the uploaded mass is known, and that mass.
// nothing_resident: an upload of no particles that nothing has been emitted into - the emitters' own agreement
// decides, whatever the flag was, and the first emitter's mass becomes the resident one.  Otherwise the flag is
// only ever cleared: by an unknown resident mass, or by an emitter whose mass differs from it.
inline PortMassRule port_mass_rule(int uniform, int known, float mass, const sph_hip_emitter* emitters, int ne,
                                   bool nothing_resident)
{
   PortMassRule r = {uniform, known, mass};
   if (ne == 0) return r;
   if (nothing_resident) {
      r.uniform = 1;
      for (int e = 1; e < ne; e++) r.uniform &= port_same_bits(emitters[e].mass, emitters[0].mass) ? 1 : 0;
      r.known = 1;
      r.mass = emitters[0].mass;
      return r;
   }
   if (!uniform) return r;
   if (!known) {
      r.uniform = 0;
      return r;
   }
   for (int e = 0; e < ne; e++)
      if (!port_same_bits(emitters[e].mass, mass)) r.uniform = 0;
   return r;
}

// ---- checks ---------------------------------------------------------------------------------------------
// Why a pair of lists is refused, or nullptr.
inline const char* port_check(const sph_hip_emitter* emitters, int ne, const sph_hip_sink* sinks, int ns,
                              const PortGrid& grid)
{
   if (ne < 0 || ns < 0) return "negative count";
   if (ne > SPH_HIP_MAX_EMITTERS) return "more than SPH_HIP_MAX_EMITTERS emitters";
   if (ns > SPH_HIP_MAX_SINKS) return "more than SPH_HIP_MAX_SINKS sinks";
   if (ne > 0 && !emitters) return "null emitter list";
   if (ns > 0 && !sinks) return "null sink list";
   for (int i = 0; i < ne; i++) {
      const sph_hip_emitter& e = emitters[i];
      if (e.axis < 0 || e.axis > 2) return "axis must be 0, 1 or 2";
      if (!(port_finite(e.origin[0]) && port_finite(e.origin[1]) && port_finite(e.origin[2]) &&
            port_finite(e.spacing) && port_finite(e.velocity[0]) && port_finite(e.velocity[1]) &&
            port_finite(e.velocity[2]) && port_finite(e.mass)))
         return "an emitter field that is not finite";
      if (!(e.spacing > 0.0f)) return "spacing must be > 0";
      if (e.count[0] < 1 || e.count[1] < 1) return "count must be >= 1";
      if ((long long)e.count[0] * e.count[1] > SPH_HIP_MAX_EMITTER_POINTS)
         return "more than SPH_HIP_MAX_EMITTER_POINTS points in one layer";
      if (!(e.mass > 0.0f)) return "mass must be > 0";
      if (e.first < 0) return "first must be >= 0";
      if (e.every < 1) return "every must be >= 1";
      if (e.layers < -1) return "layers must be >= -1";
      const int n = port_points(e), nu = e.count[0];
      const int corner[4] = {0, nu - 1, n - nu, n - 1};
      for (int c = 0; c < 4; c++) {
         float x, y, z;
         port_point(e, corner[c], x, y, z);
         if (!port_in_real_cell(grid, x, y, z)) return "a lattice corner outside the cell grid";
      }
   }
   for (int i = 0; i < ns; i++) {
      const sph_hip_sink& k = sinks[i];
      for (int c = 0; c < 3; c++) {
         if (!(port_finite(k.lo[c]) && port_finite(k.hi[c]))) return "a sink bound that is not finite";
         if (!(k.hi[c] > k.lo[c])) return "a sink needs hi > lo on every axis";
      }
   }
   return nullptr;
}
