// Launch decisions of the host code as functions of plain values: which LDS tile capacities the
// tiled FULL-mode passes get, when the neighbour lists and the trimmed slab messages grow, which
// plane ranges a slab's cell build sorts, and which phase events a timed step records.
// Pure C++17 without HIP (tests/test_launch_policy.py compiles it with g++); the runtime queries,
// environment switches and pinned feedback words are read by the callers and passed in.
#pragma once

#include <stdint.h>

#include "../../include/sph_hip.h"

// particles (= threads) of one workgroup of the tiled FULL-mode passes
#ifndef TILE_THREADS
#define TILE_THREADS 256
#endif
// The tile lives in dynamic LDS: its capacity (candidate positions per workgroup) is a launch
// parameter, chosen by the host from the tile sizes the previous steps needed, because the
// workgroups a CU can hold (and with them the latency hiding of both passes) is set by the LDS
// a workgroup asks for: 12 B (density) / 16 B (acceleration) per tile entry.
#define TILE_PAD 32                      // slots past the capacity that aligned 8-slot reads may touch
#define TILE_CAP_MAX (4096 - TILE_PAD)        // tile indices are 12-bit in narrow list entries
#define TILE_CAP_MAX_WIDE (16384 - TILE_PAD)  // ... 14-bit in wide ones

// Per-step statistics of the LDS tiles (k_tile_desc), fed back to the host's choice of tile
// capacity: how many workgroups would not fit each candidate capacity.
#define TILE_CANDS 12
enum {
   TSTAT_OVER = 0,            // [TILE_CANDS] workgroups whose tile exceeds candidate i
   TSTAT_BLOCKS = 12,         // workgroups counted
   TSTAT_MAX = 13,            // largest tile
   TSTAT_GIVEUP_DENSITY = 14, // entries of the give-up lists of the current step
   TSTAT_GIVEUP_ACCEL = 15,
   TSTAT_NO_LIST = 16,        // particles with more neighbours than their list holds (density pass)
   TSTAT_COUNT = 17
};
struct TileCaps {
   int cand[TILE_CANDS];    // ascending candidate capacities (the occupancy levels of both kernels)
   int n_cand;
   int cap_density;         // capacities the current step's launches use
   int cap_accel;
   int wide;                // list entries carry a 14-bit tile index (a capacity above 4064)
};

// trimmed slab messages grow back to their allocated size when one is more than 4/5 full
#define SLAB_GROW_FILL_NUM 4
#define SLAB_GROW_FILL_DEN 5

// ---- placement of workgroups on the XCDs ---------------------------------------------------
// Which of `nblocks` 256-particle workgroups hardware workgroup `block` computes.  The dispatcher deals
// consecutive block indices round-robin over the 8 XCDs; every residue class of block mod 8 owns a
// contiguous share of the workgroups (the first nblocks mod 8 classes one more than the others), so that
// neighbouring workgroups, which share most of their tile, meet in one L2.  ascending: a class walks its
// share from the bottom up, as the density pass does; descending: from the top down - the SAME share, so
// the acceleration pass starts each XCD where the density pass has just ended it and reads what that
// wrote (lists, rho, velB, auxc, counts) while it is still in that XCD's L2 and the Infinity Cache.
// Bijective onto [0, nblocks) for any nblocks >= 1 either way.  A placement only: no result depends on it.
#define XCD_COUNT 8
constexpr inline int xcd_share_begin(int xcd, int nblocks)
{
   return xcd < nblocks % XCD_COUNT ? xcd * (nblocks / XCD_COUNT + 1)
                                    : (nblocks % XCD_COUNT) * (nblocks / XCD_COUNT + 1) +
                                         (xcd - nblocks % XCD_COUNT) * (nblocks / XCD_COUNT);
}
constexpr inline int xcd_share_size(int xcd, int nblocks)
{
   return nblocks / XCD_COUNT + (xcd < nblocks % XCD_COUNT ? 1 : 0);
}
constexpr inline int xcd_workgroup_ascending(int block, int nblocks)
{
   return xcd_share_begin(block % XCD_COUNT, nblocks) + block / XCD_COUNT;
}
constexpr inline int xcd_workgroup_descending(int block, int nblocks)
{
   return xcd_share_begin(block % XCD_COUNT, nblocks) + xcd_share_size(block % XCD_COUNT, nblocks) - 1 -
          block / XCD_COUNT;
}

// ---- LDS tile capacity ---------------------------------------------------------------------
// For every workgroups-per-CU count B a tiled kernel can reach, the largest tile (multiple of
// 32 entries) that still lets B workgroups share a CU.  Registers and waves: the runtime's
// occupancy calculator.  LDS: the MI355X hands a workgroup its LDS (static + dynamic) in units of
// 1280 bytes out of 160 KiB per CU - measured with a sweep of pinned capacities (tools/cap_sweep.py:
// the density pass drops from 6 to 5 workgroups per CU between 2176 and 2208 entries and from 5 to
// 4 between 2624 and 2656, the acceleration pass from 4 to 3 between 2496 and 2528; the
// calculator's own rounding is finer, and a size it rated 3/CU ran at 2/CU, which rounds 1-2 used
// to cover with 2 KiB of slack per workgroup at the price of 130-190 entries per level).
#define LDS_PER_CU (160 * 1024)
#define LDS_GRANULE 1280

// relative throughput by workgroups per CU (index 1..6)
// (On the 4M column at rest, with one pass pinned to each level - tools/occupancy_prices.py,
// round 3 - the passes lose more than this below 5 per CU: density 1 / 0.97 / 0.87 / 0.74 / 0.54 at
// 6 .. 2, acceleration 1 / 0.935 / 0.82 / 0.60 at 5 .. 2.  With those figures the breaking dam,
// whose large tiles also hold more work per workgroup, ran 2-10 % slower in five of its sixteen
// windows and faster in none: the tables stay as the breaking dam tuned them.)
static const float DENSITY_THR[7] = {0.0f, 0.33f, 0.62f, 0.85f, 0.93f, 0.97f, 1.0f};
static const float ACCEL_THR[7] = {0.0f, 0.40f, 0.68f, 0.87f, 0.98f, 1.0f, 1.0f};
// what a workgroup whose tile fits no capacity costs, in units of a tiled one: the density pass
// (k_full_density_chunked) and the acceleration pass searching untiled ...
// (Round 4: 3 since that kernel confirms at the pop and stages its appends; the 600-step transient of the
// breaking 4M dam - tools/dam_windows.py - takes 1712 ms with 6, 1690 with 3, 1697 with 2, 1799 with 1.5.)
#ifndef DENSITY_GIVEUP_COST
#define DENSITY_GIVEUP_COST 3.0f
#endif
#define ACCEL_UNTILED_COST 8.0f
// ... and what a workgroup of the acceleration pass costs on the list-driven route without a tile
// (accel_from_lists)
#ifndef ACCEL_LISTED_COST
#define ACCEL_LISTED_COST 2.5f
#endif

// the capacity levels of one tiled kernel, ascending, with the workgroups per CU each allows
struct TileLevels {
   int cap[TILE_CANDS];
   int per_cu[TILE_CANDS];
   int n;
};

// blocks_at(cap): workgroups per CU of a tile of `cap` entries (0: no answer from the runtime)
template <class BlocksAt>
TileLevels search_levels(BlocksAt blocks_at, int bytes_per_entry)
{
   TileLevels t = {};
   // a workgroup may take the whole LDS of a CU (160 KiB); the 14-bit tile index of wide list
   // entries stops a little earlier for 12-byte entries
   int cap_max = TILE_CAP_MAX_WIDE;
   while (cap_max > 256 && (long long)(cap_max + TILE_PAD) * bytes_per_entry > 156 * 1024) cap_max -= 32;
   const int cap_min = 1024 - TILE_PAD;
   int prev = 0;
   for (int want = blocks_at(cap_min); want >= 1 && t.n < TILE_CANDS / 2; want--) {
      int lo = cap_min, hi = cap_max;            // largest cap with blocks_at(cap) >= want
      while (lo < hi) {
         const int mid = lo + ((hi - lo) / 32 + 1) / 2 * 32;
         if (blocks_at(mid) >= want) lo = mid;
         else hi = mid - 32;
      }
      if (lo > prev) {
         t.per_cu[t.n] = want;
         t.cap[t.n++] = prev = lo;
      }
      if (lo >= cap_max) break;
   }
   if (t.n == 0) {                                 // no answer from the runtime: a size that fits
      t.per_cu[t.n] = 3;
      t.cap[t.n++] = 3008;
   }
   return t;
}

// candidates = ascending union of both kernels' levels
inline void merge_candidates(const TileLevels& d, const TileLevels& a, TileCaps& caps)
{
   int nd = 0, na = 0;
   caps.n_cand = 0;
   while ((nd < d.n || na < a.n) && caps.n_cand < TILE_CANDS) {
      const int x = nd < d.n ? d.cap[nd] : INT32_MAX;
      const int y = na < a.n ? a.cap[na] : INT32_MAX;
      const int v = x < y ? x : y;
      if (x == v) nd++;
      if (y == v) na++;
      caps.cand[caps.n_cand++] = v;
   }
}

// workgroups of the last reported step whose tile exceeds `cap` (all of them when it is no candidate)
inline int over_at(const TileCaps& caps, const int* fb, int cap)
{
   int over = fb[TSTAT_BLOCKS];
   for (int c = 0; c < caps.n_cand; c++)
      if (caps.cand[c] == cap) over = fb[TSTAT_OVER + c];
   return over;
}

// Level with the least expected cost for the workgroups of the latest reported step.  A larger
// tile means fewer workgroups per CU (relative throughput thr), a smaller one sends the workgroups
// that do not fit down the untiled route (several times the work, and ~100 us from start to end
// however little else there is to do - launches too short to hide that must not have any).
// Nothing reported yet: the level next to 3008 entries.
inline int pick_level(const TileCaps& caps, const int* fb, const TileLevels& lv, const float* thr,
                      float untiled_cost, int over_other = -1, float listed_cost = 0.0f)
{
   const int blocks = fb[TSTAT_BLOCKS];
   if (blocks <= 0) {
      for (int l = 0; l < lv.n; l++)
         if (lv.cap[l] >= 3008) return lv.cap[l];
      return lv.cap[lv.n - 1];
   }
   const bool hides_untiled = blocks >= 8192 * 256 / TILE_THREADS;
   int best = lv.cap[lv.n - 1];
   float best_cost = 1e30f;
   for (int l = 0; l < lv.n; l++) {
      const int over = over_at(caps, fb, lv.cap[l]);
      if (over > 0 && !hides_untiled && l + 1 < lv.n) continue;
      const float f = (float)over / (float)blocks;
      const int b = lv.per_cu[l] < 1 ? 1 : (lv.per_cu[l] > 6 ? 6 : lv.per_cu[l]);
      // (acceleration pass: of the workgroups that do not fit, those that fitted the density pass
      // have their lists and take the cheaper list-driven route without a tile)
      float f_search = f;
      if (over_other >= 0) f_search = (float)(over_other < over ? over_other : over) / (float)blocks;
      const float cost = (1.0f - f) / thr[b] + untiled_cost * f_search + listed_cost * (f - f_search);
      if (cost < best_cost) {
         best_cost = cost;
         best = lv.cap[l];
      }
   }
   return best;
}

// The capacities of the step about to be launched, from the feedback counters fb[TSTAT_COUNT].
// forced > 0 (SPH_HIP_TILE_CAP) pins both; forced_accel / forced_density (SPH_HIP_TILE_CAP_ACCEL /
// _DENSITY, multiples of 32) then make one pass's capacity smaller, and are ignored when they are not.
inline void choose_caps(TileCaps& caps, const int* fb, const TileLevels& density, const TileLevels& accel,
                        int forced, int forced_accel, int forced_density)
{
   if (forced > 0) {
      caps.cap_density = caps.cap_accel = forced;
      // (tests: a smaller capacity for the acceleration pass alone sends the workgroups in between
      // down its list-driven route without a tile)
      if (forced_accel >= 256 && forced_accel < caps.cap_accel) caps.cap_accel = forced_accel;
      // (... and a smaller one for the density pass alone: workgroups that fit the acceleration
      // pass's capacity but are on the give-up lists all the same)
      if (forced_density >= 256 && forced_density < caps.cap_density) caps.cap_density = forced_density;
      caps.wide = forced > TILE_CAP_MAX;
      return;
   }
   caps.cap_density = pick_level(caps, fb, density, DENSITY_THR, DENSITY_GIVEUP_COST);
   caps.cap_accel = pick_level(caps, fb, accel, ACCEL_THR, ACCEL_UNTILED_COST,
                               over_at(caps, fb, caps.cap_density), ACCEL_LISTED_COST);
   // both passes of a step read and write the same lists: one entry format for the two
   caps.wide = caps.cap_density > TILE_CAP_MAX || caps.cap_accel > TILE_CAP_MAX;
}

// ---- neighbour lists -----------------------------------------------------------------------
// The density pass reported `without` particles with more neighbours than their lists hold out
// of `blocks` workgroups: enlarge the lists when that is more than 0.4 %.
inline bool lists_should_grow(int without, int blocks)
{
   return without > 64 && without > blocks * (TILE_THREADS / 256);
}

// the next smaller list capacity to try when an allocation fails: 1022 -> 510 -> 254
inline int smaller_list_cap(int want) { return (want / 2 - 1) & ~1; }

// ---- trimmed slab messages -----------------------------------------------------------------
// `most` records in the fullest message of any rank: back to the allocated size when that is
// more than 4/5 of the active size
inline int grown_active_records(long long most, int active, int capacity)
{
   const bool grow = most * SLAB_GROW_FILL_DEN > (long long)active * SLAB_GROW_FILL_NUM && active < capacity;
   return grow ? capacity : active;
}

// one rank's wish for the message size: what it packed last with head room, at most what the
// buffers hold, at least one record
inline int trim_records(int most, float slack, int extra, int capacity)
{
   const double want_d = (double)most * (double)slack + (double)extra;
   const int want = want_d > (double)capacity ? capacity : (int)want_d;
   return want < 1 ? 1 : want;
}

// ---- slab plane ranges (local planes, 0 = the first plane held) -----------------------------
struct PlaneRanges {
   int own_lo, own_hi;   // owned planes
   int sum_lo, sum_hi;   // density planes: one wider, clipped to what is held
   int bnd_lo, bnd_hi;   // owned planes next to a neighbouring slab end / begin here
};

inline PlaneRanges plane_ranges(int plane_lo, int plane_hi, int z0, int nz, int halo, bool have_left,
                                bool have_right)
{
   PlaneRanges r;
   r.own_lo = plane_lo - z0;
   r.own_hi = plane_hi - z0;
   r.sum_lo = r.own_lo - 1 < 0 ? 0 : r.own_lo - 1;
   r.sum_hi = r.own_hi + 1 > nz ? nz : r.own_hi + 1;
   // owned planes next to a neighbouring slab, one wider than the halo (early exchange): a
   // particle further inside cannot reach the planes that are sent within one step
   const int border = halo + 1;
   r.bnd_lo = !have_left ? r.own_lo : (r.own_lo + border < r.own_hi ? r.own_lo + border : r.own_hi);
   r.bnd_hi = !have_right ? r.own_hi : (r.own_hi - border > r.own_lo ? r.own_hi - border : r.own_lo);
   return r;
}

// ---- integrate routes -----------------------------------------------------------------------
// Whether the tiled acceleration pass of a whole-grid context also integrates and hashes
// (FusedStep), instead of a k_integrate launch behind it: `hash_too` (FULL mode, whole grid, never
// exchanged, prehash allowed), the tiled kernels, particles to move, no SPH_HIP_NO_FUSED_INTEGRATE,
// and no static obstacles - their response runs in k_integrate_obst, the fused kernels stay as tuned.
// record_loads: the step fills a row of a load recording (sph_hip_record_loads), which only
// k_integrate_loads does.  buoyancy: the step launches a kernel that stands between the acceleration pass and the
// integrate - k_buoyancy_apply (step_launches_buoyancy), k_cohesion_apply (step_launches_cohesion) or both; such a
// step keeps the prehash, in k_integrate<HASH>.
inline bool fuse_integrate(bool hash_too, bool tiled, int n, bool no_fused_integrate, int n_obstacles,
                           bool record_loads = false, bool buoyancy = false)
{
   return hash_too && tiled && n > 0 && !no_fused_integrate && n_obstacles == 0 && !record_loads && !buoyancy;
}

// Whether a slab's early-exchange step (sph_hip_slab_step_begin / _end) integrates, hashes and packs
// in its acceleration launches (FusedStep.slab), instead of k_slab_pack_early + k_integrate: not
// with SPH_HIP_NO_FUSED_SLAB, nor with static obstacles (k_slab_pack_early_obst + k_integrate_obst),
// nor while a load recording has rows left (k_slab_pack_early[_obst] + k_integrate_loads).
inline bool fuse_slab_step(bool no_fused_slab, int n_obstacles, bool record_loads = false)
{
   return !no_fused_slab && n_obstacles == 0 && !record_loads;
}

// Whether a step's integrate, and a slab's early pack, take the kernels for moving obstacles
// (k_integrate_obst_moving, k_integrate_loads_moving, k_slab_pack_early_obst_moving) and the motion clock
// advances: some entry of the motion list moves.  A context in which nothing moves launches what it
// always launched.  (n_obstacles > 0 then also keeps the step off the fused routes above.)
inline bool use_moving_kernels(int n_obstacles, int n_moving) { return n_obstacles > 0 && n_moving > 0; }

// Whether a step's integrate is k_bodies_advance followed by k_integrate_bodies (free bodies,
// body_policy.h): some entry of the body list is a body.  Such a step always records, into the caller's
// row or an internal one, and it is launched with zero particles too (the bodies still advance).  A
// context without bodies launches what it always launched, with the same arguments.  (n_obstacles > 0
// keeps the step off the fused routes above; the motion clock advances as use_moving_kernels says.)
inline bool use_body_kernels(int n_obstacles, int n_bodies) { return n_obstacles > 0 && n_bodies > 0; }

// Oriented and rotating obstacles (obstacle_policy.h, third part; no launch asks these two yet).  Whether a
// step's integrate would take kernels for posed entries: some entry of the rotation list is posed.  Such a
// list holds no body (body_policy.h: body_rotation_check), so the body kernels are no candidate for it; its
// entries that move, or stand, take their usual turn beside the posed ones.
inline bool use_posed_kernels(int n_obstacles, int n_posed) { return n_obstacles > 0 && n_posed > 0; }

// Whether the motion clock advances with a step: some entry moves (use_moving_kernels) or rotates.  A list
// that is only tilted leaves it standing.
inline bool motion_clock_runs(int n_obstacles, int n_moving, int n_rotating)
{
   return n_obstacles > 0 && (n_moving > 0 || n_rotating > 0);
}

// Motion paths (obstacle_policy.h, fourth part).  Whether a step's integrate is k_paths_eval followed by
// k_integrate_obst_path or k_integrate_loads_path: some entry of the path list has a path.  Asked ahead of
// use_moving_kernels - the path kernels give an entry without a path the turn of its motion - and the
// eval is launched with zero particles too (the shifts still advance).  Such a list holds no body
// (body_policy.h: path_body_check).  A context without paths launches what it always launched.
inline bool use_path_kernels(int n_obstacles, int n_paths) { return n_obstacles > 0 && n_paths > 0; }

// Whether the motion clock advances with a step of a context that may hold paths: some entry moves
// (use_moving_kernels) or has a path.
inline bool path_clock_runs(int n_obstacles, int n_moving, int n_paths)
{
   return n_obstacles > 0 && (n_moving > 0 || n_paths > 0);
}

// ---- ports (port_policy.h) ------------------------------------------------------------------
// Whether a step launches k_ports_apply in front of its cell build: some emitter or sink is set.  Then it
// runs every step, because after a build meta[META_N_IN] is stale and must be reset to n_live even when
// nothing fires.  A context without ports launches what it always launched.
inline bool ports_active(int n_emitters, int n_sinks) { return n_emitters > 0 || n_sinks > 0; }

// A context with ports never prehashes: its integrate cannot count for a build whose entries the ports
// change first.  (fuse_integrate(hash_too = false, ...) is then false by itself.)
inline bool ports_no_prehash(bool no_prehash_switch, int n_emitters, int n_sinks)
{
   return no_prehash_switch || ports_active(n_emitters, n_sinks);
}

// The host bound: ctx->n stays an upper bound of meta[META_N_IN]; each step adds the m it enqueues.
// Whether a step of m new points must first wait for the queued steps and tighten the bound to n_live ...
inline bool ports_must_tighten(int bound, int m, int capacity) { return (long long)bound + m > (long long)capacity; }
// ... and whether, with the live count known, the step is enqueued at all (else SPH_HIP_ERR_CAPACITY: no
// partial layer is ever emitted)
inline bool ports_layer_fits(int live, int m, int capacity) { return (long long)live + m <= (long long)capacity; }

// ---- gauges (gauge_policy.h) -------------------------------------------------------------------
// Which kernels one evaluation of a gauge set launches: k_gauges_read where the set holds a field kind,
// k_gauges_pressure where it holds a pressure kind (gauge_set_counts).  A set without a pressure kind
// launches what it always launched.
inline bool gauges_launch_field(int n_field) { return n_field > 0; }
inline bool gauges_launch_pressure(int n_pressure) { return n_pressure > 0; }

// Where the pressure kinds' particle densities come from.  Inside a step, after its density pass, the
// pass's own array (of exactly the state the other gauges saw); everywhere else - sph_hip_read_gauges,
// the pressure samplers, the stand-alone sph_hip_integrate - the context's own buffer, filled by
// k_particle_density behind the cell build, whatever an earlier sph_hip_compute_density left.
#define GAUGE_DENSITY_OF_STEP 0
#define GAUGE_DENSITY_OWN 1
inline int gauge_density_source(bool behind_step_density) { return behind_step_density ? GAUGE_DENSITY_OF_STEP : GAUGE_DENSITY_OWN; }

// Whether a step reads pressure gauges between its density and acceleration passes: it fills row `row`
// of a recording (-1: none) and the set holds a pressure kind.
inline bool step_reads_pressure(int row, int n_pressure) { return row >= 0 && gauges_launch_pressure(n_pressure); }

// ---- carried scalars (scalar_policy.h) ----------------------------------------------------------
// Whether a step launches the scalar pass (k_scalars_stage, k_scalars_step) between its density and its
// acceleration pass: the context carries scalars and has particles.  A context without scalars launches
// what it always launched.
inline bool step_launches_scalars(int n_scalars, int n) { return n_scalars > 0 && n > 0; }

// Whether a step launches k_buoyancy_apply (buoyancy_policy.h) between its acceleration pass and its integrate: a
// buoyancy is set, and the step has staged the scalars it reads (step_launches_scalars).  Such a step gives up the
// fused integrate (fuse_integrate).  A context without buoyancy launches what it always launched.
inline bool step_launches_buoyancy(bool have_buoyancy, int n_scalars, int n)
{
   return have_buoyancy && step_launches_scalars(n_scalars, n);
}

// Whether a step launches k_cohesion_apply (cohesion_policy.h) between its acceleration pass and its integrate, in
// front of buoyancy's kernel: a gamma is set and the step has particles.  Such a step gives up the fused integrate
// (fuse_integrate's last argument).  A context without cohesion launches what it always launched.
inline bool step_launches_cohesion(bool have_cohesion, int n) { return have_cohesion && n > 0; }

// Whether a step launches k_xsph_stage and k_xsph_apply (xsph_policy.h) between its acceleration pass and its
// integrate, behind cohesion's kernel and in front of buoyancy's: an eps is set and the step has particles.  Such
// a step gives up the fused integrate and keeps the prehash, as a cohesive step does.  A context without the
// setting launches what it always launched.
inline bool step_launches_xsph(bool have_xsph, int n) { return have_xsph && n > 0; }

// Whether a step launches k_viscous_stage and k_viscous_apply (viscous_policy.h) between its acceleration pass and
// its integrate, behind cohesion's kernel and in front of XSPH's: a mu is set and the step has particles.  Such a
// step gives up the fused integrate and keeps the prehash, as a smoothing step does.  A context without the setting
// launches what it always launched.
inline bool step_launches_viscous(bool have_viscous, int n) { return have_viscous && n > 0; }

// ---- step monitor (monitor_policy.h) ---------------------------------------------------------------
// The grid of k_monitor_particles: workgroups of MONITOR_THREADS lanes that stride over the live slots, one per 256
// slots up to MONITOR_MAX_BLOCKS - a bounded number of partial rows, which one workgroup folds (k_monitor_finish).
// At least one, so that a step without particles still writes its (empty) row.
#define MONITOR_THREADS 256
#define MONITOR_MAX_BLOCKS 1024
inline int monitor_grid(int n)
{
   const long long want = ((long long)(n > 0 ? n : 0) + MONITOR_THREADS - 1) / MONITOR_THREADS;
   return want < 1 ? 1 : want > MONITOR_MAX_BLOCKS ? MONITOR_MAX_BLOCKS : (int)want;
}

// Whether a step that fills a monitor row launches k_monitor_pairs behind its scalar pass: exactly when that pass
// ran (step_launches_scalars), whose staged volumes it reads.
inline bool monitor_launches_pairs(int n_scalars, int n) { return step_launches_scalars(n_scalars, n); }

// Whether a frame launches the tint pass (k_scalars_stage once, then k_tint_surface or k_tint_column per row
// chunk: tint_kernels.h): the caller is sph_hip_render_scalars and a particle is resident.  Without a particle
// there is no fluid pixel to tint; sph_hip_render and sph_hip_render_scene launch what they always launched.
inline bool frame_launches_tint(bool have_tint, int n_particles) { return have_tint && n_particles > 0; }

// How a workgroup of the scalar pass, and a lane of it, meets its neighbours.  LISTS: the lane walks the
// neighbour list the density pass wrote for the acceleration pass; ROWS: it walks the nine cell rows as
// k_particle_density does.  Same pairs, same order, same arithmetic: same bits.  wg_flag is
// nlist_overflow[wg] (neighbor_lists.h: LISTS_ALL 0, LISTS_NONE 1, LISTS_SOME 2); an untiled context
// (SPH_HIP_UNTILED=1) has no lists at all, and force_rows (SPH_HIP_SCALAR_ROWS=1, read at creation: tests and
// cost runs) sends every workgroup down the row walk.
#define SCALAR_ROUTE_LISTS 0
#define SCALAR_ROUTE_ROWS 1
#define SCALAR_FLAG_LISTS_NONE 1u
#define SCALAR_FLAG_LISTS_SOME 2u
#define SCALAR_WORD_NO_LIST 0xffffffffu   // NLIST_NO_LIST: the first list word of a lane that went without a list
constexpr inline int scalar_workgroup_route(bool tiled, bool force_rows, uint32_t wg_flag)
{
   return (tiled && !force_rows && wg_flag != SCALAR_FLAG_LISTS_NONE) ? SCALAR_ROUTE_LISTS : SCALAR_ROUTE_ROWS;
}
// a lane of a LISTS workgroup: count = its neighbours, first_word = the first 32 bits of its list (which mean
// anything but entries only in a LISTS_SOME workgroup, for a lane with neighbours)
constexpr inline int scalar_lane_route(int wg_route, uint32_t wg_flag, int count, uint32_t first_word)
{
   return (wg_route == SCALAR_ROUTE_ROWS ||
           (wg_flag == SCALAR_FLAG_LISTS_SOME && count > 0 && first_word == SCALAR_WORD_NO_LIST))
             ? SCALAR_ROUTE_ROWS
             : SCALAR_ROUTE_LISTS;
}

// ---- timing --------------------------------------------------------------------------------
// Phase boundary k of a timed step is marked by event phase_event(full, k) of the step's ring
// slot.  An event record is a barrier packet (several microseconds on the stream), so a boundary
// with no launch before it shares the previous boundary's event: FULL mode has no separate
// neighbour search, and computePressure is a no-op in the reference (src/sph.cpp:253-263).
inline int phase_event(bool full_mode, int k)
{
   if (k == 4) return 3;
   if (k == 2 && full_mode) return 1;
   return k;
}

// whether a step at timing `level` records the event of boundary k (SUMS: the interval 1 .. 5)
inline bool records_boundary(int level, bool full_mode, int k)
{
   if (level == SPH_HIP_TIMING_PHASES) return phase_event(full_mode, k) == k;
   return level == SPH_HIP_TIMING_SUMS && (k == 1 || k == 5);
}

// Which events the step about to be enqueued records: `level` on every stride-th timed step,
// nothing on the others (an event record is a barrier packet of ~10 us on the stream: sampling
// keeps the measurement from weighing on what it measures).  `seen` counts the timed steps.
inline int next_step_level(bool timed, int level, long long& seen, int stride)
{
   if (!timed || level == SPH_HIP_TIMING_OFF) return SPH_HIP_TIMING_OFF;
   const bool sample = (seen++ % stride) == 0;
   return sample ? level : SPH_HIP_TIMING_OFF;
}
