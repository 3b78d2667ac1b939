// Phase launches of a step and the step sequence built from them (no host sync inside a step
// except where the tile capacity, the pacing or the list growth needs one, as commented).
#pragma once

#include <math.h>

#include <type_traits>

#include "context.h"

namespace {

// run-time flags -> template arguments: f(std::bool_constant..., one per flag)
template <class F>
void bind_flags(F&& f) { f(); }
template <class F, class... Rest>
void bind_flags(F&& f, bool flag, Rest... rest)
{
   if (flag) bind_flags([&](auto... later) { f(std::true_type{}, later...); }, rest...);
   else bind_flags([&](auto... later) { f(std::false_type{}, later...); }, rest...);
}

PairConsts pair_consts(const sph_hip_params& p, bool fast)
{
   PairConsts k;
   k.h2 = p.h2;
   // SPH_HIP_TEST_SCREEN widens the screen (tests: many candidates then reach the exact
   // confirmation and the list rewrite; the results must not change)
   static const float screen = getenv("SPH_HIP_TEST_SCREEN") ? (float)atof(getenv("SPH_HIP_TEST_SCREEN"))
                                                             : TEST_SCREEN_FACTOR;
   k.h2_screen = p.h2 * (screen >= TEST_SCREEN_FACTOR ? screen : TEST_SCREEN_FACTOR);
   k.hscaled = p.hscaled;
   k.hscaled2 = p.hscaled2;
   k.sim_scale = p.sim_scale;
   k.kernel1 = p.kernel1;
   k.kernel2 = p.kernel2;
   k.kernel3 = p.kernel3;
   {
      // (pair_math.h: accel_pair_fast_pressure) |k2 s| * 2^-shift in [2^-8, 2^-7): times 1 / (d + 0.01)
      // <= 100 the per-pair factor stays below 1, so it cannot overflow unless the reference's own
      // term has; a zero or non-finite product keeps shift 0
      const float k2s = p.kernel2 * p.sim_scale;
      int e = 0, shift = 0;
      if (std::isfinite(k2s) && k2s != 0.0f) {
         (void)frexpf(k2s, &e);            // |k2s| = m * 2^e, m in [0.5, 1)
         shift = e + 7;
         shift = shift < -120 ? -120 : shift > 120 ? 120 : shift;
      }
      k.fast_k2s = ldexpf(k2s, -shift);
      k.fast_unscale = ldexpf(1.0f, shift);
   }
   k.rho0 = p.rho0;
   k.stiffness = p.stiffness;
   k.viscosity = p.viscosity;
   k.grav_const = p.grav_const;
   k.central_mass = p.central_mass;
   k.cx = p.central_pos[0];
   k.cy = p.central_pos[1];
   k.cz = p.central_pos[2];
   k.softening = p.softening;
   k.cfl_limit = p.cfl_limit;
   k.cfl_limit2 = p.cfl_limit2;
   k.dt = p.time_step;
   k.sim_scale_inv = p.sim_scale_inv;
   k.gx = p.gravity[0];
   k.gy = p.gravity[1];
   k.gz = p.gravity[2];
   k.damping = p.damping;
   k.max_x = p.max_x;
   k.max_y = p.max_y;
   k.max_z = p.max_z;
   k.apply_gravity = p.apply_gravity;
   k.apply_walls = p.apply_walls;
   k.skip_point_mass = fast && p.central_mass == 0.0f && p.softening >= 1.0e-12f && std::isfinite(p.grav_const) ? 1 : 0;
   // (the softening bound: pair_math.h point_mass_nan)
   return k;
}

// The kernels' UNIT_SCALE instantiations: mSimulationScale = 1 (no multiplication by it) and - what
// lets the FULL-mode density sums drop the reference's "d > hscaled" test for pairs that passed
// d2 < h2 (pair_math.h: density_accumulate<INSIDE>) - a smoothing length whose constants agree:
// sqrtf(h2) <= hscaled.  Parameters that do not (a caller may set any) take the general
// instantiations, which multiply by a scale of 1.0: the same bits.
bool unit_scale(const sph_hip_params& p)
{
   return p.sim_scale == 1.0f && p.sim_scale_inv == 1.0f && sqrtf(p.h2) <= p.hscaled;
}

// ---- phase launches (no event recording, no host sync) ---------------------------------------

// ---- LDS tile capacity (the decisions: launch_policy.h) -------------------------------------
// The capacity levels of one tiled kernel: the runtime's occupancy calculator for registers and
// waves, the MI355X's LDS granule for the rest.
template <class Kernel>
TileLevels tile_levels(Kernel kernel, int bytes_per_entry)
{
   hipFuncAttributes attr;
   size_t static_lds = 2048;   // (no answer: the old slack)
   if (hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(kernel)) == hipSuccess)
      static_lds = attr.sharedSizeBytes;
   else
      (void)hipGetLastError();
   auto blocks_at = [&](int cap) {
      int nb = 0;
      const size_t bytes = (size_t)(cap + TILE_PAD) * bytes_per_entry;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, TILE_THREADS, bytes) != hipSuccess) {
         (void)hipGetLastError();
         return 0;
      }
      const size_t granules = (static_lds + bytes + LDS_GRANULE - 1) / LDS_GRANULE;
      const int by_lds = (int)(LDS_PER_CU / (granules * LDS_GRANULE));
      return nb < by_lds ? nb : by_lds;
   };
   const TileLevels t = search_levels(blocks_at, bytes_per_entry);
   if (getenv("SPH_HIP_DEBUG")) {
      fprintf(stderr, "sph_hip: tile capacity levels (%d B/entry):", bytes_per_entry);
      for (int l = 0; l < t.n; l++) fprintf(stderr, " %d (%d/CU)", t.cap[l], blocks_at(t.cap[l]));
      fprintf(stderr, "\n");
   }
   return t;
}

// the tiled kernels may ask for all of a CU's LDS as dynamic shared memory (set per context: the
// attribute belongs to the function on the current device)
void allow_large_tiles()
{
   const int most = 160 * 1024;
   for (int m = 0; m < 16; m++) {
      bind_flags([&](auto U, auto M, auto W, auto F) {
         (void)hipFuncSetAttribute((const void*)(k_full_density_tiled<U.value, M.value, W.value, F.value>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, most);
         (void)hipFuncSetAttribute((const void*)(k_full_density_chunked<U.value, M.value, W.value, F.value>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, most);
         if constexpr (M.value || !F.value)   // (FAST never gathers masses: only its M = true form exists)
            (void)hipFuncSetAttribute((const void*)(k_full_accel_lists<U.value, M.value, W.value, F.value>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, most);
      }, (m & 1) != 0, (m & 2) != 0, (m & 4) != 0, (m & 8) != 0);
   }
   (void)hipGetLastError();
}

// The density pass of an earlier step reported particles with more neighbours than their lists
// hold (those lanes walk their candidates one by one in both passes, an order of magnitude
// slower per particle): enlarge the lists for the steps from here on.  The device has
// to be idle for the exchange of the allocation - once or twice in a run that compresses.
// Never changes results, only which route a particle takes.
void grow_lists(sph_hip_context* ctx)
{
   // the largest capacity the device has room for, at once (a second reallocation later would be
   // a second stall); allocated while the device still works through the steps already enqueued
   DevBuf<uint32_t> bigger;
   int want = ctx->list_cap_max;
   while (want > ctx->list_cap) {
      const size_t words = ctx->list_blocks * list_rows(want) * TILE_THREADS;
      if (dev_alloc(bigger, words) == hipSuccess) break;
      (void)hipGetLastError();
      bigger.reset();
      want = smaller_list_cap(want);
   }
   if (!bigger || want <= ctx->list_cap) {
      ctx->list_cap_max = ctx->list_cap;   // no memory for it: stay, and do not ask again
      return;
   }
   if (hipStreamSynchronize(ctx->stream) != hipSuccess) return;   // (an error is reported by the step itself)
   ctx->nlist = std::move(bigger);
   ctx->list_cap = want;
   ctx->list_cap_max = want < ctx->list_cap_max ? want : ctx->list_cap_max;
   ((volatile int*)ctx->tile_feedback)[TSTAT_NO_LIST] = 0;
   static const bool debug = getenv("SPH_HIP_DEBUG") != nullptr;
   if (debug) fprintf(stderr, "sph_hip: neighbour lists enlarged to %d entries\n", want);
}

// Capacities for the step about to be launched (before its k_tile_desc, which lists the
// workgroups that will not fit them), from the feedback the device left in pinned memory.
void pick_tile_caps(sph_hip_context* ctx)
{
   TileCaps& caps = ctx->caps;
   if (ctx->list_cap < ctx->list_cap_max) {
      const volatile int* word = ctx->tile_feedback;
      if (lists_should_grow(word[TSTAT_NO_LIST], word[TSTAT_BLOCKS])) grow_lists(ctx);
   }
   if (caps.n_cand == 0) {
      allow_large_tiles();
      bind_flags([&](auto F) {
         ctx->density_levels = tile_levels(k_full_density_tiled<true, true, false, F.value>, DENSITY_TILE_BYTES);
         ctx->accel_levels = tile_levels(k_full_accel_lists<true, true, false, F.value>, ACCEL_TILE_BYTES);
      }, ctx->fast != 0);
      merge_candidates(ctx->density_levels, ctx->accel_levels, caps);
      // The arithmetic was switched (sph_hip_set_arithmetic): other kernels, possibly other levels.
      // The statistics the host holds were counted against the old candidate list: they stay valid
      // when the list is the same, and mean nothing otherwise.
      bool same = ctx->n_cand_kept == caps.n_cand;
      for (int c = 0; same && c < caps.n_cand; c++) same = ctx->cand_kept[c] == caps.cand[c];
      if (!same && ctx->n_cand_kept > 0 && ctx->tile_feedback) memset(ctx->tile_feedback, 0, TSTAT_COUNT * sizeof(int));
      ctx->n_cand_kept = caps.n_cand;
      for (int c = 0; c < caps.n_cand; c++) ctx->cand_kept[c] = caps.cand[c];
   }
   int fb[TSTAT_COUNT];
   for (int i = 0; i < TSTAT_COUNT; i++) fb[i] = ((volatile int*)ctx->tile_feedback)[i];
   choose_caps(caps, fb, ctx->density_levels, ctx->accel_levels, ctx->tile_cap_forced, ctx->tile_cap_accel,
               ctx->tile_cap_density);
   static int debug_left = getenv("SPH_HIP_DEBUG") ? 6 : 0;
   if (ctx->tile_cap_forced <= 0 && debug_left > 0 && debug_left--)
      fprintf(stderr, "sph_hip: %d workgroups, largest tile %d -> capacities %d / %d\n",
              fb[TSTAT_BLOCKS], fb[TSTAT_MAX], caps.cap_density, caps.cap_accel);
}

// ---- ports (port_kernels.h; the contract and the decisions: port_policy.h, launch_policy.h) ----------------
// the cell grid as port_policy.h takes it
PortGrid port_grid(const sph_hip_context* ctx)
{
   const CellGrid& g = ctx->grid;
   return {g.nx, g.ny, g.nz_global, g.inv, g.z0, g.nz};
}

// Waits for the steps enqueued so far and reads the device's counts: the host bound ctx->n becomes n_live and
// n_owned the owned count (the same number on a context that holds the whole grid).
int ports_tighten(sph_hip_context* ctx, int32_t* meta_out = nullptr)
{
   int32_t meta[META_COUNT];
   SPH_TRY(hipMemcpyAsync(meta, ctx->meta, sizeof(meta), hipMemcpyDeviceToHost, ctx->stream));
   SPH_TRY(hipStreamSynchronize(ctx->stream));
   ctx->n = meta[META_N_LIVE];
   ctx->n_owned = meta[META_OWN_END] - meta[META_OWN_BEGIN];
   if (meta_out) memcpy(meta_out, meta, sizeof(meta));
   return SPH_HIP_OK;
}

void launch_ports_kernel(sph_hip_context* ctx, int ns, const PortFiring& f, int bound)
{
   const int sink_blocks = bound > 0 ? div_up(bound, PORT_THREADS) : 1;
   hipLaunchKernelGGL(k_ports_apply, dim3(sink_blocks + div_up(f.m, PORT_THREADS)), dim3(PORT_THREADS), 0, ctx->stream,
                      ctx->posm[ctx->cur], ctx->velp[ctx->cur], ctx->meta, ctx->sink_dev, ns, ctx->emit_dev, f,
                      sink_blocks, ctx->capacity, ctx->removed_dev);
}

// After a port step's build meta[META_N_IN] is that build's input count, which dropped entries make larger
// than n_live: a build that no port launch precedes (a phase call, the sampler's, the first step after the
// ports were cleared) sets it right first - k_ports_apply with nothing to catch and nothing to append.
int launch_ports_reset(sph_hip_context* ctx)
{
   const PortFiring none = {};
   launch_ports_kernel(ctx, 0, none, 0);
   SPH_TRY(hipGetLastError());
   ctx->n_in_stale = 0;
   return SPH_HIP_OK;
}

// The firing table of the step about to be enqueued, and whether its layers fit - decided before anything of
// the step is enqueued.  The host bound first; where that does not settle it, the device's own count.
int ports_plan(sph_hip_context* ctx, PortFiring& f)
{
   f = port_plan(ctx->emit_host, ctx->n_emit, ctx->port_step, ctx->port_fired, ctx->next_id);
   if (f.m == 0) return SPH_HIP_OK;
   if (!port_ids_fit(ctx->next_id, f.m)) {
      ctx->err = "sph_hip_step: the emitters have used up the particle ids (the next layer would reach 0xffffffff)";
      return SPH_HIP_ERR_INVALID;
   }
   if (!ports_must_tighten(ctx->n, f.m, ctx->capacity)) return SPH_HIP_OK;
   int rc = ports_tighten(ctx);
   if (rc) return rc;
   if (ports_layer_fits(ctx->n, f.m, ctx->capacity)) return SPH_HIP_OK;
   ctx->err = "sph_hip_step: port step " + std::to_string(ctx->port_step) + " would emit " + std::to_string(f.m) +
              " particles on top of " + std::to_string(ctx->n) + " live ones, more than the context capacity " +
              std::to_string(ctx->capacity) + ": nothing of the step was enqueued";
   return SPH_HIP_ERR_CAPACITY;
}

// The step's port launch, in front of its cell build, and the host's side of it: the schedule, the ids, the
// emitted totals and the bound move on.
int launch_ports(sph_hip_context* ctx, const PortFiring& f)
{
   launch_ports_kernel(ctx, ctx->n_sink, f, ctx->n);
   SPH_TRY(hipGetLastError());
   for (int q = 0; q < f.n; q++) {
      const int e = f.emitter[q];
      ctx->port_fired[e]++;
      ctx->port_emitted[e] += port_points(ctx->emit_host[e]);
   }
   ctx->n += f.m;
   ctx->next_id += (uint32_t)f.m;
   ctx->port_step++;
   ctx->n_in_stale = 0;
   if (ctx->n_sink > 0) ctx->may_hold_dead = 1;   // the build that follows drops the caught entries
   if (ctx->n_sink > 0 || f.m > 0) ctx->ids_changed = 1;
   return SPH_HIP_OK;
}

// what the cell build has to know about the slab's neighbours
SlabZone slab_zone(const sph_hip_context* ctx)
{
   SlabZone z;
   z.lo = ctx->plane_lo;
   z.hi = ctx->plane_hi;
   z.halo = ctx->halo;
   z.have_left = ctx->plane_lo > 0;
   z.have_right = ctx->plane_hi < ctx->grid.nz_global;
   z.drop_ghosts = ctx->mode == SPH_HIP_MODE_FULL;
   z.early = ctx->early_exchange;
   return z;
}

// clear_left/right: message buffers whose record counters this build zeroes (early exchange)
int launch_cell_build(sph_hip_context* ctx, void* clear_left = nullptr, void* clear_right = nullptr,
                      bool keep_sums = false)
{
   if (ctx->n_in_stale) {
      int rc = launch_ports_reset(ctx);
      if (rc) return rc;
   }
   const int n = ctx->n;  // host upper bound of entries; the exact count is meta[META_N_IN]
   if (n == 0) return SPH_HIP_OK;
   const int blocks = div_up(n, 256);
   const CellGrid g = ctx->grid;
   hipStream_t st = ctx->stream;
   const int cur = ctx->cur;
   const SlabZone zone = slab_zone(ctx);
   if (ctx->prehashed == 2) {
      // a slab whose last step was integrated and hashed by its acceleration pass: only last
      // step's ghosts (to the trash cell) and the records received since are left
      ctx->prehashed = 0;
      hipLaunchKernelGGL(k_hash_tail, dim3(SLAB_PACK_BLOCKS), dim3(256), 0, st, ctx->posm[cur], ctx->meta, g,
                         ctx->key, ctx->slot, ctx->cell_count);
   } else if (ctx->prehashed) {
      ctx->prehashed = 0;   // the last integrate hashed and counted this very state already
   } else {
      const bool ref = ctx->mode == SPH_HIP_MODE_REF;
      bind_flags([&](auto R, auto D) {
         if constexpr (!(R.value && D.value))
            hipLaunchKernelGGL((k_hash_count<R.value, D.value>), dim3(blocks), dim3(256), 0, st, ctx->posm[cur],
                               ctx->velp[cur], ctx->meta, g, zone, ctx->key, ctx->slot, ctx->cell_count,
                               R.value ? ctx->vox.get() : nullptr);
      }, ref, !ref && ctx->may_hold_dead != 0);
   }
   ctx->early_exchange = 0;  // consumed: it described the step before this build
   ctx->may_hold_dead = 0;   // the build drops dead entries
   // the scan covers the real cells plus the trash cell, so cell_start[ncells] = live entries
   const int tiles = ctx->scan_tiles;
   const int ncells_scan = g.ncells + 1;
   hipLaunchKernelGGL(k_scan_reduce, dim3(tiles), dim3(SCAN_THREADS), 0, st, ctx->cell_count,
                      ncells_scan, ctx->scan_part);
   hipLaunchKernelGGL(k_scan_final, dim3(tiles), dim3(SCAN_THREADS), 0, st, ctx->cell_count,
                      ncells_scan, ctx->scan_part, ctx->cell_start, ctx->big_cells, (uint32_t)ctx->capacity,
                      ctx->meta);
   // sorted ranges: owned planes, density planes, owned planes next to a neighbouring slab
   const PlaneRanges r = plane_ranges(ctx->plane_lo, ctx->plane_hi, g.z0, g.nz, ctx->halo, zone.have_left,
                                      zone.have_right);
   hipLaunchKernelGGL(k_scatter, dim3(blocks), dim3(256), 0, st, ctx->key, ctx->slot,
                      ctx->cell_start, ctx->meta, ctx->perm, g.nx * g.ny, g.ncells, r.own_lo, r.own_hi,
                      r.sum_lo, r.sum_hi, r.bnd_lo, r.bnd_hi, ctx->tile_stats, (int32_t*)clear_left,
                      (int32_t*)clear_right, ctx->big_cells, (uint32_t)ctx->capacity);
   // crowded cells (listed by k_scatter; none in an ordinary scene: the workgroups then leave at
   // once) are ranked by sorting, behind the per-member scan that skips them; scratch = the
   // staging buffer, idle during a step
   uint32_t* scratch_key = reinterpret_cast<uint32_t*>(ctx->stage.get());
   uint32_t* scratch_src = scratch_key + ctx->capacity;
   // keep_sums (stand-alone voxelize of a FULL-mode context that holds the whole grid): note where
   // every entry goes (in `slot`, free once k_scatter has run) and move rho / acc / ncount along
   uint32_t* remap = (keep_sums && ctx->mode == SPH_HIP_MODE_FULL && !ctx->had_exchange) ? ctx->slot : nullptr;
   if (ctx->mode == SPH_HIP_MODE_REF) {
      hipLaunchKernelGGL(k_rank_order, dim3(blocks), dim3(256), 0, st, ctx->perm, ctx->key,
                         ctx->cell_start, ctx->meta, ctx->order);
      hipLaunchKernelGGL(k_rank_big<false>, dim3(RANK_BIG_BLOCKS), dim3(256), 0, st, ctx->big_cells,
                         ctx->perm, ctx->cell_start, (const float4*)nullptr, (const float4*)nullptr,
                         (float4*)nullptr, (float4*)nullptr, ctx->order, scratch_key, scratch_src,
                         (uint32_t*)nullptr);
   } else {
      const int nxt = cur ^ 1;
      if (ctx->use_tiled) {
         // + the LDS tile layout of every 256-particle workgroup of the density range, with the
         // statistics and give-up lists for the capacities chosen here for this step's sums
         static_assert(sizeof(TileDesc) == 20 * sizeof(int), "TileDesc is 20 ints");
         pick_tile_caps(ctx);
         const int ntiles = div_up(n, TILE_THREADS), desc_blocks = div_up(ntiles, 256);
         hipLaunchKernelGGL(k_rank_gather_tile_desc, dim3(desc_blocks + blocks), dim3(256), 0, st,
                            desc_blocks, ntiles, ctx->perm, ctx->key, ctx->cell_start, ctx->meta,
                            g, ctx->posm[cur], ctx->velp[cur], ctx->posm[nxt], ctx->velp[nxt],
                            ctx->tile_desc, ctx->caps, ctx->tile_stats, ctx->giveup_density,
                            ctx->giveup_accel, remap);
      } else {
         hipLaunchKernelGGL(k_rank_gather, dim3(blocks), dim3(256), 0, st, ctx->perm, ctx->key,
                            ctx->cell_start, ctx->meta, g.ncells, ctx->posm[cur], ctx->velp[cur],
                            ctx->posm[nxt], ctx->velp[nxt], remap);
      }
      hipLaunchKernelGGL(k_rank_big<true>, dim3(RANK_BIG_BLOCKS), dim3(256), 0, st, ctx->big_cells,
                         ctx->perm, ctx->cell_start, ctx->posm[cur], ctx->velp[cur], ctx->posm[nxt],
                         ctx->velp[nxt], (uint32_t*)nullptr, scratch_key, scratch_src, remap);
      if (remap) {
         ctx->terms.valid = 0;   // velB / auxc stay where they were: formed again if an acceleration pass follows
         // a build that is not followed by the sums: their last results move with the particles
         // (temporaries in the staging buffer behind k_rank_big's scratch; the float4 part 16-byte aligned)
         float4* acc_t = reinterpret_cast<float4*>(ctx->stage.get() + ((2 * (size_t)ctx->capacity + 3) & ~(size_t)3));
         float* rho_t = reinterpret_cast<float*>(acc_t + (size_t)ctx->capacity);
         int32_t* cnt_t = reinterpret_cast<int32_t*>(rho_t + (size_t)ctx->capacity);
         hipLaunchKernelGGL(k_permute_sums, dim3(blocks), dim3(256), 0, st, remap, ctx->key, ctx->meta,
                            (uint32_t)g.ncells, ctx->rho, ctx->acc, ctx->ncount, rho_t, acc_t, cnt_t);
         SPH_TRY(hipMemcpyAsync(ctx->rho, rho_t, sizeof(float) * n, hipMemcpyDeviceToDevice, st));
         SPH_TRY(hipMemcpyAsync(ctx->acc, acc_t, sizeof(float4) * n, hipMemcpyDeviceToDevice, st));
         SPH_TRY(hipMemcpyAsync(ctx->ncount, cnt_t, sizeof(int32_t) * n, hipMemcpyDeviceToDevice, st));
      }
      ctx->cur = nxt;
      // The live set is now compacted at the front of the new buffers.  meta[N_IN] still holds
      // this build's input count: without an exchange nothing was dropped (n_live == n_in), and
      // with one, sph_hip_slab_unpack resets it to n_live before appending.
   }
   SPH_TRY(hipGetLastError());
   return SPH_HIP_OK;
}

int launch_find_neighbors(sph_hip_context* ctx)
{
   if (ctx->mode != SPH_HIP_MODE_REF || ctx->n == 0) return SPH_HIP_OK;
   const sph_hip_params& p = ctx->prm;
   hipLaunchKernelGGL(k_ref_find_neighbors, dim3(div_up(ctx->n, 256)), dim3(256), 0, ctx->stream,
                      ctx->posm[0], ctx->vox, ctx->cell_start, ctx->order, ctx->n, p.cells_x,
                      p.cells_y, p.cells_z, p.h, p.htimes2, p.h2, p.sim_scale, p.examine_count,
                      ctx->nb, ctx->nd, ctx->ncount);
   SPH_TRY(hipGetLastError());
   return SPH_HIP_OK;
}

// message buffers of a slab whose acceleration pass does the rest of the step (FusedStep.slab)
struct SlabFused {
   void* left;
   void* right;
   int capacity;
};

// tiled kernels of the two sums, specialised on (unit simulation scale, uniform mass)
void launch_density_tiled(sph_hip_context* ctx, bool unit, int blocks, const PairConsts& k)
{
   const int cap = ctx->caps.cap_density;
   const size_t lds = (size_t)(cap + TILE_PAD) * DENSITY_TILE_BYTES;
   // (a slab: the fused acceleration pass writes energy partials only for workgroups that own
   // particles; this launch zeroes the others' - same grid, one pair per workgroup)
   const bool whole = ctx->plane_lo == 0 && ctx->plane_hi == ctx->grid.nz_global;
   double* epart_clear = whole ? nullptr : ctx->epart + 2;
   // Many workgroups whose tile fits no capacity (a scene several times denser than the
   // benchmark's): a launch of its own stages their candidates through LDS piece by piece and
   // writes their lists (k_full_density_chunked) instead of the tiled kernel's first workgroups
   // walking them untiled.  Decided from what the last step reported; both kernels read the same
   // device-side list, the flag only says who works it off.
   const int reported = ((volatile int*)ctx->tile_feedback)[TSTAT_GIVEUP_DENSITY];
   const bool chunked = ctx->chunked_giveups == 1 || (ctx->chunked_giveups < 0 && reported >= 32);
   // The two kernels work on disjoint workgroups: the chunked one runs beside the tiled one on a
   // stream of its own (forked here, joined before anything else is enqueued) - alone it would
   // leave the device to ~1 000 long workgroups while the other 15 000 wait.
   hipStream_t side = ctx->stream;
   if (chunked) {
      if (!ctx->chunk_stream) {
         if (hipStreamCreateWithFlags(ctx->chunk_stream.out(), hipStreamNonBlocking) != hipSuccess ||
             event_create(ctx->ev_chunk_fork) != hipSuccess || event_create(ctx->ev_chunk_join) != hipSuccess) {
            (void)hipGetLastError();
            ctx->chunk_stream.reset();
         }
      }
      if (ctx->chunk_stream && hipEventRecord(ctx->ev_chunk_fork, ctx->stream) == hipSuccess &&
          hipStreamWaitEvent(ctx->chunk_stream, ctx->ev_chunk_fork, 0) == hipSuccess)
         side = ctx->chunk_stream;
   }
   bind_flags([&](auto U, auto M, auto W, auto F) {
      if (chunked)
         hipLaunchKernelGGL((k_full_density_chunked<U.value, M.value, W.value, F.value>), dim3(1024),
                            dim3(TILE_THREADS), lds, side, ctx->posm[ctx->cur], ctx->velp[ctx->cur],
                            ctx->cell_start, ctx->meta, ctx->grid, k, ctx->rho, ctx->velB, ctx->auxc,
                            ctx->ncount, ctx->tile_desc, ctx->nlist, ctx->nlist_overflow, cap,
                            ctx->tile_stats, ctx->giveup_density, ctx->list_cap);
      hipLaunchKernelGGL((k_full_density_tiled<U.value, M.value, W.value, F.value>), dim3(blocks),
                         dim3(TILE_THREADS), lds, ctx->stream, ctx->posm[ctx->cur], ctx->velp[ctx->cur],
                         ctx->cell_start, ctx->meta, ctx->grid, k, ctx->rho, ctx->velB, ctx->auxc,
                         ctx->ncount, ctx->tile_desc, ctx->nlist, ctx->nlist_overflow, cap,
                         ctx->tile_stats, ctx->giveup_density, ctx->tile_feedback, ctx->list_cap,
                         epart_clear, chunked ? 0 : 1);
   }, unit, ctx->uniform_mass != 0, ctx->caps.wide != 0, ctx->fast != 0);
   if (side != ctx->stream) {
      // (a failure here would leave the streams unordered: drain the side stream the hard way)
      if (hipEventRecord(ctx->ev_chunk_join, side) != hipSuccess ||
          hipStreamWaitEvent(ctx->stream, ctx->ev_chunk_join, 0) != hipSuccess) {
         (void)hipGetLastError();
         (void)hipStreamSynchronize(side);
      }
   }
}

void launch_accel_lists(sph_hip_context* ctx, bool unit, int blocks, const PairConsts& k, int part,
                        hipStream_t st, bool fused = false, const SlabFused* slab = nullptr)
{
   FusedStep fs;
   memset(&fs, 0, sizeof(fs));
   if (fused) {
      fs.on = 1;
      fs.velp_in = ctx->velp[ctx->cur];
      fs.posm_out = ctx->posm[ctx->cur ^ 1];
      fs.velp_out = ctx->velp[ctx->cur ^ 1];
      fs.epart = ctx->epart + 2;
      fs.key = ctx->key;
      fs.slot = ctx->slot;
      fs.cell_count = ctx->cell_count;
      if (slab) {
         fs.slab = 1;
         fs.zone = slab_zone(ctx);
         fs.left = (SlabMsg*)slab->left;
         fs.right = (SlabMsg*)slab->right;
         fs.msg_capacity = slab->capacity;
         fs.meta = ctx->meta;
      }
   }
   const int cap = ctx->caps.cap_accel;
   const size_t lds = (size_t)(cap + TILE_PAD) * ACCEL_TILE_BYTES;
   // (a FAST context's density pass folds the mass into B: its acceleration pass never gathers masses)
   bind_flags([&](auto U, auto M, auto W, auto F) {
      if constexpr (M.value || !F.value)
      hipLaunchKernelGGL((k_full_accel_lists<U.value, M.value, W.value, F.value>), dim3(blocks),
                         dim3(TILE_THREADS), lds, st, ctx->posm[ctx->cur], ctx->velB, ctx->rho, ctx->auxc,
                         ctx->ncount, ctx->cell_start, ctx->meta, ctx->grid, k, ctx->acc, ctx->tile_desc,
                         ctx->nlist, ctx->nlist_overflow, cap, ctx->tile_stats, ctx->giveup_accel, part,
                         ctx->list_cap, ctx->tile_feedback, fs, ctx->caps.cap_density);
   }, unit, ctx->uniform_mass != 0 || ctx->fast != 0, ctx->caps.wide != 0, ctx->fast != 0);
}

// FULL mode: the constants the j-only factors in velB / auxc were formed with (density pass)
void note_neighbor_terms(sph_hip_context* ctx, const PairConsts& k)
{
   ctx->terms.valid = 1;
   ctx->terms.fast = ctx->fast;
   ctx->terms.rho0 = k.rho0;
   ctx->terms.stiffness = k.stiffness;
   ctx->terms.kernel3 = k.kernel3;
}

// Before an acceleration pass: the reference forms p_j / rho_j^2 and rho_j^-1 m_j k3 inside
// computeAcceleration, with the constants of that call.  A density pass formed them here; if rho0,
// stiffness, kernel3 or the arithmetic (which decides the layout) have been set since, or the
// particles were moved by a stand-alone cell build, they are formed again from the density pass's
// rho.  Never within sph_hip_step: its density and acceleration passes share one set of constants.
void refresh_neighbor_terms(sph_hip_context* ctx, const PairConsts& k)
{
   const bool same = ctx->terms.valid && ctx->terms.fast == ctx->fast &&
                     memcmp(&ctx->terms.rho0, &k.rho0, sizeof(float)) == 0 &&
                     memcmp(&ctx->terms.stiffness, &k.stiffness, sizeof(float)) == 0 &&
                     memcmp(&ctx->terms.kernel3, &k.kernel3, sizeof(float)) == 0;
   if (same) return;
   bind_flags([&](auto F) {
      hipLaunchKernelGGL((k_neighbor_terms<F.value>), dim3(div_up(ctx->n, 256)), dim3(256), 0, ctx->stream,
                         ctx->posm[ctx->cur], ctx->velp[ctx->cur], ctx->rho, ctx->meta, k, ctx->velB,
                         ctx->auxc);
   }, ctx->fast != 0);
   note_neighbor_terms(ctx, k);
}

int launch_density(sph_hip_context* ctx)
{
   const int n = ctx->n;
   if (n == 0) return SPH_HIP_OK;
   const PairConsts k = pair_consts(ctx->prm, ctx->fast != 0);
   const int blocks = div_up(n, 256);
   if (ctx->mode == SPH_HIP_MODE_REF) {
      hipLaunchKernelGGL(k_ref_density, dim3(blocks), dim3(256), 0, ctx->stream, ctx->posm[0],
                         ctx->nb, ctx->nd, ctx->ncount, n, ctx->prm.examine_count, k, ctx->rho);
   } else {
      const bool unit = unit_scale(ctx->prm);
      if (ctx->use_tiled) {
         launch_density_tiled(ctx, unit, div_up(n, TILE_THREADS), k);  // give-up workgroups fall back inline
      } else {                                         // SPH_HIP_UNTILED=1: untiled everywhere
         bind_flags([&](auto U, auto F) {
            hipLaunchKernelGGL((k_full_density<U.value, F.value>), dim3(blocks), dim3(256), 0, ctx->stream,
                               ctx->posm[ctx->cur], ctx->cell_start, ctx->velp[ctx->cur], ctx->meta,
                               ctx->grid, k, ctx->rho, ctx->velB, ctx->auxc, ctx->ncount);
         }, unit, ctx->fast != 0);
      }
      note_neighbor_terms(ctx, k);
   }
   SPH_TRY(hipGetLastError());
   return SPH_HIP_OK;
}

// part: 0 = all workgroups; 1 / 2 = those with / without particles of the owned planes next to
// a neighbouring slab (early exchange; tiled FULL mode only)
int launch_accel(sph_hip_context* ctx, int part = 0, hipStream_t part_stream = nullptr, bool fused = false,
                 const SlabFused* slab = nullptr)
{
   const int n = ctx->n;
   if (n == 0) return SPH_HIP_OK;
   const PairConsts k = pair_consts(ctx->prm, ctx->fast != 0);
   const int blocks = div_up(n, 256);
   if (ctx->mode == SPH_HIP_MODE_REF) {
      hipLaunchKernelGGL(k_ref_accel, dim3(blocks), dim3(256), 0, ctx->stream, ctx->posm[0],
                         ctx->velp[0], ctx->rho, ctx->nb, ctx->nd, ctx->ncount, n,
                         ctx->prm.examine_count, k, ctx->acc);
   } else {
      refresh_neighbor_terms(ctx, k);
      const bool unit = unit_scale(ctx->prm);
      if (ctx->use_tiled) {
         // same tiling (and tile descriptors) as the density pass of this step
         launch_accel_lists(ctx, unit, div_up(n, TILE_THREADS), k, part, part ? part_stream : ctx->stream, fused, slab);
      } else {
         bind_flags([&](auto U, auto F) {
            hipLaunchKernelGGL((k_full_accel<U.value, F.value>), dim3(blocks), dim3(256), 0, ctx->stream,
                               ctx->posm[ctx->cur], ctx->velB, ctx->rho, ctx->auxc, ctx->cell_start,
                               ctx->meta, ctx->grid, k, ctx->acc, ctx->ncount);
         }, unit, ctx->fast != 0);
      }
   }
   SPH_TRY(hipGetLastError());
   return SPH_HIP_OK;
}

// `n` entries of `list` into `dev` through the pinned `stage`.  The staging is memory the previous
// call's copy may still be reading: wait for that copy (not for the steps queued before it), then copy
// behind everything enqueued so far.
template <class T>
int stage_list(sph_hip_context* ctx, const T* list, int n, PinnedBuf<T>& stage, DevBuf<T>& dev, Event& copied,
               int& pending)
{
   if (pending) SPH_TRY(hipEventSynchronize(copied));
   pending = 0;
   memcpy(stage.get(), list, sizeof(T) * (size_t)n);
   SPH_TRY(hipMemcpyAsync(dev, stage.get(), sizeof(T) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
   SPH_TRY(hipEventRecord(copied, ctx->stream));
   pending = 1;
   return SPH_HIP_OK;
}

// The motion clock of the step being enqueued (obstacle_policy.h: moving obstacles): tau at its start
// and at its end, the clock left at the end.  Host values only: they travel as kernel arguments.
void motion_tick(sph_hip_context* ctx, float tau[2])
{
   tau[0] = ctx->motion_tau;
   tau[1] = obstacle_clock_next(ctx->motion_tau, ctx->prm.time_step);
   ctx->motion_tau = tau[1];
}

// with_hash: the kernel also does the first step of the next cell build (see k_integrate);
// with static obstacles, k_integrate_obst; while a load recording has rows left, k_integrate_loads
// into the next row (an integrate without particles uses its row up too: the rows of the slabs of
// one run stay in step); while some obstacle moves, their _moving forms with the step's motion clock,
// which a slab's early pack has already taken (an integrate without particles advances it too); while
// some obstacle is a free body, k_bodies_advance and k_integrate_bodies (with zero particles the advance alone);
// while some obstacle has a motion path, k_paths_eval and the _path forms (with zero particles the eval alone)
int launch_integrate(sph_hip_context* ctx, bool with_hash = false)
{
   const int n = ctx->n;
   unsigned long long* load_row = nullptr;
   if (loads_pending(ctx)) load_row = ctx->loads_dev.get() + (size_t)ctx->loads_next++ * LOAD_ROW_WORDS;
   const bool moving = use_moving_kernels(ctx->n_obst, ctx->n_moving);
   const bool paths = use_path_kernels(ctx->n_obst, ctx->n_paths);
   if (path_clock_runs(ctx->n_obst, ctx->n_moving, ctx->n_paths) && !ctx->step_tau_taken) motion_tick(ctx, ctx->step_tau);
   ctx->step_tau_taken = 0;
   const float tau0 = ctx->step_tau[0], tau1 = ctx->step_tau[1];
   // motion paths: this step's shifts, behind the previous step's integrate on the stream
   if (paths) {
      hipLaunchKernelGGL(k_paths_eval, dim3(1), dim3(SPH_WAVE), 0, ctx->stream, ctx->paths_dev, ctx->path_keys_dev,
                         ctx->n_obst, tau0, tau1, ctx->path_shift_dev);
      if (n == 0) SPH_TRY(hipGetLastError());
   }
   // free bodies: the advance from the row the last integrate filled, then an integrate that always
   // records - into the caller's row, or into the internal row the advance has just zeroed
   const bool bodies = use_body_kernels(ctx->n_obst, ctx->n_bodies);
   if (bodies) {
      unsigned long long* clear = nullptr;
      if (!load_row) {
         ctx->body_flip ^= 1;
         load_row = clear = ctx->body_rows.get() + (size_t)ctx->body_flip * LOAD_ROW_WORDS;
      }
      hipLaunchKernelGGL(k_bodies_advance, dim3(1), dim3(SPH_WAVE), 0, ctx->stream, ctx->bodies_dev, ctx->body_state_dev,
                         ctx->n_obst, ctx->body_last_row, ctx->body_quantum, ctx->prm.time_step, clear);
      ctx->body_last_row = load_row;
      if (n == 0) SPH_TRY(hipGetLastError());
   }
   if (n == 0) return SPH_HIP_OK;
   const PairConsts k = pair_consts(ctx->prm, ctx->fast != 0);
   const int blocks = div_up(n, RED_THREADS);
   const sph_hip_obstacle_motion* motion_or_null = ctx->n_motion > 0 ? ctx->motion_dev.get() : nullptr;
   bind_flags([&](auto U, auto H) {
      if (paths && load_row)
         hipLaunchKernelGGL((k_integrate_loads_path<U.value, H.value>), dim3(blocks), dim3(RED_THREADS), 0, ctx->stream,
                            ctx->posm[ctx->cur], ctx->velp[ctx->cur], ctx->acc, ctx->meta, k, ctx->epart + 2,
                            ctx->grid, ctx->key, ctx->slot, ctx->cell_count, ctx->obst_dev, ctx->n_obst,
                            load_row, ctx->loads_quantum, motion_or_null, tau0, tau1, ctx->path_shift_dev);
      else if (paths)
         hipLaunchKernelGGL((k_integrate_obst_path<U.value, H.value>), dim3(blocks), dim3(RED_THREADS), 0, ctx->stream,
                            ctx->posm[ctx->cur], ctx->velp[ctx->cur], ctx->acc, ctx->meta, k, ctx->epart + 2,
                            ctx->grid, ctx->key, ctx->slot, ctx->cell_count, ctx->obst_dev, ctx->n_obst,
                            motion_or_null, tau0, tau1, ctx->path_shift_dev);
      else if (bodies)
         hipLaunchKernelGGL((k_integrate_bodies<U.value, H.value>), dim3(blocks), dim3(RED_THREADS), 0, ctx->stream,
                            ctx->posm[ctx->cur], ctx->velp[ctx->cur], ctx->acc, ctx->meta, k, ctx->epart + 2,
                            ctx->grid, ctx->key, ctx->slot, ctx->cell_count, ctx->obst_dev, ctx->n_obst,
                            load_row, ctx->body_quantum, ctx->n_motion > 0 ? ctx->motion_dev.get() : nullptr, tau0, tau1,
                            ctx->bodies_dev, ctx->body_state_dev);
      else if (moving && load_row)
         hipLaunchKernelGGL((k_integrate_loads_moving<U.value, H.value>), dim3(blocks), dim3(RED_THREADS), 0, ctx->stream,
                            ctx->posm[ctx->cur], ctx->velp[ctx->cur], ctx->acc, ctx->meta, k, ctx->epart + 2,
                            ctx->grid, ctx->key, ctx->slot, ctx->cell_count, ctx->obst_dev, ctx->n_obst,
                            load_row, ctx->loads_quantum, ctx->motion_dev, tau0, tau1);
      else if (moving)
         hipLaunchKernelGGL((k_integrate_obst_moving<U.value, H.value>), dim3(blocks), dim3(RED_THREADS), 0, ctx->stream,
                            ctx->posm[ctx->cur], ctx->velp[ctx->cur], ctx->acc, ctx->meta, k, ctx->epart + 2,
                            ctx->grid, ctx->key, ctx->slot, ctx->cell_count, ctx->obst_dev, ctx->n_obst,
                            ctx->motion_dev, tau0, tau1);
      else if (load_row)
         hipLaunchKernelGGL((k_integrate_loads<U.value, H.value>), dim3(blocks), dim3(RED_THREADS), 0, ctx->stream,
                            ctx->posm[ctx->cur], ctx->velp[ctx->cur], ctx->acc, ctx->meta, k, ctx->epart + 2,
                            ctx->grid, ctx->key, ctx->slot, ctx->cell_count, ctx->obst_dev, ctx->n_obst,
                            load_row, ctx->loads_quantum);
      else if (ctx->n_obst > 0)
         hipLaunchKernelGGL((k_integrate_obst<U.value, H.value>), dim3(blocks), dim3(RED_THREADS), 0, ctx->stream,
                            ctx->posm[ctx->cur], ctx->velp[ctx->cur], ctx->acc, ctx->meta, k, ctx->epart + 2,
                            ctx->grid, ctx->key, ctx->slot, ctx->cell_count, ctx->obst_dev, ctx->n_obst);
      else
         hipLaunchKernelGGL((k_integrate<U.value, H.value>), dim3(blocks), dim3(RED_THREADS), 0, ctx->stream,
                            ctx->posm[ctx->cur], ctx->velp[ctx->cur], ctx->acc, ctx->meta, k, ctx->epart + 2,
                            ctx->grid, ctx->key, ctx->slot, ctx->cell_count);
   }, unit_scale(ctx->prm), with_hash);
   ctx->energy_blocks = blocks;  // totals are formed on demand (sph_hip_get_energy)
   ctx->prehashed = with_hash ? 1 : 0;
   SPH_TRY(hipGetLastError());
   return SPH_HIP_OK;
}

// ---- tracers (tracer_kernels.h; decisions: tracer_policy.h) -------------------------------------------
// the counting sort of the slots by cell, into the other pair of arrays
int launch_tracer_sort(sph_hip_context* ctx)
{
   const int n = ctx->n_tracers, blocks = div_up(n, 256), cur = ctx->tr_cur;
   const CellGrid g = ctx->grid;
   hipStream_t st = ctx->stream;
   SPH_TRY(hipMemsetAsync(ctx->tr_cells, 0, ((size_t)ctx->scan_tiles * SCAN_TILE + 16) * sizeof(uint32_t), st));
   hipLaunchKernelGGL(k_tracer_hash, dim3(blocks), dim3(256), 0, st, ctx->tr_xi[cur], n, g, ctx->tr_cells,
                      ctx->tr_key, ctx->tr_rank);
   hipLaunchKernelGGL(k_scan_reduce, dim3(ctx->scan_tiles), dim3(SCAN_THREADS), 0, st, ctx->tr_cells, g.ncells,
                      ctx->tr_part);
   hipLaunchKernelGGL(k_tracer_scan, dim3(ctx->scan_tiles), dim3(SCAN_THREADS), 0, st, ctx->tr_cells, g.ncells,
                      ctx->tr_part);
   hipLaunchKernelGGL(k_tracer_scatter, dim3(blocks), dim3(256), 0, st, ctx->tr_xi[cur], ctx->tr_cnt[cur], n,
                      ctx->tr_key, ctx->tr_rank, ctx->tr_cells, ctx->tr_xi[cur ^ 1], ctx->tr_cnt[cur ^ 1]);
   SPH_TRY(hipGetLastError());
   ctx->tr_cur = cur ^ 1;
   ctx->tr_since_sort = 0;
   return SPH_HIP_OK;
}

// One advance of every tracer in the sorted state the cell build has just produced (posm / velp of
// ctx->cur, cell_start), with the time step in force; the row of a recording it fills travels as a kernel
// argument.  Nothing here synchronises.
int launch_tracers(sph_hip_context* ctx)
{
   const int n = ctx->n_tracers;
   if (n == 0) return SPH_HIP_OK;
   if (tracer_sort_due(n, ctx->tracer_sort_switch, ctx->tr_since_sort)) {
      int rc = launch_tracer_sort(ctx);
      if (rc) return rc;
   }
   ctx->tr_since_sort++;
   float* row = nullptr;
   if (ctx->trec_rows > 0) {
      const int r = tracer_record_row(++ctx->trec_step, ctx->trec_every, ctx->trec_rows);
      if (r >= 0) {
         row = ctx->trec_dev.get() + (size_t)r * 3 * (size_t)n;
         ctx->trec_filled = r + 1;
      }
   }
   const sph_hip_params& p = ctx->prm;
   const float pos_dt = p.time_step * p.sim_scale_inv;   // the integrate's displacement step (common_kernels.h)
   const TracerStep ts = {pos_dt, p.apply_walls, {p.max_x, p.max_y, p.max_z}, ctx->n > 0 ? 1 : 0};
   const PairConsts k = pair_consts(p, ctx->fast != 0);
   bind_flags([&](auto U) {
      hipLaunchKernelGGL((k_tracers_advance<U.value>), dim3(div_up(n, 256)), dim3(256), 0, ctx->stream,
                         ctx->tr_xi[ctx->tr_cur], ctx->tr_cnt[ctx->tr_cur], n, ctx->posm[ctx->cur], ctx->velp[ctx->cur],
                         ctx->cell_start, ctx->grid, k, ts, row);
   }, unit_scale(p));
   SPH_TRY(hipGetLastError());
   return SPH_HIP_OK;
}

// ---- gauges (gauge_kernels.h; decisions: gauge_policy.h) -------------------------------------------------
// Every gauge of a field kind evaluated once in the sorted state a cell build has just produced, into `row`
// (one reading per gauge; the entries of the pressure kinds are launch_gauges_pressure_into's, and a set
// without a field kind launches nothing here).  Nothing here synchronises.
int launch_gauges_into(sph_hip_context* ctx, sph_hip_gauge_reading* row)
{
   const int n = ctx->n_gauges;
   if (!gauges_launch_field(ctx->n_gauges_field)) return SPH_HIP_OK;
   const sph_hip_params& p = ctx->prm;
   const PairConsts k = pair_consts(p, ctx->fast != 0);
   bind_flags([&](auto U) {
      hipLaunchKernelGGL((k_gauges_read<U.value>), dim3(div_up(n, GAUGES_PER_BLOCK)), dim3(256), 0, ctx->stream,
                         ctx->gauges_dev, n, ctx->posm[ctx->cur], ctx->velp[ctx->cur], ctx->cell_start, ctx->grid, k,
                         ctx->n > 0 ? 1 : 0, row);
   }, unit_scale(p));
   SPH_TRY(hipGetLastError());
   return SPH_HIP_OK;
}

// The densities of the current sorted state into the context's own buffer (allocated here at the first
// use): behind a cell build, outside a step.  Writes nothing else.
int launch_particle_density(sph_hip_context* ctx)
{
   const int n = ctx->n;
   if (n == 0) return SPH_HIP_OK;
   if (!ctx->rho_own) {
      if (dev_alloc(ctx->rho_own, (size_t)ctx->capacity) != hipSuccess) {
         (void)hipGetLastError();
         ctx->err = "pressure readings: cannot allocate the density buffer of " + std::to_string(ctx->capacity) + " particles";
         return SPH_HIP_ERR_CAPACITY;
      }
   }
   const PairConsts k = pair_consts(ctx->prm, ctx->fast != 0);
   bind_flags([&](auto U) {
      hipLaunchKernelGGL((k_particle_density<U.value>), dim3(div_up(n, 256)), dim3(256), 0, ctx->stream,
                         ctx->posm[ctx->cur], ctx->cell_start, ctx->meta, ctx->grid, k, ctx->rho_own);
   }, unit_scale(ctx->prm));
   SPH_TRY(hipGetLastError());
   return SPH_HIP_OK;
}

// ---- velocity gradients (velgrad_kernels.h; contract: velgrad_policy.h) ----------------------------------------
// The two rows of every sorted slot of the current sorted state into the context's own arrays (allocated here at
// the first use): behind a cell build, outside a step.  The constants travel by value.  Writes nothing else, and
// nothing synchronises.
int launch_velgrad(sph_hip_context* ctx)
{
   const int n = ctx->n;
   if (n == 0) return SPH_HIP_OK;
   if (!ctx->velgrad_A || !ctx->velgrad_B) {
      DevBuf<float4> a, b;
      if (dev_alloc(a, (size_t)ctx->capacity) != hipSuccess || dev_alloc(b, (size_t)ctx->capacity) != hipSuccess) {
         (void)hipGetLastError();
         ctx->err = "velocity gradients: cannot allocate the rows of " + std::to_string(ctx->capacity) + " particles";
         return SPH_HIP_ERR_CAPACITY;
      }
      ctx->velgrad_A = std::move(a);
      ctx->velgrad_B = std::move(b);
   }
   const PairConsts k = pair_consts(ctx->prm, ctx->fast != 0);
   static_assert(TILE_THREADS == 256, "the velocity-gradient kernel maps one workgroup to 256 sorted particles");
   bind_flags([&](auto U) {
      hipLaunchKernelGGL((k_velgrad_particles<U.value>), dim3(div_up(n, TILE_THREADS)), dim3(TILE_THREADS), 0, ctx->stream,
                         ctx->posm[ctx->cur], ctx->velp[ctx->cur], ctx->cell_start, ctx->meta, ctx->grid, k,
                         ctx->velgrad_A.get(), ctx->velgrad_B.get());
   }, unit_scale(ctx->prm));
   SPH_TRY(hipGetLastError());
   return SPH_HIP_OK;
}

// The pressure kinds: k_gauges_pressure into `row`, with the particle densities of `source`
// (launch_policy.h: gauge_density_source).  A set without a pressure kind launches nothing.
int launch_gauges_pressure_into(sph_hip_context* ctx, sph_hip_gauge_reading* row, int source)
{
   const int n = ctx->n_gauges;
   if (!gauges_launch_pressure(ctx->n_gauges_pressure)) return SPH_HIP_OK;
   if (source == GAUGE_DENSITY_OWN) {
      int rc = launch_particle_density(ctx);
      if (rc) return rc;
   }
   const float* prho = source == GAUGE_DENSITY_OF_STEP ? ctx->rho.get() : ctx->rho_own.get();
   const sph_hip_params& p = ctx->prm;
   const PairConsts k = pair_consts(p, ctx->fast != 0);
   bind_flags([&](auto U) {
      hipLaunchKernelGGL((k_gauges_pressure<U.value>), dim3(div_up(n, GAUGES_PER_BLOCK)), dim3(256), 0, ctx->stream,
                         ctx->gauges_dev, n, ctx->posm[ctx->cur], prho, ctx->cell_start, ctx->grid, k,
                         ctx->n > 0 ? 1 : 0, row);
   }, unit_scale(p));
   SPH_TRY(hipGetLastError());
   return SPH_HIP_OK;
}

// One step of a gauge recording: the step is counted, and where it fills a row the field kinds are read into
// it; the row is remembered for the pressure kinds (launch_gauges_pressure).
int launch_gauges(sph_hip_context* ctx)
{
   ctx->grec_row_now = -1;
   if (ctx->grec_rows == 0) return SPH_HIP_OK;
   const int r = gauge_record_row(++ctx->grec_step, ctx->grec_every, ctx->grec_rows);
   if (r < 0) return SPH_HIP_OK;
   ctx->grec_row_now = r;
   ctx->grec_filled = r + 1;
   return launch_gauges_into(ctx, ctx->grec_dev.get() + (size_t)r * (size_t)ctx->n_gauges);
}

// The pressure kinds of the row launch_gauges has just opened, if any: behind the step's density pass
// (GAUGE_DENSITY_OF_STEP) or, in the stand-alone integrate, with the context's own densities.
int launch_gauges_pressure(sph_hip_context* ctx, int source)
{
   const int r = ctx->grec_row_now;
   ctx->grec_row_now = -1;
   if (!step_reads_pressure(r, ctx->n_gauges_pressure)) return SPH_HIP_OK;
   return launch_gauges_pressure_into(ctx, ctx->grec_dev.get() + (size_t)r * (size_t)ctx->n_gauges, source);
}

// ---- carried scalars (scalar_kernels.h; contract: scalar_policy.h; routes: launch_policy.h) ---------------
// the constants, diffusivities and sources of the pass about to be enqueued: by value in its arguments, so a
// later setter does not reach the steps already queued
ScalarStep scalar_step_of(const sph_hip_context* ctx, const PairConsts& k)
{
   ScalarStep st = {};
   st.hscaled = k.hscaled;
   st.kernel3 = k.kernel3;
   st.sim_scale = k.sim_scale;
   st.dt = k.dt;
   for (int c = 0; c < SPH_HIP_SCALAR_CHANNELS; c++) st.kappa[c] = ctx->scalar_kappa[c];
   st.n_sources = ctx->n_scalar_sources;
   for (int q = 0; q < ctx->n_scalar_sources; q++) st.sources[q] = ctx->scalar_sources[q];
   return st;
}

// Ts (and, with_volumes, Vs from the step's densities) of the current sorted state
int launch_scalars_stage(sph_hip_context* ctx, bool with_volumes)
{
   hipLaunchKernelGGL(k_scalars_stage, dim3(div_up(ctx->n, 256)), dim3(256), 0, ctx->stream, ctx->posm[ctx->cur],
                      ctx->velp[ctx->cur], with_volumes ? ctx->rho.get() : (const float*)nullptr, ctx->meta,
                      ctx->scalar_T, ctx->n_scalars, ctx->scalar_Ts, with_volumes ? ctx->scalar_Vs.get() : (float*)nullptr);
   SPH_TRY(hipGetLastError());
   return SPH_HIP_OK;
}

// One step of the scalars, behind the step's density pass: the stage, then the pass.  Nothing synchronises.
int launch_scalars(sph_hip_context* ctx)
{
   if (!step_launches_scalars(ctx->n_scalars, ctx->n)) return SPH_HIP_OK;
   int rc = launch_scalars_stage(ctx, true);
   if (rc) return rc;
   const PairConsts k = pair_consts(ctx->prm, ctx->fast != 0);
   const ScalarStep st = scalar_step_of(ctx, k);
   static_assert(TILE_THREADS == 256, "the scalar pass maps one workgroup to 256 sorted particles");
   bind_flags([&](auto U, auto W) {
      hipLaunchKernelGGL((k_scalars_step<U.value, W.value>), dim3(div_up(ctx->n, TILE_THREADS)), dim3(TILE_THREADS), 0,
                         ctx->stream, ctx->posm[ctx->cur], ctx->velp[ctx->cur], ctx->scalar_Ts, ctx->scalar_Vs, ctx->ncount,
                         ctx->cell_start, ctx->meta, ctx->grid, k.h2, st, ctx->tile_desc, ctx->nlist, ctx->nlist_overflow,
                         ctx->list_cap, ctx->use_tiled ? 1 : 0, ctx->scalar_force_rows, ctx->scalar_T, ctx->n_scalars);
   }, unit_scale(ctx->prm), ctx->caps.wide != 0);
   SPH_TRY(hipGetLastError());
   return SPH_HIP_OK;
}

// ---- buoyancy (buoyancy_kernels.h; contract: buoyancy_policy.h; decision: launch_policy.h) ------------------
// Behind the step's acceleration pass, in front of its integrate: acc and velp of the sorted state S_k, with the
// channels launch_scalars staged earlier in this step.  The setting travels by value: a later setter does not
// reach the steps already queued.  Nothing synchronises.
int launch_buoyancy(sph_hip_context* ctx)
{
   const sph_hip_params& p = ctx->prm;
   hipLaunchKernelGGL(k_buoyancy_apply, dim3(div_up(ctx->n, 256)), dim3(256), 0, ctx->stream, ctx->scalar_Ts, ctx->meta,
                      ctx->buoyancy, p.time_step, p.cfl_limit, p.cfl_limit2, ctx->acc, ctx->velp[ctx->cur]);
   SPH_TRY(hipGetLastError());
   return SPH_HIP_OK;
}

// ---- cohesion (cohesion_kernels.h; contract: cohesion_policy.h; decision: launch_policy.h) --------------------
// Behind the step's acceleration pass, in front of buoyancy and the integrate: acc of the sorted state S_k, with the
// lists and counts the step's density pass left.  gamma and the constants travel by value: a later setter does not
// reach the steps already queued.  Nothing synchronises.
int launch_cohesion(sph_hip_context* ctx)
{
   const PairConsts k = pair_consts(ctx->prm, ctx->fast != 0);
   static_assert(TILE_THREADS == 256, "the cohesion kernel maps one workgroup to 256 sorted particles");
   bind_flags([&](auto U, auto W) {
      hipLaunchKernelGGL((k_cohesion_apply<U.value, W.value>), dim3(div_up(ctx->n, TILE_THREADS)), dim3(TILE_THREADS), 0,
                         ctx->stream, ctx->posm[ctx->cur], ctx->ncount, ctx->cell_start, ctx->meta, ctx->grid, k,
                         ctx->cohesion_gamma, ctx->tile_desc, ctx->nlist, ctx->nlist_overflow, ctx->list_cap,
                         ctx->use_tiled ? 1 : 0, ctx->acc);
   }, unit_scale(ctx->prm), ctx->caps.wide != 0);
   SPH_TRY(hipGetLastError());
   return SPH_HIP_OK;
}

// ---- implicit viscous stress (viscous_implicit_kernels.h; contract: viscous_implicit_policy.h) -------------------
// What launch_viscous hands over to while the context's viscous setting carries a sweep count: the stage of S_k's
// velocities as launch_viscous launches it, then K Jacobi sweeps over the lists and counts the density pass left.
// The sweeps ping-pong between the two row sets (viscous_implicit_source, viscous_implicit_target); the last one
// writes the velocities of the sorted state, and acc is never touched.  K + 1 launches; mu, the law and the
// constants travel by value: a later setter does not reach the steps already queued.  Nothing synchronises.
int launch_viscous_implicit(sph_hip_context* ctx)
{
   const bool law = ctx->have_viscous_law != 0;
   const int K = ctx->viscous_sweeps;
   float4* const rows[2] = {ctx->viscous_R.get(), ctx->viscous_R2.get()};
   float4* const vel = ctx->velp[ctx->cur];
   bind_flags([&](auto L) {
      hipLaunchKernelGGL((k_viscous_stage<L.value>), dim3(div_up(ctx->n, 256)), dim3(256), 0, ctx->stream, vel,
                         ctx->posm[ctx->cur], ctx->rho, ctx->meta, L.value ? ctx->scalar_Ts.get() : (const float4*)nullptr,
                         ctx->viscous_mu, ctx->viscous_law, rows[0], L.value ? ctx->viscous_M.get() : (float*)nullptr);
   }, law);
   const PairConsts k = pair_consts(ctx->prm, ctx->fast != 0);
   static_assert(TILE_THREADS == 256, "the sweep kernel maps one workgroup to 256 sorted particles");
   for (int s = 0; s < K; s++) {
      const int target = viscous_implicit_target(s, K);
      const float4* const in = rows[viscous_implicit_source(s)];
      bind_flags([&](auto U, auto W, auto L, auto LAST) {
         hipLaunchKernelGGL((k_viscous_sweep<U.value, W.value, L.value, LAST.value>), dim3(div_up(ctx->n, TILE_THREADS)),
                            dim3(TILE_THREADS), 0, ctx->stream, ctx->posm[ctx->cur],
                            LAST.value ? (const float4*)nullptr : vel, in,
                            L.value ? ctx->viscous_M.get() : (const float*)nullptr, ctx->ncount, ctx->cell_start, ctx->meta,
                            ctx->grid, k, ctx->viscous_mu, ctx->tile_desc, ctx->nlist, ctx->nlist_overflow, ctx->list_cap,
                            ctx->use_tiled ? 1 : 0, LAST.value ? vel : rows[target]);
      }, unit_scale(ctx->prm), ctx->caps.wide != 0, law, target < 0);
   }
   SPH_TRY(hipGetLastError());
   return SPH_HIP_OK;
}

// ---- viscous stress (viscous_kernels.h; contract: viscous_policy.h; decision: launch_policy.h) --------------------
// Behind the step's acceleration pass and cohesion, in front of XSPH, buoyancy and the integrate: the stage of S_k's
// velocities with the densities the step's density pass left (and, with a law, of the channels launch_scalars staged
// earlier in this step), then the pass over the lists and counts the density pass left, which adds to acc of the
// sorted state.  mu, the law and the constants travel by value: a later setter does not reach the steps already
// queued.  Nothing synchronises.
int launch_viscous(sph_hip_context* ctx)
{
   if (ctx->viscous_sweeps > 0) return launch_viscous_implicit(ctx);   // (the implicit mode: its own stage and sweeps)
   const bool law = ctx->have_viscous_law != 0;
   bind_flags([&](auto L) {
      hipLaunchKernelGGL((k_viscous_stage<L.value>), dim3(div_up(ctx->n, 256)), dim3(256), 0, ctx->stream,
                         ctx->velp[ctx->cur], ctx->posm[ctx->cur], ctx->rho, ctx->meta,
                         L.value ? ctx->scalar_Ts.get() : (const float4*)nullptr, ctx->viscous_mu, ctx->viscous_law,
                         ctx->viscous_R, L.value ? ctx->viscous_M.get() : (float*)nullptr);
   }, law);
   const PairConsts k = pair_consts(ctx->prm, ctx->fast != 0);
   static_assert(TILE_THREADS == 256, "the viscous kernel maps one workgroup to 256 sorted particles");
   bind_flags([&](auto U, auto W, auto L) {
      hipLaunchKernelGGL((k_viscous_apply<U.value, W.value, L.value>), dim3(div_up(ctx->n, TILE_THREADS)),
                         dim3(TILE_THREADS), 0, ctx->stream, ctx->posm[ctx->cur], ctx->viscous_R,
                         L.value ? ctx->viscous_M.get() : (const float*)nullptr, ctx->ncount, ctx->cell_start, ctx->meta,
                         ctx->grid, k, ctx->viscous_mu, ctx->tile_desc, ctx->nlist, ctx->nlist_overflow, ctx->list_cap,
                         ctx->use_tiled ? 1 : 0, ctx->acc);
   }, unit_scale(ctx->prm), ctx->caps.wide != 0, law);
   SPH_TRY(hipGetLastError());
   return SPH_HIP_OK;
}

// ---- xsph (xsph_kernels.h; contract: xsph_policy.h; decision: launch_policy.h) ----------------------------------
// Behind the step's acceleration pass and cohesion, in front of buoyancy and the integrate: the stage of S_k's
// velocities with the densities the step's density pass left, then the pass over the lists and counts it left,
// which writes velp of the sorted state.  eps and the constants travel by value: a later setter does not reach the
// steps already queued.  Nothing synchronises.
int launch_xsph(sph_hip_context* ctx)
{
   hipLaunchKernelGGL(k_xsph_stage, dim3(div_up(ctx->n, 256)), dim3(256), 0, ctx->stream, ctx->velp[ctx->cur], ctx->rho,
                      ctx->meta, ctx->xsph_R);
   const PairConsts k = pair_consts(ctx->prm, ctx->fast != 0);
   static_assert(TILE_THREADS == 256, "the xsph kernel maps one workgroup to 256 sorted particles");
   bind_flags([&](auto U, auto W) {
      hipLaunchKernelGGL((k_xsph_apply<U.value, W.value>), dim3(div_up(ctx->n, TILE_THREADS)), dim3(TILE_THREADS), 0,
                         ctx->stream, ctx->posm[ctx->cur], ctx->xsph_R, ctx->ncount, ctx->cell_start, ctx->meta, ctx->grid,
                         k, ctx->xsph_eps, ctx->tile_desc, ctx->nlist, ctx->nlist_overflow, ctx->list_cap,
                         ctx->use_tiled ? 1 : 0, ctx->velp[ctx->cur]);
   }, unit_scale(ctx->prm), ctx->caps.wide != 0);
   SPH_TRY(hipGetLastError());
   return SPH_HIP_OK;
}

// ---- step monitor (monitor_kernels.h; contract: monitor_policy.h; grid: launch_policy.h) ------------------------
// Counts the step of a recording and picks the row it fills (mon_row_now, -1: none); on such a step of a context
// whose scalar pass has just run, k_monitor_pairs directly behind that pass, with the volumes it staged.  The
// constants travel by value.  Nothing synchronises.
int launch_monitor_pairs(sph_hip_context* ctx)
{
   const int r = monitor_record_row(++ctx->mon_step, ctx->mon_every, ctx->mon_rows);
   ctx->mon_row_now = r;
   if (r < 0 || !monitor_launches_pairs(ctx->n_scalars, ctx->n)) return SPH_HIP_OK;
   const PairConsts k = pair_consts(ctx->prm, ctx->fast != 0);
   static_assert(TILE_THREADS == 256, "the monitor's pair kernel maps one workgroup to 256 sorted particles");
   bind_flags([&](auto U, auto W) {
      hipLaunchKernelGGL((k_monitor_pairs<U.value, W.value>), dim3(div_up(ctx->n, TILE_THREADS)), dim3(TILE_THREADS), 0,
                         ctx->stream, ctx->posm[ctx->cur], ctx->scalar_Vs, ctx->ncount, ctx->cell_start, ctx->meta,
                         ctx->grid, k, ctx->tile_desc, ctx->nlist, ctx->nlist_overflow, ctx->list_cap,
                         ctx->use_tiled ? 1 : 0, ctx->scalar_force_rows, ctx->mon_pair_part);
   }, unit_scale(ctx->prm), ctx->caps.wide != 0);
   SPH_TRY(hipGetLastError());
   return SPH_HIP_OK;
}

// The row mon_row_now of the step whose integrate has just been enqueued (on either route: posm / velp of ctx->cur
// are what the step produced): k_monitor_particles over the live range the integrate took, then k_monitor_finish
// into the row, whose address travels as a kernel argument.  Nothing synchronises.
int launch_monitor(sph_hip_context* ctx)
{
   const int r = ctx->mon_row_now;
   ctx->mon_row_now = -1;
   const int blocks = monitor_grid(ctx->n);
   const bool pairs = monitor_launches_pairs(ctx->n_scalars, ctx->n);
   hipLaunchKernelGGL(k_monitor_particles, dim3(blocks), dim3(MONITOR_THREADS), 0, ctx->stream, ctx->posm[ctx->cur],
                      ctx->velp[ctx->cur], ctx->acc, ctx->rho, ctx->ncount, ctx->meta,
                      pairs ? ctx->scalar_T.get() : (const float4*)nullptr, ctx->n_scalars, ctx->mon_quantum, ctx->mon_part);
   hipLaunchKernelGGL(k_monitor_finish, dim3(1), dim3(MONITOR_THREADS), 0, ctx->stream, ctx->mon_part, blocks,
                      ctx->mon_pair_part, pairs ? div_up(ctx->n, TILE_THREADS) : 0, pairs ? 1 : 0,
                      ctx->mon_dev.get() + (size_t)r);
   SPH_TRY(hipGetLastError());
   ctx->mon_filled = r + 1;
   return SPH_HIP_OK;
}

// The fused acceleration pass did the rest of the step (FusedStep): the new state is in the other
// buffers, its energy partials one pair per tiled workgroup, and the next build's hash done
// (prehashed: 1 whole grid, 2 a slab's owned entries).
void fused_step_done(sph_hip_context* ctx, int prehashed)
{
   ctx->cur ^= 1;
   ctx->energy_blocks = div_up(ctx->n, TILE_THREADS);
   ctx->prehashed = prehashed;
}

// The state is about to change behind the back of a prehash (upload, exchange, stand-alone
// integrate): forget it, and clear the counts it left in the histogram.
int drop_prehash(sph_hip_context* ctx)
{
   if (!ctx->prehashed) return SPH_HIP_OK;
   ctx->prehashed = 0;
   SPH_TRY(hipMemsetAsync(ctx->cell_count, 0, ((size_t)ctx->scan_tiles * SCAN_TILE + 16) * sizeof(uint32_t),
                          ctx->stream));
   return SPH_HIP_OK;
}

// Keeps the host from running arbitrarily far ahead of the device.  Launch parameters that follow
// the scene - the LDS tile capacities, chosen from statistics the device writes into pinned memory
// (tile_feedback) - are fixed when a step is ENQUEUED: a host that enqueues hundreds of steps at
// once (sph_hip_run(500)) would pick them all from the state before the first one, and a scene that
// compresses meanwhile ends up with nearly every workgroup on the untiled route.  Every PACE_STEPS
// steps an event is recorded and the event of PACE_STEPS steps ago waited for: the device always has
// at least PACE_STEPS steps queued (no bubble), the statistics are at most 2 * PACE_STEPS steps old.
int pace_host(sph_hip_context* ctx)
{
   const long long k = ctx->steps_enqueued++;
   if (k % PACE_STEPS != 0) return SPH_HIP_OK;
   const int slot = (int)((k / PACE_STEPS) & 1);
   if (k >= 2 * PACE_STEPS) SPH_TRY(hipEventSynchronize(ctx->ev_pace[slot]));   // recorded 2 * PACE_STEPS steps ago
   SPH_TRY(hipEventRecord(ctx->ev_pace[slot], ctx->stream));
   return SPH_HIP_OK;
}

// The phase events of the step being enqueued: its timing level (launch_policy.h:
// next_step_level) and the event ring slot they go to.
struct StepEvents {
   Event* ev;
   int level;
   bool full;
};

StepEvents step_events(sph_hip_context* ctx, int level)
{
   return {ctx->ev[ctx->ev_steps % EV_RING], level, ctx->mode == SPH_HIP_MODE_FULL};
}

// opens a step: pacing, then the level and ring slot of its events
int open_step(sph_hip_context* ctx, bool timed, StepEvents& se)
{
   int rc = pace_host(ctx);
   if (rc) return rc;
   se = step_events(ctx, next_step_level(timed, ctx->timing_level, ctx->timing_seen, ctx->timing_stride));
   return SPH_HIP_OK;
}

// phase boundary k (0 .. 6) on stream st, if the step's level records it; boundary 6 ends the step
int mark_phase(sph_hip_context* ctx, const StepEvents& se, int k, hipStream_t st)
{
   if (records_boundary(se.level, se.full, k)) SPH_TRY(hipEventRecord(se.ev[k], st));
   if (k == 6 && se.level != SPH_HIP_TIMING_OFF) ctx->ev_steps++;
   return SPH_HIP_OK;
}

int step_impl(sph_hip_context* ctx, bool timed)
{
   int rc;
   hipStream_t st = ctx->stream;
   StepEvents se;
   // ports: what fires is planned - and a layer that does not fit refused - before anything is enqueued
   const bool ports = ports_active(ctx->n_emit, ctx->n_sink);
   PortFiring firing = {};
   if (ports && (rc = ports_plan(ctx, firing))) return rc;
   if ((rc = open_step(ctx, timed, se))) return rc;
   if ((rc = mark_phase(ctx, se, 0, st))) return rc;
   if (ports && (rc = launch_ports(ctx, firing))) return rc;
   if ((rc = launch_cell_build(ctx))) return rc;
   if (ports) ctx->n_in_stale = 1;
   if (ctx->n_tracers > 0 && (rc = launch_tracers(ctx))) return rc;   // in S_k, before anything moves
   if (ctx->grec_rows > 0 && (rc = launch_gauges(ctx))) return rc;    // likewise
   if ((rc = mark_phase(ctx, se, 1, st))) return rc;
   if ((rc = launch_find_neighbors(ctx))) return rc;
   if ((rc = mark_phase(ctx, se, 2, st))) return rc;
   if ((rc = launch_density(ctx))) return rc;
   // the pressure kinds of a row this step fills: with the densities of S_k the pass has just formed
   if (ctx->grec_row_now >= 0 && (rc = launch_gauges_pressure(ctx, gauge_density_source(true)))) return rc;
   if (ctx->n_scalars > 0 && (rc = launch_scalars(ctx))) return rc;   // carried scalars: in S_k, with its densities and lists
   if (ctx->mon_rows > 0 && (rc = launch_monitor_pairs(ctx))) return rc;   // step monitor: the step is counted, its row picked
   if ((rc = mark_phase(ctx, se, 3, st))) return rc;
   // a context that holds the whole grid and has never exchanged anything: the integrate also
   // hashes and counts for the next cell build - and the tiled acceleration pass does both itself
   const bool hash_too = ctx->mode == SPH_HIP_MODE_FULL && !ctx->had_exchange && ctx->plane_lo == 0 &&
                         ctx->plane_hi == ctx->grid.nz_global &&
                         !ports_no_prehash(ctx->no_prehash != 0, ctx->n_emit, ctx->n_sink);
   // buoyancy: one kernel between the acceleration pass and the integrate, so the step gives up the fused integrate
   const bool buoyant = step_launches_buoyancy(ctx->have_buoyancy != 0, ctx->n_scalars, ctx->n);
   // cohesion: one more such kernel, in front of buoyancy's - either of them takes the step off the fused route
   const bool cohesive = step_launches_cohesion(ctx->have_cohesion != 0, ctx->n);
   // viscous stress: two more such kernels, behind cohesion's and in front of XSPH's; the step keeps the prehash
   const bool viscous = step_launches_viscous(ctx->have_viscous != 0, ctx->n);
   const bool fused = !cohesive &&
                      fuse_integrate(hash_too, ctx->use_tiled != 0, ctx->n, ctx->no_fused_integrate != 0 || viscous,
                                     ctx->n_obst, loads_pending(ctx), buoyant);
   // xsph: two more such kernels, behind cohesion's and in front of buoyancy's; the step keeps the prehash
   const bool smoothing = step_launches_xsph(ctx->have_xsph != 0, ctx->n);
   const bool fuse_now = fused && !smoothing;
   if ((rc = launch_accel(ctx, 0, nullptr, fuse_now))) return rc;
   if (cohesive && (rc = launch_cohesion(ctx))) return rc;
   if (viscous && (rc = launch_viscous(ctx))) return rc;
   if (smoothing && (rc = launch_xsph(ctx))) return rc;
   if (buoyant && (rc = launch_buoyancy(ctx))) return rc;
   if ((rc = mark_phase(ctx, se, 5, st))) return rc;
   if (fuse_now) fused_step_done(ctx, 1);
   else if ((rc = launch_integrate(ctx, hash_too))) return rc;
   if (ctx->mon_row_now >= 0 && (rc = launch_monitor(ctx))) return rc;   // step monitor: the row of the state just produced
   return mark_phase(ctx, se, 6, st);
}

// the six phase times of the step in ring slot `ev` (see sph_hip_set_timing)
int read_phases(sph_hip_context* ctx, const Event* ev, float ms[6])
{
   for (int k = 0; k < 6; k++) ms[k] = 0.0f;
   if (ctx->timing_level == SPH_HIP_TIMING_SUMS) {
      SPH_TRY(hipEventSynchronize(ev[5]));
      SPH_TRY(hipEventElapsedTime(&ms[2], ev[1], ev[5]));
      return SPH_HIP_OK;
   }
   SPH_TRY(hipEventSynchronize(ev[6]));
   const bool full = ctx->mode == SPH_HIP_MODE_FULL;
   for (int k = 0; k < 6; k++)
      SPH_TRY(hipEventElapsedTime(&ms[k], ev[phase_event(full, k)], ev[phase_event(full, k + 1)]));
   return SPH_HIP_OK;
}

// ---- error word of the slab exchange, watched without draining the stream ------------------------
// Request a copy of meta[META_ERRORS] into the pinned watch word.  Before that, wait for the
// PREVIOUS request (made one polling interval ago): normally long done; when the host has run far
// ahead of the device it holds the host back to at most two intervals of queued steps, which is
// what makes "reported within two intervals" true.
int watch_enqueue(sph_hip_context* ctx)
{
   if (ctx->watch_pending) SPH_TRY(hipEventSynchronize(ctx->watch_event));
   SPH_TRY(hipMemcpyAsync((void*)ctx->err_watch.get(), ctx->meta + META_ERRORS, sizeof(int32_t),
                          hipMemcpyDeviceToHost, ctx->stream));
   SPH_TRY(hipEventRecord(ctx->watch_event, ctx->stream));
   ctx->watch_pending = 1;
   return SPH_HIP_OK;
}

// what the last arrived copy said
int watch_check(sph_hip_context* ctx, const char* who)
{
   const int32_t bits = ctx->err_watch[0];
   if (bits == 0) return SPH_HIP_OK;
   char text[256];
   snprintf(text, sizeof(text),
            "%s: the slab exchange lost particles, error bits %d (1 entry outside slab and halo, "
            "2 message overflow, 4 context capacity, 8 missed by the early exchange, 16 a particle id "
            "held twice)", who, (int)bits);
   ctx->err = text;
   return SPH_HIP_ERR_EXCHANGE;
}

} // namespace
