// The neighbour walk of the per-particle pair passes: k_scalars_step (scalar_kernels.h), k_monitor_pairs
// (monitor_kernels.h), k_cohesion_apply (cohesion_kernels.h) and k_xsph_apply (xsph_kernels.h), consumers of the
// neighbour lists the density pass left for the acceleration pass.  k_viscous_apply (viscous_kernels.h) and
// k_velgrad_particles (velgrad_kernels.h, the row walk only) keep copies of it: on this one their register counts and
// packed arithmetic moved (the pair walk), so what changes here changes there.
//
// One workgroup takes 256 sorted particles of the live range.  A lane takes its list a block of eight entries per
// trip, the next block requested before this one's gathers (accel_from_lists' loop: full_tiled.h); a workgroup or a
// lane without a list walks the nine cell rows as k_particle_density does (pressure_kernels.h), by the scalar pass's
// route decisions (launch_policy.h: scalar_workgroup_route, scalar_lane_route).  Same pairs, same order, same
// arithmetic on either route: same bits.  The only LDS is the kernel's copy of its TileDesc, and every local array
// is indexed by unrolled constants (none lives in scratch memory).
//
// What the walk asks of a pass's accumulator (sample_kernels.h's vocabulary; DESIGN.md: the pair walk):
//   Payload                          what a neighbour contributes besides posm[q] (an empty struct: nothing)
//   gather(q)                        loads it, the streams in the pass's own order, behind posm[q].  The list walk
//                                    gathers for all eight entries of a block before the first add, the row walk
//                                    for members only, behind the d2 < h2 test
//   add<UNIT_SCALE>(pi, pj, payload) one pair into the sums
// The accumulator holds the pass's own row, its constants and its sums; the kernel reads the sums when the walk
// has returned.
#pragma once

#include "cell_build.h"
#include "full_tiled.h"
#include "launch_policy.h"
#include "neighbor_lists.h"
#include "pair_math.h"

static_assert(SCALAR_FLAG_LISTS_NONE == LISTS_NONE && SCALAR_FLAG_LISTS_SOME == LISTS_SOME &&
                 SCALAR_WORD_NO_LIST == NLIST_NO_LIST,
              "launch_policy.h restates the list flags of neighbor_lists.h");

// What the workgroup step tells a lane.  any: the workgroup holds a live particle (workgroup-uniform); live: this
// lane does.
struct PairLane {
   int wg, tid, p;
   bool any, live;
   uint32_t flag;
   int wg_route;
};

// The workgroup step: the live range, the workgroup, its flag and route, and its TileDesc into sd.  To be called
// by every lane of the workgroup: the barrier inside tile_desc_load is reached by every lane or by none (any, the
// flag and the route are workgroup-uniform).  A workgroup past the live range reads neither its flag nor its
// descriptor; a kernel with nothing to store for it returns on !live (every lane does), k_monitor_pairs goes on to
// its fold.  tiled: the context's density pass wrote lists and flags (else nlist_overflow and desc are not read);
// force_rows: every workgroup walks the rows.
__device__ __forceinline__ PairLane pair_workgroup(const int32_t* __restrict__ meta, int tiled, int force_rows,
                                                   const uint32_t* __restrict__ nlist_overflow,
                                                   const TileDesc* __restrict__ desc, TileDesc& sd)
{
   PairLane w;
   const int begin = meta[META_SUM_BEGIN], end = meta[META_SUM_END];
   w.tid = threadIdx.x;
   w.wg = xcd_workgroup(blockIdx.x, gridDim.x);
   const int p0 = begin + w.wg * TILE_THREADS;
   w.any = p0 < end;
   w.p = p0 + w.tid;
   w.live = w.p < end;
   w.flag = (tiled && w.any) ? nlist_overflow[w.wg] : LISTS_NONE;
   w.wg_route = scalar_workgroup_route(tiled != 0, force_rows != 0, w.flag);
   if (w.any && w.wg_route == SCALAR_ROUTE_LISTS) tile_desc_load(desc, w.wg, sd);
   return w;
}

// the list walk of one lane: one 16-byte load per eight entries
template <bool UNIT_SCALE, bool WIDE, class Acc>
__device__ __forceinline__ void pair_walk_lists(int cnt, const ListReader& lr, const TileDesc& d, const float4& pi,
                                                const float4* __restrict__ posm, Acc& a)
{
   const int lastb = cnt > 0 ? (cnt - 1) >> 3 : 0;
   uint4 blk = lr.block(0);
   for (int j0 = 0; j0 < cnt; j0 += 8) {
      uint32_t entry[8];
      list_block_entries(blk, entry);
      blk = lr.block(min((j0 >> 3) + 1, lastb));
      float4 pj[8];
      typename Acc::Payload pay[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
         const uint32_t e = j0 + u < cnt ? entry[u] : entry[0];      // (entry 0 of a block in use is a neighbour)
         const int q = ListEntry<WIDE>::tile(e) - ListEntry<WIDE>::shift(d, e);
         pj[u] = posm[q];
         pay[u] = a.gather(q);
      }
#pragma unroll
      for (int u = 0; u < 8; u++)
         if (j0 + u < cnt) a.template add<UNIT_SCALE>(pi, pj[u], pay[u]);
   }
}

// the row walk of one lane (k_particle_density's: pressure_kernels.h): the nine cell rows of the particle's cell,
// itself skipped, the membership test in front of the payload's gather
template <bool UNIT_SCALE, class Acc>
__device__ __forceinline__ void pair_walk_rows(int p, const CellGrid& g, const uint32_t* __restrict__ cell_start, float h2,
                                               const float4& pi, const float4* __restrict__ posm, Acc& a)
{
   int cx, cy, cz;
   cell_of(g, pi.x, pi.y, pi.z, cx, cy, cz);
   RowRanges r;
   row_ranges(g, cell_start, cx, cy, cz, r);
#pragma unroll 1
   for (int row = 0; row < 9; row++) {
      uint32_t b, e;
      row_range(r, row, b, e);
      for (uint32_t q = b; q < e; q++) {
         if (q == (uint32_t)p) continue;
         const float4 pj = posm[q];
         float dx, dy, dz;
         const float d2 = dist2(pi.x, pi.y, pi.z, pj.x, pj.y, pj.z, dx, dy, dz);
         if (d2 < h2) a.template add<UNIT_SCALE>(pi, pj, a.gather(q));
      }
   }
}

// The lane step, for a live lane behind pair_workgroup: its list, or its rows.  pi = posm[w.p].
template <bool UNIT_SCALE, bool WIDE, class Acc>
__device__ __forceinline__ void pair_walk(const PairLane& w, const TileDesc& sd, const int32_t* __restrict__ ncount,
                                          const uint32_t* __restrict__ nlist, int list_cap, const CellGrid& g,
                                          const uint32_t* __restrict__ cell_start, float h2, const float4& pi,
                                          const float4* __restrict__ posm, Acc& a)
{
   int lane_route = SCALAR_ROUTE_ROWS;
   if (w.wg_route == SCALAR_ROUTE_LISTS) {
      const int cnt = ncount[w.p];
      const ListReader lr(nlist, w.wg, list_cap, w.tid);
      const uint32_t first_word = (w.flag == LISTS_SOME && cnt > 0) ? (lr.no_list() ? NLIST_NO_LIST : 0u) : 0u;
      lane_route = scalar_lane_route(w.wg_route, w.flag, cnt, first_word);
      if (lane_route == SCALAR_ROUTE_LISTS) pair_walk_lists<UNIT_SCALE, WIDE>(cnt, lr, sd, pi, posm, a);
   }
   if (lane_route == SCALAR_ROUTE_ROWS) pair_walk_rows<UNIT_SCALE>(w.p, g, cell_start, h2, pi, posm, a);
}
