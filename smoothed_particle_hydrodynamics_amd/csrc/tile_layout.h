// Layout of a workgroup's LDS tile as plain values: how the nine row segments of a 256-particle
// workgroup are placed in the tile (tile_layout_chain, the descriptor k_tile_desc stores), and how
// a pass of the tile fill - TILE_THREADS consecutive tile indices, one load per lane - finds its
// shift from tile index to sorted index (tile_pass_plan and the pieces it is made of, which
// tile_load() of full_tiled.h runs on workgroup-uniform values in scalar registers).
// Pure C++17, host and device (tests/test_tile_layout_cpu.py compiles it with g++).
#pragma once

#include <stdint.h>

#include "launch_policy.h"

#ifdef __HIPCC__
#define TILE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TILE_HD inline
#endif

#define TILE_SEGMENTS 9   // (dz, dy) rows around a workgroup's span of cells
// The segments after the first (k, k - 1), written out, and the descriptor words read into locals
// before anything is selected among them: on the device the words then stay in (scalar) registers.
// Written as `d = t >= B[k] ? D[k] : d` in a loop, the selects became ONE load behind a selected
// address, and the words went to scratch memory to have an address.
#define TILE_EACH_BOUNDARY(X) X(1, 0) X(2, 1) X(3, 2) X(4, 3) X(5, 4) X(6, 5) X(7, 6) X(8, 7)
#define TILE_WORDS(k, prev) const int B##k = B[k], D##k = D[k];
#define TILE_LOCALS const int D0 = D[0]; TILE_EACH_BOUNDARY(TILE_WORDS)

// Per-workgroup tile layout, computed by k_tile_desc before the sums run.
struct TileDesc {
   int D[9];      // tile index = sorted index + D[k] inside segment k
   int B[9];      // first tile index of segment k (B[0] = 0)
   int total;     // tile entries; > the launch's tile capacity => the workgroup runs untiled
   int pad;
};

// The nine segments as ranges [G[k], G[k] + len[k]) of the sorted arrays (ascending in k) -> their
// placement in the tile.  Segments come in ascending sorted position.  Where consecutive ones
// overlap or touch (short rows: a 256-particle span then covers several rows, and the dy = -1, 0,
// +1 segments of a plane are nearly the same range) they share tile storage: same index shift D,
// and only the part past the previous segment's end is new.  B[k] = first tile index of segment
// k's new part, so "tile index t in [B[k], B[k+1])  <->  sorted index t - D[k]" holds for the
// loader.  B never decreases with k.
TILE_HD void tile_layout_chain(const int (&G)[TILE_SEGMENTS], const int (&len)[TILE_SEGMENTS], TileDesc& d)
{
   int run = 0, chain_end = -1, chain_d = 0;
#ifdef __HIPCC__
#pragma unroll
#endif
   for (int k = 0; k < TILE_SEGMENTS; k++) {
      d.B[k] = run;
      if (len[k] == 0) {          // nothing to load, no lane range refers to it
         d.D[k] = run - G[k];
      } else if (G[k] <= chain_end) {
         const int seg_end = G[k] + len[k];
         d.D[k] = chain_d;
         if (seg_end > chain_end) {
            run += seg_end - chain_end;
            chain_end = seg_end;
         }
      } else {
         d.D[k] = chain_d = run - G[k];
         run += len[k];
         chain_end = G[k] + len[k];
      }
   }
   d.total = run;
   d.pad = 0;
}

// The shift of tile index t: D of the LARGEST k with B[k] <= t (B[0] = 0 <= every index).  This is
// the search every lane used to run for every load; the fill runs it once per pass, on t = the
// pass's first index.
TILE_HD int tile_shift_at(const int (&B)[TILE_SEGMENTS], const int (&D)[TILE_SEGMENTS], int t)
{
   TILE_LOCALS
   int d = D0;
#define TILE_STEP(k, prev) d = (t >= B##k) ? D##k : d;
   TILE_EACH_BOUNDARY(TILE_STEP)
#undef TILE_STEP
   return d;
}

// Bit k (1..8): boundary B[k] lies strictly inside (lo, hi) and switches to another shift than the
// one in force before it.  (B never decreases, so every index >= B[k] is >= B[k-1] as well and the
// shift in force just below B[k] is D[k-1]: a segment chained to its predecessor, D[k] = D[k-1],
// changes nothing.  Boundaries at one and the same index - empty segments - are all reported and
// applied in ascending k: the largest k wins, as in the search.)
TILE_HD uint32_t tile_pass_boundaries(const int (&B)[TILE_SEGMENTS], const int (&D)[TILE_SEGMENTS], int lo, int hi)
{
   TILE_LOCALS
   uint32_t m = 0;
#define TILE_STEP(k, prev) m |= ((B##k > lo) & (B##k < hi) & (D##k != D##prev)) ? 1u << k : 0u;
   TILE_EACH_BOUNDARY(TILE_STEP)
#undef TILE_STEP
   return m;
}

// Bit q: pass q - tile indices [q * TILE_THREADS, min((q + 1) * TILE_THREADS, total)) - holds a
// boundary of tile_pass_boundaries() strictly inside; worked out once per workgroup, so that a pass
// without one (most of them) costs a bit test.  Passes from 63 on share bit 63.
TILE_HD uint64_t tile_pass_mask(const int (&B)[TILE_SEGMENTS], const int (&D)[TILE_SEGMENTS], int total)
{
   TILE_LOCALS
   uint64_t m = 0;
#define TILE_STEP(k, prev)                                                                          \
   m |= ((B##k > 0) & (B##k < total) & (B##k % TILE_THREADS != 0) & (D##k != D##prev))             \
           ? 1ull << (B##k / TILE_THREADS < 63 ? B##k / TILE_THREADS : 63) : 0ull;
   TILE_EACH_BOUNDARY(TILE_STEP)
#undef TILE_STEP
   return m;
}
TILE_HD bool tile_pass_has_boundary(uint64_t mask, int q)
{
   return (mask >> (q < 63 ? q : 63)) & 1u;
}

// What pass q of the fill needs: the shift of its first index, and the boundaries strictly inside
// it (ascending k) with the shift each switches to.  An index t of the pass has the shift of the
// last listed boundary <= t, or `shift` if there is none: exactly tile_shift_at(t).
struct TilePassPlan {
   int first, end;    // tile indices [first, end) of the pass (empty past the tile's end)
   int shift;         // of index `first`
   int n;             // boundaries inside
   int B[TILE_SEGMENTS - 1];
   int D[TILE_SEGMENTS - 1];
};
TILE_HD void tile_pass_plan(const TileDesc& d, int q, TilePassPlan& p)
{
   p.first = q * TILE_THREADS;
   p.end = p.first + TILE_THREADS < d.total ? p.first + TILE_THREADS : d.total;
   if (p.end < p.first) p.end = p.first;
   p.shift = tile_shift_at(d.B, d.D, p.first);
   p.n = 0;
   if (!tile_pass_has_boundary(tile_pass_mask(d.B, d.D, d.total), q)) return;
   const uint32_t m = tile_pass_boundaries(d.B, d.D, p.first, p.end);
   for (int k = 1; k < TILE_SEGMENTS; k++)
      if (m >> k & 1u) {
         p.B[p.n] = d.B[k];
         p.D[p.n] = d.D[k];
         p.n++;
      }
}
