"""csrc/tile_layout.h behind an extern "C" shim (compiled with g++ by helpers.compile_shim), and the
code it replaced restated in Python: the reference of tests/test_tile_layout_cpu.py, and what
tests/test_gpu_tile_fill.py recomputes the workgroups' tile descriptors with."""
import ctypes as C

import numpy as np

from helpers import compile_shim

SEGMENTS = 9

SHIM = r"""
#include "tile_layout.h"

static TileDesc desc_of(const int* w)
{
   TileDesc d;
   for (int k = 0; k < 9; k++) { d.D[k] = w[k]; d.B[k] = w[9 + k]; }
   d.total = w[18];
   d.pad = 0;
   return d;
}

extern "C" {
int tile_threads() { return TILE_THREADS; }
int desc_words() { return (int)(sizeof(TileDesc) / sizeof(int)); }
// D[9], B[9], total, pad: TileDesc's own layout
void chain(const int* G, const int* len, int* out)
{
   int g[9], l[9];
   for (int k = 0; k < 9; k++) { g[k] = G[k]; l[k] = len[k]; }
   TileDesc d;
   tile_layout_chain(g, l, d);
   const int* w = reinterpret_cast<const int*>(&d);
   for (int i = 0; i < 20; i++) out[i] = w[i];
}
int shift_at(const int* w, int t)
{
   const TileDesc d = desc_of(w);
   return tile_shift_at(d.B, d.D, t);
}
unsigned long long pass_mask(const int* w)
{
   const TileDesc d = desc_of(w);
   return tile_pass_mask(d.B, d.D, d.total);
}
// out: first, end, shift, n, B[8], D[8]
void plan(const int* w, int q, int* out)
{
   const TileDesc d = desc_of(w);
   TilePassPlan p = {};
   tile_pass_plan(d, q, p);
   out[0] = p.first; out[1] = p.end; out[2] = p.shift; out[3] = p.n;
   for (int i = 0; i < 8; i++) { out[4 + i] = i < p.n ? p.B[i] : 0; out[12 + i] = i < p.n ? p.D[i] : 0; }
}
}
"""


def ints(values):
    values = [int(v) for v in values]
    return (C.c_int * max(1, len(values)))(*values)


class Layout:
    def __init__(self, tmp_path_factory):
        self.lib = compile_shim(SHIM, ["-O1"], tmp_path_factory)
        self.lib.pass_mask.restype = C.c_ulonglong
        self.threads = self.lib.tile_threads()
        assert self.lib.desc_words() == 20

    def chain(self, G, length):
        """-> (D[9], B[9], total) of tile_layout_chain"""
        out = ints([0] * 20)
        self.lib.chain(ints(G), ints(length), out)
        assert out[19] == 0
        return list(out[0:9]), list(out[9:18]), out[18]

    @staticmethod
    def words(D, B, total):
        return ints(list(D) + list(B) + [total, 0])

    def shift_at(self, D, B, total, t):
        return self.lib.shift_at(self.words(D, B, total), int(t))

    def pass_mask(self, D, B, total):
        return int(self.lib.pass_mask(self.words(D, B, total)))

    def plan(self, D, B, total, q):
        """-> (first, end, shift, [(B, D) of the boundaries inside])"""
        out = ints([0] * 20)
        self.lib.plan(self.words(D, B, total), int(q), out)
        n = out[3]
        assert 0 <= n <= 8
        return out[0], out[1], out[2], [(out[4 + i], out[12 + i]) for i in range(n)]


def old_search(D, B, idx):
    """what every lane ran for every load of the tile fill: D of the largest k with B[k] <= idx"""
    d = D[0]
    for k in range(1, SEGMENTS):
        if idx >= B[k]:
            d = D[k]
    return d


def old_search_all(D, B, total):
    """old_search for every index 0 .. total - 1"""
    idx = np.arange(total, dtype=np.int64)
    d = np.full(total, D[0], np.int64)
    for k in range(1, SEGMENTS):
        d = np.where(idx >= B[k], D[k], d)
    return d


def old_chain(G, length):
    """the chain-forming loop of tile_desc() as it stood in csrc/full_tiled.h -> (D, B, total)"""
    D, B = [0] * SEGMENTS, [0] * SEGMENTS
    run, chain_end, chain_d = 0, -1, 0
    for k in range(SEGMENTS):
        B[k] = run
        if length[k] == 0:
            D[k] = run - G[k]
        elif G[k] <= chain_end:
            seg_end = G[k] + length[k]
            D[k] = chain_d
            if seg_end > chain_end:
                run += seg_end - chain_end
                chain_end = seg_end
        else:
            D[k] = chain_d = run - G[k]
            run += length[k]
            chain_end = G[k] + length[k]
    return D, B, run


def plan_shifts(layout, D, B, total):
    """the shift of every tile index as the pass plans give it, with the plans' own contract checked:
    the passes cover [0, total) once and in order, and list only boundaries strictly inside"""
    T = layout.threads
    got = np.zeros(total, np.int64)
    passes = (total + T - 1) // T
    for q in range(passes):
        first, end, shift, inside = layout.plan(D, B, total, q)
        assert first == q * T and end == min(first + T, total), (q, first, end, total)
        idx = np.arange(first, end, dtype=np.int64)
        d = np.full(end - first, shift, np.int64)
        for b, dk in inside:
            assert first < b < end, (q, first, b, end)
            d = np.where(idx >= b, dk, d)
        got[first:end] = d
    # the pass behind the last one is empty
    first, end, _, inside = layout.plan(D, B, total, passes)
    assert first == passes * T and end == first and inside == []
    return got


def workgroup_descriptors(layout, p, ids, cs, ci, begin=0, end=None):
    """The tile descriptors of the 256-particle workgroups over sorted positions [begin, end), as
    tile_desc() (csrc/full_tiled.h) works them out - from the oracle's full_cells(): ids = cell per
    particle, cs = first sorted position per cell, ci = particle per sorted position.
    -> list of (D, B, total, G, len)"""
    nx, ny = int(p.full_cells_x), int(p.full_cells_y)
    ncells = nx * ny * int(p.full_cells_z)
    end = ci.size if end is None else end
    T = layout.threads
    out = []
    for p0 in range(begin, end, T):
        plast = min(p0 + T - 1, end - 1)
        c_first, c_last = int(ids[ci[p0]]), int(ids[ci[plast]])
        G, length = [0] * SEGMENTS, [0] * SEGMENTS
        for k in range(SEGMENTS):
            off = ((k // 3 - 1) * ny + (k % 3 - 1)) * nx
            lo, hi = max(c_first + off - 1, 0), min(c_last + off + 1, ncells - 1)
            if hi >= lo:
                G[k] = int(cs[lo])
                length[k] = int(cs[hi + 1]) - G[k]
        D, B, total = layout.chain(G, length)
        out.append((D, B, total, G, length))
    return out
