"""CPU checks of the host's launch decisions (csrc/launch_policy.h): the header is plain C++17,
compiled here with g++ behind a small extern "C" shim and called through ctypes.  The expected
values are worked out by hand from the formulas the library has always used."""
import ctypes as C

import pytest

from helpers import compile_shim


SHIM = r"""
#include "launch_policy.h"

static TileLevels levels(const int* cap, const int* per_cu, int n)
{
   TileLevels t = {};
   for (int i = 0; i < n; i++) { t.cap[i] = cap[i]; t.per_cu[i] = per_cu[i]; }
   t.n = n;
   return t;
}
static TileCaps cands(const int* cand, int n)
{
   TileCaps c = {};
   for (int i = 0; i < n; i++) c.cand[i] = cand[i];
   c.n_cand = n;
   return c;
}

extern "C" {
int tile_threads() { return TILE_THREADS; }
int tstat(int which) { const int v[] = {TSTAT_OVER, TSTAT_BLOCKS, TSTAT_MAX, TSTAT_COUNT}; return v[which]; }

// the runtime's answer modelled as: registers allow `nb` workgroups, LDS in 1280-byte granules
int search(int static_lds, int bytes, int nb, int* cap, int* per_cu)
{
   auto blocks_at = [&](int c) {
      const long long need = static_lds + (long long)(c + TILE_PAD) * bytes;
      const long long granules = (need + LDS_GRANULE - 1) / LDS_GRANULE;
      const int by_lds = (int)(LDS_PER_CU / (granules * LDS_GRANULE));
      return nb < by_lds ? nb : by_lds;
   };
   const TileLevels t = search_levels(blocks_at, bytes);
   for (int i = 0; i < t.n; i++) { cap[i] = t.cap[i]; per_cu[i] = t.per_cu[i]; }
   return t.n;
}
int merge(const int* d, int nd, const int* a, int na, int* out)
{
   const int one[TILE_CANDS] = {0};
   TileCaps c = {};
   merge_candidates(levels(d, one, nd), levels(a, one, na), c);
   for (int i = 0; i < c.n_cand; i++) out[i] = c.cand[i];
   return c.n_cand;
}
int pick(const int* cand, int n_cand, const int* fb, const int* cap, const int* per_cu, int n, int accel,
         int over_other)
{
   const TileCaps c = cands(cand, n_cand);
   const TileLevels lv = levels(cap, per_cu, n);
   if (!accel) return pick_level(c, fb, lv, DENSITY_THR, DENSITY_GIVEUP_COST);
   return pick_level(c, fb, lv, ACCEL_THR, ACCEL_UNTILED_COST, over_other, ACCEL_LISTED_COST);
}
void choose(const int* cand, int n_cand, const int* fb, const int* dcap, const int* dper, int dn,
            const int* acap, const int* aper, int an, int forced, int forced_accel, int forced_density, int* out)
{
   TileCaps c = cands(cand, n_cand);
   choose_caps(c, fb, levels(dcap, dper, dn), levels(acap, aper, an), forced, forced_accel, forced_density);
   out[0] = c.cap_density;
   out[1] = c.cap_accel;
   out[2] = c.wide;
}
int grow(int without, int blocks) { return lists_should_grow(without, blocks); }
int smaller(int want) { return smaller_list_cap(want); }
int grown(long long most, int active, int capacity) { return grown_active_records(most, active, capacity); }
int trim(int most, float slack, int extra, int capacity) { return trim_records(most, slack, extra, capacity); }
void ranges(int lo, int hi, int z0, int nz, int halo, int left, int right, int* out)
{
   const PlaneRanges r = plane_ranges(lo, hi, z0, nz, halo, left != 0, right != 0);
   const int v[6] = {r.own_lo, r.own_hi, r.sum_lo, r.sum_hi, r.bnd_lo, r.bnd_hi};
   for (int i = 0; i < 6; i++) out[i] = v[i];
}
int event_of(int full, int k) { return phase_event(full != 0, k); }
int records(int level, int full, int k) { return records_boundary(level, full != 0, k); }
int next_level(int timed, int level, long long* seen, int stride) { return next_step_level(timed != 0, level, *seen, stride); }
}
"""

OFF, SUMS, PHASES = 0, 1, 2


@pytest.fixture(scope="module")
def pol(tmp_path_factory):
    p = compile_shim(SHIM, ["-O1"], tmp_path_factory)
    p.trim.argtypes = [C.c_int, C.c_float, C.c_int, C.c_int]
    p.grown.argtypes = [C.c_longlong, C.c_int, C.c_int]
    return p


def ints(values, n=None):
    values = list(values) + [0] * ((n or len(values)) - len(values))
    return (C.c_int * max(1, len(values)))(*values)


def feedback(pol, blocks, over=(), largest=0):
    fb = [0] * pol.tstat(3)
    fb[pol.tstat(1)] = blocks
    fb[pol.tstat(2)] = largest
    for i, v in enumerate(over):
        fb[pol.tstat(0) + i] = v
    return ints(fb)


def pick(pol, fb, levels, per_cu, accel=False, over_other=-1, cand=None):
    cand = levels if cand is None else cand
    return pol.pick(ints(cand), len(cand), fb, ints(levels), ints(per_cu), len(levels), int(accel), over_other)


def choose(pol, fb, dlev, dper, alev, aper, forced=0, forced_accel=0, forced_density=0):
    cand = sorted(set(dlev) | set(alev))
    out = ints([0, 0, 0])
    pol.choose(ints(cand), len(cand), fb, ints(dlev), ints(dper), len(dlev), ints(alev), ints(aper), len(alev),
               forced, forced_accel, forced_density, out)
    return tuple(out)


def test_constants(pol):
    assert pol.tile_threads() == 256
    assert [pol.tstat(i) for i in range(4)] == [0, 12, 13, 17]


def test_level_search_without_an_answer(pol):
    cap, per_cu = ints([], 12), ints([], 12)
    assert pol.search(0, 12, 0, cap, per_cu) == 1
    assert (cap[0], per_cu[0]) == (3008, 3)


@pytest.mark.parametrize("static_lds,bytes_,nb", [(0, 12, 8), (2048, 12, 6), (512, 16, 5), (0, 16, 2)])
def test_level_search_finds_the_largest_tile_per_occupancy(pol, static_lds, bytes_, nb):
    def blocks(c):
        need = static_lds + (c + 32) * bytes_
        return min(nb, 160 * 1024 // (-(-need // 1280) * 1280))
    cap_max = 16384 - 32
    while cap_max > 256 and (cap_max + 32) * bytes_ > 156 * 1024:
        cap_max -= 32
    want_caps, want_per, prev = [], [], 0
    for want in range(blocks(992), 0, -1):
        if len(want_caps) >= 6:
            break
        lo = max(c for c in range(992, cap_max + 1, 32) if blocks(c) >= want)
        if lo > prev:
            want_caps.append(lo)
            want_per.append(want)
            prev = lo
        if lo >= cap_max:
            break
    cap, per_cu = ints([], 12), ints([], 12)
    n = pol.search(static_lds, bytes_, nb, cap, per_cu)
    assert list(cap)[:n] == want_caps and list(per_cu)[:n] == want_per


def test_candidates_are_the_ascending_union(pol):
    out = ints([], 12)
    n = pol.merge(ints([2176, 2624, 3008]), 3, ints([1984, 2624, 4000, 5000]), 4, out)
    assert list(out)[:n] == [1984, 2176, 2624, 3008, 4000, 5000]


def test_nothing_reported_takes_the_level_next_to_3008(pol):
    fb = feedback(pol, 0)
    assert pick(pol, fb, [2176, 2624, 3008, 3552], [6, 5, 4, 3]) == 3008
    assert pick(pol, fb, [2176, 2624, 3040, 3552], [6, 5, 4, 3]) == 3040
    assert pick(pol, fb, [1984, 2176, 2624], [6, 5, 4]) == 2624


def test_untiled_route_is_taken_only_where_it_hides(pol):
    # 10 workgroups exceed 2000 entries; every one fits 4000
    levels, per_cu = [2000, 4000], [6, 4]
    assert pick(pol, feedback(pol, 8191, [10, 0]), levels, per_cu) == 4000   # too few to hide ~100 us
    # 8192 workgroups: (1 - 10/8192) / 1.0 + 3 * 10/8192 = 1.0024 beats 1 / 0.93
    assert pick(pol, feedback(pol, 8192, [10, 0]), levels, per_cu) == 2000


def test_acceleration_prefers_the_list_driven_route(pol):
    levels, per_cu = [2000, 4000], [5, 3]
    fb = feedback(pol, 10000, [500, 0])
    # untiled search for the 5 %: 0.95 + 8 * 0.05 = 1.35 > 1 / 0.87
    assert pick(pol, fb, levels, per_cu, accel=True) == 4000
    assert pick(pol, fb, levels, per_cu, accel=True, over_other=500) == 4000
    # all of them fitted the density pass and have lists: 0.95 + 2.5 * 0.05 = 1.075 < 1.149
    assert pick(pol, fb, levels, per_cu, accel=True, over_other=0) == 2000


def test_wide_entries_exactly_above_tile_cap_max(pol):
    fb = feedback(pol, 0)
    assert choose(pol, fb, [2176, 3008], [6, 5], [2176, 3008], [5, 4]) == (3008, 3008, 0)
    assert choose(pol, fb, [2176, 4064], [6, 5], [2176, 4064], [5, 4]) == (4064, 4064, 0)
    assert choose(pol, fb, [2176, 4096], [6, 5], [2176, 3008], [5, 4]) == (4096, 3008, 1)
    assert choose(pol, fb, [2176, 3008], [6, 5], [2176, 4096], [5, 4]) == (3008, 4096, 1)
    assert choose(pol, fb, [2176], [6], [2176], [5], forced=4064)[2] == 0
    assert choose(pol, fb, [2176], [6], [2176], [5], forced=4096)[2] == 1


def test_forced_capacities_and_their_overrides(pol):
    fb = feedback(pol, 20000, [20000])   # (ignored when forced)
    lev = ([2176], [6], [2176], [5])
    assert choose(pol, fb, *lev, forced=3008) == (3008, 3008, 0)
    assert choose(pol, fb, *lev, forced=3008, forced_accel=2048) == (3008, 2048, 0)
    assert choose(pol, fb, *lev, forced=3008, forced_density=1024) == (1024, 3008, 0)
    # an override has to be smaller than the forced value and at least 256
    assert choose(pol, fb, *lev, forced=3008, forced_accel=4000, forced_density=3008) == (3008, 3008, 0)
    assert choose(pol, fb, *lev, forced=3008, forced_accel=224, forced_density=0) == (3008, 3008, 0)
    # wide follows the forced value, not the overrides
    assert choose(pol, fb, *lev, forced=6016, forced_accel=2048, forced_density=2048) == (2048, 2048, 1)


@pytest.mark.parametrize("without,blocks,grows", [(64, 0, 0), (65, 0, 1), (65, 65, 0), (66, 65, 1),
                                                  (64, 10, 0), (1000, 999, 1), (1000, 1000, 0)])
def test_list_growth_threshold(pol, without, blocks, grows):
    assert pol.grow(without, blocks) == grows


def test_list_sizes_on_allocation_failure(pol):
    assert [pol.smaller(1022), pol.smaller(510)] == [510, 254]


@pytest.mark.parametrize("most,active,capacity,new", [
    (80, 100, 200, 100),     # exactly 4/5: no
    (81, 100, 200, 200),     # more than 4/5: back to capacity
    (0, 100, 200, 100),
    (10 ** 6, 200, 200, 200),  # already at capacity: never changes
    (150, 200, 200, 200),
])
def test_message_growth(pol, most, active, capacity, new):
    assert pol.grown(most, active, capacity) == new


@pytest.mark.parametrize("most,slack,extra,capacity,want", [
    (100, 1.5, 10, 1000, 160), (1000, 2.0, 0, 1500, 1500), (0, 1.0, 0, 100, 1), (3, 1.0, 0, 100, 3),
    (0, 1.0, 7, 5, 5)])
def test_trim_size(pol, most, slack, extra, capacity, want):
    assert pol.trim(most, slack, extra, capacity) == want


@pytest.mark.parametrize("slab,want", [
    # (plane_lo, plane_hi, z0, nz, halo, left, right): own, sum, border ranges (local planes)
    ((0, 40, 0, 40, 2, 0, 0), [0, 40, 0, 40, 0, 40]),       # no neighbour
    ((20, 40, 18, 22, 2, 1, 0), [2, 22, 1, 22, 5, 22]),     # left neighbour only
    ((10, 20, 8, 14, 2, 1, 1), [2, 12, 1, 13, 5, 9]),       # both
    ((10, 12, 8, 6, 2, 1, 1), [2, 4, 1, 5, 4, 2]),          # thinner than halo + 1
])
def test_slab_plane_ranges(pol, slab, want):
    out = ints([], 6)
    pol.ranges(*slab, out)
    assert list(out) == want


def test_phase_events(pol):
    assert [pol.event_of(0, k) for k in range(7)] == [0, 1, 2, 3, 3, 5, 6]   # REF
    assert [pol.event_of(1, k) for k in range(7)] == [0, 1, 1, 3, 3, 5, 6]   # FULL
    rec = lambda level, full: [k for k in range(7) if pol.records(level, full, k)]
    assert rec(PHASES, 0) == [0, 1, 2, 3, 5, 6]
    assert rec(PHASES, 1) == [0, 1, 3, 5, 6]
    assert rec(SUMS, 0) == rec(SUMS, 1) == [1, 5]
    assert rec(OFF, 0) == rec(OFF, 1) == []


def test_timing_stride(pol):
    seen = C.c_longlong(0)
    assert [pol.next_level(1, PHASES, C.byref(seen), 3) for _ in range(7)] == [2, 0, 0, 2, 0, 0, 2]
    assert seen.value == 7
    assert pol.next_level(0, PHASES, C.byref(seen), 3) == OFF and seen.value == 7
    assert pol.next_level(1, OFF, C.byref(seen), 1) == OFF and seen.value == 7
