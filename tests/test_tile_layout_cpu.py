"""CPU checks of csrc/tile_layout.h: the layout of a workgroup's LDS tile (tile_layout_chain, moved
out of tile_desc()) and the pass plan of the tile fill (tile_pass_plan: per pass of 256 tile indices
the shift of its first index plus the boundaries strictly inside).  The header is plain C++17,
compiled with g++ behind a shim (tests/tile_layout_shim.py) as tests/test_launch_policy.py does.

Reference: the search every lane used to run for every load - D of the LARGEST k with B[k] <= idx -
restated in Python, and the chain-forming loop as it stood in csrc/full_tiled.h, restated too; the
hand-made cases carry expected values worked out by hand."""
import numpy as np
import pytest

from tile_layout_shim import Layout, old_chain, old_search, old_search_all, plan_shifts


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    lay = Layout(tmp_path_factory)
    assert lay.threads == 256
    return lay


def check_descriptor(layout, D, B, total, chained=True):
    """every index gets the old search's shift out of the plans (which cover [0, total) once and in
    order: plan_shifts), tile_shift_at is the old search, and the mask of passes is exact"""
    want = old_search_all(D, B, total)
    got = plan_shifts(layout, D, B, total)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]
    T = layout.threads
    probes = {0, total - 1, total, -1}
    for b in B:
        probes |= {b - 1, b, b + 1}
    for q in range((total + T - 1) // T + 1):
        probes |= {q * T - 1, q * T, q * T + 1}
    for t in probes:
        assert layout.shift_at(D, B, total, t) == old_search(D, B, t), t
    # bit q of the mask <=> the plan of pass q lists a boundary (an empty segment in the middle of a
    # chain is listed with its successor, which puts the chain's shift back: no index has the empty
    # segment's).  For a descriptor made by tile_layout_chain the shift falls from chain to chain and
    # never comes back, so a pass is of one shift <=> its first and last index agree.
    mask = layout.pass_mask(D, B, total)
    for q in range(min((total + T - 1) // T, 63)):
        first, end, _, inside = layout.plan(D, B, total, q)
        assert bool(mask >> q & 1) == bool(inside), (q, mask, inside)
        one_shift = bool((want[first:end] == want[first]).all())
        assert one_shift or inside, q
        if chained:
            assert one_shift == bool(want[first] == want[end - 1]), (q, inside)
    # a lane past the tile's end is clamped to the last index: a pass behind the end has every lane there
    if total > 0:
        for q in range((total + T - 1) // T, (total + T - 1) // T + 3):
            assert layout.shift_at(D, B, total, min(q * T, total - 1)) == want[total - 1]


def chain_case(layout, G, length, D, B, total):
    """tile_layout_chain gives the hand-made expectation, which is what the pre-move loop gives"""
    assert old_chain(G, length) == (D, B, total)
    assert layout.chain(G, length) == (D, B, total)
    assert all(B[k] <= B[k + 1] for k in range(8)) and B[0] == 0
    check_descriptor(layout, D, B, total)


def test_nine_separate_segments(layout):
    G = [100 + 200 * k for k in range(9)]
    length = [50] * 9
    chain_case(layout, G, length, D=[50 * k - G[k] for k in range(9)], B=[50 * k for k in range(9)], total=450)
    # pass 0 = [0, 256): boundaries 50 .. 250 inside, pass 1 = [256, 450): 300 .. 400
    first, end, shift, inside = layout.plan([50 * k - G[k] for k in range(9)], [50 * k for k in range(9)], 450, 0)
    assert (first, end, shift) == (0, 256, -100) and [b for b, _ in inside] == [50, 100, 150, 200, 250]
    first, end, shift, inside = layout.plan([50 * k - G[k] for k in range(9)], [50 * k for k in range(9)], 450, 1)
    assert (first, end, shift) == (256, 450, 250 - 1100) and [b for b, _ in inside] == [300, 350, 400]


def test_three_chains_of_three_merged_segments(layout):
    G = [1000, 1010, 1020, 5000, 5010, 5020, 9000, 9010, 9020]
    length = [40] * 9
    D = [-1000] * 3 + [60 - 5000] * 3 + [120 - 9000] * 3
    B = [0, 40, 50, 60, 100, 110, 120, 160, 170]
    chain_case(layout, G, length, D, B, 180)
    # boundaries between segments that share a shift are not reported
    _, _, shift, inside = layout.plan(D, B, 180, 0)
    assert shift == -1000 and inside == [(60, -4940), (120, -8880)]


def test_zero_length_segments_first_middle_last(layout):
    G = [7, 100, 200, 300, 400, 500, 600, 700, 800]
    length = [0, 30, 30, 0, 30, 30, 30, 30, 0]
    D = [-7, -100, -170, -240, -340, -410, -480, -550, -620]
    B = [0, 0, 30, 60, 60, 90, 120, 150, 180]
    chain_case(layout, G, length, D, B, 180)
    # index 0 belongs to segment 1 (B[1] = B[0] = 0: the largest k wins), index 60 to segment 4
    assert layout.shift_at(D, B, 180, 0) == -100 and layout.shift_at(D, B, 180, 60) == -340
    assert layout.plan(D, B, 180, 0)[2] == -100


def test_all_segments_empty_but_one(layout):
    for k_full in (0, 4, 8):
        G = [10 * k for k in range(9)]
        length = [0] * 9
        length[k_full] = 300
        D, B, total = old_chain(G, length)
        assert total == 300
        assert layout.chain(G, length) == (D, B, total)
        check_descriptor(layout, D, B, total)
        assert set(old_search_all(D, B, total).tolist()) == {-G[k_full]}


def test_partial_overlap_with_the_predecessor(layout):
    G = [100, 120, 130, 1000, 2000, 3000, 4000, 5000, 6000]
    length = [50, 50, 10, 10, 10, 10, 10, 10, 10]
    D = [-100, -100, -100, -930, -1920, -2910, -3900, -4890, -5880]
    B = [0, 50, 70, 70, 80, 90, 100, 110, 120]      # segment 1 adds 20 entries, segment 2 none
    chain_case(layout, G, length, D, B, 130)


def test_new_parts_longer_than_a_pass_and_of_exactly_one_and_two(layout):
    G = [0, 1000, 2000, 3000, 4000, 5000, 6000, 7000, 8000]
    length = [300, 256, 512, 700, 1, 255, 257, 3, 5]
    D, B, total = old_chain(G, length)
    assert B == [0, 300, 556, 1068, 1768, 1769, 2024, 2281, 2284] and total == 2289
    assert D[1] == 300 - 1000 and D[2] == 556 - 2000
    assert layout.chain(G, length) == (D, B, total)
    check_descriptor(layout, D, B, total)
    # passes inside one segment list nothing: [768, 1024) lies in segment 2, [1280, 1536) in segment 3
    assert layout.plan(D, B, total, 3)[3] == [] and layout.plan(D, B, total, 5)[3] == []
    # ... pass 6 = [1536, 1792) holds two boundaries, 1768 and 1769
    assert [b for b, _ in layout.plan(D, B, total, 6)[3]] == [1768, 1769]


def test_boundaries_exactly_on_multiples_of_a_pass(layout):
    G = [1000 * k for k in range(9)]
    length = [256, 256, 512, 256, 0, 256, 768, 256, 256]
    D, B, total = old_chain(G, length)
    assert B == [0, 256, 512, 1024, 1280, 1280, 1536, 2304, 2560] and total == 2816
    assert layout.chain(G, length) == (D, B, total)
    check_descriptor(layout, D, B, total)
    assert layout.pass_mask(D, B, total) == 0
    for q in range(11):
        first, _, shift, inside = layout.plan(D, B, total, q)
        assert inside == [] and shift == old_search(D, B, first)


@pytest.mark.parametrize("total", [0, 1, 255, 256, 257, 2048, 2049])
def test_totals_around_a_pass_and_a_batch(layout, total):
    # one segment of the whole size, and the same size split over three chains
    for length in ([0, 0, 0, 0, total, 0, 0, 0, 0], [total // 3, 0, 0, total // 3, 0, 0, total - 2 * (total // 3), 0, 0]):
        G = [50000 * k + 11 for k in range(9)]
        D, B, tot = old_chain(G, length)
        assert tot == total
        assert layout.chain(G, length) == (D, B, tot)
        check_descriptor(layout, D, B, tot)


def test_a_descriptor_no_chain_would_make(layout):
    """the plan does not need the shifts to fall: a shift that comes back (A, B, A inside one pass),
    equal shifts side by side, boundaries on top of each other"""
    D = [5, 9, 5, 5, 7, 7, 5, 1, 2]
    B = [0, 10, 20, 30, 30, 30, 40, 300, 300]
    check_descriptor(layout, D, B, 600, chained=False)
    _, _, shift, inside = layout.plan(D, B, 600, 0)
    assert shift == 5 and inside == [(10, 9), (20, 5), (30, 7), (40, 5)]


def test_random_segments(layout):
    rng = np.random.default_rng(20240611)
    sizes = [0, 0, 1, 3, 17, 100, 255, 256, 257, 400, 700]
    for case in range(3000):
        # ascending ranges of the sorted arrays: gaps, touching and overlapping neighbours, empty ones
        G, length = [], []
        pos = int(rng.integers(0, 1000))
        for k in range(9):
            n = int(rng.choice(sizes)) if rng.random() < 0.7 else int(rng.integers(0, 600))
            G.append(pos)
            length.append(n)
            step = rng.random()
            if step < 0.35:
                pos += int(rng.integers(0, max(n, 1) + 1))          # overlaps or touches
            elif step < 0.5:
                pos += n                                             # touches exactly
            else:
                pos += n + int(rng.integers(1, 2000))                # a gap: a new chain
        D, B, total = old_chain(G, length)
        assert layout.chain(G, length) == (D, B, total), case
        assert all(B[k] <= B[k + 1] for k in range(8))
        check_descriptor(layout, D, B, total)
