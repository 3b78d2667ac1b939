"""CPU: which 256-particle workgroup a hardware workgroup computes (csrc/launch_policy.h:
xcd_workgroup_ascending / xcd_workgroup_descending, the functions the kernels call).

The dispatcher deals consecutive block indices round-robin over the 8 XCDs; residue class x of
block mod 8 owns a contiguous share of the workgroups.  The density pass walks each share from the
bottom up, the single-context acceleration launch from the top down, so that it begins with what
the density pass wrote last.  What must hold, in both directions and for every grid size: the
mapping is a bijection onto [0, wgs), and an XCD computes exactly the workgroups it computed
before (the descending walk visits the ascending walk's share, backwards)."""
import ctypes as C

import pytest

from helpers import compile_shim

SHIM = r"""
#include "launch_policy.h"
extern "C" {
int xcds() { return XCD_COUNT; }
int ascending(int block, int n) { return xcd_workgroup_ascending(block, n); }
int descending(int block, int n) { return xcd_workgroup_descending(block, n); }
int share_begin(int xcd, int n) { return xcd_share_begin(xcd, n); }
int share_size(int xcd, int n) { return xcd_share_size(xcd, n); }
void fill(int n, int down, int* out)
{
   for (int b = 0; b < n; b++) out[b] = down ? xcd_workgroup_descending(b, n) : xcd_workgroup_ascending(b, n);
}
// usable in a constant expression: the kernels' own compiler folds it where the grid is known
// (17 workgroups: XCD 0 owns 0..2, XCD 1 owns 3..4; block 9 is XCD 1's second)
static_assert(xcd_workgroup_ascending(9, 17) == 4 && xcd_workgroup_descending(9, 17) == 3, "");
}
"""

SIZES = (1, 7, 8, 9, 63, 64, 65, 16384, 16385)


@pytest.fixture(scope="module")
def pol(tmp_path_factory):
    return compile_shim(SHIM, ["-O1"], tmp_path_factory)


def mapping(pol, n, down):
    out = (C.c_int * n)()
    pol.fill(n, int(down), out)
    return list(out)


def old_formula(block, n):
    """xcd_workgroup as csrc/full_tiled.h had it before the mapping moved to launch_policy.h"""
    q, r, x = n // 8, n % 8, block % 8
    return (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + block // 8


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("down", (False, True), ids=("ascending", "descending"))
def test_bijection(pol, n, down):
    m = mapping(pol, n, down)
    assert sorted(m) == list(range(n))


@pytest.mark.parametrize("n", SIZES)
def test_ascending_is_the_mapping_the_kernels_always_had(pol, n):
    assert mapping(pol, n, False) == [old_formula(b, n) for b in range(n)]


@pytest.mark.parametrize("n", SIZES)
def test_every_xcd_keeps_its_workgroups(pol, n):
    assert pol.xcds() == 8
    up, down = mapping(pol, n, False), mapping(pol, n, True)
    covered = 0
    for x in range(8):
        mine_up = up[x::8]        # blocks x, x + 8, ...: the ones the dispatcher hands XCD x
        mine_down = down[x::8]
        b, s = pol.share_begin(x, n), pol.share_size(x, n)
        assert s == len(mine_up) == n // 8 + (1 if x < n % 8 else 0)
        assert mine_up == list(range(b, b + s))              # a contiguous share, bottom up
        assert mine_down == mine_up[::-1]                    # the same share, top down
        assert b == covered                                  # shares in XCD order, no gap
        covered += s
    assert covered == n


@pytest.mark.parametrize("n", SIZES)
def test_descending_starts_where_ascending_ends(pol, n):
    """XCD x's first block of the descending walk is its last of the ascending one"""
    for x in range(min(8, n)):
        last_block = x + 8 * (pol.share_size(x, n) - 1)
        assert pol.descending(x, n) == pol.ascending(last_block, n)
        assert pol.descending(last_block, n) == pol.ascending(x, n)
