"""CPU checks of the step monitor (include/sph_hip.h: step monitor): csrc/monitor_policy.h, compiled with g++ behind
an extern "C" shim, against the numpy restatement tests/monitor_emulation.py bit for bit - seeded particles, every
way of being bad, the 2^38 term limit, signed zeros, negative channels, the empty set, the ordered key, the fold of
partial rows; every refusal text; the struct's layout; the grid; step_impl's order read from the text;
MonitorRecord's formulas on hand-made rows; the header's code under the host's sanitizers."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import monitor_emulation as ME
from helpers import compile_shim

F32 = np.float32
U32 = np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smoothed_particle_hydrodynamics_amd", "csrc")

# n slots through the header's functions, spread over `parts` partial accumulators the way the kernel's grid strides
# (slot i goes to partial i % parts), folded in the order `parts - 1 .. 0`: what the device's shuffles, LDS and
# k_monitor_finish sum to.  Rows are read at exactly the indices 0 .. n-1.
WALK = r"""
#include <math.h>
#include <stddef.h>
#include <vector>

#include "monitor_policy.h"
#include "launch_policy.h"

static MonitorAcc walk(int n, int parts, const float* pos, const float* vel, const float* mass, const uint32_t* ids,
                       const float* acc, const float* rho, const int32_t* ncount, int quantum_log2, const float* T,
                       int n_rows)
{
   std::vector<MonitorAcc> part(parts);
   for (int b = 0; b < parts; b++) monitor_clear(part[b]);
   const double scale = load_scale(quantum_log2);
   for (int i = 0; i < n; i++) {
      MonitorAcc& a = part[i % parts];
      const bool good = monitor_particle(a, pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], mass[i], vel[3 * i], vel[3 * i + 1],
                                         vel[3 * i + 2], ids[i], acc[3 * i], acc[3 * i + 1], acc[3 * i + 2], rho[i],
                                         ncount[i], scale);
      if (T && good && ids[i] < (uint32_t)n_rows)
         monitor_scalars(a, Scalar4{T[4 * ids[i]], T[4 * ids[i] + 1], T[4 * ids[i] + 2], T[4 * ids[i] + 3]});
   }
   MonitorAcc total;
   monitor_clear(total);
   for (int b = parts - 1; b >= 0; b--) monitor_merge(total, part[b]);
   return total;
}

static MonitorPairAcc walk_pairs(int n, const float* S)
{
   MonitorPairAcc a;
   monitor_pair_clear(a);
   for (int i = 0; i < n; i++) {
      MonitorPairAcc one;
      monitor_pair_clear(one);
      monitor_pair_offer(one, S[i]);
      monitor_pair_merge(a, one);
   }
   return a;
}
"""

SHIM = WALK + r"""
extern "C" {
int abi() { return SPH_HIP_ABI_VERSION; }
void run(int n, int parts, const float* pos, const float* vel, const float* mass, const uint32_t* ids, const float* acc,
         const float* rho, const int32_t* ncount, int quantum_log2, const float* T, int n_rows, long long* sum,
         int32_t* add, uint32_t* mx, uint32_t* mn)
{
   const MonitorAcc a = walk(n, parts, pos, vel, mass, ids, acc, rho, ncount, quantum_log2, T, n_rows);
   for (int i = 0; i < MON_SUMS; i++) sum[i] = a.sum[i];
   for (int i = 0; i < MON_ADDS; i++) add[i] = a.add[i];
   for (int i = 0; i < MON_MAXS; i++) mx[i] = a.mx[i];
   for (int i = 0; i < MON_MINS; i++) mn[i] = a.mn[i];
}
void row(const long long* sum, const int32_t* add, const uint32_t* mx, const uint32_t* mn, int have_scalars,
         int have_pairs, uint32_t s_key, int pair_bad, sph_hip_monitor_row* out)
{
   MonitorAcc a;
   for (int i = 0; i < MON_SUMS; i++) a.sum[i] = sum[i];
   for (int i = 0; i < MON_ADDS; i++) a.add[i] = add[i];
   for (int i = 0; i < MON_MAXS; i++) a.mx[i] = mx[i];
   for (int i = 0; i < MON_MINS; i++) a.mn[i] = mn[i];
   const MonitorPairAcc p = {s_key, pair_bad};
   *out = monitor_row_of(a, have_scalars != 0, have_pairs != 0, p);
}
void pairs(int n, const float* S, uint32_t* s_key, int32_t* pair_bad)
{
   const MonitorPairAcc a = walk_pairs(n, S);
   *s_key = a.s_key;
   *pair_bad = a.pair_bad;
}
// S_p of one particle: its members' volumes and distances in order
float pair_sum(int n, const float* V, const float* d, float hscaled, float kernel3)
{
   float S = 0.0f;
   for (int j = 0; j < n; j++) monitor_pair(S, V[j], d[j], hscaled, kernel3);
   return S;
}
uint32_t key(uint32_t bits) { return monitor_key(monitor_float(bits)); }
uint32_t unkey(uint32_t k) { return monitor_bits(monitor_unkey(k)); }
uint32_t max_bits(uint32_t k) { return monitor_bits(monitor_max_value(k)); }
uint32_t min_bits(uint32_t k) { return monitor_bits(monitor_min_value(k)); }
int grid(int n) { return monitor_grid(n); }
int launches_pairs(int n_scalars, int n) { return monitor_launches_pairs(n_scalars, n) ? 1 : 0; }
int record_row(long long step, int every, int rows) { return monitor_record_row(step, every, rows); }
int record_step(int row, int every) { return monitor_record_step(row, every); }
static const char* text(const char* w) { return w ? w : ""; }
const char* rows_check(int rows) { return text(monitor_rows_check(rows)); }
const char* every_check(int every) { return text(monitor_every_check(every)); }
const char* quantum_check(int q) { return text(monitor_quantum_check(q)); }
const char* mode_check(int full) { return text(monitor_mode_check(full != 0)); }
const char* slab_check(int whole) { return text(monitor_slab_check(whole != 0)); }
const char* ports_set_check(int set) { return text(monitor_ports_set_check(set != 0)); }
const char* ports_check(int rows, int ne, int ns) { return text(monitor_ports_check(rows, ne, ns)); }
const char* exchange_check(int rows) { return text(monitor_exchange_check(rows)); }
const char* range_check(int first, int n, int filled) { return text(monitor_range_check(first, n, filled)); }
int row_size() { return (int)sizeof(sph_hip_monitor_row); }
int row_offset(int field)
{
   switch (field) {
   case 0: return (int)offsetof(sph_hip_monitor_row, momentum);
   case 1: return (int)offsetof(sph_hip_monitor_row, kinetic);
   case 2: return (int)offsetof(sph_hip_monitor_row, mass);
   case 3: return (int)offsetof(sph_hip_monitor_row, live);
   case 4: return (int)offsetof(sph_hip_monitor_row, bad);
   case 5: return (int)offsetof(sph_hip_monitor_row, skipped);
   case 6: return (int)offsetof(sph_hip_monitor_row, lone);
   case 7: return (int)offsetof(sph_hip_monitor_row, ncount_max);
   case 8: return (int)offsetof(sph_hip_monitor_row, scalar_bad);
   case 9: return (int)offsetof(sph_hip_monitor_row, pair_bad);
   case 10: return (int)offsetof(sph_hip_monitor_row, bad_id_min);
   case 11: return (int)offsetof(sph_hip_monitor_row, v2_max);
   case 12: return (int)offsetof(sph_hip_monitor_row, a2_max);
   case 13: return (int)offsetof(sph_hip_monitor_row, rho_max);
   case 14: return (int)offsetof(sph_hip_monitor_row, rho_min);
   case 15: return (int)offsetof(sph_hip_monitor_row, s_max);
   case 16: return (int)offsetof(sph_hip_monitor_row, scalar_min);
   case 17: return (int)offsetof(sph_hip_monitor_row, scalar_max);
   case 18: return (int)offsetof(sph_hip_monitor_row, flags);
   }
   return -1;
}
}
"""

CHECKS = {"rows_check": 1, "every_check": 1, "quantum_check": 1, "mode_check": 1, "slab_check": 1, "ports_set_check": 1,
          "ports_check": 3, "exchange_check": 1, "range_check": 3}


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def key1(x):
    """the key of one float, as an int"""
    return int(ME.key(np.array([x], F32))[0])


def bits1(x):
    return int(ME.bits(np.array([x], F32))[0])


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    lib = compile_shim(SHIM, ["-O2", "-ffp-contract=off"], tmp_path_factory)
    V, I = C.c_void_p, C.c_int
    lib.run.argtypes = [I, I, V, V, V, V, V, V, V, I, V, I, V, V, V, V]
    lib.run.restype = None
    lib.row.argtypes = [V, V, V, V, I, I, C.c_uint32, I, V]
    lib.row.restype = None
    lib.pairs.argtypes = [I, V, V, V]
    lib.pairs.restype = None
    lib.pair_sum.argtypes = [I, V, V, C.c_float, C.c_float]
    lib.pair_sum.restype = C.c_float
    for name in ("key", "unkey", "max_bits", "min_bits"):
        getattr(lib, name).argtypes = [C.c_uint32]
        getattr(lib, name).restype = C.c_uint32
    lib.record_row.argtypes = [C.c_longlong, I, I]
    for name, k in CHECKS.items():
        getattr(lib, name).argtypes = [I] * k
        getattr(lib, name).restype = C.c_char_p
    return lib


class Set:
    """n particles in particle order with ids 0 .. n-1 unless given."""

    def __init__(self, pos, vel, mass, acc, rho, ncount, ids=None, T=None):
        self.pos = np.ascontiguousarray(pos, F32).reshape(-1, 3)
        self.vel = np.ascontiguousarray(vel, F32).reshape(-1, 3)
        self.acc = np.ascontiguousarray(acc, F32).reshape(-1, 3)
        self.mass = np.ascontiguousarray(mass, F32)
        self.rho = np.ascontiguousarray(rho, F32)
        self.ncount = np.ascontiguousarray(ncount, np.int32)
        self.n = self.mass.size
        self.ids = np.ascontiguousarray(np.arange(self.n) if ids is None else ids, U32)
        self.T = None if T is None else np.ascontiguousarray(T, F32).reshape(-1, 4)


def header_acc(policy, s, quantum_log2=-24, parts=1):
    a = dict(sum=np.zeros(ME.SUMS, np.int64), add=np.zeros(ME.ADDS, np.int32), mx=np.zeros(ME.MAXS, U32),
             mn=np.zeros(ME.MINS, U32))
    # exact-size copies: a read past row n-1 leaves the arrays
    policy.run(s.n, parts, ptr(s.pos.copy()), ptr(s.vel.copy()), ptr(s.mass.copy()), ptr(s.ids.copy()), ptr(s.acc.copy()),
               ptr(s.rho.copy()), ptr(s.ncount.copy()), quantum_log2, ptr(s.T), 0 if s.T is None else s.T.shape[0],
               ptr(a["sum"]), ptr(a["add"]), ptr(a["mx"]), ptr(a["mn"]))
    return a


def emulated_acc(s, quantum_log2=-24):
    return ME.particles(s.pos, s.vel, s.mass, s.ids, s.acc, s.rho, s.ncount, quantum_log2, s.T)


def same_acc(a, b):
    return all(np.array_equal(np.asarray(a[k], np.int64), np.asarray(b[k], np.int64)) for k in ("sum", "add", "mx", "mn"))


def header_row(policy, a, have_scalars, pairs):
    out = np.zeros(1, ME.ROW)
    policy.row(ptr(np.ascontiguousarray(a["sum"], np.int64)), ptr(np.ascontiguousarray(a["add"], np.int32)),
               ptr(np.ascontiguousarray(a["mx"], U32)), ptr(np.ascontiguousarray(a["mn"], U32)), int(have_scalars),
               int(pairs is not None), 0 if pairs is None else pairs[0], 0 if pairs is None else pairs[1], ptr(out))
    return out[0]


def seeded(rng, n, with_T=True):
    pos = rng.uniform(0.0, 1.0, (n, 3))
    vel = rng.uniform(-3.0, 3.0, (n, 3))
    acc = rng.uniform(-50.0, 50.0, (n, 3))
    mass = rng.uniform(0.5, 1.5, n)
    rho = rng.uniform(500.0, 1500.0, n)
    ncount = rng.integers(0, 64, n)
    T = rng.uniform(-2.0, 2.0, (n, 4)) if with_T else None
    return Set(pos, vel, mass, acc, rho, ncount, rng.permutation(n), T)


# ---- the header against the restatement -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 257, 3000])
@pytest.mark.parametrize("quantum_log2", [-24, -40, 3])
def test_header_equals_the_restatement_bit_for_bit(policy, n, quantum_log2):
    rng = np.random.default_rng(100 + n)
    for with_T in (True, False):
        s = seeded(rng, n, with_T)
        if n > 10:
            s.ncount[::9] = 0
            s.vel[5] = 0.0
            s.rho[7] = np.inf                 # a bad particle among the others
            s.vel[11, 1] = 3.0e38             # finite, its square is not: v2_max = +inf, its terms are skipped
        got, want = header_acc(policy, s, quantum_log2), emulated_acc(s, quantum_log2)
        assert same_acc(got, want), (n, with_T)
        assert int(got["add"][ME.ADD_LIVE]) == n
        if n > 10:
            assert got["add"][ME.ADD_BAD] == 1 and got["mn"][ME.MIN_BAD_ID] == s.ids[7]
            assert got["add"][ME.ADD_SKIPPED] >= 1 and got["add"][ME.ADD_LONE] > 0
            assert ME.max_value(got["mx"][ME.MAX_V2]) == np.inf
        for have_scalars, pairs in ((with_T, (key1(1.5), 2) if with_T else None), (False, None)):
            r, w = header_row(policy, got, have_scalars, pairs), ME.row_of(want, have_scalars, pairs)
            assert ME.same_rows(r, w) == []
            assert int(r["flags"]) == (3 if pairs else 0)


def good(n=4):
    """n plain particles: every field finite, unit mass"""
    return Set(np.full((n, 3), 0.5), np.full((n, 3), 0.25), np.ones(n), np.full((n, 3), 2.0), np.full(n, 1000.0),
               np.full(n, 30), T=np.full((n, 4), 0.5))


BAD_WAYS = [("pos", 0), ("pos", 1), ("pos", 2), ("vel", 0), ("vel", 1), ("vel", 2), ("acc", 0), ("acc", 1), ("acc", 2),
            ("rho", None)]


@pytest.mark.parametrize("field,axis", BAD_WAYS)
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_a_particle_bad_in_each_way_is_left_out_of_everything_else(policy, field, axis, value):
    s = good(5)
    s.ids[:] = [40, 7, 19, 3, 22]
    s.T = np.full((41, 4), 0.5, F32)
    # the bad one would win every range and change every sum and count if it took part
    s.vel[2], s.acc[2], s.rho[2], s.ncount[2], s.mass[2], s.T[19] = 100.0, 1000.0, 1.0e6, 0, 64.0, (-9.0, 9.0, np.nan, 9.0)
    arr = getattr(s, field)
    if axis is None:
        arr[2] = value
    else:
        arr[2, axis] = value
    got = header_acc(policy, s)
    assert same_acc(got, emulated_acc(s))
    rest = Set(*(np.delete(getattr(s, nm), 2, 0) for nm in ("pos", "vel", "mass", "acc", "rho", "ncount")),
               ids=np.delete(s.ids, 2), T=s.T)
    alone = header_acc(policy, rest)
    assert got["add"][ME.ADD_BAD] == 1 and got["mn"][ME.MIN_BAD_ID] == 19 and got["add"][ME.ADD_LIVE] == 5
    for k in ("sum", "mx"):
        assert np.array_equal(got[k], alone[k]), k
    assert np.array_equal(got["mn"][1:], alone["mn"][1:]) and alone["mn"][ME.MIN_BAD_ID] == ME.NO_ID
    assert np.array_equal(got["add"][2:], alone["add"][2:]) and got["add"][ME.ADD_SCALAR_BAD] == 0
    # two bad ones: the smaller id wins in either order
    s.rho[0] = -1.0e-30 if value != value else value
    for order in ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0]):
        t = Set(s.pos[order], s.vel[order], s.mass[order], s.acc[order], s.rho[order], s.ncount[order], s.ids[order], s.T)
        assert header_acc(policy, t)["mn"][ME.MIN_BAD_ID] == 19 and header_acc(policy, t)["add"][ME.ADD_BAD] == 2


def test_a_negative_density_is_bad_and_minus_zero_is_not(policy):
    s = good(3)
    s.rho[:] = [-1.0e-38, -0.0, 0.0]
    got = header_acc(policy, s)
    assert same_acc(got, emulated_acc(s))
    assert got["add"][ME.ADD_BAD] == 1 and got["mn"][ME.MIN_BAD_ID] == 0
    r = header_row(policy, got, True, None)
    assert bits1(r["rho_min"]) == 0x80000000 and bits1(r["rho_max"]) == 0


def test_terms_at_and_just_under_the_limit(policy):
    """quantum 2^0: a unit-velocity particle of mass 2^38 reaches the limit in m*vx and m (skipped), the float just
    under it does not; the kinetic term alone at the limit skips too."""
    limit = F32(2.0 ** 38)
    under = np.nextafter(limit, F32(0.0))
    for m, v, skipped in ((limit, (1.0, 0.0, 0.0), 1), (under, (1.0, 0.0, 0.0), 0), (under, (-1.0, 0.0, 0.0), 0),
                          (F32(2.0), (limit / F32(2.0), 0.0, 0.0), 1), (F32(1.0), (under, 0.0, 0.0), 1),
                          (F32(2.0 ** 37), (0.0, -2.0, 0.0), 1), (F32(1.0), (0.0, 0.0, 524288.0), 0),
                          (F32(2.0), (0.0, 0.0, 524288.0), 1)):
        s = Set([[0.5] * 3], [v], [m], [[0.0] * 3], [1000.0], [3])
        got, want = header_acc(policy, s, 0), emulated_acc(s, 0)
        assert same_acc(got, want)
        assert got["add"][ME.ADD_SKIPPED] == skipped, (m, v)
        assert (got["sum"] == 0).all() == bool(skipped)
        assert got["add"][ME.ADD_BAD] == 0 and got["mx"][ME.MAX_V2] != ME.KEY_NO_MAX     # (skipped is not bad)
    # ties go to even, and a quantum that resolves nothing sums zeros
    s = Set([[0.5] * 3] * 2, [[0.5, 1.5, 2.5], [-0.5, -1.5, -2.5]], [1.0, 1.0], [[0.0] * 3] * 2, [1.0, 1.0], [1, 1])
    got = header_acc(policy, s, 0)
    assert same_acc(got, emulated_acc(s, 0)) and got["sum"][:3].tolist() == [0, 0, 0]
    one = Set(s.pos[:1], s.vel[:1], s.mass[:1], s.acc[:1], s.rho[:1], s.ncount[:1])
    assert header_acc(policy, one, 0)["sum"].tolist() == [0, 2, 2, 4, 1]      # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 4.375 -> 4


def test_signed_zeros_in_every_range_in_both_orders(policy):
    neg, pos = F32(-0.0), F32(0.0)
    for order in ((neg, pos), (pos, neg)):
        s = good(2)
        s.rho[:] = order
        s.T[0], s.T[1] = order[0], order[1]
        got = header_acc(policy, s)
        assert same_acc(got, emulated_acc(s))
        r = header_row(policy, got, True, None)
        assert bits1(r["rho_min"]) == 0x80000000 and bits1(r["rho_max"]) == 0
        assert (ME.bits(r["scalar_min"]) == 0x80000000).all() and (ME.bits(r["scalar_max"]) == 0).all()
        # the pair pass's offer
        key = np.zeros(1, U32)
        bad = np.zeros(1, np.int32)
        policy.pairs(2, ptr(np.array(order, F32)), ptr(key), ptr(bad))
        assert (int(key[0]), int(bad[0])) == ME.pair_acc(np.array(order, F32)) and policy.max_bits(int(key[0])) == 0
    # v2 and a2 are sums of squares: a velocity of -0.0f gives +0.0f, which is a value, not "nothing offered"
    s = good(1)
    s.vel[:], s.acc[:] = neg, neg
    got = header_acc(policy, s)
    assert same_acc(got, emulated_acc(s)) and got["mx"][ME.MAX_V2] == 0x80000000 == got["mx"][ME.MAX_A2]
    assert policy.pairs(1, ptr(np.array([neg], F32)), ptr(key), ptr(bad)) is None and key[0] == 0x7FFFFFFF


def test_negative_channels_and_channels_that_are_not_finite(policy):
    s = good(4)
    s.T[:] = [[-3.0, -1.0e-40, 5.0, np.nan], [-2.0, -1.0e-45, np.inf, -7.0], [-4.5, -0.0, -np.inf, -8.0], [-2.5, -1.0, 1.0, 2.0]]
    got = header_acc(policy, s)
    assert same_acc(got, emulated_acc(s))
    r = header_row(policy, got, True, None)
    assert r["scalar_min"].tolist() == [-4.5, -1.0, 1.0, -8.0]
    assert r["scalar_max"][[0, 2, 3]].tolist() == [-2.0, 5.0, 2.0] and bits1(r["scalar_max"][1]) == 0x80000000
    assert r["scalar_bad"] == 3 and r["bad"] == 0
    # an id outside the rows carries nothing
    s.ids[3] = 99
    again = header_acc(policy, s)
    assert same_acc(again, emulated_acc(s)) and ME.min_value(again["mn"][ME.MIN_SCALAR + 1]) == F32(-1.0e-40)
    # a context without scalars: the row's scalar fields are zeros, whatever the accumulator holds
    r = header_row(policy, got, False, None)
    assert not r["scalar_min"].any() and not r["scalar_max"].any() and r["scalar_bad"] == 0 and r["flags"] == 0


def test_the_empty_set(policy):
    s = good(0)
    got = header_acc(policy, s)
    assert same_acc(got, ME.empty()) and same_acc(got, emulated_acc(s))
    for have_scalars, pairs in ((False, None), (True, (ME.KEY_NO_MAX, 0))):
        r = header_row(policy, got, have_scalars, pairs)
        assert ME.same_rows(r, ME.row_of(ME.empty(), have_scalars, pairs)) == []
        want = np.zeros((), ME.ROW)
        want["bad_id_min"], want["flags"] = ME.NO_ID, 3 if pairs else 0
        assert r.tobytes() == want.tobytes()
    key, bad = np.ones(1, U32), np.ones(1, np.int32)
    policy.pairs(0, None, ptr(key), ptr(bad))
    assert key[0] == ME.KEY_NO_MAX and bad[0] == 0


EDGE_BITS = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000, 0x3F800000,
             0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7FFFFFFF, 0xFFFFFFFF]


def test_the_ordered_key(policy):
    keys = [policy.key(b) for b in EDGE_BITS]
    assert keys == ME.key(np.array(EDGE_BITS, U32).view(F32)).tolist()
    assert [policy.unkey(k) for k in keys] == EDGE_BITS                           # the round trip
    assert ME.bits(ME.unkey(np.array(keys, U32))).tolist() == EDGE_BITS
    # the key rises with the value: -inf < -max < -1 < -min < -denormal < -0 < +0 < denormal < ... < +inf
    ordered = [0xFF800000, 0xFF7FFFFF, 0xBF800000, 0x80800000, 0x807FFFFF, 0x80000001, 0x80000000, 0x00000000, 0x00000001,
               0x007FFFFF, 0x00800000, 0x3F800000, 0x7F7FFFFF, 0x7F800000]
    ks = [policy.key(b) for b in ordered]
    assert ks == sorted(ks) and len(set(ks)) == len(ks)
    # "nothing offered" are the keys of two NaN patterns and decode to +0.0f
    assert policy.key(0xFFFFFFFF) == ME.KEY_NO_MAX and policy.key(0x7FFFFFFF) == ME.KEY_NO_MIN
    assert policy.max_bits(ME.KEY_NO_MAX) == 0 and policy.min_bits(ME.KEY_NO_MIN) == 0
    assert policy.max_bits(policy.key(0xBF800000)) == 0xBF800000 and policy.min_bits(policy.key(0x80000000)) == 0x80000000
    rng = np.random.default_rng(5)
    v = rng.integers(0, 2 ** 32, 4000, dtype=np.uint64).astype(U32).view(F32)
    v = v[np.isfinite(v)]
    assert np.array_equal(np.sort(v.astype(np.float64)), v[np.argsort(ME.key(v))].astype(np.float64))


@pytest.mark.parametrize("parts", [1, 2, 1024])
def test_a_fold_of_partials_gives_what_one_pass_gives(policy, parts):
    rng = np.random.default_rng(31)
    s = seeded(rng, 2600)                          # 1 024 partials: most hold two or three slots, none is empty
    s.rho[17], s.vel[900, 2], s.T[40, 3], s.ncount[::13] = np.nan, 3.0e38, np.inf, 0
    one = header_acc(policy, s)
    got = header_acc(policy, s, parts=parts)
    assert same_acc(got, one) and same_acc(got, emulated_acc(s))
    # the restatement's own fold
    a = ME.empty()
    for b in range(min(parts, 16)):
        sel = np.arange(s.n) % min(parts, 16) == b
        a = ME.merge(a, ME.particles(s.pos[sel], s.vel[sel], s.mass[sel], s.ids[sel], s.acc[sel], s.rho[sel],
                                     s.ncount[sel], -24, s.T))
    assert same_acc(a, one)
    # fewer slots than partials: the empty ones fold to nothing
    few = seeded(rng, 3)
    assert same_acc(header_acc(policy, few, parts=parts), header_acc(policy, few))


def test_the_pair_sum_is_the_scalar_passes_weights(policy):
    """S_p through the header against scalar_emulation's weights added in order, V_j == 0 skipped by selection, and
    members beyond hscaled (negative weights) included."""
    import scalar_emulation as SC
    rng = np.random.default_rng(9)
    hscaled, kernel3 = F32(0.05), F32(3.0e5)
    c = SC.Consts(hscaled, kernel3, F32(1.0), F32(0.0), True)
    seen_negative = False
    for k in (0, 1, 8, 9, 40):
        V = rng.uniform(0.5e-3, 2e-3, k).astype(F32)
        V[::5] = 0.0
        d = rng.uniform(0.0, 0.06, k).astype(F32)
        if k == 9:
            d[:] = rng.uniform(0.051, 0.06, k)       # every member beyond hscaled
        if k > 1:
            V[1] = np.inf if k == 8 else V[1]
        w = SC.weight(c, V, d)
        S = F32(0.0)
        with np.errstate(invalid="ignore", over="ignore"):
            for j in range(k):
                if V[j] != 0:
                    S = F32(S + w[j])
        got = F32(policy.pair_sum(k, ptr(V), ptr(d), float(hscaled), float(kernel3)))
        assert bits1(got) == bits1(S), k
        seen_negative |= bool(S < 0)
    assert seen_negative
    S = np.array([0.25, -3.0, np.nan, np.inf, -0.0, 7.5, -np.inf], F32)
    key, bad = np.zeros(1, U32), np.zeros(1, np.int32)
    policy.pairs(S.size, ptr(S), ptr(key), ptr(bad))
    assert (int(key[0]), int(bad[0])) == ME.pair_acc(S) == (key1(7.5), 3)
    policy.pairs(2, ptr(np.array([-3.0, -0.5], F32)), ptr(key), ptr(bad))       # negative sums only
    assert policy.max_bits(int(key[0])) == bits1(-0.5) and bad[0] == 0


# ---- refusals, rows, layout, grid -------------------------------------------------------------------------------
def test_every_refusal_text(policy):
    assert [policy.rows_check(r) for r in (-1, 0, 5)] == [b"rows must be >= 0", b"", b""]
    assert [policy.every_check(e) for e in (-3, 0, 1, 9)] == [b"every must be >= 1"] * 2 + [b"", b""]
    for q, ok in ((-65, False), (-64, True), (-24, True), (32, True), (33, False)):
        assert policy.quantum_check(q) == (b"" if ok else b"quantum_log2 must be in [-64, 32]")
    assert policy.mode_check(1) == b"" and policy.mode_check(0) == b"FULL and FULL_FAST contexts only"
    assert policy.slab_check(1) == b""
    assert policy.slab_check(0) == b"slab contexts (with neighbours, or that have exchanged) cannot keep a step monitor"
    assert policy.ports_set_check(0) == b"" and policy.ports_set_check(1) == b"a context with ports cannot keep a step monitor"
    for rows in (0, 4):
        for ne in (0, 2):
            for ns in (0, 3):
                want = b"a context with a step monitor cannot have ports" if rows and (ne or ns) else b""
                assert policy.ports_check(rows, ne, ns) == want
    assert policy.exchange_check(0) == b""
    assert policy.exchange_check(2) == \
        b"a context with a step monitor (sph_hip_record_monitor) cannot exchange with neighbouring slabs"
    for first, n, filled, ok in ((0, 0, 0, True), (0, 3, 3, True), (1, 2, 3, True), (3, 0, 3, True), (0, 4, 3, False),
                                 (2, 2, 3, False), (-1, 1, 3, False), (0, -1, 3, False), (2 ** 31 - 1, 2 ** 31 - 1, 3, False)):
        assert policy.range_check(first, n, filled) == (b"" if ok else b"the range leaves the rows filled so far")
    texts = {policy.rows_check(-1), policy.every_check(0), policy.quantum_check(99), policy.mode_check(0),
             policy.slab_check(0), policy.ports_set_check(1), policy.ports_check(1, 1, 0), policy.exchange_check(1),
             policy.range_check(0, 1, 0)}
    assert len(texts) == 9                                       # each refusal its own text


def test_the_host_calls_refuse_in_the_headers_words():
    text = open(os.path.join(CSRC, "sph_hip.hip")).read()
    body = text[text.index("int sph_hip_record_monitor("):text.index("int sph_hip_get_monitor_record(")]
    for call in ("monitor_rows_check(rows)", "monitor_every_check(every)", "monitor_quantum_check(quantum_log2)",
                 "monitor_mode_check(", "monitor_slab_check(", "monitor_ports_set_check("):
        assert re.search(r"if \(const char\* why = %s.*\) return refuse\(ctx, who, why\);" % re.escape(call), body), call
    # a refusal comes before anything is freed or replaced
    assert body.index("monitor_ports_set_check(") < body.index("stop_monitor_recording(ctx)")
    # the only wait is for the steps that may still write a recording being replaced
    assert body.count("hipStreamSynchronize") == 1 and "if (ctx->mon_dev) SPH_TRY(hipStreamSynchronize(ctx->stream));" in body
    getter = text[text.index("int sph_hip_get_monitor_record("):]
    getter = getter[:getter.index("\n}\n")]
    assert "monitor_range_check(first_row, n_rows, ctx->mon_filled)" in getter and "return ctx->mon_filled;" in getter
    ports = text[text.index("int sph_hip_set_ports("):]
    ports = ports[:ports.index("ports_restart(ctx)")]
    assert "monitor_ports_check(ctx->mon_rows, ne, ns)) return refuse(ctx, who, why);" in ports
    slab = open(os.path.join(CSRC, "slab_comm.h")).read()
    assert slab.count("if (monitor_exchange_check(ctx->mon_rows)) return refuse_monitor(ctx);") == 3
    # the recording survives set_params, set_arithmetic and uploads: none of them touches its state
    for begin, end in (("int sph_hip_set_params(", "int sph_hip_get_arithmetic("),
                       ("static int upload_impl(", "static int all_same_mass(")):
        assert "mon_" not in text[text.index(begin):text.index(end)]


def test_the_recording_rule(policy):
    for every in (1, 2, 7):
        for rows in (1, 3):
            filled = [policy.record_row(s, every, rows) for s in range(0, 30)]
            want = [(s - 1) // every if s >= 1 and (s - 1) % every == 0 and (s - 1) // every < rows else -1
                    for s in range(0, 30)]
            assert filled == want
            for r in range(rows):
                assert policy.record_row(policy.record_step(r, every), every, rows) == r
    assert [policy.record_step(r, 2) for r in range(3)] == [1, 3, 5]
    assert policy.record_row(2 ** 40 + 1, 2 ** 20, 2 ** 30) == 2 ** 20


def test_the_structs_size_and_offsets(policy):
    from smoothed_particle_hydrodynamics_amd import monitor as M
    assert policy.row_size() == 128 == ME.ROW.itemsize == M.ROW.itemsize == M.ROW_BYTES
    assert M.ROW == ME.ROW
    for i, name in enumerate(ME.ROW.names):
        assert policy.row_offset(i) == ME.ROW.fields[name][1], name
    assert policy.row_offset(len(ME.ROW.names)) == -1
    text = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    assert "typedef struct sph_hip_monitor_row {   /* field order is ABI: 128 bytes */" in text
    header = open(os.path.join(CSRC, "monitor_policy.h")).read()
    assert "static_assert(sizeof(sph_hip_monitor_row) == 128" in header


def test_the_grid_function(policy):
    assert [policy.grid(n) for n in (-5, 0, 1, 255, 256, 257, 512, 513)] == [1, 1, 1, 1, 1, 2, 2, 3]
    assert policy.grid(1024 * 256) == 1024 and policy.grid(1024 * 256 - 255) == 1024 and policy.grid(1023 * 256) == 1023
    assert policy.grid(1024 * 256 + 1) == 1024 and policy.grid(300000) == 1024 and policy.grid(2 ** 31 - 1) == 1024
    assert [policy.launches_pairs(ns, n) for ns in (0, 100) for n in (0, 100)] == [0, 0, 0, 1]
    header = open(os.path.join(CSRC, "launch_policy.h")).read()
    assert "#define MONITOR_THREADS 256" in header and "#define MONITOR_MAX_BLOCKS 1024" in header


# ---- signatures ------------------------------------------------------------------------------------------------
def test_prototypes_and_abi(policy, hiplib):
    from smoothed_particle_hydrodynamics_amd import lib as L
    assert policy.abi() == 7 and L.ABI_VERSION == 7
    V, I = C.c_void_p, C.c_int
    assert L.PROTOTYPES["sph_hip_record_monitor"] == (I, [V, I, I, I])
    assert L.PROTOTYPES["sph_hip_get_monitor_record"] == (I, [V, I, I, V, V])
    text = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    assert re.search(r"#define SPH_HIP_ABI_VERSION 7\b", text)
    section = text[text.index("---- step monitor"):text.index("int sph_hip_record_monitor(")]
    assert re.search(r"added without a change of\s+SPH_HIP_ABI_VERSION", section.replace("\n *", " "))
    assert re.search(r"\bint sph_hip_record_monitor\(sph_hip_context\* ctx, int rows, int every, int quantum_log2\);", text)
    assert re.search(r"\bint sph_hip_get_monitor_record\(sph_hip_context\* ctx, int first_row, int n_rows, "
                     r"sph_hip_monitor_row\* out,\s+int32_t\* steps\);", text)
    for name in ("record_monitor", "get_monitor_record"):
        assert hasattr(hiplib, "sph_hip_" + name)
    # a null context is refused without touching the device
    assert hiplib.sph_hip_record_monitor(None, 4, 1, -24) < 0
    assert hiplib.sph_hip_get_monitor_record(None, 0, 0, None, None) < 0
    from smoothed_particle_hydrodynamics_amd import build
    assert "monitor_kernels.h" in build.HEADERS and "monitor_policy.h" in build.HEADERS


# ---- step_impl's order, read from the text ------------------------------------------------------------------------
def test_step_impl_launches_in_order_and_nothing_without_a_recording():
    text = open(os.path.join(CSRC, "launch.h")).read()
    step = text[text.index("int step_impl("):text.index("// the six phase times")]
    assert step.index("launch_scalars(ctx)") < step.index("launch_monitor_pairs(ctx)") < step.index("launch_accel(ctx")
    assert (step.index("launch_integrate(ctx, hash_too)") < step.index("launch_monitor(ctx)")
            < step.index("return mark_phase(ctx, se, 6, st);"))
    assert step.index("fused_step_done(ctx, 1)") < step.index("launch_monitor(ctx)")
    # nothing launched without a recording, nothing behind the integrate on a step that fills no row
    assert "if (ctx->mon_rows > 0 && (rc = launch_monitor_pairs(ctx))) return rc;" in step
    assert "if (ctx->mon_row_now >= 0 && (rc = launch_monitor(ctx))) return rc;" in step
    assert step.count("launch_monitor") == 2 and step.count("mon_") == 2
    # the monitor never vetoes the fused integrate
    fused = step[step.index("const bool fused ="):step.index("launch_accel(ctx")]
    assert "mon_" not in fused
    pairs = text[text.index("int launch_monitor_pairs("):text.index("int launch_monitor(sph_hip_context")]
    assert pairs.index("if (r < 0 || !monitor_launches_pairs(ctx->n_scalars, ctx->n)) return SPH_HIP_OK;") < \
        pairs.index("hipLaunchKernelGGL")
    both = text[text.index("int launch_monitor_pairs("):text.index("// The fused acceleration pass did the rest")]
    assert "Synchronize" not in both and both.count("hipLaunchKernelGGL") == 3
    # the stand-alone phase calls do not record
    hip = open(os.path.join(CSRC, "sph_hip.hip")).read()
    assert hip.count("launch_monitor") == 0
    # the kernels take the state through pointers to const and use no atomics
    kernels = open(os.path.join(CSRC, "monitor_kernels.h")).read()
    code = "\n".join(line.split("//")[0] for line in kernels.splitlines())
    assert "atomic" not in code
    for name, writes in (("k_monitor_particles(", "MonitorAcc* __restrict__ part"),
                         ("k_monitor_pairs(", "MonitorPairAcc* __restrict__ part"),
                         ("k_monitor_finish(", "sph_hip_monitor_row* __restrict__ row")):
        sig = code[code.index(name):]
        sig = sig[:sig.index(")\n{")]
        pointers = re.findall(r"(const )?\w+\* __restrict__ \w+", sig)
        assert pointers.count("") == 1 and writes in sig, name          # everything const but the output


# ---- MonitorRecord ---------------------------------------------------------------------------------------------
class Params:
    time_step, sim_scale_inv, h = 0.004, 2.0, 0.05


def hand_made():
    from smoothed_particle_hydrodynamics_amd import monitor as M
    rows = np.zeros(4, M.ROW)
    rows["momentum"] = [[1 << 24, -(1 << 25), 0], [3 << 23, 0, 0], [0, 0, 0], [0, 0, 1]]
    rows["kinetic"] = [1 << 26, 1 << 20, 0, 5]
    rows["mass"] = [2001 << 24] * 4
    rows["v2_max"] = [4.0, 9.0, 0.25, 1.0]
    rows["a2_max"] = [100.0, 400.0, 0.0, 1.0]
    rows["s_max"] = [50.0, 80.0, 0.0, 60.0]
    rows["flags"] = [3, 3, 0, 3]
    rows["pair_bad"] = [0, 0, 0, 2]
    rows["bad_id_min"] = M.NO_ID
    return M.MonitorRecord(rows, [1, 3, 5, 7], -24)


def test_monitor_record_formulas():
    from smoothed_particle_hydrodynamics_amd import monitor as M
    rec = hand_made()
    assert len(rec) == 4 and rec.steps.tolist() == [1, 3, 5, 7] and rec.quantum == 2.0 ** -24
    assert rec.momentum.tolist() == [[1.0, -2.0, 0.0], [1.5, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 2.0 ** -24]]
    assert rec.kinetic.tolist() == [4.0, 0.0625, 0.0, 5 * 2.0 ** -24] and rec.mass.tolist() == [2001.0] * 4
    assert rec.rows["kinetic"].dtype == np.int64 and rec.v2_max.dtype == F32 and rec.pair_bad.tolist() == [0, 0, 0, 2]
    assert rec.speed_max.tolist() == [2.0, 3.0, 0.5, 1.0]
    per = 0.004 * 2.0 / 0.05
    assert np.allclose(rec.courant(Params), [2.0 * per, 3.0 * per, 0.5 * per, per], rtol=1e-15)
    assert np.allclose(rec.accel_number(Params), [10 * 0.004 * per, 20 * 0.004 * per, 0.0, 0.004 * per], rtol=1e-15)
    d = rec.diffusion_number([0.0, 1.0, 2.0, 0.5], 0.004)
    assert d.shape == (4, 4) and np.allclose(d[1], [0.0, 0.32, 0.64, 0.16], rtol=1e-15)
    assert np.isnan(d[2]).all() and not np.isnan(d[[0, 1, 3]]).any()
    assert rec.has_scalars.tolist() == [True, True, False, True] == rec.has_diffusion.tolist()
    assert rec.first_bad() == 3
    with pytest.raises(AttributeError):
        rec.no_such_field
    with pytest.raises(ValueError):
        M.MonitorRecord(np.zeros(2, M.ROW), [1])
    # first_bad looks at all three counters and finds the first
    for field in ("bad", "scalar_bad", "pair_bad"):
        rows = np.zeros(3, M.ROW)
        assert M.MonitorRecord(rows, [1, 2, 3]).first_bad() is None
        rows[field][1:] = 1
        assert M.MonitorRecord(rows, [1, 2, 3]).first_bad() == 1
    assert M.MonitorRecord(np.zeros(0, M.ROW), []).first_bad() is None


def test_suggest_time_step():
    from smoothed_particle_hydrodynamics_amd import monitor as M
    rec = hand_made()
    per_dt = 2.0 / 0.05
    by_speed = 0.25 / (3.0 * per_dt)                # 2.08e-3
    by_accel = math.sqrt(0.25 / (20.0 * per_dt))     # 1.77e-2
    assert rec.suggest_time_step(Params) == min(by_speed, by_accel) == by_speed
    by_diffusion = 0.5 / (2.0 * 80.0)                # 3.1e-3: not the tightest ...
    assert rec.suggest_time_step(Params, [0.0, 1.0, 2.0, 0.5]) == by_speed
    assert rec.suggest_time_step(Params, [0.0, 1.0, 20.0, 0.5]) == 0.5 / (20.0 * 80.0)        # ... until kappa grows
    assert rec.suggest_time_step(Params, [1.0] * 4, courant=10.0, diffusion=0.25) == 0.25 / 80.0
    # the suggestion keeps every row's numbers at or under the targets
    dt = rec.suggest_time_step(Params, [0.0, 1.0, 20.0, 0.5])

    class At:
        time_step, sim_scale_inv, h = dt, 2.0, 0.05
    assert rec.courant(At).max() <= 0.25 and rec.accel_number(At).max() <= 0.25
    assert np.nanmax(rec.diffusion_number([0.0, 1.0, 20.0, 0.5], dt)) <= 0.5 * (1 + 1e-15)
    # a large acceleration is what limits a run at rest
    rows = np.zeros(1, M.ROW)
    rows["a2_max"] = 1.0e8
    assert M.MonitorRecord(rows, [1]).suggest_time_step(Params) == math.sqrt(0.25 / (1.0e4 * per_dt))
    # nothing to go by
    assert M.MonitorRecord(np.zeros(2, M.ROW), [1, 2]).suggest_time_step(Params, [1.0] * 4) == math.inf
    assert M.MonitorRecord(np.zeros(0, M.ROW), []).suggest_time_step(Params) == math.inf


# ---- sanitizers ------------------------------------------------------------------------------------------------
MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
""" + WALK + r"""
static float uni(unsigned& s) { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f; }

int main()
{
   unsigned seed = 1234u;
   long long live = 0, bad = 0, skipped = 0, scalar_bad = 0, pair_bad = 0;
   double checksum = 0.0;
   const int counts[7] = {0, 1, 63, 64, 65, 257, 3000};
   const int parts[4] = {1, 2, 7, 1024};
   for (int rep = 0; rep < 140; rep++) {
      const int n = counts[rep % 7];
      // heap rows of exactly n entries: a walk past them is caught
      std::vector<float> pos(3 * n), vel(3 * n), acc(3 * n), mass(n), rho(n), T(4 * n), S(n);
      std::vector<uint32_t> ids(n);
      std::vector<int32_t> ncount(n);
      for (int i = 0; i < n; i++) {
         for (int a = 0; a < 3; a++) {
            pos[3 * i + a] = uni(seed);
            vel[3 * i + a] = 6.0f * uni(seed) - 3.0f;
            acc[3 * i + a] = 100.0f * uni(seed) - 50.0f;
         }
         for (int c = 0; c < 4; c++) T[4 * i + c] = 4.0f * uni(seed) - 2.0f;
         mass[i] = 0.5f + uni(seed);
         rho[i] = 500.0f + 1000.0f * uni(seed);
         ids[i] = (uint32_t)(n - 1 - i);
         ncount[i] = (int32_t)(64.0f * uni(seed));
         S[i] = 100.0f * uni(seed) - 20.0f;
      }
      if (n > 2 && rep % 3 == 0) rho[1] = __builtin_nanf("");
      if (n > 2 && rep % 5 == 0) vel[5] = 3.0e38f;
      if (n > 2 && rep % 4 == 0) T[6] = __builtin_inff();
      if (n > 2 && rep % 6 == 0) mass[2] = __builtin_inff();
      if (n > 2 && rep % 2 == 0) S[2] = -__builtin_inff();
      if (n > 2 && rep % 9 == 0) ids[0] = 0xfffffff0u;      // an id outside the rows of T
      const int q = rep % 11 == 0 ? 32 : rep % 13 == 0 ? -64 : -24;
      if (monitor_quantum_check(q)) return 6;
      const MonitorAcc a = walk(n, parts[rep % 4], pos.data(), vel.data(), mass.data(), ids.data(), acc.data(), rho.data(),
                                ncount.data(), q, rep % 8 == 7 ? nullptr : T.data(), n);
      const MonitorPairAcc p = walk_pairs(n, S.data());
      const sph_hip_monitor_row r = monitor_row_of(a, rep % 8 != 7, true, p);
      if (r.live != n) return 7;
      live += r.live;
      bad += r.bad;
      skipped += r.skipped;
      scalar_bad += r.scalar_bad;
      pair_bad += r.pair_bad;
      checksum += (double)r.v2_max + (double)r.rho_min + (double)r.s_max + (double)r.scalar_max[2] + (double)r.mass * 1e-12;
   }
   if (monitor_rows_check(0) || !monitor_rows_check(-1) || monitor_every_check(1) || !monitor_every_check(0) ||
       !monitor_quantum_check(33) || monitor_mode_check(true) || !monitor_mode_check(false) || monitor_slab_check(true) ||
       !monitor_slab_check(false) || monitor_ports_set_check(false) || !monitor_ports_set_check(true) ||
       monitor_ports_check(0, 1, 1) || !monitor_ports_check(1, 0, 1) || monitor_exchange_check(0) || !monitor_exchange_check(1) ||
       monitor_range_check(0, 2, 2) || !monitor_range_check(1, 2, 2))
      return 4;
   if (monitor_grid(0) != 1 || monitor_grid(300000) != MONITOR_MAX_BLOCKS || monitor_record_row(5, 2, 3) != 2 ||
       monitor_record_step(2, 2) != 5)
      return 5;
   printf("live %lld bad %lld skipped %lld scalar_bad %lld pair_bad %lld checksum %.6f\n", live, bad, skipped, scalar_bad,
          pair_bad, checksum);
   return live > 60000 && bad > 20 && skipped > 20 && scalar_bad > 10 && pair_bad > 20 ? 0 : 3;
}
"""


def test_new_header_code_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    src, exe = tmp_path / "monitor_main.cpp", tmp_path / "monitor_main"
    src.write_text(MAIN)
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == "", run.stderr
