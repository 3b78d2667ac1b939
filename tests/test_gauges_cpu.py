"""CPU checks of the gauges (include/sph_hip.h: sph_hip_set_gauges): the probe points and readings of
csrc/gauge_policy.h (compiled with g++ behind an extern "C" shim that walks the wave's trips the way
k_gauges_read does) against the numpy restatement tests/gauge_emulation.py bit for bit on canned probe answers,
the argument checks with every refusal text, the record arithmetic, the binding, and the Python side
(gauges.py, scenes.dam_break_gauged)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gauge_emulation as G
import sample_emulation as SE
from helpers import compile_shim

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = r"""
#include "gauge_policy.h"

extern "C" {
int sizes(int which) { return which == 0 ? (int)sizeof(sph_hip_gauge) : (int)sizeof(sph_hip_gauge_reading); }
int probes(const sph_hip_gauge* g) { return gauge_probes(*g); }
void probe_points(const sph_hip_gauge* g, float* xyz)
{
   for (int q = 0; q < gauge_probes(*g); q++) gauge_probe(*g, q, xyz[3 * q], xyz[3 * q + 1], xyz[3 * q + 2]);
}
// the wave's trips over canned densities: ballots, counts, the top, the two densities looked at again
void column(const sph_hip_gauge* g, const float* rho, sph_hip_gauge_reading* out)
{
   const int m = gauge_probes(*g), trips = gauge_trips(m);
   int n = 0, top = -1;
   for (int trip = 0; trip < trips; trip++) {
      unsigned long long mask = 0;
      for (int lane = 0; lane < GAUGE_WAVE; lane++) {
         const int q = trip * GAUGE_WAVE + lane;
         if (q < m && gauge_wet(rho[q], g->iso)) mask |= 1ull << lane;
      }
      n = gauge_count_wet(n, mask);
      top = gauge_top_wet(top, mask, trip);
   }
   const int b = gauge_column_again(top);
   *out = gauge_column_reading(*g, n, top, rho[b], b + 1 < m ? rho[b + 1] : 0.0f);
}
void column_tail(const sph_hip_gauge* g, int n, int k, float f0, float f1, sph_hip_gauge_reading* out)
{
   *out = gauge_column_reading(*g, n, k, f0, f1);
}
void section(const sph_hip_gauge* g, const float* rho, const float* va, sph_hip_gauge_reading* out)
{
   const int m = gauge_probes(*g), trips = gauge_trips(m);
   float a[GAUGE_WAVE], r[GAUGE_WAVE];
   for (int lane = 0; lane < GAUGE_WAVE; lane++) a[lane] = r[lane] = 0.0f;
   int n = 0, top = -1;
   for (int trip = 0; trip < trips; trip++) {
      unsigned long long mask = 0;
      for (int lane = 0; lane < GAUGE_WAVE; lane++) {
         const int q = trip * GAUGE_WAVE + lane;
         if (q >= m) continue;
         if (gauge_wet(rho[q], g->iso)) mask |= 1ull << lane;
         a[lane] = a[lane] + va[q];
         r[lane] = r[lane] + rho[q];
      }
      n = gauge_count_wet(n, mask);
      top = gauge_top_wet(top, mask, trip);
   }
   for (int d = 1; d < GAUGE_WAVE; d <<= 1) {
      float a2[GAUGE_WAVE], r2[GAUGE_WAVE];
      for (int lane = 0; lane < GAUGE_WAVE; lane++) {
         a2[lane] = a[lane] + a[lane ^ d];
         r2[lane] = r[lane] + r[lane ^ d];
      }
      for (int lane = 0; lane < GAUGE_WAVE; lane++) { a[lane] = a2[lane]; r[lane] = r2[lane]; }
   }
   (void)top;
   *out = gauge_section_reading(*g, n, a[0], r[0]);
}
void point(float rho, float vx, float vy, float vz, int count, sph_hip_gauge_reading* out)
{
   *out = gauge_point_reading(rho, vx, vy, vz, count);
}
const char* check(const sph_hip_gauge* list, int n) { const char* w = gauge_check(list, n); return w ? w : ""; }
long long record_bytes(int rows, int gauges) { return gauge_record_bytes(rows, gauges); }
const char* record_check(int rows, int every, int gauges)
{
   const char* w = gauge_record_check(rows, every, gauges);
   return w ? w : "";
}
int record_row(long long step, int every, int rows) { return gauge_record_row(step, every, rows); }
int record_steps_done(int row, int every) { return gauge_record_steps_done(row, every); }
const char* range_check(int first, int n, int have) { const char* w = gauge_range_check(first, n, have); return w ? w : ""; }
void constants(long long* out)
{
   out[0] = SPH_HIP_MAX_GAUGES; out[1] = SPH_HIP_MAX_GAUGE_PROBES; out[2] = SAMPLE_SCRATCH_BUDGET;
   out[3] = SPH_HIP_GAUGE_POINT; out[4] = SPH_HIP_GAUGE_COLUMN; out[5] = SPH_HIP_GAUGE_SECTION;
}
}
"""


class CGauge(C.Structure):
    _fields_ = [("kind", C.c_int32), ("axis", C.c_int32), ("origin", C.c_float * 3), ("spacing", C.c_float * 2),
                ("count", C.c_int32 * 2), ("iso", C.c_float)]


READING = np.dtype([("v", np.float32, (4,)), ("n", np.int32), ("k", np.int32)])


def c_gauge(g):
    s = CGauge()
    s.kind, s.axis, s.iso = g.kind, g.axis, float(g.iso)
    for c in range(3):
        s.origin[c] = float(g.origin[c])
    for c in range(2):
        s.spacing[c] = float(g.spacing[c])
        s.count[c] = int(g.count[c])
    return s


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    lib = compile_shim(SHIM, ["-O2", "-ffp-contract=off"], tmp_path_factory)
    V, I, F = C.c_void_p, C.c_int, C.c_float
    lib.probes.argtypes = [V]
    lib.probe_points.argtypes = [V, V]
    lib.column.argtypes = [V, V, V]
    lib.column_tail.argtypes = [V, I, I, F, F, V]
    lib.section.argtypes = [V, V, V, V]
    lib.point.argtypes = [F, F, F, F, I, V]
    lib.check.argtypes = [V, I]
    lib.record_bytes.restype = C.c_longlong
    lib.record_row.argtypes = [C.c_longlong, I, I]
    for f in (lib.check, lib.record_check, lib.range_check):
        f.restype = C.c_char_p
    for f in (lib.probe_points, lib.column, lib.column_tail, lib.section, lib.point, lib.constants):
        f.restype = None
    return lib


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def bits(a):
    return np.asarray(a, F32).view(np.uint32)


def same_reading(got, want):
    """a READING record against the restatement's (v, n, k)"""
    v, n, k = want
    return np.array_equal(bits(got["v"]), bits(v)) and int(got["n"]) == n and int(got["k"]) == k


def test_struct_sizes_and_constants(policy):
    assert policy.sizes(0) == 40 == C.sizeof(CGauge) and policy.sizes(1) == 24 == READING.itemsize
    k = (C.c_longlong * 6)()
    policy.constants(k)
    assert list(k) == [4096, 4096, 64 << 20, G.POINT, G.COLUMN, G.SECTION]


# ---- probe points ------------------------------------------------------------------------------------------
def test_probe_points_are_fp32_unfused(policy):
    cases = [G.point((0.3, 0.7, 0.11))]
    for axis in range(3):
        cases.append(G.column((0.05, 0.013, 0.5), axis, 0.0155, 129, 100.0))
        cases.append(G.section((0.131, 0.017, 0.023), axis, (0.0155, 0.031), (5, 13), 100.0))
    cases.append(G.section((0.1, 0.0, 0.0), 0, (0.0125, 0.0157), (64, 64), 1.0))
    for g in cases:
        s = c_gauge(g)
        m = policy.probes(C.byref(s))
        assert m == G.probe_count(g)
        got = np.zeros((m, 3), F32)
        policy.probe_points(C.byref(s), ptr(got))
        assert np.array_equal(bits(got), bits(G.probes_of(g))), g
    # a section's lattice is the sampler's: x fastest of the two other axes, ascending axis order
    g = G.section((0.25, 0.1, 0.2), 1, (0.5, 0.25), (2, 3), 1.0)
    want = SE.lattice_points((0.25, 0.1, 0.2), (0.5, 1.0, 0.25), (2, 1, 3)).reshape(-1, 3)
    assert np.array_equal(bits(G.probes_of(g)), bits(want))


# ---- columns -----------------------------------------------------------------------------------------------
COLUMN_SIZES = (1, 2, 63, 64, 65, 129)
ISO = F32(120.0)


def column_cases(m, rng):
    """Canned densities of a column of m probes, by name."""
    wet = (ISO + F32(1.0) + rng.random(m) * 200).astype(F32)
    dry = (rng.random(m) * float(ISO) * 0.99).astype(F32)
    cases = {"all wet": wet, "none wet": dry, "exactly iso is dry": np.full(m, ISO, F32)}
    for top in sorted({0, m // 2, m - 2, m - 1} & set(range(m))):
        a = dry.copy()
        a[:top + 1] = wet[:top + 1]
        cases["top %d" % top] = a
        b = a.copy()
        b[rng.random(m) < 0.3] = F32(0.5)          # gaps below the top
        b[top] = wet[top]
        cases["gaps below top %d" % top] = b
        c = a.copy()
        if top + 1 < m:
            c[top + 1] = ISO                        # fb == iso: t == 1 exactly, not wet
            cases["fb == iso above top %d" % top] = c
            d = a.copy()
            d[top + 1] = np.nan                     # NaN above the top: dry, t = NaN -> 0
            cases["NaN above top %d" % top] = d
    nan = wet.copy()
    nan[::3] = np.nan
    cases["NaN among wet"] = nan
    cases["all NaN"] = np.full(m, np.nan, F32)
    inf = dry.copy()
    inf[m // 2] = np.inf
    cases["an infinite density"] = inf
    return cases


@pytest.mark.parametrize("m", COLUMN_SIZES)
def test_columns_match_the_restatement_bit_for_bit(policy, m):
    rng = np.random.default_rng(100 + m)
    classes = set()
    for axis in range(3):
        g = G.column((0.05, 0.013, 0.5), axis, 0.0155, m, ISO)
        s = c_gauge(g)
        for name, rho in column_cases(m, rng).items():
            got = np.zeros(1, READING)
            policy.column(C.byref(s), ptr(rho), ptr(got))
            want = G.column_reading(g, rho)
            assert same_reading(got[0], want), (m, axis, name)
            n, k = want[1], want[2]
            classes.add("dry" if k < 0 else "saturated" if k == m - 1 else "interior")
            if n < k + 1:
                classes.add("gap")
            # what the reading means
            assert want[0][1] == F32(n) * g.spacing[0]
            if k >= 0:
                assert rho[k] > ISO and not (rho[k + 1:] > ISO).any()
            if 0 <= k < m - 1 and np.isfinite(rho[k + 1]):
                lo, hi = G.column_coord(g, k), G.column_coord(g, k + 1)
                assert lo <= want[0][0] <= hi
    assert {"dry", "saturated"} <= classes and (m < 3 or {"interior", "gap"} <= classes)


def test_column_interpolation_edge_values(policy):
    """gauge_column_reading given tops and densities no wet / dry pattern produces: fa == fb, a t below 0, above
    1, infinite and NaN - the clamp fminf(fmaxf(t, 0), 1) with NaN becoming 0."""
    g = G.column((0.05, 0.013, 0.5), 1, 0.0155, 65, ISO)
    s = c_gauge(g)
    seen = set()
    for f0, f1 in ((130.0, 130.0), (120.0, 120.0), (130.0, 140.0), (100.0, 110.0), (130.0, np.inf), (np.inf, 5.0),
                   (130.0, np.nan), (np.nan, 5.0), (130.0, 100.0), (130.0, 120.0), (110.0, 130.0), (np.inf, np.inf)):
        for k in (0, 31, 63):
            got = np.zeros(1, READING)
            policy.column_tail(C.byref(s), 7, k, f0, f1, ptr(got))
            want = G.column_tail(g, 7, k, F32(f0), F32(f1))
            assert same_reading(got[0], want), (f0, f1, k)
            raw = G.interpolate(g, k, f0, f1)[1]
            seen.add("nan" if np.isnan(raw) else "below" if raw < 0 else "above" if raw > 1 else "inside")
            lo, hi = G.column_coord(g, k), G.column_coord(g, k + 1)
            assert lo <= want[0][0] <= hi
            if np.isnan(raw):
                assert want[0][0] == lo
    assert seen == {"nan", "below", "above", "inside"}
    for k, f0, f1 in ((-1, 3.0, 9.0), (64, 150.0, 0.0)):
        got = np.zeros(1, READING)
        policy.column_tail(C.byref(s), 0 if k < 0 else 65, k, f0, f1, ptr(got))
        assert same_reading(got[0], G.column_tail(g, 0 if k < 0 else 65, k, F32(f0), F32(f1)))
    assert G.column_tail(g, 0, -1, F32(3.0), F32(9.0))[0].tolist() == [F32(0.013), 0.0, 0.0, 3.0]
    assert G.column_tail(g, 65, 64, F32(150.0), F32(0.0))[0][2:].tolist() == [150.0, 0.0]


# ---- sections ----------------------------------------------------------------------------------------------
SECTION_SHAPES = ((1, 1), (63, 1), (64, 1), (5, 13), (32, 32), (64, 64))


def numpy_butterfly(x):
    x = np.asarray(x, F32).copy()
    for d in (1, 2, 4, 8, 16, 32):
        x = x + x[np.arange(64) ^ d]
    return x


@pytest.mark.parametrize("shape", SECTION_SHAPES)
def test_sections_match_the_butterfly_bit_for_bit(policy, shape):
    m = shape[0] * shape[1]
    assert m in (1, 63, 64, 65, 1024, 4096)
    rng = np.random.default_rng(200 + m)
    g = G.section((0.131, 0.0, 0.0), 0, (0.0155, 0.031), shape, ISO)
    s = c_gauge(g)
    rho = (rng.random(m) * 300).astype(F32)
    signed = rng.normal(0.0, 50.0, m).astype(F32)
    cancel = signed.copy()
    cancel[1::2] = -cancel[::2][:len(cancel[1::2])]           # pairs that cancel: the order of the sum shows
    big = signed.copy()
    big[::7] *= F32(1e30)
    inf = signed.copy()
    inf[m // 2] = np.inf
    both = inf.copy()
    both[0] = -np.inf                                           # +inf and -inf: NaN (one probe: just -inf)
    for name, va in (("signed", signed), ("cancelling", cancel), ("huge", big), ("infinite", inf), ("both infinities", both)):
        got = np.zeros(1, READING)
        policy.section(C.byref(s), ptr(rho), ptr(va), ptr(got))
        with np.errstate(invalid="ignore", over="ignore"):
            want = G.section_reading(g, rho, va)
            # the butterfly written out here once more, on the lanes' sums
            lanes = np.zeros(64, F32)
            for q in range(m):
                lanes[q % 64] = lanes[q % 64] + va[q]
            total = numpy_butterfly(lanes)[0]
            area = F32(g.spacing[0] * g.spacing[1])
            assert np.array_equal(bits(want[0][0]), bits(total * area)), name
        assert same_reading(got[0], want), (shape, name)
        assert want[1] == int((rho > ISO).sum()) and want[2] == 0 and want[0][3] == 0
    if m > 1:
        assert np.isnan(G.section_reading(g, rho, both)[0][0]) and np.isinf(G.section_reading(g, rho, inf)[0][0])


def test_points_match_the_sampler_normalisation(policy):
    rng = np.random.default_rng(7)
    rows = [(0.0, 0.0, 0.0, 0.0, 0), (250.0, 10.0, -20.0, 30.0, 31), (-1.0, 5.0, 5.0, 5.0, 2),
            (np.nan, 1.0, 1.0, 1.0, 1), (np.inf, np.inf, 1.0, -1.0, 3), (1e-30, 1e30, -1e30, 0.0, 1)]
    rows += [tuple(rng.normal(100, 60, 4).astype(F32)) + (int(rng.integers(0, 60)),) for _ in range(200)]
    for rho, vx, vy, vz, c in rows:
        got = np.zeros(1, READING)
        policy.point(rho, vx, vy, vz, c, ptr(got))
        assert same_reading(got[0], G.point_reading(F32(rho), np.array([vx, vy, vz], F32), c)), (rho, vx, vy, vz)


# ---- checks ------------------------------------------------------------------------------------------------
def good_gauges():
    return [G.point((0.1, 0.2, 0.3)), G.column((0.05, 0.0, 0.5), 1, 0.0155, 129, ISO),
            G.section((0.131, 0.0, 0.0), 0, (0.0155, 0.031), (64, 64), ISO)]


def c_list(gauges):
    arr = (CGauge * max(1, len(gauges)))()
    for i, g in enumerate(gauges):
        arr[i] = c_gauge(g)
    return arr


def test_gauge_check_every_refusal(policy):
    good = good_gauges()
    arr = c_list(good)
    assert policy.check(arr, 3) == b"" and policy.check(None, 0) == b"" and policy.check(arr, 0) == b""
    assert policy.check(arr, -1) == b"negative count"
    many = (CGauge * 4097)()
    for i in range(4097):
        many[i] = c_gauge(good[0])
    assert policy.check(many, 4096) == b"" and policy.check(many, 4097) == b"more than SPH_HIP_MAX_GAUGES gauges"
    assert policy.check(None, 1) == b"null gauge list"

    def refused(index, **change):
        gs = list(good)
        g = gs[index]._asdict()
        for name, value in change.items():
            if isinstance(value, tuple) and name in ("origin", "spacing"):
                value = np.array(value, F32)
            g[name] = value
        gs[index] = G.Gauge(**g)
        return policy.check(c_list(gs), 3)

    for i in range(3):
        assert refused(i, kind=3) == refused(i, kind=-1) == b"unknown gauge kind"
        assert refused(i, axis=3) == refused(i, axis=-1) == b"axis must be 0, 1 or 2"
        for bad in (np.nan, np.inf, -np.inf):
            # unused fields included: a point's spacing and iso, a column's second spacing
            assert refused(i, origin=(0.1, bad, 0.3)) == b"a field that is not finite"
            assert refused(i, spacing=(bad, 0.01)) == refused(i, spacing=(0.01, bad)) == b"a field that is not finite"
            assert refused(i, iso=F32(bad)) == b"a field that is not finite"
    # a point uses no spacing, count or iso; a column only the first of each
    assert refused(0, spacing=(0.0, -1.0), count=(0, -5), iso=F32(-1.0)) == b""
    assert refused(1, spacing=(0.01, -1.0), count=(7, -5)) == b""
    assert refused(1, spacing=(0.0, 0.0)) == refused(1, spacing=(-0.01, 0.0)) == b"spacing must be > 0"
    assert refused(2, spacing=(0.01, 0.0)) == refused(2, spacing=(0.0, 0.01)) == b"spacing must be > 0"
    assert refused(1, count=(0, 0)) == refused(2, count=(4, 0)) == refused(2, count=(-1, 4)) == b"count must be >= 1"
    assert refused(1, count=(4096, 0)) == refused(2, count=(4096, 1)) == refused(2, count=(1, 4096)) == b""
    big = b"more than SPH_HIP_MAX_GAUGE_PROBES probes in one gauge"
    assert refused(1, count=(4097, 0)) == refused(2, count=(64, 65)) == refused(2, count=(2 ** 31 - 1, 2 ** 31 - 1)) == big
    assert refused(1, iso=F32(0.0)) == refused(2, iso=F32(-3.0)) == b"iso must be > 0"


def test_record_arithmetic(policy):
    assert policy.record_bytes(10, 4096) == 10 * 4096 * 24
    assert policy.record_bytes(2 ** 20, 4096) == 24 * 2 ** 32             # no 32-bit overflow
    assert policy.record_check(10, 3, 4096) == b"" and policy.record_check(0, 1, 0) == b""
    assert policy.record_check(-1, 1, 10) == b"rows must be >= 0"
    assert policy.record_check(1, 0, 10) == b"every must be >= 1"
    assert policy.record_check(1, 1, 0) == b"no gauges are set"
    # the budget: 64 MiB holds 2 796 202 readings of 24 bytes: 682 rows of 4 096 gauges, 2 796 202 rows of one
    assert (64 << 20) // 24 == 2796202
    assert policy.record_check(682, 1, 4096) == b"" and policy.record_check(683, 1, 4096) == b"the rows exceed the 64 MiB scratch budget"
    assert policy.record_check(2796202, 1, 1) == b"" and b"64 MiB" in policy.record_check(2796203, 1, 1)
    # rows=10, every=3: steps 1, 4, ..., 28 read the gauges, after 0, 3, ..., 27 steps
    rows = [policy.record_row(s, 3, 10) for s in range(0, 40)]
    assert [s for s, r in enumerate(rows) if r >= 0] == list(range(1, 29, 3))
    assert [r for r in rows if r >= 0] == list(range(10))
    assert [policy.record_steps_done(r, 3) for r in range(10)] == list(range(0, 28, 3))
    assert [policy.record_row(s, 1, 3) for s in range(1, 6)] == [0, 1, 2, -1, -1]
    assert policy.range_check(0, 0, 0) == b"" and policy.range_check(2, 3, 5) == b""
    for bad in ((-1, 1, 5), (0, -1, 5), (3, 3, 5), (2 ** 31 - 1, 2 ** 31 - 1, 5)):
        assert policy.range_check(*bad) == b"the range leaves the rows filled so far"


# ---- the restatement itself ------------------------------------------------------------------------------------
def test_restatement_on_a_still_column(hiplib):
    """The dam column at rest with every particle moving at one velocity: a column gauge through it finds the
    free surface within one probe spacing plus h of the fill height, a point gauge the sampler's answer, and a
    section's flow is its density sum times that velocity up to the rounding of the sums."""
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, _, mass = scenes.dam_break(4000)
    u = np.array([0.5, -0.25, 0.125], F32)
    vel = np.tile(u, (4000, 1)).reshape(-1)
    h = float(p.h)
    g = SE.Grid(p, pos, vel, mass)
    rho_own = g.sample(pos.reshape(-1, 3))[0]
    iso = F32(0.5) * F32(np.median(rho_own))
    gauges = [G.column((0.05, 0.0, 0.5), 1, h / 2, int(1.0 / (h / 2)) + 1, iso), G.point((0.05, 0.4, 0.5)),
              G.section((0.05, 0.0, 0.0), 0, (h / 2, h / 2), (24, 30), iso), G.column((0.6, 0.0, 0.5), 1, h / 2, 65, iso)]
    out, info = G.evaluate(p, pos, vel, mass, gauges, with_info=True)
    assert abs(float(out.v[0, 0]) - 0.75) < 1.5 * h and out.k[0] >= 0 and out.n[0] > 0.5 / (h / 2)
    rho, v, c = g.sample(np.array([[0.05, 0.4, 0.5]], F32))
    assert np.array_equal(bits(out.v[1]), bits(np.concatenate([rho, v[0]]))) and out.n[1] == c[0]
    members = G.walk(g, G.probes_of(gauges[2]))[2].sum()
    area = F32(h / 2) * F32(h / 2)
    assert out.v[2, 2] > 0 and out.n[2] > 0
    assert abs(float(out.v[2, 0]) / float(area) - float(out.v[2, 2]) * 0.5) <= float(out.v[2, 2]) * 0.5 * 2.0 ** -23 * (members + 64)
    assert out.k[3] == -1 and out.n[3] == 0 and out.v[3].tolist() == [0.0, 0.0, 0.0, 0.0]
    assert info.dry == 1 and info.interior + info.saturated == 1
    # nothing resident: zeros, columns dry at their base
    empty = G.evaluate(p, np.zeros(0, F32), np.zeros(0, F32), np.zeros(0, F32), gauges)
    assert (empty.n == 0).all() and empty.k.tolist() == [-1, 0, 0, -1] and not empty.v.any()


# ---- the Python side -------------------------------------------------------------------------------------------
def test_gauge_tuples_and_structs(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import gauges as PG
    assert C.sizeof(PG.SphGauge) == 40 and PG.READING.itemsize == 24
    assert (PG.POINT, PG.COLUMN, PG.SECTION, PG.MAX_GAUGES, PG.MAX_GAUGE_PROBES) == (0, 1, 2, 4096, 4096)
    pt = S.PointGauge((0.1, 0.2, 0.3))
    col = S.ColumnGauge((0.05, 0.0, 0.5), 1, 0.0155, 129, 120.0)
    sec = S.SectionGauge((0.131, 0.0, 0.0), 0, (0.0155, 0.031), (5, 13), 120.0)
    assert pt._fields == ("point",) and col._fields == ("base", "axis", "spacing", "samples", "iso")
    assert sec._fields == ("corner", "axis", "spacing", "shape", "iso")
    arr, n = PG.as_array([pt, col, sec])
    assert n == 3 and PG.as_array([]) == (None, 0)
    assert [arr[i].kind for i in range(3)] == [0, 1, 2] and list(arr[2].count) == [5, 13] and arr[1].count[0] == 129
    back = [PG.from_struct(arr[i]) for i in range(3)]
    assert type(back[0]) is S.PointGauge and type(back[1]) is S.ColumnGauge and type(back[2]) is S.SectionGauge
    assert back[1].samples == 129 and back[1].axis == 1 and F32(back[1].spacing) == F32(0.0155)
    assert back[2].shape == (5, 13) and back[0].point == tuple(F32(v) for v in (0.1, 0.2, 0.3))
    # the restatement reads the same fields
    for mine, theirs in zip((G.point((0.1, 0.2, 0.3)), G.column((0.05, 0.0, 0.5), 1, 0.0155, 129, 120.0),
                             G.section((0.131, 0.0, 0.0), 0, (0.0155, 0.031), (5, 13), 120.0)), (pt, col, sec)):
        got = G.of(theirs)
        assert got.kind == mine.kind and got.axis == mine.axis and got.count == mine.count and got.iso == mine.iso
        assert np.array_equal(got.origin, mine.origin) and np.array_equal(got.spacing, mine.spacing)
    rec = S.GaugeRecord(np.array([0, 3], np.int32), np.arange(24, dtype=F32).reshape(2, 3, 4), np.zeros((2, 3), np.int32),
                        np.zeros((2, 3), np.int32))
    assert rec._fields == ("steps", "v", "n", "k")
    assert rec.level(1).tolist() == [4.0, 16.0] and rec.depth(1).tolist() == [5.0, 17.0] and rec.flow(2).tolist() == [8.0, 20.0]
    rho, u = rec.probe(0)
    assert rho.tolist() == [0.0, 12.0] and u.tolist() == [[1.0, 2.0, 3.0], [13.0, 14.0, 15.0]]
    assert S.GaugeReadings(1, 2, 3)._fields == ("v", "n", "k")


def test_dam_break_gauged_scene(hiplib):
    from smoothed_particle_hydrodynamics_amd import gauges as PG
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass, gauges = scenes.dam_break_gauged(5000)
    assert pos.shape == vel.shape == (15000,) and mass.shape == (5000,)
    assert p.apply_walls == 1 and p.apply_gravity == 1 and p.gravity[1] < 0
    assert (vel.reshape(-1, 3)[:, 0] == F32(0.7)).all()
    kinds = [type(g) for g in gauges]
    assert kinds == [PG.ColumnGauge] * 4 + [PG.SectionGauge, PG.PointGauge]
    h = float(p.h)
    for g, x in zip(gauges[:4], (0.05, 0.3, 0.6, 0.9)):
        assert g.base == (x, 0.0, 0.5) and g.axis == 1 and g.spacing == 0.5 * h
        assert 1.0 - 0.5 * h < (g.samples - 1) * g.spacing <= 1.0 and g.samples <= 4096
    sec = gauges[4]
    assert sec.corner == (0.2, 0.0, 0.0) and sec.axis == 0 and sec.shape[0] * sec.shape[1] <= 4096
    assert (sec.shape[0] - 1) * sec.spacing[0] <= 1.0 < sec.shape[0] * sec.spacing[0] + 1e-6
    assert gauges[5].point == (0.05, 0.375, 0.5)
    arr, n = PG.as_array(gauges)
    assert n == 6
    # iso: about half the median density the restatement finds at the particles' own positions, rho0-free
    grid = SE.Grid(p, pos, vel, mass)
    median = float(np.median(grid.sample(pos.reshape(-1, 3))[0]))
    iso = gauges[0].iso
    assert all(g.iso == iso for g in gauges[:5]) and 0.35 * median < iso < 0.65 * median
    out = G.evaluate(p, pos, vel, mass, [G.of(g) for g in gauges])
    assert out.k[0] >= 0 and abs(float(out.v[0, 0]) - 0.75) < 1.5 * h       # the column stands 0.75 high
    assert out.k[1:4].tolist() == [-1, -1, -1] and out.n[4] == 0 and out.n[5] > 0
    # a fine scene keeps the section within a gauge's probe limit
    big = scenes.dam_break_gauged(200000)[4]
    assert big[4].shape[0] * big[4].shape[1] <= 4096 and big[0].samples <= 4096


def test_prototypes_match_the_header(hiplib):
    from smoothed_particle_hydrodynamics_amd import gauges as PG
    from smoothed_particle_hydrodynamics_amd import lib as L
    V, I, P = C.c_void_p, C.c_int, C.POINTER
    assert L.PROTOTYPES["sph_hip_set_gauges"] == (I, [V, P(PG.SphGauge), I])
    assert L.PROTOTYPES["sph_hip_get_gauges"] == (I, [V, P(PG.SphGauge), I])
    assert L.PROTOTYPES["sph_hip_read_gauges"] == (I, [V, V])
    assert L.PROTOTYPES["sph_hip_record_gauges"] == (I, [V, I, I])
    assert L.PROTOTYPES["sph_hip_get_gauge_record"] == (I, [V, I, I, V, V])
    text = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    assert re.search(r"#define SPH_HIP_ABI_VERSION 7\b", text) and L.ABI_VERSION == 7
    for name in ("set_gauges", "get_gauges", "read_gauges", "record_gauges", "get_gauge_record"):
        assert hasattr(hiplib, "sph_hip_" + name)
        assert re.search(r"\bint sph_hip_%s\(" % name, text)
    for name, value in (("GAUGE_POINT", 0), ("GAUGE_COLUMN", 1), ("GAUGE_SECTION", 2), ("MAX_GAUGES", 4096),
                        ("MAX_GAUGE_PROBES", 4096)):
        assert re.search(r"#define SPH_HIP_%s\s+%d\b" % (name, value), text)
    # a null context is refused without touching the device
    assert hiplib.sph_hip_set_gauges(None, None, 0) < 0 and hiplib.sph_hip_get_gauges(None, None, 0) < 0
    assert hiplib.sph_hip_record_gauges(None, 1, 1) < 0 and hiplib.sph_hip_read_gauges(None, None) < 0
