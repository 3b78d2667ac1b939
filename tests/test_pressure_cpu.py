"""CPU checks of the pressure readings (include/sph_hip.h: pressure readings): the restatement's particle densities
against the oracle's FULL density pass; the readings of csrc/gauge_policy.h (compiled with g++ behind an
extern "C" shim that walks the wave's trips the way k_gauges_pressure does) against the numpy restatement
tests/pressure_emulation.py bit for bit on canned probe answers; the argument checks with every refusal text; the
host's decisions; the layout; an analytic anchor; the Python side and scenes.dam_break_sensors; and the classes
the GPU test's sensors must show."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gauge_emulation as G
import pressure_emulation as P
import sample_emulation as SE
from helpers import compile_shim, to_oracle_params

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = r"""
#include "gauge_policy.h"
#include "launch_policy.h"

extern "C" {
int sizes(int which) { return which == 0 ? (int)sizeof(sph_hip_gauge) : (int)sizeof(sph_hip_gauge_reading); }
void constants(long long* out)
{
   out[0] = SPH_HIP_GAUGE_PRESSURE; out[1] = SPH_HIP_GAUGE_PRESSURE_PATCH; out[2] = SPH_HIP_ABI_VERSION;
   out[3] = GAUGE_LAUNCH_FIELD; out[4] = GAUGE_LAUNCH_PRESSURE; out[5] = GAUGE_DENSITY_OF_STEP; out[6] = GAUGE_DENSITY_OWN;
}
int probes(const sph_hip_gauge* g) { return gauge_probes(*g); }
int field_probes(const sph_hip_gauge* g) { return gauge_field_probes(*g); }
int pressure_probes(const sph_hip_gauge* g) { return gauge_pressure_probes(*g); }
void probe_points(const sph_hip_gauge* g, float* xyz)
{
   for (int q = 0; q < gauge_probes(*g); q++) gauge_probe(*g, q, xyz[3 * q], xyz[3 * q + 1], xyz[3 * q + 2]);
}
float particle_pressure(float rho, float rho0, float stiffness) { return gauge_particle_pressure(rho, rho0, stiffness); }
float quotient(float pw, float rho) { return gauge_pressure_quotient(pw, rho); }
void point(float rho, float pw, int count, sph_hip_gauge_reading* out) { *out = gauge_pressure_reading(rho, pw, count); }
// the wave's trips over canned sums: a lane without a probe walks nothing (zero sums) and is not wet
void patch(const sph_hip_gauge* g, const float* rho, const float* pw, sph_hip_gauge_reading* out)
{
   const int m = gauge_pressure_probes(*g), trips = gauge_trips(m);
   float a[GAUGE_WAVE], r[GAUGE_WAVE];
   for (int lane = 0; lane < GAUGE_WAVE; lane++) a[lane] = r[lane] = 0.0f;
   int n = 0;
   for (int trip = 0; trip < trips; trip++) {
      unsigned long long mask = 0;
      for (int lane = 0; lane < GAUGE_WAVE; lane++) {
         const int q = trip * GAUGE_WAVE + lane;
         const bool has = q < m;
         const float s_rho = has ? rho[q] : 0.0f, s_pw = has ? pw[q] : 0.0f;
         const bool wet = has && gauge_wet(s_rho, g->iso);
         if (wet) mask |= 1ull << lane;
         gauge_patch_add(wet, s_rho, s_pw, a[lane], r[lane]);
      }
      n = gauge_count_wet(n, mask);
   }
   for (int d = 1; d < GAUGE_WAVE; d <<= 1) {
      float a2[GAUGE_WAVE], r2[GAUGE_WAVE];
      for (int lane = 0; lane < GAUGE_WAVE; lane++) {
         a2[lane] = a[lane] + a[lane ^ d];
         r2[lane] = r[lane] + r[lane ^ d];
      }
      for (int lane = 0; lane < GAUGE_WAVE; lane++) { a[lane] = a2[lane]; r[lane] = r2[lane]; }
   }
   *out = gauge_patch_reading(*g, n, a[0], r[0]);
}
const char* check(const sph_hip_gauge* list, int n) { const char* w = gauge_check(list, n); return w ? w : ""; }
// the host's decisions
int is_pressure(int kind) { return gauge_is_pressure(kind) ? 1 : 0; }
int read_by(int kind) { return gauge_read_by(kind); }
void set_counts(const sph_hip_gauge* list, int n, int* out) { gauge_set_counts(list, n, out); }
int set_has_pressure(const sph_hip_gauge* list, int n) { return gauge_set_has_pressure(list, n) ? 1 : 0; }
int launch_field(int n) { return gauges_launch_field(n) ? 1 : 0; }
int launch_pressure(int n) { return gauges_launch_pressure(n) ? 1 : 0; }
int density_source(int behind) { return gauge_density_source(behind != 0); }
int step_reads(int row, int n_pressure) { return step_reads_pressure(row, n_pressure) ? 1 : 0; }
int record_row(long long step, int every, int rows) { return gauge_record_row(step, every, rows); }
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


def c_list(gauges):
    arr = (CGauge * max(1, len(gauges)))()
    for i, g in enumerate(gauges):
        arr[i] = c_gauge(g)
    return arr


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    lib = compile_shim(SHIM, ["-O2", "-ffp-contract=off"], tmp_path_factory)
    V, I, F = C.c_void_p, C.c_int, C.c_float
    for f in (lib.probes, lib.field_probes, lib.pressure_probes):
        f.argtypes = [V]
    lib.probe_points.argtypes = [V, V]
    lib.particle_pressure.argtypes = [F, F, F]
    lib.quotient.argtypes = [F, F]
    lib.particle_pressure.restype = lib.quotient.restype = F
    lib.point.argtypes = [F, F, I, V]
    lib.patch.argtypes = [V, V, V, V]
    lib.check.argtypes = [V, I]
    lib.check.restype = C.c_char_p
    lib.set_counts.argtypes = [V, I, V]
    lib.set_has_pressure.argtypes = [V, I]
    lib.record_row.argtypes = [C.c_longlong, I, I]
    for f in (lib.probe_points, lib.point, lib.patch, lib.constants, lib.set_counts):
        f.restype = None
    return lib


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def bits(a):
    return np.asarray(a, F32).view(np.uint32)


def same_reading(got, want):
    v, n, k = want
    return np.array_equal(bits(got["v"]), bits(v)) and int(got["n"]) == n and int(got["k"]) == k


# ---- layout ------------------------------------------------------------------------------------------------
def test_layout_kinds_and_abi(policy):
    assert policy.sizes(0) == 40 == C.sizeof(CGauge) and policy.sizes(1) == 24 == READING.itemsize
    k = (C.c_longlong * 7)()
    policy.constants(k)
    assert list(k) == [P.PRESSURE, P.PRESSURE_PATCH, 7, 0, 1, 0, 1] and (P.PRESSURE, P.PRESSURE_PATCH) == (4, 5)
    text = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    assert re.search(r"#define SPH_HIP_ABI_VERSION 7\b", text)
    assert re.search(r"#define SPH_HIP_GAUGE_PRESSURE\s+4\b", text) and re.search(r"#define SPH_HIP_GAUGE_PRESSURE_PATCH\s+5\b", text)
    assert not re.search(r"#define SPH_HIP_GAUGE_\w+\s+3\b", text)
    for name in ("sample_pressure_points", "sample_pressure_lattice"):
        assert re.search(r"\bint sph_hip_%s\(" % name, text)
    assert "no pressure reading" not in text


# ---- particle densities --------------------------------------------------------------------------------------
def test_particle_densities_equal_the_oracles_full_density():
    """The restatement's rho_j on a small seeded scene, three states running, equal the oracle's FULL density pass
    bit for bit - and the pressures (rho_j - rho0) * stiffness have both signs once rho0 is the median."""
    from oracle.oracle import Oracle, build
    from smoothed_particle_hydrodynamics_amd import scenes
    build(ref=False)
    orc = Oracle()
    p, pos, vel, mass = scenes.dam_break(3000, speed=4.0)
    p.rho0 = float(np.median(P.particle_density(p, pos, vel, mass)))
    op = to_oracle_params(p)
    pos, vel = pos.copy(), vel.copy()
    for s in range(3):
        mine = P.particle_density(p, pos, vel, mass)
        ref = orc.step(op, pos, vel, mass, mode="full")           # (advances pos and vel)
        assert np.array_equal(bits(mine), bits(ref["rho"])), "state %d" % s
        pr = P.particle_pressure(p, mine)
        assert (pr > 0).any() and (pr < 0).any()


def test_particle_pressure_and_quotient(policy):
    rng = np.random.default_rng(5)
    rho = np.concatenate([(rng.random(200) * 3e5).astype(F32), np.array([0.0, -0.0, np.inf, np.nan, 3e38, 1e-40], F32)])
    for rho0, k in ((0.1, 0.001), (2.3e5, 0.001), (1000.0, 3.0), (0.0, 0.0), (3e38, 3e38)):
        class Prm:
            pass
        Prm.rho0, Prm.stiffness = rho0, k
        want = P.particle_pressure(Prm, rho)
        got = np.array([policy.particle_pressure(float(r), rho0, k) for r in rho], F32)
        assert np.array_equal(bits(got), bits(want))
    pw = np.array([1.5, -2.5, 0.0, np.inf, -np.inf, np.nan, 3e38, 7.0, 7.0, 7.0, 7.0, 7.0], F32)
    rh = np.array([3.0, 7.0, 2.0, 2.0, 2.0, 2.0, 1e-3, 0.0, -0.0, np.nan, -1.0, np.inf], F32)
    got = np.array([policy.quotient(float(a), float(b)) for a, b in zip(pw, rh)], F32)
    assert np.array_equal(bits(got), bits(P.quotient(pw, rh)))
    assert got[7:11].tolist() == [0.0, 0.0, 0.0, 0.0] and got[11] == 0.0 and np.isnan(got[5]) and np.isinf(got[6])


# ---- the point reading -----------------------------------------------------------------------------------------
def test_point_reading_matches_the_restatement(policy):
    cases = [(120.5, 3000.25, 17), (120.5, -3000.25, 17), (0.0, 0.0, 0), (0.0, 5.0, 3), (-0.0, 5.0, 3), (np.nan, 5.0, 2),
             (5.0, np.nan, 2), (np.inf, 5.0, 1), (5.0, np.inf, 1), (5.0, -np.inf, 1), (1e-38, 3e38, 9), (-3.0, 6.0, 4)]
    seen = set()
    for rho, pw, count in cases:
        got = np.zeros(1, READING)
        policy.point(rho, pw, count, ptr(got))
        want = P.point_reading(F32(rho), F32(pw), count)
        assert same_reading(got[0], want), (rho, pw, count)
        v = want[0]
        assert bits(v[1]) == bits(F32(rho)) and bits(v[2]) == bits(F32(pw)) and v[3] == 0.0
        if not rho > 0:
            assert bits(v[0]) == bits(F32(0.0))      # zero, negative zero, negative and NaN densities: +0
            seen.add("zeroed")
    assert "zeroed" in seen


# ---- patches -----------------------------------------------------------------------------------------------------
ISO = F32(120.0)
PATCH_SHAPES = ((1, 1), (7, 9), (8, 8), (5, 13), (32, 32), (64, 64))      # 1, 63, 64, 65, 1 024 and 4 096 probes


def patch_cases(m, rng):
    """Canned (rho, pw) of a patch of m probes, by name."""
    wet = (ISO + F32(1.0) + rng.random(m) * 200).astype(F32)
    dry = (rng.random(m) * float(ISO) * 0.99).astype(F32)
    pw = ((rng.random(m) - 0.5) * 4e4).astype(F32)
    mixed = np.where(rng.random(m) < 0.5, wet, dry).astype(F32)
    cases = {"all wet": (wet, pw), "none wet": (dry, pw), "exactly iso is dry": (np.full(m, ISO, F32), pw),
             "partly wet": (mixed, pw)}
    # pressures of both signs that cancel: pairs +x, -x over one density
    flat = np.full(m, F32(200.0))
    cancel = np.zeros(m, F32)
    half = m // 2
    cancel[:half] = (rng.random(half) * 1e4 + 1).astype(F32)
    cancel[half:2 * half] = -cancel[:half]
    cases["cancelling"] = (flat, cancel)
    for name, bad in (("huge", F32(3e38)), ("inf", F32(np.inf)), ("-inf", F32(-np.inf)), ("nan", F32(np.nan))):
        w = pw.copy()
        w[::5] = bad
        if name == "huge":
            w[1::5] = F32(-3e38)
        cases["%s pressure sums among wet" % name] = (wet, w)
        cases["%s pressure sums among dry" % name] = (dry, w)
        cases["%s pressure sums, partly wet" % name] = (mixed, w)
    r = wet.copy()
    r[::3] = np.nan
    cases["NaN densities are dry"] = (r, pw)
    r = dry.copy()
    r[m // 2] = np.inf
    cases["an infinite density is wet"] = (r, pw)
    return cases


@pytest.mark.parametrize("shape", PATCH_SHAPES)
def test_patches_match_the_restatement_bit_for_bit(policy, shape):
    m = shape[0] * shape[1]
    rng = np.random.default_rng(300 + m)
    classes = set()
    for axis in range(3):
        g = P.patch((0.131, 0.017, 0.023), axis, (0.0155, 0.031), shape, ISO)
        s = c_gauge(g)
        assert policy.probes(C.byref(s)) == policy.pressure_probes(C.byref(s)) == m and policy.field_probes(C.byref(s)) == 0
        for name, (rho, pw) in patch_cases(m, rng).items():
            got = np.zeros(1, READING)
            policy.patch(C.byref(s), ptr(rho), ptr(pw), ptr(got))
            want = P.patch_reading(g, rho, pw)
            assert same_reading(got[0], want), (shape, axis, name)
            v, n, k = want
            with np.errstate(invalid="ignore"):
                wet = rho > ISO
            assert n == int(wet.sum()) and k == 0
            area = F32(g.spacing[0] * g.spacing[1])
            assert bits(v[1]) == bits(F32(n) * area)
            classes.add("full" if n == m else "dry" if n == 0 else "partial")
            if n == 0:
                # nothing is divided, nothing was added: the mean, the force and the density sum are +0
                assert bits(v[2]) == bits(F32(0.0)) and bits(v[0]) == bits(F32(0.0) * area) and bits(v[3]) == bits(F32(0.0))
            elif name in ("all wet", "partly wet"):
                # what the reading means: the mean of the wet probes' pressures, the force that mean times the area
                pr = P.quotient(pw, rho)[wet].astype(np.float64)
                assert abs(float(v[2]) - pr.mean()) <= 1e-4 * np.abs(pr).max()
                assert abs(float(v[0]) - pr.sum() * float(area)) <= 1e-4 * np.abs(pr).sum() * float(area)
            if name == "cancelling" and m > 1:
                assert abs(float(v[2])) <= 1e-3 * 1e4 / 200.0
            if "among dry" in name:
                assert n == 0 and not np.isnan(v).any()          # a dry probe adds nothing, whatever its sums
            if name == "nan pressure sums among wet":
                assert np.isnan(v[0]) and np.isnan(v[2]) and not np.isnan(v[3])
    assert {"full", "dry"} <= classes and (m == 1 or "partial" in classes)


def test_patch_probes_are_the_sections(policy):
    for axis in range(3):
        g = P.patch((0.131, 0.017, 0.023), axis, (0.0155, 0.031), (5, 13), ISO)
        sec = G.section((0.131, 0.017, 0.023), axis, (0.0155, 0.031), (5, 13), ISO)
        s = c_gauge(g)
        got = np.zeros((65, 3), F32)
        policy.probe_points(C.byref(s), ptr(got))
        assert np.array_equal(bits(got), bits(G.probes_of(sec))) and np.array_equal(bits(got), bits(P.probes_of(g)))
    g = P.point((0.3, 0.7, 0.11))
    s = c_gauge(g)
    got = np.zeros((1, 3), F32)
    policy.probe_points(C.byref(s), ptr(got))
    assert policy.probes(C.byref(s)) == 1 and np.array_equal(bits(got[0]), bits(g.origin))


# ---- gauge_check -------------------------------------------------------------------------------------------------
def good_gauges():
    return [P.point((0.1, 0.2, 0.3)), P.patch((0.131, 0.0, 0.0), 0, (0.0155, 0.031), (64, 64), ISO),
            G.column((0.05, 0.0, 0.5), 1, 0.0155, 129, ISO)]


def test_gauge_check_takes_the_new_kinds_and_refuses_with_its_own_texts(policy):
    good = good_gauges()
    assert policy.check(c_list(good), 3) == b""

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
        assert refused(i, kind=3) == refused(i, kind=-1) == refused(i, kind=6) == b"unknown gauge kind"
    for i in range(2):
        assert refused(i, axis=3) == refused(i, axis=-1) == b"axis must be 0, 1 or 2"
        for bad in (np.nan, np.inf, -np.inf):
            # unused fields included: a point's spacing and iso
            assert refused(i, origin=(0.1, bad, 0.3)) == b"a field that is not finite"
            assert refused(i, spacing=(bad, 0.01)) == refused(i, spacing=(0.01, bad)) == b"a field that is not finite"
            assert refused(i, iso=F32(bad)) == b"a field that is not finite"
    # a pressure point uses no spacing, count or iso
    assert refused(0, spacing=(0.0, -1.0), count=(0, -5), iso=F32(-1.0)) == b""
    assert refused(1, spacing=(0.01, 0.0)) == refused(1, spacing=(-0.5, 0.01)) == b"spacing must be > 0"
    assert refused(1, count=(4, 0)) == refused(1, count=(-1, 4)) == b"count must be >= 1"
    assert refused(1, count=(4096, 1)) == refused(1, count=(1, 4096)) == b""
    big = b"more than SPH_HIP_MAX_GAUGE_PROBES probes in one gauge"
    assert refused(1, count=(64, 65)) == refused(1, count=(2 ** 31 - 1, 2 ** 31 - 1)) == big
    own = b"a pressure patch's iso must be > 0"
    assert refused(1, iso=F32(0.0)) == refused(1, iso=F32(-3.0)) == own
    assert refused(2, iso=F32(0.0)) == b"iso must be > 0"           # the other kinds keep their text
    texts = {b"unknown gauge kind", b"axis must be 0, 1 or 2", b"a field that is not finite", b"spacing must be > 0",
             b"count must be >= 1", big, own, b"iso must be > 0"}
    assert len(texts) == 8


# ---- the host's decisions ------------------------------------------------------------------------------------------
def test_host_decisions(policy):
    # which launch reads which gauge
    assert [policy.is_pressure(k) for k in (-1, 0, 1, 2, 3, 4, 5, 6)] == [0, 0, 0, 0, 0, 1, 1, 0]
    assert [policy.read_by(k) for k in (0, 1, 2, 4, 5)] == [0, 0, 0, 1, 1]
    field = [G.point((0.1, 0.2, 0.3)), G.column((0.05, 0.0, 0.5), 1, 0.0155, 129, ISO),
             G.section((0.131, 0.0, 0.0), 0, (0.0155, 0.031), (5, 13), ISO)]
    pres = good_gauges()[:2]
    for g, m in zip(field, (1, 129, 65)):
        s = c_gauge(g)
        assert policy.probes(C.byref(s)) == policy.field_probes(C.byref(s)) == m and policy.pressure_probes(C.byref(s)) == 0
    for g, m in zip(pres, (1, 4096)):
        s = c_gauge(g)
        assert policy.probes(C.byref(s)) == policy.pressure_probes(C.byref(s)) == m and policy.field_probes(C.byref(s)) == 0
    # whether a set holds a pressure kind, and how many gauges each launch reads
    out = (C.c_int * 2)()
    for gs, want in ((field, (3, 0)), (pres, (0, 2)), (field + pres, (3, 2)), ([], (0, 0)), ([pres[1]] + field, (3, 1))):
        policy.set_counts(c_list(gs), len(gs), out)
        assert tuple(out) == want
        assert policy.set_has_pressure(c_list(gs), len(gs)) == int(want[1] > 0)
        # a set without a pressure kind launches what it always launched: k_gauges_read alone
        assert policy.launch_field(want[0]) == int(want[0] > 0) and policy.launch_pressure(want[1]) == int(want[1] > 0)
    # where the density comes from: the step's own pass behind it, the context's buffer everywhere else
    assert policy.density_source(1) == 0 and policy.density_source(0) == 1
    # a step reads pressure gauges only where it fills a row and the set holds a pressure kind
    assert [policy.step_reads(r, n) for r, n in ((-1, 0), (-1, 3), (0, 0), (0, 1), (7, 2))] == [0, 0, 0, 1, 1]
    # the unchanged record arithmetic decides the row: rows=10, every=3
    rows = [policy.record_row(s, 3, 10) for s in range(0, 40)]
    assert [s for s, r in enumerate(rows) if r >= 0] == list(range(1, 29, 3))
    assert [policy.step_reads(r, 1) for r in rows].count(1) == 10


# ---- anchor: Shepard reproduces a constant ----------------------------------------------------------------------------
def test_shepard_reproduces_a_constant_pressure():
    """A cubic lattice block with spacing a = 2^-4 and a < h < a * sqrt(2): every coordinate and every difference of
    two is exact in fp32, and a particle's neighbours are its 6 lattice neighbours at d2 = a^2 exactly.  Every
    interior particle (one lattice step or more inside the block) therefore sums six IDENTICAL terms - the sum of
    equal values does not depend on their order - and all interior particles share one density rho_i bit for bit,
    hence one pressure P = (rho_i - rho0) * stiffness.

    For a probe whose members are all interior, with c = count members and u = 2^-24:
        pw   = sum of t_j * P: one rounding per product, (1 + d) with |d| <= u, and one per addition of the
               c - 1 later terms, all of the sign of P: |pw - P * T| <= (1 + (c - 1)) u |P| T to first order,
               T the exact sum of the t_j
        rho  = sum of t_j, all positive: c - 1 additions: |rho - T| <= (c - 1) u T
        pw / rho: one more rounding
    so |pressure / P - 1| <= (c + (c - 1) + 1) u = 2 c u to first order; (2 c + 2) u covers the second-order
    terms (c <= 16 here: (2 c u)^2 < 4e-12 is far below u).  Checked for P > 0 and P < 0."""
    from smoothed_particle_hydrodynamics_amd import scenes
    a, h, side = 2.0 ** -4, 0.08, 12
    assert a < h < a * np.sqrt(2.0)
    p = scenes.default_params(h, [6, 6, 6])
    assert float(p.max_x) > (side + 1) * a
    i = np.arange(side)
    z, y, x = np.meshgrid(i, i, i, indexing="ij")
    ijk = np.stack([x, y, z], -1).reshape(-1, 3)
    pos = ((ijk + 1).astype(F32) * F32(a)).astype(F32)
    vel = np.zeros_like(pos)
    mass = np.ones(len(pos), F32)
    rho = P.particle_density(p, pos, vel, mass)
    interior = ((ijk >= 1) & (ijk <= side - 2)).all(1)
    shared = rho[interior]
    assert interior.sum() == (side - 2) ** 3 and (bits(shared) == bits(shared)[0]).all() and shared[0] > 0
    assert (rho[~interior] < shared[0]).all()
    grid = SE.Grid(p, pos, vel, mass)
    order = P.canonical_order(p, pos)
    rng = np.random.default_rng(11)
    lo, hi = 2 * a + h, (side - 1) * a - h
    deep = ((ijk >= 2) & (ijk <= side - 3)).all(1)          # probes on particles: their six neighbours are interior too
    probes = np.concatenate([(lo + rng.random((400, 3)) * (hi - lo)).astype(F32), pos[deep][::17]])
    probe, idx, _ = P.members(grid, probes)
    assert interior[order][idx].all()                       # every member of every probe is interior
    checked = set()
    for rho0 in (0.25 * float(shared[0]), 4.0 * float(shared[0])):
        p.rho0, p.stiffness = rho0, 0.75
        want = float(P.particle_pressure(p, shared[:1])[0])          # the fp32 value the members carry
        got, r, count = P.sample(p, pos, vel, mass, probes)
        assert (count > 0).all() and count.max() >= 2 and count.max() <= 16
        err = np.abs(got.astype(np.float64) / want - 1.0)
        assert (err <= (2.0 * count + 2.0) * 2.0 ** -24).all(), float((err / ((2.0 * count + 2.0) * 2.0 ** -24)).max())
        checked.add(np.sign(want))
    assert checked == {1.0, -1.0}


# ---- the Python side ------------------------------------------------------------------------------------------------
def test_python_classes_round_trip(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import gauges as PG
    from smoothed_particle_hydrodynamics_amd import lib as L
    assert (PG.PRESSURE, PG.PRESSURE_PATCH) == (4, 5) and C.sizeof(PG.SphGauge) == 40 and L.ABI_VERSION == 7
    pt = S.PressureGauge((0.1, 0.2, 0.3))
    pa = S.PressurePatch((0.131, 0.0, 0.0), 0, (0.0155, 0.031), (5, 13), 120.0)
    assert pt._fields == ("point",) and pa._fields == ("corner", "axis", "spacing", "shape", "iso")
    arr, n = PG.as_array([pt, pa, S.PointGauge((0.5, 0.5, 0.5))])
    assert n == 3 and [arr[i].kind for i in range(3)] == [4, 5, 0] and list(arr[1].count) == [5, 13]
    back = [PG.from_struct(arr[i]) for i in range(3)]
    assert type(back[0]) is S.PressureGauge and type(back[1]) is S.PressurePatch and type(back[2]) is S.PointGauge
    assert back[0].point == tuple(F32(v) for v in (0.1, 0.2, 0.3)) and back[1].shape == (5, 13) and back[1].axis == 0
    assert F32(back[1].iso) == F32(120.0) and back[1].spacing == tuple(F32(v) for v in (0.0155, 0.031))
    unknown = PG.SphGauge()
    unknown.kind = 3
    with pytest.raises(ValueError, match="unknown"):
        PG.from_struct(unknown)
    # the restatement reads the same fields
    for mine, theirs in ((P.point((0.1, 0.2, 0.3)), pt), (P.patch((0.131, 0.0, 0.0), 0, (0.0155, 0.031), (5, 13), 120.0), pa)):
        got = G.of(theirs)
        assert got.kind == mine.kind and got.axis == mine.axis and got.count == mine.count and got.iso == mine.iso
        assert np.array_equal(got.origin, mine.origin) and np.array_equal(got.spacing, mine.spacing)
    # the series helpers
    v = np.arange(24, dtype=F32).reshape(2, 3, 4)
    rec = S.GaugeRecord(np.array([0, 3], np.int32), v, np.zeros((2, 3), np.int32), np.zeros((2, 3), np.int32))
    assert rec._fields == ("steps", "v", "n", "k") and rec.kinds is None
    with pytest.raises(ValueError, match="kinds"):
        rec.pressure(0)
    assert rec.pressure(0, pt).tolist() == [0.0, 12.0] and rec.pressure(1, pa).tolist() == [6.0, 18.0]
    assert rec.pressure(1, PG.PRESSURE_PATCH).tolist() == [6.0, 18.0] and rec.force(1).tolist() == [4.0, 16.0]
    rec.kinds = (4, 5, 0)
    assert rec.pressure(0).tolist() == [0.0, 12.0] and rec.pressure(1).tolist() == [6.0, 18.0]
    with pytest.raises(ValueError, match="not a pressure gauge"):
        rec.pressure(2)
    now = S.GaugeReadings(v[0], np.zeros(3, np.int32), np.zeros(3, np.int32))
    now.kinds = (4, 5, 0)
    assert now._fields == ("v", "n", "k") and now.pressure(0) == 0.0 and now.pressure(1) == 6.0 and now.force(1) == 4.0
    # the bindings
    V, I, Pt = C.c_void_p, C.c_int, C.POINTER
    assert L.PROTOTYPES["sph_hip_sample_pressure_points"] == (I, [V, I, V, V, V, V])
    assert L.PROTOTYPES["sph_hip_sample_pressure_lattice"] == (I, [V, Pt(C.c_float * 3), Pt(C.c_float * 3), Pt(C.c_int32 * 3),
                                                                   V, V, V])
    for name in ("sample_pressure_points", "sample_pressure_lattice"):
        assert hasattr(hiplib, "sph_hip_" + name)
    assert hiplib.sph_hip_sample_pressure_points(None, 0, None, None, None, None) < 0
    assert hasattr(S.SPH, "samplePressure") and hasattr(S.SPH, "samplePressureLattice")


def test_dam_break_sensors_scene(hiplib):
    from smoothed_particle_hydrodynamics_amd import gauges as PG
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass, gauges = scenes.dam_break_sensors(5000)
    q, qpos, qvel, qmass, gauged = scenes.dam_break_gauged(5000)
    # dam_break_gauged's surging dam
    assert np.array_equal(pos, qpos) and np.array_equal(vel, qvel) and np.array_equal(mass, qmass)
    assert bytes(p) == bytes(q) and p.apply_walls == 1 and p.apply_gravity == 1
    assert (vel.reshape(-1, 3)[:, 0] == F32(0.7)).all()
    kinds = [type(g) for g in gauges]
    assert kinds == [PG.PressureGauge] * 16 + [PG.PressurePatch] * 2
    h = float(p.h)
    box = (float(p.max_x), float(p.max_y), float(p.max_z))           # the walls the simulation keeps
    assert all(1.0 <= b < 1.0 + 2.0 * h for b in box)
    # a line of points up the downstream wall on the mid-plane
    ys = [g.point[1] for g in gauges[:16]]
    assert all(g.point[0] == box[0] and g.point[2] == 0.5 for g in gauges[:16])
    assert ys == sorted(ys) and 0.0 < ys[0] and ys[-1] <= box[1] and len(set(ys)) == 16
    # one patch over the lower part of that wall, one on the floor under the column
    wall, floor = gauges[16], gauges[17]
    assert wall.axis == 0 and wall.corner == (box[0], 0.0, 0.0)
    assert floor.axis == 1 and floor.corner == (0.0, 0.0, 0.0)
    for g, extent in ((wall, (0.25 * box[1], box[2])), (floor, (0.1, 1.0))):
        assert g.shape[0] * g.shape[1] <= 4096 and g.spacing[0] == g.spacing[1] > 0
        for a in range(2):
            assert (g.shape[a] - 1) * g.spacing[a] <= extent[a] < g.shape[a] * g.spacing[a] + 1e-6
        pts = P.probes_of(G.of(g))
        assert (pts >= 0).all() and (pts <= np.array(box, F32)).all()           # inside the box
    assert (P.probes_of(G.of(wall))[:, 0] == F32(box[0])).all() and (P.probes_of(G.of(floor))[:, 1] == 0).all()
    # iso is formed as dam_break_gauged forms it: about half the median density at the particles' own positions
    iso = wall.iso
    assert iso == floor.iso == gauged[0].iso
    median = float(np.median(SE.Grid(p, pos, vel, mass).sample(pos.reshape(-1, 3))[0]))
    assert 0.35 * median < iso < 0.65 * median
    arr, n = PG.as_array(gauges)
    assert n == 18
    out = P.evaluate(p, pos, vel, mass, [G.of(g) for g in gauges])
    assert not out.n[:17].any() and out.n[17] > 0 and out.v[17, 2] > 0          # the column stands on the floor patch only
    big = scenes.dam_break_sensors(200000)[4]
    assert all(g.shape[0] * g.shape[1] <= 4096 for g in big[16:])


# ---- the classes the GPU test's sensors must show ----------------------------------------------------------------------
def test_the_gpu_sensors_show_every_class_on_the_cpu():
    """tests/test_gpu_pressure.py's scene stepped by the oracle, read by the restatement alone: every class occurs
    within the 31 states, and the figures written into that file are these."""
    import test_gpu_pressure as T
    assert T.cpu_figures() == T.CPU_FIGURES
