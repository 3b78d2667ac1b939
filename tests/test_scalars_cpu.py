"""CPU checks of the carried scalars (include/sph_hip.h: carried scalars): csrc/scalar_policy.h, compiled with g++
behind an extern "C" shim that walks one particle's candidates the way k_scalars_step's row walk does, against
the numpy restatement tests/scalar_emulation.py bit for bit; every refusal text; the layout and the binding; the
launch decisions beside the unchanged ones; a uniform field; the convexity of the explicit scheme in float64;
the header's code under the host's sanitizers; the Python side and the two scenes."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pressure_emulation as PE
import scalar_emulation as SC
from helpers import compile_shim

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smoothed_particle_hydrodynamics_amd", "csrc")

# one particle over its candidates in the order given: the membership test, the distance, the volume, the sums,
# the update and the sources, every operation through the header's functions
WALK = r"""
#include "scalar_policy.h"
#include "launch_policy.h"

static void walk(const float* consts, const float* kappa, const sph_hip_scalar_source* src, int n_src, const float* pi,
                 const float* Ti, int k, const float* pj, const float* Tj, const float* mj, const float* rhoj, float* out)
{
   ScalarStep st = {};
   st.hscaled = consts[0];
   st.kernel3 = consts[1];
   st.sim_scale = consts[2];
   st.dt = consts[4];
   const float h2 = consts[3];
   const bool unit = consts[5] != 0.0f;
   for (int c = 0; c < 4; c++) st.kappa[c] = kappa[c];
   st.n_sources = n_src;
   for (int q = 0; q < n_src; q++) st.sources[q] = src[q];
   const Scalar4 ti = {Ti[0], Ti[1], Ti[2], Ti[3]};
   Scalar4 s = {0.0f, 0.0f, 0.0f, 0.0f};
   for (int j = 0; j < k; j++) {
      const float dx = pi[0] - pj[3 * j], dy = pi[1] - pj[3 * j + 1], dz = pi[2] - pj[3 * j + 2];
      const float d2 = dx * dx + dy * dy + dz * dz;
      if (!(d2 < h2)) continue;
      const Scalar4 tj = {Tj[4 * j], Tj[4 * j + 1], Tj[4 * j + 2], Tj[4 * j + 3]};
      scalar_pair(s, ti, tj, scalar_volume(mj[j], rhoj[j]), scalar_distance(d2, st.sim_scale, unit), st.hscaled, st.kernel3);
   }
   const Scalar4 r = scalar_finish(ti, s, st, pi[0], pi[1], pi[2]);
   out[0] = r.c0; out[1] = r.c1; out[2] = r.c2; out[3] = r.c3;
}
"""

SHIM = WALK + r"""
extern "C" {
void layout(int* out)
{
   out[0] = (int)sizeof(sph_hip_scalar_source); out[1] = SPH_HIP_SCALAR_CHANNELS; out[2] = SPH_HIP_MAX_SCALAR_SOURCES;
   out[3] = SPH_HIP_SCALAR_HOLD; out[4] = SPH_HIP_SCALAR_ADD; out[5] = SPH_HIP_ABI_VERSION;
   out[6] = (int)sizeof(Scalar4); out[7] = SCALAR_ROUTE_LISTS; out[8] = SCALAR_ROUTE_ROWS;
}
void particle(const float* consts, const float* kappa, const sph_hip_scalar_source* src, int n_src, const float* pi,
              const float* Ti, int k, const float* pj, const float* Tj, const float* mj, const float* rhoj, float* out)
{
   walk(consts, kappa, src, n_src, pi, Ti, k, pj, Tj, mj, rhoj, out);
}
float shepard(float a, float rho) { return scalar_shepard(a, rho); }
static const char* text(const char* w) { return w ? w : ""; }
const char* context_check(int ports_set, int ids_changed) { return text(scalar_context_check(ports_set != 0, ids_changed != 0)); }
const char* ports_check(int n_scalars, int ne, int ns) { return text(scalar_ports_check(n_scalars, ne, ns)); }
const char* set_check(int n, const float* v, const float* k, int live) { return text(scalar_set_check(n, v, k, live)); }
const char* source_check(const sph_hip_scalar_source* list, int n) { return text(scalar_source_check(list, n)); }
const char* have_check(int n) { return text(scalar_have_check(n)); }
const char* range_check(int first, int n, int have) { return text(scalar_range_check(first, n, have)); }
// the launch decisions, the new ones and some of the unchanged ones
int launches(int n_scalars, int n) { return step_launches_scalars(n_scalars, n) ? 1 : 0; }
int wg_route(int tiled, int force_rows, unsigned flag) { return scalar_workgroup_route(tiled != 0, force_rows != 0, flag); }
int lane_route(int wg, unsigned flag, int count, unsigned first_word) { return scalar_lane_route(wg, flag, count, first_word); }
int fuse(int hash_too, int tiled, int n, int no_fused, int n_obst, int loads) { return fuse_integrate(hash_too, tiled, n, no_fused, n_obst, loads) ? 1 : 0; }
int reads_pressure(int row, int n_pressure) { return step_reads_pressure(row, n_pressure) ? 1 : 0; }
int ports_on(int ne, int ns) { return ports_active(ne, ns) ? 1 : 0; }
}
"""


class CSource(C.Structure):
    _fields_ = [("lo", C.c_float * 3), ("hi", C.c_float * 3), ("channel", C.c_int32), ("kind", C.c_int32),
                ("value", C.c_float)]


def c_sources(sources):
    arr = (CSource * max(1, len(sources)))()
    for i, q in enumerate(sources):
        for a in range(3):
            arr[i].lo[a] = float(q.lo[a])
            arr[i].hi[a] = float(q.hi[a])
        arr[i].channel, arr[i].kind, arr[i].value = int(q.channel), int(q.kind), float(q.value)
    return arr


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    lib = compile_shim(SHIM, ["-O2", "-ffp-contract=off"], tmp_path_factory)
    V, I, U, F = C.c_void_p, C.c_int, C.c_uint, C.c_float
    lib.layout.argtypes = [V]
    lib.particle.argtypes = [V, V, V, I, V, V, I, V, V, V, V, V]
    lib.layout.restype = lib.particle.restype = None
    lib.shepard.argtypes = [F, F]
    lib.shepard.restype = F
    lib.set_check.argtypes = [I, V, V, I]
    lib.source_check.argtypes = [V, I]
    lib.wg_route.argtypes = [I, I, U]
    lib.lane_route.argtypes = [I, U, I, U]
    for f in (lib.context_check, lib.ports_check, lib.set_check, lib.source_check, lib.have_check, lib.range_check):
        f.restype = C.c_char_p
    return lib


# ---- the header against the restatement ----------------------------------------------------------------------
H = F32(0.05)
KAPPAS = np.array([0.0, 0.8, 1.6, 0.8], F32)


def consts(sim_scale=1.0):
    s = F32(sim_scale)
    hs = F32(H * s)
    k3 = F32(45.0 / (np.pi * float(hs) ** 6))
    h2 = F32(H * H)
    unit = s == F32(1.0) and np.sqrt(h2) <= hs
    return SC.Consts(hs, k3, s, h2, bool(unit))


def case(rng, k, c):
    """One particle and k candidates (most of them members), with the contract's corners in the data."""
    pi = rng.uniform(0.2, 0.8, 3).astype(F32)
    pj = (pi + rng.uniform(-0.8, 0.8, (k, 3)).astype(F32) * H).astype(F32)
    Ti = rng.uniform(-1.0, 1.0, 4).astype(F32)
    Ti[0] = F32(-0.0)                                  # the carried channel (kappa = 0): the sign bit must survive
    Tj = rng.uniform(-1.0, 1.0, (k, 4)).astype(F32)
    mj = rng.uniform(0.5, 1.5, k).astype(F32)
    rhoj = rng.uniform(5e3, 2e4, k).astype(F32)
    if k > 0:
        rhoj[0] = 0.0                                  # a neighbour that contributes nothing
        Tj[0] = F32(1e30)
    if k > 3:
        rhoj[3] = -1.0
    around = (pi - H, pi + H)
    sources = [SC.hold(around[0], around[1], 1, 0.25),                  # holds
               SC.add(around[0], around[1], 2, 3.0),                    # adds value * dt
               SC.hold((pi[0], around[0][1], around[0][2]), around[1], 3, 9.0),   # the particle ON the lo face: outside
               SC.hold(around[0], (around[1][0], pi[1], around[1][2]), 3, 9.0),   # ... ON the hi face: outside
               SC.add(around[0], around[1], 1, -2.0)]                   # list order: after the HOLD of channel 1
    return pi, Ti, pj, Tj, mj, rhoj, sources


@pytest.mark.parametrize("sim_scale", [1.0, 0.5])
@pytest.mark.parametrize("k", [0, 1, 7, 8, 9, 200])
def test_header_equals_the_restatement_bit_for_bit(policy, k, sim_scale):
    c = consts(sim_scale)
    dt = F32(0.004)
    rng = np.random.default_rng(1000 + k)
    members = 0
    for rep in range(8):
        pi, Ti, pj, Tj, mj, rhoj, sources = case(rng, k, c)
        if rep % 2:
            sources = []
        want = SC.particle(c, dt, KAPPAS, sources, pi, Ti, pj, Tj, mj, rhoj)
        got = np.zeros(4, F32)
        cc = np.array([c.hscaled, c.kernel3, c.sim_scale, c.h2, dt, 1.0 if c.unit else 0.0], F32)
        policy.particle(ptr(cc), ptr(KAPPAS), c_sources(sources), len(sources), ptr(pi), ptr(Ti), k, ptr(pj),
                        ptr(np.ascontiguousarray(Tj)), ptr(mj), ptr(rhoj), ptr(got))
        assert np.array_equal(bits(got), bits(want)), (k, rep, got, want)
        # what the case is there to show
        assert bits(got)[0] == 0x80000000                                   # -0.0f carried by selection
        assert np.isfinite(got).all()                                       # the 1e30 rows of rho_j = 0 never entered
        if sources:
            assert got[1] == F32(F32(0.25) + F32(-2.0) * dt) and got[3] != F32(9.0)
        d = pi[None, :] - pj
        members += int((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2] < c.h2).sum())
    assert (members > 0) == (k > 0)
    if k >= 7:
        assert 0 < members < 8 * k          # members and non-members both


def test_a_neighbour_without_density_is_skipped_by_selection(policy):
    c = consts()
    pi = np.array([0.5, 0.5, 0.5], F32)
    pj = np.array([[0.51, 0.5, 0.5], [0.5, 0.52, 0.5]], F32)
    Ti = np.array([1.0, 1.0, 1.0, 1.0], F32)
    Tj = np.array([[np.inf, np.nan, -np.inf, 5.0], [2.0, 2.0, 2.0, 2.0]], F32)
    mj = np.ones(2, F32)
    for dead in (0.0, -3.0, np.nan):
        rhoj = np.array([dead, 1e4], F32)
        want = SC.particle(c, F32(0.004), [1.0] * 4, [], pi, Ti, pj, Tj, mj, rhoj)
        got = np.zeros(4, F32)
        cc = np.array([c.hscaled, c.kernel3, c.sim_scale, c.h2, 0.004, 1.0], F32)
        policy.particle(ptr(cc), ptr(np.ones(4, F32)), c_sources([]), 0, ptr(pi), ptr(Ti), 2, ptr(pj), ptr(Tj), ptr(mj),
                        ptr(rhoj), ptr(got))
        assert np.array_equal(bits(got), bits(want)) and np.isfinite(got).all() and (got > 1.0).all()


def test_shepard_quotient(policy):
    for a, rho in ((3.0, 2.0), (3.0, 0.0), (3.0, -1.0), (0.0, 5.0), (1.0, np.nan)):
        want = SC.PE.quotient(F32(a), F32(rho))
        assert bits(F32(policy.shepard(a, rho))) == bits(want)


# ---- refusals ------------------------------------------------------------------------------------------------
def test_every_refusal_text(policy):
    assert policy.context_check(0, 0) == b""
    assert policy.context_check(1, 0) == b"a context with ports cannot carry scalars"
    assert policy.context_check(0, 1) == b"ports have changed the particle set: upload first"
    assert policy.ports_check(0, 1, 1) == b"" and policy.ports_check(10, 0, 0) == b""
    assert policy.ports_check(10, 1, 0) == policy.ports_check(10, 0, 1) == b"a context that carries scalars cannot have ports"

    v = np.zeros((5, 4), F32)
    k = np.array([0.0, 1.0, 2.0, 1.0], F32)
    assert policy.set_check(5, ptr(v), ptr(k), 5) == b""
    assert policy.set_check(0, ptr(v), ptr(k), 5) == b"" and policy.set_check(5, None, None, 7) == b""   # off
    assert policy.set_check(-1, ptr(v), ptr(k), 5) == b"negative count"
    assert policy.set_check(4, ptr(v), ptr(k), 5) == b"n must equal the particle count"
    assert policy.set_check(5, ptr(v), None, 5) == b"null diffusivity array"
    for bad in (-1.0, np.nan, np.inf):
        kk = k.copy()
        kk[2] = bad
        assert policy.set_check(5, ptr(v), ptr(kk), 5) == b"a diffusivity that is not finite and >= 0"
    for bad in (np.nan, np.inf, -np.inf):
        vv = v.copy()
        vv[4, 3] = bad
        assert policy.set_check(5, ptr(vv), ptr(k), 5) == b"a value that is not finite"

    good = [SC.hold((0, 0, 0), (1, 1, 1), 0, 1.0), SC.add((0, 0, 0), (1, 1, 1), 3, -1.0)]
    assert policy.source_check(c_sources(good), 2) == b"" and policy.source_check(None, 0) == b""
    assert policy.source_check(c_sources(good * 4), 8) == b""
    assert policy.source_check(c_sources(good), -1) == b"negative count"
    assert policy.source_check(c_sources(good * 5), 9) == b"more than SPH_HIP_MAX_SCALAR_SOURCES sources"
    assert policy.source_check(None, 1) == b"null source list"

    def refused(**change):
        return policy.source_check(c_sources([good[0], good[1]._replace(**change)]), 2)

    assert refused(channel=-1) == refused(channel=4) == b"channel must be 0 .. 3"
    assert refused(kind=2) == refused(kind=-1) == b"unknown source kind"
    assert refused(lo=np.array([0, np.nan, 0], F32)) == b"a box that is not finite"
    assert refused(hi=np.array([1, 1, np.inf], F32)) == b"a box that is not finite"
    assert refused(lo=np.array([0, 1, 0], F32)) == b"lo must be < hi on every axis"
    assert refused(hi=np.array([-1, 1, 1], F32)) == b"lo must be < hi on every axis"
    assert refused(value=F32(np.nan)) == refused(value=F32(np.inf)) == b"a value that is not finite"

    assert policy.have_check(3) == b"" and policy.have_check(0) == b"the context carries no scalars"
    assert policy.range_check(0, 5, 5) == policy.range_check(5, 0, 5) == b""
    for first, n in ((-1, 1), (0, -1), (3, 3), (6, 0)):
        assert policy.range_check(first, n, 5) == b"the range leaves what the context holds"


def test_the_host_calls_refuse_in_the_headers_words():
    """Every check's text reaches the caller through refuse(): the entry points name the checks."""
    text = open(os.path.join(CSRC, "sph_hip.hip")).read()
    body = text[text.index("int sph_hip_set_scalars("):text.index("int sph_hip_extract_surface(")]
    for check in ("scalar_context_check", "scalar_set_check", "scalar_source_check", "scalar_have_check",
                  "scalar_range_check"):
        assert check in body
    # REF and slab contexts: the sampler's own refusals - in sph_hip_set_scalars itself, and for the two sampler
    # calls in the samplers' shared driver, which asks sample_check first and the call's own refusal next
    assert body.count("sample_check(ctx, who)") == 1
    assert body.count("scalars_refusal,") == 2 and "return scalar_have_check(ctx->n_scalars);" in body
    assert "sample_points_run(ctx, call," in body and "sample_lattice_run(ctx, call," in body
    driver = text[text.index("int sample_refusals("):text.index("int sample_zero(")]
    assert 0 < driver.index("sample_check(ctx, c.who)") < driver.index("c.refusal(ctx)")
    for run in ("int sample_points_run(", "int sample_lattice_run("):
        assert "sample_refusals(ctx, c," in text[text.index(run):text.index(run) + 600]
    ports = text[text.index("int sph_hip_set_ports("):text.index("int sph_hip_get_ports(")]
    assert "scalar_ports_check(ctx->n_scalars, ne, ns)" in ports
    upload = text[text.index("static int upload_impl("):text.index("static int all_same_mass(")]
    assert "ctx->n_scalars = 0;" in upload and "ctx->n_scalar_sources = 0;" in upload


# ---- layouts ---------------------------------------------------------------------------------------------------
def test_layout_and_binding(policy, hiplib):
    from smoothed_particle_hydrodynamics_amd import lib as L
    from smoothed_particle_hydrodynamics_amd import scalars as S
    out = np.zeros(9, np.int32)
    policy.layout(ptr(out))
    assert tuple(out) == (36, 4, 8, 0, 1, 7, 16, 0, 1)
    assert C.sizeof(S.SphScalarSource) == 36 == C.sizeof(CSource)
    for name, off in (("lo", 0), ("hi", 12), ("channel", 24), ("kind", 28), ("value", 32)):
        assert getattr(S.SphScalarSource, name).offset == off
    assert (S.CHANNELS, S.MAX_SOURCES, S.HOLD, S.ADD) == (4, 8, 0, 1) and L.ABI_VERSION == 7
    V, I, Q = C.c_void_p, C.c_int, C.POINTER
    assert L.PROTOTYPES["sph_hip_set_scalars"] == (I, [V, I, V, V])
    assert L.PROTOTYPES["sph_hip_get_scalars"] == (I, [V, I, I, V])
    assert L.PROTOTYPES["sph_hip_set_scalar_sources"] == (I, [V, Q(S.SphScalarSource), I])
    assert L.PROTOTYPES["sph_hip_get_scalar_sources"] == (I, [V, Q(S.SphScalarSource), I])
    assert L.PROTOTYPES["sph_hip_sample_scalars_points"] == (I, [V, I, V, V, V, V])
    text = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    assert re.search(r"#define SPH_HIP_ABI_VERSION 7\b", text)
    section = text[text.index("---- carried scalars"):text.index("int sph_hip_set_scalars(")]
    assert re.search(r"added without a change of\s+SPH_HIP_ABI_VERSION", section.replace("\n *", " "))
    assert "do NOT advance the" in section and "<= 1" in section
    for name in ("set_scalars", "get_scalars", "set_scalar_sources", "get_scalar_sources", "sample_scalars_points",
                 "sample_scalars_lattice"):
        assert hasattr(hiplib, "sph_hip_" + name)
        assert re.search(r"\bint sph_hip_%s\(" % name, text)
    # a null context is refused without touching the device
    assert hiplib.sph_hip_set_scalars(None, 0, None, None) < 0
    assert hiplib.sph_hip_get_scalars(None, 0, 0, None) < 0
    assert hiplib.sph_hip_set_scalar_sources(None, None, 0) < 0
    assert hiplib.sph_hip_get_scalar_sources(None, None, 0) < 0
    assert hiplib.sph_hip_sample_scalars_points(None, 0, None, None, None, None) < 0
    assert hiplib.sph_hip_sample_scalars_lattice(None, None, None, None, None, None, None) < 0


# ---- decisions -------------------------------------------------------------------------------------------------
def test_launch_decisions(policy):
    LISTS, ROWS = 0, 1
    ALL, NONE, SOME, NO_LIST = 0, 1, 2, 0xFFFFFFFF
    assert [policy.launches(ns, n) for ns, n in ((0, 0), (0, 100), (100, 0), (100, 100))] == [0, 0, 0, 1]
    # a workgroup: lists wherever the density pass left them
    assert policy.wg_route(1, 0, ALL) == LISTS and policy.wg_route(1, 0, SOME) == LISTS
    assert policy.wg_route(1, 0, NONE) == ROWS
    for flag in (ALL, NONE, SOME):
        assert policy.wg_route(0, 0, flag) == ROWS          # an untiled context has no lists
        assert policy.wg_route(1, 1, flag) == ROWS          # SPH_HIP_SCALAR_ROWS=1
    # a lane: the rows only where it carries the marker in a LISTS_SOME workgroup
    assert policy.lane_route(LISTS, SOME, 300, NO_LIST) == ROWS
    assert policy.lane_route(LISTS, SOME, 300, 0x00010002) == LISTS
    assert policy.lane_route(LISTS, SOME, 0, NO_LIST) == LISTS      # no neighbours: the word means nothing
    assert policy.lane_route(LISTS, ALL, 40, NO_LIST) == LISTS      # (two entries 0xffff cannot be valid, but ALL means all)
    assert policy.lane_route(ROWS, NONE, 40, 0) == ROWS and policy.lane_route(ROWS, ALL, 0, 0) == ROWS
    # beside the unchanged ones: scalars are no argument of any of them
    assert policy.fuse(1, 1, 100, 0, 0, 0) == 1 and policy.fuse(1, 1, 100, 0, 1, 0) == 0 and policy.fuse(1, 0, 100, 0, 0, 0) == 0
    assert policy.reads_pressure(0, 1) == 1 and policy.reads_pressure(-1, 1) == 0 and policy.reads_pressure(0, 0) == 0
    assert policy.ports_on(0, 0) == 0 and policy.ports_on(1, 0) == 1
    text = open(os.path.join(CSRC, "launch.h")).read()
    step = text[text.index("int step_impl("):text.index("// the six phase times")]
    assert step.index("launch_density(ctx)") < step.index("launch_scalars(ctx)") < step.index("launch_accel(ctx")
    assert "ctx->n_scalars > 0 && (rc = launch_scalars(ctx))" in step     # nothing launched without scalars


# ---- a uniform field, and the convexity of the scheme ----------------------------------------------------------
@pytest.fixture(scope="module")
def block(hiplib):
    """2 001 seeded particles with their densities: the GPU test's scene."""
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dam_break(2001)
    rho = PE.particle_density(p, pos, vel, mass)
    return p, pos, vel, mass, rho


def test_a_uniform_field_stays_uniform_by_bits(block):
    p, pos, vel, mass, rho = block
    T = np.empty((mass.size, 4), F32)
    T[:] = np.array([0.3, -7.25, 1e-20, 300.0], F32)
    out = SC.step(p, pos, vel, mass, rho, T, [0.0, 50.0, 100.0, 50.0])
    assert np.array_equal(bits(out), bits(T))
    assert (rho > 0).all() and SC.stability(p, pos, vel, mass, rho).max() > 0      # (the sums were not empty)


def test_the_restatement_steps_each_particle_as_the_single_particle_walk(block):
    """The vectorised step and the one-particle walk the header is pinned to agree on real neighbourhoods."""
    p, pos, vel, mass, rho = block
    rng = np.random.default_rng(5)
    T = rng.uniform(-1, 1, (mass.size, 4)).astype(F32)
    kappa = np.array([0.0, 20.0, 40.0, 20.0], F32)
    src = [SC.hold((0.0, 0.0, 0.0), (0.05, 0.3, 0.5), 1, 2.0), SC.add((0.0, 0.2, 0.0), (0.2, 0.5, 1.0), 2, 4.0)]
    out = SC.step(p, pos, vel, mass, rho, T, kappa, src)
    order = PE.canonical_order(p, pos)
    xyz = pos.reshape(-1, 3)
    c = SC.consts_of(p)
    for i in (0, 17, 1000, 2000):
        want = SC.particle(c, F32(p.time_step), kappa, src, xyz[i], T[i], xyz[order[order != i]], T[order[order != i]],
                           mass[order[order != i]], rho[order[order != i]])
        assert np.array_equal(bits(out[i]), bits(want))
    assert not np.array_equal(out[:, 1], T[:, 1]) and np.array_equal(bits(out[:, 0]), bits(T[:, 0]))


def test_the_scheme_is_convex_below_the_stability_limit(hiplib):
    """float64, a 12^3 rest lattice: with dt * kappa * max_i sum_j V_j L(d_ij) chosen from the data to be 1/2, every
    step keeps every value inside the initial [min, max]."""
    from smoothed_particle_hydrodynamics_amd.lib import default_params
    m = 12
    a = 0.02
    h = 2.1 * a                                      # ~38 lattice neighbours inside h
    cells = [int(np.ceil((m + 1) * a / (2 * h)))] * 3
    p = default_params(float(h), cells)
    ax = (0.5 + np.arange(m)) * a
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    pos = np.stack([x, y, z], -1).astype(F32).reshape(-1)
    n = m ** 3
    vel, mass = np.zeros(3 * n, F32), np.ones(n, F32)
    rho = PE.particle_density(p, pos, vel, mass)
    assert (rho > 0).all()
    S = SC.stability(p, pos, vel, mass, rho)                  # dt * sum_j V_j L
    kappa = 0.5 / S.max()
    limit = kappa * S.max()
    assert limit <= 0.5 and limit > 0.49 and S.min() > 0

    # the same formula in float64 over the same pairs
    import sample_emulation as SE
    c = SC.consts_of(p)
    grid = SE.Grid(p, pos, vel, mass)
    order = PE.canonical_order(p, pos)
    probe, idx, d2 = PE.members(grid, grid.pos, exclude_self=True)
    V = (grid.mass.astype(np.float64) / rho[order].astype(np.float64))
    w = V[idx] * float(c.kernel3) * (float(c.hscaled) - np.sqrt(d2.astype(np.float64)))
    assert (w >= 0).all() and probe.size > 30 * n // 2
    rng = np.random.default_rng(11)
    T = rng.uniform(-2.0, 3.0, n)
    lo, hi = T.min(), T.max()
    dt = float(p.time_step)
    for _ in range(25):
        s = np.bincount(probe, weights=(T[idx] - T[probe]) * w, minlength=n)
        T = T + (dt * kappa) * s
        assert T.min() >= lo - 1e-12 and T.max() <= hi + 1e-12
    assert T.max() - T.min() < 0.9 * (hi - lo)               # and it does diffuse


# ---- sanitizers ------------------------------------------------------------------------------------------------
MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
""" + WALK + r"""
static float uni(unsigned& s) { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f; }

int main()
{
   unsigned seed = 12345u;
   const float h = 0.05f;
   const float consts[6] = {h, 45.0f / (3.14159265f * h * h * h * h * h * h), 1.0f, h * h, 0.004f, 1.0f};
   const float kappa[4] = {0.0f, 0.8f, 1.6f, 0.8f};
   double checksum = 0.0;
   int accepted = 0, refused = 0;
   for (int rep = 0; rep < 400; rep++) {
      const int k = rep % 7 == 0 ? 0 : rep % 211;
      std::vector<float> pj(3 * k + 1), Tj(4 * k + 1), mj(k + 1), rhoj(k + 1);
      float pi[3], Ti[4], out[4];
      for (int a = 0; a < 3; a++) pi[a] = 0.2f + 0.6f * uni(seed);
      for (int c = 0; c < 4; c++) Ti[c] = uni(seed);
      for (int j = 0; j < k; j++) {
         for (int a = 0; a < 3; a++) pj[3 * j + a] = pi[a] + (1.6f * uni(seed) - 0.8f) * h;
         for (int c = 0; c < 4; c++) Tj[4 * j + c] = uni(seed);
         mj[j] = 0.5f + uni(seed);
         rhoj[j] = j % 13 == 0 ? 0.0f : 5e3f + 1e4f * uni(seed);
      }
      sph_hip_scalar_source src[SPH_HIP_MAX_SCALAR_SOURCES + 1];
      const int n_src = rep % (SPH_HIP_MAX_SCALAR_SOURCES + 2);
      for (int q = 0; q < SPH_HIP_MAX_SCALAR_SOURCES + 1; q++) {
         for (int a = 0; a < 3; a++) {
            src[q].lo[a] = uni(seed) - 0.5f;
            src[q].hi[a] = src[q].lo[a] + (rep % 5 == 0 && q == 1 ? 0.0f : 1.0f);
         }
         src[q].channel = rep % 11 == 0 && q == 0 ? 4 : (q + rep) % 4;
         src[q].kind = (q + rep) % 2;
         src[q].value = uni(seed);
      }
      if (scalar_source_check(src, n_src)) {
         refused++;
         continue;
      }
      accepted++;
      walk(consts, kappa, src, n_src, pi, Ti, k, pj.data(), Tj.data(), mj.data(), rhoj.data(), out);
      for (int c = 0; c < 4; c++) checksum += out[c];
      std::vector<float> values(4 * (k + 1), 0.5f);
      if (rep % 3 == 0) values[4 * k + 3] = __builtin_inff();
      if (scalar_set_check(k + 1, values.data(), kappa, k + 1 + rep % 2)) refused++;
      if (scalar_range_check(rep % 9 - 1, k, k + rep % 3)) refused++;
   }
   printf("accepted %d refused %d checksum %.6f\n", accepted, refused, checksum);
   return accepted > 100 && refused > 100 ? 0 : 3;
}
"""


def test_new_header_code_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    src, exe = tmp_path / "scalar_main.cpp", tmp_path / "scalar_main"
    src.write_text(MAIN)
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == "", run.stderr
    assert run.stdout.split()[0] == "accepted"


# ---- the Python side -------------------------------------------------------------------------------------------
def test_python_classes_and_padding():
    from smoothed_particle_hydrodynamics_amd import ScalarSource
    from smoothed_particle_hydrodynamics_amd import scalars as S
    q = ScalarSource.hold((0, 0.1, 0.2), (1, 2, 3), 2, 0.75)
    a = ScalarSource.add((0, 0, 0), (1, 1, 1), 0, -4.0)
    assert (q.kind, a.kind) == (S.HOLD, S.ADD) and q != a
    arr, n = S.as_array([q, a])
    assert n == 2 and S.from_struct(arr[0]) == q and S.from_struct(arr[1]) == a and hash(S.from_struct(arr[0])) == hash(q)
    assert S.as_array([]) == (None, 0) and "channel=2" in repr(q)
    v = S.pad_values(np.arange(3.0))
    assert v.shape == (3, 4) and v.dtype == F32 and (v[:, 0] == [0, 1, 2]).all() and not v[:, 1:].any()
    v = S.pad_values(np.ones((5, 3)))
    assert v.shape == (5, 4) and (v[:, :3] == 1).all() and not v[:, 3].any()
    with pytest.raises(ValueError):
        S.pad_values(np.ones((5, 5)))
    assert (S.pad_diffusivity(2.0) == 2.0).all() and S.pad_diffusivity(2.0).shape == (4,)
    assert tuple(S.pad_diffusivity([0.0, 3.0])) == (0.0, 3.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        S.pad_diffusivity(np.ones(5))


def test_the_scenes(hiplib):
    from smoothed_particle_hydrodynamics_amd import scalars as S
    from smoothed_particle_hydrodynamics_amd import scenes
    n = 3000
    p, pos, vel, mass, values, kappa, sources = scenes.heated_floor(n)
    assert values.shape == (n, 4) and not values.any() and kappa[0] > 0 and not kappa[1:].any()
    assert p.apply_gravity == 1 and p.apply_walls == 1 and not vel.any()
    assert len(sources) == 1 and sources[0].kind == S.HOLD and sources[0].channel == 0 and sources[0].value == 1.0
    y = pos.reshape(-1, 3)[:, 1]
    inside = (y > sources[0].lo[1]) & (y < sources[0].hi[1])
    assert 0 < inside.sum() < n // 2 and sources[0].lo[0] < 0 and sources[0].hi[0] > p.max_x
    # the diffusivity it picks keeps the step convex in this very state
    rho = PE.particle_density(p, pos, vel, mass)
    worst = float(kappa[0]) * SC.stability(p, pos, vel, mass, rho).max()
    assert 0.05 < worst <= 1.0, worst

    p, pos, vel, mass, values, kappa = scenes.dam_break_dyed(n)
    assert values.shape == (n, 4) and not kappa.any() and set(np.unique(values[:, 0])) == {0.0, 1.0}
    assert abs(values[:, 0].mean() - 0.5) < 0.05 and not values[:, 1:].any()
    x = pos.reshape(-1, 3)[:, 0]
    assert x[values[:, 0] == 1].max() < x[values[:, 0] == 0].min()
    assert (vel.reshape(-1, 3)[:, 0] == F32(0.7)).all()
