"""CPU checks of buoyancy (include/sph_hip.h: buoyancy): csrc/buoyancy_policy.h, compiled with g++ behind an
extern "C" shim that walks rows the way k_buoyancy_apply does, against the numpy restatement
tests/buoyancy_emulation.py bit for bit; weightlessness through the oracle's integrate; every refusal text; the
layout and the binding; the launch decisions beside the unchanged ones; the Python side and the two scenes; the two
scenes stepped on the restatement; the header's code under the host's sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import buoyancy_emulation as BE
import scalar_emulation as SC
from helpers import compile_shim

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smoothed_particle_hydrodynamics_amd", "csrc")

# rows in the order given, every operation through the header's functions: what one lane of the kernel does
WALK = r"""
#include "buoyancy_policy.h"
#include "launch_policy.h"

static int walk(const sph_hip_buoyancy* b, int n, const float* Ts, float* acc, float* vel, float dt, float cfl_limit,
                float cfl_limit2)
{
   int touched = 0;
   for (int p = 0; p < n; p++) {
      const Scalar4 t = {Ts[4 * p], Ts[4 * p + 1], Ts[4 * p + 2], Ts[4 * p + 3]};
      const float s = buoyancy_excess(*b, t);
      if (!buoyancy_acts(s)) continue;
      touched++;
      buoyancy_apply(*b, s, dt, cfl_limit, cfl_limit2, acc[3 * p], acc[3 * p + 1], acc[3 * p + 2], vel[3 * p],
                     vel[3 * p + 1], vel[3 * p + 2]);
   }
   return touched;
}
"""

SHIM = WALK + r"""
#include <stddef.h>
extern "C" {
void layout(int* out)
{
   out[0] = (int)sizeof(sph_hip_buoyancy); out[1] = (int)offsetof(sph_hip_buoyancy, beta);
   out[2] = (int)offsetof(sph_hip_buoyancy, reference); out[3] = (int)offsetof(sph_hip_buoyancy, gravity);
   out[4] = SPH_HIP_ABI_VERSION; out[5] = SPH_HIP_SCALAR_CHANNELS;
}
int rows(const sph_hip_buoyancy* b, int n, const float* Ts, float* acc, float* vel, float dt, float cfl_limit, float cfl_limit2)
{
   return walk(b, n, Ts, acc, vel, dt, cfl_limit, cfl_limit2);
}
static const char* text(const char* w) { return w ? w : ""; }
const char* set_check(const sph_hip_buoyancy* b, int n_scalars) { return text(buoyancy_set_check(b, n_scalars)); }
int is_off(const sph_hip_buoyancy* b) { return buoyancy_is_off(b) ? 1 : 0; }
// the launch decisions: the new one, and fuse_integrate in its three call forms
int launches(int have, int n_scalars, int n) { return step_launches_buoyancy(have != 0, n_scalars, n) ? 1 : 0; }
int launches_scalars(int n_scalars, int n) { return step_launches_scalars(n_scalars, n) ? 1 : 0; }
int fuse5(int hash_too, int tiled, int n, int no_fused, int n_obst) { return fuse_integrate(hash_too, tiled, n, no_fused, n_obst) ? 1 : 0; }
int fuse6(int hash_too, int tiled, int n, int no_fused, int n_obst, int loads) { return fuse_integrate(hash_too, tiled, n, no_fused, n_obst, loads) ? 1 : 0; }
int fuse7(int hash_too, int tiled, int n, int no_fused, int n_obst, int loads, int buoyancy)
{
   return fuse_integrate(hash_too, tiled, n, no_fused, n_obst, loads, buoyancy) ? 1 : 0;
}
}
"""


class CBuoyancy(C.Structure):
    _fields_ = [("beta", C.c_float * 4), ("reference", C.c_float * 4), ("gravity", C.c_float * 3)]


def c_setting(b):
    out = CBuoyancy()
    for c in range(4):
        out.beta[c] = float(b.beta[c])
        out.reference[c] = float(b.reference[c])
    for a in range(3):
        out.gravity[a] = float(b.gravity[a])
    return out


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


class P:
    """the three parameters apply() reads"""

    def __init__(self, dt, cfl_limit):
        self.time_step = F32(dt)
        self.cfl_limit = F32(cfl_limit)
        self.cfl_limit2 = F32(F32(cfl_limit) * F32(cfl_limit))


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    lib = compile_shim(SHIM, ["-O2", "-ffp-contract=off"], tmp_path_factory)
    V, I, F = C.c_void_p, C.c_int, C.c_float
    lib.layout.argtypes = [V]
    lib.layout.restype = None
    lib.rows.argtypes = [V, I, V, V, V, F, F, F]
    lib.set_check.argtypes = [V, I]
    lib.set_check.restype = C.c_char_p
    lib.is_off.argtypes = [V]
    return lib


def header_rows(policy, b, p, Ts, acc, vel):
    a, v = np.ascontiguousarray(acc, F32).copy(), np.ascontiguousarray(vel, F32).copy()
    cb = c_setting(b)
    touched = policy.rows(C.byref(cb), Ts.shape[0], ptr(np.ascontiguousarray(Ts, F32)), ptr(a), ptr(v),
                          float(p.time_step), float(p.cfl_limit), float(p.cfl_limit2))
    return a, v, touched


# ---- the header against the restatement ----------------------------------------------------------------------
def seeded_rows(rng, n, b):
    """n rows with the contract's corners in the first ones."""
    Ts = rng.uniform(-2.0, 2.0, (n, 4)).astype(F32)
    acc = rng.uniform(-30.0, 30.0, (n, 3)).astype(F32)
    vel = rng.uniform(-3.0, 3.0, (n, 3)).astype(F32)
    Ts[0:4] = b.reference                     # s == 0 exactly: rows 0 .. 3 are left alone ...
    acc[0] = [-0.0, 0.0, -0.0]                # ... and keep their -0.0f's
    vel[1] = [0.0, -0.0, -0.0]
    acc[2, 1] = np.nan                        # (and whatever else they hold)
    Ts[4, 1] = np.nan                         # non-finite channels: untouched
    Ts[5, 0] = np.inf
    Ts[6, 3] = -np.inf
    Ts[7] = [np.inf, -np.inf, 0.0, 0.0]       # inf - inf
    return Ts, acc.reshape(-1), vel.reshape(-1)


SETTINGS = {
    "two_channels": BE.setting([0.31, -0.07, 0.0, 0.0], [0.25, 1.5, 0.0, 0.0], [0.0, -9.81, 0.0]),
    "one_channel": BE.setting([0.0, 0.0, 0.45, 0.0], [9.0, 9.0, -0.5, 9.0], [0.3, -9.81, 1.7]),   # zero on all but one
    "all_channels": BE.setting([0.11, -0.23, 0.37, 2.0], [0.1, 0.2, 0.3, 0.4], [1.0, 2.0, -3.0]),
}


@pytest.mark.parametrize("name", list(SETTINGS))
@pytest.mark.parametrize("cfl_limit", [10000.0, 12.0])
def test_header_equals_the_restatement_bit_for_bit(policy, name, cfl_limit):
    b = SETTINGS[name]
    p = P(0.004, cfl_limit)
    n = 600
    Ts, acc, vel = seeded_rows(np.random.default_rng(2024), n, b)
    if cfl_limit < 100.0:
        # rows whose a alone already sits at the limit: what accel_end's clamp left
        at = BE.clamp(acc.reshape(-1, 3)[20:40] * F32(100.0), p.cfl_limit, p.cfl_limit2)
        acc.reshape(-1, 3)[20:40] = at
    want_a, want_v, on = BE.apply(p, b, Ts, acc, vel)
    got_a, got_v, touched = header_rows(policy, b, p, Ts, acc, vel)
    assert np.array_equal(bits(got_a), bits(want_a)) and np.array_equal(bits(got_v), bits(want_v))
    assert touched == int(on.sum())
    # what the rows are there to show: rows 0 .. 7 keep every bit, the others move
    assert not on[:8].any() and on[8:].all()
    assert np.array_equal(bits(got_a)[:24], bits(acc)[:24]) and np.array_equal(bits(got_v)[:24], bits(vel)[:24])
    assert bits(got_a)[0] == 0x80000000 and bits(got_v)[4] == 0x80000000
    assert (bits(got_v.reshape(-1, 3)[8:]) != bits(vel.reshape(-1, 3)[8:])).any(1).all()
    # the clamp: with the default limit nothing is clamped; with the lowered one a + b is on some rows and not on others
    s = BE.excess(b, Ts)[on]
    total = acc.reshape(-1, 3)[on] + (-s)[:, None] * b.gravity[None, :]
    over = ((total[:, 0] * total[:, 0] + total[:, 1] * total[:, 1]) + total[:, 2] * total[:, 2]) > p.cfl_limit2
    if cfl_limit < 100.0:
        assert over.sum() > 50 and (~over).sum() > 5
        length = np.linalg.norm(want_a.reshape(-1, 3)[on][over].astype(np.float64), axis=1)
        assert np.abs(length / cfl_limit - 1.0).max() < 1e-6
        before = np.linalg.norm(acc.reshape(-1, 3)[20:40].astype(np.float64), axis=1)
        assert np.abs(before / cfl_limit - 1.0).max() < 1e-6          # the rows that came in at the limit
    else:
        assert not over.any()


def test_the_rows_tell_a_fused_multiply_add_from_a_multiply_and_an_add(policy):
    """v + b * dt and s + beta * (T - reference), evaluated with the product kept exact (float64 holds the product
    of two float32 exactly), differ from the unfused values on many of the seeded rows: a translation unit built
    without -ffp-contract=off on a machine with FMA would fail the comparison above."""
    b = SETTINGS["all_channels"]
    p = P(0.004, 10000.0)
    Ts, acc, vel = seeded_rows(np.random.default_rng(2024), 600, b)
    s = BE.excess(b, Ts)
    fused_s = np.zeros(600, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(4):
            d = (Ts[:, c] - b.reference[c]).astype(F32)
            fused_s = (fused_s.astype(np.float64) + np.float64(b.beta[c]) * d.astype(np.float64)).astype(F32)
    ok = BE.acts(s)
    assert (bits(fused_s[ok]) != bits(s[ok])).sum() > 20
    _, want_v, on = BE.apply(p, b, Ts, acc, vel)
    bb = ((-s[on])[:, None] * b.gravity[None, :]).astype(F32)
    fused_v = (vel.reshape(-1, 3)[on].astype(np.float64) + bb.astype(np.float64) * np.float64(p.time_step)).astype(F32)
    assert (bits(fused_v) != bits(want_v.reshape(-1, 3)[on])).sum() > 20
    got_a, got_v, _ = header_rows(policy, b, p, Ts, acc, vel)
    assert np.array_equal(bits(got_v), bits(want_v))


# ---- weightlessness --------------------------------------------------------------------------------------------
def test_a_particle_with_excess_one_is_weightless(oracle, policy):
    """s = 1 and a = gravity: a' is exactly zero, and the oracle's integrate gives nv = (v - g*dt) + g*dt bit for bit
    (its position moves by exactly vh = v - g*dt)."""
    op = oracle.params_for_h(0.05, (10, 10, 10))
    op.central_mass = 0.0
    op.apply_gravity, op.apply_walls = 1, 0
    g = np.array([0.7, -9.81, 0.013], F32)
    for a in range(3):
        op.gravity[a] = g[a]
    dt = F32(op.time_step)
    n = 64
    rng = np.random.default_rng(8)
    b = BE.setting([0.5, 0.0, 0.0, 0.25], [1.0, 0.0, 0.0, -1.0], g)
    Ts = rng.uniform(-1.0, 1.0, (n, 4)).astype(F32)
    Ts[:, 0], Ts[:, 3] = 2.0, 1.0                      # 0.5 * (2 - 1) + 0.25 * (1 - -1) = 1 exactly
    assert (BE.excess(b, Ts) == 1.0).all()
    pos = rng.uniform(0.1, 0.4, 3 * n).astype(F32)
    vel = rng.uniform(-2.0, 2.0, 3 * n).astype(F32)
    acc = np.tile(g, n).astype(F32)
    for apply in (lambda: BE.apply(op, b, Ts, acc, vel)[:2], lambda: header_rows(policy, b, op, Ts, acc, vel)[:2]):
        a2, v2 = apply()
        assert not bits(a2).any()                       # +0.0f in every component
        x, v = pos.copy(), np.ascontiguousarray(v2).copy()
        oracle.integrate(op, x, v, np.ascontiguousarray(a2), np.ones(n, F32))
        gdt = (g * dt).astype(F32)
        vh = (vel.reshape(-1, 3) - gdt[None, :]).astype(F32)
        want_v = (vh + gdt[None, :]).astype(F32)
        assert np.array_equal(bits(v), bits(want_v.reshape(-1)))
        want_x = pos.reshape(-1, 3) + vh * F32(dt * F32(op.sim_scale_inv))
        assert np.array_equal(bits(x), bits(want_x.astype(F32).reshape(-1)))


# ---- refusals ------------------------------------------------------------------------------------------------
def test_every_refusal_text(policy):
    good = c_setting(SETTINGS["two_channels"])
    assert policy.set_check(C.byref(good), 100) == b"" and policy.is_off(C.byref(good)) == 0
    assert policy.set_check(C.byref(good), 0) == b"the context carries no scalars"
    # off: never refused, scalars or not, whatever reference and gravity hold
    assert policy.set_check(None, 0) == b"" and policy.is_off(None) == 1
    off = c_setting(BE.setting([0.0, -0.0, 0.0, 0.0], [np.nan] * 4, [np.inf] * 3))
    assert policy.set_check(C.byref(off), 0) == b"" and policy.is_off(C.byref(off)) == 1
    for bad in (np.nan, np.inf, -np.inf):
        for c in range(4):
            q = c_setting(SETTINGS["two_channels"])
            q.beta[c] = bad
            assert policy.set_check(C.byref(q), 100) == policy.set_check(C.byref(q), 0) == b"a beta that is not finite"
            q = c_setting(SETTINGS["two_channels"])
            q.reference[c] = bad
            assert policy.set_check(C.byref(q), 100) == b"a reference that is not finite"
        for a in range(3):
            q = c_setting(SETTINGS["two_channels"])
            q.gravity[a] = bad
            assert policy.set_check(C.byref(q), 100) == b"a gravity that is not finite"


def test_the_host_calls_refuse_in_the_headers_words():
    text = open(os.path.join(CSRC, "sph_hip.hip")).read()
    body = text[text.index("int sph_hip_set_buoyancy("):text.index("int sph_hip_get_buoyancy(")]
    assert 'buoyancy_set_check(b, ctx->n_scalars)) return refuse(ctx, "sph_hip_set_buoyancy", why)' in body
    assert "hipStreamSynchronize" not in body and "hipDeviceSynchronize" not in body      # the setter does not wait
    upload = text[text.index("static int upload_impl("):text.index("static int all_same_mass(")]
    assert "ctx->have_buoyancy = 0;" in upload
    off = text[text.index("int sph_hip_set_scalars("):text.index("int sph_hip_get_scalars(")]
    assert "ctx->have_buoyancy = 0;" in off


# ---- layouts ---------------------------------------------------------------------------------------------------
def test_layout_and_binding(policy, hiplib):
    from smoothed_particle_hydrodynamics_amd import lib as L
    from smoothed_particle_hydrodynamics_amd import scalars as S
    out = np.zeros(6, np.int32)
    policy.layout(ptr(out))
    assert tuple(out) == (44, 0, 16, 32, 7, 4)
    assert C.sizeof(S.SphBuoyancy) == 44 == C.sizeof(CBuoyancy)
    for name, off in (("beta", 0), ("reference", 16), ("gravity", 32)):
        assert getattr(S.SphBuoyancy, name).offset == off
    assert L.ABI_VERSION == 7
    V, I, Q = C.c_void_p, C.c_int, C.POINTER
    assert L.PROTOTYPES["sph_hip_set_buoyancy"] == (I, [V, Q(S.SphBuoyancy)])
    assert L.PROTOTYPES["sph_hip_get_buoyancy"] == (I, [V, Q(S.SphBuoyancy)])
    text = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    assert re.search(r"#define SPH_HIP_ABI_VERSION 7\b", text)
    section = text[text.index("---- buoyancy"):text.index("int sph_hip_set_buoyancy(")]
    assert re.search(r"added without a change of\s+SPH_HIP_ABI_VERSION", section.replace("\n *", " "))
    assert "do NOT apply" in section and "one step early" in section and "44 bytes" in section
    scalars = text[text.index("---- carried scalars"):text.index("int sph_hip_set_scalars(")]
    assert "no buoyancy" not in scalars and "(buoyancy, below)" in scalars
    for name in ("set_buoyancy", "get_buoyancy"):
        assert hasattr(hiplib, "sph_hip_" + name)
        assert re.search(r"\bint sph_hip_%s\(" % name, text)
    # a null context is refused without touching the device
    assert hiplib.sph_hip_set_buoyancy(None, None) < 0
    assert hiplib.sph_hip_get_buoyancy(None, None) < 0


# ---- decisions -------------------------------------------------------------------------------------------------
def test_launch_decisions(policy):
    cases = [(have, ns, n) for have in (0, 1) for ns in (0, 100) for n in (0, 100)]
    assert [policy.launches(*c) for c in cases] == [0, 0, 0, 0, 0, 0, 0, 1]
    assert [policy.launches_scalars(ns, n) for ns, n in ((0, 0), (0, 100), (100, 0), (100, 100))] == [0, 0, 0, 1]
    # fuse_integrate: the old call forms give their old answers, and buoyancy switches the fused route off
    for hash_too in (0, 1):
        for tiled in (0, 1):
            for n in (0, 100):
                for no_fused in (0, 1):
                    for n_obst in (0, 2):
                        old = int(bool(hash_too and tiled and n > 0 and not no_fused and n_obst == 0))
                        assert policy.fuse5(hash_too, tiled, n, no_fused, n_obst) == old
                        for loads in (0, 1):
                            old6 = int(bool(old and not loads))
                            assert policy.fuse6(hash_too, tiled, n, no_fused, n_obst, loads) == old6
                            assert policy.fuse7(hash_too, tiled, n, no_fused, n_obst, loads, 0) == old6
                            assert policy.fuse7(hash_too, tiled, n, no_fused, n_obst, loads, 1) == 0
    assert policy.fuse5(1, 1, 100, 0, 0) == 1
    text = open(os.path.join(CSRC, "launch.h")).read()
    step = text[text.index("int step_impl("):text.index("// the six phase times")]
    assert (step.index("launch_scalars(ctx)") < step.index("launch_accel(ctx") < step.index("launch_buoyancy(ctx)")
            < step.index("launch_integrate(ctx"))
    assert "if (buoyant && (rc = launch_buoyancy(ctx))) return rc;" in step       # nothing launched without it
    assert "loads_pending(ctx), buoyant);" in step
    # the stand-alone phase calls do not apply it
    hip = open(os.path.join(CSRC, "sph_hip.hip")).read()
    assert hip.count("launch_buoyancy(") == 0 and text.count("launch_buoyancy(ctx)") == 1


# ---- the Python side -------------------------------------------------------------------------------------------
def test_python_classes():
    from smoothed_particle_hydrodynamics_amd import Buoyancy
    from smoothed_particle_hydrodynamics_amd import scalars as S
    b = Buoyancy(0.25)
    assert b.beta == (0.25, 0.0, 0.0, 0.0) and b.reference == (0.0,) * 4 and b.gravity is None
    with pytest.raises(ValueError):
        b.to_struct()
    g = b.with_gravity((0.0, -9.81, 0.0))
    assert g.gravity == tuple(float(F32(x)) for x in (0.0, -9.81, 0.0)) and g.beta == b.beta and g != b
    assert g.with_gravity((1.0, 2.0, 3.0)) is g                      # its own gravity stands
    q = Buoyancy([0.1, -0.2], [1.0, 2.0, 3.0], (0.0, 0.0, -1.0))
    s = q.to_struct()
    assert C.sizeof(s) == 44 and tuple(s.beta) == q.beta and tuple(s.reference) == q.reference
    assert tuple(s.gravity) == (0.0, 0.0, -1.0)
    assert S.buoyancy_from_struct(s) == q and hash(S.buoyancy_from_struct(s)) == hash(q) and "beta=" in repr(q)
    with pytest.raises(ValueError):
        Buoyancy(np.ones(5))
    assert BE.of(q).beta.dtype == F32 and tuple(BE.of(q).gravity) == (0.0, 0.0, -1.0)


def test_the_scenes(hiplib):
    from smoothed_particle_hydrodynamics_amd import scalars as S
    from smoothed_particle_hydrodynamics_amd import scenes
    n = 3000
    base = scenes.heated_floor(n)
    p, pos, vel, mass, values, kappa, sources, b = scenes.thermal_plume(n)
    for got, want in zip((pos, vel, mass, values, kappa), base[1:6]):
        assert np.array_equal(got, want)                               # heated_floor's still tank
    assert bytes(p) == bytes(base[0])
    assert len(sources) == 1 and sources[0].kind == S.HOLD and sources[0].channel == 0 and sources[0].value == 1.0
    slab, plate = base[6][0], sources[0]
    assert (plate.lo[1], plate.hi[1]) == (slab.lo[1], slab.hi[1])      # as thick as the slab ...
    for a in (0, 2):                                                   # ... shrunk to the middle of the floor
        assert slab.lo[a] < 0 < plate.lo[a] < plate.hi[a] < (p.max_x, 0, p.max_z)[a] < slab.hi[a]
        assert abs(0.5 * (plate.lo[a] + plate.hi[a]) - 0.5 * (p.max_x, 0, p.max_z)[a]) < 1e-6
    xyz = pos.reshape(-1, 3)
    inside = ((xyz > np.array(plate.lo, F32)) & (xyz < np.array(plate.hi, F32))).all(1)
    assert 20 < inside.sum() < n // 10
    assert isinstance(b, S.Buoyancy) and b.beta[0] > 0 and not any(b.beta[1:]) and not any(b.reference)
    assert b.gravity == tuple(p.gravity) and b.gravity[1] < 0

    p, pos, vel, mass, values, kappa, sources, b = scenes.lock_exchange(n)
    assert np.array_equal(pos, base[1]) and not vel.any() and sources == [] and not kappa.any()
    assert p.apply_gravity == 1 and p.apply_walls == 1
    assert set(np.unique(values[:, 0])) == {0.0, 1.0} and not values[:, 1:].any()
    x = pos.reshape(-1, 3)[:, 0]
    assert x[values[:, 0] == 1].max() < 0.5 * p.max_x <= x[values[:, 0] == 0].min()
    assert 0.3 < values[:, 0].mean() < 0.7
    assert b.beta[0] < 0 and not any(b.beta[1:]) and b.gravity == tuple(p.gravity)
    # no existing scene function changed its output
    again = scenes.heated_floor(n)
    assert all(np.array_equal(a, c) for a, c in zip(base[1:6], again[1:6])) and base[6] == again[6]


# ---- physics on the restatement --------------------------------------------------------------------------------
STEPS = 100


def run_scene(orc, scene, beta):
    """STEPS steps of the restatement with the scene's buoyancy at `beta` on channel 0 (0: none); (pos, T)."""
    p, pos, vel, mass, T, kappa, sources, b = scene
    src = [SC.Source(np.array(q.lo, F32), np.array(q.hi, F32), q.channel, q.kind, F32(q.value)) for q in sources]
    bb = None if beta == 0.0 else BE.setting([beta], b.reference, b.gravity)
    for _ in range(STEPS):
        out = BE.step(orc, p, pos, vel, mass, T, kappa, src, bb)
        pos, vel, T = out["pos"], out["vel"], out["T"]
    assert np.isfinite(pos).all() and np.isfinite(vel).all() and np.isfinite(T).all()
    return pos, T, int(out["touched"].sum())


@pytest.mark.parametrize("name", ["lock_exchange", "thermal_plume"])
def test_the_marked_fluid_moves_the_way_of_the_force(oracle, hiplib, name):
    """About 3 000 particles, 100 steps.  The marked particles - the salty half; the particles the run without
    buoyancy ends warmer than a quarter of the plate's temperature - end higher or lower on average than in the same
    run with beta = 0, in the direction of -beta * gravity, and the other way with beta negated.  The condition is
    the sign, strictly.  beta is the scene's own (0.2, a fifth of the weight): on the restatement alone it moves the
    means by 2 to 10 % of the pool's depth, the relaxing random fill being the same in all three runs."""
    from smoothed_particle_hydrodynamics_amd import scenes
    scene = getattr(scenes, name)(3000)
    beta = scene[7].beta[0]
    up = -np.sign(beta) * np.sign(scene[7].gravity[1])          # the y direction of -beta * gravity
    assert up == (1.0 if name == "thermal_plume" else -1.0)
    pos0, T0, touched0 = run_scene(oracle, scene, 0.0)
    marked = scene[4][:, 0] == 1 if name == "lock_exchange" else T0[:, 0] > 0.25
    assert 300 < marked.sum() < 2000 and touched0 == 0
    height = {}
    for bt in (beta, -beta):
        pos, _, touched = run_scene(oracle, scene, bt)
        height[bt] = float(pos.reshape(-1, 3)[marked, 1].astype(np.float64).mean())
        assert touched >= marked.sum() // 2
    ref = float(pos0.reshape(-1, 3)[marked, 1].astype(np.float64).mean())
    print("%s: mean height of %d marked particles: beta 0 %.6f, %+.2f %.6f, %+.2f %.6f" %
          (name, marked.sum(), ref, beta, height[beta], -beta, height[-beta]))
    assert (height[beta] - ref) * up > 0
    assert (height[-beta] - ref) * up < 0


# ---- sanitizers ------------------------------------------------------------------------------------------------
MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
""" + WALK + r"""
static float uni(unsigned& s) { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f; }

int main()
{
   unsigned seed = 4711u;
   double checksum = 0.0;
   int accepted = 0, refused = 0, touched = 0, rows = 0;
   for (int rep = 0; rep < 300; rep++) {
      const int n = rep % 5 == 0 ? 0 : 1 + rep % 97;
      std::vector<float> Ts(4 * n), acc(3 * n), vel(3 * n);      // exactly the rows: a lane past them is caught
      for (int i = 0; i < 4 * n; i++) Ts[i] = rep % 7 == 3 && i % 9 == 0 ? 0.5f : 4.0f * uni(seed) - 2.0f;
      for (int i = 0; i < 3 * n; i++) {
         acc[i] = 60.0f * uni(seed) - 30.0f;
         vel[i] = 6.0f * uni(seed) - 3.0f;
      }
      if (n > 2) Ts[4] = rep % 2 ? __builtin_nanf("") : __builtin_inff();
      sph_hip_buoyancy b;
      for (int c = 0; c < 4; c++) {
         b.beta[c] = rep % 11 == 0 ? 0.0f : uni(seed) - 0.5f;
         b.reference[c] = rep % 7 == 3 ? 0.5f : uni(seed);
      }
      for (int a = 0; a < 3; a++) b.gravity[a] = 20.0f * uni(seed) - 10.0f;
      if (rep % 13 == 0) b.beta[rep % 4] = __builtin_inff();
      if (rep % 17 == 0) b.gravity[rep % 3] = __builtin_nanf("");
      if (rep % 19 == 0) b.reference[rep % 4] = -__builtin_inff();
      if (buoyancy_set_check(&b, rep % 23 == 0 ? 0 : n) || buoyancy_is_off(&b)) {
         refused++;
         continue;
      }
      accepted++;
      const float limit = rep % 2 ? 10000.0f : 12.0f;
      touched += walk(&b, n, Ts.data(), acc.data(), vel.data(), 0.004f, limit, limit * limit);
      rows += n;
      for (int i = 0; i < 3 * n; i++) checksum += (double)acc[i] + (double)vel[i];
   }
   if (buoyancy_set_check(nullptr, 0) || !buoyancy_is_off(nullptr)) return 4;
   printf("accepted %d refused %d rows %d touched %d checksum %.6f\n", accepted, refused, rows, touched, checksum);
   return accepted > 100 && refused > 50 && touched > 1000 && touched < rows ? 0 : 3;
}
"""


def test_new_header_code_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    src, exe = tmp_path / "buoyancy_main.cpp", tmp_path / "buoyancy_main"
    src.write_text(MAIN)
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == "", run.stderr
    assert run.stdout.split()[0] == "accepted"
