"""CPU checks of the tracers (include/sph_hip.h: sph_hip_set_tracers): the advance of csrc/tracer_policy.h
(compiled with g++ behind an extern "C" shim) against the numpy restatement tests/tracer_emulation.py bit for
bit, the sort and record decisions, a float64 check of the restatement itself in a uniformly translating fluid,
the binding, and the Python side (scenes.tracer_lattice, scenes.dam_break_dye, lib.Tracers)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sample_emulation as SE
import tracer_emulation as T
from helpers import compile_shim

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = r"""
#include "tracer_policy.h"

// the two probes' answers of one case, handed out in order; notes where the second probe was asked
struct Canned {
   const float* u1; int c1; const float* u2; int c2; float* xm; mutable int calls;
   int operator()(float px, float py, float pz, float& ux, float& uy, float& uz) const
   {
      const float* u = calls == 0 ? u1 : u2;
      if (calls == 1) { xm[0] = px; xm[1] = py; xm[2] = pz; }
      ux = u[0]; uy = u[1]; uz = u[2];
      return calls++ == 0 ? c1 : c2;
   }
};

extern "C" {
void advance(float* x, int32_t* wet, int32_t* dry, const float* u1, const int* c1, const float* u2, const int* c2,
             const float* pos_dt, const int* walls, const float* maxv, float* xm, int* probes, int m)
{
   for (int k = 0; k < m; k++) {
      const TracerStep st = {pos_dt[k], walls[k], {maxv[0], maxv[1], maxv[2]}, 1};
      const Canned s = {u1 + 3 * k, c1[k], u2 + 3 * k, c2[k], xm + 3 * k, 0};
      tracer_advance(x[3 * k], x[3 * k + 1], x[3 * k + 2], wet[k], dry[k], st, s);
      probes[k] = s.calls;
   }
}
const char* check(int n, const float* xyz) { const char* w = tracer_check(n, xyz); return w ? w : ""; }
int sort_switch(const char* env) { return tracer_sort_switch(env); }
int resort_every(int sw) { return tracer_resort_every(sw); }
int resort_every_default() { return tracer_resort_every(); }
int use_sort(int count, int sw) { return tracer_use_sort(count, sw); }
int use_sort_default(int count) { return tracer_use_sort(count); }
int sort_due(int count, int sw, long long since) { return tracer_sort_due(count, sw, since); }
long long record_bytes(int rows, int count) { return tracer_record_bytes(rows, count); }
const char* record_check(int rows, int every, int count)
{
   const char* w = tracer_record_check(rows, every, count);
   return w ? w : "";
}
int record_row(long long step, int every, int rows) { return tracer_record_row(step, every, rows); }
int record_step(int row, int every) { return tracer_record_step(row, every); }
const char* range_check(int first, int n, int have) { const char* w = tracer_range_check(first, n, have); return w ? w : ""; }
void constants(long long* out)
{
   out[0] = TRACER_RESORT_EVERY; out[1] = TRACER_SORT_MIN_COUNT; out[2] = TRACER_SORT_DEFAULT;
   out[3] = SAMPLE_SCRATCH_BUDGET;
}
}
"""


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    lib = compile_shim(SHIM, ["-O2", "-ffp-contract=off"], tmp_path_factory)
    V = C.c_void_p
    lib.advance.argtypes = [V] * 12 + [C.c_int]
    lib.advance.restype = None
    lib.check.argtypes = [C.c_int, V]
    lib.sort_switch.argtypes = [C.c_char_p]
    lib.sort_due.argtypes = [C.c_int, C.c_int, C.c_longlong]
    lib.record_bytes.restype = C.c_longlong
    lib.record_row.argtypes = [C.c_longlong, C.c_int, C.c_int]
    for f in (lib.check, lib.record_check, lib.range_check):
        f.restype = C.c_char_p
    return lib


def same_bits(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


MAXV = np.array([1.0, 2.0, 1.5], F32)


class Scale:
    """the one parameter displacement_step reads"""

    def __init__(self, sim_scale_inv):
        self.sim_scale_inv = sim_scale_inv


def canned_cases(seed=5, m=4000):
    """Random probe answers around the box [0, MAXV]: every branch of steps 2 to 5 among them.  dt is the
    displacement step the advance is handed (tracer_emulation.displacement_step): the time step at unit scale,
    and from row 1400 on what sim_scale_inv = 2 and 0.5 make of it."""
    rng = np.random.default_rng(seed)
    x = (rng.random((m, 3)) * MAXV).astype(F32)
    u1 = rng.normal(0.0, 3.0, (m, 3)).astype(F32)
    u2 = (u1 + rng.normal(0.0, 0.5, (m, 3))).astype(F32)
    c1 = rng.integers(0, 40, m).astype(np.int32)
    c2 = rng.integers(0, 40, m).astype(np.int32)
    dt = np.full(m, 0.02, F32)
    walls = np.ones(m, np.int32)
    c1[:300] = 0                                   # dry: no members
    c2[300:600] = 0                                # the midpoint finds nothing: u = u1
    c1[300:] = np.maximum(c1[300:], 1)
    u2[600:650] = F32(3.0e38)                      # x + u * dt overflows? no: 6e36 - stays finite
    u2[650:700, 0] = np.inf                        # y not finite
    u2[700:750, 1] = -np.inf
    u2[750:800, 2] = np.nan
    u1[800:850] = np.nan                           # u1 NaN but the midpoint has members: u2 decides
    dt[850:900] = F32(3.0e38)                      # y overflows to +-inf
    c2[850:900] = 5
    for a in range(3):                             # clamps on each face, low and high
        u2[900 + 40 * a:920 + 40 * a, a] = F32(-500.0)
        u2[920 + 40 * a:940 + 40 * a, a] = F32(500.0)
    c2[900:1020] = 7
    walls[1020:1200] = 0                           # walls off: the same moves leave the box
    for a in range(3):
        u2[1020 + 40 * a:1040 + 40 * a, a] = F32(-500.0)
        u2[1040 + 40 * a:1060 + 40 * a, a] = F32(500.0)
    c2[1020:1140] = 7
    dt[1200:1300] = F32(0.0)                       # dt == 0: wet, in place
    x[1300:1320] = 0.0                             # on the faces themselves
    x[1320:1340] = MAXV
    dt[1400:2000] = T.displacement_step(Scale(2.0), F32(0.02))    # off unit scale: twice and half the time step
    dt[2000:2600] = T.displacement_step(Scale(0.5), F32(0.02))
    wet0 = rng.integers(0, 100, m).astype(np.int32)
    dry0 = rng.integers(0, 100, m).astype(np.int32)
    return x, wet0, dry0, u1, c1, u2, c2, dt, walls


def test_advance_matches_the_restatement_bit_for_bit(policy):
    x, wet0, dry0, u1, c1, u2, c2, dt, walls = canned_cases()
    m = len(x)
    gx, gw, gd = x.copy(), wet0.copy(), dry0.copy()
    xm = np.zeros((m, 3), F32)
    probes = np.zeros(m, np.int32)
    policy.advance(ptr(gx), ptr(gw), ptr(gd), ptr(u1), ptr(c1), ptr(u2), ptr(c2), ptr(dt), ptr(walls), ptr(MAXV),
                   ptr(xm), ptr(probes), m)
    taken = {k: 0 for k in T.Info._fields}
    for d in np.unique(dt):
        for w in (0, 1):
            sel = (dt == d) & (walls == w)
            if not sel.any():
                continue
            st, info = T.finish(T.State(x[sel], wet0[sel], dry0[sel]), u1[sel], c1[sel], u2[sel], c2[sel], d, w, MAXV)
            assert same_bits(gx[sel], st.x)
            assert np.array_equal(gw[sel], st.wet) and np.array_equal(gd[sel], st.dry)
            # the second probe is asked at the restatement's midpoint, and only by tracers with members
            has = c1[sel] > 0
            assert np.array_equal(probes[sel], np.where(has, 2, 1))
            assert same_bits(xm[sel][has], T.midpoint(x[sel], u1[sel], d)[has])
            for k in taken:
                taken[k] += int(np.asarray(getattr(info, k)).sum())
    # every branch was there to be compared
    assert all(v > 0 for v in taken.values()), taken
    # the displacement steps off unit scale were among them, and they are one fp32 product
    assert np.unique(dt).tolist() == [0.0, float(F32(0.01)), float(F32(0.02)), float(F32(0.04)), float(F32(3.0e38))]
    assert T.displacement_step(Scale(1.0), F32(0.02)) == F32(0.02)
    assert T.displacement_step(Scale(3.0), F32(0.1)).tobytes() == (F32(0.1) * F32(3.0)).tobytes()
    assert (gw + gd == wet0 + dry0 + 1).all()
    # walls off: some tracer is outside the box afterwards; dt == 0: wet and exactly in place
    off = walls == 0
    assert ((gx[off] < 0) | (gx[off] > MAXV)).any()
    z = (dt == 0) & (c1 > 0) & np.isfinite(u2).all(1) & np.isfinite(u1).all(1)
    assert z.any() and same_bits(gx[z], x[z]) and (gw[z] == wet0[z] + 1).all()


def test_clamp_faces_each_hit(policy):
    x, wet0, dry0, u1, c1, u2, c2, dt, walls = canned_cases()
    _, info = T.finish(T.State(x[900:1020], wet0[900:1020], dry0[900:1020]), u1[900:1020], c1[900:1020], u2[900:1020],
                       c2[900:1020], F32(0.02), 1, MAXV)
    assert info.clamp_lo.any(0).all() and info.clamp_hi.any(0).all()


def test_tracer_check(policy):
    ok = np.zeros(6, F32)
    assert policy.check(2, ptr(ok)) == b"" and policy.check(0, None) == b""
    assert b"negative" in policy.check(-1, ptr(ok))
    assert b"null" in policy.check(1, None)
    for bad in (np.nan, np.inf, -np.inf):
        a = ok.copy()
        a[4] = bad
        assert b"not finite" in policy.check(2, ptr(a))


def test_sort_decisions(policy):
    k = (C.c_longlong * 4)()
    policy.constants(k)
    every, min_count, default_on, budget = list(k)
    assert every >= 1 and budget == 64 << 20
    assert policy.resort_every_default() == policy.resort_every(-1) == every
    assert policy.resort_every(0) == 0 and policy.resort_every(1) == 1 and policy.resort_every(7) == 7
    # the switch: unset, garbage, numbers
    assert policy.sort_switch(None) == -1 and policy.sort_switch(b"") == -1 and policy.sort_switch(b"x1") == -1
    assert policy.sort_switch(b"0") == 0 and policy.sort_switch(b"1") == 1 and policy.sort_switch(b"7") == 7
    # pinned: on for any cadence > 0 (two tracers at least), off for 0
    assert policy.use_sort(257, 7) == 1 and policy.use_sort(2, 1) == 1 and policy.use_sort(10 ** 6, 0) == 0
    assert policy.use_sort(1, 1) == 0 and policy.use_sort(0, 1) == 0
    # default: by TRACER_SORT_DEFAULT and the count
    assert policy.use_sort_default(min_count - 1) == 0
    assert policy.use_sort_default(min_count) == policy.use_sort(min_count, -1) == (1 if default_on else 0)
    # due: only when sorting at all, once the cadence has passed
    assert policy.sort_due(5000, 7, 6) == 0 and policy.sort_due(5000, 7, 7) == 1 and policy.sort_due(5000, 1, 1) == 1
    assert policy.sort_due(5000, 0, 10 ** 9) == 0
    assert policy.sort_due(min_count, -1, every) == (1 if default_on else 0)
    assert policy.sort_due(min_count, -1, every - 1) == 0


def test_record_arithmetic(policy):
    assert policy.record_bytes(10, 4096) == 10 * 4096 * 12
    assert policy.record_bytes(2 ** 20, 2 ** 20) == 12 * 2 ** 40          # no 32-bit overflow
    assert policy.record_check(10, 3, 4096) == b"" and policy.record_check(0, 1, 0) == b""
    assert b"rows" in policy.record_check(-1, 1, 10)
    assert b"every" in policy.record_check(1, 0, 10)
    # the budget: 64 MiB holds 5 592 405 positions of 12 bytes, 1 365 rows of 4 096 tracers
    fits = (64 << 20) // 12
    assert policy.record_check(1, 1, fits) == b"" and b"64 MiB" in policy.record_check(1, 1, fits + 1)
    assert policy.record_check(1365, 1, 4096) == b"" and b"64 MiB" in policy.record_check(1366, 1, 4096)
    # rows=10, every=3: steps 1, 4, ..., 28
    rows = [policy.record_row(s, 3, 10) for s in range(0, 40)]
    assert [s for s, r in enumerate(rows) if r >= 0] == list(range(1, 29, 3))
    assert [r for r in rows if r >= 0] == list(range(10))
    assert [policy.record_step(r, 3) for r in range(10)] == list(range(1, 29, 3))
    assert [policy.record_row(s, 1, 3) for s in range(1, 6)] == [0, 1, 2, -1, -1]
    assert policy.range_check(0, 0, 0) == b"" and policy.range_check(2, 3, 5) == b""
    for bad in ((-1, 1, 5), (0, -1, 5), (3, 3, 5), (2 ** 31 - 1, 2 ** 31 - 1, 5)):
        assert policy.range_check(*bad) != b""


# ---- the restatement itself --------------------------------------------------------------------------
def test_uniform_translation_carries_every_wet_tracer_at_v(hiplib):
    """2 000 particles that all move at v: the Shepard velocity of every probe with members is v up to the
    rounding of its sums.  With c members, t_j >= 0: sum(t_j * v) carries c roundings (one product, c - 1
    additions), sum(t_j) c - 1, the quotient one: |u - v| <= |v| * gamma(2c), gamma(k) = k eps / (1 - k eps),
    eps = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1) - evaluated in float64."""
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, _, mass = scenes.dam_break(2000)
    v = np.array([0.375, -1.25, 0.8125], F32)
    vel = np.tile(v, (2000, 1))
    pos = pos.reshape(-1, 3)
    rng = np.random.default_rng(3)
    lo, hi = pos.min(0) - 2 * F32(p.h), pos.max(0) + 2 * F32(p.h)
    x = np.concatenate([pos[::4], (lo + rng.random((500, 3)) * (hi - lo)).astype(F32)])
    dt = F32(p.time_step)
    g = SE.Grid(p, pos, vel, mass)
    _, u1, c1 = g.sample(x)
    _, u2, c2 = g.sample(T.midpoint(x, u1, dt))
    eps = 2.0 ** -24

    def bound(c):
        k = 2.0 * c.astype(np.float64)
        return np.abs(v.astype(np.float64))[None, :] * (k * eps / (1.0 - k * eps))[:, None]

    wet = c1 > 0
    assert wet.sum() > 500 and (~wet).sum() > 10
    assert (np.abs(u1[wet].astype(np.float64) - v) <= bound(c1[wet])).all()
    both = wet & (c2 > 0)
    assert both.sum() > 500
    assert (np.abs(u2[both].astype(np.float64) - v) <= bound(c2[both])).all()
    # and the advance moves them by v * dt: the velocity's bound times dt, plus the product's and the sum's rounding
    st, info = T.advance(p, pos, vel, mass, T.initial(x), dt, with_info=True)
    assert np.array_equal(info.wet, wet) and np.array_equal(st.wet, wet.astype(np.int32))
    assert same_bits(st.x[~wet], x[~wet]) and (st.dry[~wet] == 1).all()
    want = x.astype(np.float64) + v.astype(np.float64) * float(dt)
    slack = bound(np.maximum(c1, c2)) * float(dt) + 2 * eps * (np.abs(want) + abs(float(dt)) * np.abs(v))
    assert not p.apply_walls
    assert (np.abs(st.x[both].astype(np.float64) - want[both]) <= slack[both]).all()


def carried_check(p, x0, count, tracers_after, particles_after, particles_before):
    """The property of scale_cases.carried_scene: (holds, worst excess over the bound) of tracers set on particles,
    one step on, against those particles' new positions."""
    import scale_cases
    bound = scale_cases.carried_bound(p, count, np.concatenate([particles_before, particles_after]))
    err = np.abs(np.asarray(tracers_after, np.float64) - np.asarray(particles_after, np.float64))
    return bool((err <= bound).all()), float((err / bound).max())


def test_tracers_are_carried_off_unit_scale(oracle, hiplib):
    """sim_scale_inv = 2, a fluid in uniform translation without forces: after one step a tracer set on a particle
    lies on that particle's new position - the oracle's -, within the rounding of the Shepard quotient and of the
    move.  The arithmetic that advances a tracer by u * dt (sim_scale_inv left out) misses it by |v0_c| * dt."""
    import scale_cases
    from helpers import to_oracle_params
    p, pos, vel, mass, rows = scale_cases.carried_scene()
    x0 = pos.reshape(-1, 3)[rows].copy()
    st, info = T.advance(p, pos, vel, mass, T.initial(x0), p.time_step, with_info=True)
    count = SE.Grid(p, pos, vel, mass).sample(x0, velocity=False)[2]
    assert info.wet.all() and (count > 8).all()
    opos, ovel = pos.copy(), vel.copy()
    out = oracle.step(to_oracle_params(p), opos, ovel, mass, mode="full")
    assert not out["acc"].any()                    # every acceleration is exactly zero
    after = opos.reshape(-1, 3)[rows]
    # the oracle alone: a particle goes where x + v0 * pos_dt says, within the bound's last two roundings
    pos_dt = float(T.displacement_step(p, p.time_step))
    exact = x0.astype(np.float64) + np.array(scale_cases.V0, np.float64) * pos_dt
    assert carried_check(p, x0, np.zeros(len(rows)), exact, after, x0)[0]
    assert pos_dt == 2.0 * float(F32(p.time_step))
    ok, worst = carried_check(p, x0, count, st.x, after, x0)
    assert ok, worst
    # the old contract - the time step where the displacement step belongs: sim_scale_inv = 1 in the move, the
    # samples' arithmetic unchanged (sim_scale is still 0.5)
    q = p.copy()
    q.sim_scale_inv = 1.0
    assert not SE.unit_scale(q)
    old = T.advance(q, pos, vel, mass, T.initial(x0), p.time_step)
    ok_old, worst_old = carried_check(p, x0, count, old.x, after, x0)
    assert not ok_old and worst_old > 1000.0
    # and at unit scale the displacement step is the time step, bit for bit
    q.sim_scale = 1.0
    assert T.displacement_step(q, p.time_step).tobytes() == F32(p.time_step).tobytes()


def test_no_particles_every_tracer_is_dry(hiplib):
    from smoothed_particle_hydrodynamics_amd import scenes
    p, _, _, _ = scenes.dam_break(2000)
    x = np.array([[0.1, 0.2, 0.3], [5.0, 5.0, 5.0]], F32)
    st = T.advance(p, np.zeros(0, F32), np.zeros(0, F32), np.zeros(0, F32), T.initial(x), p.time_step)
    assert same_bits(st.x, x) and st.dry.tolist() == [1, 1] and st.wet.tolist() == [0, 0]


# ---- the Python side -------------------------------------------------------------------------------------
def test_tracer_lattice_is_fp32_unfused(hiplib):
    from smoothed_particle_hydrodynamics_amd import scenes
    lo, hi, s = (0.1, 0.2, 0.3), (0.75, 0.5, 0.35), 0.1
    pts = scenes.tracer_lattice(lo, hi, s)
    assert pts.dtype == np.float32 and pts.shape == (7 * 4 * 1, 3)
    want = SE.lattice_points(lo, (s, s, s), (7, 4, 1)).reshape(-1, 3)
    assert same_bits(pts, want)
    assert (pts >= np.array(lo, F32)).all() and (pts <= np.array(hi, F32)).all()
    assert scenes.tracer_lattice(lo, hi, (0.5, 0.1, 0.1)).shape == (2 * 4 * 1, 3)
    assert scenes.tracer_lattice((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), 0.1).shape == (0, 3)
    with pytest.raises(ValueError):
        scenes.tracer_lattice(lo, hi, 0.0)


def test_dam_break_dye_shapes(hiplib):
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass, tracers = scenes.dam_break_dye(5000)
    assert pos.shape == vel.shape == (15000,) and mass.shape == (5000,)
    assert p.apply_walls == 1 and p.apply_gravity == 1 and p.gravity[1] < 0
    assert (vel.reshape(-1, 3)[:, 0] == F32(0.7)).all()
    assert tracers.dtype == np.float32 and tracers.ndim == 2 and tracers.shape[1] == 3 and len(tracers) > 100
    # through the column, inside it
    assert (tracers > 0).all() and (tracers < np.array([0.1, 0.75, 1.0], F32)).all()
    for a in range(3):
        assert len(np.unique(tracers[:, a])) >= 2
    # every tracer starts among particles
    g = SE.Grid(p, pos, vel, mass)
    assert (g.sample(tracers)[2] > 0).mean() > 0.95


def test_tracers_round_trip_through_the_tuples(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    t = S.Tracers(np.zeros((2, 3), F32), np.array([1, 2], np.int32), np.array([3, 4], np.int32))
    assert t._fields == ("position", "wet_steps", "dry_steps") and t.wet_steps.tolist() == [1, 2]
    st = T.State(t.position, t.wet_steps, t.dry_steps)
    back = S.Tracers(*st)
    assert back.position is t.position and back.dry_steps.tolist() == [3, 4]
    path = S.TracerPath(np.array([1, 4], np.int32), np.zeros((2, 2, 3), F32))
    assert path._fields == ("steps", "positions")


def test_prototypes_match_the_header(hiplib):
    from smoothed_particle_hydrodynamics_amd import lib as L
    V, I = C.c_void_p, C.c_int
    assert L.PROTOTYPES["sph_hip_set_tracers"] == (I, [V, I, V])
    assert L.PROTOTYPES["sph_hip_get_tracers"] == (I, [V, I, I, V, V, V])
    assert L.PROTOTYPES["sph_hip_tracer_count"] == (I, [V])
    assert L.PROTOTYPES["sph_hip_record_tracers"] == (I, [V, I, I])
    assert L.PROTOTYPES["sph_hip_get_tracer_path"] == (I, [V, I, I, V, V])
    text = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    assert re.search(r"#define SPH_HIP_ABI_VERSION 7\b", text) and L.ABI_VERSION == 7
    for name in ("set_tracers", "get_tracers", "tracer_count", "record_tracers", "get_tracer_path"):
        assert hasattr(hiplib, "sph_hip_" + name)
        assert re.search(r"\bint sph_hip_%s\(" % name, text)
    # a null context is refused without touching the device
    assert hiplib.sph_hip_set_tracers(None, 0, None) < 0 and hiplib.sph_hip_tracer_count(None) < 0
