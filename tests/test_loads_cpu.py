"""CPU checks of the load recording (include/sph_hip.h: sph_hip_record_loads / sph_hip_get_loads): the
numpy restatement tests/load_emulation.py anchored to the reference's wall response (oracle.boundary),
csrc/load_policy.h (compiled with g++ behind an extern "C" shim) against the restatement int64 for
int64, the integrate routes of csrc/launch_policy.h with their new default argument, the refusals of the
two entry points, and the Python side (lib.Loads)."""
import ctypes as C

import numpy as np
import pytest

import load_emulation as L
import obstacle_emulation as E
from helpers import compile_shim

F32 = np.float32

SHIM = r"""
#include "load_policy.h"
#include "launch_policy.h"

extern "C" {
const char* check(int rows, int quantum_log2)
{
   const char* why = load_check(rows, quantum_log2);
   return why ? why : "";
}
const char* range_check(int first_row, int n_rows, int rows)
{
   const char* why = load_range_check(first_row, n_rows, rows);
   return why ? why : "";
}
int term(float m, const float* vb, const float* va, int quantum_log2, long long* q)
{
   return load_term(m, vb, va, load_scale(quantum_log2), q) ? 1 : 0;
}
void respond(const float* maxv, int apply_walls, const sph_hip_obstacle* list, int n, int m, const float* p,
             float* v, float* q, const float* mass, float dt, float damping, int quantum_log2, long long* row)
{
   const LoadRowAdder rec = {row, load_scale(quantum_log2)};
   for (int i = 0; i < m; i++) {
      if (apply_walls) load_walls_respond(maxv, damping, p + 3 * i, v + 3 * i, dt, q + 3 * i, mass[i], rec);
      load_obstacles_respond(list, n, p + 3 * i, v + 3 * i, q + 3 * i, dt, damping, mass[i], rec);
   }
}
int fused_integrate5(int hash_too, int tiled, int n, int no_fused, int n_obst)
{
   return fuse_integrate(hash_too != 0, tiled != 0, n, no_fused != 0, n_obst);
}
int fused_integrate6(int hash_too, int tiled, int n, int no_fused, int n_obst, int record)
{
   return fuse_integrate(hash_too != 0, tiled != 0, n, no_fused != 0, n_obst, record != 0);
}
int fused_slab2(int no_fused_slab, int n_obst) { return fuse_slab_step(no_fused_slab != 0, n_obst); }
int fused_slab3(int no_fused_slab, int n_obst, int record)
{
   return fuse_slab_step(no_fused_slab != 0, n_obst, record != 0);
}
void constants(long long* out)
{
   out[0] = SPH_HIP_LOAD_SOLIDS; out[1] = LOAD_ROW_WORDS; out[2] = LOAD_ROW_COUNT; out[3] = LOAD_ROW_SKIPPED;
   out[4] = LOAD_QUANTUM_DEFAULT; out[5] = LOAD_QUANTUM_MIN; out[6] = LOAD_QUANTUM_MAX;
   out[7] = SPH_HIP_ABI_VERSION; out[8] = SPH_HIP_MAX_OBSTACLES;
}
}
"""


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    from smoothed_particle_hydrodynamics_amd.obstacles import SphObstacle
    lib = compile_shim(SHIM, ["-O2", "-ffp-contract=off"], tmp_path_factory)
    lib.check.argtypes = [C.c_int, C.c_int]
    lib.check.restype = C.c_char_p
    lib.range_check.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.range_check.restype = C.c_char_p
    lib.term.argtypes = [C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.respond.argtypes = [C.c_void_p, C.c_int, C.POINTER(SphObstacle), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                            C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_void_p]
    lib.constants.argtypes = [C.POINTER(C.c_longlong)]
    return lib


def same_bits(a, b):
    """bit for bit; a NaN equals a NaN (its sign and payload are the host's business)"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    nan = np.isnan(a) & np.isnan(b)
    return np.array_equal(np.where(nan, F32(0), a).view(np.uint32), np.where(nan, F32(0), b).view(np.uint32))


def header_respond(lib, maxv, apply_walls, obst, P, V, Q, mass, dt, damping, quantum_log2):
    """the header's walls and obstacles with its serial recorder: (V, Q, impulse, count, skipped)"""
    from smoothed_particle_hydrodynamics_amd.obstacles import as_array
    arr, n = as_array(obst)
    maxv = np.ascontiguousarray(maxv, F32)
    p = np.ascontiguousarray(P, F32).reshape(-1, 3)
    v = np.ascontiguousarray(V, F32).reshape(-1, 3).copy()
    q = np.ascontiguousarray(Q, F32).reshape(-1, 3).copy()
    m = np.ascontiguousarray(mass, F32)
    row = np.zeros(5 * L.SOLIDS, np.int64)
    lib.respond(maxv.ctypes.data, int(apply_walls), arr, n, p.shape[0], p.ctypes.data, v.ctypes.data, q.ctypes.data,
                m.ctypes.data, dt, damping, int(quantum_log2), row.ctypes.data)
    S = L.SOLIDS
    return v, q, row[:3 * S].reshape(S, 3), row[3 * S:4 * S], row[4 * S:]


# ---- constants, refusals, routes ------------------------------------------------------------------

def test_constants_and_abi(policy):
    from smoothed_particle_hydrodynamics_amd import lib as B
    out = (C.c_longlong * 9)()
    policy.constants(out)
    S = L.SOLIDS
    assert list(out) == [S, 5 * S, 3 * S, 4 * S, L.QUANTUM_LOG2, -64, 32, 7, L.MAX_OBSTACLES]
    assert B.LOAD_SOLIDS == S == 70 and B.LOAD_QUANTUM_LOG2 == L.QUANTUM_LOG2 and B.ABI_VERSION == 7
    assert len(B.LOAD_NAMES) == S and B.LOAD_NAMES[:7] == ("x-lo", "x-hi", "y-lo", "y-hi", "z-lo", "z-hi",
                                                            "obstacle 0")
    assert B.PROTOTYPES["sph_hip_record_loads"] == (C.c_int, [C.c_void_p, C.c_int, C.c_int])
    res, args = B.PROTOTYPES["sph_hip_get_loads"]
    assert res is C.c_int and len(args) == 7


def test_recording_refusals(policy):
    assert policy.check(0, -24) == b"" and policy.check(1, -64) == b"" and policy.check(1 << 20, 32) == b""
    assert policy.check(-1, -24) != b""
    assert policy.check(4, -65) != b"" and policy.check(4, 33) != b""
    assert policy.range_check(0, 0, 0) == b"" and policy.range_check(0, 5, 5) == b""
    assert policy.range_check(5, 0, 5) == b"" and policy.range_check(2, 3, 5) == b""
    assert policy.range_check(-1, 1, 5) != b"" and policy.range_check(0, -1, 5) != b""
    assert policy.range_check(0, 6, 5) != b"" and policy.range_check(3, 3, 5) != b""
    assert policy.range_check(6, 0, 5) != b""
    assert policy.range_check(1, 2 ** 31 - 1, 5) != b""          # no overflow of first_row + n_rows


def test_entry_points_exist_and_refuse_a_null_context(hiplib):
    assert hiplib.sph_hip_record_loads(None, 4, -24) == -1
    done = C.c_int32(-5)
    assert hiplib.sph_hip_get_loads(None, 0, 0, None, None, None, C.byref(done)) == -1
    assert done.value == -5


def test_routes_unfused_while_recording(policy):
    for hash_too in (0, 1):
        for tiled in (0, 1):
            for n in (0, 5):
                for no_fused in (0, 1):
                    for n_obst in (0, 1, 64):
                        old = bool(hash_too and tiled and n > 0 and not no_fused and n_obst == 0)
                        args = (hash_too, tiled, n, no_fused, n_obst)
                        assert bool(policy.fused_integrate5(*args)) == old            # the default: not recording
                        assert bool(policy.fused_integrate6(*args, 0)) == old
                        assert not policy.fused_integrate6(*args, 1)
    for no_fused_slab in (0, 1):
        for n_obst in (0, 1, 64):
            old = not no_fused_slab and n_obst == 0
            assert bool(policy.fused_slab2(no_fused_slab, n_obst)) == old
            assert bool(policy.fused_slab3(no_fused_slab, n_obst, 0)) == old
            assert not policy.fused_slab3(no_fused_slab, n_obst, 1)


# ---- the anchor to the reference ------------------------------------------------------------------

@pytest.mark.parametrize("damping", [0.001, 0.5])
def test_wall_restatement_is_the_reference_wall(oracle, damping):
    """the numpy walls give oracle.boundary's final (v, q) bit for bit on test_boundary_gravity's
    wall-crossing cases"""
    from test_boundary_gravity import crossing_cases
    p = oracle.params_for_h(0.1)
    p.damping = damping
    pos, vel, dt, newpos = crossing_cases(p)
    ov, oq = oracle.boundary(p, pos, vel, dt, newpos)
    maxv = F32([p.max_x, p.max_y, p.max_z])
    row = L.Row()
    ev, eq = L.walls(maxv, F32(p.damping), pos, vel, newpos, F32(dt), np.ones(pos.size // 3, F32), row)
    assert same_bits(ev.reshape(-1), ov) and same_bits(eq.reshape(-1), oq)
    Q = newpos.reshape(-1, 3)
    crossed = (Q < 0) | (Q > maxv)
    assert row.count.sum() + row.skipped.sum() >= crossed.any(1).sum() > 1000
    assert (row.count[:6] > 0).all() and not row.count[6:].any()


# ---- the header against the restatement -----------------------------------------------------------

QUANTA = (-24, -30, -10, 0, 32, -64)


def _masses(m, rng):
    """mostly 1, some of any size, a few large enough for their terms to be skipped"""
    mass = np.ones(m, F32)
    k = m // 10
    mass[:k] = rng.uniform(0.1, 8.0, k).astype(F32)
    mass[k:k + k // 4] = F32(1e9)
    mass[k + k // 4:k + k // 2] = F32(3e38)          # m * dv overflows to inf
    return rng.permutation(mass)


def wall_cases(maxv, m, dt, rng):
    """old positions inside the box, new ones around it: faces, edges, corners that meet three walls,
    zero velocity components (division by zero), NaN velocities"""
    P = (rng.random((m, 3)) * maxv).astype(F32)
    V = rng.uniform(-900.0, 900.0, (m, 3)).astype(F32)
    V[rng.random((m, 3)) < 0.1] = 0.0
    k = m // 5
    sgn = rng.choice([-1.0, 1.0], (k, 3)).astype(F32)
    corner = np.where(sgn > 0, maxv, F32(0)).astype(F32)
    off = (rng.uniform(0.001, 0.2, (k, 3)) * maxv).astype(F32)
    P[:k] = corner - sgn * off
    V[:k] = (sgn * off * F32(1.0 / dt) * rng.uniform(1.1, 4.0, (k, 1))).astype(F32)
    Q = (P + V * F32(dt)).astype(F32)
    V[k:k + k // 20, 1] = np.nan                      # a NaN component, the new position still crossing
    V[k + k // 20:k + k // 10] = np.nan
    return P, V, Q


def _shifted(o, origin):
    """the obstacle's struct moved by -origin (every field, the unused ones too: they stay finite)"""
    s = o.as_struct()
    for c in range(3):
        s.center[c] = float(F32(s.center[c]) - origin[c])
        s.lo[c] = float(F32(s.lo[c]) - origin[c])
        s.hi[c] = float(F32(s.hi[c]) - origin[c])
    return s


def check_cases(policy, maxv, apply_walls, obst, P, V, Q, mass, dt, damping, quantum_log2):
    hv, hq, imp, cnt, skp = header_respond(policy, maxv, apply_walls, obst, P, V, Q, mass, dt, damping, quantum_log2)
    ev, eq, row = L.respond(maxv, apply_walls, obst, P, V, Q, dt, damping, mass, quantum_log2)
    assert same_bits(hv, ev) and same_bits(hq, eq)
    assert row.same(imp, cnt, skp), (quantum_log2, np.flatnonzero(row.count != cnt), np.flatnonzero(row.skipped != skp))
    return row


def test_walls_header_equals_numpy(policy):
    rng = np.random.default_rng(4100)
    dt, damping = F32(0.004), F32(0.6)
    maxv = F32([6.4, 3.2, 1.6])
    total = np.zeros(L.SOLIDS, np.int64)
    skipped = cases = three = 0
    for e in QUANTA:
        P, V, Q = wall_cases(maxv, 20000, dt, rng)
        mass = _masses(P.shape[0], rng)
        row = check_cases(policy, maxv, 1, [], P, V, Q, mass, dt, damping, e)
        total += row.count
        skipped += int(row.skipped.sum())
        cases += P.shape[0]
        three += int((((Q < 0) | (Q > maxv)).sum(1) == 3).sum())
        if e == -24:
            # the walls alone are what handle_boundaries gives: the restatement without a recorder
            wv, wq = L.walls(maxv, damping, P, V, Q, dt)
            ev, eq, _ = L.respond(maxv, 1, [], P, V, Q, dt, damping, mass, e)
            assert same_bits(wv, ev) and same_bits(wq, eq)
    assert cases >= 100000 and three > 5000
    assert (total[:6] > 5000).all() and not total[6:].any() and skipped > 1000


@pytest.mark.parametrize("kind", [E.SPHERE, E.BOX, E.CYLINDER], ids=["sphere", "box", "cylinder"])
def test_obstacles_header_equals_numpy(policy, kind):
    """every obstacle of a seeded set with the cases of test_obstacles_cpu around it, a second obstacle
    overlapping it, inside a box whose walls cut through the cases: a wall and an obstacle in one step"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    from test_obstacles_cpu import _extent, _obstacle_set, cases
    rng = np.random.default_rng(4200 + kind)
    dt, damping = F32(0.004), F32(0.6)
    total = both = overlap = zero_terms = skipped = 0
    for i, o in enumerate(_obstacle_set(kind, rng)):
        lo, hi = _extent(o)
        mid = (lo + hi) * F32(0.5)
        other = O.Sphere(mid + F32(0.3) * (hi - lo), F32(0.6) * float((hi - lo).max()))
        obst = [o, other]
        e = QUANTA[i % len(QUANTA)]
        P, V, Q = cases(o, 26000, dt, rng)
        V[rng.random(P.shape[0]) < 0.01, 0] = np.nan
        mass = _masses(P.shape[0], rng)
        # the walls of a box a quarter wider than the obstacle on every side: many cases cross one
        origin = (lo - F32(0.25) * (hi - lo)).astype(F32)
        maxv = (F32(1.5) * (hi - lo)).astype(F32)
        P, Q = (P - origin).astype(F32), (Q - origin).astype(F32)
        shifted = [_shifted(s, origin) for s in obst]
        row = check_cases(policy, maxv, 1, shifted, P, V, Q, mass, dt, damping, e)
        # what the totals are made of, from the restatement
        wv, wq = L.walls(maxv, damping, P, V, Q, dt)
        at_wall = ((Q < 0) | (Q > maxv)).any(1)
        in0 = E.inside(shifted[0], wq)
        v1, q1 = E.respond_one(shifted[0], P, wv, wq, dt, damping)
        in1 = E.inside(shifted[1], q1)
        both += int((at_wall & (in0 | in1)).sum())
        overlap += int((in0 & in1).sum())
        zero_terms += int((in0 & (v1 == wv).all(1)).sum())
        assert row.count[6] + row.skipped[6] == in0.sum() and row.count[7] + row.skipped[7] == in1.sum()
        assert not row.count[8:].any() and not row.skipped[8:].any()
        skipped += int(row.skipped.sum())
        total += P.shape[0]
    assert total >= 100000
    assert both > 500 and overlap > 500 and zero_terms > 100 and skipped > 100, (both, overlap, zero_terms, skipped)


def test_term_by_term(policy):
    """load_term on its own: ties go to even, the skip bound is exclusive, NaN and inf are skipped"""
    def term(m, vb, va, e):
        q = np.zeros(3, np.int64)
        vb, va = np.ascontiguousarray(vb, F32), np.ascontiguousarray(va, F32)
        ok = policy.term(m, vb.ctypes.data, va.ctypes.data, e, q.ctypes.data)
        eq, eok = L.term([m], vb, va, e)
        assert bool(ok) == bool(eok[0]) and (not ok or np.array_equal(q, eq[0]))
        return bool(ok), q
    ok, q = term(1.0, [0.5, 1.5, -2.5], [0, 0, 0], 0)
    assert ok and list(q) == [0, 2, -2]
    ok, q = term(2.0, [3.0, 0.0, 0.0], [-3.0, 0.0, 0.0], -24)
    assert ok and list(q) == [12 << 24, 0, 0]
    assert term(1.0, [2.0 ** 14, 0, 0], [0, 0, 0], -24)[0] is False        # exactly 2^38 quanta
    assert term(1.0, [np.nextafter(F32(2.0 ** 14), F32(0)), 0, 0], [0, 0, 0], -24)[0] is True
    assert term(1.0, [np.nan, 0, 0], [0, 0, 0], -24)[0] is False
    assert term(3e38, [4.0, 0, 0], [-4.0, 0, 0], -24)[0] is False            # m * dv = inf
    assert term(1.0, [1e-30, 0, 0], [0, 0, 0], -64)[0] is True
    ok, q = term(1.0, [5.0, 5.0, 5.0], [5.0, 5.0, 5.0], -24)                  # a fallback that left v alone
    assert ok and not q.any()


# ---- the scene of the GPU tests -------------------------------------------------------------------

def test_walled_scene_terms_are_far_below_the_skip_bound():
    """test_gpu_obstacles.walled_scene has unit masses and speed 90: a reflection gives at most
    2 * |v| per component, so even a tenfold speed-up stays below the 16384 the default quantum holds"""
    pytest.importorskip("smoothed_particle_hydrodynamics_amd.lib")
    from test_gpu_obstacles import walled_scene
    p, pos, vel, mass, obst = walled_scene()
    assert (mass == 1).all()
    vmax = float(np.abs(vel).max())
    assert 2.0 * 10.0 * vmax < 2.0 ** (38 + L.QUANTUM_LOG2)
    dt, damping = F32(p.time_step), F32(p.damping)
    maxv = F32([p.max_x, p.max_y, p.max_z])
    P = pos.reshape(-1, 3)
    V = vel.reshape(-1, 3)
    responses = 0
    for k in (1, 5, 20):          # what a particle meets within k steps of free flight
        Q = (P + V * (dt * F32(k) * F32(1.0 / p.sim_scale))).astype(F32)
        _, _, row = L.respond(maxv, 1, obst, P, V, Q, dt, damping, mass)
        assert not row.skipped.any()
        responses += int(row.count.sum())
    assert responses > 200


# ---- Python side ------------------------------------------------------------------------------------

def test_loads_object():
    from smoothed_particle_hydrodynamics_amd.lib import LOAD_SOLIDS, Loads
    rng = np.random.default_rng(2)
    a = Loads(rng.integers(-2 ** 40, 2 ** 40, (3, LOAD_SOLIDS, 3)), rng.integers(0, 9, (3, LOAD_SOLIDS)),
              np.zeros((3, LOAD_SOLIDS), np.int64), -24)
    assert a.quantum == 2.0 ** -24 and a.impulse.dtype == np.float64
    assert np.array_equal(a.impulse, a.impulse_q * 2.0 ** -24)
    assert np.array_equal(a.force(0.004), a.impulse / 0.004)
    assert a.names[0] == "x-lo" and a.names[6] == "obstacle 0" and len(a.names) == LOAD_SOLIDS
    b = a + a
    assert np.array_equal(b.impulse_q, 2 * a.impulse_q) and np.array_equal(b.count, 2 * a.count)
    with pytest.raises(ValueError):
        a + Loads(a.impulse_q, a.count, a.skipped, -20)
