"""CPU checks of the moving obstacles (include/sph_hip.h: sph_hip_set_obstacle_motion): the struct layout,
the refusals, the displacement and the motion clock, the per-particle response and the load recorder of
csrc/obstacle_policy.h / load_policy.h (compiled with g++ behind an extern "C" shim) against the numpy
restatement tests/moving_obstacle_emulation.py bit for bit, the anchors to the static response, the route
decision of csrc/launch_policy.h, and the Python side (obstacles.Motion, scenes.dam_break_gate)."""
import ctypes as C
import math

import numpy as np
import pytest

import load_emulation as L
import moving_obstacle_emulation as M
import obstacle_emulation as E
from helpers import compile_shim
from test_loads_cpu import same_bits as same_bits_nan
from test_obstacles_cpu import _extent, _obstacle_set, cases, same_bits

F32 = np.float32

SHIM = r"""
#include <stddef.h>
#include "load_policy.h"
#include "launch_policy.h"

extern "C" {
const char* motion_check(const sph_hip_obstacle_motion* list, int n, int n_obstacles)
{
   const char* why = obstacle_motion_check(list, n, n_obstacles);
   return why ? why : "";
}
int count_moving(const sph_hip_obstacle_motion* list, int n) { return obstacles_moving(list, n); }
float s_of(const sph_hip_obstacle_motion* m, float tau) { return obstacle_motion_s(*m, tau); }
void displacement(const sph_hip_obstacle_motion* m, float tau, float* D) { obstacle_displacement(*m, tau, D); }
void at(const sph_hip_obstacle* o, const sph_hip_obstacle_motion* m, float tau, sph_hip_obstacle* out)
{
   *out = obstacle_at(*o, m, tau);
}
float clock_next(float tau, float dt) { return obstacle_clock_next(tau, dt); }
void respond_static(const sph_hip_obstacle* list, int n, int m, const float* p, float* v, float* q, float dt,
                    float damping)
{
   for (int i = 0; i < m; i++) obstacles_respond(list, n, p + 3 * i, v + 3 * i, q + 3 * i, dt, damping);
}
void respond(const sph_hip_obstacle* list, const sph_hip_obstacle_motion* motion, int n, int m, const float* p,
             float* v, float* q, float dt, float damping, float tau0, float tau1)
{
   for (int i = 0; i < m; i++)
      obstacles_respond_moving(list, motion, n, p + 3 * i, v + 3 * i, q + 3 * i, dt, damping, tau0, tau1);
}
void respond_loads(const float* maxv, int apply_walls, const sph_hip_obstacle* list,
                   const sph_hip_obstacle_motion* motion, int n, int m, const float* p, float* v, float* q,
                   const float* mass, float dt, float damping, float tau0, float tau1, int quantum_log2,
                   long long* row)
{
   const LoadRowAdder rec = {row, load_scale(quantum_log2)};
   for (int i = 0; i < m; i++) {
      if (apply_walls) load_walls_respond(maxv, damping, p + 3 * i, v + 3 * i, dt, q + 3 * i, mass[i], rec);
      load_obstacles_respond_moving(list, motion, n, p + 3 * i, v + 3 * i, q + 3 * i, dt, damping, tau0, tau1,
                                    mass[i], rec);
   }
}
int moving_kernels(int n_obst, int n_moving) { return use_moving_kernels(n_obst, n_moving); }
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
#define OFF(f) (long long)offsetof(sph_hip_obstacle_motion, f)
void layout(long long* out)
{
   out[0] = sizeof(sph_hip_obstacle_motion);
   out[1] = OFF(velocity); out[2] = OFF(start); out[3] = OFF(stop);
   out[4] = SPH_HIP_ABI_VERSION; out[5] = sizeof(sph_hip_obstacle); out[6] = SPH_HIP_MAX_OBSTACLES;
}
}
"""


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    from smoothed_particle_hydrodynamics_amd.obstacles import SphObstacle, SphObstacleMotion
    lib = compile_shim(SHIM, ["-O2", "-ffp-contract=off"], tmp_path_factory)
    PO, PM, V = C.POINTER(SphObstacle), C.POINTER(SphObstacleMotion), C.c_void_p
    lib.motion_check.argtypes = [PM, C.c_int, C.c_int]
    lib.motion_check.restype = C.c_char_p
    lib.count_moving.argtypes = [PM, C.c_int]
    lib.s_of.argtypes = [PM, C.c_float]
    lib.s_of.restype = C.c_float
    lib.displacement.argtypes = [PM, C.c_float, V]
    lib.at.argtypes = [PO, PM, C.c_float, PO]
    lib.clock_next.argtypes = [C.c_float, C.c_float]
    lib.clock_next.restype = C.c_float
    lib.respond_static.argtypes = [PO, C.c_int, C.c_int, V, V, V, C.c_float, C.c_float]
    lib.respond.argtypes = [PO, PM, C.c_int, C.c_int, V, V, V, C.c_float, C.c_float, C.c_float, C.c_float]
    lib.respond_loads.argtypes = [V, C.c_int, PO, PM, C.c_int, C.c_int, V, V, V, V, C.c_float, C.c_float, C.c_float,
                                  C.c_float, C.c_int, V]
    lib.layout.argtypes = [C.POINTER(C.c_longlong)]
    return lib


def _arrays(P, V, Q):
    p = np.ascontiguousarray(P, F32).reshape(-1, 3)
    return p, np.ascontiguousarray(V, F32).reshape(-1, 3).copy(), np.ascontiguousarray(Q, F32).reshape(-1, 3).copy()


def header_static(lib, obstacles, P, V, Q, dt, damping):
    from smoothed_particle_hydrodynamics_amd.obstacles import as_array
    arr, n = as_array(obstacles)
    p, v, q = _arrays(P, V, Q)
    lib.respond_static(arr, n, p.shape[0], p.ctypes.data, v.ctypes.data, q.ctypes.data, dt, damping)
    return v, q


def header_respond(lib, obstacles, motions, P, V, Q, dt, damping, tau0, tau1):
    from smoothed_particle_hydrodynamics_amd.obstacles import as_array, as_motion_array
    arr, n = as_array(obstacles)
    mot, _ = as_motion_array(motions)
    p, v, q = _arrays(P, V, Q)
    lib.respond(arr, mot, n, p.shape[0], p.ctypes.data, v.ctypes.data, q.ctypes.data, dt, damping, tau0, tau1)
    return v, q


def header_loads(lib, maxv, apply_walls, obstacles, motions, P, V, Q, mass, dt, damping, tau0, tau1, quantum_log2):
    from smoothed_particle_hydrodynamics_amd.obstacles import as_array, as_motion_array
    arr, n = as_array(obstacles)
    mot, _ = as_motion_array(motions)
    maxv = np.ascontiguousarray(maxv, F32)
    p, v, q = _arrays(P, V, Q)
    m = np.ascontiguousarray(mass, F32)
    row = np.zeros(5 * L.SOLIDS, np.int64)
    lib.respond_loads(maxv.ctypes.data, int(apply_walls), arr, mot, n, p.shape[0], p.ctypes.data, v.ctypes.data,
                      q.ctypes.data, m.ctypes.data, dt, damping, tau0, tau1, int(quantum_log2), row.ctypes.data)
    S = L.SOLIDS
    return v, q, row[:3 * S].reshape(S, 3), row[3 * S:4 * S], row[4 * S:]


# ---- layout, constants, refusals ---------------------------------------------------------------

def test_struct_layout_and_constants(policy):
    from smoothed_particle_hydrodynamics_amd import lib as B
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    out = (C.c_longlong * 7)()
    policy.layout(out)
    S = O.SphObstacleMotion
    assert list(out) == [20, S.velocity.offset, S.start.offset, S.stop.offset, 7, 48, 64]
    assert C.sizeof(S) == 20 and [S.velocity.offset, S.start.offset, S.stop.offset] == [0, 12, 16]
    assert B.ABI_VERSION == 7
    assert B.PROTOTYPES["sph_hip_set_obstacle_motion"] == (C.c_int, [C.c_void_p, C.POINTER(S), C.c_int])
    assert B.PROTOTYPES["sph_hip_get_obstacle_motion"] == (C.c_int, [C.c_void_p, C.POINTER(S), C.c_int,
                                                                      C.POINTER(C.c_float)])
    assert B.PROTOTYPES["sph_hip_get_obstacles_now"] == (C.c_int, [C.c_void_p, C.POINTER(O.SphObstacle), C.c_int])


def test_refusals(policy):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    ok = [O.Motion((1, 0, 0)), None, O.Motion((0, -2, 0.5), 0.25, 0.75), O.Motion((0, 0, 3), 1.0, 1.0)]
    arr, n = O.as_motion_array(ok)
    assert policy.motion_check(arr, 4, 4) == b"" and policy.count_moving(arr, 4) == 3
    assert policy.motion_check(None, 0, 4) == b"" and policy.motion_check(None, 0, 0) == b""
    assert policy.motion_check(arr, 0, 4) == b""                      # n = 0 clears, whatever the list
    assert policy.motion_check(arr, 3, 4) != b"" and policy.motion_check(arr, 4, 3) != b""
    assert policy.motion_check(arr, 4, 0) != b"" and policy.motion_check(arr, -1, 4) != b""
    assert policy.motion_check(None, 4, 4) != b""

    def refused(mutate):
        s = ok[2].as_struct()
        mutate(s)
        a, k = O.as_motion_array([s])
        return policy.motion_check(a, k, 1) != b""

    for bad in (np.nan, np.inf, -np.inf):
        for c in range(3):
            assert refused(lambda s: s.velocity.__setitem__(c, bad))
        assert refused(lambda s: setattr(s, "start", bad))
    assert refused(lambda s: setattr(s, "start", -0.5))
    assert refused(lambda s: setattr(s, "stop", 0.125))               # stop < start
    assert refused(lambda s: setattr(s, "stop", np.nan))
    assert refused(lambda s: setattr(s, "stop", -np.inf))
    assert not refused(lambda s: setattr(s, "stop", np.inf))
    assert not refused(lambda s: setattr(s, "stop", 0.25))            # stop == start
    assert not refused(lambda s: setattr(s, "start", -0.0))
    assert not refused(lambda s: s.velocity.__setitem__(0, 0.0))


def test_entry_points_exist_and_refuse_a_null_context(hiplib):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    arr, n = O.as_motion_array([O.Motion((1, 0, 0))])
    assert hiplib.sph_hip_set_obstacle_motion(None, arr, n) == -1
    clock = C.c_float(-5.0)
    assert hiplib.sph_hip_get_obstacle_motion(None, arr, 1, C.byref(clock)) == -1 and clock.value == -5.0
    out, _ = O.as_array([O.Sphere((0, 0, 0), 1.0)])
    assert hiplib.sph_hip_get_obstacles_now(None, out, 1) == -1


# ---- displacement and clock ---------------------------------------------------------------------

def test_displacement_matches_the_restatement(policy):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(11)
    motions = [O.Motion((0.3, -1.7, 2.5), 0.125, 0.7), O.Motion((1e-3, 0, -4e2), 0.0, math.inf),
               O.Motion((-0.0, 5.0, 0.0), 0.3, 0.3), O.Motion(rng.normal(0, 9, 3), 0.011, 0.013)]
    for m in motions:
        st = m.as_struct()
        taus = [0.0, float(m.start) * 0.5, float(m.start), float(np.nextafter(m.start, F32(9)))]
        taus += [float(m.stop)] if np.isfinite(m.stop) else [1e30, 3.0e38]
        taus += [float(m.start) + 0.25 * min(float(m.stop) - float(m.start), 4.0), 2.0 * float(m.start) + 5.0]
        taus += list(rng.uniform(0.0, 1.0, 50))
        for tau in taus:
            tau = F32(tau)
            D = np.zeros(3, F32)
            policy.displacement(C.byref(st), tau, D.ctypes.data)
            assert same_bits(D, M.displacement(m, tau)) and same_bits(D, m.displacement(tau))
            assert same_bits(F32(policy.s_of(C.byref(st), tau)), M.s_of(m, tau))
            if tau <= m.start:
                assert not (D != 0).any()
            if tau >= m.stop:
                assert same_bits(D, (m.velocity * F32(m.stop - m.start)).astype(F32))


def test_obstacle_at_matches_the_restated_shift(policy):
    """obstacle_at is what sph_hip_get_obstacles_now returns: all three of center, lo and hi are shifted,
    the unused fields included; an entry that does not move comes back untouched, -0 fields too"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(12)
    for kind in (E.SPHERE, E.BOX, E.CYLINDER):
        for o in _obstacle_set(kind, rng):
            st = o.as_struct()
            st.lo[0] = -0.0
            m = O.Motion(rng.normal(0, 3, 3), 0.1, 0.9)
            for tau in (0.0, 0.1, 0.5, 0.9, 7.0):
                out = O.SphObstacle()
                policy.at(C.byref(st), C.byref(m.as_struct()), tau, C.byref(out))
                assert bytes(out) == bytes(M.obstacle_at(st, m, tau))
                rest = O.Motion((0, 0, 0), 0.1, 0.9)
                policy.at(C.byref(st), C.byref(rest.as_struct()), tau, C.byref(out))
                assert bytes(out) == bytes(st)
                policy.at(C.byref(st), None, tau, C.byref(out))
                assert bytes(out) == bytes(st)
            moved = M.obstacle_at(st, m, 0.5)
            D = M.displacement(m, 0.5)
            assert same_bits(list(moved.hi), (np.array(list(st.hi), F32) + D).astype(F32))
        # a moving entry is shifted even by D == 0: -0 + (+0) = +0, which is why one at rest is not
        plus = O.Motion((1.0, 1.0, 1.0), 0.1, 0.9)
        policy.at(C.byref(st), C.byref(plus.as_struct()), 0.0, C.byref(out))
        assert math.copysign(1.0, out.lo[0]) == 1.0 and math.copysign(1.0, st.lo[0]) == -1.0


def test_clock_is_an_fp32_running_sum(policy):
    dt = F32(0.004)
    tau = F32(0.0)
    want = M.clock(dt, 1000)
    differs = 0
    for k in range(1000):
        assert same_bits(tau, want[k])
        differs += int(tau != F32(k) * dt)
        tau = F32(policy.clock_next(tau, dt))
    assert same_bits(tau, want[1000])
    assert differs > 100, "the running sum is not k * dt"


# ---- the response, header vs numpy -------------------------------------------------------------

def _timings(rng, dt):
    """(motion start, stop, tau0, tau1): inside the interval, straddling start, straddling stop, before the
    start, after the stop, dt == 0 (tau1 == tau0)"""
    dt = F32(dt)
    t0 = F32(rng.uniform(0.05, 0.2))
    out = [(0.0, math.inf, t0, F32(t0 + dt)),
           (float(t0 + dt * F32(0.3)), math.inf, t0, F32(t0 + dt)),
           (0.0, float(t0 + dt * F32(0.6)), t0, F32(t0 + dt)),
           (float(t0 + F32(1.0)), math.inf, t0, F32(t0 + dt)),
           (0.0, float(t0 * F32(0.5)), t0, F32(t0 + dt)),
           (0.0, math.inf, t0, t0)]
    return out


def moving_cases(o, motion, tau0, tau1, m, dt, rng):
    """test_obstacles_cpu.cases around the obstacle as it stands at tau1 - faces, edges, corners, grazing
    lines, q on the surface - plus: p inside the obstacle at tau0, a solid overtaking particles at rest,
    particles overtaking the solid"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    D0, D1 = M.displacement(motion, tau0), M.displacement(motion, tau1)
    o1 = O.from_struct(M.shifted(o, D1))
    o0 = O.from_struct(M.shifted(o, D0))
    P, V, Q = cases(o1, m, dt, rng)
    k = m // 10
    lo0, hi0 = _extent(o0)
    # p inside the obstacle at tau0
    a = slice(5 * k, 6 * k)
    P[a] = (lo0 + rng.random((k, 3)) * (hi0 - lo0)).astype(F32)
    Q[a] = (P[a] + V[a] * F32(dt)).astype(F32)
    # the solid overtakes particles at rest: q = p just ahead of where it stood
    b = slice(6 * k, 7 * k)
    lo1, hi1 = _extent(o1)
    P[b] = (lo1 + rng.random((k, 3)) * (hi1 - lo1)).astype(F32)
    V[b] = 0.0
    Q[b] = P[b]
    # particles overtaking the solid: along its velocity, faster, from behind
    c = slice(7 * k, 8 * k)
    vel = M.motion_fields(motion)[0]
    V[c] = (vel * rng.uniform(1.2, 4.0, (k, 1))).astype(F32)
    Q[c] = (lo1 + rng.random((k, 3)) * (hi1 - lo1)).astype(F32)
    P[c] = (Q[c] - V[c] * F32(dt)).astype(F32)
    return P, V, Q


def _motion_for(o, rng, start, stop):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    lo, hi = _extent(o)
    speed = float((hi - lo).mean()) * float(rng.choice([2.0, 20.0, 200.0]))   # extents per unit time
    v = (rng.normal(0.0, 1.0, 3) * speed).astype(F32)
    v[rng.random(3) < 0.25] = 0.0
    if not (v != 0).any():
        v[0] = F32(speed)
    return O.Motion(v, start, stop)


@pytest.mark.parametrize("kind", [E.SPHERE, E.BOX, E.CYLINDER], ids=["sphere", "box", "cylinder"])
def test_header_equals_numpy_bit_for_bit(policy, kind):
    rng = np.random.default_rng(2000 + kind)
    dt, damping = F32(0.004), F32(0.6)
    total = active = boosted = 0
    for o in _obstacle_set(kind, rng):
        for start, stop, tau0, tau1 in _timings(rng, dt):
            step = dt if tau1 != tau0 else F32(0.0)
            motion = _motion_for(o, rng, start, stop)
            P, V, Q = moving_cases(o, motion, tau0, tau1, 5000, dt, rng)
            hv, hq = header_respond(policy, [o], [motion], P, V, Q, step, damping, tau0, tau1)
            ev, eq, act = M.respond_one(o, motion, P, V, Q, step, damping, tau0, tau1)
            assert same_bits(hv, ev) and same_bits(hq, eq), (kind, start, stop, tau0, tau1)
            assert same_bits(hv[~act], V[~act]) and same_bits(hq[~act], Q[~act])
            total += P.shape[0]
            active += int(act.sum())
            d = M.displacement(motion, tau1) - M.displacement(motion, tau0)
            boosted += int(act.sum()) if (d != 0).any() else 0
    assert total >= 100000
    assert active > 10000 and boosted > 4000, (active, boosted)


def test_mixed_lists_header_equals_numpy(policy):
    """resting and moving entries in one list, overlapping, applied in list order; a resting entry with
    -0 fields keeps them (its fallback writes them into q)"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(78)
    neg = O.Box((-0.0, -1.0, -0.5), (1.2, 0.3, 0.5)).as_struct()
    neg.lo[0] = -0.0
    obst = [O.Sphere((0.0, 0.0, 0.0), 0.7), neg, O.Cylinder(1, (0.4, 0.0, 0.3), 0.5, -0.8, 0.8),
            O.Box((-0.9, -0.2, -0.2), (-0.1, 0.6, 0.7))]
    motions = [O.Motion((30.0, 0.0, -12.0), 0.0, math.inf), None, O.Motion((0.0, 25.0, 0.0), 0.101, 0.2),
               O.Motion((0.0, 0.0, 0.0), 0.0, 1.0)]
    dt, damping = F32(0.004), F32(0.3)
    tau0 = F32(0.1)
    tau1 = F32(tau0 + dt)
    P, V, Q = cases(O.Box((-1.0, -1.0, -1.0), (1.2, 1.0, 1.0)), 100000, dt, rng)
    hv, hq = header_respond(policy, obst, motions, P, V, Q, dt, damping, tau0, tau1)
    ev, eq = M.respond(obst, motions, P, V, Q, dt, damping, tau0, tau1)
    assert same_bits(hv, ev) and same_bits(hq, eq)
    sv, sq = header_static(policy, obst, P, V, Q, dt, damping)
    assert not same_bits(hq, sq)
    on_neg_face = (hq[:, 0] == 0) & np.signbit(hq[:, 0])
    assert on_neg_face.sum() > 10, "the resting box's -0 face must reach some q"


# ---- anchors ------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [E.SPHERE, E.BOX, E.CYLINDER], ids=["sphere", "box", "cylinder"])
def test_at_rest_is_the_static_response(policy, kind):
    """a Motion with zero velocity, and a motion that has not started (D == 0), give obstacles_respond"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(3000 + kind)
    dt, damping = F32(0.004), F32(0.6)
    obst = _obstacle_set(kind, rng)
    P, V, Q = cases(O.Box((-3.0, -3.0, -3.0), (3.0, 3.0, 3.0)), 40000, dt, rng)
    sv, sq = header_static(policy, obst, P, V, Q, dt, damping)
    assert not same_bits(sq, Q)
    tau0 = F32(0.5)
    tau1 = F32(tau0 + dt)
    for motions in ([O.Motion((0, 0, 0))] * 4, [O.Motion((0.0, -0.0, 0.0), 0.1, 0.2)] * 4,
                    [O.Motion((50.0, -20.0, 7.0), 0.75, 2.0)] * 4, [None, O.Motion((1, 2, 3), 1.0), None, None]):
        hv, hq = header_respond(policy, obst, motions, P, V, Q, dt, damping, tau0, tau1)
        assert same_bits(hv, sv) and same_bits(hq, sq)
        ev, eq = M.respond(obst, motions, P, V, Q, dt, damping, tau0, tau1)
        assert same_bits(ev, sv) and same_bits(eq, sq)


def test_dyadic_inputs_are_the_boosted_static_problem(policy):
    """Small dyadic rationals everywhere: d, ue = d / dt, p + d and v - ue are exact, so the moving
    response is the static response of the boosted problem (formed here in float64), boosted back"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(31)
    dt, damping = F32(2.0 ** -6), F32(0.5)
    box = O.Box((0.25, -0.5, 0.0), (1.0, 0.75, 1.5))
    motion = O.Motion((4.0, -2.0, 0.0), 0.0, math.inf)
    tau0 = F32(8 * dt)
    tau1 = F32(tau0 + dt)
    d = np.float64([4.0, -2.0, 0.0]) * float(dt)
    o1 = O.Box(box.lo.astype(np.float64) + 9 * d, box.hi.astype(np.float64) + 9 * d)
    m = 40000
    P = (rng.integers(-48, 144, (m, 3)) / 64.0).astype(F32)
    V = (rng.integers(-64, 64, (m, 3)) / 2.0).astype(F32)
    Q = (P.astype(np.float64) + V.astype(np.float64) * float(dt)).astype(F32)
    assert np.array_equal(Q.astype(np.float64), P.astype(np.float64) + V.astype(np.float64) * float(dt))
    hv, hq = header_respond(policy, [box], [motion], P, V, Q, dt, damping, tau0, tau1)
    ue = d / float(dt)
    pr = (P.astype(np.float64) + d).astype(F32)
    w = (V.astype(np.float64) - ue).astype(F32)
    sv, sq = header_static(policy, [o1], pr, w, Q, dt, damping)
    act = E.inside(o1, Q)
    assert act.sum() > 1000
    back = np.where(act[:, None], sv.astype(np.float64) + ue, V.astype(np.float64))
    assert np.array_equal(back.astype(F32).astype(np.float64), back)      # exact in fp32
    assert same_bits(hv, back.astype(F32)) and same_bits(hq, sq)


def test_piston_leaves_fluid_at_rest_at_twice_its_speed(policy):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(32)
    dt, damping = F32(0.004), F32(0.6)
    u = F32(12.5)
    piston = O.Box((0.0, 0.0, 0.0), (0.5, 1.0, 1.0))
    motion = O.Motion((u, 0.0, 0.0))
    tau0 = F32(0.2)
    tau1 = F32(tau0 + dt)
    face0 = F32(0.5) + M.displacement(motion, tau0)[0]
    face1 = F32(0.5) + M.displacement(motion, tau1)[0]
    m = 5000
    P = np.stack([rng.uniform(float(face0), float(face1), m), rng.uniform(0.1, 0.9, m), rng.uniform(0.1, 0.9, m)],
                 1).astype(F32)
    P = P[(P[:, 0] > face0) & (P[:, 0] < face1)]
    V = np.zeros_like(P)
    hv, hq = header_respond(policy, [piston], [motion], P, V, P, dt, damping, tau0, tau1)
    assert P.shape[0] > 4000
    assert np.allclose(hv[:, 0], 2.0 * float(u), rtol=1e-5) and not hv[:, 1:].any()
    assert (hq[:, 0] >= face1).all()
    assert same_bits(hq[:, 1:], P[:, 1:])
    # the static response, which takes the solid to be at rest, never sets the fluid in motion
    sv, _ = header_static(policy, [O.from_struct(M.shifted(piston, M.displacement(motion, tau1)))], P, V, P, dt,
                          damping)
    assert not sv.any()


# ---- loads --------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [E.SPHERE, E.BOX, E.CYLINDER], ids=["sphere", "box", "cylinder"])
def test_moving_recorder_equals_numpy(policy, kind):
    rng = np.random.default_rng(4000 + kind)
    dt, damping = F32(0.004), F32(0.6)
    maxv = F32([2.5, 2.5, 2.5])
    total = responses = 0
    for o in _obstacle_set(kind, rng):
        for start, stop, tau0, tau1 in _timings(rng, dt):
            step = dt if tau1 != tau0 else F32(0.0)
            motion = _motion_for(o, rng, start, stop)
            P, V, Q = moving_cases(o, motion, tau0, tau1, 5000, dt, rng)
            mass = rng.uniform(0.5, 2.0, P.shape[0]).astype(F32)
            # (the obstacles lie about the origin: with the walls on, most particles meet x-lo .. z-lo first)
            for walls in (False, True):
                hv, hq, imp, cnt, skp = header_loads(policy, maxv, walls, [o], [motion], P, V, Q, mass, step,
                                                     damping, tau0, tau1, L.QUANTUM_LOG2)
                ev, eq, row = M.integrate_respond(maxv, walls, [o], [motion], P, V, Q, step, damping, tau0, tau1,
                                                  mass)
                assert same_bits_nan(hv, ev) and same_bits_nan(hq, eq)
                assert row.same(imp, cnt, skp), (kind, start, stop, walls)
                if not walls:
                    total += P.shape[0]
                    responses += int(cnt[6] + skp[6])
    assert total >= 100000 and responses > 10000


def test_single_moving_obstacle_records_the_momentum_it_takes(policy):
    """one moving obstacle, no walls: the row's impulse is the sum of m * (v_in - v_out) over the particles
    inside it, term by term in quanta"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(41)
    dt, damping = F32(0.004), F32(0.6)
    o = O.Sphere((0.3, -0.2, 0.1), 0.8)
    motion = O.Motion((40.0, -15.0, 5.0), 0.05, 1.0)
    tau0 = F32(0.3)
    tau1 = F32(tau0 + dt)
    P, V, Q = moving_cases(o, motion, tau0, tau1, 50000, dt, rng)
    mass = rng.uniform(0.5, 2.0, P.shape[0]).astype(F32)
    hv, hq, imp, cnt, skp = header_loads(policy, F32([9, 9, 9]), False, [o], [motion], P, V, Q, mass, dt, damping,
                                         tau0, tau1, L.QUANTUM_LOG2)
    act = E.inside(M.shifted(o, M.displacement(motion, tau1)), Q)
    q, ok = L.term(mass, V, hv, L.QUANTUM_LOG2)
    act, big = act & ok, act & ~ok            # (a term of 2^38 quanta or more is skipped, and counted as such)
    assert np.array_equal(imp[6], q[act].sum(0)) and cnt[6] == act.sum() > 5000 and skp[6] == big.sum()
    assert not imp[:6].any() and not imp[7:].any()
    want = (mass.astype(np.float64)[:, None] * (V.astype(np.float64) - hv.astype(np.float64)))[act].sum(0)
    got = imp[6] * 2.0 ** L.QUANTUM_LOG2
    bound = cnt[6] * 2.0 ** L.QUANTUM_LOG2 + 2.0 ** -22 * (mass[:, None] * (np.abs(V) + np.abs(hv)))[act].sum(0)
    assert (np.abs(got - want) <= bound).all()


# ---- routes -------------------------------------------------------------------------------------

def test_routes(policy):
    for n_obst in (0, 1, 3, 64):
        for n_moving in (0, 1, 3, 64):
            assert bool(policy.moving_kernels(n_obst, n_moving)) == (n_obst > 0 and n_moving > 0)
    # the existing decisions, with their argument lists as they were
    for hash_too in (0, 1):
        for tiled in (0, 1):
            for n in (0, 5):
                for no_fused in (0, 1):
                    for n_obst in (0, 1, 64):
                        base = bool(hash_too and tiled and n > 0 and not no_fused and n_obst == 0)
                        assert bool(policy.fused_integrate5(hash_too, tiled, n, no_fused, n_obst)) == base
                        assert bool(policy.fused_integrate6(hash_too, tiled, n, no_fused, n_obst, 0)) == base
                        assert not policy.fused_integrate6(hash_too, tiled, n, no_fused, n_obst, 1)
    for no_fused_slab in (0, 1):
        for n_obst in (0, 1, 64):
            base = not no_fused_slab and n_obst == 0
            assert bool(policy.fused_slab2(no_fused_slab, n_obst)) == base
            assert bool(policy.fused_slab3(no_fused_slab, n_obst, 0)) == base
            assert not policy.fused_slab3(no_fused_slab, n_obst, 1)


# ---- Python side --------------------------------------------------------------------------------

def test_motion_round_trips():
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    m = O.Motion((0.25, -3.0, 1e-3), 0.125, 2.5)
    st = m.as_struct()
    assert [st.velocity[0], st.velocity[1], st.start, st.stop] == [0.25, -3.0, 0.125, 2.5]
    assert O.motion_from_struct(st) == m and m.moves()
    d = O.Motion((1, 0, 0))
    assert d.start == 0.0 and d.stop == math.inf and d.as_struct().stop == math.inf
    arr, n = O.as_motion_array([m, None, st])
    assert n == 3 and bytes(arr[0]) == bytes(st) == bytes(arr[2])
    rest = O.motion_from_struct(arr[1])
    assert not rest.moves() and rest == O.Motion((0, 0, 0))
    assert O.as_motion_array([])[1] == 0
    assert same_bits(m.displacement(1.0), M.displacement(st, 1.0))
    assert "Motion" in repr(m)


def test_gate_scene(hiplib):
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass, obst, motions = scenes.dam_break_gate(20000, 0.5)
    gate, lift = obst[0], motions[0]
    assert len(obst) == len(motions) == 1 and pos.size == 3 * mass.size == vel.size
    assert p.apply_gravity == 1 and p.apply_walls == 1 and p.gravity[1] < 0
    x = pos.reshape(-1, 3)
    assert not (gate.signed_distance(x) < 0).any()
    h = float(p.h)
    assert float(gate.lo[0]) - x[:, 0].max() == pytest.approx(h, rel=0.05)      # one kernel radius from the face
    assert lift.moves() and lift.velocity[1] == F32(0.5) and not lift.velocity[[0, 2]].any()
    up = lift.displacement(1e9)
    assert float(gate.lo[1]) + float(up[1]) > x[:, 1].max()                     # clear of the column, then at rest
    assert same_bits(lift.displacement(float(lift.stop)), up)
