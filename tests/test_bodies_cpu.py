"""CPU checks of the free bodies (include/sph_hip.h: sph_hip_set_bodies): the struct layouts, every refusal of
the check functions, the advance and the body's turn of csrc/body_policy.h (compiled with g++ behind an
extern "C" shim) against the numpy restatement tests/body_emulation.py bit for bit, the anchors to the static
and the moving response, the route decision of csrc/launch_policy.h, the quantum rule in both directions, and
the Python side (obstacles.Body, scenes.dam_break_debris)."""
import ctypes as C
import math

import numpy as np
import pytest

import body_emulation as B
import load_emulation as L
import moving_obstacle_emulation as M
import obstacle_emulation as E
from helpers import compile_shim
from test_loads_cpu import same_bits as same_bits_nan
from test_moving_obstacles_cpu import _motion_for, moving_cases
from test_obstacles_cpu import _obstacle_set, same_bits

F32 = np.float32

SHIM = r"""
#include <stddef.h>
#include "body_policy.h"
#include "launch_policy.h"

extern "C" {
const char* check(const sph_hip_body* list, int n, int n_obstacles, const sph_hip_obstacle_motion* motion, int n_motion,
                  int quantum_log2)
{
   const char* why = body_check(list, n, n_obstacles, motion, n_motion, quantum_log2);
   return why ? why : "";
}
const char* motion_check(const sph_hip_obstacle_motion* motion, int n_motion, const sph_hip_body* bodies, int n_bodies)
{
   const char* why = body_motion_check(motion, n_motion, bodies, n_bodies);
   return why ? why : "";
}
const char* refuses_recording(int n_bodies, int body_quantum, int rows, int quantum_log2)
{
   const char* why = body_refuses_recording(n_bodies, body_quantum, rows, quantum_log2);
   return why ? why : "";
}
const char* refuses_bodies(int rows_left, int recording_quantum, int n_bodies, int quantum_log2)
{
   const char* why = recording_refuses_bodies(rows_left, recording_quantum, n_bodies, quantum_log2);
   return why ? why : "";
}
int count(const sph_hip_body* list, int n) { return bodies_count(list, n); }
void initial(const sph_hip_body* b, BodyState* s) { *s = body_initial(*b); }
// m cases: body k, state k, its obstacle index idx[k], the impulse q[3k..] and skipped count sk[k] of that
// column in an otherwise empty row (has_row[k] == 0: a null row), quantum e[k], time step dt[k]
void advance(const sph_hip_body* bodies, BodyState* states, const int* idx, const long long* q, const long long* sk,
             const int* has_row, const int* e, const float* dt, int m)
{
   for (int k = 0; k < m; k++) {
      long long row[LOAD_ROW_WORDS] = {0};
      for (int c = 0; c < 3; c++) row[3 * (6 + idx[k]) + c] = q[3 * k + c];
      row[LOAD_ROW_SKIPPED + 6 + idx[k]] = sk[k];
      body_advance(bodies[k], states[k], has_row[k] ? row : nullptr, idx[k], e[k], dt[k]);
   }
}
void respond(const float* maxv, int apply_walls, const sph_hip_obstacle* list, const sph_hip_obstacle_motion* motion,
             const sph_hip_body* bodies, const BodyState* states, int n, int m, const float* p, float* v, float* q,
             const float* mass, float dt, float damping, float tau0, float tau1, int quantum_log2, long long* row)
{
   const LoadRowAdder rec = {row, load_scale(quantum_log2)};
   for (int i = 0; i < m; i++) {
      if (apply_walls) load_walls_respond(maxv, damping, p + 3 * i, v + 3 * i, dt, q + 3 * i, mass[i], rec);
      body_obstacles_respond(list, motion, bodies, states, n, p + 3 * i, v + 3 * i, q + 3 * i, dt, damping, tau0, tau1,
                             mass[i], rec);
   }
}
// the contract's one line, for one obstacle: returns how many rows were inside
int turn(const sph_hip_obstacle* o, const BodyState* s, int m, const float* p, float* v, float* q, float dt,
         float damping)
{
   int in = 0;
   for (int i = 0; i < m; i++) in += body_turn(*o, *s, p + 3 * i, v + 3 * i, q + 3 * i, dt, damping) ? 1 : 0;
   return in;
}
void respond_moving(const float* maxv, int apply_walls, const sph_hip_obstacle* list,
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
int body_kernels(int n_obst, int n_bodies) { return use_body_kernels(n_obst, n_bodies); }
int moving_kernels(int n_obst, int n_moving) { return use_moving_kernels(n_obst, n_moving); }
int fused_integrate(int hash_too, int tiled, int n, int no_fused, int n_obst, int record)
{
   return fuse_integrate(hash_too != 0, tiled != 0, n, no_fused != 0, n_obst, record != 0);
}
int fused_slab(int no_fused_slab, int n_obst, int record) { return fuse_slab_step(no_fused_slab != 0, n_obst, record != 0); }
#define OFF(f) (long long)offsetof(sph_hip_body, f)
#define SOFF(f) (long long)offsetof(sph_hip_body_state, f)
#define DOFF(f) (long long)offsetof(BodyState, f)
void layout(long long* out)
{
   out[0] = sizeof(sph_hip_body);
   out[1] = OFF(mass); out[2] = OFF(velocity); out[3] = OFF(accel); out[4] = OFF(free_axes);
   out[5] = OFF(travel_lo); out[6] = OFF(travel_hi);
   out[7] = sizeof(sph_hip_body_state);
   out[8] = SOFF(displacement); out[9] = SOFF(velocity); out[10] = SOFF(skipped); out[11] = SOFF(steps);
   out[12] = SPH_HIP_ABI_VERSION;
   out[13] = sizeof(BodyState);
   out[14] = DOFF(D); out[15] = DOFF(Dprev); out[16] = DOFF(V); out[17] = DOFF(skipped); out[18] = DOFF(steps);
}
}
"""


class DevState(C.Structure):
    """Mirror of csrc/body_policy.h's BodyState"""

    _fields_ = [("D", C.c_float * 3), ("Dprev", C.c_float * 3), ("V", C.c_float * 3), ("unused", C.c_float),
                ("skipped", C.c_int64), ("steps", C.c_int64)]


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    from smoothed_particle_hydrodynamics_amd.obstacles import SphBody, SphObstacle, SphObstacleMotion
    lib = compile_shim(SHIM, ["-O2", "-ffp-contract=off"], tmp_path_factory)
    PO, PM, PB, PS, V = (C.POINTER(SphObstacle), C.POINTER(SphObstacleMotion), C.POINTER(SphBody),
                         C.POINTER(DevState), C.c_void_p)
    lib.check.argtypes = [PB, C.c_int, C.c_int, PM, C.c_int, C.c_int]
    lib.motion_check.argtypes = [PM, C.c_int, PB, C.c_int]
    lib.refuses_recording.argtypes = [C.c_int] * 4
    lib.refuses_bodies.argtypes = [C.c_int] * 4
    for f in (lib.check, lib.motion_check, lib.refuses_recording, lib.refuses_bodies):
        f.restype = C.c_char_p
    lib.count.argtypes = [PB, C.c_int]
    lib.initial.argtypes = [PB, PS]
    lib.advance.argtypes = [PB, PS, V, V, V, V, V, V, C.c_int]
    lib.respond.argtypes = [V, C.c_int, PO, PM, PB, PS, C.c_int, C.c_int, V, V, V, V, C.c_float, C.c_float, C.c_float,
                            C.c_float, C.c_int, V]
    lib.turn.argtypes = [PO, PS, C.c_int, V, V, V, C.c_float, C.c_float]
    lib.respond_moving.argtypes = [V, C.c_int, PO, PM, C.c_int, C.c_int, V, V, V, V, C.c_float, C.c_float, C.c_float,
                                   C.c_float, C.c_int, V]
    lib.layout.argtypes = [C.POINTER(C.c_longlong)]
    return lib


def dev_states(st):
    """a ctypes array of BodyState from a B.State"""
    n = st.steps.size
    arr = (DevState * max(1, n))()
    for i in range(n):
        arr[i].D[:] = [float(x) for x in st.D[i]]
        arr[i].Dprev[:] = [float(x) for x in st.Dprev[i]]
        arr[i].V[:] = [float(x) for x in st.V[i]]
        arr[i].skipped, arr[i].steps = int(st.skipped[i]), int(st.steps[i])
    return arr


def _arrays(P, V, Q):
    p = np.ascontiguousarray(P, F32).reshape(-1, 3)
    return p, np.ascontiguousarray(V, F32).reshape(-1, 3).copy(), np.ascontiguousarray(Q, F32).reshape(-1, 3).copy()


def _row_parts(row):
    S = L.SOLIDS
    return row[:3 * S].reshape(S, 3), row[3 * S:4 * S], row[4 * S:]


def header_respond(lib, maxv, apply_walls, obst, motions, bodies, st, P, V, Q, mass, dt, damping, tau0, tau1, e):
    """body_obstacles_respond with the header's serial recorder: (V, Q, impulse, count, skipped)"""
    from smoothed_particle_hydrodynamics_amd.obstacles import as_array, as_body_array, as_motion_array
    arr, n = as_array(obst)
    mot = as_motion_array(motions)[0] if motions else None
    bod, _ = as_body_array(bodies)
    maxv = np.ascontiguousarray(maxv, F32)
    p, v, q = _arrays(P, V, Q)
    m = np.ascontiguousarray(mass, F32)
    row = np.zeros(5 * L.SOLIDS, np.int64)
    lib.respond(maxv.ctypes.data, int(apply_walls), arr, mot, bod, dev_states(st), n, p.shape[0], p.ctypes.data,
                v.ctypes.data, q.ctypes.data, m.ctypes.data, dt, damping, tau0, tau1, int(e), row.ctypes.data)
    return (v, q) + _row_parts(row)


def header_moving(lib, maxv, apply_walls, obst, motions, P, V, Q, mass, dt, damping, tau0, tau1, e):
    from smoothed_particle_hydrodynamics_amd.obstacles import as_array, as_motion_array
    arr, n = as_array(obst)
    mot, _ = as_motion_array(motions)
    maxv = np.ascontiguousarray(maxv, F32)
    p, v, q = _arrays(P, V, Q)
    m = np.ascontiguousarray(mass, F32)
    row = np.zeros(5 * L.SOLIDS, np.int64)
    lib.respond_moving(maxv.ctypes.data, int(apply_walls), arr, mot, n, p.shape[0], p.ctypes.data, v.ctypes.data,
                       q.ctypes.data, m.ctypes.data, dt, damping, tau0, tau1, int(e), row.ctypes.data)
    return (v, q) + _row_parts(row)


def header_advance_one(lib, body, state, i, q, skipped, has_row, e, dt):
    """one body_advance of the header on ctypes structs `body` and `state` (in place)"""
    idx, q, sk = np.array([i], np.int32), np.ascontiguousarray(q, np.int64), np.array([skipped], np.int64)
    has, e, dt = np.array([int(has_row)], np.int32), np.array([e], np.int32), np.array([dt], F32)
    lib.advance(C.pointer(body), C.pointer(state), idx.ctypes.data, q.ctypes.data, sk.ctypes.data, has.ctypes.data,
                e.ctypes.data, dt.ctypes.data, 1)


# ---- layout, refusals, routes, the quantum rule -------------------------------------------------

def test_struct_layout_and_abi(policy):
    from smoothed_particle_hydrodynamics_amd import lib as Lb
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    out = (C.c_longlong * 19)()
    policy.layout(out)
    assert list(out) == [56, 0, 4, 16, 28, 32, 44, 40, 0, 12, 24, 32, 7, 56, 0, 12, 24, 40, 48]
    assert C.sizeof(O.SphBody) == 56 and C.sizeof(O.SphBodyState) == 40 and C.sizeof(DevState) == 56
    assert [getattr(O.SphBody, f).offset for f, _ in O.SphBody._fields_] == [0, 4, 16, 28, 32, 44]
    assert [getattr(O.SphBodyState, f).offset for f, _ in O.SphBodyState._fields_] == [0, 12, 24, 32]
    assert Lb.ABI_VERSION == 7
    assert Lb.PROTOTYPES["sph_hip_set_bodies"] == (C.c_int, [C.c_void_p, C.POINTER(O.SphBody), C.c_int, C.c_int])
    res, args = Lb.PROTOTYPES["sph_hip_get_bodies"]
    assert res is C.c_int and len(args) == 4


def test_entry_points_exist_and_refuse_a_null_context(hiplib):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    arr, n = O.as_body_array([O.Body(1.0)])
    assert hiplib.sph_hip_set_bodies(None, arr, n, -24) == -1
    st = (O.SphBodyState * 1)()
    assert hiplib.sph_hip_get_bodies(None, arr, st, 1) == -1


def test_refusals(policy):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    inf, nan = math.inf, math.nan

    def why(bodies, n_obst=None, motions=(), e=-24):
        arr, n = O.as_body_array(bodies)
        mot, nm = O.as_motion_array(motions)
        return policy.check(arr, n, len(bodies) if n_obst is None else n_obst, mot if nm else None, nm, e)

    good = O.Body(2.0, (1, 2, 3), (0, -9.8, 0), (True, False, True), (-inf, -1, 0), (inf, 0, 2))
    assert why([good, None, good]) == b"" and why([]) == b"" and why([], n_obst=3) == b""
    assert why([None, None]) == b""
    assert why([O.Body(1e-38), O.Body(3e38)]) == b""
    assert b"obstacle count" in why([good], n_obst=2) and b"obstacle count" in why([good, good], n_obst=1)
    assert policy.check(None, 2, 2, None, 0, -24) == b"null body list"
    assert b"quantum_log2" in why([good], e=-65) and b"quantum_log2" in why([good], e=33)
    assert why([good], e=-64) == b"" and why([good], e=32) == b""
    for mass in (-1.0, inf, -inf, nan):
        assert b"mass" in why([O.Body(mass)]), mass
    for c in range(3):
        for bad in (inf, -inf, nan):
            v = [0.0, 0.0, 0.0]
            v[c] = bad
            assert b"velocity" in why([O.Body(1.0, velocity=v)])
            assert b"accel" in why([O.Body(1.0, accel=v)])
        lo, hi = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
        lo[c] = 0.5
        assert b"travel" in why([O.Body(1.0, travel_lo=lo)])
        hi[c] = -0.5
        assert b"travel" in why([O.Body(1.0, travel_hi=hi)])
        lo[c] = nan
        assert b"travel" in why([O.Body(1.0, travel_lo=lo)])
        hi[c] = nan
        assert b"travel" in why([O.Body(1.0, travel_hi=hi)])
    assert why([O.Body(1.0, travel_lo=(-0.0, 0, 0), travel_hi=(0.0, -0.0, 0))]) == b""
    s = O.Body(1.0).as_struct()
    for bits in (8, 15, 1 << 31):
        s.free_axes = bits
        assert b"free_axes" in why([s])
    for bits in range(8):
        s.free_axes = bits
        assert why([s]) == b""
    # a field of an entry that is not a body is not looked at
    z = O.SphBody()
    z.velocity[0] = nan
    z.free_axes = 99
    assert why([z]) == b""
    # a body and a motion that moves exclude each other, in both directions
    moving, resting = O.Motion((1, 0, 0)), O.Motion((0, 0, 0), 0.1, 0.2)
    assert b"motion moves" in why([good, None], motions=[moving, None])
    assert why([good, None], motions=[resting, moving]) == b"" and why([good, None], motions=[None, moving]) == b""

    def motion_why(motions, bodies):
        mot, nm = O.as_motion_array(motions)
        arr, n = O.as_body_array(bodies)
        return policy.motion_check(mot, nm, arr, n)

    assert b"is a body" in motion_why([moving, None], [good, None])
    assert motion_why([resting, moving], [good, None]) == b"" and motion_why([], [good, None]) == b""
    assert motion_why([moving, moving], []) == b""
    arr, n = O.as_body_array([good, None, O.Body(1.0), z])
    assert policy.count(arr, n) == 2 and policy.count(arr, 0) == 0


def test_quantum_rule_in_both_directions(policy):
    """while bodies are set a recording with another quantum is refused; bodies are refused while a recording
    with another quantum has rows left"""
    for e in (-64, -24, 0, 32):
        for other in (-30, -24, 5):
            refused = other != e
            assert (policy.refuses_recording(2, e, 10, other) != b"") == refused
            assert policy.refuses_recording(0, e, 10, other) == b""      # no bodies: any quantum
            assert policy.refuses_recording(2, e, 0, other) == b""       # rows = 0 stops a recording
            assert (policy.refuses_bodies(3, other, 1, e) != b"") == refused
            assert policy.refuses_bodies(0, other, 1, e) == b""          # a recording that is used up
            assert policy.refuses_bodies(3, other, 0, e) == b""          # a list without a body


def test_routes(policy):
    """use_body_kernels next to the unchanged decisions"""
    for n_obst in (0, 1, 64):
        for k in (0, 1, 3):
            assert bool(policy.body_kernels(n_obst, k)) == (n_obst > 0 and k > 0)
            assert bool(policy.moving_kernels(n_obst, k)) == (n_obst > 0 and k > 0)
    for hash_too in (0, 1):
        for tiled in (0, 1):
            for n in (0, 5):
                for no_fused in (0, 1):
                    for n_obst in (0, 2):
                        base = bool(hash_too and tiled and n > 0 and not no_fused and n_obst == 0)
                        assert bool(policy.fused_integrate(hash_too, tiled, n, no_fused, n_obst, 0)) == base
                        assert not policy.fused_integrate(hash_too, tiled, n, no_fused, n_obst, 1)
    for no_fused_slab in (0, 1):
        for n_obst in (0, 1):
            assert bool(policy.fused_slab(no_fused_slab, n_obst, 0)) == (not no_fused_slab and n_obst == 0)
            assert not policy.fused_slab(no_fused_slab, n_obst, 1)
    # a list with a body has an obstacle: every fused route is already off
    assert not policy.fused_integrate(1, 1, 5, 0, 1, 0) and not policy.fused_slab(0, 1, 0)


# ---- the advance, header vs numpy ---------------------------------------------------------------

def advance_cases(m, rng):
    """m random advances: impulses up to 2^62 of both signs, masses across the fp32 range, stops that are hit,
    straddled, infinite and zero, masked axes, null rows, dt == 0, non-zero skipped"""
    from smoothed_particle_hydrodynamics_amd.obstacles import SphBody
    big = rng.random(m) < 0.5
    mass = np.where(big, np.exp2(rng.uniform(-126, 127, m)), np.exp2(rng.uniform(-4, 14, m))).astype(F32)
    mass[mass == 0] = F32(1.0)
    mag = np.floor(np.exp2(rng.uniform(0, 62, (m, 3)))).astype(np.int64)
    q = np.where(rng.random((m, 3)) < 0.5, -mag, mag)
    q[rng.random((m, 3)) < 0.05] = 0
    q[: m // 100] = np.int64(2 ** 62) * rng.choice([-1, 1], (m // 100, 3))
    e = rng.integers(-64, 33, m).astype(np.int32)
    dt = np.exp2(rng.uniform(-12, 0, m)).astype(F32)
    dt[rng.random(m) < 0.05] = 0.0
    accel = (rng.normal(0, 10, (m, 3)) * (rng.random((m, 3)) < 0.7)).astype(F32)
    D = (rng.normal(0, 0.3, (m, 3))).astype(F32)
    V = (rng.normal(0, 30, (m, 3)) * (rng.random((m, 3)) < 0.9)).astype(F32)
    span_lo = np.exp2(rng.uniform(-10, 1, (m, 3))).astype(F32)
    span_hi = np.exp2(rng.uniform(-10, 1, (m, 3))).astype(F32)
    lo = np.where(rng.random((m, 3)) < 0.25, -np.inf, -span_lo).astype(F32)
    hi = np.where(rng.random((m, 3)) < 0.25, np.inf, span_hi).astype(F32)
    lo[rng.random((m, 3)) < 0.1] = 0.0
    hi[rng.random((m, 3)) < 0.1] = 0.0
    D = np.clip(D, lo, hi).astype(F32)               # a state the advance itself can have left
    free = rng.random((m, 3)) < 0.75
    has_row = (rng.random(m) < 0.9).astype(np.int32)
    sk = np.where(rng.random(m) < 0.3, rng.integers(1, 1 << 40, m), 0).astype(np.int64)
    idx = rng.integers(0, 64, m).astype(np.int32)
    bodies = (SphBody * m)()
    states = (DevState * m)()
    steps0 = rng.integers(0, 1 << 40, m)
    skipped0 = rng.integers(0, 1 << 40, m)
    for k in range(m):
        b, s = bodies[k], states[k]
        b.mass = float(mass[k])
        b.accel[:] = [float(x) for x in accel[k]]
        b.free_axes = int(free[k, 0]) | int(free[k, 1]) << 1 | int(free[k, 2]) << 2
        b.travel_lo[:] = [float(x) for x in lo[k]]
        b.travel_hi[:] = [float(x) for x in hi[k]]
        s.D[:] = [float(x) for x in D[k]]
        s.V[:] = [float(x) for x in V[k]]
        s.Dprev[:] = [9.0, 9.0, 9.0]
        s.steps, s.skipped = int(steps0[k]), int(skipped0[k])
    return dict(mass=mass, q=q, e=e, dt=dt, accel=accel, D=D, V=V, lo=lo, hi=hi, free=free, has_row=has_row, sk=sk,
                idx=idx, bodies=bodies, states=states, steps0=steps0, skipped0=skipped0)


def test_advance_header_equals_numpy_bit_for_bit(policy):
    rng = np.random.default_rng(1700)
    m = 120000
    c = advance_cases(m, rng)
    c["q"] = np.ascontiguousarray(c["q"], np.int64)
    policy.advance(c["bodies"], c["states"], c["idx"].ctypes.data, c["q"].ctypes.data,
                   c["sk"].ctypes.data, c["has_row"].ctypes.data, c["e"].ctypes.data, c["dt"].ctypes.data, m)
    got = np.frombuffer(c["states"], dtype=np.dtype([("D", F32, 3), ("Dprev", F32, 3), ("V", F32, 3), ("u", F32),
                                                      ("skipped", np.int64), ("steps", np.int64)]))
    q = np.where(c["has_row"][:, None] != 0, c["q"], 0)
    D, V = B.advance_arrays(c["mass"], c["accel"], c["free"], c["lo"], c["hi"], c["D"], c["V"], q, c["e"], c["dt"])
    assert same_bits_nan(got["D"], D) and same_bits_nan(got["V"], V)
    assert same_bits(got["Dprev"], c["D"])
    assert np.array_equal(got["steps"], c["steps0"] + 1)
    assert np.array_equal(got["skipped"], c["skipped0"] + np.where(c["has_row"] != 0, c["sk"], 0))
    # a masked component is untouched; the cases do reach what they are meant to
    masked = ~c["free"]
    assert same_bits(got["D"][masked], c["D"][masked]) and same_bits(got["V"][masked], c["V"][masked])
    free = c["free"]
    at_lo = free & (D == c["lo"]) & (V == 0) & (c["D"] != c["lo"])
    at_hi = free & (D == c["hi"]) & (V == 0) & (c["D"] != c["hi"])
    moved = free & np.isfinite(D) & (D != c["D"]) & (D > c["lo"]) & (D < c["hi"])
    assert at_lo.sum() > 5000 and at_hi.sum() > 5000 and moved.sum() > 50000, (at_lo.sum(), at_hi.sum(), moved.sum())
    assert (np.abs(c["q"]) == 2 ** 62).any() and (c["has_row"] == 0).sum() > 5000 and (c["dt"] == 0).sum() > 2000
    assert ((c["sk"] != 0) & (c["has_row"] != 0)).sum() > 10000
    assert (~np.isfinite(V)).any() and (np.abs(V[np.isfinite(V)]) > 1e30).any(), "masses across the fp32 range"


def test_advance_of_a_list_equals_the_per_body_restatement(policy):
    """B.advance (what the GPU tests step with) against the header, entry by entry, non-bodies skipped"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(5)
    bodies = [O.Body(40.0, (3, -2, 1), (0, -9.8, 0), (True, True, False), (-0.01, -0.5, 0), (0.02, 0.5, 0)), None,
              O.Body(7.5, (0, 0, 4), (1, 0, 0), (False, False, True))]
    st = B.State(bodies)
    arr, n = O.as_body_array(bodies)
    dev = (DevState * n)()
    for i in range(n):
        policy.initial(C.pointer(arr[i]), C.pointer(dev[i]))
    for k in range(40):
        row = None
        if k > 0:
            row = L.Row(-20)
            row.impulse[6:9] = rng.integers(-2 ** 30, 2 ** 30, (3, 3))
            row.skipped[6:9] = rng.integers(0, 3, 3)
        st = B.advance(bodies, st, row, -20, 0.001)
        for i in range(n):
            q = row.impulse[6 + i] if row is not None else np.zeros(3, np.int64)
            header_advance_one(policy, arr[i], dev[i], i, q, row.skipped[6 + i] if row is not None else 0,
                               row is not None, -20, 0.001)
            assert same_bits(list(dev[i].D), st.D[i]) and same_bits(list(dev[i].V), st.V[i]), (k, i)
            assert same_bits(list(dev[i].Dprev), st.Dprev[i])
            assert dev[i].steps == st.steps[i] and dev[i].skipped == st.skipped[i]
    assert st.steps.tolist() == [40, 0, 40] and not st.D[1].any() and not st.V[1].any()
    assert st.D[0, 0] in (F32(-0.01), F32(0.02)) or st.V[0, 0] != 0     # the first body reaches a stop on x
    assert st.D[0, 2] == 0 and st.V[0, 2] == 0 and st.D[2, 0] == 0, "a masked component stays at zero"


def test_a_body_on_a_stop_pushed_into_it_stays_there(policy):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    bodies = [O.Body(5.0, accel=(0.0, -9.8, 3.0), travel_lo=(0.0, 0.0, -1.0), travel_hi=(0.0, 1.0, 0.0))]
    st = B.State(bodies)
    arr, _ = O.as_body_array(bodies)
    dev = DevState()
    policy.initial(arr, C.pointer(dev))
    for k in range(25):
        st = B.advance(bodies, st, None, -24, 0.01)
        header_advance_one(policy, arr[0], dev, 0, np.zeros(3, np.int64), 0, False, -24, 0.01)
        for D, V in ((st.D[0], st.V[0]), (np.array(list(dev.D), F32), np.array(list(dev.V), F32))):
            assert same_bits(D, np.zeros(3, F32)) and same_bits(V, np.zeros(3, F32)), k
    assert st.steps[0] == 25 == dev.steps


# ---- the body's turn and its recorder -----------------------------------------------------------

@pytest.mark.parametrize("kind", [E.SPHERE, E.BOX, E.CYLINDER], ids=["sphere", "box", "cylinder"])
def test_body_turn_equals_the_moving_turn_fed_the_same_shifts(policy, kind):
    """header against header and against numpy: a body whose state holds D0 = D(tau0), D1 = D(tau1) of a
    motion responds and records exactly as load_obstacles_respond_moving does under that motion"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(3100 + kind)
    dt, damping, e = F32(0.004), F32(0.6), -24
    maxv = F32([1e9, 1e9, 1e9])
    inside = 0
    for o in _obstacle_set(kind, rng)[:6]:
        t0 = F32(rng.uniform(0.05, 0.2))
        for tau0, tau1, step in ((t0, F32(t0 + dt), dt), (t0, t0, F32(0.0))):
            motion = _motion_for(o, rng, 0.0, math.inf)
            P, V, Q = moving_cases(o, motion, tau0, tau1, 3000, dt, rng)
            mass = rng.uniform(0.5, 2.0, P.shape[0]).astype(F32)
            bodies = [O.Body(3.0)]
            st = B.State(bodies)
            st.Dprev[0], st.D[0] = M.displacement(motion, tau0), M.displacement(motion, tau1)
            hv, hq, hi, hc, hs = header_respond(policy, maxv, 0, [o], [], bodies, st, P, V, Q, mass, step, damping,
                                                tau0, tau1, e)
            mv, mq, mi, mc, ms = header_moving(policy, maxv, 0, [o], [motion], P, V, Q, mass, step, damping, tau0,
                                               tau1, e)
            assert same_bits(hv, mv) and same_bits(hq, mq)
            assert np.array_equal(hi, mi) and np.array_equal(hc, mc) and np.array_equal(hs, ms)
            ev, eq, row = B.integrate_respond(maxv, 0, [o], [], bodies, st, P, V, Q, step, damping, tau0, tau1, mass, e)
            assert same_bits(hv, ev) and same_bits(hq, eq) and row.same(hi, hc, hs)
            # the contract's one line
            p, v, q = _arrays(P, V, Q)
            arr, _ = O.as_array([o])
            n_in = policy.turn(arr, dev_states(st), p.shape[0], p.ctypes.data, v.ctypes.data, q.ctypes.data, step,
                               damping)
            assert same_bits(v, hv) and same_bits(q, hq) and n_in == hc[6] + hs[6]
            inside += n_in
    assert inside > 5000, inside


def test_mixed_list_header_equals_numpy(policy):
    """a body, an entry under a motion and one at rest in one list, walls on, with and without a motion list"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(77)
    obst = [O.Sphere((0.5, 0.5, 0.5), 0.2), O.Box((0.55, 0.3, 0.3), (0.9, 0.7, 0.8)), O.Cylinder(1, (0.3, 0, 0.7), 0.15, 0.1, 0.9)]
    bodies = [None, O.Body(50.0, free=(True, True, False)), None]
    st = B.State(bodies)
    st.Dprev[1], st.D[1] = F32([0.01, -0.02, 0]), F32([0.03, -0.01, 0])
    dt, damping = F32(0.002), F32(0.5)
    m = 30000
    P = rng.uniform(-0.02, 1.02, (m, 3)).astype(F32)
    V = rng.normal(0, 40, (m, 3)).astype(F32)
    Q = (P + V * dt).astype(F32)
    mass = rng.uniform(0.5, 2.0, m).astype(F32)
    maxv = F32([1, 1, 1])
    for motions in ([O.Motion((0, 30, 0)), None, O.Motion((0, 0, 0))], []):
        hv, hq, hi, hc, hs = header_respond(policy, maxv, 1, obst, motions, bodies, st, P, V, Q, mass, dt, damping,
                                            0.01, F32(0.01) + dt, -24)
        ev, eq, row = B.integrate_respond(maxv, 1, obst, motions, bodies, st, P, V, Q, dt, damping, 0.01,
                                          F32(0.01) + dt, mass, -24)
        assert same_bits_nan(hv, ev) and same_bits_nan(hq, eq) and row.same(hi, hc, hs)
        assert (hc[6:9] > 100).all() and hc[:6].sum() > 100, hc[:9]


def test_no_free_axis_is_the_static_list(policy):
    """free_axes = 0: the shifts stay zero, and the turn is the static response bit for bit"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(78)
    obst = [O.Sphere((0.5, 0.5, 0.5), 0.2), O.Box((0.55, 0.3, 0.3), (0.9, 0.7, 0.8)), O.Cylinder(1, (0.3, 0, 0.7), 0.15, 0.1, 0.9)]
    bodies = [O.Body(5.0, (1, 2, 3), (0, -9.8, 0), (False, False, False)) for _ in obst]
    st = B.State(bodies)
    row = L.Row()
    row.impulse[6:9] = 1 << 40
    for _ in range(3):
        st = B.advance(bodies, st, row, -24, 0.002)
    assert not st.D.any() and not st.Dprev.any() and not st.V.any() and st.steps.tolist() == [3, 3, 3]
    dt, damping = F32(0.002), F32(0.5)
    m = 30000
    P = rng.uniform(-0.02, 1.02, (m, 3)).astype(F32)
    V = rng.normal(0, 40, (m, 3)).astype(F32)
    Q = (P + V * dt).astype(F32)
    mass = np.ones(m, F32)
    maxv = F32([1, 1, 1])
    hv, hq, hi, hc, hs = header_respond(policy, maxv, 1, obst, [], bodies, st, P, V, Q, mass, dt, damping, 0.0, dt, -24)
    ev, eq, want = L.respond(maxv, 1, obst, P, V, Q, dt, damping, mass)
    assert same_bits_nan(hv, ev) and same_bits_nan(hq, eq) and want.same(hi, hc, hs)
    assert (hc[6:9] > 100).all()


# ---- Python side --------------------------------------------------------------------------------

def test_body_round_trips():
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    b = O.Body(12.5, (1, -2, 0.5), (0, -9.81, 0), (True, False, True), (-1, 0, -math.inf), (2, 0, math.inf))
    s = b.as_struct()
    assert s.mass == 12.5 and s.free_axes == 5 and s.travel_hi[2] == math.inf and list(s.velocity) == [1, -2, 0.5]
    assert O.body_from_struct(s) == b and "Body" in repr(b)
    d = O.Body(3.0)
    assert d.free_axes == 7 and list(d.travel_lo) == [-math.inf] * 3 and list(d.travel_hi) == [math.inf] * 3
    arr, n = O.as_body_array([b, None, s])
    assert n == 3 and bytes(arr[0]) == bytes(s) == bytes(arr[2]) and bytes(arr[1]) == bytes(56)
    assert O.body_from_struct(arr[1]) is None and O.as_body_array([])[1] == 0
    assert B.is_body(b) and not B.is_body(None) and not B.is_body(arr[1])


def test_debris_scene(hiplib):
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass, obst, bodies = scenes.dam_break_debris(20000)
    box, body = obst[0], bodies[0]
    assert len(obst) == len(bodies) == 1 and pos.size == 3 * mass.size == vel.size
    assert p.apply_gravity == 1 and p.apply_walls == 1 and p.gravity[1] < 0
    x = pos.reshape(-1, 3)
    assert not (box.signed_distance(x) < 0).any()
    h = float(p.h)
    assert float(box.lo[0]) - x[:, 0].max() == pytest.approx(3.0 * h, rel=0.05)     # downstream of the column
    assert float(box.lo[1]) == 0.0                                                  # on the floor
    assert body.free == (True, False, False) and not body.velocity.any() and not body.accel.any()
    assert body.travel_lo[0] == 0 and float(box.hi[0]) + float(body.travel_hi[0]) <= float(p.max_x) - 0.99 * h
    column = 0.1 * 0.75 * 1.0
    size = (box.hi - box.lo).astype(np.float64)
    displaced = 20000 / column * float(size.prod())
    assert float(body.mass) == pytest.approx(6.0 * displaced, rel=1e-4) and float(body.mass) >= 4.0 * displaced
    with pytest.raises(ValueError):
        scenes.dam_break_debris(20000, density_ratio=2.0)
