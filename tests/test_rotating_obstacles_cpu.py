"""CPU checks of the oriented and rotating obstacles' contract (csrc/obstacle_policy.h, third part): the
struct layout, the refusals, obstacle_sincos, the frame changes and the angle, the per-particle response and
the load recorder of csrc/obstacle_policy.h / load_policy.h (compiled with g++ behind an extern "C" shim)
against the numpy restatement tests/rotating_obstacle_emulation.py bit for bit, the anchors to the static and
the moving response, the route decisions of csrc/launch_policy.h, and the Python side (obstacles.Rotation,
scenes.dam_break_ramp, scenes.stirred_tank)."""
import ctypes as C
import math

import numpy as np
import pytest

import load_emulation as L
import moving_obstacle_emulation as M
import obstacle_emulation as E
import rotating_obstacle_emulation as R
from helpers import compile_shim, to_oracle_params
from test_loads_cpu import same_bits as same_bits_nan
from test_obstacles_cpu import _extent, _obstacle_set, cases, same_bits

F32 = np.float32

SHIM = r"""
#include <stddef.h>
#include "load_policy.h"
#include "body_policy.h"
#include "launch_policy.h"

extern "C" {
const char* rot_check(const sph_hip_obstacle_rotation* list, int n, int n_obstacles)
{
   const char* why = obstacle_rotation_check(list, n, n_obstacles);
   return why ? why : "";
}
const char* rot_motion_check(const sph_hip_obstacle_rotation* rot, int n_rot, const sph_hip_obstacle_motion* motion,
                             int n_motion)
{
   const char* why = obstacle_rotation_motion_check(rot, n_rot, motion, n_motion);
   return why ? why : "";
}
const char* rot_body_check(const sph_hip_obstacle_rotation* rot, int n_rot, const sph_hip_body* bodies, int n_bodies)
{
   const char* why = body_rotation_check(rot, n_rot, bodies, n_bodies);
   return why ? why : "";
}
int count_posed(const sph_hip_obstacle_rotation* list, int n) { return obstacles_posed(list, n); }
int count_rotating(const sph_hip_obstacle_rotation* list, int n) { return obstacles_rotating(list, n); }
void sincos_many(const float* theta, long long n, float* cs, float* sn)
{
   for (long long i = 0; i < n; i++) obstacle_sincos(theta[i], cs[i], sn[i]);
}
float theta_of(const sph_hip_obstacle_rotation* r, float tau) { return obstacle_theta(*r, tau); }
// which: 0 to_body, 1 to_world, 2 vec_to_body, 3 vec_to_world
void frames(const sph_hip_obstacle_rotation* r, float cs, float sn, int which, int m, const float* x, float* y)
{
   for (int i = 0; i < m; i++) {
      if (which == 0) obstacle_to_body(*r, cs, sn, x + 3 * i, y + 3 * i);
      else if (which == 1) obstacle_to_world(*r, cs, sn, x + 3 * i, y + 3 * i);
      else if (which == 2) obstacle_vec_to_body(*r, cs, sn, x + 3 * i, y + 3 * i);
      else obstacle_vec_to_world(*r, cs, sn, x + 3 * i, y + 3 * i);
   }
}
void respond_static(const sph_hip_obstacle* list, int n, int m, const float* p, float* v, float* q, float dt,
                    float damping)
{
   for (int i = 0; i < m; i++) obstacles_respond(list, n, p + 3 * i, v + 3 * i, q + 3 * i, dt, damping);
}
void respond_moving(const sph_hip_obstacle* list, const sph_hip_obstacle_motion* motion, int n, int m, const float* p,
                    float* v, float* q, float dt, float damping, float tau0, float tau1)
{
   for (int i = 0; i < m; i++)
      obstacles_respond_moving(list, motion, n, p + 3 * i, v + 3 * i, q + 3 * i, dt, damping, tau0, tau1);
}
// the pose table as the device's first wave forms it, then every particle
void respond(const sph_hip_obstacle* list, const sph_hip_obstacle_motion* motion, const sph_hip_obstacle_rotation* rot,
             int n, int m, const float* p, float* v, float* q, float dt, float damping, float tau0, float tau1)
{
   ObstaclePose pose[SPH_HIP_MAX_OBSTACLES];
   for (int i = 0; i < n; i++) pose[i] = obstacle_pose_of_step(rot[i], tau0, tau1);
   for (int i = 0; i < m; i++)
      obstacles_respond_posed(list, motion, rot, pose, n, p + 3 * i, v + 3 * i, q + 3 * i, dt, damping, tau0, tau1);
}
void turn_with_pose(const sph_hip_obstacle* o, const sph_hip_obstacle_rotation* r, float cs0, float sn0, float cs1,
                    float sn1, int still, int m, const float* p, float* v, float* q, float dt, float damping,
                    unsigned char* in)
{
   const ObstaclePose ps = {cs0, sn0, cs1, sn1, 1, still};
   for (int i = 0; i < m; i++) in[i] = obstacle_turn_posed(*o, *r, ps, p + 3 * i, v + 3 * i, q + 3 * i, dt, damping);
}
void respond_loads(const float* maxv, int apply_walls, const sph_hip_obstacle* list,
                   const sph_hip_obstacle_motion* motion, const sph_hip_obstacle_rotation* rot, int n, int m,
                   const float* p, float* v, float* q, const float* mass, float dt, float damping, float tau0,
                   float tau1, int quantum_log2, long long* row)
{
   const LoadRowAdder rec = {row, load_scale(quantum_log2)};
   ObstaclePose pose[SPH_HIP_MAX_OBSTACLES];
   for (int i = 0; i < n; i++) pose[i] = obstacle_pose_of_step(rot[i], tau0, tau1);
   for (int i = 0; i < m; i++) {
      if (apply_walls) load_walls_respond(maxv, damping, p + 3 * i, v + 3 * i, dt, q + 3 * i, mass[i], rec);
      load_obstacles_respond_posed(list, motion, rot, pose, n, p + 3 * i, v + 3 * i, q + 3 * i, dt, damping, tau0,
                                   tau1, mass[i], rec);
   }
}
int posed_kernels(int n_obst, int n_posed) { return use_posed_kernels(n_obst, n_posed); }
int clock_runs(int n_obst, int n_moving, int n_rotating) { return motion_clock_runs(n_obst, n_moving, n_rotating); }
int moving_kernels(int n_obst, int n_moving) { return use_moving_kernels(n_obst, n_moving); }
int body_kernels(int n_obst, int n_bodies) { return use_body_kernels(n_obst, n_bodies); }
int fused_integrate6(int hash_too, int tiled, int n, int no_fused, int n_obst, int record)
{
   return fuse_integrate(hash_too != 0, tiled != 0, n, no_fused != 0, n_obst, record != 0);
}
int fused_slab3(int no_fused_slab, int n_obst, int record)
{
   return fuse_slab_step(no_fused_slab != 0, n_obst, record != 0);
}
#define OFF(f) (long long)offsetof(sph_hip_obstacle_rotation, f)
void layout(long long* out)
{
   out[0] = sizeof(sph_hip_obstacle_rotation);
   out[1] = OFF(axis); out[2] = OFF(pivot); out[3] = OFF(angle); out[4] = OFF(rate); out[5] = OFF(start);
   out[6] = OFF(stop);
   out[7] = SPH_HIP_ABI_VERSION; out[8] = sizeof(sph_hip_obstacle); out[9] = sizeof(ObstaclePose);
}
}
"""


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    from smoothed_particle_hydrodynamics_amd.obstacles import SphBody, SphObstacle, SphObstacleMotion, SphObstacleRotation
    lib = compile_shim(SHIM, ["-O2", "-ffp-contract=off"], tmp_path_factory)
    PO, PM, PR, V = C.POINTER(SphObstacle), C.POINTER(SphObstacleMotion), C.POINTER(SphObstacleRotation), C.c_void_p
    f = C.c_float
    lib.rot_check.argtypes = [PR, C.c_int, C.c_int]
    lib.rot_check.restype = C.c_char_p
    lib.rot_motion_check.argtypes = [PR, C.c_int, PM, C.c_int]
    lib.rot_motion_check.restype = C.c_char_p
    lib.rot_body_check.argtypes = [PR, C.c_int, C.POINTER(SphBody), C.c_int]
    lib.rot_body_check.restype = C.c_char_p
    lib.count_posed.argtypes = lib.count_rotating.argtypes = [PR, C.c_int]
    lib.sincos_many.argtypes = [V, C.c_longlong, V, V]
    lib.theta_of.argtypes = [PR, f]
    lib.theta_of.restype = f
    lib.frames.argtypes = [PR, f, f, C.c_int, C.c_int, V, V]
    lib.respond_static.argtypes = [PO, C.c_int, C.c_int, V, V, V, f, f]
    lib.respond_moving.argtypes = [PO, PM, C.c_int, C.c_int, V, V, V, f, f, f, f]
    lib.respond.argtypes = [PO, PM, PR, C.c_int, C.c_int, V, V, V, f, f, f, f]
    lib.turn_with_pose.argtypes = [PO, PR, f, f, f, f, C.c_int, C.c_int, V, V, V, f, f, V]
    lib.respond_loads.argtypes = [V, C.c_int, PO, PM, PR, C.c_int, C.c_int, V, V, V, V, f, f, f, f, C.c_int, V]
    lib.layout.argtypes = [C.POINTER(C.c_longlong)]
    return lib


def _arrays(P, V, Q):
    p = np.ascontiguousarray(P, F32).reshape(-1, 3)
    return p, np.ascontiguousarray(V, F32).reshape(-1, 3).copy(), np.ascontiguousarray(Q, F32).reshape(-1, 3).copy()


def _lists(obstacles, motions, rotations):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    arr, n = O.as_array(obstacles)
    mot = O.as_motion_array(motions)[0] if motions else None
    rot, _ = O.as_rotation_array(rotations)
    return arr, mot, rot, n


def header_sincos(lib, theta):
    t = np.ascontiguousarray(theta, F32).reshape(-1)
    cs, sn = np.zeros_like(t), np.zeros_like(t)
    lib.sincos_many(t.ctypes.data, t.size, cs.ctypes.data, sn.ctypes.data)
    return cs, sn


def header_static(lib, obstacles, P, V, Q, dt, damping):
    from smoothed_particle_hydrodynamics_amd.obstacles import as_array
    arr, n = as_array(obstacles)
    p, v, q = _arrays(P, V, Q)
    lib.respond_static(arr, n, p.shape[0], p.ctypes.data, v.ctypes.data, q.ctypes.data, dt, damping)
    return v, q


def header_respond(lib, obstacles, motions, rotations, P, V, Q, dt, damping, tau0, tau1):
    arr, mot, rot, n = _lists(obstacles, motions, rotations)
    p, v, q = _arrays(P, V, Q)
    lib.respond(arr, mot, rot, n, p.shape[0], p.ctypes.data, v.ctypes.data, q.ctypes.data, dt, damping, tau0, tau1)
    return v, q


def header_turn(lib, o, r, pose, still, P, V, Q, dt, damping):
    p, v, q = _arrays(P, V, Q)
    inside = np.zeros(p.shape[0], np.uint8)
    st = o if hasattr(o, "_fields_") else o.as_struct()
    lib.turn_with_pose(C.byref(st), C.byref(r.as_struct()), pose[0], pose[1], pose[2], pose[3], int(still), p.shape[0],
                       p.ctypes.data, v.ctypes.data, q.ctypes.data, dt, damping, inside.ctypes.data)
    return v, q, inside.astype(bool)


def header_loads(lib, maxv, apply_walls, obstacles, motions, rotations, P, V, Q, mass, dt, damping, tau0, tau1,
                 quantum_log2):
    arr, mot, rot, n = _lists(obstacles, motions, rotations)
    maxv = np.ascontiguousarray(maxv, F32)
    p, v, q = _arrays(P, V, Q)
    m = np.ascontiguousarray(mass, F32)
    row = np.zeros(5 * L.SOLIDS, np.int64)
    lib.respond_loads(maxv.ctypes.data, int(apply_walls), arr, mot, rot, n, p.shape[0], p.ctypes.data, v.ctypes.data,
                      q.ctypes.data, m.ctypes.data, dt, damping, tau0, tau1, int(quantum_log2), row.ctypes.data)
    S = L.SOLIDS
    return v, q, row[:3 * S].reshape(S, 3), row[3 * S:4 * S], row[4 * S:]


# ---- layout, constants, refusals ---------------------------------------------------------------

def test_struct_layout_and_constants(policy):
    from smoothed_particle_hydrodynamics_amd import lib as B
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    out = (C.c_longlong * 10)()
    policy.layout(out)
    S = O.SphObstacleRotation
    offsets = [S.axis.offset, S.pivot.offset, S.angle.offset, S.rate.offset, S.start.offset, S.stop.offset]
    assert list(out) == [32] + offsets + [7, 48, 24]
    assert C.sizeof(S) == 32 and offsets == [0, 4, 16, 20, 24, 28]
    assert C.sizeof(O.SphObstacle) == 48 and B.ABI_VERSION == 7
    # the contract only: no entry point takes a rotation list yet
    assert not [name for name in B.PROTOTYPES if "rotation" in name or "poses" in name]


def test_refusals(policy):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    ok = [O.Rotation(2, (1, 2, 3), 0.5), None, O.Rotation(0, (0, 0, 0), -1.0, 3.0, 0.25, 0.75),
          O.Rotation(1, (0, 1, 0), 0.0, -2.0, 1.0, 1.0)]
    arr, n = O.as_rotation_array(ok)
    assert policy.rot_check(arr, 4, 4) == b"" and policy.count_posed(arr, 4) == 3 and policy.count_rotating(arr, 4) == 2
    assert policy.rot_check(None, 0, 4) == b"" and policy.rot_check(None, 0, 0) == b""
    assert policy.rot_check(arr, 0, 4) == b""                         # n = 0 clears, whatever the list
    count = b"the rotation count must be 0 or the obstacle count"
    assert policy.rot_check(arr, 3, 4) == count and policy.rot_check(arr, 4, 3) == count
    assert policy.rot_check(arr, 4, 0) == count and policy.rot_check(arr, -1, 4) == count
    assert policy.rot_check(None, 4, 4) == b"null rotation list"

    def why(mutate):
        s = ok[2].as_struct()
        mutate(s)
        a, k = O.as_rotation_array([s])
        return policy.rot_check(a, k, 1)

    for bad in (-1, 3, 7):
        assert why(lambda s: setattr(s, "axis", bad)) == b"a rotation's axis must be 0, 1 or 2"
    for bad in (np.nan, np.inf, -np.inf):
        for c in range(3):
            assert why(lambda s: s.pivot.__setitem__(c, bad)) == b"a rotation's pivot must be finite"
        assert why(lambda s: setattr(s, "angle", bad)) == b"a rotation's angle and rate must be finite"
        assert why(lambda s: setattr(s, "rate", bad)) == b"a rotation's angle and rate must be finite"
        assert why(lambda s: setattr(s, "start", bad)) == b"a rotation's start must be finite and >= 0"
    assert why(lambda s: setattr(s, "start", -0.5)) == b"a rotation's start must be finite and >= 0"
    assert why(lambda s: setattr(s, "stop", 0.125)) == b"a rotation needs stop >= start"
    assert why(lambda s: setattr(s, "stop", np.nan)) == b"a rotation needs stop >= start"
    assert why(lambda s: setattr(s, "stop", -np.inf)) == b"a rotation needs stop >= start"
    within = b"a rotation's angle must stay within 8192 radians"
    assert why(lambda s: setattr(s, "angle", 8192.5)) == within
    assert why(lambda s: setattr(s, "angle", -8193.0)) == within
    assert why(lambda s: setattr(s, "angle", 8192.0)) == within + b" until its stop"     # 8192 + 3 * 0.5
    assert why(lambda s: (setattr(s, "angle", 8192.0), setattr(s, "rate", 0.0))) == b""
    assert why(lambda s: setattr(s, "rate", 16384.0)) == within + b" until its stop"     # 1 + 16384 * 0.5 = 8193
    assert why(lambda s: setattr(s, "rate", -16384.0)) == within + b" until its stop"
    assert why(lambda s: (setattr(s, "rate", 16382.0), setattr(s, "angle", -1.0))) == b""    # 1 + 8191 = 8192
    assert why(lambda s: (setattr(s, "rate", 1e30), setattr(s, "stop", np.inf))) == b""      # an open end is not summed
    assert why(lambda s: setattr(s, "stop", np.inf)) == b""
    assert why(lambda s: setattr(s, "stop", 0.25)) == b""             # stop == start
    assert why(lambda s: setattr(s, "start", -0.0)) == b""
    assert why(lambda s: setattr(s, "pivot", (C.c_float * 3)(-0.0, 1e30, -1e30))) == b""


def test_mirror_refusals_of_motion_and_bodies(policy):
    """a posed entry excludes a moving motion on its obstacle, and posed entries exclude bodies in one list:
    one function per pair, asked by both setters"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rot, _ = O.as_rotation_array([O.Rotation(2, (0, 0, 0), 0.5), None, O.Rotation(1, (0, 0, 0), 0.0, 2.0)])
    flat, _ = O.as_rotation_array([None, O.Rotation(0, (1, 1, 1)), O.Rotation(0, (1, 1, 1), -0.0, 0.0)])
    moves = b"a posed entry on an obstacle whose motion moves"
    mot, _ = O.as_motion_array([None, O.Motion((1, 0, 0)), O.Motion((0, 0, 0))])
    assert policy.rot_motion_check(rot, 3, mot, 3) == b""
    assert policy.rot_motion_check(rot, 3, None, 0) == b"" and policy.rot_motion_check(None, 0, mot, 3) == b""
    for i in (0, 2):
        m = [None, None, None]
        m[i] = O.Motion((0, 0, -1e-30))
        assert policy.rot_motion_check(rot, 3, O.as_motion_array(m)[0], 3) == moves
        assert policy.rot_motion_check(flat, 3, O.as_motion_array(m)[0], 3) == b""
    body = O.Body(5.0)
    for i in range(3):
        b = [None, None, None]
        b[i] = body
        got = policy.rot_body_check(rot, 3, O.as_body_array(b)[0], 3)
        assert got == (b"posed entries and bodies in one obstacle list" if i == 1
                       else b"a posed entry on an obstacle that is a body")
        assert policy.rot_body_check(flat, 3, O.as_body_array(b)[0], 3) == b""
    assert policy.rot_body_check(rot, 3, O.as_body_array([None] * 3)[0], 3) == b""
    assert policy.rot_body_check(rot, 3, None, 0) == b"" and policy.rot_body_check(None, 0, O.as_body_array([body])[0], 1) == b""


# ---- obstacle_sincos -------------------------------------------------------------------------------

SINCOS_BOUND = 2.0 ** -22      # |cs - cos|, |sn - sin| (the issue's bound: four ulp of 1.0)
UNIT_BOUND = 2.0 ** -21        # |cs^2 + sn^2 - 1|


def _sincos_checked(policy, theta):
    """header == restatement in bits; returns the three maxima against float64"""
    cs, sn = header_sincos(policy, theta)
    ecs, esn = R.sincos(theta)
    assert same_bits(cs, ecs) and same_bits(sn, esn)
    t = np.asarray(theta, F32).astype(np.float64)
    c, s = cs.astype(np.float64), sn.astype(np.float64)
    return float(np.abs(c - np.cos(t)).max()), float(np.abs(s - np.sin(t)).max()), float(np.abs(c * c + s * s - 1.0).max())


def test_sincos_on_seeded_angles(policy):
    rng = np.random.default_rng(5)
    theta = rng.uniform(-R.MAX_ANGLE, R.MAX_ANGLE, 4_000_000).astype(F32)
    theta[:1000] = rng.uniform(-4.0, 4.0, 1000).astype(F32)
    ec, es, eu = _sincos_checked(policy, theta)
    print("obstacle_sincos on 4M angles: max |cs - cos| = %.3g, |sn - sin| = %.3g, |cs^2 + sn^2 - 1| = %.3g" % (ec, es, eu))
    assert ec <= SINCOS_BOUND and es <= SINCOS_BOUND and eu <= UNIT_BOUND


def test_sincos_at_the_quadrant_boundaries(policy):
    """the float neighbours of every multiple of pi/2 (where the zero crossings are, and where the absolute
    error shows as a relative one) and of every odd multiple of pi/4 (where the quadrant changes) up to 8192"""
    k = np.arange(-2 * 5216, 2 * 5216 + 1, dtype=np.float64)
    centre = (k * (math.pi / 4.0)).astype(F32)
    centre = centre[np.abs(centre) <= R.MAX_ANGLE]
    theta = [centre]
    up, down = centre, centre
    for _ in range(3):
        up = np.nextafter(up, F32(np.inf))
        down = np.nextafter(down, F32(-np.inf))
        theta += [up, down]
    theta = np.concatenate(theta)
    theta = theta[np.abs(theta) <= R.MAX_ANGLE]
    ec, es, eu = _sincos_checked(policy, theta)
    print("obstacle_sincos at %d boundary angles: max |cs - cos| = %.3g, |sn - sin| = %.3g, |cs^2 + sn^2 - 1| = %.3g"
          % (theta.size, ec, es, eu))
    assert ec <= SINCOS_BOUND and es <= SINCOS_BOUND and eu <= UNIT_BOUND
    assert theta.size > 70000 and (np.abs(theta) == F32(R.MAX_ANGLE)).sum() == 0 and np.abs(theta).max() > 8191.0


def test_sincos_at_zero_and_denormals(policy):
    tiny = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, -1.1754942e-38, 1.17549435e-38, 1e-30,
                     -8192.0, 8192.0], F32)
    ec, es, eu = _sincos_checked(policy, tiny)
    assert ec <= SINCOS_BOUND and es <= SINCOS_BOUND and eu <= UNIT_BOUND
    cs, sn = header_sincos(policy, tiny[:9])
    assert (cs == 1.0).all() and same_bits(sn[2:], tiny[2:9]) and (sn[:2] == 0).all()


# ---- frame changes and the angle --------------------------------------------------------------------

def test_frames_match_the_restatement(policy):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(6)
    X = rng.uniform(-3.0, 3.0, (20000, 3)).astype(F32)
    for axis in range(3):
        r = O.Rotation(axis, rng.uniform(-1.0, 1.0, 3), 0.3)
        for t in (0.0, 0.3, -2.5, 100.0, 8000.0):
            cs, sn = R.sincos(F32(t))
            for which, fn in enumerate((R.to_body, R.to_world, R.vec_to_body, R.vec_to_world)):
                Y = np.zeros_like(X)
                policy.frames(C.byref(r.as_struct()), cs, sn, which, X.shape[0], X.ctypes.data, Y.ctypes.data)
                assert same_bits(Y, fn(r, cs, sn, X)), (axis, t, which)
                assert same_bits(Y[:, axis], X[:, axis])
            # there and back: to the rounding of the two products and the two sums
            back = R.to_world(r, cs, sn, R.to_body(r, cs, sn, X))
            assert np.abs(back.astype(np.float64) - X).max() < 64 * 2.0 ** -24
            # the float64 frames of obstacles.Rotation agree to fp32 rounding
            rr = O.Rotation(axis, r.pivot, t)
            assert np.abs(rr.to_body(X) - R.to_body(r, cs, sn, X)).max() < 64 * 2.0 ** -24
            assert np.abs(rr.to_world(X) - R.to_world(r, cs, sn, X)).max() < 64 * 2.0 ** -24
            assert np.abs(rr.to_world(rr.to_body(X)) - X).max() < 1e-12


def test_theta_matches_the_restatement(policy):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(7)
    rots = [O.Rotation(2, (0, 0, 0), 0.5, 3.0, 0.125, 0.7), O.Rotation(0, (0, 0, 0), -1.25, -40.0, 0.0, math.inf),
            O.Rotation(1, (0, 0, 0), 2.0, 7.0, 0.3, 0.3), O.Rotation(1, (0, 0, 0), 1.0, 0.0, 0.0, math.inf)]
    for r in rots:
        st = r.as_struct()
        taus = [0.0, float(r.start) * 0.5, float(r.start), float(np.nextafter(r.start, F32(9)))]
        taus += [float(r.stop), float(r.stop) + 1.0] if np.isfinite(r.stop) else [100.0, 1e30]
        taus += [float(r.start) + 0.25 * min(float(r.stop) - float(r.start), 4.0)] + list(rng.uniform(0.0, 1.0, 50))
        for tau in taus:
            tau = F32(tau)
            got = F32(policy.theta_of(C.byref(st), tau))
            assert same_bits(got, R.theta(r, tau)) and same_bits(got, r.angle_at(tau))
            if tau <= r.start:
                assert same_bits(got, F32(r.angle + F32(r.rate * F32(0))))                    # before the start
            if tau >= r.stop:
                assert same_bits(got, F32(r.angle + F32(r.rate * F32(r.stop - r.start))))     # at and after the stop
    inside = rots[0]
    assert same_bits(R.theta(inside, 0.5), F32(F32(0.5) + F32(F32(3.0) * F32(F32(0.5) - F32(0.125)))))
    assert same_bits(R.theta(rots[1], 2.0), F32(-81.25))                                      # stop = inf: it goes on


# ---- the response, header vs numpy ------------------------------------------------------------------

def _timings(rng, dt):
    """(rate != 0, start, stop, tau0, tau1): tilted at rest, turning inside the interval, straddling the start,
    straddling the stop, before the start, dt == 0 (tau1 == tau0)"""
    dt = F32(dt)
    t0 = F32(rng.uniform(0.05, 0.2))
    return [(False, 0.0, math.inf, t0, F32(t0 + dt)),
            (True, 0.0, math.inf, t0, F32(t0 + dt)),
            (True, float(t0 + dt * F32(0.3)), math.inf, t0, F32(t0 + dt)),
            (True, 0.0, float(t0 + dt * F32(0.6)), t0, F32(t0 + dt)),
            (True, float(t0 + F32(1.0)), math.inf, t0, F32(t0 + dt)),
            (True, 0.0, math.inf, t0, t0)]


def _rotation_for(o, rng, turning, start, stop):
    """a pivot within two extents of the solid, a tilt of up to a turn and a half, and - turning - an angle
    swept per step of 0.004 between 0.005 and 0.4 radians"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    lo, hi = _extent(o)
    pivot = (lo + hi) * F32(0.5) + rng.uniform(-2.0, 2.0, 3).astype(F32) * (hi - lo)
    angle = F32(rng.uniform(-9.0, 9.0))
    rate = F32(rng.choice([-1.0, 1.0]) * rng.choice([1.25, 12.0, 100.0])) if turning else F32(0.0)
    return O.Rotation(int(rng.integers(0, 3)), pivot, angle, rate, start, stop)


def posed_cases(o, r, tau0, tau1, m, dt, rng):
    """test_obstacles_cpu.cases around the solid in its own frame - faces, edges, corners, grazing lines, q on
    the surface, p inside - taken to the world: p with the pose at tau0, q and v with the pose at tau1; plus a
    tenth at rest that the turning solid sweeps over (q = p inside it at tau1)"""
    P, V, Q = cases(o, m, dt, rng)
    cs0, sn0 = R.sincos(R.theta(r, tau0))
    cs1, sn1 = R.sincos(R.theta(r, tau1))
    Pw = R.to_world(r, cs0, sn0, P)
    Qw = R.to_world(r, cs1, sn1, Q)
    Vw = R.vec_to_world(r, cs1, sn1, V)
    k = m // 10
    lo, hi = _extent(o)
    a = slice(6 * k, 7 * k)
    Pw[a] = R.to_world(r, cs1, sn1, (lo + rng.random((k, 3)) * (hi - lo)).astype(F32))
    Vw[a] = 0.0
    Qw[a] = Pw[a]
    return Pw, Vw, Qw


@pytest.mark.parametrize("kind", [E.SPHERE, E.BOX, E.CYLINDER], ids=["sphere", "box", "cylinder"])
def test_header_equals_numpy_bit_for_bit(policy, kind):
    rng = np.random.default_rng(5000 + kind)
    dt, damping = F32(0.004), F32(0.6)
    total = active = turned = 0
    for o in _obstacle_set(kind, rng):
        for turning, start, stop, tau0, tau1 in _timings(rng, dt):
            step = dt if tau1 != tau0 else F32(0.0)
            r = _rotation_for(o, rng, turning, start, stop)
            P, V, Q = posed_cases(o, r, tau0, tau1, 5000, dt, rng)
            hv, hq = header_respond(policy, [o], None, [r], P, V, Q, step, damping, tau0, tau1)
            ev, eq, act = R.respond_one(o, None, r, P, V, Q, step, damping, tau0, tau1)
            assert same_bits_nan(hv, ev) and same_bits_nan(hq, eq), (kind, turning, start, stop, tau0, tau1)
            assert same_bits_nan(hv[~act], V[~act]) and same_bits_nan(hq[~act], Q[~act])
            # the same with a motion list that does not move beside it
            mv, mq = header_respond(policy, [o], [None], [r], P, V, Q, step, damping, tau0, tau1)
            assert same_bits_nan(mv, hv) and same_bits_nan(mq, hq)
            total += P.shape[0]
            active += int(act.sum())
            turned += int(act.sum()) if R.turns(r, tau0, tau1) else 0
    assert total >= 120000
    assert active > 10000 and turned > 2000, (active, turned)


def test_mixed_lists_header_equals_numpy(policy):
    """a resting box with -0 fields, a piston and a paddle in one list, overlapping, applied in list order"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(79)
    neg = O.Box((-0.0, -1.0, -0.5), (1.2, 0.3, 0.5)).as_struct()
    neg.lo[0] = -0.0
    obst = [neg, O.Box((-0.9, -0.2, -0.2), (-0.1, 0.6, 0.7)), O.Box((-0.6, -0.2, -0.9), (0.6, 0.2, 0.9)),
            O.Cylinder(1, (0.4, 0.0, 0.3), 0.5, -0.8, 0.8)]
    motions = [None, O.Motion((30.0, 0.0, -12.0), 0.09, math.inf), None, None]
    rotations = [None, None, O.Rotation(2, (0.0, 0.0, 0.0), 0.4, 50.0), O.Rotation(0, (0.0, 0.2, 0.1), -0.7)]
    dt, damping = F32(0.004), F32(0.3)
    tau0 = F32(0.1)
    tau1 = F32(tau0 + dt)
    P, V, Q = cases(O.Box((-1.0, -1.0, -1.0), (1.2, 1.0, 1.0)), 100000, dt, rng)
    hv, hq = header_respond(policy, obst, motions, rotations, P, V, Q, dt, damping, tau0, tau1)
    ev, eq = R.respond(obst, motions, rotations, P, V, Q, dt, damping, tau0, tau1)
    assert same_bits_nan(hv, ev) and same_bits_nan(hq, eq)
    nv, nq = header_respond(policy, obst, None, rotations, P, V, Q, dt, damping, tau0, tau1)   # no motion list at all
    xv, xq = R.respond(obst, [], rotations, P, V, Q, dt, damping, tau0, tau1)
    assert same_bits_nan(nv, xv) and same_bits_nan(nq, xq) and not same_bits_nan(nq, hq)
    sv, sq = header_static(policy, obst, P, V, Q, dt, damping)
    assert not same_bits_nan(hq, sq)
    on_neg_face = (hq[:, 0] == 0) & np.signbit(hq[:, 0])
    assert on_neg_face.sum() > 10, "the resting box's -0 face must reach some q"
    for i in range(4):       # every entry acts
        one_r = [r if j == i else None for j, r in enumerate(rotations)]
        _, _, act = R.respond_one(obst[i], motions[i], one_r[i], P, V, Q, dt, damping, tau0, tau1)
        assert act.sum() > 1000


# ---- anchors ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [E.SPHERE, E.BOX, E.CYLINDER], ids=["sphere", "box", "cylinder"])
def test_an_unposed_entry_takes_the_turn_it_always_took(policy, kind):
    """rotations that are None, all zero, or -0 with a start and a stop: obstacles_respond without motions,
    obstacles_respond_moving with them, bit for bit"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(6000 + kind)
    dt, damping = F32(0.004), F32(0.6)
    obst = _obstacle_set(kind, rng)
    P, V, Q = cases(O.Box((-3.0, -3.0, -3.0), (3.0, 3.0, 3.0)), 40000, dt, rng)
    sv, sq = header_static(policy, obst, P, V, Q, dt, damping)
    assert not same_bits(sq, Q)
    tau0 = F32(0.5)
    tau1 = F32(tau0 + dt)
    motions = [O.Motion((30.0, 0.0, -12.0)), None, O.Motion((0.0, 25.0, 0.0), 0.101, 0.6), O.Motion((0, 0, 0))]
    arr, mot, _, n = _lists(obst, motions, [None] * 4)
    p, mv, mq = _arrays(P, V, Q)
    policy.respond_moving(arr, mot, n, p.shape[0], p.ctypes.data, mv.ctypes.data, mq.ctypes.data, dt, damping, tau0, tau1)
    assert not same_bits(mq, sq)
    for rotations in ([None] * 4, [O.Rotation(1, (1, 2, 3))] * 4, [O.Rotation(2, (0.5, 0.5, 0.5), -0.0, 0.0, 0.1, 0.2)] * 4,
                      [O.Rotation(0, (0, 0, 0), 0.0, -0.0)] * 4):
        hv, hq = header_respond(policy, obst, None, rotations, P, V, Q, dt, damping, tau0, tau1)
        assert same_bits(hv, sv) and same_bits(hq, sq)
        ev, eq = R.respond(obst, [], rotations, P, V, Q, dt, damping, tau0, tau1)
        assert same_bits(ev, sv) and same_bits(eq, sq)
        hv, hq = header_respond(policy, obst, motions, rotations, P, V, Q, dt, damping, tau0, tau1)
        assert same_bits(hv, mv) and same_bits(hq, mq)
        ev, eq = R.respond(obst, motions, rotations, P, V, Q, dt, damping, tau0, tau1)
        assert same_bits(ev, mv) and same_bits(eq, mq)


def _quarter_turned(o, axis, cs, sn):
    """the static obstacle that holds x exactly when o holds to_body(cs, sn, x) about the origin, for
    (cs, sn) a quarter turn: a box with u and w exchanged and negated accordingly; a cylinder along `axis`
    about the origin itself"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    u, w = (axis + 1) % 3, (axis + 2) % 3
    # body_u = cs * x_u + sn * x_w, body_w = cs * x_w - sn * x_u: (world axis, sign) per body axis
    src = {u: (u, cs) if cs else (w, sn), w: (w, cs) if cs else (u, -sn), axis: (axis, 1)}
    if o.kind == E.CYLINDER:
        if o.axis == axis:
            return o
        # a cylinder along u or w about the origin: along the world axis its own is taken to, its caps with it
        c, s = src[o.axis]
        lo, hi = (float(o.lo), float(o.hi)) if s > 0 else (-float(o.hi), -float(o.lo))
        return O.Cylinder(c, (0.0, 0.0, 0.0), o.radius, lo, hi)
    lo, hi = np.zeros(3, F32), np.zeros(3, F32)
    for b, (c, s) in src.items():
        lo[c], hi[c] = (o.lo[b], o.hi[b]) if s > 0 else (-o.hi[b], -o.lo[b])
    return O.Box(lo, hi)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_quarter_turns_are_the_static_response_with_axes_exchanged(policy, axis):
    """(cs, sn) given as (0, 1), (-1, 0) and (0, -1) about the origin: every product is exact, so the posed
    turn is the static response of the box with u and w exchanged, of the cylinder along the axis itself, and
    of a cylinder along u or w taken to the other of the two (their sums of two squares commute) - compared
    with ==, on seeded lines without ties between axes"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(60 + axis)
    dt, damping = F32(0.004), F32(0.6)
    u, w = (axis + 1) % 3, (axis + 2) % 3
    lo, hi = np.zeros(3, F32), np.zeros(3, F32)
    lo[[axis, u, w]] = [-0.4, 0.3, -0.2]
    hi[[axis, u, w]] = [0.5, 1.1, 0.45]
    centre = np.zeros(3, F32)
    solids = [O.Box(lo, hi), O.Cylinder(axis, centre, 0.7, -0.4, 0.5), O.Cylinder(u, centre, 0.6, 0.2, 0.9),
              O.Cylinder(w, centre, 0.5, -0.7, -0.1)]
    r = O.Rotation(axis, (0.0, 0.0, 0.0), 1.0)
    m = 30000
    for o in solids:
        for cs, sn in ((0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)):
            twin = _quarter_turned(o, axis, cs, sn)
            tlo, thi = _extent(twin)
            ext = thi - tlo
            P = (tlo - ext + rng.random((m, 3)) * 3 * ext).astype(F32)
            V = (rng.normal(0.0, 1.0, (m, 3)) * 300.0).astype(F32)
            Q = (P + V * (F32(dt) * rng.choice([0.3, 1.0, 2.0], m).astype(F32))[:, None]).astype(F32)
            Q[:m // 4] = (tlo + rng.random((m // 4, 3)) * ext).astype(F32)
            hv, hq, act = header_turn(policy, o, r, (cs, sn, cs, sn), True, P, V, Q, dt, damping)
            sv, sq = header_static(policy, [twin], P, V, Q, dt, damping)
            assert act.sum() > 3000 and np.array_equal(act, E.inside(twin, Q))
            assert not np.isnan(hv).any() and not np.isnan(hq).any()
            assert np.array_equal(hv, sv) and np.array_equal(hq, sq), (o, cs, sn)
            ev, eq, eact = R.respond_posed(o, r, cs, sn, cs, sn, True, P, V, Q, dt, damping)
            assert same_bits(hv, ev) and same_bits(hq, eq) and np.array_equal(act, eact)


def test_paddle_leaves_fluid_at_rest_at_twice_its_speed(policy):
    """A blade along +x turning about z through the origin: its face y = 0 at distance r from the pivot moves
    along its normal at omega * r, and particles at rest that it sweeps over leave at 2 * omega * r along that
    normal, with nothing along the face.  All inputs are dyadic (angle 0, rate 4, dt = 2^-8, tau0 = 8 dt, so
    theta0 = 2^-3 and theta1 = 9 * 2^-6 exactly).  The contract's formulas formed in float64 with the true
    cosines and sines give 4 |p| sin(dtheta / 2) cos(phi + dtheta / 2 - theta1) / dt along the normal - 2 omega r
    to second order in dtheta - and 0 along the face; the fp32 result may differ from that by its own rounding: obstacle_sincos (2^-22
    on each of four values that multiply lengths up to 2 |p| and speeds up to 2 omega r) and the difference
    pc - p of two positions rounded to 2^-24 |p| each, divided by dt."""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(33)
    dt, damping = F32(2.0 ** -8), F32(0.5)
    omega = 4.0
    blade = O.Box((0.5, -0.125, -1.0), (1.5, 0.0, 1.0))
    r = O.Rotation(2, (0.0, 0.0, 0.0), 0.0, omega)
    tau0 = F32(8 * dt)
    tau1 = F32(tau0 + dt)
    th0, th1 = float(R.theta(r, tau0)), float(R.theta(r, tau1))
    assert (th0, th1) == (2.0 ** -3, 9 * 2.0 ** -6)
    m = 6000
    rad = rng.uniform(0.6, 1.4, m)
    phi = th0 + rng.uniform(0.05, 0.95, m) * (th1 - th0)
    P = np.stack([rad * np.cos(phi), rad * np.sin(phi), rng.uniform(-0.9, 0.9, m)], 1).astype(F32)
    V = np.zeros_like(P)
    hv, hq = header_respond(policy, [blade], None, [r], P, V, P, dt, damping, tau0, tau1)
    ev, eq, act = R.respond_one(blade, None, r, P, V, P, dt, damping, tau0, tau1)
    assert same_bits(hv, ev) and same_bits(hq, eq) and act.all()
    normal = np.array([-math.sin(th1), math.cos(th1), 0.0])
    along = np.array([math.cos(th1), math.sin(th1), 0.0])
    # ue = (R(dtheta) p - p) / dt is the chord of the particle's own circle: 2 |p| sin(dtheta / 2) / dt long, at
    # right angles to the bisector at phi + dtheta / 2; the reflection doubles its part along the normal
    x = P.astype(np.float64)
    dist = np.hypot(x[:, 0], x[:, 1])
    at = np.arctan2(x[:, 1], x[:, 0])
    dth = th1 - th0
    want_n = 4.0 * dist * math.sin(dth / 2) * np.cos(at + dth / 2 - th1) / float(dt)
    arm = dist * np.cos(at - th1)                                    # r: the distance from the pivot along the face
    assert np.allclose(want_n, 2.0 * omega * arm, rtol=dth ** 2, atol=0)   # 2 omega r to second order in dtheta
    bound = 8 * 2.0 ** -22 * (2.0 * omega * dist) + 6 * 2.0 ** -24 * dist / float(dt)
    got = hv.astype(np.float64)
    assert (np.abs(got @ normal - want_n) <= bound).all(), np.abs(got @ normal - want_n).max()
    assert (np.abs(got @ along) <= bound).all() and not got[:, 2].any()
    assert (got @ normal > 1.9 * omega * 0.55).all()
    # left on or ahead of the face as it stands at tau1, z untouched
    body_y = (-math.sin(th1)) * hq[:, 0].astype(np.float64) + math.cos(th1) * hq[:, 1].astype(np.float64)
    assert (body_y > -2.0 ** -20).all() and same_bits(hq[:, 2], P[:, 2])
    # tilted at rest at theta1, the same blade never sets the fluid in motion
    sv, _ = header_respond(policy, [blade], None, [O.Rotation(2, (0, 0, 0), th1)], P, V, P, dt, damping, tau0, tau1)
    assert not sv.any()


# ---- loads --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [E.SPHERE, E.BOX, E.CYLINDER], ids=["sphere", "box", "cylinder"])
def test_posed_recorder_equals_numpy(policy, kind):
    rng = np.random.default_rng(7000 + kind)
    dt, damping = F32(0.004), F32(0.6)
    maxv = F32([2.5, 2.5, 2.5])
    total = responses = 0
    for o in _obstacle_set(kind, rng):
        for turning, start, stop, tau0, tau1 in _timings(rng, dt):
            step = dt if tau1 != tau0 else F32(0.0)
            r = _rotation_for(o, rng, turning, start, stop)
            P, V, Q = posed_cases(o, r, tau0, tau1, 5000, dt, rng)
            mass = rng.uniform(0.5, 2.0, P.shape[0]).astype(F32)
            for walls in (False, True):
                hv, hq, imp, cnt, skp = header_loads(policy, maxv, walls, [o], None, [r], P, V, Q, mass, step, damping,
                                                     tau0, tau1, L.QUANTUM_LOG2)
                ev, eq, row = R.integrate_respond(maxv, walls, [o], [], [r], P, V, Q, step, damping, tau0, tau1, mass)
                assert same_bits_nan(hv, ev) and same_bits_nan(hq, eq)
                assert row.same(imp, cnt, skp), (kind, turning, start, stop, walls)
                if not walls:
                    total += P.shape[0]
                    responses += int(cnt[6] + skp[6])
                    _, _, act = R.respond_one(o, None, r, P, V, Q, step, damping, tau0, tau1)
                    assert cnt[6] + skp[6] == act.sum() and not imp[:6].any() and not imp[7:].any()
    assert total >= 120000 and responses > 10000


# ---- routes ---------------------------------------------------------------------------------------------

def test_routes(policy):
    for n_obst in (0, 1, 3, 64):
        for k in (0, 1, 3, 64):
            assert bool(policy.posed_kernels(n_obst, k)) == (n_obst > 0 and k > 0)
            # the unchanged decisions
            assert bool(policy.moving_kernels(n_obst, k)) == (n_obst > 0 and k > 0)
            assert bool(policy.body_kernels(n_obst, k)) == (n_obst > 0 and k > 0)
            for j in (0, 1, 64):
                assert bool(policy.clock_runs(n_obst, k, j)) == (n_obst > 0 and (k > 0 or j > 0))
                # without a rotating entry the clock runs exactly when the moving kernels are taken
                assert bool(policy.clock_runs(n_obst, k, 0)) == bool(policy.moving_kernels(n_obst, k))
    for hash_too in (0, 1):
        for tiled in (0, 1):
            for n in (0, 5):
                for no_fused in (0, 1):
                    for n_obst in (0, 1, 64):
                        base = bool(hash_too and tiled and n > 0 and not no_fused and n_obst == 0)
                        assert bool(policy.fused_integrate6(hash_too, tiled, n, no_fused, n_obst, 0)) == base
                        assert not policy.fused_integrate6(hash_too, tiled, n, no_fused, n_obst, 1)
    for no_fused_slab in (0, 1):
        for n_obst in (0, 1, 64):
            assert bool(policy.fused_slab3(no_fused_slab, n_obst, 0)) == (not no_fused_slab and n_obst == 0)
            assert not policy.fused_slab3(no_fused_slab, n_obst, 1)


# ---- Python side ----------------------------------------------------------------------------------------

def test_rotation_round_trips():
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    r = O.Rotation(1, (0.25, -3.0, 1e-3), 0.5, -2.0, 0.125, 2.5)
    st = r.as_struct()
    assert [st.axis, st.pivot[0], st.pivot[1], st.angle, st.rate, st.start, st.stop] == [1, 0.25, -3.0, 0.5, -2.0, 0.125, 2.5]
    assert O.rotation_from_struct(st) == r and r.posed() and r.rotates()
    d = O.Rotation(2, (0, 0, 0), 0.3)
    assert d.rate == 0 and d.start == 0.0 and d.stop == math.inf and d.posed() and not d.rotates()
    assert same_bits(d.angle_at(5.0), F32(0.3)) and same_bits(r.angle_at(1.0), R.theta(st, 1.0))
    arr, n = O.as_rotation_array([r, None, st])
    assert n == 3 and bytes(arr[0]) == bytes(st) == bytes(arr[2])
    flat = O.rotation_from_struct(arr[1])
    assert not flat.posed() and not flat.rotates() and flat == O.Rotation(0, (0, 0, 0)) and flat.stop == math.inf
    assert O.as_rotation_array([])[1] == 0
    assert "Rotation" in repr(r) and r != d
    with pytest.raises(ValueError):
        O.Rotation(3, (0, 0, 0))


def test_carve_and_inside_any_with_rotations():
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    from smoothed_particle_hydrodynamics_amd import scenes
    rng = np.random.default_rng(8)
    pts = rng.uniform(-1.0, 1.0, (20000, 3))
    box = O.Box((-0.8, -0.1, -0.5), (0.8, 0.1, 0.5))
    quarter = O.Rotation(2, (0.0, 0.0, 0.0), math.pi / 2)
    plain = O.inside_any(pts, [box])
    assert np.array_equal(plain, O.inside_any(pts, [box], None)) and np.array_equal(plain, O.inside_any(pts, [box], [None]))
    assert np.array_equal(plain, O.inside_any(pts, [box], [O.Rotation(2, (0.3, 0.3, 0.3))]))
    with pytest.raises(ValueError):
        O.inside_any(pts, [box], [quarter, None])
    turned = O.inside_any(pts, [box], [quarter])
    upright = O.Box((-0.1, -0.8, -0.5), (0.1, 0.8, 0.5))
    edge = np.abs(upright.signed_distance(pts)) < 1e-9
    assert np.array_equal(turned[~edge], O.inside_any(pts, [upright])[~edge]) and turned.sum() > 500
    assert not np.array_equal(turned, plain)
    pos = pts.astype(F32).reshape(-1)
    vel = np.zeros_like(pos)
    mass = np.ones(pts.shape[0], F32)
    a = scenes.carve(pos, vel, mass, [box])
    b = scenes.carve(pos, vel, mass, [box], None)
    assert all(same_bits(x, y) for x, y in zip(a, b)) and a[2].size == (~O.inside_any(pts.astype(F32), [box])).sum()
    c = scenes.carve(pos, vel, mass, [box], [quarter])
    assert c[2].size == (~O.inside_any(pts.astype(F32), [box], [quarter])).sum() and not same_bits(c[0][:300], a[0][:300])


def _stepped_on_the_cpu(oracle, p, pos, vel, mass, obst, rotations, steps):
    """`steps` steps of the oracle, each followed by the restated response: the final (pos, vel), how many
    particle-steps a posed solid changed, and the clock"""
    op = to_oracle_params(p)
    dt, damping = F32(p.time_step), F32(p.damping)
    pos, vel = pos.copy(), vel.copy()
    tau = F32(0.0)
    runs = R.clock_runs([], rotations)
    changed = 0
    for _ in range(steps):
        P = pos.copy()
        oracle.step(op, pos, vel, mass, "full")
        tau1 = F32(tau + dt) if runs else tau
        V, Q = R.respond(obst, [], rotations, P, vel, pos, dt, damping, tau, tau1)
        changed += int(((V.reshape(-1) != vel) | (Q.reshape(-1) != pos)).reshape(-1, 3).any(1).sum())
        pos, vel, tau = np.ascontiguousarray(Q.reshape(-1)), np.ascontiguousarray(V.reshape(-1)), tau1
    return pos, vel, changed, tau


def test_ramp_scene(oracle):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass, obst, rotations = scenes.dam_break_ramp(20000)
    ramp, tilt = obst[0], rotations[0]
    assert len(obst) == len(rotations) == 1 and pos.size == 3 * mass.size == vel.size
    assert p.apply_gravity == 1 and p.apply_walls == 1 and p.gravity[1] < 0
    assert tilt.axis == 2 and tilt.posed() and not tilt.rotates()
    assert float(tilt.angle) == pytest.approx(math.radians(20.0), rel=1e-6)
    x = pos.reshape(-1, 3)
    assert not O.inside_any(x, obst, rotations).any()
    # the upper face rises downstream: its far edge stands above the floor, its near edge on it
    far = tilt.to_world([[float(ramp.hi[0]), 0.0, 0.5]])[0]
    near = tilt.to_world([[float(ramp.lo[0]), 0.0, 0.5]])[0]
    assert far[1] == pytest.approx((float(ramp.hi[0]) - float(ramp.lo[0])) * math.sin(math.radians(20.0)), rel=1e-5)
    assert near[1] == pytest.approx(0.0, abs=1e-7) and near[0] - x[:, 0].max() == pytest.approx(0.25 * float(p.h), rel=0.05)
    steep = scenes.dam_break_ramp(20000, slope_deg=35.0)[5][0]
    assert float(steep.angle) == pytest.approx(math.radians(35.0), rel=1e-6)
    # stepped as built: the surge (0.7 per unit time) crosses the quarter kernel radius to the ramp's foot in 11 steps
    assert 0.25 * float(p.h) / (0.7 * float(p.time_step)) < 12
    fpos, fvel, changed, tau = _stepped_on_the_cpu(oracle, p, pos, vel, mass, obst, rotations, 20)
    assert np.isfinite(fpos).all() and np.isfinite(fvel).all()
    assert changed > 0 and tau == 0.0, "a tilted solid answers, and leaves the clock standing"


def test_stirred_tank_scene(oracle):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass, obst, rotations = scenes.stirred_tank(20000, 40.0)
    paddle, turn = obst[0], rotations[0]
    assert len(obst) == len(rotations) == 1 and pos.size == 3 * mass.size == vel.size and not vel.any()
    assert p.apply_gravity == 1 and p.apply_walls == 1 and p.gravity[1] < 0
    assert turn.axis == 1 and turn.rotates() and turn.rate == F32(40.0) and turn.angle == 0
    assert float(turn.pivot[0]) == pytest.approx(0.5 * float(p.max_x)) and float(turn.pivot[2]) == pytest.approx(0.5 * float(p.max_z))
    x = pos.reshape(-1, 3)
    assert not O.inside_any(x, obst).any() and float(paddle.hi[1]) > x[:, 1].max() and float(paddle.lo[1]) < 0
    other = scenes.stirred_tank(20000, -40.0, stop=0.5)[5][0]
    assert other.rate == F32(-40.0) and other.stop == F32(0.5)
    fpos, fvel, changed, tau = _stepped_on_the_cpu(oracle, p, pos, vel, mass, obst, rotations, 20)
    assert np.isfinite(fpos).all() and np.isfinite(fvel).all()
    assert changed > 0 and same_bits(tau, M.clock(p.time_step, 20)[-1])
