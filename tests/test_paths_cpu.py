"""CPU checks of the motion paths (include/sph_hip.h: sph_hip_set_obstacle_paths): the struct layout, every
refusal and both pair checks, path_displacement, k_paths_eval's lane loop, the per-particle turn and the load
recorder of csrc/obstacle_policy.h / load_policy.h (compiled with g++ behind an extern "C" shim) against the
numpy restatement tests/path_emulation.py bit for bit, the anchors to the moving obstacles, the route
decisions of csrc/launch_policy.h, the Python side (obstacles.MotionPath, scenes.wave_flume), and the new
header code once under the sanitizers in a program of its own."""
import ctypes as C
import math
import shutil
import subprocess

import numpy as np
import pytest

import load_emulation as L
import moving_obstacle_emulation as M
import obstacle_emulation as E
import path_emulation as PE
import wedge_emulation as W
from helpers import CSRC, compile_shim
from test_obstacles_cpu import _obstacle_set, cases, same_bits
from test_wedges_cpu import wedge_set

F32 = np.float32

CALLS = r"""
#include <stddef.h>
#include <string.h>
#include "body_policy.h"
#include "launch_policy.h"

extern "C" {
const char* check(const sph_hip_motion_path* paths, int n, const sph_hip_motion_key* keys, int n_keys, int n_obstacles)
{
   const char* why = path_check(paths, n, keys, n_keys, n_obstacles);
   return why ? why : "";
}
const char* check_motion(const sph_hip_motion_path* paths, int n_paths, const sph_hip_obstacle_motion* motion, int n_motion)
{
   const char* why = path_motion_check(paths, n_paths, motion, n_motion);
   return why ? why : "";
}
const char* check_body(const sph_hip_motion_path* paths, int n_paths, const sph_hip_body* bodies, int n_bodies)
{
   const char* why = path_body_check(paths, n_paths, bodies, n_bodies);
   return why ? why : "";
}
int count_paths(const sph_hip_motion_path* paths, int n) { return paths_count(paths, n); }
void displacements(const sph_hip_motion_path* P, const sph_hip_motion_key* keys, const float* tau, int m, float* D)
{
   for (int i = 0; i < m; i++) path_displacement(*P, keys, tau[i], D + 3 * i);
}
void velocities(const sph_hip_motion_path* P, const sph_hip_motion_key* keys, const float* tau, int m, float* v)
{
   for (int i = 0; i < m; i++) path_velocity(*P, keys, tau[i], v + 3 * i);
}
void eval(const sph_hip_motion_path* paths, const sph_hip_motion_key* keys, int n, float tau0, float tau1, PathShift* out)
{
   paths_eval(paths, keys, n, tau0, tau1, out);
}
void at(const sph_hip_obstacle* o, const sph_hip_motion_path* P, const sph_hip_motion_key* keys,
        const sph_hip_obstacle_motion* m, float tau, sph_hip_obstacle* out)
{
   *out = path_obstacle_at(*o, P, keys, m, tau);
}
void respond(const sph_hip_obstacle* list, const sph_hip_obstacle_motion* motion, const sph_hip_motion_path* paths,
             const sph_hip_motion_key* keys, int n, int m, const float* p, float* v, float* q, float dt, float damping,
             float tau0, float tau1)
{
   PathShift shift[SPH_HIP_MAX_OBSTACLES];
   paths_eval(paths, keys, n, tau0, tau1, shift);
   for (int i = 0; i < m; i++)
      obstacles_respond_path(list, motion, shift, n, p + 3 * i, v + 3 * i, q + 3 * i, dt, damping, tau0, tau1);
}
void respond_moving(const sph_hip_obstacle* list, const sph_hip_obstacle_motion* motion, int n, int m, const float* p,
                    float* v, float* q, float dt, float damping, float tau0, float tau1)
{
   for (int i = 0; i < m; i++)
      obstacles_respond_moving(list, motion, n, p + 3 * i, v + 3 * i, q + 3 * i, dt, damping, tau0, tau1);
}
void respond_loads(const float* maxv, int apply_walls, const sph_hip_obstacle* list, const sph_hip_obstacle_motion* motion,
                   const sph_hip_motion_path* paths, const sph_hip_motion_key* keys, int n, int m, const float* p,
                   float* v, float* q, const float* mass, float dt, float damping, float tau0, float tau1,
                   int quantum_log2, long long* row)
{
   const LoadRowAdder rec = {row, load_scale(quantum_log2)};
   PathShift shift[SPH_HIP_MAX_OBSTACLES];
   if (paths) paths_eval(paths, keys, n, tau0, tau1, shift);
   for (int i = 0; i < m; i++) {
      if (apply_walls) load_walls_respond(maxv, damping, p + 3 * i, v + 3 * i, dt, q + 3 * i, mass[i], rec);
      if (paths)
         load_obstacles_respond_path(list, motion, shift, n, p + 3 * i, v + 3 * i, q + 3 * i, dt, damping, tau0, tau1,
                                     mass[i], rec);
      else
         load_obstacles_respond_moving(list, motion, n, p + 3 * i, v + 3 * i, q + 3 * i, dt, damping, tau0, tau1,
                                       mass[i], rec);
   }
}
}
"""

SHIM = CALLS + r"""
extern "C" {
int path_kernels(int n_obst, int n_paths) { return use_path_kernels(n_obst, n_paths); }
int path_clock(int n_obst, int n_moving, int n_paths) { return path_clock_runs(n_obst, n_moving, n_paths); }
int moving_kernels(int n_obst, int n_moving) { return use_moving_kernels(n_obst, n_moving); }
int body_kernels(int n_obst, int n_bodies) { return use_body_kernels(n_obst, n_bodies); }
int old_clock(int n_obst, int n_moving, int n_rotating) { return motion_clock_runs(n_obst, n_moving, n_rotating); }
int fused_integrate(int hash_too, int tiled, int n, int no_fused, int n_obst, int record)
{
   return fuse_integrate(hash_too != 0, tiled != 0, n, no_fused != 0, n_obst, record != 0);
}
void layout(long long* out)
{
   out[0] = sizeof(sph_hip_motion_key); out[1] = offsetof(sph_hip_motion_key, t); out[2] = offsetof(sph_hip_motion_key, d);
   out[3] = sizeof(sph_hip_motion_path); out[4] = offsetof(sph_hip_motion_path, first);
   out[5] = offsetof(sph_hip_motion_path, count); out[6] = offsetof(sph_hip_motion_path, start);
   out[7] = offsetof(sph_hip_motion_path, cycle); out[8] = SPH_HIP_ABI_VERSION; out[9] = sizeof(sph_hip_obstacle);
   out[10] = SPH_HIP_MAX_PATH_KEYS; out[11] = sizeof(PathShift); out[12] = offsetof(PathShift, D1);
   out[13] = offsetof(PathShift, has_path); out[14] = SPH_HIP_MAX_OBSTACLES;
}
}
"""


class Shift(C.Structure):
    """mirror of PathShift (csrc/obstacle_policy.h): 32 bytes"""
    _fields_ = [("D0", C.c_float * 3), ("D1", C.c_float * 3), ("has_path", C.c_int32), ("pad", C.c_int32)]


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    lib = compile_shim(SHIM, ["-O2", "-ffp-contract=off"], tmp_path_factory)
    PO, PM, PP, PK, PB, V = (C.POINTER(O.SphObstacle), C.POINTER(O.SphObstacleMotion), C.POINTER(O.SphMotionPath),
                             C.POINTER(O.SphMotionKey), C.POINTER(O.SphBody), C.c_void_p)
    lib.check.argtypes = [PP, C.c_int, PK, C.c_int, C.c_int]
    lib.check_motion.argtypes = [PP, C.c_int, PM, C.c_int]
    lib.check_body.argtypes = [PP, C.c_int, PB, C.c_int]
    for f in (lib.check, lib.check_motion, lib.check_body):
        f.restype = C.c_char_p
    lib.count_paths.argtypes = [PP, C.c_int]
    lib.displacements.argtypes = [PP, PK, V, C.c_int, V]
    lib.velocities.argtypes = [PP, PK, V, C.c_int, V]
    lib.eval.argtypes = [PP, PK, C.c_int, C.c_float, C.c_float, C.POINTER(Shift)]
    lib.at.argtypes = [PO, PP, PK, PM, C.c_float, PO]
    lib.respond.argtypes = [PO, PM, PP, PK, C.c_int, C.c_int, V, V, V] + [C.c_float] * 4
    lib.respond_moving.argtypes = [PO, PM, C.c_int, C.c_int, V, V, V] + [C.c_float] * 4
    lib.respond_loads.argtypes = [V, C.c_int, PO, PM, PP, PK, C.c_int, C.c_int, V, V, V, V] + [C.c_float] * 4 + [C.c_int, V]
    lib.layout.argtypes = [C.POINTER(C.c_longlong)]
    return lib


def _arrays(P, V, Q):
    p = np.ascontiguousarray(P, F32).reshape(-1, 3)
    return p, np.ascontiguousarray(V, F32).reshape(-1, 3).copy(), np.ascontiguousarray(Q, F32).reshape(-1, 3).copy()


def _lists(obstacles, paths, motions):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    arr, n = O.as_array(obstacles)
    mot = O.as_motion_array(motions)[0] if motions else None
    pa, _, ka, _ = O.as_path_arrays(paths) if paths else (None, 0, None, 0)
    return arr, n, mot, pa, ka


def header_respond(lib, obstacles, paths, motions, P, V, Q, dt, damping, tau0, tau1):
    arr, n, mot, pa, ka = _lists(obstacles, paths, motions)
    p, v, q = _arrays(P, V, Q)
    lib.respond(arr, mot, pa, ka, n, p.shape[0], p.ctypes.data, v.ctypes.data, q.ctypes.data, dt, damping, tau0, tau1)
    return v, q


def header_moving(lib, obstacles, motions, P, V, Q, dt, damping, tau0, tau1):
    arr, n, mot, _, _ = _lists(obstacles, None, motions)
    p, v, q = _arrays(P, V, Q)
    lib.respond_moving(arr, mot, n, p.shape[0], p.ctypes.data, v.ctypes.data, q.ctypes.data, dt, damping, tau0, tau1)
    return v, q


def header_loads(lib, maxv, apply_walls, obstacles, paths, motions, P, V, Q, mass, dt, damping, tau0, tau1,
                 quantum_log2=L.QUANTUM_LOG2):
    arr, n, mot, pa, ka = _lists(obstacles, paths, motions)
    maxv = np.ascontiguousarray(maxv, F32)
    p, v, q = _arrays(P, V, Q)
    m = np.ascontiguousarray(mass, F32)
    row = np.zeros(5 * L.SOLIDS, np.int64)
    lib.respond_loads(maxv.ctypes.data, int(apply_walls), arr, mot, pa, ka, n, p.shape[0], p.ctypes.data,
                      v.ctypes.data, q.ctypes.data, m.ctypes.data, dt, damping, tau0, tau1, int(quantum_log2),
                      row.ctypes.data)
    S = L.SOLIDS
    return v, q, row[:3 * S].reshape(S, 3), row[3 * S:4 * S], row[4 * S:]


def header_displacements(lib, path, taus, first=0, n_keys_total=None, velocity=False):
    """path_displacement (or path_velocity) at every tau, the path's keys placed at `first` of a longer list"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    k = path.times.size
    total = n_keys_total or first + k
    keys = np.full((total, 4), np.nan, F32)
    keys[first:first + k, 0] = path.times
    keys[first:first + k, 1:] = path.displacements
    karr = (O.SphMotionKey * total).from_buffer_copy(keys.tobytes())
    s = O.SphMotionPath(first, k, float(path.start), int(path.cycle))
    taus = np.ascontiguousarray(taus, F32)
    out = np.zeros((taus.size, 3), F32)
    (lib.velocities if velocity else lib.displacements)(C.byref(s), karr, taus.ctypes.data, taus.size, out.ctypes.data)
    return out


# ---- layout, constants, refusals ---------------------------------------------------------------

def test_struct_layout_and_constants(policy):
    from smoothed_particle_hydrodynamics_amd import lib as B
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    out = (C.c_longlong * 15)()
    policy.layout(out)
    K, P = O.SphMotionKey, O.SphMotionPath
    assert list(out) == [16, 0, 4, 16, 0, 4, 8, 12, 7, 48, 16384, 32, 12, 24, 64]
    assert C.sizeof(K) == 16 and [K.t.offset, K.d.offset] == [0, 4]
    assert C.sizeof(P) == 16 and [P.first.offset, P.count.offset, P.start.offset, P.cycle.offset] == [0, 4, 8, 12]
    assert C.sizeof(Shift) == 32 and C.sizeof(O.SphObstacle) == 48
    assert B.ABI_VERSION == 7 and O.MAX_PATH_KEYS == 16384
    assert B.PROTOTYPES["sph_hip_set_obstacle_paths"] == (C.c_int, [C.c_void_p, C.POINTER(P), C.c_int, C.POINTER(K),
                                                                     C.c_int])
    assert B.PROTOTYPES["sph_hip_get_obstacle_paths"] == (C.c_int, [C.c_void_p, C.POINTER(P), C.c_int, C.POINTER(K),
                                                                     C.c_int, C.c_void_p])


def _good_paths():
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    return [O.MotionPath.stroke((0.5, 0.0, -0.25), 2.0), None,
            O.MotionPath([0.0, 0.5, 1.5], [(0, 0, 0), (1, 2, 3), (0, 0, 0)], 0.25, True)]


def test_every_refusal_has_its_text(policy):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    pa, n, ka, nk = O.as_path_arrays(_good_paths())
    assert policy.check(pa, 3, ka, nk, 3) == b"" and policy.count_paths(pa, 3) == 2
    assert policy.check(None, 0, None, 0, 3) == b"" and policy.check(pa, 0, ka, nk, 3) == b""   # n = 0 clears
    texts = set()

    def refused(mutate, n_paths=3, n_obst=3, n_keys=None, no_paths=False, no_keys=False):
        pa, _, ka, nk = O.as_path_arrays(_good_paths())
        mutate(pa, ka)
        why = policy.check(None if no_paths else pa, n_paths, None if no_keys else ka, nk if n_keys is None else n_keys,
                           n_obst)
        texts.add(why)
        return why

    none = lambda pa, ka: None                                                             # noqa: E731
    assert b"count must be 0 or the obstacle count" in refused(none, n_paths=2)
    assert b"count must be 0 or the obstacle count" in refused(none, n_obst=4)
    assert b"count must be 0 or the obstacle count" in refused(none, n_paths=-1)
    assert refused(none, no_paths=True) == b"null path list"
    assert refused(none, no_keys=True) == b"null key list"
    assert b"key count must be in [0, 16384]" in refused(none, n_keys=-1)
    assert b"key count must be in [0, 16384]" in refused(none, n_keys=16385)
    assert b"at least two keys" in refused(lambda pa, ka: setattr(pa[0], "count", 1))
    assert b"key count must be >= 0" in refused(lambda pa, ka: setattr(pa[0], "count", -2))
    for first, count in ((-1, 2), (4, 2), (5, 2), (0, 6), (2 ** 31 - 1, 2), (1, 2 ** 31 - 1)):
        def rng(pa, ka, first=first, count=count):
            pa[2].first, pa[2].count = first, count
        assert b"leave the key list" in refused(rng), (first, count)
    assert b"first key must be at t = 0" in refused(lambda pa, ka: setattr(ka[0], "t", 0.125))
    assert b"first key must be at t = 0" in refused(lambda pa, ka: setattr(ka[2], "t", -0.5))
    for bad in (0.5, 0.25, np.nan, np.inf):                          # keys 2..4 are (0, 0.5, 1.5)
        assert b"finite and strictly increasing" in refused(lambda pa, ka, bad=bad: setattr(ka[4], "t", bad)), bad
    assert b"finite and strictly increasing" in refused(lambda pa, ka: setattr(ka[3], "t", np.nan))
    for bad in (np.nan, np.inf, -np.inf):
        for c in range(3):
            assert b"displacements must be finite" in refused(lambda pa, ka, bad=bad, c=c: ka[3].d.__setitem__(c, bad))
        assert b"start must be finite and >= 0" in refused(lambda pa, ka, bad=bad: setattr(pa[0], "start", bad))
    assert b"start must be finite and >= 0" in refused(lambda pa, ka: setattr(pa[2], "start", -0.5))
    for c in range(3):
        assert b"cyclic path must end" in refused(lambda pa, ka, c=c: ka[4].d.__setitem__(c, 0.5))
    assert b"cyclic path must end" in refused(lambda pa, ka: setattr(pa[0], "cycle", 1))
    assert len(texts) == 12 and b"" not in texts, texts
    # what is allowed: -0 as the first time and as a start, a cyclic path ending at -0 for +0, count == 0 with
    # any first, cycle values other than 1
    assert refused(lambda pa, ka: setattr(ka[0], "t", -0.0)) == b""
    assert refused(lambda pa, ka: setattr(pa[0], "start", -0.0)) == b""
    assert refused(lambda pa, ka: ka[4].d.__setitem__(1, -0.0)) == b""
    assert refused(lambda pa, ka: setattr(pa[1], "first", 999)) == b""
    assert refused(lambda pa, ka: setattr(pa[2], "cycle", -7)) == b""
    full = [O.MotionPath(np.arange(16384, dtype=F32), np.zeros((16384, 3), F32))]
    pa, n, ka, nk = O.as_path_arrays(full)
    assert nk == 16384 and policy.check(pa, 1, ka, nk, 1) == b""


def test_pair_checks_in_both_directions(policy):
    """path_motion_check and path_body_check are each one function: the new paths against the motions / bodies
    in force, and the new motions / bodies against the paths in force"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    pa, n, ka, nk = O.as_path_arrays(_good_paths())
    on_free = O.as_motion_array([None, O.Motion((1, 0, 0)), O.Motion((0, 0, 0), 0.0, 1.0)])[0]
    on_path = O.as_motion_array([None, None, O.Motion((0, -2, 0))])[0]
    assert policy.check_motion(pa, 3, on_free, 3) == b""
    assert policy.check_motion(pa, 3, on_path, 3) == b"a path on an obstacle whose motion moves"
    assert policy.check_motion(pa, 3, None, 0) == b"" and policy.check_motion(None, 0, on_path, 3) == b""
    body = O.Body(5.0)
    some, _ = O.as_body_array([None, body, None])
    nobody, _ = O.as_body_array([None, None, None])
    assert b"paths and free bodies in one obstacle list" in policy.check_body(pa, 3, some, 3)
    assert policy.check_body(pa, 3, nobody, 3) == b"" and policy.check_body(pa, 3, None, 0) == b""
    assert policy.check_body(None, 0, some, 3) == b""
    empty, _, _, _ = O.as_path_arrays([None, None, None])
    assert policy.check_body(empty, 3, some, 3) == b"" and policy.check_motion(empty, 3, on_path, 3) == b""


# ---- path_displacement ----------------------------------------------------------------------------

def seeded_path(k, rng, cycle, start=0.0, ulp_segments=False):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    t = np.concatenate([[0.0], np.cumsum(rng.uniform(0.001, 0.02, k - 1))]).astype(F32)
    if ulp_segments:                                                 # every second segment one ulp long
        for j in range(1, k, 2):
            t[j] = np.nextafter(t[j - 1], F32(np.inf))
        t = np.maximum.accumulate(t)
        for j in range(1, k):
            if not t[j] > t[j - 1]:
                t[j] = np.nextafter(t[j - 1], F32(np.inf))
    d = rng.normal(0.0, 0.3, (k, 3)).astype(F32)
    if cycle:
        d[-1] = d[0]
    return O.MotionPath(t, d, start, cycle)


def probe_taus(path, rng):
    """tau on every key, one float either side of it, before the start, at T and beyond, wraps, up to 1e6"""
    start, t = F32(path.start), path.times
    on = (start + t).astype(F32)
    taus = [on, np.nextafter(on, F32(-np.inf)), np.nextafter(on, F32(np.inf))]
    T = t[-1]
    taus.append(F32([0.0, float(start) * 0.5, float(start), float(start + T), float(start + T) * 1.5 + 1.0, 1e6, 3.0e38]))
    taus.append((start + T * F32(rng.uniform(0.0, 1000.0, 300))).astype(F32))      # over 1 000 wraps when cyclic
    taus.append((start + T * np.arange(0, 1001, 37, dtype=F32)).astype(F32))       # on whole periods
    taus.append(rng.uniform(0.0, 1e6, 100).astype(F32))
    return np.concatenate(taus)


@pytest.mark.parametrize("k", [2, 3, 64, 1024])
def test_displacement_matches_the_restatement(policy, k):
    rng = np.random.default_rng(500 + k)
    for cycle in (False, True):
        for start, first, ulp in ((0.0, 0, False), (0.375, 5, False), (0.01, 3, True)):
            path = seeded_path(k, rng, cycle, start, ulp)
            taus = probe_taus(path, rng)
            got = header_displacements(policy, path, taus, first, first + k + 2)
            vel = header_displacements(policy, path, taus, first, first + k + 2, velocity=True)
            want = np.array([PE.displacement(path, tau) for tau in taus])
            assert same_bits(got, want), (k, cycle, start)
            assert same_bits(got, np.array([path.displacement_at(tau) for tau in taus]))
            assert same_bits(vel, np.array([PE.velocity(path, tau) for tau in taus]))
            assert same_bits(vel, np.array([path.velocity_at(tau) for tau in taus]))
            assert np.isfinite(got).all()
            before = taus < F32(start)
            assert same_bits(got[before], np.broadcast_to(path.displacements[0] + F32(0) * F32(0), (int(before.sum()), 3)))
            assert not vel[before].any()
            if not cycle:
                after = (taus - F32(start)).astype(F32) > path.times[-1]
                assert after.sum() > 100 and not vel[after].any()
                assert np.allclose(got[after], path.displacements[-1], rtol=0, atol=2e-6)


# ---- k_paths_eval's lane loop ---------------------------------------------------------------------

@pytest.mark.parametrize("n,every", [(1, 1), (63, 1), (63, 2), (64, 1), (64, 2), (64, 65)])
def test_eval_lane_loop(policy, n, every):
    """paths_eval is k_paths_eval with the lanes as a loop: lane i = obstacle i; every `every`-th entry has a
    path (65: none), of differing key counts"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(600 + n + every)
    paths = [seeded_path(2 + (i * 37) % 60, rng, i % 3 == 0, 0.002 * (i % 5)) if i % every == 0 and every < 65 else None
             for i in range(n)]
    pa, _, ka, nk = O.as_path_arrays(paths)
    for tau0, tau1 in ((0.0, 0.004), (0.004, 0.008), (0.3, 0.3), (12.0, 12.5)):
        out = (Shift * n)()
        policy.eval(pa, ka, n, tau0, tau1, out)
        want, has = PE.shifts(paths, tau0, tau1)
        got = np.array([[list(s.D0), list(s.D1)] for s in out], F32)
        assert same_bits(got, want)
        assert [s.has_path for s in out] == [int(h) for h in has] and not any(s.pad for s in out)


def test_obstacle_at_with_a_path(policy):
    """path_obstacle_at is what sph_hip_get_obstacles_now returns: an entry with a path is always shifted (-0 + 0
    = +0), one without takes obstacle_at with its motion"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(61)
    solids = [o for kind in (E.SPHERE, E.BOX, E.CYLINDER) for o in _obstacle_set(kind, rng)[:2]] + wedge_set()[:3]
    path = seeded_path(5, rng, False, 0.1)
    path.displacements[0] = 0.0
    pa, _, ka, _ = O.as_path_arrays([path])
    motion = O.Motion((1.0, -2.0, 0.5), 0.1, 0.9)
    for o in solids:
        st = o.as_struct()
        st.lo[0] = -0.0
        for tau in (0.0, 0.1, 0.11, 0.5, 7.0):
            out = O.SphObstacle()
            policy.at(C.byref(st), pa, ka, None, tau, C.byref(out))
            assert bytes(out) == bytes(PE.obstacle_at(st, path, None, tau))
            policy.at(C.byref(st), None, None, C.byref(motion.as_struct()), tau, C.byref(out))
            assert bytes(out) == bytes(PE.obstacle_at(st, None, motion, tau)) == bytes(W.obstacle_at(st, motion, tau))
            policy.at(C.byref(st), None, None, None, tau, C.byref(out))
            assert bytes(out) == bytes(st)
        policy.at(C.byref(st), pa, ka, None, 0.0, C.byref(out))
        assert not (path.displacement_at(0.0) != 0).any()
        assert math.copysign(1.0, out.lo[0]) == 1.0 and math.copysign(1.0, st.lo[0]) == -1.0


# ---- the turn, header vs numpy --------------------------------------------------------------------

def timed_paths(o_ext, rng, dt):
    """(MotionPath, tau0, tau1) around a solid of extent o_ext: inside a segment, straddling the start,
    straddling the last key, before the start, after the end, dt == 0, reversing direction inside the step, and
    a cyclic path after several wraps"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    dt = F32(dt)
    t0 = F32(rng.uniform(0.05, 0.2))
    t1 = F32(t0 + dt)
    far = (rng.normal(0.0, 1.0, 3) * o_ext * float(rng.choice([2.0, 20.0, 200.0]))).astype(F32)   # per unit time
    far[rng.random(3) < 0.25] = 0.0
    if not (far != 0).any():
        far[0] = F32(o_ext)
    step = (far * dt).astype(F32)
    turn_at = float(t0 + dt * F32(0.5))
    period = float(dt) * 3.5
    return [
        (O.MotionPath([0.0, 1.0], [(0, 0, 0), far]), t0, t1),
        (O.MotionPath([0.0, 1.0], [(0, 0, 0), far], float(t0 + dt * F32(0.3))), t0, t1),
        (O.MotionPath([0.0, float(t0 + dt * F32(0.6))], [(0, 0, 0), far * F32(t0)]), t0, t1),
        (O.MotionPath([0.0, 1.0], [(0, 0, 0), far], float(t0 + F32(1.0))), t0, t1),
        (O.MotionPath([0.0, float(t0 * F32(0.5))], [step, far * F32(t0)]), t0, t1),
        (O.MotionPath([0.0, 1.0], [(0, 0, 0), far]), t0, t0),
        (O.MotionPath([0.0, turn_at, 2.0 * turn_at], [(0, 0, 0), far * F32(turn_at), (0, 0, 0)]), t0, t1),
        (O.MotionPath([0.0, 0.3 * period, 0.8 * period, period], [(0, 0, 0), step * F32(2), -step, (0, 0, 0)], 0.01,
                      True), t0, t1),
    ]


def _box_of(o):
    """the bounding box of a solid struct, as an obstacles.Box (what cases() aims at)"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    kind, axis, c, r, lo, hi = E.fields(o)
    if kind == E.SPHERE:
        return O.Box(c - r, c + r)
    if kind == E.CYLINDER:
        blo, bhi = c - r, c + r
        blo[axis], bhi[axis] = lo[axis], hi[axis]
        return O.Box(blo, bhi)
    return O.Box(lo, hi)


def path_cases(o, D0, D1, m, dt, rng):
    """test_obstacles_cpu.cases around the solid as it stands at tau1 - faces, edges, corners, grazing lines, q on
    the surface - plus: p inside the solid as it stood at tau0, the solid overtaking particles at rest, particles
    overtaking the solid"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    o1 = W.shifted(o, D1)
    b1, b0 = _box_of(o1), _box_of(W.shifted(o, D0))
    aim = b1 if int(o1.kind) == W.WEDGE else O.from_struct(o1)
    P, V, Q = cases(aim, m, dt, rng)
    k = m // 10
    a = slice(5 * k, 6 * k)
    P[a] = (b0.lo + rng.random((k, 3)) * (b0.hi - b0.lo)).astype(F32)
    Q[a] = (P[a] + V[a] * F32(dt)).astype(F32)
    b = slice(6 * k, 7 * k)
    P[b] = (b1.lo + rng.random((k, 3)) * (b1.hi - b1.lo)).astype(F32)
    V[b] = 0.0
    Q[b] = P[b]
    c = slice(7 * k, 8 * k)
    with np.errstate(all="ignore"):
        vel = ((np.asarray(D1, F32) - np.asarray(D0, F32)) / F32(dt if dt > 0 else 1.0)).astype(F32)
    V[c] = (vel * rng.uniform(1.2, 4.0, (k, 1))).astype(F32)
    Q[c] = (b1.lo + rng.random((k, 3)) * (b1.hi - b1.lo)).astype(F32)
    P[c] = (Q[c] - V[c] * F32(dt)).astype(F32)
    return P, V, Q


def solids_of(kind, rng):
    return wedge_set() if kind == W.WEDGE else _obstacle_set(kind, rng)


KINDS = [E.SPHERE, E.BOX, E.CYLINDER, W.WEDGE]
KIND_IDS = ["sphere", "box", "cylinder", "wedge"]


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_turn_header_equals_numpy_bit_for_bit(policy, kind):
    rng = np.random.default_rng(7000 + kind)
    dt, damping = F32(0.004), F32(0.6)
    solids = solids_of(kind, rng)
    rows = 120000 // (8 * len(solids)) + 1
    total = active = boosted = 0
    for o in solids:
        ext = float((_box_of(o.as_struct()).hi - _box_of(o.as_struct()).lo).mean())
        for path, tau0, tau1 in timed_paths(ext, rng, dt):
            step = dt if tau1 != tau0 else F32(0.0)
            D0, D1 = PE.displacement(path, tau0), PE.displacement(path, tau1)
            P, V, Q = path_cases(o, D0, D1, rows, dt, rng)
            hv, hq = header_respond(policy, [o], [path], None, P, V, Q, step, damping, tau0, tau1)
            ev, eq, act = PE.respond_one(o, path, None, P, V, Q, step, damping, tau0, tau1)
            assert same_bits(hv, ev) and same_bits(hq, eq), (kind, path, tau0, tau1)
            assert same_bits(hv[~act], V[~act]) and same_bits(hq[~act], Q[~act])
            total += P.shape[0]
            active += int(act.sum())
            boosted += int(act.sum()) if (D1 != D0).any() else 0
    assert total >= 120000
    assert active > 10000 and boosted > 4000, (active, boosted)


def mixed_list():
    """a static box with -0 fields, a cylinder on a Motion, a sphere and a wedge on paths, overlapping"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    neg = O.Box((-0.0, -1.0, -0.5), (1.2, 0.3, 0.5)).as_struct()
    neg.lo[0] = -0.0
    obst = [neg, O.Cylinder(1, (0.4, 0.0, 0.3), 0.5, -0.8, 0.8), O.Sphere((0.0, 0.0, 0.0), 0.7),
            O.Wedge.ramp((-0.9, -0.2, -0.2), (-0.1, 0.6, 0.7), 0, 1)]
    motions = [None, O.Motion((0.0, 25.0, 0.0), 0.101, 0.2), None, None]
    paths = [None, None, O.MotionPath.sine((0.1, 0.0, -0.04), 0.03, 16),
             O.MotionPath([0.0, 0.05, 0.15], [(0, 0, 0), (0.5, 0.1, 0.0), (0, 0, 0)], 0.06)]
    return obst, paths, motions


def test_mixed_list_header_equals_numpy(policy):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(79)
    obst, paths, motions = mixed_list()
    dt, damping = F32(0.004), F32(0.3)
    tau0 = F32(0.1)
    tau1 = F32(tau0 + dt)
    P, V, Q = cases(O.Box((-1.0, -1.0, -1.0), (1.2, 1.0, 1.0)), 100000, dt, rng)
    hv, hq = header_respond(policy, obst, paths, motions, P, V, Q, dt, damping, tau0, tau1)
    ev, eq = PE.respond(obst, paths, motions, P, V, Q, dt, damping, tau0, tau1)
    assert same_bits(hv, ev) and same_bits(hq, eq)
    mv, mq = header_moving(policy, obst, motions, P, V, Q, dt, damping, tau0, tau1)
    assert not same_bits(hq, mq), "the paths must change something"
    on_neg_face = (hq[:, 0] == 0) & np.signbit(hq[:, 0])
    assert on_neg_face.sum() > 10, "the static box's -0 face must reach some q"
    # without paths in the list every entry takes the turn it takes now
    nv, nq = header_respond(policy, obst, [None] * 4, motions, P, V, Q, dt, damping, tau0, tau1)
    assert same_bits(nv, mv) and same_bits(nq, mq)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_recorder_equals_numpy(policy, kind):
    rng = np.random.default_rng(8000 + kind)
    dt, damping = F32(0.004), F32(0.6)
    maxv = F32([2.5, 2.5, 2.5])
    responses = 0
    for o in solids_of(kind, rng)[:3]:
        ext = float((_box_of(o.as_struct()).hi - _box_of(o.as_struct()).lo).mean())
        for path, tau0, tau1 in timed_paths(ext, rng, dt):
            step = dt if tau1 != tau0 else F32(0.0)
            P, V, Q = path_cases(o, PE.displacement(path, tau0), PE.displacement(path, tau1), 3000, dt, rng)
            mass = rng.uniform(0.5, 2.0, P.shape[0]).astype(F32)
            for walls in (False, True):
                hv, hq, imp, cnt, skp = header_loads(policy, maxv, walls, [o], [path], None, P, V, Q, mass, step,
                                                     damping, tau0, tau1)
                ev, eq, row = PE.integrate_respond(maxv, walls, [o], [path], None, P, V, Q, step, damping, tau0, tau1,
                                                   mass)
                assert same_bits(hv, ev) and same_bits(hq, eq)
                assert row.same(imp, cnt, skp), (kind, path, walls)
                responses += int(cnt[6])
    assert responses > 10000


def test_mixed_list_recorder(policy):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(80)
    obst, paths, motions = mixed_list()
    dt, damping = F32(0.004), F32(0.3)
    maxv = F32([1.2, 1.0, 1.0])
    for tau0 in (0.0, 0.06, 0.1, 0.204):
        tau0 = F32(tau0)
        tau1 = F32(tau0 + dt)
        P, V, Q = cases(O.Box((-1.0, -1.0, -1.0), (1.2, 1.0, 1.0)), 30000, dt, rng)
        mass = rng.uniform(0.5, 2.0, 30000).astype(F32)
        hv, hq, imp, cnt, skp = header_loads(policy, maxv, True, obst, paths, motions, P, V, Q, mass, dt, damping, tau0,
                                             tau1, -20)
        ev, eq, row = PE.integrate_respond(maxv, True, obst, paths, motions, P, V, Q, dt, damping, tau0, tau1, mass, -20)
        assert same_bits(hv, ev) and same_bits(hq, eq) and row.same(imp, cnt, skp), tau0
        assert (cnt[6:10] > 50).all(), (tau0, cnt[6:10])


# ---- anchors ------------------------------------------------------------------------------------

def test_two_key_path_is_the_motion(policy):
    """Dyadic v, T and start: w = u / T and v * T are exact, so the two-key path (0, 0) -> (T, v * T) started at
    `start` and Motion(v, start, start + T) have the same D, the same response and the same loads"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(33)
    dt, damping = F32(2.0 ** -8), F32(0.5)
    v, T, start = F32([4.0, -2.5, 0.75]), F32(0.25), F32(0.125)
    path = O.MotionPath([0.0, T], [(0, 0, 0), (v * T).astype(F32)], start)
    motion = O.Motion(v, start, float(start + T))
    assert np.array_equal((v * T).astype(np.float64), v.astype(np.float64) * float(T))
    obst = [O.Sphere((0.4, 0.5, 0.5), 0.3), O.Box((0.9, 0.1, 0.2), (1.4, 0.8, 0.9)),
            O.Cylinder(2, (0.3, 1.2, 0.0), 0.2, 0.1, 1.1), O.Wedge.ramp((1.5, 0.05, 0.05), (2.0, 0.5, 1.0), 0, 1)]
    maxv = F32([3.0, 3.0, 3.0])
    acted = 0
    for tau in M.clock(dt, 120):
        D = PE.displacement(path, tau)
        assert np.array_equal(D, M.displacement(motion, tau)), tau
        if tau <= start:
            assert not D.any()
        if tau >= start + T:
            assert np.array_equal(D, (v * T).astype(F32))
    for tau0 in (0.0, 0.125 - 2.0 ** -9, 0.125, 0.2, 0.375 - 2.0 ** -9, 0.375, 0.5):
        tau0 = F32(tau0)
        tau1 = F32(tau0 + dt)
        for o in obst:
            P, V, Q = path_cases(o, PE.displacement(path, tau0), PE.displacement(path, tau1), 4000, dt, rng)
            mass = rng.uniform(0.5, 2.0, P.shape[0]).astype(F32)
            a = header_loads(policy, maxv, True, [o], [path], None, P, V, Q, mass, dt, damping, tau0, tau1)
            b = header_loads(policy, maxv, True, [o], None, [motion], P, V, Q, mass, dt, damping, tau0, tau1)
            for x, y in zip(a, b):
                assert np.array_equal(x, y, equal_nan=x.dtype == F32), (tau0, o, np.argwhere(x != y)[:4])
            acted += int(a[3][6])
    assert acted > 5000


def test_piston_on_a_path_leaves_fluid_at_rest_at_twice_its_speed(policy):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(34)
    dt, damping = F32(0.004), F32(0.6)
    u = F32(12.5)
    piston = O.Box((0.0, 0.0, 0.0), (0.5, 1.0, 1.0))
    path = O.MotionPath.stroke((float(u) * 2.0, 0.0, 0.0), 2.0)
    tau0 = F32(0.2)
    tau1 = F32(tau0 + dt)
    face0 = F32(0.5) + PE.displacement(path, tau0)[0]
    face1 = F32(0.5) + PE.displacement(path, tau1)[0]
    P = np.stack([rng.uniform(float(face0), float(face1), 5000), rng.uniform(0.1, 0.9, 5000),
                  rng.uniform(0.1, 0.9, 5000)], 1).astype(F32)
    P = P[(P[:, 0] > face0) & (P[:, 0] < face1)]
    V = np.zeros_like(P)
    hv, hq = header_respond(policy, [piston], [path], None, P, V, P, dt, damping, tau0, tau1)
    assert P.shape[0] > 4000
    assert np.allclose(hv[:, 0], 2.0 * float(u), rtol=1e-4) and not hv[:, 1:].any()
    assert (hq[:, 0] >= face1).all() and same_bits(hq[:, 1:], P[:, 1:])
    assert np.allclose(PE.velocity(path, tau0), [float(u), 0, 0]) and same_bits(PE.velocity(path, tau0), path.velocity_at(tau0))


def test_sine_stays_close_to_the_sine():
    """MotionPath.sine(A, period, K) against A sin(2 pi tau / period) in float64, over the first three periods.
    The bound, per component of amplitude A:
      interpolation  a chord of f over a segment of length s errs by at most max|f''| s^2 / 8; here s = period / K
                     and |f''| <= A (2 pi / period)^2: A (2 pi / K)^2 / 8.
      fp32           e = 2^-24.  The keys: d_k rounded, A e; t_k rounded, at most period e each, which moves the
                     chord by at most its slope times 2 period e = 4 pi A e.  The path time: k T and u - k T rounded
                     with u < 3 period, at most 4 period e, times the slope: 8 pi A e.  The interpolation itself
                     (a difference, a quotient, a product and a sum of values not above A): 2 A e.
                     Together A e (1 + 4 pi + 8 pi + 2) < 24 A 2^-23."""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(35)
    for K, period, amp in ((64, 0.4, (0.03, 0.0, 0.0)), (16, 0.008, (0.05, -0.02, 0.01)), (256, 3.0, (1.0, 2.0, -0.5))):
        path = O.MotionPath.sine(amp, period, K)
        assert path.cycle and path.times.size == K + 1 and path.times[0] == 0
        assert path.displacements[0].tobytes() == path.displacements[-1].tobytes()
        A = np.abs(np.float64(amp))
        bound = A * (2.0 * math.pi / K) ** 2 / 8.0 + 24.0 * A * 2.0 ** -23
        taus = rng.uniform(0.0, 3.0 * period, 4000).astype(F32)
        got = np.array([path.displacement_at(tau) for tau in taus], np.float64)
        want = np.sin(2.0 * math.pi * taus.astype(np.float64) / period)[:, None] * np.float64(amp)[None, :]
        err = np.abs(got - want).max(0)
        print("K", K, "error", err, "bound", bound)
        assert (err <= bound).all()
        assert (err[A > 0] > 0.2 * (A * (2.0 * math.pi / K) ** 2 / 8.0)[A > 0]).all(), "the chords must be felt"


# ---- routes ---------------------------------------------------------------------------------------

def test_route_decisions(policy):
    for n_obst in (0, 1, 64):
        for n_paths in (0, 1, 64):
            assert policy.path_kernels(n_obst, n_paths) == int(n_obst > 0 and n_paths > 0)
            for n_moving in (0, 2):
                assert policy.path_clock(n_obst, n_moving, n_paths) == int(n_obst > 0 and (n_moving > 0 or n_paths > 0))
                # without paths the clock runs exactly when it ran
                assert policy.path_clock(n_obst, n_moving, 0) == policy.old_clock(n_obst, n_moving, 0)
    # the unchanged decisions
    assert policy.moving_kernels(3, 1) == 1 and policy.moving_kernels(3, 0) == 0 and policy.moving_kernels(0, 1) == 0
    assert policy.body_kernels(3, 1) == 1 and policy.body_kernels(3, 0) == 0
    assert policy.old_clock(3, 0, 1) == 1 and policy.old_clock(3, 0, 0) == 0
    assert policy.fused_integrate(1, 1, 100, 0, 0, 0) == 1
    assert policy.fused_integrate(1, 1, 100, 0, 1, 0) == 0      # a list with obstacles is unfused already


# ---- Python ---------------------------------------------------------------------------------------

def test_python_round_trips():
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    paths = _good_paths() + [O.MotionPath.sine((0.0, 0.2, 0.0), 0.5, 8, start=0.25)]
    pa, n, ka, nk = O.as_path_arrays(paths)
    assert n == 4 and nk == 2 + 3 + 9
    assert [(s.first, s.count, s.cycle) for s in pa] == [(0, 2, 0), (0, 0, 0), (2, 3, 1), (5, 9, 1)]
    back = O.paths_from_arrays(pa, n, ka)
    assert back == paths and back[1] is None
    assert paths[0] != paths[2] and paths[0] != O.MotionPath.stroke((0.5, 0.0, -0.25), 2.5)
    assert paths[0] == O.MotionPath([0.0, 2.0], [(0, 0, 0), (0.5, 0.0, -0.25)])
    assert paths[0] != O.MotionPath([0.0, 2.0], [(-0.0, 0, 0), (0.5, 0.0, -0.25)])       # bitwise
    assert "2 keys" in repr(paths[0]) and "cyclic" in repr(paths[2]) and "cyclic" not in repr(paths[0])
    s = O.MotionPath.stroke((1.0, 2.0, 3.0), 0.5, start=1.0)
    assert s.times.tolist() == [0.0, 0.5] and not s.cycle and s.start == 1.0
    assert same_bits(s.displacement_at(1.25), F32([0.5, 1.0, 1.5])) and same_bits(s.displacement_at(9.0), F32([1, 2, 3]))
    assert not s.displacement_at(0.5).any() and not s.velocity_at(0.5).any() and not s.velocity_at(9.0).any()
    assert same_bits(s.velocity_at(1.25), F32([2.0, 4.0, 6.0]))
    with pytest.raises(ValueError):
        O.MotionPath([0.0, 1.0], [(0, 0, 0)])
    with pytest.raises(ValueError):
        O.MotionPath.sine((1, 0, 0), 1.0, 1)
    empty = O.as_path_arrays([])
    assert empty[1] == 0 and empty[3] == 0


def test_wave_flume_as_built(policy):
    from smoothed_particle_hydrodynamics_amd import gauges as G
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass, obst, paths, cols = scenes.wave_flume(20000, 0.06, 0.4, 15.0)
    h = float(p.h)
    piston, beach = obst
    assert isinstance(piston, O.Box) and isinstance(beach, O.Wedge) and W.check(beach) == ""
    assert float(piston.hi[0] - piston.lo[0]) == pytest.approx(2.0 * h, rel=1e-5)
    assert piston.lo[1] < 0 and piston.hi[1] > float(p.max_y) and piston.lo[2] < 0 and piston.hi[2] > float(p.max_z)
    assert beach.normal[0] < 0 < beach.normal[1] and beach.lo[1] == 0.0 and float(beach.hi[0]) >= 2.0
    assert math.degrees(math.atan2(-float(beach.normal[0]), float(beach.normal[1]))) == pytest.approx(15.0, abs=1e-3)
    assert p.apply_gravity == 1 and p.apply_walls == 1 and p.gravity[1] < 0
    assert paths[1] is None and paths[0].cycle and paths[0].times.size == 65
    assert float(paths[0].times[-1]) == pytest.approx(0.4) and not paths[0].displacements[:, 1:].any()
    assert float(np.abs(paths[0].displacements[:, 0]).max()) == pytest.approx(0.03, rel=1e-6)
    assert float(piston.lo[0]) - 0.03 > 0.0, "the piston's back face stays inside the tank"
    pa, n, ka, nk = O.as_path_arrays(paths)
    assert policy.check(pa, n, ka, nk, 2) == b""
    x = pos.reshape(-1, 3)
    assert 0 < mass.size <= 20000 and not vel.any() and not O.inside_any(x, obst).any()
    assert x[:, 0].min() >= float(piston.hi[0]) and x[:, 1].max() <= 0.25
    assert len(cols) == 4 and all(isinstance(g, G.ColumnGauge) and g.axis == 1 for g in cols)
    xs = [g.base[0] for g in cols]
    assert xs == sorted(xs) and float(piston.hi[0]) + 0.03 < xs[0] and xs[-1] < float(beach.lo[0])
    assert all(g.base[2] == pytest.approx(0.5 * float(p.max_z)) and g.iso > 0 for g in cols)
    with pytest.raises(ValueError):
        scenes.wave_flume(20000, 0.06, 0.4, 2.0)


def test_wave_flume_steps_on_the_cpu(oracle):
    """wave_flume at 20 000 particles, 20 FULL steps with the oracle and the restatement: everything finite,
    nobody inside a solid beyond rounding, and some particle changed by the paddle while it moved"""
    from helpers import to_oracle_params
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass, obst, paths, _ = scenes.wave_flume(20000)
    op = to_oracle_params(p)
    clock = M.clock(p.time_step, 20)
    counts = [0, 0]
    for k in range(20):
        pos, vel, _ = PE.oracle_step(oracle, op, obst, paths, None, pos, vel, mass, clock[k], clock[k + 1], counts=counts)
    print("changed by the paddle while moving / standing:", counts)
    assert np.isfinite(pos).all() and np.isfinite(vel).all()
    assert counts[0] > 0
    face = float(obst[0].hi[0]) + float(PE.displacement(paths[0], clock[-1])[0])
    assert face > float(obst[0].hi[0]) and pos.reshape(-1, 3)[:, 0].min() >= face - 1e-6


# ---- the new header code under the sanitizers, in a program of its own ----------------------------

MAIN = CALLS + r"""
#include <stdio.h>
#include <stdlib.h>
// hostile path lists: counts, firsts, times and displacements that are huge, tiny, zero, NaN or infinite
// (path_check's business is to refuse them: only an accepted list is ever evaluated, as on the device), and for
// the accepted ones hostile clocks, particles and time steps through every function of the fourth part
static unsigned long long state = 88172645463325252ull;
static unsigned next() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (unsigned)(state >> 32); }
static float pick()
{
   static const float odd[] = {0.0f, -0.0f, 1.0f, -1.0f, 0.5f, 1e-30f, -1e-30f, 1e30f, -1e30f, 3.4e38f, -3.4e38f,
                               INFINITY, -INFINITY, NAN, 1e-45f, 1e6f};
   const unsigned r = next();
   if (r & 1) return odd[(r >> 1) % (sizeof(odd) / sizeof(odd[0]))];
   return ((int)(r >> 8) % 2001 - 1000) / 500.0f;
}
int main()
{
   enum { N = 5, KEYS = 64 };
   long long checksum = 0;
   int refused = 0, accepted = 0;
   for (int k = 0; k < 20000; k++) {
      sph_hip_motion_key keys[KEYS];
      sph_hip_motion_path paths[N];
      const bool tame = k % 2 == 0;
      int used = 0;
      for (int i = 0; i < N; i++) {
         const int count = tame ? (i == 1 ? 0 : 2 + (int)(next() % 9)) : (int)(next() % 12) - 2;
         paths[i].first = tame ? used : (int)(next() % 70) - 3;
         paths[i].count = count;
         paths[i].start = tame ? (float)(next() % 8) * 0.125f : pick();
         paths[i].cycle = (int)(next() % 3) - 1;
         float t = 0.0f;
         for (int j = 0; j < count && used + j < KEYS; j++) {
            sph_hip_motion_key& key = keys[used + j];
            key.t = tame ? t : pick();
            t += (next() & 1) ? 1e-3f * (1 + next() % 50) : t * 1.1920929e-7f + 1e-45f;
            for (int c = 0; c < 3; c++) key.d[c] = tame && (next() % 16) ? ((int)(next() % 200) - 100) / 50.0f : pick();
         }
         if (tame && count > 0 && paths[i].cycle)
            for (int c = 0; c < 3; c++) keys[used + count - 1].d[c] = keys[used].d[c];
         if (count > 0) used += count;
         if (used > KEYS) used = KEYS;
      }
      for (int j = used; j < KEYS; j++) keys[j].t = keys[j].d[0] = keys[j].d[1] = keys[j].d[2] = NAN;
      if (path_check(paths, N, keys, used, N)) {
         refused++;
         continue;
      }
      accepted++;
      sph_hip_obstacle list[N];
      memset(list, 0, sizeof(list));
      for (int i = 0; i < N; i++) {
         list[i].kind = i % 4;
         list[i].axis = i % 3;
         list[i].radius = i % 4 == 3 ? 0.25f : 0.5f;
         for (int c = 0; c < 3; c++) {
            list[i].center[c] = i % 4 == 3 ? (c == 1 ? 1.0f : 0.0f) : 0.25f * i;
            list[i].lo[c] = -0.5f + 0.25f * i;
            list[i].hi[c] = 0.5f + 0.25f * i;
         }
      }
      sph_hip_obstacle_motion motion[N];
      memset(motion, 0, sizeof(motion));
      motion[1].velocity[0] = 3.0f;
      motion[1].stop = INFINITY;
      checksum += path_motion_check(paths, N, motion, N) ? 1 : 0;
      float p[3 * 8], v[3 * 8], q[3 * 8], mass[8];
      for (int i = 0; i < 24; i++) {
         p[i] = pick();
         v[i] = (i / 3) % 3 == 0 ? 0.0f : pick();
         q[i] = (i / 3) % 2 ? p[i] : pick();
      }
      for (int i = 0; i < 8; i++) mass[i] = 1.0f;
      const float dt = k % 3 ? 0.004f : 0.0f;
      const float tau0 = k % 5 ? fabsf(pick()) : 0.0f, tau1 = k % 7 ? tau0 + dt : pick();
      PathShift shift[N];
      eval(paths, keys, N, tau0, tau1, shift);
      for (int i = 0; i < N; i++) {
         float vel[3];
         sph_hip_obstacle now;
         at(&list[i], &paths[i], keys, &motion[i], tau1, &now);
         if (path_is(paths[i])) {
            velocities(&paths[i], keys, &tau1, 1, vel);
            checksum += vel[0] == 0.0f;
         }
         checksum += shift[i].has_path + (now.lo[0] == list[i].lo[0]);
      }
      respond(list, k & 1 ? motion : nullptr, paths, keys, N, 8, p, v, q, dt, 0.6f, tau0, tau1);
      long long row[LOAD_ROW_WORDS];
      memset(row, 0, sizeof(row));
      const float maxv[3] = {4.0f, 4.0f, 4.0f};
      respond_loads(maxv, k & 1, list, k & 2 ? motion : nullptr, paths, keys, N, 8, p, v, q, mass, dt, 0.6f, tau0, tau1,
                    -24, row);
      checksum += row[LOAD_ROW_COUNT + 6] + row[LOAD_ROW_COUNT + 8];
   }
   printf("accepted %d refused %d checksum %lld\n", accepted, refused, checksum);
   return accepted > 1000 && refused > 1000 ? 0 : 3;
}
"""


def test_new_header_code_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    src, exe = tmp_path / "path_main.cpp", tmp_path / "path_main"
    src.write_text(MAIN)
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == "", run.stderr
    assert run.stdout.split()[0] == "accepted"
