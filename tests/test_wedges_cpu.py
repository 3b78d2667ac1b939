"""CPU checks of the wedge obstacle (include/sph_hip.h: SPH_HIP_OBSTACLE_WEDGE): constants and every
refusal, the response of csrc/obstacle_policy.h (compiled with g++ behind an extern "C" shim) against the
numpy restatement tests/wedge_emulation.py bit for bit on seeded cases of every class, the anchors to the
box, a physical anchor, the shift, the moved response, the loads and a wedge body on mixed lists,
scene_hit_wedge, the Python side (obstacles.Wedge, scenes.dam_break_beach, scenes.channel_weir) and one
run of the new header code under the address and undefined-behaviour sanitizers in a stand-alone host
program."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import body_emulation as B
import load_emulation as L
import moving_obstacle_emulation as M
import obstacle_emulation as E
import wedge_emulation as W
from helpers import compile_shim
from test_bodies_cpu import DevState, dev_states
from test_loads_cpu import same_bits as same_bits_nan
from test_obstacles_cpu import cases, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smoothed_particle_hydrodynamics_amd", "csrc")
F32 = np.float32
PER_CLASS = 120000

# what both the shim and the sanitizer program call
CALLS = r"""
#include <stddef.h>
#include "body_policy.h"
#include "scene_policy.h"

extern "C" {
void respond(const sph_hip_obstacle* list, int n, int m, const float* p, float* v, float* q, float dt,
             float damping)
{
   for (int i = 0; i < m; i++) obstacles_respond(list, n, p + 3 * i, v + 3 * i, q + 3 * i, dt, damping);
}
void shifted(const sph_hip_obstacle* o, const float* D, sph_hip_obstacle* out) { *out = obstacle_shifted(*o, D); }
// walls when apply_walls, then the list: with bodies body_obstacles_respond, else with motions
// load_obstacles_respond_moving, else load_obstacles_respond; the row is the header's serial recorder's
void respond_full(const float* maxv, int apply_walls, const sph_hip_obstacle* list, const sph_hip_obstacle_motion* motion,
                  const sph_hip_body* bodies, const BodyState* states, int n, int m, const float* p, float* v, float* q,
                  const float* mass, float dt, float damping, float tau0, float tau1, int quantum_log2, long long* row)
{
   const LoadRowAdder rec = {row, load_scale(quantum_log2)};
   for (int i = 0; i < m; i++) {
      float *vi = v + 3 * i, *qi = q + 3 * i;
      if (apply_walls) load_walls_respond(maxv, damping, p + 3 * i, vi, dt, qi, mass[i], rec);
      if (bodies)
         body_obstacles_respond(list, motion, bodies, states, n, p + 3 * i, vi, qi, dt, damping, tau0, tau1, mass[i], rec);
      else if (motion)
         load_obstacles_respond_moving(list, motion, n, p + 3 * i, vi, qi, dt, damping, tau0, tau1, mass[i], rec);
      else
         load_obstacles_respond(list, n, p + 3 * i, vi, qi, dt, damping, mass[i], rec);
   }
}
void hit_many(const sph_hip_obstacle* o, const float* eye, const float* d, int n, float* t, float* nrm, int* ok)
{
   for (int i = 0; i < n; i++) {
      float ti = 0.0f, ni[3] = {0.0f, 0.0f, 0.0f};
      ok[i] = scene_hit(*o, eye + 3 * i, d + 3 * i, ti, ni) ? 1 : 0;
      t[i] = ok[i] ? ti : 0.0f;
      for (int c = 0; c < 3; c++) nrm[3 * i + c] = ok[i] ? ni[c] : 0.0f;
   }
}
const char* check(const sph_hip_obstacle* list, int n)
{
   const char* why = obstacle_check(list, n);
   return why ? why : "";
}
}
"""

SHIM = CALLS + r"""
extern "C" {
void constants(long long* out)
{
   out[0] = sizeof(sph_hip_obstacle);
   out[1] = SPH_HIP_OBSTACLE_SPHERE; out[2] = SPH_HIP_OBSTACLE_BOX; out[3] = SPH_HIP_OBSTACLE_CYLINDER;
   out[4] = SPH_HIP_OBSTACLE_WEDGE; out[5] = SPH_HIP_MAX_OBSTACLES; out[6] = SPH_HIP_ABI_VERSION;
}
}
"""


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    from smoothed_particle_hydrodynamics_amd.obstacles import SphBody, SphObstacle, SphObstacleMotion
    lib = compile_shim(SHIM, ["-O2", "-ffp-contract=off"], tmp_path_factory)
    PO, PM, PB, PS, V = (C.POINTER(SphObstacle), C.POINTER(SphObstacleMotion), C.POINTER(SphBody),
                         C.POINTER(DevState), C.c_void_p)
    lib.check.argtypes = [PO, C.c_int]
    lib.check.restype = C.c_char_p
    lib.respond.argtypes = [PO, C.c_int, C.c_int, V, V, V, C.c_float, C.c_float]
    lib.shifted.argtypes = [PO, V, PO]
    lib.respond_full.argtypes = [V, C.c_int, PO, PM, PB, PS, C.c_int, C.c_int, V, V, V, V, C.c_float, C.c_float,
                                 C.c_float, C.c_float, C.c_int, V]
    lib.hit_many.argtypes = [PO, V, V, C.c_int, V, V, V]
    lib.constants.argtypes = [C.POINTER(C.c_longlong)]
    return lib


def header_respond(lib, obstacles, P, V, Q, dt, damping):
    from smoothed_particle_hydrodynamics_amd.obstacles import as_array
    arr, n = as_array(obstacles)
    p = np.ascontiguousarray(P, F32).reshape(-1, 3)
    v = np.ascontiguousarray(V, F32).reshape(-1, 3).copy()
    q = np.ascontiguousarray(Q, F32).reshape(-1, 3).copy()
    lib.respond(arr, n, p.shape[0], p.ctypes.data, v.ctypes.data, q.ctypes.data, dt, damping)
    return v, q


def header_full(lib, maxv, apply_walls, obst, motions, bodies, st, P, V, Q, mass, dt, damping, tau0, tau1,
                e=L.QUANTUM_LOG2):
    """(V, Q, impulse, count, skipped) of the header's walls + list with its serial recorder"""
    from smoothed_particle_hydrodynamics_amd.obstacles import as_array, as_body_array, as_motion_array
    arr, n = as_array(obst)
    mot = as_motion_array(motions)[0] if motions else None
    bod = as_body_array(bodies)[0] if bodies else None
    states = dev_states(st) if bodies else None
    maxv = np.ascontiguousarray(maxv, F32)
    p = np.ascontiguousarray(P, F32).reshape(-1, 3)
    v = np.ascontiguousarray(V, F32).reshape(-1, 3).copy()
    q = np.ascontiguousarray(Q, F32).reshape(-1, 3).copy()
    m = np.ascontiguousarray(mass, F32)
    row = np.zeros(5 * L.SOLIDS, np.int64)
    lib.respond_full(maxv.ctypes.data, int(apply_walls), arr, mot, bod, states, n, p.shape[0], p.ctypes.data,
                     v.ctypes.data, q.ctypes.data, m.ctypes.data, dt, damping, tau0, tau1, int(e), row.ctypes.data)
    S = L.SOLIDS
    return v, q, row[:3 * S].reshape(S, 3), row[3 * S:4 * S], row[4 * S:]


# ---- constants and refusals ----------------------------------------------------------------------

def test_constants_and_layout(policy):
    from smoothed_particle_hydrodynamics_amd import lib as Lb
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    out = (C.c_longlong * 7)()
    policy.constants(out)
    assert list(out) == [48, 0, 1, 2, 3, 64, 7]
    assert (O.SPHERE, O.BOX, O.CYLINDER, O.WEDGE) == (0, 1, 2, 3) and C.sizeof(O.SphObstacle) == 48
    assert (Lb.OBSTACLE_SPHERE, Lb.OBSTACLE_BOX, Lb.OBSTACLE_CYLINDER, Lb.OBSTACLE_WEDGE) == (0, 1, 2, 3)
    assert Lb.ABI_VERSION == 7
    s = O.Wedge((0, 0, 0), (1, 2, 3), (0, 3, 4), 1.5).as_struct()
    assert s.kind == 3 and list(s.center) == [0.0, float(F32(0.6)), float(F32(0.8))] and s.radius == 1.5
    assert list(s.lo) == [0, 0, 0] and list(s.hi) == [1, 2, 3]


def test_every_refusal_has_its_text(policy):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    good = O.Wedge((0, 0, 0), (1, 2, 3), (0, 3, 4), 1.5)

    def why(mutate=None):
        s = good.as_struct()
        if mutate:
            mutate(s)
        a, k = O.as_array([s])
        got = policy.check(a, k).decode()
        assert got == W.check(s)
        return got

    assert why() == ""
    assert why(lambda s: setattr(s, "kind", 4)) == "unknown obstacle kind"
    assert why(lambda s: setattr(s, "axis", 77)) == ""                      # axis is ignored
    for bad in (np.nan, np.inf, -np.inf):
        for field in ("center", "lo", "hi"):
            for c in range(3):
                assert why(lambda s: getattr(s, field).__setitem__(c, bad)) == "obstacle fields must be finite"
        assert why(lambda s: setattr(s, "radius", bad)) == "obstacle fields must be finite"
    for a in range(3):
        assert why(lambda s: s.lo.__setitem__(a, s.hi[a])) == "a wedge needs lo < hi on every axis"
        assert why(lambda s: s.hi.__setitem__(a, -1.0)) == "a wedge needs lo < hi on every axis"
    unit = "a wedge's normal must have unit length"
    assert why(lambda s: s.center.__setitem__(1, 0.0)) == unit             # |n|^2 = 0.64
    assert why(lambda s: s.center.__setitem__(0, 0.01)) == unit            # |n|^2 = 1 + 1e-4
    assert why(lambda s: [s.center.__setitem__(k, 0.0) for k in range(3)]) == unit
    # the bound 2^-20 itself, formed in double from the float fields
    n1 = float(np.nextafter(F32(1.0), F32(2.0)))                            # |n|^2 - 1 = 2^-22 + 2^-46
    assert why(lambda s: [s.center.__setitem__(0, 0.0), s.center.__setitem__(1, 0.0), s.center.__setitem__(2, n1)]) == ""
    n8 = float(F32(1.0 + 2.0 ** -20))                                       # |n|^2 - 1 = 2^-19 + 2^-40
    assert why(lambda s: [s.center.__setitem__(0, 0.0), s.center.__setitem__(1, 0.0), s.center.__setitem__(2, n8)]) == unit
    empty = "a wedge's plane leaves nothing of its box"
    assert why(lambda s: setattr(s, "radius", 0.0)) == empty               # n.c >= 0 at every corner, = 0 at lo
    assert why(lambda s: setattr(s, "radius", -5.0)) == empty
    assert why(lambda s: setattr(s, "radius", 1e-6)) == ""                 # the corner lo alone
    assert why(lambda s: setattr(s, "radius", 1e30)) == ""                 # cuts nothing off: allowed
    # a wedge after other kinds, and the count rules as before
    arr, n = O.as_array([O.Sphere((1, 1, 1), 0.5), good, O.Box((0, 0, 0), (1, 1, 1))])
    assert policy.check(arr, n) == b""
    bad = good.as_struct()
    bad.radius = -5.0
    arr, n = O.as_array([O.Sphere((1, 1, 1), 0.5), bad])
    assert policy.check(arr, n).decode() == empty
    # the old kinds' refusals keep their texts
    s = O.Box((0, 0, 0), (1, 1, 1)).as_struct()
    s.hi[1] = 0.0
    arr, n = O.as_array([s])
    assert policy.check(arr, n) == b"a box needs lo < hi on every axis"


# ---- the response, header vs numpy, class by class ------------------------------------------------

def wedge_set():
    """six wedges: a floor ramp, a falling ramp along z, a corner cut by a plane with three components, an
    overhang (normal with a downward component), the 45 degree wedge and an axis-normal cut on dyadic numbers"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    return [O.Wedge.ramp((0.0, 0.0, 0.0), (2.0, 1.0, 1.5), 0, 1),
            O.Wedge.ramp((-1.0, 0.5, -2.0), (0.5, 1.25, 1.0), 2, 1, rising=False),
            O.Wedge((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (1.0, 1.0, 1.0), 0.3),
            O.Wedge((-1.0, -0.5, 0.0), (1.0, 0.5, 2.0), (0.6, -0.64, 0.48), 0.2),
            O.Wedge((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (-1.0, 1.0, 0.0), 0.0),
            O.Wedge((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.0, 1.0, 0.0), 0.5)]


def _geom(o):
    n = o.normal.astype(np.float64)
    return o.lo.astype(np.float64), o.hi.astype(np.float64), n, float(o.offset)


def _fill(rows, m):
    """m rows out of `rows` (tiled when there are fewer)"""
    assert rows.shape[0] > 0
    return rows[np.arange(m) % rows.shape[0]]


def _in_wedge(o, m, rng):
    lo, hi, n, d = _geom(o)
    x = lo + rng.random((6 * m, 3)) * (hi - lo)
    return _fill(x[x @ n < d - 1e-3], m)


def _on_cut_face(o, m, rng):
    lo, hi, n, d = _geom(o)
    x = lo + rng.random((8 * m, 3)) * (hi - lo)
    x = x - n * (x @ n - d)[:, None]
    keep = ((x > lo + 1e-3) & (x < hi - 1e-3)).all(1)
    return _fill(x[keep], m)


def _on_box_face(o, face, m, rng):
    """points of box face `face` (2a lo, 2a + 1 hi) that bound the solid (n.x < d); may be empty"""
    lo, hi, n, d = _geom(o)
    x = lo + rng.random((8 * m, 3)) * (hi - lo)
    x[:, face >> 1] = (hi if face & 1 else lo)[face >> 1]
    return x[x @ n < d - 1e-2]


def _speed(o, m, dt, rng):
    lo, hi, _, _ = _geom(o)
    return rng.uniform(0.05, 0.6, m) * float((hi - lo).min()) / float(dt)


def _aimed(o, target, inward, m, dt, rng, spread=0.7):
    """(P, V, Q): lines that reach `target` points at a time inside the step, along `inward` plus noise"""
    u = inward + spread * rng.normal(0.0, 1.0, (m, 3)) * 0.5
    u /= np.linalg.norm(u, axis=1)[:, None]
    V = u * _speed(o, m, dt, rng)[:, None]
    t_in = rng.uniform(0.05, 0.95, m) * float(dt)
    P = target - V * t_in[:, None]
    f = rng.choice([1.0, 1.0, 1.5, 4.0], m)
    Q = P + V * (float(dt) * f)[:, None]
    return P.astype(F32), V.astype(F32), Q.astype(F32)


def class_cut(o, m, dt, rng):
    _, _, n, _ = _geom(o)
    return _aimed(o, _on_cut_face(o, m, rng), -n, m, dt, rng)


def class_box(o, m, dt, rng):
    parts = []
    faces = [f for f in range(6) if _on_box_face(o, f, 64, rng).shape[0] > 0]
    k = -(-m // len(faces))
    for f in faces:
        inward = np.zeros(3)
        inward[f >> 1] = -1.0 if f & 1 else 1.0
        parts.append(_aimed(o, _fill(_on_box_face(o, f, k, rng), k), inward, k, dt, rng))
    return tuple(np.concatenate([p[i] for p in parts])[:m] for i in range(3))


def class_ties(o, m, dt, rng):
    """lines through the edges between the cut face and the box faces.  An axis-normal cut on dyadic numbers
    gives exact ties (p = e - v*t with few bits each); on the other wedges the line is aimed at the edge and
    rounding decides which side of the tie it falls on."""
    lo, hi, n, d = _geom(o)
    a = int(np.argmax(np.abs(n)))
    if abs(n[a]) == 1.0:
        t = 2.0 ** -9
        e = np.floor((lo + rng.random((m, 3)) * (hi - lo)) * 64.0) / 64.0
        e[:, a] = d
        b = (a + 1 + rng.integers(0, 2, m)) % 3                              # the box axis of the edge
        side = rng.random(m) < 0.5
        e[np.arange(m), b] = np.where(side, hi[b], lo[b])
        V = np.round(rng.uniform(-1.0, 1.0, (m, 3)) * 32.0) * 4.0
        V[:, a] = -np.sign(n[a]) * (np.abs(V[:, a]) + 4.0)
        V[np.arange(m), b] = np.where(side, -1.0, 1.0) * (np.abs(V[np.arange(m), b]) + 4.0)
        P = e - V * t
        Q = P + V * float(dt)
        return P.astype(F32), V.astype(F32), Q.astype(F32)
    # a point of the plane on a box face: move a face point along the in-face direction onto the plane
    x = lo + rng.random((8 * m, 3)) * (hi - lo)
    b = np.argsort(np.abs(n))[rng.integers(0, 2, 8 * m)]                      # a box axis other than the steepest
    side = rng.random(8 * m) < 0.5
    x[np.arange(8 * m), b] = np.where(side, hi[b], lo[b])
    x[:, a] += (d - x @ n) / n[a]
    keep = ((x >= lo) & (x <= hi)).all(1)
    x, b, side = _fill(x[keep], m), _fill(b[keep], m), _fill(side[keep], m)
    inward = -np.tile(n, (m, 1))
    inward[np.arange(m), b] += np.where(side, -1.0, 1.0)
    return _aimed(o, x, inward, m, dt, rng, spread=0.3)


def class_grazing(o, m, dt, rng):
    """p on the cut plane as nearly as fp32 gives it, v along the plane as nearly; q just below the face"""
    lo, hi, n, _ = _geom(o)
    c = _on_cut_face(o, m, rng)
    u = rng.normal(0.0, 1.0, (m, 3))
    u -= n * (u @ n)[:, None]
    u /= np.linalg.norm(u, axis=1)[:, None]
    V = u * _speed(o, m, dt, rng)[:, None] * 0.3
    Q = c + V * float(dt) - n * (rng.uniform(0.0, 1e-3, m) * float((hi - lo).min()))[:, None]
    return c.astype(F32), V.astype(F32), Q.astype(F32)


def class_g_zero(o, m, dt, rng):
    """n.v == 0 exactly: needs a normal whose fp32 components cancel (the 45 degree and axis-normal wedges)"""
    lo, hi, n, _ = _geom(o)
    V = (rng.normal(0.0, 1.0, (m, 3)) * _speed(o, m, dt, rng)[:, None]).astype(F32)
    nz = np.flatnonzero(n)
    if nz.size == 1:
        V[:, nz[0]] = 0.0
    else:
        assert nz.size == 2 and abs(n[nz[0]]) == abs(n[nz[1]])
        V[:, nz[1]] = V[:, nz[0]] * F32(-np.sign(n[nz[0]]) * np.sign(n[nz[1]]))
    Q = _in_wedge(o, m, rng).astype(F32)
    P = (Q - V * F32(dt) * rng.uniform(0.2, 3.0, (m, 1)).astype(F32)).astype(F32)
    return P, V, Q


def class_inside(o, m, dt, rng):
    """p inside: the fallback, q near each of the seven faces in turn"""
    lo, hi, n, d = _geom(o)
    ext = float((hi - lo).min())
    parts = []
    for f in range(7):
        k = -(-m // 7)
        if f == 6:
            s = _on_cut_face(o, k, rng)
            inward = -n
        else:
            pts = _on_box_face(o, f, k, rng)
            if pts.shape[0] == 0:
                continue
            s = _fill(pts, k)
            inward = np.zeros(3)
            inward[f >> 1] = -1.0 if f & 1 else 1.0
        parts.append(s + inward * (rng.uniform(1e-5, 2e-3, k) * ext)[:, None])
    Q = _fill(np.concatenate(parts), m)
    Q = Q[rng.permutation(m)]
    P = _in_wedge(o, m, rng)
    V = rng.normal(0.0, 1.0, (m, 3)) * _speed(o, m, dt, rng)[:, None]
    V[rng.random((m, 3)) < 0.1] = 0.0
    return P.astype(F32), V.astype(F32), Q.astype(F32)


def class_rest(o, m, dt, rng):
    lo, hi, _, _ = _geom(o)
    Q = _in_wedge(o, m, rng)
    P = np.where(rng.random((m, 1)) < 0.5, Q, lo - 0.5 * (hi - lo) + rng.random((m, 3)) * 2.0 * (hi - lo))
    return P.astype(F32), np.zeros((m, 3), F32), Q.astype(F32)


def class_dt_zero(o, m, dt, rng):
    k = m // 2
    a, b = class_cut(o, k, dt, rng), class_box(o, m - k, dt, rng)
    return tuple(np.concatenate([a[i], b[i]]) for i in range(3))


def _tie_count(o, P, V):
    """rows whose plane entry time equals the slabs' entry time exactly"""
    _, _, n, d, lo, hi = E.fields(o)
    with np.errstate(all="ignore"):
        t = np.full(P.shape[0], -np.inf, F32)
        for a in range(3):
            _, t0, _ = E._slab(P[:, a], V[:, a], lo[a], hi[a])
            t = np.where((V[:, a] != 0) & (t0 > t), t0, t)
        g = W.plane_dot(n, V)
        s = (-(W.plane_dot(n, P) - d)) / g
    return int(((g < 0) & (s == t)).sum())


CLASSES = {"cut": class_cut, "box": class_box, "ties": class_ties, "grazing": class_grazing, "g_zero": class_g_zero,
           "inside": class_inside, "rest": class_rest, "dt_zero": class_dt_zero}


@pytest.mark.parametrize("name", list(CLASSES))
def test_header_equals_numpy_bit_for_bit(policy, name):
    rng = np.random.default_rng(3000 + list(CLASSES).index(name))
    dt_gen, damping = F32(0.004), F32(0.6)
    dt = F32(0.0) if name == "dt_zero" else dt_gen
    wedges = wedge_set()
    if name == "g_zero":
        from smoothed_particle_hydrodynamics_amd import obstacles as O
        wedges = wedges[4:] + [O.Wedge((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.0, -1.0, 1.0), 0.0),
                               O.Wedge((0.0, 0.0, 0.0), (1.0, 2.0, 1.0), (1.0, 0.0, 1.0), 1.0),
                               O.Wedge((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (-1.0, 0.0, 0.0), -0.25),
                               O.Wedge((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.0, 0.0, 1.0), 0.75)]
    per = -(-PER_CLASS // len(wedges))
    total = 0
    cls_count = np.zeros(4, np.int64)
    faces = np.zeros(7, np.int64)
    entry_faces = np.zeros(7, np.int64)
    ties = g_zero = 0
    for o in wedges:
        P, V, Q = CLASSES[name](o, per, dt_gen, rng)
        hv, hq = header_respond(policy, [o], P, V, Q, dt, damping)
        ev, eq, cls, which = W.respond_one(o, P, V, Q, dt, damping, classify=True)
        assert same_bits(hv, ev) and same_bits(hq, eq), (name, o)
        untouched = ~W.inside(o, Q)
        assert (cls[untouched] == W.UNTOUCHED).all() and (cls[~untouched] != W.UNTOUCHED).all()
        assert same_bits(hv[untouched], V[untouched]) and same_bits(hq[untouched], Q[untouched])
        total += P.shape[0]
        cls_count += np.bincount(cls, minlength=4)
        faces += np.bincount(which[cls == W.FALLBACK], minlength=7)
        entry_faces += np.bincount(which[(cls == W.CUT_ENTRY) | (cls == W.BOX_ENTRY)], minlength=7)
        ties += _tie_count(o, P, V)
        with np.errstate(all="ignore"):
            g_zero += int(((W.plane_dot(E.fields(o)[2], V) == 0) & ~untouched & V.any(1)).sum())
    assert total >= PER_CLASS
    print(name, "rows", total, "untouched/cut/box/fallback", cls_count.tolist(), "fallback faces", faces.tolist(),
          "entry faces", entry_faces.tolist(), "exact ties", ties, "g == 0", g_zero)
    if name == "cut":
        assert cls_count[W.CUT_ENTRY] > 30000
    elif name == "box":
        assert cls_count[W.BOX_ENTRY] > 30000 and (entry_faces[:6] > 500).all()
    elif name == "ties":
        assert ties > 5000 and cls_count[W.CUT_ENTRY] > 5000 and cls_count[W.BOX_ENTRY] > 5000
    elif name == "grazing":
        assert cls_count[W.CUT_ENTRY] + cls_count[W.FALLBACK] > 30000 and faces[6] > 1000
    elif name == "g_zero":
        assert g_zero > 30000 and cls_count[W.BOX_ENTRY] > 1000 and cls_count[W.FALLBACK] > 1000
    elif name == "inside":
        assert cls_count[W.FALLBACK] > 60000 and (faces > 500).all(), faces
    elif name == "rest":
        assert cls_count[W.FALLBACK] == total and faces[6] > 1000
    else:
        assert cls_count[W.CUT_ENTRY] > 10000 and cls_count[W.BOX_ENTRY] > 10000


def test_chained_mixed_list_header_equals_numpy(policy):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(78)
    obst = [O.Sphere((0.0, 0.0, 0.0), 0.7), O.Wedge.ramp((-1.0, -1.0, -0.5), (1.2, 0.3, 0.5), 0, 1),
            O.Cylinder(1, (0.4, 0.0, 0.3), 0.5, -0.8, 0.8), O.Wedge((-0.5, -0.5, -1.0), (0.9, 1.0, 1.0), (0.6, -0.8, 0.0), 0.1),
            O.Box((-0.2, -1.0, -0.5), (1.2, 0.3, 0.5))]
    dt, damping = F32(0.004), F32(0.3)
    P, V, Q = cases(O.Box((-1.0, -1.0, -1.0), (1.2, 1.0, 1.0)), 60000, dt, rng)
    hv, hq = header_respond(policy, obst, P, V, Q, dt, damping)
    ev, eq = W.respond(obst, None, None, None, P, V, Q, dt, damping)
    assert same_bits(hv, ev) and same_bits(hq, eq)
    assert not same_bits(hq, Q)


def test_result_not_behind_the_cut_face_beyond_rounding(policy):
    """a single wedge leaves nobody deeper behind the cut face than the rounding of the last formula allows:
    inside the box's slabs n.q - d >= -2^-20 * (largest |coordinate| + |d|), ten times the five roundings of
    n.q - d"""
    rng = np.random.default_rng(6)
    dt, damping = F32(0.004), F32(0.6)
    for o in wedge_set():
        for gen in (class_cut, class_grazing, class_inside):
            P, V, Q = gen(o, 20000, dt, rng)
            _, hq, cls, which = W.respond_one(o, P, V, Q, dt, damping, classify=True)
            face = (which == 6) & np.isfinite(hq).all(1)
            assert face.sum() > 1000
            x = hq[face].astype(np.float64)
            depth = x @ o.normal.astype(np.float64) - float(o.offset)      # < 0: behind the cut face
            inbox = ((x > o.lo) & (x < o.hi)).all(1)
            tol = 2.0 ** -20 * (np.abs(x).max() + abs(float(o.offset)))
            assert (depth[inbox] >= -tol).all(), (o, float(depth[inbox].min()), tol)


# ---- anchors ---------------------------------------------------------------------------------------

def test_uncut_wedge_is_the_box(policy):
    """a plane that cuts nothing off: every output equals Box(lo, hi)'s"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(11)
    dt, damping = F32(0.004), F32(0.6)
    for normal in ((0.6, 0.8, 0.0), (-1.0, 2.0, -3.0), (0.0, 0.0, 1.0)):
        lo, hi = (-0.5, 0.25, 1.0), (0.75, 1.5, 1.75)
        box, wedge = O.Box(lo, hi), O.Wedge(lo, hi, normal, 100.0)
        P, V, Q = cases(box, 40000, dt, rng)
        bv, bq = header_respond(policy, [box], P, V, Q, dt, damping)
        wv, wq = header_respond(policy, [wedge], P, V, Q, dt, damping)
        assert same_bits(wv, bv) and same_bits(wq, bq)
        ev, eq = W.respond_one(wedge, P, V, Q, dt, damping)
        assert same_bits(ev, bv) and same_bits(eq, bq)
        assert int(E.inside(box, Q).sum()) > 5000


@pytest.mark.parametrize("a", [0, 1, 2])
def test_axis_normal_wedge_is_the_shorter_box(policy, a):
    """n = +e_a, d = c strictly inside the box: every output equals Box with hi[a] = c, by ==.
    The box stands where lo[a] >= c / 2 > 0, so that the plane fallback's q_a + (c - q_a) is exactly c
    (both operations are exact there).  The tie rule excludes exactly these rows, where the two solids pick
    different faces of equal merit: an entry with g < 0 whose plane time (c - p_a) / v_a equals the largest
    slab entry time and that slab's axis b is above a (the shorter box takes a, the lowest axis; the wedge
    takes the box face b); a fallback whose dpl = c - q_a equals the smallest box candidate and that
    candidate comes after hi[a] in the box's order (the shorter box takes hi[a], the wedge the other)."""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(20 + a)
    dt, damping = F32(0.004), F32(0.6)
    lo, hi = [1.0, 2.0, 0.75], [2.0, 3.5, 1.5]
    c = [1.5, 2.75, 1.25][a]
    n = [0.0, 0.0, 0.0]
    n[a] = 1.0
    short_hi = list(hi)
    short_hi[a] = c
    box, wedge = O.Box(lo, short_hi), O.Wedge(lo, hi, n, c)
    P, V, Q = cases(box, 60000, dt, rng)
    lo32, hi32 = F32(lo), F32(short_hi)
    with np.errstate(all="ignore"):
        t = np.full(P.shape[0], -np.inf, F32)
        ax = np.full(P.shape[0], -1)
        for b in range(3):
            if b == a:
                continue
            _, t0, _ = E._slab(P[:, b], V[:, b], lo32[b], hi32[b])
            take = (V[:, b] != 0) & (t0 > t)
            t, ax = np.where(take, t0, t), np.where(take, b, ax)
        s_pl = (F32(c) - P[:, a]) / V[:, a]
        entry_tie = (V[:, a] < 0) & (s_pl == t) & (ax > a)
        best = np.full(P.shape[0], np.inf, F32)
        later = np.zeros(P.shape[0], bool)
        for b in range(3):
            for k, cand in enumerate((Q[:, b] - lo32[b], hi32[b] - Q[:, b])):
                if b == a and k == 1:
                    continue
                take = cand < best
                best = np.where(take, cand, best)
                later = np.where(take, b > a, later)
        fallback_tie = (F32(c) - Q[:, a] == best) & later
    excluded = E.inside(box, Q) & (entry_tie | fallback_tie)
    keep = ~excluded
    print("axis", a, "rows", P.shape[0], "excluded by the tie rule", int(excluded.sum()))
    assert excluded.sum() < P.shape[0] // 20
    bv, bq = header_respond(policy, [box], P, V, Q, dt, damping)
    wv, wq = header_respond(policy, [wedge], P, V, Q, dt, damping)
    same = lambda x, y: np.array_equal(x[keep], y[keep], equal_nan=True)     # noqa: E731
    assert same(wv, bv) and same(wq, bq)
    assert int(E.inside(box, Q)[keep].sum()) > 8000 and np.array_equal(W.inside(wedge, Q), E.inside(box, Q))


def test_falling_onto_a_45_degree_face(policy):
    """A particle falling along -y onto the face y = x (n = (-s, s, 0), s = fl(sqrt(1/2))) leaves along -x with
    the speed it came with.  On dyadic inputs every operation but three is exact: s carries half an ulp
    (relative 2^-24.5, and the result has it twice, as s*s), and the product n_c * dot rounds once (2^-24);
    dot = v_y * s, the doubling and both subtractions are exact.  So each component is within
    (2 * 2^-24.5 + 2^-24) * |v| < 3 * 2^-24 * |v| of (-|v|, 0, 0); the inter point and the move are exact
    up to the same three roundings of the velocity times the time left."""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    wedge = O.Wedge((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (-1.0, 1.0, 0.0), 0.0)
    dt, damping = F32(2.0 ** -8), F32(0.5)
    for speed in (4.0, 64.0, 0.25):
        P = F32([[0.5, 0.5 + speed * 2.0 ** -10, 0.5]])                       # reaches the face at t = 2^-10
        V = F32([[0.0, -speed, 0.0]])
        Q = (P + V * dt).astype(F32)
        assert W.inside(wedge, Q).all() and not W.inside(wedge, P).any()
        hv, hq = header_respond(policy, [wedge], P, V, Q, dt, damping)
        ev, eq, cls, _ = W.respond_one(wedge, P, V, Q, dt, damping, classify=True)
        assert same_bits(hv, ev) and same_bits(hq, eq) and cls[0] == W.CUT_ENTRY
        bound = 3.0 * 2.0 ** -24 * speed
        assert abs(float(hv[0, 0]) + speed) <= bound and abs(float(hv[0, 1])) <= bound and hv[0, 2] == 0.0
        assert abs(math.hypot(float(hv[0, 0]), float(hv[0, 1])) - speed) <= 2.0 * bound
        left = (2.0 ** -8 - 2.0 ** -10) * 0.5
        want = np.array([0.5 - speed * left, 0.5, 0.5])
        assert np.abs(hq[0].astype(np.float64) - want).max() <= bound * left + 2.0 ** -24


# ---- shift, moved response, loads, bodies ---------------------------------------------------------

def test_shifted_wedge_rule_and_unchanged_old_rule(policy):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(31)
    old = [O.Sphere((1.0, -2.0, 3.0), 0.5), O.Box((0, 0, 0), (1, 2, 3)), O.Cylinder(2, (1.0, 1.0, 9.0), 0.3, 0.0, 1.0)]
    for o in old + wedge_set():
        for _ in range(50):
            D = (rng.normal(0.0, 1.0, 3) * rng.choice([1e-3, 1.0, 1e3])).astype(F32)
            D[rng.random(3) < 0.2] = 0.0
            src, out = o.as_struct(), O.SphObstacle()
            policy.shifted(C.byref(src), D.ctypes.data, C.byref(out))
            assert bytes(out) == bytes(W.shifted(o, D))
            if o.kind != O.WEDGE:
                assert bytes(out) == bytes(M.shifted(o, D))                  # the unused fields included
                assert list(out.center) == [float(x) for x in (F32(list(src.center)) + D)]
            else:
                n = F32(list(src.center))
                assert list(out.center) == list(src.center) and out.kind == 3
                assert out.radius == float(F32(src.radius) + F32(F32(F32(n[0] * D[0]) + F32(n[1] * D[1])) + F32(n[2] * D[2])))
                assert list(out.lo) == [float(x) for x in (F32(list(src.lo)) + D)]
    # a shift along the plane leaves the offset alone; one along the normal moves it by the length
    w = O.Wedge((0, 0, 0), (1, 1, 1), (0.0, 1.0, 0.0), 0.5)
    assert W.shifted(w, F32([3.0, 0.0, -2.0])).radius == 0.5 and W.shifted(w, F32([0.0, 0.25, 0.0])).radius == 0.75


def mixed_list():
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    return [O.Wedge.ramp((0.1, 0.0, -0.2), (0.9, 0.4, 1.4), 0, 1), O.Sphere((0.65, 0.7, 0.7), 0.2),
            O.Wedge((0.2, 0.6, 0.2), (0.7, 1.1, 0.9), (0.6, -0.8, 0.0), -0.45), O.Box((0.9, 0.2, 0.3), (1.2, 0.55, 0.9)),
            O.Wedge((0.0, 0.3, 0.9), (0.5, 0.6, 1.3), (0.0, 0.0, 1.0), 50.0), O.Cylinder(2, (0.3, 1.0, 0.0), 0.15, 0.2, 1.2)]


def mixed_cases(m, dt, rng):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    P, V, Q = cases(O.Box((0.0, 0.0, 0.0), (1.2, 1.1, 1.3)), m, dt, rng)
    V = (V * F32(0.1)).astype(F32)
    Q = (P + V * (F32(dt) * rng.choice([0.5, 1.0, 1.0, 2.0], m).astype(F32))[:, None]).astype(F32)
    k = m // 3
    Q[:k] = (rng.random((k, 3)) * F32([1.2, 1.1, 1.3])).astype(F32)
    return P, V, Q


def same_rows(row, impulse, count, skipped):
    return row.same(impulse, count, skipped)


@pytest.mark.parametrize("walls", [0, 1], ids=["no-walls", "walls"])
def test_moved_response_and_loads_on_mixed_lists(policy, walls):
    """the moved response and the loads, int64 for int64: wedges, a sphere, a box and a cylinder in one list,
    every second entry moving, at clocks before, during and after the motions"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(41 + walls)
    dt, damping = F32(0.004), F32(0.6)
    obst = mixed_list()
    motions = [O.Motion((8.0, 3.0, -2.0), 0.008, 0.02), None, O.Motion((0.0, -5.0, 4.0), 0.0, math.inf), None,
               O.Motion((0.0, 0.0, 6.0), 0.004, 0.012), O.Motion((-3.0, 0.0, 0.0), 0.0, 0.016)]
    maxv = F32([1.2, 1.1, 1.3])
    mass = rng.uniform(0.5, 2.0, 30000).astype(F32)
    moved_rows = 0
    for tau0 in (0.0, 0.004, 0.008, 0.016, 0.024):
        tau0 = F32(tau0)
        tau1 = F32(tau0 + dt)
        P, V, Q = mixed_cases(30000, dt, rng)
        for mot in (None, motions):
            hv, hq, imp, cnt, skp = header_full(policy, maxv, walls, obst, mot, None, None, P, V, Q, mass, dt, damping,
                                                tau0, tau1)
            ev, eq, row = W.integrate_respond(maxv, walls, obst, mot, None, None, P, V, Q, dt, damping, tau0, tau1, mass)
            assert same_bits_nan(hv, ev) and same_bits_nan(hq, eq), (walls, float(tau0), mot is not None)
            assert same_rows(row, imp, cnt, skp)
            assert (cnt[6:12] > 0).all(), cnt[:12]
            moved_rows += int(cnt[6:12].sum())
            if mot is not None:
                for i, (o, m_) in enumerate(zip(obst, mot)):                   # obstacle_at: the host's "now"
                    assert bytes(W.obstacle_at(o, m_, tau1)) == bytes(W.shifted(o, M.displacement(m_, tau1))
                                                                      if M.moves(m_) else o.as_struct())
    assert moved_rows > 20000


def test_wedge_body_on_a_mixed_list(policy):
    """a wedge that is a body, a box that is one, and entries that are not, over states that moved, rest and
    were stopped: particles and the row against the restatement"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(51)
    dt, damping = F32(0.004), F32(0.6)
    obst = mixed_list()
    bodies = [O.Body(40.0, free=(True, False, False)), None, O.Body(25.0, velocity=(0.0, 1.0, 0.0)), O.Body(30.0), None, None]
    maxv = F32([1.2, 1.1, 1.3])
    mass = rng.uniform(0.5, 2.0, 30000).astype(F32)
    st = B.State(bodies)
    turned = 0
    for k in range(4):
        st.Dprev = st.D.copy()
        if k < 3:                                                            # k == 3: at rest, D == Dprev
            for i, b in enumerate(bodies):
                if b is not None:
                    st.D[i] = (st.D[i] + F32(rng.normal(0.0, 0.01, 3)) * F32(b.free)).astype(F32)
        P, V, Q = mixed_cases(30000, dt, rng)
        hv, hq, imp, cnt, skp = header_full(policy, maxv, 1, obst, None, bodies, st, P, V, Q, mass, dt, damping, 0.0, dt)
        cl = W.Classes()
        ev, eq, row = W.integrate_respond(maxv, 1, obst, None, bodies, st, P, V, Q, dt, damping, F32(0.0), dt, mass,
                                          classes=cl)
        assert same_bits_nan(hv, ev) and same_bits_nan(hq, eq)
        assert same_rows(row, imp, cnt, skp)
        assert min(cl.counts()) > 0, cl.counts()
        turned += int(cnt[6] + cnt[8])
    assert turned > 4000


# ---- scene_hit_wedge -----------------------------------------------------------------------------

def c_hit(policy, o, eye, d):
    o = W._struct(o)
    d = np.ascontiguousarray(d, F32).reshape(-1, 3)
    k = d.shape[0]
    eye = np.asarray(eye, F32)
    eye = np.ascontiguousarray(np.broadcast_to(eye, (k, 3)) if eye.ndim == 1 else eye.reshape(k, 3))
    t, nrm, ok = np.zeros(k, F32), np.zeros((k, 3), F32), np.zeros(k, np.int32)
    policy.hit_many(C.byref(o), eye.ctypes.data, d.ctypes.data, k, t.ctypes.data, nrm.ctypes.data, ok.ctypes.data)
    return ok.astype(bool), t, nrm


def unit(d):
    d = np.asarray(d, np.float64).reshape(-1, 3)
    return (d / np.linalg.norm(d, axis=1)[:, None]).astype(F32)


def scene_cases(o, m, rng):
    """(eye (m, 3), d (m, 3)): seeded rays from outside and from inside the solid, rays parallel to the cut
    face, rays through the edges of the cut face, rays along the axes from eyes on the slab planes (NaN slabs)"""
    lo, hi, n, d = _geom(o)
    ext = hi - lo
    k = m // 5
    eye = lo - ext + rng.random((m, 3)) * 3.0 * ext
    target = lo + rng.random((m, 3)) * ext
    eye[:k] = _in_wedge(o, k, rng)                                           # the eye inside
    dirs = target - eye
    u = rng.normal(0.0, 1.0, (k, 3))                                         # parallel to the cut face
    dirs[k:2 * k] = u - n * (u @ n)[:, None]
    nz = np.flatnonzero(n)
    if nz.size <= 2:                                                         # exactly parallel where fp32 allows it
        v = rng.normal(0.0, 1.0, (k // 2, 3))
        if nz.size == 1:
            v[:, nz[0]] = 0.0
        elif abs(n[nz[0]]) == abs(n[nz[1]]):
            v[:, nz[1]] = -v[:, nz[0]] * np.sign(n[nz[0]]) * np.sign(n[nz[1]])
        dirs[k:k + k // 2] = v
    dirs[2 * k:3 * k] = _edge_points(o, k, rng) - eye[2 * k:3 * k]            # through the edges of the cut face
    ax = rng.integers(0, 3, k)                                               # NaN slabs: d_a == 0, eye_a on a plane
    s = slice(3 * k, 4 * k)
    e = np.zeros((k, 3))
    e[np.arange(k), (ax + 1) % 3] = rng.choice([-1.0, 1.0], k)
    dirs[s] = e + (rng.random((k, 1)) < 0.5) * np.eye(3)[(ax + 2) % 3] * rng.normal(0.0, 1.0, (k, 1))
    eye[s][np.arange(k), ax] = np.where(rng.random(k) < 0.5, lo[ax], hi[ax])
    dirs[np.linalg.norm(dirs, axis=1) == 0] = (1.0, 0.0, 0.0)
    return eye.astype(F32), unit(dirs)


def _edge_points(o, k, rng):
    lo, hi, n, d = _geom(o)
    a = int(np.argmax(np.abs(n)))
    x = lo + rng.random((8 * k, 3)) * (hi - lo)
    b = np.argsort(np.abs(n))[rng.integers(0, 2, 8 * k)]
    x[np.arange(8 * k), b] = np.where(rng.random(8 * k) < 0.5, hi[b], lo[b])
    x[:, a] += (d - x @ n) / n[a]
    keep = ((x >= lo) & (x <= hi)).all(1)
    return _fill(x[keep], k)


def ray_subclasses(o, eye, d):
    """masks over rays: a NaN product in some slab (which fminf / fmaxf then drop), g == 0, the plane's and the box's entries
    within 64 ulp of each other on a ray that enters through them, and those two exactly equal"""
    import scene_emulation as SC
    _, _, n, off, lo, hi = E.fields(o)
    with np.errstate(all="ignore"):
        sl = [SC.slab(eye[:, a], d[:, a], lo[a], hi[a]) for a in range(3)]
        nan_slab = ((d == 0) & ((eye == lo) | (eye == hi))).any(1)           # (lo_a - eye_a) * (1 / d_a) is 0 * inf
        b0 = np.fmax(np.fmax(sl[0][0], sl[1][0]), sl[2][0])
        b1 = np.fmin(np.fmin(sl[0][1], sl[1][1]), sl[2][1])
        g = W.plane_dot(n, d)
        f = (W.plane_dot(n, eye) - off).astype(F32)
        s = ((-f) / g).astype(F32)
        entering = (g < 0) & (b0 > 0) & (s > 0) & (np.fmax(b0, s) <= b1)
        on_edge = entering & (np.abs(s - b0) <= 64 * np.spacing(np.abs(b0)))
    return nan_slab, g == 0, on_edge, on_edge & (s == b0)


def boxn_of(nrm):
    """nrm where it is a box face's normal (one component +-1, the others 0), NaN elsewhere"""
    face = ((np.abs(nrm) == 1).sum(1) == 1) & ((nrm == 0).sum(1) == 2)
    return np.where(face[:, None], nrm, F32(np.nan)).astype(F32)


def test_scene_hit_wedge_bit_for_bit(policy):
    rng = np.random.default_rng(61)
    for o in wedge_set():
        eye, d = scene_cases(o, 50000, rng)
        ok, t, nrm = c_hit(policy, o, eye, d)
        eh, et, en = W.hit(o, eye, d)
        assert np.array_equal(ok, eh)
        assert same_bits(t[ok], et[ok]) and same_bits(nrm[ok], en[ok])
        inside = ok & (t == 0) & W.inside(o, eye)
        cut = ok & ~inside & (nrm == E.fields(o)[2]).all(1)
        print(o, "hits", int(ok.sum()), "eye inside", int(inside.sum()), "cut face", int(cut.sum()),
              "box faces", int((ok & ~inside & ~cut).sum()))
        assert inside.sum() > 5000 and cut.sum() > 2000 and (ok & ~inside & ~cut).sum() > 2000 and (~ok).sum() > 2000
        assert same_bits(nrm[inside], -d[inside])
        nan_slab, par, on_edge, tie = ray_subclasses(o, eye, d)
        k = eye.shape[0] // 5
        par = par[k:2 * k]                                                   # of the rays built parallel to the face
        print("   NaN slabs", int(nan_slab.sum()), "exactly parallel (g == 0)", int(par.sum()), "through an edge",
              int(on_edge.sum()), "of them exact ties", int(tie.sum()))
        # the k axis rays from an eye on a slab plane all form a NaN in that slab; of the k rays aimed (in
        # float64, then rounded) at an edge of the cut face, those that come from outside and meet the face from
        # its front have their two entries within rounding of each other, some exactly: there a box face wins;
        # a normal with at most two components, equal in size, has directions with g == 0 exactly
        assert nan_slab.sum() >= k and on_edge.sum() > 0 and tie.sum() > 0
        assert same_bits(nrm[tie & ok], boxn_of(nrm[tie & ok])) and (tie & ok).sum() > 0
        n_ = E.fields(o)[2]
        nz = np.flatnonzero(n_)
        if nz.size == 1 or (nz.size == 2 and abs(n_[nz[0]]) == abs(n_[nz[1]])):
            assert par.sum() >= k // 2
    # an uncut wedge is the box, a ray for a ray; exactly parallel rays above and below the face
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    import scene_emulation as SC
    box, uncut = O.Box((0, 0, 0), (1, 2, 3)), O.Wedge((0, 0, 0), (1, 2, 3), (0.6, 0.8, 0.0), 100.0)
    eye, d = scene_cases(O.Wedge((0, 0, 0), (1, 2, 3), (0.6, 0.8, 0.0), 1.0), 20000, rng)   # rays about the same box
    bo, bt, bn = SC.hit(box, eye, d)
    wo, wt, wn = c_hit(policy, uncut, eye, d)
    assert np.array_equal(bo, wo) and same_bits(bt[bo], wt[bo]) and same_bits(bn[bo], wn[bo])
    w = O.Wedge((0, 0, 0), (1, 1, 1), (0.0, 1.0, 0.0), 0.5)
    ok, t, nrm = c_hit(policy, w, F32([[-1, 0.25, 0.5], [-1, 0.5, 0.5], [-1, 0.75, 0.5]]), F32([[1, 0, 0]] * 3))
    assert ok.tolist() == [True, False, False] and t[0] == 1.0 and nrm[0].tolist() == [-1.0, 0.0, 0.0]


# ---- Python side ---------------------------------------------------------------------------------

def test_wedge_python_round_trips_and_distances():
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    w = O.Wedge((0, 0, 0), (2, 1, 3), (0.0, 3.0, 4.0), 2.0)
    assert w.normal.dtype == F32 and np.array_equal(w.normal, F32([0.0, 0.6, 0.8])) and w.offset == F32(2.0)
    n64 = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    assert np.array_equal(O.Wedge((0, 0, 0), (1, 1, 1), (1, 2, 3), 0.5).normal, n64.astype(F32))
    back = O.from_struct(w.as_struct())
    assert isinstance(back, O.Wedge) and bytes(back.as_struct()) == bytes(w.as_struct())
    assert bytes(O.from_struct(back.as_struct()).as_struct()) == bytes(w.as_struct())
    assert repr(w).startswith("Wedge(") and "0.6" in repr(w)
    arr, k = O.as_array([w, O.Box((0, 0, 0), (1, 1, 1)), w.as_struct()])
    assert k == 3 and arr[0].kind == 3 and arr[1].kind == 1 and bytes(arr[2]) == bytes(w.as_struct())
    with pytest.raises(ValueError):
        O.Wedge((0, 0, 0), (1, 1, 1), (0, 0, 0), 1.0)
    # signed distance: the max of the box's and the plane's, float64
    pts = [[1.0, 0.5, 0.5], [1.0, 0.5, 2.5], [1.0, 0.9, 2.9], [3.0, 0.5, 0.5], [1.0, 0.5, 1.0]]
    plane = np.array(pts) @ w.normal.astype(np.float64) - 2.0
    box = O.Box((0, 0, 0), (2, 1, 3)).signed_distance(pts)
    assert np.array_equal(w.signed_distance(pts), np.maximum(box, plane))
    assert (w.signed_distance(pts) < 0).tolist() == [True, False, False, False, True]
    assert O.inside_any(pts, [w]).tolist() == [True, False, False, False, True]
    assert O.inside_any(pts, [O.Sphere((3, 0.5, 0.5), 0.1), w]).tolist() == [True, False, False, True, True]
    rng = np.random.default_rng(3)
    x = rng.uniform(-0.5, 3.5, (20000, 3))
    near = np.abs(w.signed_distance(x)) < 1e-6
    assert np.array_equal(O.inside_any(x, [w])[~near], W.inside(w, x.astype(F32))[~near])


def test_wedge_ramp():
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    r = O.Wedge.ramp((1.0, 0.0, -1.0), (3.0, 1.0, 2.0), 0, 1)
    assert np.allclose(r.normal, np.array([-1.0, 2.0, 0.0]) / math.sqrt(5.0)) and r.normal[2] == 0
    for edge in ([1.0, 0.0, 0.3], [3.0, 1.0, 1.7], [2.0, 0.5, 0.0]):         # lower edge, upper edge, half way
        assert abs(float(np.dot(r.normal.astype(np.float64), edge)) - float(r.offset)) < 1e-6
    assert O.inside_any([[2.9, 0.5, 0.0], [1.1, 0.5, 0.0], [2.0, 0.49, 0.0], [2.0, 0.51, 0.0]], [r]).tolist() == \
        [True, False, True, False]
    f = O.Wedge.ramp((1.0, 0.0, -1.0), (3.0, 1.0, 2.0), 0, 1, rising=False)
    assert np.allclose(f.normal, np.array([1.0, 2.0, 0.0]) / math.sqrt(5.0))
    assert O.inside_any([[2.9, 0.5, 0.0], [1.1, 0.5, 0.0]], [f]).tolist() == [False, True]
    z = O.Wedge.ramp((0, 0, 0), (1, 1, 4), 2, 0)                              # run z, up x
    assert np.allclose(z.normal, np.array([4.0, 0.0, -1.0]) / math.sqrt(17.0)) and abs(float(z.offset)) < 1e-7
    for bad in ((0, 0), (3, 1), (0, -1)):
        with pytest.raises(ValueError):
            O.Wedge.ramp((0, 0, 0), (1, 1, 1), *bad)
    assert W.check(r) == "" and W.check(f) == "" and W.check(z) == ""


def test_carve_with_a_wedge():
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    from smoothed_particle_hydrodynamics_amd import scenes
    r = O.Wedge.ramp((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 0, 1)
    pos = F32([[0.9, 0.1, 0.5], [0.1, 0.9, 0.5], [0.5, 0.4, 0.5], [0.5, 0.6, 0.5], [1.5, 0.1, 0.5]]).reshape(-1)
    vel = np.arange(15, dtype=F32)
    mass = F32([1, 2, 3, 4, 5])
    p2, v2, m2 = scenes.carve(pos, vel, mass, [r])
    assert m2.tolist() == [2, 4, 5] and np.array_equal(v2, np.concatenate([vel[3:6], vel[9:15]]))
    assert np.array_equal(p2.reshape(-1, 3)[0], F32([0.1, 0.9, 0.5]))


@pytest.mark.parametrize("scene", ["beach", "weir"])
def test_scenes_step_on_the_cpu(oracle, scene):
    """dam_break_beach and channel_weir at 20 000 particles, 20 FULL steps with the oracle and the
    restatement: everything finite, carved, and some particle turned by a cut face"""
    from helpers import to_oracle_params
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    from smoothed_particle_hydrodynamics_amd import scenes
    if scene == "beach":
        p, pos, vel, mass, obst = scenes.dam_break_beach(20000)
        assert len(obst) == 1 and isinstance(obst[0], O.Wedge)
    else:
        p, pos, vel, mass, obst, emitters, sinks = scenes.channel_weir(20000)
        assert [o.kind for o in obst] == [O.WEDGE, O.BOX, O.WEDGE] and len(emitters) == 1 and len(sinks) == 1
        assert obst[0].hi[0] == obst[1].lo[0] and obst[1].hi[0] == obst[2].lo[0]
        assert obst[0].normal[0] < 0 < obst[0].normal[1] and obst[2].normal[0] > 0 and obst[2].normal[1] > 0
    assert p.apply_gravity == 1 and p.apply_walls == 1 and p.gravity[1] < 0
    assert 0 < mass.size <= 20000 and pos.size == 3 * mass.size == vel.size
    assert not O.inside_any(pos.reshape(-1, 3), obst).any()
    for o in obst:
        if o.kind == O.WEDGE:
            assert W.check(o) == "" and o.lo[1] == 0.0 and o.lo[2] < 0.0 and o.hi[2] > float(p.max_z)
    op = to_oracle_params(p)
    cl = W.Classes()
    for _ in range(20):
        pos, vel, _, _ = W.oracle_step(oracle, op, obst, None, None, None, None, pos, vel, mass, 0.0, 0.0, classes=cl)
    print(scene, "particles", mass.size, "cut / box / fallback", cl.counts(), "fallback faces", cl.fallback_faces.tolist())
    assert np.isfinite(pos).all() and np.isfinite(vel).all()
    assert cl.cut + int(cl.fallback_faces[6]) > 0


# ---- the new header code under the sanitizers, in a program of its own ----------------------------

MAIN = CALLS + r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
// hostile wedges and particles: fields that are huge, tiny, zero, NaN or infinite (obstacle_check's business
// is to refuse some of them; the response must still touch nothing it does not own), zero velocities, huge
// offsets, dt == 0, every function the wedge added a branch to
static unsigned long long state = 88172645463325252ull;
static unsigned next() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (unsigned)(state >> 32); }
static float pick()
{
   static const float odd[] = {0.0f, -0.0f, 1.0f, -1.0f, 0.5f, 1e-30f, -1e-30f, 1e30f, -1e30f, 3.4e38f, -3.4e38f,
                               INFINITY, -INFINITY, NAN, 0.70710678f, -0.70710678f};
   const unsigned r = next();
   if (r & 1) return odd[(r >> 1) % (sizeof(odd) / sizeof(odd[0]))];
   return ((int)(r >> 8) % 2001 - 1000) / 500.0f;
}
int main()
{
   long long checksum = 0;
   int refused = 0, accepted = 0;
   for (int k = 0; k < 20000; k++) {
      sph_hip_obstacle o;
      memset(&o, 0, sizeof(o));
      o.kind = SPH_HIP_OBSTACLE_WEDGE;
      o.axis = (int)next();
      const bool tame = k % 4 == 0;
      for (int c = 0; c < 3; c++) {
         o.center[c] = pick();
         o.lo[c] = tame ? -1.0f - (next() % 4) : pick();
         o.hi[c] = tame ? 1.0f + (next() % 4) : pick();
      }
      if (tame) {
         const float len = sqrtf(o.center[0] * o.center[0] + o.center[1] * o.center[1] + o.center[2] * o.center[2]);
         if (len > 0.0f && isfinite(len)) for (int c = 0; c < 3; c++) o.center[c] /= len;
      }
      o.radius = pick();
      if (obstacle_check(&o, 1)) refused++; else accepted++;
      float p[3 * 8], v[3 * 8], q[3 * 8], mass[8], D[3] = {pick(), pick(), pick()};
      for (int i = 0; i < 24; i++) {
         p[i] = pick();
         v[i] = (i / 3) % 3 == 0 ? 0.0f : pick();
         q[i] = (i / 3) % 2 ? p[i] : pick();
      }
      for (int i = 0; i < 8; i++) mass[i] = 1.0f;
      const float dt = k % 3 ? 0.004f : 0.0f;
      respond(&o, 1, 8, p, v, q, dt, 0.6f);
      sph_hip_obstacle s;
      shifted(&o, D, &s);
      respond(&s, 1, 8, p, v, q, dt, 0.6f);
      sph_hip_obstacle_motion m = {{pick(), pick(), pick()}, 0.0f, INFINITY};
      long long row[LOAD_ROW_WORDS];
      memset(row, 0, sizeof(row));
      const float maxv[3] = {4.0f, 4.0f, 4.0f};
      respond_full(maxv, k & 1, &o, &m, nullptr, nullptr, 1, 8, p, v, q, mass, dt, 0.6f, 0.004f, 0.008f, -24, row);
      sph_hip_body b = {5.0f, {0, 0, 0}, {0, 0, 0}, 7u, {-INFINITY, -INFINITY, -INFINITY}, {INFINITY, INFINITY, INFINITY}};
      BodyState st = body_initial(b);
      for (int c = 0; c < 3; c++) st.D[c] = D[c];
      respond_full(maxv, k & 1, &o, nullptr, &b, &st, 1, 8, p, v, q, mass, dt, 0.6f, 0.0f, 0.0f, -24, row);
      float t[8], nrm[24];
      int ok[8];
      hit_many(&o, p, v, 8, t, nrm, ok);
      for (int i = 0; i < 8; i++) checksum += ok[i];
      checksum += row[LOAD_ROW_COUNT + 6];
   }
   printf("accepted %d refused %d checksum %lld\n", accepted, refused, checksum);
   return accepted > 0 && refused > 0 ? 0 : 3;
}
"""


def test_new_header_code_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    src, exe = tmp_path / "wedge_main.cpp", tmp_path / "wedge_main"
    src.write_text(MAIN)
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == "", run.stderr
    assert run.stdout.split()[0] == "accepted"
