"""CPU checks of the static obstacles (include/sph_hip.h: sph_hip_set_obstacles): the struct layout and
constants, the argument checks and the per-particle response of csrc/obstacle_policy.h (compiled with
g++ behind an extern "C" shim) against the numpy restatement tests/obstacle_emulation.py bit for bit,
the anchor to the reference's wall response (oracle.boundary), the bound on what is left inside, the
integrate routes of csrc/launch_policy.h, and the Python side (obstacles.py, scenes.carve)."""
import ctypes as C

import numpy as np
import pytest

import obstacle_emulation as E
from helpers import compile_shim

F32 = np.float32

SHIM = r"""
#include <stddef.h>
#include "obstacle_policy.h"
#include "launch_policy.h"

extern "C" {
const char* check(const sph_hip_obstacle* list, int n)
{
   const char* why = obstacle_check(list, n);
   return why ? why : "";
}
void respond(const sph_hip_obstacle* list, int n, int m, const float* p, float* v, float* q, float dt,
             float damping)
{
   for (int i = 0; i < m; i++) obstacles_respond(list, n, p + 3 * i, v + 3 * i, q + 3 * i, dt, damping);
}
int fused_integrate(int hash_too, int tiled, int n, int no_fused, int n_obst)
{
   return fuse_integrate(hash_too != 0, tiled != 0, n, no_fused != 0, n_obst);
}
int fused_slab(int no_fused_slab, int n_obst) { return fuse_slab_step(no_fused_slab != 0, n_obst); }
#define OFF(f) (long long)offsetof(sph_hip_obstacle, f)
void layout(long long* out)
{
   out[0] = sizeof(sph_hip_obstacle);
   out[1] = OFF(kind); out[2] = OFF(axis); out[3] = OFF(center); out[4] = OFF(radius);
   out[5] = OFF(lo); out[6] = OFF(hi);
   out[7] = SPH_HIP_OBSTACLE_SPHERE; out[8] = SPH_HIP_OBSTACLE_BOX; out[9] = SPH_HIP_OBSTACLE_CYLINDER;
   out[10] = SPH_HIP_MAX_OBSTACLES; out[11] = SPH_HIP_ABI_VERSION;
}
}
"""


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    from smoothed_particle_hydrodynamics_amd.obstacles import SphObstacle
    lib = compile_shim(SHIM, ["-O2", "-ffp-contract=off"], tmp_path_factory)
    lib.check.argtypes = [C.POINTER(SphObstacle), C.c_int]
    lib.check.restype = C.c_char_p
    lib.respond.argtypes = [C.POINTER(SphObstacle), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                            C.c_float, C.c_float]
    lib.layout.argtypes = [C.POINTER(C.c_longlong)]
    return lib


def header_respond(lib, obstacles, P, V, Q, dt, damping):
    from smoothed_particle_hydrodynamics_amd.obstacles import as_array
    arr, n = as_array(obstacles)
    p = np.ascontiguousarray(P, F32).reshape(-1, 3)
    v = np.ascontiguousarray(V, F32).reshape(-1, 3).copy()
    q = np.ascontiguousarray(Q, F32).reshape(-1, 3).copy()
    lib.respond(arr, n, p.shape[0], p.ctypes.data, v.ctypes.data, q.ctypes.data, dt, damping)
    return v, q


def same_bits(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


# ---- layout, constants, refusals ---------------------------------------------------------------

def test_struct_layout_and_constants(policy):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    out = (C.c_longlong * 12)()
    policy.layout(out)
    S = O.SphObstacle
    assert list(out) == [48, S.kind.offset, S.axis.offset, S.center.offset, S.radius.offset, S.lo.offset,
                         S.hi.offset, O.SPHERE, O.BOX, O.CYLINDER, O.MAX_OBSTACLES, 7]
    assert C.sizeof(S) == 48 and [S.kind.offset, S.axis.offset, S.center.offset, S.radius.offset,
                                  S.lo.offset, S.hi.offset] == [0, 4, 8, 20, 24, 36]


def test_refusals(policy):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    ok = [O.Sphere((1, 1, 1), 0.5), O.Box((0, 0, 0), (1, 2, 3)), O.Cylinder(2, (1, 1, 0), 0.3, 0.0, 1.0)]
    arr, n = O.as_array(ok)
    assert policy.check(arr, n) == b""
    assert policy.check(None, 0) == b""
    assert policy.check(arr, -1) != b""
    assert policy.check(None, 1) != b""
    big = (O.SphObstacle * 65)()
    for i in range(65):
        big[i] = ok[0].as_struct()
    assert policy.check(big, 64) == b""
    assert policy.check(big, 65) != b""

    def refused(mutate, base=0):
        s = ok[base].as_struct()
        mutate(s)
        a, k = O.as_array([s])
        return policy.check(a, k) != b""

    assert refused(lambda s: setattr(s, "kind", 3))
    assert refused(lambda s: setattr(s, "kind", -1))
    assert refused(lambda s: setattr(s, "radius", 0.0))
    assert refused(lambda s: setattr(s, "radius", -1.0))
    assert refused(lambda s: setattr(s, "radius", 0.0), 2)
    for bad in (np.nan, np.inf, -np.inf):
        for base in range(3):
            assert refused(lambda s: s.center.__setitem__(1, bad), base)
            assert refused(lambda s: s.lo.__setitem__(0, bad), base)      # unused fields included
            assert refused(lambda s: setattr(s, "radius", bad), base)
    assert refused(lambda s: s.lo.__setitem__(1, 2.0), 1)                # lo == hi
    assert refused(lambda s: s.lo.__setitem__(2, 4.0), 1)                # lo > hi
    assert refused(lambda s: s.hi.__setitem__(2, 0.0), 2)                # on the cylinder's axis
    assert not refused(lambda s: s.hi.__setitem__(0, -5.0), 2)           # not on its axis: unused
    assert refused(lambda s: setattr(s, "axis", 3), 2)
    assert refused(lambda s: setattr(s, "axis", -1), 2)
    assert not refused(lambda s: setattr(s, "axis", 7), 0)               # a sphere has no axis


# ---- the response, header vs numpy ---------------------------------------------------------------

def _obstacle_set(kind, rng):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    out = []
    for _ in range(4):
        c = rng.uniform(-2.0, 2.0, 3).astype(F32)
        if kind == E.SPHERE:
            out.append(O.Sphere(c, F32(rng.uniform(0.2, 1.0))))
        elif kind == E.BOX:
            half = rng.uniform(0.2, 1.0, 3).astype(F32)
            out.append(O.Box(c - half, c + half))
        else:
            a = int(rng.integers(0, 3))
            h = F32(rng.uniform(0.2, 1.0))
            out.append(O.Cylinder(a, c, F32(rng.uniform(0.2, 1.0)), c[a] - h, c[a] + h))
    return out


def _extent(o):
    """(lo, hi) of the obstacle's bounding box, float32"""
    _, axis, c, r, lo, hi = E.fields(o)
    if o.kind == E.SPHERE:
        return c - r, c + r
    if o.kind == E.BOX:
        return lo, hi
    blo, bhi = c - r, c + r
    blo[axis], bhi[axis] = lo[axis], hi[axis]
    return blo, bhi


def cases(o, m, dt, rng):
    """m seeded (p, v, q) around obstacle o: p outside and inside, lines through faces, edges and
    corners, grazing lines, zero velocity components, q on the surface, entries beyond dt"""
    lo, hi = _extent(o)
    ext = hi - lo
    mid = (lo + hi) * F32(0.5)
    P = (lo - ext + rng.random((m, 3)) * 3 * ext).astype(F32)
    V = rng.normal(0.0, 1.0, (m, 3)).astype(F32) * F32(rng.choice([10.0, 300.0, 3000.0]))
    V[rng.random((m, 3)) < 0.15] = 0.0                                       # zero components
    V[rng.random(m) < 0.02] = 0.0                                            # at rest
    k = m // 8
    # corners and edges: p beyond a corner along the diagonal, v straight at it (ties between axes)
    sgn = rng.choice([-1.0, 1.0], (k, 3)).astype(F32)
    corner = np.where(sgn > 0, hi, lo).astype(F32)
    off = F32(rng.uniform(0.01, 0.3)) * ext
    P[:k] = corner + sgn * off
    V[:k] = -sgn * off * F32(1.0 / dt) * F32(rng.uniform(0.5, 3.0))
    edge = rng.random(k) < 0.5
    ax = rng.integers(0, 3, k)
    P[:k][edge, ax[edge]] = mid[ax[edge]]
    V[:k][edge, ax[edge]] = 0.0
    # grazing: p on a face plane, v parallel to it
    g = slice(k, 2 * k)
    ax = rng.integers(0, 3, k)
    side = rng.random(k) < 0.5
    P[g][np.arange(k), ax] = np.where(side, lo[ax], hi[ax])
    V[g][np.arange(k), ax] = 0.0
    # q: mostly the drift p + v*dt*f (f > 1: entries beyond dt), then anywhere inside the box (lines
    # that miss), then snapped onto the surface
    f = rng.choice([0.3, 1.0, 1.0, 2.0, 5.0], m).astype(F32)
    Q = (P + V * (F32(dt) * f)[:, None]).astype(F32)
    r2 = slice(2 * k, 3 * k)
    Q[r2] = (lo + rng.random((k, 3)) * ext).astype(F32)
    s = slice(3 * k, 4 * k)
    ax = rng.integers(0, 3, k)
    side = rng.random(k) < 0.5
    Q[s][np.arange(k), ax] = np.where(side, lo[ax], hi[ax])
    if o.kind == E.SPHERE:
        _, _, c, r, _, _ = E.fields(o)
        d = rng.normal(0.0, 1.0, (k, 3))
        Q[s] = (c + (d / np.linalg.norm(d, axis=1)[:, None]) * r).astype(F32)
    # p exactly inside for some, q exactly p for a few
    P[4 * k:4 * k + k // 4] = (lo + rng.random((k // 4, 3)) * ext).astype(F32)
    Q[4 * k + k // 4:4 * k + k // 2] = P[4 * k + k // 4:4 * k + k // 2]
    return P, V, Q


@pytest.mark.parametrize("kind", [E.SPHERE, E.BOX, E.CYLINDER], ids=["sphere", "box", "cylinder"])
def test_header_equals_numpy_bit_for_bit(policy, kind):
    rng = np.random.default_rng(1000 + kind)
    dt, damping = F32(0.004), F32(0.6)
    total = active = hits = 0
    for o in _obstacle_set(kind, rng):
        P, V, Q = cases(o, 25000, dt, rng)
        hv, hq = header_respond(policy, [o], P, V, Q, dt, damping)
        ev, eq = E.respond_one(o, P, V, Q, dt, damping)
        assert same_bits(hv, ev) and same_bits(hq, eq)
        moved = E.inside(o, Q)
        untouched = ~moved
        assert same_bits(hv[untouched], V[untouched]) and same_bits(hq[untouched], Q[untouched])
        total += P.shape[0]
        active += int(moved.sum())
        hits += int((moved & ~E.inside(o, P)).sum())
    assert total >= 100000
    assert active > 5000 and hits > 2000, (active, hits)


def test_chained_list_header_equals_numpy(policy):
    """one obstacle of each kind, overlapping, applied in list order"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    rng = np.random.default_rng(77)
    obst = [O.Sphere((0.0, 0.0, 0.0), 0.7), O.Box((-0.2, -1.0, -0.5), (1.2, 0.3, 0.5)),
            O.Cylinder(1, (0.4, 0.0, 0.3), 0.5, -0.8, 0.8)]
    dt, damping = F32(0.004), F32(0.3)
    P, V, Q = cases(O.Box((-1.0, -1.0, -1.0), (1.2, 1.0, 1.0)), 60000, dt, rng)
    hv, hq = header_respond(policy, obst, P, V, Q, dt, damping)
    ev, eq = E.respond(obst, P, V, Q, dt, damping)
    assert same_bits(hv, ev) and same_bits(hq, eq)
    assert not same_bits(hq, Q)


def test_result_not_inside_beyond_rounding(policy):
    """a single obstacle leaves no particle strictly inside by more than 4 ulp of the obstacle's
    coordinates (the last rounding of a surface point or of the reflected move)"""
    rng = np.random.default_rng(5)
    dt, damping = F32(0.004), F32(0.6)
    for kind in (E.SPHERE, E.BOX, E.CYLINDER):
        for o in _obstacle_set(kind, rng):
            P, V, Q = cases(o, 20000, dt, rng)
            _, hq = header_respond(policy, [o], P, V, Q, dt, damping)
            lo, hi = _extent(o)
            scale = float(np.abs(np.concatenate([lo, hi])).max())
            tol = 4.0 * scale * 2.0 ** -23
            d = o.signed_distance(hq)
            ok = np.isfinite(hq).all(1)
            assert (d[ok] >= -tol).all(), (o, float(d[ok].min()), tol)


# ---- the anchor to the reference's wall ---------------------------------------------------------

@pytest.mark.parametrize("axis", [0, 1, 2])
def test_half_space_box_is_the_reference_wall(policy, oracle, axis):
    """A box that covers the half-space beyond the wall max_{x,y,z} gives what the reference's own
    wall response (oracle.boundary) gives to the crossing cases of test_boundary_gravity that cross
    that wall alone with t <= dt, bit for bit."""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    from test_boundary_gravity import crossing_cases
    p = oracle.params_for_h(0.1)
    p.damping = 0.5
    pos, vel, dt, newpos = crossing_cases(p)
    P, V, Q = (a.reshape(-1, 3) for a in (pos, vel, newpos))
    L = np.float32([p.max_x, p.max_y, p.max_z])
    others = [a for a in range(3) if a != axis]
    with np.errstate(all="ignore"):
        t = (L[axis] - P[:, axis]) / V[:, axis]
    sel = (Q[:, axis] > L[axis]) & (t <= F32(dt))
    for a in others:
        sel &= (Q[:, a] >= 0) & (Q[:, a] <= L[a])
    assert sel.sum() > 100
    lo = [-1e30] * 3
    hi = [1e30] * 3
    lo[axis] = float(L[axis])
    box = O.Box(lo, hi)
    ov, oq = oracle.boundary(p, P[sel].reshape(-1), V[sel].reshape(-1), dt, Q[sel].reshape(-1))
    hv, hq = header_respond(policy, [box], P[sel], V[sel], Q[sel], F32(dt), F32(p.damping))
    assert same_bits(hv, ov.reshape(-1, 3)) and same_bits(hq, oq.reshape(-1, 3))
    ev, eq = E.respond_one(box, P[sel], V[sel], Q[sel], F32(dt), F32(p.damping))
    assert same_bits(ev, hv) and same_bits(eq, hq)


# ---- routes -------------------------------------------------------------------------------------

def test_routes_unfused_exactly_with_obstacles(policy):
    for hash_too in (0, 1):
        for tiled in (0, 1):
            for n in (0, 5):
                for no_fused in (0, 1):
                    for n_obst in (0, 1, 64):
                        want = bool(hash_too and tiled and n > 0 and not no_fused and n_obst == 0)
                        assert bool(policy.fused_integrate(hash_too, tiled, n, no_fused, n_obst)) == want
    for no_fused_slab in (0, 1):
        for n_obst in (0, 1, 8, 64):
            assert bool(policy.fused_slab(no_fused_slab, n_obst)) == (not no_fused_slab and n_obst == 0)


# ---- Python side --------------------------------------------------------------------------------

def test_signed_distance_and_structs():
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    s = O.Sphere((1.0, 2.0, 3.0), 0.5)
    assert np.allclose(s.signed_distance([[1.0, 2.0, 3.0], [2.0, 2.0, 3.0]]), [-0.5, 0.5])
    b = O.Box((0, 0, 0), (1, 2, 3))
    assert np.allclose(b.signed_distance([[0.5, 1.0, 1.5], [2.0, 1.0, 1.5], [2.0, 3.0, 1.5]]),
                       [-0.5, 1.0, np.sqrt(2.0)])
    c = O.Cylinder(2, (1.0, 1.0, 99.0), 0.5, 0.0, 2.0)
    assert np.allclose(c.signed_distance([[1.0, 1.0, 1.0], [2.0, 1.0, 1.0], [1.0, 1.0, 3.0], [1.0, 1.2, 1.9]]),
                       [-0.5, 0.5, 1.0, -0.1])
    for o in (s, b, c):
        back = O.from_struct(o.as_struct())
        assert bytes(back.as_struct()) == bytes(o.as_struct())
    st = c.as_struct()
    assert st.kind == O.CYLINDER and st.axis == 2 and st.lo[2] == 0.0 and st.hi[2] == 2.0


def test_carve_and_pillar_scene():
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    from smoothed_particle_hydrodynamics_amd import scenes
    pos = np.float32([[0.1, 0.1, 0.1], [1.0, 1.0, 1.0], [0.5, 0.5, 0.5], [1.7, 1.0, 1.0]]).reshape(-1)
    vel = np.arange(12, dtype=np.float32)
    mass = np.float32([1, 2, 3, 4])
    p2, v2, m2 = scenes.carve(pos, vel, mass, [O.Sphere((1.0, 1.0, 1.0), 0.6)])
    assert np.array_equal(m2, [1, 3, 4])
    assert np.array_equal(v2, np.concatenate([vel[0:3], vel[6:12]]))
    assert np.array_equal(p2.reshape(-1, 3)[1], [0.5, 0.5, 0.5])


def test_pillar_scene_needs_no_gpu_to_plan():
    pytest.importorskip("smoothed_particle_hydrodynamics_amd.lib")
    from smoothed_particle_hydrodynamics_amd import scenes
    try:
        p, pos, vel, mass, obst = scenes.dam_break_pillar(20000)
    except Exception as exc:     # default_params needs the built library, not a GPU
        pytest.skip("library not built: %s" % exc)
    assert p.apply_gravity == 1 and p.apply_walls == 1 and p.gravity[1] < 0
    assert len(obst) == 1 and obst[0].axis == 1
    assert not (obst[0].signed_distance(pos.reshape(-1, 3)) < 0).any()
    assert pos.size == 3 * mass.size == vel.size
