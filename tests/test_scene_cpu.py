"""CPU checks of the scene renderer (include/sph_hip.h: sph_hip_render_scene): the C ABI and its binding,
the refusals of csrc/scene_policy.h, its ray-solid functions (compiled with g++ behind an extern "C" shim,
as tests/test_render_cpu.py does) bit for bit against the numpy restatement tests/scene_emulation.py on
seeded rays and directed cases, their accuracy against the same geometry in float64, the composite on top
of render_emulation.Frame, and one run of the directed cases under the address and undefined-behaviour
sanitizers in a stand-alone host program."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import render_emulation as E
import scene_emulation as SC
from helpers import compile_shim
from test_render_cpu import good
from test_sample_cpu import header_prototype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smoothed_particle_hydrodynamics_amd", "csrc")
F32 = np.float32
PER_KIND = 200000

# what both the shim and the sanitizer program call
CALLS = r"""
#include <stddef.h>
#include "scene_policy.h"

extern "C" {
// eyes and directions one per ray; ok[i] = hit
void hit_many(const sph_hip_obstacle* o, const float* eye, const float* d, int n, float* t, float* nrm, int* ok)
{
   for (int i = 0; i < n; i++) {
      float ti = 0.0f, ni[3] = {0.0f, 0.0f, 0.0f};
      ok[i] = scene_hit(*o, eye + 3 * i, d + 3 * i, ti, ni) ? 1 : 0;
      t[i] = ok[i] ? ti : 0.0f;
      for (int c = 0; c < 3; c++) nrm[3 * i + c] = ok[i] ? ni[c] : 0.0f;
   }
}
void nearest_many(const sph_hip_obstacle* list, int count, const float* eye, const float* d, int n, float* t,
                  float* nrm, int* id)
{
   for (int i = 0; i < n; i++) {
      float ni[3] = {0.0f, 0.0f, 0.0f};
      const bool any = scene_nearest(list, count, eye + 3 * i, d + 3 * i, t[i], ni, id[i]);
      for (int c = 0; c < 3; c++) nrm[3 * i + c] = any ? ni[c] : 0.0f;
   }
}
}
"""

SHIM = CALLS + r"""
extern "C" {
const char* check(const sph_hip_camera* cam, const sph_hip_render_params* rp, const sph_hip_scene_params* sp,
                  const float* albedo, int n_albedo, int n_obstacles, int w, int h, int flags)
{
   const char* why = scene_check(cam, rp, sp, albedo, n_albedo, n_obstacles, w, h, flags);
   return why ? why : "";
}
void layout(long long* out)
{
   out[0] = sizeof(sph_hip_scene_params);
   out[1] = offsetof(sph_hip_scene_params, albedo);
   out[2] = offsetof(sph_hip_scene_params, ambient);
   out[3] = offsetof(sph_hip_scene_params, diffuse);
   out[4] = sizeof(SceneSolid);
   out[5] = offsetof(SceneSolid, vel);
   out[6] = offsetof(SceneSolid, alb);
}
int pixel_dirs(const sph_hip_camera* cam, int w, int h, float* d, int* ok)
{
   for (int py = 0; py < h; py++)
      for (int px = 0; px < w; px++) {
         float di[3] = {0.0f, 0.0f, 0.0f};
         const int i = py * w + px;
         ok[i] = scene_pixel_dir(*cam, w, h, px, py, di) ? 1 : 0;
         for (int c = 0; c < 3; c++) d[3 * i + c] = di[c];
      }
   return 0;
}
unsigned shade(const float* n, const float* light, const float* albedo, float ambient, float diffuse)
{
   return scene_shade(n, light, albedo, ambient, diffuse);
}
int in_front(float t_solid, float depth_fluid) { return scene_in_front(t_solid, depth_fluid) ? 1 : 0; }
void motion_velocity(const sph_hip_obstacle_motion* m, float tau, float* v) { scene_motion_velocity(*m, tau, v); }
long long id_bytes(int w, int rows) { return scene_id_bytes(w, rows); }
long long pixel_bytes() { return RENDER_PIXEL_BYTES; }
}
"""


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    from smoothed_particle_hydrodynamics_amd.lib import SphCamera
    lib = compile_shim(SHIM, ["-O2", "-ffp-contract=off"], tmp_path_factory)
    lib.check.restype = C.c_char_p
    lib.layout.argtypes = [C.POINTER(C.c_longlong)]
    lib.pixel_dirs.argtypes = [C.POINTER(SphCamera), C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.shade.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float]
    lib.shade.restype = C.c_uint
    lib.in_front.argtypes = [C.c_float, C.c_float]
    lib.motion_velocity.argtypes = [C.c_void_p, C.c_float, C.c_void_p]
    lib.id_bytes.restype = C.c_longlong
    lib.pixel_bytes.restype = C.c_longlong
    return lib


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def c_hit(policy, o, eye, d):
    o = SC._struct(o)
    d = np.ascontiguousarray(d, F32).reshape(-1, 3)
    n = d.shape[0]
    eye = np.ascontiguousarray(np.broadcast_to(np.asarray(eye, F32), (n, 3)))
    t, nrm, ok = np.zeros(n, F32), np.zeros((n, 3), F32), np.zeros(n, np.int32)
    policy.hit_many(C.byref(o), ptr(eye), ptr(d), n, ptr(t), ptr(nrm), ptr(ok))
    return ok.astype(bool), t, nrm


def c_nearest(policy, solids, eye, d):
    from smoothed_particle_hydrodynamics_amd.obstacles import as_array
    arr, k = as_array([SC._struct(o) for o in solids])
    d = np.ascontiguousarray(d, F32).reshape(-1, 3)
    n = d.shape[0]
    eye = np.ascontiguousarray(np.broadcast_to(np.asarray(eye, F32), (n, 3)))
    t, nrm, sid = np.zeros(n, F32), np.zeros((n, 3), F32), np.zeros(n, np.int32)
    policy.nearest_many(arr, k, ptr(eye), ptr(d), n, ptr(t), ptr(nrm), ptr(sid))
    return t, nrm, sid


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def assert_hits_equal(got, want, what):
    """(hit, t, normal) bit for bit; t and normal where hit"""
    gh, gt, gn = got
    wh, wt, wn = want
    assert (gh == wh).all(), "%s: hit/miss differs on %d rays, first %d" % (what, (gh != wh).sum(),
                                                                         np.flatnonzero(gh != wh)[0])
    bad = np.flatnonzero(gh & ((bits(gt) != bits(wt)) | (bits(gn) != bits(wn)).any(1)))
    assert bad.size == 0, "%s: %d rays differ, first %d: t %r vs %r, normal %r vs %r" % (
        what, bad.size, bad[0], gt[bad[0]], wt[bad[0]], gn[bad[0]], wn[bad[0]])


def unit(v):
    """directions normalised as the renderer normalises a pixel's: fp32, unfused"""
    v = np.ascontiguousarray(v, F32).reshape(-1, 3)
    ln = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    return (v / ln[:, None]).astype(F32)


# ---- C ABI ---------------------------------------------------------------------------------------------
def test_scene_symbol_is_exported(hiplib):
    assert hasattr(hiplib, "sph_hip_render_scene")


def test_scene_prototype_matches_the_header():
    from smoothed_particle_hydrodynamics_amd.lib import PROTOTYPES, SphCamera, SphRenderParams, SphSceneParams
    assert header_prototype("sph_hip_render_scene") == [
        "sph_hip_context* ctx", "const sph_hip_camera* cam", "const sph_hip_render_params* rp",
        "const sph_hip_scene_params* sp", "const float* solid_albedo_rgb", "int n_albedo", "int width", "int height",
        "int flags", "uint8_t* rgba", "float* depth", "float* normal_xyz", "float* velocity_xyz",
        "int32_t* first_inside", "int32_t* solid_id"]
    res, args = PROTOTYPES["sph_hip_render_scene"]
    assert res is C.c_int and len(args) == 15 and args[0] is C.c_void_p
    assert args[1]._type_ is SphCamera and args[2]._type_ is SphRenderParams and args[3]._type_ is SphSceneParams
    assert args[4] is C.c_void_p and args[5:9] == [C.c_int] * 4 and args[9:] == [C.c_void_p] * 6


def test_scene_params_match_the_c_layout(policy):
    from smoothed_particle_hydrodynamics_amd.lib import SphSceneParams
    out = (C.c_longlong * 7)()
    policy.layout(out)
    assert list(out)[:4] == [20, 0, 12, 16]
    assert [C.sizeof(SphSceneParams)] + [getattr(SphSceneParams, f).offset for f in ("albedo", "ambient", "diffuse")] \
        == [20, 0, 12, 16]
    assert list(out)[4:] == [72, 48, 60]            # the device's list entry: obstacle, velocity, albedo


def test_abi_version_and_note():
    from smoothed_particle_hydrodynamics_amd.lib import ABI_VERSION
    text = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    assert "#define SPH_HIP_ABI_VERSION 7" in text and ABI_VERSION == 7
    block = text[text.index("---- scene renderer"):text.index("int sph_hip_render_scene(")]
    assert "added without a change of SPH_HIP_ABI_VERSION" in block


def test_scratch_of_the_pass(policy):
    assert policy.pixel_bytes() == 40               # the renderer's own scratch is untouched
    for w, rows in ((1, 1), (13, 7), (1280, 720), (16384, 96)):
        b = policy.id_bytes(w, rows)
        assert b % 256 == 0 and 4 * w * rows <= b < 4 * w * rows + 256


def test_render_result_gains_solid_id():
    from smoothed_particle_hydrodynamics_amd import RenderResult
    assert RenderResult._fields == ("rgba", "depth", "normal", "velocity", "first_inside", "solid_id")
    assert RenderResult(1, 2, 3, 4, 5).solid_id is None


# ---- refusals ------------------------------------------------------------------------------------------------
def scene_params(albedo=(0.7, 0.7, 0.7), ambient=0.2, diffuse=0.8):
    from smoothed_particle_hydrodynamics_amd.lib import SphSceneParams
    sp = SphSceneParams()
    sp.albedo[:] = list(albedo)
    sp.ambient, sp.diffuse = ambient, diffuse
    return sp


def test_scene_check_refusals(policy):
    cam, rp = good()
    sp = scene_params()
    alb = np.full((3, 3), 0.5, F32)

    def check(cam_=cam, rp_=rp, sp_=sp, alb_=None, n_alb=0, n_obst=3, w=64, h=48, flags=0):
        return policy.check(C.byref(cam_) if cam_ is not None else None, C.byref(rp_) if rp_ is not None else None,
                            C.byref(sp_) if sp_ is not None else None, None if alb_ is None else ptr(alb_), n_alb,
                            n_obst, w, h, flags)

    assert check() == b"" and check(alb_=alb, n_alb=3) == b"" and check(flags=1) == b"" and check(n_obst=0) == b""
    assert check(sp_=None) == b"null scene params"
    for bad in (np.nan, np.inf, -np.inf):
        for c in range(3):
            s = scene_params()
            s.albedo[c] = bad
            assert check(sp_=s) == b"scene params must be finite"
        assert check(sp_=scene_params(ambient=bad)) == b"scene params must be finite"
        assert check(sp_=scene_params(diffuse=bad)) == b"scene params must be finite"
        a = alb.copy()
        a[2, 1] = bad
        assert check(alb_=a, n_alb=3) == b"a solid's albedo must be finite"
    for n_alb in (1, 2, 4, 64, -1):
        assert check(alb_=alb, n_alb=n_alb) == b"the albedo count must be 0 or the obstacle count"
    assert check(alb_=alb, n_alb=3, n_obst=0) == b"the albedo count must be 0 or the obstacle count"
    assert check(alb_=None, n_alb=3) == b"null albedo array"
    for flags in (2, 4, -1, 1 << 30, 3):
        assert check(flags=flags) == b"flag bits other than SPH_HIP_RENDER_VELOCITY"
    # the camera, the params and the size are render_check's, with its texts
    assert check(cam_=None) == b"null camera or render params"
    assert check(w=0) == b"width and height must be in [1, 16384]"
    rp2 = good()[1]
    rp2.step = 0.0
    assert check(rp_=rp2) == b"step must be > 0"


def test_motion_velocity_rule(policy):
    from smoothed_particle_hydrodynamics_amd.obstacles import Motion
    m = Motion((0.0, 0.25, -0.5), 1.0, 3.0)
    for tau, on in ((0.0, False), (np.nextafter(F32(1.0), F32(0)), False), (1.0, True), (2.0, True),
                    (np.nextafter(F32(3.0), F32(0)), True), (3.0, False), (9.0, False)):
        v = np.zeros(3, F32)
        st = m.as_struct()
        policy.motion_velocity(C.byref(st), float(tau), ptr(v))
        want = SC.motion_velocity(m, tau)
        assert bits(v).tolist() == bits(want).tolist() and bool(v.any()) == on, tau
    rest = Motion((0.0, 0.0, 0.0), 0.0, np.inf).as_struct()
    v = np.ones(3, F32)
    policy.motion_velocity(C.byref(rest), 1.0, ptr(v))
    assert not v.any()


# ---- header against restatement, seeded ------------------------------------------------------------------------
def solid_of(kind, rng, axis=None):
    from smoothed_particle_hydrodynamics_amd.obstacles import Box, Cylinder, Sphere
    c = rng.uniform(0.1, 0.9, 3)
    if kind == "sphere":
        return Sphere(c, rng.uniform(0.05, 0.3))
    if kind == "box":
        half = rng.uniform(0.03, 0.3, 3)
        return Box(c - half, c + half)
    a = int(rng.integers(0, 3)) if axis is None else axis
    half = rng.uniform(0.05, 0.4)
    return Cylinder(a, c, rng.uniform(0.04, 0.25), c[a] - half, c[a] + half)


def bounds_of(o):
    """the solid's bounding box, float64"""
    s = SC._struct(o)
    cen, r = np.array(list(s.center), np.float64), float(s.radius)
    lo, hi = np.array(list(s.lo), np.float64), np.array(list(s.hi), np.float64)
    if s.kind == SC.SPHERE:
        return cen - r, cen + r
    if s.kind == SC.BOX:
        return lo, hi
    blo, bhi = cen - r, cen + r
    blo[s.axis], bhi[s.axis] = lo[s.axis], hi[s.axis]
    return blo, bhi


DIAGONAL = float(np.sqrt(3.0))   # of the unit domain the solids stand in


def seeded_rays(o, rng, n):
    """n rays toward the solid's neighbourhood: each from an eye of its own within 4 box diagonals of the
    solid (one in sixteen inside its bounding box), aimed at a point of the bounding box grown by a quarter."""
    blo, bhi = bounds_of(o)
    mid, ext = 0.5 * (blo + bhi), bhi - blo
    target = mid + (rng.uniform(-0.625, 0.625, (n, 3))) * ext
    away = rng.normal(size=(n, 3))
    away /= np.linalg.norm(away, axis=1)[:, None]
    dist = rng.uniform(0.6 * np.linalg.norm(ext), 4.0 * DIAGONAL, n)
    eye = target + away * dist[:, None]
    near = rng.random(n) < 1.0 / 16.0
    eye[near] = (mid + rng.uniform(-0.5, 0.5, (n, 3)) * ext)[near]
    eye = eye.astype(F32)
    d = unit((target - eye.astype(np.float64)).astype(F32))
    return eye, d


@pytest.fixture(scope="module")
def seeded():
    """per kind: [(solid, eyes, directions)] - ten solids of PER_KIND / 10 rays each"""
    out = {}
    for k, kind in enumerate(("sphere", "box", "cylinder")):
        rng = np.random.default_rng(2100 + k)
        out[kind] = []
        for j in range(10):
            o = solid_of(kind, rng, axis=j % 3)
            out[kind].append((o,) + seeded_rays(o, rng, PER_KIND // 10))
    return out


@pytest.mark.parametrize("kind", ["sphere", "box", "cylinder"])
def test_header_equals_restatement_on_seeded_rays(policy, seeded, kind):
    total = hits = inside = 0
    for o, eye, d in seeded[kind]:
        got = c_hit(policy, o, eye, d)
        assert_hits_equal(got, SC.hit(o, eye, d), "%s %r" % (kind, o))
        total += len(d)
        hits += int(got[0].sum())
        inside += int((got[0] & (got[1] == 0)).sum())
    assert total >= PER_KIND
    assert 0.3 * total < hits < 0.95 * total, (hits, total)     # both outcomes are well represented
    assert inside > 0.01 * total, inside                        # ... and so is an eye inside the solid


def test_nearest_equals_restatement_on_seeded_lists(policy):
    rng = np.random.default_rng(77)
    for count in (1, 3, 17, 64):
        solids = [solid_of(("sphere", "box", "cylinder")[i % 3], rng) for i in range(count)]
        n = 20000
        target = rng.uniform(0.0, 1.0, (n, 3))
        eye = (target + rng.normal(size=(n, 3)) * 1.5).astype(F32)
        d = unit((target - eye).astype(F32))
        gt, gn, gi = c_nearest(policy, solids, eye, d)
        wt, wn, wi = SC.nearest(solids, eye, d)
        assert (gi == wi).all() and (bits(gt) == bits(wt)).all() and (bits(gn) == bits(wn)).all(), count
        assert (gi >= 0).sum() > (n // 10 if count >= 17 else 100)
        if count == 64:
            assert len(set(gi.tolist())) > 20


def test_pixel_direction_is_the_renderers(policy):
    from smoothed_particle_hydrodynamics_amd import Camera
    cams = [(Camera.look_at((0.5, 0.5, 3.0), (0.5, 0.5, 0.5), (0, 1, 0), 40, 65, 49), 65, 49),
            (Camera((0.2, 0.3, 2.0), (0.0, 0.0, -1.0), (0.5, 0, 0), (0, 0.4, 0)), 13, 7),
            (Camera((0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)), 4, 3),
            (Camera((0, 0, 0), (1e30, 0, 0), (1e30, 0, 0), (0, 1e30, 0)), 4, 3)]
    for cam, W, H in cams:
        d, ok = np.zeros((W * H, 3), F32), np.zeros(W * H, np.int32)
        st = cam.as_struct()
        policy.pixel_dirs(C.byref(st), W, H, ptr(d), ptr(ok))
        py, px = np.divmod(np.arange(W * H), W)
        wd, wok = E.pixel_rays(cam, W, H, px, py)
        assert (ok.astype(bool) == wok).all()
        assert (bits(d)[wok] == bits(wd)[wok]).all()
    assert not ok.all()


# ---- directed cases ----------------------------------------------------------------------------------------------
def directed_cases():
    """[(name, solids, eye (3,), directions (n, 3) before normalisation)]"""
    from smoothed_particle_hydrodynamics_amd.obstacles import Box, Cylinder, Sphere
    sph = Sphere((0.5, 0.5, 0.5), 0.25)
    box = Box((0.25, 0.25, 0.25), (0.75, 0.5, 1.0))
    cyl = [Cylinder(a, (0.5, 0.5, 0.5), 0.25, 0.25, 0.75) for a in range(3)]
    fan = np.array([[x, y, z] for x in (-1, -0.5, 0, 0.5, 1) for y in (-1, 0, 0.25, 1) for z in (-1, 0, 1)
                    if (x, y, z) != (0, 0, 0)], np.float64)
    out = []
    # eye inside each solid, and at its centre
    for name, o in (("sphere", sph), ("box", box), ("cyl x", cyl[0]), ("cyl y", cyl[1]), ("cyl z", cyl[2])):
        out.append(("inside " + name, [o], (0.5, 0.4, 0.6), fan))
        out.append(("centre of " + name, [o], (0.5, 0.5, 0.5) if o is not box else (0.5, 0.375, 0.625), fan))
    # eye on the surface, looking every way: in, out and along it
    out.append(("on the sphere", [sph], (0.5, 0.5, 0.75), fan))
    out.append(("on a box face", [box], (0.5, 0.25, 0.5), fan))
    out.append(("on a box edge", [box], (0.25, 0.25, 0.5), fan))
    out.append(("on a box corner", [box], (0.75, 0.5, 1.0), fan))
    out.append(("on the cylinder's side", [cyl[1]], (0.75, 0.5, 0.5), fan))
    out.append(("on the cylinder's cap", [cyl[1]], (0.5, 0.75, 0.5), fan))
    out.append(("on the cylinder's rim", [cyl[1]], (0.75, 0.75, 0.5), fan))
    # tangent rays: the discriminant of either sign next to 0
    eye = np.array([0.5, 0.5, 2.0])
    xt = 1.5 * (1.0 / 6.0) / np.sqrt(35.0 / 36.0)   # the limb of the sphere and of the cylinder from 1.5 away
    tang = np.array([[xt * (1.0 + k * 2.0 ** -22), 0.0, -1.5] for k in range(-40, 41)])
    for scale in (0.99, 0.9999, 1.0, 1.0001, 1.01):
        t2 = tang.copy()
        t2[:, 0] *= scale
        out.append(("tangent to the sphere x%g" % scale, [sph], eye, t2))
        out.append(("tangent to the cylinder's side x%g" % scale, [cyl[1]], eye, t2))
    # exactly tangent in exact arithmetic: eye at x = center + r, looking along z
    out.append(("exactly tangent", [sph, cyl[1]], (0.75, 0.5, 2.0), np.array([[0, 0, -1.0], [0, 0, 1.0]])))
    # parallel to the cylinder's axis: inside, outside, and on the circle
    for a in range(3):
        e = np.zeros(3)
        e[a] = 1.0
        for off, where in ((0.1, "inside"), (0.3, "outside"), (0.25, "on")):
            eye = np.array([0.5, 0.5, 0.5])
            eye[a] = 2.0
            eye[(a + 1) % 3] += off
            out.append(("parallel to axis %d %s the circle" % (a, where), [cyl[a]], eye, np.array([e, -e])))
            eye2 = eye.copy()
            eye2[a] = 0.5
            out.append(("parallel to axis %d %s, eye between the caps" % (a, where), [cyl[a]], eye2, np.array([e, -e])))
    # along a box face plane with a zero direction component: the NaN corner of the slab
    for a in range(3):
        for plane in ("lo", "hi"):
            eye = np.array([0.5, 0.375, 0.625])
            eye[a] = getattr(box, plane)[a]
            eye[(a + 1) % 3] = 2.0
            dirs = []
            for s in (-1.0, 1.0):
                for tilt in (0.0, 0.1, -0.1):
                    v = np.zeros(3)
                    v[(a + 1) % 3] = s
                    v[(a + 2) % 3] = tilt
                    dirs.append(v)
                    dirs.append(np.where(v == 0, -0.0, v))
            out.append(("along the %s face plane of axis %d" % (plane, a), [box], eye, np.array(dirs)))
    # through a box edge and a corner: two or three slabs give the same t0 (dyadic numbers: exact)
    out.append(("through an edge", [Box((0.25, 0.25, 0.25), (0.75, 0.75, 0.75))], (-0.25, -0.25, 0.5),
                np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 0.125]])))
    out.append(("through a corner", [Box((0.25, 0.25, 0.25), (0.75, 0.75, 0.75))], (-0.25, -0.25, -0.25),
                np.array([[1.0, 1.0, 1.0]])))
    out.append(("through an edge, axis aligned", [Box((0.25, 0.25, 0.25), (0.75, 0.75, 0.75))], (0.25, 0.25, -1.0),
                np.array([[0.0, 0.0, 1.0], [-0.0, 0.0, 1.0], [0.0, -0.0, 1.0]])))
    # entering the cylinder exactly on the rim: side and cap bounds are equal
    out.append(("onto the rim", [Cylinder(2, (0.5, 0.5, 0.0), 0.25, 0.25, 0.75)], (1.75, 0.5, 1.75),
                np.array([[-1.0, 0.0, -1.0]])))
    out.append(("onto the rim, axis x", [Cylinder(0, (0.0, 0.5, 0.5), 0.25, 0.25, 0.75)], (1.75, 1.75, 0.5),
                np.array([[-1.0, -1.0, 0.0]])))
    # wholly behind the eye
    out.append(("behind the eye", [sph, box] + cyl, (0.5, 0.5, 3.0), np.array([[0.0, 0.0, 1.0], [0.1, -0.1, 1.0]])))
    # two solids at the same t: the lower index wins
    twin = [Box((0.25, 0.25, 0.25), (0.75, 0.75, 0.75)), sph, cyl[2]]
    out.append(("two solids at the same t", twin, (0.5, 0.5, 2.0), np.array([[0.0, 0.0, -1.0], [0.0, 0.125, -1.0]])))
    out.append(("two solids at the same t, reversed", twin[::-1], (0.5, 0.5, 2.0), np.array([[0.0, 0.0, -1.0]])))
    # 64 solids
    rng = np.random.default_rng(5)
    many = [solid_of(("sphere", "box", "cylinder")[i % 3], rng) for i in range(64)]
    out.append(("64 solids", many, (0.5, 0.5, 2.5), fan * np.array([0.3, 0.3, 1.0]) - np.array([0, 0, 1.5])))
    return [(name, solids, np.array(eye, np.float64), np.array(dirs, np.float64)) for name, solids, eye, dirs in out]


DIRECTED = directed_cases()


@pytest.mark.parametrize("case", DIRECTED, ids=[c[0] for c in DIRECTED])
def test_directed_cases_equal_the_restatement(policy, case):
    name, solids, eye, dirs = case
    d = unit(dirs)
    for o in solids:
        assert_hits_equal(c_hit(policy, o, eye, d), SC.hit(o, eye, d), name)
    gt, gn, gi = c_nearest(policy, solids, eye, d)
    wt, wn, wi = SC.nearest(solids, eye, d)
    assert (gi == wi).all() and (bits(gt) == bits(wt)).all() and (bits(gn) == bits(wn)).all(), name


def case(name):
    return [c for c in DIRECTED if c[0] == name][0]


def test_directed_cases_mean_what_they_say(policy):
    """the outcomes the contract states, read off the header's own answers"""
    _, solids, eye, dirs = case("inside sphere")
    h, t, n = c_hit(policy, solids[0], eye, unit(dirs))
    assert h.all() and (t == 0).all() and (bits(n) == bits(-unit(dirs))).all()
    _, solids, eye, dirs = case("behind the eye")
    for o in solids:
        assert not c_hit(policy, o, eye, unit(dirs))[0].any()
    # edges and corners: the first of x, y, z among equal slabs, the sign opposite to d
    _, solids, eye, dirs = case("through an edge")
    h, t, n = c_hit(policy, solids[0], eye, unit(dirs))
    assert h.all() and n.tolist() == [[-1, 0, 0], [-1, 0, 0]]
    _, solids, eye, dirs = case("through a corner")
    h, t, n = c_hit(policy, solids[0], eye, unit(dirs))
    assert h.all() and n.tolist() == [[-1, 0, 0]]
    # the rim: on equal bounds the side wins - a radial normal (a dyadic direction, so that the tie is exact)
    _, solids, eye, dirs = case("onto the rim")
    h, t, n = c_hit(policy, solids[0], eye, dirs.astype(F32))
    assert h.all() and t[0] == 1.0 and n[0].tolist() == [1.0, 0.0, 0.0]
    h, t, n = c_hit(policy, solids[0], eye, (dirs * np.array([1.0, 1.0, 0.9375])).astype(F32))   # the cap comes later
    assert h.all() and n[0].tolist() == [0.0, 0.0, 1.0]
    # parallel to the axis: a cap normal inside the circle, a miss outside and on it
    for a in range(3):
        c = case("parallel to axis %d inside the circle" % a)
        h, t, n = c_hit(policy, c[1][0], c[2], unit(c[3]))
        assert h.tolist() == [False, True] and n[1, a] == 1.0 and abs(n[1]).sum() == 1.0
        for where in ("outside", "on"):
            c = case("parallel to axis %d %s the circle" % (a, where))
            assert not c_hit(policy, c[1][0], c[2], unit(c[3]))[0].any()
        c = case("parallel to axis %d inside, eye between the caps" % a)
        h, t, n = c_hit(policy, c[1][0], c[2], unit(c[3]))
        assert h.all() and (t == 0).all()
    # tangents: both outcomes occur next to the limb
    for what in ("sphere", "cylinder's side"):
        seen = set()
        for c in DIRECTED:
            if c[0].startswith("tangent to the " + what):
                seen |= set(c_hit(policy, c[1][0], c[2], unit(c[3]))[0].tolist())
        assert seen == {True, False}
    # a tie between two solids goes to the lower index, whichever solid that is
    for name in ("two solids at the same t", "two solids at the same t, reversed"):
        _, solids, eye, dirs = case(name)
        t, n, i = c_nearest(policy, solids, eye, unit(dirs))
        each = [c_hit(policy, o, eye, unit(dirs))[1][0] for o in solids]
        assert each == [1.25, 1.25, 1.25] and i[0] == 0 and t[0] == 1.25
    # the NaN corner: a ray in a face plane with a zero component across it misses, and no NaN comes out
    for c in DIRECTED:
        if c[0].startswith("along the "):
            h, t, n = c_hit(policy, c[1][0], c[2], unit(c[3]))
            assert not h.any() and np.isfinite(t).all() and np.isfinite(n).all(), c[0]


# ---- accuracy, independent of the restatement ----------------------------------------------------------------------
DISC_CUT = 1e-5      # rays whose float64 discriminant is below this share of b*b graze: excluded
EDGE_ANGLE = 1e-5    # radians: rays that pass a box edge, a cylinder's rim or the eye's own surface this close
# Worst case of the header over the seeded rays (deterministic on a CPU; DESIGN.md section 21 records it):
#   |t - t64| / max(1, t64): sphere 5.34e-5, box 1.73e-7, cylinder 3.73e-5; the normal's largest component
#   error: sphere 1.83e-3, box 0, cylinder 4.07e-3.  (The quadratics subtract two numbers of the size of the
#   squared eye distance, up to 50 here, to get one of the size of r * r: that is where the bits go.)  The
#   bounds are four times those figures.
T_BOUND = {"sphere": 4 * 5.34e-5, "box": 4 * 1.73e-7, "cylinder": 4 * 3.73e-5}
N_BOUND = {"sphere": 4 * 1.83e-3, "box": 0.0, "cylinder": 4 * 4.07e-3}


def reference64(o, eye, d):
    """(hit, t, normal, excluded) in float64 on the same fp32 inputs, written geometrically, not as the
    contract orders its operations"""
    s = SC._struct(o)
    e, d = eye.astype(np.float64), d.astype(np.float64)
    n = len(d)
    cen, r = np.array(list(s.center), np.float64), float(s.radius)
    lo, hi = np.array(list(s.lo), np.float64), np.array(list(s.hi), np.float64)
    normal = np.zeros((n, 3))
    excl = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        def circle(idx):
            oc = e[:, idx] - cen[idx]
            dd = (d[:, idx] ** 2).sum(1)
            b = (oc * d[:, idx]).sum(1)
            c = (oc ** 2).sum(1) - r * r
            disc = b * b - dd * c
            graze = np.abs(disc) < DISC_CUT * b * b
            sq = np.sqrt(np.maximum(disc, 0.0))
            return disc >= 0, (-b - sq) / dd, (-b + sq) / dd, graze

        def slabs(idx):
            u0, u1 = (lo[idx] - e[:, idx]) / d[:, idx], (hi[idx] - e[:, idx]) / d[:, idx]
            return np.minimum(u0, u1), np.maximum(u0, u1)

        if s.kind == SC.SPHERE:
            ok, t0, t1, graze = circle([0, 1, 2])
            excl |= graze
            kind = np.zeros(n, int)
        elif s.kind == SC.BOX:
            nr, fr = slabs([0, 1, 2])
            t0, t1 = nr.max(1), fr.min(1)
            ok = np.ones(n, bool)
            kind = nr.argmax(1)
            # the angle at the eye between the ray and each of the 12 edges
            excl |= edge_angle(e, d, lo, hi) < EDGE_ANGLE
        else:
            a = int(s.axis)
            u, w = (a + 1) % 3, (a + 2) % 3
            ok, s0, s1, graze = circle([u, w])
            excl |= graze
            c0, c1 = slabs([a])
            c0, c1 = c0[:, 0], c1[:, 0]
            t0, t1 = np.maximum(s0, c0), np.minimum(s1, c1)
            kind = np.where(s0 >= c0, 0, 1)
            # the rim: both lower (or both upper) bounds within the angle, seen from the eye
            scale = np.maximum(np.abs(t0), 1e-3)
            excl |= ok & ((np.abs(s0 - c0) < EDGE_ANGLE * scale) | (np.abs(t1 - t0) < EDGE_ANGLE * scale))
        hit = ok & (t0 <= t1) & (t1 >= 0)
        inside = hit & (t0 < 0)
        # the eye within the angle's reach of the surface itself: inside and outside are one rounding apart
        excl |= np.abs(t0) < EDGE_ANGLE
        t = np.where(inside, 0.0, t0)
        p = e + t[:, None] * d
        if s.kind == SC.SPHERE:
            normal = (p - cen) / r
        elif s.kind == SC.BOX:
            normal[np.arange(n), kind] = -np.sign(d[np.arange(n), kind])
        else:
            normal[:, u] = np.where(kind == 0, (p[:, u] - cen[u]) / r, 0.0)
            normal[:, w] = np.where(kind == 0, (p[:, w] - cen[w]) / r, 0.0)
            normal[:, a] = np.where(kind == 0, 0.0, -np.sign(d[:, a]))
        normal = np.where(inside[:, None], -d, normal)
    return hit, t, normal, excl


def edge_angle(e, d, lo, hi):
    """the smallest angle (radians, small-angle form: distance over range) at which rays e + t d, t >= 0,
    pass one of the 12 edges of the box [lo, hi]"""
    best = np.full(len(d), np.inf)
    for a in range(3):
        u, w = (a + 1) % 3, (a + 2) % 3
        for cu in (lo[u], hi[u]):
            for cw in (lo[w], hi[w]):
                p0 = np.zeros(3)
                p0[a], p0[u], p0[w] = lo[a], cu, cw
                ev = np.zeros(3)
                ev[a] = hi[a] - lo[a]
                # closest points of the line e + t d and the segment p0 + s ev, s in [0, 1]
                r0 = e - p0
                dd, de, ee = (d * d).sum(1), d @ ev, float(ev @ ev)
                dr, er = (d * r0).sum(1), r0 @ ev
                den = dd * ee - de * de
                sgm = np.clip(np.where(den > 0, (dd * er - de * dr) / np.where(den > 0, den, 1.0), 0.0), 0.0, 1.0)
                t = np.maximum((sgm * de - dr) / dd, 0.0)
                gap = np.linalg.norm((e + t[:, None] * d) - (p0 + sgm[:, None] * ev), axis=1)
                best = np.minimum(best, gap / np.maximum(t, 1e-9))
    return best


def accuracy_figures(policy, seeded, kind):
    worst_t = worst_n = 0.0
    total = excluded = compared = 0
    for o, eye, d in seeded[kind]:
        h, t, nrm = c_hit(policy, o, eye, d)
        h64, t64, n64, excl = reference64(o, eye, d)
        keep = ~excl
        total += len(d)
        excluded += int(excl.sum())
        assert (h[keep] == h64[keep]).all(), "%s: hit/miss differs from float64 on %d rays away from grazing" % (
            kind, (h[keep] != h64[keep]).sum())
        sel = keep & h
        compared += int(sel.sum())
        worst_t = max(worst_t, float((np.abs(t[sel] - t64[sel]) / np.maximum(1.0, t64[sel])).max()))
        worst_n = max(worst_n, float(np.abs(nrm[sel] - n64[sel]).max()))
    return worst_t, worst_n, excluded / total, compared


@pytest.mark.parametrize("kind", ["sphere", "box", "cylinder"])
def test_accuracy_against_float64(policy, seeded, kind):
    worst_t, worst_n, share, compared = accuracy_figures(policy, seeded, kind)
    print("%s: |t - t64| / max(1, t64) <= %.3g, |n - n64| <= %.3g, %.2f %% excluded, %d hits compared" % (
        kind, worst_t, worst_n, 100 * share, compared))
    assert share <= 0.02, share
    assert compared > PER_KIND // 4
    assert worst_t <= T_BOUND[kind], (worst_t, T_BOUND[kind])
    assert worst_n <= N_BOUND[kind], (worst_n, N_BOUND[kind])


# ---- the composite ---------------------------------------------------------------------------------------------------
class Cam:
    def __init__(self, eye, forward, right, up):
        self.eye, self.forward, self.right, self.up = (np.array(v, F32) for v in (eye, forward, right, up))


def test_composite_rules():
    from smoothed_particle_hydrodynamics_amd.obstacles import Box, Sphere
    cam = Cam((0.5, 0.5, 3.0), (0, 0, -1), (0.25, 0, 0), (0, 0.25, 0))
    _, rp = good()
    rp.background[:] = [9, 8, 7, 6]
    W, H = 18, 14
    n = W * H
    solids = [Sphere((0.5, 0.5, 0.5), 0.4), Box((0.0, 0.0, 0.0), (0.4, 0.4, 0.2))]
    vel_s = np.array([[0.0, 0.5, 0.0], [1.0, 2.0, 3.0]], F32)
    alb_s = np.array([[0.9, 0.1, 0.1], [0.1, 0.9, 0.1]], F32)
    sp = scene_params((0.5, 0.5, 0.5), 0.3, 0.6)
    py, px = np.divmod(np.arange(n), W)
    d, ok = E.pixel_rays(cam, W, H, px, py)
    t_s, n_s, id_s = SC.nearest(solids, cam.eye, d)
    assert {0, 1, -1} <= set(id_s.tolist())
    # a fluid frame: in front of the solid on the left third, exactly at its depth in the middle, behind it
    # on the right, absent in every third row
    depth = np.where(px < 6, F32(0.5), np.where(px < 12, t_s, F32(4.0))).astype(F32)
    depth[py % 3 == 0] = np.inf
    first = np.where(np.isfinite(depth), 5, -1).astype(np.int32)
    fluid = E.Frame(np.full((n, 4), 77, np.uint8), depth, np.full((n, 3), 0.5, F32), np.full((n, 3), 0.25, F32), first)
    out = SC.composite(fluid, solids, cam, rp, sp, W, H, velocities=vel_s, albedos=alb_s)
    hit = id_s >= 0
    row = py % 3 != 0
    front = hit & (px < 6) & row
    equal = hit & (px >= 6) & (px < 12) & row
    behind = hit & (((px >= 12) & row) | ~row)
    assert front.any() and equal.any() and (behind & row).any() and (behind & ~row).any()
    for keep in (front, equal, ~hit):        # the fluid in front; the strict < at equal depth; no solid
        assert (out.solid_id[keep] == -1).all()
        for f in E.Frame._fields:
            assert np.ascontiguousarray(getattr(out, f)[keep]).tobytes() == \
                np.ascontiguousarray(getattr(fluid, f)[keep]).tobytes(), f
    assert (out.solid_id[behind] == id_s[behind]).all()
    assert (out.first_inside[behind] == -1).all()
    assert (bits(out.depth[behind]) == bits(t_s[behind])).all()
    assert (bits(out.normal[behind]) == bits(n_s[behind])).all()
    assert (out.velocity[behind] == vel_s[id_s[behind]]).all()
    assert (out.rgba[behind] == SC.shade(n_s[behind], rp.light, alb_s[id_s[behind]], 0.3, 0.6)).all()
    assert (out.rgba[behind, 3] == 255).all() and len({tuple(c) for c in out.rgba[behind, :3].tolist()}) > 4
    # without the velocity flag a solid pixel's velocity is 0; default albedo is the scene's
    plain = SC.composite(fluid, solids, cam, rp, sp, W, H, velocities=vel_s, velocity=False)
    assert (plain.velocity[behind] == 0).all()
    assert (plain.rgba[behind] == SC.shade(n_s[behind], rp.light, np.full((int(behind.sum()), 3), 0.5, F32), 0.3, 0.6)).all()
    # a frame without solids is unchanged bit for bit
    none = SC.composite(fluid, [], cam, rp, sp, W, H)
    assert (none.solid_id == -1).all()
    for f in E.Frame._fields:
        assert getattr(none, f).tobytes() == getattr(fluid, f).tobytes()
    # over the background frame (no particle resident) the solids stand alone
    alone = SC.composite(SC.background(rp, n), solids, cam, rp, sp, W, H)
    assert (alone.solid_id == id_s).all() and (alone.rgba[~hit] == [9, 8, 7, 6]).all()


def test_shade_and_strict_depth_match_the_header(policy):
    rng = np.random.default_rng(3)
    nrm = unit(rng.normal(size=(500, 3)))
    alb = rng.uniform(0, 1.2, (500, 3)).astype(F32)
    light = np.array([0.4, 0.8, 0.45], F32)
    want = SC.shade(nrm, light, alb, 0.2, 0.8)
    for i in range(500):
        got = policy.shade(ptr(nrm[i]), ptr(light), ptr(alb[i]), 0.2, 0.8)
        assert [got & 255, got >> 8 & 255, got >> 16 & 255, got >> 24] == want[i].tolist()
    inf = float("inf")
    assert [policy.in_front(a, b) for a, b in ((1.0, 1.0), (1.0, inf), (0.0, 0.0), (1.0, 2.0), (2.0, 1.0),
                                                (inf, inf))] == [0, 1, 0, 1, 0, 0]


# ---- the functions under the sanitizers, in a program of their own ------------------------------------------------------
MAIN = CALLS + r"""
#include <stdio.h>
#include <stdlib.h>
// stdin: count, then per case: n_solids, the solids' 12 words each, n_rays, eye[3], directions
int main()
{
   int cases = 0, hits = 0;
   if (scanf("%d", &cases) != 1) return 2;
   for (int c = 0; c < cases; c++) {
      int ns = 0, nr = 0;
      if (scanf("%d", &ns) != 1 || ns < 0 || ns > SPH_HIP_MAX_OBSTACLES) return 2;
      sph_hip_obstacle* list = (sph_hip_obstacle*)malloc(sizeof(sph_hip_obstacle) * (ns > 0 ? ns : 1));
      for (int i = 0; i < ns; i++) {
         sph_hip_obstacle& o = list[i];
         if (scanf("%d %d %a %a %a %a %a %a %a %a %a %a", &o.kind, &o.axis, &o.center[0], &o.center[1], &o.center[2],
                   &o.radius, &o.lo[0], &o.lo[1], &o.lo[2], &o.hi[0], &o.hi[1], &o.hi[2]) != 12) return 2;
      }
      float eye1[3];
      if (scanf("%d %a %a %a", &nr, &eye1[0], &eye1[1], &eye1[2]) != 4 || nr < 1) return 2;
      float* eye = (float*)malloc(sizeof(float) * 3 * nr);
      float* d = (float*)malloc(sizeof(float) * 3 * nr);
      float* t = (float*)malloc(sizeof(float) * nr);
      float* nrm = (float*)malloc(sizeof(float) * 3 * nr);
      int* id = (int*)malloc(sizeof(int) * nr);
      for (int i = 0; i < nr; i++) {
         for (int k = 0; k < 3; k++) eye[3 * i + k] = eye1[k];
         if (scanf("%a %a %a", &d[3 * i], &d[3 * i + 1], &d[3 * i + 2]) != 3) return 2;
      }
      for (int i = 0; i < ns; i++) hit_many(list + i, eye, d, nr, t, nrm, id);
      nearest_many(list, ns, eye, d, nr, t, nrm, id);
      for (int i = 0; i < nr; i++) hits += id[i] >= 0;
      free(list); free(eye); free(d); free(t); free(nrm); free(id);
   }
   printf("cases %d hits %d\n", cases, hits);
   return 0;
}
"""


def test_directed_cases_under_the_sanitizers(policy, tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    src, exe = tmp_path / "scene_main.cpp", tmp_path / "scene_main"
    src.write_text(MAIN)
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    lines = [str(len(DIRECTED))]
    want_hits = 0
    for name, solids, eye, dirs in DIRECTED:
        d = unit(dirs)
        lines.append(str(len(solids)))
        for o in solids:
            s = SC._struct(o)
            vals = [s.center[0], s.center[1], s.center[2], s.radius] + list(s.lo) + list(s.hi)
            lines.append("%d %d " % (s.kind, s.axis) + " ".join(float(v).hex() for v in vals))
        lines.append("%d " % len(d) + " ".join(float(F32(v)).hex() for v in eye))
        lines += [" ".join(float(v).hex() for v in row) for row in d]
        want_hits += int((c_nearest(policy, solids, eye, d)[2] >= 0).sum())
    run = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == "", run.stderr
    assert run.stdout.split() == ["cases", str(len(DIRECTED)), "hits", str(want_hits)]
