"""CPU checks of the renderer (include/sph_hip.h: sph_hip_render): the C ABI and its binding, the
argument checks, byte quantisation and row chunking of csrc/render_policy.h (compiled with g++ behind
an extern "C" shim, as tests/test_surface_cpu.py does), the numpy restatement the GPU tests check
against (tests/render_emulation.py) on analytic fields, and write_png."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

import render_emulation as E
from helpers import compile_shim
from test_sample_cpu import header_prototype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

SHIM = r"""
#include <stddef.h>
#include "render_policy.h"

extern "C" {
const char* check(const sph_hip_camera* cam, const sph_hip_render_params* rp, int w, int h, int flags)
{
   const char* why = render_check(cam, rp, w, h, flags);
   return why ? why : "";
}
int quant(float v) { return render_byte(v); }
int chunk_rows(int w, int h) { return render_chunk_rows(w, h); }
long long scratch_bytes(int w, int rows) { return render_scratch_bytes(w, rows); }
long long budget() { return RENDER_SCRATCH_BUDGET; }
#define OFF(T, f) (long long)offsetof(T, f)
void layout(long long* out)
{
   out[0] = sizeof(sph_hip_camera);
   out[1] = OFF(sph_hip_camera, eye); out[2] = OFF(sph_hip_camera, forward);
   out[3] = OFF(sph_hip_camera, right); out[4] = OFF(sph_hip_camera, up);
   out[5] = sizeof(sph_hip_render_params);
   out[6] = OFF(sph_hip_render_params, box_lo); out[7] = OFF(sph_hip_render_params, box_hi);
   out[8] = OFF(sph_hip_render_params, step); out[9] = OFF(sph_hip_render_params, iso);
   out[10] = OFF(sph_hip_render_params, refine); out[11] = OFF(sph_hip_render_params, grad_step);
   out[12] = OFF(sph_hip_render_params, light); out[13] = OFF(sph_hip_render_params, albedo);
   out[14] = OFF(sph_hip_render_params, ambient); out[15] = OFF(sph_hip_render_params, diffuse);
   out[16] = OFF(sph_hip_render_params, background); out[17] = OFF(sph_hip_render_params, max_samples);
}
}
"""


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    from smoothed_particle_hydrodynamics_amd.lib import SphCamera, SphRenderParams
    lib = compile_shim(SHIM, ["-O1"], tmp_path_factory)
    lib.check.argtypes = [C.POINTER(SphCamera), C.POINTER(SphRenderParams), C.c_int, C.c_int, C.c_int]
    lib.check.restype = C.c_char_p
    lib.quant.argtypes = [C.c_float]
    lib.scratch_bytes.argtypes = [C.c_int, C.c_int]
    lib.scratch_bytes.restype = C.c_longlong
    lib.budget.restype = C.c_longlong
    lib.layout.argtypes = [C.POINTER(C.c_longlong)]
    return lib


# ---- C ABI -----------------------------------------------------------------------------------------
def test_render_symbol_is_exported(hiplib):
    assert hasattr(hiplib, "sph_hip_render")


def test_render_prototype_matches_the_header():
    from smoothed_particle_hydrodynamics_amd.lib import PROTOTYPES, SphCamera, SphRenderParams
    assert header_prototype("sph_hip_render") == [
        "sph_hip_context* ctx", "const sph_hip_camera* cam", "const sph_hip_render_params* rp", "int width",
        "int height", "int flags", "uint8_t* rgba", "float* depth", "float* normal_xyz", "float* velocity_xyz",
        "int32_t* first_inside"]
    res, args = PROTOTYPES["sph_hip_render"]
    assert res is C.c_int and len(args) == 11 and args[0] is C.c_void_p
    assert args[1]._type_ is SphCamera and args[2]._type_ is SphRenderParams
    assert args[3:6] == [C.c_int] * 3 and args[6:] == [C.c_void_p] * 5


def test_structs_match_the_c_layout(policy):
    from smoothed_particle_hydrodynamics_amd.lib import SphCamera, SphRenderParams
    out = (C.c_longlong * 18)()
    policy.layout(out)
    cam = [C.sizeof(SphCamera)] + [getattr(SphCamera, f).offset for f in ("eye", "forward", "right", "up")]
    rp = [C.sizeof(SphRenderParams)] + [getattr(SphRenderParams, f).offset for f in (
        "box_lo", "box_hi", "step", "iso", "refine", "grad_step", "light", "albedo", "ambient", "diffuse",
        "background", "max_samples")]
    assert list(out) == cam + rp
    assert cam[0] == 48 and rp[0] == 80


def test_flag_and_abi_version():
    from smoothed_particle_hydrodynamics_amd.lib import ABI_VERSION
    text = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    assert "#define SPH_HIP_RENDER_VELOCITY 1" in text
    assert "#define SPH_HIP_ABI_VERSION 7" in text and ABI_VERSION == 7


# ---- policy: refusals -----------------------------------------------------------------------------------
def good():
    from smoothed_particle_hydrodynamics_amd import Camera
    from smoothed_particle_hydrodynamics_amd.lib import SphRenderParams
    cam = Camera.look_at((0.5, 0.5, 3.0), (0.5, 0.5, 0.5), (0, 1, 0), 40, 64, 48).as_struct()
    rp = SphRenderParams()
    rp.box_lo[:] = [-0.1, -0.1, -0.1]
    rp.box_hi[:] = [1.1, 1.1, 1.1]
    rp.step, rp.iso, rp.refine, rp.grad_step = 0.01, 1.0, 8, 0.01
    rp.light[:] = [0.0, 1.0, 1.0]
    rp.albedo[:] = [0.5, 0.5, 0.5]
    rp.ambient, rp.diffuse = 0.2, 0.8
    rp.background[:] = [0, 0, 0, 255]
    rp.max_samples = 1 << 16
    return cam, rp


def refusals():
    """(what, camera/params mutator, width, height, flags, message fragment)"""
    out = []
    for w, h in ((0, 48), (64, 0), (16385, 48), (64, 16385), (-1, 48)):
        out.append(("size %dx%d" % (w, h), None, w, h, 0, b"width and height"))
    for flags in (2, 4, -1, 1 << 30):
        out.append(("flags %d" % flags, None, 64, 48, flags, b"flag"))
    for field in ("eye", "forward", "right", "up"):
        for bad in (np.nan, np.inf, -np.inf):
            out.append(("camera %s %r" % (field, bad), ("cam", field, 1, bad), 64, 48, 0, b"finite"))
    for field in ("box_lo", "box_hi", "light", "albedo"):
        out.append(("params %s nan" % field, ("rp", field, 2, np.nan), 64, 48, 0, b"finite"))
    for field in ("step", "iso", "grad_step", "ambient", "diffuse"):
        for bad in (np.nan, np.inf):
            out.append(("params %s %r" % (field, bad), ("rp", field, None, bad), 64, 48, 0, b"finite"))
    for field, msg in (("step", b"step"), ("grad_step", b"grad_step"), ("iso", b"iso")):
        for bad in (0.0, -0.0, -1.0):
            out.append(("params %s %r" % (field, bad), ("rp", field, None, bad), 64, 48, 0, msg))
    for bad in (-1, 31, 1 << 20):
        out.append(("refine %d" % bad, ("rp", "refine", None, bad), 64, 48, 0, b"refine"))
    for a in range(3):
        out.append(("box equal axis %d" % a, ("box", a, 0.5, 0.5), 64, 48, 0, b"box_lo"))
        out.append(("box inverted axis %d" % a, ("box", a, 0.6, 0.5), 64, 48, 0, b"box_lo"))
    out.append(("zero light", ("light0",), 64, 48, 0, b"light"))
    for bad in (0, -1, (1 << 24) + 1):
        out.append(("max_samples %d" % bad, ("rp", "max_samples", None, bad), 64, 48, 0, b"max_samples"))
    return out


def apply(cam, rp, mut):
    if mut is None:
        return
    if mut[0] == "box":
        rp.box_lo[mut[1]], rp.box_hi[mut[1]] = mut[2], mut[3]
    elif mut[0] == "light0":
        rp.light[:] = [0.0, -0.0, 0.0]
    else:
        obj = cam if mut[0] == "cam" else rp
        if mut[2] is None:
            setattr(obj, mut[1], mut[3])
        else:
            getattr(obj, mut[1])[mut[2]] = mut[3]


REFUSALS = refusals()


def test_good_arguments_pass(policy):
    cam, rp = good()
    assert policy.check(C.byref(cam), C.byref(rp), 64, 48, 0) == b""
    assert policy.check(C.byref(cam), C.byref(rp), 16384, 16384, 1) == b""
    rp.refine, rp.max_samples = 0, 1
    assert policy.check(C.byref(cam), C.byref(rp), 1, 1, 0) == b""
    rp.refine, rp.max_samples = 30, 1 << 24
    assert policy.check(C.byref(cam), C.byref(rp), 1, 1, 0) == b""
    assert policy.check(None, C.byref(rp), 1, 1, 0) != b"" and policy.check(C.byref(cam), None, 1, 1, 0) != b""


@pytest.mark.parametrize("case", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(policy, case):
    what, mut, w, h, flags, msg = case
    cam, rp = good()
    apply(cam, rp, mut)
    why = policy.check(C.byref(cam), C.byref(rp), w, h, flags)
    assert msg in why, (what, why)


# ---- policy: quantisation and chunks ------------------------------------------------------------------------
def test_byte_quantisation_matches_the_emulation(policy):
    vals = [0.0, -0.0, 1.0, -1.0, 2.0, np.nan, np.inf, -np.inf, 1e-30, 0.5, 0.999999]
    for k in range(256):
        # values whose scaled form lands just below, at and just above each half step k + 0.5
        x = F32((k + 0.5) / 255.0)
        for v in (x, np.nextafter(x, F32(0)), np.nextafter(x, F32(2)), np.nextafter(np.nextafter(x, F32(0)), F32(0)),
                  F32(k / 255.0)):
            vals.append(float(v))
    v = np.array(vals, F32)
    want = np.array([policy.quant(float(x)) for x in v])
    got = E.quantise(v).astype(int)
    assert (got == want).all(), np.flatnonzero(got != want)
    assert E.quantise(F32(0.0)) == 0 and E.quantise(F32(1.0)) == 255 and E.quantise(F32(np.nan)) == 0
    # at the half steps both neighbours appear: the rounding is really exercised
    assert len(set(want.tolist())) == 256


@pytest.mark.parametrize("w,h", [(16384, 16384), (1280, 720), (1, 1), (1, 16384), (16384, 1), (333, 7777),
                                 (4096, 4096)])
def test_row_chunks_stay_in_budget(policy, w, h):
    rows = policy.chunk_rows(w, h)
    assert 1 <= rows <= h
    assert policy.scratch_bytes(w, rows) <= policy.budget()
    if rows < h:
        assert rows % 8 == 0 or rows < 8
        assert policy.scratch_bytes(w, rows + 8) > policy.budget()
    # every byte an output needs: 40 per pixel at least
    assert policy.scratch_bytes(w, rows) >= 40 * w * rows


def test_1280x720_is_one_chunk(policy):
    assert policy.chunk_rows(1280, 720) == 720


# ---- emulation on analytic fields ------------------------------------------------------------------------------
class Cam:
    def __init__(self, eye, forward, right, up):
        self.eye, self.forward, self.right, self.up = (np.array(v, F32) for v in (eye, forward, right, up))


def params(step=0.01, iso=1.0, refine=8, gs=1e-3, lo=(-2, -2, -2), hi=(2, 2, 2), max_samples=1 << 16):
    from smoothed_particle_hydrodynamics_amd.lib import SphRenderParams
    rp = SphRenderParams()
    rp.box_lo[:], rp.box_hi[:] = list(lo), list(hi)
    rp.step, rp.iso, rp.refine, rp.grad_step = step, iso, refine, gs
    rp.light[:] = [0.3, 0.5, 0.8]
    rp.albedo[:] = [0.9, 0.6, 0.3]
    rp.ambient, rp.diffuse = 0.1, 0.9
    rp.background[:] = [10, 20, 30, 40]
    rp.max_samples = max_samples
    return rp


def ball(R=1.0, c=(0.0, 0.0, 0.0)):
    c = np.array(c, np.float64)

    def f(p):
        return (R + 1.0 - np.sqrt(((np.asarray(p, np.float64) - c) ** 2).sum(1))).astype(F32)
    return f


def ray_sphere(eye, d, R):
    """float64 distance along unit d from eye to the sphere |p| = R (first entry), NaN on a miss"""
    e, d = np.asarray(eye, np.float64), np.asarray(d, np.float64)
    b = d @ e
    c = e @ e - R * R
    disc = b * b - c
    with np.errstate(invalid="ignore"):
        return np.where(disc >= 0, -b - np.sqrt(disc), np.nan)


CAMERAS = [((0.0, 0.0, 4.0), (0.0, 0.0, 0.0)), ((3.0, 1.5, 2.0), (0.1, -0.2, 0.0)),
           ((-2.5, -2.5, 1.0), (0.0, 0.0, 0.0)), ((0.3, 3.5, 0.2), (0.0, 0.0, 0.0))]


@pytest.mark.parametrize("eye,target", CAMERAS)
def test_ball_depth_and_normals(eye, target):
    from smoothed_particle_hydrodynamics_amd import Camera
    W, H = 48, 36
    cam = Camera.look_at(eye, target, (0, 0, 1) if abs(eye[2]) < 3.9 else (0, 1, 0), 50, W, H)
    rp = params(lo=(-1.6, -1.6, -1.6), hi=(1.6, 1.6, 1.6))
    fr = E.render(ball(), cam, rp, W, H)
    py, px = np.divmod(np.arange(W * H), W)
    d, _ = E.pixel_rays(cam, W, H, px, py)
    t = ray_sphere(cam.eye, d, 1.0)
    hit = fr.first_inside >= 0
    # a ray that grazes the sphere within a step may miss between samples; every other hit agrees
    clear = np.isfinite(t) & (np.abs(ray_sphere(cam.eye, d, 0.98)) > 0)
    assert (hit[clear]).all()
    assert not hit[~np.isfinite(t)].any()
    assert hit.sum() > 100
    # the bisection brackets the crossing within step / 2^refine along the ray; the field's fp32 rounding
    # (~2e-7) moves it by that over the incidence cosine, so grazing rays are held to the normals only
    p = np.asarray(cam.eye, np.float64) + fr.depth[hit, None].astype(np.float64) * d[hit]
    want_n = p / np.linalg.norm(p, axis=1, keepdims=True)
    cos = np.abs((want_n * d[hit]).sum(1))
    tol = float(rp.step) / 2 ** rp.refine + 1e-6 / np.maximum(cos, 1e-3)
    err = np.abs(fr.depth[hit] - t[hit])
    assert (err[cos > 0.05] <= tol[cos > 0.05]).all(), err.max()
    assert np.abs(fr.normal[hit] - want_n).max() < 1e-3
    assert (fr.rgba[~hit] == [10, 20, 30, 40]).all() and (fr.rgba[hit, 3] == 255).all()
    assert np.isinf(fr.depth[~hit]).all() and (fr.normal[~hit] == 0).all()
    # shading is the contract's, from the normal
    l = np.array([0.3, 0.5, 0.8], F32)
    l = l / np.sqrt((l[0] * l[0] + l[1] * l[1]) + l[2] * l[2])
    n = fr.normal[hit]
    w = F32(0.1) + F32(0.9) * np.fmax((n[:, 0] * l[0] + n[:, 1] * l[1]) + n[:, 2] * l[2], F32(0))
    assert (fr.rgba[hit, 0] == E.quantise(F32(0.9) * w)).all()


def test_camera_inside_the_ball():
    cam = Cam((0.1, 0.2, 0.0), (0, 0, -1), (0.5, 0, 0), (0, 0.4, 0))
    rp = params()
    fr = E.render(ball(), cam, rp, 16, 12)
    assert (fr.first_inside == 0).all()
    d, _ = E.pixel_rays(cam, 16, 12, *np.divmod(np.arange(16 * 12), 16)[::-1])
    tnear, _, _ = E.box_interval(cam.eye, d, rp.box_lo, rp.box_hi)
    assert (fr.depth == tnear).all() and (fr.depth == 0).all()


def test_axis_aligned_rays_and_box_misses():
    # forward along -z, no right/up components in x at the centre column: zero direction components
    cam = Cam((0.0, 0.0, 5.0), (0, 0, -1), (1.0, 0, 0), (0, 1.0, 0))
    rp = params(lo=(-1.5, -1.5, -1.5), hi=(1.5, 1.5, 1.5))
    W, H = 9, 9   # pixel (4, 4) looks straight down -z: d = (0, 0, -1)
    fr = E.render(ball(), cam, rp, W, H)
    d, _ = E.pixel_rays(cam, W, H, [4], [4])
    assert d[0, 0] == 0 and d[0, 1] == 0
    assert fr.first_inside[4 * W + 4] >= 0
    assert abs(fr.depth[4 * W + 4] - 4.0) <= float(rp.step) / 2 ** 8 + 1e-5
    # a camera looking away from the box and one beside it along a zero component: every ray misses
    away = Cam((0.0, 0.0, 5.0), (0, 0, 1), (0.2, 0, 0), (0, 0.2, 0))
    assert (E.render(ball(), away, rp, 8, 8).first_inside == -1).all()
    beside = Cam((0.0, 3.0, 5.0), (0, 0, -1), (0.0, 0, 0), (0, 0.0, 0))
    fr = E.render(ball(), beside, rp, 4, 4)
    assert (fr.first_inside == -1).all() and np.isinf(fr.depth).all()
    # a zero direction: len 0 misses
    zero = Cam((0.0, 0.0, 5.0), (0, 0, 0), (0, 0, 0), (0, 0, 0))
    assert (E.render(ball(), zero, rp, 3, 3).first_inside == -1).all()
    # NaN corner of the slab test: eye on the upper x face with d_x = +0: t1 = 0 * inf = NaN, so the
    # C99 rules give far_x = fmaxf(-inf, NaN) = -inf, and the ray misses
    face = Cam((1.5, 0.0, 5.0), (0, 0, -1), (0, 0, 0), (0, 0, 0))
    d, ok = E.pixel_rays(face, 1, 1, [0], [0])
    tn, tf, hit = E.box_interval(face.eye, d, rp.box_lo, rp.box_hi)
    assert ok[0] and not hit[0] and tf[0] == -np.inf
    # on the lower face: t0 = NaN, t1 = +inf, near_x = fminf(NaN, inf) = +inf: a miss as well
    face = Cam((-1.5, 0.0, 5.0), (0, 0, -1), (0, 0, 0), (0, 0, 0))
    d, ok = E.pixel_rays(face, 1, 1, [0], [0])
    tn, tf, hit = E.box_interval(face.eye, d, rp.box_lo, rp.box_hi)
    assert ok[0] and not hit[0] and tn[0] == np.inf


def test_max_samples_caps_the_march():
    cam = Cam((0.0, 0.0, 5.0), (0, 0, -1), (0, 0, 0), (0, 0, 0))
    rp = params(step=0.01, lo=(-1.5, -1.5, -1.5), hi=(1.5, 1.5, 1.5))
    # the surface is 0.5 past the box face: 50 steps
    fr = E.render(ball(), cam, rp, 1, 1)
    assert fr.first_inside[0] == 50 or fr.first_inside[0] == 51
    k = int(fr.first_inside[0])
    assert E.render(ball(), cam, params(step=0.01, lo=(-1.5,) * 3, hi=(1.5,) * 3, max_samples=k), 1, 1).first_inside[0] == -1
    assert E.render(ball(), cam, params(step=0.01, lo=(-1.5,) * 3, hi=(1.5,) * 3, max_samples=k + 1), 1, 1
                    ).first_inside[0] == k


def test_refine_zero_gives_the_sample():
    cam = Cam((0.2, 0.1, 5.0), (0, 0, -1), (0.3, 0, 0), (0, 0.3, 0))
    rp = params(refine=0)
    fr = E.render(ball(), cam, rp, 8, 8)
    hit = fr.first_inside >= 0
    assert hit.sum() > 10
    d, _ = E.pixel_rays(cam, 8, 8, *np.divmod(np.arange(64), 8)[::-1])
    tnear, _, _ = E.box_interval(cam.eye, d, rp.box_lo, rp.box_hi)
    want = (tnear + fr.first_inside.astype(F32) * F32(rp.step)).astype(F32)
    assert (fr.depth[hit] == want[hit]).all()


def test_a_subset_of_pixels_is_the_frame_restricted():
    cam = Cam((0.2, 0.1, 5.0), (0, 0, -1), (0.3, 0, 0), (0, 0.3, 0))
    rp = params()
    full = E.render(ball(), cam, rp, 10, 6)
    rng = np.random.default_rng(1)
    idx = rng.choice(60, 17, replace=False)
    py, px = np.divmod(idx, 10)
    sub = E.render(ball(), cam, rp, 10, 6, pixels=(px, py))
    for a, b in zip(full, sub):
        assert (a[idx] == b).all() if a.dtype != F32 else a[idx].tobytes() == b.tobytes()


# ---- write_png -------------------------------------------------------------------------------------------------
def read_png(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, ihdr = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + body) & 0xFFFFFFFF
        if tag == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    W, H, depth, ctype, _, _, interlace = ihdr
    assert depth == 8 and ctype == 6 and interlace == 0
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + 4 * W)
    assert (raw[:, 0] == 0).all()   # filter 0 on every row
    return raw[:, 1:].reshape(H, W, 4)


@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (48, 64)])
def test_write_png_round_trips(tmp_path, shape):
    from smoothed_particle_hydrodynamics_amd import write_png
    img = np.random.default_rng(5).integers(0, 256, shape + (4,), dtype=np.uint8)
    path = tmp_path / "f.png"
    write_png(str(path), img)
    assert read_png(str(path)).tobytes() == img.tobytes()
