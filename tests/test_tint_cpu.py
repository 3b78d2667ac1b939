"""CPU checks of the scalar renderer (include/sph_hip.h: sph_hip_render_scalars): the C ABI and its binding, the
refusals of csrc/tint_policy.h, its map, shade and column functions (compiled with g++ behind an extern "C"
shim, as tests/test_scene_cpu.py does) bit for bit against the numpy restatement tests/tint_emulation.py on
seeded and directed values, the launch decision, one run of the directed cases under the address and
undefined-behaviour sanitizers in a stand-alone host program, the restatement itself on an analytic case (a rest
lattice block with a uniform channel), the colour tables and renderScalars' argument handling."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import render_emulation as E
import tint_emulation as TE
from helpers import compile_shim
from test_render_cpu import good
from test_sample_cpu import header_prototype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smoothed_particle_hydrodynamics_amd", "csrc")
F32 = np.float32

# what both the shim and the sanitizer program call
CALLS = r"""
#include <stddef.h>
#include "launch_policy.h"
#include "tint_policy.h"

extern "C" {
const char* check(const sph_hip_camera* cam, const sph_hip_render_params* rp, const sph_hip_scene_params* sp,
                  const float* albedo, int n_albedo, int n_obstacles, int n_scalars, const sph_hip_tint_params* tp,
                  const float* table, int w, int h, int flags)
{
   const char* why = tint_check(cam, rp, sp, albedo, n_albedo, n_obstacles, n_scalars, tp, table, w, h, flags);
   return why ? why : "";
}
void map_many(const float* v, int n, float lo, float hi, int n_colors, const float* table, float* col)
{
   for (int i = 0; i < n; i++) tint_map(v[i], lo, hi, n_colors, table, col + 3 * i);
}
void weight_many(const float* normal, int n, const float* light, float ambient, float diffuse, float* w)
{
   for (int i = 0; i < n; i++) w[i] = tint_weight(normal + 3 * i, light, ambient, diffuse);
}
void pixel_many(const float* col, const float* w, int n, unsigned* rgba)
{
   for (int i = 0; i < n; i++) rgba[i] = tint_pixel(col + 3 * i, w[i]);
}
float column_sequence(const float* rho, const float* a, int n, float iso, float step)
{
   float A = 0.0f;
   for (int i = 0; i < n; i++) A = tint_column_add(A, rho[i], a[i], iso, step);
   return A;
}
}
"""

SHIM = CALLS + r"""
extern "C" {
void layout(long long* out)
{
   out[0] = sizeof(sph_hip_tint_params);
   out[1] = offsetof(sph_hip_tint_params, channel);
   out[2] = offsetof(sph_hip_tint_params, mode);
   out[3] = offsetof(sph_hip_tint_params, lo);
   out[4] = offsetof(sph_hip_tint_params, hi);
   out[5] = offsetof(sph_hip_tint_params, n_colors);
   out[6] = offsetof(sph_hip_tint_params, flags);
   out[7] = SPH_HIP_ABI_VERSION;
   out[8] = SPH_HIP_TINT_SURFACE;
   out[9] = SPH_HIP_TINT_COLUMN;
   out[10] = SPH_HIP_TINT_FLAT;
   out[11] = SPH_HIP_TINT_MAX_COLORS;
   out[12] = TINT_TABLE_FLOATS;
}
long long scalar_bytes(int w, int rows) { return tint_scalar_bytes(w, rows); }
int launches_tint(int have_tint, int n) { return frame_launches_tint(have_tint != 0, n) ? 1 : 0; }
// decisions that stand unchanged beside the new ones
int launches_scalars(int n_scalars, int n) { return step_launches_scalars(n_scalars, n) ? 1 : 0; }
long long id_bytes(int w, int rows) { return scene_id_bytes(w, rows); }
int chunk_rows(int w, int h) { return render_chunk_rows(w, h); }
long long scratch_bytes(int w, int rows) { return render_scratch_bytes(w, rows); }
long long pixel_bytes() { return RENDER_PIXEL_BYTES; }
}
"""


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    lib = compile_shim(SHIM, ["-O2", "-ffp-contract=off"], tmp_path_factory)
    lib.check.restype = C.c_char_p
    lib.layout.argtypes = [C.POINTER(C.c_longlong)]
    lib.map_many.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p]
    lib.weight_many.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_void_p]
    lib.pixel_many.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.column_sequence.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float]
    lib.column_sequence.restype = C.c_float
    for f in (lib.scalar_bytes, lib.id_bytes, lib.scratch_bytes, lib.pixel_bytes):
        f.restype = C.c_longlong
    return lib


def c_map(policy, v, lo, hi, table):
    v = np.ascontiguousarray(v, F32).reshape(-1)
    table = np.ascontiguousarray(table, F32).reshape(-1, 3)
    col = np.zeros((v.size, 3), F32)
    policy.map_many(ptr(v), v.size, float(lo), float(hi), table.shape[0], ptr(table), ptr(col))
    return col


def assert_same(got, want, what):
    bad = np.flatnonzero((bits(got).reshape(got.shape[0], -1) != bits(want).reshape(want.shape[0], -1)).any(1))
    assert bad.size == 0, "%s: %d differ, first %d: %r vs %r" % (what, bad.size, bad[0], got[bad[0]], want[bad[0]])


def seeded_table(rng, n, wild=False):
    t = rng.uniform(0.0, 1.0, (n, 3)).astype(F32)
    if wild:    # negative entries and entries above 1: render_byte clamps the product
        t[::2] = rng.uniform(-0.8, 2.5, t[::2].shape).astype(F32)
    return t


# ---- C ABI ---------------------------------------------------------------------------------------------
def test_symbol_struct_and_prototype(hiplib, policy):
    from smoothed_particle_hydrodynamics_amd import lib as L
    assert hasattr(hiplib, "sph_hip_render_scalars")
    out = (C.c_longlong * 13)()
    policy.layout(out)
    assert list(out) == [24, 0, 4, 8, 12, 16, 20, 7, 0, 1, 1, 256, 768]
    S = L.SphTintParams
    assert C.sizeof(S) == 24 and [getattr(S, f).offset for f, _ in S._fields_] == [0, 4, 8, 12, 16, 20]
    assert [f for f, _ in S._fields_] == ["channel", "mode", "lo", "hi", "n_colors", "flags"]
    assert header_prototype("sph_hip_render_scalars") == [
        "sph_hip_context* ctx", "const sph_hip_camera* cam", "const sph_hip_render_params* rp",
        "const sph_hip_scene_params* sp", "const float* solid_albedo_rgb", "int n_albedo",
        "const sph_hip_tint_params* tp", "const float* table_rgb", "int width", "int height", "int flags",
        "uint8_t* rgba", "float* depth", "float* normal_xyz", "float* velocity_xyz", "int32_t* first_inside",
        "int32_t* solid_id", "float* scalar"]
    res, args = L.PROTOTYPES["sph_hip_render_scalars"]
    V, I = C.c_void_p, C.c_int
    assert res is I and len(args) == 18 and args[0] is V
    assert [a._type_ for a in (args[1], args[2], args[3], args[6])] == [L.SphCamera, L.SphRenderParams,
                                                                        L.SphSceneParams, S]
    assert args[4] is V and args[5] is I and args[7] is V and args[8:11] == [I] * 3 and args[11:] == [V] * 7
    text = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    assert re.search(r"#define SPH_HIP_ABI_VERSION 7\b", text) and L.ABI_VERSION == 7
    section = text[text.index("---- scalar renderer"):text.index("int sph_hip_render_scalars(")]
    for word in ("SURFACE", "COLUMN", "map", "shade", "Solids do NOT", "SPH_HIP_RENDER_NOSKIP"):
        assert word in section, word
    # the scene renderer's struct and prototype stand as they were
    assert C.sizeof(L.SphSceneParams) == 20 and len(L.PROTOTYPES["sph_hip_render_scene"][1]) == 15
    assert len(L.PROTOTYPES["sph_hip_render"][1]) == 11


# ---- refusals ---------------------------------------------------------------------------------------------
def tint_params(**kw):
    from smoothed_particle_hydrodynamics_amd.lib import SphTintParams
    tp = SphTintParams(0, 0, 0.0, 1.0, 2, 0)
    for k, v in kw.items():
        setattr(tp, k, v)
    return tp


def test_every_refusal_text(policy):
    from smoothed_particle_hydrodynamics_amd.lib import SphSceneParams
    cam, rp = good()
    sp = SphSceneParams()
    sp.albedo[:] = [0.7, 0.7, 0.7]
    sp.ambient, sp.diffuse = 0.2, 0.8
    table = np.array([[0, 0, 0], [1, 1, 1]], F32)
    alb = np.zeros((2, 3), F32)

    def check(cam_=cam, rp_=rp, sp_=sp, albedo=None, n_albedo=0, n_obst=2, n_scalars=100, tp=None, table_=table, w=64,
              h=48, flags=0, null_tp=False):
        tp = tint_params() if tp is None else tp
        ref = lambda s: None if s is None else C.byref(s)
        return policy.check(ref(cam_), ref(rp_), ref(sp_), None if albedo is None else ptr(albedo), n_albedo, n_obst,
                            n_scalars, None if null_tp else C.byref(tp), None if table_ is None else ptr(table_), w, h,
                            flags).decode()

    assert check() == "" and check(sp_=None) == "" and check(albedo=alb, n_albedo=2) == ""
    assert check(flags=1) == "" and check(sp_=None, flags=1) == ""
    assert check(tp=tint_params(channel=3, mode=1, n_colors=256, flags=1),
                 table_=np.zeros((256, 3), F32)) == ""
    # the scene renderer's refusals, with scene params and without
    for sp_ in (sp, None):
        assert check(sp_=sp_, flags=2) == "flag bits other than SPH_HIP_RENDER_VELOCITY"
        assert check(sp_=sp_, cam_=None) == "null camera or render params"
        assert check(sp_=sp_, w=0) == "width and height must be in [1, 16384]"
        bad = type(rp).from_buffer_copy(rp)
        bad.step = 0.0
        assert check(sp_=sp_, rp_=bad) == "step must be > 0"
    bad_sp = SphSceneParams.from_buffer_copy(sp)
    bad_sp.ambient = float("nan")
    assert check(sp_=bad_sp) == "scene params must be finite"
    assert check(albedo=alb, n_albedo=1) == "the albedo count must be 0 or the obstacle count"
    assert check(n_albedo=2) == "null albedo array"
    # ... and this entry point's own
    assert check(sp_=None, albedo=alb) == "solid albedos without scene params"
    assert check(sp_=None, n_albedo=2) == "solid albedos without scene params"
    assert check(n_scalars=0) == "the context carries no scalars"
    assert check(null_tp=True) == "null tint params or colour table"
    assert check(table_=None) == "null tint params or colour table"
    for ch in (-1, 4):
        assert check(tp=tint_params(channel=ch)) == "channel must be 0 .. 3"
    for mode in (-1, 2):
        assert check(tp=tint_params(mode=mode)) == "unknown tint mode"
    assert check(tp=tint_params(flags=2)) == "unknown tint flag bits"
    for n in (1, 0, -3, 257):
        assert check(tp=tint_params(n_colors=n)) == "n_colors must be in [2, 256]"
    for kw in ({"lo": float("nan")}, {"hi": float("inf")}, {"lo": float("-inf")}):
        assert check(tp=tint_params(**kw)) == "tint range must be finite"
    for lo, hi in ((1.0, 1.0), (2.0, 1.0)):
        assert check(tp=tint_params(lo=lo, hi=hi)) == "tint range needs lo < hi"
    for v in (np.nan, np.inf, -np.inf):
        t = table.copy()
        t[1, 2] = v
        assert check(table_=t) == "a colour table entry that is not finite"
    # an entry beyond n_colors rows is not read
    t = np.array([[0, 0, 0], [1, 1, 1], [np.nan, 0, 0]], F32)
    assert check(table_=t) == ""
    # the order: the scene's checks, the scalars, then the tint's
    assert check(flags=2, n_scalars=0) == "flag bits other than SPH_HIP_RENDER_VELOCITY"
    assert check(n_scalars=0, null_tp=True) == "the context carries no scalars"


# ---- the map ---------------------------------------------------------------------------------------------
DIRECTED = [F32(-0.25), F32(1.75), F32(-3.0), F32(9.0), F32(np.nan), F32(np.inf), F32(-np.inf), F32(-0.0), F32(0.0),
            F32(0.75), np.nextafter(F32(1.75), F32(0)), np.nextafter(F32(-0.25), F32(0))]
LO, HI = F32(-0.25), F32(1.75)


@pytest.mark.parametrize("rows", [2, 3, 17, 256])
def test_map_equals_the_restatement(policy, rows):
    rng = np.random.default_rng(100 + rows)
    for wild in (False, True):
        table = seeded_table(rng, rows, wild)
        v = np.concatenate([rng.uniform(-1.0, 2.5, 20000).astype(F32), np.array(DIRECTED, F32)])
        got, want = c_map(policy, v, LO, HI, table), TE.color_map(v, LO, HI, table)
        assert_same(got, want, "map %d rows wild=%s" % (rows, wild))
        d = len(DIRECTED)
        assert_same(got[-d:-d + 1], table[:1], "exactly lo")
        # (the high end is row n - 2 with fr = 1: t[n-2] + 1.0f * (t[n-1] - t[n-2]), the last row to a rounding)
        top = (table[-2] + F32(1.0) * (table[-1] - table[-2])).astype(F32)[None, :]
        assert np.abs(top - table[-1:]).max() <= 2.0 ** -22 * np.abs(table).max()
        assert_same(got[-d + 1:-d + 2], top, "exactly hi")
        assert_same(got[-d + 2:-d + 3], table[:1], "below")
        assert_same(got[-d + 3:-d + 4], top, "above")
        assert_same(got[-d + 4:-d + 5], table[:1], "NaN lands on row 0")
        assert_same(got[-d + 5:-d + 6], top, "+inf")
        assert_same(got[-d + 6:-d + 7], table[:1], "-inf")
        assert np.isfinite(got).all()


def test_map_lands_on_every_interior_row(policy):
    table = seeded_table(np.random.default_rng(5), 5, wild=True)
    v = np.array([0.0, 0.25, 0.5, 0.75, 1.0], F32)       # u * 4 is exactly the row
    got = c_map(policy, v, 0.0, 1.0, table)
    assert_same(got[:4], table[:4], "rows of a 5-row table")          # fr = 0: the row itself
    assert_same(got[4:], (table[3] + F32(1.0) * (table[4] - table[3])).astype(F32)[None, :], "the last row")
    assert_same(got, TE.color_map(v, 0.0, 1.0, table), "rows of a 5-row table, restatement")
    mid = c_map(policy, np.array([0.125], F32), 0.0, 1.0, table)
    assert_same(mid, (table[0] + F32(0.5) * (table[1] - table[0]))[None, :].astype(F32), "half way")


# ---- the shade ---------------------------------------------------------------------------------------------
def test_shade_equals_the_restatement(policy):
    rng = np.random.default_rng(9)
    n = 20000
    normal = rng.normal(size=(n, 3)).astype(F32)
    normal /= np.linalg.norm(normal, axis=1, keepdims=True).astype(F32)
    normal[:50] = 0.0                                       # a hit without a gradient
    col = rng.uniform(-0.8, 2.5, (n, 3)).astype(F32)
    light = np.array([0.4, 0.8, 0.45], F32)
    w = np.zeros(n, F32)
    policy.weight_many(ptr(normal), n, ptr(light), 0.2, 0.8, ptr(w))
    want_w = TE.weight(normal, light, 0.2, 0.8)
    assert np.array_equal(bits(w), bits(want_w))
    for flat, ww in ((False, w), (True, np.ones(n, F32))):
        rgba = np.zeros(n, np.uint32)
        policy.pixel_many(ptr(col), ptr(ww), n, ptr(rgba))
        want = TE.pixel(col, ww)
        assert np.array_equal(rgba.view(np.uint8).reshape(n, 4), want), flat
        assert (want[:, 3] == 255).all() and (want[:, :3] == 0).any() and (want[:, :3] == 255).any()
    # the renderer's own formula: a table of two equal rows gives render's byte of albedo * w
    alb = np.array([0.25, 0.55, 0.9], F32)
    col = np.tile(alb, (n, 1))
    rgba = np.zeros(n, np.uint32)
    policy.pixel_many(ptr(col), ptr(w), n, ptr(rgba))
    for c in range(3):
        assert np.array_equal(rgba.view(np.uint8).reshape(n, 4)[:, c], E.quantise(alb[c] * want_w))


# ---- the column's accumulation ----------------------------------------------------------------------------------
def test_column_accumulation_on_scripted_sequences(policy):
    iso, step = F32(2.0), F32(0.0125)
    nan = F32(np.nan)
    cases = {
        "outside between inside": ([3.0, 1.0, 0.0, 4.0, 2.5], [1.5, 9.0, 9.0, -2.0, 2.5]),
        "rho exactly iso is outside": ([2.0, 2.0, 3.0], [7.0, 7.0, 3.0]),
        "a NaN rho is outside": ([nan, 3.0, nan], [1.0, 6.0, 1.0]),
        "first_inside is the last sample": ([5.0], [2.5]),
        "nothing inside": ([0.0, 1.0], [4.0, 4.0]),
        "empty": ([], []),
    }
    want_by_hand = {"rho exactly iso is outside": F32(F32(3.0) / F32(3.0)) * step,
                    "a NaN rho is outside": F32(F32(6.0) / F32(3.0)) * step,
                    "first_inside is the last sample": F32(F32(2.5) / F32(5.0)) * step,
                    "nothing inside": F32(0.0), "empty": F32(0.0)}
    for name, (rho, a) in cases.items():
        rho, a = np.array(rho, F32), np.array(a, F32)
        got = F32(policy.column_sequence(ptr(rho), ptr(a), rho.size, iso, step))
        want = TE.column_sequence(rho, a, iso, step)
        assert bits(got) == bits(want), (name, got, want)
        if name in want_by_hand:
            assert bits(got) == bits(F32(want_by_hand[name])), name
    rng = np.random.default_rng(3)
    rho = rng.uniform(0.0, 4.0, 500).astype(F32)
    a = (rho * rng.uniform(-1.0, 1.0, 500).astype(F32)).astype(F32)
    got = F32(policy.column_sequence(ptr(rho), ptr(a), 500, iso, step))
    assert bits(got) == bits(TE.column_sequence(rho, a, iso, step)) and got != 0


# ---- decisions --------------------------------------------------------------------------------------------------
def test_scratch_and_launch_decisions(policy):
    assert policy.scalar_bytes(64, 48) == 64 * 48 * 4 and policy.scalar_bytes(13, 7) == 512
    assert policy.scalar_bytes(16384, 96) == 16384 * 96 * 4 and policy.scalar_bytes(1, 1) == 256
    assert [policy.launches_tint(h, n) for h, n in ((1, 100), (1, 0), (0, 100), (0, 0))] == [1, 0, 0, 0]
    # unchanged beside it
    assert [policy.launches_scalars(s, n) for s, n in ((5, 5), (0, 5), (5, 0))] == [1, 0, 0]
    assert policy.id_bytes(13, 7) == 512 and policy.pixel_bytes() == 40
    assert policy.chunk_rows(16384, 104) == 96 and policy.chunk_rows(64, 48) == 48
    assert policy.scratch_bytes(64, 48) == 64 * 48 * 40 + 256


# ---- the directed cases under the sanitizers -------------------------------------------------------------------
MAIN = CALLS + r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
int main()
{
   const float nan = nanf(""), inf = INFINITY;
   const float values[] = {-0.25f, 1.75f, -3.0f, 9.0f, nan, inf, -inf, -0.0f, 0.0f, 0.75f};
   const int nv = (int)(sizeof(values) / sizeof(values[0]));
   const int rows[] = {2, 3, 17, 256};
   int checked = 0;
   for (int r = 0; r < 4; r++) {
      // exactly 3 * rows floats on the heap: a read past the table is an error
      float* table = (float*)malloc(sizeof(float) * 3 * rows[r]);
      for (int i = 0; i < 3 * rows[r]; i++) table[i] = (float)(i % 7) * 0.4f - 0.5f;
      float* col = (float*)malloc(sizeof(float) * 3 * nv);
      float* w = (float*)malloc(sizeof(float) * nv);
      unsigned* rgba = (unsigned*)malloc(sizeof(unsigned) * nv);
      map_many(values, nv, -0.25f, 1.75f, rows[r], table, col);
      const float light[3] = {0.4f, 0.8f, 0.45f};
      weight_many(col, nv, light, 0.2f, 0.8f, w);
      pixel_many(col, w, nv, rgba);
      for (int i = 0; i < nv; i++) checked += (rgba[i] >> 24) == 255u;
      sph_hip_tint_params tp = {0, 0, -0.25f, 1.75f, rows[r], 0};
      sph_hip_camera cam;
      sph_hip_render_params rp;
      memset(&cam, 0, sizeof(cam));
      memset(&rp, 0, sizeof(rp));
      if (strcmp(check(&cam, &rp, NULL, NULL, 0, 0, 10, &tp, table, 8, 8, 0), "step must be > 0")) return 3;
      free(table); free(col); free(w); free(rgba);
   }
   const float rho[] = {3.0f, 1.0f, 2.0f, nan, 4.0f}, a[] = {1.5f, 9.0f, 9.0f, 1.0f, -3.0f};
   const float A = column_sequence(rho, a, 5, 2.0f, 0.0125f);
   const float one[] = {5.0f}, a1[] = {2.5f};
   const float B = column_sequence(one, a1, 1, 2.0f, 0.0125f);
   printf("checked %d A %a B %a\n", checked, A, B);
   return 0;
}
"""


def test_directed_cases_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    src, exe = tmp_path / "tint_main.cpp", tmp_path / "tint_main"
    src.write_text(MAIN)
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    step = F32(0.0125)
    A = TE.column_sequence([3.0, 1.0, 2.0, np.nan, 4.0], [1.5, 9.0, 9.0, 1.0, -3.0], 2.0, step)
    B = TE.column_sequence([5.0], [2.5], 2.0, step)
    words = run.stdout.split()
    assert words[:3] == ["checked", "40", "A"] and words[4] == "B", run.stdout
    assert float.fromhex(words[3]) == float(A) != 0.0 and float.fromhex(words[5]) == float(B) != 0.0, run.stdout


# ---- the restatement on an analytic case -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lattice(hiplib):
    """16^3 particles at rest on a cubic lattice filling [0, 0.5]^3, and an axis-aligned view down -z"""
    from smoothed_particle_hydrodynamics_amd import Camera, scenes
    from smoothed_particle_hydrodynamics_amd.lib import SphRenderParams
    m = 16
    p, _, _, mass = scenes.dam_break(m ** 3, fill=(0.5, 0.5, 0.5))
    s = 0.5 / m
    ax = (np.arange(m) + 0.5) * s
    pos = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3).astype(F32)
    vel = np.zeros_like(pos)
    h = float(p.h)
    W, H = 9, 7
    cam = Camera((0.25, 0.25, 2.5), (0.0, 0.0, -1.0), (0.03, 0, 0), (0, 0.03 * H / W, 0))
    rp = SphRenderParams()
    rp.box_lo[:] = [-h, -h, -h]
    rp.box_hi[:] = [float(p.max_x) + h, float(p.max_y) + h, float(p.max_z) + h]
    rp.step = rp.grad_step = float(F32(0.5) * F32(h))
    rp.refine = 8
    rp.light[:] = [0.4, 0.8, 0.45]
    rp.albedo[:] = [0.25, 0.55, 0.9]
    rp.ambient, rp.diffuse = 0.2, 0.8
    rp.background[:] = [0, 0, 0, 255]
    rp.max_samples = 1 << 16
    return p, pos, vel, mass, cam, rp, W, H


def lattice_frames(lattice, value):
    p, pos, vel, mass, cam, rp, W, H = lattice
    T = np.zeros((pos.shape[0], 4), F32)
    T[:, 2] = F32(value)
    walk = TE.Walk(p, pos, vel, mass, T)
    rho = walk.density(pos)
    rp.iso = float(F32(0.5) * np.median(rho))
    fluid = E.render(walk.density, cam, rp, W, H)
    table = np.array([[0, 0, 1], [1, 0, 0]], F32)
    out = {}
    for mode in (TE.SURFACE, TE.COLUMN):
        out[mode] = TE.tint(fluid, walk, cam, rp, TE.Tint(2, mode, 0.0, 1.0, TE.FLAT), table, W, H)
    return walk, fluid, out


def test_restatement_on_a_lattice_with_the_channel_one(lattice):
    """A check of the restatement (tests/tint_emulation.py), not of the library: analytic values on a rest lattice."""
    p, pos, vel, mass, cam, rp, W, H = lattice
    walk, fluid, out = lattice_frames(lattice, 1.0)
    hit = fluid.first_inside >= 0
    assert hit.sum() == W * H                       # the view lies inside the block's footprint
    # t * 1.0f is t: the channel's sum is rho bit for bit, and the quotient exactly 1
    assert (out[TE.SURFACE].scalar[hit] == 1.0).all()
    assert (out[TE.SURFACE].rgba[hit] == [255, 0, 0, 255]).all()
    # the column: step accumulated once per inside sample
    py, px = np.divmod(np.arange(W * H), W)
    A, count = TE.column(walk, cam, rp, W, H, px, py, fluid.first_inside, 2)
    assert np.array_equal(bits(A), bits(out[TE.COLUMN].scalar))
    step = F32(rp.step)
    for i in range(W * H):
        acc = F32(0.0)
        for _ in range(int(count[i])):
            acc = F32(acc + step)
        assert bits(acc) == bits(A[i]), i
    # ... and that is the block's chord along the ray: test_gpu_render.py's bound for one face (h) on both
    # faces, plus one step
    d, _ = E.pixel_rays(cam, W, H, px, py)
    d = d.astype(np.float64)
    e = np.array([float(v) for v in cam.eye], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (0.0 - e) / d, (0.5 - e) / d
    chord = np.nanmin(np.maximum(t0, t1), 1) - np.nanmax(np.minimum(t0, t1), 1)
    assert (chord > 0.49).all()
    h = float(p.h)
    err = np.abs(A.astype(np.float64) - chord)
    print("chord %.4f .. %.4f, column %.4f .. %.4f, worst error %.4f of %.4f allowed" % (
        chord.min(), chord.max(), A.min(), A.max(), err.max(), 2 * h + float(step)))
    assert err.max() <= 2 * h + float(step)


def test_restatement_on_a_lattice_with_a_uniform_channel(lattice):
    """A check of the restatement (tests/tint_emulation.py), not of the library: the Shepard value's rounding bound."""
    p, pos, vel, mass, cam, rp, W, H = lattice
    walk, fluid, out = lattice_frames(lattice, 0.75)
    hit = np.flatnonzero(fluid.first_inside >= 0)
    py, px = np.divmod(hit, W)
    d, _ = E.pixel_rays(cam, W, H, px, py)
    _, _, count = walk(E.point_at(E._v(cam.eye), fluid.depth[hit], d), 2)
    v = out[TE.SURFACE].scalar[hit].astype(np.float64)
    # one rounding per product, per add and for the division
    bound = (count.astype(np.float64) + 2.0) * 2.0 ** -23
    assert (count > 0).all() and (np.abs(v - 0.75) / 0.75 <= bound).all(), np.abs(v / 0.75 - 1).max()


# ---- colour tables --------------------------------------------------------------------------------------------------
def test_colormaps():
    from smoothed_particle_hydrodynamics_amd import colormaps as CM
    for make, first, last in ((CM.heat, (0, 0, 0), (1, 1, 1)), (CM.gray, (0, 0, 0), (1, 1, 1)),
                              (CM.diverging, (0.23, 0.30, 0.75), (0.70, 0.02, 0.15))):
        for n in (2, 3, 17, 256):
            t = make(n)
            assert t.shape == (n, 3) and t.dtype == np.float32 and np.isfinite(t).all()
            assert np.array_equal(t[0], np.array(first, F32)) and np.array_equal(t[-1], np.array(last, F32))
            assert t.min() >= 0 and t.max() <= 1
        assert make().shape == (256, 3)
    assert np.array_equal(CM.diverging(3)[1], np.ones(3, F32))
    t = CM.dye((0.9, 0.1, 0.2))
    assert t.shape == (2, 3) and t.dtype == np.float32
    assert np.array_equal(t, np.array([(0.25, 0.55, 0.9), (0.9, 0.1, 0.2)], F32))
    t = CM.dye((1, 0, 0), water=(0, 0, 1), n=5)
    assert t.shape == (5, 3) and np.array_equal(t[2], np.array([0.5, 0, 0.5], F32))
    for bad in (1, 0, 257):
        with pytest.raises(ValueError):
            CM.heat(bad)


# ---- renderScalars' argument handling ---------------------------------------------------------------------------------
class Recorder:
    """an SPH whose calls into the library are recorded, not made"""

    def __new__(cls):
        from smoothed_particle_hydrodynamics_amd import SPH, default_params

        class Fake(SPH):
            def __init__(self):
                self._params = default_params(1000)
                self.calls = []

            def call(self, name, *args):
                self.calls.append((name, args))
                return 0

            def getParticleBounds(self):
                return (1.0, 1.0, 1.0)

            def __del__(self):
                pass

        return Fake()


def struct_bytes(arg):
    return bytes(arg._obj) if hasattr(arg, "_obj") else arg


def test_render_scalars_argument_handling(hiplib):
    from smoothed_particle_hydrodynamics_amd import Camera, ScalarRenderResult, colormaps
    from smoothed_particle_hydrodynamics_amd.lib import SphTintParams
    cam = Camera.look_at((0.5, 0.5, 3.0), (0.5, 0.5, 0.5), (0, 1, 0), 40, 20, 10)
    sph = Recorder()
    common = dict(step=0.01, refine=3, box=((0, 0, 0), (1, 2, 3)), light=(0, 1, 0), ambient=0.3, diffuse=0.6,
                  background=(1, 2, 3, 4), max_samples=77, velocity=True)
    plain = sph.render(cam, 20, 10, 1.5, **common)
    tinted = sph.renderScalars(cam, 20, 10, 1.5, 2, (-1.0, 3.0), **common)
    (n0, a0), (n1, a1) = sph.calls
    assert n0 == "sph_hip_render" and n1 == "sph_hip_render_scalars"
    # camera, params, size and flags are render's
    assert struct_bytes(a0[0]) == struct_bytes(a1[0]) and struct_bytes(a0[1]) == struct_bytes(a1[1])
    assert a0[2:5] == (20, 10, 1) and a1[7:10] == (20, 10, 1)
    assert a1[2] is None and a1[3] is None and a1[4] == 0
    tp = a1[5]._obj
    assert isinstance(tp, SphTintParams)
    assert (tp.channel, tp.mode, tp.lo, tp.hi, tp.n_colors, tp.flags) == (2, 0, -1.0, 3.0, 256, 0)
    assert isinstance(tinted, ScalarRenderResult) and tinted._fields == plain._fields + ("scalar",)
    assert tinted.scalar.shape == (10, 20) and tinted.scalar.dtype == np.float32 and tinted.solid_id is None
    for f in ("rgba", "depth", "normal", "velocity", "first_inside"):
        assert getattr(tinted, f).shape == getattr(plain, f).shape and getattr(tinted, f).dtype == getattr(plain, f).dtype
    # column, flat, a table of its own, solids
    sph.calls.clear()
    scene = sph.render(cam, 20, 10, 1.5, solids=True, solid_colors=[(1, 0, 0)], solid_ambient=0.5)
    tinted = sph.renderScalars(cam, 20, 10, 1.5, 0, (0, 1), colormap=colormaps.dye((1, 0, 0)), mode="column", flat=True,
                               solids=True, solid_colors=[(1, 0, 0)], solid_ambient=0.5)
    (n0, a0), (n1, a1) = sph.calls
    assert n0 == "sph_hip_render_scene" and n1 == "sph_hip_render_scalars"
    assert struct_bytes(a0[2]) == struct_bytes(a1[2]) and a0[4] == a1[4] == 1      # scene params, albedo count
    tp = a1[5]._obj
    assert (tp.channel, tp.mode, tp.n_colors, tp.flags) == (0, 1, 2, 1)
    assert tinted.velocity is None and tinted.solid_id.shape == scene.solid_id.shape == (10, 20)
    with pytest.raises(ValueError):
        sph.renderScalars(cam, 20, 10, 1.5, 0, (0, 1), mode="volume")
    with pytest.raises(ValueError):
        sph.renderScalars(cam, 0, 10, 1.5, 0, (0, 1))
    with pytest.raises(ValueError):
        sph.renderScalars(cam, 20, 10, 1.5, 0, (0, 1), colormap=np.zeros((4, 4)))


def test_dyed_cut_box(hiplib):
    from smoothed_particle_hydrodynamics_amd import scenes
    p = scenes.dam_break_dyed(1000)[0]
    lo, hi = scenes.dyed_cut_box(p)
    h = F32(p.h)
    assert lo.dtype == hi.dtype == np.float32 and (lo == F32(0) - h).all()
    assert hi[0] == F32(p.max_x) + h and hi[1] == F32(p.max_y) + h and hi[2] == F32(0.5) * F32(p.max_z)
