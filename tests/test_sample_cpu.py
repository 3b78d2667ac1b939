"""CPU checks of the field sampler (include/sph_hip.h: sph_hip_sample_points / _lattice): the C ABI
and its binding, the refusals that need no device, the launch decisions of csrc/sample_policy.h
(compiled with g++ behind an extern "C" shim, as tests/test_launch_policy.py does), and the numpy
emulation the GPU tests check against (tests/sample_emulation.py), against a float64 brute force."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sample_emulation as E
from helpers import compile_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = -1

SHIM = r"""
#include "sample_policy.h"

extern "C" {
int threads() { return SAMPLE_THREADS; }
int n_bricks() { return SAMPLE_N_BRICKS; }
void brick_table(int i, int* out) { out[0] = SAMPLE_BRICKS[i].bx; out[1] = SAMPLE_BRICKS[i].by; out[2] = SAMPLE_BRICKS[i].bz; }
int tile_cap() { return SAMPLE_TILE_CAP; }
int tile_bytes(int vel) { return vel ? SAMPLE_TILE_BYTES_VELOCITY : SAMPLE_TILE_BYTES_DENSITY; }
int cell_budget() { return SAMPLE_CELL_BUDGET; }
int chunk_points() { return SAMPLE_CHUNK_POINTS; }
int max_rows() { return SAMPLE_MAX_ROWS; }
int tile_cells_axis(int points, double spacing) { return sample_tile_cells_axis(points, spacing); }
long long brick_of(const int* dims, const double* spacing, int* out)
{
   const SampleBrick b = sample_brick(dims, spacing);
   out[0] = b.bx; out[1] = b.by; out[2] = b.bz;
   return sample_tile_cells(b, dims, spacing);
}
int route(int which) { const int v[] = {SAMPLE_ROUTE_DEFAULT, SAMPLE_ROUTE_UNTILED, SAMPLE_ROUTE_TILED}; return v[which]; }
int use_tiled(const int* dims, const double* spacing, int cap, int route_switch)
{
   return sample_use_tiled(sample_brick(dims, spacing), dims, spacing, cap, route_switch) ? 1 : 0;
}
void lattice_chunk(const int* dims, const int* brick, long long max_points, int* out)
{
   const SampleBrick b = {brick[0], brick[1], brick[2]};
   const SampleChunk c = sample_lattice_chunk(dims, b, max_points);
   out[0] = c.ex; out[1] = c.ey; out[2] = c.ez;
}
int points_chunk(int n, int max_points) { return sample_points_chunk(n, max_points); }
int chunk_forced(long long value) { return sample_chunk_forced(value); }
int chunk_limit(int limit, int forced) { return sample_chunk_limit(limit, forced); }
long long budget() { return SAMPLE_SCRATCH_BUDGET; }
const char* check(const float* origin, const float* spacing, const int32_t* dims)
{
   const char* why = lattice_check(origin, spacing, dims);
   return why ? why : "";
}
}
"""

@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    lib = compile_shim(SHIM, ["-O1"], tmp_path_factory)
    lib.use_tiled.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int, C.c_int]
    lib.lattice_chunk.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_longlong, C.POINTER(C.c_int)]
    lib.tile_cells_axis.argtypes = [C.c_int, C.c_double]
    lib.brick_of.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int)]
    lib.brick_of.restype = C.c_longlong
    lib.budget.restype = C.c_longlong
    lib.chunk_forced.argtypes = [C.c_longlong]
    lib.check.argtypes = [C.c_void_p] * 3
    lib.check.restype = C.c_char_p
    return lib


DEFAULT, UNTILED, TILED = 0, 1, 2   # the route switch: none, SPH_HIP_SAMPLE_UNTILED=1, SPH_HIP_SAMPLE_TILED=1


def tiled(policy, dims, spacing, switch=TILED, cap=None):
    """1 where sample_policy.h sends the lattice through the LDS tile under the given switch"""
    d = (C.c_int * 3)(*dims)
    s = (C.c_double * 3)(*spacing)
    return policy.use_tiled(d, s, policy.tile_cap() if cap is None else cap, policy.route(switch))


def brick(policy, dims, spacing):
    """(brick shape, its worst-case tile cells) sample_policy.h chooses for the lattice"""
    out = (C.c_int * 3)()
    cells = policy.brick_of((C.c_int * 3)(*dims), (C.c_double * 3)(*spacing), out)
    return tuple(out), cells


def chunk(policy, dims, most, shape=(8, 8, 4)):
    out = (C.c_int * 3)()
    policy.lattice_chunk((C.c_int * 3)(*dims), (C.c_int * 3)(*shape), most, out)
    return tuple(out)


def forced_chunks(policy, dims, cells):
    """Three values of SPH_HIP_SAMPLE_CHUNK for the lattice `dims` (spacing `cells` cell edges): the chunks of
    the first cut the lattice along z only (whole planes), those of the second along y as well (whole
    x-rows), those of the third along x too - one layer, one row, one single brick at a time.  The shapes
    are asserted here on sample_lattice_chunk, and that the clamp leaves the values alone."""
    nx, ny, nz = dims
    shape, _ = brick(policy, dims, cells)
    bx, by, bz = shape
    assert bx < nx and by < ny and bz < nz, "the lattice must exceed its brick %r along every axis" % (shape,)
    values = (nx * ny * bz, nx * bz * by, bx * by * bz)
    cut_z, cut_y, cut_x = (chunk(policy, dims, v, shape) for v in values)
    assert cut_z == (nx, ny, bz)
    assert cut_y == (nx, by, bz)
    assert cut_x == (bx, by, bz)
    for v in values:
        assert policy.chunk_forced(v) == v
    return values


# ---- C ABI -------------------------------------------------------------------------------------
def header_prototype(name):
    text = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_sampler_symbols_are_exported(hiplib):
    for name in ("sph_hip_sample_points", "sph_hip_sample_lattice"):
        assert hasattr(hiplib, name)


def test_sampler_prototypes_match_the_header():
    from smoothed_particle_hydrodynamics_amd.lib import PROTOTYPES
    P = C.POINTER
    pts = header_prototype("sph_hip_sample_points")
    assert pts == ["sph_hip_context* ctx", "int n", "const float* xyz", "float* density", "float* velocity_xyz",
                   "int32_t* count"]
    assert PROTOTYPES["sph_hip_sample_points"] == (
        C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
    lat = header_prototype("sph_hip_sample_lattice")
    assert lat == ["sph_hip_context* ctx", "const float origin[3]", "const float spacing[3]",
                   "const int32_t dims[3]", "float* density", "float* velocity_xyz", "int32_t* count"]
    restype, args = PROTOTYPES["sph_hip_sample_lattice"]
    assert restype is C.c_int and len(args) == 7
    assert args[0] is C.c_void_p and args[4:] == [C.c_void_p] * 3
    assert args[1] == P(C.c_float * 3) and args[2] == P(C.c_float * 3) and args[3] == P(C.c_int32 * 3)


def test_abi_version_is_seven(hiplib):
    from smoothed_particle_hydrodynamics_amd import lib as L
    assert L.ABI_VERSION == 7 == hiplib.sph_hip_abi_version()


def lattice_args(origin=(0.0, 0.0, 0.0), spacing=(0.1, 0.1, 0.1), dims=(4, 4, 4)):
    return (C.byref((C.c_float * 3)(*origin)), C.byref((C.c_float * 3)(*spacing)),
            C.byref((C.c_int32 * 3)(*dims)))


@pytest.mark.parametrize("n", [0, 1, -1])
def test_sample_points_refuses_a_null_context(hiplib, n):
    xyz = np.zeros(3, np.float32)
    assert hiplib.sph_hip_sample_points(None, n, xyz.ctypes.data_as(C.c_void_p), None, None, None) == ERR_INVALID
    assert hiplib.sph_hip_sample_points(None, n, None, None, None, None) == ERR_INVALID


@pytest.mark.parametrize("origin,spacing,dims", [
    ((0.0, 0.0, 0.0), (0.1, 0.1, 0.1), (4, 4, 4)),                 # only the NULL context is wrong
    ((0.0, 0.0, 0.0), (0.1, 0.1, 0.1), (0, 4, 4)),
    ((0.0, 0.0, 0.0), (0.1, 0.1, 0.1), (4, -1, 4)),
    ((float("nan"), 0.0, 0.0), (0.1, 0.1, 0.1), (4, 4, 4)),
    ((0.0, float("inf"), 0.0), (0.1, 0.1, 0.1), (4, 4, 4)),
    ((0.0, 0.0, 0.0), (0.0, 0.1, 0.1), (4, 4, 4)),
    ((0.0, 0.0, 0.0), (0.1, -0.1, 0.1), (4, 4, 4)),
    ((0.0, 0.0, 0.0), (0.1, 0.1, float("nan")), (4, 4, 4)),
    ((0.0, 0.0, 0.0), (0.1, 0.1, float("inf")), (4, 4, 4)),
    ((0.0, 0.0, 0.0), (0.1, 0.1, 0.1), (2048, 1024, 1024)),        # 2^31 points
])
def test_sample_lattice_refuses_a_null_context_and_bad_arguments(hiplib, origin, spacing, dims):
    assert hiplib.sph_hip_sample_lattice(None, *lattice_args(origin, spacing, dims), None, None, None) == ERR_INVALID


def test_sample_lattice_refuses_null_arrays(hiplib):
    assert hiplib.sph_hip_sample_lattice(None, None, None, None, None, None, None) == ERR_INVALID


# ---- lattice argument checks (csrc/sample_policy.h: lattice_check, sph_hip_sample_lattice and
# sph_hip_extract_surface) --------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
BAD_LATTICE = "dims must be positive, the origin finite, the spacing finite and positive"
TOO_MANY = "more than 2^31 - 1 lattice points"


def lattice_refusal(policy, origin=(0.0, 0.0, 0.0), spacing=(0.1, 0.1, 0.1), dims=(4, 4, 4)):
    """lattice_check's reason, "" where the lattice is accepted; None stands for a null array"""
    arrays = [None if v is None else C.cast((t * 3)(*v), C.c_void_p)
              for t, v in ((C.c_float, origin), (C.c_float, spacing), (C.c_int32, dims))]
    return policy.check(*arrays).decode()


@pytest.mark.parametrize("origin,spacing,dims,why", [
    # the cases test_sample_lattice_refuses_a_null_context_and_bad_arguments and
    # test_gpu_surface.py::test_bad_arguments_are_refused list
    ((0.0, 0.0, 0.0), (0.1, 0.1, 0.1), (0, 4, 4), BAD_LATTICE),
    ((0.0, 0.0, 0.0), (0.1, 0.1, 0.1), (4, -1, 4), BAD_LATTICE),
    ((0.0, 0.0, 0.0), (0.1, 0.1, 0.1), (2, 2, 0), BAD_LATTICE),
    ((NAN, 0.0, 0.0), (0.1, 0.1, 0.1), (4, 4, 4), BAD_LATTICE),
    ((0.0, INF, 0.0), (0.1, 0.1, 0.1), (4, 4, 4), BAD_LATTICE),
    ((0.0, 0.0, -INF), (0.1, 0.1, 0.1), (4, 4, 4), BAD_LATTICE),
    ((0.0, 0.0, 0.0), (0.0, 0.1, 0.1), (4, 4, 4), BAD_LATTICE),
    ((0.0, 0.0, 0.0), (0.1, -0.0, 0.1), (4, 4, 4), BAD_LATTICE),
    ((0.0, 0.0, 0.0), (0.1, -0.1, 0.1), (4, 4, 4), BAD_LATTICE),
    ((0.0, 0.0, 0.0), (0.1, 0.1, NAN), (4, 4, 4), BAD_LATTICE),
    ((0.0, 0.0, 0.0), (NAN, 0.1, 0.1), (4, 4, 4), BAD_LATTICE),
    ((0.0, 0.0, 0.0), (0.1, 0.1, INF), (4, 4, 4), BAD_LATTICE),
    ((0.0, 0.0, 0.0), (0.1, 0.1, 0.1), (2048, 1024, 1024), TOO_MANY),     # 2^31 points
    ((0.0, 0.0, 0.0), (0.1, 0.1, 0.1), (2 ** 31 - 1, 2, 1), TOO_MANY),
    ((0.0, 0.0, 0.0), (0.1, 0.1, 0.1), (65536, 65536, 0), TOO_MANY),      # the count is checked axis by axis
    ((0.0, 0.0, 0.0), (0.1, 0.1, 0.1), (2 ** 31 - 1, 1, -1), BAD_LATTICE),
    # valid edge cases
    ((0.0, 0.0, 0.0), (0.1, 0.1, 0.1), (4, 4, 4), ""),
    ((0.0, 0.0, 0.0), (0.1, 0.1, 0.1), (1, 1, 1), ""),
    ((0.0, 0.0, 0.0), (0.1, 0.1, 0.1), (2 ** 31 - 1, 1, 1), ""),
    ((0.0, 0.0, 0.0), (0.1, 0.1, 0.1), (1, 1, 2 ** 31 - 1), ""),
    ((0.0, 0.0, 0.0), (0.1, 0.1, 0.1), (2047, 1024, 1024), ""),
    ((-3e38, 3e38, 0.0), (1e-45, 3e38, 1.0), (4, 4, 4), ""),              # a denormal spacing is positive
])
def test_lattice_check(policy, origin, spacing, dims, why):
    assert lattice_refusal(policy, origin, spacing, dims) == why


def test_lattice_check_refuses_null_arrays(policy):
    for k in range(3):
        args = [(0.0, 0.0, 0.0), (0.1, 0.1, 0.1), (4, 4, 4)]
        args[k] = None
        assert lattice_refusal(policy, *args) == "null origin, spacing or dims"
    assert lattice_refusal(policy, None, None, None) == "null origin, spacing or dims"


# ---- launch decisions (csrc/sample_policy.h) -------------------------------------------------------
def test_brick_and_tile_constants(policy):
    assert policy.threads() == 256
    shapes = []
    for i in range(policy.n_bricks()):
        out = (C.c_int * 3)()
        policy.brick_table(i, out)
        shapes.append(tuple(out))
    assert shapes[0] == (8, 8, 4) and len(set(shapes)) == len(shapes)
    assert all(a * b * c == 256 for a, b, c in shapes)
    assert policy.tile_cap() == 2560 and policy.max_rows() == 64 and policy.cell_budget() == 8
    # 70 KiB with velocity: two workgroups fit the MI355X's 160 KiB of LDS per CU; 40 KiB without
    assert policy.tile_cap() * policy.tile_bytes(1) == 71680
    assert 2 * (policy.tile_cap() * policy.tile_bytes(1) + 1024) <= 160 * 1024
    assert policy.tile_cap() * policy.tile_bytes(0) == 40960


@pytest.mark.parametrize("points,spacing,cells", [
    (1, 7.0, 3), (8, 0.25, 5), (8, 0.5, 7), (4, 0.25, 4), (4, 0.5, 5), (8, 1.0 / 7.0, 5), (8, 0.0, 4),
    (2, 0.99, 4), (8, 1.0, 11)])
def test_tile_cells_per_axis(policy, points, spacing, cells):
    assert policy.tile_cells_axis(points, spacing) == cells


def test_brick_follows_the_spacing(policy):
    big = (256, 256, 256)
    assert brick(policy, big, (0.25, 0.25, 0.25)) == ((8, 8, 4), 100)      # 5 * 5 * 4 cells
    assert brick(policy, big, (0.5, 0.25, 0.1)) == ((4, 8, 8), 100)       # fine along z: a brick deep in z
    # lattices over the 4M dam column's bounding box (cell units: 0.1 x 0.75 x 1.0 of a 191-cell box)
    assert brick(policy, big, (0.075, 0.56, 0.75)) == ((32, 4, 2), 120)
    assert brick(policy, (128, 128, 128), (0.15, 1.13, 1.51)) == ((32, 8, 1), 264)
    # a z-slice fills the brick with one plane
    assert brick(policy, (512, 512, 1), (0.25, 0.25, 9.0))[0] == (16, 16, 1)


@pytest.mark.parametrize("spacing", [(0.25, 0.25, 0.25), (0.5, 0.5, 0.5), (0.075, 0.56, 0.75), (0.05, 0.05, 0.05)])
def test_default_route_never_tiles(policy, spacing):
    """measured slower than the per-probe walk at every spacing tried"""
    assert tiled(policy, (256, 256, 256), spacing, switch=TILED) == 1
    assert tiled(policy, (256, 256, 256), spacing, switch=DEFAULT) == 0
    assert tiled(policy, (256, 256, 256), spacing, switch=UNTILED) == 0


def test_route_by_spacing_and_capacity(policy):
    """where the tile fits (the route SPH_HIP_SAMPLE_TILED=1 takes)"""
    big = (256, 256, 256)
    assert tiled(policy, big, (0.25, 0.25, 0.25)) == 1          # 100 cells * 8 = 800 entries
    assert tiled(policy, big, (0.5, 0.5, 0.5)) == 1             # 8 x 8 x 4: 7 * 7 * 5 = 245 cells
    assert tiled(policy, big, (0.075, 0.56, 0.75)) == 1
    assert tiled(policy, (128, 128, 128), (0.15, 1.13, 1.51)) == 1   # 264 * 8 = 2112 <= 2560
    assert tiled(policy, (64, 64, 64), (0.3, 2.26, 3.0)) == 0        # the tile would not fit
    assert tiled(policy, big, (1.0, 1.0, 1.0)) == 0             # one probe per neighbourhood
    assert tiled(policy, big, (2.0, 2.0, 2.0)) == 0
    assert tiled(policy, big, (0.25, 0.25, 0.25), switch=UNTILED) == 0
    # the capacity decides: the same lattice with a smaller tile walks per probe
    assert tiled(policy, big, (0.25, 0.25, 0.25), cap=800) == 1
    assert tiled(policy, big, (0.25, 0.25, 0.25), cap=799) == 0


def test_route_ignores_the_spacing_of_single_point_axes(policy):
    # a z-slice: one plane, its spacing says nothing about the tile
    assert tiled(policy, (512, 512, 1), (0.25, 0.25, 100.0)) == 1
    # two planes far apart: bricks one plane deep
    assert tiled(policy, (512, 512, 2), (0.25, 0.25, 100.0)) == 1
    assert brick(policy, (512, 512, 2), (0.25, 0.25, 100.0))[0] == (16, 16, 1)
    # a single point on every axis but one, a cell or more apart: untiled
    assert tiled(policy, (1, 1, 4096), (0.5, 0.5, 1.0)) == 0
    assert tiled(policy, (2, 2, 2), (0.5, 0.5, 0.5)) == 1


def test_lattice_chunks(policy):
    most = policy.chunk_points()
    assert most == 1 << 21
    assert policy.budget() == 8 * 4 * most      # the point-probe chunk: 8 words per probe
    assert chunk(policy, (128, 128, 128), most) == (128, 128, 128)       # 2^21 exactly: one chunk
    assert chunk(policy, (128, 128, 129), most) == (128, 128, 128)
    assert chunk(policy, (256, 256, 256), most) == (256, 256, 32)        # whole z-slabs of bricks
    assert chunk(policy, (700, 5, 4000), most) == (700, 5, 596)
    # a plane too large for a slab of bricks: rows of bricks, then runs of bricks
    assert chunk(policy, (1000, 1000, 10), most) == (1000, 520, 4)
    assert chunk(policy, (4096, 4096, 16), most) == (4096, 128, 4)
    assert chunk(policy, (1 << 20, 1024, 4), most) == (65536, 8, 4)
    assert chunk(policy, (1 << 20, 1024, 2), most) == (131072, 8, 2)
    assert chunk(policy, (1 << 30, 1, 1), most) == (most, 1, 1)
    # the brick shape sets the multiples
    assert chunk(policy, (1 << 18, 1024, 4), most, (32, 4, 2)) == (1 << 18, 4, 2)
    assert chunk(policy, (1 << 20, 1024, 4), most, (32, 4, 2)) == (262144, 4, 2)


@pytest.mark.parametrize("shape", [(8, 8, 4), (32, 4, 2), (64, 4, 1), (4, 8, 8)])
@pytest.mark.parametrize("dims", [(256, 256, 256), (4096, 4096, 16), (1 << 20, 1024, 4), (1 << 30, 1, 2),
                                  (3000, 2999, 7), (700, 5, 4000), (1, 1, 2 ** 31 - 1)])
def test_lattice_chunks_cover_whole_bricks_within_the_bound(policy, dims, shape):
    most = policy.chunk_points()
    ex, ey, ez = chunk(policy, dims, most, shape)
    assert 0 < ex <= dims[0] and 0 < ey <= dims[1] and 0 < ez <= dims[2]
    assert ex * ey * ez <= most
    # a chunk that does not span an axis is made of whole bricks along it
    for e, d, b in zip((ex, ey, ez), dims, shape):
        assert e == d or e % b == 0


def test_forced_chunk_is_clamped(policy):
    """SPH_HIP_SAMPLE_CHUNK: 0 (and anything below) is off; otherwise at least one brick, at most the limit"""
    most = policy.chunk_points()
    assert policy.threads() == 256 and most == 1 << 21
    for off in (0, -1, -(1 << 40)):
        assert policy.chunk_forced(off) == 0
    for low in (1, 2, 255, 256):
        assert policy.chunk_forced(low) == 256
    for v in (257, 1000, most - 1, most):
        assert policy.chunk_forced(v) == v
    for high in (most + 1, 1 << 31, 1 << 40):
        assert policy.chunk_forced(high) == most
    # a call keeps a smaller limit of its own (the scalar point sampler: half the limit)
    assert policy.chunk_limit(most, 0) == most and policy.chunk_limit(most // 2, 0) == most // 2
    assert policy.chunk_limit(most, 1000) == 1000 and policy.chunk_limit(most // 2, 1000) == 1000
    assert policy.chunk_limit(most // 2, most) == most // 2 and policy.chunk_limit(most, most) == most
    # at the smallest forced value a lattice chunk is one whole brick of every shape, never empty
    for i in range(policy.n_bricks()):
        shape = (C.c_int * 3)()
        policy.brick_table(i, shape)
        assert chunk(policy, (100, 100, 100), 256, tuple(shape)) == tuple(shape)


def test_forced_chunks_cut_along_z_then_y_then_x(policy):
    assert forced_chunks(policy, (37, 45, 19), (0.25, 0.25, 0.25)) == (37 * 45 * 4, 37 * 4 * 8, 256)


def test_point_chunks(policy):
    most = policy.chunk_points()
    assert policy.points_chunk(0, most) == 0
    assert policy.points_chunk(most, most) == most
    assert policy.points_chunk(most + 1, most) == most
    assert policy.points_chunk(1000, most) == 1000


# ---- the emulation the GPU tests lean on -----------------------------------------------------------
def test_cell_coord_matches_the_build_on_edge_values():
    inv, n = np.float32(10.0), 8
    x = np.array([-1.0, 0.0, 0.05, 0.1, 0.7999, 0.8, 5.0, np.nan, np.inf, -np.inf, 3e9], np.float32)
    assert E.cell_coord(x, inv, n).tolist() == [0, 0, 0, 1, 7, 7, 7, 0, 0, 0, 0]


@pytest.fixture(scope="module")
def small_scene(hiplib):
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dam_break(4096, speed=0.05)
    return p, pos.reshape(-1, 3), vel.reshape(-1, 3), mass


def test_emulation_matches_a_float64_brute_force(small_scene):
    p, pos, vel, mass = small_scene
    rng = np.random.default_rng(7)
    lo, hi = pos.min(0), pos.max(0)
    probes = np.concatenate([
        (lo + rng.random((400, 3)) * (hi - lo)).astype(np.float32),   # inside the column and its surface
        pos[rng.choice(len(pos), 100, replace=False)],                # on particles: their own term counts
    ])
    g = E.Grid(p, pos, vel, mass)
    rho, v, cnt = g.sample(probes)
    rho64, v64 = E.brute_force64(p, pos, vel, mass, probes)
    assert (rho > 0).sum() > 450
    np.testing.assert_allclose(rho, rho64, rtol=1e-5, atol=1e-5 * float(rho64.max()))
    scale = float(np.abs(v64).max())
    np.testing.assert_allclose(v, v64, rtol=1e-5, atol=1e-5 * scale)
    # the count is the fp32 membership over ALL particles, not only the 27 cells walked
    d = probes[:, None, :] - pos[None, :, :]
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    assert np.array_equal(cnt, (d2 < np.float32(p.h2)).sum(1))
    # a probe on a particle counts that particle
    assert (cnt[400:] >= 1).all()


def test_emulation_of_far_and_non_finite_probes(small_scene):
    p, pos, vel, mass = small_scene
    g = E.Grid(p, pos, vel, mass)
    probes = np.array([[-5.0, -5.0, -5.0], [50.0, 0.5, 0.5], [np.nan, 0.0, 0.0], [np.inf, 0.1, 0.1],
                       [-np.inf, 0.0, 0.0], [0.05, np.nan, 0.5]], np.float32)
    rho, v, cnt = g.sample(probes)
    assert not rho.any() and not v.any() and not cnt.any()
    assert not np.signbit(rho).any() and not np.signbit(v).any()


def test_emulation_without_velocity_gives_the_same_density(small_scene):
    p, pos, vel, mass = small_scene
    g = E.Grid(p, pos, vel, mass)
    probes = pos[:64] + np.float32(0.001)
    a = g.sample(probes)
    b = g.sample(probes, velocity=False)
    assert b[1] is None and np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])


def test_lattice_points_are_fp32_unfused():
    pts = E.lattice_points((0.1, 0.2, 0.3), (0.01, 0.02, 0.03), (5, 4, 3))
    assert pts.shape == (3, 4, 5, 3) and pts.dtype == np.float32
    i = np.arange(5, dtype=np.float32)
    assert np.array_equal(pts[2, 3, :, 0], np.float32(0.1) + i * np.float32(0.01))
    assert np.array_equal(pts[2, 3, 0, 2], np.float32(0.3) + np.float32(2.0) * np.float32(0.03))
