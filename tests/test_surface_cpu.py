"""CPU checks of the iso-surface extractor (include/sph_hip.h: sph_hip_extract_surface): the C ABI and
its binding, the tables and slab sizing of csrc/surface_policy.h (compiled with g++ behind an
extern "C" shim, as tests/test_sample_cpu.py does), the numpy restatement the GPU tests check
against (tests/surface_emulation.py) on analytic fields, and write_ply."""
import ctypes as C
import os

import numpy as np
import pytest

import surface_emulation as E
from helpers import compile_shim
from test_sample_cpu import header_prototype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

SHIM = r"""
#include "surface_policy.h"

extern "C" {
int edge_dir(int e) { return surf_edge_dir(e); }
int tet_corner(int t, int i) { return surf_tet_corner(t, i); }
int case_n(int t, int m) { return SURF_CASES.c[t][m].n; }
int case_key(int t, int m, int k) { return SURF_CASES.c[t][m].key[k]; }
int key_corner(int key) { return surf_key_corner(key); }
int key_edge(int key) { return surf_key_edge(key); }
int tet_case(int t, int cube_in) { return surf_tet_case(t, cube_in); }
int planes(const int* dims, int vel, int forced) { return surf_planes(dims, vel != 0, forced); }
long long scratch_bytes(const int* dims, int planes, int vel) { return surf_scratch(dims, planes, vel != 0).bytes; }
long long budget() { return SURF_SCRATCH_BUDGET; }
const char* check(float iso, int flags)
{
   const char* why = surf_check(iso, flags);
   return why ? why : "";
}
}
"""


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    lib = compile_shim(SHIM, ["-O1"], tmp_path_factory)
    lib.planes.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int]
    lib.scratch_bytes.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int]
    lib.scratch_bytes.restype = C.c_longlong
    lib.budget.restype = C.c_longlong
    lib.check.argtypes = [C.c_float, C.c_int]
    lib.check.restype = C.c_char_p
    return lib


# ---- C ABI -----------------------------------------------------------------------------------------
def test_surface_symbols_are_exported(hiplib):
    for name in ("sph_hip_extract_surface", "sph_hip_download_surface"):
        assert hasattr(hiplib, name)


def test_surface_prototypes_match_the_header():
    from smoothed_particle_hydrodynamics_amd.lib import PROTOTYPES
    P = C.POINTER
    assert header_prototype("sph_hip_extract_surface") == [
        "sph_hip_context* ctx", "const float origin[3]", "const float spacing[3]", "const int32_t dims[3]",
        "float iso", "int flags", "int32_t counts[2]"]
    res, args = PROTOTYPES["sph_hip_extract_surface"]
    assert res is C.c_int and args[0] is C.c_void_p and args[4] is C.c_float and args[5] is C.c_int
    assert [a._type_ for a in args[1:4]] == [C.c_float * 3, C.c_float * 3, C.c_int32 * 3]
    assert args[6]._type_ == C.c_int32 * 2 and all(issubclass(a, C._Pointer) for a in args[1:4] + [args[6]])
    assert header_prototype("sph_hip_download_surface") == [
        "sph_hip_context* ctx", "float* vertices_xyz", "float* normals_xyz", "float* velocity_xyz",
        "int32_t* triangles"]
    assert PROTOTYPES["sph_hip_download_surface"] == (C.c_int, [C.c_void_p] * 5)
    del P


def test_flags_and_abi_version():
    from smoothed_particle_hydrodynamics_amd.lib import ABI_VERSION
    text = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    assert "#define SPH_HIP_SURFACE_NORMALS  1" in text and "#define SPH_HIP_SURFACE_VELOCITY 2" in text
    assert "#define SPH_HIP_ABI_VERSION 7" in text and ABI_VERSION == 7


# ---- policy: tables -------------------------------------------------------------------------------------
def corner(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], np.int64)


def test_edge_list_and_kuhn_split(policy):
    assert [policy.edge_dir(e) for e in range(7)] == [1, 2, 4, 3, 5, 6, 7]
    for t, (a, b) in enumerate(E.TET_AB):
        assert [policy.tet_corner(t, i) for i in range(4)] == [0, a, a | b, 7]
    # the six tetrahedra fill the cube: volumes 1/6 each, disjoint (sum = 1)
    vol = 0.0
    for t in range(6):
        c = [corner(policy.tet_corner(t, i)) for i in range(4)]
        vol += abs(np.linalg.det(np.stack([c[1] - c[0], c[2] - c[0], c[3] - c[0]]))) / 6.0
    assert vol == pytest.approx(1.0)


def test_every_tetrahedron_edge_is_a_lattice_edge(policy):
    dirs = [tuple(corner(policy.edge_dir(e))) for e in range(7)]
    for t in range(6):
        for i in range(4):
            for j in range(i + 1, 4):
                lo, hi = policy.tet_corner(t, i), policy.tet_corner(t, j)
                assert lo & hi == lo, "corner %d is not below %d" % (lo, hi)
                assert tuple(corner(hi) - corner(lo)) in dirs


@pytest.mark.parametrize("t", range(6))
def test_case_table_orientation_and_start(policy, t):
    path = [policy.tet_corner(t, i) for i in range(4)]
    for m in range(16):
        k = bin(m).count("1")
        n = policy.case_n(t, m)
        assert n == (0 if k in (0, 4) else 1 if k in (1, 3) else 2), (t, m)
        if n == 0:
            continue
        keys = [policy.case_key(t, m, q) for q in range(n + 2)]
        ins = [c for q, c in enumerate(path) if (m >> q) & 1]
        out = [c for q, c in enumerate(path) if not (m >> q) & 1]
        ends = []
        for key in keys:
            lo = policy.key_corner(key)
            hi = lo | policy.edge_dir(policy.key_edge(key))
            assert lo != hi and lo & hi == lo
            assert (lo in ins) != (hi in ins), "edge %d-%d does not cross (t %d, m %d)" % (lo, hi, t, m)
            assert lo in path and hi in path
            ends.append((lo, hi))
        assert len(set(ends)) == len(ends) == len(ins) * len(out)
        # the cycle starts at its smallest key: the smallest vertex id of the cube (ids grow with keys)
        assert keys[0] == min(keys)
        if n == 2:   # consecutive quad edges share a corner
            for q in range(4):
                assert set(ends[q]) & set(ends[(q + 1) % 4])
        mid = [0.5 * (corner(lo) + corner(hi)) for lo, hi in ends]
        toward = np.mean([corner(c) for c in out], 0) - np.mean([corner(c) for c in ins], 0)
        for tri in ([0, 1, 2],) if n == 1 else ([0, 1, 2], [0, 2, 3]):
            v0, v1, v2 = (mid[q] for q in tri)
            assert np.dot(np.cross(v1 - v0, v2 - v0), toward) > 0, (t, m, tri)


def test_tet_case_reads_the_path_corners(policy):
    for t in range(6):
        path = [policy.tet_corner(t, i) for i in range(4)]
        for cin in range(256):
            want = sum(((cin >> path[i]) & 1) << i for i in range(4))
            assert policy.tet_case(t, cin) == want


# ---- policy: slabs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(256, 256, 256), (64, 256, 256), (1024, 1024, 64), (3, 5, 7), (1, 1, 1),
                                  (4096, 4096, 8), (17, 3000, 40)])
@pytest.mark.parametrize("vel", [0, 1])
def test_slab_sizing_stays_in_budget(policy, dims, vel):
    d = (C.c_int * 3)(*dims)
    P = policy.planes(d, vel, 0)
    assert 1 <= P <= dims[2]
    if P > 1 or policy.scratch_bytes(d, 1, vel) <= policy.budget():
        assert policy.scratch_bytes(d, P, vel) <= policy.budget()
    if P < dims[2]:
        assert policy.scratch_bytes(d, P + 1, vel) > policy.budget()
    for forced in (1, 2, 3, 10 ** 6):
        assert policy.planes(d, vel, forced) == min(forced, dims[2])
    # sampled points: the P planes and the halo (1 below, 2 above) where the lattice has them
    plane = dims[0] * dims[1]
    one = policy.scratch_bytes(d, 1, vel)
    assert one >= plane * min(4, dims[2]) * (20 if vel else 8)


def test_256_cubed_fits_several_planes(policy):
    d = (C.c_int * 3)(256, 256, 256)
    assert policy.planes(d, 1, 0) >= 8 and policy.planes(d, 0, 0) >= policy.planes(d, 1, 0)


# ---- emulation on analytic fields ---------------------------------------------------------------------------
def field(shape, origin, spacing, fn):
    X, Y, Z = E.lattice_axes(origin, spacing, shape)
    z, y, x = np.meshgrid(Z.astype(np.float64), Y.astype(np.float64), X.astype(np.float64), indexing="ij")
    return fn(x, y, z).astype(F32)


def ball(R, c=(0.0, 0.0, 0.0)):
    # iso 1: inside where R - |x - c| + 1 > 1
    return lambda x, y, z: R + 1.0 - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)


@pytest.mark.parametrize("spacing", [(0.1, 0.1, 0.1), (0.05, 0.08, 0.13), (0.13, 0.05, 0.07), (0.2, 0.2, 0.2)])
def test_sphere_is_closed_with_euler_two(spacing):
    R = 1.0
    origin = (-1.5, -1.45, -1.55)
    shape = tuple(int(np.ceil(3.1 / s)) + 1 for s in spacing)
    f = field(shape, origin, spacing, ball(R))
    m = E.extract(f, origin, spacing, 1.0)
    assert len(m.triangles) > 100
    assert E.is_closed_oriented(m.triangles)
    assert E.euler(m.triangles) == 2
    r = np.sqrt((m.vertices.astype(np.float64) ** 2).sum(1))
    assert np.abs(r - R).max() <= max(spacing)
    assert E.volume(m.vertices, m.triangles) > 0
    # normals point away from the centre (toward lower values)
    assert (np.einsum("ij,ij->i", m.normals.astype(np.float64), m.vertices) > 0).mean() > 0.99


def test_sphere_volume_at_a_fine_spacing():
    spacing = (0.02, 0.02, 0.02)
    origin = (-1.2, -1.2, -1.2)
    f = field((121, 121, 121), origin, spacing, ball(1.0))
    m = E.extract(f, origin, spacing, 1.0, normals=False)
    assert E.volume(m.vertices, m.triangles) == pytest.approx(4.0 / 3.0 * np.pi, rel=0.01)


def test_torus_has_euler_zero():
    spacing = (0.05, 0.06, 0.05)
    origin = (-1.6, -1.6, -0.6)
    shape = (65, 55, 25)

    def torus(x, y, z):
        return 1.0 + 0.3 - np.sqrt((np.sqrt(x * x + y * y) - 1.0) ** 2 + z * z)

    m = E.extract(field(shape, origin, spacing, torus), origin, spacing, 1.0)
    assert E.is_closed_oriented(m.triangles) and E.euler(m.triangles) == 0
    assert E.volume(m.vertices, m.triangles) == pytest.approx(2 * np.pi ** 2 * 1.0 * 0.09, rel=0.05)


def test_two_balls_have_euler_four():
    spacing = (0.07, 0.07, 0.07)
    origin = (-1.0, -1.0, -1.0)
    shape = (60, 30, 30)

    def two(x, y, z):
        return np.maximum(ball(0.6)(x, y, z), ball(0.6, (2.5, 0.0, 0.0))(x, y, z))

    m = E.extract(field(shape, origin, spacing, two), origin, spacing, 1.0)
    assert E.is_closed_oriented(m.triangles) and E.euler(m.triangles) == 4


def test_cut_ball_is_open_on_the_lattice_faces():
    spacing = (0.1, 0.1, 0.1)
    origin = (-1.5, -1.5, -0.45)      # the lattice cuts the ball at z = -0.45
    shape = (31, 31, 21)
    f = field(shape, origin, spacing, ball(1.0))
    m = E.extract(f, origin, spacing, 1.0)
    assert not E.is_closed_oriented(m.triangles)
    assert E.is_manifold(m.triangles)
    b = E.boundary_edges(m.triangles)
    assert len(b) > 0
    z = m.vertices[b.reshape(-1), 2]
    assert (z == F32(origin[2])).all()


def test_nan_and_exact_iso_values_stay_a_manifold():
    rng = np.random.default_rng(3)
    spacing = (0.1, 0.1, 0.1)
    origin = (-1.5, -1.5, -1.5)
    f = field((31, 31, 31), origin, spacing, ball(1.0))
    # quantise: many points exactly at iso, and NaNs scattered inside and out
    f = (np.round(f * F32(4)) / F32(4)).astype(F32)
    assert (f == F32(1.0)).sum() > 100
    nan = rng.random(f.shape) < 0.03
    nan[0, :, :] = nan[-1, :, :] = nan[:, 0, :] = nan[:, -1, :] = nan[:, :, 0] = nan[:, :, -1] = False
    f[nan] = np.nan
    m = E.extract(f, origin, spacing, 1.0)
    assert len(m.triangles) > 100
    assert E.is_closed_oriented(m.triangles)
    assert np.isfinite(m.vertices).all()
    ln = np.sqrt((m.normals.astype(np.float64) ** 2).sum(1))
    assert ((np.abs(ln - 1) < 1e-5) | (ln == 0)).all()


# ---- write_ply ----------------------------------------------------------------------------------------------
def read_ply(path):
    with open(path, "rb") as f:
        data = f.read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = int(next(l for l in lines if l.startswith("element vertex")).split()[-1])
    nf = int(next(l for l in lines if l.startswith("element face")).split()[-1])
    props = [l.split()[-1] for l in lines if l.startswith("property float")]
    vert = np.frombuffer(body, dtype=[(p, "<f4") for p in props], count=nv)
    face = np.frombuffer(body, dtype=[("n", "u1"), ("i", "<i4", (3,))], count=nf, offset=vert.nbytes)
    assert (face["n"] == 3).all()
    v = np.stack([vert[p] for p in ("x", "y", "z")], 1)
    n = np.stack([vert[p] for p in ("nx", "ny", "nz")], 1) if "nx" in props else None
    return v, face["i"], n


@pytest.mark.parametrize("with_normals", [True, False])
def test_write_ply_round_trips(tmp_path, with_normals):
    from smoothed_particle_hydrodynamics_amd import SurfaceMesh, write_ply
    spacing = (0.2, 0.2, 0.2)
    origin = (-1.5, -1.5, -1.5)
    m = E.extract(field((16, 16, 16), origin, spacing, ball(1.0)), origin, spacing, 1.0, normals=with_normals)
    mesh = SurfaceMesh(m.vertices, m.triangles, m.normals, None)
    path = tmp_path / "s.ply"
    write_ply(str(path), mesh)
    v, t, n = read_ply(str(path))
    assert v.tobytes() == m.vertices.tobytes() and t.astype(np.int32).tobytes() == m.triangles.tobytes()
    if with_normals:
        assert n.tobytes() == m.normals.tobytes()
    else:
        assert n is None


# ---- iso and flag checks (csrc/surface_policy.h: surf_check) ------------------------------------------
@pytest.mark.parametrize("iso,flags,why", [
    # the cases test_gpu_surface.py::test_bad_arguments_are_refused lists
    (0.0, 0, "iso must be finite and positive"),
    (-1.0, 0, "iso must be finite and positive"),
    (float("nan"), 0, "iso must be finite and positive"),
    (float("inf"), 0, "iso must be finite and positive"),
    (-float("inf"), 0, "iso must be finite and positive"),
    (1.0, 4, "unknown flag bits"),
    (1.0, 8, "unknown flag bits"),
    (1.0, -1, "unknown flag bits"),
    (1.0, 1 << 30, "unknown flag bits"),
    (-0.0, 4, "iso must be finite and positive"),     # the iso is checked first
    # valid edge cases: both flags, either, none; the smallest and largest positive floats
    (1.0, 0, ""),
    (1.0, 1, ""),
    (1.0, 2, ""),
    (1.0, 3, ""),
    (1e-45, 3, ""),
    (3.4e38, 0, ""),
])
def test_surf_check(policy, iso, flags, why):
    assert policy.check(iso, flags).decode() == why
