"""The field sampler on an MI355X (include/sph_hip.h: sph_hip_sample_points / _lattice), checked bit
for bit against the numpy emulation of tests/sample_emulation.py (itself checked against a float64
brute force by tests/test_sample_cpu.py), and checked not to change the simulation."""
import ctypes as C

import numpy as np
import pytest

import sample_emulation as E
from test_sample_cpu import DEFAULT, TILED, forced_chunks, policy, tiled  # noqa: F401  (policy: the g++ shim of sample_policy.h)

pytestmark = pytest.mark.gpu

F32 = np.float32


def make(scene, mode=None):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = scene
    sph = S.SPH(mass.size, p, mode=S.MODE_FULL if mode is None else mode, device=0)
    sph.setParticles(pos, vel, mass)
    return sph


def state(sph, mass):
    part = sph.syncParticles()
    return part.mPosition.reshape(-1, 3).copy(), part.mVelocity.reshape(-1, 3).copy(), mass


def same(a, b):
    """bit-identical float / int arrays (NaN patterns included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_fields(got, want, what):
    for name, g, w in zip(("density", "velocity", "count"), got, want):
        if w is None:
            assert g is None, what + " " + name
            continue
        bad = np.flatnonzero(np.ascontiguousarray(g).view(np.uint32 if g.dtype == F32 else np.int32).reshape(-1) !=
                             np.ascontiguousarray(w).view(np.uint32 if w.dtype == F32 else np.int32).reshape(-1))
        assert bad.size == 0, "%s %s: %d of %d differ, first at %d: %r vs %r" % (
            what, name, bad.size, g.size, bad[0], g.reshape(-1)[bad[0]], w.reshape(-1)[bad[0]])


def probe_set(p, pos, rng, n_random=2500, n_on=500):
    lo, hi = pos.min(0), pos.max(0)
    pad = F32(3 * p.h)
    box = np.array([p.max_x, p.max_y, p.max_z], F32)
    special = np.array([
        [-1.0, -1.0, -1.0], [box[0] + 1.0, 0.5, 0.5], [0.5 * box[0], 0.5 * box[1], -0.3],   # outside the box
        [np.nan, 0.1, 0.1], [0.1, np.nan, 0.1], [np.inf, 0.1, 0.1], [-np.inf, 0.1, 0.1],
        [0.05, np.inf, -np.inf], [np.nan, np.nan, np.nan], [3e38, 3e38, 3e38]], F32)
    return np.concatenate([
        (lo - pad + rng.random((n_random, 3)) * (hi - lo + 2 * pad)).astype(F32),   # in, around and above the fluid
        pos[rng.choice(len(pos), n_on, replace=False)],                             # exactly on particles
        (box * F32(0.9) + rng.random((64, 3)) * F32(0.05)).astype(F32),             # empty space inside the box
        special]).astype(F32)


@pytest.fixture(scope="module")
def dam():
    from smoothed_particle_hydrodynamics_amd import scenes
    return scenes.dam_break(32768, speed=0.05)


@pytest.fixture(scope="module")
def dense():
    from smoothed_particle_hydrodynamics_amd import scenes
    return scenes.dense_block(16384)


# ---- 1. point probes == the emulation ------------------------------------------------------------
@pytest.mark.parametrize("which", ["dam", "dense"])
def test_points_match_the_emulation(request, which):
    scene = request.getfixturevalue(which)
    p, mass = scene[0], scene[3]
    with make(scene) as sph:
        sph.run(2)
        pos, vel, _ = state(sph, mass)
        probes = probe_set(p, pos, np.random.default_rng(11))
        got = sph.sampleFields(probes)
        got_nv = sph.sampleFields(probes, velocity=False)
    g = E.Grid(p, pos, vel, mass)
    want = g.sample(probes)
    assert_fields(got, want, which)
    assert_fields(got_nv, (want[0], None, want[2]), which + " without velocity")
    # the self term: a probe on a particle counts it, and the far / non-finite probes give zeros
    assert (got[2][2500:3000] >= 1).all()
    tail = slice(len(probes) - 10, None)
    assert not got[0][tail].any() and not got[1][tail].any() and not got[2][tail].any()
    assert (got[2][:2500] == 0).any() and (got[2][:2500] > 20).any()


def test_zero_probes_do_nothing(dam):
    with make(dam) as sph:
        rho, vel, cnt = sph.sampleFields(np.zeros((0, 3), F32))
        assert rho.size == 0 and vel.shape == (0, 3) and cnt.size == 0


# ---- 2. lattices: tiled == untiled == points == emulation ---------------------------------------
def surface_lattice(p):
    h = F32(p.h)
    spacing = (h / F32(4),) * 3
    origin = (F32(0.0), F32(0.75) - F32(6) * h, F32(0.3))     # straddles the column's top (y = 0.75) and its side
    shape = (40, 48, 20)
    return origin, spacing, shape


def test_lattice_tiled_untiled_points_and_emulation_agree(dam, policy, monkeypatch):
    p, mass = dam[0], dam[3]
    origin, spacing, shape = surface_lattice(p)
    cells = [float(s) * float(F32(p.full_cell_inv)) for s in spacing]
    assert tiled(policy, shape, cells, TILED) == 1, "SPH_HIP_SAMPLE_TILED=1 must take the tiled route here"
    assert tiled(policy, shape, cells, DEFAULT) == 0
    pts = E.lattice_points(origin, spacing, shape)
    out = {}
    for route, env in (("tiled", "SPH_HIP_SAMPLE_TILED"), ("untiled", "SPH_HIP_SAMPLE_UNTILED"), ("default", None)):
        monkeypatch.delenv("SPH_HIP_SAMPLE_TILED", raising=False)
        monkeypatch.delenv("SPH_HIP_SAMPLE_UNTILED", raising=False)
        if env:
            monkeypatch.setenv(env, "1")
        with make(dam) as sph:      # (the switches are read when the context is created)
            sph.run(2)
            pos, vel, _ = state(sph, mass)
            out[route] = (pos, sph.sampleLattice(origin, spacing, shape),
                          sph.sampleLattice(origin, spacing, shape, velocity=False))
            if route == "default":
                pts_got = sph.sampleFields(pts.reshape(-1, 3))
    assert same(out["tiled"][0], out["untiled"][0]) and same(out["tiled"][0], out["default"][0])
    a, a_nv = out["tiled"][1], out["tiled"][2]
    want = E.Grid(p, pos, vel, mass).sample(pts.reshape(-1, 3))
    nz, ny, nx = shape[2], shape[1], shape[0]
    assert a[0].shape == (nz, ny, nx) and a[1].shape == (nz, ny, nx, 3) and a[2].shape == (nz, ny, nx)
    assert_fields(a, out["untiled"][1], "tiled vs untiled")
    assert_fields(a, out["default"][1], "tiled vs default")
    assert_fields((a[0].reshape(-1), a[1].reshape(-1, 3), a[2].reshape(-1)), pts_got, "lattice vs points")
    assert_fields(pts_got, want, "lattice vs emulation")
    assert_fields(a_nv, (a[0], None, a[2]), "tiled without velocity")
    assert_fields(out["untiled"][2], (a[0], None, a[2]), "untiled without velocity")
    # it does straddle the surface: empty and full points, and bricks with nothing at all
    assert (a[2] == 0).sum() > 1000 and (a[2] > 20).sum() > 1000


def test_lattice_slices_and_thin_lattices(dam):
    p, mass = dam[0], dam[3]
    h = F32(p.h)
    with make(dam) as sph:
        pos, vel, _ = state(sph, mass)
        g = E.Grid(p, pos, vel, mass)
        for origin, spacing, shape in (((0.0, 0.0, 0.5), (h / 5, h / 5, 1.0), (40, 160, 1)),   # a z-slice
                                       ((0.01, 0.2, 0.1), (h / 3, 1.0, 1.0), (37, 1, 1)),     # a line
                                       ((0.02, 0.7, 0.2), (2 * h, 2 * h, 2 * h), (5, 9, 13))):  # coarse: untiled
            got = sph.sampleLattice(origin, spacing, shape)
            want = g.sample(E.lattice_points(origin, spacing, shape).reshape(-1, 3))
            assert_fields((got[0].reshape(-1), got[1].reshape(-1, 3), got[2].reshape(-1)), want, str(shape))


# ---- 2b. chunks: a forced chunk size changes no bit ------------------------------------------------
def odd_lattice(p):
    """surface_lattice with dims that are multiples of no brick"""
    origin, spacing, _ = surface_lattice(p)
    return origin, spacing, (37, 45, 19)


def test_chunked_lattices_equal_the_unchunked_one(dam, policy, monkeypatch):
    p = dam[0]
    origin, spacing, shape = odd_lattice(p)
    cells = [float(s) * float(F32(p.full_cell_inv)) for s in spacing]
    cut_z, cut_y, cut_x = forced_chunks(policy, shape, cells)     # (asserts the three chunk shapes)
    assert tiled(policy, shape, cells, TILED) == 1
    for env in ("SPH_HIP_SAMPLE_TILED", "SPH_HIP_SAMPLE_UNTILED", "SPH_HIP_SAMPLE_CHUNK"):
        monkeypatch.delenv(env, raising=False)
    pts = E.lattice_points(origin, spacing, shape).reshape(-1, 3)
    with make(dam) as sph:      # (the switches are read when the context is created)
        whole = sph.sampleLattice(origin, spacing, shape)
        whole_nv = sph.sampleLattice(origin, spacing, shape, velocity=False)
        by_points = sph.sampleFields(pts)
    # the unchunked call is the point sampler's, which test_points_match_the_emulation pins
    assert_fields((whole[0].reshape(-1), whole[1].reshape(-1, 3), whole[2].reshape(-1)), by_points, "lattice vs points")
    assert_fields(whole_nv, (whole[0], None, whole[2]), "unchunked without velocity")
    assert (whole[2] == 0).sum() > 1000 and (whole[2] > 20).sum() > 1000
    for forced, route in ((cut_z, None), (cut_y, None), (cut_x, None), (cut_x, "SPH_HIP_SAMPLE_TILED")):
        monkeypatch.setenv("SPH_HIP_SAMPLE_CHUNK", str(forced))
        monkeypatch.delenv("SPH_HIP_SAMPLE_TILED", raising=False)
        if route:
            monkeypatch.setenv(route, "1")
        what = "chunks of %d, %s" % (forced, route or "default route")
        with make(dam) as sph:
            assert_fields(sph.sampleLattice(origin, spacing, shape), whole, what)
            assert_fields(sph.sampleLattice(origin, spacing, shape, velocity=False), whole_nv, what + ", no velocity")


def test_chunked_points_equal_the_unchunked_ones(dam, monkeypatch):
    p = dam[0]
    probes = probe_set(p, dam[1].reshape(-1, 3), np.random.default_rng(17), 2000, 426)
    n = len(probes)
    assert n == 2500                                   # chunks of 1000, 1000 and 500 probes
    monkeypatch.delenv("SPH_HIP_SAMPLE_CHUNK", raising=False)
    with make(dam) as sph:
        whole = sph.sampleFields(probes)
    assert (whole[2] == 0).any() and (whole[2][2000:] > 0).any()
    monkeypatch.setenv("SPH_HIP_SAMPLE_CHUNK", "1000")
    with make(dam) as sph:
        assert_fields(sph.sampleFields(probes), whole, "chunks of 1000")
        assert_fields(sph.sampleFields(probes, velocity=False), (whole[0], None, whole[2]), "chunks of 1000, no velocity")
        # one output null at a time: the others are written as before, the null one is left alone
        for skip in range(3):
            out = [np.full(n, 7, F32), np.full((n, 3), 7, F32), np.full(n, 7, np.int32)]
            ptrs = [None if i == skip else a.ctypes.data for i, a in enumerate(out)]
            sph.call("sph_hip_sample_points", n, probes.ctypes.data, *ptrs)
            for i, (a, w) in enumerate(zip(out, whole)):
                assert same(a, np.full_like(a, 7) if i == skip else w), "null output %d: output %d" % (skip, i)


# ---- 3. arithmetics and refusals ------------------------------------------------------------------
def test_full_and_full_fast_sample_the_same(dam):
    import smoothed_particle_hydrodynamics_amd as S
    p = dam[0]
    probes = probe_set(p, dam[1].reshape(-1, 3), np.random.default_rng(3), 1500, 200)
    origin, spacing, shape = surface_lattice(p)
    out = []
    for mode in (S.MODE_FULL, S.MODE_FULL_FAST):
        with make(dam, mode) as sph:      # (no step: the two arithmetics would move the particles apart)
            out.append((sph.sampleFields(probes), sph.sampleLattice(origin, spacing, shape)))
    assert_fields(out[0][0], out[1][0], "points")
    assert_fields(out[0][1], out[1][1], "lattice")


def test_ref_and_slab_contexts_are_refused(dam):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd.lib import SphHipError, load_library
    p, pos, vel, mass = dam
    with make(dam, S.MODE_REF) as sph:
        with pytest.raises(SphHipError, match="FULL and FULL_FAST"):
            sph.sampleFields(np.zeros((4, 3), F32))
        with pytest.raises(SphHipError, match="FULL and FULL_FAST"):
            sph.sampleLattice((0, 0, 0), (0.1, 0.1, 0.1), (2, 2, 2))
    lib = load_library()
    ctx = C.c_void_p()
    params = p.copy()
    assert lib.sph_hip_create_slab(C.byref(ctx), C.byref(params), 4096, 0, 0, p.full_cells_z // 2) == 0
    try:
        xyz = np.zeros(3, F32)
        assert lib.sph_hip_sample_points(ctx, 1, xyz.ctypes.data_as(C.c_void_p), None, None, None) == -1
        assert b"slab" in lib.sph_hip_last_error(ctx)
        o, s, d = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(0.1, 0.1, 0.1), (C.c_int32 * 3)(2, 2, 2)
        assert lib.sph_hip_sample_lattice(ctx, C.byref(o), C.byref(s), C.byref(d), None, None, None) == -1
    finally:
        lib.sph_hip_destroy(ctx)


def test_bad_arguments_on_a_live_context(dam):
    from smoothed_particle_hydrodynamics_amd.lib import SphHipError
    with make(dam) as sph:
        lib, ctx = sph._lib, sph._ctx
        assert lib.sph_hip_sample_points(ctx, -1, None, None, None, None) == -1
        assert lib.sph_hip_sample_points(ctx, 0, None, None, None, None) == 0
        for origin, spacing, shape in (((0, 0, 0), (0.1, 0.1, 0.1), (0, 2, 2)),
                                       ((np.nan, 0, 0), (0.1, 0.1, 0.1), (2, 2, 2)),
                                       ((0, 0, 0), (0.1, -0.1, 0.1), (2, 2, 2)),
                                       ((0, 0, 0), (0.1, 0.1, np.inf), (2, 2, 2)),
                                       ((0, 0, 0), (0.1, 0.0, 0.1), (2, 2, 2))):
            with pytest.raises(SphHipError):
                sph.sampleLattice(origin, spacing, shape)
        o, s, d = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(0.1, 0.1, 0.1), (C.c_int32 * 3)(2048, 1024, 1024)
        assert lib.sph_hip_sample_lattice(ctx, C.byref(o), C.byref(s), C.byref(d), None, None, None) == -1
        assert b"2^31" in lib.sph_hip_last_error(ctx)


# ---- 4. no effect on the trajectory -------------------------------------------------------------
def snapshot(sph):
    part = sph.syncParticles()
    return [part.mPosition.copy(), part.mVelocity.copy(), part.mDensity.copy(), part.mAcceleration.copy(),
            part.mNeighborCount.copy(), np.array(sph.energy(), F32)]


def test_sampling_does_not_change_the_trajectory(dam):
    import smoothed_particle_hydrodynamics_amd as S
    p = dam[0]
    origin, spacing, shape = surface_lattice(p)
    probes = probe_set(p, dam[1].reshape(-1, 3), np.random.default_rng(5), 1000, 100)
    with make(dam, S.MODE_FULL_FAST) as a:
        for _ in range(6):
            a.step()
        want = snapshot(a)
    with make(dam, S.MODE_FULL_FAST) as b:
        for _ in range(3):
            b.step()            # the fused integrate leaves its prehash for the next cell build
        before = snapshot(b)
        b.sampleFields(probes)
        b.sampleLattice(origin, spacing, shape)
        after = snapshot(b)
        b.sampleFields(probes[:10], velocity=False)
        for _ in range(3):
            b.step()
        got = snapshot(b)
    for x, y in zip(before, after):
        assert same(x, y), "download changed across a sample call"
    for i, (x, y) in enumerate(zip(want, got)):
        assert same(x, y), "the trajectory changed (array %d)" % i


# ---- 5. cross-check with the density pass ---------------------------------------------------------
@pytest.mark.parametrize("which", ["dam", "dense"])
def test_samples_at_particles_agree_with_the_density_pass(request, which):
    p, pos, vel, mass = request.getfixturevalue(which)
    with make((p, pos, vel, mass)) as sph:
        rho, _, cnt = sph.sampleFields(pos.reshape(-1, 3), velocity=False)
        sph.step()
        part = sph.syncParticles()
    assert np.array_equal(cnt, part.mNeighborCount + 1)
    self_term = mass.astype(F32) * (F32(p.kernel1) * (F32(p.hscaled2) * F32(p.hscaled2) * F32(p.hscaled2)))
    diff = np.abs(rho.astype(np.float64) - self_term - part.mDensity)
    assert (diff <= 1e-6 * (part.mDensity.astype(np.float64) + self_term)).all(), float(diff.max())


# ---- 6. at size ---------------------------------------------------------------------------------
def test_4m_column_lattice(policy, monkeypatch):
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dam_break(4 * 1024 * 1024, speed=0.05)
    pts3 = pos.reshape(-1, 3)
    lo, hi = pts3.min(0), pts3.max(0)
    shape = (128, 128, 128)
    spacing = tuple((hi - lo) / F32(127))
    origin = tuple(lo)
    cells = [float(s) * float(F32(p.full_cell_inv)) for s in spacing]
    assert tiled(policy, shape, cells, TILED) == 1
    monkeypatch.setenv("SPH_HIP_SAMPLE_TILED", "1")
    with make((p, pos, vel, mass)) as sph:
        a = sph.sampleLattice(origin, spacing, shape)
    monkeypatch.delenv("SPH_HIP_SAMPLE_TILED")
    monkeypatch.setenv("SPH_HIP_SAMPLE_UNTILED", "1")
    with make((p, pos, vel, mass)) as sph:
        b = sph.sampleLattice(origin, spacing, shape)
    assert_fields(a, b, "4M tiled vs untiled")
    assert (a[2] > 0).mean() > 0.5
    rng = np.random.default_rng(9)
    pick = rng.choice(a[0].size, 2000, replace=False)
    lat = E.lattice_points(origin, spacing, shape).reshape(-1, 3)[pick]
    want = E.Grid(p, pts3, vel.reshape(-1, 3), mass).sample(lat)
    assert_fields((a[0].reshape(-1)[pick], a[1].reshape(-1, 3)[pick], a[2].reshape(-1)[pick]), want,
                  "4M lattice vs emulation")
