"""The iso-surface extractor on an MI355X (include/sph_hip.h: sph_hip_extract_surface), checked bit
for bit against the numpy restatement of tests/surface_emulation.py applied to the sampler's lattice
(sample_emulation's, or the device's own sampleLattice output), and checked not to change the
simulation."""
import ctypes as C

import numpy as np
import pytest

import sample_emulation as SE
import surface_emulation as E

pytestmark = pytest.mark.gpu

F32 = np.float32
NORMALS, VELOCITY = 1, 2


def make(scene, mode=None):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = scene
    sph = S.SPH(mass.size, p, mode=S.MODE_FULL if mode is None else mode, device=0)
    sph.setParticles(pos, vel, mass)
    return sph


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_mesh(got, want, what):
    for name in ("vertices", "triangles", "normals", "velocity"):
        g, w = getattr(got, name), getattr(want, name)
        if w is None or g is None:
            assert g is None and w is None, "%s %s" % (what, name)
            continue
        assert g.shape == w.shape, "%s %s: shape %s vs %s" % (what, name, g.shape, w.shape)
        bad = np.flatnonzero(np.ascontiguousarray(g).view(np.int32).reshape(-1) !=
                             np.ascontiguousarray(w).view(np.int32).reshape(-1))
        assert bad.size == 0, "%s %s: %d of %d differ, first at %d: %r vs %r" % (
            what, name, bad.size, g.size, bad[0], g.reshape(-1)[bad[0]], w.reshape(-1)[bad[0]])


def padded_lattice(p, pos, per_h=2.0, pad_h=1.5):
    """a lattice reaching pad_h * h beyond the particles (and past the box where they touch it)"""
    h = F32(p.h)
    lo, hi = pos.min(0) - F32(pad_h) * h, pos.max(0) + F32(pad_h) * h
    lo = np.minimum(lo, F32(-0.5) * h)   # past the box's lower faces: zeros there
    s = h / F32(per_h)
    shape = tuple(int(v) for v in np.ceil((hi - lo) / s).astype(int) + 1)
    return tuple(float(v) for v in lo), (float(s),) * 3, shape


def iso_of(rho):
    return float(F32(0.5) * np.median(rho[rho > 0]))


def state(sph, mass):
    part = sph.syncParticles()
    return part.mPosition.reshape(-1, 3).copy(), part.mVelocity.reshape(-1, 3).copy(), mass


def emulated_lattice(p, pos, vel, mass, origin, spacing, shape):
    pts = SE.lattice_points(origin, spacing, shape).reshape(-1, 3)
    rho, v, _ = SE.Grid(p, pos, vel, mass).sample(pts)
    return rho.reshape(shape[::-1]), v.reshape(tuple(shape[::-1]) + (3,))


@pytest.fixture(scope="module")
def scenes3():
    from smoothed_particle_hydrodynamics_amd import scenes
    return {"dam": scenes.dam_break(32768, speed=0.05), "sphere": scenes.reference_sphere(16384),
            "dense": scenes.dense_block(16384)}


# ---- 1. device == emulation of the emulated lattice; closed on a padded lattice --------------------
@pytest.mark.parametrize("which", ["dam", "sphere", "dense"])
def test_mesh_matches_the_emulation_and_is_closed(scenes3, which):
    scene = scenes3[which]
    p, mass = scene[0], scene[3]
    with make(scene) as sph:
        sph.run(2)
        pos, vel, _ = state(sph, mass)
        origin, spacing, shape = padded_lattice(p, pos)
        rho, v = emulated_lattice(p, pos, vel, mass, origin, spacing, shape)
        iso = iso_of(rho)
        got = sph.extractSurface(origin, spacing, shape, iso, normals=True, velocity=True)
        plain = sph.extractSurface(origin, spacing, shape, iso, normals=False)
    want = E.extract(rho, origin, spacing, iso, velocity=v, normals=True)
    assert len(want.triangles) > 1000, which
    assert_mesh(got, want, which)
    assert same(plain.vertices, got.vertices) and same(plain.triangles, got.triangles)
    assert plain.normals is None and plain.velocity is None
    assert E.is_closed_oriented(got.triangles), which
    assert E.volume(got.vertices, got.triangles) > 0
    print("%s: lattice %s, V = %d, T = %d, chi = %d" % (which, shape, len(got.vertices), len(got.triangles),
                                                        E.euler(got.triangles)))


# ---- 2. at 4M particles, against the device's own lattice ------------------------------------------
def test_4m_mesh_matches_the_emulation_of_the_device_lattice():
    from smoothed_particle_hydrodynamics_amd import scenes
    scene = scenes.dam_break(4 * 1024 * 1024, speed=0.05)
    p, pos, vel, mass = scene
    pts = pos.reshape(-1, 3)
    lo, hi = pts.min(0), pts.max(0)
    shape = (48, 160, 208)
    spacing = tuple(float(v) for v in (hi - lo) / F32(np.array(shape) - 1) * F32(1.02))
    origin = tuple(float(v) for v in lo - F32(0.01) * (hi - lo))
    with make(scene) as sph:
        rho, v, _ = sph.sampleLattice(origin, spacing, shape)
        iso = iso_of(rho)
        got = sph.extractSurface(origin, spacing, shape, iso, normals=True, velocity=True)
    want = E.extract(rho, origin, spacing, iso, velocity=v, normals=True)
    assert len(want.triangles) > 10000
    assert_mesh(got, want, "4M")


# ---- 3. slab independence ---------------------------------------------------------------------------
def test_slab_size_does_not_change_the_bytes(scenes3, monkeypatch):
    scene = scenes3["dam"]
    p, pos0 = scene[0], scene[1].reshape(-1, 3)
    origin, spacing, shape = padded_lattice(p, pos0)
    lattices = [(origin, spacing, shape), (origin, spacing, (shape[0], shape[1], 1)),
                (origin, spacing, (shape[0], shape[1], 2)), (origin, spacing, (1, shape[1], shape[2])),
                (origin, spacing, (2, shape[1], shape[2])), (origin, spacing, (shape[0], 1, shape[2])),
                (origin, spacing, (shape[0], 2, shape[2]))]
    # mid-column planes for the thin lattices, so that they cut the fluid
    mid = tuple(float(v) for v in pos0.mean(0))
    lattices = [lattices[0]] + [((mid[0] if s[0] <= 2 else o[0], mid[1] if s[1] <= 2 else o[1],
                                  mid[2] if s[2] <= 2 else o[2]), sp, s) for o, sp, s in lattices[1:]]
    out = {}
    for planes in (None, 1, 2, 3):
        monkeypatch.delenv("SPH_HIP_SURFACE_PLANES", raising=False)
        if planes:
            monkeypatch.setenv("SPH_HIP_SURFACE_PLANES", str(planes))
        with make(scene) as sph:
            sph.run(2)
            rho, _, _ = sph.sampleLattice(*lattices[0])
            iso = iso_of(rho)
            out[planes] = [sph.extractSurface(o, s, d, iso, normals=True, velocity=True) for o, s, d in lattices]
    for planes in (1, 2, 3):
        for i, (a, b) in enumerate(zip(out[None], out[planes])):
            assert_mesh(b, a, "planes=%d lattice %d" % (planes, i))
    assert sum(len(m.vertices) for m in out[None][1:]) > 0
    assert len(out[None][0].triangles) > 1000


# ---- 4. FULL == FULL_FAST -----------------------------------------------------------------------------
def test_full_and_full_fast_give_the_same_mesh(scenes3):
    import smoothed_particle_hydrodynamics_amd as S
    scene = scenes3["dam"]
    p, mass = scene[0], scene[3]
    with make(scene) as sph:
        sph.run(2)
        pos, vel, _ = state(sph, mass)
    origin, spacing, shape = padded_lattice(p, pos)
    meshes = []
    for mode in (S.MODE_FULL, S.MODE_FULL_FAST):
        with make((p, pos.reshape(-1), vel.reshape(-1), mass), mode) as sph:
            rho, _, _ = sph.sampleLattice(origin, spacing, shape)
            meshes.append(sph.extractSurface(origin, spacing, shape, iso_of(rho), normals=True, velocity=True))
    assert_mesh(meshes[1], meshes[0], "FULL_FAST vs FULL")


# ---- 5. no effect on the run; lifetime of the kept mesh ---------------------------------------------
def snapshot(sph):
    part = sph.syncParticles()
    return [part.mPosition.copy(), part.mVelocity.copy(), part.mDensity.copy(), part.mAcceleration.copy(),
            part.mNeighborCount.copy(), np.array(sph.energy(), F32)]


def test_extraction_does_not_change_the_run(scenes3):
    import smoothed_particle_hydrodynamics_amd as S
    scene = scenes3["dam"]
    p = scene[0]
    origin, spacing, shape = padded_lattice(p, scene[1].reshape(-1, 3))
    with make(scene, S.MODE_FULL_FAST) as a:
        for _ in range(6):
            a.step()
        want = snapshot(a)
    with make(scene, S.MODE_FULL_FAST) as b:
        for _ in range(3):
            b.step()
        before = snapshot(b)
        m = b.extractSurface(origin, spacing, shape, float(F32(0.5) * np.median(before[2])), normals=True,
                             velocity=True)
        after = snapshot(b)
        for _ in range(3):
            b.step()
        got = snapshot(b)
    assert len(m.triangles) > 0
    for x, y in zip(before, after):
        assert same(x, y), "download changed across an extraction"
    for i, (x, y) in enumerate(zip(want, got)):
        assert same(x, y), "the trajectory changed (array %d)" % i


def download(sph, nv, nt, normals=True, velocity=True):
    v = np.zeros((nv, 3), F32)
    n = np.zeros((nv, 3), F32) if normals else None
    u = np.zeros((nv, 3), F32) if velocity else None
    t = np.zeros((nt, 3), np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = sph._lib.sph_hip_download_surface(sph._ctx, p(v), p(n), p(u), p(t))
    return rc, (v, t, n, u)


def test_kept_mesh_lifetime(scenes3):
    scene = scenes3["dam"]
    p = scene[0]
    origin, spacing, shape = padded_lattice(p, scene[1].reshape(-1, 3))
    with make(scene) as sph:
        lib, ctx = sph._lib, sph._ctx
        rc, _ = download(sph, 0, 0)
        assert rc == -1 and b"no mesh" in lib.sph_hip_last_error(ctx)
        sph.step()
        iso = float(F32(0.5) * np.median(sph.syncParticles().mDensity))
        a = sph.extractSurface(origin, spacing, shape, iso, normals=True, velocity=False)
        sph.run(3)
        rc, got = download(sph, len(a.vertices), len(a.triangles), velocity=False)
        assert rc == 0 and same(got[0], a.vertices) and same(got[1], a.triangles) and same(got[2], a.normals)
        rc, _ = download(sph, len(a.vertices), len(a.triangles), velocity=True)
        assert rc == -1 and b"did not compute" in lib.sph_hip_last_error(ctx)
        b = sph.extractSurface(origin, spacing, shape, 1.5 * iso, normals=False, velocity=True)
        assert not same(a.vertices, b.vertices)
        rc, _ = download(sph, len(b.vertices), len(b.triangles), normals=True, velocity=True)
        assert rc == -1
        rc, got = download(sph, len(b.vertices), len(b.triangles), normals=False, velocity=True)
        assert rc == 0 and same(got[0], b.vertices) and same(got[3], b.velocity)
        # a refused extraction keeps nothing
        o, s, d = (C.c_float * 3)(*origin), (C.c_float * 3)(*spacing), (C.c_int32 * 3)(*shape)
        assert lib.sph_hip_extract_surface(ctx, C.byref(o), C.byref(s), C.byref(d), C.c_float(-1.0), 0, None) == -1
        rc, _ = download(sph, 0, 0, normals=False, velocity=False)
        assert rc == -1


# ---- 6. refusals -----------------------------------------------------------------------------------------
def test_ref_and_slab_contexts_are_refused(scenes3):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd.lib import SphHipError, load_library
    scene = scenes3["dam"]
    p = scene[0]
    with make(scene, S.MODE_REF) as sph:
        with pytest.raises(SphHipError, match="FULL and FULL_FAST"):
            sph.extractSurface((0, 0, 0), (0.1, 0.1, 0.1), (2, 2, 2), 1.0)
    lib = load_library()
    ctx = C.c_void_p()
    params = p.copy()
    assert lib.sph_hip_create_slab(C.byref(ctx), C.byref(params), 4096, 0, 0, p.full_cells_z // 2) == 0
    try:
        o, s, d = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(0.1, 0.1, 0.1), (C.c_int32 * 3)(2, 2, 2)
        counts = (C.c_int32 * 2)()
        assert lib.sph_hip_extract_surface(ctx, C.byref(o), C.byref(s), C.byref(d), C.c_float(1.0), 0,
                                           C.byref(counts)) == -1
        assert b"slab" in lib.sph_hip_last_error(ctx)
    finally:
        lib.sph_hip_destroy(ctx)


def test_bad_arguments_are_refused(scenes3):
    from smoothed_particle_hydrodynamics_amd.lib import SphHipError
    with make(scenes3["dam"]) as sph:
        lib, ctx = sph._lib, sph._ctx
        for origin, spacing, shape in (((0, 0, 0), (0.1, 0.1, 0.1), (0, 2, 2)),
                                       ((0, 0, 0), (0.1, 0.1, 0.1), (2, -1, 2)),
                                       ((np.nan, 0, 0), (0.1, 0.1, 0.1), (2, 2, 2)),
                                       ((0, np.inf, 0), (0.1, 0.1, 0.1), (2, 2, 2)),
                                       ((0, 0, 0), (0.1, -0.1, 0.1), (2, 2, 2)),
                                       ((0, 0, 0), (0.1, 0.1, np.inf), (2, 2, 2)),
                                       ((0, 0, 0), (0.1, 0.0, 0.1), (2, 2, 2)),
                                       ((0, 0, 0), (np.nan, 0.1, 0.1), (2, 2, 2))):
            with pytest.raises(SphHipError):
                sph.extractSurface(origin, spacing, shape, 1.0)
        for iso in (0.0, -1.0, np.nan, np.inf, -np.inf):
            with pytest.raises(SphHipError, match="iso"):
                sph.extractSurface((0, 0, 0), (0.1, 0.1, 0.1), (2, 2, 2), iso)
        o, s, d = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(0.1, 0.1, 0.1), (C.c_int32 * 3)(2, 2, 2)
        for flags in (4, 8, -1, 1 << 30):
            assert lib.sph_hip_extract_surface(ctx, C.byref(o), C.byref(s), C.byref(d), C.c_float(1.0), flags,
                                               None) == -1
            assert b"flag" in lib.sph_hip_last_error(ctx)
        for ptrs in ((None, C.byref(s), C.byref(d)), (C.byref(o), None, C.byref(d)), (C.byref(o), C.byref(s), None)):
            assert lib.sph_hip_extract_surface(ctx, *ptrs, C.c_float(1.0), 0, None) == -1
        big = (C.c_int32 * 3)(2048, 1024, 1024)
        assert lib.sph_hip_extract_surface(ctx, C.byref(o), C.byref(s), C.byref(big), C.c_float(1.0), 0, None) == -1
        assert b"2^31" in lib.sph_hip_last_error(ctx)


# ---- 7. the breaking dam ---------------------------------------------------------------------------------
def test_breaking_dam_surface():
    """bench.py's 4M dam in its breaking phase (step 510): the mesh of the device's own lattice
    matches the emulation, and a lattice padded past the fluid and the box gives a closed manifold"""
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_breaking_dam import N, dam_scene
    p, pos, vel, mass = dam_scene()
    with S.SPH(N, p, mode=S.MODE_FULL_FAST) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setTiming(S.TIMING_OFF)
        sph.run(510)
        part = sph.syncParticles()
        pts = part.mPosition.reshape(-1, 3)
        h = F32(p.h)
        lo = np.minimum(pts.min(0) - F32(2) * h, F32(-0.5) * h)
        hi = pts.max(0) + F32(2) * h
        shape = (128, 128, 128)
        spacing = tuple(float(v) for v in (hi - lo) / F32(127))
        origin = tuple(float(v) for v in lo)
        rho, v, _ = sph.sampleLattice(origin, spacing, shape)
        iso = iso_of(rho)
        got = sph.extractSurface(origin, spacing, shape, iso, normals=True, velocity=True)
    want = E.extract(rho, origin, spacing, iso, velocity=v, normals=True)
    assert_mesh(got, want, "breaking dam")
    assert E.is_closed_oriented(got.triangles)
    assert E.volume(got.vertices, got.triangles) > 0
    print("breaking dam, step 510: V = %d, T = %d, chi = %d" % (len(got.vertices), len(got.triangles),
                                                               E.euler(got.triangles)))
