"""The renderer on an MI355X (include/sph_hip.h: sph_hip_render), checked bit for bit against the numpy
restatement of tests/render_emulation.py over the sampler's emulated field (tests/sample_emulation.py),
checked against the geometry of the dam column, and checked not to change the simulation."""
import ctypes as C

import numpy as np
import pytest

import render_emulation as E
import sample_emulation as SE

pytestmark = pytest.mark.gpu

F32 = np.float32


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


def flat(fr):
    """a RenderResult as the emulation's flattened Frame"""
    H, W = fr.depth.shape
    vel = fr.velocity if fr.velocity is not None else np.zeros((H, W, 3), F32)
    return E.Frame(fr.rgba.reshape(-1, 4), fr.depth.reshape(-1), fr.normal.reshape(-1, 3), vel.reshape(-1, 3),
                   fr.first_inside.reshape(-1))


def assert_frame(got, want, what, index=None):
    for name in E.Frame._fields:
        g, w = getattr(got, name), getattr(want, name)
        if index is not None:
            g = g[index]
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape, "%s %s: shape %s vs %s" % (what, name, g.shape, w.shape)
        gv = g.view(np.uint8 if g.dtype == np.uint8 else np.int32).reshape(g.shape[0], -1)
        wv = w.view(np.uint8 if w.dtype == np.uint8 else np.int32).reshape(w.shape[0], -1)
        bad = np.flatnonzero((gv != wv).any(1))
        assert bad.size == 0, "%s %s: %d of %d pixels differ, first %d: %r vs %r" % (
            what, name, bad.size, g.shape[0], bad[0], g[bad[0]], w[bad[0]])


def state(sph, mass):
    part = sph.syncParticles()
    return part.mPosition.reshape(-1, 3).copy(), part.mVelocity.reshape(-1, 3).copy(), mass


def iso_of(sph, pos):
    rho = sph.sampleFields(pos[::7], velocity=False)[0]
    return float(F32(0.5) * np.median(rho[rho > 0]))


def cameras(p, pos, rho_at):
    """outside the box, inside the box (in empty space), inside the fluid, axis-aligned, grazing"""
    from smoothed_particle_hydrodynamics_amd import Camera
    box = np.array([p.max_x, p.max_y, p.max_z], np.float64)
    lo, hi = pos.min(0).astype(np.float64), pos.max(0).astype(np.float64)
    c, ext = 0.5 * (lo + hi), hi - lo
    W, H = 64, 48
    out = {"outside": (Camera.look_at(c + np.array([0.9, 0.7, 1.6]) * box.max(), c, (0, 1, 0), 40, W, H), W, H)}
    # inside the box, away from the fluid: the emptiest of a few candidates
    cand = np.array([[fx, fy, fz] for fx in (0.1, 0.5, 0.9) for fy in (0.1, 0.5, 0.9) for fz in (0.1, 0.5, 0.9)])
    cand = cand * box
    dens = rho_at(cand.astype(F32))
    eye = cand[int(np.argmin(dens))]
    out["inside box"] = (Camera.look_at(eye, c, (0, 1, 0) if abs(eye[1] - c[1]) < 0.9 * np.linalg.norm(eye - c)
                                        else (1, 0, 0), 70, W, H), W, H)
    # inside the fluid: the particle nearest the fluid's centre, looking toward a corner of the box
    eye = pos[int(np.argmin(((pos - c) ** 2).sum(1)))].astype(np.float64)
    out["inside fluid"] = (Camera.look_at(eye, box * 0.97, (0, 1, 0), 60, W, H), W, H)
    # axis-aligned: odd sizes, so that the middle row and column have zero direction components
    W2, H2 = 65, 49
    half = 0.6 * max(ext[0], ext[1])
    out["axis"] = (Camera((c[0], c[1], hi[2] + 2.0 * ext[2] + 0.3), (0.0, 0.0, -1.0), (half / 2.0, 0, 0),
                          (0, half / 2.0 * H2 / W2, 0)), W2, H2)
    # grazing: along the fluid's top, from beyond the box
    eye = np.array([c[0], hi[1] - 0.02 * ext[1], -0.6 * box[2]])
    out["grazing"] = (Camera.look_at(eye, (c[0], hi[1] - 0.02 * ext[1], c[2]), (0, 1, 0), 30, W, H), W, H)
    return out


@pytest.fixture(scope="module")
def scenes3():
    from smoothed_particle_hydrodynamics_amd import scenes
    return {"dam": scenes.dam_break(32768, speed=0.05), "sphere": scenes.reference_sphere(16384),
            "dense": scenes.dense_block(16384)}


# ---- 1. device == emulation, five cameras, three scenes -----------------------------------------------
@pytest.mark.parametrize("which", ["dam", "sphere", "dense"])
def test_frames_match_the_emulation(scenes3, which):
    scene = scenes3[which]
    p, mass = scene[0], scene[3]
    with make(scene) as sph:
        sph.run(2)
        pos, vel, _ = state(sph, mass)
        iso = iso_of(sph, pos)
        grid = SE.Grid(p, pos, vel, mass)
        field, vfield = E.grid_fields(grid)
        hits = 0
        for name, (cam, W, H) in cameras(p, pos, field).items():
            got = sph.render(cam, W, H, iso, velocity=True)
            plain = sph.render(cam, W, H, iso)
            rp = sph.renderParams(iso)
            want = E.render(field, cam, rp, W, H, velocity_field=vfield)
            assert_frame(flat(got), want, "%s %s" % (which, name))
            for f in ("rgba", "depth", "normal", "first_inside"):
                assert same(getattr(plain, f), getattr(got, f)), "%s %s: %s with / without velocity" % (which, name, f)
            assert plain.velocity is None
            n = int((got.first_inside >= 0).sum())
            hits += n
            print("%s %s: %d of %d pixels hit" % (which, name, n, W * H))
            if name == "inside fluid":
                assert (got.first_inside == 0).mean() > 0.2
        assert hits > 2000


# ---- 2. the skip route changes no bit; FULL == FULL_FAST ----------------------------------------------
def test_skip_route_gives_the_same_bytes(scenes3, monkeypatch):
    scene = scenes3["dam"]
    p, mass = scene[0], scene[3]
    frames = {}
    for noskip in (False, True):
        monkeypatch.delenv("SPH_HIP_RENDER_NOSKIP", raising=False)
        if noskip:
            monkeypatch.setenv("SPH_HIP_RENDER_NOSKIP", "1")
        with make(scene) as sph:
            sph.run(2)
            pos, _, _ = state(sph, mass)
            iso = iso_of(sph, pos)
            cams = cameras(p, pos, lambda x: sph.sampleFields(x, velocity=False)[0])
            frames[noskip] = [sph.render(cam, W, H, iso, velocity=True, refine=r)
                              for r, (cam, W, H) in zip((8, 0, 3, 8, 12), cams.values())]
    for i, (a, b) in enumerate(zip(frames[False], frames[True])):
        for f in a._fields:
            assert same(getattr(a, f), getattr(b, f)), "camera %d: %s" % (i, f)
    assert sum(int((fr.first_inside >= 0).sum()) for fr in frames[False]) > 1000


def test_full_and_full_fast_give_the_same_frame(scenes3):
    import smoothed_particle_hydrodynamics_amd as S
    scene = scenes3["dam"]
    p, mass = scene[0], scene[3]
    with make(scene) as sph:
        sph.run(2)
        pos, vel, _ = state(sph, mass)
    out = []
    for mode in (S.MODE_FULL, S.MODE_FULL_FAST):
        with make((p, pos.reshape(-1), vel.reshape(-1), mass), mode) as sph:
            iso = iso_of(sph, pos)
            cams = cameras(p, pos, lambda x: sph.sampleFields(x, velocity=False)[0])
            out.append([sph.render(cam, W, H, iso, velocity=True) for cam, W, H in cams.values()])
    for a, b in zip(*out):
        for f in a._fields:
            assert same(getattr(a, f), getattr(b, f)), f


# ---- 3. no effect on the run ------------------------------------------------------------------------------
def snapshot(sph):
    part = sph.syncParticles()
    return [part.mPosition.copy(), part.mVelocity.copy(), part.mDensity.copy(), part.mAcceleration.copy(),
            part.mNeighborCount.copy(), np.array(sph.energy(), F32)]


def test_rendering_does_not_change_the_run(scenes3):
    import smoothed_particle_hydrodynamics_amd as S
    scene = scenes3["dam"]
    p = scene[0]
    pos0 = scene[1].reshape(-1, 3)
    with make(scene, S.MODE_FULL_FAST) as a:
        for _ in range(6):
            a.step()
        want = snapshot(a)
    with make(scene, S.MODE_FULL_FAST) as b:
        for _ in range(3):
            b.step()            # the fused integrate leaves its prehash for the next cell build
        before = snapshot(b)
        cam, W, H = cameras(p, pos0, lambda x: np.zeros(len(x), F32))["outside"]
        fr = b.render(cam, W, H, float(F32(0.5) * np.median(before[2])), velocity=True)
        after = snapshot(b)
        for _ in range(3):
            b.step()
        got = snapshot(b)
    assert (fr.first_inside >= 0).sum() > 0
    for x, y in zip(before, after):
        assert same(x, y), "download changed across a render"
    for i, (x, y) in enumerate(zip(want, got)):
        assert same(x, y), "the trajectory changed (array %d)" % i


# ---- 4. at size: the 4M column, and bench.py's dam at step 510 -------------------------------------------
def check_at_size(sph, p, pos, vel, mass, what):
    from smoothed_particle_hydrodynamics_amd import Camera
    W, H = 320, 180
    box = np.array([p.max_x, p.max_y, p.max_z], np.float64)
    c = 0.5 * box
    cam = Camera.look_at(c + np.array([1.1, 0.6, 1.5]) * box.max(), c, (0, 1, 0), 45, W, H)
    iso = iso_of(sph, pos)
    got = sph.render(cam, W, H, iso, velocity=True)
    hit = got.first_inside >= 0
    assert hit.sum() > 1000, what
    # a 16 x 16 window around a silhouette pixel, and 256 seeded random pixels, against the emulation
    edge = hit & ~np.roll(hit, 1, axis=1)
    ys, xs = np.nonzero(edge[8:H - 8, 8:W - 8])
    y0, x0 = ys[len(ys) // 2] + 8 - 8, xs[len(xs) // 2] + 8 - 8
    wy, wx = np.meshgrid(np.arange(y0, y0 + 16), np.arange(x0, x0 + 16), indexing="ij")
    rng = np.random.default_rng(11)
    ry, rx = rng.integers(0, H, 256), rng.integers(0, W, 256)
    py = np.concatenate([wy.reshape(-1), ry])
    px = np.concatenate([wx.reshape(-1), rx])
    field, vfield = E.grid_fields(SE.Grid(p, pos, vel, mass))
    want = E.render(field, cam, sph.renderParams(iso), W, H, velocity_field=vfield, pixels=(px, py))
    assert_frame(flat(got), want, what, index=py * W + px)
    assert 0 < (want.first_inside >= 0).sum() < len(px)
    # every hit pixel's depth lies inside: the sampler agrees at eye + depth * d
    yy, xx = np.nonzero(hit)
    d, ok = E.pixel_rays(cam, W, H, xx, yy)
    assert ok.all()
    pts = E.point_at(cam.eye, got.depth[yy, xx], d)
    rho = sph.sampleFields(pts, velocity=False)[0]
    assert (rho > F32(iso)).all(), "%s: %d hit pixels are not inside" % (what, int((rho <= F32(iso)).sum()))
    return got


def test_4m_column_at_size():
    from smoothed_particle_hydrodynamics_amd import scenes
    scene = scenes.dam_break(4 * 1024 * 1024, speed=0.05)
    p, pos, vel, mass = scene
    with make(scene) as sph:
        check_at_size(sph, p, pos.reshape(-1, 3), vel.reshape(-1, 3), mass, "4M column")


def test_breaking_dam_at_size():
    """bench.py's 4M dam in its breaking phase (step 510), built as tests/test_gpu_surface.py builds it"""
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_breaking_dam import N, dam_scene
    p, pos, vel, mass = dam_scene()
    with S.SPH(N, p, mode=S.MODE_FULL_FAST) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setTiming(S.TIMING_OFF)
        sph.run(510)
        pos, vel, _ = state(sph, mass)
        check_at_size(sph, p, pos, vel, mass, "breaking dam, step 510")


# ---- 5. geometry of the column at rest, independent of the emulation ------------------------------------
def test_column_geometry():
    from smoothed_particle_hydrodynamics_amd import Camera, scenes
    p, pos, vel, mass = scenes.dam_break(262144)
    pts = pos.reshape(-1, 3)
    h = float(p.h)
    top = np.array(scenes.dam_break_params(262144)[1], np.float64)   # the column [0, top]
    W, H = 64, 96
    eye = (0.05, 0.375, 1.9)
    cam = Camera.look_at(eye, (0.05, 0.375, 0.0), (0, 1, 0), 50, W, H)
    with make((p, pos, vel, mass)) as sph:
        # a quarter of the median density: the random fill's face is rough at half the median
        # (the level wanders by up to 2h), while f is 0 at h beyond the outermost particle whatever the iso
        iso = float(F32(0.5) * F32(iso_of(sph, pts)))
        fr = sph.render(cam, W, H, iso)
    py, px = np.divmod(np.arange(W * H), W)
    d, _ = E.pixel_rays(cam, W, H, px, py)
    d = d.astype(np.float64)
    e = np.array(eye, np.float64)

    def enter(lo, hi):
        with np.errstate(divide="ignore", invalid="ignore"):
            t0, t1 = (lo - e) / d, (hi - e) / d
        tn = np.nanmax(np.minimum(t0, t1), 1)
        tf = np.nanmin(np.maximum(t0, t1), 1)
        return np.where(tn <= tf, tn, np.nan)

    hit = fr.first_inside.reshape(-1) >= 0
    grown = enter(np.full(3, -2 * h), top + 2 * h)
    shrunk = enter(np.full(3, 2 * h), top - 2 * h)
    assert not hit[np.isnan(grown)].any(), "a pixel is hit whose ray misses the column grown by 2h"
    inner = ~np.isnan(shrunk)
    assert inner.sum() > 300
    assert hit[inner].mean() >= 0.99, hit[inner].mean()
    t_col = enter(np.zeros(3), top)
    sel = inner & hit
    err = np.abs(fr.depth.reshape(-1)[sel] - t_col[sel])
    assert err.max() <= h, (err.max(), h)


# ---- 6. edge cases and refusals --------------------------------------------------------------------------------
def test_empty_context_renders_background():
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import Camera, scenes
    p = scenes.dam_break(32768)[0]
    with S.SPH(32768, p, mode=S.MODE_FULL, device=0) as sph:
        cam = Camera.look_at((0.5, 0.5, 3.0), (0.05, 0.4, 0.5), (0, 1, 0), 40, 40, 30)
        fr = sph.render(cam, 40, 30, 1.0, velocity=True, background=(1, 2, 3, 4))
    assert (fr.rgba == [1, 2, 3, 4]).all() and np.isinf(fr.depth).all() and (fr.depth > 0).all()
    assert (fr.normal == 0).all() and (fr.velocity == 0).all() and (fr.first_inside == -1).all()


def test_refusals_leave_a_working_context(scenes3):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import Camera
    from smoothed_particle_hydrodynamics_amd.lib import SphHipError, load_library
    from test_render_cpu import REFUSALS, apply
    scene = scenes3["dam"]
    p, pos = scene[0], scene[1].reshape(-1, 3)
    cam0 = Camera.look_at((0.5, 0.5, 3.0), (0.05, 0.4, 0.5), (0, 1, 0), 40, 32, 24)
    with make(scene) as sph:
        lib, ctx = sph._lib, sph._ctx
        iso = iso_of(sph, pos)
        want = sph.render(cam0, 32, 24, iso)
        px = lambda a: a.ctypes.data_as(C.c_void_p)
        rgba = np.zeros((24, 32, 4), np.uint8)
        for what, mut, w, h, flags, msg in REFUSALS:
            cam, rp = cam0.as_struct(), sph.renderParams(iso)
            apply(cam, rp, mut)
            rc = lib.sph_hip_render(ctx, C.byref(cam), C.byref(rp), w, h, flags, px(rgba), None, None, None, None)
            assert rc == -1, what
            assert msg in lib.sph_hip_last_error(ctx), what
        assert lib.sph_hip_render(ctx, None, C.byref(sph.renderParams(iso)), 32, 24, 0, None, None, None, None,
                                  None) == -1
        got = sph.render(cam0, 32, 24, iso)
        for f in want._fields:
            assert same(getattr(want, f), getattr(got, f)), f
        assert (got.first_inside >= 0).any()
    with make(scene, S.MODE_REF) as sph:
        with pytest.raises(SphHipError, match="FULL and FULL_FAST"):
            sph.render(cam0, 8, 8, 1.0)
    lib = load_library()
    ctx = C.c_void_p()
    params = p.copy()
    assert lib.sph_hip_create_slab(C.byref(ctx), C.byref(params), 4096, 0, 0, p.full_cells_z // 2) == 0
    try:
        from test_render_cpu import good
        cam, rp = good()
        assert lib.sph_hip_render(ctx, C.byref(cam), C.byref(rp), 8, 8, 0, None, None, None, None, None) == -1
        assert b"slab" in lib.sph_hip_last_error(ctx)
    finally:
        lib.sph_hip_destroy(ctx)
