"""The scalar renderer on an MI355X (include/sph_hip.h: sph_hip_render_scalars): the frame's fluid pixels coloured
by a carried channel, SURFACE and COLUMN, checked bit for bit - rgba, depth, normal, velocity, first_inside,
solid_id and scalar - against the numpy restatement (tests/tint_emulation.py on top of render_emulation,
scene_emulation and the scalar sampler's sums), checked against the two renderers where they must agree, and
checked not to change the run.  The skip route is read at context creation, so it runs in child processes (this
file with a word)."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import render_emulation as E
import sample_emulation as SE
import scene_emulation as SCN
import tint_emulation as TE
from test_gpu_render import cameras, iso_of, make, same, snapshot, state
from test_gpu_scalars import N, block_scene
from test_gpu_scene_render import DEFAULT, assert_scene

pytestmark = pytest.mark.gpu

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MODES = {TE.SURFACE: "surface", TE.COLUMN: "column"}


def flat(fr):
    """a ScalarRenderResult as the emulation's flattened TintFrame"""
    H, W = fr.depth.shape
    vel = fr.velocity if fr.velocity is not None else np.zeros((H, W, 3), F32)
    sid = fr.solid_id if fr.solid_id is not None else np.full((H, W), -1, np.int32)
    return TE.TintFrame(fr.rgba.reshape(-1, 4), fr.depth.reshape(-1), fr.normal.reshape(-1, 3), vel.reshape(-1, 3),
                        fr.first_inside.reshape(-1), sid.reshape(-1), fr.scalar.reshape(-1))


def assert_tint(got, want, what, index=None):
    """all seven outputs bit for bit"""
    assert_scene(got, want, what, index)
    g = got.scalar if index is None else got.scalar[index]
    bad = np.flatnonzero(g.view(np.int32) != want.scalar.view(np.int32))
    assert bad.size == 0, "%s scalar: %d pixels differ, first %d: %r vs %r" % (what, bad.size, bad[0], g[bad[0]],
                                                                              want.scalar[bad[0]])


def with_scalars(scene, T, kappa, mode=None):
    sph = make(scene[:4], mode)
    sph.setScalars(T, kappa)
    return sph


class Restated:
    """the restatement of one state: the fluid pass's frames and the fluid pixels' values, computed once per view"""

    def __init__(self, sph, p, mass, solids=None, velocities=None):
        self.sph, self.p = sph, p
        self.pos, self.vel, _ = state(sph, mass)
        self.T = sph.getScalars()
        self.walk = TE.Walk(p, self.pos, self.vel, mass, self.T)
        self.fields = E.grid_fields(self.walk.grid)
        self.solids, self.velocities = solids, velocities
        self.cache = {}

    def frame(self, key, iso, cam, W, H, velocity, pixels, render_args):
        k = ("frame", key, velocity)
        if k not in self.cache:
            rp = self.sph.renderParams(iso, **render_args)
            fr = E.render(self.fields[0], cam, rp, W, H, velocity_field=self.fields[1] if velocity else None,
                          pixels=pixels)
            if self.solids is not None:
                fr = SCN.composite(fr, self.solids, cam, rp, DEFAULT, W, H, self.velocities, None, velocity, pixels)
            self.cache[k] = (rp, fr)
        return self.cache[k]

    def want(self, key, iso, cam, W, H, channel, mode, lo, hi, table, flat_=False, velocity=True, pixels=None,
             **render_args):
        """the TintFrame; `key` names the view (camera, size, pixels and render arguments) for the cache"""
        rp, fr = self.frame(key, iso, cam, W, H, velocity, pixels, render_args)
        k = ("values", key, mode)
        if k not in self.cache:
            self.cache[k] = TE.values(fr, self.walk, cam, rp, mode, W, H, pixels)
        v = self.cache[k][:, channel]
        return TE.tint(fr, None, cam, rp, TE.Tint(channel, mode, lo, hi, TE.FLAT if flat_ else 0), table, W, H, pixels,
                       v=v)


def seeded_table(n, seed=4):
    t = np.random.default_rng(seed).uniform(0.0, 1.0, (n, 3)).astype(F32)
    t[::3] = np.random.default_rng(seed + 1).uniform(-0.5, 1.8, t[::3].shape).astype(F32)
    return t


RANGES = {TE.SURFACE: (-0.05, 0.08), TE.COLUMN: (-0.003, 0.004)}     # values fall outside both


# ---- 1. the seeded block: every channel, both modes, FLAT and shaded, 2 and 256 rows --------------------------
@pytest.fixture(scope="module")
def block():
    p, pos, vel, mass, T, kappa = block_scene()
    return (p, pos, vel, mass), T, kappa


@pytest.mark.parametrize("view", ["outside", "inside fluid", "grazing"])
def test_block_frames_match_the_restatement(block, view):
    scene, T, kappa = block
    p, mass = scene[0], scene[3]
    with with_scalars(scene, T, kappa) as sph:
        sph.run(3)
        R = Restated(sph, p, mass)
        assert (R.T < 0).any() and (np.abs(R.T) > 0.5).any()
        iso = iso_of(sph, R.pos)
        cam, W, H = cameras(p, R.pos, R.fields[0])[view]
        tinted = 0
        for mode in (TE.SURFACE, TE.COLUMN):
            lo, hi = RANGES[mode]
            for channel in range(4):
                for flat_ in (False, True):
                    for rows in (2, 256):
                        table = seeded_table(rows)
                        got = sph.renderScalars(cam, W, H, iso, channel, (lo, hi), table, MODES[mode], flat_,
                                                velocity=True)
                        want = R.want(view, iso, cam, W, H, channel, mode, lo, hi, table, flat_)
                        assert_tint(flat(got), want, "block %s %s ch%d flat=%s rows=%d" % (view, MODES[mode], channel,
                                                                                          flat_, rows))
                        assert got.solid_id is None
            hit = want.first_inside >= 0
            tinted += int(hit.sum())
            v = want.scalar[hit]
            print("block %s %s: %d of %d pixels tinted, scalar %.4g .. %.4g" % (view, MODES[mode], hit.sum(), W * H,
                                                                                v.min(), v.max()))
            assert ((v < lo) | (v > hi)).any() and (want.scalar[~hit] == 0).all()
        if view == "inside fluid":
            assert (want.first_inside == 0).mean() > 0.2
        assert tinted > 200


def test_full_and_full_fast_give_the_same_bytes(block):
    import smoothed_particle_hydrodynamics_amd as S
    scene, T, kappa = block
    p, mass = scene[0], scene[3]
    with with_scalars(scene, T, kappa) as sph:
        sph.run(3)
        pos, vel, _ = state(sph, mass)
        Tk = sph.getScalars()
    out = []
    for mode in (S.MODE_FULL, S.MODE_FULL_FAST):
        with with_scalars((p, pos.reshape(-1), vel.reshape(-1), mass), Tk, kappa, mode) as sph:
            iso = iso_of(sph, pos)
            field = lambda pts: sph.sampleFields(pts, velocity=False)[0]
            frames = []
            for cam, W, H in cameras(p, pos, field).values():
                for m in ("surface", "column"):
                    frames.append(sph.renderScalars(cam, W, H, iso, 1, RANGES[TE.COLUMN], seeded_table(17), m,
                                                    velocity=True))
            out.append(frames)
    for a, b in zip(*out):
        for f in a._fields:
            assert same(getattr(a, f), getattr(b, f)), f
    assert sum(int((fr.first_inside >= 0).sum()) for fr in out[0]) > 1000


# ---- 2. the dyed dam ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dyed():
    from smoothed_particle_hydrodynamics_amd import scenes
    return scenes.dam_break_dyed(20000)


def test_dyed_dam_surface_column_and_section(dyed):
    from smoothed_particle_hydrodynamics_amd import Camera, colormaps, scenes
    p, mass, T, kappa = dyed[0], dyed[3], dyed[4], dyed[5]
    W, H = 64, 48
    with with_scalars(dyed, T, kappa) as sph:
        sph.run(20)
        R = Restated(sph, p, mass)
        iso = iso_of(sph, R.pos)
        c = 0.5 * (R.pos.min(0) + R.pos.max(0)).astype(np.float64)
        cam = Camera.look_at(c + [0.5, 0.6, 1.6], c, (0, 1, 0), 40, W, H)
        # SURFACE: a concentration is a convex combination of 0 and 1 up to the sums' roundings
        got = sph.renderScalars(cam, W, H, iso, 0, (0.0, 1.0), colormaps.dye((0.9, 0.1, 0.2)))
        assert_tint(flat(got), R.want("front", iso, cam, W, H, 0, TE.SURFACE, 0.0, 1.0, colormaps.dye((0.9, 0.1, 0.2)),
                                      velocity=False), "dyed surface")
        hit = got.first_inside >= 0
        v = got.scalar[hit]
        print("dyed surface: %d pixels, scalar %.6f .. %.6f, %d below 0.5, %d above" % (hit.sum(), v.min(), v.max(),
                                                                                        (v < 0.5).sum(), (v > 0.5).sum()))
        assert hit.sum() > 300 and v.min() >= 0.0 and v.max() <= 1.0 + 2.0 ** -20
        assert (v < 0.5).any() and (v > 0.5).any()
        # COLUMN with dye(): the dye's depth along the ray
        table = colormaps.dye((0.9, 0.1, 0.2), n=5)
        got = sph.renderScalars(cam, W, H, iso, 0, (0.0, 0.1), table, "column")
        assert_tint(flat(got), R.want("front", iso, cam, W, H, 0, TE.COLUMN, 0.0, 0.1, table, velocity=False),
                    "dyed column")
        assert (got.scalar[hit] > 0).any() and (got.scalar[~hit] == 0).all()
        # the FLAT section: the marched box cut at the tank's mid-plane, seen from the cut side
        box = scenes.dyed_cut_box(p)
        eye = (float(c[0]), float(c[1]), float(p.max_z) + 1.2)
        cam = Camera.look_at(eye, (float(c[0]), float(c[1]), 0.0), (0, 1, 0), 40, W, H)
        got = sph.renderScalars(cam, W, H, iso, 0, (0.0, 1.0), colormaps.heat(), flat=True, box=box)
        want = R.want("section", iso, cam, W, H, 0, TE.SURFACE, 0.0, 1.0, colormaps.heat(), True, velocity=False,
                      box=box)
        assert_tint(flat(got), want, "dyed section")
        cut = got.first_inside == 0
        print("dyed section: %d pixels enter inside the fluid" % cut.sum())
        assert cut.sum() > 100 and (got.scalar[cut] > 0.5).any() and (got.scalar[cut] < 0.5).any()


# ---- 3. the heated floor: the interior shows where the surface does not ------------------------------------------------
def test_heated_floor_column_sees_below_the_surface():
    from smoothed_particle_hydrodynamics_amd import Camera, scenes
    # an explicit step carries a (tiny) non-zero value one kernel radius further, so after 20 steps the heat has
    # reached 22 radii above the floor at the most: a pool 29 radii deep keeps its surface at exactly the initial 0
    scene = scenes.heated_floor(200000, depth=1.0)
    assert 1.0 / float(scene[0].h) > 26
    p, T, kappa, sources = scene[0], scene[4], scene[5], scene[6]
    W, H = 64, 48
    with with_scalars(scene, T, kappa) as sph:
        sph.setScalarSources(sources)
        sph.run(20)
        pos = state(sph, scene[3])[0]
        iso = iso_of(sph, pos)
        cam = Camera.look_at((0.5, 2.6, 0.9), (0.5, 1.0, 0.5), (0, 0, -1), 40, W, H)
        surf = sph.renderScalars(cam, W, H, iso, 0, (0.0, 1.0))
        col = sph.renderScalars(cam, W, H, iso, 0, (0.0, 0.05), mode="column")
        for f in ("depth", "normal", "first_inside"):
            assert same(getattr(surf, f), getattr(col, f)), f
        hit = surf.first_inside >= 0
        cold = hit & (surf.scalar.view(np.int32) == 0)         # exactly the initial value, +0
        print("heated floor: %d hit pixels, %d with the initial value at the surface, surface %.4g .. %.4g" % (
            hit.sum(), cold.sum(), surf.scalar[hit].min(), surf.scalar[hit].max()))
        # the rays that reach the heated layer (y = h) inside the tank; a ray near the frame's edge leaves the fluid
        # through a side wall above it and has met nothing warm
        py, px = np.divmod(np.arange(W * H), W)
        d = E.pixel_rays(cam, W, H, px, py)[0].astype(np.float64)
        h = float(p.h)
        t = (h - 2.6) / d[:, 1]
        x, z = 0.5 + t * d[:, 0], 0.9 + t * d[:, 2]
        deep = ((x > 2 * h) & (x < 1.0 - 2 * h) & (z > 2 * h) & (z < 1.0 - 2 * h)).reshape(H, W) & cold
        print("%d of them reach the heated layer, column there %.4g .. %.4g; %d of the others are 0" % (
            deep.sum(), col.scalar[deep].min(), col.scalar[deep].max(), (col.scalar[cold & ~deep] == 0).sum()))
        assert cold.sum() > 500 and deep.sum() > 300 and (col.scalar[deep] > 0).all()
        assert (col.rgba[cold] != surf.rgba[cold]).any()


# ---- 4. solids ---------------------------------------------------------------------------------------------------------
def test_pillar_scene_with_scalars():
    from smoothed_particle_hydrodynamics_amd import scenes
    from test_gpu_scene_render import pillar_cameras
    scene = scenes.dam_break_pillar(20000)
    p, mass, obst = scene[0], scene[3], scene[4]
    T = np.random.default_rng(12).uniform(-1.0, 1.0, (mass.size, 4)).astype(F32)
    with with_scalars(scene, T, np.zeros(4, F32)) as sph:
        sph.setObstacles(obst)
        sph.run(2)
        R = Restated(sph, p, mass, solids=obst)
        iso = iso_of(sph, R.pos)
        views = pillar_cameras(p, R.pos, obst[0])
        table = seeded_table(17)
        for name in ("outside", "grazing"):
            cam, W, H = views[name]
            scene_fr = sph.render(cam, W, H, iso, velocity=True, solids=True)
            for mode in (TE.SURFACE, TE.COLUMN):
                got = sph.renderScalars(cam, W, H, iso, 3, (-0.5, 0.5), table, MODES[mode], velocity=True, solids=True)
                assert_tint(flat(got), R.want(name, iso, cam, W, H, 3, mode, -0.5, 0.5, table), "pillar %s %s" % (
                    name, MODES[mode]))
                solid = got.solid_id >= 0
                fluid = got.first_inside >= 0
                assert solid.sum() > 50 and fluid.sum() > 50 and not (solid & fluid).any()
                # a solid's pixels carry the scene renderer's bytes and no scalar; so does every miss
                for f in ("rgba", "depth", "normal", "velocity", "first_inside", "solid_id"):
                    a, b = getattr(got, f), getattr(scene_fr, f)
                    assert same(a[~fluid], b[~fluid]), f
                    if f != "rgba":
                        assert same(a, b), f
                assert (got.scalar[~fluid] == 0).all()
                assert (got.rgba[fluid] != scene_fr.rgba[fluid]).any(1).mean() > 0.9     # and the fluid is tinted


# ---- 5. equalities with the two renderers ----------------------------------------------------------------------------
def test_equalities_with_the_renderers(block):
    scene, T, kappa = block
    p, mass = scene[0], scene[3]
    albedo = (0.25, 0.55, 0.9)
    with with_scalars(scene, T, kappa) as sph:
        sph.run(3)
        pos = state(sph, mass)[0]
        iso = iso_of(sph, pos)
        field = lambda pts: sph.sampleFields(pts, velocity=False)[0]
        for name, (cam, W, H) in cameras(p, pos, field).items():
            plain = sph.render(cam, W, H, iso, velocity=True, albedo=albedo)
            scene_fr = sph.render(cam, W, H, iso, velocity=True, albedo=albedo, solids=True)
            for mode in ("surface", "column"):
                # no scene params == scene params without obstacles
                a = sph.renderScalars(cam, W, H, iso, 2, (-0.3, 0.3), seeded_table(9), mode, velocity=True)
                b = sph.renderScalars(cam, W, H, iso, 2, (-0.3, 0.3), seeded_table(9), mode, velocity=True, solids=True)
                assert a.solid_id is None and (b.solid_id == -1).all()
                for f in ("rgba", "depth", "normal", "velocity", "first_inside", "scalar"):
                    assert same(getattr(a, f), getattr(b, f)), (name, mode, f)
                for f in ("depth", "normal", "velocity", "first_inside"):
                    assert same(getattr(a, f), getattr(plain, f)), (name, mode, f)
                # two equal rows of the albedo, shaded: render_byte(albedo_c * w) is the renderer's expression
                c = sph.renderScalars(cam, W, H, iso, 2, (-0.3, 0.3), np.array([albedo, albedo], F32), mode,
                                      velocity=True, albedo=albedo, solids=True)
                for f in ("rgba", "depth", "normal", "velocity", "first_inside", "solid_id"):
                    assert same(getattr(c, f), getattr(scene_fr, f)), (name, mode, f)
                assert same(c.scalar, b.scalar)


# ---- 6. the skip route, in child processes -----------------------------------------------------------------------------
def child_frames():
    """the block's frames, both modes, from outside and from inside the fluid: a digest per output"""
    scene, T, kappa = (lambda s: (s[:4], s[4], s[5]))(block_scene())
    p, mass = scene[0], scene[3]
    out = {}
    with with_scalars(scene, T, kappa) as sph:
        sph.run(3)
        pos = state(sph, mass)[0]
        iso = iso_of(sph, pos)
        field = lambda pts: sph.sampleFields(pts, velocity=False)[0]
        views = cameras(p, pos, field)
        for name in ("outside", "inside fluid", "inside box"):
            cam, W, H = views[name]
            for mode in ("surface", "column"):
                fr = sph.renderScalars(cam, W, H, iso, 1, RANGES[TE.COLUMN], seeded_table(17), mode, velocity=True)
                for f in fr._fields:
                    if getattr(fr, f) is not None:
                        out["%s %s %s" % (name, mode, f)] = hashlib.sha256(
                            np.ascontiguousarray(getattr(fr, f)).tobytes()).hexdigest()
                out["%s %s hits" % (name, mode)] = int((fr.first_inside >= 0).sum())
    return out


def test_skip_route_gives_the_same_bytes():
    outs = []
    for noskip in ("0", "1"):
        env = dict(os.environ, SPH_HIP_RENDER_NOSKIP=noskip)
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "frames"], env=env, capture_output=True,
                             text=True, cwd=ROOT, timeout=300)
        assert run.returncode == 0, run.stdout + run.stderr
        outs.append(json.loads(run.stdout.strip().splitlines()[-1]))
    assert outs[0] == outs[1], sorted(k for k in outs[0] if outs[0][k] != outs[1].get(k))
    assert outs[0]["outside column hits"] > 100 and outs[0]["inside fluid surface hits"] > 100


# ---- 7. chunks and a ragged frame -----------------------------------------------------------------------------------------
def test_two_chunks_and_a_ragged_frame(block):
    from smoothed_particle_hydrodynamics_amd import Camera
    scene, T, kappa = block
    p, mass = scene[0], scene[3]
    with with_scalars(scene, T, kappa) as sph:
        sph.run(3)
        R = Restated(sph, p, mass)
        iso = iso_of(sph, R.pos)
        c = 0.5 * (R.pos.min(0) + R.pos.max(0)).astype(np.float64)
        ext = (R.pos.max(0) - R.pos.min(0)).astype(np.float64)
        W, H = 16384, 104
        rows = ((64 << 20) - 7 * 256) // (W * 40) // 8 * 8
        assert rows == 96 and rows < H
        # seen from +x, looking at a point above the column: the rows on either side of the chunk boundary, near the
        # frame's bottom, cross the column's face along its whole width in z
        aim = np.array([c[0], R.pos[:, 1].max() + 0.05 * ext[1], c[2]])
        cam = Camera.look_at(aim + [1.5, 0, 0], aim, (0, 1, 0), 35, W, H)
        table = seeded_table(17)
        got = sph.renderScalars(cam, W, H, iso, 1, (-0.5, 0.5), table, velocity=True)
        rng = np.random.default_rng(8)
        py = np.concatenate([rng.integers(0, H, 4096), np.repeat(np.arange(rows - 2, rows + 2), W)])
        px = np.concatenate([rng.integers(0, W, 4096), np.tile(np.arange(W), 4)])
        hit_cols = np.flatnonzero((got.first_inside >= 0).any(0))
        assert hit_cols.size > 20
        px[:2048] = rng.choice(hit_cols, 2048)                 # weigh the random pixels toward the fluid
        want = R.want("two chunks", iso, cam, W, H, 1, TE.SURFACE, -0.5, 0.5, table, pixels=(px, py))
        assert_tint(flat(got), want, "two chunks", index=py * W + px)
        for r in range(rows - 2, rows + 2):
            assert (got.first_inside[r] >= 0).sum() > 20, r
        assert (want.first_inside[:4096] >= 0).sum() > 20
        W, H = 13, 7
        cam = Camera.look_at(c + [0.4, 0.3, 1.1], c, (0, 1, 0), 40, W, H)
        for mode in (TE.SURFACE, TE.COLUMN):
            got = sph.renderScalars(cam, W, H, iso, 1, RANGES[mode], table, MODES[mode], velocity=True)
            assert_tint(flat(got), R.want("13x7", iso, cam, W, H, 1, mode, RANGES[mode][0], RANGES[mode][1], table),
                        "13x7 " + MODES[mode])
            assert (got.first_inside >= 0).sum() > 5


# ---- 8. max_samples cuts columns short ----------------------------------------------------------------------------------
def test_max_samples_cuts_the_columns(block):
    scene, T, kappa = block
    p, mass = scene[0], scene[3]
    with with_scalars(scene, T, kappa) as sph:
        sph.run(3)
        R = Restated(sph, p, mass)
        iso = iso_of(sph, R.pos)
        cam, W, H = cameras(p, R.pos, R.fields[0])["outside"]
        whole = sph.renderScalars(cam, W, H, iso, 2, RANGES[TE.COLUMN], seeded_table(17), "column")
        first = whole.first_inside[whole.first_inside >= 0]
        M = int(np.median(first)) + 1
        table = seeded_table(17)
        got = sph.renderScalars(cam, W, H, iso, 2, RANGES[TE.COLUMN], table, "column", velocity=True, max_samples=M)
        want = R.want("cut", iso, cam, W, H, 2, TE.COLUMN, RANGES[TE.COLUMN][0], RANGES[TE.COLUMN][1], table,
                      max_samples=M)
        assert_tint(flat(got), want, "max_samples %d" % M)
        last = got.first_inside == M - 1
        kept = got.first_inside >= 0
        print("max_samples %d: %d hits of %d kept, %d with first_inside at the last sample" % (
            M, kept.sum(), first.size, last.sum()))
        assert last.sum() > 0 and 0 < kept.sum() < first.size
        # such a column is its one sample; and a column cut short differs from the whole one
        one = sph.renderScalars(cam, W, H, iso, 2, (-1.0, 1.0), table, "surface", max_samples=M)
        assert (np.abs(got.scalar[last]) <= np.float32(sph.renderParams(iso).step) * 1.0001).all()
        assert same(one.first_inside, got.first_inside)
        both = kept & (whole.first_inside < M - 1)
        assert (got.scalar[both] != whole.scalar[both]).any()


# ---- 9. the channel exactly 1: the fluid's thickness ------------------------------------------------------------------------
def test_unit_channel_column_is_the_thickness(block):
    scene, _, kappa = block
    p, mass = scene[0], scene[3]
    T = np.zeros((N, 4), F32)
    T[:, 3] = 1.0
    with with_scalars(scene, T, np.zeros(4, F32)) as sph:
        sph.run(3)
        R = Restated(sph, p, mass)
        iso = iso_of(sph, R.pos)
        cam, W, H = cameras(p, R.pos, R.fields[0])["outside"]
        got = sph.renderScalars(cam, W, H, iso, 3, (0.0, 0.2), mode="column")
        surf = sph.renderScalars(cam, W, H, iso, 3, (0.0, 1.0))
        rp = sph.renderParams(iso)
        fr = E.render(R.fields[0], cam, rp, W, H)
        h = np.flatnonzero(fr.first_inside >= 0)
        py, px = np.divmod(h, W)
        _, count = TE.column(R.walk, cam, rp, W, H, px, py, fr.first_inside[h], 3)
        step = F32(rp.step)
        want = np.zeros(W * H, F32)
        for i, n in zip(h, count):
            acc = F32(0.0)
            for _ in range(int(n)):
                acc = F32(acc + step)
            want[i] = acc
        assert same(got.scalar.reshape(-1), want) and count.min() >= 1 and count.max() > 3
        assert (surf.scalar.reshape(-1)[h] == 1.0).all()


# ---- 10. the run is unchanged --------------------------------------------------------------------------------------------------
def test_a_tint_frame_does_not_change_the_run():
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import Camera, scenes
    gate = scenes.dam_break_gate(20000, 0.5)
    n = gate[3].size
    T = np.random.default_rng(2).uniform(0.0, 1.0, (n, 4)).astype(F32)
    kappa = np.array([0.0, 1.0, 0.5, 0.0], F32) * F32(scenes.scalar_stable_kappa(gate[0], 0.1))
    # from upstream of the gate: the column's free face and, beside it, the gate
    c = np.array([float(gate[4][0].hi[0]), 0.4 * gate[0].max_y, 0.5 * gate[0].max_z])
    cam = Camera.look_at(c + [-0.9, 0.6, 1.4], c, (0, 1, 0), 45, 64, 48)

    def start():
        sph = with_scalars(gate, T, kappa, S.MODE_FULL_FAST)
        sph.setObstacles(gate[4])
        sph.setObstacleMotion(gate[5])
        return sph

    def everything(sph):
        return snapshot(sph) + [sph.getScalars(), np.array([sph.getObstacleMotion()[1]], F32)]

    with start() as a:
        for _ in range(13):
            a.step()
        want = everything(a)
    with start() as b:
        for _ in range(3):
            b.step()
        before = everything(b)
        iso = float(F32(0.5) * np.median(before[2]))
        frames = [b.renderScalars(cam, 64, 48, iso, 1, (0.0, 1.0), mode=m, velocity=True, solids=True)
                  for m in ("surface", "column")]
        after = everything(b)
        for _ in range(10):
            b.step()
        got = everything(b)
    for fr in frames:
        assert (fr.solid_id >= 0).any() and (fr.first_inside >= 0).sum() > 100 and (fr.scalar != 0).any()
    for i, (x, y) in enumerate(zip(before, after)):
        assert same(x, y), "array %d changed across a tint frame" % i
    for i, (x, y) in enumerate(zip(want, got)):
        assert same(x, y), "the trajectory changed (array %d)" % i


# ---- 11. refusals on the device path, and nothing resident ------------------------------------------------------------------
def test_refusals_name_the_entry_point(block):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import Camera
    from smoothed_particle_hydrodynamics_amd.lib import SphHipError, SphTintParams, load_library
    from test_render_cpu import good
    scene, T, kappa = block
    p = scene[0]
    cam0 = Camera.look_at((1.3, 0.9, 1.9), (0.05, 0.35, 0.5), (0, 1, 0), 45, 32, 24)
    who = "sph_hip_render_scalars: "
    with make(scene, S.MODE_REF) as sph:
        with pytest.raises(SphHipError, match=who + "FULL and FULL_FAST"):
            sph.renderScalars(cam0, 8, 8, 1.0, 0, (0, 1))
    with make(scene) as sph:
        with pytest.raises(SphHipError, match=who + "the context carries no scalars"):
            sph.renderScalars(cam0, 32, 24, 1.0, 0, (0, 1))
        sph.setScalars(T, kappa)
        iso = iso_of(sph, scene[1].reshape(-1, 3))
        want = sph.renderScalars(cam0, 32, 24, iso, 0, (0, 1), mode="column", solids=True)
        for kw, text in ((dict(channel=4), "channel must be 0 .. 3"), (dict(channel=-1), "channel must be 0 .. 3"),
                         (dict(value_range=(1.0, 1.0)), "tint range needs lo < hi"),
                         (dict(value_range=(0.0, np.inf)), "tint range must be finite"),
                         (dict(colormap=np.zeros((1, 3), F32)), r"n_colors must be in \[2, 256\]"),
                         (dict(colormap=np.zeros((257, 3), F32)), r"n_colors must be in \[2, 256\]"),
                         (dict(colormap=np.array([[0, 0, 0], [np.nan, 0, 0]], F32)),
                          "a colour table entry that is not finite"),
                         (dict(step=0.0), "step must be > 0"),
                         (dict(solids=True, solid_colors=np.zeros((2, 3), F32)), "the albedo count"),
                         (dict(solids=True, solid_albedo=(0.5, np.nan, 0.5)), "scene params must be finite")):
            args = dict(channel=0, value_range=(0.0, 1.0))
            args.update(kw)
            with pytest.raises(SphHipError, match=who + text):
                sph.renderScalars(cam0, 32, 24, 1.0, **args)
        lib, ctx = sph._lib, sph._ctx
        cam, rp = cam0.as_struct(), sph.renderParams(iso)
        table = np.array([[0, 0, 0], [1, 1, 1]], F32)
        tptr = table.ctypes.data_as(C.c_void_p)
        alb = np.zeros((1, 3), F32)

        def call(tp, table_=tptr, albedo=None, n_albedo=0, flags=0):
            return lib.sph_hip_render_scalars(ctx, C.byref(cam), C.byref(rp), None, albedo, n_albedo,
                                              None if tp is None else C.byref(tp), table_, 32, 24, flags, None, None,
                                              None, None, None, None, None)

        for args, text in (((None,), b"null tint params or colour table"),
                           ((SphTintParams(0, 0, 0.0, 1.0, 2, 0), None), b"null tint params or colour table"),
                           ((SphTintParams(0, 2, 0.0, 1.0, 2, 0),), b"unknown tint mode"),
                           ((SphTintParams(0, 0, 0.0, 1.0, 2, 2),), b"unknown tint flag bits"),
                           ((SphTintParams(0, 0, 0.0, 1.0, 2, 0), tptr, alb.ctypes.data_as(C.c_void_p), 0),
                            b"solid albedos without scene params"),
                           ((SphTintParams(0, 0, 0.0, 1.0, 2, 0), tptr, None, 1), b"solid albedos without scene params"),
                           ((SphTintParams(0, 0, 0.0, 1.0, 2, 0), tptr, None, 0, 2), b"flag bits other than")):
            assert call(*args) == -1
            assert b"sph_hip_render_scalars: " + text in lib.sph_hip_last_error(ctx), (text, lib.sph_hip_last_error(ctx))
        # every output NULL is a frame computed for its time
        assert call(SphTintParams(0, 1, 0.0, 1.0, 2, 1)) == 0
        got = sph.renderScalars(cam0, 32, 24, iso, 0, (0, 1), mode="column", solids=True)      # the context still works
        for f in want._fields:
            assert same(getattr(want, f), getattr(got, f)), f
        assert (got.first_inside >= 0).any() and (got.scalar != 0).any()
        # an upload drops the scalars
        sph.setParticles(scene[1], scene[2], scene[3])
        with pytest.raises(SphHipError, match=who + "the context carries no scalars"):
            sph.renderScalars(cam0, 32, 24, 1.0, 0, (0, 1))
    lib = load_library()
    ctx = C.c_void_p()
    params = p.copy()
    assert lib.sph_hip_create_slab(C.byref(ctx), C.byref(params), 4096, 0, 0, p.full_cells_z // 2) == 0
    try:
        cam, rp = good()
        tp = SphTintParams(0, 0, 0.0, 1.0, 2, 0)
        table = np.array([[0, 0, 0], [1, 1, 1]], F32)
        assert lib.sph_hip_render_scalars(ctx, C.byref(cam), C.byref(rp), None, None, 0, C.byref(tp),
                                          table.ctypes.data_as(C.c_void_p), 8, 8, 0, None, None, None, None, None, None,
                                          None) == -1
        err = lib.sph_hip_last_error(ctx)
        assert b"sph_hip_render_scalars" in err and b"slab" in err
    finally:
        lib.sph_hip_destroy(ctx)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    assert sys.argv[1] == "frames"
    print(json.dumps(child_frames()))
