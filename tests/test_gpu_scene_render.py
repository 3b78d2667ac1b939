"""The scene renderer on an MI355X (include/sph_hip.h: sph_hip_render_scene): the context's obstacles, gates
and bodies drawn into the renderer's frame, checked bit for bit against the numpy restatement
(tests/scene_emulation.py on top of tests/render_emulation.py over the sampler's emulated field,
tests/sample_emulation.py), checked to equal sph_hip_render without solids, and checked not to change the
simulation."""
import collections
import ctypes as C

import numpy as np
import pytest

import render_emulation as E
import sample_emulation as SE
import scene_emulation as SC
from test_gpu_render import assert_frame, iso_of, make, same, snapshot, state

pytestmark = pytest.mark.gpu

F32 = np.float32
SceneParams = collections.namedtuple("SceneParams", ["albedo", "ambient", "diffuse"])
DEFAULT = SceneParams((0.72, 0.72, 0.72), 0.2, 0.8)      # SPH.render's defaults


def flat(fr):
    """a RenderResult of render(..., solids=True) as the emulation's flattened SceneFrame"""
    H, W = fr.depth.shape
    vel = fr.velocity if fr.velocity is not None else np.zeros((H, W, 3), F32)
    return SC.SceneFrame(fr.rgba.reshape(-1, 4), fr.depth.reshape(-1), fr.normal.reshape(-1, 3), vel.reshape(-1, 3),
                         fr.first_inside.reshape(-1), fr.solid_id.reshape(-1))


def assert_scene(got, want, what, index=None):
    """all six outputs bit for bit"""
    assert_frame(got, want, what, index)
    g = got.solid_id if index is None else got.solid_id[index]
    bad = np.flatnonzero(g != want.solid_id)
    assert bad.size == 0, "%s solid_id: %d pixels differ, first %d: %d vs %d" % (what, bad.size, bad[0], g[bad[0]],
                                                                                 want.solid_id[bad[0]])


def fluid_fields(p, sph, mass):
    pos, vel, _ = state(sph, mass)
    return pos, E.grid_fields(SE.Grid(p, pos, vel, mass))


def want_frame(sph, fields, iso, solids, cam, W, H, velocities=None, albedos=None, sp=DEFAULT, velocity=True,
               pixels=None, **render_args):
    rp = sph.renderParams(iso, **render_args)
    n = W * H if pixels is None else len(pixels[0])
    if fields is None:
        fluid = SC.background(rp, n)
    else:
        fluid = E.render(fields[0], cam, rp, W, H, velocity_field=fields[1] if velocity else None, pixels=pixels)
    return SC.composite(fluid, solids, cam, rp, sp, W, H, velocities, albedos, velocity, pixels)


def with_obstacles(scene, mode=None):
    sph = make(scene[:4], mode)
    sph.setObstacles(scene[4])
    return sph


def report(what, fr):
    sid = fr.solid_id
    print("%s: %d solid pixels (ids %s), %d fluid pixels of %d" % (
        what, (sid >= 0).sum(), sorted(set(sid[sid >= 0].tolist())), (fr.first_inside >= 0).sum(), sid.size))


# ---- 1. device == restatement on the pillar scene, five cameras ---------------------------------------------
def pillar_cameras(p, pos, pillar):
    """outside the box, inside the box in empty space, inside the fluid, straight down the pillar's axis (the
    centre ray of the odd-sized frame is parallel to it), grazing along the pillar's side"""
    from smoothed_particle_hydrodynamics_amd import Camera
    box = np.array([p.max_x, p.max_y, p.max_z], np.float64)
    c = 0.5 * box
    ax = np.array([float(pillar.center[0]), 0.0, float(pillar.center[2])])
    r = float(pillar.radius)
    W, H = 64, 48
    out = {"outside": (Camera.look_at(c + np.array([0.9, 0.7, 1.6]) * box.max(), c, (0, 1, 0), 40, W, H), W, H)}
    out["inside box"] = (Camera.look_at(box * np.array([0.85, 0.8, 0.9]), ax + [0, 0.3 * box[1], 0], (0, 1, 0), 70, W, H),
                         W, H)
    lo, hi = pos.min(0).astype(np.float64), pos.max(0).astype(np.float64)
    mid = 0.5 * (lo + hi)
    eye = pos[int(np.argmin(((pos - mid) ** 2).sum(1)))].astype(np.float64)
    out["inside fluid"] = (Camera.look_at(eye, ax + [0, eye[1], 0], (0, 1, 0), 60, W, H), W, H)
    W2, H2 = 65, 49
    half = 2.5 * r
    out["down the axis"] = (Camera((ax[0], float(pillar.hi) + 1.0, ax[2]), (0.0, -1.0, 0.0), (half, 0, 0),
                                   (0, 0, -half * H2 / W2)), W2, H2)
    eye = np.array([ax[0] + r, 0.5 * box[1], -0.6 * box[2]])
    out["grazing"] = (Camera.look_at(eye, (ax[0] + r, 0.5 * box[1], ax[2]), (0, 1, 0), 30, W, H), W, H)
    return out


@pytest.fixture(scope="module")
def pillar():
    from smoothed_particle_hydrodynamics_amd import scenes
    return scenes.dam_break_pillar(20000)


def test_pillar_frames_match_the_restatement(pillar):
    p, mass, obst = pillar[0], pillar[3], pillar[4]
    with with_obstacles(pillar) as sph:
        sph.run(2)
        pos, fields = fluid_fields(p, sph, mass)
        iso = iso_of(sph, pos)
        solid = fluid = 0
        for name, (cam, W, H) in pillar_cameras(p, pos, obst[0]).items():
            got = sph.render(cam, W, H, iso, velocity=True, solids=True)
            want = want_frame(sph, fields, iso, obst, cam, W, H)
            report(name, got)
            assert_scene(flat(got), want, "pillar " + name)
            plain = sph.render(cam, W, H, iso, solids=True)
            assert plain.velocity is None
            for f in ("rgba", "depth", "normal", "first_inside", "solid_id"):
                assert same(getattr(plain, f), getattr(got, f)), "%s: %s with / without velocity" % (name, f)
            assert ((got.solid_id >= 0) <= (got.first_inside == -1)).all()
            solid += int((got.solid_id >= 0).sum())
            fluid += int((got.first_inside >= 0).sum())
            if name == "down the axis":
                assert got.solid_id[H // 2, W // 2] == 0 and got.normal[H // 2, W // 2].tolist() == [0.0, 1.0, 0.0]
                assert got.depth[H // 2, W // 2] == 1.0
        assert solid > 1000 and fluid > 1000, (solid, fluid)


# ---- 2. all three kinds in one list ---------------------------------------------------------------------------
def test_every_kind_in_one_list():
    from smoothed_particle_hydrodynamics_amd import Camera, scenes
    from smoothed_particle_hydrodynamics_amd.obstacles import Box, Cylinder, Sphere
    scene = scenes.dam_break(20000, speed=0.05)
    p, pos0, mass = scene[0], scene[1].reshape(-1, 3), scene[3]
    box = np.array([p.max_x, p.max_y, p.max_z], np.float64)
    lo, hi = pos0.min(0).astype(np.float64), pos0.max(0).astype(np.float64)
    mid, ext = 0.5 * (lo + hi), hi - lo
    big = float(box.max())
    # seen from +z: a sphere in front of the fluid, a box behind it and reaching out to its side, cylinders about
    # every axis through and beside it, one solid sticking out of the marched box, one far outside it
    solids = [Sphere(mid + [0.1 * ext[0], 0.2 * ext[1], 0.5 * ext[2] + 0.15 * big], 0.08 * big),
              Box(lo - [0.2 * big, 0.0, 0.3 * big], [hi[0] + 0.3 * big, mid[1], lo[2] - 0.05 * big]),
              Cylinder(0, mid + [0, 0.3 * ext[1], 0], 0.04 * big, lo[0] - 0.1 * big, hi[0] + 0.4 * big),
              Cylinder(1, [hi[0] + 0.2 * big, 0, mid[2]], 0.06 * big, -0.1 * big, 0.6 * big),
              Cylinder(2, mid - [0, 0.25 * ext[1], 0], 0.03 * big, lo[2] - 0.2 * big, hi[2] + 0.2 * big),
              Sphere([hi[0] + 0.9 * big, 0.7 * big, 0.3 * big], 0.12 * big)]
    colors = np.array([[0.9, 0.2, 0.2], [0.2, 0.9, 0.2], [0.2, 0.2, 0.9], [0.9, 0.9, 0.2], [0.9, 0.2, 0.9],
                       [0.2, 0.9, 0.9]], F32)
    sp = SceneParams((0.5, 0.5, 0.5), 0.35, 0.6)
    W, H = 65, 49
    target = mid + [0.25 * big, 0, 0]
    cams = {"front": Camera.look_at(target + [0.2 * big, 0.3 * big, 1.8 * big], target, (0, 1, 0), 42, W, H),
            "from behind": Camera.look_at(target + [-0.3 * big, 0.5 * big, -1.9 * big], target, (0, 1, 0), 42, W, H),
            "inside the box solid": Camera.look_at([mid[0], 0.5 * (lo[1] + mid[1]), lo[2] - 0.15 * big], mid + [0, 0, big],
                                                   (0, 1, 0), 70, W, H)}
    with make(scene) as sph:
        sph.setObstacles(solids)
        fields = E.grid_fields(SE.Grid(p, pos0, scene[2].reshape(-1, 3), mass))
        iso = iso_of(sph, pos0)
        seen = set()
        for name, cam in cams.items():
            got = sph.render(cam, W, H, iso, velocity=True, solids=True, solid_colors=colors, solid_ambient=0.35,
                             solid_diffuse=0.6, solid_albedo=(0.5, 0.5, 0.5))
            want = want_frame(sph, fields, iso, solids, cam, W, H, albedos=colors, sp=sp)
            report(name, got)
            assert_scene(flat(got), want, "kinds " + name)
            seen |= set(got.solid_id.reshape(-1).tolist())
            if name == "inside the box solid":
                assert (got.solid_id == 1).all() and (got.depth == 0).all()
            else:
                assert (got.first_inside >= 0).sum() > 50
        assert seen >= {-1, 0, 1, 2, 3, 4, 5}, seen
        # the default colour: one albedo for every solid
        cam = cams["front"]
        got = sph.render(cam, W, H, iso, solids=True)
        assert_scene(flat(got), want_frame(sph, fields, iso, solids, cam, W, H, velocity=False), "kinds default albedo")


# ---- 3. no solids: the renderer's frame, byte for byte ---------------------------------------------------------
def test_without_solids_the_frame_is_the_renderers():
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import Camera, scenes
    scene = scenes.dam_break(20000, speed=0.05)
    p, pos0 = scene[0], scene[1].reshape(-1, 3)
    box = np.array([p.max_x, p.max_y, p.max_z], np.float64)
    c = 0.5 * (pos0.min(0) + pos0.max(0)).astype(np.float64)
    for mode in (S.MODE_FULL, S.MODE_FULL_FAST):
        with make(scene, mode) as sph:
            sph.run(2)
            iso = iso_of(sph, pos0)
            for W, H in ((64, 48), (65, 49)):
                cam = Camera.look_at(c + np.array([0.9, 0.7, 1.6]) * box.max(), c, (0, 1, 0), 40, W, H)
                for velocity in (False, True):
                    a = sph.render(cam, W, H, iso, velocity=velocity)
                    b = sph.render(cam, W, H, iso, velocity=velocity, solids=True)
                    assert a.solid_id is None and b.solid_id.dtype == np.int32 and (b.solid_id == -1).all()
                    for f in E.Frame._fields:
                        assert same(getattr(a, f), getattr(b, f)), (mode, W, H, velocity, f)
                    assert (a.first_inside >= 0).sum() > 100
            # obstacles set and cleared again: still the renderer's frame
            sph.setObstacles(scenes.dam_break_pillar(20000)[4])
            sph.setObstacles([])
            b = sph.render(cam, W, H, iso, velocity=True, solids=True)
            for f in E.Frame._fields:
                assert same(getattr(a, f), getattr(b, f)), f


# ---- 4. solids that have moved ---------------------------------------------------------------------------------
def test_a_lifting_gate_is_drawn_where_it_stands():
    from smoothed_particle_hydrodynamics_amd import Camera, scenes
    scene = scenes.dam_break_gate(20000, 0.5)
    p, mass, obst, motions = scene[0], scene[3], scene[4], scene[5]
    W, H = 64, 48
    with with_obstacles(scene) as sph:
        sph.setObstacleMotion(motions)
        sph.run(20)
        now = sph.getObstacles(now=True)
        clock = sph.getObstacleMotion()[1]
        assert clock > 0 and float(now[0].lo[1]) > float(obst[0].lo[1])          # it has lifted
        pos, fields = fluid_fields(p, sph, mass)
        iso = iso_of(sph, pos)
        c = np.array([float(obst[0].hi[0]), 0.4 * p.max_y, 0.5 * p.max_z])
        vel_s = np.array([SC.motion_velocity(motions[0], clock)], F32)
        assert vel_s.tolist() == [[0.0, 0.5, 0.0]]
        for name, eye in (("downstream", c + [1.2, 0.5, 1.3]), ("upstream", c + [-0.9, 0.6, 1.4])):
            cam = Camera.look_at(eye, c, (0, 1, 0), 45, W, H)
            got = sph.render(cam, W, H, iso, velocity=True, solids=True)
            report("gate " + name, got)
            assert_scene(flat(got), want_frame(sph, fields, iso, now, cam, W, H, velocities=vel_s), "gate " + name)
            gate = got.solid_id == 0
            assert gate.sum() > 200 and (got.velocity[gate] == [0.0, 0.5, 0.0]).all()
            # ... and not where it was set: the list as set gives another frame
            stale = want_frame(sph, fields, iso, obst, cam, W, H, velocities=vel_s)
            assert (stale.depth != flat(got).depth).any()
        assert sph.getObstacleMotion()[1] == clock


@pytest.mark.parametrize("pushed", [False, True], ids=["as the scene sets it", "with a starting velocity"])
def test_a_body_is_drawn_where_the_device_has_moved_it(pushed):
    from smoothed_particle_hydrodynamics_amd import Camera, scenes
    from smoothed_particle_hydrodynamics_amd.obstacles import Body
    scene = scenes.dam_break_debris(20000)
    p, mass, obst, bodies = scene[0], scene[3], scene[4], scene[5]
    if pushed:
        b = bodies[0]
        bodies = [Body(b.mass, (0.4, 0.0, 0.0), b.accel, b.free, b.travel_lo, b.travel_hi)]
    W, H = 64, 48
    with with_obstacles(scene) as sph:
        sph.setBodies(bodies)
        sph.run(40)
        st = sph.getBodies()
        now = sph.getObstacles(now=True)
        print("displacement %r velocity %r" % (st.displacement[0].tolist(), st.velocity[0].tolist()))
        if pushed:
            assert st.displacement[0, 0] > 0 and st.velocity[0, 0] > 0
        assert float(now[0].lo[0]) == float(F32(obst[0].lo[0]) + st.displacement[0, 0])
        pos, fields = fluid_fields(p, sph, mass)
        iso = iso_of(sph, pos)
        c = 0.5 * (np.array(now[0].lo, np.float64) + np.array(now[0].hi, np.float64))
        cam = Camera.look_at(c + [0.3, 0.27, 0.55], c, (0, 1, 0), 45, W, H)
        got = sph.render(cam, W, H, iso, velocity=True, solids=True)
        report("debris", got)
        assert_scene(flat(got), want_frame(sph, fields, iso, now, cam, W, H, velocities=st.velocity), "debris")
        box = got.solid_id == 0
        assert box.sum() > 100 and (got.velocity[box] == st.velocity[0]).all()
        after = sph.getBodies()
        assert same(after.displacement, st.displacement) and same(after.velocity, st.velocity)
        assert (after.steps == st.steps).all()


# ---- 5. no particles, solids set ----------------------------------------------------------------------------------
def test_solids_without_particles_stand_over_the_background(pillar):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import Camera
    from smoothed_particle_hydrodynamics_amd.obstacles import Sphere
    p = pillar[0]
    solids = list(pillar[4]) + [Sphere((0.7, 0.3, 0.5), 0.15)]
    with S.SPH(20000, p, mode=S.MODE_FULL, device=0) as sph:
        sph.setObstacles(solids)
        for W, H in ((64, 48), (65, 49), (13, 7)):
            cam = Camera.look_at((1.4, 0.9, 2.1), (0.5, 0.4, 0.5), (0, 1, 0), 40, W, H)
            args = dict(box=((-0.1, -0.1, -0.1), (1.1, 1.1, 1.1)), background=(1, 2, 3, 4))
            got = sph.render(cam, W, H, 1.0, velocity=True, solids=True, **args)
            assert_scene(flat(got), want_frame(sph, None, 1.0, solids, cam, W, H, **args), "no particles %dx%d" % (W, H))
            assert {-1, 0, 1} <= set(got.solid_id.reshape(-1).tolist())
            assert (got.rgba[got.solid_id < 0] == [1, 2, 3, 4]).all() and (got.first_inside == -1).all()
            # without solids drawn, the same context gives the renderer's background frame
            bare = sph.render(cam, W, H, 1.0, **args)
            assert (bare.rgba == [1, 2, 3, 4]).all() and np.isinf(bare.depth).all()


# ---- 6. chunks and ragged tiles ------------------------------------------------------------------------------------------
def test_two_chunks_and_a_ragged_frame(pillar):
    from smoothed_particle_hydrodynamics_amd import Camera
    from smoothed_particle_hydrodynamics_amd.obstacles import Box
    p, mass = pillar[0], pillar[3]
    # a slab across the view, so that solid pixels lie on both sides of the chunk boundary all along the rows
    solids = list(pillar[4]) + [Box((-400.0, -3.0, -0.3), (400.0, 0.3, -0.2))]
    with make(pillar[:4]) as sph:
        sph.setObstacles(solids)
        sph.run(2)
        pos, fields = fluid_fields(p, sph, mass)
        iso = iso_of(sph, pos)
        W, H = 16384, 104
        # render_chunk_rows: (64 MiB - 7 * 256) / (W * 40 bytes) = 102 rows, rounded down to whole 8-row tiles
        rows = ((64 << 20) - 7 * 256) // (W * 40) // 8 * 8
        assert rows == 96 and rows < H
        cam = Camera.look_at((0.5, 0.45, 2.6), (0.5, 0.4, 0.5), (0, 1, 0), 35, W, H)
        got = sph.render(cam, W, H, iso, velocity=True, solids=True)
        rng = np.random.default_rng(8)
        py = np.concatenate([rng.integers(0, H, 4096), np.repeat(np.arange(rows - 2, rows + 2), W)])
        px = np.concatenate([rng.integers(0, W, 4096), np.tile(np.arange(W), 4)])
        # the fluid and the pillar fill the frame's middle only: weigh the random pixels toward it
        px[:2048] = W // 2 + rng.integers(-300, 300, 2048)
        want = want_frame(sph, fields, iso, solids, cam, W, H, pixels=(px, py))
        assert_scene(flat(got), want, "two chunks", index=py * W + px)
        for r in range(rows - 2, rows + 2):
            assert (got.solid_id[r] == 1).sum() > W // 2, r
        assert {-1, 0, 1} <= set(want.solid_id.tolist()) and (want.first_inside >= 0).sum() > 20
        W, H = 13, 7
        cam = Camera.look_at((1.2, 0.8, 1.9), (0.4, 0.35, 0.5), (0, 1, 0), 40, W, H)
        got = sph.render(cam, W, H, iso, velocity=True, solids=True)
        assert_scene(flat(got), want_frame(sph, fields, iso, solids, cam, W, H), "13x7")
        assert (got.solid_id >= 0).any() and (got.first_inside >= 0).any()


# ---- 7. the run is unchanged --------------------------------------------------------------------------------------------------
def test_a_scene_render_does_not_change_the_run():
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import Camera, scenes
    gate = scenes.dam_break_gate(20000, 0.5)
    debris = scenes.dam_break_debris(20000)
    cam = Camera.look_at((1.3, 0.9, 1.9), (0.3, 0.35, 0.5), (0, 1, 0), 45, 64, 48)

    def start(scene, mode):
        sph = with_obstacles(scene, mode)
        if scene is gate:
            sph.setObstacleMotion(scene[5])
        else:
            sph.setBodies(scene[5])
        return sph

    def solids_state(sph):
        st = sph.getBodies()
        return [np.array([sph.getObstacleMotion()[1]], F32), st.displacement, st.velocity, st.steps]

    for scene in (gate, debris):
        with start(scene, S.MODE_FULL_FAST) as a:
            for _ in range(13):
                a.step()
            want = snapshot(a) + solids_state(a)
        with start(scene, S.MODE_FULL_FAST) as b:
            for _ in range(3):
                b.step()            # the fused integrate leaves its prehash for the next cell build
            before = snapshot(b) + solids_state(b)
            fr = b.render(cam, 64, 48, float(F32(0.5) * np.median(before[2])), velocity=True, solids=True)
            after = snapshot(b) + solids_state(b)
            for _ in range(10):
                b.step()
            got = snapshot(b) + solids_state(b)
        assert (fr.solid_id >= 0).any() and (fr.first_inside >= 0).any()
        for i, (x, y) in enumerate(zip(before, after)):
            assert same(x, y), "array %d changed across a scene render" % i
        for i, (x, y) in enumerate(zip(want, got)):
            assert same(x, y), "the trajectory changed (array %d)" % i


def test_full_and_full_fast_give_the_same_scene(pillar):
    import smoothed_particle_hydrodynamics_amd as S
    p, mass, obst = pillar[0], pillar[3], pillar[4]
    with with_obstacles(pillar) as sph:
        sph.run(2)
        pos, vel, _ = state(sph, mass)
    out = []
    for mode in (S.MODE_FULL, S.MODE_FULL_FAST):
        with make((p, pos.reshape(-1), vel.reshape(-1), mass), mode) as sph:
            sph.setObstacles(obst)
            iso = iso_of(sph, pos)
            out.append([sph.render(cam, W, H, iso, velocity=True, solids=True)
                        for cam, W, H in pillar_cameras(p, pos, obst[0]).values()])
    for a, b in zip(*out):
        for f in a._fields:
            assert same(getattr(a, f), getattr(b, f)), f
    assert sum(int((fr.solid_id >= 0).sum()) for fr in out[0]) > 1000


# ---- 8. refusals on the device path ------------------------------------------------------------------------------------------
def test_refusals_name_the_entry_point(pillar):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import Camera
    from smoothed_particle_hydrodynamics_amd.lib import SphHipError, SphSceneParams, load_library
    from test_render_cpu import good
    p = pillar[0]
    cam0 = Camera.look_at((1.3, 0.9, 1.9), (0.3, 0.35, 0.5), (0, 1, 0), 45, 32, 24)
    with with_obstacles(pillar, S.MODE_REF) as sph:
        with pytest.raises(SphHipError, match="sph_hip_render_scene: FULL and FULL_FAST"):
            sph.render(cam0, 8, 8, 1.0, solids=True)
    with with_obstacles(pillar) as sph:
        want = sph.render(cam0, 32, 24, 1.0, solids=True)
        for colors in (np.zeros((2, 3), F32), np.zeros((64, 3), F32)):
            with pytest.raises(SphHipError, match="sph_hip_render_scene: the albedo count"):
                sph.render(cam0, 32, 24, 1.0, solids=True, solid_colors=colors)
        with pytest.raises(SphHipError, match="sph_hip_render_scene: scene params must be finite"):
            sph.render(cam0, 32, 24, 1.0, solids=True, solid_albedo=(0.5, np.nan, 0.5))
        with pytest.raises(SphHipError, match="sph_hip_render_scene: step must be > 0"):
            sph.render(cam0, 32, 24, 1.0, solids=True, step=0.0)
        lib, ctx = sph._lib, sph._ctx
        cam, rp = cam0.as_struct(), sph.renderParams(1.0)
        sp = SphSceneParams()
        assert lib.sph_hip_render_scene(ctx, C.byref(cam), C.byref(rp), None, None, 0, 32, 24, 0, None, None, None,
                                        None, None, None) == -1
        assert b"sph_hip_render_scene: null scene params" in lib.sph_hip_last_error(ctx)
        assert lib.sph_hip_render_scene(ctx, C.byref(cam), C.byref(rp), C.byref(sp), None, 0, 32, 24, 2, None, None,
                                        None, None, None, None) == -1
        assert b"sph_hip_render_scene: flag bits" in lib.sph_hip_last_error(ctx)
        got = sph.render(cam0, 32, 24, 1.0, solids=True)          # the context still works
        for f in want._fields:
            assert same(getattr(want, f), getattr(got, f)), f
        assert (got.solid_id == 0).any()
    lib = load_library()
    ctx = C.c_void_p()
    params = p.copy()
    assert lib.sph_hip_create_slab(C.byref(ctx), C.byref(params), 4096, 0, 0, p.full_cells_z // 2) == 0
    try:
        cam, rp = good()
        sp = SphSceneParams()
        assert lib.sph_hip_render_scene(ctx, C.byref(cam), C.byref(rp), C.byref(sp), None, 0, 8, 8, 0, None, None, None,
                                        None, None, None) == -1
        err = lib.sph_hip_last_error(ctx)
        assert b"sph_hip_render_scene" in err and b"slab" in err
    finally:
        lib.sph_hip_destroy(ctx)
