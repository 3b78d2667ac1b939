"""GPU: wedge obstacles (include/sph_hip.h: SPH_HIP_OBSTACLE_WEDGE) through every route that takes obstacles -
the integrate kernels of REF, FULL and FULL_FAST, motions, loads, bodies, slabs, the scene renderer - against
the numpy restatement tests/wedge_emulation.py bit for bit, and the dam breaking onto a beach.

The figures CPU_* are what the same scene gives on the CPU, the oracle's FULL step driving the restatement;
`python tests/test_gpu_wedges.py` prints them again.  FULL mode is bit-identical to the oracle, so its counts
equal them; REF's neighbours and FULL_FAST's arithmetic differ in the particles, so there every class must
occur and the counts are printed."""
import functools
import os

import numpy as np
import pytest

import body_emulation as B
import load_emulation as L
import moving_obstacle_emulation as M
import wedge_emulation as W
from helpers import to_oracle_params
from test_gpu_obstacles import check_ke, mode_of, same_bits, state

pytestmark = pytest.mark.gpu

F32 = np.float32
MODES = ["ref", "full", "fast"]
STEPS = 20

# the wedges' turns of wedge_scene() over STEPS steps on the CPU: cut-face entries, box-face entries, fallbacks
CPU_CUT = 4618
CPU_BOX = 3793
CPU_FALLBACK = 169
CPU_FIGURES = (CPU_CUT, CPU_BOX, CPU_FALLBACK)


def wedge_list():
    """a floor ramp, an overhanging wedge (its normal points down and along +x), a wedge whose plane cuts
    nothing off, and a sphere"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    return [O.Wedge.ramp((0.2, 0.0, -0.1), (1.0, 0.45, 1.5), 0, 1),
            O.Wedge((0.3, 0.7, 0.3), (0.8, 1.1, 1.0), (0.6, -0.8, 0.0), -0.39),
            O.Wedge((1.05, 0.2, 0.3), (1.25, 0.55, 0.9), (0.0, 0.0, 1.0), 50.0),
            O.Sphere((0.15, 0.9, 0.7), 0.12)]


@functools.lru_cache(maxsize=None)
def _wedge_scene(n):
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dense_block(n, lo=(0.02, 0.02, 0.02), hi=(1.3, 1.2, 1.4), speed=90.0)
    p.apply_gravity = 1
    p.apply_walls = 1
    p.gravity[1] = -9.8
    p.damping = 0.6
    obst = wedge_list()
    pos, vel, mass = scenes.carve(pos, vel, mass, obst)
    return p, pos, vel, mass, obst


def wedge_scene(n=20000):
    """test_gpu_obstacles.walled_scene's block (walls and gravity on, damping 0.6) with wedge_list() in its
    way, the particles inside the solids dropped"""
    p, pos, vel, mass, obst = _wedge_scene(n)
    return p, pos.copy(), vel.copy(), mass.copy(), obst


def phases(sph):
    sph.voxelizeParticles()
    sph.findNeighbors()
    sph.computeDensity()
    sph.computeAcceleration()


def cpu_figures():
    """the wedges' turns over STEPS FULL steps of wedge_scene() with the oracle and the restatement"""
    from oracle.oracle import Oracle
    p, pos, vel, mass, obst = wedge_scene()
    op = to_oracle_params(p)
    cl = W.Classes()
    oracle = Oracle()
    for _ in range(STEPS):
        pos, vel, _, _ = W.oracle_step(oracle, op, obst, None, None, None, None, pos, vel, mass, 0.0, 0.0, classes=cl)
    return cl.counts()


@pytest.mark.parametrize("mode", MODES)
def test_integrate_pinned_per_step(oracle, hiplib, mode):
    """voxelize .. compute_acceleration on the device, download; oracle.integrate on that state, then the
    restated response on (p, v, q) must be what sph_hip_integrate wrote - for 20 steps in a row"""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, obst = wedge_scene()
    op = to_oracle_params(p)
    dt, damping = F32(p.time_step), F32(p.damping)
    cl = W.Classes()
    with S.SPH(mass.size, p, mode=mode_of(S, mode)) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setObstacles(obst)
        assert [bytes(o.as_struct()) for o in sph.getObstacles()] == [bytes(o.as_struct()) for o in obst]
        for k in range(STEPS):
            phases(sph)
            part = sph.getParticles()
            P, V0, A = part.mPosition.copy(), part.mVelocity.copy(), part.mAcceleration.copy()
            sph.integrate()
            got_pos, got_vel = state(sph)
            opos, ovel = P.copy(), V0.copy()
            oracle.integrate(op, opos, ovel, A, mass)
            ev, eq = W.respond(obst, None, None, None, P, ovel, opos, dt, damping, classes=cl)
            assert same_bits(got_vel, ev.reshape(-1)) and same_bits(got_pos, eq.reshape(-1)), "step %d" % k
            check_ke(sph, got_vel, mass)
    print("%s: cut-face entries, box-face entries, fallbacks %r (CPU %r); fallback faces %s" %
          (mode, cl.counts(), CPU_FIGURES, cl.fallback_faces.tolist()))
    assert min(cl.counts()) > 0, "all three classes are meant to occur"
    if mode == "full":
        assert cl.counts() == CPU_FIGURES


@pytest.mark.parametrize("mode", ["ref", "full"])
def test_routes_agree(hiplib, mode):
    """sph_hip_run(k), k x sph_hip_step and the phase-by-phase calls give the same bits with wedges"""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, obst = wedge_scene()
    k = 12
    out = []
    for route in ("run", "step", "phases"):
        with S.SPH(mass.size, p, mode=mode_of(S, mode)) as sph:
            sph.setParticles(pos, vel, mass)
            sph.setObstacles(obst)
            if route == "run":
                sph.run(k)
            elif route == "step":
                for _ in range(k):
                    sph.step()
            else:
                for _ in range(k):
                    phases(sph)
                    sph.integrate()
            x, v = state(sph)
            check_ke(sph, v, mass)
            out.append((x, v))
    for x, v in out[1:]:
        assert same_bits(x, out[0][0]) and same_bits(v, out[0][1])
    assert not W.inside(obst[2], out[0][0].reshape(-1, 3)).any()


@pytest.mark.parametrize("mode", MODES)
def test_set_then_cleared_is_never_set(hiplib, mode):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, obst = wedge_scene()
    out = []
    for with_obst in (False, True):
        with S.SPH(mass.size, p, mode=mode_of(S, mode)) as sph:
            sph.setParticles(pos, vel, mass)
            if with_obst:
                sph.setObstacles(obst)
                assert len(sph.getObstacles()) == 4
                sph.setObstacles([])
                assert sph.getObstacles() == []
            sph.run(50)
            out.append(state(sph) + (sph.energy(),))
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()
    assert out[0][2] == out[1][2]


def piston():
    """a sloped piston - a wedge whose cut face looks along +x and up - driven along +x by a Motion that
    starts after two steps and stops after ten, and the list's sphere at rest"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    obst = [O.Wedge((0.05, 0.0, -0.1), (0.45, 0.9, 1.5), (0.8, 0.6, 0.0), 0.5), O.Sphere((0.9, 0.5, 0.7), 0.15)]
    return obst, [O.Motion((15.0, 0.0, 0.0), 0.008, 0.04), None]


def piston_scene():
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass, _ = wedge_scene()
    obst, motions = piston()
    pos, vel, mass = scenes.carve(pos, vel, mass, obst)
    return p, pos, vel, mass, obst, motions


@pytest.mark.parametrize("mode", ["ref", "full"])
def test_moving_wedge_pinned_per_step(oracle, hiplib, mode):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    p, pos, vel, mass, obst, motions = piston_scene()
    free = to_oracle_params(p)
    free.apply_walls = 0
    dt, damping = F32(p.time_step), F32(p.damping)
    maxv = F32([p.max_x, p.max_y, p.max_z])
    clock = M.clock(dt, STEPS)
    cl = W.Classes()
    moved_steps = 0
    with S.SPH(mass.size, p, mode=mode_of(S, mode)) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setObstacles(obst)
        sph.setObstacleMotion(motions)
        for k in range(STEPS):
            phases(sph)
            part = sph.getParticles()
            P, V0, A = part.mPosition.copy(), part.mVelocity.copy(), part.mAcceleration.copy()
            sph.integrate()
            got_pos, got_vel = state(sph)
            opos, ovel = P.copy(), V0.copy()
            oracle.integrate(free, opos, ovel, A, mass)
            ev, eq, _ = W.integrate_respond(maxv, p.apply_walls, obst, motions, None, None, P, ovel, opos, dt, damping,
                                            clock[k], clock[k + 1], mass, classes=cl)
            assert same_bits(got_vel, ev.reshape(-1)) and same_bits(got_pos, eq.reshape(-1)), "step %d" % k
            check_ke(sph, got_vel, mass)
            assert same_bits(F32(sph.getObstacleMotion()[1]), clock[k + 1])
            arr = (O.SphObstacle * O.MAX_OBSTACLES)()
            n = sph.call("sph_hip_get_obstacles_now", arr, O.MAX_OBSTACLES)
            assert [bytes(arr[i]) for i in range(n)] == [bytes(W.obstacle_at(o, m, clock[k + 1]))
                                                         for o, m in zip(obst, motions)]
            moved_steps += int((M.displacement(motions[0], clock[k + 1]) != M.displacement(motions[0], clock[k])).any())
        now = sph.getObstacles(now=True)
        assert [bytes(o.as_struct()) for o in now] == [bytes(W.obstacle_at(o, m, clock[STEPS])) for o, m in zip(obst, motions)]
        assert isinstance(now[0], O.Wedge) and np.array_equal(now[0].normal, obst[0].normal) and now[0].offset > obst[0].offset
        assert [bytes(o.as_struct()) for o in sph.getObstacles()] == [bytes(o.as_struct()) for o in obst]
    print("piston: moved in %d steps; turns %r" % (moved_steps, cl.counts()))
    assert 0 < moved_steps < STEPS and cl.cut > 200


@pytest.mark.parametrize("mode", ["ref", "full"])
def test_loads_on_wedges(oracle, hiplib, mode):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, obst = wedge_scene()
    free = to_oracle_params(p)
    free.apply_walls = 0
    dt, damping = F32(p.time_step), F32(p.damping)
    maxv = F32([p.max_x, p.max_y, p.max_z])
    rows = []
    with S.SPH(mass.size, p, mode=mode_of(S, mode)) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setObstacles(obst)
        sph.recordLoads(STEPS)
        for k in range(STEPS):
            phases(sph)
            part = sph.getParticles()
            P, V0, A = part.mPosition.copy(), part.mVelocity.copy(), part.mAcceleration.copy()
            sph.integrate()
            got_pos, got_vel = state(sph)
            opos, ovel = P.copy(), V0.copy()
            oracle.integrate(free, opos, ovel, A, mass)
            ev, eq, row = W.integrate_respond(maxv, p.apply_walls, obst, None, None, None, P, ovel, opos, dt, damping,
                                              0.0, 0.0, mass)
            assert same_bits(got_vel, ev.reshape(-1)) and same_bits(got_pos, eq.reshape(-1)), "step %d" % k
            rows.append(row)
        loads = sph.getLoads()
    for r, row in enumerate(rows):
        assert row.same(loads.impulse_q[r], loads.count[r], loads.skipped[r]), "row %d" % r
    assert not loads.skipped.any() and (loads.count[:, 6:10].sum(0) > 0).all()
    assert not loads.count[:, 10:].any() and not loads.impulse_q[:, 10:].any()
    ramp = loads.impulse_q[:, 6].sum(0)
    print("impulse on the ramp, quanta:", ramp.tolist())
    assert ramp[0] != 0 and ramp[1] < 0, "the ramp is pushed down, and along its run"


def wedge_body():
    """the floor ramp a body: 4000 unit masses, free along x only, its travel ending inside the domain"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    return [O.Body(4000.0, free=(True, False, False), travel_lo=(-0.15, 0.0, 0.0), travel_hi=(0.25, 0.0, 0.0)),
            None, None, None]


@pytest.mark.parametrize("mode", ["ref", "full"])
def test_wedge_body_pinned_per_step(oracle, hiplib, mode):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    p, pos, vel, mass, obst = wedge_scene()
    bodies = wedge_body()
    free = to_oracle_params(p)
    free.apply_walls = 0
    dt, damping = F32(p.time_step), F32(p.damping)
    maxv = F32([p.max_x, p.max_y, p.max_z])
    E = L.QUANTUM_LOG2
    st, row = B.State(bodies), None
    cl = W.Classes()
    with S.SPH(mass.size, p, mode=mode_of(S, mode)) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setObstacles(obst)
        sph.setBodies(bodies)
        for k in range(STEPS):
            phases(sph)
            part = sph.getParticles()
            P, V0, A = part.mPosition.copy(), part.mVelocity.copy(), part.mAcceleration.copy()
            sph.integrate()
            got_pos, got_vel = state(sph)
            opos, ovel = P.copy(), V0.copy()
            oracle.integrate(free, opos, ovel, A, mass)
            st = B.advance(bodies, st, row, E, dt)
            ev, eq, row = W.integrate_respond(maxv, p.apply_walls, obst, None, bodies, st, P, ovel, opos, dt, damping,
                                              0.0, 0.0, mass, E, classes=cl)
            assert same_bits(got_vel, ev.reshape(-1)) and same_bits(got_pos, eq.reshape(-1)), "step %d" % k
            check_ke(sph, got_vel, mass)
            got = sph.getBodies()
            assert same_bits(got.displacement, st.D) and same_bits(got.velocity, st.V), "body state after step %d" % k
            assert np.array_equal(got.skipped, st.skipped) and np.array_equal(got.steps, st.steps)
            arr = (O.SphObstacle * O.MAX_OBSTACLES)()
            n = sph.call("sph_hip_get_obstacles_now", arr, O.MAX_OBSTACLES)
            assert n == 4 and bytes(arr[0]) == bytes(W.shifted(obst[0], st.D[0]))
            assert [bytes(arr[i]) for i in range(1, 4)] == [bytes(o.as_struct()) for o in obst[1:]]
    print("wedge body: displacement %s velocity %s; wedge turns %r" % (st.D[0], st.V[0], cl.counts()))
    assert st.steps.tolist() == [STEPS, 0, 0, 0] and not st.skipped.any()
    assert st.D[0][0] != 0 and st.D[0][1] == 0 and st.D[0][2] == 0, "the surge is meant to push the ramp along x"


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "early-exchange"])
def test_slabs_equal_single_context(hiplib, overlap):
    """a moving block cut into 4 slabs, with wedges that straddle the cuts: the same bits as one context for
    30 steps, and no exchange error"""
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    from smoothed_particle_hydrodynamics_amd import scenes
    from smoothed_particle_hydrodynamics_amd import slab as SL
    from test_gpu_slabs import build_group, moving_block
    world = 4
    p, pos, vel, mass = moving_block()
    cuts = SL.plan_cuts(p, pos.reshape(-1, 3)[:, 2], world)
    edge = 1.0 / p.full_cell_inv
    zc, z1 = cuts[world // 2] * edge, cuts[1] * edge
    obst = [O.Wedge.ramp((1.2, 1.0, zc - 0.3), (2.0, 1.5, zc + 0.3), 0, 1),
            O.Wedge((1.0, 1.0, z1 - 0.15), (1.4, 1.3, z1 + 0.2), (0.0, 0.6, 0.8), 0.6 * 1.15 + 0.8 * z1),
            O.Wedge.ramp((1.6, 1.6, 0.5), (1.9, 2.0, 3.5), 2, 1, rising=False), O.Sphere((2.0, 1.2, zc), 0.2)]
    pos, vel, mass = scenes.carve(pos, vel, mass, obst)
    steps = 30
    group, _ = build_group(S, p, pos, vel, mass, world, overlap)
    for s in group.slabs:
        s.set_obstacles(obst)
        assert [bytes(o.as_struct()) for o in s.get_obstacles()] == [bytes(o.as_struct()) for o in obst]
    for _ in range(steps):
        group.step()
    got = group.gather(mass.size)
    assert (got["owner"] >= 0).all()
    for s in group.slabs:
        assert s.status()["errors"] == 0
    with S.SPH(mass.size, p) as one:
        one.setParticles(pos, vel, mass)
        one.setObstacles(obst)
        one.run(steps)
        x, v = state(one)
    assert same_bits(got["pos"], x) and same_bits(got["vel"], v)
    with S.SPH(mass.size, p) as none:
        none.setParticles(pos, vel, mass)
        none.run(steps)
        assert not same_bits(state(none)[0], x), "the block is meant to run into the wedges"
    for s in group.slabs:
        s.close()


def test_scene_frames_match_the_restatement(hiplib):
    """a 64x48 frame of the list from outside and with the eye inside the ramp: rgba, depth, normal, velocity,
    first_inside and solid_id equal the restatement's"""
    import render_emulation as RE
    from smoothed_particle_hydrodynamics_amd import Camera
    from test_gpu_render import iso_of, make
    from test_gpu_scene_render import DEFAULT, assert_scene, flat, fluid_fields, report
    p, pos, vel, mass, obst = wedge_scene()
    Wd, Hd = 64, 48
    cams = {"outside": Camera.look_at((-1.0, 1.6, 2.6), (0.6, 0.4, 0.7), (0, 1, 0), 40, Wd, Hd),
            "inside the ramp": Camera.look_at((0.8, 0.1, 0.7), (0.3, 0.9, 0.7), (0, 1, 0), 60, Wd, Hd)}
    assert W.inside(obst[0], F32([[0.8, 0.1, 0.7]])).all()
    with make((p, pos, vel, mass)) as sph:
        sph.setObstacles(obst)
        sph.run(2)
        x, fields = fluid_fields(p, sph, mass)
        iso = iso_of(sph, x)
        for name, cam in cams.items():
            got = sph.render(cam, Wd, Hd, iso, velocity=True, solids=True)
            rp = sph.renderParams(iso)
            fluid = RE.render(fields[0], cam, rp, Wd, Hd, velocity_field=fields[1])
            want = W.composite(fluid, obst, cam, rp, DEFAULT, Wd, Hd)
            report(name, got)
            assert_scene(flat(got), want, "wedges " + name)
            ids = set(got.solid_id[got.solid_id >= 0].tolist())
            if name == "outside":
                assert 0 in ids and len(ids) >= 2, ids
                cut = (got.solid_id == 0) & (got.normal == obst[0].normal).all(-1)
                assert cut.sum() > 20, "the ramp's cut face is meant to be seen"
            else:
                assert ids == {0} and (got.depth == 0).all(), "the eye is inside the ramp: every pixel is its"


def test_refused_wedges_keep_the_previous_list(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, obst = wedge_scene(4000)
    with S.SPH(mass.size, p) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setObstacles(obst)

        def refused(mutate, text):
            bad = obst[0].as_struct()
            mutate(bad)
            with pytest.raises(S.SphHipError) as err:
                sph.setObstacles([obst[3], bad])
            assert text in str(err.value), str(err.value)
            assert [bytes(o.as_struct()) for o in sph.getObstacles()] == [bytes(o.as_struct()) for o in obst]

        refused(lambda s: setattr(s, "kind", 4), "unknown obstacle kind")
        refused(lambda s: setattr(s, "radius", float("nan")), "obstacle fields must be finite")
        refused(lambda s: s.center.__setitem__(2, float("inf")), "obstacle fields must be finite")
        refused(lambda s: s.lo.__setitem__(1, 0.45), "a wedge needs lo < hi on every axis")
        refused(lambda s: s.center.__setitem__(1, 0.5), "a wedge's normal must have unit length")
        refused(lambda s: setattr(s, "radius", -10.0), "a wedge's plane leaves nothing of its box")
        sph.run(3)


def test_dam_breaks_onto_a_beach(hiplib):
    """dam_break_beach(20000), 200 steps: everything finite, no call reports an error (a single context's
    status is every call's return value, which SPH raises on; the error word is the slab exchange's), some particle higher on the slope
    than the still-water level (the column's volume spread over the floor), and nobody deeper behind the cut
    face than fp32 rounding allows: inside the beach's box n.q - d >= -2^-20 * (largest |coordinate| + |d|),
    ten times the five roundings of that formula"""
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass, obst = scenes.dam_break_beach(20000)
    beach = obst[0]
    with S.SPH(mass.size, p) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setObstacles(obst)
        sph.run(200)
        x, v = state(sph)
    x = x.reshape(-1, 3).astype(np.float64)
    assert np.isfinite(x).all() and np.isfinite(v).all()
    n, d = beach.normal.astype(np.float64), float(beach.offset)
    above = x @ n - d
    inbox = ((x > beach.lo) & (x < beach.hi)).all(1)
    tol = 2.0 ** -20 * (np.abs(x).max() + abs(d))
    assert inbox.sum() > 0, "no particle between the beach's slabs: the depth bound would check nothing"
    assert above[inbox].min() >= -tol, (above[inbox].min(), tol)
    still = (0.1 * 0.75 * 1.0) / (1.0 * 1.0)      # the column's volume over the unit box's floor area
    over = (x[:, 0] > beach.lo[0]) & (x[:, 0] < beach.hi[0])
    on_slope = over & (above < 2.0 * float(p.h)) & (x[:, 1] > still)
    print("over the beach %d, on the slope above the still-water level %.3f: %d, highest %.3f; deepest %.3g (tol %.3g)" %
          (over.sum(), still, on_slope.sum(), x[over, 1].max() if over.any() else 0.0, above[inbox].min(), tol))
    assert on_slope.sum() > 0


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(dict(zip(("CPU_CUT", "CPU_BOX", "CPU_FALLBACK"), cpu_figures())))
