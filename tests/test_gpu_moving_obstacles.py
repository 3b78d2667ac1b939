"""GPU: moving obstacles (include/sph_hip.h: sph_hip_set_obstacle_motion).  Every integrate route -
k_integrate_obst_moving for a single context (REF, FULL, FULL_FAST), k_slab_pack_early_obst_moving for
slabs, k_integrate_loads_moving under a load recording - equals the oracle's integrate followed by the
numpy restatement of the response (tests/moving_obstacle_emulation.py) with the test's own fp32 clock, bit
for bit; motions at rest or cleared change nothing; and a gate lifted from a dam releases it."""
import math

import numpy as np
import pytest

import load_emulation as L
import moving_obstacle_emulation as M
from helpers import to_oracle_params
from test_gpu_obstacles import check_ke, mode_of, same_bits, state, walled_scene

pytestmark = pytest.mark.gpu

F32 = np.float32
MODES = ["ref", "full", "fast"]


def walled_motions():
    """walled_scene's sphere, box and cylinder driven: the sphere along -y from the sixth step on, the box
    along +x as a piston, the cylinder for six steps and then at rest (time_step = 0.001).  With these the
    oracle alone, over 20 steps, has 3308 particle-steps changed by an obstacle in a step in which it
    moved and 1500 by one at rest (checked on the CPU before the speeds were fixed)."""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    return [O.Motion((0.0, -20.0, 0.0), 0.005), O.Motion((25.0, 0.0, 0.0)), O.Motion((15.0, 10.0, 0.0), 0.0, 0.006)]


def phases(sph):
    sph.voxelizeParticles()
    sph.findNeighbors()
    sph.computeDensity()
    sph.computeAcceleration()


def restated_turns(obst, motions, P, V, Q, dt, damping, tau0, tau1):
    """M.respond, counting the particles each turn changed: (V, Q, changed while moving, changed at rest)"""
    V, Q = (np.asarray(a, F32).reshape(-1, 3) for a in (V, Q))
    moving = resting = 0
    for o, m in zip(obst, motions):
        V2, Q2, _ = M.respond_one(o, m, P, V, Q, dt, damping, tau0, tau1)
        changed = int(((V2 != V) | (Q2 != Q)).any(1).sum())
        if (M.displacement(m, tau1) != M.displacement(m, tau0)).any():
            moving += changed
        else:
            resting += changed
        V, Q = V2, Q2
    return V, Q, moving, resting


def obstacles_now_are(sph, obst, motions, tau):
    """sph_hip_get_obstacles_now against the restated shift, every field of every struct"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    arr = (O.SphObstacle * O.MAX_OBSTACLES)()
    n = sph.call("sph_hip_get_obstacles_now", arr, O.MAX_OBSTACLES)
    want = [bytes(M.obstacle_at(o, m, tau)) for o, m in zip(obst, motions)]
    return [bytes(arr[i]) for i in range(n)] == want


@pytest.mark.parametrize("mode", MODES)
def test_integrate_pinned_per_step(oracle, hiplib, mode):
    """voxelize .. compute_acceleration on the device, download; oracle.integrate on that state, then the
    restated moving response with the test's own clock must be what sph_hip_integrate wrote - 20 steps"""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, obst = walled_scene()
    motions = walled_motions()
    op = to_oracle_params(p)
    dt, damping = F32(p.time_step), F32(p.damping)
    clock = M.clock(dt, 20)
    moving = resting = 0
    with S.SPH(mass.size, p, mode=mode_of(S, mode)) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setObstacles(obst)
        sph.setObstacleMotion(motions)
        assert sph.getObstacleMotion() == (motions, 0.0)
        for k in range(20):
            phases(sph)
            part = sph.getParticles()
            P, V0, A = part.mPosition.copy(), part.mVelocity.copy(), part.mAcceleration.copy()
            sph.integrate()
            got_pos, got_vel = state(sph)
            opos, ovel = P.copy(), V0.copy()
            oracle.integrate(op, opos, ovel, A, mass)
            ev, eq, mv, rs = restated_turns(obst, motions, P, ovel, opos, dt, damping, clock[k], clock[k + 1])
            assert same_bits(got_vel, ev.reshape(-1)) and same_bits(got_pos, eq.reshape(-1)), "step %d" % k
            check_ke(sph, got_vel, mass)
            assert same_bits(F32(sph.getObstacleMotion()[1]), clock[k + 1])
            assert obstacles_now_are(sph, obst, motions, clock[k + 1])
            moving += mv
            resting += rs
        assert [bytes(o.as_struct()) for o in sph.getObstacles()] == [bytes(o.as_struct()) for o in obst]
    print("changed by a moving obstacle: %d particle-steps, by one at rest: %d" % (moving, resting))
    assert moving > 200 and resting > 200, "the scene is meant to run into the obstacles, moving and at rest"


@pytest.mark.parametrize("mode", MODES)
def test_at_rest_or_cleared_is_static(hiplib, mode):
    """motions set and cleared, and motions with zero velocity: 50 steps as with static obstacles"""
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    p, pos, vel, mass, obst = walled_scene()
    out = []
    for case in ("static", "cleared", "zero"):
        with S.SPH(mass.size, p, mode=mode_of(S, mode)) as sph:
            sph.setParticles(pos, vel, mass)
            sph.setObstacles(obst)
            if case == "cleared":
                sph.setObstacleMotion(walled_motions())
                sph.setObstacleMotion([])
                assert sph.getObstacleMotion() == ([], 0.0)
            elif case == "zero":
                sph.setObstacleMotion([O.Motion((0, 0, 0)), None, O.Motion((0.0, -0.0, 0.0), 0.01, 0.02)])
            sph.run(50)
            out.append(state(sph) + (sph.energy(),))
            assert sph.getObstacleMotion()[1] == 0.0, "nothing moves: the clock stands"
    for x, v, e in out[1:]:
        assert same_bits(x, out[0][0]) and same_bits(v, out[0][1]) and e == out[0][2]


@pytest.mark.parametrize("mode", ["ref", "full"])
def test_routes_agree(hiplib, mode):
    """sph_hip_run(k), k x sph_hip_step and the phase calls give the same bits and the same clock; a time
    step set between two steps is the next step's"""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, obst = walled_scene()
    motions = walled_motions()
    k = 8
    dt2 = 0.0015
    mid = M.clock(p.time_step, k)[-1]
    end = M.clock(dt2, k, mid)[-1]
    out = []
    for route in ("run", "step", "phases"):
        with S.SPH(mass.size, p, mode=mode_of(S, mode)) as sph:
            sph.setParticles(pos, vel, mass)
            sph.setObstacles(obst)
            sph.setObstacleMotion(motions)
            for half in range(2):
                if route == "run":
                    sph.run(k)
                elif route == "step":
                    for _ in range(k):
                        sph.step()
                else:
                    for _ in range(k):
                        phases(sph)
                        sph.integrate()
                if half == 0:
                    assert same_bits(F32(sph.getObstacleMotion()[1]), mid)
                    sph.setTimeStep(dt2)
            x, v = state(sph)
            check_ke(sph, v, mass)
            assert same_bits(F32(sph.getObstacleMotion()[1]), end)
            assert obstacles_now_are(sph, obst, motions, end)
            out.append((x, v))
    for x, v in out[1:]:
        assert same_bits(x, out[0][0]) and same_bits(v, out[0][1])


def test_refused_motions_keep_the_previous_ones(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    p, pos, vel, mass, obst = walled_scene(4000)
    motions = walled_motions()
    with S.SPH(mass.size, p) as sph:
        sph.setParticles(pos, vel, mass)
        with pytest.raises(S.SphHipError, match="obstacle count"):
            sph.setObstacleMotion([O.Motion((1, 0, 0))])
        sph.setObstacleMotion([])
        sph.setObstacles(obst)
        sph.setObstacleMotion(motions)
        sph.run(3)
        tau = sph.getObstacleMotion()[1]
        assert tau > 0.0
        for bad in ([motions[0], motions[1]], motions + [motions[0]],
                    [O.Motion((np.nan, 0, 0)), None, None], [O.Motion((np.inf, 0, 0)), None, None],
                    [None, O.Motion((1, 0, 0), -1.0), None], [None, O.Motion((1, 0, 0), np.inf), None],
                    [None, None, O.Motion((1, 0, 0), 2.0, 1.0)], [None, None, O.Motion((1, 0, 0), 0.0, np.nan)]):
            with pytest.raises(S.SphHipError):
                sph.setObstacleMotion(bad)
        with pytest.raises(S.SphHipError, match="null motion list"):
            sph.call("sph_hip_set_obstacle_motion", None, 3)
        assert sph.getObstacleMotion() == (motions, tau)
        sph.run(2)
        # a new obstacle list stands still, with the clock at 0
        sph.setObstacles(obst[:2])
        assert sph.getObstacleMotion() == ([], 0.0)
        assert [bytes(o.as_struct()) for o in sph.getObstacles(now=True)] == [bytes(o.as_struct()) for o in obst[:2]]
        sph.run(2)


def slab_scene(world):
    """test_gpu_obstacles' slab scene with a piston below the middle cut that is driven along +z across
    it, the sphere on that cut driven from the eleventh step on, the cylinder for ten steps"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    from smoothed_particle_hydrodynamics_amd import scenes
    from smoothed_particle_hydrodynamics_amd import slab as SL
    from test_gpu_slabs import moving_block
    p, pos, vel, mass = moving_block()
    cuts = SL.plan_cuts(p, pos.reshape(-1, 3)[:, 2], world)
    zc = cuts[world // 2] * (1.0 / p.full_cell_inv)
    obst = [O.Sphere((1.6, 1.6, zc), 0.3), O.Box((1.0, 1.0, zc - 0.35), (1.4, 1.3, zc - 0.05)),
            O.Cylinder(2, (2.0, 1.2, 0.0), 0.2, 0.5, 3.5)]
    motions = [O.Motion((-8.0, 0.0, 6.0), 0.01), O.Motion((0.0, 0.0, 10.0)), O.Motion((-10.0, 12.0, 0.0), 0.0, 0.01)]
    pos, vel, mass = scenes.carve(pos, vel, mass, obst)
    return p, pos, vel, mass, obst, motions, zc


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "early-exchange"])
@pytest.mark.parametrize("world", [4, 8])
def test_slabs_equal_single_context(hiplib, world, overlap):
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_slabs import build_group
    p, pos, vel, mass, obst, motions, zc = slab_scene(world)
    steps = 30
    group, _ = build_group(S, p, pos, vel, mass, world, overlap)
    group.set_obstacles(obst)
    group.set_obstacle_motion(motions)
    for _ in range(steps):
        group.step()
    got = group.gather(mass.size)
    assert (got["owner"] >= 0).all()
    clocks = [s.get_obstacle_motion()[1] for s in group.slabs]
    for s in group.slabs:
        assert s.status()["errors"] == 0 and s.settings()["obstacle_motion"] == motions
    with S.SPH(mass.size, p) as one:
        one.setParticles(pos, vel, mass)
        one.setObstacles(obst)
        one.setObstacleMotion(motions)
        one.run(steps)
        x, v = state(one)
        tau = one.getObstacleMotion()[1]
        piston = one.getObstacles(now=True)[1]
    assert same_bits(got["pos"], x) and same_bits(got["vel"], v)
    assert clocks == [tau] * world and same_bits(F32(tau), M.clock(p.time_step, steps)[-1])
    assert float(obst[1].hi[2]) < zc < float(piston.hi[2]), "the piston is meant to cross the middle cut"
    for s in group.slabs:
        s.close()


def test_a_slab_refuses_inside_an_open_step(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_slabs import build_group
    p, pos, vel, mass, obst, motions, _ = slab_scene(2)
    group, _ = build_group(S, p, pos, vel, mass, 2, True)
    group.set_obstacles(obst)
    group.set_obstacle_motion(motions)
    for _ in range(2):
        group.step()
    for s in group.slabs:
        s.step_begin(None)
    for s in group.slabs:
        with pytest.raises(S.SphHipError, match="not between"):
            s.set_obstacle_motion([])
    for s in group.slabs:
        s.step_end()
    for s in group.slabs:
        got, tau = s.get_obstacle_motion()
        assert got == motions and same_bits(F32(tau), M.clock(p.time_step, 3)[-1])
        s.close()


# ---- loads --------------------------------------------------------------------------------------

def test_rows_pinned_per_step(oracle, hiplib):
    """FULL, 20 rows: every row k_integrate_loads_moving writes is the restatement's on the oracle's
    integrate, and the particles are those of the run without a recording"""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, obst = walled_scene()
    motions = walled_motions()
    free = to_oracle_params(p)
    free.apply_walls = 0
    dt, damping = F32(p.time_step), F32(p.damping)
    maxv = F32([p.max_x, p.max_y, p.max_z])
    steps = 20
    clock = M.clock(dt, steps)
    rows = []
    with S.SPH(mass.size, p, mode=S.MODE_FULL) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setObstacles(obst)
        sph.setObstacleMotion(motions)
        sph.recordLoads(steps)
        for k in range(steps):
            phases(sph)
            part = sph.getParticles()
            P, V0, A = part.mPosition.copy(), part.mVelocity.copy(), part.mAcceleration.copy()
            sph.integrate()
            got_pos, got_vel = state(sph)
            opos, ovel = P.copy(), V0.copy()
            oracle.integrate(free, opos, ovel, A, mass)
            ev, eq, row = M.integrate_respond(maxv, p.apply_walls, obst, motions, P, ovel, opos, dt, damping,
                                              clock[k], clock[k + 1], mass)
            assert same_bits(got_vel, ev.reshape(-1)) and same_bits(got_pos, eq.reshape(-1)), "step %d" % k
            rows.append(row)
        loads = sph.getLoads()
    assert loads.count.shape == (steps, L.SOLIDS)
    for r, row in enumerate(rows):
        assert row.same(loads.impulse_q[r], loads.count[r], loads.skipped[r]), "row %d" % r
    assert not loads.skipped.any() and (loads.count[:, 6:9].sum(0) > 50).all(), loads.count[:, 6:9].sum(0)


@pytest.mark.parametrize("mode", MODES)
def test_a_recording_changes_no_particle(hiplib, mode):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, obst = walled_scene()
    out = []
    for record in (False, True):
        with S.SPH(mass.size, p, mode=mode_of(S, mode)) as sph:
            sph.setParticles(pos, vel, mass)
            sph.setObstacles(obst)
            sph.setObstacleMotion(walled_motions())
            if record:
                sph.recordLoads(40)      # the last 10 steps take k_integrate_obst_moving again
            sph.run(50)
            out.append(state(sph) + (sph.energy(), sph.getObstacleMotion()[1]))
            if record:
                assert sph.getLoads().count[:, 6:9].sum() > 200
    assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][1], out[1][1])
    assert out[0][2:] == out[1][2:]


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "early-exchange"])
def test_slab_rows_sum_to_the_single_context(hiplib, overlap):
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_slabs import build_group
    world, steps = 4, 30
    p, pos, vel, mass, obst, motions, _ = slab_scene(world)
    group, _ = build_group(S, p, pos, vel, mass, world, overlap)
    group.set_obstacles(obst)
    group.set_obstacle_motion(motions)
    group.record_loads(steps)
    for _ in range(steps):
        group.step()
    total = group.get_loads()
    got = group.gather(mass.size)
    for s in group.slabs:
        assert s.status()["errors"] == 0
        s.close()
    with S.SPH(mass.size, p) as one:
        one.setParticles(pos, vel, mass)
        one.setObstacles(obst)
        one.setObstacleMotion(motions)
        one.recordLoads(steps)
        one.run(steps)
        want = one.getLoads()
        x, v = state(one)
    assert same_bits(got["pos"], x) and same_bits(got["vel"], v)
    assert np.array_equal(total.impulse_q, want.impulse_q) and np.array_equal(total.count, want.count)
    assert np.array_equal(total.skipped, want.skipped) and not want.skipped.any()
    assert (want.count[:, 6:9].sum(0) > 0).all(), "the block is meant to run into every obstacle"


# ---- the gate -----------------------------------------------------------------------------------

def test_a_lifted_gate_releases_the_dam(hiplib):
    """scenes.dam_break_gate, 100 000 particles: nobody is downstream of the gate until its lower edge is
    one kernel radius above the floor, some are afterwards; all finite, nobody inside the gate"""
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass, obst, motions = scenes.dam_break_gate(100000, 0.5)
    gate, lift = obst[0], motions[0]
    h = float(p.h)
    plane = float(gate.hi[0])
    # steps until the lower edge, which starts one kernel radius below the floor, is one above it
    held = int(math.floor(2.0 * h / (0.5 * p.time_step)))
    with S.SPH(mass.size, p) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setObstacles(obst)
        sph.setObstacleMotion(motions)
        downstream = []
        for steps in (held // 2, held - held // 2, 130):
            sph.run(steps)
            x, v = (a.reshape(-1, 3) for a in state(sph))
            now = sph.getObstacles(now=True)[0]
            assert np.isfinite(x).all() and np.isfinite(v).all()
            tol = 4.0 * 2.0 ** -23 * max(float(np.abs(now.lo).max()), float(np.abs(now.hi).max()))
            assert now.signed_distance(x).min() >= -tol
            downstream.append(int((x[:, 0] > plane).sum()))
            edge = float(now.lo[1])
        assert float(gate.lo[1]) + float(lift.displacement(M.clock(p.time_step, held)[-1])[1]) <= h
    print("downstream of the gate after %d, %d and %d steps: %s; lower edge at %.4f, h %.4f" %
          (held // 2, held, held + 130, downstream, edge, h))
    assert downstream[0] == 0 and downstream[1] == 0
    assert downstream[2] > 100 and edge > h
