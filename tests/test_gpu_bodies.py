"""GPU: free bodies (include/sph_hip.h: sph_hip_set_bodies).  k_bodies_advance and k_integrate_bodies (REF,
FULL, FULL_FAST) equal the oracle's integrate followed by the numpy restatement (tests/body_emulation.py) step
by step, bit for bit, the body state included; the rows a recording keeps are the impulses the bodies
consume; a recording changes nothing; a body without a free axis is a static obstacle; the entry points
agree; stops hold; refusals leave everything as it was; and the dam's surge pushes a piece of debris."""
import math

import numpy as np
import pytest

import body_emulation as B
import load_emulation as L
import moving_obstacle_emulation as M
from helpers import to_oracle_params
from test_gpu_moving_obstacles import phases
from test_gpu_obstacles import check_ke, mode_of, same_bits, state, walled_scene

pytestmark = pytest.mark.gpu

F32 = np.float32
MODES = ["ref", "full", "fast"]
E = L.QUANTUM_LOG2


def walled_bodies():
    """walled_scene's box a body free in x and y - 4000 unit masses, about four times the fluid it displaces,
    thrown along (20, 10, 0) under the scene's gravity, its travel ending inside the domain -, the sphere under
    a Motion, the cylinder at rest.  On the CPU (the oracle's FULL step and the restatement, 30 steps) the body
    changes 1401 particle-steps while it moves and its velocity takes an impulse in 29 of the 30 steps."""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    bodies = [None, O.Body(4000.0, (20.0, 10.0, 0.0), (0.0, -9.8, 0.0), (True, True, False), (-0.5, -0.15, 0.0),
                           (1.0, 0.5, 0.0)), None]
    motions = [O.Motion((0.0, -20.0, 0.0), 0.005), None, None]
    return bodies, motions


def bodies_are(sph, st):
    """sph_hip_get_bodies against a B.State, every word"""
    got = sph.getBodies()
    return (same_bits(got.displacement, st.D) and same_bits(got.velocity, st.V) and
            np.array_equal(got.skipped, st.skipped) and np.array_equal(got.steps, st.steps))


def body_state(sph):
    got = sph.getBodies()
    return got.displacement.copy(), got.velocity.copy(), got.skipped.copy(), got.steps.copy()


def same_body_state(a, b):
    return same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


def obstacles_now_are(sph, obst, motions, bodies, st, tau):
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    arr = (O.SphObstacle * O.MAX_OBSTACLES)()
    n = sph.call("sph_hip_get_obstacles_now", arr, O.MAX_OBSTACLES)
    want = [bytes(M.shifted(o, st.D[i]) if B.is_body(b) else M.obstacle_at(o, m, tau))
            for i, (o, m, b) in enumerate(zip(obst, motions, bodies))]
    return [bytes(arr[i]) for i in range(n)] == want


def pinned_steps(oracle, sph, p, obst, motions, bodies, mass, steps, st=None, row=None):
    """`steps` steps by the phase calls, each integrate pinned to the oracle's plus the restatement: particles,
    KE, body state, obstacles now.  Returns (State, rows, particle-steps the body changed while it moved, steps
    in which an impulse changed its velocity)."""
    free = to_oracle_params(p)
    free.apply_walls = 0
    dt, damping = F32(p.time_step), F32(p.damping)
    maxv = F32([p.max_x, p.max_y, p.max_z])
    clock = M.clock(dt, steps)
    st = B.State(bodies) if st is None else st
    rows, by_body, kicks = [], 0, 0
    for k in range(steps):
        phases(sph)
        part = sph.getParticles()
        P, V0, A = part.mPosition.copy(), part.mVelocity.copy(), part.mAcceleration.copy()
        sph.integrate()
        got_pos, got_vel = state(sph)
        opos, ovel = P.copy(), V0.copy()
        oracle.integrate(free, opos, ovel, A, mass)
        if row is not None and (row.impulse[L.WALLS + 1][:2] != 0).any():
            kicks += 1
        st = B.advance(bodies, st, row, E, dt)
        changed = [0] * len(obst)
        ev, eq, row = B.integrate_respond(maxv, p.apply_walls, obst, motions, bodies, st, P, ovel, opos, dt, damping,
                                          clock[k], clock[k + 1], mass, E, changed)
        assert same_bits(got_vel, ev.reshape(-1)) and same_bits(got_pos, eq.reshape(-1)), "step %d" % k
        check_ke(sph, got_vel, mass)
        assert bodies_are(sph, st), "body state after step %d" % k
        assert obstacles_now_are(sph, obst, motions, bodies, st, clock[k + 1])
        if (st.D[1] != st.Dprev[1]).any():
            by_body += changed[1]
        rows.append(row)
    return st, rows, by_body, kicks


@pytest.mark.parametrize("mode", MODES)
def test_integrate_pinned_per_step(oracle, hiplib, mode):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, obst = walled_scene()
    bodies, motions = walled_bodies()
    with S.SPH(mass.size, p, mode=mode_of(S, mode)) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setObstacles(obst)
        sph.setObstacleMotion(motions)
        sph.setBodies(bodies)
        got = sph.getBodies()
        assert got.bodies == bodies and bodies_are(sph, B.State(bodies))
        st, rows, by_body, kicks = pinned_steps(oracle, sph, p, obst, motions, bodies, mass, 30)
        assert same_bits(F32(sph.getObstacleMotion()[1]), M.clock(p.time_step, 30)[-1])
        assert [bytes(o.as_struct()) for o in sph.getObstacles()] == [bytes(o.as_struct()) for o in obst]
    print("changed by the body while it moved: %d particle-steps; impulse steps: %d; displacement %s" %
          (by_body, kicks, st.D[1]))
    assert st.steps.tolist() == [0, 30, 0] and not st.skipped.any()
    assert by_body > 200, "the body is meant to run into the fluid"
    assert kicks >= 10, "the fluid is meant to push the body"


def test_rows_and_bodies_agree(oracle, hiplib):
    """a recording of the same quantum: its 20 rows are the restatement's, and row k's column is exactly the
    impulse the advance of step k + 1 consumed (the 21st step reads the last row and fills an internal one)"""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, obst = walled_scene()
    bodies, motions = walled_bodies()
    steps = 20
    with S.SPH(mass.size, p, mode=S.MODE_FULL) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setObstacles(obst)
        sph.setObstacleMotion(motions)
        sph.setBodies(bodies, E)
        sph.recordLoads(steps, E)
        st, rows, _, _ = pinned_steps(oracle, sph, p, obst, motions, bodies, mass, steps)
        loads = sph.getLoads()
        assert loads.count.shape == (steps, L.SOLIDS)
        for r, row in enumerate(rows):
            assert row.same(loads.impulse_q[r], loads.count[r], loads.skipped[r]), "row %d" % r
        assert not loads.skipped.any() and loads.count[:, 7].sum() > 200
        # one more step: the advance consumes the recording's last row
        sph.step()
        last = L.Row(E)
        last.impulse[:], last.skipped[:] = loads.impulse_q[-1], loads.skipped[-1]
        after = B.advance(bodies, st, last, E, F32(p.time_step))
        assert bodies_are(sph, after) and (after.V[1] != st.V[1]).any()
        assert sph.getLoads().count.shape == (steps, L.SOLIDS)
    # the device's own rows, fed to the restated advance, reproduce the restated states
    replay = B.State(bodies)
    replay = B.advance(bodies, replay, None, E, F32(p.time_step))
    for r in range(steps):
        row = L.Row(E)
        row.impulse[:], row.skipped[:] = loads.impulse_q[r], loads.skipped[r]
        replay = B.advance(bodies, replay, row, E, F32(p.time_step))
    assert same_bits(replay.D, after.D) and same_bits(replay.V, after.V)


@pytest.mark.parametrize("mode", MODES)
def test_a_recording_changes_nothing(hiplib, mode):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, obst = walled_scene()
    bodies, motions = walled_bodies()
    out = []
    for record in (False, True):
        with S.SPH(mass.size, p, mode=mode_of(S, mode)) as sph:
            sph.setParticles(pos, vel, mass)
            sph.setObstacles(obst)
            sph.setObstacleMotion(motions)
            sph.setBodies(bodies, E)
            if record:
                sph.run(5)
                sph.recordLoads(30, E)   # rows for steps 6 .. 35; internal rows before and after
            else:
                with pytest.raises(S.SphHipError, match="another quantum_log2"):
                    sph.recordLoads(30, E + 4)
                sph.run(5)
                with pytest.raises(S.SphHipError, match="another quantum_log2"):
                    sph.recordLoads(30, E - 1)
            sph.run(45)
            out.append(state(sph) + (sph.energy(), sph.getObstacleMotion()[1]) + body_state(sph))
            if record:
                assert sph.getLoads().count[:, 7].sum() > 100
                sph.recordLoads(0, E + 4)    # stopping a recording is never refused
    assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][1], out[1][1])
    assert out[0][2:4] == out[1][2:4]
    assert same_body_state(out[0][4:], out[1][4:]) and out[0][7].tolist() == [0, 50, 0]


@pytest.mark.parametrize("mode", MODES)
def test_no_free_axis_is_a_static_obstacle(hiplib, mode):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    p, pos, vel, mass, obst = walled_scene()
    fixed = O.Body(10.0, (5.0, 5.0, 5.0), (0.0, -9.8, 0.0), (False, False, False))
    out = []
    for with_bodies in (False, True):
        with S.SPH(mass.size, p, mode=mode_of(S, mode)) as sph:
            sph.setParticles(pos, vel, mass)
            sph.setObstacles(obst)
            if with_bodies:
                sph.setBodies([fixed, fixed, None])
            sph.run(50)
            out.append(state(sph) + (sph.energy(),))
            if with_bodies:
                got = sph.getBodies()
                assert not got.displacement.any() and not got.velocity.any() and got.steps.tolist() == [50, 50, 0]
    assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][1], out[1][1]) and out[0][2] == out[1][2]


@pytest.mark.parametrize("mode", ["ref", "full"])
def test_entry_points_agree(hiplib, mode):
    """sph_hip_run(k), k x sph_hip_step and the phase calls: the same particles and the same body state, a time
    step set between two steps being the next step's; run(30) in one call equals 30 single steps"""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, obst = walled_scene()
    bodies, motions = walled_bodies()
    k = 8
    out = []
    for route in ("run", "step", "phases", "run30", "step30"):
        with S.SPH(mass.size, p, mode=mode_of(S, mode)) as sph:
            sph.setParticles(pos, vel, mass)
            sph.setObstacles(obst)
            sph.setObstacleMotion(motions)
            sph.setBodies(bodies)
            if route == "run30":
                sph.run(30)
            elif route == "step30":
                for _ in range(30):
                    sph.step()
            else:
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
                        sph.setTimeStep(0.0015)
            x, v = state(sph)
            check_ke(sph, v, mass)
            out.append((x, v, body_state(sph)))
    for x, v, b in out[1:3]:
        assert same_bits(x, out[0][0]) and same_bits(v, out[0][1]) and same_body_state(b, out[0][2])
    assert same_bits(out[3][0], out[4][0]) and same_bits(out[3][1], out[4][1]) and same_body_state(out[3][2], out[4][2])
    assert out[0][2][3].tolist() == [0, 2 * k, 0] and out[3][2][3].tolist() == [0, 30, 0]
    assert not same_bits(out[0][2][0], out[3][2][0])


def test_a_body_driven_into_a_stop_stays_there(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    p, pos, vel, mass, obst = walled_scene()
    hi = (0.03125, 0.0, 0.0)
    # (its own drive, 3 velocity units per step, outweighs what the fluid gives it: below 1 per step)
    bodies = [None, O.Body(8000.0, (10.0, 0.0, 0.0), (3000.0, 0.0, 0.0), (True, False, False), (0.0, 0.0, 0.0), hi), None]
    with S.SPH(mass.size, p) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setObstacles(obst)
        sph.setBodies(bodies)
        sph.run(1)
        first = sph.getBodies()
        assert 0.0 < first.displacement[1, 0] < hi[0] and first.velocity[1, 0] > 0
        sph.run(19)
        got = sph.getBodies()
        assert same_bits(got.displacement[1], F32(hi)) and same_bits(got.velocity[1], np.zeros(3, F32))
        assert got.steps.tolist() == [0, 20, 0]
        at_stop = B.State(bodies)
        at_stop.D[1] = F32(hi)
        assert obstacles_now_are(sph, obst, [None] * 3, bodies, at_stop, 0.0)      # every field of every struct
        now = sph.getObstacles(now=True)
        assert same_bits(now[1].lo, (obst[1].lo + F32(hi)).astype(F32)) and same_bits(now[1].hi, (obst[1].hi + F32(hi)).astype(F32))
        assert bytes(now[0].as_struct()) == bytes(obst[0].as_struct())
        x, v = state(sph)
        assert np.isfinite(x).all() and np.isfinite(v).all()


def test_refusals_leave_everything_as_it_was(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    from smoothed_particle_hydrodynamics_amd import slab as SL
    from test_gpu_slabs import build_group
    p, pos, vel, mass, obst = walled_scene(4000)
    bodies, motions = walled_bodies()
    with S.SPH(mass.size, p) as sph:
        sph.setParticles(pos, vel, mass)
        with pytest.raises(S.SphHipError, match="obstacle count"):
            sph.setBodies([O.Body(1.0)])
        sph.setObstacles(obst)
        sph.setObstacleMotion(motions)
        sph.setBodies(bodies)
        sph.run(3)
        before = body_state(sph)
        tau = sph.getObstacleMotion()[1]
        nan = math.nan
        for bad in ([bodies[1]], bodies + [None],
                    [O.Body(4.0), None, None],                                   # the sphere's motion moves
                    [None, O.Body(-1.0), None], [None, O.Body(math.inf), None], [None, O.Body(nan), None],
                    [None, O.Body(1.0, velocity=(nan, 0, 0)), None], [None, O.Body(1.0, accel=(0, math.inf, 0)), None],
                    [None, O.Body(1.0, travel_lo=(0.1, 0, 0)), None], [None, O.Body(1.0, travel_hi=(0, -0.1, 0)), None]):
            with pytest.raises(S.SphHipError):
                sph.setBodies(bad)
        s = bodies[1].as_struct()
        s.free_axes = 8
        with pytest.raises(S.SphHipError, match="free_axes"):
            sph.setBodies([None, s, None])
        with pytest.raises(S.SphHipError, match="quantum_log2"):
            sph.setBodies(bodies, 33)
        with pytest.raises(S.SphHipError, match="null body list"):
            sph.call("sph_hip_set_bodies", None, 3, E)
        with pytest.raises(S.SphHipError, match="is a body"):
            sph.setObstacleMotion([None, O.Motion((1, 0, 0)), None])
        assert sph.getBodies().bodies == bodies and same_body_state(body_state(sph), before)
        assert sph.getObstacleMotion() == ([motions[0], O.Motion((0, 0, 0)), O.Motion((0, 0, 0))], tau)
        # the quantum rule, the other direction: a recording of another quantum with rows left
        sph.setBodies([])
        assert sph.getBodies().bodies == []
        sph.recordLoads(4, E + 2)
        with pytest.raises(S.SphHipError, match="rows left"):
            sph.setBodies(bodies, E)
        sph.setBodies(bodies, E + 2)
        sph.run(4)
        sph.setBodies(bodies, E)          # the recording is used up
        sph.run(2)
        assert sph.getBodies().steps.tolist() == [0, 2, 0]
        # a new obstacle list is nobody's body
        sph.setObstacles(obst[:2])
        assert sph.getBodies().bodies == [] and sph.getObstacleMotion() == ([], 0.0)
        assert [bytes(o.as_struct()) for o in sph.getObstacles(now=True)] == [bytes(o.as_struct()) for o in obst[:2]]
        sph.run(2)
    # slab contexts hold no bodies
    assert not hasattr(SL.HipSlab, "setBodies") and not hasattr(SL.HipSlab, "set_bodies")
    assert not hasattr(SL.LocalSlabGroup, "set_bodies")
    from test_gpu_slabs import moving_block
    bp, bpos, bvel, bmass = moving_block()
    group, _ = build_group(S, bp, bpos, bvel, bmass, 2)
    group.set_obstacles(obst)
    arr, n = O.as_body_array([None, bodies[1], None])
    for s in group.slabs:
        with pytest.raises(S.SphHipError, match="slab contexts"):
            s.call("sph_hip_set_bodies", arr, n, E)
        lst = (O.SphBody * 4)()
        assert s.call("sph_hip_get_bodies", lst, None, 4) == 0
    group.step()
    for s in group.slabs:
        assert s.status()["errors"] == 0
        s.close()


def test_the_surge_pushes_the_debris(hiplib):
    """scenes.dam_break_debris, 100 000 particles.  Stepped on the CPU first (the oracle's FULL step and the
    restatement): the box's displacement is exactly zero up to and including step DEBRIS_REST and positive from
    step DEBRIS_MOVES on."""
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass, obst, bodies = scenes.dam_break_debris(100000)
    with S.SPH(mass.size, p) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setObstacles(obst)
        sph.setBodies(bodies)
        seen = []
        done = 0
        for upto in (DEBRIS_REST // 2, DEBRIS_REST, DEBRIS_MOVES, DEBRIS_MOVES + 40, DEBRIS_MOVES + 80, DEBRIS_MOVES + 120):
            sph.run(upto - done)
            done = upto
            got = sph.getBodies()
            x, v = state(sph)
            assert np.isfinite(x).all() and np.isfinite(v).all()
            assert np.isfinite(got.displacement).all() and np.isfinite(got.velocity).all()
            assert got.skipped.tolist() == [0] and got.steps.tolist() == [upto]
            assert not got.displacement[0, 1:].any() and not got.velocity[0, 1:].any()
            seen.append(float(got.displacement[0, 0]))
            now = sph.getObstacles(now=True)[0]
            assert same_bits(now.lo, (obst[0].lo + got.displacement[0]).astype(F32))
    print("debris displacement after %s steps: %s" % ([DEBRIS_REST // 2, DEBRIS_REST, DEBRIS_MOVES, DEBRIS_MOVES + 40,
                                                       DEBRIS_MOVES + 80, DEBRIS_MOVES + 120], seen))
    assert seen[0] == 0.0 and seen[1] == 0.0
    assert seen[2] > 0.0 and all(b >= a for a, b in zip(seen[2:], seen[3:]))
    assert seen[-1] > seen[2] and seen[-1] <= float(bodies[0].travel_hi[0])


# from the CPU run of this scene (B.oracle_step, 200 steps): the surge's first response at the box is in step
# 77, whose row the advance of step 78 consumes; the displacement is 4.05e-7 after step 78, 4.57e-4 after 100,
# 4.85e-3 after 150 and 1.43e-2 after 200, the velocity 0.24 then
DEBRIS_REST = 77
DEBRIS_MOVES = 78
