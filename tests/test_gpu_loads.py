"""GPU: the load recording (include/sph_hip.h: sph_hip_record_loads / sph_hip_get_loads).  Every row
k_integrate_loads writes equals the numpy restatement (tests/load_emulation.py) applied to the oracle's
integrate int64 for int64, in REF, FULL and FULL_FAST; a recording changes no particle; sph_hip_run,
sph_hip_step, the phase calls and any number of slabs give the same rows; the recorded impulse closes the
particles' momentum balance; and the dam breaking against a pillar loads the pillar."""
import ctypes as C

import numpy as np
import pytest

import load_emulation as L
from helpers import to_oracle_params
from test_gpu_obstacles import mode_of, same_bits, state, walled_scene

pytestmark = pytest.mark.gpu

F32 = np.float32
MODES = ["ref", "full", "fast"]


def pinned_steps(S, oracle, mode, steps, quantum_log2=L.QUANTUM_LOG2):
    """walled_scene phase by phase with a recording on.  Per step: the oracle's integrate WITHOUT walls
    on the downloaded state gives every particle's (v, q) before any collision, the restatement the
    responses and the row.  Returns (device Loads, expected rows, per step (mass, v_before, v_final))."""
    p, pos, vel, mass, obst = walled_scene()
    free = to_oracle_params(p)
    free.apply_walls = 0
    dt, damping = F32(p.time_step), F32(p.damping)
    maxv = F32([p.max_x, p.max_y, p.max_z])
    rows, velocities = [], []
    with S.SPH(mass.size, p, mode=mode_of(S, mode)) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setObstacles(obst)
        sph.recordLoads(steps, quantum_log2)
        for _ in range(steps):
            sph.voxelizeParticles()
            sph.findNeighbors()
            sph.computeDensity()
            sph.computeAcceleration()
            part = sph.getParticles()
            P, V0, A = part.mPosition.copy(), part.mVelocity.copy(), part.mAcceleration.copy()
            sph.integrate()
            got_pos, got_vel = state(sph)
            opos, ovel = P.copy(), V0.copy()
            oracle.integrate(free, opos, ovel, A, mass)
            ev, eq, row = L.respond(maxv, p.apply_walls, obst, P, ovel, opos, dt, damping, mass, quantum_log2)
            assert same_bits(got_vel, ev.reshape(-1)) and same_bits(got_pos, eq.reshape(-1))
            rows.append(row)
            velocities.append((mass, ovel.reshape(-1, 3).copy(), got_vel.reshape(-1, 3).copy()))
        loads = sph.getLoads()
    return loads, rows, velocities


@pytest.mark.parametrize("mode", MODES)
def test_rows_pinned_per_step(oracle, hiplib, mode):
    import smoothed_particle_hydrodynamics_amd as S
    steps = 20
    loads, rows, _ = pinned_steps(S, oracle, mode, steps)
    assert loads.impulse_q.shape == (steps, L.SOLIDS, 3) and loads.impulse_q.dtype == np.int64
    assert loads.count.shape == loads.skipped.shape == (steps, L.SOLIDS)
    for r, row in enumerate(rows):
        assert row.same(loads.impulse_q[r], loads.count[r], loads.skipped[r]), "row %d" % r
    assert not loads.skipped.any()
    assert loads.count[:, 6:9].sum() > 200, "the scene is meant to run into the obstacles"
    assert not loads.count[:, 9:].any() and not loads.impulse_q[:, 9:].any()
    walls_hit = (np.abs(loads.impulse_q[:, :6]).sum((0, 2)) > 0).sum()
    assert walls_hit >= 3, loads.count[:, :6].sum(0)
    assert loads.quantum == 2.0 ** -24
    assert np.array_equal(loads.force(0.004), loads.impulse_q * 2.0 ** -24 / 0.004)


@pytest.mark.parametrize("mode", ["ref", "full"])
def test_another_quantum_is_pinned_too(oracle, hiplib, mode):
    import smoothed_particle_hydrodynamics_amd as S
    loads, rows, _ = pinned_steps(S, oracle, mode, 6, quantum_log2=-10)
    for r, row in enumerate(rows):
        assert row.same(loads.impulse_q[r], loads.count[r], loads.skipped[r]), "row %d" % r
    assert loads.count.sum() > 0 and loads.quantum_log2 == -10


@pytest.mark.parametrize("mode", MODES)
def test_momentum_closure(oracle, hiplib, mode):
    """Over all solids, the recorded impulse is the momentum the particles lost to collisions:
    sum_s impulse[s] = sum_i m_i (v_before_i - v_final_i), formed in float64, per component, within
    count * 2^e (half a quantum per term, doubled) + 2^-22 * sum_i |m_i| (|v_before_i| + |v_final_i|)
    (the fp32 rounding of a term's difference and product, 2^-24 each relative to at most
    |m| (|vb| + |va|), over the at most two or three responses a particle has, doubled)."""
    import smoothed_particle_hydrodynamics_amd as S
    loads, _, velocities = pinned_steps(S, oracle, mode, 20)
    responses = 0
    for r, (mass, before, final) in enumerate(velocities):
        m = mass.astype(np.float64)[:, None]
        lost = (m * (before.astype(np.float64) - final.astype(np.float64))).sum(0)
        got = loads.impulse[r].sum(0)
        count = int(loads.count[r].sum())
        bound = count * loads.quantum + 2.0 ** -22 * (np.abs(m) * (np.abs(before) + np.abs(final))).sum(0)
        print("step %2d: %5d responses, impulse %s, |error| %s, bound %s" % (r, count, got, np.abs(got - lost), bound))
        assert (np.abs(got - lost) <= bound).all(), (r, got, lost, bound)
        responses += count
    assert responses > 200


@pytest.mark.parametrize("obstacles", [True, False], ids=["obstacles", "walls-only"])
@pytest.mark.parametrize("mode", MODES)
def test_a_recording_changes_no_particle(hiplib, mode, obstacles):
    """50 steps with a recording (k_integrate_loads) and without (k_integrate_obst; without obstacles
    k_integrate in REF and the fused acceleration pass in FULL): the same bits, the same energies"""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, obst = walled_scene()
    out = []
    for record in (False, True):
        with S.SPH(mass.size, p, mode=mode_of(S, mode)) as sph:
            sph.setParticles(pos, vel, mass)
            if obstacles:
                sph.setObstacles(obst)
            if record:
                sph.recordLoads(50)
            sph.run(50)
            out.append(state(sph) + (sph.energy(),))
            if record:
                loads = sph.getLoads()
                assert loads.count.shape[0] == 50 and loads.count[:, :6].sum() > 0
                assert bool(loads.count[:, 6:].any()) == obstacles
    assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][1], out[1][1])
    assert out[0][2] == out[1][2]


@pytest.mark.parametrize("mode", ["ref", "full"])
def test_routes_give_the_same_rows(hiplib, mode):
    """sph_hip_run(k), k x sph_hip_step and the phase calls fill identical rows; rows beyond the
    recording are not written, and the steps go on as without one"""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, obst = walled_scene()
    k, extra = 20, 5
    out = []
    for route in ("run", "step", "phases", "none"):
        with S.SPH(mass.size, p, mode=mode_of(S, mode)) as sph:
            sph.setParticles(pos, vel, mass)
            sph.setObstacles(obst)
            if route != "none":
                sph.recordLoads(k)
            if route in ("run", "none"):
                sph.run(k + extra)
            elif route == "step":
                for _ in range(k + extra):
                    sph.step()
            else:
                for _ in range(k + extra):
                    sph.voxelizeParticles()
                    sph.findNeighbors()
                    sph.computeDensity()
                    sph.computeAcceleration()
                    sph.integrate()
            loads = sph.getLoads() if route != "none" else None
            out.append((loads,) + state(sph))
    first = out[0][0]
    assert first.impulse_q.shape[0] == k and first.count.sum() > 200
    for loads, _, _ in out[1:3]:
        assert np.array_equal(loads.impulse_q, first.impulse_q) and np.array_equal(loads.count, first.count)
        assert np.array_equal(loads.skipped, first.skipped) and loads.impulse_q.shape[0] == k
    for _, x, v in out[1:]:
        assert same_bits(x, out[0][1]) and same_bits(v, out[0][2])


def test_refusals_keep_the_previous_recording(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, obst = walled_scene(4000)
    with S.SPH(mass.size, p) as sph:
        sph.setParticles(pos, vel, mass)
        with pytest.raises(S.SphHipError, match="nothing is being recorded"):
            sph.getLoads()
        sph.recordLoads(4)
        sph.run(2)
        for bad in ((-1, -24), (4, 33), (4, -65)):
            with pytest.raises(S.SphHipError):
                sph.recordLoads(*bad)
        done = C.c_int32()
        for first, n in ((-1, 1), (0, 5), (3, 2), (5, 0)):
            with pytest.raises(S.SphHipError, match="leaves the allocated rows|must be >= 0"):
                sph.call("sph_hip_get_loads", first, n, None, None, None, C.byref(done))
        sph.run(1)
        loads = sph.getLoads()
        assert loads.count.shape[0] == 3
        # a second recording restarts at row 0, zeroed; rows = 0 stops and frees
        sph.recordLoads(2, -20)
        assert sph.getLoads().count.shape[0] == 0
        sph.run(3)
        again = sph.getLoads()
        assert again.count.shape[0] == 2 and again.quantum_log2 == -20
        sph.recordLoads(0)
        with pytest.raises(S.SphHipError, match="nothing is being recorded"):
            sph.getLoads()
        sph.run(1)


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "early-exchange"])
@pytest.mark.parametrize("world", [4, 8])
def test_slabs_sum_to_the_single_context(hiplib, world, overlap):
    """test_gpu_obstacles' slab scene (obstacles straddling the cuts): the slabs' rows, added up, are
    the single FULL context's, row for row over 30 steps"""
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    from smoothed_particle_hydrodynamics_amd import scenes
    from smoothed_particle_hydrodynamics_amd import slab as SL
    from test_gpu_slabs import build_group, moving_block
    p, pos, vel, mass = moving_block()
    cuts = SL.plan_cuts(p, pos.reshape(-1, 3)[:, 2], world)
    edge = 1.0 / p.full_cell_inv
    zc = cuts[world // 2] * edge
    z1 = cuts[1] * edge
    obst = [O.Sphere((1.6, 1.6, zc), 0.3), O.Box((1.0, 1.0, z1 - 0.15), (1.4, 1.3, z1 + 0.2)),
            O.Cylinder(2, (2.0, 1.2, 0.0), 0.2, 0.5, 3.5)]
    pos, vel, mass = scenes.carve(pos, vel, mass, obst)
    steps = 30
    group, _ = build_group(S, p, pos, vel, mass, world, overlap)
    for s in group.slabs:
        s.set_obstacles(obst)
    group.record_loads(steps)
    for _ in range(steps):
        group.step()
    total = group.get_loads()
    per_slab = [s.get_loads() for s in group.slabs]
    got = group.gather(mass.size)
    for s in group.slabs:
        assert s.status()["errors"] == 0
        s.close()
    with S.SPH(mass.size, p) as one:
        one.setParticles(pos, vel, mass)
        one.setObstacles(obst)
        one.recordLoads(steps)
        one.run(steps)
        want = one.getLoads()
        x, v = state(one)
    assert same_bits(got["pos"], x) and same_bits(got["vel"], v)
    assert total.impulse_q.shape[0] == steps
    assert np.array_equal(total.impulse_q, want.impulse_q) and np.array_equal(total.count, want.count)
    assert np.array_equal(total.skipped, want.skipped) and not want.skipped.any()
    assert want.count[:, 6:9].sum() > 0, "the block is meant to run into the obstacles"
    print("responses per slab:", [int(l.count.sum()) for l in per_slab], "single context:", int(want.count.sum()))


def test_a_slab_refuses_inside_an_open_step(hiplib):
    """between sph_hip_slab_step_begin and _end the recording may not change; the one in force goes on"""
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_slabs import build_group, moving_block
    p, pos, vel, mass = moving_block()
    group, _ = build_group(S, p, pos, vel, mass, 2, True)
    group.record_loads(8)
    for _ in range(3):
        group.step()
    for s in group.slabs:
        s.step_begin(None)
    for s in group.slabs:
        with pytest.raises(S.SphHipError, match="not between"):
            s.record_loads(4)
    for s in group.slabs:
        s.step_end()
    for s in group.slabs:
        done = C.c_int32()
        s.call("sph_hip_get_loads", 0, 0, None, None, None, C.byref(done))
        assert done.value == 4
        assert s.get_loads().count.shape == (4, L.SOLIDS)
        s.close()


def test_dam_loads_the_pillar(hiplib):
    """scenes.dam_break_pillar, 1M particles, 500 steps: nothing on the pillar before the surge reaches
    it, then a load pushing it downstream (+x); no term is skipped"""
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass, obst = scenes.dam_break_pillar(1 << 20)
    steps = 500
    with S.SPH(mass.size, p) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setObstacles(obst)
        sph.recordLoads(steps)
        sph.run(steps)
        loads = sph.getLoads()
        x, v = state(sph)
    assert np.isfinite(x).all() and np.isfinite(v).all()
    assert loads.count.shape[0] == steps and not loads.skipped.any()
    pillar = loads.impulse[:, 6]
    assert np.isfinite(loads.force(p.time_step)).all()
    hit = np.flatnonzero(loads.count[:, 6])
    print("pillar: first response at step %d, %d responses, impulse %s; floor responses %d" %
          (hit[0] if hit.size else -1, loads.count[:, 6].sum(), pillar.sum(0), loads.count[:, 2].sum()))
    assert hit.size > 0 and hit[0] > 0, "the surge reaches the pillar after a while"
    assert not loads.impulse_q[:hit[0], 6].any()
    assert pillar.sum(0)[0] > 0, "the surge pushes the pillar downstream"
    assert not loads.count[:, 7:].any()
