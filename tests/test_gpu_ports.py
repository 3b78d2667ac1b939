"""GPU: ports (include/sph_hip.h: sph_hip_set_ports) - emitters and sinks on a single context.  FULL against
the oracle stepped by the numpy restatement (tests/port_emulation.py) bit for bit, FULL_FAST against the
existing route fed the same edits, filling from empty, draining and refilling, the capacity refusal, the rest
of the scene (obstacle, loads, gauges) on a port context, the untiled and small-tile routes, clearing and the
refusals.  Every grid is 16^3 cells or smaller, every state 6 000 particles or fewer."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import gauge_emulation as G
import load_emulation as L
import port_emulation as PE
from helpers import to_oracle_params

pytestmark = pytest.mark.gpu

F32 = np.float32
N0 = 3001            # the block: not a multiple of 64, nor is any count 3001 + 324 k - (what the sink took)
STEPS = 30


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if np.asarray(a).dtype == F32 else np.asarray(a)


def block_scene():
    """h = 1/16 on a 16^3 FULL grid over the unit cube, walls and gravity on, no point mass: a block of N0 unit
    masses with ~32 neighbours and random velocities; one emitter of 18 x 18 points blowing along -x into it
    every third step; one sink box inside the block, which the block's particles keep drifting into."""
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    p = scenes.default_params(0.0625, (8, 8, 8))
    p.central_mass = 0.0
    p.apply_walls = 1
    p.apply_gravity = 1
    p.gravity[0], p.gravity[1], p.gravity[2] = 0.0, -9.81, 0.0
    assert (p.full_cells_x, p.full_cells_y, p.full_cells_z) == (16, 16, 16)
    pos = scenes.box_fill(N0, (0.02, 0.02, 0.02), (0.52, 0.47, 0.44), 11)
    vel = scenes.box_fill(N0, (-30.0,) * 3, (30.0,) * 3, 12)
    mass = np.ones(N0, F32)
    emitters = [S.Emitter(0, (0.7, 0.2, 0.2), (18, 18), 0.0317, (-15.0, 0.0, 0.0), 1.0, first=0, every=3)]
    sinks = [S.Sink((0.1, 0.1, 0.1), (0.25, 0.25, 0.25))]
    return p, pos, vel, mass, emitters, sinks


def snapshot(run):
    return dict(ids=run.ids.copy(), pos=run.pos.copy(), vel=run.vel.copy(), rho=run.rho.copy(), acc=run.acc.copy(),
                ncount=run.ncount.copy(), emitted=run.emitted.copy(), removed=run.removed.copy(), live=run.live,
                next_id=run.next_id, history=list(run.history))


@functools.lru_cache(maxsize=None)
def block_reference():
    """The block scene stepped STEPS steps by the restatement, computed once and shared (read only)."""
    from oracle.oracle import Oracle
    p, pos, vel, mass, emitters, sinks = block_scene()
    run = PE.PortRun(to_oracle_params(p), pos, vel, mass, emitters, sinks)
    orc = Oracle()
    for _ in range(STEPS):
        assert run.step(orc)
    return snapshot(run)


def live_state(sph):
    """sph_hip_download_live sorted by id"""
    ids, pos, vel, rho, acc, cnt = sph.downloadLive()
    o = np.argsort(ids, kind="stable")
    return dict(ids=ids[o], pos=pos.reshape(-1, 3)[o], vel=vel.reshape(-1, 3)[o], rho=rho[o], acc=acc.reshape(-1, 3)[o],
                ncount=cnt[o])


def same_state(got, want, what=""):
    for k in ("ids", "pos", "vel", "rho", "acc", "ncount"):
        assert got[k].shape == want[k].shape, "%s %s: %r against %r" % (what, k, got[k].shape, want[k].shape)
        assert np.array_equal(bits(got[k]), bits(want[k])), "%s %s differs" % (what, k)


def check_totals(sph, want):
    t, _, _ = sph.getPorts()
    assert t.emitted.tolist() == want["emitted"].tolist() and t.removed.tolist() == want["removed"].tolist()
    assert t.live == want["live"] and t.next_id == want["next_id"]


def error_word(sph):
    live, owned, err = C.c_int32(), C.c_int32(), C.c_int32()
    sph.call("sph_hip_slab_status", C.byref(live), C.byref(owned), C.byref(err))
    return err.value


def run_block(S, steps=STEPS, mode=None):
    p, pos, vel, mass, emitters, sinks = block_scene()
    sph = S.SPH(mass.size, p, mode=S.MODE_FULL if mode is None else mode, capacity=6000)
    sph.setParticles(pos, vel, mass)
    sph.setPorts(emitters, sinks)
    sph.run(steps)
    return sph


# ---- 1. FULL against the oracle ------------------------------------------------------------------------------
def test_full_equals_the_oracle(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    want = block_reference()
    hist = want["history"]
    # the case is what it is meant to be: removals in several steps, one of them a step that also emits; a
    # layer of more than one 256-lane block appended behind a count that is no multiple of 64
    assert sum(1 for _, r, _ in hist if r > 0) >= 4
    assert any(r > 0 and m > 0 for _, r, m in hist[1:])
    assert all(m == 324 for _, _, m in hist[::3]) and any(live % 64 for live, _, m in hist if m)
    assert want["live"] <= 6000
    with run_block(S) as sph:
        same_state(live_state(sph), want, "after run(30)")
        check_totals(sph, want)
        assert error_word(sph) == 0
        # the Python mirror: the live rows in ascending id order
        part = sph.getParticles()
        assert np.array_equal(part.mId, want["ids"]) and sph.getParticleCount() == want["live"]
        assert np.array_equal(bits(part.mPosition), bits(want["pos"].reshape(-1)))
        assert np.array_equal(part.mNeighborCount, want["ncount"])
        t, emitters, sinks = sph.getPorts()
        assert emitters == block_scene()[4] and sinks == block_scene()[5]


# ---- 2. FULL_FAST against the existing route -----------------------------------------------------------------
def test_fast_equals_the_existing_route(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, emitters, sinks = block_scene()
    edits = PE.PortRun(to_oracle_params(p), pos, vel, mass, emitters, sinks)
    with S.SPH(N0, p, mode=S.MODE_FULL_FAST, capacity=6000) as sph, \
            S.SPH(N0, p, mode=S.MODE_FULL_FAST, capacity=6000) as plain:
        sph.setParticles(pos, vel, mass)
        sph.setPorts(emitters, sinks)
        for step in range(10):
            now = live_state(sph)
            assert np.array_equal(now["ids"], edits.ids)
            edits.pos, edits.vel = now["pos"].copy(), now["vel"].copy()
            assert edits.apply_ports()
            n = edits.live
            plain.call("sph_hip_slab_upload", n, np.ascontiguousarray(edits.pos).ctypes.data_as(C.c_void_p),
                       np.ascontiguousarray(edits.vel).ctypes.data_as(C.c_void_p),
                       np.ascontiguousarray(edits.mass).ctypes.data_as(C.c_void_p),
                       np.ascontiguousarray(edits.ids).ctypes.data_as(C.c_void_p), 1)
            plain.step()
            sph.step()
            same_state(live_state(sph), live_state(plain), "step %d" % step)
        t, _, _ = sph.getPorts()
        assert t.emitted.tolist() == edits.emitted.tolist() and t.removed.tolist() == edits.removed.tolist()
        assert t.live == edits.live and error_word(sph) == 0 and edits.removed[0] > 0


# ---- 3. filling from empty -----------------------------------------------------------------------------------
def test_filling_from_empty(oracle, hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass, emitters, sinks = scenes.filling_tank(20000, speed=10.0)
    assert max(p.full_cells_x, p.full_cells_y, p.full_cells_z) <= 16
    e = emitters[0]
    run = PE.PortRun(to_oracle_params(p), pos, vel, mass, emitters, sinks)
    for _ in range(12):
        assert run.step(oracle)
    layers = 1 + 11 // e.every
    assert run.live == layers * e.points and layers >= 2
    with S.SPH(0, p, capacity=20000) as sph:
        sph.setParticles(pos, vel, mass)
        assert sph.getParticleCount() == 0
        sph.setPorts(emitters, sinks)
        sph.run(12)
        assert sph.getParticleCount() == layers * e.points
        same_state(live_state(sph), snapshot(run), "12 steps from empty")
        check_totals(sph, snapshot(run))
        assert error_word(sph) == 0


# ---- 4. drain and refill -------------------------------------------------------------------------------------
def test_drain_and_refill(oracle, hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, emitters, _ = block_scene()
    refill = [S.Emitter(0, (0.7, 0.2, 0.2), (18, 18), 0.0317, (-15.0, 0.0, 0.0), 1.0, first=5, every=2)]
    drain = [S.Sink((-1.0, -1.0, -1.0), (0.6, 2.0, 2.0))]      # the whole block; the inlet plane is outside it
    run = PE.PortRun(to_oracle_params(p), pos, vel, mass, refill, drain)
    with S.SPH(N0, p, capacity=6000) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setPorts(refill, drain)
        sph.run(3)
        for _ in range(3):
            assert run.step(oracle)
        assert run.live == 0 and sph.getParticleCount() == 0 and sph.getPorts()[0].removed.tolist() == [N0]
        assert live_state(sph)["ids"].size == 0
        sph.run(2)                       # further steps with nothing resident
        sph.run(6)                       # the emitter refills the tank: layers in steps 5, 7 and 9
        for _ in range(8):
            assert run.step(oracle)
        assert run.live > 0 and run.layers_emitted == 3
        same_state(live_state(sph), snapshot(run), "refilled")
        check_totals(sph, snapshot(run))
        assert error_word(sph) == 0


# ---- 5. capacity ---------------------------------------------------------------------------------------------
def test_capacity_refusal(oracle, hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, emitters, _ = block_scene()
    cap = N0 + 324 + 162
    run = PE.PortRun(to_oracle_params(p), pos, vel, mass, emitters, [], capacity=cap)
    with S.SPH(N0, p, capacity=cap) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setPorts(emitters, [])
        with pytest.raises(S.SphHipError) as exc:
            sph.run(10)
        assert "(-3)" in str(exc.value) and "more than the context capacity %d" % cap in str(exc.value)
        assert "nothing of the step was enqueued" in str(exc.value)
        accepted = 0
        while run.step(oracle):
            accepted += 1
        assert accepted == 3 and run.live == N0 + 324
        same_state(live_state(sph), snapshot(run), "after the last accepted step")
        check_totals(sph, snapshot(run))
        # the schedule did not advance: the same step is refused again
        with pytest.raises(S.SphHipError, match="port step 3 would emit 324"):
            sph.step()
        check_totals(sph, snapshot(run))
        # without ports the context steps on
        sph.setPorts()
        run.set_ports()
        sph.run(2)
        for _ in range(2):
            assert run.step(oracle)
        same_state(live_state(sph), snapshot(run), "after clearing")
        assert error_word(sph) == 0


# ---- 6. with the rest of the scene ---------------------------------------------------------------------------
def test_with_obstacle_loads_and_gauges(oracle, hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    from smoothed_particle_hydrodynamics_amd import scenes
    steps = 20
    p, pos, vel, mass, emitters, sinks = scenes.channel_flow(3000, box=(1.0, 0.5, 0.5), speed=10.0)
    assert (p.full_cells_x, p.full_cells_y, p.full_cells_z) == (16, 8, 8)
    p.damping = 0.6
    obst = [O.Cylinder(1, (0.5, 0.0, 0.25), 0.06, -1.0, 2.0)]
    pos, vel, mass = scenes.carve(pos, vel, mass, obst)
    vel = scenes.box_fill(mass.size, (-20.0,) * 3, (20.0,) * 3, 3)     # something that runs into the pillar
    iso = 0.5 * 3000 / (1.0 * 0.25 * 0.5) * float(p.kernel1) * float(p.sim_scale) ** 6 * float(p.h) ** 9 * 64.0 * np.pi / 315.0
    gauges = [S.ColumnGauge((0.2, 0.0, 0.25), 1, 0.5 * p.h, 12, iso), S.ColumnGauge((0.02, 0.0, 0.25), 1, 0.5 * p.h, 12, iso),
              S.PointGauge((0.3, 0.1, 0.25))]
    eg = [G.of(g) for g in gauges]
    op, free = to_oracle_params(p), to_oracle_params(p)
    free.apply_walls = 0
    dt, damping, maxv = F32(p.time_step), F32(p.damping), F32([p.max_x, p.max_y, p.max_z])
    rows, readings = [], []

    def respond(P, V0, acc, m):
        qpos, qvel = P.copy(), V0.copy()
        oracle.integrate(free, qpos, qvel, acc, m)
        V, Q, row = L.respond(maxv, 1, obst, P, qvel, qpos, dt, damping, m)
        rows.append(row)
        return V, Q

    def read(run):
        readings.append(G.evaluate(p, np.ascontiguousarray(run.pos.reshape(-1)), np.ascontiguousarray(run.vel.reshape(-1)),
                                   run.mass, eg))

    run = PE.PortRun(op, pos, vel, mass, emitters, sinks)
    for _ in range(steps):
        assert run.step(oracle, respond, read)
    assert run.layers_emitted >= 2 and run.removed[0] > 0 and run.live <= 6000
    with S.SPH(mass.size, p, capacity=6000) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setObstacles(obst)
        sph.setGauges(gauges)
        sph.setPorts(emitters, sinks)
        sph.recordLoads(steps)
        sph.recordGauges(steps)
        sph.run(steps)
        same_state(live_state(sph), snapshot(run), "channel")
        check_totals(sph, snapshot(run))
        loads = sph.getLoads()
        assert loads.impulse_q.shape[0] == steps
        for r, row in enumerate(rows):
            assert row.same(loads.impulse_q[r], loads.count[r], loads.skipped[r]), "load row %d" % r
        assert loads.count[:, 6].sum() > 0, "the scene is meant to run into the pillar"
        rec = sph.getGaugeRecord()
        assert rec.steps.tolist() == list(range(steps))
        for r in range(steps):
            assert G.same_readings(G.Readings(rec.v[r], rec.n[r], rec.k[r]), readings[r]), "gauge row %d" % r
        assert rec.n[:, 2].max() > 0 and error_word(sph) == 0


# ---- 7. routes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", [("SPH_HIP_UNTILED", "1"), ("SPH_HIP_TILE_CAP", "256")])
def test_routes_give_the_same_bits(hiplib, switch):
    import smoothed_particle_hydrodynamics_amd as S
    want = block_reference()
    old = os.environ.get(switch[0])
    os.environ[switch[0]] = switch[1]          # read at creation
    try:
        sph = run_block(S)
    finally:
        if old is None:
            del os.environ[switch[0]]
        else:
            os.environ[switch[0]] = old
    with sph:
        stats = sph.tile_stats()
        if switch[0] == "SPH_HIP_TILE_CAP":
            assert stats["capacity_density"] == 256
        same_state(live_state(sph), want, "=".join(switch))
        check_totals(sph, want)
        assert error_word(sph) == 0


# ---- 8. clearing and refusals --------------------------------------------------------------------------------
def test_clearing_and_refusals(oracle, hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, emitters, sinks = block_scene()
    run = PE.PortRun(to_oracle_params(p), pos, vel, mass, emitters, sinks)
    n = mass.size
    out = [np.zeros(3 * 6000, F32), np.zeros(3 * 6000, F32), np.zeros(6000, F32), np.zeros(3 * 6000, F32),
           np.zeros(6000, np.int32)]
    args = [a.ctypes.data_as(C.c_void_p) for a in out]
    with S.SPH(n, p, capacity=6000) as sph:
        sph.setParticles(pos, vel, mass)
        sph.call("sph_hip_download", *args)                    # before any port step: as always
        sph.setPorts(emitters, sinks)
        sph.call("sph_hip_download", *args)                    # ... and with ports set but no step taken
        sph.run(4)
        for _ in range(4):
            assert run.step(oracle)
        sph.setPorts()                                          # cleared: the default route from here on
        run.set_ports()
        assert sph.getPorts()[1:] == ([], [])
        sph.run(3)
        for _ in range(3):
            assert run.step(oracle)
        same_state(live_state(sph), snapshot(run), "default route after clearing")
        assert error_word(sph) == 0
        for name, extra in (("sph_hip_download", []), ("sph_hip_download_async", [None, None])):
            with pytest.raises(S.SphHipError, match="use sph_hip_download_live") as exc:
                sph.call(name, *args, *extra)
            assert "ids are no longer 0..n-1" in str(exc.value) and name in str(exc.value)
        # ports set again and stepped, then an upload: the download works, the schedule restarts at step 0
        late = [S.Emitter(0, (0.7, 0.2, 0.2), (18, 18), 0.0317, (-15.0, 0.0, 0.0), 1.0, first=0, every=3)]
        sph.setPorts(late, [])
        sph.run(2)                                              # port steps 0 and 1: one layer
        assert sph.getPorts()[0].emitted.tolist() == [324]
        sph.setParticles(pos, vel, mass)
        t, kept, _ = sph.getPorts()
        assert kept == late and t.emitted.tolist() == [0] and t.live == n and t.next_id == n
        sph.call("sph_hip_download", *args)
        assert np.array_equal(bits(out[0][:3 * n]), bits(pos))
        sph.step()                                              # port step 0 again: the emitter fires
        t, _, _ = sph.getPorts()
        assert t.emitted.tolist() == [324] and t.live == n + 324 and t.next_id == n + 324
        again = PE.PortRun(to_oracle_params(p), pos, vel, mass, late, [])
        assert again.step(oracle)
        same_state(live_state(sph), snapshot(again), "after the upload")
    # REF and slab contexts refuse
    from smoothed_particle_hydrodynamics_amd import scenes
    pr, rpos, rvel, rmass = scenes.dense_block(512)
    with S.SPH(512, pr, mode=S.MODE_REF) as ref:
        ref.setParticles(rpos, rvel, rmass)
        with pytest.raises(S.SphHipError, match="FULL and FULL_FAST contexts only"):
            ref.setPorts(emitters, sinks)
    from smoothed_particle_hydrodynamics_amd.lib import Context
    from smoothed_particle_hydrodynamics_amd import ports as PP
    slab = Context("sph_hip_create_slab", C.byref(p), 4096, 0, 0, 8)
    try:
        ea, ne = PP.as_emitter_array(emitters)
        with pytest.raises(S.SphHipError, match="slab contexts"):
            slab.call("sph_hip_set_ports", ea, ne, None, 0)
    finally:
        slab.close()
