"""GPU: gauges (include/sph_hip.h: sph_hip_set_gauges).  k_gauges_read inside sph_hip_step, sph_hip_run and the
phase calls, and in sph_hip_read_gauges, equals the numpy restatement (tests/gauge_emulation.py) on the state
each step starts from, bit for bit; gauges and their recording change no particle; recordings, refusals and
edge cases.

The figures CPU_* are what the same scene gives on the CPU, the oracle's FULL step driving the restatement
(DESIGN.md section 19); `python tests/test_gpu_gauges.py` prints them again.  FULL mode is bit-identical to
the oracle, so its counts equal them; FULL_FAST's arithmetic differs in the particles, so there every class
must occur and the counts are printed."""
import functools
import os

import numpy as np
import pytest

import gauge_emulation as G
import sample_emulation as SE
from helpers import to_oracle_params

pytestmark = pytest.mark.gpu

F32 = np.float32
STEPS = 30
SPEED = 4.0

# cpu_figures(): gauge evaluations of each class over the STEPS states the steps start from
# (gauge_emulation.Info: interior, saturated, dry, gap, clamped, both_signs, partial).  No interior top can
# clamp: fa > iso >= fb puts t in (0, 1]; tests/test_gauges_cpu.py covers the clamp.
CPU_INTERIOR = 262
CPU_SATURATED = 42
CPU_DRY = 56
CPU_GAP = 292
CPU_CLAMPED = 0
CPU_BOTH_SIGNS = 74
CPU_PARTIAL = 115
CPU_FIGURES = (CPU_INTERIOR, CPU_SATURATED, CPU_DRY, CPU_GAP, CPU_CLAMPED, CPU_BOTH_SIGNS, CPU_PARTIAL)


@functools.lru_cache(maxsize=None)
def scene():
    """scenes.dam_break(20000, speed=SPEED), gravity and walls on (the tracer tests' scene, h = 0.031), iso = half
    the median of the restatement's density at the particles' own positions, and the gauges: (params, pos, vel,
    mass, iso, gauges)."""
    from smoothed_particle_hydrodynamics_amd import scenes
    from smoothed_particle_hydrodynamics_amd.gauges import ColumnGauge, PointGauge, SectionGauge
    p, pos, vel, mass = scenes.dam_break(20000, speed=SPEED)
    p.apply_gravity = 1
    p.apply_walls = 1
    p.gravity[0], p.gravity[1], p.gravity[2] = 0.0, -9.81, 0.0
    x = pos.reshape(-1, 3)
    own = SE.Grid(p, pos, vel, mass).sample(x, velocity=False)[0]
    iso = float(F32(0.5) * F32(np.median(own)))
    h = float(F32(p.h))
    s = float(F32(0.5) * F32(p.h))
    gauges = []
    # columns up y: one probe, fewer than a wave, one short of a wave, a wave, one more, more than two waves
    for m in (1, 20, 63, 64, 65, 129):
        gauges.append(ColumnGauge((0.05, 0.0, 0.5), 1, s, m, iso))
    gauges.append(ColumnGauge((0.6, 0.0, 0.5), 1, s, 65, iso))              # dry at first
    gauges.append(ColumnGauge((-0.002, 0.0, 0.5), 1, s, 65, iso))           # its base just outside the box
    gauges.append(ColumnGauge((0.0, 0.3, 0.5), 0, s, 65, iso))              # along x through the fluid
    gauges.append(ColumnGauge((0.05, 0.3, 0.0), 2, s, 65, iso))             # along z through the fluid
    gauges.append(ColumnGauge((0.0, 0.75, 0.5), 0, s, 65, iso))             # along x in the column's top face
    gauges.append(ColumnGauge((0.1, 0.0, 0.25), 1, s, 65, iso))             # up y in the column's free face
    # sections with normal x at x = 0.1 + h over y in [0, 0.8], z in [0, 1]
    plane = 0.1 + h
    gauges.append(SectionGauge((plane, 0.0, 0.0), 0, (0.8 / 31, 1.0 / 31), (32, 32), iso))
    gauges.append(SectionGauge((plane, 0.0, 0.0), 0, (0.8, 1.0), (1, 1), iso))
    gauges.append(SectionGauge((plane, 0.0, 0.0), 0, (0.8 / 4, 1.0 / 12), (5, 13), iso))
    gauges.append(SectionGauge((plane, 0.0, 0.0), 0, (0.8 / 63, 1.0 / 63), (64, 64), iso))
    gauges.append(SectionGauge((0.0, 0.4, 0.0), 1, (0.2 / 7, 1.0 / 31), (8, 32), iso))      # normal y, through the fluid
    gauges.append(SectionGauge((0.05, 0.0, 0.5), 2, (0.15 / 7, 0.9 / 31), (8, 32), iso))    # normal z, through the fluid
    gauges.append(SectionGauge((0.7, 0.0, 0.0), 0, (0.8 / 31, 1.0 / 31), (32, 32), iso))    # in the empty half
    # points: on particles, in the empty box, outside the box and at extremes
    rng = np.random.default_rng(19)
    for q in x[rng.choice(len(x), 64, replace=False)]:
        gauges.append(PointGauge(tuple(float(c) for c in q)))
    for q in (np.array([0.5, 0.1, 0.1], F32) + rng.random((64, 3)) * np.array([0.4, 0.8, 0.8])).astype(F32):
        gauges.append(PointGauge(tuple(float(c) for c in q)))
    for q in ((-0.001, 0.3, 0.5), (0.05, -0.001, 0.5), (0.05, 0.3, 1.001), (1.5, 1.5, 1.5), (3e38, 0.3, 0.5),
              (0.05, -3e38, 0.5), (3e38, 3e38, 3e38), (-3e38, -3e38, -3e38)):
        gauges.append(PointGauge(q))
    return p, pos, vel, mass, iso, tuple(gauges)


N_COLUMNS, N_SECTIONS, N_POINTS = 12, 7, 136
FIRST_POINT = N_COLUMNS + N_SECTIONS


def emu(gauges):
    return [G.of(g) for g in gauges]


def cpu_figures():
    """scene() stepped by the oracle's FULL step, the restatement reading the gauges in each step's starting
    state: the classes summed over the STEPS states, every one of them present (but the clamp, which cannot be)."""
    from oracle.oracle import Oracle, build
    build(ref=False)
    orc = Oracle()
    p, pos, vel, mass, iso, gauges = scene()
    op = to_oracle_params(p)
    eg = emu(gauges)
    pos, vel = pos.copy(), vel.copy()
    total = np.zeros(len(G.Info._fields), np.int64)
    for _ in range(STEPS):
        total += np.array(G.evaluate(p, pos, vel, mass, eg, with_info=True)[1])
        orc.step(op, pos, vel, mass, mode="full")
    check_classes(total)
    return tuple(int(v) for v in total)


def check_classes(total):
    """The run is not vacuous: every class of reading occurred (a clamped t cannot: fa > iso >= fb)."""
    info = G.Info(*[int(v) for v in total])
    assert info.interior > 0 and info.saturated > 0 and info.dry > 0 and info.gap > 0, info
    assert info.both_signs > 0 and info.partial > 0, info
    assert info.clamped == 0, info


def mode_of(S, name):
    return {"full": S.MODE_FULL, "fast": S.MODE_FULL_FAST}[name]


def particles(sph):
    part = sph.getParticles()
    return part.mPosition.copy(), part.mVelocity.copy()


def row_of(rec, r):
    return G.Readings(rec.v[r], rec.n[r], rec.k[r])


def fresh(S, mode="full", with_gauges=True):
    p, pos, vel, mass, _, gauges = scene()
    sph = S.SPH(mass.size, p, mode=mode_of(S, mode))
    sph.setParticles(pos, vel, mass)
    if with_gauges:
        sph.setGauges(gauges)
    return sph


# ---- per-step pin, and the figures -------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["full", "fast"])
def test_every_step_equals_the_restatement(hiplib, mode):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, iso, gauges = scene()
    eg = emu(gauges)
    assert len(gauges) == N_COLUMNS + N_SECTIONS + N_POINTS
    with fresh(S, mode) as sph:
        assert len(sph.getGauges()) == len(gauges)
        sph.recordGauges(STEPS + 1)
        want, total = [], np.zeros(len(G.Info._fields), np.int64)
        for _ in range(STEPS):
            gpos, gvel = particles(sph)
            out, info = G.evaluate(p, gpos, gvel, mass, eg, with_info=True)
            want.append(out)
            total += np.array(info)
            sph.step()
        rec = sph.getGaugeRecord()
        assert rec.steps.tolist() == list(range(STEPS)) and rec.v.shape == (STEPS, len(gauges), 4)
        for r in range(STEPS):
            assert G.same_readings(row_of(rec, r), want[r]), "row %d" % r
        gpos, gvel = particles(sph)
        assert G.same_readings(sph.readGauges(), G.evaluate(p, gpos, gvel, mass, eg))
    print("gauge classes %r (CPU %r)" % (G.Info(*[int(v) for v in total]), CPU_FIGURES))
    check_classes(total)
    if mode == "full":
        assert tuple(int(v) for v in total) == CPU_FIGURES


def test_point_gauges_equal_the_sampler(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, iso, gauges = scene()
    pts = np.array([g.point for g in gauges[FIRST_POINT:]], F32)
    with fresh(S, "fast") as sph:
        for k in range(3):
            got = sph.readGauges()
            rho, u, cnt = sph.sampleFields(pts)
            assert np.array_equal(got.v[FIRST_POINT:, 0].view(np.uint32), rho.view(np.uint32))
            assert np.array_equal(got.v[FIRST_POINT:, 1:].view(np.uint32), u.view(np.uint32))
            assert np.array_equal(got.n[FIRST_POINT:], cnt) and not got.k[FIRST_POINT:].any()
            assert (cnt[:64] > 0).all() and not cnt[64:128].any()
            sph.run(5)


# ---- gauges change nothing ------------------------------------------------------------------------------------
def full_state(sph):
    part = sph.getParticles()
    return [part.mPosition.copy(), part.mVelocity.copy(), part.mDensity.copy(), part.mAcceleration.copy(),
            part.mNeighborCount.copy()], sph.energy()


@pytest.mark.parametrize("mode", ["full", "fast"])
def test_gauges_and_a_recording_change_no_particle(hiplib, mode):
    import smoothed_particle_hydrodynamics_amd as S
    out = []
    for with_gauges in (False, True):
        with fresh(S, mode, with_gauges) as sph:
            if with_gauges:
                sph.recordGauges(60)
            sph.run(50)
            if with_gauges:
                # a read in the middle of the comparison changes nothing either
                before = sph.getParticles().mPosition.tobytes()
                sph.readGauges()
                sph.syncParticles()
                assert sph.getParticles().mPosition.tobytes() == before
                assert len(sph.getGaugeRecord().steps) == 50
            out.append(full_state(sph))
    for a, b in zip(out[0][0], out[1][0]):
        assert a.tobytes() == b.tobytes()
    assert out[0][1] == out[1][1]


@pytest.mark.parametrize("mode", ["full", "fast"])
def test_gauges_change_nothing_with_tracers_obstacles_and_a_body(hiplib, mode):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd.gauges import ColumnGauge, PointGauge, SectionGauge
    from smoothed_particle_hydrodynamics_amd.obstacles import Body
    from test_gpu_obstacles import walled_scene
    p, pos, vel, mass, obst = walled_scene()
    bodies = [Body(5000.0, free=(True, False, False), travel_lo=(-0.2, 0.0, 0.0), travel_hi=(0.2, 0.0, 0.0)), None, None]
    tracers = pos.reshape(-1, 3)[::8].copy()
    iso = float(F32(0.5) * F32(np.median(SE.Grid(p, pos, vel, mass).sample(pos.reshape(-1, 3), velocity=False)[0])))
    h = float(p.h)
    gauges = [ColumnGauge((0.6, 0.0, 0.7), 1, h / 2, 40, iso), SectionGauge((0.65, 0.0, 0.0), 0, (h / 2, h / 2), (30, 32), iso),
              PointGauge((0.5, 0.5, 0.5))]
    out = []
    for with_gauges in (False, True):
        with S.SPH(mass.size, p, mode=mode_of(S, mode)) as sph:
            sph.setParticles(pos, vel, mass)
            sph.setObstacles(obst)
            sph.setBodies(bodies)
            sph.setTracers(tracers)
            if with_gauges:
                sph.setGauges(gauges)
                sph.recordGauges(STEPS, 2)
            sph.run(STEPS)
            got = sph.getBodies()
            t = sph.getTracers()
            out.append(full_state(sph) + (got.displacement.tobytes(), got.velocity.tobytes(), t.position.tobytes(),
                                          t.wet_steps.tobytes(), t.dry_steps.tobytes()))
            if with_gauges:
                rec = sph.getGaugeRecord()
                assert rec.steps.tolist() == list(range(0, STEPS, 2)) and rec.n[:, :2].any() and rec.n[:, 2].any()
    for a, b in zip(out[0][0], out[1][0]):
        assert a.tobytes() == b.tobytes()
    assert out[0][1:] == out[1][1:]


# ---- stepping ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["full", "fast"])
def test_run_step_and_phase_calls_give_the_same_record(hiplib, mode):
    import smoothed_particle_hydrodynamics_amd as S
    out = []
    for route in ("run", "step", "phases"):
        with fresh(S, mode) as sph:
            sph.recordGauges(STEPS)
            if route == "run":
                sph.run(STEPS)
            for _ in range(STEPS if route != "run" else 0):
                if route == "step":
                    sph.step()
                else:
                    sph.voxelizeParticles()
                    sph.findNeighbors()
                    sph.computeDensity()
                    sph.computeAcceleration()
                    sph.integrate()
            rec = sph.getGaugeRecord()
            out.append((rec, particles(sph)))
    assert out[0][0].steps.tolist() == list(range(STEPS)) and out[0][0].n.any()
    for rec, _ in out[1:]:
        assert np.array_equal(rec.steps, out[0][0].steps) and G.same_readings(rec, out[0][0])


def test_time_step_and_read_only_calls_between_steps(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, iso, gauges = scene()
    eg = emu(gauges)
    with fresh(S, "full") as sph:
        sph.recordGauges(6)
        want = []
        for k in range(6):
            if k == 3:
                sph.setTimeStep(0.0025)
            gpos, gvel = particles(sph)
            if k % 2:
                # a sampler, extractor or gauge read between steps moves the particles in memory and no reading
                sph.sampleFields(pos.reshape(-1, 3)[:100])
                sph.extractSurface((0.0, 0.0, 0.0), (0.05, 0.05, 0.05), (8, 16, 20), iso)
                sph.readGauges()
            want.append(G.evaluate(sph.getParams(), gpos, gvel, mass, eg))
            sph.step()
        rec = sph.getGaugeRecord()
        assert rec.steps.tolist() == list(range(6)) and F32(sph.getTimeStep()) == F32(0.0025)
        for r in range(6):
            assert G.same_readings(row_of(rec, r), want[r]), "row %d" % r


# ---- recording --------------------------------------------------------------------------------------------------
def test_recording_rows_and_steps(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import SphHipError
    p, pos, vel, mass, iso, gauges = scene()
    with fresh(S, "fast") as sph:
        assert len(sph.getGaugeRecord().steps) == 0
        sph.step()
        assert len(sph.getGaugeRecord().steps) == 0          # no recording: nothing is kept
        sph.recordGauges(10, 3)
        seen = {}
        for s in range(STEPS):
            seen[s] = sph.readGauges()
            sph.step()
        rec = sph.getGaugeRecord()
        assert rec.steps.tolist() == list(range(0, 28, 3)) and rec.v.shape == (10, len(gauges), 4)
        for r, s in enumerate(rec.steps):
            assert G.same_readings(row_of(rec, r), seen[int(s)]), "row %d" % r
        # above the 64 MiB budget: refused, the old recording stays
        fits = (64 << 20) // (24 * len(gauges))
        with pytest.raises(SphHipError, match="64 MiB"):
            sph.recordGauges(fits + 1, 1)
        for bad, why in (((-1, 1), "rows"), ((1, 0), "every")):
            with pytest.raises(SphHipError, match=why):
                sph.recordGauges(*bad)
        again = sph.getGaugeRecord()
        assert again.steps.tolist() == rec.steps.tolist() and G.same_readings(again, rec)
        for first, n in ((-1, 1), (0, 11), (10, 1)):
            with pytest.raises(SphHipError, match="range"):
                sph.call("sph_hip_get_gauge_record", first, n, None, None)
        # the last row that fits is accepted
        sph.recordGauges(fits, 1)
        # a partly filled recording returns the filled rows only
        sph.recordGauges(5, 2)
        sph.run(4)
        assert sph.getGaugeRecord().steps.tolist() == [0, 2]
        # a recording goes on across an upload, a setter and a change of arithmetic
        gpos, gvel = particles(sph)
        sph.setParticles(gpos, gvel, mass)
        sph.setStiffness(sph.getStiffness())
        sph.setArithmetic(S.ARITH_EXACT)
        sph.setArithmetic(S.ARITH_FAST)
        sph.run(2)
        assert sph.getGaugeRecord().steps.tolist() == [0, 2, 4]
        # setting gauges ends a recording; rows = 0 stops one
        sph.setGauges(gauges[:10])
        sph.run(2)
        assert len(sph.getGaugeRecord().steps) == 0
        sph.recordGauges(4)
        sph.recordGauges(0)
        sph.step()
        assert len(sph.getGaugeRecord().steps) == 0
        # no gauges: a recording is refused, a read does nothing
        sph.setGauges([])
        with pytest.raises(SphHipError, match="no gauges"):
            sph.recordGauges(3)
        sph.recordGauges(0)
        assert sph.readGauges().v.shape == (0, 4) and sph.getGauges() == []
        sph.run(2)


# ---- refusals and edge cases ----------------------------------------------------------------------------------------
def test_refusals_keep_the_old_set_and_recording(hiplib):
    import ctypes as C

    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import SphHipError, scenes
    from smoothed_particle_hydrodynamics_amd import gauges as PG
    from smoothed_particle_hydrodynamics_amd.slab import HipSlab
    p, pos, vel, mass, iso, gauges = scene()
    col, sec, pt = gauges[4], gauges[14], gauges[FIRST_POINT]
    nan, inf = float("nan"), float("inf")
    bad = [
        (col._replace(axis=3), "axis"), (sec._replace(axis=-1), "axis"),
        (col._replace(base=(0.05, nan, 0.5)), "not finite"), (pt._replace(point=(inf, 0.0, 0.0)), "not finite"),
        (sec._replace(spacing=(0.01, -inf)), "not finite"), (col._replace(iso=nan), "not finite"),
        (col._replace(spacing=0.0), "spacing"), (sec._replace(spacing=(0.01, -0.01)), "spacing"),
        (col._replace(samples=0), "count"), (sec._replace(shape=(4, 0)), "count"),
        (col._replace(samples=4097), "probes"), (sec._replace(shape=(64, 65)), "probes"),
        (col._replace(iso=0.0), "iso"), (sec._replace(iso=-1.0), "iso"),
    ]
    unknown = pt.to_struct()
    unknown.kind = 3
    bad.append((unknown, "kind"))
    unused = pt.to_struct()               # an unused field that is not finite
    unused.spacing[1] = nan
    bad.append((unused, "not finite"))
    with fresh(S, "full") as sph:
        sph.recordGauges(40)
        sph.run(3)
        kept = sph.getGauges()
        assert [type(g) for g in kept] == [type(g) for g in gauges]
        for k, (g, why) in enumerate(bad):
            with pytest.raises(SphHipError, match=why):
                sph.setGauges(list(gauges[:3]) + [g])
            assert sph.getGauges() == kept
        with pytest.raises(SphHipError, match="negative"):
            sph.call("sph_hip_set_gauges", None, -1)
        with pytest.raises(SphHipError, match="null"):
            sph.call("sph_hip_set_gauges", None, 2)
        many = (PG.SphGauge * 4097)()
        for i in range(4097):
            many[i] = pt.to_struct()
        with pytest.raises(SphHipError, match="SPH_HIP_MAX_GAUGES"):
            sph.call("sph_hip_set_gauges", many, 4097)
        assert sph.getGauges() == kept
        # the recording went on through every refusal
        sph.run(2)
        rec = sph.getGaugeRecord()
        assert rec.steps.tolist() == [0, 1, 2, 3, 4] and rec.v.shape[1] == len(gauges)
        # the gauges survive an upload, a setter and a change of arithmetic
        gpos, gvel = particles(sph)
        before = sph.readGauges()
        sph.setParticles(gpos, gvel, mass)
        sph.setStiffness(sph.getStiffness())
        sph.setArithmetic(S.ARITH_FAST)
        sph.setArithmetic(S.ARITH_EXACT)
        assert sph.getGauges() == kept and G.same_readings(sph.readGauges(), before)
        # the most a context takes: 4 096 gauges
        sph.call("sph_hip_set_gauges", many, 4096)
        got = sph.readGauges()
        assert got.v.shape == (4096, 4) and (got.n == got.n[0]).all() and got.n[0] > 0
        # clearing
        sph.setGauges([])
        assert sph.getGauges() == [] and sph.call("sph_hip_get_gauges", None, 0) == 0
        sph.run(2)
    q, rpos, rvel, rmass = scenes.dense_block(2000)
    with S.SPH(rmass.size, q, mode=S.MODE_REF) as ref:
        ref.setParticles(rpos, rvel, rmass)
        with pytest.raises(SphHipError, match="FULL"):
            ref.setGauges(gauges[:4])
        assert ref.getGauges() == []
    with HipSlab(p, 0, p.full_cells_z // 2, 20000, 1024, has_left=False) as slab:
        arr, n = PG.as_array(gauges[:4])
        with pytest.raises(SphHipError, match="slab"):
            slab.call("sph_hip_set_gauges", arr, n)
    assert C.sizeof(PG.SphGauge) == 40


def test_an_empty_context_reads_zeros_and_dry_columns(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, iso, gauges = scene()
    eg = emu(gauges)
    want = G.evaluate(p, pos[:0], vel[:0], mass[:0], eg)
    assert (want.k[:N_COLUMNS] == -1).all() and not want.n.any() and not want.v[N_COLUMNS:].any()
    with S.SPH(mass.size, p, mode=S.MODE_FULL) as sph:
        sph.setGauges(gauges)
        sph.recordGauges(3)
        assert G.same_readings(sph.readGauges(), want)
        sph.run(3)
        rec = sph.getGaugeRecord()
        assert rec.steps.tolist() == [0, 1, 2]
        for r in range(3):
            assert G.same_readings(row_of(rec, r), want)
        # after particles were resident and are gone again, the same
        sph.setParticles(pos, vel, mass)
        sph.step()
        assert sph.readGauges().n.any()
        sph.setParticles(pos[:0], vel[:0], mass[:0])
        assert G.same_readings(sph.readGauges(), want)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(dict(zip(G.Info._fields, cpu_figures())))
