"""GPU: the feature passes off unit scale.  Every kernel that sums over neighbours exists as UNIT_SCALE true and
false (csrc/launch.h: unit_scale); the features' own files run the true one only.  Here the samplers (points and
lattices, every route), k_particle_density, the gauges of all five kinds, the carried scalars, the tracers, the
surface extractor, the three renderers and every hooked integrate (static obstacles, load recordings, Motions,
MotionPaths, a free Body, buoyancy, ports) run
under the parameter sets of tests/scale_cases.py - SCALED (sim_scale = 0.5), SHELL (hscaled = 0.95 h at a scale of
1) and, for the point samplers, SCALED_UP - and are held to the numpy restatements bit for bit, exactly as each
feature's own file holds them at unit scale.  The restatements model both arithmetics already
(sample_emulation.density_terms, scalar_emulation.Consts.unit).

The states only the general instantiations reach - a probe with members and a density of zero, a scalar pair with
a negative weight, a wet tracer that does not move - are asserted on the restatements' output, so that a scene
that loses them fails instead of testing nothing.  The figures CPU_* are what the scenes give on the CPU (the
restatements alone, in each scene's first state); `python tests/test_gpu_off_unit_scale.py` prints them again and
tests/test_off_unit_scale_cpu.py checks them."""
import functools
import os

import numpy as np
import pytest

import gauge_emulation as G
import pressure_emulation as P
import sample_emulation as SE
import scalar_emulation as SC
import scale_cases
import tracer_emulation as T
from helpers import to_oracle_params
from test_sample_cpu import TILED, policy, tiled  # noqa: F401  (policy: the g++ shim of sample_policy.h)

pytestmark = pytest.mark.gpu

F32 = np.float32
FLAVOURS = scale_cases.FLAVOURS
GAUGE_STEPS = 5
SCALAR_STEPS = 5
TRACER_STEPS = 10

# cpu_figures(): the scene of the point probes, gauges and tracers (scale_cases.block_scene) in its first state
CPU_SHELL_ZERO_DENSITY_PROBES = 911       # SHELL: point probes with count > 0 and rho == 0 (the bar: >= 64)
CPU_SHELL_ON_WITH_ZERO_TERM = 417         # SHELL: of the 512 on-particle probes, those with a member whose term is 0 (>= 5 %)
CPU_SHELL_TRACERS_WET_UNMOVED = 811       # SHELL: tracers wet and unmoved in the first step (>= 32)
CPU_SHELL_NEGATIVE_PAIRS = 5640           # SHELL: scalar pairs with a negative weight in the scalars' scene (>= N / 100)
CPU_SCALED_ISO_INSIDE = (8950, 7766)      # SCALED: (lattice points with members, of them inside the iso): 10 % .. 90 %
CPU_SCALED_ZERO_DENSITY_PROBES = 0        # SCALED drops no pair: the state does not exist there


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same(got, want, what):
    """bit for bit (float arrays as uint32, int arrays as they are), with the first difference in the message"""
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, "%s [%d]: %r %s against %r %s" % (what, k, g.shape, g.dtype, w.shape, w.dtype)
        bad = np.flatnonzero(g.reshape(-1).view(np.uint32) != w.reshape(-1).view(np.uint32))
        assert bad.size == 0, "%s [%d]: %d of %d differ, first at %d: %r against %r" % (
            what, k, bad.size, g.size, bad[0], g.reshape(-1)[bad[0]], w.reshape(-1)[bad[0]])


def mode_of(S, name):
    return {"full": S.MODE_FULL, "fast": S.MODE_FULL_FAST}[name]


def particles(sph):
    part = sph.getParticles()
    return part.mPosition.copy(), part.mVelocity.copy()


def context(S, scene, mode="full"):
    p, pos, vel, mass = scene[:4]
    sph = S.SPH(mass.size, p, mode=mode_of(S, mode))
    sph.setParticles(pos, vel, mass)
    return sph


# ---- the scene of the probes, and what the restatements say of it -----------------------------------------------
@functools.lru_cache(maxsize=None)
def probe_scene(flavour):
    """(params, pos, vel, mass, Probes, every probe, seeded scalars (n, 4), iso) of scale_cases.block_scene"""
    p, pos, vel, mass = scale_cases.block_scene(flavour)
    pr = scale_cases.probes(p, pos, vel, mass)
    values = np.random.default_rng(41).uniform(-1.0, 1.0, (mass.size, 4)).astype(F32)
    return p, pos, vel, mass, pr, scale_cases.every(pr), values, scale_cases.iso_of(p, pos, vel, mass, pr.on)


@functools.lru_cache(maxsize=None)
def probe_answers(flavour):
    """The restatements' answers on probe_scene's first state - computed once, shared, never changed: the field
    sampler's, the pressure sampler's, the scalar sampler's."""
    p, pos, vel, mass, pr, ev, values, iso = probe_scene(flavour)
    return SE.Grid(p, pos, vel, mass).sample(ev), P.sample(p, pos, vel, mass, ev), SC.sample(p, pos, vel, mass, values, ev)


def zero_density_probes(flavour):
    rho, _, count = probe_answers(flavour)[0]
    return int(((count > 0) & (rho == 0)).sum())


def on_probes_with_a_zero_term(flavour):
    p, pos, vel, mass, pr, ev, values, iso = probe_scene(flavour)
    return int((scale_cases.zero_term_members(p, pos, vel, mass, pr.on) > 0).sum())


def check_probe_conditions(flavour):
    """The states the flavour is there for exist in the restatement's answers."""
    p, pos, vel, mass, pr, ev, values, iso = probe_scene(flavour)
    rho, vel_, count = probe_answers(flavour)[0]
    on, empty = scale_cases.span(pr, "on"), scale_cases.span(pr, "empty")
    assert (count[on] >= 1).all() and not count[empty].any() and not rho[empty].any()
    if flavour == "SHELL":
        assert zero_density_probes(flavour) == CPU_SHELL_ZERO_DENSITY_PROBES >= 64
        assert on_probes_with_a_zero_term(flavour) == CPU_SHELL_ON_WITH_ZERO_TERM >= 0.05 * len(pr.on)
        shell = scale_cases.span(pr, "shell")
        assert len(pr.shell) >= 64 and (count[shell] == 1).all() and not rho[shell].any() and not vel_[shell].any()
        # the pressure and the scalars take the rho > 0 ? ... : 0 branch there too
        assert not probe_answers(flavour)[1][0][shell].any() and not probe_answers(flavour)[2][0][shell].any()
    elif flavour == "SCALED":
        assert zero_density_probes(flavour) == CPU_SCALED_ZERO_DENSITY_PROBES == 0
        assert (rho[on] > 0).all()
    else:
        assert zero_density_probes(flavour) >= 64          # SCALED_UP: most members fall outside hscaled


# ---- point samplers --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", scale_cases.POINT_FLAVOURS)
def test_point_samplers_equal_the_restatements(hiplib, flavour):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, pr, ev, values, iso = probe_scene(flavour)
    check_probe_conditions(flavour)
    want_f, want_p, want_s = probe_answers(flavour)
    got = {}
    for mode in ("full", "fast"):
        with context(S, (p, pos, vel, mass), mode) as sph:
            sph.setScalars(values)
            got[mode] = (sph.sampleFields(ev), sph.samplePressure(ev), sph.sampleScalars(ev))
            assert_same(sph.sampleFields(ev, velocity=False)[::2], want_f[::2], "%s %s fields without velocity" % (flavour, mode))
        assert_same(got[mode][0], want_f, "%s %s fields" % (flavour, mode))
        assert_same(got[mode][1], want_p, "%s %s pressure" % (flavour, mode))
        assert_same(got[mode][2], want_s, "%s %s scalars" % (flavour, mode))
    # and the restatement's cut-off is the float64 interpolation's: the bar of tests/test_sample_cpu.py
    rho, v, _ = got["full"][0]
    rho64, v64 = SE.brute_force64(p, pos, vel, mass, ev)
    np.testing.assert_allclose(rho, rho64, rtol=1e-5, atol=1e-5 * float(rho64.max()))
    np.testing.assert_allclose(v, v64, rtol=1e-5, atol=1e-5 * float(np.abs(v64).max()))


# ---- lattice samplers ------------------------------------------------------------------------------------------------
def block_lattice(p):
    """21 x 19 x 23 points h / 4 apart over a corner of the compressed block: multiples of no brick (8 x 8 x 4)"""
    s = float(F32(p.h) / F32(4))
    return (0.3, 0.3, 0.3), (s, s, s), (21, 19, 23)


@functools.lru_cache(maxsize=None)
def lattice_answers(flavour):
    p, pos, vel, mass, pr, ev, values, iso = probe_scene(flavour)
    origin, spacing, shape = block_lattice(p)
    pts = SE.lattice_points(origin, spacing, shape).reshape(-1, 3)
    return (SE.Grid(p, pos, vel, mass).sample(pts), P.sample(p, pos, vel, mass, pts),
            SC.sample(p, pos, vel, mass, values, pts))


def iso_inside(flavour):
    """(lattice points with members, of them those inside the flavour's iso)"""
    iso = probe_scene(flavour)[7]
    rho, _, count = lattice_answers(flavour)[0]
    return int((count > 0).sum()), int(((count > 0) & (rho > F32(iso))).sum())


ROUTES = (("default", {}), ("tiled", {"SPH_HIP_SAMPLE_TILED": "1"}), ("untiled", {"SPH_HIP_SAMPLE_UNTILED": "1"}),
          ("chunked", {"SPH_HIP_SAMPLE_CHUNK": "256"}), ("tiled_chunked", {"SPH_HIP_SAMPLE_TILED": "1", "SPH_HIP_SAMPLE_CHUNK": "256"}))


@pytest.mark.parametrize("route", [r[0] for r in ROUTES])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_lattice_samplers_equal_the_restatements(hiplib, policy, monkeypatch, flavour, route):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, pr, ev, values, iso = probe_scene(flavour)
    origin, spacing, shape = block_lattice(p)
    cells = [float(s) * float(F32(p.full_cell_inv)) for s in spacing]
    assert tiled(policy, shape, cells, TILED) == 1, "SPH_HIP_SAMPLE_TILED=1 must take the tiled route here"
    want_f, want_p, want_s = lattice_answers(flavour)
    with_members, inside = iso_inside(flavour)
    assert (want_f[2] == 0).any() and with_members > 1000
    if flavour == "SCALED":
        assert (with_members, inside) == CPU_SCALED_ISO_INSIDE and 0.1 * with_members <= inside <= 0.9 * with_members
    else:
        assert ((want_f[2] > 0) & (want_f[0] == 0)).any()       # counted, and dry
    for env in ("SPH_HIP_SAMPLE_TILED", "SPH_HIP_SAMPLE_UNTILED", "SPH_HIP_SAMPLE_CHUNK"):
        monkeypatch.delenv(env, raising=False)
    for k, v in dict(ROUTES)[route].items():
        monkeypatch.setenv(k, v)                               # (read when the context is created)
    nz, ny, nx = shape[2], shape[1], shape[0]
    with context(S, (p, pos, vel, mass)) as sph:
        sph.setScalars(values)
        f = sph.sampleLattice(origin, spacing, shape)
        f_nv = sph.sampleLattice(origin, spacing, shape, velocity=False)
        q = sph.samplePressureLattice(origin, spacing, shape)
        s = sph.sampleScalarLattice(origin, spacing, shape)
    assert f[0].shape == (nz, ny, nx) and f[1].shape == (nz, ny, nx, 3) and s[0].shape == (nz, ny, nx, 4)
    what = "%s %s " % (flavour, route)
    assert_same((f[0].reshape(-1), f[1].reshape(-1, 3), f[2].reshape(-1)), want_f, what + "fields")
    assert_same((f_nv[0].reshape(-1), f_nv[2].reshape(-1)), want_f[::2], what + "fields without velocity")
    assert f_nv[1] is None
    assert_same([a.reshape(-1) for a in q], want_p, what + "pressure")
    assert_same((s[0].reshape(-1, 4), s[1].reshape(-1), s[2].reshape(-1)), want_s, what + "scalars")


# ---- k_particle_density, and the gauges ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gauge_scene(flavour):
    """probe_scene with one gauge of each of the five kinds, and a PointGauge and a PressureGauge on a shell probe
    (under SHELL: a member, and a density of zero) and on a particle."""
    from smoothed_particle_hydrodynamics_amd.gauges import ColumnGauge, PointGauge, PressureGauge, PressurePatch, SectionGauge
    p, pos, vel, mass, pr, ev, values, iso = probe_scene(flavour)
    shell = tuple(float(c) for c in pr.shell[0])
    on = tuple(float(c) for c in pr.on[0])
    gauges = (PointGauge(shell), PressureGauge(shell), PointGauge(on), PressureGauge(on),
              ColumnGauge((0.65, 0.0, 0.65), 1, 0.05, 32, iso),                       # up through the layer and the block
              SectionGauge((0.65, 0.1, 0.1), 0, (1.4 / 15, 1.4 / 15), (16, 16), iso),  # across the box through the block
              PressurePatch((0.65, 0.3, 0.3), 0, (0.7 / 12, 0.7 / 12), (13, 13), iso))
    return p, pos, vel, mass, gauges


def check_gauge_conditions(flavour, first):
    """on the restatement's readings of the first state"""
    if flavour == "SHELL":
        # a member, no density: the Shepard velocity and the pressure quotient take their zero branch
        assert first.n[0] == 1 and not first.v[0].any() and first.n[1] == 1 and not first.v[1].any()
    assert first.n[2] >= 1 and first.v[2][0] > 0 and first.n[3] >= 1
    # the column is wet and not saturated, the section and the patch partly wet: the iso selects something, not all
    assert 0 < first.n[4] < 32 and 0 < first.n[5] < 256 and 0 < first.n[6] < 169


@pytest.mark.parametrize("mode", ["full", "fast"])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_particle_density_on_a_fresh_upload(hiplib, flavour, mode):
    """no step taken: the pressure sampler and readGauges form the particles' densities themselves"""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, gauges = gauge_scene(flavour)
    ev = probe_scene(flavour)[5]
    eg = [G.of(g) for g in gauges]
    want = P.evaluate(p, pos, vel, mass, eg)
    check_gauge_conditions(flavour, want)
    with context(S, (p, pos, vel, mass), mode) as sph:
        assert_same(sph.samplePressure(ev), probe_answers(flavour)[1], "%s pressure on a fresh upload" % flavour)
    with context(S, (p, pos, vel, mass), mode) as sph:
        sph.setGauges(gauges)
        assert G.same_readings(sph.readGauges(), want)


@pytest.mark.parametrize("mode", ["full", "fast"])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_every_gauge_row_equals_the_restatement(hiplib, flavour, mode):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, gauges = gauge_scene(flavour)
    eg = [G.of(g) for g in gauges]
    with context(S, (p, pos, vel, mass), mode) as sph:
        sph.setGauges(gauges)
        sph.recordGauges(GAUGE_STEPS)
        want = []
        gpos, gvel = particles(sph)
        for k in range(GAUGE_STEPS):
            sph.step()
            part = sph.getParticles()
            # the density this step's own pass formed for the state it started from serves the rows between; the
            # first and the last row use the restatement's (tests/test_gpu_pressure.py's rule)
            density = None if k in (0, GAUGE_STEPS - 1) else part.mDensity.copy()
            want.append(P.evaluate(p, gpos, gvel, mass, eg, density=density))
            if density is not None and mode == "full":
                assert same_bits(density, P.particle_density(p, gpos, gvel, mass))
            gpos, gvel = part.mPosition.copy(), part.mVelocity.copy()
        check_gauge_conditions(flavour, want[0])
        rec = sph.getGaugeRecord()
        assert rec.steps.tolist() == list(range(GAUGE_STEPS)) and rec.v.shape == (GAUGE_STEPS, len(gauges), 4)
        for r in range(GAUGE_STEPS):
            assert G.same_readings(G.Readings(rec.v[r], rec.n[r], rec.k[r]), want[r]), "row %d" % r
        assert G.same_readings(sph.readGauges(), P.evaluate(p, gpos, gvel, mass, eg))


# ---- carried scalars ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scalar_scene(flavour):
    """tests/test_gpu_scalars.py's block under the flavour: two diffusing channels (k, 2k), two carried ones, and a
    HOLD over the column's foot."""
    from smoothed_particle_hydrodynamics_amd import scenes
    from test_gpu_scalars import block_scene
    p, pos, vel, mass, values, _ = block_scene()
    scale_cases.apply(p, flavour)
    k = scenes.scalar_stable_kappa(p, 0.1)
    kappa = np.array([0.0, k, 2.0 * k, 0.0], F32)
    h = float(p.h)
    top = (float(p.max_x) + h, float(p.max_y) + h, float(p.max_z) + h)
    return p, pos, vel, mass, values, kappa, (SC.hold((-h, -h, -h), (top[0], 0.2, top[2]), 1, 2.5),)


def negative_weight_pairs(p, pos, vel, mass, rho):
    """ordered pairs (i, j) of the state whose weight V_j * (kernel3 * (hscaled - d)) is negative"""
    c = SC.consts_of(p)
    grid = SE.Grid(p, pos, vel, mass)
    order = P.canonical_order(p, pos)
    V = SC.volume(grid.mass, np.asarray(rho, F32)[order])
    probe, idx, d2 = P.members(grid, grid.pos, exclude_self=True)
    return int((SC.weight(c, V[idx], SC.distance(c, d2)) < 0).sum())


@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("mode", ["full", "fast"])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_scalar_steps_equal_the_restatement(hiplib, monkeypatch, flavour, mode, rows):
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_scalars import api_sources, bits, checked_steps, same
    p, pos, vel, mass, values, kappa, sources = scalar_scene(flavour)
    monkeypatch.delenv("SPH_HIP_SCALAR_ROWS", raising=False)
    if rows:
        monkeypatch.setenv("SPH_HIP_SCALAR_ROWS", "1")          # (read when the context is created)
    negative = negative_weight_pairs(p, pos, vel, mass, P.particle_density(p, pos, vel, mass))
    if flavour == "SHELL":
        assert negative == CPU_SHELL_NEGATIVE_PAIRS and negative >= mass.size / 100
    else:
        assert negative == 0
    with context(S, (p, pos, vel, mass), mode) as sph:
        sph.setScalars(values, kappa)
        sph.setScalarSources(api_sources(sources))
        out = checked_steps(sph, p, mass, values, kappa, list(sources), SCALAR_STEPS)
    assert same(out[:, 0], values[:, 0]) and same(out[:, 3], values[:, 3])         # carried: the bits kept
    assert (bits(out[:, 2]) != bits(values[:, 2])).mean() > 0.9                      # diffusing
    assert (out[:, 1] == F32(2.5)).any()                                             # held


# ---- tracers ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tracer_scene(flavour):
    """scale_cases.block_scene with the walls on, a tracer on every probe of the point samplers' set"""
    p, pos, vel, mass = scale_cases.block_scene(flavour, walls=True)
    return p, pos, vel, mass, scale_cases.every(scale_cases.probes(p, pos, vel, mass))


def wet_and_unmoved(info):
    return int((info.wet & ~info.moved).sum())


@pytest.mark.parametrize("mode", ["full", "fast"])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_every_tracer_step_equals_the_restatement(hiplib, flavour, mode):
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_tracers import got_state, same_state
    p, pos, vel, mass, tracers = tracer_scene(flavour)
    with context(S, (p, pos, vel, mass), mode) as sph:
        sph.setTracers(tracers)
        sph.recordTracers(TRACER_STEPS)
        want = T.initial(tracers)
        moved = np.zeros(len(tracers), bool)
        for k in range(TRACER_STEPS):
            gpos, gvel = particles(sph)
            want, info = T.advance(p, gpos, gvel, mass, want, p.time_step, with_info=True)
            moved |= info.moved
            if k == 0 and flavour == "SHELL":
                # members, a density of zero, a Shepard velocity of zero: wet, and in place
                assert wet_and_unmoved(info) == CPU_SHELL_TRACERS_WET_UNMOVED >= 32
            sph.step()
            assert same_state(got_state(sph), want), "step %d" % k
            assert same_bits(sph.getTracerPath().positions[k], want.x), "row %d" % k
        assert moved.sum() > 1000 and (want.dry == TRACER_STEPS).sum() > 64
        if flavour == "SCALED":
            # the restatement of the contract as it once read - the time step where the displacement step belongs:
            # sim_scale_inv = 1 in the move, the samples' arithmetic unchanged (sim_scale is still 0.5) - leaves
            # these bits in the first step already
            old = p.copy()
            old.sim_scale_inv = 1.0
            assert not SE.unit_scale(old)
            a = T.advance(p, pos, vel, mass, T.initial(tracers), p.time_step)
            b = T.advance(old, pos, vel, mass, T.initial(tracers), p.time_step)
            assert (a.x.view(np.uint32) != b.x.view(np.uint32)).any(1).sum() > 1000


@pytest.mark.parametrize("mode", ["full", "fast"])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_the_tracer_slot_order_never_shows(hiplib, monkeypatch, flavour, mode):
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_tracers import got_state, same_state
    p, pos, vel, mass, tracers = tracer_scene(flavour)
    out = []
    for switch in ("0", "1"):
        monkeypatch.setenv("SPH_HIP_TRACER_SORT", switch)       # (read when the context is created)
        with context(S, (p, pos, vel, mass), mode) as sph:
            sph.setTracers(tracers)
            sph.recordTracers(TRACER_STEPS)
            sph.run(TRACER_STEPS)
            path = sph.getTracerPath()
            out.append((got_state(sph), path.steps.copy(), path.positions.copy()))
    monkeypatch.delenv("SPH_HIP_TRACER_SORT")
    assert out[0][0].wet.sum() > 0 and out[0][1].tolist() == list(range(1, TRACER_STEPS + 1))
    assert same_state(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and same_bits(out[0][2], out[1][2])
    assert same_bits(out[0][2][-1], out[0][0].x)


@pytest.mark.parametrize("mode", ["full", "fast"])
def test_tracers_are_carried_off_unit_scale(oracle, hiplib, mode):
    """scale_cases.carried_scene: sim_scale_inv = 2, a fluid in uniform translation without forces.  After one step a
    tracer set on a particle lies on that particle's new position - the oracle's, not the device's - within
    scale_cases.carried_bound.  Advancing by u * dt, as the contract once read, misses that by |v0_c| * dt."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, rows = scale_cases.carried_scene()
    x0 = pos.reshape(-1, 3)[rows].copy()
    count = SE.Grid(p, pos, vel, mass).sample(x0, velocity=False)[2]
    opos, ovel = pos.copy(), vel.copy()
    out = oracle.step(to_oracle_params(p), opos, ovel, mass, mode="full")
    assert not out["acc"].any()
    after = opos.reshape(-1, 3)[rows]
    with context(S, (p, pos, vel, mass), mode) as sph:
        sph.setTracers(x0)
        sph.step()
        t = sph.getTracers()
    assert (t.wet_steps == 1).all()
    bound = scale_cases.carried_bound(p, count, np.concatenate([x0, after]))
    err = np.abs(t.position.astype(np.float64) - after.astype(np.float64))
    print("worst error over its bound: %.3g" % float((err / bound).max()))
    assert (err <= bound).all(), float((err / bound).max())
    # the bar sees the old arithmetic: |v0_c| * dt is thousands of times the bound
    assert (np.abs(np.array(scale_cases.V0)) * float(F32(p.time_step)) > 1000.0 * bound).all()


# ---- the surface extractor and the three renderers ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def column_scene(flavour):
    """scale_cases.dam_scene with seeded scalars and the flavour's iso (half the median density on every fortieth
    particle), and a box standing in the empty half of the tank"""
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    p, pos, vel, mass = scale_cases.dam_scene(flavour)
    iso = scale_cases.iso_of(p, pos, vel, mass, pos.reshape(-1, 3)[::40])
    values = np.random.default_rng(43).uniform(-1.0, 1.0, (mass.size, 4)).astype(F32)
    return p, pos, vel, mass, iso, values, [O.Box((0.45, 0.0, 0.3), (0.6, 0.5, 0.7))]


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_surface_equals_the_restatement(hiplib, flavour):
    import smoothed_particle_hydrodynamics_amd as S
    import surface_emulation as SU
    from test_gpu_surface import assert_mesh, emulated_lattice, padded_lattice
    p, pos, vel, mass, iso, values, solids = column_scene(flavour)
    x = pos.reshape(-1, 3)
    origin, spacing, shape = padded_lattice(p, x, per_h=0.6, pad_h=1.5)
    assert max(shape) <= 24
    rho, v = emulated_lattice(p, x, vel.reshape(-1, 3), mass, origin, spacing, shape)
    want = SU.extract(rho, origin, spacing, iso, velocity=v, normals=True)
    assert len(want.triangles) > 1000 and SU.is_closed_oriented(want.triangles) and SU.volume(want.vertices, want.triangles) > 0
    if flavour == "SHELL":
        pts = SE.lattice_points(origin, spacing, shape).reshape(-1, 3)
        count = SE.Grid(p, pos, vel, mass).sample(pts, velocity=False)[2]
        assert ((count > 0) & (rho.reshape(-1) == 0)).any()        # corners that are counted and dry
    with context(S, (p, pos, vel, mass)) as sph:
        got = sph.extractSurface(origin, spacing, shape, iso, normals=True, velocity=True)
    assert_mesh(got, want, flavour)


@pytest.mark.parametrize("noskip", [False, True], ids=["skip", "noskip"])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_renderers_equal_the_restatements(hiplib, monkeypatch, flavour, noskip):
    """render, render(solids=True) and renderScalars in both modes: every output, on every second row of a 64 x 48
    frame, with and without the empty-cell skip"""
    import render_emulation as RE
    import smoothed_particle_hydrodynamics_amd as S
    import tint_emulation as TE
    from smoothed_particle_hydrodynamics_amd import Camera
    from test_gpu_render import assert_frame
    from test_gpu_render import flat as flat_frame
    from test_gpu_scene_render import assert_scene, want_frame
    from test_gpu_scene_render import flat as flat_scene
    from test_gpu_tint import MODES, RANGES, Restated, assert_tint, seeded_table
    from test_gpu_tint import flat as flat_tint
    p, pos, vel, mass, iso, values, solids = column_scene(flavour)
    monkeypatch.delenv("SPH_HIP_RENDER_NOSKIP", raising=False)
    if noskip:
        monkeypatch.setenv("SPH_HIP_RENDER_NOSKIP", "1")        # (read when the context is created)
    W, H = 64, 48
    py, px = [a.reshape(-1) for a in np.meshgrid(np.arange(0, H, 2), np.arange(W), indexing="ij")]
    index = py * W + px
    x = pos.reshape(-1, 3).astype(np.float64)
    c = 0.5 * (x.min(0) + x.max(0))
    cam = Camera.look_at(c + np.array([1.1, 0.5, 1.3]), c + np.array([0.2, 0.0, 0.0]), (0, 1, 0), 40, W, H)
    with context(S, (p, pos, vel, mass)) as sph:
        sph.setScalars(values)
        sph.setObstacles(solids)
        R = Restated(sph, p, mass, solids)
        plain = sph.render(cam, W, H, iso, velocity=True)
        want = RE.render(R.fields[0], cam, sph.renderParams(iso), W, H, velocity_field=R.fields[1], pixels=(px, py))
        assert_frame(flat_frame(plain), want, flavour + " render", index=index)
        inside = int((want.first_inside >= 0).sum())
        assert 100 < inside < len(index) - 100, "the iso must select some of the frame, not none or all of it"
        scene = sph.render(cam, W, H, iso, velocity=True, solids=True)
        want = want_frame(sph, R.fields, iso, solids, cam, W, H, pixels=(px, py))
        assert_scene(flat_scene(scene), want, flavour + " render with solids", index=index)
        assert (want.solid_id == 0).sum() > 50 and (want.first_inside >= 0).sum() > 100
        # without the velocity output: the other instantiation of the shading pass, the same bytes
        for solid in (False, True):
            bare = sph.render(cam, W, H, iso, solids=solid)
            assert bare.velocity is None
            for name in ("rgba", "depth", "normal", "first_inside"):
                assert same_bits(getattr(bare, name), getattr(scene if solid else plain, name)), name
        table = seeded_table(256)
        for mode in (TE.SURFACE, TE.COLUMN):
            lo, hi = RANGES[mode]
            for flat_ in (False, True):
                got = sph.renderScalars(cam, W, H, iso, 1, (lo, hi), table, MODES[mode], flat_, solids=True, velocity=True)
                want = R.want("view", iso, cam, W, H, 1, mode, lo, hi, table, flat_, pixels=(px, py))
                assert_tint(flat_tint(got), want, "%s renderScalars %s flat=%s" % (flavour, MODES[mode], flat_), index=index)
            hit = want.first_inside >= 0
            assert hit.sum() > 100 and (want.scalar[hit] != 0).any()


# ---- hooked integrates ------------------------------------------------------------------------------------------------------
HOOK_STEPS = 3


def hooked_scene(flavour):
    """tests/test_gpu_paths.py's scene under the flavour: the walled block (walls and gravity on, damping 0.6) with a
    sphere, a box, a cylinder and a wedge in its way; the paths and motions of that file, and
    tests/test_gpu_moving_obstacles.py's motions"""
    from test_gpu_moving_obstacles import walled_motions
    from test_gpu_paths import path_scene
    p, pos, vel, mass, obst, paths, path_motions = path_scene()
    scale_cases.apply(p, flavour)
    return p, pos, vel, mass, obst, paths, path_motions, walled_motions() + [None]


def pinned_integrates(oracle, sph, p, mass, respond, record):
    """HOOK_STEPS steps by the phase calls, as the features' own files pin them: voxelize .. compute_acceleration on
    the device, download; the oracle's integrate on that state (without walls under a load recording, whose
    restatement handles them), then respond(k, P, V, Q) -> (V, Q, Row or None) must be what sph_hip_integrate wrote,
    bit for bit in FULL and FULL_FAST alike.  Returns (rows, particle-steps a solid or a wall changed)."""
    from test_gpu_obstacles import check_ke, state
    from test_gpu_wedges import phases
    op = to_oracle_params(p)
    if record:
        op.apply_walls = 0
    rows, changed = [], 0
    for k in range(HOOK_STEPS):
        phases(sph)
        part = sph.getParticles()
        P0, V0, A = part.mPosition.copy(), part.mVelocity.copy(), part.mAcceleration.copy()
        sph.integrate()
        got_pos, got_vel = state(sph)
        opos, ovel = P0.copy(), V0.copy()
        oracle.integrate(op, opos, ovel, A, mass)
        ev, eq, row = respond(k, P0, ovel, opos)
        assert_same((got_vel, got_pos), (ev.reshape(-1), eq.reshape(-1)), "step %d (velocity, position)" % k)
        check_ke(sph, got_vel, mass)
        rows.append(row)
        changed += int((np.asarray(eq, F32).reshape(-1, 3) != opos.reshape(-1, 3)).any(1).sum())
    return rows, changed


def check_rows(sph, rows):
    """a load recording against the restatement's rows, int64 for int64"""
    loads = sph.getLoads()
    assert loads.impulse_q.dtype == np.int64 and loads.impulse_q.shape[0] == HOOK_STEPS
    for r, row in enumerate(rows):
        assert row.same(loads.impulse_q[r], loads.count[r], loads.skipped[r]), "row %d" % r
    assert loads.count.sum() > 0 and not loads.skipped.any()


@pytest.mark.parametrize("record", [False, True], ids=["plain", "loads"])
@pytest.mark.parametrize("route", ["static", "motion", "path"])
@pytest.mark.parametrize("mode", ["full", "fast"])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_hooked_integrates_equal_the_oracle_and_the_restatement(oracle, hiplib, flavour, mode, route, record):
    """k_integrate_obst, _obst_moving and _obst_path, and under a load recording k_integrate_loads, _loads_moving
    and _loads_path: the four kinds of static obstacle (a wedge among them), Motions, MotionPaths"""
    import load_emulation as L
    import moving_obstacle_emulation as M
    import path_emulation as PE
    import smoothed_particle_hydrodynamics_amd as S
    import wedge_emulation as W
    p, pos, vel, mass, obst, paths, path_motions, motions = hooked_scene(flavour)
    dt, damping = F32(p.time_step), F32(p.damping)
    maxv = F32([p.max_x, p.max_y, p.max_z])
    clock = M.clock(dt, HOOK_STEPS)
    walls = int(p.apply_walls)

    def respond(k, P0, V, Q):
        t0, t1 = clock[k], clock[k + 1]
        if route == "path":
            if record:
                return PE.integrate_respond(maxv, walls, obst, paths, path_motions, P0, V, Q, dt, damping, t0, t1, mass)
            return PE.respond(obst, paths, path_motions, P0, V, Q, dt, damping, t0, t1) + (None,)
        m = motions if route == "motion" else None
        if record:
            return W.integrate_respond(maxv, walls, obst, m, None, None, P0, V, Q, dt, damping, t0, t1, mass)
        return W.respond(obst, m, None, None, P0, V, Q, dt, damping, t0, t1) + (None,)

    def start(sph):
        sph.setObstacles(obst)
        if route == "motion":
            sph.setObstacleMotion(motions)
        elif route == "path":
            sph.setObstacleMotion(path_motions)
            sph.setObstaclePaths(paths)
        if record:
            sph.recordLoads(HOOK_STEPS, L.QUANTUM_LOG2)

    with context(S, (p, pos, vel, mass), mode) as sph:
        start(sph)
        rows, changed = pinned_integrates(oracle, sph, p, mass, respond, record)
        if record:
            check_rows(sph, rows)
        phased = particles(sph)
    print("%s %s %s: %d particle-steps changed by a wall or a solid" % (flavour, mode, route, changed))
    assert changed > 50, "the scene is meant to run into the walls and the solids"
    if mode == "full":
        # the queued steps give the phase calls' bits
        with context(S, (p, pos, vel, mass), mode) as sph:
            start(sph)
            sph.run(HOOK_STEPS)
            assert_same(particles(sph), phased, "run against the phase calls")
            if record:
                check_rows(sph, rows)


@pytest.mark.parametrize("mode", ["full", "fast"])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_a_free_body_off_unit_scale(oracle, hiplib, flavour, mode):
    """k_integrate_bodies: tests/test_gpu_bodies.py's pin - particles, kinetic energy, body state and the obstacles as
    they stand, every step - under the flavour"""
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_bodies import pinned_steps, walled_bodies
    from test_gpu_obstacles import walled_scene
    p, pos, vel, mass, obst = walled_scene()
    scale_cases.apply(p, flavour)
    bodies, motions = walled_bodies()
    with context(S, (p, pos, vel, mass), mode) as sph:
        sph.setObstacles(obst)
        sph.setObstacleMotion(motions)
        sph.setBodies(bodies)
        st, rows, by_body, kicks = pinned_steps(oracle, sph, p, obst, motions, bodies, mass, HOOK_STEPS)
    assert st.steps.tolist() == [0, HOOK_STEPS, 0] and not st.skipped.any() and (st.D[1] != 0).any()
    assert sum(int(r.count.sum()) for r in rows) > 50


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_buoyancy_off_unit_scale(oracle, hiplib, flavour):
    """the buoyant context's own integrate: FULL against the oracle stepped by tests/buoyancy_emulation.py bit for bit,
    FULL_FAST against FULL from the same state with the bars of tests/test_gpu_full_fast.py"""
    import buoyancy_emulation as BE
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_buoyancy import against_step, block_buoyancy, emu_of, start, state_of
    from test_gpu_full_fast import check_fast, check_fast_position, check_fast_velocity
    from test_gpu_scalars import block_scene, block_sources, same
    p, pos, vel, mass, values, kappa = block_scene()
    scale_cases.apply(p, flavour)
    sources = block_sources(p)
    buoyancy = block_buoyancy()
    b = emu_of(buoyancy, p)
    n = mass.size
    for k in range(HOOK_STEPS):
        out = BE.step(oracle, p, pos, vel, mass, values, kappa, sources, b)
        assert out["touched"].sum() > n - 20
        got = {}
        for mode in ("full", "fast"):
            with S.SPH(n, p, mode=mode_of(S, mode)) as sph:
                start(sph, pos, vel, mass, values, kappa, sources, buoyancy)
                sph.step()
                got[mode] = (sph.getParticles(), state_of(sph), sph.getScalars())
        assert against_step(got["full"][1], got["full"][2], out) == [], "step %d" % k
        full, fast = got["full"][0], got["fast"][0]
        ref = {"ncount": full.mNeighborCount, "rho": full.mDensity, "acc": full.mAcceleration}
        worst, allowed = check_fast(fast, ref, p, mass, "state %d" % k)
        check_fast_velocity(fast.mVelocity, full.mVelocity, allowed, p.time_step, "state %d" % k)
        check_fast_position(fast.mPosition, full.mPosition, p, "state %d" % k)
        assert same(got["full"][2], got["fast"][2])
        pos, vel, values = full.mPosition.copy(), full.mVelocity.copy(), got["full"][2]


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_ports_off_unit_scale(oracle, hiplib, flavour):
    """a port context's integrate, one emitter and one sink: FULL against the oracle stepped by
    tests/port_emulation.py bit for bit; FULL_FAST, as tests/test_gpu_ports.py holds it, against the existing route
    fed the restatement's edits"""
    import ctypes as C

    import port_emulation as PO
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_ports import block_scene, check_totals, error_word, live_state, same_state, snapshot
    p, pos, vel, mass, emitters, sinks = block_scene()
    scale_cases.apply(p, flavour)
    run = PO.PortRun(to_oracle_params(p), pos, vel, mass, emitters, sinks)
    for _ in range(HOOK_STEPS):
        assert run.step(oracle)
    want = snapshot(run)
    assert sum(m for _, _, m in want["history"]) > 0 and sum(r for _, r, _ in want["history"]) > 0, want["history"]
    with S.SPH(mass.size, p, mode=S.MODE_FULL, capacity=6000) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setPorts(emitters, sinks)
        sph.run(HOOK_STEPS)
        same_state(live_state(sph), want, "%s after run(%d)" % (flavour, HOOK_STEPS))
        check_totals(sph, want)
        assert error_word(sph) == 0
    edits = PO.PortRun(to_oracle_params(p), pos, vel, mass, emitters, sinks)
    with S.SPH(mass.size, p, mode=S.MODE_FULL_FAST, capacity=6000) as sph, \
            S.SPH(mass.size, p, mode=S.MODE_FULL_FAST, capacity=6000) as plain:
        sph.setParticles(pos, vel, mass)
        sph.setPorts(emitters, sinks)
        for step in range(HOOK_STEPS):
            now = live_state(sph)
            assert np.array_equal(now["ids"], edits.ids)
            edits.pos, edits.vel = now["pos"].copy(), now["vel"].copy()
            assert edits.apply_ports()
            plain.call("sph_hip_slab_upload", edits.live, np.ascontiguousarray(edits.pos).ctypes.data_as(C.c_void_p),
                       np.ascontiguousarray(edits.vel).ctypes.data_as(C.c_void_p),
                       np.ascontiguousarray(edits.mass).ctypes.data_as(C.c_void_p),
                       np.ascontiguousarray(edits.ids).ctypes.data_as(C.c_void_p), 1)
            plain.step()
            sph.step()
            same_state(live_state(sph), live_state(plain), "%s fast step %d" % (flavour, step))
        t, _, _ = sph.getPorts()
        assert t.emitted.tolist() == edits.emitted.tolist() and t.removed.tolist() == edits.removed.tolist()
        assert t.live == edits.live and error_word(sph) == 0


# ---- the figures ---------------------------------------------------------------------------------------------------------
def cpu_figures():
    """The CPU_* constants again, from the restatements alone (the first state of every scene: no step is needed)."""
    p, pos, vel, mass, tracers = tracer_scene("SHELL")
    _, info = T.advance(p, pos, vel, mass, T.initial(tracers), p.time_step, with_info=True)
    sp, spos, svel, smass = scalar_scene("SHELL")[:4]
    return {"CPU_SHELL_ZERO_DENSITY_PROBES": zero_density_probes("SHELL"),
            "CPU_SHELL_ON_WITH_ZERO_TERM": on_probes_with_a_zero_term("SHELL"),
            "CPU_SHELL_TRACERS_WET_UNMOVED": wet_and_unmoved(info),
            "CPU_SHELL_NEGATIVE_PAIRS": negative_weight_pairs(sp, spos, svel, smass, P.particle_density(sp, spos, svel, smass)),
            "CPU_SCALED_ISO_INSIDE": iso_inside("SCALED"),
            "CPU_SCALED_ZERO_DENSITY_PROBES": zero_density_probes("SCALED")}


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for name, value in cpu_figures().items():
        print("%s = %r" % (name, value))
