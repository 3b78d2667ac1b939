"""GPU: the feature passes on unequal particle masses.  The core step is held to the oracle with unequal masses; every
GPU test of the features built since uploads np.ones(n), behind the UNIFORM_MASS instantiations of the density and
acceleration passes (csrc/launch.h: uniform_mass), and with pj.w == pi.w == 1.0f a feature kernel that took the wrong
mass would give the same bits.  Here the composed step (scalars, buoyancy, cohesion, XSPH, a monitor), its routes, the
velocity gradients, the samplers, k_particle_density, the gauges, the tracers, the surface extractor, the renderers,
every hooked integrate with its load recording, a free body and the ports run under the flavours of
tests/mass_cases.py - SPREAD, TWO_SPECIES and, where said, ODD_ONE - and are held to the numpy restatements bit for
bit, exactly as each feature's own file holds them with unit masses: a case that only repeats an existing test with
other masses calls that test with its scene replaced (unequal()), so the assertions are the same ones.

That the inputs are not vacuous - that a kernel which took the probing particle's mass, or none, would give other
bits in nearly every row - is computed by the restatements alone: the figures CPU_* below, which
`python tests/test_gpu_unequal_masses.py` prints again and tests/test_unequal_masses_cpu.py checks (DESIGN.md
section 35)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cohesion_emulation as CE
import mass_cases
import monitor_emulation as ME
import pressure_emulation as P
import sample_emulation as SE
import scalar_emulation as SC
import scale_cases
import velgrad_emulation as VE
import xsph_emulation as XE
from helpers import to_oracle_params

pytestmark = pytest.mark.gpu

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FLAVOURS = mass_cases.FLAVOURS
N = 2001
EPS = 0.5            # tests/test_gpu_xsph.py's
GAMMA = 0.02         # tests/test_gpu_cohesion.py's
Q = -24              # tests/test_gpu_monitor.py's quantum
STEPS = 3            # the most any case here takes

# cpu_figures(): rows of the 2 001-particle block, of 2 001 with a member, in which the restatement differs from its
# own_mass variant / from the unit-mass run (the bar: >= 90 % of the rows with a member, each)
CPU_ROWS_WITH_A_MEMBER = 2001
CPU_SPREAD = {"cohesion": (2001, 2001), "xsph": (2001, 2001), "scalars": (2001, 2001), "velgrad": (2001, 2001),
              "pressure": (2001, 2001), "density": (2001, 2001)}
CPU_TWO_SPECIES = {"cohesion": (2001, 2000), "xsph": (2001, 2001), "scalars": (2001, 2001), "velgrad": (1999, 1999),
                   "pressure": (2001, 2001), "density": (2001, 2001)}
CPU_ODD_ONE = (767, 1869, 42)       # the odd particle, particles farther than 2h from it (>= 1 000), inside its support (>= 30)
CPU_XSPH_SPREAD_G = 0.6845          # eps * max_i sum_j g_ij under SPREAD (<= 1), to four places


def same(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def mode_of(S, name):
    return {"full": S.MODE_FULL, "fast": S.MODE_FULL_FAST}[name]


# ---- an existing test, with the masses replaced ----------------------------------------------------------------------
@pytest.fixture
def unequal(monkeypatch):
    """unequal(flavour): from here to the end of the test the scenes the existing GPU tests build carry the flavour's
    masses - positions, velocities, parameters and everything else as they are - and scale_cases.apply leaves the
    parameters at unit scale.  The existing test functions called behind it assert what they always assert."""
    def install(flavour, emitter_mass=None):
        import test_gpu_obstacles
        import test_gpu_off_unit_scale as OU
        import test_gpu_paths
        import test_gpu_scalars
        import test_gpu_velgrad

        def remassed(build, at=3):
            def scene(*args, **kwargs):
                out = list(build(*args, **kwargs))
                out[at] = mass_cases.masses(flavour, out[0], out[1])
                return tuple(out)
            return scene

        assert flavour in FLAVOURS + ("ODD_ONE",)
        monkeypatch.setattr(scale_cases, "apply", lambda p, _flavour: p)
        monkeypatch.setattr(scale_cases, "block_scene", lambda _f, params_for_h=None, walls=False: mass_cases.probe_block(flavour, walls))
        monkeypatch.setattr(scale_cases, "dam_scene", lambda _f: mass_cases.dam(flavour))
        monkeypatch.setattr(scale_cases, "carried_scene", remassed(scale_cases.carried_scene))
        monkeypatch.setattr(test_gpu_scalars, "block_scene", remassed(test_gpu_scalars.block_scene))
        monkeypatch.setattr(test_gpu_velgrad, "block_scene", remassed(test_gpu_velgrad.block_scene))
        monkeypatch.setattr(test_gpu_paths, "path_scene", remassed(test_gpu_paths.path_scene))
        monkeypatch.setattr(test_gpu_obstacles, "walled_scene", remassed(test_gpu_obstacles.walled_scene))
        for name in ("GAUGE_STEPS", "SCALAR_STEPS", "TRACER_STEPS"):
            monkeypatch.setattr(OU, name, STEPS)
        return OU
    return install


# ---- 1. the composed step ---------------------------------------------------------------------------------------------
def start_all(sph, scene, sources, buoyancy, monitor_rows=0):
    """the block with scalars (four channels, the block's sources), buoyancy, cohesion, XSPH and a monitor recording"""
    from test_gpu_scalars import api_sources
    p, pos, vel, mass, T, kappa = scene
    sph.setParticles(pos, vel, mass)
    sph.setScalars(T, kappa)
    sph.setScalarSources(api_sources(sources))
    sph.setBuoyancy(buoyancy)
    sph.setCohesion(GAMMA)
    sph.setVelocitySmoothing(EPS)
    if monitor_rows:
        sph.recordMonitor(monitor_rows)


def composed(oracle, p, pos, vel, mass, T, kappa, sources, b):
    """xsph_emulation.step of the composed context, with the neighbour counts the monitor's row needs"""
    out = XE.step(oracle, p, pos, vel, mass, EPS, GAMMA, T, kappa, sources, b)
    op = to_oracle_params(p)
    _, cs, ci = oracle.full_cells(op, np.ascontiguousarray(pos, F32))
    out["ncount"] = oracle.full_density(op, np.ascontiguousarray(pos, F32), mass, cs, ci)[1]
    return out


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_the_composed_step_equals_the_restatements(oracle, hiplib, flavour):
    """FULL, two single steps: positions, velocities, accelerations, densities and scalars against
    xsph_emulation.step, the monitor's rows against monitor_emulation.step_row, bit for bit."""
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_buoyancy import against_step, block_buoyancy, emu_of, state_of
    from test_gpu_monitor import differing
    from test_gpu_scalars import block_sources
    p, pos, vel, mass, T, kappa = mass_cases.block(flavour)
    sources, buoyancy = block_sources(p), block_buoyancy()
    b = emu_of(buoyancy, p)
    want = []
    with S.SPH(N, p) as sph:
        start_all(sph, (p, pos, vel, mass, T, kappa), sources, buoyancy, monitor_rows=2)
        for k in range(2):
            out = composed(oracle, p, pos, vel, mass, T, kappa, sources, b)
            want.append(ME.step_row(p, (pos, vel, mass), out, Q, out["T"]))
            sph.step()
            got, T_got = state_of(sph), sph.getScalars()
            assert against_step(got, T_got, out) == [], "step %d" % k
            assert np.array_equal(got["mNeighborCount"], out["ncount"])
            assert out["touched"].sum() > N - 20                                   # the smoothing touched nearly all
            assert mass_cases.rows_differing(out["acc"].reshape(-1, 3), out["acc_before"].reshape(-1, 3)).sum() > N - 50
            pos, vel, T = got["mPosition"], got["mVelocity"], T_got
        rec = sph.getMonitorRecord()
        stats = sph.tileStats()
        assert stats["workgroups"] == 8 and stats["untiled_density"] == 0          # the list route
    assert len(rec) == 2 and rec.quantum_log2 == Q
    for k in range(2):
        assert differing(rec.rows[k], want[k]) == [], "monitor row %d" % k
    assert (rec.flags == 3).all() and (rec.live == N).all() and (rec.bad == 0).all() and (rec.skipped == 0).all()
    total = float(mass.astype(np.float64).sum())
    assert total != float(N)
    assert np.allclose(rec.mass, total, rtol=1e-6)                               # (tests/test_gpu_monitor.py's bar)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_the_composed_step_in_fast_against_full(hiplib, flavour):
    """FULL_FAST from the same two states as FULL: neighbour counts and densities the same bits, forces, velocities and
    positions within the existing bars (tests/test_gpu_full_fast.py), the scalars the same bits, and the monitor's row
    the restatement's of the context's own state - as buoyancy's, cohesion's and the monitor's own FAST tests do it."""
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_buoyancy import block_buoyancy
    from test_gpu_full_fast import check_fast, check_fast_position, check_fast_velocity
    from test_gpu_monitor import differing, own_row
    from test_gpu_scalars import block_sources
    p, pos, vel, mass, T, kappa = mass_cases.block(flavour)
    sources, buoyancy = block_sources(p), block_buoyancy()
    for k in range(2):
        got = {}
        for mode in ("full", "fast"):
            with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
                start_all(sph, (p, pos, vel, mass, T, kappa), sources, buoyancy, monitor_rows=1)
                sph.step()
                part = sph.getParticles()
                row = sph.getMonitorRecord().rows[0]
                assert differing(row, own_row(sph, p, (pos, vel), mass)) == [], (mode, k)
                got[mode] = (part, sph.getScalars(), row)
        full, fast = got["full"][0], got["fast"][0]
        ref = {"ncount": full.mNeighborCount, "rho": full.mDensity, "acc": full.mAcceleration}
        worst, allowed = check_fast(fast, ref, p, mass, "%s state %d" % (flavour, k))
        check_fast_velocity(fast.mVelocity, full.mVelocity, allowed, p.time_step, "%s state %d" % (flavour, k))
        check_fast_position(fast.mPosition, full.mPosition, p, "%s state %d" % (flavour, k))
        assert same(got["full"][1], got["fast"][1])
        for nm in ("s_max", "pair_bad", "rho_max", "rho_min", "ncount_max", "lone", "mass", "live"):
            assert got["full"][2][nm].tobytes() == got["fast"][2][nm].tobytes(), nm
        pos, vel, T = full.mPosition.copy(), full.mVelocity.copy(), got["full"][1]


# ---- 2. routes: one child process per setting -------------------------------------------------------------------------------
ROUTES = {
    "untiled": {"SPH_HIP_UNTILED": "1"},
    "lists_none": {"SPH_HIP_TILE_CAP": "256"},     # no tile of this scene fits: every workgroup is LISTS_NONE
    "lists_some": {"SPH_HIP_LIST_CAP": "16"},      # most particles have more than 16 neighbours: NLIST_NO_LIST lanes
    "wide": {"SPH_HIP_TILE_CAP": "4096"},          # above 4064: 14-bit tile indices in the entries
    "scalar_rows": {"SPH_HIP_SCALAR_ROWS": "1"},   # the scalar pass and the monitor's pair pass walk the cell rows
}
STATE = ("mPosition", "mVelocity", "mAcceleration", "mDensity")


def route_run(route="default"):
    """FULL and FULL_FAST: the composed context under SPREAD after one and after two steps, its scalars, its monitor
    rows, the neighbour counts and the tile statistics"""
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_buoyancy import block_buoyancy
    from test_gpu_scalars import block_sources
    scene = mass_cases.block("SPREAD")
    sources, buoyancy = block_sources(scene[0]), block_buoyancy()
    result, stats = {}, {}
    for mode in ("full", "fast"):
        with S.SPH(N, scene[0], mode=mode_of(S, mode)) as sph:
            start_all(sph, scene, sources, buoyancy, monitor_rows=2)
            for tag in ("1", "2"):
                sph.step()
                part = sph.getParticles()
                for nm in STATE:
                    result[mode + tag + nm] = getattr(part, nm).copy()
                result[mode + tag + "T"] = sph.getScalars()
            result[mode + "_counts"] = part.mNeighborCount.copy()
            result[mode + "_monitor"] = np.frombuffer(sph.getMonitorRecord().rows.tobytes(), np.uint8)
            stats[mode] = sph.tileStats() if route != "untiled" else {}
    result["stats"] = json.dumps(stats)
    return result


@pytest.fixture(scope="module")
def default_route(hiplib):
    return route_run()


@pytest.mark.parametrize("route", list(ROUTES))
def test_every_route_gives_the_default_routes_bytes(default_route, route, tmp_path):
    """(the default route is itself held to the restatements by the two tests above: the same context, the same steps)"""
    from test_gpu_cohesion import ROUTE_SWITCHES
    env = {k: v for k, v in os.environ.items() if k not in ROUTE_SWITCHES}
    env.update(ROUTES[route])
    out_path = str(tmp_path / "route.npz")
    run = subprocess.run([sys.executable, os.path.abspath(__file__), route, out_path], env=env, capture_output=True,
                         text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    got = np.load(out_path)
    assert sorted(got.files) == sorted(default_route)
    for name in default_route:
        if name != "stats":
            assert got[name].tobytes() == np.ascontiguousarray(default_route[name]).tobytes(), (route, name)
    # the setting produced the route it is there for, or the case proves nothing
    stats = json.loads(str(got["stats"]))
    base = json.loads(default_route["stats"])
    for mode in ("full", "fast"):
        st, counts = stats[mode], got[mode + "_counts"]
        assert base[mode]["workgroups"] == 8 and base[mode]["untiled_density"] == 0 and base[mode]["wide_entries"] == 0
        if route == "scalar_rows":
            assert st["workgroups"] == 8 and st["untiled_density"] == 0 and st["wide_entries"] == 0
        elif route == "lists_none":
            assert st["capacity_density"] == 256 and st["largest_tile"] > 256 and st["workgroups"] == 8
            assert st["untiled_density"] >= 7
        elif route == "lists_some":
            assert st["list_capacity"] == 16 and st["untiled_density"] == 0
            assert (counts > 16).sum() > 100 and (counts <= 16).sum() > 100
        elif route == "wide":
            assert st["wide_entries"] == 1 and st["capacity_density"] == 4096 and st["untiled_density"] == 0
        else:
            assert route == "untiled" and st == {}       # (an untiled context keeps no tile statistics)


# ---- 3. ODD_ONE against an all-unit twin --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["full", "fast"])
def test_one_heavy_particle_changes_its_support_and_nothing_far_from_it(oracle, hiplib, mode):
    """One step of the composed context from the same state with all masses 1 (the twin: UNIFORM_MASS = true) and with
    the particle that has the most neighbours at 2.0f (the general instantiations).  A particle farther than 2h from
    the odd one has no member whose density changed: it keeps the twin's bits in density, acceleration, velocity,
    position and scalars.  A particle inside the odd one's support has another density wherever the doubled term is
    not below an ulp of its sum (40 of the 42: DESIGN.md section 35).  In FULL both states equal the restatement."""
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_buoyancy import against_step, block_buoyancy, emu_of, state_of
    from test_gpu_scalars import block_sources
    scene = mass_cases.block("ODD_ONE")
    p, pos, vel, mass, T, kappa = scene
    odd = mass_cases.odd_particle(p, pos)
    assert mass[odd] == mass_cases.ODD_MASS and (np.delete(mass, odd) == 1).all()
    x = pos.reshape(-1, 3)
    d = x - x[odd]
    d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    far = np.sqrt(d2.astype(np.float64)) > 2.0 * float(F32(p.h))
    inside = d2 < F32(p.h2)
    inside[odd] = False
    assert (odd, int(far.sum()), int(inside.sum())) == CPU_ODD_ONE and far.sum() >= 1000 and inside.sum() >= 30
    sources, buoyancy = block_sources(p), block_buoyancy()
    got = {}
    for name, m in (("twin", np.ones(N, F32)), ("odd", mass)):
        with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
            start_all(sph, (p, pos, vel, m, T, kappa), sources, buoyancy)
            sph.step()
            got[name] = (state_of(sph), sph.getScalars())
    (twin, T_twin), (heavy, T_heavy) = got["twin"], got["odd"]
    for nm in STATE:
        rows = 3 if nm != "mDensity" else 1
        a, c = heavy[nm].reshape(-1, rows), twin[nm].reshape(-1, rows)
        assert not mass_cases.rows_differing(a[far], c[far]).any(), nm
    assert not mass_cases.rows_differing(T_heavy[far], T_twin[far]).any()
    # inside the support the odd particle's term is doubled: the density differs wherever that term is at least one
    # ulp of the sum (2^-23 of it) - at the support's rim, where (hscaled2 - d2)^3 vanishes, the sum may absorb it
    term = SE.density_terms(p, d2[inside], np.ones(int(inside.sum()), F32))
    seen_by = term >= F32(2.0 ** -23) * twin["mDensity"][inside]
    assert seen_by.sum() >= 30 and seen_by.sum() >= inside.sum() - 2
    assert mass_cases.rows_differing(heavy["mDensity"][inside], twin["mDensity"][inside])[seen_by].all()
    assert np.array_equal(heavy["mNeighborCount"], twin["mNeighborCount"])
    if mode == "full":
        for m, (state, T_got) in ((np.ones(N, F32), got["twin"]), (mass, got["odd"])):
            out = XE.step(oracle, p, pos, vel, m, EPS, GAMMA, T, kappa, sources, emu_of(buoyancy, p))
            assert against_step(state, T_got, out) == []


# ---- 4. the velocity gradients' entry points -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["full", "fast"])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_velocity_gradients_on_particles(hiplib, unequal, flavour, mode):
    import test_gpu_velgrad as VG
    unequal(flavour)
    assert not mass_cases.uniform(VG.block()[3])
    VG.test_particles_equal_the_restatement(hiplib, mode)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_velocity_gradients_at_points_on_a_lattice_and_rendered(hiplib, unequal, flavour):
    import smoothed_particle_hydrodynamics_amd as S
    import test_gpu_velgrad as VG
    unequal(flavour)
    sph, p, pos0, mass = VG.stepped_block(S)
    assert not mass_cases.uniform(mass)
    with sph:
        pos, vel, want = VG.restated(p, sph, mass)
        seen = VG.observe(sph, p, pos0)
    VG.test_samplers_equal_the_shepard_restatement((p, pos0, mass, pos, vel, want, seen))
    VG.test_frames_equal_the_tint_restatement(hiplib, False)


# ---- 5. the samplers, the pressure and the gauges ---------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_point_samplers_equal_the_restatements(hiplib, unequal, flavour):
    """the field, pressure and scalar samplers at scale_cases.probes' families - on particles, jittered, empty, on the
    faces, outside - in both modes"""
    import smoothed_particle_hydrodynamics_amd as S
    OU = unequal(flavour)
    p, pos, vel, mass, pr, ev, values, iso = OU.probe_scene(flavour)
    assert not mass_cases.uniform(mass) and len(ev) > 1200
    want_f, want_p, want_s = OU.probe_answers(flavour)
    rho, _, count = want_f
    on, empty = scale_cases.span(pr, "on"), scale_cases.span(pr, "empty")
    assert (count[on] >= 1).all() and (rho[on] > 0).all() and not count[empty].any() and not rho[empty].any()
    for mode in ("full", "fast"):
        with OU.context(S, (p, pos, vel, mass), mode) as sph:
            sph.setScalars(values)
            OU.assert_same(sph.sampleFields(ev), want_f, "%s %s fields" % (flavour, mode))
            OU.assert_same(sph.sampleFields(ev, velocity=False)[::2], want_f[::2], "%s %s fields without velocity" % (flavour, mode))
            OU.assert_same(sph.samplePressure(ev), want_p, "%s %s pressure" % (flavour, mode))
            OU.assert_same(sph.sampleScalars(ev), want_s, "%s %s scalars" % (flavour, mode))


@pytest.mark.parametrize("route", ["default", "tiled", "untiled"])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_lattice_samplers_equal_the_restatements(hiplib, unequal, monkeypatch, flavour, route):
    """a 21 x 19 x 23 lattice over a corner of the compressed block: the tile copy of the masses (tm[..] = pj.w) on the
    tiled route, the global walk on the untiled one"""
    import smoothed_particle_hydrodynamics_amd as S
    OU = unequal(flavour)
    p, pos, vel, mass, pr, ev, values, iso = OU.probe_scene(flavour)
    origin, spacing, shape = OU.block_lattice(p)
    want_f, want_p, want_s = OU.lattice_answers(flavour)
    assert (want_f[2] == 0).any() and (want_f[2] > 0).sum() > 1000
    for env in ("SPH_HIP_SAMPLE_TILED", "SPH_HIP_SAMPLE_UNTILED", "SPH_HIP_SAMPLE_CHUNK"):
        monkeypatch.delenv(env, raising=False)
    for k, v in dict(OU.ROUTES)[route].items():
        monkeypatch.setenv(k, v)                               # (read when the context is created)
    with OU.context(S, (p, pos, vel, mass)) as sph:
        sph.setScalars(values)
        f = sph.sampleLattice(origin, spacing, shape)
        q = sph.samplePressureLattice(origin, spacing, shape)
        s = sph.sampleScalarLattice(origin, spacing, shape)
    what = "%s %s " % (flavour, route)
    OU.assert_same((f[0].reshape(-1), f[1].reshape(-1, 3), f[2].reshape(-1)), want_f, what + "fields")
    OU.assert_same([a.reshape(-1) for a in q], want_p, what + "pressure")
    OU.assert_same((s[0].reshape(-1, 4), s[1].reshape(-1), s[2].reshape(-1)), want_s, what + "scalars")


@pytest.mark.parametrize("mode", ["full", "fast"])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_particle_density_on_a_fresh_upload_and_every_gauge_row(hiplib, unequal, flavour, mode):
    """k_particle_density before any step, then the five kinds of gauge and the two pressure gauges, every recorded row"""
    OU = unequal(flavour)
    assert not mass_cases.uniform(OU.gauge_scene(flavour)[3])
    OU.test_particle_density_on_a_fresh_upload(hiplib, flavour, mode)
    OU.test_every_gauge_row_equals_the_restatement(hiplib, flavour, mode)


# ---- 6. tracers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["full", "fast"])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_every_tracer_step_equals_the_restatement(hiplib, unequal, flavour, mode):
    OU = unequal(flavour)
    assert not mass_cases.uniform(OU.tracer_scene(flavour)[3])
    OU.test_every_tracer_step_equals_the_restatement(hiplib, flavour, mode)


@pytest.mark.parametrize("mode", ["full", "fast"])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_tracers_are_carried_whatever_the_masses(oracle, hiplib, unequal, flavour, mode):
    """stiffness = viscosity = 0, no gravity, no walls, every particle at V0: the Shepard quotient of equal velocities
    does not depend on the weights, so a tracer set on a particle stays on it within scale_cases.carried_bound, at
    unit scale (pos_dt = dt)."""
    OU = unequal(flavour)
    p, _, _, mass, _ = scale_cases.carried_scene()
    assert SE.unit_scale(p) and not mass_cases.uniform(mass)
    OU.test_tracers_are_carried_off_unit_scale(oracle, hiplib, mode)


# ---- 7. the surface extractor and the three renderers --------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_surface_equals_the_restatement(hiplib, unequal, flavour):
    OU = unequal(flavour)
    assert not mass_cases.uniform(OU.column_scene(flavour)[3])
    OU.test_surface_equals_the_restatement(hiplib, flavour)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_renderers_equal_the_restatements(hiplib, unequal, monkeypatch, flavour):
    OU = unequal(flavour)
    OU.test_renderers_equal_the_restatements(hiplib, monkeypatch, flavour, False)


# ---- 8. hooked integrates and loads ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("record", [False, True], ids=["plain", "loads"])
@pytest.mark.parametrize("route", ["static", "motion", "path"])
@pytest.mark.parametrize("mode", ["full", "fast"])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_hooked_integrates_equal_the_oracle_and_the_restatement(oracle, hiplib, unequal, flavour, mode, route, record):
    """the static (a wedge among the four obstacles), motion and path routes, each with and without a load recording,
    whose rows are m * (v_before - v_after) in quanta, int64 for int64"""
    OU = unequal(flavour)
    assert not mass_cases.uniform(OU.hooked_scene(flavour)[3])
    OU.test_hooked_integrates_equal_the_oracle_and_the_restatement(oracle, hiplib, flavour, mode, route, record)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_a_free_body_is_hit_by_the_particles_own_masses(oracle, hiplib, unequal, flavour):
    """tests/test_gpu_bodies.py's pin over three steps, and the body's velocity is not the unit-mass run's"""
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_bodies import pinned_steps, walled_bodies
    OU = unequal(flavour)
    from test_gpu_obstacles import walled_scene                  # (the scene as unequal() left it)
    OU.test_a_free_body_off_unit_scale(oracle, hiplib, flavour, "fast")
    p, pos, vel, mass, obst = walled_scene()
    assert not mass_cases.uniform(mass)
    bodies, motions = walled_bodies()
    ends = []
    for m in (mass, np.ones(mass.size, F32)):
        with OU.context(S, (p, pos, vel, m)) as sph:
            sph.setObstacles(obst)
            sph.setObstacleMotion(motions)
            sph.setBodies(bodies)
            st, rows, _, _ = pinned_steps(oracle, sph, p, obst, motions, bodies, m, OU.HOOK_STEPS)
            assert sum(int(r.count.sum()) for r in rows) > 50
            ends.append(st.V[1].copy())
    assert not same(ends[0], ends[1])


# ---- 9. ports -----------------------------------------------------------------------------------------------------------------------
NEXT = float(np.nextafter(F32(1.0), F32(2.0)))


def port_block(flavour, emitter_masses, firsts=(0, 0), xs=(0.7, 0.7)):
    """tests/test_gpu_ports.py's block under the flavour and its sink, with that file's emitter (18 x 18 points
    blowing along -x every third step) once per mass of emitter_masses: from port step firsts[k] on, its plane at
    x = xs[k]"""
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_ports import block_scene
    p, pos, vel, _, _, sinks = block_scene()
    mass = mass_cases.masses(flavour, p, pos)
    emitters = [S.Emitter(0, (xs[k], 0.2, 0.2), (18, 18), 0.0317, (-15.0, 0.0, 0.0), m, first=firsts[k], every=3)
                for k, m in enumerate(emitter_masses)]
    return p, pos, vel, mass, emitters, sinks


def port_run(oracle, scene, steps, on_applied=None):
    """(PortRun after `steps` steps, its snapshot); on_applied sees the last step's state behind its ports"""
    import port_emulation as PO
    from test_gpu_ports import snapshot
    p, pos, vel, mass, emitters, sinks = scene
    run = PO.PortRun(to_oracle_params(p), pos, vel, mass, emitters, sinks)
    for k in range(steps):
        assert run.step(oracle, on_applied=on_applied if k == steps - 1 else None)
    return run, snapshot(run)


def fast_against_the_general_route(S, scene, steps):
    """tests/test_gpu_ports.py's FULL_FAST pin: the port context against a context without ports that is fed the
    restatement's edits before every step - uploaded as masses that are not all equal, so that it runs the general
    instantiations whatever the port context decides for itself."""
    import port_emulation as PO
    from test_gpu_ports import error_word, live_state, same_state
    p, pos, vel, mass, emitters, sinks = scene
    edits = PO.PortRun(to_oracle_params(p), pos, vel, mass, emitters, sinks)
    with S.SPH(mass.size, p, mode=S.MODE_FULL_FAST, capacity=6000) as sph, \
            S.SPH(mass.size, p, mode=S.MODE_FULL_FAST, capacity=6000) as plain:
        sph.setParticles(pos, vel, mass)
        sph.setPorts(emitters, sinks)
        for step in range(steps):
            now = live_state(sph)
            assert np.array_equal(now["ids"], edits.ids)
            edits.pos, edits.vel = now["pos"].copy(), now["vel"].copy()
            assert edits.apply_ports()
            plain.call("sph_hip_slab_upload", edits.live, np.ascontiguousarray(edits.pos).ctypes.data_as(C.c_void_p),
                       np.ascontiguousarray(edits.vel).ctypes.data_as(C.c_void_p),
                       np.ascontiguousarray(edits.mass).ctypes.data_as(C.c_void_p),
                       np.ascontiguousarray(edits.ids).ctypes.data_as(C.c_void_p), 0)
            plain.step()
            sph.step()
            same_state(live_state(sph), live_state(plain), "fast step %d" % step)
        t, _, _ = sph.getPorts()
        assert t.emitted.tolist() == edits.emitted.tolist() and t.removed.tolist() == edits.removed.tolist()
        assert t.live == edits.live and error_word(sph) == 0


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_ports_into_unequal_residents(oracle, hiplib, flavour):
    """the ports' block with the flavour's residents, one emitter of mass 2.5 and the sink, three steps: FULL against
    PortRun bit for bit; FULL_FAST against the general route fed the restatement's edits.  download_live returns no
    masses: that every survivor kept its own mass against its id is held through the densities and accelerations of
    the rows by id, which are sums over the neighbours' masses."""
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_ports import check_totals, error_word, live_state, same_state
    scene = port_block(flavour, [2.5])
    p, pos, vel, mass, emitters, sinks = scene
    run, want = port_run(oracle, scene, STEPS)
    assert sum(m for _, _, m in want["history"]) > 0 and sum(r for _, r, _ in want["history"]) > 0, want["history"]
    survivors = run.ids[run.ids < mass.size]
    assert survivors.size < mass.size and same(run.mass[:survivors.size], mass[survivors])
    with S.SPH(mass.size, p, mode=S.MODE_FULL, capacity=6000) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setPorts(emitters, sinks)
        sph.run(STEPS)
        same_state(live_state(sph), want, "%s after run(%d)" % (flavour, STEPS))
        check_totals(sph, want)
        assert error_word(sph) == 0
    fast_against_the_general_route(S, scene, STEPS)


def kept_flag_density(p, pos, mass):
    """the densities of a density pass that takes pi.w for every neighbour: UNIFORM_MASS on masses that are not"""
    return mass_cases.own_mass(P.particle_density, p, pos, np.zeros(3 * mass.size, F32), mass)


def ulp_scene():
    """A unit-mass block, one emitter of mass 1.0f from step 0 and one of the next float above it from step 1, its
    plane where the first emitter's layer stands by then; no sink."""
    p, pos, vel, mass, emitters, _ = port_block("UNIT", [1.0, NEXT], firsts=(0, 1))
    return p, pos, vel, mass, emitters, []


def ulp_figures(oracle):
    """(PortRun's snapshot after two steps, rows of the second step's state whose density a kept flag would change,
    of them rows that are not the heavier emitter's)"""
    seen = {}
    scene = ulp_scene()
    _, want = port_run(oracle, scene, 2, on_applied=lambda r: seen.update(pos=r.pos.copy(), mass=r.mass.copy()))
    heavy = seen["mass"] != 1
    assert heavy.sum() == 324
    kept = kept_flag_density(scene[0], np.ascontiguousarray(seen["pos"].reshape(-1)), seen["mass"])
    differ = mass_cases.rows_differing(want["rho"], kept)          # (rows in id order in both: nothing is removed)
    return want, int(differ.sum()), int(differ[~heavy].sum())


def test_an_emitter_one_ulp_heavier_clears_the_uniform_mass_flag(oracle, hiplib):
    """The upload sets uniform_mass; the second emitter's mass differs from the resident one in bits, so the rule
    (port_policy.h: port_mass_rule) must clear it.  After the step in which that emitter's layer enters, the densities
    are the oracle's in FULL - which a pass that kept the flag misses in the rows counted here, particles of the
    block and of the first layer among them - and the general route's in FULL_FAST."""
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_ports import check_totals, error_word, live_state, same_state
    scene = ulp_scene()
    p, pos, vel, mass, emitters, sinks = scene
    assert mass_cases.uniform(mass) and F32(NEXT) != F32(1.0) and not mass_cases.uniform(F32([e.mass for e in emitters]))
    want, differ, differ_light = ulp_figures(oracle)
    assert differ >= 100 and differ_light >= 50, (differ, differ_light)
    with S.SPH(mass.size, p, mode=S.MODE_FULL, capacity=6000) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setPorts(emitters, sinks)
        sph.run(2)
        same_state(live_state(sph), want, "two steps")
        check_totals(sph, want)
        assert error_word(sph) == 0
    fast_against_the_general_route(S, scene, 2)


@pytest.mark.parametrize("agree", [True, False], ids=["agreeing", "disagreeing"])
def test_an_empty_upload_filled_by_two_emitters(oracle, hiplib, agree):
    """Nothing resident: the emitters' own agreement decides.  Two emitters of mass 2.5 (the flag may be set: the
    resident mass is theirs) and two of 2.5 and 1.5 (it must be clear), their planes 0.03 apart so that their
    particles are each other's neighbours: FULL against PortRun bit for bit after three steps, FULL_FAST against the
    general route."""
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_ports import check_totals, error_word, live_state, same_state
    p, _, _, _, emitters, _ = port_block("UNIT", [2.5, 2.5 if agree else 1.5], xs=(0.7, 0.73))
    empty = np.zeros(0, F32)
    scene = (p, empty, empty, empty, emitters, [])
    seen = {}
    run, want = port_run(oracle, scene, STEPS, on_applied=lambda r: seen.update(pos=r.pos.copy(), mass=r.mass.copy()))
    assert want["live"] == 2 * 324 and (want["ncount"] > 0).all()
    assert mass_cases.uniform(seen["mass"]) == agree
    if not agree:
        kept = kept_flag_density(p, np.ascontiguousarray(seen["pos"].reshape(-1)), seen["mass"])
        assert mass_cases.rows_differing(want["rho"], kept).sum() >= 324
    with S.SPH(0, p, mode=S.MODE_FULL, capacity=6000) as sph:
        sph.setParticles(empty, empty, empty)
        sph.setPorts(emitters, [])
        sph.run(STEPS)
        same_state(live_state(sph), want, "after run(%d)" % STEPS)
        check_totals(sph, want)
        assert error_word(sph) == 0
    fast_against_the_general_route(S, scene, STEPS)


# ---- the figures ---------------------------------------------------------------------------------------------------------
def block_rows(flavour):
    """Per feature: (rows that differ from the own_mass variant, rows that differ from the unit-mass run) on the
    2 001-particle block, by the restatements alone; and the rows with a member."""
    p, pos, vel, mass, T, kappa = mass_cases.block(flavour)
    unit = np.ones(N, F32)
    rho, rho1 = P.particle_density(p, pos, vel, mass), P.particle_density(p, pos, vel, unit)
    on = pos.reshape(-1, 3)
    calls = {"cohesion": lambda m, r: CE.sums(p, pos, vel, m),
             "xsph": lambda m, r: XE.sums(p, pos, vel, m, r),
             "scalars": lambda m, r: SC.step(p, pos, vel, m, r, T, kappa),
             "velgrad": lambda m, r: VE.rows(p, pos, vel, m),
             "pressure": lambda m, r: P.sample(p, pos, vel, m, on)[0],
             "density": lambda m, r: P.sample(p, pos, vel, m, on)[1]}
    out = {}
    for name, fn in calls.items():
        real = fn(mass, rho)
        own = mass_cases.own_mass(fn, mass, rho, own=mass)
        out[name] = (int(mass_cases.rows_differing(real, own).sum()), int(mass_cases.rows_differing(real, fn(unit, rho1)).sum()))
    return out, int((mass_cases.neighbour_counts(p, pos) > 0).sum())


def odd_one_figures():
    p, pos, vel, mass, _, _ = mass_cases.block("ODD_ONE")
    odd = mass_cases.odd_particle(p, pos)
    x = pos.reshape(-1, 3)
    d = x - x[odd]
    d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    return odd, int((np.sqrt(d2.astype(np.float64)) > 2.0 * float(F32(p.h))).sum()), int((d2 < F32(p.h2)).sum()) - 1


def cpu_figures():
    """The CPU_* constants again, from the restatements alone (the first state of the block: no step is needed)."""
    p, pos, vel, mass, _, _ = mass_cases.block("SPREAD")
    info = XE.sums(p, pos, vel, mass, P.particle_density(p, pos, vel, mass), with_info=True)[1]
    spread, members = block_rows("SPREAD")
    return {"CPU_ROWS_WITH_A_MEMBER": members, "CPU_SPREAD": spread, "CPU_TWO_SPECIES": block_rows("TWO_SPECIES")[0],
            "CPU_ODD_ONE": odd_one_figures(), "CPU_XSPH_SPREAD_G": round(EPS * float(info["g_sum"].max()), 4)}


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    if len(sys.argv) == 3:
        np.savez(sys.argv[2], **route_run(sys.argv[1]))
    else:
        for name, value in cpu_figures().items():
            print("%s = %r" % (name, value))
