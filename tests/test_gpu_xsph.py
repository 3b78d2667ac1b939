"""GPU: XSPH velocity smoothing (include/sph_hip.h: xsph).  k_xsph_stage and k_xsph_apply between the acceleration
pass and the integrate, against the numpy restatement tests/xsph_emulation.py composed with the oracle's phases, bit
for bit, on the scalars' 2 001-particle block (eight workgroups, the last with one live lane; seeded velocities,
gravity and walls on).  The routes are set by switches that are read at context creation, so each runs in a child
process of its own (this file with a route name)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gauge_emulation as G
import load_emulation as L
import moving_obstacle_emulation as M
import path_emulation as PE
import pressure_emulation as PR
import scale_cases
import xsph_emulation as XE
from helpers import to_oracle_params
from test_gpu_cohesion import ROUTES, ROUTE_SWITCHES, STATE, against_step, block, same_state, state_of
from test_gpu_scalars import N, api_sources, bits, block_scene, block_sources, mode_of, same

pytestmark = pytest.mark.gpu

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EPS = 0.5           # Monaghan's usual choice; on the block the median |dv| is 0.15 beside a median |v| of 0.30
GAMMA = 0.02        # test_gpu_cohesion's


def start(sph, pos, vel, mass, eps=None):
    sph.setParticles(pos, vel, mass)
    if eps is not None:
        sph.setVelocitySmoothing(eps)


# ---- FULL single steps against the restatement -------------------------------------------------------------------
def test_full_single_steps_equal_the_restatement(oracle, hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    with S.SPH(N, p) as sph:
        start(sph, pos, vel, mass, EPS)
        for k in range(3):
            out = XE.step(oracle, p, pos, vel, mass, EPS)
            sph.step()
            got = state_of(sph)
            assert against_step(got, out) == [], "step %d" % k
            assert out["touched"].sum() > N - 20                              # nearly every particle is touched
            assert (bits(out["dv"]) & 0x7fffffff).reshape(-1, 3).any(1).sum() > N - 20
            assert same(out["acc"], out["acc_before"])                        # acc is not touched
            pos, vel = got["mPosition"], got["mVelocity"]
        stats = sph.tileStats()
        assert stats["workgroups"] == 8 and stats["untiled_density"] == 0          # the list route
    # the step is not the plain one
    plain = XE.step(oracle, p, pos, vel, mass, 0.0)
    again = XE.step(oracle, p, pos, vel, mass, EPS)
    differ = (bits(plain["vel"]) != bits(again["vel"])).reshape(-1, 3).any(1).sum()
    assert differ > N - 20 and same(plain["rho"], again["rho"]) and same(plain["acc"], again["acc"])


# ---- FULL_FAST: the velocity change through apply() on the twin's state ------------------------------------------------
def test_fast_velocity_change_is_apply_on_the_twins_state(oracle, hiplib):
    """A FULL_FAST twin without the smoothing, stepped from the same S_k, yields the step's densities and
    accelerations (the smoothing touches neither); the smoothing context's new velocities and positions are the
    integrate's from apply()'s v' and the twin's a.  Two states: the block, and what the smoothing context made of it."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    op = to_oracle_params(p)
    for k in range(2):
        with S.SPH(N, p, mode=S.MODE_FULL_FAST) as twin, S.SPH(N, p, mode=S.MODE_FULL_FAST) as sph:
            start(twin, pos, vel, mass)
            start(sph, pos, vel, mass, EPS)
            twin.step()
            sph.step()
            t, got = state_of(twin), state_of(sph)
            assert same(got["mAcceleration"], t["mAcceleration"]) and same(got["mDensity"], t["mDensity"])
            assert np.array_equal(got["mNeighborCount"], t["mNeighborCount"])
            v1, on, dv = XE.apply(p, EPS, pos, vel, mass, t["mDensity"])
            assert on.sum() > N - 20
            # the twin's own integrate from (pos, vel, a) is the oracle's: then so is the smoothing context's from v'
            x0, w0 = pos.copy(), vel.copy()
            oracle.integrate(op, x0, w0, t["mAcceleration"].copy(), mass)
            assert same(t["mPosition"], x0) and same(t["mVelocity"], w0), "state %d: the twin" % k
            x1, w1 = pos.copy(), np.ascontiguousarray(v1, F32).copy()
            oracle.integrate(op, x1, w1, t["mAcceleration"].copy(), mass)
            assert same(got["mVelocity"], w1) and same(got["mPosition"], x1), "state %d" % k
            assert not same(w1, w0)
            pos, vel = got["mPosition"], got["mVelocity"]


# ---- queued steps ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["full", "fast"])
def test_queued_steps_equal_single_steps(hiplib, mode):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    out = []
    for queued in (True, False):
        with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
            start(sph, pos, vel, mass, EPS)
            if queued:
                sph.run(5)
            else:
                for _ in range(5):
                    sph.step()
            out.append((state_of(sph), sph.energy()))
    assert same_state(out[0][0], out[1][0]) == [] and out[0][1] == out[1][1]
    with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
        start(sph, pos, vel, mass)
        sph.run(5)
        assert not same(sph.getParticles().mVelocity, out[0][0]["mVelocity"])      # (the smoothing did act)


def test_a_setter_between_queued_steps_does_not_reach_them(oracle, hiplib):
    """eps travels by value: run(2) with EPS, a new eps, run(1) - the restatement with the settings in that order."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    with S.SPH(N, p) as sph:
        start(sph, pos, vel, mass, EPS)
        sph.run(2)
        sph.setVelocitySmoothing(0.125)
        sph.run(1)
        got = state_of(sph)
    for e in (EPS, EPS, 0.125):
        out = XE.step(oracle, p, pos, vel, mass, e)
        pos, vel = out["pos"], out["vel"]
    assert against_step(got, out) == []


# ---- off ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["full", "fast"])
def test_zero_none_and_never_set_equal_a_plain_context(hiplib, mode):
    """eps = 0, -0.0f, None and "never set" over 20 steps: byte for byte the same state, counts and energies."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    out = []
    for setting in ("never", None, 0.0, -0.0):
        with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
            sph.setParticles(pos, vel, mass)
            if setting != "never":
                sph.setVelocitySmoothing(setting)
            assert sph.getVelocitySmoothing() == 0.0
            sph.run(19)
            sph.step()
            st = state_of(sph)
            out.append([st[nm] for nm in STATE + ("mNeighborCount",)] + list(sph.energy()))
    for other in out[1:]:
        for a, c in zip(out[0], other):
            assert np.asarray(a).tobytes() == np.asarray(c).tobytes()


# ---- routes: one child process per setting ---------------------------------------------------------------------------
def route_run(route="default"):
    """FULL and FULL_FAST: the state after 1 and after 3 steps of the block with the smoothing, and the tile statistics"""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    result, stats = {}, {}
    for mode in ("full", "fast"):
        with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
            start(sph, pos, vel, mass, EPS)
            for steps, tag in ((1, "1"), (2, "3")):
                sph.step() if steps == 1 else sph.run(steps)
                st = state_of(sph)
                for nm in STATE:
                    result[mode + tag + nm] = st[nm]
            result[mode + "_counts"] = st["mNeighborCount"]
            stats[mode] = sph.tileStats() if route != "untiled" else {}
    result["stats"] = json.dumps(stats)
    return result


@pytest.fixture(scope="module")
def default_route(hiplib):
    return route_run()


@pytest.mark.parametrize("route", list(ROUTES))
def test_every_route_gives_the_same_bits(oracle, default_route, route, tmp_path):
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
            assert same(got[name], default_route[name]) if "counts" not in name else \
                np.array_equal(got[name], default_route[name]), (route, name)
    # and the bits are the restatement's
    p, pos, vel, mass = block()
    out = XE.step(oracle, p, pos, vel, mass, EPS)
    for nm, key in (("mPosition", "pos"), ("mVelocity", "vel"), ("mAcceleration", "acc"), ("mDensity", "rho")):
        assert same(got["full1" + nm], out[key]), (route, nm)
    # the setting produced the route it is there for, or the case proves nothing
    stats = json.loads(str(got["stats"]))
    for mode in ("full", "fast"):
        st, counts = stats[mode], got[mode + "_counts"]
        if route in ("default", "no_fused_integrate"):
            assert st["workgroups"] == 8 and st["untiled_density"] == 0 and st["wide_entries"] == 0
            assert counts.max() <= st["list_capacity"]                       # every lane has its list
        elif route == "lists_none":
            # every workgroup with 256 particles gave up its tile (the last one, a single particle, may keep its own)
            assert st["capacity_density"] == 256 and st["largest_tile"] > 256 and st["workgroups"] == 8
            assert st["untiled_density"] >= 7
        elif route == "lists_some":
            assert st["list_capacity"] == 16 and st["untiled_density"] == 0
            # lanes without a list (more neighbours than it holds) beside lanes with one, in every full workgroup
            assert (counts > 16).sum() > 100 and (counts <= 16).sum() > 100
        elif route == "wide":
            assert st["wide_entries"] == 1 and st["capacity_density"] == 4096 and st["untiled_density"] == 0
        else:
            assert route == "untiled" and st == {}       # (an untiled context keeps no tile statistics)


# ---- edge shapes ------------------------------------------------------------------------------------------------------
def tiny(n):
    """n <= 2 particles of the block's box, inside h of each other"""
    p, _, _, _ = block()
    h = float(p.h)
    pos = np.array([[0.05, 0.3, 0.5], [0.05 + 0.4 * h, 0.3 + 0.3 * h, 0.5]], F32)[:n].reshape(-1)
    vel = np.array([[0.1, -0.2, 0.3], [-0.3, 0.1, 0.05]], F32)[:n].reshape(-1)
    return p, np.ascontiguousarray(pos), np.ascontiguousarray(vel), np.ones(n, F32)


def test_one_particle_has_no_neighbour_and_keeps_its_bits(oracle, hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = tiny(1)
    out = XE.step(oracle, p, pos, vel, mass, EPS)
    assert not out["touched"].any() and out["rho"][0] == 0          # (its staged inverse density is inf: never read)
    states = []
    for eps in (EPS, None):
        with S.SPH(1, p) as sph:
            start(sph, pos, vel, mass, eps)
            sph.step()
            states.append(state_of(sph))
            sph.run(3)
            states.append(state_of(sph))
    assert against_step(states[0], out) == []
    assert same_state(states[0], states[2]) == [] and same_state(states[1], states[3]) == []


def test_two_particles_inside_h_of_each_other(oracle, hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = tiny(2)
    with S.SPH(2, p) as sph:
        start(sph, pos, vel, mass, EPS)
        for k in range(3):
            out = XE.step(oracle, p, pos, vel, mass, EPS)
            sph.step()
            got = state_of(sph)
            assert against_step(got, out) == [], "step %d" % k
            assert out["touched"].all() and (got["mNeighborCount"] == 1).all()
            # the two changes are each other's negation, bit for bit: momentum is conserved
            assert np.array_equal(bits(out["dv"][0]) ^ np.uint32(0x80000000), bits(out["dv"][1]))
            pos, vel = got["mPosition"], got["mVelocity"]


def test_one_live_lane_in_the_second_workgroup(oracle, hiplib):
    """257 particles of the block's box at the block's density: the second workgroup has a single live lane."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    n = 257
    pos, vel, mass = pos[:3 * n].copy(), vel[:3 * n].copy(), mass[:n].copy()
    pos.reshape(-1, 3)[:] = (pos.reshape(-1, 3) * F32(0.5)).astype(F32)    # an eighth of the volume: ~32 neighbours each
    with S.SPH(n, p) as sph:
        start(sph, pos, vel, mass, EPS)
        for k in range(3):
            out = XE.step(oracle, p, pos, vel, mass, EPS)
            sph.step()
            got = state_of(sph)
            assert against_step(got, out) == [], "step %d" % k
            assert out["touched"].sum() > 200
            pos, vel = got["mPosition"], got["mVelocity"]
        assert sph.tileStats()["workgroups"] == 2


def test_a_clump_beyond_the_list_capacity(oracle, hiplib):
    """400 of the block's particles in a cube of edge 0.4 h: each of them has more than 254 neighbours, more than the
    lists hold at first - those lanes walk the rows in the first step, the host enlarges the lists, and the later
    steps walk the longer lists.  Every step against the restatement."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    rng = np.random.default_rng(5)
    x = pos.reshape(-1, 3).copy()
    x[:400] = np.array([0.05, 0.3, 0.5], F32) + rng.uniform(-0.2, 0.2, (400, 3)).astype(F32) * F32(p.h)
    pos = np.ascontiguousarray(x.reshape(-1))
    with S.SPH(N, p) as sph:
        start(sph, pos, vel, mass, EPS)
        caps = []
        for k in range(4):
            out = XE.step(oracle, p, pos, vel, mass, EPS)
            sph.step()
            got = state_of(sph)
            caps.append(sph.tileStats()["list_capacity"])
            assert against_step(got, out) == [], "step %d" % k
            assert (got["mNeighborCount"] > 254).sum() > 64 and out["touched"].sum() > N - 20
            pos, vel = got["mPosition"], got["mVelocity"]
    assert caps[0] == 254 and caps[-1] > 254, caps


# ---- off unit scale -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", scale_cases.FLAVOURS)
def test_off_unit_scale_against_the_restatement(oracle, hiplib, flavour):
    """scale_cases.block_scene (6 000 particles: a compressed block, a layer, a spray without neighbours) with the
    walls on: FULL against the restatement for two steps.  Under SHELL there are members beyond hscaled, whose
    weight is +0.0f."""
    import smoothed_particle_hydrodynamics_amd as S
    import sample_emulation as SE
    p, pos, vel, mass = scale_cases.block_scene(flavour, walls=True)
    assert not SE.unit_scale(p)
    n = mass.size
    with S.SPH(n, p) as sph:
        start(sph, pos, vel, mass, EPS)
        for k in range(2):
            out = XE.step(oracle, p, pos, vel, mass, EPS)
            sph.step()
            got = state_of(sph)
            assert against_step(got, out) == [], "step %d" % k
            assert 5000 < out["touched"].sum() < n                 # the spray's lone particles are left alone
            pos, vel = got["mPosition"], got["mVelocity"]


# ---- beside other features ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cohesive", [False, True])
@pytest.mark.parametrize("scalars", [False, True])
@pytest.mark.parametrize("buoyant", [False, True])
def test_beside_cohesion_scalars_and_buoyancy(oracle, hiplib, cohesive, scalars, buoyant):
    """Every combination of the three settings beside the smoothing: two FULL steps against the composed restatements -
    cohesion, then the smoothing, then buoyancy, whose b*dt is added to the smoothed velocity.  Buoyancy without
    scalars does not exist: the setter refuses it, and the context steps as one without."""
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_buoyancy import block_buoyancy, emu_of
    p, pos, vel, mass, T, kappa = block_scene()
    sources = block_sources(p)
    buoyancy = block_buoyancy()
    b = emu_of(buoyancy, p) if buoyant and scalars else None
    gamma = GAMMA if cohesive else 0.0
    if not scalars:
        T = None
    with S.SPH(N, p) as sph:
        sph.setParticles(pos, vel, mass)
        if scalars:
            sph.setScalars(T, kappa)
            sph.setScalarSources(api_sources(sources))
        if buoyant and scalars:
            sph.setBuoyancy(buoyancy)
        elif buoyant:
            with pytest.raises(S.SphHipError):
                sph.setBuoyancy(buoyancy)
        if cohesive:
            sph.setCohesion(GAMMA)
        sph.setVelocitySmoothing(EPS)
        for k in range(2):
            out = XE.step(oracle, p, pos, vel, mass, EPS, gamma, T, kappa if scalars else None, sources if scalars else (), b)
            sph.step()
            got = state_of(sph)
            assert against_step(got, out) == [], "step %d" % k
            if scalars:
                T = sph.getScalars()
                assert same(T, out["T"]), "step %d" % k
            pos, vel = got["mPosition"], got["mVelocity"]
    # each of the settings did act
    args = (T, kappa if scalars else None, sources if scalars else ())
    both = XE.step(oracle, p, pos, vel, mass, EPS, gamma, *args, b)
    assert not same(both["vel"], XE.step(oracle, p, pos, vel, mass, 0.0, gamma, *args, b)["vel"])
    if cohesive:
        assert not same(both["acc"], XE.step(oracle, p, pos, vel, mass, EPS, 0.0, *args, b)["acc"])
    if b is not None:
        assert not same(both["acc"], XE.step(oracle, p, pos, vel, mass, EPS, gamma, *args, None)["acc"])


def test_an_obstacle_on_a_path_a_load_recording_a_pressure_gauge_and_a_monitor_beside_the_smoothing(oracle, hiplib):
    """Four single FULL steps of the block with a box on a sine path, a load recording, two pressure gauges and a
    monitor recording, every step against the restatements fed with the EMULATED state: xsph_emulation.step with
    path_emulation's integrate in place of the oracle's, pressure_emulation's readings in S_k, load_emulation's rows."""
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    p, pos, vel, mass = block()
    dt, damping = F32(p.time_step), F32(p.damping)
    maxv = F32([p.max_x, p.max_y, p.max_z])
    obst = [O.Box((0.02, 0.0, 0.3), (0.06, 0.2, 0.6))]
    paths = [O.MotionPath.sine((0.0, 0.02, 0.03), 8.0 * float(dt), 16)]
    gauges = [S.PressureGauge((0.05, 0.1, 0.5)), S.PressureGauge((0.05, 0.4, 0.2))]
    eg = [G.of(g) for g in gauges]
    steps = 4
    clock = M.clock(dt, steps)
    rows = []

    def integrate_at(k):
        def integrate(op, x, v, a, m):
            free = type(op).from_buffer_copy(bytes(op))       # (the oracle's parameters with the walls off)
            free.apply_walls = 0
            P = x.copy()
            oracle.integrate(free, x, v, a, m)
            V, Q, row = PE.integrate_respond(maxv, int(op.apply_walls), obst, paths, None, P, v, x, dt, damping, clock[k],
                                             clock[k + 1], m)
            v[:] = np.ascontiguousarray(V, F32).reshape(-1)
            x[:] = np.ascontiguousarray(Q, F32).reshape(-1)
            rows.append(row)
        return integrate

    with S.SPH(N, p) as sph:
        start(sph, pos, vel, mass, EPS)
        sph.setObstacles(obst)                       # none of them is refused
        sph.setObstaclePaths(paths)
        sph.setGauges(gauges)
        sph.recordGauges(steps)
        sph.recordLoads(steps)
        sph.recordMonitor(steps)
        readings = []
        for k in range(steps):
            readings.append(PR.evaluate(p, pos, vel, mass, eg))
            out = XE.step(oracle, p, pos, vel, mass, EPS, integrate=integrate_at(k))
            sph.step()
            assert against_step(state_of(sph), out) == [], "step %d" % k
            assert out["touched"].sum() > N - 20
            pos, vel = out["pos"], out["vel"]
        rec = sph.getGaugeRecord()
        loads = sph.getLoads()
        mon = sph.getMonitorRecord()
        assert sph.getVelocitySmoothing() == EPS
    for r in range(steps):
        assert G.same_readings(G.Readings(rec.v[r], rec.n[r], rec.k[r]), readings[r]), "gauge row %d" % r
        assert rows[r].same(loads.impulse_q[r], loads.count[r], loads.skipped[r]), "load row %d" % r
    assert rec.n.min() > 0 and loads.count[:, L.WALLS].sum() > 0 and loads.count[:, :L.WALLS].sum() > 0
    assert len(mon.rows) == steps and (mon.rows["live"] == N).all() and (mon.rows["bad"] == 0).all()
    # the last row's peak speed is the state's: the monitor reads what the integrate made of the smoothed velocity
    v = vel.reshape(-1, 3)
    v2 = ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).astype(np.float64).max()
    assert abs(float(mon.rows["v2_max"][-1]) / v2 - 1.0) < 1e-6


# ---- a whole scene ---------------------------------------------------------------------------------------------------
def test_dam_break_smoothed_100_queued_steps_equal_the_restatement(oracle, hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass, eps = scenes.dam_break_smoothed(2000)
    with S.SPH(mass.size, p) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setVelocitySmoothing(eps)
        assert sph.getVelocitySmoothing() == float(F32(eps))
        sph.run(100)
        got = state_of(sph)
    touched = []
    for _ in range(100):
        out = XE.step(oracle, p, pos, vel, mass, eps)
        touched.append(int(out["touched"].sum()))
        pos, vel = out["pos"], out["vel"]
    assert against_step(got, out) == []
    # the first step of the uniform surge changes nothing by bits; the broken dam's noise is smoothed
    assert touched[0] == 0 and touched[-1] > mass.size - 20 and np.isfinite(out["pos"]).all()


# ---- refusals, the getter, an upload ------------------------------------------------------------------------------------
def test_refusals_getter_and_what_drops_the_setting(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    from smoothed_particle_hydrodynamics_amd.ports import Sink
    from smoothed_particle_hydrodynamics_amd.slab import HipSlab
    p, pos, vel, mass = block()

    def refused(call, *args, text):
        with pytest.raises(S.SphHipError) as e:
            call(*args)
        assert text in str(e.value), str(e.value)

    with S.SPH(N, p) as sph:
        sph.setParticles(pos, vel, mass)
        assert sph.getVelocitySmoothing() == 0.0
        sph.setVelocitySmoothing(0.25)
        assert sph.getVelocitySmoothing() == 0.25
        for bad in (np.nan, np.inf, -np.inf):
            refused(sph.setVelocitySmoothing, bad, text="an eps that is not finite")
        for bad in (-0.25, 1.5, float(np.nextafter(F32(1.0), F32(2.0)))):
            refused(sph.setVelocitySmoothing, bad, text="an eps outside [0, 1]")
        assert sph.getVelocitySmoothing() == 0.25              # a refused call keeps what is set
        sph.setVelocitySmoothing(1.0)                          # the range's end is inside
        assert sph.getVelocitySmoothing() == 1.0
        sph.step()
        assert sph.getVelocitySmoothing() == 1.0
        sph.setVelocitySmoothing(None)                         # None and 0 switch it off
        assert sph.getVelocitySmoothing() == 0.0
        sph.setVelocitySmoothing(0.125)
        sph.setVelocitySmoothing(-0.0)
        assert sph.getVelocitySmoothing() == 0.0 and not np.signbit(sph.getVelocitySmoothing())
        # ports both ways
        sink = Sink((0.9, 0.9, 0.9), (1.0, 1.0, 1.0))
        sph.setPorts([], [sink])
        refused(sph.setVelocitySmoothing, 0.25, text="a context with ports cannot have velocity smoothing")
        sph.setVelocitySmoothing(0.0)                          # off is never refused
        sph.setPorts([], [])
        sph.setVelocitySmoothing(0.25)
        refused(sph.setPorts, [], [sink], text="a context with velocity smoothing cannot have ports")
        sph.setPorts([], [])                                   # (clearing ports is no port)
        assert sph.getVelocitySmoothing() == 0.25
        sph.setParticles(pos, vel, mass)                       # an upload drops it
        assert sph.getVelocitySmoothing() == 0.0
        sph.step()                                             # and a step launches nothing for it
    # REF mode
    rp, rpos, rvel, rmass = scenes.dense_block(512)
    with S.SPH(512, rp, mode=S.MODE_REF) as sph:
        sph.setParticles(rpos, rvel, rmass)
        refused(sph.setVelocitySmoothing, 0.25, text="FULL and FULL_FAST contexts only")
        sph.setVelocitySmoothing(0.0)
        assert sph.getVelocitySmoothing() == 0.0
    # a slab context
    with HipSlab(p, 0, p.full_cells_z // 2, 4096, 1024, has_left=False) as slab:
        with pytest.raises(S.SphHipError, match="slab contexts"):
            slab.call("sph_hip_set_xsph", C.c_float(0.25))
        slab.call("sph_hip_set_xsph", C.c_float(0.0))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    np.savez(sys.argv[2], **route_run(sys.argv[1]))
