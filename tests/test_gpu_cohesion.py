"""GPU: cohesion (include/sph_hip.h: cohesion).  k_cohesion_apply between the acceleration pass and the integrate,
against the numpy restatement tests/cohesion_emulation.py composed with the oracle's phases, bit for bit, on the
scalars' 2 001-particle block (eight workgroups, the last with one live lane; seeded velocities, gravity and walls
on).  The routes are set by switches that are read at context creation, so each runs in a child process of its own
(this file with a route name)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import buoyancy_emulation as BE
import cohesion_emulation as CE
import gauge_emulation as G
import load_emulation as L
import moving_obstacle_emulation as M
import path_emulation as PE
import pressure_emulation as PR
import scale_cases
from helpers import to_oracle_params
from test_gpu_scalars import N, api_sources, bits, block_scene, block_sources, mode_of, same

pytestmark = pytest.mark.gpu

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GAMMA = 0.02        # on the block the median |c| is 4.2 beside a median |a| of 9.8 (gravity)
# route name -> environment; what the tile statistics must show is asserted in the test
ROUTES = {
    "default": {},
    "untiled": {"SPH_HIP_UNTILED": "1"},
    "lists_none": {"SPH_HIP_TILE_CAP": "256"},     # no tile of this scene fits: every workgroup is LISTS_NONE
    "lists_some": {"SPH_HIP_LIST_CAP": "16"},      # most particles have more than 16 neighbours: NLIST_NO_LIST lanes
    "wide": {"SPH_HIP_TILE_CAP": "4096"},          # above 4064: 14-bit tile indices in the entries
    "no_fused_integrate": {"SPH_HIP_NO_FUSED_INTEGRATE": "1"},
}
ROUTE_SWITCHES = ("SPH_HIP_UNTILED", "SPH_HIP_NO_FUSED_INTEGRATE", "SPH_HIP_NO_PREHASH", "SPH_HIP_TILE_CAP",
                  "SPH_HIP_LIST_CAP", "SPH_HIP_TILE_CAP_ACCEL", "SPH_HIP_TILE_CAP_DENSITY", "SPH_HIP_CHUNKED",
                  "SPH_HIP_SCALAR_ROWS")
STATE = ("mPosition", "mVelocity", "mAcceleration", "mDensity")


def block():
    p, pos, vel, mass, _, _ = block_scene()
    return p, pos, vel, mass


def start(sph, pos, vel, mass, gamma=None):
    sph.setParticles(pos, vel, mass)
    if gamma is not None:
        sph.setCohesion(gamma)


def state_of(sph):
    part = sph.getParticles()
    return {nm: getattr(part, nm).copy() for nm in STATE + ("mNeighborCount",)}


def same_state(got, want, names=STATE):
    return [nm for nm in names if not same(got[nm], want[nm])]


def against_step(got, out):
    """the names of what differs between a context after a step and the restatement's step"""
    want = {"mPosition": out["pos"], "mVelocity": out["vel"], "mAcceleration": out["acc"], "mDensity": out["rho"]}
    return same_state(got, want)


# ---- FULL single steps against the restatement -------------------------------------------------------------------
def test_full_single_steps_equal_the_restatement(oracle, hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    with S.SPH(N, p) as sph:
        start(sph, pos, vel, mass, GAMMA)
        for k in range(3):
            out = CE.step(oracle, p, pos, vel, mass, GAMMA)
            sph.step()
            got = state_of(sph)
            assert against_step(got, out) == [], "step %d" % k
            assert out["touched"].sum() > N - 20
            assert (bits(out["acc"]) != bits(out["acc_before"])).reshape(-1, 3).any(1).sum() > N - 50
            pos, vel = got["mPosition"], got["mVelocity"]
        stats = sph.tileStats()
        assert stats["workgroups"] == 8 and stats["untiled_density"] == 0          # the list route
    # the step is not the one without cohesion
    plain = CE.step(oracle, p, pos, vel, mass, 0.0)
    again = CE.step(oracle, p, pos, vel, mass, GAMMA)
    assert not same(plain["vel"], again["vel"]) and same(plain["rho"], again["rho"])


# ---- the acceleration read back is the twin's plus c, clamped ------------------------------------------------------
@pytest.mark.parametrize("mode", ["full", "fast"])
def test_acceleration_is_the_twins_through_apply(hiplib, mode):
    """A twin context without cohesion, stepped from the same S_k, yields a; the cohesive context's accelerations
    are apply()'s a' - in both arithmetics the same c bits.  Two states: the block, and what the cohesive context
    made of it."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    for k in range(2):
        with S.SPH(N, p, mode=mode_of(S, mode)) as twin, S.SPH(N, p, mode=mode_of(S, mode)) as sph:
            start(twin, pos, vel, mass)
            start(sph, pos, vel, mass, GAMMA)
            twin.step()
            sph.step()
            a = twin.getParticles().mAcceleration.copy()
            got = state_of(sph)
            want, on, _ = CE.apply(p, GAMMA, pos, vel, mass, a)
            assert same(got["mAcceleration"], want), "state %d" % k
            assert on.sum() > N - 20 and not same(want, a)
            assert same(got["mDensity"], twin.getParticles().mDensity)
            assert np.array_equal(got["mNeighborCount"], twin.getParticles().mNeighborCount)
            pos, vel = got["mPosition"], got["mVelocity"]


# ---- FULL_FAST after the step: the existing bar against FULL -----------------------------------------------------------
def test_fast_state_after_the_step_against_full(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_full_fast import check_fast, check_fast_position, check_fast_velocity
    p, pos, vel, mass = block()
    for k in range(3):
        out = {}
        for mode in ("full", "fast"):
            with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
                start(sph, pos, vel, mass, GAMMA)
                sph.step()
                out[mode] = sph.getParticles()
        full, fast = out["full"], out["fast"]
        ref = {"ncount": full.mNeighborCount, "rho": full.mDensity, "acc": full.mAcceleration}
        worst, allowed = check_fast(fast, ref, p, mass, "state %d" % k)
        check_fast_velocity(fast.mVelocity, full.mVelocity, allowed, p.time_step, "state %d" % k)
        check_fast_position(fast.mPosition, full.mPosition, p, "state %d" % k)
        print("state %d: worst force rel err %.3g (bar 1e-4, every particle)" % (k, worst))
        pos, vel = full.mPosition.copy(), full.mVelocity.copy()


# ---- queued steps ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["full", "fast"])
def test_queued_steps_equal_single_steps(hiplib, mode):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    out = []
    for queued in (True, False):
        with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
            start(sph, pos, vel, mass, GAMMA)
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
        assert not same(sph.getParticles().mPosition, out[0][0]["mPosition"])      # (cohesion did act)


def test_a_setter_between_queued_steps_does_not_reach_them(oracle, hiplib):
    """gamma travels by value: run(2) with GAMMA, a new gamma, run(1) - the restatement with the gammas in that order."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    with S.SPH(N, p) as sph:
        start(sph, pos, vel, mass, GAMMA)
        sph.run(2)
        sph.setCohesion(-0.5 * GAMMA)
        sph.run(1)
        got = state_of(sph)
    for g in (GAMMA, GAMMA, -0.5 * GAMMA):
        out = CE.step(oracle, p, pos, vel, mass, g)
        pos, vel = out["pos"], out["vel"]
    assert against_step(got, out) == []


# ---- off ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["full", "fast"])
def test_zero_gamma_and_never_set_equal_a_plain_context(hiplib, mode):
    """gamma = 0, gamma = -0.0f and "never set" over 20 steps: byte for byte the same state, counts and energies."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    out = []
    for gamma in (None, 0.0, -0.0):
        with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
            start(sph, pos, vel, mass, gamma)
            assert sph.getCohesion() == 0.0
            sph.run(19)
            sph.step()
            st = state_of(sph)
            out.append([st[nm] for nm in STATE + ("mNeighborCount",)] + list(sph.energy()))
    for other in out[1:]:
        for a, c in zip(out[0], other):
            assert np.asarray(a).tobytes() == np.asarray(c).tobytes()


# ---- the clamp ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["full", "fast"])
def test_a_lowered_cfl_limit_clamps_the_total(oracle, hiplib, mode):
    """cfl_limit at the median |a| of the block by the oracle: the acceleration pass clamps half of the particles
    to it, and of those cohesion pushes some beyond it - clamped again - and some back inside."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    op = to_oracle_params(p)
    _, cs, ci = oracle.full_cells(op, pos)
    rho, _ = oracle.full_density(op, pos, mass, cs, ci)
    free = oracle.full_accel(op, pos, vel, mass, rho, cs, ci).reshape(-1, 3)
    limit = F32(np.median(np.linalg.norm(free.astype(np.float64), axis=1)))
    p.cfl_limit = limit
    p.cfl_limit2 = F32(limit * limit)
    out = CE.step(oracle, p, pos, vel, mass, GAMMA)
    on = out["touched"]
    total = (out["acc_before"].reshape(-1, 3) + out["c"]).astype(F32)
    over = ((total[:, 0] * total[:, 0] + total[:, 1] * total[:, 1]) + total[:, 2] * total[:, 2]) > p.cfl_limit2
    at_limit = np.abs(np.linalg.norm(out["acc_before"].reshape(-1, 3).astype(np.float64), axis=1) / limit - 1.0) < 1e-6
    assert (over & on).sum() > 100 and (~over & on).sum() > 100              # both kinds occur ...
    assert (over & on & at_limit).sum() > 50 and (~over & on & at_limit).sum() > 50      # ... among those that came in clamped
    with S.SPH(N, p, mode=mode_of(S, mode)) as sph, S.SPH(N, p, mode=mode_of(S, mode)) as twin:
        start(sph, pos, vel, mass, GAMMA)
        start(twin, pos, vel, mass)
        sph.step()
        twin.step()
        got = state_of(sph)
        if mode == "full":
            assert against_step(got, out) == []
        want, _, _ = CE.apply(p, GAMMA, pos, vel, mass, twin.getParticles().mAcceleration)
        assert same(got["mAcceleration"], want)
        norm = np.linalg.norm(got["mAcceleration"].reshape(-1, 3).astype(np.float64), axis=1)
        assert norm.max() <= float(limit) * (1.0 + 1e-6)


# ---- routes: one child process per setting ---------------------------------------------------------------------------
def route_run(route="default"):
    """FULL and FULL_FAST: the state after 1 and after 3 steps of the block with cohesion, and the tile statistics"""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    result, stats = {}, {}
    for mode in ("full", "fast"):
        with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
            start(sph, pos, vel, mass, GAMMA)
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
    out = CE.step(oracle, p, pos, vel, mass, GAMMA)
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


# ---- off unit scale -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", scale_cases.FLAVOURS)
def test_off_unit_scale_against_the_restatement(oracle, hiplib, flavour):
    """scale_cases.block_scene (6 000 particles: a compressed block, a layer, a spray without neighbours) with the
    walls on: FULL against the restatement for two steps, FULL_FAST's accelerations through apply() on its own twin.
    Under SHELL there are members beyond hscaled, which add +0.0f times their separation."""
    import smoothed_particle_hydrodynamics_amd as S
    import sample_emulation as SE
    p, pos, vel, mass = scale_cases.block_scene(flavour, walls=True)
    assert not SE.unit_scale(p)
    n = mass.size
    with S.SPH(n, p) as sph:
        start(sph, pos, vel, mass, GAMMA)
        for k in range(2):
            out = CE.step(oracle, p, pos, vel, mass, GAMMA)
            sph.step()
            got = state_of(sph)
            assert against_step(got, out) == [], "step %d" % k
            assert 5000 < out["touched"].sum() < n                 # the spray's lone particles are left alone
            pos, vel = got["mPosition"], got["mVelocity"]
    with S.SPH(n, p, mode=S.MODE_FULL_FAST) as twin, S.SPH(n, p, mode=S.MODE_FULL_FAST) as sph:
        start(twin, pos, vel, mass)
        start(sph, pos, vel, mass, GAMMA)
        twin.step()
        sph.step()
        want, on, _ = CE.apply(p, GAMMA, pos, vel, mass, twin.getParticles().mAcceleration)
        assert same(sph.getParticles().mAcceleration, want) and on.sum() > 5000


# ---- beside other features ---------------------------------------------------------------------------------------------
def test_cohesion_with_scalars_and_buoyancy(oracle, hiplib):
    """One context with carried scalars, their sources, a buoyancy and cohesion: three FULL steps against the composed
    restatements - cohesion first, buoyancy's a is what cohesion left."""
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_buoyancy import block_buoyancy, emu_of
    p, pos, vel, mass, T, kappa = block_scene()
    sources = block_sources(p)
    buoyancy = block_buoyancy()
    b = emu_of(buoyancy, p)
    with S.SPH(N, p) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setScalars(T, kappa)
        sph.setScalarSources(api_sources(sources))
        sph.setBuoyancy(buoyancy)
        sph.setCohesion(GAMMA)
        for k in range(3):
            out = CE.step(oracle, p, pos, vel, mass, GAMMA, T, kappa, sources, b)
            sph.step()
            got, T_got = state_of(sph), sph.getScalars()
            assert against_step(got, out) == [] and same(T_got, out["T"]), "step %d" % k
            pos, vel, T = got["mPosition"], got["mVelocity"], T_got
    # each of the two did act
    only_b = CE.step(oracle, p, pos, vel, mass, 0.0, T, kappa, sources, b)
    only_c = CE.step(oracle, p, pos, vel, mass, GAMMA, T, kappa, sources, None)
    both = CE.step(oracle, p, pos, vel, mass, GAMMA, T, kappa, sources, b)
    assert not same(both["acc"], only_b["acc"]) and not same(both["acc"], only_c["acc"])


def test_an_obstacle_on_a_path_a_load_recording_and_a_pressure_gauge_beside_cohesion(oracle, hiplib):
    """Four single FULL steps of the block with a box on a sine path, a load recording and two pressure gauges, every
    step against the restatements fed with the EMULATED state: cohesion_emulation.step with path_emulation's
    integrate in place of the oracle's, pressure_emulation's readings in S_k, load_emulation's rows."""
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
        start(sph, pos, vel, mass, GAMMA)
        sph.setObstacles(obst)
        sph.setObstaclePaths(paths)
        sph.setGauges(gauges)
        sph.recordGauges(steps)
        sph.recordLoads(steps)
        readings = []
        for k in range(steps):
            readings.append(PR.evaluate(p, pos, vel, mass, eg))
            out = CE.step(oracle, p, pos, vel, mass, GAMMA, integrate=integrate_at(k))
            sph.step()
            assert against_step(state_of(sph), out) == [], "step %d" % k
            pos, vel = out["pos"], out["vel"]
        rec = sph.getGaugeRecord()
        loads = sph.getLoads()
    for r in range(steps):
        assert G.same_readings(G.Readings(rec.v[r], rec.n[r], rec.k[r]), readings[r]), "gauge row %d" % r
        assert rows[r].same(loads.impulse_q[r], loads.count[r], loads.skipped[r]), "load row %d" % r
    assert rec.n.min() > 0 and loads.count[:, L.WALLS].sum() > 0 and loads.count[:, :L.WALLS].sum() > 0


# ---- a whole scene ---------------------------------------------------------------------------------------------------
def test_droplet_100_queued_steps_equal_the_restatement(oracle, hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass, gamma = scenes.droplet(3000)
    with S.SPH(mass.size, p) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setCohesion(gamma)
        assert sph.getCohesion() == float(F32(gamma))
        sph.run(100)
        got = state_of(sph)
    g = float(F32(gamma))
    for _ in range(100):
        out = CE.step(oracle, p, pos, vel, mass, g)
        pos, vel = out["pos"], out["vel"]
    assert against_step(got, out) == []
    assert out["touched"].all() and np.isfinite(out["pos"]).all()


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
        assert sph.getCohesion() == 0.0
        sph.setCohesion(0.25)
        assert sph.getCohesion() == 0.25
        for bad in (np.nan, np.inf, -np.inf):
            refused(sph.setCohesion, bad, text="a gamma that is not finite")
        assert sph.getCohesion() == 0.25                       # a refused call keeps what is set
        sph.setCohesion(-1.5)                                  # a repulsion is allowed
        assert sph.getCohesion() == -1.5
        sph.step()
        assert sph.getCohesion() == -1.5
        sph.setCohesion(None)                                  # None and 0 switch it off
        assert sph.getCohesion() == 0.0
        sph.setCohesion(0.125)
        sph.setCohesion(-0.0)
        assert sph.getCohesion() == 0.0 and not np.signbit(sph.getCohesion())
        # ports both ways
        sink = Sink((0.9, 0.9, 0.9), (1.0, 1.0, 1.0))
        sph.setPorts([], [sink])
        refused(sph.setCohesion, 0.25, text="a context with ports cannot have cohesion")
        sph.setCohesion(0.0)                                   # off is never refused
        sph.setPorts([], [])
        sph.setCohesion(0.25)
        refused(sph.setPorts, [], [sink], text="a context with cohesion cannot have ports")
        sph.setPorts([], [])                                   # (clearing ports is no port)
        assert sph.getCohesion() == 0.25
        sph.setParticles(pos, vel, mass)                       # an upload drops it
        assert sph.getCohesion() == 0.0
        sph.step()                                             # and a step launches nothing for it
    # REF mode
    rp, rpos, rvel, rmass = scenes.dense_block(512)
    with S.SPH(512, rp, mode=S.MODE_REF) as sph:
        sph.setParticles(rpos, rvel, rmass)
        refused(sph.setCohesion, 0.25, text="FULL and FULL_FAST contexts only")
        sph.setCohesion(0.0)
        assert sph.getCohesion() == 0.0
    # a slab context
    with HipSlab(p, 0, p.full_cells_z // 2, 4096, 1024, has_left=False) as slab:
        import ctypes as C
        with pytest.raises(S.SphHipError, match="slab contexts"):
            slab.call("sph_hip_set_cohesion", C.c_float(0.25))
        slab.call("sph_hip_set_cohesion", C.c_float(0.0))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    np.savez(sys.argv[2], **route_run(sys.argv[1]))
