"""GPU: the viscous stress (include/sph_hip.h: viscous stress).  k_viscous_stage and k_viscous_apply between the
acceleration pass and the integrate, against the numpy restatement tests/viscous_emulation.py composed with the
oracle's phases, bit for bit, on the scalars' 2 001-particle block (eight workgroups, the last with one live lane;
seeded velocities, gravity and walls on).  The routes are set by switches that are read at context creation, so each
runs in a child process of its own (this file with a route name)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gauge_emulation as G
import load_emulation as L
import mass_cases
import moving_obstacle_emulation as M
import path_emulation as PE
import pressure_emulation as PR
import scale_cases
import viscous_emulation as VE
from helpers import to_oracle_params
from test_gpu_cohesion import ROUTES, ROUTE_SWITCHES, STATE, against_step, block, same_state, state_of
from test_gpu_scalars import N, api_sources, bits, block_scene, block_sources, mode_of, same

pytestmark = pytest.mark.gpu

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GAMMA = 0.02        # test_gpu_cohesion's
EPS = 0.5           # test_gpu_xsph's


def block_mu(p, fraction=0.1):
    """a tenth of the bulk's explicit limit (scenes.viscous_stable_mu), as fp32: on the block the median |c| is of the
    order of gravity"""
    from smoothed_particle_hydrodynamics_amd import scenes
    return float(F32(scenes.viscous_stable_mu(p, fraction)))


def laws():
    """2 keys on channel 1 (a HOLD source and an ADD act on it) and 16 keys on channel 2 (it diffuses, and an ADD acts
    on it); the block's channels are seeded in [-1, 1)"""
    from smoothed_particle_hydrodynamics_amd import ViscosityLaw
    return {2: ViscosityLaw(1, [-0.5, 0.5], [3.0, 0.5]), 16: ViscosityLaw.exponential(2, 0.0, 1.5, -0.75, 0.75)}


def start(sph, pos, vel, mass, mu=None, law=None):
    sph.setParticles(pos, vel, mass)
    if mu is not None:
        sph.setViscousStress(mu, law)


# ---- FULL single steps against the restatement -------------------------------------------------------------------
def test_full_single_steps_equal_the_restatement(oracle, hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    mu = block_mu(p)
    with S.SPH(N, p) as sph:
        start(sph, pos, vel, mass, mu)
        for k in range(3):
            out = VE.step(oracle, p, pos, vel, mass, mu)
            sph.step()
            got = state_of(sph)
            assert against_step(got, out) == [], "step %d" % k
            assert out["touched"].sum() > N - 20                              # nearly every particle is touched
            assert (bits(out["acc"]) != bits(out["acc_before"])).reshape(-1, 3).any(1).sum() > N - 20
            pos, vel = got["mPosition"], got["mVelocity"]
        stats = sph.tileStats()
        assert stats["workgroups"] == 8 and stats["untiled_density"] == 0          # the list route
    # the step is not the plain one
    plain = VE.step(oracle, p, pos, vel, mass, 0.0)
    again = VE.step(oracle, p, pos, vel, mass, mu)
    differ = (bits(plain["vel"]) != bits(again["vel"])).reshape(-1, 3).any(1).sum()
    assert differ > N - 20 and same(plain["rho"], again["rho"]) and same(plain["acc"], again["acc_before"])


# ---- FULL_FAST: apply() on the twin's accelerations and densities ------------------------------------------------------
def test_fast_acceleration_is_apply_on_the_twins_state(oracle, hiplib):
    """A FULL_FAST twin without the term, stepped from the same S_k, yields the step's densities and accelerations; the
    viscous context's accelerations are apply()'s a' from them, and its new velocities and positions the oracle's
    integrate from a'.  Two states: the block, and what the viscous context made of it."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    mu = block_mu(p)
    op = to_oracle_params(p)
    for k in range(2):
        with S.SPH(N, p, mode=S.MODE_FULL_FAST) as twin, S.SPH(N, p, mode=S.MODE_FULL_FAST) as sph:
            start(twin, pos, vel, mass)
            start(sph, pos, vel, mass, mu)
            twin.step()
            sph.step()
            t, got = state_of(twin), state_of(sph)
            assert same(got["mDensity"], t["mDensity"]) and np.array_equal(got["mNeighborCount"], t["mNeighborCount"])
            a1, on, _, _ = VE.apply(p, mu, pos, vel, mass, t["mDensity"], t["mAcceleration"])
            assert on.sum() > N - 20 and not same(a1, t["mAcceleration"])
            assert same(got["mAcceleration"], a1), "state %d" % k
            # the twin's own integrate from (pos, vel, a) is the oracle's: then so is the viscous context's from a'
            x0, w0 = pos.copy(), vel.copy()
            oracle.integrate(op, x0, w0, t["mAcceleration"].copy(), mass)
            assert same(t["mPosition"], x0) and same(t["mVelocity"], w0), "state %d: the twin" % k
            x1, w1 = pos.copy(), vel.copy()
            oracle.integrate(op, x1, w1, np.ascontiguousarray(a1, F32).copy(), mass)
            assert same(got["mVelocity"], w1) and same(got["mPosition"], x1), "state %d" % k
            assert not same(w1, w0)
            pos, vel = got["mPosition"], got["mVelocity"]


# ---- queued steps ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["full", "fast"])
def test_queued_steps_equal_single_steps(hiplib, mode):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    mu = block_mu(p)
    out = []
    for queued in (True, False):
        with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
            start(sph, pos, vel, mass, mu)
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
        assert not same(sph.getParticles().mVelocity, out[0][0]["mVelocity"])      # (the term did act)


def test_a_setter_between_queued_steps_does_not_reach_them(oracle, hiplib):
    """mu and the law travel by value: run(2) with mu, a new mu with a law, run(1), the law dropped, run(1) - the
    restatement with the settings in that order."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, T, kappa = block_scene()
    kappa = np.zeros(4, F32)                                  # (the channels are only carried)
    mu = block_mu(p)
    law = laws()[2]
    with S.SPH(N, p) as sph:
        start(sph, pos, vel, mass, mu)
        sph.setScalars(T, kappa)
        sph.run(2)
        sph.setViscousStress(0.5 * mu, law)
        sph.run(1)
        sph.setViscousStress(0.25 * mu)
        sph.run(1)
        got = state_of(sph)
    for m, lw in ((mu, None), (mu, None), (0.5 * mu, VE.of(law)), (0.25 * mu, None)):
        out = VE.step(oracle, p, pos, vel, mass, m, lw, T=T, kappa=kappa)
        pos, vel = out["pos"], out["vel"]
    assert against_step(got, out) == []


# ---- off ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["full", "fast"])
def test_zero_none_and_never_set_equal_a_plain_context(hiplib, mode):
    """mu = 0, -0.0f, None and "never set" over 20 steps: byte for byte the same state, counts and energies."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    out = []
    for setting in ("never", None, 0.0, -0.0):
        with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
            sph.setParticles(pos, vel, mass)
            if setting != "never":
                sph.setViscousStress(setting)
            assert sph.getViscousStress() == (0.0, None)
            sph.run(19)
            sph.step()
            st = state_of(sph)
            out.append([st[nm] for nm in STATE + ("mNeighborCount",)] + list(sph.energy()))
    for other in out[1:]:
        for a, c in zip(out[0], other):
            assert np.asarray(a).tobytes() == np.asarray(c).tobytes()


# ---- routes: one child process per setting ---------------------------------------------------------------------------
def route_run(route="default"):
    """FULL and FULL_FAST: the state after 1 and after 3 steps of the block with the term - the second and third with
    a law - and the tile statistics"""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, T, _ = block_scene()
    mu = block_mu(p)
    result, stats = {}, {}
    for mode in ("full", "fast"):
        with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
            start(sph, pos, vel, mass, mu)
            sph.setScalars(T, np.zeros(4, F32))
            for steps, tag in ((1, "1"), (2, "3")):
                sph.step() if steps == 1 else sph.run(steps)
                st = state_of(sph)
                for nm in STATE:
                    result[mode + tag + nm] = st[nm]
                sph.setViscousStress(mu, laws()[16])
            result[mode + "_counts"] = st["mNeighborCount"]
            stats[mode] = sph.tileStats() if route != "untiled" else {}
    result["stats"] = json.dumps(stats)
    return result


@pytest.fixture(scope="module")
def default_route(hiplib):
    return route_run()


@pytest.mark.parametrize("route", list(ROUTES))
def test_every_route_gives_the_same_bits(oracle, default_route, route, tmp_path):
    assert sorted(ROUTES) == ["default", "lists_none", "lists_some", "no_fused_integrate", "untiled", "wide"]
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
    # and the bits are the restatement's: the first step with a constant mu, the next two with the law
    p, pos, vel, mass, T, _ = block_scene()
    mu = block_mu(p)
    kappa = np.zeros(4, F32)
    out = VE.step(oracle, p, pos, vel, mass, mu, T=T, kappa=kappa)
    for nm, key in (("mPosition", "pos"), ("mVelocity", "vel"), ("mAcceleration", "acc"), ("mDensity", "rho")):
        assert same(got["full1" + nm], out[key]), (route, nm)
    lw = VE.of(laws()[16])
    for _ in range(2):
        out = VE.step(oracle, p, out["pos"], out["vel"], mass, mu, lw, T=T, kappa=kappa)
    for nm, key in (("mPosition", "pos"), ("mVelocity", "vel"), ("mAcceleration", "acc"), ("mDensity", "rho")):
        assert same(got["full3" + nm], out[key]), (route, nm)
    assert out["touched"].sum() > N - 20
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
    """n <= 2 particles of the block's box, inside h of each other, of unequal masses"""
    p, _, _, _ = block()
    h = float(p.h)
    pos = np.array([[0.05, 0.3, 0.5], [0.05 + 0.4 * h, 0.3 + 0.3 * h, 0.5]], F32)[:n].reshape(-1)
    vel = np.array([[0.1, -0.2, 0.3], [-0.3, 0.1, 0.05]], F32)[:n].reshape(-1)
    return p, np.ascontiguousarray(pos), np.ascontiguousarray(vel), np.array([1.0, 3.0], F32)[:n].copy()


def test_one_particle_has_no_neighbour_and_keeps_its_bits(oracle, hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = tiny(1)
    mu = block_mu(p)
    out = VE.step(oracle, p, pos, vel, mass, mu)
    assert not out["touched"].any() and out["rho"][0] == 0          # (its staged volume is 0: it is left alone)
    states = []
    for setting in (mu, None):
        with S.SPH(1, p) as sph:
            start(sph, pos, vel, mass, setting)
            sph.step()
            states.append(state_of(sph))
            sph.run(3)
            states.append(state_of(sph))
    assert against_step(states[0], out) == []
    assert same_state(states[0], states[2]) == [] and same_state(states[1], states[3]) == []


def test_two_particles_inside_h_of_each_other(oracle, hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = tiny(2)
    mu = block_mu(p)
    with S.SPH(2, p) as sph:
        start(sph, pos, vel, mass, mu)
        for k in range(3):
            out = VE.step(oracle, p, pos, vel, mass, mu)
            sph.step()
            got = state_of(sph)
            assert against_step(got, out) == [], "step %d" % k
            assert out["touched"].all() and (got["mNeighborCount"] == 1).all()
            # masses 1 and 3: the two forces are each other's negation, so c_0 = -3 * c_1 to a rounding of the division
            c = out["c"].astype(np.float64)
            assert np.abs(c[0] + 3.0 * c[1]).max() <= 2.0 ** -22 * np.abs(c[0]).max() and np.abs(c[0]).max() > 0
            pos, vel = got["mPosition"], got["mVelocity"]


def test_one_live_lane_in_the_second_workgroup(oracle, hiplib):
    """257 particles of the block's box at the block's density: the second workgroup has a single live lane."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    mu = block_mu(p)
    n = 257
    pos, vel, mass = pos[:3 * n].copy(), vel[:3 * n].copy(), mass[:n].copy()
    pos.reshape(-1, 3)[:] = (pos.reshape(-1, 3) * F32(0.5)).astype(F32)    # an eighth of the volume: ~32 neighbours each
    with S.SPH(n, p) as sph:
        start(sph, pos, vel, mass, mu)
        for k in range(3):
            out = VE.step(oracle, p, pos, vel, mass, mu)
            sph.step()
            got = state_of(sph)
            assert against_step(got, out) == [], "step %d" % k
            assert out["touched"].sum() > 200
            pos, vel = got["mPosition"], got["mVelocity"]
        assert sph.tileStats()["workgroups"] == 2


def test_a_clump_beyond_the_list_capacity(oracle, hiplib):
    """400 of the block's particles in a cube of edge 0.4 h: each of them has more than 254 neighbours, more than the
    lists hold at first - those lanes walk the rows in the first step, the host enlarges the lists, and the later
    steps walk the longer lists.  Every step against the restatement.  (The clump is far outside the explicit range:
    the bits are what is checked.)"""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    mu = block_mu(p)
    rng = np.random.default_rng(5)
    x = pos.reshape(-1, 3).copy()
    x[:400] = np.array([0.05, 0.3, 0.5], F32) + rng.uniform(-0.2, 0.2, (400, 3)).astype(F32) * F32(p.h)
    pos = np.ascontiguousarray(x.reshape(-1))
    with S.SPH(N, p) as sph:
        start(sph, pos, vel, mass, mu)
        caps = []
        for k in range(4):
            out = VE.step(oracle, p, pos, vel, mass, mu)
            sph.step()
            got = state_of(sph)
            caps.append(sph.tileStats()["list_capacity"])
            assert against_step(got, out) == [], "step %d" % k
            assert (got["mNeighborCount"] > 254).sum() > 64 and out["touched"].sum() > N - 20
            pos, vel = got["mPosition"], got["mVelocity"]
    assert caps[0] == 254 and caps[-1] > 254, caps


# ---- off unit scale, unequal masses -----------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", scale_cases.FLAVOURS)
def test_off_unit_scale_against_the_restatement(oracle, hiplib, flavour):
    """scale_cases.block_scene (6 000 particles: a compressed block, a layer, a spray without neighbours) with the
    walls on: FULL against the restatement for two steps.  Under SHELL there are members beyond hscaled, whose
    Laplacian is negative."""
    import smoothed_particle_hydrodynamics_amd as S
    import sample_emulation as SE
    p, pos, vel, mass = scale_cases.block_scene(flavour, walls=True)
    assert not SE.unit_scale(p)
    mu = block_mu(p)
    n = mass.size
    with S.SPH(n, p) as sph:
        start(sph, pos, vel, mass, mu)
        for k in range(2):
            out = VE.step(oracle, p, pos, vel, mass, mu)
            sph.step()
            got = state_of(sph)
            assert against_step(got, out) == [], "step %d" % k
            assert 5000 < out["touched"].sum() < n                 # the spray's lone particles are left alone
            pos, vel = got["mPosition"], got["mVelocity"]


@pytest.mark.parametrize("with_law", [False, True])
@pytest.mark.parametrize("flavour", mass_cases.FLAVOURS)
def test_unequal_masses_against_the_restatement(oracle, hiplib, flavour, with_law):
    """mass_cases' block: the particle's own mass divides the sum, every volume carries its particle's mass.  Two FULL
    steps; a kernel that read the neighbour's mass for the particle's own would differ in nearly every row."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, T, _ = mass_cases.block(flavour)
    assert not mass_cases.uniform(mass)
    mu = block_mu(p)
    kappa = np.zeros(4, F32)
    law = laws()[2] if with_law else None
    with S.SPH(N, p) as sph:
        start(sph, pos, vel, mass)
        sph.setScalars(T, kappa)
        sph.setViscousStress(mu, law)
        for k in range(2):
            out = VE.step(oracle, p, pos, vel, mass, mu, VE.of(law), T=T, kappa=kappa)
            sph.step()
            got = state_of(sph)
            assert against_step(got, out) == [], "step %d" % k
            assert out["touched"].sum() > N - 20
            unit = VE.apply(p, mu, pos, vel, np.ones(N, F32), out["rho"], out["acc_before"], VE.of(law), T)[2]
            assert mass_cases.rows_differing(unit, out["c"]).sum() > 0.9 * N
            pos, vel = got["mPosition"], got["mVelocity"]


# ---- with a law ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keys", [2, 16])
def test_a_law_on_a_channel_that_changes_in_the_same_step(oracle, hiplib, keys):
    """The block's scalars with their diffusivities and sources: the law's channel diffuses and is driven in the very
    step that reads it.  The staged viscosities come from the channels as they stood BEFORE the step (Ts, what
    buoyancy reads); with the new ones the accelerations would differ.  Three FULL steps, then setScalars(None) drops the
    law and keeps mu."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, T, kappa = block_scene()
    sources = block_sources(p)
    mu = block_mu(p)
    law = laws()[keys]
    lw = VE.of(law)
    assert kappa[law.channel] > 0 or any(q.channel == law.channel for q in sources)
    with S.SPH(N, p) as sph:
        start(sph, pos, vel, mass)
        sph.setScalars(T, kappa)
        sph.setScalarSources(api_sources(sources))
        sph.setViscousStress(mu, law)
        assert sph.getViscousStress() == (mu, law)
        for k in range(3):
            out = VE.step(oracle, p, pos, vel, mass, mu, lw, T=T, kappa=kappa, sources=sources)
            sph.step()
            got = state_of(sph)
            assert against_step(got, out) == [], "step %d" % k
            assert same(sph.getScalars(), out["T"]), "step %d" % k
            assert out["touched"].sum() > N - 20
            # the law does act, and the channels of before the step are the ones it reads
            const = VE.apply(p, mu, pos, vel, mass, out["rho"], out["acc_before"])[0]
            late = VE.apply(p, mu, pos, vel, mass, out["rho"], out["acc_before"], lw, out["T"])[0]
            assert mass_cases.rows_differing(const.reshape(-1, 3), out["acc"].reshape(-1, 3)).sum() > 0.9 * N
            assert mass_cases.rows_differing(late.reshape(-1, 3), out["acc"].reshape(-1, 3)).sum() > 0.2 * N
            pos, vel, T = got["mPosition"], got["mVelocity"], out["T"]
        sph.setScalars(None)
        assert sph.getViscousStress() == (mu, None)                  # the law went with the scalars, mu stayed
        out = VE.step(oracle, p, pos, vel, mass, mu)
        sph.step()
        assert against_step(state_of(sph), out) == []


# ---- beside other features ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cohesive", [False, True])
@pytest.mark.parametrize("smoothing", [False, True])
@pytest.mark.parametrize("scalars", [False, True])
@pytest.mark.parametrize("buoyant", [False, True])
def test_beside_cohesion_xsph_scalars_and_buoyancy(oracle, hiplib, cohesive, smoothing, scalars, buoyant):
    """Every combination of the four settings beside the term: two FULL steps against the composed restatements -
    cohesion, the viscous stress (with a law where there are scalars), XSPH, then buoyancy.  Buoyancy without scalars
    does not exist: the setter refuses it, and the context steps as one without."""
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_buoyancy import block_buoyancy, emu_of
    p, pos, vel, mass, T, kappa = block_scene()
    sources = block_sources(p)
    buoyancy = block_buoyancy()
    b = emu_of(buoyancy, p) if buoyant and scalars else None
    gamma = GAMMA if cohesive else 0.0
    eps = EPS if smoothing else 0.0
    mu = block_mu(p)
    law = laws()[16] if scalars else None
    lw = VE.of(law)
    if not scalars:
        T = None
    with S.SPH(N, p) as sph:
        sph.setParticles(pos, vel, mass)
        if scalars:
            sph.setScalars(T, kappa)
            sph.setScalarSources(api_sources(sources))
        else:
            with pytest.raises(S.SphHipError, match="a viscosity law on a context without scalars"):
                sph.setViscousStress(mu, laws()[16])
        if buoyant and scalars:
            sph.setBuoyancy(buoyancy)
        elif buoyant:
            with pytest.raises(S.SphHipError):
                sph.setBuoyancy(buoyancy)
        if cohesive:
            sph.setCohesion(GAMMA)
        if smoothing:
            sph.setVelocitySmoothing(EPS)
        sph.setViscousStress(mu, law)
        args = (kappa if scalars else None, sources if scalars else (), b)
        for k in range(2):
            out = VE.step(oracle, p, pos, vel, mass, mu, lw, gamma, eps, T, *args)
            sph.step()
            got = state_of(sph)
            assert against_step(got, out) == [], "step %d" % k
            if scalars:
                assert same(sph.getScalars(), out["T"]), "step %d" % k
                T = out["T"]
            pos, vel = got["mPosition"], got["mVelocity"]
    # each of the settings did act
    both = VE.step(oracle, p, pos, vel, mass, mu, lw, gamma, eps, T, *args)
    assert not same(both["acc"], VE.step(oracle, p, pos, vel, mass, 0.0, None, gamma, eps, T, *args)["acc"])
    if cohesive:
        assert not same(both["acc"], VE.step(oracle, p, pos, vel, mass, mu, lw, 0.0, eps, T, *args)["acc"])
    if smoothing:
        assert not same(both["vel"], VE.step(oracle, p, pos, vel, mass, mu, lw, gamma, 0.0, T, *args)["vel"])
    if b is not None:
        assert not same(both["acc"], VE.step(oracle, p, pos, vel, mass, mu, lw, gamma, eps, T, args[0], args[1], None)["acc"])


def test_an_obstacle_on_a_path_a_load_recording_two_pressure_gauges_and_a_monitor_beside_the_term(oracle, hiplib):
    """Four single FULL steps of the block with a box on a sine path, a load recording, two pressure gauges and a
    monitor recording, every step against the restatements fed with the EMULATED state: viscous_emulation.step with
    path_emulation's integrate in place of the oracle's, pressure_emulation's readings in S_k, load_emulation's rows."""
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    p, pos, vel, mass = block()
    mu = block_mu(p)
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
        start(sph, pos, vel, mass, mu)
        sph.setObstacles(obst)                       # none of them is refused
        sph.setObstaclePaths(paths)
        sph.setGauges(gauges)
        sph.recordGauges(steps)
        sph.recordLoads(steps)
        sph.recordMonitor(steps)
        readings = []
        for k in range(steps):
            readings.append(PR.evaluate(p, pos, vel, mass, eg))
            out = VE.step(oracle, p, pos, vel, mass, mu, integrate=integrate_at(k))
            sph.step()
            assert against_step(state_of(sph), out) == [], "step %d" % k
            assert out["touched"].sum() > N - 20
            pos, vel = out["pos"], out["vel"]
        rec = sph.getGaugeRecord()
        loads = sph.getLoads()
        mon = sph.getMonitorRecord()
        assert sph.getViscousStress() == (mu, None)
    for r in range(steps):
        assert G.same_readings(G.Readings(rec.v[r], rec.n[r], rec.k[r]), readings[r]), "gauge row %d" % r
        assert rows[r].same(loads.impulse_q[r], loads.count[r], loads.skipped[r]), "load row %d" % r
    assert rec.n.min() > 0 and loads.count[:, L.WALLS].sum() > 0 and loads.count[:, :L.WALLS].sum() > 0
    assert len(mon.rows) == steps and (mon.rows["live"] == N).all() and (mon.rows["bad"] == 0).all()
    # the last row's peak acceleration is the state's: the monitor reads the total the term left in acc
    a = out["acc"].reshape(-1, 3)
    a2 = ((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]).astype(np.float64).max()
    assert abs(float(mon.rows["a2_max"][-1]) / a2 - 1.0) < 1e-6


# ---- a whole scene ---------------------------------------------------------------------------------------------------
def test_dam_break_viscous_100_queued_steps_equal_the_restatement(oracle, hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    p0 = scenes.dam_break_params(2000)[0]
    p, pos, vel, mass, mu = scenes.dam_break_viscous(2000, block_mu(p0))
    with S.SPH(mass.size, p) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setViscousStress(mu)
        assert sph.getViscousStress() == (float(F32(mu)), None)
        sph.run(100)
        got = state_of(sph)
    touched = []
    for _ in range(100):
        out = VE.step(oracle, p, pos, vel, mass, mu)
        touched.append(int(out["touched"].sum()))
        pos, vel = out["pos"], out["vel"]
    assert against_step(got, out) == []
    # the first step of the uniform surge stores nothing; the broken dam's velocity differences are damped
    assert touched[0] == 0 and touched[-1] > mass.size - 20 and np.isfinite(out["pos"]).all()


# ---- refusals, the getter, an upload ------------------------------------------------------------------------------------
def test_refusals_getter_and_what_drops_the_setting(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import ViscosityLaw, scenes
    from smoothed_particle_hydrodynamics_amd.ports import Sink
    from smoothed_particle_hydrodynamics_amd.slab import HipSlab
    p, pos, vel, mass, T, kappa = block_scene()
    law = laws()[2]

    def refused(call, *args, text):
        with pytest.raises(S.SphHipError) as e:
            call(*args)
        assert text in str(e.value), str(e.value)

    with S.SPH(N, p) as sph:
        sph.setParticles(pos, vel, mass)
        assert sph.getViscousStress() == (0.0, None)
        sph.setViscousStress(0.25)
        assert sph.getViscousStress() == (0.25, None)
        for bad in (np.nan, np.inf, -np.inf):
            refused(sph.setViscousStress, bad, text="a viscosity that is not finite")
        for bad in (-0.25, -1e-30):
            refused(sph.setViscousStress, bad, text="a negative viscosity")
        refused(sph.setViscousStress, 0.5, law, text="a viscosity law on a context without scalars")
        assert sph.getViscousStress() == (0.25, None)              # a refused call keeps what is set
        sph.setScalars(T, kappa)
        for bad, text in ((ViscosityLaw(4, [0.0, 1.0], [1.0, 1.0]), "a law channel outside 0..3"),
                          (ViscosityLaw(-1, [0.0, 1.0], [1.0, 1.0]), "a law channel outside 0..3"),
                          (ViscosityLaw(0, [0.0], [1.0]), "a law with fewer than 2 or more than 16 keys"),
                          (ViscosityLaw(0, [0.0, np.inf], [1.0, 1.0]), "a key value that is not finite"),
                          (ViscosityLaw(0, [0.0, 0.0], [1.0, 1.0]), "key values that are not strictly ascending"),
                          (ViscosityLaw(0, [1.0, 0.0], [1.0, 1.0]), "key values that are not strictly ascending"),
                          (ViscosityLaw(0, [0.0, 1.0], [1.0, np.nan]), "a key factor that is not finite"),
                          (ViscosityLaw(0, [0.0, 1.0], [-1.0, 1.0]), "a negative key factor")):
            refused(sph.setViscousStress, 0.5, bad, text=text)
        assert sph.getViscousStress() == (0.25, None)
        sph.setViscousStress(0.5, law)
        assert sph.getViscousStress() == (0.5, law)
        sph.step()
        assert sph.getViscousStress() == (0.5, law)
        sph.setViscousStress(0.125)                            # no law given: a constant mu again
        assert sph.getViscousStress() == (0.125, None)
        sph.setViscousStress(None, law)                        # None and 0 switch it off, law and all
        assert sph.getViscousStress() == (0.0, None)
        sph.setViscousStress(0.125, law)
        sph.setViscousStress(-0.0)
        mu, none = sph.getViscousStress()
        assert mu == 0.0 and not np.signbit(mu) and none is None
        # the outputs of the C call are optional, one by one
        sph.setViscousStress(0.75, law)
        m, have = C.c_float(0.0), C.c_int(0)
        sph.call("sph_hip_get_viscous_stress", C.byref(m), None, None)
        sph.call("sph_hip_get_viscous_stress", None, None, C.byref(have))
        assert (m.value, have.value) == (0.75, 1)
        # ports both ways
        sink = Sink((0.9, 0.9, 0.9), (1.0, 1.0, 1.0))
        sph.setScalars(None)                                   # (scalars and ports exclude each other)
        assert sph.getViscousStress() == (0.75, None)
        sph.setViscousStress(0.0)
        sph.setPorts([], [sink])
        refused(sph.setViscousStress, 0.25, text="a context with ports cannot have viscous stress")
        sph.setViscousStress(0.0)                              # off is never refused
        sph.setPorts([], [])
        sph.setViscousStress(0.25)
        refused(sph.setPorts, [], [sink], text="a context with viscous stress cannot have ports")
        sph.setPorts([], [])                                   # (clearing ports is no port)
        assert sph.getViscousStress() == (0.25, None)
        sph.setParticles(pos, vel, mass)                       # an upload drops it
        assert sph.getViscousStress() == (0.0, None)
        sph.step()                                             # and a step launches nothing for it
    # REF mode
    rp, rpos, rvel, rmass = scenes.dense_block(512)
    with S.SPH(512, rp, mode=S.MODE_REF) as sph:
        sph.setParticles(rpos, rvel, rmass)
        refused(sph.setViscousStress, 0.25, text="FULL and FULL_FAST contexts only")
        sph.setViscousStress(0.0)
        assert sph.getViscousStress() == (0.0, None)
    # a slab context
    with HipSlab(p, 0, p.full_cells_z // 2, 4096, 1024, has_left=False) as slab:
        with pytest.raises(S.SphHipError, match="slab contexts"):
            slab.call("sph_hip_set_viscous_stress", C.c_float(0.25), None)
        slab.call("sph_hip_set_viscous_stress", C.c_float(0.0), None)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    np.savez(sys.argv[2], **route_run(sys.argv[1]))
