"""GPU: the implicit viscous stress (include/sph_hip.h: implicit viscous stress).  k_viscous_stage and K launches of
k_viscous_sweep between the acceleration pass and the integrate, against the numpy restatement
tests/viscous_implicit_emulation.py composed with the oracle's phases, bit for bit, on the scalars' 2 001-particle block
(eight workgroups, the last with one live lane; seeded velocities, gravity and walls on) at a mu five times the bulk's
explicit limit.  The routes are set by switches that are read at context creation, so each runs in a child process of
its own (this file with a route name)."""
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
import viscous_implicit_emulation as VI
from helpers import to_oracle_params
from test_gpu_cohesion import ROUTES, ROUTE_SWITCHES, STATE, against_step, block, same_state, state_of
from test_gpu_scalars import N, api_sources, bits, block_scene, block_sources, mode_of, same

pytestmark = pytest.mark.gpu

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GAMMA = 0.02        # test_gpu_cohesion's
EPS = 0.5           # test_gpu_xsph's


def block_mu(p, fraction=5.0):
    """five times the bulk's explicit limit (scenes.viscous_stable_mu), as fp32: what the mode is for"""
    from smoothed_particle_hydrodynamics_amd import scenes
    return float(F32(scenes.viscous_stable_mu(p, fraction)))


def law16():
    """16 keys on channel 2 (it diffuses, and an ADD acts on it); the block's channels are seeded in [-1, 1)"""
    from smoothed_particle_hydrodynamics_amd import ViscosityLaw
    return ViscosityLaw.exponential(2, 0.0, 1.5, -0.75, 0.75)


def start(sph, pos, vel, mass, mu=None, sweeps=None, law=None):
    sph.setParticles(pos, vel, mass)
    if mu is not None:
        sph.setViscousStress(mu, law)
    if sweeps is not None:
        sph.setViscousSolver(sweeps)


def rows_differing(a, b):
    return (bits(a) != bits(b)).reshape(-1, 3).any(1).sum()


# ---- FULL single steps against the restatement -------------------------------------------------------------------
@pytest.mark.parametrize("sweeps", [1, 2, 3, 64])
def test_full_single_steps_equal_the_restatement(oracle, hiplib, sweeps):
    """Odd and even counts: the last sweep reads either row set.  Positions, velocities, accelerations and densities."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    mu = block_mu(p)
    with S.SPH(N, p) as sph:
        start(sph, pos, vel, mass, mu, sweeps)
        assert sph.getViscousSolver() == sweeps and sph.getViscousStress() == (mu, None)
        for k in range(2):
            out = VI.step(oracle, p, pos, vel, mass, mu, sweeps)
            sph.step()
            got = state_of(sph)
            assert against_step(got, out) == [], "step %d" % k
            assert out["touched"].sum() > N - 20                              # nearly every particle is touched
            # neither the explicit step nor the plain one
            explicit = VE.step(oracle, p, pos, vel, mass, mu)
            plain = VE.step(oracle, p, pos, vel, mass, 0.0)
            assert rows_differing(explicit["vel"], out["vel"]) > N - 20 and rows_differing(plain["vel"], out["vel"]) > N - 20
            assert same(out["acc"], plain["acc"]) and not same(out["acc"], explicit["acc"])     # acc is not touched
            pos, vel = got["mPosition"], got["mVelocity"]
        stats = sph.tileStats()
        assert stats["workgroups"] == 8 and stats["untiled_density"] == 0          # the list route


# ---- FULL_FAST: solve() on the twin's densities ---------------------------------------------------------------------
def test_fast_velocities_are_solve_on_the_twins_state(oracle, hiplib):
    """A FULL_FAST twin without the term, stepped from the same S_k, yields the step's densities and accelerations; the
    implicit context's accelerations are the twin's by bits, and its new velocities and positions the oracle's
    integrate from solve()'s velocities.  Two states: the block, and what the implicit context made of it."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    mu = block_mu(p)
    op = to_oracle_params(p)
    for k in range(2):
        with S.SPH(N, p, mode=S.MODE_FULL_FAST) as twin, S.SPH(N, p, mode=S.MODE_FULL_FAST) as sph:
            start(twin, pos, vel, mass)
            start(sph, pos, vel, mass, mu, 3)
            twin.step()
            sph.step()
            t, got = state_of(twin), state_of(sph)
            assert same(got["mDensity"], t["mDensity"]) and np.array_equal(got["mNeighborCount"], t["mNeighborCount"])
            assert same(got["mAcceleration"], t["mAcceleration"]), "state %d" % k
            v1, on = VI.solve(p, mu, pos, vel, mass, t["mDensity"], 3)
            assert on.sum() > N - 20 and rows_differing(v1, vel) > N - 20
            x1, w1 = pos.copy(), v1.copy()
            oracle.integrate(op, x1, w1, t["mAcceleration"].copy(), mass)
            assert same(got["mVelocity"], w1) and same(got["mPosition"], x1), "state %d" % k
            assert not same(w1, t["mVelocity"])
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
            start(sph, pos, vel, mass, mu, 4)
            if queued:
                sph.run(5)
            else:
                for _ in range(5):
                    sph.step()
            out.append((state_of(sph), sph.energy()))
    assert same_state(out[0][0], out[1][0]) == [] and out[0][1] == out[1][1]
    with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
        start(sph, pos, vel, mass, mu)
        sph.run(5)
        assert not same(sph.getParticles().mVelocity, out[0][0]["mVelocity"])      # (not the explicit term)


def test_a_setter_between_queued_steps_does_not_reach_them(oracle, hiplib):
    """The count travels by value: run(2) explicitly, 4 sweeps, run(2), 0 again, run(1) - the restatement with the
    settings in that order."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    mu = block_mu(p, 0.1)                       # (inside the explicit range: the explicit steps stay tame)
    with S.SPH(N, p) as sph:
        start(sph, pos, vel, mass, mu, 0)
        sph.run(2)
        sph.setViscousSolver(4)
        sph.run(2)
        sph.setViscousSolver(0)
        sph.run(1)
        got = state_of(sph)
    for sweeps in (0, 0, 4, 4, 0):
        out = VI.step(oracle, p, pos, vel, mass, mu, sweeps)
        pos, vel = out["pos"], out["vel"]
    assert against_step(got, out) == []


# ---- with a law ------------------------------------------------------------------------------------------------------
def test_a_law_on_a_channel_that_changes_in_the_same_step(oracle, hiplib):
    """The block's scalars with their diffusivities and sources: the 16-key law's channel diffuses and is driven in the
    very step that reads it.  The staged viscosities come from the channels as they stood BEFORE the step.  Three
    FULL steps, then setScalars(None) drops the law and keeps mu and the count."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, T, kappa = block_scene()
    sources = block_sources(p)
    mu = block_mu(p)
    law = law16()
    lw = VE.of(law)
    assert kappa[law.channel] > 0 and any(q.channel == law.channel for q in sources)
    with S.SPH(N, p) as sph:
        start(sph, pos, vel, mass)
        sph.setScalars(T, kappa)
        sph.setScalarSources(api_sources(sources))
        sph.setViscousStress(mu, law)
        sph.setViscousSolver(3)
        for k in range(3):
            out = VI.step(oracle, p, pos, vel, mass, mu, 3, lw, T=T, kappa=kappa, sources=sources)
            sph.step()
            got = state_of(sph)
            assert against_step(got, out) == [], "step %d" % k
            assert same(sph.getScalars(), out["T"]), "step %d" % k
            assert out["touched"].sum() > N - 20
            # the law does act, and the channels of before the step are the ones it reads
            const = VI.step(oracle, p, pos, vel, mass, mu, 3, None, T=T, kappa=kappa, sources=sources)
            late = VI.solve(p, mu, pos, vel, mass, out["rho"], 3, lw, out["T"])[0]
            mine = VI.solve(p, mu, pos, vel, mass, out["rho"], 3, lw, T)[0]
            assert rows_differing(const["vel"], out["vel"]) > 0.9 * N and rows_differing(late, mine) > 0.2 * N
            pos, vel, T = got["mPosition"], got["mVelocity"], out["T"]
        sph.setScalars(None)
        assert sph.getViscousStress() == (mu, None) and sph.getViscousSolver() == 3
        out = VI.step(oracle, p, pos, vel, mass, mu, 3)
        sph.step()
        assert against_step(state_of(sph), out) == []


# ---- off ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["full", "fast"])
def test_zero_none_and_never_set_equal_the_explicit_step(hiplib, mode):
    """sweeps = 0, None and "never set" over 20 steps: byte for byte the explicit context's state, counts and
    energies - also where a count was set and taken back."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    mu = block_mu(p, 0.1)
    out = []
    for setting in ("never", None, 0, "back"):
        with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
            start(sph, pos, vel, mass, mu)
            if setting == "back":
                sph.setViscousSolver(5)
                sph.setViscousSolver(0)
            elif setting != "never":
                sph.setViscousSolver(setting)
            assert sph.getViscousSolver() == 0
            sph.run(19)
            sph.step()
            st = state_of(sph)
            out.append([st[nm] for nm in STATE + ("mNeighborCount",)] + list(sph.energy()))
    for other in out[1:]:
        for a, c in zip(out[0], other):
            assert np.asarray(a).tobytes() == np.asarray(c).tobytes()


@pytest.mark.parametrize("mode", ["full", "fast"])
def test_a_count_without_a_viscosity_equals_a_plain_context(hiplib, mode):
    """mu = 0 with sweeps = 8: nothing is launched, 20 steps equal a plain context's byte for byte."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    out = []
    for sweeps in (None, 8):
        with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
            start(sph, pos, vel, mass, 0.0 if sweeps else None, sweeps)
            assert sph.getViscousSolver() == (sweeps or 0) and sph.getViscousStress() == (0.0, None)
            sph.run(19)
            sph.step()
            st = state_of(sph)
            out.append([st[nm] for nm in STATE + ("mNeighborCount",)] + list(sph.energy()))
    for a, c in zip(out[0], out[1]):
        assert np.asarray(a).tobytes() == np.asarray(c).tobytes()


# ---- routes: one child process per setting ---------------------------------------------------------------------------
def route_run(route="default"):
    """FULL and FULL_FAST: the state after one step of the block with two sweeps, and the tile statistics"""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    mu = block_mu(p)
    result, stats = {}, {}
    for mode in ("full", "fast"):
        with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
            start(sph, pos, vel, mass, mu, 2)
            sph.step()
            st = state_of(sph)
            for nm in STATE:
                result[mode + nm] = st[nm]
            result[mode + "_counts"] = st["mNeighborCount"]
            stats[mode] = sph.tileStats() if route != "untiled" else {}
    result["stats"] = json.dumps(stats)
    return result


@pytest.mark.parametrize("route", list(ROUTES))
def test_every_route_gives_the_restatements_bits(oracle, route, tmp_path):
    assert sorted(ROUTES) == ["default", "lists_none", "lists_some", "no_fused_integrate", "untiled", "wide"]
    env = {k: v for k, v in os.environ.items() if k not in ROUTE_SWITCHES}
    env.update(ROUTES[route])
    out_path = str(tmp_path / "route.npz")
    run = subprocess.run([sys.executable, os.path.abspath(__file__), route, out_path], env=env, capture_output=True,
                         text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    got = np.load(out_path)
    p, pos, vel, mass = block()
    mu = block_mu(p)
    out = VI.step(oracle, p, pos, vel, mass, mu, 2)
    assert out["touched"].sum() > N - 20
    for nm, key in (("mPosition", "pos"), ("mVelocity", "vel"), ("mAcceleration", "acc"), ("mDensity", "rho")):
        assert same(got["full" + nm], out[key]), (route, nm)
    # FULL_FAST: the same velocities in front of the integrate - solve() on its own densities gives what it integrated
    v1, _ = VI.solve(p, mu, pos, vel, mass, got["fastmDensity"], 2)
    x1, w1 = pos.copy(), v1.copy()
    oracle.integrate(to_oracle_params(p), x1, w1, got["fastmAcceleration"].copy(), mass)
    assert same(got["fastmVelocity"], w1) and same(got["fastmPosition"], x1), route
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
    out = VI.step(oracle, p, pos, vel, mass, mu, 4)
    assert not out["touched"].any() and out["rho"][0] == 0          # (its staged volume is 0: it is left alone)
    states = []
    for setting in (mu, None):
        with S.SPH(1, p) as sph:
            start(sph, pos, vel, mass, setting, 4)
            sph.step()
            states.append(state_of(sph))
            sph.run(3)
            states.append(state_of(sph))
    assert against_step(states[0], out) == []
    assert same_state(states[0], states[2]) == [] and same_state(states[1], states[3]) == []


@pytest.mark.parametrize("sweeps", [1, 4])
def test_two_particles_of_masses_one_and_three(oracle, hiplib, sweeps):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = tiny(2)
    mu = block_mu(p)
    with S.SPH(2, p) as sph:
        start(sph, pos, vel, mass, mu, sweeps)
        for k in range(3):
            out = VI.step(oracle, p, pos, vel, mass, mu, sweeps)
            sph.step()
            got = state_of(sph)
            assert against_step(got, out) == [], "step %d" % k
            assert out["touched"].all() and (got["mNeighborCount"] == 1).all()
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
        start(sph, pos, vel, mass, mu, 3)
        for k in range(3):
            out = VI.step(oracle, p, pos, vel, mass, mu, 3)
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
    mu = block_mu(p)
    rng = np.random.default_rng(5)
    x = pos.reshape(-1, 3).copy()
    x[:400] = np.array([0.05, 0.3, 0.5], F32) + rng.uniform(-0.2, 0.2, (400, 3)).astype(F32) * F32(p.h)
    pos = np.ascontiguousarray(x.reshape(-1))
    with S.SPH(N, p) as sph:
        start(sph, pos, vel, mass, mu, 2)
        caps = []
        for k in range(4):
            out = VI.step(oracle, p, pos, vel, mass, mu, 2)
            sph.step()
            got = state_of(sph)
            caps.append(sph.tileStats()["list_capacity"])
            assert against_step(got, out) == [], "step %d" % k
            assert (got["mNeighborCount"] > 254).sum() > 64 and out["touched"].sum() > N - 20
            pos, vel = got["mPosition"], got["mVelocity"]
    assert caps[0] == 254 and caps[-1] > 254, caps


# ---- off unit scale, unequal masses -----------------------------------------------------------------------------------
def test_scaled_against_the_restatement(oracle, hiplib):
    """scale_cases.block_scene (6 000 particles: a compressed block, a layer, a spray without neighbours) with the
    walls on and sim_scale = 0.5: FULL against the restatement for two steps."""
    import smoothed_particle_hydrodynamics_amd as S
    import sample_emulation as SE
    p, pos, vel, mass = scale_cases.block_scene("SCALED", walls=True)
    assert not SE.unit_scale(p)
    mu = block_mu(p)
    n = mass.size
    with S.SPH(n, p) as sph:
        start(sph, pos, vel, mass, mu, 3)
        for k in range(2):
            out = VI.step(oracle, p, pos, vel, mass, mu, 3)
            sph.step()
            got = state_of(sph)
            assert against_step(got, out) == [], "step %d" % k
            assert 5000 < out["touched"].sum() < n                 # the spray's lone particles are left alone
            pos, vel = got["mPosition"], got["mVelocity"]


@pytest.mark.parametrize("flavour", ["SPREAD", "TWO_SPECIES"])
def test_unequal_masses_against_the_restatement(oracle, hiplib, flavour):
    """mass_cases' block: the particle's own mass stands in den, every volume carries its particle's mass.  Two FULL
    steps; a kernel that read the neighbour's mass for the particle's own would differ in nearly every row."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, _, _ = mass_cases.block(flavour)
    assert not mass_cases.uniform(mass)
    mu = block_mu(p)
    with S.SPH(N, p) as sph:
        start(sph, pos, vel, mass, mu, 3)
        for k in range(2):
            out = VI.step(oracle, p, pos, vel, mass, mu, 3)
            sph.step()
            got = state_of(sph)
            assert against_step(got, out) == [], "step %d" % k
            assert out["touched"].sum() > N - 20
            unit = VI.solve(p, mu, pos, vel, np.ones(N, F32), out["rho"], 3)[0]
            mine = VI.solve(p, mu, pos, vel, mass, out["rho"], 3)[0]
            assert rows_differing(unit, mine) > 0.9 * N
            pos, vel = got["mPosition"], got["mVelocity"]


# ---- beside other features ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cohesive", [False, True])
@pytest.mark.parametrize("smoothing", [False, True])
@pytest.mark.parametrize("scalars", [False, True])
@pytest.mark.parametrize("buoyant", [False, True])
def test_beside_cohesion_xsph_scalars_and_buoyancy(oracle, hiplib, cohesive, smoothing, scalars, buoyant):
    """Every combination of the four settings beside the mode: two FULL steps against the composed restatements -
    cohesion, the sweeps (with a law where there are scalars), XSPH on the velocities they left, then buoyancy.
    Buoyancy without scalars does not exist: the setter refuses it, and the context steps as one without."""
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_buoyancy import block_buoyancy, emu_of
    p, pos, vel, mass, T, kappa = block_scene()
    sources = block_sources(p)
    buoyancy = block_buoyancy()
    b = emu_of(buoyancy, p) if buoyant and scalars else None
    gamma = GAMMA if cohesive else 0.0
    eps = EPS if smoothing else 0.0
    mu = block_mu(p)
    law = law16() if scalars else None
    lw = VE.of(law)
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
        if smoothing:
            sph.setVelocitySmoothing(EPS)
        sph.setViscousSolver(2)                       # (the count may come first: it waits for a mu)
        sph.setViscousStress(mu, law)
        args = (kappa if scalars else None, sources if scalars else (), b)
        for k in range(2):
            out = VI.step(oracle, p, pos, vel, mass, mu, 2, lw, gamma, eps, T, *args)
            sph.step()
            got = state_of(sph)
            assert against_step(got, out) == [], "step %d" % k
            if scalars:
                assert same(sph.getScalars(), out["T"]), "step %d" % k
                T = out["T"]
            pos, vel = got["mPosition"], got["mVelocity"]
    # each of the settings did act
    both = VI.step(oracle, p, pos, vel, mass, mu, 2, lw, gamma, eps, T, *args)
    assert not same(both["vel"], VI.step(oracle, p, pos, vel, mass, 0.0, 2, None, gamma, eps, T, *args)["vel"])
    assert not same(both["vel"], VI.step(oracle, p, pos, vel, mass, mu, 0, lw, gamma, eps, T, *args)["vel"])
    if cohesive:
        assert not same(both["acc"], VI.step(oracle, p, pos, vel, mass, mu, 2, lw, 0.0, eps, T, *args)["acc"])
    if smoothing:
        assert not same(both["vel"], VI.step(oracle, p, pos, vel, mass, mu, 2, lw, gamma, 0.0, T, *args)["vel"])
    if b is not None:
        assert not same(both["acc"], VI.step(oracle, p, pos, vel, mass, mu, 2, lw, gamma, eps, T, args[0], args[1], None)["acc"])


def test_an_obstacle_on_a_path_a_load_recording_two_pressure_gauges_and_a_monitor_beside_the_mode(oracle, hiplib):
    """Four single FULL steps of the block with a box on a sine path, a load recording, two pressure gauges and a
    monitor recording, every step against the restatements fed with the EMULATED state: the composed step with
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
        start(sph, pos, vel, mass, mu, 3)
        sph.setObstacles(obst)                       # none of them is refused
        sph.setObstaclePaths(paths)
        sph.setGauges(gauges)
        sph.recordGauges(steps)
        sph.recordLoads(steps)
        sph.recordMonitor(steps)
        readings = []
        for k in range(steps):
            readings.append(PR.evaluate(p, pos, vel, mass, eg))
            out = VI.step(oracle, p, pos, vel, mass, mu, 3, integrate=integrate_at(k))
            sph.step()
            assert against_step(state_of(sph), out) == [], "step %d" % k
            assert out["touched"].sum() > N - 20
            pos, vel = out["pos"], out["vel"]
        rec = sph.getGaugeRecord()
        loads = sph.getLoads()
        mon = sph.getMonitorRecord()
        assert sph.getViscousStress() == (mu, None) and sph.getViscousSolver() == 3
    for r in range(steps):
        assert G.same_readings(G.Readings(rec.v[r], rec.n[r], rec.k[r]), readings[r]), "gauge row %d" % r
        assert rows[r].same(loads.impulse_q[r], loads.count[r], loads.skipped[r]), "load row %d" % r
    assert rec.n.min() > 0 and loads.count[:, L.WALLS].sum() > 0 and loads.count[:, :L.WALLS].sum() > 0
    assert len(mon.rows) == steps and (mon.rows["live"] == N).all() and (mon.rows["bad"] == 0).all()


# ---- a whole scene ---------------------------------------------------------------------------------------------------
def test_dam_break_honey_100_queued_steps_equal_the_restatement(oracle, hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass, mu, sweeps = scenes.dam_break_honey(2000)
    assert sweeps == 8 and abs(scenes.viscous_number(p, mu) - 5.0) < 1e-9
    with S.SPH(mass.size, p) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setViscousStress(mu)
        sph.setViscousSolver(sweeps)
        assert sph.getViscousStress() == (float(F32(mu)), None) and sph.getViscousSolver() == 8
        sph.run(100)
        got = state_of(sph)
    touched = []
    for _ in range(100):
        out = VI.step(oracle, p, pos, vel, mass, mu, sweeps)
        touched.append(int(out["touched"].sum()))
        pos, vel = out["pos"], out["vel"]
    assert against_step(got, out) == []
    # the first step of the uniform surge stores nothing; the broken dam's velocity differences are damped
    assert touched[0] == 0 and touched[-1] > mass.size - 20 and np.isfinite(out["pos"]).all()


# ---- refusals, the getter, an upload ------------------------------------------------------------------------------------
def test_refusals_getter_and_what_drops_the_count(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    from smoothed_particle_hydrodynamics_amd.ports import Sink
    from smoothed_particle_hydrodynamics_amd.slab import HipSlab
    p, pos, vel, mass, T, kappa = block_scene()

    def refused(call, *args, text):
        with pytest.raises(S.SphHipError) as e:
            call(*args)
        assert text in str(e.value), str(e.value)

    with S.SPH(N, p) as sph:
        sph.setParticles(pos, vel, mass)
        assert sph.getViscousSolver() == 0
        sph.setViscousSolver(8)                                 # without a mu: kept, and nothing is launched for it
        assert sph.getViscousSolver() == 8 and sph.getViscousStress() == (0.0, None)
        for bad in (-1, 65, 1000):
            refused(sph.setViscousSolver, bad, text="a sweep count outside 0..64")
        assert sph.getViscousSolver() == 8                      # a refused call keeps what is set
        for ok in (64, 1, 0, None, 2):
            sph.setViscousSolver(ok)
            assert sph.getViscousSolver() == (ok or 0)
        sph.setViscousStress(0.25)
        assert sph.getViscousSolver() == 2                      # the explicit setter does not touch the count
        sph.setViscousStress(0.0)
        assert sph.getViscousSolver() == 2
        refused(sph.call, "sph_hip_get_viscous_implicit", None, text="null output")
        # setScalars(None) keeps it
        sph.setScalars(T, kappa)
        sph.setScalars(None)
        assert sph.getViscousSolver() == 2
        # ports both ways
        sink = Sink((0.9, 0.9, 0.9), (1.0, 1.0, 1.0))
        refused(sph.setPorts, [], [sink], text="a context with an implicit viscous solver cannot have ports")
        sph.setViscousSolver(0)
        sph.setPorts([], [sink])
        refused(sph.setViscousSolver, 4, text="a context with ports cannot have an implicit viscous solver")
        sph.setViscousSolver(0)                                 # 0 is never refused
        sph.setPorts([], [])
        sph.setViscousSolver(4)
        sph.setPorts([], [])                                    # (clearing ports is no port)
        sph.setViscousStress(0.25)
        sph.setParticles(pos, vel, mass)                        # an upload drops the count with the rest
        assert sph.getViscousSolver() == 0 and sph.getViscousStress() == (0.0, None)
        sph.step()                                              # and a step launches nothing for it
    # REF mode
    rp, rpos, rvel, rmass = scenes.dense_block(512)
    with S.SPH(512, rp, mode=S.MODE_REF) as sph:
        sph.setParticles(rpos, rvel, rmass)
        refused(sph.setViscousSolver, 4, text="FULL and FULL_FAST contexts only")
        refused(sph.setViscousSolver, 99, text="a sweep count outside 0..64")      # the range is looked at first
        sph.setViscousSolver(0)
        assert sph.getViscousSolver() == 0
    # a slab context
    with HipSlab(p, 0, p.full_cells_z // 2, 4096, 1024, has_left=False) as slab:
        with pytest.raises(S.SphHipError, match="slab contexts .* cannot have an implicit viscous solver"):
            slab.call("sph_hip_set_viscous_implicit", C.c_int(4))
        slab.call("sph_hip_set_viscous_implicit", C.c_int(0))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    np.savez(sys.argv[2], **route_run(sys.argv[1]))
