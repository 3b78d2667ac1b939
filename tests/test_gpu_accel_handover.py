"""GPU: the single-context acceleration launch walks each XCD's share of the workgroups from the top
down (csrc/launch_policy.h: xcd_workgroup_descending; csrc/full_tiled.h: accel_part_workgroup), the
density pass from the bottom up.  The mapping is a placement only: every sum per particle, the
energy partial sums (indexed by workgroup) and the next build's counts must stay what they were.

What can go wrong is a grid size at which the descending walk is no bijection or leaves its share
(a workgroup computed twice is integrated and counted twice, one left out keeps stale state), so
the scenes are dam columns of 1, 7, 8, 9 and 65 workgroups - fewer than the XCDs, one less, as
many, one more, and shares of unequal size - two steps each, so that the second step's cell build
runs on the keys, slots and counts the first step's acceleration pass wrote.

Exact mode: positions, velocities, densities, accelerations and neighbour counts equal the oracle
bit for bit.  The energies: the device sums fp64 partial sums in a fixed order and the oracle fp32
terms serially, so they are held to check_energy's bar against the oracle (tests/helpers.py) and
BIT FOR BIT against the same context with the separate integrate kernel
(SPH_HIP_NO_FUSED_INTEGRATE=1), whose partial sums are the same ones and whose workgroups do not go
through the acceleration pass's mapping.
Tolerance mode: the bar of tests/test_gpu_full_fast.py (check_fast, strict: counts and densities
equal to the exact arithmetic's, every force within 1e-4 relative), each step from the state the
GPU started it from.

One scene has gravity and the walls on and a clump whose particles have more neighbours than a
list holds: its workgroups are flagged LISTS_SOME and their marker lanes walk the tile.  That the
clump is there is asserted on the oracle's counts before the GPU runs.
"""
import numpy as np
import pytest

from helpers import check_energy, to_oracle_params
from test_gpu_full_fast import check_fast, check_fast_position, check_fast_velocity
from test_gpu_full_mode import check_state

pytestmark = pytest.mark.gpu

NLIST_CAP = 254          # csrc/neighbor_lists.h: the list capacity a context starts with
WORKGROUPS = (1, 7, 8, 9, 65)
STEPS = 2
ROUTE_VARS = ("SPH_HIP_UNTILED", "SPH_HIP_TILE_CAP", "SPH_HIP_TILE_CAP_ACCEL", "SPH_HIP_TILE_CAP_DENSITY",
              "SPH_HIP_LIST_CAP", "SPH_HIP_CHUNKED", "SPH_HIP_NO_FUSED_INTEGRATE")
FIELDS = ("mPosition", "mVelocity", "mDensity", "mAcceleration", "mNeighborCount")


def column(wgs):
    from smoothed_particle_hydrodynamics_amd import scenes
    return scenes.dam_break(256 * wgs, seed=42, speed=0.05)


def clump_under_gravity():
    """9 workgroups of the moving column, gravity along -y and the walls on, 300 of its particles
    moved to within h / 2 of one point: each of them has more neighbours than a list holds"""
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = column(9)
    p.apply_gravity = 1
    p.apply_walls = 1
    p.gravity[0], p.gravity[1], p.gravity[2] = 0.0, -9.81, 0.0
    P = pos.reshape(-1, 3).copy()
    u = scenes.box_fill(300, (-1.0,) * 3, (1.0,) * 3, seed=9).reshape(-1, 3)
    P[1000:1300] = np.float32([0.05, 0.4, 0.5]) + np.float32(0.49 / np.sqrt(3.0)) * np.float32(p.h) * u
    return p, np.ascontiguousarray(P.reshape(-1)), vel, mass


def clump_precondition(ref):
    without = ref["ncount"] > NLIST_CAP
    assert without.sum() >= 300 and ref["ncount"].max() <= 1022, (int(without.sum()), int(ref["ncount"].max()))
    assert np.isfinite(ref["acc"]).all()


SCENES = [pytest.param(lambda w=w: column(w), w, None, id="%d-workgroups" % w) for w in WORKGROUPS]
SCENES.append(pytest.param(clump_under_gravity, 9, clump_precondition, id="gravity-walls-clump"))


def clean_env(monkeypatch):
    for k in ROUTE_VARS:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("make,wgs,precondition", SCENES)
def test_exact_mode_equals_the_oracle(oracle, hiplib, monkeypatch, make, wgs, precondition):
    import smoothed_particle_hydrodynamics_amd as S
    clean_env(monkeypatch)
    p, pos, vel, mass = make()
    assert mass.size == 256 * wgs
    op = to_oracle_params(p)
    opos, ovel = pos.copy(), vel.copy()
    fused = []
    with S.SPH(mass.size, p, mode=S.MODE_FULL) as sph:
        sph.setParticles(pos, vel, mass)
        for s in range(STEPS):
            ref = oracle.step(op, opos, ovel, mass, mode="full")
            if s == 0 and precondition is not None:
                precondition(ref)
            sph.step()
            part = sph.getParticles()
            if s == 0:
                ts = sph.tileStats()
                assert ts["workgroups"] == wgs, ts
            check_state(part, ref, "step %d" % s)
            assert np.array_equal(part.mPosition, opos), "step %d position" % s
            assert np.array_equal(part.mVelocity, ovel), "step %d velocity" % s
            energy = sph.energy()
            check_energy(energy, (ref["ke"], ref["pe"]), part.mVelocity, mass)
            fused.append([getattr(part, k).copy() for k in FIELDS] + [np.array(energy)])
        assert sph.getGrid().sum() == mass.size
    # the separate integrate kernel: the same partial sums, none of them by a mapped workgroup
    monkeypatch.setenv("SPH_HIP_NO_FUSED_INTEGRATE", "1")
    with S.SPH(mass.size, p, mode=S.MODE_FULL) as sph:
        sph.setParticles(pos, vel, mass)
        for s in range(STEPS):
            sph.step()
            part = sph.getParticles()
            separate = [getattr(part, k) for k in FIELDS] + [np.array(sph.energy())]
            for name, a, b in zip(FIELDS + ("energy",), fused[s], separate):
                assert np.array_equal(a, b), "step %d: %s differs from the separate integrate kernel's" % (s, name)


@pytest.mark.parametrize("make,wgs,precondition", SCENES)
def test_tolerance_mode_meets_its_bar(oracle, hiplib, monkeypatch, make, wgs, precondition):
    import smoothed_particle_hydrodynamics_amd as S
    clean_env(monkeypatch)
    p, pos, vel, mass = make()
    op = to_oracle_params(p)
    with S.SPH(mass.size, p, mode=S.MODE_FULL_FAST) as sph:
        assert sph.getArithmetic() == S.ARITH_FAST
        sph.setParticles(pos, vel, mass)
        cur_pos, cur_vel = pos.copy(), vel.copy()
        for s in range(STEPS):
            opos, ovel = cur_pos.copy(), cur_vel.copy()
            ref = oracle.step(op, opos, ovel, mass, mode="full")
            if s == 0 and precondition is not None:
                precondition(ref)
            sph.step()
            part = sph.getParticles()
            if s == 0:
                assert sph.tileStats()["workgroups"] == wgs
            worst, allowed = check_fast(part, ref, p, mass, "step %d" % s)      # strict: no clause
            print("step %d: worst force rel err %.3g" % (s, worst))
            check_fast_velocity(part.mVelocity, ovel, allowed, p.time_step, "step %d" % s)
            check_fast_position(part.mPosition, opos, p, "step %d" % s)
            ke, pe = sph.energy()
            assert ke == pytest.approx(ref["ke"], rel=1e-4, abs=1e-30)
            cur_pos, cur_vel = part.mPosition.copy(), part.mVelocity.copy()
        assert sph.getGrid().sum() == mass.size
