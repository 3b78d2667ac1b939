"""GPU, BASELINE full size (C3: 4 194 304-particle dam-break, the bench workload).

The oracle cannot step 4M particles in test time, so parity at this size is shown through
  * an EXACT check on a sub-slab: the particles within 2h (+margin) of a thin z-window are handed
    to the oracle with the same parameters and grid; cell ids and the (cell, id) canonical order
    are unchanged by restricting the set, and with a 2h halo every interior particle (and each of
    its neighbours' densities) sees its complete neighbourhood — so density, acceleration,
    neighbour count, new position and new velocity of the interior particles must equal the full
    run's bit for bit;
  * size-independent properties: every id downloaded exactly once, per-cell occupancy sums to N,
    the neighbour relation is symmetric (sum of counts even and equal to twice the pair count of
    the window), a second context with 2 slabs gives identical checksums.
The window check is made twice: on step 1 of the column at rest (as the dam-break starts), and on
step 3 of a column that moves (seeded velocity field), where v_j - v_i != 0 and the order-sensitive
viscous sum of src/sph.cpp:875-882 - the reason for the canonical order - is live.  Both states are
also stepped with the tolerance-mode arithmetic (SPH_HIP_MODE_FULL_FAST, bench.py's headline) and
held to the north star's bar as written: neighbour counts and densities identical, acceleration
within 1e-4 relative for EVERY particle of the window against the oracle, and for EVERY one of the
4 194 304 particles against the exact mode (whose window is the oracle's, bit for bit) - no share
clause, no magnitude-sum clause.
"""
import hashlib

import numpy as np
import pytest

from helpers import to_oracle_params

pytestmark = pytest.mark.gpu

N = 4 * 1024 * 1024


@pytest.fixture(scope="module")
def big_run(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dam_break(N)
    with S.SPH(N, p) as sph:
        sph.setParticles(pos, vel, mass)
        sph.step()
        part = sph.getParticles()
        out = dict(p=p, pos0=pos, vel0=vel, mass=mass, pos=part.mPosition.copy(),
                   vel=part.mVelocity.copy(), rho=part.mDensity.copy(),
                   acc=part.mAcceleration.copy(), ncount=part.mNeighborCount.copy(),
                   grid=sph.getGrid().copy(), energy=sph.energy())
        # the same first step with the tolerance-mode arithmetic, from the same state
        sph.setArithmetic(S.ARITH_FAST)
        sph.setParticles(pos, vel, mass)
        sph.step()
        assert sph.getArithmetic() == S.ARITH_FAST
        part = sph.getParticles()
        out["fast"] = dict(pos=part.mPosition.copy(), vel=part.mVelocity.copy(), rho=part.mDensity.copy(),
                           acc=part.mAcceleration.copy(), ncount=part.mNeighborCount.copy())
    return out


def test_c3_properties(big_run):
    r = big_run
    assert r["grid"].sum() == N
    assert r["ncount"].sum() % 2 == 0                    # d2(i,j) == d2(j,i): symmetric relation
    assert 30.0 < r["ncount"].mean() < 32.5              # ~32 by construction of h
    assert np.isfinite(r["acc"]).all() and np.isfinite(r["rho"]).all()
    assert (r["rho"] > 0).sum() > 0.999 * N
    # every particle was integrated exactly once: positions moved by v_half*dt from the inputs
    assert np.abs(r["pos"] - r["pos0"]).max() < 1e-3
    assert np.isfinite(r["energy"]).all()


def test_c3_window_matches_oracle_exactly(oracle, big_run):
    r = big_run
    p = r["p"]
    op = to_oracle_params(p)
    h = np.float32(p.h)
    z = r["pos0"].reshape(-1, 3)[:, 2]
    z0, z1 = np.float32(0.400), np.float32(0.420)
    margin = np.float32(2.0) * h * np.float32(1.05) + np.float32(2.0) / np.float32(p.full_cell_inv)
    sub = np.nonzero((z >= z0 - margin) & (z < z1 + margin))[0]          # ascending ids
    inner = (z[sub] >= z0) & (z[sub] < z1)
    assert inner.sum() > 50000 and sub.size < 600000
    spos = np.ascontiguousarray(r["pos0"].reshape(-1, 3)[sub]).reshape(-1)
    svel = np.ascontiguousarray(r["vel0"].reshape(-1, 3)[sub]).reshape(-1)
    smass = np.ascontiguousarray(r["mass"][sub])
    ref = oracle.step(op, spos, svel, smass, mode="full")
    ids = sub[inner]
    assert np.array_equal(r["ncount"][ids], ref["ncount"][inner])
    assert np.array_equal(r["rho"][ids], ref["rho"][inner])
    assert np.array_equal(r["acc"].reshape(-1, 3)[ids], ref["acc"].reshape(-1, 3)[inner])
    assert np.array_equal(r["pos"].reshape(-1, 3)[ids], spos.reshape(-1, 3)[inner])
    assert np.array_equal(r["vel"].reshape(-1, 3)[ids], svel.reshape(-1, 3)[inner])
    assert r["ncount"][ids].sum() > 1500000               # > 1.5M neighbour pairs checked exactly


@pytest.fixture(scope="module")
def moved_run(hiplib):
    """3 steps of the moving column, exact and tolerance-mode arithmetic, with the state before
    the last step"""
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dam_break(N, speed=0.05)
    out = dict(p=p, mass=mass)
    with S.SPH(N, p) as sph:
        sph.setParticles(pos, vel, mass)
        sph.run(2)
        part = sph.getParticles()
        out["pos0"], out["vel0"] = part.mPosition.copy(), part.mVelocity.copy()
        sph.step()
        part = sph.getParticles()
        out["exact"] = dict(pos=part.mPosition.copy(), vel=part.mVelocity.copy(), rho=part.mDensity.copy(),
                            acc=part.mAcceleration.copy(), ncount=part.mNeighborCount.copy())
        # the same third step with the tolerance-mode arithmetic, from the same state
        sph.setArithmetic(S.ARITH_FAST)
        sph.setParticles(out["pos0"], out["vel0"], mass)
        sph.step()
        part = sph.getParticles()
        out["fast"] = dict(pos=part.mPosition.copy(), vel=part.mVelocity.copy(), rho=part.mDensity.copy(),
                           acc=part.mAcceleration.copy(), ncount=part.mNeighborCount.copy())
    return out


def oracle_window(oracle, r, z0, z1):
    """the oracle's step on the particles within 2h (+ margin) of the z-window [z0, z1)"""
    p = r["p"]
    h = np.float32(p.h)
    z = r["pos0"].reshape(-1, 3)[:, 2]
    margin = np.float32(2.0) * h * np.float32(1.05) + np.float32(2.0) / np.float32(p.full_cell_inv)
    sub = np.nonzero((z >= z0 - margin) & (z < z1 + margin))[0]          # ascending ids
    inner = (z[sub] >= z0) & (z[sub] < z1)
    assert inner.sum() > 50000 and sub.size < 600000
    spos = np.ascontiguousarray(r["pos0"].reshape(-1, 3)[sub]).reshape(-1)
    svel = np.ascontiguousarray(r["vel0"].reshape(-1, 3)[sub]).reshape(-1)
    smass = np.ascontiguousarray(r["mass"][sub])
    before = (spos.copy(), svel.copy())
    ref = oracle.step(to_oracle_params(p), spos, svel, smass, mode="full")
    return sub, inner, ref, spos, svel, smass, before


def test_c3_moved_state_window_matches_oracle_exactly(oracle, moved_run):
    """step 3 of the moving column: non-zero v_j - v_i in every viscous term"""
    r, got = moved_run, moved_run["exact"]
    assert np.abs(r["vel0"]).max() > 0.01
    sub, inner, ref, spos, svel, _, _ = oracle_window(oracle, r, np.float32(0.400), np.float32(0.420))
    ids = sub[inner]
    assert np.array_equal(got["ncount"][ids], ref["ncount"][inner])
    assert np.array_equal(got["rho"][ids], ref["rho"][inner])
    assert np.array_equal(got["acc"].reshape(-1, 3)[ids], ref["acc"].reshape(-1, 3)[inner])
    assert np.array_equal(got["pos"].reshape(-1, 3)[ids], spos.reshape(-1, 3)[inner])
    assert np.array_equal(got["vel"].reshape(-1, 3)[ids], svel.reshape(-1, 3)[inner])
    assert got["ncount"][ids].sum() > 1500000


def fast_window_strict(oracle, r, got, exact, what):
    """tolerance-mode results `got` of the step from (r.pos0, r.vel0): strict bar on the oracle's
    window, strict bar on all 4M particles against the exact mode"""
    from test_gpu_full_fast import check_fast, check_fast_velocity, fast_against_exact

    class Part:
        pass

    assert np.array_equal(got["ncount"], exact["ncount"])     # all 4M particles
    assert np.array_equal(got["rho"], exact["rho"])           # the density sum is the exact mode's
    sub, inner, ref, spos, svel, smass, before = oracle_window(oracle, r, np.float32(0.400), np.float32(0.420))
    ids = sub[inner]
    part = Part()
    part.mNeighborCount = got["ncount"][ids]
    part.mDensity = got["rho"][ids]
    part.mAcceleration = np.ascontiguousarray(got["acc"].reshape(-1, 3)[ids]).reshape(-1)
    wref = dict(ncount=ref["ncount"][inner], rho=ref["rho"][inner],
                acc=np.ascontiguousarray(ref["acc"].reshape(-1, 3)[inner]).reshape(-1))
    worst, allowed = check_fast(part, wref, r["p"], r["mass"], what)         # strict: no clause
    check_fast_velocity(got["vel"].reshape(-1, 3)[ids], svel.reshape(-1, 3)[inner], allowed, r["p"].time_step, what)
    # and over the whole scene against the exact mode (= the oracle wherever it was checked)
    rel = fast_against_exact(got["acc"], exact["acc"], what)
    print("%s, tolerance mode: window vs oracle max force rel err %.3g; all %d particles vs exact mode: max "
          "%.3g, 0 beyond 1e-4" % (what, worst, rel.size, rel.max()))


def test_c3_moved_state_window_tolerance_mode(oracle, moved_run):
    """step 3 of the moving column with SPH_HIP_MODE_FULL_FAST's arithmetic: the north star's bar
    as written, for every particle"""
    fast_window_strict(oracle, moved_run, moved_run["fast"], moved_run["exact"], "C3 moved state")


def test_c3_at_rest_window_tolerance_mode(oracle, big_run):
    """the first step of the column at rest - the state bench.py's headline steps - with the
    tolerance-mode arithmetic, same bar"""
    r = big_run
    exact = dict(ncount=r["ncount"], rho=r["rho"], acc=r["acc"])
    fast_window_strict(oracle, r, r["fast"], exact, "C3 at rest")


def test_c3_two_slabs_identical(big_run):
    """the same step as two z-slabs exchanging halos: identical per-particle results"""
    import torch
    from smoothed_particle_hydrodynamics_amd import slab as SL
    r = big_run
    p = r["p"]
    zz = r["pos0"].reshape(-1, 3)[:, 2]
    cuts = SL.plan_cuts(p, zz, 2)
    hist = np.bincount(SL.plane_of(p, zz), minlength=p.full_cells_z)
    stream = torch.cuda.Stream()
    slabs = []
    for k in range(2):
        cap, msg = SL.slab_capacities(hist, cuts, k)
        s = SL.HipSlab(p, cuts[k], cuts[k + 1], cap, msg, device=0, has_left=k > 0, has_right=k < 1,
                       stream=stream)
        s.upload(*SL.split_scene(p, cuts, k, r["pos0"], r["vel0"], r["mass"]), all_masses_equal=True)
        slabs.append(s)
    group = SL.LocalSlabGroup(slabs)
    group.step()
    got = group.gather(N)
    for s in slabs:
        assert s.status()["errors"] == 0
        s.close()
    for k in ("pos", "vel", "rho", "acc", "ncount"):
        assert hashlib.sha256(got[k].tobytes()).digest() == hashlib.sha256(r[k].tobytes()).digest(), k
