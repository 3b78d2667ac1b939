"""GPU parity, FULL mode with tolerance-mode pair arithmetic (SPH_HIP_MODE_FULL_FAST).

The reference's shipped binary is built with -O3 -ffast-math -funsafe-math-optimizations -mfma
(reference CMakeLists.txt:21): it is not the IEEE evaluation of src/sph.cpp (2.1e-5
relative between the two on accelerations).  FAST mode keeps what decides which pairs are summed
and in which order - the exact membership test of src/sph.cpp:641,653, the canonical order, the
viscous rescale inside the loop (:880-882) - and relaxes the per-pair arithmetic (csrc/pair_math.h).

Bar (against the CPU oracle, every step started from the SAME state on both sides):
  * neighbour counts identical;
  * acceleration: |a - a_ref| <= 1e-4 * max(|a|, |a_ref|) for EVERY particle - the north star's
    tolerance, asserted as written (STRICT) in every test of this file, of test_gpu_full_size.py
    and of test_gpu_c4_c5.py, i.e. on every BASELINE configuration and on every committed scene.
    One escape clause exists and is used by tests/test_gpu_random_scenes.py (adversarial seeded
    draws: clusters, duplicates, densities next to rho0) and tests/test_gpu_breaking_dam.py (the
    compressed dam, ~170 neighbours) ONLY, which print how many particles took it: a particle's ~30
    pair terms of either sign (src/sph.cpp:866-882) can cancel to less
    than a hundredth of their magnitude sum T (oracle_full_accel_scale), and there any evaluation
    that is not the reference's bit for bit - the reference's own -ffast-math build included -
    differs from it by rounding errors of the terms; such a particle passes with
    |a - a_ref| <= 1e-6 * T (16 fp32 ulps of the magnitude sum), at most 0.5 % of a scene's
    particles may need it (check_fast(..., scale=...): the clause is on only when a scale is given);
  * density: IDENTICAL to the oracle - the density sum keeps the reference's arithmetic (the pressure
    p = (rho - rho0) * k amplifies an error of rho by rho / (rho - rho0): a tolerance-mode density
    sum 2e-6 off made accelerations 4e-4 off next to particles whose density is near rho0);
  * new velocity: |v - v_ref| <= 1e-4 * max(|v|, |v_ref|) + dt * (what the particle's acceleration
    was allowed above) - the velocity is v + a dt / 2 plus the point-mass term, so a particle at
    rest inherits its acceleration's bar, cancellation clause included (seeded random scene 305,
    velocities of 1e-6: a force that passes by the second clause is a velocity 2.5e-3 off);
    new position within 1e-6 of the cell edge (+ 2 ulps of the coordinate).
Non-finite values (helpers.finite_parts): wherever a component of either side is not finite, the
other side's is of the same class - NaN, +inf or -inf - and the bars above apply to the components
that are finite on both sides; a density or count that is NaN on one side is NaN on the other.
The exact mode (tests/test_gpu_full_mode.py) stays the bit-for-bit gate.
"""
import os

import numpy as np
import pytest

from helpers import NONFINITE_SCENES, finite_parts, nonfinite_scene, pin_sha, to_oracle_params, vec_rel

pytestmark = pytest.mark.gpu

FORCE_RTOL = 1e-4
FORCE_COND_TOL = 1e-6      # of the magnitude sum of a particle's terms
FORCE_COND_SHARE = 0.005   # particles that may need the second clause
CLAUSE_USED = {"particles": 0, "scenes": 0}   # how often the clause was taken (random scenes, breaking dam)


def check_fast(part, ref, p, mass, what="", scale=None):
    """-> (largest relative force error, the absolute force error each particle was allowed).
    scale=None (every caller but the random scenes and the breaking dam): STRICT - 1e-4 relative for every
    particle."""
    assert np.array_equal(part.mNeighborCount, ref["ncount"]), "%s neighbour counts differ at %d particles" % (
        what, int((part.mNeighborCount != ref["ncount"]).sum()))
    assert np.array_equal(part.mDensity, ref["rho"], equal_nan=True), what + " density not bit-identical"
    a, b = finite_parts(np.reshape(part.mAcceleration, (-1, 3)), np.reshape(ref["acc"], (-1, 3)), what + " force")
    rel = vec_rel(a, b)
    allowed = FORCE_RTOL * np.maximum(np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1))
    over = rel > FORCE_RTOL
    if over.any():
        assert scale is not None, "%s force rel err %g at %d particles" % (what, rel.max(), int(over.sum()))
        err = np.linalg.norm(a - b, axis=1)
        T = scale()
        cond = err[over] / T[over]
        assert cond.max() <= FORCE_COND_TOL, "%s force error %g of the terms' magnitude sum (rel %g)" % (
            what, cond.max(), rel.max())
        assert over.mean() <= FORCE_COND_SHARE, "%s: %d particles beyond 1e-4 relative" % (what, int(over.sum()))
        allowed = np.maximum(allowed, FORCE_COND_TOL * T)
        CLAUSE_USED["particles"] += int(over.sum())
        CLAUSE_USED["scenes"] += 1
        print("%s: %d of %d particles beyond 1e-4 relative took the cancellation clause (worst %.3g of the "
              "terms' magnitude sum)" % (what, int(over.sum()), rel.size, float(cond.max())))
    return rel.max(), allowed


def check_fast_velocity(vel, ref_vel, allowed_force, dt, what=""):
    v, r = finite_parts(np.reshape(vel, (-1, 3)), np.reshape(ref_vel, (-1, 3)), what + " velocity")
    err = np.linalg.norm(v - r, axis=1)
    bar = FORCE_RTOL * np.maximum(np.linalg.norm(v, axis=1), np.linalg.norm(r, axis=1)) + float(dt) * allowed_force
    bad = err > bar
    assert not bad.any(), "%s velocity: %d particles beyond the bar, worst %g of it" % (
        what, int(bad.sum()), float((err[bad] / np.maximum(bar[bad], 1e-300)).max()))


def check_fast_position(pos, ref_pos, p, what=""):
    """new positions within 1e-6 of the cell edge + 2 ulps of the coordinate, component by component"""
    edge = 1.0 / float(p.full_cell_inv)
    a, b = finite_parts(pos, ref_pos, what + " position")
    bad = np.abs(a - b) > 1e-6 * edge + 2.0 ** -22 * np.abs(b)
    assert not bad.any(), "%s position: %d components beyond the bar" % (what, int(bad.sum()))


def fast_against_exact(acc, exact_acc, what=""):
    """-> per-particle relative force error of a tolerance-mode step against the exact mode's from the
    same state, after the non-finite rule; asserts that no particle is beyond 1e-4"""
    a, b = finite_parts(np.reshape(acc, (-1, 3)), np.reshape(exact_acc, (-1, 3)), what + " force")
    rel = vec_rel(a, b)
    assert (rel > FORCE_RTOL).sum() == 0, "%s: %d of %d particles beyond 1e-4 of the exact mode, worst %g" % (
        what, (rel > FORCE_RTOL).sum(), rel.size, rel.max())
    return rel


def run_fast(oracle, p, pos, vel, mass, steps=1, mode=None):
    """every step: the oracle starts from the state the GPU starts from"""
    import smoothed_particle_hydrodynamics_amd as S
    op = to_oracle_params(p)
    worst = 0.0
    with S.SPH(mass.size, p, mode=S.MODE_FULL_FAST if mode is None else mode) as sph:
        if mode is not None:
            sph.setArithmetic(S.ARITH_FAST)
        assert sph.getArithmetic() == S.ARITH_FAST
        sph.setParticles(pos, vel, mass)
        cur_pos, cur_vel = pos.copy(), vel.copy()
        for s in range(steps):
            sph.step()
            part = sph.getParticles()
            opos, ovel = cur_pos.copy(), cur_vel.copy()
            ref = oracle.step(op, opos, ovel, mass, mode="full")
            w, allowed = check_fast(part, ref, p, mass, "step %d" % s)      # strict: no clause
            worst = max(worst, w)
            check_fast_velocity(part.mVelocity, ovel, allowed, p.time_step, "step %d" % s)
            check_fast_position(part.mPosition, opos, p, "step %d" % s)
            ke, pe = sph.energy()
            assert ke == pytest.approx(ref["ke"], rel=1e-4, abs=1e-30)
            cur_pos, cur_vel = part.mPosition.copy(), part.mVelocity.copy()
    return worst


def test_fast_dam_break_20k_10_steps(oracle, hiplib):
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dam_break(20000, speed=0.05)
    run_fast(oracle, p, pos, vel, mass, steps=10)


def test_fast_dam_break_256k_moving(oracle, hiplib):
    """BASELINE config C2, with a velocity field so that the viscous sum is live"""
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dam_break(262144, speed=0.05)
    worst = run_fast(oracle, p, pos, vel, mass, steps=2)
    print("C2 moving, tolerance mode: worst force rel err %.3g (bar 1e-4, every particle)" % worst)


def test_fast_dam_break_256k_at_rest(oracle, hiplib):
    """BASELINE config C2 as the dam-break starts (the state bench.py steps): all 262 144 particles
    against the oracle, three steps"""
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dam_break(262144)
    worst = run_fast(oracle, p, pos, vel, mass, steps=3)
    print("C2 at rest, tolerance mode: worst force rel err %.3g (bar 1e-4, every particle)" % worst)


def test_fast_dense_block_with_point_mass_and_motion(oracle, hiplib):
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dense_block(12000, speed=20.0)
    run_fast(oracle, p, pos, vel, mass, steps=10)


def test_fast_unequal_masses_and_scale(oracle, hiplib):
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dense_block(6000, speed=5.0)
    mass = (0.5 + scenes.uniform01(11, np.arange(mass.size))).astype(np.float32)
    p.sim_scale = 0.5
    p.sim_scale_inv = 2.0
    run_fast(oracle, p, pos, vel, mass, steps=3)


def test_fast_edge_cases(oracle, hiplib):
    """duplicates (d = 0), particles outside the box, particles on cell faces, an over-full cell,
    an isolated particle"""
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dense_block(5000, lo=(-0.2, 0.0, 0.1), hi=(0.8, 0.6, 0.7), seed=5)
    pos = pos.reshape(-1, 3)
    pos[:50] = pos[50:100]
    edge = np.float32(1.0) / np.float32(p.full_cell_inv)
    pos[100:200] = edge * np.round(pos[100:200] / edge)
    pos[200:210] = [9.0, -4.0, 3.0]
    pos[210:700] = np.float32([3.31, 3.32, 3.33]) + np.float32(0.09) * (pos[210:700] % 1.0)
    pos[700] = [5.5, 5.5, 5.5]
    run_fast(oracle, p, np.ascontiguousarray(pos.reshape(-1)), vel, mass, steps=2)


def test_fast_distances_below_the_fast_root_s_range(oracle, hiplib):
    """squared distances below 2^-102: the batched root of the pressure loop takes its other path"""
    from test_gpu_full_mode import _tiny_distance_scene
    p, pos, vel, mass = _tiny_distance_scene()
    run_fast(oracle, p, pos, vel, mass, steps=2)


def test_fast_large_smoothing_length(oracle, hiplib):
    """h = 1e4 (the reference's comments speak of astrophysical units): kernel2 = -45 / (pi h^6) =
    -1.4e-23.  The pressure sum's running scale is taken from the exponent of kernel2 * sim_scale
    (PairConsts::fast_k2s); the fixed 2^-64 of round 3 left 9 significant bits of it here."""
    from smoothed_particle_hydrodynamics_amd import default_params, scenes
    h = 1.0e4
    p = default_params(h, (4, 4, 4))
    p.central_mass = 0.0
    assert abs(p.kernel2 * p.sim_scale) < 2e-19
    n = 1500
    pos = scenes.box_fill(n, (2.0e4,) * 3, (6.8e4,) * 3, seed=3)
    vel = scenes.box_fill(n, (-50.0,) * 3, (50.0,) * 3, seed=4)
    for mscale in (1.0, 1.0e11):          # negative pressures (rhoiInv = 1) / positive ones
        mass = (np.float32(mscale) * (0.5 + scenes.uniform01(11, np.arange(n)))).astype(np.float32)
        # (positive pressures of ~5e-4 make the in-loop viscous rescale mu / p_i = 20 per neighbour
        # with the default mu: the reference's own sum overflows after 30 of them)
        p.viscosity = 0.01 if mscale == 1.0 else 1.0e-5
        run_fast(oracle, p, pos, vel, mass, steps=2)


def test_fast_subnormal_pressure_of_a_lane_past_its_count(oracle, hiplib):
    """rho0 = -1e-36: an isolated particle (rho = 0) has the pressure 1e-39, a positive subnormal,
    1 / p = inf and A = p * rhoiInv^2 = inf.  In the tiled pressure loop a lane past its count takes
    itself as a neighbour of factor zero: 0 * inf must not reach its sum (every route the same bits,
    and the oracle's: the particle's acceleration is the point-mass term alone)."""
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dense_block(4000, lo=(1.0, 1.0, 1.0), hi=(1.8, 1.8, 1.8))
    p.rho0 = -1.0e-36
    pos = pos.reshape(-1, 3)
    # isolated particles: in the sorted order they share waves with the block's busy lanes only if
    # their cells are adjacent in cell-id order - put them right beside the block, one cell row away
    pos[5] = [1.4, 1.4, 2.05]
    pos[6] = [1.0, 2.05, 1.4]
    pos[7] = [0.6, 1.4, 1.4]
    pos = np.ascontiguousarray(pos.reshape(-1))
    run_fast(oracle, p, pos, vel, mass, steps=2)
    out = []
    for env in ({}, {"SPH_HIP_UNTILED": "1"}):
        for k, v in env.items():
            os.environ[k] = v
        try:
            with S.SPH(mass.size, p, mode=S.MODE_FULL_FAST) as sph:
                sph.setParticles(pos, vel, mass)
                sph.step()
                part = sph.getParticles()
                out.append((part.mAcceleration.copy(), part.mNeighborCount.copy()))
        finally:
            for k in env:
                os.environ.pop(k, None)
    assert (out[0][1][5:8] == 0).all()
    assert np.isfinite(out[0][0]).all()
    assert np.array_equal(out[0][0], out[1][0])


@pytest.mark.parametrize("n", [1, 2, 64, 257])
def test_fast_tiny_counts(oracle, hiplib, n):
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dense_block(n, lo=(3.0, 3.0, 3.0), hi=(3.25, 3.25, 3.25))
    run_fast(oracle, p, pos, vel, mass, steps=2)


def same_bits(a, b):
    """bit-identical arrays, every NaN written as the one quiet NaN first: the NaN pattern and the sign
    of every zero count, a NaN's payload (x86 and the GPU make different ones) does not"""
    return pin_sha(a) == pin_sha(b)


@pytest.mark.parametrize("env", [{}, {"SPH_HIP_UNTILED": "1"}, {"SPH_HIP_LIST_CAP": "30"}],
                         ids=["default", "untiled", "list-cap-30"])
@pytest.mark.parametrize("case", NONFINITE_SCENES)
def test_nonfinite_point_mass_term(oracle, hiplib, case, env, monkeypatch):
    """scenes without a point mass in which a position or the central position is not finite
    (helpers.nonfinite_scene; the oracle's answers are the reference's, test_oracle_vs_reference.py):
    FULL bit for bit; FULL_FAST, which skips the term's arithmetic (pair_math.h point_mass_nan), to
    the bar with its non-finite rule - NaN in exactly the components the reference has it in.  Two
    steps, every step from the GPU's state, on the default, untiled and list-less routes."""
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    for k in ("SPH_HIP_UNTILED", "SPH_HIP_TILE_CAP", "SPH_HIP_LIST_CAP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p, pos, vel, mass = nonfinite_scene(case)
    q, qpos, qvel, _ = scenes.dam_break(mass.size, speed=0.05)     # the scene is the moving dam-break's
    for i in range(3):
        q.central_pos[i] = p.central_pos[i]
    fin = np.isfinite(pos)
    assert bytes(q) == bytes(p) and np.array_equal(qvel, vel) and np.array_equal(qpos[fin], pos[fin])
    op = to_oracle_params(p)
    nan_rows = 0
    with S.SPH(mass.size, p, mode=S.MODE_FULL) as sph:
        sph.setParticles(pos, vel, mass)
        cur_pos, cur_vel = pos.copy(), vel.copy()
        for step in range(2):
            sph.step()
            part = sph.getParticles()
            ref = oracle.step(op, cur_pos, cur_vel, mass, mode="full")
            what = "%s, FULL, step %d: " % (case, step)
            assert np.array_equal(part.mNeighborCount, ref["ncount"]), what + "neighbour counts"
            for name, got, want in (("density", part.mDensity, ref["rho"]), ("acceleration", part.mAcceleration, ref["acc"]),
                                    ("position", part.mPosition, cur_pos), ("velocity", part.mVelocity, cur_vel)):
                assert same_bits(got, want), what + name
            nan_rows = max(nan_rows, int(np.isnan(ref["acc"]).reshape(-1, 3).any(axis=1).sum()))
    assert nan_rows >= (5 if case == "particles" else mass.size)     # the scenes do reach the NaN cases
    worst = run_fast(oracle, p, pos, vel, mass, steps=2)
    print("%s %s: FULL bit-identical, FULL_FAST worst force rel err %.3g" % (case, env or "default", worst))


@pytest.mark.parametrize("env", [{"SPH_HIP_UNTILED": "1"}, {"SPH_HIP_TILE_CAP": "512"}, {"SPH_HIP_LIST_CAP": "30"}])
def test_fast_every_route_same_bits(oracle, hiplib, env, monkeypatch):
    """tiled, untiled, give-up workgroups, particles without a
    list: the FAST arithmetic is written out operation by operation, so every route produces the
    same bits as the default one - a slab's recomputed ghost densities equal their owner's"""
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dam_break(60000, speed=0.05)
    out = []
    for e in ({}, env):
        for k in ("SPH_HIP_UNTILED", "SPH_HIP_TILE_CAP", "SPH_HIP_LIST_CAP"):
            monkeypatch.delenv(k, raising=False)
        for k, v in e.items():
            monkeypatch.setenv(k, v)
        with S.SPH(mass.size, p, mode=S.MODE_FULL_FAST) as sph:
            sph.setParticles(pos, vel, mass)
            sph.run(2)
            sph.step()
            part = sph.getParticles()
            out.append({k: getattr(part, k).copy() for k in ("mPosition", "mVelocity", "mDensity",
                                                            "mAcceleration", "mNeighborCount")})
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k


def test_switching_arithmetic_on_a_live_context(oracle, hiplib):
    """exact -> fast -> exact on one context: the exact steps are the oracle's bits again"""
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dam_break(30000, speed=0.05)
    op = to_oracle_params(p)
    with S.SPH(mass.size, p) as sph:
        assert sph.getArithmetic() == S.ARITH_EXACT
        sph.setParticles(pos, vel, mass)
        sph.step()
        sph.setArithmetic(S.ARITH_FAST)
        sph.step()
        sph.setArithmetic(S.ARITH_EXACT)
        mid = sph.getParticles()
        opos, ovel = mid.mPosition.copy(), mid.mVelocity.copy()
        sph.step()
        part = sph.getParticles()
        ref = oracle.step(op, opos, ovel, mass, mode="full")
        assert np.array_equal(part.mDensity, ref["rho"])
        assert np.array_equal(part.mAcceleration, ref["acc"])
        assert np.array_equal(part.mPosition, opos)


def test_fast_is_refused_for_ref_mode(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dense_block(1000)
    with S.SPH(mass.size, p, mode=S.MODE_REF) as sph:
        with pytest.raises(S.SphHipError):
            sph.setArithmetic(S.ARITH_FAST)
