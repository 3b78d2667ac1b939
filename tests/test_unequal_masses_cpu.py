"""CPU: the inputs of tests/test_gpu_unequal_masses.py are not vacuous, by the restatements alone - under the flavours
of tests/mass_cases.py nearly every row of every feature's output tells a neighbour's mass from the probing particle's
own and from no mass at all; the figures CPU_* pinned in that file are what the restatements give, and they clear the
bars stated in DESIGN.md section 35.  Properties of cohesion and XSPH under unequal masses, on the restatements; and
every branch of the uniform-mass rule with emitters (csrc/port_policy.h: port_mass_rule) through a g++ shim."""
import ctypes as C
import math

import numpy as np
import pytest

import cohesion_emulation as CE
import mass_cases
import monitor_emulation as ME
import pressure_emulation as PE
import sample_emulation as SE
import test_gpu_unequal_masses as UM
import xsph_emulation as XE
from helpers import compile_shim, to_oracle_params

F32 = np.float32
N = UM.N
FEATURES = ("cohesion", "xsph", "scalars", "velgrad", "pressure", "density")


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- the flavours ------------------------------------------------------------------------------------------------
def test_the_flavours_are_what_they_say(hiplib):
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, unit, _, _ = mass_cases.block("UNIT")
    assert unit.size == N and mass_cases.uniform(unit) and (unit == 1).all()
    spread = mass_cases.masses("SPREAD", p, pos)
    assert np.array_equal(bits(spread), bits((0.5 + scenes.uniform01(11, np.arange(N))).astype(F32)))
    assert spread.min() >= 0.5 and spread.max() < 1.5 and np.unique(spread).size > N - 10
    two = mass_cases.masses("TWO_SPECIES", p, pos)
    assert sorted(np.unique(two).tolist()) == [1.0, 4.0] and 0.4 < (two == 1).mean() < 0.6
    # both species stand in nearly every support
    grid = SE.Grid(p, pos, vel, two)
    probe, idx, _ = PE.members(grid, grid.pos, exclude_self=True)
    light = np.bincount(probe, weights=grid.mass[idx] == 1, minlength=N)
    heavy = np.bincount(probe, weights=grid.mass[idx] == 4, minlength=N)
    assert ((light > 0) & (heavy > 0)).mean() > 0.97
    for flavour in mass_cases.FLAVOURS + ("ODD_ONE",):
        assert not mass_cases.uniform(mass_cases.masses(flavour, p, pos))
    with pytest.raises(ValueError):
        mass_cases.masses("HEAVY", p, pos)
    # the other scenes: the positions, velocities and parameters are the existing ones
    import param_cases
    q, qpos, qvel, qmass = mass_cases.probe_block("SPREAD")
    r, rpos, rvel, rmass = param_cases.scene(scenes.default_params)
    assert bytes(q) == bytes(r) and qpos.tobytes() == rpos.tobytes() and qvel.tobytes() == rvel.tobytes()
    assert qmass.size == rmass.size == 6000 and not mass_cases.uniform(qmass)


def test_odd_one_is_unit_mass_almost_everywhere(hiplib):
    p, pos, vel, mass, _, _ = mass_cases.block("ODD_ONE")
    odd, far, inside = UM.odd_one_figures()
    assert (odd, far, inside) == UM.CPU_ODD_ONE
    assert far >= 1000 and inside >= 30
    assert mass[odd] == 2 and (np.delete(mass, odd) == 1).all()
    assert mass_cases.neighbour_counts(p, pos)[odd] == inside == mass_cases.neighbour_counts(p, pos).max()


def test_own_mass_changes_nothing_where_the_masses_are_equal(hiplib):
    """the probe itself: with one mass everywhere a neighbour's mass is one's own, in bits, in every restatement it
    follows - and a walk it cannot follow is refused, not left as it is"""
    p, pos, vel, mass, T, kappa = mass_cases.block("UNIT")
    mass = (mass * F32(1.25)).astype(F32)
    rho = PE.particle_density(p, pos, vel, mass)
    on = pos.reshape(-1, 3)
    for fn in (lambda: CE.sums(p, pos, vel, mass), lambda: XE.sums(p, pos, vel, mass, rho),
               lambda: UM.SC.step(p, pos, vel, mass, rho, T, kappa), lambda: UM.VE.rows(p, pos, vel, mass),
               lambda: np.stack(PE.sample(p, pos, vel, mass, on)[:2], 1)):
        assert not mass_cases.rows_differing(fn(), mass_cases.own_mass(fn, own=mass)).any()
    with pytest.raises(AssertionError):
        mass_cases.own_mass(SE.Grid(p, pos, vel, mass).sample, on)
    with pytest.raises(AssertionError):
        mass_cases.own_mass(PE.sample, p, pos, vel, mass, on)           # free probes, and no mass given for them
    # and the restatements are as they were
    assert PE.members.__module__ == "pressure_emulation" and SE.density_terms.__module__ == "sample_emulation"
    # the pressure sampler's density is the field sampler's
    assert np.array_equal(bits(PE.sample(p, pos, vel, mass, on)[1]), bits(SE.Grid(p, pos, vel, mass).sample(on, velocity=False)[0]))


# ---- the figures ---------------------------------------------------------------------------------------------------
def test_the_pinned_figures_are_the_restatements_and_clear_the_bars(hiplib):
    fig = UM.cpu_figures()
    for name, value in fig.items():
        assert getattr(UM, name) == value, (name, value)
    members = fig["CPU_ROWS_WITH_A_MEMBER"]
    assert members == N
    for flavour in ("CPU_SPREAD", "CPU_TWO_SPECIES"):
        assert sorted(fig[flavour]) == sorted(FEATURES)
        for feature, (own, unit) in fig[flavour].items():
            print("%s %s: %d of %d rows differ from own_mass, %d from the unit-mass run" % (flavour, feature, own, members, unit))
            assert own >= 0.9 * members and unit >= 0.9 * members, (flavour, feature)
    assert fig["CPU_XSPH_SPREAD_G"] <= 1.0


def test_the_monitors_row_and_the_whole_step_differ_from_the_unit_mass_run(oracle, hiplib):
    p, pos, vel, mass, T, kappa = mass_cases.block("SPREAD")
    unit = np.ones(N, F32)
    op = to_oracle_params(p)
    rows, steps = [], []
    for m in (mass, unit):
        out = XE.step(oracle, p, pos, vel, m, UM.EPS, UM.GAMMA)
        _, cs, ci = oracle.full_cells(op, pos)
        out["ncount"] = oracle.full_density(op, pos, m, cs, ci)[1]
        rows.append(ME.step_row(p, (pos, vel, m), out, UM.Q))
        steps.append(out)
    for name in ("mass", "momentum", "kinetic"):
        assert rows[0][name].tobytes() != rows[1][name].tobytes(), name
    assert rows[0]["live"] == rows[1]["live"] == N
    # the row's mass is the float64 sum of the masses: every fp32 mass is a whole number of quanta of 2^-24
    assert int(rows[0]["mass"]) == int(round(float(mass.astype(np.float64).sum()) * 2.0 ** 24))
    for key, width in (("acc", 3), ("vel", 3), ("pos", 3), ("rho", 1)):
        differ = mass_cases.rows_differing(steps[0][key].reshape(-1, width), steps[1][key].reshape(-1, width))
        assert differ.sum() == N, key
    assert steps[0]["touched"].all()


def test_the_walled_blocks_loads_differ_from_the_unit_mass_ones(oracle, hiplib):
    """three steps of the walled obstacle block by the oracle and the restatement: in every step that has a contact
    the recorded row is not the unit-mass run's"""
    import moving_obstacle_emulation as M
    import path_emulation as PA
    p, pos, vel, mass, obst, paths, motions = mass_cases.walled("SPREAD")
    assert not mass_cases.uniform(mass)
    clock = M.clock(p.time_step, UM.STEPS)
    op = to_oracle_params(p)
    rows = {}
    for name, m in (("spread", mass), ("unit", np.ones(mass.size, F32))):
        x, v = pos.copy(), vel.copy()
        rows[name] = []
        for k in range(UM.STEPS):
            x, v, row = PA.oracle_step(oracle, op, obst, paths, motions, x, v, m, clock[k], clock[k + 1])
            rows[name].append(row)
    contacts = 0
    for a, b in zip(rows["spread"], rows["unit"]):
        if a.count.sum() or b.count.sum():
            contacts += 1
            assert not np.array_equal(a.impulse, b.impulse)
    print("%d of %d steps have a contact; first row: %d responses" % (contacts, UM.STEPS, int(rows["spread"][0].count.sum())))
    assert contacts >= 1


def test_the_emitter_one_ulp_heavier_shows_in_the_densities(oracle, hiplib):
    """tests/test_gpu_unequal_masses.py's ulp scene: a density pass that kept the uniform-mass flag would give other
    bits in hundreds of rows, particles of the block and of the first emitter's layer among them"""
    _, differ, differ_light = UM.ulp_figures(oracle)
    print("%d rows differ, %d of them not the heavier emitter's" % (differ, differ_light))
    assert differ >= 100 and differ_light >= 50


# ---- cohesion and XSPH under unequal masses, on the restatements -----------------------------------------------------
@pytest.fixture(scope="module")
def spread_pairs(hiplib):
    p, pos, vel, mass, _, _ = mass_cases.block("SPREAD")
    grid = SE.Grid(p, pos, vel, mass)
    probe, idx, d2 = PE.members(grid, grid.pos, exclude_self=True)
    return p, pos, vel, mass, grid, probe, idx, d2


def test_cohesions_pair_term_is_antisymmetric_up_to_the_masses(spread_pairs):
    """The pair term is (m_j * W) * r.  Its mass-free part W * r is the bitwise negation of (j, i)'s on every ordered
    pair (the same d2, the same W, r negated).  The momentum addend m_i * ((m_j * W) * r) is NOT the bitwise negation
    of m_j * ((m_i * W) * (-r)) in fp32: the two round m_i and m_j in at different places.  With TWO_SPECIES' masses,
    powers of two, every product is exact and the negation holds bit for bit; under SPREAD the two differ in the last
    places on most pairs (the figure is printed) and what holds is the bound of the next test."""
    p, pos, vel, mass, grid, probe, idx, d2 = spread_pairs
    r = grid.pos[probe] - grid.pos[idx]
    one = np.ones(probe.size, F32)
    assert probe.size > 40000
    assert np.array_equal(np.sort(probe * N + idx), np.sort(idx * N + probe))     # every ordered pair with its mirror
    free, back = CE.pair_terms(p, d2, one, r), CE.pair_terms(p, d2, one, -r)
    assert np.array_equal(bits(free) ^ np.uint32(0x80000000), bits(back)) and np.abs(free).max() > 0

    def addends(m):
        mi, mj = m[probe][:, None], m[idx]
        there = (mi * CE.pair_terms(p, d2, mj, r)).astype(F32)
        here = (mj[:, None] * CE.pair_terms(p, d2, m[probe], -r)).astype(F32)
        return there, here

    two = np.where(grid.mass < 1, F32(1.0), F32(4.0)).astype(F32)                  # (in the grid's order: any draw will do)
    there, here = addends(two)
    assert np.array_equal(bits(there) ^ np.uint32(0x80000000), bits(here))
    there, here = addends(grid.mass)
    off = (bits(there) ^ np.uint32(0x80000000) != bits(here)).any(1)
    print("SPREAD: %d of %d ordered pairs' momentum addends are not each other's negation in fp32" % (off.sum(), off.size))
    rel = np.abs(there.astype(np.float64) + here.astype(np.float64)) / np.maximum(np.abs(there.astype(np.float64)), 1e-300)
    # three roundings on each side - (m W), (. r), (m .) - of at most 2^-24 relative each: 6 * 2^-24 to first order
    assert rel.max() <= 7 * 2.0 ** -24


def test_cohesion_conserves_the_mass_weighted_momentum_and_no_other(spread_pairs):
    """|sum_i m_i c_i| per component is within (kmax + 4) * 2^-24 * sum_i |m_i c_i| - the rounding of the per-particle
    sums; a kernel that weights by the probing particle's own mass misses that bound, and so does the unweighted sum."""
    p, pos, vel, mass, grid, probe, idx, d2 = spread_pairs
    kmax = int(np.bincount(probe).max())
    m64 = mass.astype(np.float64)[:, None]
    c = CE.accel(UM.GAMMA, CE.sums(p, pos, vel, mass)).astype(np.float64)
    own = CE.accel(UM.GAMMA, mass_cases.own_mass(CE.sums, p, pos, vel, mass)).astype(np.float64)
    for a in range(3):
        T = float(np.abs(m64[:, 0] * c[:, a]).sum())
        bound = (kmax + 4) * 2.0 ** -24 * T
        total = math.fsum(m64[:, 0] * c[:, a])
        wrong = math.fsum(m64[:, 0] * own[:, a])
        bare = math.fsum(c[:, a])
        print("component %d: sum m c %.3e, bound %.3e, sum |m c| %.3e; own mass %.3e; unweighted %.3e" % (a, total, bound, T, wrong, bare))
        assert T > 1000 and abs(total) <= bound
        assert abs(wrong) > 100 * bound and abs(bare) > 100 * bound


def test_xsph_under_unequal_masses_is_what_it_is(spread_pairs):
    """DESIGN.md section 34 says "equal masses": g_ij = m_j W (1/rho_i + 1/rho_j) / 2 is not symmetric under SPREAD.
    What is pinned: eps * max_i sum_j g_ij <= 1, so every v' is a convex combination of S_k's velocities, and the
    kinetic energy about the mass-weighted mean velocity falls on the block."""
    p, pos, vel, mass, grid, probe, idx, d2 = spread_pairs
    rho = PE.particle_density(p, pos, vel, mass)
    s, info = XE.sums(p, pos, vel, mass, rho, with_info=True)
    R = XE.stage(grid.vel, rho[PE.canonical_order(p, pos)])
    g = XE.weights(p, d2, grid.mass[idx], R[probe][:, 3], R[idx][:, 3])
    mirror = np.argsort(idx * N + probe, kind="stable")                 # (j, i) in the order of (i, j)
    assert (bits(g) != bits(g[mirror])).mean() > 0.9                    # not symmetric
    worst = UM.EPS * float(info["g_sum"].max())
    assert round(worst, 4) == UM.CPU_XSPH_SPREAD_G and worst <= 1.0
    new, on, _ = XE.apply(p, UM.EPS, pos, vel, mass, rho)
    before, after = XE.kinetic_about_mean(vel, mass), XE.kinetic_about_mean(new, mass)
    print("eps * max_i sum_j g_ij = %.4f; kinetic energy about the mass-weighted mean: %.6e -> %.6e" % (worst, before, after))
    assert on.all() and after < before


# ---- the uniform-mass rule with emitters -------------------------------------------------------------------------------
SHIM = r"""
#include "port_policy.h"

extern "C" {
// out: {uniform, known}; returns the resident mass's bits
unsigned rule(int uniform, int known, float mass, const float* emitter_mass, int ne, int nothing_resident, int* out)
{
   sph_hip_emitter e[SPH_HIP_MAX_EMITTERS] = {};
   for (int i = 0; i < ne; i++) e[i].mass = emitter_mass[i];
   const PortMassRule r = port_mass_rule(uniform, known, mass, e, ne, nothing_resident != 0);
   out[0] = r.uniform;
   out[1] = r.known;
   unsigned b;
   memcpy(&b, &r.mass, sizeof(b));
   return b;
}
int same_bits(float a, float b) { return port_same_bits(a, b) ? 1 : 0; }
}
"""


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    lib = compile_shim(SHIM, ["-O2", "-ffp-contract=off"], tmp_path_factory)
    lib.rule.argtypes = [C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.rule.restype = C.c_uint32
    lib.same_bits.argtypes = [C.c_float, C.c_float]
    return lib


def rule(policy, uniform, known, mass, emitters, nothing_resident=False):
    """(uniform, known, the resident mass's bits) after port_mass_rule"""
    e = np.ascontiguousarray(emitters, F32)
    out = (C.c_int * 2)()
    b = policy.rule(int(uniform), int(known), float(F32(mass)), e.ctypes.data_as(C.c_void_p), e.size, int(nothing_resident), out)
    return out[0], out[1], b


def word(v):
    return int(np.array([v], F32).view(np.uint32)[0])


NEXT = np.nextafter(F32(1.0), F32(2.0))


def test_no_emitter_changes_nothing(policy):
    for uniform in (0, 1):
        for known in (0, 1):
            for nothing in (False, True):
                assert rule(policy, uniform, known, 1.5, [], nothing) == (uniform, known, word(1.5))


def test_emitters_equal_to_the_upload_in_bits_keep_the_flag(policy):
    assert rule(policy, 1, 1, 1.0, [1.0]) == (1, 1, word(1.0))
    assert rule(policy, 1, 1, 2.5, [2.5, 2.5, 2.5]) == (1, 1, word(2.5))
    assert rule(policy, 1, 1, -0.0, [-0.0]) == (1, 1, word(-0.0))


def test_the_next_float_clears_the_flag(policy):
    assert NEXT != F32(1.0) and policy.same_bits(1.0, float(NEXT)) == 0 and policy.same_bits(float(NEXT), float(NEXT)) == 1
    assert rule(policy, 1, 1, 1.0, [NEXT]) == (0, 1, word(1.0))
    assert rule(policy, 1, 1, 1.0, [1.0, NEXT]) == (0, 1, word(1.0))
    assert rule(policy, 1, 1, 1.0, [NEXT, 1.0]) == (0, 1, word(1.0))
    assert rule(policy, 1, 1, NEXT, [1.0]) == (0, 1, word(NEXT))
    # eight emitters, the last one off
    assert rule(policy, 1, 1, 1.0, [1.0] * 7 + [NEXT]) == (0, 1, word(1.0))


def test_the_zeros_differ_in_bits(policy):
    """-0.0f == +0.0f compares true; the rule compares bits (port_check refuses such masses before they get here: the
    rule does not rely on it)"""
    assert policy.same_bits(-0.0, 0.0) == 0 and policy.same_bits(0.0, 0.0) == 1
    assert rule(policy, 1, 0, 7.0, [-0.0, 0.0], nothing_resident=True) == (0, 1, word(-0.0))
    assert rule(policy, 0, 0, 7.0, [0.0, 0.0], nothing_resident=True) == (1, 1, word(0.0))
    assert rule(policy, 1, 1, 0.0, [-0.0]) == (0, 1, word(0.0))
    # and a NaN has its own bits
    nan = float("nan")
    assert policy.same_bits(nan, nan) == 1
    assert rule(policy, 1, 1, nan, [nan])[0] == 1


def test_an_unknown_upload_mass_clears_the_flag(policy):
    assert rule(policy, 1, 0, 1.0, [1.0]) == (0, 0, word(1.0))
    assert rule(policy, 1, 0, 0.0, [0.0]) == (0, 0, word(0.0))


def test_an_empty_upload_is_decided_by_the_emitters_alone(policy):
    for uniform in (0, 1):
        for known in (0, 1):
            # agreeing: the flag is set whatever it was, and their mass becomes the resident one
            assert rule(policy, uniform, known, 9.0, [2.5], True) == (1, 1, word(2.5))
            assert rule(policy, uniform, known, 9.0, [2.5, 2.5, 2.5], True) == (1, 1, word(2.5))
            # disagreeing: clear, and the first emitter's mass is recorded
            assert rule(policy, uniform, known, 9.0, [2.5, 1.5], True) == (0, 1, word(2.5))
            assert rule(policy, uniform, known, 9.0, [1.0, 1.0, NEXT], True) == (0, 1, word(1.0))


def test_a_clear_flag_stays_clear(policy):
    assert rule(policy, 0, 1, 1.0, [1.0]) == (0, 1, word(1.0))
    assert rule(policy, 0, 1, 1.0, [1.0, 1.0]) == (0, 1, word(1.0))
    assert rule(policy, 0, 0, 1.0, [1.0]) == (0, 0, word(1.0))
    assert rule(policy, 0, 1, 1.0, [NEXT]) == (0, 1, word(1.0))


def test_the_library_calls_the_header(hiplib):
    """sph_hip.hip keeps no second copy of the decision"""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "smoothed_particle_hydrodynamics_amd", "csrc", "sph_hip.hip")) as f:
        src = f.read()
    body = src[src.index("static void ports_mass_rule"):]
    body = body[:body.index("\n}\n")]
    assert "port_mass_rule(" in body and "memcmp" not in body and "for (" not in body
