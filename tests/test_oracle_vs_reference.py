"""The CPU restatement against the reference's own compiled sph.cpp.  Live where
oracle/_ref/libsphref.so can be loaded (`make -C oracle ref` where the reference tree exists; the
built library travels with the tree); elsewhere against what that library computed for the same
inputs, pinned in tests/golden/reference_pins.json (helpers.reference_pins: SHA-256 of every array,
exact numbers).  test_oracle_golden.py carries more pins of the same kind."""
import numpy as np
import pytest

import param_cases
from helpers import NONFINITE_SCENES, live_mask, pin_sha, reference_pins

CONSTANT_NAMES = ["h", "h2", "hscaled", "hscaled2", "hscaled6", "hscaled9", "htimes2", "htimes2inv",
                  "kernel1", "kernel2", "kernel3", "softening", "rho0", "stiffness", "viscosity",
                  "time_step", "cfl_limit", "cfl_limit2", "grav_const", "central_mass"]


def test_constructor_constants(oracle):
    """A0: every constant SPH::SPH() derives (reference src/sph.cpp:46-98)"""
    p = oracle.params_for_h(0.1)
    ref = reference_pins("constructor_constants", lambda R: {"constants": list(R.constants())})
    c = np.float32(ref["constants"])
    for i, nm in enumerate(CONSTANT_NAMES):
        assert np.float32(getattr(p, nm)) == c[i], nm
    assert list(np.float32(p.central_pos)) == list(c[20:23])
    assert np.float32(p.cell_size) == c[23]
    assert [np.float32(p.max_x), np.float32(p.max_y), np.float32(p.max_z)] == list(c[24:27])
    assert np.float32(p.sim_scale) == c[27] and np.float32(p.damping) == c[28]
    assert [p.cells_x, p.cells_y, p.cells_z] == [int(v) for v in c[29:32]]


def _ref_phases(p, n, cap):
    """the reference's phases one by one on its default scene, every intermediate result"""
    def run(R):
        out = {}
        R.configure(p, n)
        R.init_sphere()
        s = R.get_state()
        out.update(pos0=s["pos"], vel0=s["vel"], mass=s["mass"])
        R.voxelize()
        out["voxel_coords"], out["voxel_ids"] = R.get_voxels()
        out["grid_counts"] = R.get_grid_counts(32 ** 3)
        R.find_neighbors()
        nb, nd = R.get_lists()
        out["ncount"] = R.get_state()["ncount"]
        live = live_mask(out["ncount"], cap)
        out["nb_live"], out["nd_live"] = nb[live], nd[live]
        R.compute_density()
        out["rho"] = R.get_state()["rho"]
        R.compute_acceleration()
        out["acc"] = R.get_state()["acc"]
        R.integrate()
        s = R.get_state()
        out["pos"], out["vel"] = s["pos"], s["vel"]
        out["energy"] = R.energy()
        return out
    return run


@pytest.mark.parametrize("m", [8, 32, 96])
def test_ref_phases_bit_exact(oracle, m):
    """A0', A1-A6 phase by phase on the reference's default scene at N = m*1024"""
    p = oracle.params_for_h(0.1)
    n = m * 1024
    cap = p.examine_count
    ref = reference_pins("ref_phases_M%d" % m, _ref_phases(p, n, cap))
    pos, vel = oracle.init_sphere(p, n)
    assert pin_sha(pos) == ref["pos0"] and pin_sha(vel) == ref["vel0"]
    mass = np.ones(n, np.float32)
    assert pin_sha(mass) == ref["mass"]

    oc, oi, cs, ci = oracle.voxelize(p, pos)
    assert pin_sha(oc) == ref["voxel_coords"] and pin_sha(oi) == ref["voxel_ids"]
    assert pin_sha(np.diff(cs).astype(np.int32)) == ref["grid_counts"]

    onb, ond, ocnt = oracle.find_neighbors(p, pos, oc, cs, ci)
    assert pin_sha(ocnt) == ref["ncount"]
    live = live_mask(ocnt, cap)
    assert pin_sha(onb[live]) == ref["nb_live"] and pin_sha(ond[live]) == ref["nd_live"]

    orho = oracle.density_lists(p, cap, onb, ond, ocnt, mass)
    assert pin_sha(orho) == ref["rho"]

    oacc = oracle.accel_lists(p, cap, onb, ond, ocnt, pos, vel, mass, orho)
    assert pin_sha(oacc) == ref["acc"]

    oke, ope = oracle.integrate(p, pos, vel, oacc, mass)
    assert pin_sha(pos) == ref["pos"] and pin_sha(vel) == ref["vel"]
    assert [oke, ope] == ref["energy"]


def test_ref_five_whole_steps_through_SPH_step(oracle):
    """SPH::step() itself, five times, on a scene where the search finds many neighbours"""
    from test_oracle_golden import box_fill
    p = oracle.params_for_h(0.1)
    n = 20000
    pos = box_fill(n, (1.0, 1.0, 1.0), (2.4, 2.2, 2.3), 17)
    vel = box_fill(n, (-3.0,) * 3, (3.0,) * 3, 18)
    mass = np.ones(n, np.float32)

    def run(R):
        R.configure(p, n)
        R.set_state(pos, vel, mass)
        for _ in range(5):
            R.step()
        s = R.get_state()
        return {k: s[k] for k in ("pos", "vel", "rho", "acc", "ncount")}

    ref = reference_pins("five_whole_steps", run)
    for _ in range(5):
        out = oracle.step(p, pos, vel, mass, mode="ref")
    for name, a in (("pos", pos), ("vel", vel), ("rho", out["rho"]), ("acc", out["acc"]),
                    ("ncount", out["ncount"])):
        assert pin_sha(a) == ref[name], name
    assert out["ncount"].max() > 20


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_full_mode_against_reference_pair_functions(oracle, scale):
    """FULL mode: the oracle's lists (canonical order) fed to the reference's own
    computeDensity / computeAcceleration == the oracle's list-free FULL sums."""
    from test_oracle_golden import box_fill
    p = oracle.params_for_h(0.1)
    p.sim_scale = scale            # exercises the scaled branches (reference src/sph.cpp:668,847-849)
    p.sim_scale_inv = 1.0 / scale
    n = 15000
    pos = box_fill(n, (2.0, 2.0, 2.0), (3.3, 3.4, 3.2), 27)
    vel = box_fill(n, (-8.0,) * 3, (8.0,) * 3, 28)
    mass = (0.5 + box_fill(n, (0,) * 3, (1,) * 3, 29)[:n]).astype(np.float32)
    cap = 128
    nb, nd, cnt, worst = oracle.full_build_lists(p, pos, cap)
    assert worst <= cap and cnt.mean() > 20

    def run(R):
        R.configure(p, n)
        R.set_state(pos, vel, mass)
        R.set_lists(cap, nb, nd, cnt)
        R.compute_density()
        R.compute_acceleration()
        s = R.get_state()
        out = {"rho": s["rho"], "acc": s["acc"]}
        R.integrate()
        s = R.get_state()
        out.update(pos=s["pos"], vel=s["vel"], energy=R.energy())
        return out

    ref = reference_pins("full_pair_functions_scale%g" % scale, run)
    ids, cs, ci = oracle.full_cells(p, pos)
    orho, ocnt = oracle.full_density(p, pos, mass, cs, ci)
    oacc = oracle.full_accel(p, pos, vel, mass, orho, cs, ci)
    assert np.array_equal(ocnt, cnt)
    assert pin_sha(orho) == ref["rho"]
    assert pin_sha(oacc) == ref["acc"]
    opos, ovel = pos.copy(), vel.copy()
    energies = oracle.integrate(p, opos, ovel, oacc, mass)
    assert pin_sha(opos) == ref["pos"] and pin_sha(ovel) == ref["vel"]
    assert list(energies) == ref["energy"]


@pytest.mark.parametrize("case", NONFINITE_SCENES)
def test_full_mode_nonfinite_point_mass_term_against_reference(oracle, case):
    """A scene without a point mass (central_mass = 0, the dam-break) where a position or the central
    position is not finite: the term -G * 0 * (rs / d3) is NaN in a component whose rs is infinite and
    in every component once one rs is NaN, +-0 elsewhere - the oracle (the tolerance mode's checker)
    has that from the reference, through density, acceleration and the integration's second kick."""
    from helpers import nonfinite_scene
    p, pos, vel, mass = nonfinite_scene(case, oracle.params_for_h)
    n = mass.size
    cap = 128
    nb, nd, cnt, worst = oracle.full_build_lists(p, pos, cap)
    assert worst <= cap

    def run(R):
        R.configure(p, n)
        R.set_state(pos, vel, mass)
        R.set_lists(cap, nb, nd, cnt)
        R.compute_density()
        R.compute_acceleration()
        s = R.get_state()
        out = {"rho": s["rho"], "acc": s["acc"]}
        R.integrate()
        s = R.get_state()
        out.update(pos=s["pos"], vel=s["vel"], energy=R.energy())
        return out

    ref = reference_pins("full_nonfinite_point_mass_" + case, run)
    ids, cs, ci = oracle.full_cells(p, pos)
    orho, ocnt = oracle.full_density(p, pos, mass, cs, ci)
    oacc = oracle.full_accel(p, pos, vel, mass, orho, cs, ci)
    assert np.array_equal(ocnt, cnt)
    assert pin_sha(orho) == ref["rho"]
    assert pin_sha(oacc) == ref["acc"]
    opos, ovel = pos.copy(), vel.copy()
    energies = oracle.integrate(p, opos, ovel, oacc, mass)
    assert pin_sha(opos) == ref["pos"] and pin_sha(ovel) == ref["vel"]
    assert list(energies) == ref["energy"]
    acc = oacc.reshape(-1, 3)
    if case == "particles":
        # the NaN patterns the pins hold, spelled out
        assert np.isnan(acc[10, 0]) and np.isfinite(acc[10, 1:]).all()
        assert np.isnan(acc[20, 1]) and np.isfinite(acc[20, [0, 2]]).all()
        assert np.isnan(acc[30, 2]) and np.isfinite(acc[30, :2]).all()
        assert np.isnan(acc[40]).all() and np.isnan(acc[50]).all()
        others = np.setdiff1d(np.arange(n), [10, 20, 30, 40, 50])
        assert np.isfinite(acc[others]).all()
    elif case == "central_x_inf":
        # rs_x = -inf: x is inf / inf, y and z are finite / inf = 0
        assert np.isnan(acc[:, 0]).all() and np.isfinite(acc[:, 1:]).all()
    else:
        # rs_z = NaN: dot and d3 are NaN, and so is every component
        assert np.isnan(acc).all()


def _param_case_id(case):
    return case.name


@pytest.mark.parametrize("case", param_cases.CASES, ids=_param_case_id)
def test_ref_steps_on_constant_cases(oracle, case):
    """REF mode on every case of tests/param_cases.py: two whole SPH::step() calls of the reference
    (its list size through ref_set_examine_count) against two oracle steps.  With the walls on, the
    reference's own handleBoundaryConditions (defined, never called by step()) is applied after
    each step: what the oracle's integration does in place."""
    p, pos, vel, mass = param_cases.scene(oracle.params_for_h, case)
    n = mass.size

    def run(R):
        R.configure(p, n)
        R.set_state(pos, vel, mass)
        out = {}
        for s in range(2):
            old = R.get_state()["pos"]
            R.step()
            st = R.get_state()
            if p.apply_walls:
                v, q = R.boundary(old, st["vel"], p.time_step, st["pos"])
                R.set_state(q, v)
                st["pos"], st["vel"] = q, v
            for k in ("pos", "vel", "rho", "acc", "ncount"):
                out["%s%d" % (k, s)] = st[k]
            out["energy%d" % s] = R.energy()
        return out

    ref = reference_pins("param_case_ref_" + case.name, run)
    opos, ovel = pos.copy(), vel.copy()
    for s in range(2):
        out = oracle.step(p, opos, ovel, mass, mode="ref")
        for k, a in (("pos", opos), ("vel", ovel), ("rho", out["rho"]), ("acc", out["acc"]),
                     ("ncount", out["ncount"])):
            assert pin_sha(a) == ref["%s%d" % (k, s)], "%s step %d: %s" % (case.name, s, k)
        assert [out["ke"], out["pe"]] == ref["energy%d" % s], "%s step %d: energy" % (case.name, s)
    assert out["ncount"].max() <= case.overrides.get("examine_count", 32)


@pytest.mark.parametrize("case", param_cases.FULL_CASES, ids=_param_case_id)
def test_full_mode_on_constant_cases(oracle, case):
    """FULL mode on every case of tests/param_cases.py, two steps: the oracle's lists fed to the
    reference's computeDensity / computeAcceleration, then its integrate (and, with the walls on, its
    handleBoundaryConditions), against the oracle's list-free FULL step."""
    p, pos, vel, mass = param_cases.scene(oracle.params_for_h, case)
    n = mass.size
    cap = 256
    lists = []
    states = [(pos.copy(), vel.copy())]
    opos, ovel = pos.copy(), vel.copy()
    outs = []
    for s in range(2):
        nb, nd, cnt, worst = oracle.full_build_lists(p, opos, cap)
        assert worst <= cap
        lists.append((nb, nd, cnt))
        outs.append(oracle.step(p, opos, ovel, mass, mode="full"))
        assert np.array_equal(outs[-1]["ncount"], cnt)
        states.append((opos.copy(), ovel.copy()))

    def run(R):
        R.configure(p, n)
        R.set_state(pos, vel, mass)
        out = {}
        for s in range(2):
            old = R.get_state()["pos"]
            R.set_lists(cap, *lists[s])
            R.compute_density()
            R.compute_acceleration()
            st = R.get_state()
            out["rho%d" % s], out["acc%d" % s] = st["rho"], st["acc"]
            R.integrate()
            st = R.get_state()
            if p.apply_walls:
                v, q = R.boundary(old, st["vel"], p.time_step, st["pos"])
                R.set_state(q, v)
                st["pos"], st["vel"] = q, v
            out["pos%d" % s], out["vel%d" % s] = st["pos"], st["vel"]
            out["energy%d" % s] = R.energy()
        return out

    ref = reference_pins("param_case_full_" + case.name, run)
    for s in range(2):
        what = "%s step %d: " % (case.name, s)
        assert pin_sha(outs[s]["rho"]) == ref["rho%d" % s], what + "rho"
        assert pin_sha(outs[s]["acc"]) == ref["acc%d" % s], what + "acc"
        assert pin_sha(states[s + 1][0]) == ref["pos%d" % s], what + "pos"
        assert pin_sha(states[s + 1][1]) == ref["vel%d" % s], what + "vel"
        assert [outs[s]["ke"], outs[s]["pe"]] == ref["energy%d" % s], what + "energy"
