"""GPU: the step monitor (include/sph_hip.h: step monitor).  k_monitor_particles, k_monitor_pairs and k_monitor_finish
against the numpy restatement tests/monitor_emulation.py, bit for bit: on the scalars' 2 001-particle block (eight
workgroups, the last with one live lane; seeded velocities, gravity and walls on) with carried scalars, their
sources, cohesion and a buoyancy, against the oracle's step chained with the committed restatements; in FULL_FAST and
everywhere else against the restatement applied to the context's own downloaded state.  Every field of a row is a
maximum, a minimum, a count or an integer sum, so a row is the same bytes on every route; the routes are set by
switches that are read at context creation, so each runs in a child process of its own (this file with a route
name)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cohesion_emulation as CE
import monitor_emulation as ME
import scalar_emulation as SC
import scale_cases
from helpers import to_oracle_params
from test_gpu_scalars import N, api_sources, block_scene, block_sources, mode_of, same

pytestmark = pytest.mark.gpu

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GAMMA = 0.02
Q = -24
ROUTES = {
    "default": {},
    "untiled": {"SPH_HIP_UNTILED": "1"},
    "lists_none": {"SPH_HIP_TILE_CAP": "256"},     # no tile of this scene fits: every workgroup is LISTS_NONE
    "lists_some": {"SPH_HIP_LIST_CAP": "16"},      # most particles have more than 16 neighbours: NLIST_NO_LIST lanes
    "no_fused_integrate": {"SPH_HIP_NO_FUSED_INTEGRATE": "1"},
    "scalar_rows": {"SPH_HIP_SCALAR_ROWS": "1"},   # the scalar pass and the monitor's pair pass walk the cell rows
}
ROUTE_SWITCHES = ("SPH_HIP_UNTILED", "SPH_HIP_NO_FUSED_INTEGRATE", "SPH_HIP_NO_PREHASH", "SPH_HIP_TILE_CAP",
                  "SPH_HIP_LIST_CAP", "SPH_HIP_TILE_CAP_ACCEL", "SPH_HIP_TILE_CAP_DENSITY", "SPH_HIP_CHUNKED",
                  "SPH_HIP_SCALAR_ROWS")


def start_all(sph, pos, vel, mass, T, kappa, sources, buoyancy, gamma=GAMMA):
    """the block with everything that stands between the acceleration pass and the integrate"""
    sph.setParticles(pos, vel, mass)
    sph.setScalars(T, kappa)
    sph.setScalarSources(api_sources(sources))
    sph.setBuoyancy(buoyancy)
    sph.setCohesion(gamma)


def downloaded(sph):
    part = sph.getParticles()
    return dict(pos=part.mPosition.copy(), vel=part.mVelocity.copy(), acc=part.mAcceleration.copy(),
                rho=part.mDensity.copy(), ncount=part.mNeighborCount.copy())


def own_row(sph, p, before, mass, quantum_log2=Q, scalars=True):
    """The restatement's row of the step just taken from `before` = (pos, vel), fed with the context's own
    downloaded state and scalars."""
    return ME.step_row(p, (before[0], before[1], mass), downloaded(sph), quantum_log2, sph.getScalars() if scalars else None)


def differing(got, want):
    names = ME.same_rows(got, want)
    return [(nm, got[nm].tolist(), np.asarray(want[nm]).tolist()) for nm in names]


# ---- 1. FULL single steps against the oracle chained with the restatements -----------------------------------------
def test_full_single_steps_equal_the_composed_restatement(oracle, hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_buoyancy import block_buoyancy, emu_of
    p, pos, vel, mass, T, kappa = block_scene()
    sources, buoyancy = block_sources(p), block_buoyancy()
    b = emu_of(buoyancy, p)
    op = to_oracle_params(p)
    want = []
    with S.SPH(N, p) as sph:
        start_all(sph, pos, vel, mass, T, kappa, sources, buoyancy)
        sph.recordMonitor(3)
        for k in range(3):
            out = CE.step(oracle, p, pos, vel, mass, GAMMA, T, kappa, sources, b)
            _, cs, ci = oracle.full_cells(op, np.ascontiguousarray(pos, F32))
            _, cnt = oracle.full_density(op, np.ascontiguousarray(pos, F32), mass, cs, ci)
            after = dict(pos=out["pos"], vel=out["vel"], acc=out["acc"], rho=out["rho"], ncount=cnt)
            want.append(ME.step_row(p, (pos, vel, mass), after, Q, out["T"]))
            sph.step()
            got = downloaded(sph)
            assert same(got["pos"], out["pos"]) and same(got["acc"], out["acc"]) and same(sph.getScalars(), out["T"])
            pos, vel, T = got["pos"], got["vel"], sph.getScalars()
        rec = sph.getMonitorRecord()
    assert len(rec) == 3 and rec.steps.tolist() == [1, 2, 3] and rec.quantum_log2 == Q
    for k in range(3):
        assert differing(rec.rows[k], want[k]) == [], "row %d" % k
    # the rows say something: everything is valid, nothing is wrong, and the figures are the block's
    assert (rec.flags == 3).all() and (rec.live == N).all() and rec.first_bad() is None
    assert (rec.bad == 0).all() and (rec.bad_id_min == ME.NO_ID).all() and (rec.skipped == 0).all()
    assert (rec.v2_max > 0).all() and (rec.a2_max > 0).all() and (rec.rho_min > 0).all() and (rec.rho_max > rec.rho_min).all()
    assert (rec.ncount_max > 16).all() and (rec.s_max > 0).all()
    assert np.allclose(rec.mass, float(mass.astype(np.float64).sum()), rtol=1e-6)
    assert (rec.rows["momentum"] != 0).any(1).all() and (rec.rows["kinetic"] > 0).all()
    assert rec.rows[0].tobytes() != rec.rows[1].tobytes()
    # kappa is a tenth of the bulk's stability limit
    assert 0.0 < np.nanmax(rec.diffusion_number(kappa, p.time_step)) < 1.0


# ---- 2. FULL_FAST: the context's own state through the restatement ---------------------------------------------------
def test_fast_rows_from_the_own_state_and_s_max_equals_fulls(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_buoyancy import block_buoyancy
    p, pos, vel, mass, T, kappa = block_scene()
    sources, buoyancy = block_sources(p), block_buoyancy()
    rows = {}
    for mode in ("full", "fast"):
        with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
            start_all(sph, pos, vel, mass, T, kappa, sources, buoyancy)
            sph.recordMonitor(2)
            before = (pos, vel)
            for k in range(2):
                sph.step()
                want = own_row(sph, p, before, mass)
                got = sph.getMonitorRecord()
                assert len(got) == k + 1
                assert differing(got.rows[k], want) == [], (mode, k)
                st = downloaded(sph)
                before = (st["pos"], st["vel"])
            rows[mode] = sph.getMonitorRecord().rows
    # step 1 starts from the same state in both arithmetics: densities and members are identical by contract
    for nm in ("s_max", "pair_bad", "rho_max", "rho_min", "ncount_max", "lone", "mass", "live"):
        assert rows["full"][0][nm].tobytes() == rows["fast"][0][nm].tobytes(), nm


# ---- 3. routes: one child process per setting ------------------------------------------------------------------------
def route_run(route="default"):
    """Three single steps each of: the block with scalars, sources, buoyancy and cohesion (FULL); the block with
    scalars alone, whose step may fuse its integrate (FULL and FULL_FAST); the block without scalars (FULL).  The rows'
    bytes, the neighbour counts and the tile statistics."""
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_buoyancy import block_buoyancy
    p, pos, vel, mass, T, kappa = block_scene()
    sources, buoyancy = block_sources(p), block_buoyancy()
    result, stats = {}, {}
    for tag, mode in (("all", "full"), ("scalars", "full"), ("scalars_fast", "fast"), ("plain", "full")):
        with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
            if tag == "all":
                start_all(sph, pos, vel, mass, T, kappa, sources, buoyancy)
            else:
                sph.setParticles(pos, vel, mass)
                if tag != "plain":
                    sph.setScalars(T, kappa)
            sph.recordMonitor(3)
            for _ in range(3):
                sph.step()
            rec = sph.getMonitorRecord()
            assert len(rec) == 3
            result[tag] = np.frombuffer(rec.rows.tobytes(), np.uint8)
            result[tag + "_counts"] = sph.getParticles().mNeighborCount.copy()
            stats[tag] = sph.tileStats() if route != "untiled" else {}
    result["stats"] = json.dumps(stats)
    return result


@pytest.fixture(scope="module")
def default_route(hiplib):
    return route_run()


@pytest.mark.parametrize("route", list(ROUTES))
def test_every_route_gives_the_same_bytes(default_route, route, tmp_path):
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
            assert np.array_equal(got[name], default_route[name]), (route, name, differing(
                np.frombuffer(got[name].tobytes(), ME.ROW), np.frombuffer(default_route[name].tobytes(), ME.ROW))
                if "counts" not in name else None)
    rows = np.frombuffer(got["all"].tobytes(), ME.ROW)
    assert (rows["flags"] == 3).all() and (rows["live"] == N).all() and (rows["s_max"] > 0).all()
    assert (np.frombuffer(got["plain"].tobytes(), ME.ROW)["flags"] == 0).all()
    # the setting produced the route it is there for, or the case proves nothing (SPH_HIP_NO_FUSED_INTEGRATE and
    # SPH_HIP_SCALAR_ROWS leave the tile statistics as they are: no statistic reports them)
    stats = json.loads(str(got["stats"]))
    for tag in ("all", "scalars", "scalars_fast", "plain"):
        st, counts = stats[tag], got[tag + "_counts"]
        if route in ("default", "no_fused_integrate", "scalar_rows"):
            assert st["workgroups"] == 8 and st["untiled_density"] == 0 and st["wide_entries"] == 0
            assert counts.max() <= st["list_capacity"]                       # every lane has its list
        elif route == "lists_none":
            assert st["capacity_density"] == 256 and st["largest_tile"] > 256 and st["workgroups"] == 8
            assert st["untiled_density"] >= 7
        elif route == "lists_some":
            assert st["list_capacity"] == 16 and st["untiled_density"] == 0
            assert (counts > 16).sum() > 100 and (counts <= 16).sum() > 100
        else:
            assert route == "untiled" and st == {}       # (an untiled context keeps no tile statistics)


# ---- 4. queueing ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["full", "fast"])
def test_queued_steps_fill_the_rows_single_steps_fill(hiplib, mode):
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_buoyancy import block_buoyancy
    p, pos, vel, mass, T, kappa = block_scene()
    sources, buoyancy = block_sources(p), block_buoyancy()
    recs = {}
    for how in ("queued", "single", "every1"):
        with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
            start_all(sph, pos, vel, mass, T, kappa, sources, buoyancy)
            sph.recordMonitor(6 if how == "every1" else 3, every=1 if how == "every1" else 2)
            if how == "queued":
                sph.run(6)
            else:
                for _ in range(6):
                    sph.step()
            recs[how] = sph.getMonitorRecord()
    assert len(recs["queued"]) == 3 and recs["queued"].steps.tolist() == [1, 3, 5] == recs["single"].steps.tolist()
    assert recs["queued"].rows.tobytes() == recs["single"].rows.tobytes()
    assert recs["every1"].steps.tolist() == [1, 2, 3, 4, 5, 6]
    assert recs["every1"].rows[[0, 2, 4]].tobytes() == recs["queued"].rows.tobytes()
    assert recs["every1"].rows[1].tobytes() != recs["every1"].rows[2].tobytes()


def test_a_setter_between_queued_runs_does_not_reach_the_rows_already_queued(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, T, kappa = block_scene()
    rows = {}
    for how in ("setter", "single", "never"):
        with S.SPH(N, p) as sph:
            sph.setParticles(pos, vel, mass)
            sph.setScalars(T, kappa)
            sph.setCohesion(GAMMA)
            sph.recordMonitor(3)
            if how == "setter":
                sph.run(2)
                sph.setCohesion(-0.5 * GAMMA)
                sph.run(1)
            elif how == "single":
                sph.step()
                sph.step()
                sph.synchronize()
                sph.setCohesion(-0.5 * GAMMA)
                sph.step()
            else:
                sph.run(3)
            rows[how] = sph.getMonitorRecord().rows
    assert rows["setter"].tobytes() == rows["single"].tobytes()
    assert rows["setter"][:2].tobytes() == rows["never"][:2].tobytes()
    assert rows["setter"][2]["a2_max"] != rows["never"][2]["a2_max"] or \
        rows["setter"][2].tobytes() != rows["never"][2].tobytes()               # (the new gamma did act on step 3)


@pytest.mark.parametrize("mode", ["full", "fast"])
def test_a_recording_changes_no_particle(hiplib, mode):
    """20 steps with and without a recording (every step recorded; every third): byte for byte the same state,
    counts, scalars and energies."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, T, kappa = block_scene()
    out = []
    for record in (None, 1, 3):
        with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
            sph.setParticles(pos, vel, mass)
            sph.setScalars(T, kappa)
            if record:
                sph.recordMonitor(20, every=record)
            sph.run(19)
            sph.step()
            st = downloaded(sph)
            out.append([st[nm] for nm in ("pos", "vel", "acc", "rho", "ncount")] + [sph.getScalars()] + list(sph.energy()))
            if record:
                assert len(sph.getMonitorRecord()) == (20 if record == 1 else 7)
    for other in out[1:]:
        for a, c in zip(out[0], other):
            assert np.asarray(a).tobytes() == np.asarray(c).tobytes()


# ---- 5. edges of the grid -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_lane_and_workgroup_boundaries(hiplib, n):
    """The first n particles of the block with their scalars: a single lane, a workgroup short of one lane, a full
    one, and one lane into the second - a finish over one and over two partials of either kind."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, T, kappa = block_scene()
    pos, vel, mass, T = pos[:3 * n].copy(), vel[:3 * n].copy(), mass[:n].copy(), T[:n].copy()
    with S.SPH(n, p) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setScalars(T, kappa)
        sph.recordMonitor(2)
        before = (pos, vel)
        for k in range(2):
            sph.step()
            want = own_row(sph, p, before, mass)
            got = sph.getMonitorRecord().rows[k]
            assert differing(got, want) == [], (n, k)
            assert got["live"] == n and got["flags"] == 3
            st = downloaded(sph)
            before = (st["pos"], st["vel"])
        if n == 1:
            assert got["lone"] == 1 and got["ncount_max"] == 0 and got["s_max"] == 0.0


def test_the_stride_loop_runs_twice(hiplib):
    """300 000 particles, one step, no scalars: 1 172 workgroups' worth of slots on the bounded grid of 1 024, so the
    first 37 856 lanes visit a second slot.  The per-particle fields against the restatement on the downloaded state."""
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    n = 300000
    assert n > 1024 * 256
    p, pos, vel, mass = scenes.dam_break(n, speed=0.3)
    p.apply_gravity = 1
    p.apply_walls = 1
    p.gravity[0], p.gravity[1], p.gravity[2] = 0.0, -9.81, 0.0
    with S.SPH(n, p) as sph:
        sph.setParticles(pos, vel, mass)
        sph.recordMonitor(1)
        sph.step()
        st = downloaded(sph)
        rec = sph.getMonitorRecord()
    want = ME.step_row(p, (pos, vel, mass), st, Q, None)
    assert differing(rec.rows[0], want) == []
    assert rec.live[0] == n and rec.flags[0] == 0 and rec.bad[0] == 0 and rec.skipped[0] == 0
    assert rec.rows["mass"][0] == int(n) << 24 and rec.v2_max[0] > 0


# ---- 6. off unit scale ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["SCALED", "SHELL"])
def test_off_unit_scale_against_the_restatement(hiplib, flavour):
    """scale_cases.block_scene (6 000 particles: a compressed block, a layer, a spray without neighbours) with the
    walls on.  Under SHELL there are members beyond hscaled, whose weights are negative: particles whose S_p is
    negative exist, and the ordered key puts them below the others."""
    import smoothed_particle_hydrodynamics_amd as S
    import sample_emulation as SE
    p, pos, vel, mass = scale_cases.block_scene(flavour, walls=True)
    assert not SE.unit_scale(p)
    n = mass.size
    rng = np.random.default_rng(3)
    T = rng.uniform(-1.0, 1.0, (n, 4)).astype(F32)
    kappa = np.array([0.0, 1.0e-7, 2.0e-7, 1.0e-7], F32)
    with S.SPH(n, p) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setScalars(T, kappa)
        sph.setCohesion(GAMMA)
        sph.recordMonitor(2)
        before = (pos, vel)
        for k in range(2):
            sph.step()
            st = downloaded(sph)
            want = ME.step_row(p, (before[0], before[1], mass), st, Q, sph.getScalars())
            got = sph.getMonitorRecord().rows[k]
            assert differing(got, want) == [], (flavour, k)
            if k == 0:
                sums = ME.pair_sums(p, before[0], before[1], mass, st["rho"])
                if flavour == "SHELL":
                    assert (sums < 0).sum() > 0                 # negative sums took part in the maximum
                assert got["lone"] > 0 and got["s_max"] == sums[np.isfinite(sums)].max()
            before = (st["pos"], st["vel"])


# ---- 7. a run that goes wrong, made from finite input only ----------------------------------------------------------------
def test_a_diffusivity_beyond_the_limit_shows_in_the_row(hiplib):
    """Channel 2 with a diffusivity of 3e38, which setScalars accepts: after one step the restatement itself gives
    channels that are not finite.  scalar_bad is the restatement's count, the other channels' ranges are those of the
    run with the block's own diffusivity, no particle is bad, and first_bad() names the row."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, T, kappa = block_scene()
    wild = kappa.copy()
    wild[2] = F32(3.0e38)
    rows = {}
    for tag, kap in (("tame", kappa), ("wild", wild)):
        with S.SPH(N, p) as sph:
            sph.setParticles(pos, vel, mass)
            sph.setScalars(T, kap)
            sph.recordMonitor(4)
            sph.step()
            rho = sph.getParticles().mDensity.copy()
            T_emulated = SC.step(p, pos, vel, mass, rho, T, kap, [])
            T_got = sph.getScalars()
            assert same(T_got, T_emulated)
            rec = sph.getMonitorRecord()
            assert differing(rec.rows[0], own_row(sph, p, (pos, vel), mass)) == []
            rows[tag] = (rec, T_emulated)
    rec, T_emulated = rows["wild"]
    lost = int((~np.isfinite(T_emulated)).any(1).sum())
    assert lost > N // 2 and np.isfinite(T_emulated[:, [0, 1, 3]]).all()
    assert rec.scalar_bad[0] == lost and rec.bad[0] == 0 and rec.pair_bad[0] == 0 and rec.first_bad() == 0
    tame = rows["tame"][0]
    assert tame.first_bad() is None and tame.scalar_bad[0] == 0
    for ch in (0, 1, 3):
        assert rec.scalar_min[0, ch].tobytes() == tame.scalar_min[0, ch].tobytes()
        assert rec.scalar_max[0, ch].tobytes() == tame.scalar_max[0, ch].tobytes()
    for nm in ("s_max", "v2_max", "a2_max", "rho_max", "rho_min", "momentum", "kinetic", "mass"):
        assert rec.rows[nm][0].tobytes() == tame.rows[nm][0].tobytes(), nm
    # the diffusion number said so beforehand, and the suggestion would have kept the step convex
    assert rec.diffusion_number(wild, p.time_step)[0, 2] > 1e30
    assert rec.suggest_time_step(p, wild) * float(wild[2]) * float(rec.s_max[0]) <= 0.5 * (1 + 1e-12)


# ---- 8. the remaining host behaviour ---------------------------------------------------------------------------------
def test_flags_and_what_the_recording_survives(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, T, kappa = block_scene()
    with S.SPH(N, p) as sph:
        sph.setParticles(pos, vel, mass)
        assert len(sph.getMonitorRecord()) == 0                    # no recording: no rows, no refusal
        sph.recordMonitor(8, quantum_log2=-20)
        sph.step()                                                 # row 0: no scalars
        sph.setScalars(T, kappa)
        before = downloaded(sph)
        sph.step()                                                 # row 1: scalars
        want1 = own_row(sph, p, (before["pos"], before["vel"]), mass, -20)
        sph.setScalars(None)
        sph.step()                                                 # row 2: none again
        sph.setGravity(sph.getGravity())                           # (sph_hip_set_params)
        sph.setArithmetic(S.ARITH_FAST)
        sph.step()                                                 # row 3: behind set_params and set_arithmetic
        sph.setArithmetic(S.ARITH_EXACT)
        sph.setParticles(pos[:3 * 700].copy(), vel[:3 * 700].copy(), mass[:700].copy())      # an upload
        sph.step()                                                 # row 4: the new particles
        want4 = ME.step_row(p, (pos[:3 * 700], vel[:3 * 700], mass[:700]), downloaded(sph), -20, None)
        rec = sph.getMonitorRecord()
        assert len(rec) == 5 and rec.steps.tolist() == [1, 2, 3, 4, 5] and rec.quantum_log2 == -20
        assert rec.flags.tolist() == [0, 3, 0, 0, 0] and rec.live.tolist() == [N, N, N, N, 700]
        assert differing(rec.rows[1], want1) == [] and differing(rec.rows[4], want4) == []
        for r in (0, 2, 3, 4):                                     # fields that are not valid hold zeros
            row = rec.rows[r]
            assert not row["scalar_min"].any() and not row["scalar_max"].any()
            assert row["scalar_bad"] == 0 and row["pair_bad"] == 0 and row["s_max"].tobytes() == b"\0\0\0\0"
        assert np.allclose(rec.mass[:4], float(mass.astype(np.float64).sum()), rtol=1e-5)
        # rows = 0 stops and frees; steps after it record nothing; a new recording counts from 1 again
        sph.recordMonitor(0)
        sph.step()
        assert len(sph.getMonitorRecord()) == 0
        sph.recordMonitor(2, every=3)
        sph.run(7)
        rec = sph.getMonitorRecord()
        assert len(rec) == 2 and rec.steps.tolist() == [1, 4]      # the rows are full: steps 7 .. record nothing
        sph.run(3)
        assert sph.getMonitorRecord().rows.tobytes() == rec.rows.tobytes()


def test_refusals_and_the_getters_range(hiplib):
    import ctypes as C
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    from smoothed_particle_hydrodynamics_amd.ports import Sink
    from smoothed_particle_hydrodynamics_amd.slab import HipSlab
    p, pos, vel, mass, T, kappa = block_scene()

    def refused(call, *args, text, **kw):
        with pytest.raises(S.SphHipError) as e:
            call(*args, **kw)
        assert text in str(e.value), str(e.value)

    with S.SPH(N, p) as sph:
        sph.setParticles(pos, vel, mass)
        sph.recordMonitor(3)
        sph.step()
        refused(sph.recordMonitor, -1, text="rows must be >= 0")
        refused(sph.recordMonitor, 4, every=0, text="every must be >= 1")
        refused(sph.recordMonitor, 4, quantum_log2=33, text="quantum_log2 must be in [-64, 32]")
        refused(sph.recordMonitor, 4, quantum_log2=-65, text="quantum_log2 must be in [-64, 32]")
        sph.step()
        rec = sph.getMonitorRecord()
        assert len(rec) == 2 and rec.steps.tolist() == [1, 2]      # a refused call keeps the recording
        # the getter's range
        out = np.zeros(3, ME.ROW)
        steps = np.zeros(3, np.int32)
        assert sph.call("sph_hip_get_monitor_record", 1, 1, out.ctypes.data_as(C.c_void_p),
                        steps.ctypes.data_as(C.c_void_p)) == 2
        assert out[0].tobytes() == rec.rows[1].tobytes() and steps[0] == 2
        assert sph.call("sph_hip_get_monitor_record", 2, 0, None, None) == 2
        for first, n in ((0, 3), (2, 1), (-1, 1), (0, -1)):
            refused(sph.call, "sph_hip_get_monitor_record", first, n, out.ctypes.data_as(C.c_void_p), None,
                    text="the range leaves the rows filled so far")
        # ports both ways
        sink = Sink((0.9, 0.9, 0.9), (1.0, 1.0, 1.0))
        refused(sph.setPorts, [], [sink], text="a context with a step monitor cannot have ports")
        sph.setPorts([], [])                                       # (clearing ports is no port)
        sph.recordMonitor(0)
        sph.setPorts([], [sink])
        refused(sph.recordMonitor, 3, text="a context with ports cannot keep a step monitor")
        sph.recordMonitor(0)                                       # stopping is never refused
    # REF mode
    rp, rpos, rvel, rmass = scenes.dense_block(512)
    with S.SPH(512, rp, mode=S.MODE_REF) as sph:
        sph.setParticles(rpos, rvel, rmass)
        refused(sph.recordMonitor, 3, text="FULL and FULL_FAST contexts only")
        sph.recordMonitor(0)
    # a slab context
    with HipSlab(p, 0, p.full_cells_z // 2, 4096, 1024, has_left=False) as slab:
        with pytest.raises(S.SphHipError, match="slab contexts"):
            slab.call("sph_hip_record_monitor", 3, 1, Q)
        slab.call("sph_hip_record_monitor", 0, 1, Q)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    np.savez(sys.argv[2], **route_run(sys.argv[1]))
