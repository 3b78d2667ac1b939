"""GPU, the breaking dam against the oracle: bench.py's breaking_dam side record - the 4M-particle column
with uniform gravity and walls - as it falls, at its peak of compression and at the steps bench.py times.

Every other 4M oracle window (test_gpu_full_size.py) looks at a column without gravity, at ~32
neighbours.  Here the scene compresses to a mean of well over 100 neighbours, and the adaptive machinery
fires on its own: lists grow, the density pass gives workgroups up to the untiled route, the list-driven
acceleration route reads blocks of eight entries, particles outgrow their lists, capacity levels move
from step to step.  Two trajectories, exact and tolerance-mode arithmetic, are each run on ONE context
that is never re-uploaded, so that the routes and capacities are the ones the run chose itself.  The
checkpoints are chosen on each trajectory by its own neighbour statistics (a first pass), and a second
pass from the same upload - asserted to reach them with the same statistics - downloads the state there,
takes one step and downloads the results.  Downloads do not perturb a run (test_gpu_sample.py,
test_sampling_does_not_change_the_trajectory).

Against the oracle, on a z-band in the fluid and on the band against the z = 0 wall (test_gpu_full_size.
oracle_window: the band's particles and everything within 2h + margin of it):
  * exact: count, density, acceleration, position and velocity of every interior particle bit for bit;
  * tolerance mode: counts and densities identical; forces, velocities and positions to the bar of
    test_gpu_full_fast.py with its non-finite rule and its cancellation clause (scale: the oracle's
    magnitude sums on the window), which prints how many particles took it.
At the peak the tolerance-mode pre-state is also stepped with the exact arithmetic in a fresh context:
all 4M counts and densities identical, the same non-finite pattern, at most FORCE_COND_SHARE of the
particles beyond 1e-4 relative.
"""
import numpy as np
import pytest

from helpers import finite_parts, nonfinite_mismatch, to_oracle_params, vec_rel
from test_sample_cpu import policy  # noqa: F401  (the g++ shim of sample_policy.h)

pytestmark = pytest.mark.gpu

N = 4 * 1024 * 1024
LAST = 511                       # bench.py times steps 500-520
PEAK_RANGE = (380, 480)          # the worst 20-step windows of the transient (profiles/r4_dam_transient_windows.txt)
BANDS = {"interior": (np.float32(0.40), np.float32(0.42)),
         "wall": (np.float32(-np.inf), np.float32(0.02))}    # against z = 0, and whatever is below it


def dam_scene():
    """exactly bench.breaking_dam's scene"""
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dam_break(N)
    p.apply_gravity = 1
    p.apply_walls = 1
    p.gravity[0], p.gravity[1], p.gravity[2] = 0.0, -9.81, 0.0
    return p, pos, vel, mass


def choose_checkpoints(mean):
    """mean[s]: the mean neighbour count after step s + 1 (neighborStats).  -> {name: steps taken
    before the checkpoint's step}"""
    start = mean[0]
    falling = next((s for s in range(60, 300) if mean[s] >= 1.5 * start), None)   # the column has begun to compress
    assert falling is not None, "the column never compressed by half before step 300: %s" % mean[60:300:20]
    peak = max(range(*PEAK_RANGE), key=lambda s: (mean[s], -s))
    return {"falling": falling, "peak": peak, "bench": LAST - 1}


@pytest.fixture(scope="module")
def dam(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = dam_scene()
    out = dict(p=p, mass=mass)
    for name, mode in (("exact", S.MODE_FULL), ("fast", S.MODE_FULL_FAST)):
        with S.SPH(N, p, mode=mode) as sph:                    # pass 1: the statistics
            sph.setParticles(pos, vel, mass)
            sph.setTiming(S.TIMING_OFF)
            mean = []
            for _ in range(LAST):
                sph.step()
                mean.append(sph.neighborStats()[0])
        at = choose_checkpoints(mean)
        cps = {}
        with S.SPH(N, p, mode=mode) as sph:                    # pass 2: the checkpoints
            sph.setParticles(pos, vel, mass)
            sph.setTiming(S.TIMING_OFF)
            done = 0
            for cp, steps in sorted(at.items(), key=lambda kv: kv[1]):
                sph.run(steps - done)
                part = sph.getParticles()
                pre = dict(pos0=part.mPosition.copy(), vel0=part.mVelocity.copy())
                sph.step()
                done = steps + 1
                part = sph.getParticles()
                assert sph.neighborStats()[0] == mean[steps], "%s %s: pass 2 is not pass 1" % (name, cp)
                cps[cp] = dict(pre, p=p, mass=mass, step=steps, mean=float(part.mNeighborCount.mean()),
                               pos=part.mPosition.copy(), vel=part.mVelocity.copy(), rho=part.mDensity.copy(),
                               acc=part.mAcceleration.copy(), ncount=part.mNeighborCount.copy(),
                               tile=sph.tileStats(), energy=sph.energy())
        out[name] = dict(mean=mean, at=at, cps=cps)
    return out


def test_checkpoints_by_statistics(dam):
    for name in ("exact", "fast"):
        d = dam[name]
        m, at = d["mean"], d["at"]
        print("%s: start mean %d; falling step %d (mean %d), peak step %d (mean %d), bench step %d (mean %d)" % (
            name, m[0], at["falling"], m[at["falling"]], at["peak"], m[at["peak"]], at["bench"], m[at["bench"]]))
        assert 30 <= m[0] <= 33                                          # the column at rest: ~32 by construction
        assert m[at["falling"]] >= 1.5 * m[0] and at["falling"] < at["peak"]
        assert m[at["peak"]] > 100                                       # the compressed dam (~172)
        assert m[at["bench"]] < m[at["peak"]]                           # the flow has relaxed again
        for cp, c in d["cps"].items():
            assert c["step"] == at[cp]
            assert np.isfinite(c["acc"]).all() and np.isfinite(c["pos"]).all() and np.isfinite(c["rho"]).all()
            assert np.isfinite(c["energy"]).all()
            assert c["ncount"].sum() % 2 == 0                            # d2(i,j) == d2(j,i): symmetric relation


def test_peak_route_mix_fired(dam):
    """the organic route mix at the peak: grown lists, untiled density workgroups, particles whose count
    exceeds their list"""
    for name in ("exact", "fast"):
        c = dam[name]["cps"]["peak"]
        t = c["tile"]
        listless = int((c["ncount"] > t["list_capacity"]).sum())
        print("%s peak (step %d): mean neighbours %.1f, max %d; list_capacity %d, untiled_density %d, "
              "untiled_acceleration %d, largest_tile %d, wide_entries %d, capacity levels %d/%d, particles "
              "beyond their list %d" % (name, c["step"], c["mean"], int(c["ncount"].max()), t["list_capacity"],
                                        t["untiled_density"], t["untiled_acceleration"], t["largest_tile"],
                                        t["wide_entries"], t["capacity_density"], t["capacity_acceleration"], listless))
        if name == "fast":                  # the route mix bench.py's breaking dam times
            assert t["list_capacity"] >= 510
            assert t["untiled_density"] > 0
            assert c["mean"] > 100


def window_refs(oracle, c, band):
    from test_gpu_full_size import oracle_window
    z0, z1 = BANDS[band]
    sub, inner, ref, spos, svel, smass, before = oracle_window(oracle, c, z0, z1)
    assert inner.sum() > 20000
    return sub, inner, ref, spos, svel, smass, before


@pytest.mark.parametrize("band", sorted(BANDS))
@pytest.mark.parametrize("cp", ["falling", "peak", "bench"])
def test_exact_window_matches_oracle(oracle, dam, cp, band):
    import time
    c = dam["exact"]["cps"][cp]
    t0 = time.perf_counter()
    sub, inner, ref, spos, svel, _, _ = window_refs(oracle, c, band)
    ids = sub[inner]
    print("exact %s (step %d), %s band: %d interior of %d particles, oracle %.1f s" % (
        cp, c["step"], band, ids.size, sub.size, time.perf_counter() - t0))
    assert np.array_equal(c["ncount"][ids], ref["ncount"][inner])
    assert np.array_equal(c["rho"][ids], ref["rho"][inner])
    assert np.array_equal(c["acc"].reshape(-1, 3)[ids], ref["acc"].reshape(-1, 3)[inner])
    assert np.array_equal(c["pos"].reshape(-1, 3)[ids], spos.reshape(-1, 3)[inner])
    assert np.array_equal(c["vel"].reshape(-1, 3)[ids], svel.reshape(-1, 3)[inner])


@pytest.mark.parametrize("band", sorted(BANDS))
@pytest.mark.parametrize("cp", ["falling", "peak", "bench"])
def test_fast_window_against_oracle(oracle, dam, cp, band):
    import time
    from types import SimpleNamespace
    from test_gpu_full_fast import CLAUSE_USED, check_fast, check_fast_position, check_fast_velocity
    c = dam["fast"]["cps"][cp]
    p = c["p"]
    t0 = time.perf_counter()
    sub, inner, ref, spos, svel, smass, (bpos, bvel) = window_refs(oracle, c, band)
    t1 = time.perf_counter()
    ids = sub[inner]
    part = SimpleNamespace(mNeighborCount=c["ncount"][ids], mDensity=c["rho"][ids],
                           mAcceleration=np.ascontiguousarray(c["acc"].reshape(-1, 3)[ids]).reshape(-1))
    wref = dict(ncount=ref["ncount"][inner], rho=ref["rho"][inner],
                acc=np.ascontiguousarray(ref["acc"].reshape(-1, 3)[inner]).reshape(-1))
    what = "fast %s (step %d), %s band" % (cp, c["step"], band)
    scale = lambda: np.maximum(oracle.full_accel_scale(to_oracle_params(p), bpos, bvel, smass, ref["rho"])[inner], 1e-300)
    before_clause = CLAUSE_USED["particles"]
    worst, allowed = check_fast(part, wref, p, smass[inner], what, scale=scale)
    clause = CLAUSE_USED["particles"] - before_clause
    check_fast_velocity(c["vel"].reshape(-1, 3)[ids], svel.reshape(-1, 3)[inner], allowed, p.time_step, what)
    check_fast_position(c["pos"].reshape(-1, 3)[ids], spos.reshape(-1, 3)[inner], p, what)
    print("%s: %d interior of %d particles, max force rel err %.3g, %d particles took the cancellation "
          "clause, oracle %.1f s" % (what, ids.size, sub.size, worst, clause, t1 - t0))


def test_fast_peak_against_exact_whole_scene(dam):
    """the tolerance-mode pre-state at the peak, stepped with the exact arithmetic in a fresh context:
    all 4M particles"""
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_full_fast import FORCE_COND_SHARE, FORCE_RTOL
    c = dam["fast"]["cps"]["peak"]
    with S.SPH(N, c["p"], mode=S.MODE_FULL) as sph:
        sph.setParticles(c["pos0"], c["vel0"], c["mass"])
        sph.step()
        part = sph.getParticles()
        assert np.array_equal(part.mNeighborCount, c["ncount"])
        assert np.array_equal(part.mDensity, c["rho"], equal_nan=True)
        for name, a, b in (("acceleration", c["acc"], part.mAcceleration), ("velocity", c["vel"], part.mVelocity),
                           ("position", c["pos"], part.mPosition)):
            assert not nonfinite_mismatch(a, b).any(), name + ": non-finite patterns differ"
        rel = vec_rel(*finite_parts(c["acc"].reshape(-1, 3), part.mAcceleration.reshape(-1, 3), "peak"))
        beyond = int((rel > FORCE_RTOL).sum())
    print("fast peak (step %d) vs exact from the same state, all %d particles: max force rel err %.3g, %d beyond "
          "1e-4 (%.4f %%)" % (c["step"], N, float(rel.max()), beyond, 100.0 * beyond / N))
    assert beyond <= FORCE_COND_SHARE * N


def brick_totals(policy, grid, origin, spacing, shape):
    """the particles each brick of the lattice stages (sample_kernels.h, k_sample_lattice: the cells of
    its first and last point per axis, one cell around, clamped to the grid), from the brick shape
    sample_policy.h chooses"""
    import sample_emulation as E
    from test_sample_cpu import brick
    p = grid.p
    cells = [float(s) * float(np.float32(p.full_cell_inv)) for s in spacing]
    (bx, by, bz), _ = brick(policy, shape, cells)
    n = grid.n
    totals = []
    for b2 in range(-(-shape[2] // bz)):
        for b1 in range(-(-shape[1] // by)):
            for b0 in range(-(-shape[0] // bx)):
                lo, hi = [], []
                for a, (b, w) in enumerate(((b0, bx), (b1, by), (b2, bz))):
                    first, last = b * w, min(shape[a], (b + 1) * w) - 1
                    x0 = np.float32(origin[a]) + np.float32(first) * np.float32(spacing[a])
                    x1 = np.float32(origin[a]) + np.float32(last) * np.float32(spacing[a])
                    lo.append(max(int(E.cell_coord(np.array([x0]), grid.inv, n[a])[0]) - 1, 0))
                    hi.append(min(int(E.cell_coord(np.array([x1]), grid.inv, n[a])[0]) + 1, n[a] - 1))
                t = 0
                for z in range(lo[2], hi[2] + 1):
                    for y in range(lo[1], hi[1] + 1):
                        row = (z * n[1] + y) * n[0]
                        t += int(grid.start[row + hi[0] + 1] - grid.start[row + lo[0]])
                totals.append(t)
    return np.array(totals)


def test_sampler_on_the_compressed_dam(dam, policy, monkeypatch):
    """the field sampler on the tolerance-mode state after the peak step, uploaded into fresh FULL
    contexts: the lattice's bricks stage more than SAMPLE_TILE_CAP particles in the dense flow and fewer
    near its surface, so the data - not a switch - sends bricks of one lattice down both paths of
    k_sample_lattice; tiled, untiled and default routes give the same bits, 2000 lattice points those of
    the emulation, and samples at particles agree with the density pass"""
    import sample_emulation as E
    import smoothed_particle_hydrodynamics_amd as S
    from test_sample_cpu import DEFAULT, TILED, tiled
    c = dam["fast"]["cps"]["peak"]
    p, mass = c["p"], c["mass"]
    pos, vel = c["pos"].reshape(-1, 3), c["vel"].reshape(-1, 3)
    # from the floor to above the free surface, around the most compressed region, at the coarsest
    # spacing (0.7, 0.7, 0.65 cells) for which the shim still tiles: the bricks' tiles are as large as
    # the tiled route allows (320 cells at worst; at 0.5 cells no brick of this state stages more than
    # 2305 particles)
    edge = np.float32(1.0) / np.float32(p.full_cell_inv)
    spacing = (np.float32(0.7) * edge, np.float32(0.7) * edge, np.float32(0.65) * edge)
    dense = pos[c["ncount"] > 100]
    top = np.float32(1.2) * np.percentile(pos[:, 1], 99.9).astype(np.float32)
    shape = (96, min(128, int(np.ceil(top / spacing[1])) + 1), 96)
    mid = np.median(dense, axis=0).astype(np.float32)
    origin = (max(np.float32(0.0), mid[0] - np.float32(48) * spacing[0]), np.float32(0.0),
              max(np.float32(0.0), mid[2] - np.float32(48) * spacing[2]))
    cells = [float(s) * float(np.float32(p.full_cell_inv)) for s in spacing]
    assert tiled(policy, shape, cells, TILED) == 1 and tiled(policy, shape, cells, DEFAULT) == 0
    grid = E.Grid(p, pos, vel, mass)
    totals = brick_totals(policy, grid, origin, spacing, shape)
    cap = policy.tile_cap()
    over, fit = int((totals > cap).sum()), int(((totals > 0) & (totals <= cap)).sum())
    print("compressed-dam lattice %s, spacing %s cells: %d bricks, %d stage more than %d particles, %d fit "
          "(largest %d)" % (shape, ["%.2f" % x for x in cells], totals.size, over, cap, fit, int(totals.max())))
    assert over > 0 and fit > 0
    out = {}
    for route, env in (("tiled", "SPH_HIP_SAMPLE_TILED"), ("untiled", "SPH_HIP_SAMPLE_UNTILED"), ("default", None)):
        monkeypatch.delenv("SPH_HIP_SAMPLE_TILED", raising=False)
        monkeypatch.delenv("SPH_HIP_SAMPLE_UNTILED", raising=False)
        if env:
            monkeypatch.setenv(env, "1")
        with S.SPH(N, p, mode=S.MODE_FULL) as sph:       # (the switches are read when the context is created)
            sph.setParticles(c["pos"], c["vel"], mass)
            out[route] = sph.sampleLattice(origin, spacing, shape)
    for route in ("untiled", "default"):
        for name, a, b in zip(("density", "velocity", "count"), out["tiled"], out[route]):
            assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), "tiled vs %s: %s" % (route, name)
    a = out["tiled"]
    rng = np.random.default_rng(11)
    pick = rng.choice(a[0].size, 2000, replace=False)
    want = grid.sample(E.lattice_points(origin, spacing, shape).reshape(-1, 3)[pick])
    for name, g, w in zip(("density", "velocity", "count"), (a[0].reshape(-1)[pick], a[1].reshape(-1, 3)[pick],
                                                           a[2].reshape(-1)[pick]), want):
        assert np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes(), "lattice vs emulation: " + name
    # at particles: count = neighbours + 1, density = the density pass + the particle's own term.  The
    # 500 most crowded particles are among them (none outgrows its list at this state: the lists have
    # grown past the largest count, test_peak_route_mix_fired prints both)
    crowded = np.argsort(c["ncount"], kind="stable")[-500:]
    ids = np.unique(np.concatenate([crowded, rng.choice(N, 1500, replace=False)]))
    monkeypatch.delenv("SPH_HIP_SAMPLE_TILED", raising=False)
    monkeypatch.delenv("SPH_HIP_SAMPLE_UNTILED", raising=False)
    with S.SPH(N, p, mode=S.MODE_FULL) as sph:
        sph.setParticles(c["pos"], c["vel"], mass)
        rho, _, cnt = sph.sampleFields(pos[ids], velocity=False)
        sph.step()
        part = sph.syncParticles()
    assert np.array_equal(cnt, part.mNeighborCount[ids] + 1)
    self_term = mass[ids].astype(np.float32) * (np.float32(p.kernel1) * (np.float32(p.hscaled2) * np.float32(p.hscaled2) *
                                                                         np.float32(p.hscaled2)))
    diff = np.abs(rho.astype(np.float64) - self_term - part.mDensity[ids])
    assert (diff <= 1e-6 * (part.mDensity[ids].astype(np.float64) + self_term)).all(), float(diff.max())
    print("samples at %d particles (neighbour counts up to %d): count = neighbours + 1, density within %.2g" % (
        ids.size, int(part.mNeighborCount[ids].max()), float((diff / (part.mDensity[ids] + self_term)).max())))
