"""GPU: the tile fill of the density pass (tile_load, csrc/full_tiled.h) takes a pass's shift from
tile index to sorted index from workgroup-uniform values - the descriptor's words in scalar
registers (csrc/tile_layout.h) - and spends one compare and select per lane only on a boundary that
really lies inside the pass.  The tile's contents must be what the per-lane search of the nine
segments put there (the acceleration pass still runs that search and fills its own tile from the
same descriptor), so every output of every route stays what it was.

What can go wrong is a pass that takes the wrong segment's shift: tiles of nine distinct shifts,
tiles whose three planes merge into three chains, segments clamped at the grid's first and last
cell and empty ones, a segment longer than several passes, tiles of more than one batch of eight
passes, the wide-entry instantiations, a ragged last workgroup, slabs with ghosts.

Every scene's precondition is asserted on the CPU before the GPU runs: the workgroups' descriptors
are recomputed from the oracle's full_cells() through the header itself (tests/tile_layout_shim.py),
and the shape the case is about must occur - and the device must report the same largest tile.

Bar: exact arithmetic bit-identical to the oracle (check_state of tests/test_gpu_full_mode.py);
tolerance mode through check_fast of tests/test_gpu_full_fast.py; the tiled route equal to the
list-driven and untiled routes bit for bit, forced through the environment as
tests/test_gpu_full_mode.py forces them."""
import numpy as np
import pytest

from helpers import to_oracle_params
from test_gpu_full_fast import check_fast
from test_gpu_full_mode import check_state
from tile_layout_shim import Layout, old_search_all, workgroup_descriptors

pytestmark = pytest.mark.gpu

ROUTE_VARS = ("SPH_HIP_UNTILED", "SPH_HIP_TILE_CAP", "SPH_HIP_TILE_CAP_ACCEL", "SPH_HIP_TILE_CAP_DENSITY",
              "SPH_HIP_LIST_CAP", "SPH_HIP_CHUNKED")
FIELDS = ("mPosition", "mVelocity", "mDensity", "mAcceleration", "mNeighborCount")
BATCH = 8 * 256          # tile entries of one batch of the fill (TILE_BATCH loads of 256 lanes)


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    return Layout(tmp_path_factory)


class Tiles:
    """the workgroups' descriptors of a scene and what the cases ask of them"""

    def __init__(self, layout, oracle, p, pos):
        ids, cs, ci = oracle.full_cells(to_oracle_params(p), pos)
        self.desc = workgroup_descriptors(layout, p, ids, cs, ci)
        self.totals = [d[2] for d in self.desc]
        self.shifts = []          # per workgroup: the shift of every tile index
        self.inside = []          # per workgroup: boundaries inside each pass
        for D, B, total, _, _ in self.desc:
            self.shifts.append(old_search_all(D, B, total))
            self.inside.append([len(layout.plan(D, B, total, q)[3]) for q in range((total + 255) // 256)])

    def distinct_shifts(self):
        return [len(set(s.tolist())) for s in self.shifts]

    def passes_with(self, n):
        return sum(sum(1 for k in w if (k == n if n < 2 else k >= 2)) for w in self.inside)

    def longest_new_part(self):
        return max(max(e - b for b, e in zip(B, B[1:] + [total])) for _, B, total, _, _ in self.desc)

    def longest_run_of_one_shift(self):
        best = 0
        for s in self.shifts:
            cuts = np.flatnonzero(np.diff(s) != 0)
            edges = np.concatenate([[-1], cuts, [s.size - 1]])
            best = max(best, int(np.diff(edges).max()))
        return best


def step_on_route(S, scene, mode, env, monkeypatch, stats=None):
    p, pos, vel, mass = scene
    for k in ROUTE_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with S.SPH(mass.size, p, mode=mode) as sph:
        sph.setParticles(pos, vel, mass)
        sph.step()
        part = sph.getParticles()
        if stats is not None:
            stats.update(sph.tileStats())
        return {k: getattr(part, k).copy() for k in FIELDS}


class Part:
    def __init__(self, out):
        for k in FIELDS:
            setattr(self, k, out[k])


def check_scene(S, oracle, layout, scene, monkeypatch, precondition, cap=None):
    """one step from the scene's state: exact arithmetic on the tiled route against the oracle bit for
    bit; tolerance mode on the tiled route against the oracle (check_fast), on the list-driven and
    untiled routes against the tiled one bit for bit.  cap: the tile capacity pinned for the tiled route."""
    p, pos, vel, mass = scene
    tiles = Tiles(layout, oracle, p, pos)
    precondition(tiles)
    ref = oracle.step(to_oracle_params(p), pos.copy(), vel.copy(), mass, mode="full")
    tiled = {} if cap is None else {"SPH_HIP_TILE_CAP": str(cap)}
    routes = {"tiled": tiled,
              "list-driven": {"SPH_HIP_TILE_CAP": "6016", "SPH_HIP_TILE_CAP_ACCEL": "256"},
              "untiled": {"SPH_HIP_UNTILED": "1"}}
    stats = {r: {} for r in routes}
    exact_stats = {}
    exact = step_on_route(S, scene, S.MODE_FULL, tiled, monkeypatch, exact_stats)
    out = {r: step_on_route(S, scene, S.MODE_FULL_FAST, env, monkeypatch, stats[r]) for r, env in routes.items()}
    # the tiled route is the one that ran, on the tiles the precondition looked at
    for st in (exact_stats, stats["tiled"]):
        assert st["untiled_acceleration"] == 0 and st["untiled_density"] == 0, st
        assert st["largest_tile"] == max(tiles.totals) and st["workgroups"] == len(tiles.totals), (st, max(tiles.totals))
    # (the list-driven route: every workgroup whose tile does not fit 256 entries walks its lists)
    listed = sum(1 for x in tiles.totals if x > 256)
    assert listed >= len(tiles.totals) - 1 and stats["list-driven"]["untiled_acceleration"] == listed, stats["list-driven"]
    assert stats["list-driven"]["untiled_density"] == 0, stats["list-driven"]
    check_state(Part(exact), ref, "exact, tiled route")
    worst, _ = check_fast(Part(out["tiled"]), ref, p, mass, "tiled route")
    print("worst force rel err %.3g, tiles %d .. %d" % (worst, min(tiles.totals), max(tiles.totals)))
    for r in ("list-driven", "untiled"):
        for k in FIELDS:
            assert np.array_equal(out["tiled"][k], out[r][k], equal_nan=k != "mNeighborCount"), (r, k)
    return stats["tiled"]


def long_rows(n, neighbors, seed):
    """a channel 44 to 48 cells long and 6 x 6 across, filled: a row holds more particles than a
    workgroup, so the nine row segments of a workgroup in the channel's middle lie apart"""
    from smoothed_particle_hydrodynamics_amd import scenes
    box = (8.0, 0.7, 0.7) if neighbors == 32.0 else (6.0, 0.6, 0.6)
    return scenes.dam_break(n, box=box, fill=(1.0, 1.0, 1.0), neighbors=neighbors, seed=seed, speed=0.05)


def test_a_nine_distinct_shifts_in_one_tile(oracle, hiplib, layout, monkeypatch):
    """rows much longer than a workgroup's span"""
    import smoothed_particle_hydrodynamics_amd as S
    scene = long_rows(6000, 32.0, 3)

    def precondition(t):
        assert max(t.distinct_shifts()) == 9 and t.passes_with(2) >= 10, (t.distinct_shifts(), t.passes_with(2))
        assert max(t.totals) <= 3008
    check_scene(S, oracle, layout, scene, monkeypatch, precondition, cap=3008)


def test_b_three_shifts_passes_with_no_and_with_one_boundary(oracle, hiplib, layout, monkeypatch):
    """a column narrower than the span: the three segments of a plane merge"""
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    scene = scenes.dam_break(12000, seed=42, speed=0.05)

    def precondition(t):
        assert max(t.distinct_shifts()) == 3, t.distinct_shifts()
        assert t.passes_with(0) >= 50 and t.passes_with(1) >= 50 and t.passes_with(2) == 0
    check_scene(S, oracle, layout, scene, monkeypatch, precondition)


def test_c_segments_clamped_and_empty_at_the_grid_s_ends(oracle, hiplib, layout, monkeypatch):
    """fluid against the first and the last cell of the grid"""
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    scene = scenes.dam_break(5000, fill=(1.0, 1.0, 1.0), seed=5, speed=0.05)
    p = scene[0]

    def precondition(t):
        n = scene[3].size
        first, last = t.desc[0], t.desc[-1]
        # the first workgroup's rows below and behind the grid are empty, its own row starts at sorted
        # position 0 (clamped: there is no cell -1); the last workgroup's ends at the last position
        assert first[4][0] == 0 and first[4][4] > 0 and first[3][4] == 0, first
        assert last[4][8] == 0 and last[3][4] + last[4][4] == n, last
        assert sum(1 for d in t.desc for length in d[4] if length == 0) >= 10
        assert p.full_cells_x * p.full_cells_y * p.full_cells_z == 1000
    check_scene(S, oracle, layout, scene, monkeypatch, precondition)


def test_d_a_segment_longer_than_several_passes(oracle, hiplib, layout, monkeypatch):
    """sparse fill, 2 to 3 neighbours per particle: a 256-particle span covers hundreds of cells"""
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    scene = scenes.dam_break(20000, box=(2.0, 0.5, 0.5), fill=(1.0, 1.0, 1.0), neighbors=2.5, seed=42, speed=0.05)

    def precondition(t):
        assert t.longest_new_part() > 2 * 256, t.longest_new_part()
        assert t.longest_run_of_one_shift() >= 3 * 256, t.longest_run_of_one_shift()   # two whole passes inside
        assert t.passes_with(0) >= 100 and t.passes_with(1) >= 100
    check_scene(S, oracle, layout, scene, monkeypatch, precondition)


def test_e_more_than_one_batch(oracle, hiplib, layout, monkeypatch):
    """tiles beyond 2048 entries (a denser channel, the capacity raised to the narrow entries' limit)"""
    import smoothed_particle_hydrodynamics_amd as S
    scene = long_rows(10000, 48.0, 4)

    def precondition(t):
        big = [x for x in t.totals if x > BATCH]
        assert len(big) >= 10 and max(t.totals) <= 4064, (len(big), max(t.totals))
        # ... with changes of shift inside the passes of the second batch
        assert any(sum(w[8:]) > 0 for w in t.inside)
    st = check_scene(S, oracle, layout, scene, monkeypatch, precondition, cap=4064)
    assert st["wide_entries"] == 0 and st["capacity_density"] == 4064, st


def test_f_wide_entries(oracle, hiplib, layout, monkeypatch):
    """the wide-entry instantiations: capacity 6016, tiles beyond 4096 entries (three batches)"""
    import smoothed_particle_hydrodynamics_amd as S
    scene = long_rows(16000, 90.0, 6)

    def precondition(t):
        # (tile indices that need the wide entries' 14 bits, in tiles of three batches)
        assert sum(1 for x in t.totals if x > 4096) >= 3 and max(t.totals) <= 6016, max(t.totals)
        assert any(sum(w[8:]) > 0 for w in t.inside)
    st = check_scene(S, oracle, layout, scene, monkeypatch, precondition, cap=6016)
    assert st["wide_entries"] == 1, st


def test_g_ragged_last_workgroup(oracle, hiplib, layout, monkeypatch):
    """2 999 particles: the last workgroup holds 183, its tile is filled for them alone"""
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    scene = scenes.dam_break(2999, seed=42, speed=0.05)

    def precondition(t):
        assert scene[3].size % 256 == 183 and len(t.totals) == 12
        assert t.totals[-1] % 256 != 0          # ... and its last pass is a partial one
    check_scene(S, oracle, layout, scene, monkeypatch, precondition)


def test_g_two_slabs_with_ghosts_equal_the_single_context(oracle, hiplib, monkeypatch):
    """one column as two logical slabs: the passes run over ranges that begin and end with ghosts,
    descriptors indexed by workgroups of the slab's own range.  Tolerance mode, against the single
    context bit for bit; the single context against the oracle."""
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    from test_gpu_slabs import build_group
    for k in ROUTE_VARS + ("SPH_HIP_NO_FUSED_SLAB",):
        monkeypatch.delenv(k, raising=False)
    p, pos, vel, mass = scenes.dam_break(6001, seed=42, speed=0.05)
    ref = oracle.step(to_oracle_params(p), pos.copy(), vel.copy(), mass, mode="full")
    group, cuts = build_group(S, p, pos, vel, mass, 2, "two-streams")
    try:
        for s in group.slabs:
            s.set_arithmetic(S.ARITH_FAST)
        owned = [s.status()["owned"] for s in group.slabs]
        assert min(owned) > 1000, owned
        group.step()
        got = group.gather(mass.size)
        for s in group.slabs:
            assert s.status()["errors"] == 0
    finally:
        for s in group.slabs:
            s.close()
    with S.SPH(mass.size, p, mode=S.MODE_FULL_FAST) as one:
        one.setParticles(pos, vel, mass)
        one.step()
        part = one.getParticles()
        check_fast(part, ref, p, mass, "single context")
        for k, want in (("ncount", part.mNeighborCount), ("rho", part.mDensity), ("acc", part.mAcceleration),
                        ("pos", part.mPosition), ("vel", part.mVelocity)):
            assert np.array_equal(got[k], want), k
