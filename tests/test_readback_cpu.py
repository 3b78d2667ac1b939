"""CPU: the references that tests/test_gpu_readback.py holds the read-back paths to, pinned to each
other without a GPU and without the product library.

The occupancy a host reads back (sph_hip_download_async's voxel counts, SPH.getGrid()) has two
independent restatements: the oracle's cell builds (oracle_voxelize, oracle_full_cells) and numpy's
bincount of (cz * ny + cy) * nx + cx (helpers.grid_occupancy).  They must agree on the shared scene
(helpers.readback_scene): a non-cubic grid, most particles clamped, particles on voxel faces, non-finite
coordinates.  oracle.neighbor_stats is checked at the values the GPU tests rely on."""
import numpy as np
import pytest

from helpers import READBACK_COUNTS, READBACK_NONFINITE_ROWS, grid_occupancy, readback_scene


def ref_grid(p):
    return (p.cells_x, p.cells_y, p.cells_z)


def full_grid(p):
    return (p.full_cells_x, p.full_cells_y, p.full_cells_z)


@pytest.mark.parametrize("n", READBACK_COUNTS)
def test_both_grids_numpy_restatement_equals_the_oracle(oracle, n):
    p, pos, _, _ = readback_scene(n, oracle.params_for_h)
    assert pos.size == 3 * n
    assert len({*ref_grid(p)}) == 3 and len({*full_grid(p)}) == 3     # no two extents alike
    coords, ids, cs, _ = oracle.voxelize(p, pos)
    my_ids, my_counts = grid_occupancy(pos, p.htimes2inv, ref_grid(p))
    assert np.array_equal(ids, my_ids)
    c = coords.reshape(-1, 3).astype(np.int64)
    assert np.array_equal((c[:, 2] * p.cells_y + c[:, 1]) * p.cells_x + c[:, 0], my_ids)
    assert np.array_equal(np.diff(cs), my_counts) and my_counts.sum() == n
    ids, cs, _ = oracle.full_cells(p, pos)
    my_ids, my_counts = grid_occupancy(pos, p.full_cell_inv, full_grid(p))
    assert np.array_equal(ids, my_ids)
    assert np.array_equal(np.diff(cs), my_counts) and my_counts.sum() == n


def test_the_scene_reaches_every_edge(oracle):
    """some particle clamped on each of the six faces, crowded and empty voxels, particles exactly on voxel
    faces, and the non-finite rows in the cells the oracle gives them: coordinate 0 on every axis that is
    not finite ((int)floor() of +-inf and NaN is INT_MIN, clamped)"""
    p, pos, _, _ = readback_scene(6000, oracle.params_for_h)
    xyz = pos.reshape(-1, 3)
    fin = np.isfinite(xyz).all(axis=1)
    assert (~fin).sum() == len(READBACK_NONFINITE_ROWS) and not fin[list(READBACK_NONFINITE_ROWS)].any()
    outside = np.zeros(fin.sum(), bool)
    for grid, inv in ((ref_grid(p), p.htimes2inv), (full_grid(p), p.full_cell_inv)):
        for a in range(3):
            raw = np.floor(xyz[fin, a] * np.float32(inv))
            assert (raw < 0).any() and (raw >= grid[a]).any(), "no particle clamped on a face of axis %d" % a
            outside |= (raw < 0) | (raw >= grid[a])
    assert 0.7 < outside.mean() < 0.8
    on_face = xyz[100:400] * np.float32(p.htimes2inv)     # what cell_coord takes the floor of
    assert np.allclose(on_face, np.round(on_face), rtol=2.0 ** -22, atol=0.0)
    assert (on_face == np.round(on_face)).mean() > 0.5
    coords, ids, cs, _ = oracle.voxelize(p, pos)
    counts = np.diff(cs)
    assert counts.max() > 1 and counts.min() == 0
    coords = coords.reshape(-1, 3)
    my_ids, _ = grid_occupancy(pos, p.htimes2inv, ref_grid(p))
    full_ids, _ = grid_occupancy(pos, p.full_cell_inv, full_grid(p))
    for row in READBACK_NONFINITE_ROWS:
        bad = ~np.isfinite(xyz[row])
        assert (coords[row][bad] == 0).all()
        assert my_ids[row] == ids[row]
        assert full_ids[row] == oracle.full_cells(p, pos)[0][row]
    assert (coords[50] == 0).all() and ids[50] == 0


def test_oracle_neighbor_stats(oracle):
    """(sum / n in integer division, max, min started at 34: reference src/sph.cpp:204-232)"""
    assert oracle.neighbor_stats(np.array([35, 99, 60], np.int32)) == (64, 99, 34)
    assert oracle.neighbor_stats(np.array([0], np.int32)) == (0, 0, 0)
    assert oracle.neighbor_stats(np.array([3, 4], np.int32)) == (3, 4, 3)
    big = np.full(70000, 40000, np.int32)
    assert int(big.astype(np.int64).sum()) > 2 ** 31
    assert oracle.neighbor_stats(big) == (40000, 40000, 34)
    big[0] = 39999
    assert oracle.neighbor_stats(big) == (39999, 40000, 34)      # 2 799 999 999 // 70 000
