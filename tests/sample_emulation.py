"""numpy restatement of the field sampler (include/sph_hip.h: sph_hip_sample_points), the checker of
tests/test_gpu_sample.py and tests/test_sample_cpu.py.

Every probe's members are the particles with fp32 d2 = (dx*dx + dy*dy) + dz*dz < h2, visited in
canonical order - ascending FULL cell id (floor(x * inv) clamped per axis, the cell build's formula),
then ascending particle index - and summed one by one in fp32.  numpy evaluates float32 arrays
operation by operation with IEEE rounding and never fuses, so the bits are the device's.
"""
import numpy as np

F32 = np.float32


def cell_coord(x, inv, ncell):
    """csrc/sph_device.h cell_coord: (int)floor(x * inv) as cvttsd2si does it (out of range and NaN
    give INT_MIN), clamped to [0, ncell)."""
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(np.asarray(x, F32) * F32(inv))
        ok = (f >= F32(-2147483648.0)) & (f < F32(2147483648.0))
    c = np.where(ok, f, -2147483648.0).astype(np.int64)
    return np.clip(c, 0, ncell - 1)


def unit_scale(p):
    """csrc/launch.h unit_scale: the density pass's choice of arithmetic."""
    return F32(p.sim_scale) == F32(1.0) and F32(p.sim_scale_inv) == F32(1.0) and \
        np.sqrt(F32(p.h2)) <= F32(p.hscaled)


def density_terms(p, d2, mass):
    """t_j for members with squared distance d2 (fp32 arrays)."""
    unit = unit_scale(p)
    d = np.sqrt(d2.astype(F32))
    if not unit:
        d = d * F32(p.sim_scale)
    t = F32(p.hscaled2) - d * d
    t = t * t * t
    w = F32(p.kernel1) * t
    term = mass.astype(F32) * w
    if not unit:
        term = np.where(d > F32(p.hscaled), F32(0.0), term).astype(F32)
    return term


class Grid:
    """The particles in canonical order and the FULL grid's cell ranges."""

    def __init__(self, p, pos, vel, mass):
        self.p = p
        self.n = (p.full_cells_x, p.full_cells_y, p.full_cells_z)
        self.inv = F32(p.full_cell_inv)
        pos = np.asarray(pos, F32).reshape(-1, 3)
        c = [cell_coord(pos[:, a], self.inv, self.n[a]) for a in range(3)]
        cell = (c[2] * self.n[1] + c[1]) * self.n[0] + c[0]
        order = np.lexsort((np.arange(cell.size), cell))
        self.pos = pos[order]
        self.vel = np.asarray(vel, F32).reshape(-1, 3)[order]
        self.mass = np.asarray(mass, F32).reshape(-1)[order]
        ncells = self.n[0] * self.n[1] * self.n[2]
        self.start = np.zeros(ncells + 1, np.int64)
        self.start[1:] = np.cumsum(np.bincount(cell, minlength=ncells))

    def candidates(self, probes):
        """(probe row, sorted particle index) of every candidate in canonical order per probe."""
        nx, ny, nz = self.n
        cx, cy, cz = [cell_coord(probes[:, a], self.inv, self.n[a]) for a in range(3)]
        x0, x1 = np.maximum(cx - 1, 0), np.minimum(cx + 1, nx - 1)
        starts, ends = [], []
        for k in range(9):
            z, y = cz + k // 3 - 1, cy + k % 3 - 1
            ok = (z >= 0) & (z < nz) & (y >= 0) & (y < ny)
            row = (np.clip(z, 0, nz - 1) * ny + np.clip(y, 0, ny - 1)) * nx
            starts.append(np.where(ok, self.start[row + x0], 0))
            ends.append(np.where(ok, self.start[row + x1 + 1], 0))
        s = np.stack(starts, 1).reshape(-1)
        ln = (np.stack(ends, 1).reshape(-1) - s)
        probe = np.repeat(np.repeat(np.arange(probes.shape[0]), 9), ln)
        first = np.repeat(np.cumsum(ln) - ln, ln)
        idx = np.repeat(s, ln) + (np.arange(ln.sum()) - first)
        return probe, idx

    def sample(self, probes, velocity=True):
        """(density, velocity or None, count) of the probes, bit for bit."""
        probes = np.asarray(probes, F32).reshape(-1, 3)
        m = probes.shape[0]
        probe, idx = self.candidates(probes)
        with np.errstate(invalid="ignore", over="ignore"):
            d = probes[probe] - self.pos[idx]
            d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
            member = d2 < F32(self.p.h2)
        probe, idx, d2 = probe[member], idx[member], d2[member]
        t = density_terms(self.p, d2, self.mass[idx])
        count = np.bincount(probe, minlength=m).astype(np.int32)
        # members are grouped by probe, in order: column j holds every probe's j-th member
        first = np.zeros(m + 1, np.int64)
        first[1:] = np.cumsum(count)
        col = np.arange(probe.size) - first[probe]
        rho = np.zeros(m, F32)
        vnum = np.zeros((m, 3), F32)
        v = self.vel[idx]
        for j in range(int(count.max()) if m else 0):
            sel = col == j
            rows = probe[sel]
            rho[rows] = rho[rows] + t[sel]
            if velocity:
                vnum[rows] = vnum[rows] + t[sel][:, None] * v[sel]
        if not velocity:
            return rho, None, count
        with np.errstate(invalid="ignore", divide="ignore"):
            vel = np.where((rho > 0)[:, None], vnum / rho[:, None], F32(0.0)).astype(F32)
        return rho, vel, count


def lattice_points(origin, spacing, shape):
    """The lattice origin + (float)i * spacing, fp32 unfused, as (nz, ny, nx, 3)."""
    ax = [F32(origin[a]) + np.arange(shape[a], dtype=np.int64).astype(F32) * F32(spacing[a]) for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x, y, z], -1).astype(F32)


def brute_force64(p, pos, vel, mass, probes):
    """float64 SPH interpolation over ALL particles (no cells): (density, velocity)."""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    vel = np.asarray(vel, np.float64).reshape(-1, 3)
    mass = np.asarray(mass, np.float64).reshape(-1)
    probes = np.asarray(probes, np.float64).reshape(-1, 3)
    rho = np.zeros(len(probes))
    vnum = np.zeros((len(probes), 3))
    for a in range(0, len(probes), 64):
        d = probes[a:a + 64, None, :] - pos[None, :, :]
        d2 = (d * d).sum(-1)
        dd = np.sqrt(d2) * float(p.sim_scale)
        t = np.where((d2 < float(p.h2)) & (dd <= float(p.hscaled)),
                     mass[None, :] * float(p.kernel1) * (float(p.hscaled2) - dd * dd) ** 3, 0.0)
        rho[a:a + 64] = t.sum(1)
        vnum[a:a + 64] = t @ vel
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.where((rho > 0)[:, None], vnum / rho[:, None], 0.0)
    return rho, v
