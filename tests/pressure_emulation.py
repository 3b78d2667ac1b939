"""numpy restatement of the pressure readings (csrc/gauge_policy.h; include/sph_hip.h: pressure readings) on top
of the field sampler's restatement (sample_emulation.Grid) and the gauges' (gauge_emulation), the checker of
tests/test_gpu_pressure.py and tests/test_pressure_cpu.py.

    rho_j    the FULL density pass's density of particle j: over the particles within h of it, itself excluded,
             in canonical order, the sampler's term (density_untiled adds nothing where the term would be 0: the
             same bits, a density is never negative and never -0)
    P_j      (rho_j - rho0) * stiffness, not clamped
    pwalk    the sampler's members and terms t_j at a probe (a particle there included): rho = sum t_j,
             pw = sum t_j * P_j, count - in canonical order
    pressure rho > 0 ? pw / rho : 0
    PRESSURE        v = {pressure, rho, pw, 0}, n = count, k = 0
    PRESSURE_PATCH  SECTION's probes; lane l of 64 adds, for its WET probes l, l + 64, ... in order, the probe's
             pressure to a and its rho to r, both from 0.0f; the lanes are summed by the butterfly;
             v = {a_sum * area, (float)n * area, n > 0 ? a_sum / (float)n : 0, r_sum}, n = wet probes, k = 0
numpy evaluates float32 arrays operation by operation with IEEE rounding and never fuses, so the bits are the
device's."""
import collections

import numpy as np

import gauge_emulation as G
import sample_emulation as SE

F32 = np.float32
PRESSURE, PRESSURE_PATCH = 4, 5
WAVE = G.WAVE

# which classes one evaluation held, as counts of gauges: patches fully wet, partly wet and dry; points with a
# positive and with a negative pressure; readings with count == 0
Info = collections.namedtuple("Info", ["full", "partial", "dry", "positive", "negative", "empty"])


def point(p):
    return G.Gauge(PRESSURE, 0, np.asarray(p, F32).reshape(3), np.zeros(2, F32), (0, 0), F32(0.0))


def patch(corner, axis, spacing, shape, iso):
    return G.Gauge(PRESSURE_PATCH, int(axis), np.asarray(corner, F32).reshape(3), np.asarray(spacing, F32).reshape(2),
                   (int(shape[0]), int(shape[1])), F32(iso))


def is_pressure(g):
    return g.kind in (PRESSURE, PRESSURE_PATCH)


def probes_of(g):
    """The gauge's probes in index order: a patch has SECTION's rectangle, a point its origin."""
    if g.kind == PRESSURE_PATCH:
        return G.probes_of(g._replace(kind=G.SECTION))
    if g.kind == PRESSURE:
        return G.probes_of(g._replace(kind=G.POINT))
    return G.probes_of(g)


def canonical_order(p, pos):
    """The permutation sample_emulation.Grid sorts the particles by: ascending FULL cell id, then index."""
    pos = np.asarray(pos, F32).reshape(-1, 3)
    n = (p.full_cells_x, p.full_cells_y, p.full_cells_z)
    c = [SE.cell_coord(pos[:, a], F32(p.full_cell_inv), n[a]) for a in range(3)]
    cell = (c[2] * n[1] + c[1]) * n[0] + c[0]
    return np.lexsort((np.arange(cell.size), cell))


def ordered_sums(probe, m, columns):
    """Per probe row (0 .. m - 1) the fp32 sums of each array of `columns`, its entries added one by one in the
    order they stand (entries are grouped by probe): a list of float32 (m,) arrays, and the counts."""
    count = np.bincount(probe, minlength=m).astype(np.int32)
    first = np.zeros(m + 1, np.int64)
    first[1:] = np.cumsum(count)
    col = np.arange(probe.size) - first[probe]
    by_col = np.argsort(col, kind="stable")
    ends = np.cumsum(np.bincount(col, minlength=1)) if probe.size else np.zeros(1, np.int64)
    sums = [np.zeros(m, F32) for _ in columns]
    at = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for e in ends:
            sel = by_col[at:e]
            at = e
            rows = probe[sel]
            for s, c in zip(sums, columns):
                s[rows] = s[rows] + c[sel]
    return sums, count


def members(grid, probes, exclude_self=False):
    """(probe row, sorted particle index, d2) of every member of every probe, in canonical order per probe; with
    exclude_self probe row i is sorted particle i and is not its own member."""
    probe, idx = grid.candidates(probes)
    if exclude_self:
        keep = probe != idx
        probe, idx = probe[keep], idx[keep]
    with np.errstate(invalid="ignore", over="ignore"):
        d = probes[probe] - grid.pos[idx]
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        member = d2 < F32(grid.p.h2)
    return probe[member], idx[member], d2[member]


def particle_density_sorted(grid):
    """rho_j of every particle of the grid's state, in the grid's (canonical) order."""
    n = grid.mass.size
    if n == 0:
        return np.zeros(0, F32)
    probe, idx, d2 = members(grid, grid.pos, exclude_self=True)
    t = SE.density_terms(grid.p, d2, grid.mass[idx])
    return ordered_sums(probe, n, [t])[0][0]


def particle_density(p, pos, vel, mass):
    """rho_j of every particle, in the order the particles were given."""
    grid = SE.Grid(p, pos, vel, mass)
    out = np.zeros(grid.mass.size, F32)
    out[canonical_order(p, pos)] = particle_density_sorted(grid)
    return out


def particle_pressure(p, rho):
    with np.errstate(invalid="ignore", over="ignore"):
        return ((np.asarray(rho, F32) - F32(p.rho0)) * F32(p.stiffness)).astype(F32)


def pwalk(grid, prho_sorted, probes):
    """The raw sums of the probes over the state of `grid` (None: nothing resident) with the particle densities
    prho_sorted (canonical order): rho (m,), pw (m,), count (m,)."""
    probes = np.asarray(probes, F32).reshape(-1, 3)
    m = probes.shape[0]
    if grid is None or grid.mass.size == 0 or m == 0:
        return np.zeros(m, F32), np.zeros(m, F32), np.zeros(m, np.int32)
    probe, idx, d2 = members(grid, probes)
    t = SE.density_terms(grid.p, d2, grid.mass[idx])
    with np.errstate(invalid="ignore", over="ignore"):
        tp = (t * particle_pressure(grid.p, prho_sorted[idx])).astype(F32)
    (rho, pw), count = ordered_sums(probe, m, [t, tp])
    return rho, pw, count


def quotient(pw, rho):
    """pressure = rho > 0 ? pw / rho : 0, elementwise."""
    pw, rho = np.asarray(pw, F32), np.asarray(rho, F32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return np.where(rho > 0, pw / np.where(rho > 0, rho, F32(1.0)), F32(0.0)).astype(F32)


def point_reading(rho, pw, count):
    """(v[4], n, k) of a pressure point from its probe's raw sums."""
    return np.array([quotient(pw, rho), rho, pw, 0.0], F32), int(count), 0


def masked_lane_sums(values, take):
    """The 64 lanes' accumulators: lane l adds values[q] for q = l, l + 64, ... in order where take[q], from 0.0f;
    a probe not taken, or missing, adds nothing."""
    values, take = np.asarray(values, F32), np.asarray(take, bool)
    m = values.size
    trips = (m + WAVE - 1) // WAVE
    pad = np.zeros(trips * WAVE, F32)
    pad[:m] = values
    has = np.zeros(trips * WAVE, bool)
    has[:m] = take
    pad, has = pad.reshape(trips, WAVE), has.reshape(trips, WAVE)
    acc = np.zeros(WAVE, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(trips):
            acc = np.where(has[t], acc + pad[t], acc).astype(F32)
    return acc


def patch_reading(g, rho, pw):
    """(v[4], n, k) of a patch from its probes' raw sums."""
    rho, pw = np.asarray(rho, F32), np.asarray(pw, F32)
    with np.errstate(invalid="ignore"):
        wet = rho > g.iso
    n = int(wet.sum())
    a = G.butterfly(masked_lane_sums(quotient(pw, rho), wet))
    r = G.butterfly(masked_lane_sums(rho, wet))
    area = F32(g.spacing[0] * g.spacing[1])
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mean = F32(a / F32(n)) if n > 0 else F32(0.0)
        return np.array([a * area, F32(n) * area, mean, r], F32), n, 0


def sample(p, pos, vel, mass, probes, density=None):
    """sph_hip_sample_pressure_points: (pressure, rho, count) of the probes.  density: the particles' rho_j in the
    order given (default: the restatement's own)."""
    probes = np.asarray(probes, F32).reshape(-1, 3)
    if np.asarray(mass).size == 0:
        m = probes.shape[0]
        return np.zeros(m, F32), np.zeros(m, F32), np.zeros(m, np.int32)
    grid = SE.Grid(p, pos, vel, mass)
    prho = particle_density_sorted(grid) if density is None else np.asarray(density, F32)[canonical_order(p, pos)]
    rho, pw, count = pwalk(grid, prho, probes)
    return quotient(pw, rho), rho, count


def evaluate(p, pos, vel, mass, gauges, density=None, with_info=False):
    """Every gauge of `gauges` (Gauge tuples of any kind) in the state (pos, vel, mass) under the parameters p: the
    field kinds by gauge_emulation, the pressure kinds here.  density: the particles' rho_j in the order given
    (default: the restatement's own).  Returns Readings, and with_info the classes as an Info of counts."""
    gauges = list(gauges)
    field = [i for i, g in enumerate(gauges) if not is_pressure(g)]
    pres = [i for i, g in enumerate(gauges) if is_pressure(g)]
    v = np.zeros((len(gauges), 4), F32)
    n = np.zeros(len(gauges), np.int32)
    k = np.zeros(len(gauges), np.int32)
    if field:
        out = G.evaluate(p, pos, vel, mass, [gauges[i] for i in field])
        v[field], n[field], k[field] = out.v, out.n, out.k
    info = dict.fromkeys(Info._fields, 0)
    if pres:
        have = np.asarray(mass).size > 0
        grid = SE.Grid(p, pos, vel, mass) if have else None
        prho = None
        if have:
            prho = particle_density_sorted(grid) if density is None else \
                np.asarray(density, F32)[canonical_order(p, pos)]
        pts = [probes_of(gauges[i]) for i in pres]
        rho, pw, count = pwalk(grid, prho, np.concatenate(pts))
        at = 0
        for i, q in zip(pres, pts):
            g, m = gauges[i], len(q)
            r, w, c = rho[at:at + m], pw[at:at + m], count[at:at + m]
            at += m
            if g.kind == PRESSURE:
                v[i], n[i], k[i] = point_reading(r[0], w[0], c[0])
                info["positive"] += int(v[i][0] > 0)
                info["negative"] += int(v[i][0] < 0)
                info["empty"] += int(c[0] == 0)
            else:
                v[i], n[i], k[i] = patch_reading(g, r, w)
                info["full"] += int(n[i] == m)
                info["partial"] += int(0 < n[i] < m)
                info["dry"] += int(n[i] == 0)
    out = G.Readings(v, n, k)
    return (out, Info(**info)) if with_info else out
