"""numpy restatement of the gauges (csrc/gauge_policy.h; include/sph_hip.h: sph_hip_set_gauges) on top of the
field sampler's restatement (sample_emulation.Grid), the checker of tests/test_gpu_gauges.py and
tests/test_gauges_cpu.py.

walk(S, p): the sampler's raw sums at p - rho, (vx, vy, vz) = sum of t_j * v_j, count - in canonical order.
    POINT    v = {rho, vx / rho, vy / rho, vz / rho} (0 where rho <= 0), n = count, k = 0
    COLUMN   probe k = the base with coordinate `axis` replaced by origin[axis] + (float)k * spacing[0]; wet
             when rho > iso; n = wet probes, k = the largest wet index or -1, v[1] = (float)n * spacing[0];
             k == -1: v = {origin[axis], ., 0, rho_0}; k == m - 1: v = {p_k, ., rho_k, 0}; otherwise
             t = fmin(fmax((iso - rho_k) / (rho_(k+1) - rho_k), 0), 1), v = {p_k + t * (p_(k+1) - p_k), ., rho_k, rho_(k+1)}
    SECTION  probe q = j * nu + i; lane l of 64 adds its probes l, l + 64, ... in order to a (the raw velocity
             sum of the normal axis) and r (rho), both from 0.0f; the lanes are summed by the butterfly
             x = x + x[lane ^ d], d = 1 .. 32; v = {a_sum * area, (float)n * area, r_sum, 0}, area = spacing[0] * spacing[1]
numpy evaluates float32 arrays operation by operation with IEEE rounding and never fuses, so the bits are the
device's."""
import collections

import numpy as np

import sample_emulation as SE

F32 = np.float32
POINT, COLUMN, SECTION = 0, 1, 2
WAVE = 64

# sph_hip_gauge's fields: origin (3,), spacing (2,), count (2,)
Gauge = collections.namedtuple("Gauge", ["kind", "axis", "origin", "spacing", "count", "iso"])
# one evaluation of a gauge list: v float32 (n, 4), n and k int32 (n,)
Readings = collections.namedtuple("Readings", ["v", "n", "k"])
# which classes one evaluation held, as counts of gauges: columns with an interior top (0 <= k < m - 1),
# saturated (k == m - 1), dry (k == -1), with a dry probe below the top (n < k + 1), with a clamped t;
# sections with flow of both signs among their probes, and partly wet (0 < n < probes)
Info = collections.namedtuple("Info", ["interior", "saturated", "dry", "gap", "clamped", "both_signs", "partial"])


def point(p):
    return Gauge(POINT, 0, np.asarray(p, F32).reshape(3), np.zeros(2, F32), (0, 0), F32(0.0))


def column(base, axis, spacing, samples, iso):
    return Gauge(COLUMN, int(axis), np.asarray(base, F32).reshape(3), np.array([spacing, 0.0], F32), (int(samples), 0),
                 F32(iso))


def section(corner, axis, spacing, shape, iso):
    return Gauge(SECTION, int(axis), np.asarray(corner, F32).reshape(3), np.asarray(spacing, F32).reshape(2),
                 (int(shape[0]), int(shape[1])), F32(iso))


def of(g):
    """A package gauge (gauges.PointGauge / ColumnGauge / SectionGauge, or their C struct) as a Gauge."""
    s = g.to_struct() if hasattr(g, "to_struct") else g
    return Gauge(int(s.kind), int(s.axis), np.array(list(s.origin), F32), np.array(list(s.spacing), F32),
                 (int(s.count[0]), int(s.count[1])), F32(s.iso))


def probe_count(g):
    return g.count[0] if g.kind == COLUMN else g.count[0] * g.count[1] if g.kind == SECTION else 1


def column_coord(g, k):
    return (g.origin[g.axis] + np.asarray(k, np.int64).astype(F32) * g.spacing[0]).astype(F32)


def probes_of(g):
    """The gauge's probes in index order: float32 (probes, 3)."""
    m = probe_count(g)
    pts = np.tile(g.origin.astype(F32), (m, 1))
    q = np.arange(m, dtype=np.int64)
    if g.kind == COLUMN:
        pts[:, g.axis] = column_coord(g, q)
    elif g.kind == SECTION:
        u, v = [a for a in range(3) if a != g.axis]
        i, j = q % g.count[0], q // g.count[0]
        pts[:, u] = g.origin[u] + i.astype(F32) * g.spacing[0]
        pts[:, v] = g.origin[v] + j.astype(F32) * g.spacing[1]
    return pts


def walk(grid, probes):
    """The raw sums of the probes over the state of `grid` (None: nothing resident): rho (m,), vsum (m, 3),
    count (m,)."""
    probes = np.asarray(probes, F32).reshape(-1, 3)
    m = probes.shape[0]
    rho, vsum, count = np.zeros(m, F32), np.zeros((m, 3), F32), np.zeros(m, np.int32)
    if grid is None or grid.mass.size == 0 or m == 0:
        return rho, vsum, count
    probe, idx = grid.candidates(probes)
    with np.errstate(invalid="ignore", over="ignore"):
        d = probes[probe] - grid.pos[idx]
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        member = d2 < F32(grid.p.h2)
    probe, idx, d2 = probe[member], idx[member], d2[member]
    t = SE.density_terms(grid.p, d2, grid.mass[idx])
    count = np.bincount(probe, minlength=m).astype(np.int32)
    first = np.zeros(m + 1, np.int64)
    first[1:] = np.cumsum(count)
    col = np.arange(probe.size) - first[probe]
    v = grid.vel[idx]
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(int(count.max())):
            sel = col == j
            rows = probe[sel]
            rho[rows] = rho[rows] + t[sel]
            vsum[rows] = vsum[rows] + t[sel][:, None] * v[sel]
    return rho, vsum, count


def butterfly(x):
    """x = x + x[lane ^ d] for d = 1, 2, 4, 8, 16, 32 over 64 lane values: every lane ends with the same sum."""
    x = np.asarray(x, F32).copy()
    lane = np.arange(WAVE)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in (1, 2, 4, 8, 16, 32):
            x = (x + x[lane ^ d]).astype(F32)
    assert (x.view(np.uint32) == x.view(np.uint32)[0]).all() or np.isnan(x).all()
    return x[0]


def lane_sums(values):
    """The 64 lanes' accumulators over `values` by probe index: lane l adds values[l], values[l + 64], ... in
    order, from 0.0f; a lane without a probe in a trip adds nothing."""
    values = np.asarray(values, F32)
    m = values.size
    trips = (m + WAVE - 1) // WAVE
    pad = np.zeros(trips * WAVE, F32)
    pad[:m] = values
    has = (np.arange(trips * WAVE) < m).reshape(trips, WAVE)
    pad = pad.reshape(trips, WAVE)
    acc = np.zeros(WAVE, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(trips):
            acc = np.where(has[t], acc + pad[t], acc).astype(F32)
    return acc


def point_reading(rho, vsum, count):
    """(v[4], n, k) of a point gauge from its probe's raw sums."""
    rho = F32(rho)
    vsum = np.asarray(vsum, F32).reshape(3)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        u = (vsum / rho).astype(F32) if rho > 0 else np.zeros(3, F32)
    return np.array([rho, u[0], u[1], u[2]], F32), int(count), 0


def interpolate(g, k, fa, fb):
    """(level, t before the clamp) of an interior top."""
    fa, fb = F32(fa), F32(fb)
    pk, pk1 = column_coord(g, k), column_coord(g, k + 1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        raw = F32(F32(g.iso - fa) / F32(fb - fa))
        t = F32(np.fmin(np.fmax(raw, F32(0.0)), F32(1.0)))
        return F32(pk + F32(t * F32(pk1 - pk))), raw


def column_tail(g, n, k, f0, f1):
    """The reading of a column from its wet count, its top and the two densities walked again."""
    m = g.count[0]
    depth = F32(F32(n) * g.spacing[0])
    if k < 0:
        return np.array([g.origin[g.axis], depth, 0.0, f0], F32), int(n), int(k)
    if k == m - 1:
        return np.array([column_coord(g, k), depth, f0, 0.0], F32), int(n), int(k)
    level, _ = interpolate(g, k, f0, f1)
    return np.array([level, depth, f0, f1], F32), int(n), int(k)


def column_reading(g, rho):
    """(v[4], n, k) of a column from its probes' densities."""
    rho = np.asarray(rho, F32)
    m = g.count[0]
    with np.errstate(invalid="ignore"):
        wet = rho > g.iso
    n = int(wet.sum())
    k = int(np.flatnonzero(wet)[-1]) if n else -1
    b = max(k, 0)
    return column_tail(g, n, k, rho[b], rho[b + 1] if b + 1 < m else F32(0.0))


def section_reading(g, rho, normal_sum):
    """(v[4], n, k) of a section from its probes' densities and raw velocity sums along the normal."""
    rho = np.asarray(rho, F32)
    with np.errstate(invalid="ignore"):
        n = int((rho > g.iso).sum())
    a = butterfly(lane_sums(normal_sum))
    r = butterfly(lane_sums(rho))
    area = F32(g.spacing[0] * g.spacing[1])
    with np.errstate(invalid="ignore", over="ignore"):
        return np.array([a * area, F32(n) * area, r, 0.0], F32), n, 0


def evaluate(p, pos, vel, mass, gauges, with_info=False):
    """Every gauge of `gauges` (Gauge tuples) in the state (pos, vel, mass) under the parameters p: Readings, and
    the classes it held as an Info of counts."""
    gauges = list(gauges)
    grid = SE.Grid(p, pos, vel, mass) if np.asarray(mass).size else None
    pts = [probes_of(g) for g in gauges]
    rho, vsum, count = walk(grid, np.concatenate(pts) if pts else np.zeros((0, 3), F32))
    v = np.zeros((len(gauges), 4), F32)
    n = np.zeros(len(gauges), np.int32)
    k = np.zeros(len(gauges), np.int32)
    info = dict.fromkeys(Info._fields, 0)
    at = 0
    for i, g in enumerate(gauges):
        m = len(pts[i])
        r, s, c = rho[at:at + m], vsum[at:at + m], count[at:at + m]
        at += m
        if g.kind == POINT:
            v[i], n[i], k[i] = point_reading(r[0], s[0], c[0])
        elif g.kind == COLUMN:
            v[i], n[i], k[i] = column_reading(g, r)
            if k[i] < 0:
                info["dry"] += 1
            elif k[i] == m - 1:
                info["saturated"] += 1
            else:
                info["interior"] += 1
                raw = interpolate(g, int(k[i]), r[k[i]], r[k[i] + 1])[1]
                info["clamped"] += int(not (F32(0.0) <= raw <= F32(1.0)))
            info["gap"] += int(n[i] < k[i] + 1)
        else:
            v[i], n[i], k[i] = section_reading(g, r, s[:, g.axis])
            info["both_signs"] += int((s[:, g.axis] > 0).any() and (s[:, g.axis] < 0).any())
            info["partial"] += int(0 < n[i] < m)
    out = Readings(v, n, k)
    return (out, Info(**info)) if with_info else out


def same_readings(a, b):
    return np.array_equal(np.asarray(a.v, F32).view(np.uint32), np.asarray(b.v, F32).view(np.uint32)) and \
        np.array_equal(a.n, b.n) and np.array_equal(a.k, b.k)
