"""numpy restatement of the carried scalars (csrc/scalar_policy.h; include/sph_hip.h: carried scalars) on top of
the field sampler's restatement (sample_emulation.Grid) and the pressure readings' (pressure_emulation: members
in canonical order, sums added one by one), the checker of tests/test_gpu_scalars.py and tests/test_scalars_cpu.py.

    V_j      rho_j > 0 ? m_j / rho_j : 0, rho_j the density pass's value of the state
    pairs    j with (dx*dx + dy*dy) + dz*dz < h2, (dx, dy, dz) = r_i - r_j, i excluded, in canonical order
    d        sqrt(d2), times sim_scale unless unit scale
    w_j      V_j * (kernel3 * (hscaled - d))
    s_c      0, then for every j with V_j != 0 in order: s_c = s_c + (T_j,c - T_i,c) * w_j
    T_i,c'   kappa[c] > 0 ? T_i,c + (dt * kappa[c]) * s_c : T_i,c (the bits kept)
    sources  in list order, where lo < r_i < hi strictly on every axis: HOLD T_channel = value,
             ADD T_channel = T_channel + value * dt
numpy evaluates float32 arrays operation by operation with IEEE rounding and never fuses, so the bits are the
device's."""
import collections

import numpy as np

import pressure_emulation as PE
import sample_emulation as SE

F32 = np.float32
CHANNELS = 4
HOLD, ADD = 0, 1

# {lo[3], hi[3], channel, kind, value}
Source = collections.namedtuple("Source", ["lo", "hi", "channel", "kind", "value"])

# the constants of the pair arithmetic: fp32 hscaled, kernel3, sim_scale, h2 and whether the context runs at unit
# scale (sample_emulation.unit_scale)
Consts = collections.namedtuple("Consts", ["hscaled", "kernel3", "sim_scale", "h2", "unit"])


def consts_of(p):
    return Consts(F32(p.hscaled), F32(p.kernel3), F32(p.sim_scale), F32(p.h2), bool(SE.unit_scale(p)))


def hold(lo, hi, channel, value):
    return Source(np.asarray(lo, F32).reshape(3), np.asarray(hi, F32).reshape(3), int(channel), HOLD, F32(value))


def add(lo, hi, channel, value):
    return Source(np.asarray(lo, F32).reshape(3), np.asarray(hi, F32).reshape(3), int(channel), ADD, F32(value))


def volume(mass, rho):
    mass, rho = np.asarray(mass, F32), np.asarray(rho, F32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        pos = rho > 0
        return np.where(pos, mass / np.where(pos, rho, F32(1.0)), F32(0.0)).astype(F32)


def distance(c, d2):
    d = np.sqrt(np.asarray(d2, F32))
    if not c.unit:
        d = d * c.sim_scale
    return d.astype(F32)


def weight(c, V, d):
    with np.errstate(invalid="ignore", over="ignore"):
        L = c.kernel3 * (c.hscaled - d)
        return (V * L).astype(F32)


def pair_terms(c, d2, Vj, Tj, Ti):
    """(terms (k, 4), on (k,)) of k pairs: the addends of the four sums, and which pairs are added at all."""
    w = weight(c, np.asarray(Vj, F32), distance(c, d2))
    with np.errstate(invalid="ignore", over="ignore"):
        terms = ((np.asarray(Tj, F32) - np.asarray(Ti, F32)) * w[:, None]).astype(F32)
    return terms, np.asarray(Vj, F32) != 0


def update(T, s, dt, kappa):
    """T' of rows T (m, 4) with the sums s (m, 4)."""
    T, s = np.asarray(T, F32), np.asarray(s, F32)
    kappa = np.asarray(kappa, F32).reshape(CHANNELS)
    out = T.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for ch in range(CHANNELS):
            if kappa[ch] > 0:
                out[:, ch] = T[:, ch] + (F32(dt) * kappa[ch]) * s[:, ch]
    return out


def apply_sources(T, pos, dt, sources):
    """The sources in list order on rows T (m, 4) of particles at pos (m, 3); returns the new rows."""
    T = np.asarray(T, F32).copy()
    pos = np.asarray(pos, F32).reshape(-1, 3)
    for q in sources:
        with np.errstate(invalid="ignore"):
            inside = ((pos > q.lo[None, :]) & (pos < q.hi[None, :])).all(1)
        if q.kind == HOLD:
            T[inside, q.channel] = F32(q.value)
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                T[inside, q.channel] = T[inside, q.channel] + F32(q.value) * F32(dt)
    return T


def particle(c, dt, kappa, sources, pi, Ti, pj, Tj, mj, rhoj):
    """One particle at pi carrying Ti with the CANDIDATES pj (k, 3), Tj (k, 4), mj, rhoj in the order given: the
    members are those with d2 < h2.  Returns its new row - what tests/test_scalars_cpu.py's g++ program computes
    with the header's functions."""
    pi = np.asarray(pi, F32).reshape(3)
    Ti = np.asarray(Ti, F32).reshape(1, CHANNELS)
    pj = np.asarray(pj, F32).reshape(-1, 3)
    Tj = np.asarray(Tj, F32).reshape(-1, CHANNELS)
    with np.errstate(invalid="ignore", over="ignore"):
        d = pi[None, :] - pj
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        member = d2 < c.h2
    terms, on = pair_terms(c, d2[member], volume(np.asarray(mj, F32)[member], np.asarray(rhoj, F32)[member]), Tj[member], Ti)
    s = np.zeros((1, CHANNELS), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in terms[on]:
            s[0] = s[0] + t
    return apply_sources(update(Ti, s, dt, kappa), pi[None, :], dt, sources)[0]


def step(p, pos, vel, mass, rho, T, kappa, sources=(), dt=None):
    """One step of the scalars in the state (pos, vel, mass) with the particle densities rho, everything in
    particle (ID) order: the new rows T' (n, 4) in the same order."""
    c = consts_of(p)
    dt = F32(p.time_step if dt is None else dt)
    T = np.asarray(T, F32).reshape(-1, CHANNELS)
    n = T.shape[0]
    if n == 0:
        return T.copy()
    order = PE.canonical_order(p, pos)
    grid = SE.Grid(p, pos, vel, mass)
    Ts = T[order]
    Vs = volume(grid.mass, np.asarray(rho, F32)[order])
    probe, idx, d2 = PE.members(grid, grid.pos, exclude_self=True)
    terms, on = pair_terms(c, d2, Vs[idx], Ts[idx], Ts[probe])
    sums, _ = PE.ordered_sums(probe[on], n, [terms[on][:, ch] for ch in range(CHANNELS)])
    new = apply_sources(update(Ts, np.stack(sums, 1), dt, kappa), grid.pos, dt, sources)
    out = np.zeros_like(T)
    out[order] = new
    return out


def stability(p, pos, vel, mass, rho, dt=None):
    """dt * sum_j V_j * L(d_ij) per particle (float64, particle order): times kappa[c] it must stay <= 1 for a
    step to be a convex combination."""
    c = consts_of(p)
    dt = float(p.time_step if dt is None else dt)
    order = PE.canonical_order(p, pos)
    grid = SE.Grid(p, pos, vel, mass)
    Vs = volume(grid.mass, np.asarray(rho, F32)[order]).astype(np.float64)
    probe, idx, d2 = PE.members(grid, grid.pos, exclude_self=True)
    d = np.sqrt(d2.astype(np.float64)) * (1.0 if c.unit else float(c.sim_scale))
    w = Vs[idx] * float(c.kernel3) * (float(c.hscaled) - d)
    out = np.zeros(grid.mass.size)
    out[order] = np.bincount(probe, weights=w, minlength=grid.mass.size) * dt
    return out


def sample(p, pos, vel, mass, T, probes):
    """sph_hip_sample_scalars_points: (channels (m, 4), rho (m,), count (m,)) of the probes."""
    probes = np.asarray(probes, F32).reshape(-1, 3)
    m = probes.shape[0]
    if np.asarray(mass).size == 0 or m == 0:
        return np.zeros((m, CHANNELS), F32), np.zeros(m, F32), np.zeros(m, np.int32)
    grid = SE.Grid(p, pos, vel, mass)
    Ts = np.asarray(T, F32).reshape(-1, CHANNELS)[PE.canonical_order(p, pos)]
    probe, idx, d2 = PE.members(grid, probes)
    t = SE.density_terms(grid.p, d2, grid.mass[idx])
    with np.errstate(invalid="ignore", over="ignore"):
        cols = [t] + [(t * Ts[idx, ch]).astype(F32) for ch in range(CHANNELS)]
    sums, count = PE.ordered_sums(probe, m, cols)
    rho = sums[0]
    return np.stack([PE.quotient(a, rho) for a in sums[1:]], 1), rho, count
