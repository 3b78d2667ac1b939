"""numpy restatement of the viscous stress (csrc/viscous_policy.h; include/sph_hip.h: viscous stress) on top of the
field sampler's restatement (sample_emulation: the canonical order), the pressure readings' (pressure_emulation:
members in canonical order, sums added one by one), the scalars' (scalar_emulation: the volume, the distance),
cohesion's (cohesion_emulation: the guard, the clamped add) and XSPH's (xsph_emulation: its apply in the composed step),
the checker of tests/test_gpu_viscous.py and tests/test_viscous_cpu.py.

    law      factor(x): f_0 where !(x > x_0); f_{K-1} where x >= x_{K-1}; else f_k + u * (f_{k+1} - f_k),
             u = (x - x_k) / (x_{k+1} - x_k), x_k <= x < x_{k+1}
    stage    R = (v.x, v.y, v.z, V), V = rho > 0 ? m / rho : 0; with a law M = mu * factor(Ts.c)
    members  j with (dx*dx + dy*dy) + dz*dz < h2, (dx, dy, dz) = r_i - r_j, i excluded, in canonical order
    L        kernel3 * (hscaled - d), d = sqrt(d2) times sim_scale unless unit scale
    g_ij     (m_ij * (V_i * V_j)) * L, m_ij = 0.5 * (M_i + M_j) with a law, else mu
    s        0, then for every member with V_j != 0 in order: s = s + g_ij * (R_j.xyz - R_i.xyz)
    c        s / m_i
    guard    V_i == 0, m_i not > 0, c == 0 in all three components, or not finite in any: the row does not change
    a'       clamp(a + c); the velocity is not touched
    N_i      dt * (1 / m_i) * sum_j m_ij V_i V_j L in float64: the step is a convex combination while N_i <= 1
numpy evaluates float32 arrays operation by operation with IEEE rounding and never fuses, so the bits are the
device's.  step() composes one whole FULL step from the oracle's phases (test infrastructure), cohesion's apply(),
this apply(), XSPH's apply() and, where the context carries scalars or a buoyancy, their restatements."""
import collections

import numpy as np

import buoyancy_emulation as BE
import cohesion_emulation as CE
import pressure_emulation as PE
import sample_emulation as SE
import scalar_emulation as SC
import xsph_emulation as XE
from helpers import to_oracle_params

F32 = np.float32
MAX_KEYS = 16

# a law: the channel, the key values (K,) and the key factors (K,), fp32
Law = collections.namedtuple("Law", ["channel", "values", "factors"])


def law(channel, values, factors):
    return Law(int(channel), np.asarray(values, F32).reshape(-1).copy(), np.asarray(factors, F32).reshape(-1).copy())


def of(viscosity_law):
    """The restatement's form of a smoothed_particle_hydrodynamics_amd.ViscosityLaw (None stays None)."""
    if viscosity_law is None:
        return None
    return law(viscosity_law.channel, viscosity_law.values, viscosity_law.factors)


def factor(lw, x):
    """The law at the values x (any shape), fp32."""
    x = np.asarray(x, F32)
    v, f = lw.values, lw.factors
    K = v.size
    out = np.full(x.shape, f[0], F32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        above = x > v[0]
        for k in range(K - 1):
            inside = above & (x >= v[k]) & (x < v[k + 1])
            u = ((x - v[k]) / (v[k + 1] - v[k])).astype(F32)
            t = (f[k] + (u * (f[k + 1] - f[k])).astype(F32)).astype(F32)
            out = np.where(inside, t, out)
        out = np.where(above & (x >= v[K - 1]), f[K - 1], out)
    return out.astype(F32)


def stage(vel, mass, rho):
    """R (n, 4) of rows in any one order: vel (3n,) or (n, 3), mass (n,), rho (n,)."""
    vel = np.asarray(vel, F32).reshape(-1, 3)
    return np.concatenate([vel, SC.volume(mass, rho)[:, None]], 1).astype(F32)


def stage_mu(mu, lw, Ts):
    """M (n,) of the staged channel rows Ts (n, 4)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (F32(mu) * factor(lw, np.asarray(Ts, F32).reshape(-1, 4)[:, lw.channel])).astype(F32)


def pair_mu(mu, Mi, Mj):
    """m_ij of k pairs: the mean of the staged viscosities, or mu where there is no law (Mi is None)."""
    if Mi is None:
        return F32(mu)
    with np.errstate(invalid="ignore", over="ignore"):
        return (F32(0.5) * (np.asarray(Mi, F32) + np.asarray(Mj, F32))).astype(F32)


def pair_terms(p, mu, d2, Ri, Rj, Mi=None, Mj=None):
    """The addends (k, 3) of k members: d2 (k,), the particles' own staged rows Ri (k, 4), the neighbours' Rj
    (k, 4) and, with a law, the staged viscosities of both.  Returns (terms, on, g): on (k,) which members are added
    at all."""
    c = SC.consts_of(p)
    Ri = np.asarray(Ri, F32).reshape(-1, 4)
    Rj = np.asarray(Rj, F32).reshape(-1, 4)
    d = SC.distance(c, d2)
    with np.errstate(invalid="ignore", over="ignore"):
        L = (c.kernel3 * (c.hscaled - d)).astype(F32)
        vv = (Ri[:, 3] * Rj[:, 3]).astype(F32)
        g = ((pair_mu(mu, Mi, Mj) * vv).astype(F32) * L).astype(F32)
        dv = (Rj[:, :3] - Ri[:, :3]).astype(F32)
        return (g[:, None] * dv).astype(F32), Rj[:, 3] != 0, g


def accel(s, m):
    """c (k, 3) of the sums s (k, 3) and the particles' own masses m (k,)."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return (np.asarray(s, F32).reshape(-1, 3) / np.asarray(m, F32).reshape(-1, 1)).astype(F32)


def acts(Vi, m, c):
    with np.errstate(invalid="ignore"):
        return (np.asarray(Vi, F32) != 0) & (np.asarray(m, F32) > 0) & CE.acts(c)


def add(p, acc, c, Vi, m):
    """Rows acc (k, 3) with the viscous accelerations c (k, 3): (acc', touched)."""
    acc = np.asarray(acc, F32).reshape(-1, 3)
    c = np.asarray(c, F32).reshape(-1, 3)
    on = acts(Vi, m, c)
    out = acc.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        out[on] = BE.clamp(acc[on] + c[on], p.cfl_limit, p.cfl_limit2)
    return out, on


def particle(p, mu, pi, mi, Ri, pj, Rj, acc, Mi=None, Mj=None, dt=None):
    """One particle at pi with the mass mi, its staged row Ri (4,) and its acceleration acc (3,), and the CANDIDATES
    pj (k, 3), Rj (k, 4) in the order given - the members are those with d2 < h2; with a law its staged viscosity
    Mi and the candidates' Mj (k,).  Returns (acc', touched, c, N): what tests/test_viscous_cpu.py's g++ shim
    computes with the header's functions, and N_i."""
    pi = np.asarray(pi, F32).reshape(3)
    pj = np.asarray(pj, F32).reshape(-1, 3)
    Ri = np.asarray(Ri, F32).reshape(4)
    Rj = np.asarray(Rj, F32).reshape(-1, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        r = pi[None, :] - pj
        d2 = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2]
        member = d2 < F32(p.h2)
    k = int(member.sum())
    have_law = Mi is not None
    terms, on, g = pair_terms(p, mu, d2[member], np.repeat(Ri[None, :], k, 0), Rj[member],
                              np.repeat(F32(Mi), k) if have_law else None,
                              np.asarray(Mj, F32)[member] if have_law else None)
    s = np.zeros(3, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in terms[on]:
            s = s + t
    c = accel(s.reshape(1, 3), np.array([mi], F32))
    out, touched = add(p, np.asarray(acc, F32).reshape(1, 3), c, Ri[3:4], np.array([mi], F32))
    dt = float(p.time_step if dt is None else dt)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        N = dt * float(g[on].astype(np.float64).sum()) / float(mi) if float(mi) != 0 else np.inf
    return out[0], bool(touched[0]), c[0], N


def sums(p, mu, pos, vel, mass, rho, lw=None, T=None, with_info=False):
    """s of every particle of the state, (n, 3) in particle order; lw with the channel rows T (n, 4) in particle
    order: the law.  with_info also dict(g_sum (n,) float64: the sum of every particle's g_ij over the members that
    are added, count (n,), probe, idx, terms, on: the addends in device order, probe the canonical index of the
    particle each belongs to and idx its neighbour's, R (n, 4) and order)."""
    n = np.asarray(mass).size
    order = PE.canonical_order(p, pos)
    grid = SE.Grid(p, pos, vel, mass)
    R = stage(grid.vel, grid.mass, np.asarray(rho, F32).reshape(-1)[order])
    M = None if lw is None else stage_mu(mu, lw, np.asarray(T, F32).reshape(-1, 4)[order])
    probe, idx, d2 = PE.members(grid, grid.pos, exclude_self=True)
    terms, on, g = pair_terms(p, mu, d2, R[probe], R[idx], None if M is None else M[probe], None if M is None else M[idx])
    cols, _ = PE.ordered_sums(probe[on], n, [terms[on][:, a] for a in range(3)])
    out = np.zeros((n, 3), F32)
    out[order] = np.stack(cols, 1)
    if not with_info:
        return out
    g_sum = np.zeros(n, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        g_sum[order] = np.bincount(probe[on], weights=g[on].astype(np.float64), minlength=n)
    cnt = np.zeros(n, np.int32)
    cnt[order] = np.bincount(probe, minlength=n)
    return out, dict(g_sum=g_sum, count=cnt, probe=probe, idx=idx, terms=terms, on=on, R=R, order=order)


def apply(p, mu, pos, vel, mass, rho, acc, lw=None, T=None, dt=None, with_info=False):
    """The kernel pair on the state (pos, vel, mass) with the densities rho (n,) and the accelerations acc (3n,),
    everything in particle order.  Returns (acc' (3n,), touched (n,), c (n, 3), N (n,)): N_i = dt * g_sum_i / m_i in
    float64; with_info also sums' dict."""
    mass = np.asarray(mass, F32).reshape(-1)
    s, info = sums(p, mu, pos, vel, mass, rho, lw, T, with_info=True)
    c = accel(s, mass)
    out, on = add(p, acc, c, SC.volume(mass, rho), mass)
    dt = float(p.time_step if dt is None else dt)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        N = dt * info["g_sum"] / mass.astype(np.float64)
    res = (np.ascontiguousarray(out.reshape(-1)), on, c, N)
    return res + (info,) if with_info else res


def step(orc, p, pos, vel, mass, mu, lw=None, gamma=0.0, eps=0.0, T=None, kappa=None, sources=(), b=None, integrate=None):
    """One whole FULL step of a context with the viscous stress mu (0 or None: none) and its law lw (None: a constant
    mu), the cohesion gamma, the smoothing eps and, with T, carried scalars and the buoyancy b (None: none),
    everything in particle order: the oracle's cells and densities, the scalars' step, the oracle's accelerations,
    cohesion's apply(), this apply() - with the channels T as they stood before the step - XSPH's apply(), buoyancy's
    apply(), the oracle's integrate - or integrate(op, pos, vel, acc, mass), in place on pos and vel, where a
    context's integrate does more.  Returns dict(pos, vel, acc, acc_before, rho, T, touched, c, N); nothing given is
    changed."""
    op = to_oracle_params(p)
    pos = np.ascontiguousarray(pos, F32).copy()
    vel = np.ascontiguousarray(vel, F32).copy()
    mass = np.ascontiguousarray(mass, F32)
    _, cs, ci = orc.full_cells(op, pos)
    rho, _ = orc.full_density(op, pos, mass, cs, ci)
    T_new = None
    if T is not None:
        T = np.asarray(T, F32).reshape(-1, 4)
        idle = not np.asarray(kappa, F32).any() and len(sources) == 0
        T_new = T.copy() if idle else SC.step(p, pos, vel, mass, rho, T, kappa, sources)
    acc = orc.full_accel(op, pos, vel, mass, rho, cs, ci)
    before = acc.copy()
    touched = np.zeros(mass.size, bool)
    c = np.zeros((mass.size, 3), F32)
    N = np.zeros(mass.size)
    if gamma:
        acc, _, _ = CE.apply(p, gamma, pos, vel, mass, acc)
    if mu:
        acc, touched, c, N = apply(p, mu, pos, vel, mass, rho, acc, lw, T)
    if eps:
        vel, _, _ = XE.apply(p, eps, pos, vel, mass, rho)
    if b is not None:
        acc, vel, _ = BE.apply(p, b, T, acc, vel)
    acc, vel = np.ascontiguousarray(acc, F32), np.ascontiguousarray(vel, F32)
    (integrate or orc.integrate)(op, pos, vel, acc, mass)
    return dict(pos=pos, vel=vel, acc=acc, acc_before=before, rho=rho, T=T_new, touched=touched, c=c, N=N)


kinetic_about_mean = XE.kinetic_about_mean
