"""numpy restatement of XSPH velocity smoothing (csrc/xsph_policy.h; include/sph_hip.h: xsph) on top of the field
sampler's restatement (sample_emulation: the canonical order, the density pass's pair term), the pressure readings'
(pressure_emulation: members in canonical order, sums added one by one) and cohesion's (cohesion_emulation: the
guard, the composed step), the checker of tests/test_gpu_xsph.py and tests/test_xsph_cpu.py.

    stage    R = (v.x, v.y, v.z, 1 / rho), one correctly rounded division
    members  j with (dx*dx + dy*dy) + dz*dz < h2, (dx, dy, dz) = r_i - r_j, i excluded, in canonical order
    w_j      m_j * (kernel1 * (hscaled2 - d*d)^3), d = sqrt(d2) times sim_scale unless unit scale; off unit scale
             +0 where d > hscaled (sample_emulation.density_terms)
    g_ij     w_j * (0.5 * (R_i.w + R_j.w))
    s        0, then for every member in order: s = s + g_ij * (R_j.xyz - R_i.xyz)
    dv       eps * s
    guard    dv == 0 in all three components, or not finite in any: the row does not change
    v'       v + dv; no clamp, acc is not touched
numpy evaluates float32 arrays operation by operation with IEEE rounding and never fuses, so the bits are the
device's.  step() composes one whole FULL step from the oracle's phases (test infrastructure), cohesion's apply(),
this apply() and, where the context carries scalars or a buoyancy, their restatements."""
import numpy as np

import buoyancy_emulation as BE
import cohesion_emulation as CE
import pressure_emulation as PE
import sample_emulation as SE
import scalar_emulation as SC
from helpers import to_oracle_params

F32 = np.float32


def stage(vel, rho):
    """R (n, 4) of rows in any one order: vel (3n,) or (n, 3), rho (n,)."""
    vel = np.asarray(vel, F32).reshape(-1, 3)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rinv = (F32(1.0) / np.asarray(rho, F32).reshape(-1)).astype(F32)
    return np.concatenate([vel, rinv[:, None]], 1).astype(F32)


def weights(p, d2, mass_j, rinv_i, rinv_j):
    """g_ij (k,) of k members."""
    with np.errstate(invalid="ignore", over="ignore"):
        w = SE.density_terms(p, np.asarray(d2, F32), np.asarray(mass_j, F32))
        mean = (F32(0.5) * (np.asarray(rinv_i, F32) + np.asarray(rinv_j, F32))).astype(F32)
        return (w * mean).astype(F32)


def pair_terms(p, d2, mass_j, Ri, Rj):
    """The addends (k, 3) of k members: d2 (k,), the neighbours' masses (k,), the particles' own staged rows Ri
    (k, 4) and the neighbours' Rj (k, 4).  Returns (terms, g)."""
    Ri = np.asarray(Ri, F32).reshape(-1, 4)
    Rj = np.asarray(Rj, F32).reshape(-1, 4)
    g = weights(p, d2, mass_j, Ri[:, 3], Rj[:, 3])
    with np.errstate(invalid="ignore", over="ignore"):
        dv = (Rj[:, :3] - Ri[:, :3]).astype(F32)
        return (g[:, None] * dv).astype(F32), g


def change(eps, s):
    with np.errstate(invalid="ignore", over="ignore"):
        return (F32(eps) * np.asarray(s, F32)).astype(F32)


acts = CE.acts      # cohesion's rule: some component not zero, every component finite


def add(vel, dv):
    """Rows vel (m, 3) with the changes dv (m, 3): (vel', touched)."""
    vel = np.asarray(vel, F32).reshape(-1, 3)
    dv = np.asarray(dv, F32).reshape(-1, 3)
    on = acts(dv)
    out = vel.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        out[on] = vel[on] + dv[on]
    return out, on


def particle(p, eps, pi, Ri, pj, mj, Rj):
    """One particle at pi with its staged row Ri (4,) and the CANDIDATES pj (k, 3), mj (k,), Rj (k, 4) in the order
    given - the members are those with d2 < h2: (v', touched, dv) - what tests/test_xsph_cpu.py's g++ shim computes
    with the header's functions."""
    pi = np.asarray(pi, F32).reshape(3)
    pj = np.asarray(pj, F32).reshape(-1, 3)
    Ri = np.asarray(Ri, F32).reshape(4)
    Rj = np.asarray(Rj, F32).reshape(-1, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        r = pi[None, :] - pj
        d2 = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2]
        member = d2 < F32(p.h2)
    k = int(member.sum())
    terms, _ = pair_terms(p, d2[member], np.asarray(mj, F32)[member], np.repeat(Ri[None, :], k, 0), Rj[member])
    s = np.zeros(3, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in terms:
            s = s + t
    dv = change(eps, s)
    out, on = add(Ri[None, :3], dv.reshape(1, 3))
    return out[0], bool(on[0]), dv


def sums(p, pos, vel, mass, rho, with_info=False):
    """s of every particle of the state, (n, 3) in particle order; with_info also dict(g_sum (n,) float64: the sum
    of every particle's weights, count (n,), probe, terms: the addends in device order, probe the canonical index
    of the particle each belongs to)."""
    n = np.asarray(mass).size
    if n == 0:
        out = np.zeros((0, 3), F32)
        return (out, dict(g_sum=np.zeros(0), count=np.zeros(0, np.int32), probe=np.zeros(0, np.int64),
                          terms=np.zeros((0, 3), F32))) if with_info else out
    order = PE.canonical_order(p, pos)
    grid = SE.Grid(p, pos, vel, mass)
    R = stage(grid.vel, np.asarray(rho, F32).reshape(-1)[order])
    probe, idx, d2 = PE.members(grid, grid.pos, exclude_self=True)
    terms, g = pair_terms(p, d2, grid.mass[idx], R[probe], R[idx])
    cols, count = PE.ordered_sums(probe, n, [terms[:, a] for a in range(3)])
    out = np.zeros((n, 3), F32)
    out[order] = np.stack(cols, 1)
    if not with_info:
        return out
    g_sum = np.zeros(n, np.float64)
    g_sum[order] = np.bincount(probe, weights=g.astype(np.float64), minlength=n)
    cnt = np.zeros(n, np.int32)
    cnt[order] = count
    return out, dict(g_sum=g_sum, count=cnt, probe=probe, terms=terms)


def apply(p, eps, pos, vel, mass, rho):
    """The kernel pair on the state (pos, vel, mass) with the densities rho (n,), everything in particle order.
    Returns (vel' (3n,), touched (n,), dv (n, 3))."""
    dv = change(eps, sums(p, pos, vel, mass, rho))
    out, on = add(vel, dv)
    return np.ascontiguousarray(out.reshape(-1)), on, dv


def step(orc, p, pos, vel, mass, eps, gamma=0.0, T=None, kappa=None, sources=(), b=None, integrate=None):
    """One whole FULL step of a context with the smoothing eps (0 or None: none), the cohesion gamma (0 or None:
    none) and, with T, carried scalars and the buoyancy b (None: none), everything in particle order: the oracle's
    cells and densities, the scalars' step, the oracle's accelerations, cohesion's apply(), this apply(), buoyancy's
    apply() on what the two left, the oracle's integrate - or integrate(op, pos, vel, acc, mass), in place on pos
    and vel, where a context's integrate does more.  Returns dict(pos, vel, acc, acc_before, vel_before, rho, T,
    touched, dv); nothing given is changed."""
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
    vel_before = vel.copy()
    touched = np.zeros(mass.size, bool)
    dv = np.zeros((mass.size, 3), F32)
    if gamma:
        acc, _, _ = CE.apply(p, gamma, pos, vel, mass, acc)
    if eps:
        vel, touched, dv = apply(p, eps, pos, vel, mass, rho)
    if b is not None:
        acc, vel, _ = BE.apply(p, b, T, acc, vel)
    acc, vel = np.ascontiguousarray(acc, F32), np.ascontiguousarray(vel, F32)
    (integrate or orc.integrate)(op, pos, vel, acc, mass)
    return dict(pos=pos, vel=vel, acc=acc, acc_before=before, vel_before=vel_before, rho=rho, T=T_new, touched=touched,
                dv=dv)


def kinetic_about_mean(vel, mass):
    """sum_i m_i |v_i - vbar|^2 / 2 in float64, vbar the mass-weighted mean velocity."""
    v = np.asarray(vel, np.float64).reshape(-1, 3)
    m = np.asarray(mass, np.float64)
    vbar = (m[:, None] * v).sum(0) / m.sum()
    return float(0.5 * (m * ((v - vbar) ** 2).sum(1)).sum())
