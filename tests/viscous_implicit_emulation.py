"""numpy restatement of the implicit viscous stress (csrc/viscous_implicit_policy.h; include/sph_hip.h: implicit viscous
stress) on top of the explicit term's restatement (viscous_emulation: the stage, the staged viscosities, the members and
pair_terms' g), the checker of tests/test_gpu_viscous_implicit.py and tests/test_viscous_implicit_cpu.py.

    stage    viscous_emulation's: X0 = R = (v, V), M with a law
    sweep    for particle i with v0 = its own velocity of the step's state, over the explicit term's members in its
             order with V_j != 0, from the rows Xa of the sweep before:
                 s = s + g_ij * (Xa_j.xyz - v0),  D = D + g_ij          both from 0, g_ij viscous_emulation.pair_terms'
             den = m_i + dt * D;  dv = (dt * s) / den
    guard    acts = V_i != 0 and m_i > 0 and den > 0 and cohesion's rule on dv
    store    not the last sweep: Xb_i = (acts ? v0 + dv : v0, V_i); the last: v_i = v0 + dv where acts
numpy evaluates float32 arrays operation by operation with IEEE rounding and never fuses, so the bits are the
device's.  step() composes one whole FULL step as viscous_emulation.step does, with solve() in apply()'s place: the
velocities change in front of XSPH and buoyancy, the accelerations do not."""
import numpy as np

import buoyancy_emulation as BE
import cohesion_emulation as CE
import pressure_emulation as PE
import sample_emulation as SE
import scalar_emulation as SC
import viscous_emulation as VE
import xsph_emulation as XE
from helpers import to_oracle_params

F32 = np.float32
MAX_SWEEPS = 64


def change(s, D, m, dt):
    """(den (k,), dv (k, 3)) of the sums s (k, 3), D (k,) and the particles' own masses m (k,)."""
    dt = F32(dt)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        den = (np.asarray(m, F32) + (dt * np.asarray(D, F32)).astype(F32)).astype(F32)
        dv = ((dt * np.asarray(s, F32).reshape(-1, 3)).astype(F32) / den.reshape(-1, 1)).astype(F32)
    return den, dv


def acts(Vi, m, den, dv):
    with np.errstate(invalid="ignore"):
        return (np.asarray(Vi, F32) != 0) & (np.asarray(m, F32) > 0) & (np.asarray(den, F32) > 0) & CE.acts(dv)


def moved(v0, dv, on):
    """v0 + dv where on, else v0: (k, 3)"""
    v0 = np.asarray(v0, F32).reshape(-1, 3)
    out = v0.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        out[on] = (v0[on] + dv[on]).astype(F32)
    return out


def particle(p, mu, pi, mi, v0, Vi, pj, Xj, Mi=None, Mj=None, dt=None):
    """One particle at pi with the mass mi, its own velocity v0 (3,) and volume Vi, and the CANDIDATES pj (k, 3) with
    the rows Xj (k, 4) of the sweep before, in the order given - the members are those with d2 < h2; with a law its
    staged viscosity Mi and the candidates' Mj (k,).  Returns (x (3,): v0 + dv where it acts, else v0; acts; dv (3,);
    s (3,); D; den): what tests/test_viscous_implicit_cpu.py's g++ shim computes with the header's functions."""
    pi = np.asarray(pi, F32).reshape(3)
    pj = np.asarray(pj, F32).reshape(-1, 3)
    v0 = np.asarray(v0, F32).reshape(3)
    Xj = np.asarray(Xj, F32).reshape(-1, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        r = pi[None, :] - pj
        d2 = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2]
        member = d2 < F32(p.h2)
    k = int(member.sum())
    have_law = Mi is not None
    Ri = np.repeat(np.concatenate([v0, [F32(Vi)]]).astype(F32)[None, :], k, 0)
    terms, on, g = VE.pair_terms(p, mu, d2[member], Ri, Xj[member], np.repeat(F32(Mi), k) if have_law else None,
                                 np.asarray(Mj, F32)[member] if have_law else None)
    s, D = np.zeros(3, F32), F32(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for t, w in zip(terms[on], g[on]):
            s = s + t
            D = F32(D + w)
    dt = F32(p.time_step if dt is None else dt)
    m = np.array([mi], F32)
    den, dv = change(s.reshape(1, 3), np.array([D], F32), m, dt)
    on_i = acts(np.array([Vi], F32), m, den, dv)
    return moved(v0, dv, on_i)[0], bool(on_i[0]), dv[0], s, D, den[0]


class Pairs:
    """The pairs of a state, formed once for every sweep of a step: the canonical order, the staged rows R and
    viscosities M, and per member (probe, idx, g, on) in device order."""

    def __init__(self, p, mu, pos, vel, mass, rho, lw=None, T=None):
        self.p, self.n = p, np.asarray(mass).size
        self.order = PE.canonical_order(p, pos)
        grid = SE.Grid(p, pos, vel, mass)
        self.mass = grid.mass
        self.R = VE.stage(grid.vel, grid.mass, np.asarray(rho, F32).reshape(-1)[self.order])
        self.M = None if lw is None else VE.stage_mu(mu, lw, np.asarray(T, F32).reshape(-1, 4)[self.order])
        probe, idx, d2 = PE.members(grid, grid.pos, exclude_self=True)
        M = self.M
        _, on, g = VE.pair_terms(p, mu, d2, self.R[probe], self.R[idx], None if M is None else M[probe],
                                 None if M is None else M[idx])
        self.count = np.bincount(probe, minlength=self.n)
        self.probe, self.idx, self.g = probe[on], idx[on], g[on]
        self.v0 = self.R[:, :3].copy()
        self.V = self.R[:, 3].copy()

    def sums(self, X):
        """(s (n, 3), D (n,)) of the rows X (n, 3), everything in canonical order."""
        with np.errstate(invalid="ignore", over="ignore"):
            terms = (self.g[:, None] * (X[self.idx] - self.v0[self.probe]).astype(F32)).astype(F32)
        cols, _ = PE.ordered_sums(self.probe, self.n, [terms[:, 0], terms[:, 1], terms[:, 2], self.g])
        return np.stack(cols[:3], 1), cols[3]

    def sweep(self, X, dt):
        """One sweep from the rows X (n, 3): (X' (n, 3), acts (n,), dv, s, D, den), in canonical order."""
        s, D = self.sums(X)
        den, dv = change(s, D, self.mass, dt)
        on = acts(self.V, self.mass, den, dv)
        return moved(self.v0, dv, on), on, dv, s, D, den

    def unsorted(self, a):
        out = np.zeros_like(a)
        out[self.order] = a
        return out


def solve(p, mu, pos, vel, mass, rho, sweeps, lw=None, T=None, dt=None, with_info=False):
    """K Jacobi sweeps on the state (pos, vel, mass) with the densities rho (n,), everything in particle order.
    Returns (vel' (3n,), touched (n,): whom the last sweep stored); with_info also dict(iterates: the velocities
    (n, 3) after every sweep, s1: the first sweep's s (n, 3), g_sum (n,) float64, N (n,), count (n,), pairs)."""
    assert 1 <= int(sweeps) <= MAX_SWEEPS
    dt = F32(p.time_step if dt is None else dt)
    pairs = Pairs(p, mu, pos, vel, mass, rho, lw, T)
    X, iterates, s1, on = pairs.v0, [], None, None
    for k in range(int(sweeps)):
        X, on, _, s, _, _ = pairs.sweep(X, dt)
        if k == 0:
            s1 = s
        if with_info:
            iterates.append(pairs.unsorted(X))
    out = np.ascontiguousarray(pairs.unsorted(X).reshape(-1))
    touched = pairs.unsorted(on)
    if not with_info:
        return out, touched
    g_sum = np.bincount(pairs.probe, weights=pairs.g.astype(np.float64), minlength=pairs.n)
    with np.errstate(invalid="ignore", divide="ignore"):
        N = float(dt) * g_sum / pairs.mass.astype(np.float64)
    return out, touched, dict(iterates=iterates, s1=pairs.unsorted(s1), g_sum=pairs.unsorted(g_sum), N=pairs.unsorted(N),
                              count=pairs.unsorted(pairs.count), pairs=pairs)


def residual_sum(pairs, X, dt):
    """sum_i r_i per component in float64, r_i = m_i (x_i - v0_i) - dt * sum_j g_ij (x_j - x_i), X (n, 3) in canonical
    order: what the momentum defect sum_i m_i (x_i - v0_i) of a truncated solve equals (g_ij == g_ji by bits, so the
    pair sums cancel)."""
    X64, v64, g64 = X.astype(np.float64), pairs.v0.astype(np.float64), pairs.g.astype(np.float64)
    r = pairs.mass.astype(np.float64)[:, None] * (X64 - v64)
    pull = g64[:, None] * (X64[pairs.idx] - X64[pairs.probe])
    for a in range(3):
        r[:, a] -= float(dt) * np.bincount(pairs.probe, weights=pull[:, a], minlength=pairs.n)
    return r.sum(0)


def step(orc, p, pos, vel, mass, mu, sweeps, lw=None, gamma=0.0, eps=0.0, T=None, kappa=None, sources=(), b=None,
         integrate=None):
    """One whole FULL step of a context with the viscous stress mu, its law lw and the sweep count `sweeps` (0 or
    None: viscous_emulation.step, the explicit term), composed as viscous_emulation.step composes it with solve() in
    apply()'s place.  Returns dict(pos, vel, acc, rho, T, touched); nothing given is changed."""
    if not sweeps or not mu:
        return VE.step(orc, p, pos, vel, mass, mu, lw, gamma, eps, T, kappa, sources, b, integrate)
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
    if gamma:
        acc, _, _ = CE.apply(p, gamma, pos, vel, mass, acc)
    vel, touched = solve(p, mu, pos, vel, mass, rho, sweeps, lw, T)
    if eps:
        vel, _, _ = XE.apply(p, eps, pos, vel, mass, rho)
    if b is not None:
        acc, vel, _ = BE.apply(p, b, T, acc, vel)
    acc, vel = np.ascontiguousarray(acc, F32), np.ascontiguousarray(vel, F32)
    (integrate or orc.integrate)(op, pos, vel, acc, mass)
    return dict(pos=pos, vel=vel, acc=acc, rho=rho, T=T_new, touched=touched)


kinetic_about_mean = XE.kinetic_about_mean
