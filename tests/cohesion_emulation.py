"""numpy restatement of cohesion (csrc/cohesion_policy.h; include/sph_hip.h: cohesion) on top of the field sampler's
restatement (sample_emulation: the canonical order, the density pass's pair term) and the pressure readings'
(pressure_emulation: members in canonical order, sums added one by one), the checker of tests/test_gpu_cohesion.py
and tests/test_cohesion_cpu.py.

    members  j with (dx*dx + dy*dy) + dz*dz < h2, (dx, dy, dz) = r_i - r_j, i excluded, in canonical order
    w_j      m_j * (kernel1 * (hscaled2 - d*d)^3), d = sqrt(d2) times sim_scale unless unit scale; off unit scale
             +0 where d > hscaled (sample_emulation.density_terms)
    s        0, then for every member in order: s = s + w_j * r, r = (dx, dy, dz), times sim_scale first unless unit scale
    c        (-gamma) * s
    guard    c == 0 in all three components, or not finite in any: the row does not change
    a'       a + c, then accel_end's clamp (buoyancy_emulation.clamp)
numpy evaluates float32 arrays operation by operation with IEEE rounding and never fuses, so the bits are the
device's.  step() composes one whole FULL step from the oracle's phases (test infrastructure), apply() and, where
the context carries scalars or a buoyancy, their restatements."""
import numpy as np

import buoyancy_emulation as BE
import pressure_emulation as PE
import sample_emulation as SE
import scalar_emulation as SC
from helpers import to_oracle_params

F32 = np.float32


def pair_terms(p, d2, mass_j, r):
    """The addends (k, 3) of k members: d2 (k,), the neighbours' masses (k,), the separations r_i - r_j (k, 3)."""
    with np.errstate(invalid="ignore", over="ignore"):
        w = SE.density_terms(p, np.asarray(d2, F32), np.asarray(mass_j, F32))
        r = np.asarray(r, F32)
        if not SE.unit_scale(p):
            r = r * F32(p.sim_scale)
        return (w[:, None] * r).astype(F32)


def accel(gamma, s):
    with np.errstate(invalid="ignore", over="ignore"):
        return ((-F32(gamma)) * np.asarray(s, F32)).astype(F32)


def acts(c):
    c = np.asarray(c, F32).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        return (c != 0).any(1) & (np.abs(c) <= F32(3.402823466e38)).all(1)


def add(p, acc, c):
    """Rows acc (m, 3) with the cohesive accelerations c (m, 3): (acc', touched)."""
    acc = np.asarray(acc, F32).reshape(-1, 3)
    c = np.asarray(c, F32).reshape(-1, 3)
    on = acts(c)
    out = acc.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        out[on] = BE.clamp(acc[on] + c[on], p.cfl_limit, p.cfl_limit2)
    return out, on


def particle(p, gamma, pi, pj, mj, acc):
    """One particle at pi with the CANDIDATES pj (k, 3), mj (k,) in the order given - the members are those with
    d2 < h2 - and its acceleration acc (3,): (acc', touched, c) - what tests/test_cohesion_cpu.py's g++ shim
    computes with the header's functions."""
    pi = np.asarray(pi, F32).reshape(3)
    pj = np.asarray(pj, F32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        r = pi[None, :] - pj
        d2 = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2]
        member = d2 < F32(p.h2)
    terms = pair_terms(p, d2[member], np.asarray(mj, F32)[member], r[member])
    s = np.zeros(3, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in terms:
            s = s + t
    c = accel(gamma, s)
    out, on = add(p, np.asarray(acc, F32).reshape(1, 3), c.reshape(1, 3))
    return out[0], bool(on[0]), c


def sums(p, pos, vel, mass):
    """s of every particle of the state, (n, 3) in particle order."""
    n = np.asarray(mass).size
    if n == 0:
        return np.zeros((0, 3), F32)
    order = PE.canonical_order(p, pos)
    grid = SE.Grid(p, pos, vel, mass)
    probe, idx, d2 = PE.members(grid, grid.pos, exclude_self=True)
    with np.errstate(invalid="ignore", over="ignore"):
        r = grid.pos[probe] - grid.pos[idx]
    terms = pair_terms(p, d2, grid.mass[idx], r)
    cols, _ = PE.ordered_sums(probe, n, [terms[:, a] for a in range(3)])
    out = np.zeros((n, 3), F32)
    out[order] = np.stack(cols, 1)
    return out


def apply(p, gamma, pos, vel, mass, acc):
    """The kernel on the state (pos, vel, mass) with the accelerations acc (3n,), everything in particle order.
    Returns (acc' (3n,), touched (n,), c (n, 3))."""
    c = accel(gamma, sums(p, pos, vel, mass))
    out, on = add(p, acc, c)
    return np.ascontiguousarray(out.reshape(-1)), on, c


def step(orc, p, pos, vel, mass, gamma, T=None, kappa=None, sources=(), b=None, integrate=None):
    """One whole FULL step of a context with the cohesion gamma (0 or None: none) and, with T, carried scalars and
    the buoyancy b (None: none), everything in particle order: the oracle's cells and densities, the scalars' step,
    the oracle's accelerations, apply(), buoyancy's apply() on what cohesion left, the oracle's integrate - or
    integrate(op, pos, vel, acc, mass), in place on pos and vel, where a context's integrate does more.  Returns
    dict(pos, vel, acc, acc_before, rho, T, touched, c); nothing given is changed."""
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
    if gamma:
        acc, touched, c = apply(p, gamma, pos, vel, mass, acc)
    if b is not None:
        acc, vel, _ = BE.apply(p, b, T, acc, vel)
        acc, vel = np.ascontiguousarray(acc), np.ascontiguousarray(vel)
    (integrate or orc.integrate)(op, pos, vel, acc, mass)
    return dict(pos=pos, vel=vel, acc=acc, acc_before=before, rho=rho, T=T_new, touched=touched, c=c)


def shell(pos, h):
    """Which particles of a cubic fill stand within h/2 of a face of its bounding box."""
    x = np.asarray(pos, np.float64).reshape(-1, 3)
    return (np.minimum(x - x.min(0), x.max(0) - x).min(1) < 0.5 * float(h))


def inward_fraction(pos, c, h):
    """The share of shell particles whose c points towards the centroid (float64)."""
    x = np.asarray(pos, np.float64).reshape(-1, 3)
    sh = shell(pos, h)
    radial = ((x.mean(0) - x) * np.asarray(c, np.float64).reshape(-1, 3)).sum(1)
    return float((radial[sh] > 0).mean()), int(sh.sum())


def rms_radius(pos):
    x = np.asarray(pos, np.float64).reshape(-1, 3)
    return float(np.sqrt(((x - x.mean(0)) ** 2).sum(1).mean()))
