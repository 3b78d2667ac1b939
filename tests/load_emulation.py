"""numpy restatement of the load recording (csrc/load_policy.h, include/sph_hip.h: loads on walls and
obstacles), vectorised over particles.  The walls are restated from handle_boundaries / apply_boundary
(csrc/common_kernels.h; SPH::handleBoundaryConditions / applyBoundary, reference src/sph.cpp:1025-1148),
every operation in fp32 in its order; the obstacles go through obstacle_emulation.respond_one, one
obstacle at a time; the term of a response is load_policy.h's.  The checker the CPU test (the header
under g++) and the GPU tests (k_integrate_loads) are compared with, int64 for int64."""
import numpy as np

import obstacle_emulation as E

F32 = np.float32
WALLS = 6
MAX_OBSTACLES = 64
SOLIDS = WALLS + MAX_OBSTACLES
QUANTUM_LOG2 = -24
TERM_LIMIT = 2.0 ** 38


def term(mass, vb, va, quantum_log2):
    """load_term on rows: (q int64 (m, 3), ok (m,)); q is 0 where the response is skipped"""
    vb, va = (np.asarray(a, F32).reshape(-1, 3) for a in (vb, va))
    m = np.asarray(mass, F32).reshape(-1)
    with np.errstate(all="ignore"):
        d = (vb - va).astype(F32)
        j = (m[:, None] * d).astype(F32)
        s = j.astype(np.float64) * 2.0 ** (-int(quantum_log2))
        ok = (np.isfinite(s) & (np.abs(s) < TERM_LIMIT)).all(1)
        q = np.rint(np.where(ok[:, None], s, 0.0)).astype(np.int64)
    return q, ok


class Row:
    """one row of a recording: impulse (SOLIDS, 3), count, skipped (SOLIDS,), all int64"""

    def __init__(self, quantum_log2=QUANTUM_LOG2):
        self.quantum_log2 = int(quantum_log2)
        self.impulse = np.zeros((SOLIDS, 3), np.int64)
        self.count = np.zeros(SOLIDS, np.int64)
        self.skipped = np.zeros(SOLIDS, np.int64)

    def add(self, solid, hit, mass, vb, va):
        """the responses of the rows `hit` on column `solid`"""
        q, ok = term(mass, vb, va, self.quantum_log2)
        self.impulse[solid] += q[hit & ok].sum(0)
        self.count[solid] += int((hit & ok).sum())
        self.skipped[solid] += int((hit & ~ok).sum())

    def same(self, impulse, count, skipped):
        return (np.array_equal(self.impulse, impulse) and np.array_equal(self.count, count) and
                np.array_equal(self.skipped, skipped))


def walls_one_axis(axis, maxv, damping, P, V, Q, dt):
    """one axis of handle_boundaries on rows: (lo, hi, new V, new Q)"""
    dt, damping = F32(dt), F32(damping)
    with np.errstate(all="ignore"):
        lo = Q[:, axis] < 0
        hi = ~lo & (Q[:, axis] > maxv[axis])
        dist = np.where(lo, -P[:, axis] / V[:, axis], (maxv[axis] - P[:, axis]) / V[:, axis]).astype(F32)
        normal = np.zeros_like(V)
        normal[:, axis] = np.where(lo, F32(1), F32(-1))
        inter = P + (V * dist[:, None])
        dot = (V[:, 0] * normal[:, 0] + V[:, 1] * normal[:, 1]) + V[:, 2] * normal[:, 2]
        refl = V - ((normal * dot[:, None]) * F32(2))
        remaining = dt - dist
        q_new = inter + refl * (remaining * damping)[:, None]
    act = (lo | hi)[:, None]
    return lo, hi, np.where(act, refl, V).astype(F32), np.where(act, q_new, Q).astype(F32)


def walls(maxv, damping, P, V, Q, dt, mass=None, row=None):
    """handle_boundaries on rows (x, then y, then z), adding every response to `row`: new (V, Q)"""
    maxv = np.asarray(maxv, F32)
    P, V, Q = (np.asarray(a, F32).reshape(-1, 3) for a in (P, V, Q))
    for axis in range(3):
        lo, hi, V2, Q2 = walls_one_axis(axis, maxv, damping, P, V, Q, dt)
        if row is not None:
            row.add(2 * axis, lo, mass, V, V2)
            row.add(2 * axis + 1, hi, mass, V, V2)
        V, Q = V2, Q2
    return V, Q


def obstacles(obst, P, V, Q, dt, damping, mass=None, row=None):
    """obstacles_respond on rows, one obstacle at a time, adding every response to `row`: new (V, Q)"""
    P, V, Q = (np.asarray(a, F32).reshape(-1, 3) for a in (P, V, Q))
    for i, o in enumerate(obst):
        inside = E.inside(o, Q)
        V2, Q2 = E.respond_one(o, P, V, Q, dt, damping)
        if row is not None:
            row.add(WALLS + i, inside, mass, V, V2)
        V, Q = V2, Q2
    return V, Q


def respond(maxv, apply_walls, obst, P, V, Q, dt, damping, mass, quantum_log2=QUANTUM_LOG2):
    """What integrate does to (old position P, new velocity V, new position Q) after the drift and the
    kick - walls when apply_walls, then the obstacles - and the row it records: (V, Q, Row)"""
    row = Row(quantum_log2)
    P, V, Q = (np.asarray(a, F32).reshape(-1, 3) for a in (P, V, Q))
    if apply_walls:
        V, Q = walls(maxv, damping, P, V, Q, dt, mass, row)
    V, Q = obstacles(obst, P, V, Q, dt, damping, mass, row)
    return V, Q, row
