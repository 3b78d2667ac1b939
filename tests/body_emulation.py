"""numpy restatement of the free bodies (csrc/body_policy.h; include/sph_hip.h: sph_hip_set_bodies), built on
moving_obstacle_emulation (the response in the frame that moves with the solid) and load_emulation (the
walls and the rows).  Every operation is the header's, in fp32, in its order.  The checker the CPU test (the
header under g++) and the GPU tests (k_bodies_advance, k_integrate_bodies) are compared with, bit for bit."""
import numpy as np

import load_emulation as L
import moving_obstacle_emulation as M
import obstacle_emulation as E

F32 = np.float32


def body_fields(b):
    """(mass, velocity[3], accel[3], free[3] bool, travel_lo[3], travel_hi[3]) from an sph_hip_body struct, an
    obstacles.Body, or None (not a body: mass 0)"""
    if b is None:
        z = np.zeros(3, F32)
        return F32(0), z, z, np.zeros(3, bool), z, z
    if not hasattr(b, "_fields_"):
        b = b.as_struct()
    free = np.array([bool(b.free_axes >> c & 1) for c in range(3)])
    return (F32(b.mass), np.array(list(b.velocity), F32), np.array(list(b.accel), F32), free,
            np.array(list(b.travel_lo), F32), np.array(list(b.travel_hi), F32))


def is_body(b):
    return bool(body_fields(b)[0] != 0)


def advance_arrays(mass, accel, free, lo, hi, D, V, q, e, dt):
    """the per-component part of body_advance on rows: mass, e, dt (m,), the others (m, 3); q int64 the
    impulse in quanta (zeros for a null row).  Returns new (D, V) float32 (m, 3); a masked component is
    returned untouched."""
    mass, dt = np.asarray(mass, F32).reshape(-1, 1), np.asarray(dt, F32).reshape(-1, 1)
    accel, lo, hi, D, V = (np.asarray(a, F32).reshape(-1, 3) for a in (accel, lo, hi, D, V))
    free = np.asarray(free, bool).reshape(-1, 3)
    e = np.asarray(e, np.int32).reshape(-1, 1)
    with np.errstate(all="ignore"):
        J = np.ldexp(np.asarray(q, np.int64).reshape(-1, 3).astype(np.float64), e).astype(F32)
        V2 = (V + (J / mass).astype(F32)).astype(F32)
        V2 = (V2 + (accel * dt).astype(F32)).astype(F32)
        D2 = (D + (V2 * dt).astype(F32)).astype(F32)
        below = D2 < lo
        D2 = np.where(below, lo, D2)
        V2 = np.where(below, F32(0), V2)
        above = D2 > hi
        D2 = np.where(above, hi, D2)
        V2 = np.where(above, F32(0), V2)
    return np.where(free, D2, D).astype(F32), np.where(free, V2, V).astype(F32)


class State:
    """the device state of every obstacle's body: D, Dprev, V float32 (n, 3); skipped, steps int64 (n,)"""

    def __init__(self, bodies):
        n = len(bodies)
        self.D, self.Dprev, self.V = (np.zeros((n, 3), F32) for _ in range(3))
        self.skipped, self.steps = np.zeros(n, np.int64), np.zeros(n, np.int64)
        for i, b in enumerate(bodies):
            _, vel, _, free, _, _ = body_fields(b)
            if is_body(b):
                self.V[i] = np.where(free, vel, F32(0))

    def copy(self):
        other = State([])
        other.D, other.Dprev, other.V = self.D.copy(), self.Dprev.copy(), self.V.copy()
        other.skipped, other.steps = self.skipped.copy(), self.steps.copy()
        return other


def advance(bodies, st, row, quantum_log2, dt):
    """body_advance for every obstacle: `row` is the L.Row the previous integrate filled, or None.
    Returns the new State."""
    out = st.copy()
    for i, b in enumerate(bodies):
        if not is_body(b):
            continue
        mass, _, accel, free, lo, hi = body_fields(b)
        q = row.impulse[L.WALLS + i] if row is not None else np.zeros(3, np.int64)
        out.Dprev[i] = st.D[i]
        D, V = advance_arrays([mass], accel, free, lo, hi, st.D[i], st.V[i], q, [quantum_log2], [dt])
        out.D[i], out.V[i] = D[0], V[0]
        if row is not None:
            out.skipped[i] += row.skipped[L.WALLS + i]
        out.steps[i] += 1
    return out


def moved_one(o, D0, D1, P, V, Q, dt, damping):
    """obstacle_respond_moved(obstacle_shifted(o, D1), D0, D1, ...) for every row: new (V, Q, inside)"""
    P, V, Q = (np.asarray(a, F32).reshape(-1, 3) for a in (P, V, Q))
    D0, D1 = np.asarray(D0, F32), np.asarray(D1, F32)
    o1 = M.shifted(o, D1)
    act = E.inside(o1, Q)
    d = (D1 - D0).astype(F32)
    if not (d != 0).any():
        V2, Q2 = E.respond_one(o1, P, V, Q, dt, damping)
        return V2, Q2, act
    with np.errstate(all="ignore"):
        ue = (d / F32(dt)).astype(F32)
        pr = (P + d).astype(F32)
        w = (V - ue).astype(F32)
        w2, Q2 = E.respond_one(o1, pr, w, Q, dt, damping)
        V2 = np.where(act[:, None], w2 + ue, V).astype(F32)
    return V2, Q2, act


def respond(obst, motions, bodies, st, P, V, Q, dt, damping, tau0, tau1, mass=None, row=None, changed=None):
    """body_obstacles_respond on rows: every obstacle in order - the body turn, the turn of its motion, or the
    static turn - adding every turn to `row`; changed[i] (a list of ints) grows by the rows turn i changed.
    Returns new (V, Q)."""
    V = np.asarray(V, F32).reshape(-1, 3)
    Q = np.asarray(Q, F32).reshape(-1, 3)
    for i, (o, m, b) in enumerate(zip(obst, M.motions_for(obst, motions), bodies)):
        if is_body(b):
            V2, Q2, act = moved_one(o, st.Dprev[i], st.D[i], P, V, Q, dt, damping)
        else:
            V2, Q2, act = M.respond_one(o, m, P, V, Q, dt, damping, tau0, tau1)
        if row is not None:
            row.add(L.WALLS + i, act, mass, V, V2)
        if changed is not None:
            changed[i] += int(((V2 != V) | (Q2 != Q)).any(1).sum())
        V, Q = V2, Q2
    return V, Q


def integrate_respond(maxv, apply_walls, obst, motions, bodies, st, P, V, Q, dt, damping, tau0, tau1, mass,
                      quantum_log2=L.QUANTUM_LOG2, changed=None):
    """What k_integrate_bodies does to (P, V, Q) after the drift and the kick - walls when apply_walls, then
    the obstacles with the bodies as `st` (already advanced for this step) places them - and the row it
    records: (V, Q, Row)"""
    row = L.Row(quantum_log2)
    P, V, Q = (np.asarray(a, F32).reshape(-1, 3) for a in (P, V, Q))
    if apply_walls:
        V, Q = L.walls(maxv, damping, P, V, Q, dt, mass, row)
    V, Q = respond(obst, motions, bodies, st, P, V, Q, dt, damping, tau0, tau1, mass, row, changed)
    return V, Q, row


def oracle_step(oracle, op, obst, motions, bodies, st, prev_row, pos, vel, mass, tau0, tau1,
                quantum_log2=L.QUANTUM_LOG2, changed=None):
    """One FULL step on the CPU: the oracle's sums and integrate (walls off: `op` is a copy the caller keeps),
    the advance from prev_row, and the restated response.  pos, vel: float32 (3n,), replaced in the returned
    tuple (pos, vel, State, Row)."""
    free = type(op)()
    import ctypes as C
    C.memmove(C.byref(free), C.byref(op), C.sizeof(op))
    walls = int(op.apply_walls)
    free.apply_walls = 0
    _, cs, ci = oracle.full_cells(op, pos)
    rho, _ = oracle.full_density(op, pos, mass, cs, ci)
    acc = oracle.full_accel(op, pos, vel, mass, rho, cs, ci)
    P = pos.copy()
    q, v = pos.copy(), vel.copy()
    oracle.integrate(free, q, v, acc, mass)
    dt, damping = F32(op.time_step), F32(op.damping)
    st = advance(bodies, st, prev_row, quantum_log2, dt)
    maxv = F32([op.max_x, op.max_y, op.max_z])
    V, Q, row = integrate_respond(maxv, walls, obst, motions, bodies, st, P, v, q, dt, damping, tau0, tau1, mass,
                                  quantum_log2, changed)
    return np.ascontiguousarray(Q.reshape(-1)), np.ascontiguousarray(V.reshape(-1)), st, row
