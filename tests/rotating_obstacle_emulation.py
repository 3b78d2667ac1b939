"""numpy restatement of the oriented and rotating obstacles (csrc/obstacle_policy.h: the contract's third
part), vectorised over particles and built on the static
and the moving restatements: obstacle_emulation.respond_one answers in the frame fixed to the solid,
moving_obstacle_emulation takes the turn of every entry that is not posed, load_emulation supplies the walls
and the rows.  Every operation is the header's, in fp32, in its order.  The checker the CPU test (the header
under g++) is compared with, bit for bit."""
import numpy as np

import load_emulation as L
import moving_obstacle_emulation as M
import obstacle_emulation as E

F32 = np.float32

TWO_OVER_PI = F32(0.636619772367581343)
PIO2_1 = F32(1.5703125)                    # pi/2 = PIO2_1 + PIO2_2 + PIO2_3: 8 bits, 11 bits, the rest
PIO2_2 = F32(4.837512969970703125e-4)
PIO2_3 = F32(7.54978995489188216e-8)
S1, S2, S3 = F32(-1.6666654611e-1), F32(8.3321608736e-3), F32(-1.9515295891e-4)
C1, C2, C3 = F32(4.166664568298827e-2), F32(-1.388731625493765e-3), F32(2.443315711809948e-5)
MAX_ANGLE = 8192.0


def sincos(theta):
    """obstacle_sincos: (cs, sn) float32 arrays of the shape of theta"""
    t = np.asarray(theta, F32)
    with np.errstate(all="ignore"):
        k = np.rint(t * TWO_OVER_PI).astype(F32)
        r = (t - k * PIO2_1).astype(F32)
        r = (r - k * PIO2_2).astype(F32)
        r = (r - k * PIO2_3).astype(F32)
        z = (r * r).astype(F32)
        s = (S3 * z + S2).astype(F32)
        s = (s * z + S1).astype(F32)
        s = ((s * z) * r + r).astype(F32)
        c = (C3 * z + C2).astype(F32)
        c = (c * z + C1).astype(F32)
        c = ((c * z) * z - F32(0.5) * z).astype(F32)
        c = (c + F32(1.0)).astype(F32)
        q = k.astype(np.int32) & 3
    cs = np.where(q == 0, c, np.where(q == 1, -s, np.where(q == 2, -c, s))).astype(F32)
    sn = np.where(q == 0, s, np.where(q == 1, c, np.where(q == 2, -s, -c))).astype(F32)
    return cs, sn


def rotation_fields(r):
    """(axis, pivot[3], angle, rate, start, stop) in float32 from an sph_hip_obstacle_rotation struct, an
    obstacles.Rotation, or None (unposed)"""
    if r is None:
        return 0, np.zeros(3, F32), F32(0), F32(0), F32(0), F32(np.inf)
    return int(r.axis), np.array(list(r.pivot), F32), F32(r.angle), F32(r.rate), F32(r.start), F32(r.stop)


def posed(r):
    _, _, angle, rate, _, _ = rotation_fields(r)
    return bool(angle != 0 or rate != 0)


def rotates(r):
    return bool(rotation_fields(r)[3] != 0)


def theta(r, tau):
    _, _, angle, rate, start, stop = rotation_fields(r)
    tau = F32(tau)
    s = F32((start if tau < start else stop if tau > stop else tau) - start)
    with np.errstate(all="ignore"):
        return F32(angle + F32(rate * s))


def pose(r, tau):
    """(angle, cs, sn) at motion clock tau, float32[3]"""
    if not posed(r):
        return np.array([0.0, 1.0, 0.0], F32)
    t = theta(r, tau)
    cs, sn = sincos(t)
    return np.array([t, cs, sn], F32)


def _uw(r):
    a, pivot = rotation_fields(r)[:2]
    return a, (a + 1) % 3, (a + 2) % 3, pivot


def to_body(r, cs, sn, X):
    a, u, w, pv = _uw(r)
    X = np.asarray(X, F32).reshape(-1, 3)
    cs, sn = F32(cs), F32(sn)
    with np.errstate(all="ignore"):
        du, dw = (X[:, u] - pv[u]).astype(F32), (X[:, w] - pv[w]).astype(F32)
        Y = X.copy()
        Y[:, u] = pv[u] + ((cs * du).astype(F32) + (sn * dw).astype(F32)).astype(F32)
        Y[:, w] = pv[w] + ((cs * dw).astype(F32) - (sn * du).astype(F32)).astype(F32)
    return Y


def to_world(r, cs, sn, Y):
    a, u, w, pv = _uw(r)
    Y = np.asarray(Y, F32).reshape(-1, 3)
    cs, sn = F32(cs), F32(sn)
    with np.errstate(all="ignore"):
        du, dw = (Y[:, u] - pv[u]).astype(F32), (Y[:, w] - pv[w]).astype(F32)
        X = Y.copy()
        X[:, u] = pv[u] + ((cs * du).astype(F32) - (sn * dw).astype(F32)).astype(F32)
        X[:, w] = pv[w] + ((sn * du).astype(F32) + (cs * dw).astype(F32)).astype(F32)
    return X


def vec_to_body(r, cs, sn, X):
    a, u, w, _ = _uw(r)
    X = np.asarray(X, F32).reshape(-1, 3)
    cs, sn = F32(cs), F32(sn)
    with np.errstate(all="ignore"):
        Y = X.copy()
        Y[:, u] = ((cs * X[:, u]).astype(F32) + (sn * X[:, w]).astype(F32)).astype(F32)
        Y[:, w] = ((cs * X[:, w]).astype(F32) - (sn * X[:, u]).astype(F32)).astype(F32)
    return Y


def vec_to_world(r, cs, sn, Y):
    a, u, w, _ = _uw(r)
    Y = np.asarray(Y, F32).reshape(-1, 3)
    cs, sn = F32(cs), F32(sn)
    with np.errstate(all="ignore"):
        X = Y.copy()
        X[:, u] = ((cs * Y[:, u]).astype(F32) - (sn * Y[:, w]).astype(F32)).astype(F32)
        X[:, w] = ((sn * Y[:, u]).astype(F32) + (cs * Y[:, w]).astype(F32)).astype(F32)
    return X


def respond_posed(o, r, cs0, sn0, cs1, sn1, still, P, V, Q, dt, damping):
    """a posed entry's turn with the pose given: new (V, Q, inside)"""
    P, V, Q = (np.asarray(a, F32).reshape(-1, 3) for a in (P, V, Q))
    q1 = to_body(r, cs1, sn1, Q)
    act = E.inside(o, q1)
    p0 = to_body(r, cs0, sn0, P)
    with np.errstate(all="ignore"):
        if still:
            w = vec_to_body(r, cs1, sn1, V)
            w2, q2 = E.respond_one(o, p0, w, q1, dt, damping)
            v2 = vec_to_world(r, cs1, sn1, w2)
        else:
            pc = to_world(r, cs1, sn1, p0)
            d = (pc - P).astype(F32)
            ue = (d / F32(dt)).astype(F32)
            wv = (V - ue).astype(F32)
            w = vec_to_body(r, cs1, sn1, wv)
            w2, q2 = E.respond_one(o, p0, w, q1, dt, damping)
            v2 = (vec_to_world(r, cs1, sn1, w2) + ue).astype(F32)
        x2 = to_world(r, cs1, sn1, q2)
    V2 = np.where(act[:, None], v2, V).astype(F32)
    Q2 = np.where(act[:, None], x2, Q).astype(F32)
    return V2, Q2, act


def respond_one(o, m, r, P, V, Q, dt, damping, tau0, tau1):
    """one entry's turn for every row: new (V, Q, inside).  An entry that is not posed takes the turn of
    its motion (moving_obstacle_emulation.respond_one)."""
    if not posed(r):
        return M.respond_one(o, m, P, V, Q, dt, damping, tau0, tau1)
    t0, t1 = theta(r, tau0), theta(r, tau1)
    cs0, sn0 = sincos(t0)
    cs1, sn1 = sincos(t1)
    return respond_posed(o, r, cs0, sn0, cs1, sn1, bool(t1 == t0), P, V, Q, dt, damping)


def turns(r, tau0, tau1):
    """whether a posed entry's angle differs between the two ends of the step"""
    return posed(r) and bool(theta(r, tau1) != theta(r, tau0))


def rotations_for(obst, rotations):
    rotations = list(rotations) if rotations else []
    return rotations if rotations else [None] * len(obst)


def respond(obst, motions, rotations, P, V, Q, dt, damping, tau0, tau1, mass=None, row=None):
    """every obstacle of the list in order (p fixed), adding every turn to `row`: new (V, Q)"""
    V = np.asarray(V, F32).reshape(-1, 3)
    Q = np.asarray(Q, F32).reshape(-1, 3)
    for i, (o, m, r) in enumerate(zip(obst, M.motions_for(obst, motions), rotations_for(obst, rotations))):
        V2, Q2, act = respond_one(o, m, r, P, V, Q, dt, damping, tau0, tau1)
        if row is not None:
            row.add(L.WALLS + i, act, mass, V, V2)
        V, Q = V2, Q2
    return V, Q


def integrate_respond(maxv, apply_walls, obst, motions, rotations, P, V, Q, dt, damping, tau0, tau1, mass,
                      quantum_log2=L.QUANTUM_LOG2):
    """what integrate does to (P, V, Q) after the drift and the kick - walls when apply_walls, then the
    obstacles - and the row it records: (V, Q, Row)"""
    row = L.Row(quantum_log2)
    P, V, Q = (np.asarray(a, F32).reshape(-1, 3) for a in (P, V, Q))
    if apply_walls:
        V, Q = L.walls(maxv, damping, P, V, Q, dt, mass, row)
    V, Q = respond(obst, motions, rotations, P, V, Q, dt, damping, tau0, tau1, mass, row)
    return V, Q, row


def clock_runs(motions, rotations):
    """the clock rule: some entry moves or rotates"""
    return any(M.moves(m) for m in motions or ()) or any(rotates(r) for r in rotations or ())
