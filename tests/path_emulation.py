"""numpy restatement of the motion paths (csrc/obstacle_policy.h, fourth part; include/sph_hip.h:
sph_hip_set_obstacle_paths), built on the existing restatements: moving_obstacle_emulation supplies the
clock, the motions and, through wedge_emulation, the moved response (obstacle_respond_moved with two
shifts) for every kind of solid; load_emulation the walls and the rows.  The path arithmetic - path time,
segment, shift, velocity - is restated here from the header's contract, every operation in fp32 in its
order.  The checker the CPU test (the header under g++) and the GPU tests (k_paths_eval,
k_integrate_obst_path, k_integrate_loads_path) are compared with, bit for bit."""
import numpy as np

import load_emulation as L
import moving_obstacle_emulation as M
import wedge_emulation as W

F32 = np.float32


def path_fields(path):
    """(times float32 (K,), displacements float32 (K, 3), start float32, cycle bool) of an
    obstacles.MotionPath"""
    return (np.asarray(path.times, F32).reshape(-1), np.asarray(path.displacements, F32).reshape(-1, 3),
            F32(path.start), bool(path.cycle))


def segment(path, tau):
    """(j, u, clamped): the segment in force at tau, the path time, whether it was clamped"""
    t, _, start, cycle = path_fields(path)
    T = t[-1]
    with np.errstate(all="ignore"):
        u = F32(F32(tau) - start)
        clamped = bool(u < 0)
        if u < 0:
            u = F32(0)
        if not cycle:
            if u > T:
                u = T
                clamped = True
        else:
            if u >= T:
                turns = F32(np.floor(F32(u / T)))
                u = F32(u - F32(turns * T))
            if u < 0:
                u = F32(0)
            if u >= T:
                u = F32(0)
    j = int(np.flatnonzero(t[:-1] <= u).max())
    return j, F32(u), clamped


def displacement(path, tau):
    """D(tau), float32[3]"""
    t, d, _, _ = path_fields(path)
    j, u, _ = segment(path, tau)
    with np.errstate(all="ignore"):
        w = F32(F32(u - t[j]) / F32(t[j + 1] - t[j]))
        return (d[j] + (w * (d[j + 1] - d[j]).astype(F32)).astype(F32)).astype(F32)


def velocity(path, tau):
    """the velocity of the segment in force at tau, 0 while the path time is clamped: float32[3]"""
    t, d, _, _ = path_fields(path)
    j, _, clamped = segment(path, tau)
    if clamped:
        return np.zeros(3, F32)
    with np.errstate(all="ignore"):
        return ((d[j + 1] - d[j]).astype(F32) / F32(t[j + 1] - t[j])).astype(F32)


def paths_for(obst, paths):
    paths = list(paths or [])
    return paths if paths else [None] * len(obst)


def shifts(paths, tau0, tau1):
    """what k_paths_eval writes for a step: float32 (n, 2, 3) - D0 and D1, zeros for an entry without a
    path - and has_path (n,)"""
    out = np.zeros((len(paths), 2, 3), F32)
    has = np.zeros(len(paths), bool)
    for i, p in enumerate(paths):
        if p is not None:
            out[i, 0], out[i, 1], has[i] = displacement(p, tau0), displacement(p, tau1), True
    return out, has


def obstacle_at(o, path, m, tau):
    """the sph_hip_obstacle struct at motion clock tau: always shifted along a path, otherwise by its motion"""
    if path is None:
        return W.obstacle_at(o, m, tau)
    return W.shifted(o, displacement(path, tau))


def respond_one(o, path, m, P, V, Q, dt, damping, tau0, tau1):
    """one entry's turn for every row: new (V, Q, inside)"""
    if path is None:
        return W.turn(o, m, P, V, Q, dt, damping, tau0, tau1)[:3]
    return W.moved_one(o, displacement(path, tau0), displacement(path, tau1), P, V, Q, dt, damping)[:3]


def respond(obst, paths, motions, P, V, Q, dt, damping, tau0, tau1, mass=None, row=None, counts=None):
    """every obstacle of the list in order (p fixed), adding every turn to `row`: new (V, Q).  counts: a
    two-entry list that receives the rows a path entry changed in a step in which it moved / stood."""
    V = np.asarray(V, F32).reshape(-1, 3)
    Q = np.asarray(Q, F32).reshape(-1, 3)
    for i, (o, p, m) in enumerate(zip(obst, paths_for(obst, paths), M.motions_for(obst, motions or []))):
        V2, Q2, act = respond_one(o, p, m, P, V, Q, dt, damping, tau0, tau1)
        if row is not None:
            row.add(L.WALLS + i, act, mass, V, V2)
        if counts is not None and p is not None:
            changed = int(((V2 != V) | (Q2 != Q)).any(1).sum())
            counts[0 if (displacement(p, tau1) != displacement(p, tau0)).any() else 1] += changed
        V, Q = V2, Q2
    return V, Q


def integrate_respond(maxv, apply_walls, obst, paths, motions, P, V, Q, dt, damping, tau0, tau1, mass,
                      quantum_log2=L.QUANTUM_LOG2, counts=None):
    """what integrate does to (P, V, Q) after the drift and the kick - walls when apply_walls, then the
    obstacles - and the row it records: (V, Q, Row)"""
    row = L.Row(quantum_log2)
    P, V, Q = (np.asarray(a, F32).reshape(-1, 3) for a in (P, V, Q))
    if apply_walls:
        V, Q = L.walls(maxv, damping, P, V, Q, dt, mass, row)
    V, Q = respond(obst, paths, motions, P, V, Q, dt, damping, tau0, tau1, mass, row, counts)
    return V, Q, row


def oracle_step(oracle, op, obst, paths, motions, pos, vel, mass, tau0, tau1, quantum_log2=L.QUANTUM_LOG2,
                counts=None):
    """one FULL step on the CPU: the oracle's cells, density, acceleration and integrate (walls off), then
    integrate_respond.  Returns (pos, vel, Row)."""
    import ctypes as C
    free = type(op)()
    C.memmove(C.byref(free), C.byref(op), C.sizeof(op))
    walls = int(op.apply_walls)
    free.apply_walls = 0
    _, cs, ci = oracle.full_cells(op, pos)
    rho, _ = oracle.full_density(op, pos, mass, cs, ci)
    acc = oracle.full_accel(op, pos, vel, mass, rho, cs, ci)
    P = pos.copy()
    q, v = pos.copy(), vel.copy()
    oracle.integrate(free, q, v, acc, mass)
    maxv = F32([op.max_x, op.max_y, op.max_z])
    V, Q, row = integrate_respond(maxv, walls, obst, paths, motions, P, v, q, F32(op.time_step), F32(op.damping),
                                  tau0, tau1, mass, quantum_log2, counts)
    return np.ascontiguousarray(Q.reshape(-1)), np.ascontiguousarray(V.reshape(-1)), row
