"""numpy restatement of the static-obstacle response (csrc/obstacle_policy.h, include/sph_hip.h:
static obstacles), vectorised over particles: every operation is the header's, in fp32, in its order,
and branches are evaluated on every row and selected.  The checker the CPU test (the header under g++)
and the GPU tests (k_integrate_obst and k_slab_pack_early_obst) are compared with, bit for bit."""
import numpy as np

F32 = np.float32
SPHERE, BOX, CYLINDER = 0, 1, 2
INF = F32(np.inf)


def fields(o):
    """(kind, axis, center[3], radius, lo[3], hi[3]) as float32 from an sph_hip_obstacle struct or an
    obstacles.Sphere / Box / Cylinder"""
    if not hasattr(o, "center") or not hasattr(o, "_fields_"):
        o = o.as_struct()
    return (int(o.kind), int(o.axis), np.array(list(o.center), F32), F32(o.radius),
            np.array(list(o.lo), F32), np.array(list(o.hi), F32))


def inside(o, x):
    kind, axis, c, r, lo, hi = fields(o)
    if kind == SPHERE:
        d = x - c
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] < r * r
    if kind == BOX:
        return ((lo[0] < x[:, 0]) & (x[:, 0] < hi[0]) & (lo[1] < x[:, 1]) & (x[:, 1] < hi[1]) &
                (lo[2] < x[:, 2]) & (x[:, 2] < hi[2]))
    a, u, w = axis, (axis + 1) % 3, (axis + 2) % 3
    du, dw = x[:, u] - c[u], x[:, w] - c[w]
    return (lo[a] < x[:, a]) & (x[:, a] < hi[a]) & (du * du + dw * dw < r * r)


def _slab(p, v, lo, hi):
    """obstacle_slab on columns: (ok, t0, t1)"""
    moving = v != 0
    t0 = np.where(moving, (np.where(v > 0, lo, hi) - p) / v, -INF).astype(F32)
    t1 = np.where(moving, (np.where(v > 0, hi, lo) - p) / v, INF).astype(F32)
    ok = moving | ((lo < p) & (p < hi))
    return ok, t0, t1


def respond_one(o, P, V, Q, dt, damping):
    """obstacle_respond for every row; returns new (V, Q) (float32 (m, 3) arrays, inputs unchanged)"""
    kind, axis, c, r, lo, hi = fields(o)
    P, V, Q = (np.asarray(a, F32).reshape(-1, 3) for a in (P, V, Q))
    dt, damping = F32(dt), F32(damping)
    m = P.shape[0]
    V, Q = V.copy(), Q.copy()
    with np.errstate(all="ignore"):
        act = inside(o, Q)
        hit = act & ~inside(o, P) & ((V[:, 0] != 0) | (V[:, 1] != 0) | (V[:, 2] != 0))
        kind_n = np.full(m, -1, np.int64)
        if kind == BOX:
            t = np.full(m, -INF, F32)
            t_exit = np.full(m, INF, F32)
            for a in range(3):
                ok, t0, t1 = _slab(P[:, a], V[:, a], lo[a], hi[a])
                hit &= ok
                take = (V[:, a] != 0) & (t0 > t)
                t = np.where(take, t0, t)
                kind_n = np.where(take, a, kind_n)
                t_exit = np.where(t1 < t_exit, t1, t_exit)
        elif kind == SPHERE:
            d0 = P - c
            A = (V[:, 0] * V[:, 0] + V[:, 1] * V[:, 1]) + V[:, 2] * V[:, 2]
            B = (d0[:, 0] * V[:, 0] + d0[:, 1] * V[:, 1]) + d0[:, 2] * V[:, 2]
            C = ((d0[:, 0] * d0[:, 0] + d0[:, 1] * d0[:, 1]) + d0[:, 2] * d0[:, 2]) - r * r
            D = B * B - A * C
            s = np.sqrt(D)
            t = (-B - s) / A
            t_exit = (-B + s) / A
            hit &= D > 0
            kind_n[:] = 3
        else:
            a, u, w = axis, (axis + 1) % 3, (axis + 2) % 3
            ok, tc0, tc1 = _slab(P[:, a], V[:, a], lo[a], hi[a])
            hit &= ok
            d0u, d0w = P[:, u] - c[u], P[:, w] - c[w]
            A = V[:, u] * V[:, u] + V[:, w] * V[:, w]
            C = (d0u * d0u + d0w * d0w) - r * r
            B = d0u * V[:, u] + d0w * V[:, w]
            D = B * B - A * C
            s = np.sqrt(D)
            pos_a = A > 0
            tr0 = np.where(pos_a, (-B - s) / A, -INF).astype(F32)
            tr1 = np.where(pos_a, (-B + s) / A, INF).astype(F32)
            hit &= np.where(pos_a, D > 0, d0u * d0u + d0w * d0w < r * r)
            cap = tc0 >= tr0
            t = np.where(cap, tc0, tr0).astype(F32)
            kind_n = np.where(cap, a, 4)
            t_exit = np.where(tc1 < tr1, tc1, tr1).astype(F32)
        hit &= (t >= 0) & (t < t_exit)

        # valid entry
        inter = P + V * t[:, None]
        n = np.zeros((m, 3), F32)
        for b in range(3):
            n[:, b] = np.where(kind_n == b, np.where(V[:, b] > 0, F32(-1), F32(1)), n[:, b])
        if kind == SPHERE:
            n = np.where((kind_n == 3)[:, None], (inter - c) / r, n).astype(F32)
        if kind == CYLINDER:
            side = kind_n == 4
            n[:, u] = np.where(side, (inter[:, u] - c[u]) / r, n[:, u])
            n[:, w] = np.where(side, (inter[:, w] - c[w]) / r, n[:, w])
        dot = (V[:, 0] * n[:, 0] + V[:, 1] * n[:, 1]) + V[:, 2] * n[:, 2]
        refl = V - (n * dot[:, None]) * F32(2)
        rem = dt - t
        remaining = np.where(rem > 0, rem, F32(0)).astype(F32)
        q_hit = inter + refl * (remaining * damping)[:, None]

        # fallback
        nf = np.zeros((m, 3), F32)
        qf = Q.copy()
        if kind == SPHERE:
            d = Q - c
            ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            pos_l = ln > 0
            nf = np.where(pos_l[:, None], d / ln[:, None], np.array([1, 0, 0], F32)).astype(F32)
            qf = c + nf * r
        elif kind == BOX:
            best = np.full(m, INF, F32)
            face = np.zeros(m, np.int64)
            for a in range(3):
                dlo, dhi = Q[:, a] - lo[a], hi[a] - Q[:, a]
                face = np.where(dlo < best, 2 * a, face)
                best = np.where(dlo < best, dlo, best)
                face = np.where(dhi < best, 2 * a + 1, face)
                best = np.where(dhi < best, dhi, best)
            for a in range(3):
                qf[:, a] = np.where(face == 2 * a, lo[a], np.where(face == 2 * a + 1, hi[a], qf[:, a]))
                nf[:, a] = np.where(face == 2 * a, F32(-1), np.where(face == 2 * a + 1, F32(1), F32(0)))
        else:
            du, dw = Q[:, u] - c[u], Q[:, w] - c[w]
            ln = np.sqrt(du * du + dw * dw)
            dlo, dhi, dside = Q[:, a] - lo[a], hi[a] - Q[:, a], r - ln
            f_lo = (dlo <= dhi) & (dlo <= dside)
            f_hi = ~f_lo & (dhi <= dside)
            f_side = ~f_lo & ~f_hi
            pos_l = ln > 0
            nu = np.where(pos_l, du / ln, F32(1)).astype(F32)
            nw = np.where(pos_l, dw / ln, F32(0)).astype(F32)
            qf[:, a] = np.where(f_lo, lo[a], np.where(f_hi, hi[a], Q[:, a]))
            nf[:, a] = np.where(f_lo, F32(-1), np.where(f_hi, F32(1), F32(0)))
            nf[:, u] = np.where(f_side, nu, F32(0))
            nf[:, w] = np.where(f_side, nw, F32(0))
            qf[:, u] = np.where(f_side, c[u] + nu * r, Q[:, u])
            qf[:, w] = np.where(f_side, c[w] + nw * r, Q[:, w])
        dotf = (V[:, 0] * nf[:, 0] + V[:, 1] * nf[:, 1]) + V[:, 2] * nf[:, 2]
        mm = np.where(dotf < 0, dotf, F32(0)).astype(F32)
        v_fb = V - nf * (mm * F32(2))[:, None]

        hit2 = hit[:, None]
        fb2 = (act & ~hit)[:, None]
        V_out = np.where(hit2, refl, np.where(fb2, v_fb, V)).astype(F32)
        Q_out = np.where(hit2, q_hit, np.where(fb2, qf, Q)).astype(F32)
    return V_out, Q_out


def respond(obstacles, P, V, Q, dt, damping):
    """every obstacle of the list in order (p fixed): new (V, Q), float32 (m, 3)"""
    V = np.asarray(V, F32).reshape(-1, 3)
    Q = np.asarray(Q, F32).reshape(-1, 3)
    for o in obstacles:
        V, Q = respond_one(o, P, V, Q, dt, damping)
    return V, Q


def energy_terms(vel, mass):
    """the per-particle KE terms of integrate on the final velocity, summed in f64 (as check_energy)"""
    v = np.asarray(vel, F32).reshape(-1, 3)
    dot = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    term = (F32(0.5) * np.asarray(mass, F32)) * dot
    return float(term[dot > 0].astype(np.float64).sum())
