"""numpy restatement of the velocity gradients (csrc/velgrad_policy.h; include/sph_hip.h: velocity gradients) on top of
the field sampler's restatement (sample_emulation: the canonical order, the density pass's pair term) and the pressure
readings' (pressure_emulation: members in canonical order, sums added one by one), the checker of
tests/test_gpu_velgrad.py and tests/test_velgrad_cpu.py.

    members  j with (dx*dx + dy*dy) + dz*dz < h2, (dx, dy, dz) = r_i - r_j, i excluded, in canonical order
    w_j      m_j * (kernel1 * (hscaled2 - d*d)^3), d = sqrt(d2) times sim_scale unless unit scale; off unit scale
             +0 where d > hscaled (sample_emulation.density_terms)
    r, u     r = (dx, dy, dz), times sim_scale first unless unit scale; u = v_i - v_j
    sums     from 0, per member q_a = w * r_a, p_a = w * u_a, then M_ab = M_ab + q_a * r_b (xx xy xz yy yz zz) and
             B_ab = B_ab + p_a * r_b (all nine)
    inverse  c00 = m11*m22 - m12*m12   c01 = m02*m12 - m01*m22   c02 = m01*m12 - m02*m11
             c11 = m00*m22 - m02*m02   c12 = m01*m02 - m00*m12   c22 = m00*m11 - m01*m01
             det = (m00*c00 + m01*c01) + m02*c02, t = ((m00 + m11) + m22) * (1/3 in fp32)
    valid    count >= 3 and det > 2^-10 * ((t*t)*t)
    G_ab     ((B_a0*c_0b + B_a1*c_1b) + B_a2*c_2b) / det = dv_a / dx_b per unit of SCALED length: v = A x gives
             A / sim_scale
    rows     (w_x, w_y, w_z, div) = (G_zy - G_yz, G_xz - G_zx, G_yx - G_xy, (G_xx + G_yy) + G_zz)
             s_ab = 0.5 * (G_ab + G_ba); ss = ((G_xx^2 + G_yy^2) + G_zz^2) + 2 * ((s_xy^2 + s_xz^2) + s_yz^2)
             ww = (w_x^2 + w_y^2) + w_z^2; oo = 0.5 * ww
             (strain, Q, |w|, valid) = (sqrt(2 * ss), 0.5 * (oo - ss), sqrt(ww), 1)
    guard    not valid, or one of the eight not finite: eight +0
No power-of-two rescaling of M is applied (velgrad_policy.h: Range).  numpy evaluates float32 arrays operation by
operation with IEEE rounding and never fuses, so the bits are the device's."""
import numpy as np

import pressure_emulation as PE
import sample_emulation as SE

F32 = np.float32
MIN_MEMBERS = 3
MIN_DET_RATIO = F32(2.0 ** -10)
THIRD = F32(1.0) / F32(3.0)
QUANTITIES = ("vorticity_x", "vorticity_y", "vorticity_z", "divergence", "strain_rate", "q", "vorticity_magnitude",
              "valid")
# the order of the fifteen sums: M's six, then B's nine (row a = velocity component, column b = direction)
M_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
B_PAIRS = tuple((a, b) for a in range(3) for b in range(3))


def pair_terms(p, d2, mass_j, r, u):
    """The fifteen addends of k members, a list of (k,) float32 arrays: d2 (k,), the neighbours' masses (k,), the
    separations r_i - r_j (k, 3) and the velocity differences v_i - v_j (k, 3)."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        w = SE.density_terms(p, np.asarray(d2, F32), np.asarray(mass_j, F32))
        r = np.asarray(r, F32).reshape(-1, 3)
        u = np.asarray(u, F32).reshape(-1, 3)
        if not SE.unit_scale(p):
            r = r * F32(p.sim_scale)
        q = (w[:, None] * r).astype(F32)
        pw = (w[:, None] * u).astype(F32)
        return [(q[:, a] * r[:, b]).astype(F32) for a, b in M_PAIRS] + [(pw[:, a] * r[:, b]).astype(F32) for a, b in B_PAIRS]


def solve(sums, count):
    """From the fifteen sums ((m,) each) and the member counts: (valid (m,), G (m, 3, 3), det (m,), t (m,))."""
    mxx, mxy, mxz, myy, myz, mzz = [np.asarray(s, F32) for s in sums[:6]]
    B = [np.asarray(s, F32) for s in sums[6:]]
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        c00 = myy * mzz - myz * myz
        c01 = mxz * myz - mxy * mzz
        c02 = mxy * myz - mxz * myy
        c11 = mxx * mzz - mxz * mxz
        c12 = mxy * mxz - mxx * myz
        c22 = mxx * myy - mxy * mxy
        det = (mxx * c00 + mxy * c01) + mxz * c02
        t = ((mxx + myy) + mzz) * THIRD
        valid = (np.asarray(count) >= MIN_MEMBERS) & (det > MIN_DET_RATIO * ((t * t) * t))
        C = ((c00, c01, c02), (c01, c11, c12), (c02, c12, c22))
        G = np.zeros((mxx.size, 3, 3), F32)
        for a in range(3):
            for b in range(3):
                G[:, a, b] = ((B[3 * a] * C[0][b] + B[3 * a + 1] * C[1][b]) + B[3 * a + 2] * C[2][b]) / det
    return valid, G, det, t


def finish(sums, count):
    """The eight values (m, 8) float32 of m particles from their sums and counts."""
    valid, G, _, _ = solve(sums, count)
    out = np.zeros((G.shape[0], 8), F32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        gxx, gxy, gxz = G[:, 0, 0], G[:, 0, 1], G[:, 0, 2]
        gyx, gyy, gyz = G[:, 1, 0], G[:, 1, 1], G[:, 1, 2]
        gzx, gzy, gzz = G[:, 2, 0], G[:, 2, 1], G[:, 2, 2]
        wx, wy, wz = gzy - gyz, gxz - gzx, gyx - gxy
        div = (gxx + gyy) + gzz
        sxy, sxz, syz = F32(0.5) * (gxy + gyx), F32(0.5) * (gxz + gzx), F32(0.5) * (gyz + gzy)
        ss = ((gxx * gxx + gyy * gyy) + gzz * gzz) + F32(2.0) * ((sxy * sxy + sxz * sxz) + syz * syz)
        ww = (wx * wx + wy * wy) + wz * wz
        oo = F32(0.5) * ww
        rows = np.stack([wx, wy, wz, div, np.sqrt(F32(2.0) * ss), F32(0.5) * (oo - ss), np.sqrt(ww),
                         np.ones_like(wx)], 1).astype(F32)
        ok = valid & (np.abs(rows) <= F32(3.402823466e38)).all(1)
    out[ok] = rows[ok]
    return out


def particle_sums(p, pi, vi, pj, vj, mj):
    """One particle at pi with velocity vi and the CANDIDATES pj (k, 3), vj (k, 3), mj (k,) in the order given - the
    members are those with d2 < h2: (the fifteen sums as (1,) arrays, the member count)."""
    pi = np.asarray(pi, F32).reshape(3)
    vi = np.asarray(vi, F32).reshape(3)
    pj = np.asarray(pj, F32).reshape(-1, 3)
    vj = np.asarray(vj, F32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        r = pi[None, :] - pj
        d2 = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2]
        member = d2 < F32(p.h2)
        u = vi[None, :] - vj
    terms = pair_terms(p, d2[member], np.asarray(mj, F32)[member], r[member], u[member])
    sums = [np.zeros(1, F32) for _ in terms]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for j in range(int(member.sum())):
            for s, t in zip(sums, terms):
                s[0] = s[0] + t[j]
    return sums, int(member.sum())


def particle(p, pi, vi, pj, vj, mj):
    """The eight values of one particle: what tests/test_velgrad_cpu.py's g++ shim computes with the header."""
    sums, count = particle_sums(p, pi, vi, pj, vj, mj)
    return finish(sums, np.array([count]))[0]


def state_sums(p, pos, vel, mass):
    """(the fifteen sums, the counts, the canonical order) of every particle of the state, rows in canonical order."""
    order = PE.canonical_order(p, pos)
    grid = SE.Grid(p, pos, vel, mass)
    probe, idx, d2 = PE.members(grid, grid.pos, exclude_self=True)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        r = grid.pos[probe] - grid.pos[idx]
        u = grid.vel[probe] - grid.vel[idx]
    terms = pair_terms(p, d2, grid.mass[idx], r, u)
    sums, count = PE.ordered_sums(probe, grid.mass.size, terms)
    return sums, count, order


def rows_sorted(p, pos, vel, mass):
    """The eight values (n, 8) by sorted slot (canonical order)."""
    if np.asarray(mass).size == 0:
        return np.zeros((0, 8), F32)
    sums, count, _ = state_sums(p, pos, vel, mass)
    return finish(sums, count)


def rows(p, pos, vel, mass):
    """sph_hip_get_velocity_gradients: the eight values (n, 8) in particle order."""
    n = np.asarray(mass).size
    out = np.zeros((n, 8), F32)
    if n:
        out[PE.canonical_order(p, pos)] = rows_sorted(p, pos, vel, mass)
    return out


def gradients(p, pos, vel, mass):
    """(valid (n,), G (n, 3, 3) float32, det / t^3 (n,) float64, counts (n,)) in particle order: the fit itself."""
    sums, count, order = state_sums(p, pos, vel, mass)
    valid, G, det, t = solve(sums, count)
    n = order.size
    v, g, ratio, c = np.zeros(n, bool), np.zeros((n, 3, 3), F32), np.zeros(n), np.zeros(n, np.int32)
    v[order], g[order], c[order] = valid, G, count
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio[order] = det.astype(np.float64) / t.astype(np.float64) ** 3
    return v, g, ratio, c


def gradients64(p, pos, vel, mass):
    """The same sums over the same fp32 inputs and the same fp32 weights, evaluated in float64 and solved with
    numpy.linalg: (G (n, 3, 3) float64, cond(M) (n,)) in particle order, NaN / inf where M is singular."""
    order = PE.canonical_order(p, pos)
    grid = SE.Grid(p, pos, vel, mass)
    n = grid.mass.size
    probe, idx, d2 = PE.members(grid, grid.pos, exclude_self=True)
    w = SE.density_terms(p, d2, grid.mass[idx]).astype(np.float64)
    r = (grid.pos[probe] - grid.pos[idx]).astype(np.float64)       # (the fp32 differences, as the kernel forms them)
    u = (grid.vel[probe] - grid.vel[idx]).astype(np.float64)
    if not SE.unit_scale(p):
        r = r * float(F32(p.sim_scale))
    M = np.zeros((n, 3, 3))
    B = np.zeros((n, 3, 3))
    for a in range(3):
        for b in range(3):
            M[:, a, b] = np.bincount(probe, weights=w * r[:, a] * r[:, b], minlength=n)
            B[:, a, b] = np.bincount(probe, weights=w * u[:, a] * r[:, b], minlength=n)
    G = np.full((n, 3, 3), np.nan)
    cond = np.full(n, np.inf)
    sv = np.linalg.svd(M, compute_uv=False)
    ok = sv[:, 2] > 0
    cond[ok] = sv[ok, 0] / sv[ok, 2]
    good = ok & (cond < 1e12)
    G[good] = B[good] @ np.linalg.inv(M[good])
    out_G, out_c = np.full((n, 3, 3), np.nan), np.full(n, np.inf)
    out_G[order], out_c[order] = G, cond
    return out_G, out_c


def sample(p, pos, vel, mass, rows8, probes, group):
    """sph_hip_sample_velocity_gradients_points: scalar_emulation's Shepard restatement with the rows rows8 (n, 8, in
    particle order) of `group` (0: columns 0..3, 1: columns 4..7) in the place of the channels."""
    import scalar_emulation as SC
    T = np.asarray(rows8, F32).reshape(-1, 8)[:, 4 * group:4 * group + 4]
    return SC.sample(p, pos, vel, mass, T, probes)
