"""numpy restatement of the step monitor (csrc/monitor_policy.h; include/sph_hip.h: step monitor), operation for
operation, the checker of tests/test_monitor_cpu.py and tests/test_gpu_monitor.py.

    bad       x, v, a (three components each) or rho not finite (|v| <= FLT_MAX is the test), or rho < 0: counted, the
              id offered to bad_id_min, left out of everything else
    ranges    v2 = (vx*vx + vy*vy) + vz*vz, a2 likewise, rho, ncount; lone counts ncount == 0
    key       bits | 0x80000000 where the sign bit is clear, ~bits where it is set; a maximum over nothing is key 0, a
              minimum over nothing key 0xffffffff, both decode to +0.0f
    sums      m*vx, m*vy, m*vz, (0.5f*m)*v2, m in fp32, widened to float64, times 2^-quantum_log2; all five finite and
              below 2^38 in magnitude: rint (ties to even) into int64 sums, else skipped += 1
    scalars   per channel the finite values feed min and max by the key; scalar_bad counts rows with a value that is not
    S_p       0.0f, then S_p = S_p + V_j * (kernel3 * (hscaled - d)) over p's members in canonical order with V_j != 0
              (scalar_emulation.weight and distance: the scalar pass's own)
numpy evaluates float32 arrays operation by operation with IEEE rounding and never fuses, so the bits are the
device's.  An accumulator is a dict(sum int64[5], add int64[5], mx uint32[8], mn uint32[6]) - MonitorAcc's slots."""
import numpy as np

import pressure_emulation as PE
import sample_emulation as SE
import scalar_emulation as SC

F32 = np.float32
U32 = np.uint32
FLT_MAX = F32(3.402823466e38)
TERM_LIMIT = 274877906944.0       # 2^38
NO_ID = 0xFFFFFFFF
KEY_NO_MAX, KEY_NO_MIN = 0, 0xFFFFFFFF
SUMS, ADDS, MAXS, MINS = 5, 5, 8, 6
ADD_LIVE, ADD_BAD, ADD_SKIPPED, ADD_LONE, ADD_SCALAR_BAD = range(5)
MAX_NCOUNT, MAX_V2, MAX_A2, MAX_RHO, MAX_SCALAR = 0, 1, 2, 3, 4
MIN_BAD_ID, MIN_RHO, MIN_SCALAR = 0, 1, 2
SCALARS_VALID, DIFFUSION_VALID = 1, 2

# sph_hip_monitor_row
ROW = np.dtype([("momentum", "<i8", (3,)), ("kinetic", "<i8"), ("mass", "<i8"),
                ("live", "<i4"), ("bad", "<i4"), ("skipped", "<i4"), ("lone", "<i4"), ("ncount_max", "<i4"),
                ("scalar_bad", "<i4"), ("pair_bad", "<i4"), ("bad_id_min", "<u4"),
                ("v2_max", "<f4"), ("a2_max", "<f4"), ("rho_max", "<f4"), ("rho_min", "<f4"), ("s_max", "<f4"),
                ("scalar_min", "<f4", (4,)), ("scalar_max", "<f4", (4,)), ("flags", "<u4")])


def bits(v):
    return np.ascontiguousarray(v, F32).view(U32)


def key(v):
    b = bits(v)
    return np.where(b & U32(0x80000000), ~b, b | U32(0x80000000)).astype(U32)


def unkey(k):
    k = np.asarray(k, U32)
    return np.where(k & U32(0x80000000), k & U32(0x7FFFFFFF), ~k).astype(U32).view(F32)


def max_value(k):
    return F32(0.0) if int(k) == KEY_NO_MAX else unkey(np.array([k], U32))[0]


def min_value(k):
    return F32(0.0) if int(k) == KEY_NO_MIN else unkey(np.array([k], U32))[0]


def finite(v):
    with np.errstate(invalid="ignore"):
        return np.abs(np.asarray(v, F32)) <= FLT_MAX


def empty():
    return dict(sum=np.zeros(SUMS, np.int64), add=np.zeros(ADDS, np.int64), mx=np.full(MAXS, KEY_NO_MAX, U32),
                mn=np.full(MINS, KEY_NO_MIN, U32))


def merge(a, b):
    return dict(sum=a["sum"] + b["sum"], add=a["add"] + b["add"], mx=np.maximum(a["mx"], b["mx"]),
                mn=np.minimum(a["mn"], b["mn"]))


def square(v):
    v = np.asarray(v, F32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).astype(F32)


def is_bad(pos, vel, acc, rho):
    pos, vel, acc = (np.asarray(a, F32).reshape(-1, 3) for a in (pos, vel, acc))
    rho = np.asarray(rho, F32)
    ok = finite(pos).all(1) & finite(vel).all(1) & finite(acc).all(1) & finite(rho)
    with np.errstate(invalid="ignore"):
        return ~ok | (rho < 0)


def terms(mass, vel, v2, quantum_log2):
    """(quanta int64 (k, 5), ok (k,)) of k particles."""
    m = np.asarray(mass, F32)
    v = np.asarray(vel, F32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        hm = F32(0.5) * m
        t = np.stack([m * v[:, 0], m * v[:, 1], m * v[:, 2], hm * np.asarray(v2, F32), m], 1).astype(F32)
        s = t.astype(np.float64) * np.ldexp(1.0, -int(quantum_log2))
        ok = (np.isfinite(s) & (np.abs(s) < TERM_LIMIT)).all(1)
    q = np.zeros(s.shape, np.int64)
    q[ok] = np.rint(s[ok]).astype(np.int64)
    return q, ok


def particles(pos, vel, mass, ids, acc, rho, ncount, quantum_log2, T=None):
    """The accumulator of a set of live slots, in any order: T (rows by id, or None: the context carries none)."""
    pos, vel, acc = (np.asarray(a, F32).reshape(-1, 3) for a in (pos, vel, acc))
    mass, rho = np.asarray(mass, F32), np.asarray(rho, F32)
    ids, ncount = np.asarray(ids, np.int64), np.asarray(ncount, np.int64)
    a = empty()
    a["add"][ADD_LIVE] = mass.size
    bad = is_bad(pos, vel, acc, rho)
    a["add"][ADD_BAD] = int(bad.sum())
    if bad.any():
        a["mn"][MIN_BAD_ID] = U32(ids[bad].min())
    g = ~bad
    if g.any():
        v2, a2 = square(vel[g]), square(acc[g])
        a["mx"][MAX_V2] = key(v2).max()
        a["mx"][MAX_A2] = key(a2).max()
        rk = key(rho[g])
        a["mx"][MAX_RHO], a["mn"][MIN_RHO] = rk.max(), rk.min()
        a["mx"][MAX_NCOUNT] = U32(max(int(ncount[g].max()), 0))
        a["add"][ADD_LONE] = int((ncount[g] == 0).sum())
        q, ok = terms(mass[g], vel[g], v2, quantum_log2)
        a["sum"] = q[ok].sum(0).astype(np.int64)
        a["add"][ADD_SKIPPED] = int((~ok).sum())
        if T is not None:
            T = np.asarray(T, F32).reshape(-1, 4)
            inside = ids[g] < T.shape[0]
            rows = T[ids[g][inside]]
            f = finite(rows)
            for c in range(4):
                if f[:, c].any():
                    k = key(rows[f[:, c], c])
                    a["mx"][MAX_SCALAR + c], a["mn"][MIN_SCALAR + c] = k.max(), k.min()
            a["add"][ADD_SCALAR_BAD] = int((~f.all(1)).sum())
    return a


def pair_sums(p, pos, vel, mass, rho):
    """S_p of every particle of the state S_k (pos, vel, mass) with the step's densities rho, in particle order."""
    n = np.asarray(mass).size
    if n == 0:
        return np.zeros(0, F32)
    c = SC.consts_of(p)
    order = PE.canonical_order(p, pos)
    grid = SE.Grid(p, pos, vel, mass)
    Vs = SC.volume(grid.mass, np.asarray(rho, F32)[order])
    probe, idx, d2 = PE.members(grid, grid.pos, exclude_self=True)
    w = SC.weight(c, Vs[idx], SC.distance(c, d2))
    on = Vs[idx] != 0
    sums, _ = PE.ordered_sums(probe[on], n, [w[on]])
    out = np.zeros(n, F32)
    out[order] = sums[0]
    return out


def pair_acc(S):
    """(key of the largest finite S_p, the number that are not finite)"""
    S = np.asarray(S, F32)
    f = finite(S)
    return (int(key(S[f]).max()) if f.any() else KEY_NO_MAX), int((~f).sum())


def row_of(a, have_scalars=False, pairs=None):
    """The row of a folded accumulator; pairs: pair_acc's result, or None where the pair pass did not run."""
    r = np.zeros((), ROW)
    r["momentum"] = a["sum"][:3]
    r["kinetic"], r["mass"] = a["sum"][3], a["sum"][4]
    r["live"], r["bad"], r["skipped"], r["lone"] = (a["add"][i] for i in (ADD_LIVE, ADD_BAD, ADD_SKIPPED, ADD_LONE))
    r["ncount_max"] = int(a["mx"][MAX_NCOUNT])
    r["bad_id_min"] = a["mn"][MIN_BAD_ID]
    r["v2_max"], r["a2_max"] = max_value(a["mx"][MAX_V2]), max_value(a["mx"][MAX_A2])
    r["rho_max"], r["rho_min"] = max_value(a["mx"][MAX_RHO]), min_value(a["mn"][MIN_RHO])
    if have_scalars:
        r["scalar_bad"] = a["add"][ADD_SCALAR_BAD]
        for c in range(4):
            r["scalar_min"][c] = min_value(a["mn"][MIN_SCALAR + c])
            r["scalar_max"][c] = max_value(a["mx"][MAX_SCALAR + c])
    if pairs is not None:
        r["s_max"] = max_value(pairs[0])
        r["pair_bad"] = pairs[1]
    r["flags"] = (SCALARS_VALID if have_scalars else 0) | (DIFFUSION_VALID if pairs is not None else 0)
    return r


def step_row(p, before, after, quantum_log2, T_after=None):
    """The row of one step.  before: (pos, vel, mass) of S_k in particle order; after: dict(pos, vel, acc, rho, ncount)
    the step produced, in the same order (ids 0 .. n-1); T_after: the channels as the step left them, or None."""
    pos_k, vel_k, mass = before
    n = np.asarray(mass).size
    a = particles(after["pos"], after["vel"], mass, np.arange(n), after["acc"], after["rho"], after["ncount"],
                  quantum_log2, T_after)
    pairs = None
    if T_after is not None and n > 0:
        pairs = pair_acc(pair_sums(p, pos_k, vel_k, mass, after["rho"]))
    return row_of(a, T_after is not None and n > 0, pairs)


def same_rows(got, want):
    """the names of the fields in which two rows (or arrays of rows) differ, by bytes"""
    got, want = np.asarray(got, ROW), np.asarray(want, ROW)
    return [nm for nm in ROW.names if np.ascontiguousarray(got[nm]).tobytes() != np.ascontiguousarray(want[nm]).tobytes()]
