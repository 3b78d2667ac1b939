"""numpy restatement of the iso-surface extractor (include/sph_hip.h: sph_hip_extract_surface), the
checker of tests/test_gpu_surface.py and tests/test_surface_cpu.py.  Written from the header's
contract, not from csrc/surface_policy.h's tables: the triangles of every tetrahedron case are
oriented here from the geometry at the edge midpoints and started at their smallest vertex id at
run time.  numpy evaluates float32 arrays operation by operation with IEEE rounding and never
fuses, so vertices, normals and velocities carry the device's bits.

`extract` works on any density lattice f[nz, ny, nx] (float32): sample_emulation's, the device's
own sampleLattice output, or an analytic field.
"""
import collections

import numpy as np

F32 = np.float32

# the seven positive-direction edges of a lattice point, as (dx, dy, dz), in canonical order
EDGES = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]
# Kuhn split: tetrahedron {0, a, a|b, 7} for these (a, b), corner c = x + 2y + 4z
TET_AB = [(1, 2), (1, 4), (2, 1), (2, 4), (4, 1), (4, 2)]

Mesh = collections.namedtuple("Mesh", ["vertices", "triangles", "normals", "velocity"])


def corner_xyz(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1])


def edge_of(lo, hi):
    """(corner offset of the owning point, edge place) of the cube edge between corners lo < hi"""
    d = corner_xyz(hi) - corner_xyz(lo)
    return lo, EDGES.index(tuple(int(v) for v in d))


def lattice_axes(origin, spacing, shape):
    """origin + (float)i * spacing per axis, fp32 unfused: (x[nx], y[ny], z[nz])"""
    return [F32(origin[a]) + np.arange(shape[a], dtype=np.int64).astype(F32) * F32(spacing[a]) for a in range(3)]


def gradient(f, spacing):
    """the lattice gradient (g[..., 0] along x), the header's per-axis rule"""
    g = np.zeros(f.shape + (3,), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            ax = 2 - a   # f is [z, y, x]
            n = f.shape[ax]
            s = F32(spacing[a])
            if n == 1:
                continue
            out = np.moveaxis(g[..., a], ax, 0)
            v = np.moveaxis(f, ax, 0)
            out[0] = (v[1] - v[0]) / s
            out[n - 1] = (v[n - 1] - v[n - 2]) / s
            if n > 2:
                out[1:n - 1] = (v[2:] - v[:n - 2]) / (F32(2.0) * s)
    return g


def extract(f, origin, spacing, iso, velocity=None, normals=True):
    """The mesh of {f > iso}: Mesh(vertices (V,3), triangles (T,3) int32, normals or None,
    velocity (V,3) of the given velocity lattice [nz, ny, nx, 3] or None)."""
    f = np.ascontiguousarray(f, F32)
    nz, ny, nx = f.shape
    iso = F32(iso)
    with np.errstate(invalid="ignore"):
        inside = f > iso
    # crossing edges and vertex ids: rank in (lattice index, edge place) order
    cross = np.zeros((nz, ny, nx, 7), bool)
    for e, (dx, dy, dz) in enumerate(EDGES):
        a = inside[:nz - dz, :ny - dy, :nx - dx]
        b = inside[dz:, dy:, dx:]
        cross[:nz - dz, :ny - dy, :nx - dx, e] = a != b
    flat = cross.reshape(-1, 7)
    ids = np.full(flat.shape, -1, np.int64)
    ids[flat] = np.arange(int(flat.sum()))
    p, e = np.nonzero(flat)                      # sorted by point, then edge: id order
    k, rem = np.divmod(p, nx * ny)
    j, i = np.divmod(rem, nx)
    d = np.array(EDGES)[e]
    kb, jb, ib = k + d[:, 2], j + d[:, 1], i + d[:, 0]
    fa, fb = f[k, j, i], f[kb, jb, ib]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = (iso - fa) / (fb - fa)
        t = np.fmin(np.fmax(t, F32(0.0)), F32(1.0)).astype(F32)
        X, Y, Z = lattice_axes(origin, spacing, (nx, ny, nz))
        xa = np.stack([X[i], Y[j], Z[k]], 1)
        xb = np.stack([X[ib], Y[jb], Z[kb]], 1)
        verts = (xa + t[:, None] * (xb - xa)).astype(F32)
        nrm = None
        if normals:
            G = gradient(f, spacing)
            ga, gb = G[k, j, i], G[kb, jb, ib]
            g = (ga + t[:, None] * (gb - ga)).astype(F32)
            ln = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
            ok = np.isfinite(ln) & (ln > F32(0.0))
            nrm = np.where(ok[:, None], -(g / ln[:, None]), F32(0.0)).astype(F32)
        vel = None
        if velocity is not None:
            vv = np.asarray(velocity, F32).reshape(nz, ny, nx, 3)
            va, vb = vv[k, j, i], vv[kb, jb, ib]
            vel = (va + t[:, None] * (vb - va)).astype(F32)
    tris = triangles(inside, ids, spacing)
    return Mesh(verts, tris, nrm, vel)


def _cycle(t, m, spacing):
    """The oriented cycle of (corner, corner) edges of tetrahedron t in case m, or None"""
    a, b = TET_AB[t]
    path = [0, a, a | b, 7]
    ins = [path[q] for q in range(4) if (m >> q) & 1]
    out = [path[q] for q in range(4) if not (m >> q) & 1]
    if not ins or not out:
        return None
    if len(ins) == 1:
        cyc = [(ins[0], o) for o in out]
    elif len(out) == 1:
        cyc = [(q, out[0]) for q in ins]
    else:
        cyc = [(ins[0], out[0]), (ins[0], out[1]), (ins[1], out[1]), (ins[1], out[0])]
    sp = np.asarray(spacing, np.float64)
    pos = lambda c: corner_xyz(c) * sp
    mid = [0.5 * (pos(u) + pos(v)) for u, v in cyc]
    nrm = np.cross(mid[1] - mid[0], mid[2] - mid[0])
    toward = np.mean([pos(c) for c in out], 0) - np.mean([pos(c) for c in ins], 0)
    if np.dot(nrm, toward) < 0:
        cyc = cyc[:1] + cyc[1:][::-1]
    return [edge_of(min(u, v), max(u, v)) for u, v in cyc]


def triangles(inside, ids, spacing):
    nz, ny, nx = inside.shape
    if nx < 2 or ny < 2 or nz < 2:
        return np.zeros((0, 3), np.int32)
    kk, jj, ii = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    kk, jj, ii = kk.reshape(-1), jj.reshape(-1), ii.reshape(-1)
    corner_in = [inside[kk + ((c >> 2) & 1), jj + ((c >> 1) & 1), ii + (c & 1)] for c in range(8)]
    cube = (kk * ny + jj) * nx + ii
    keys, rows = [], []
    for t, (a, b) in enumerate(TET_AB):
        path = [0, a, a | b, 7]
        case = sum(corner_in[path[q]].astype(np.int64) << q for q in range(4))
        for m in range(1, 15):
            sel = np.flatnonzero(case == m)
            if sel.size == 0:
                continue
            cyc = _cycle(t, m, spacing)
            vid = np.stack([ids[cube[sel] + (c & 1) + ((c >> 1) & 1) * nx + ((c >> 2) & 1) * nx * ny, e]
                            for c, e in cyc], 1)
            assert (vid >= 0).all()
            start = np.argmin(vid, 1)
            n = vid.shape[1]
            vid = vid[np.arange(len(sel))[:, None], (start[:, None] + np.arange(n)[None, :]) % n]
            if n == 3:
                keys.append(cube[sel] * 12 + 2 * t)
                rows.append(vid)
            else:
                keys += [cube[sel] * 12 + 2 * t, cube[sel] * 12 + 2 * t + 1]
                rows += [vid[:, [0, 1, 2]], vid[:, [0, 2, 3]]]
    if not rows:
        return np.zeros((0, 3), np.int32)
    key = np.concatenate(keys)
    tri = np.concatenate(rows)
    return tri[np.argsort(key, kind="stable")].astype(np.int32)


# ---- mesh checks -----------------------------------------------------------------------------------
def directed_edges(tri):
    t = np.asarray(tri, np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def is_closed_oriented(tri):
    """every undirected edge used by exactly two triangles, once in each direction"""
    if len(tri) == 0:
        return True
    de = directed_edges(tri)
    n = int(de.max()) + 1
    code = de[:, 0] * n + de[:, 1]
    if np.unique(code).size != code.size:
        return False
    rev = np.sort(de[:, 1] * n + de[:, 0])
    return np.array_equal(np.sort(code), rev)


def boundary_edges(tri):
    """directed edges whose reverse is not in the mesh"""
    de = directed_edges(tri)
    n = int(de.max()) + 1
    code = de[:, 0] * n + de[:, 1]
    rev = de[:, 1] * n + de[:, 0]
    return de[~np.isin(code, rev)]


def is_manifold(tri):
    """every undirected edge used by at most two triangles, never twice in one direction"""
    if len(tri) == 0:
        return True
    de = directed_edges(tri)
    n = int(de.max()) + 1
    code = de[:, 0] * n + de[:, 1]
    und = np.minimum(de[:, 0], de[:, 1]) * n + np.maximum(de[:, 0], de[:, 1])
    return np.unique(code).size == code.size and np.bincount(np.unique(und, return_inverse=True)[1]).max() <= 2


def euler(tri):
    """V - E + F over the vertices the triangles use"""
    t = np.asarray(tri, np.int64)
    v = np.unique(t).size
    de = directed_edges(t)
    und = np.unique(np.minimum(de[:, 0], de[:, 1]) * (int(t.max()) + 1) + np.maximum(de[:, 0], de[:, 1]))
    return v - und.size + len(t)


def volume(vertices, tri):
    """enclosed volume by the divergence theorem (float64)"""
    v = np.asarray(vertices, np.float64)
    t = np.asarray(tri, np.int64)
    return float(np.einsum("ij,ij->i", v[t[:, 0]], np.cross(v[t[:, 1]], v[t[:, 2]])).sum() / 6.0)
