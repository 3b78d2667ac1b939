"""numpy restatement of the scalar renderer (include/sph_hip.h: sph_hip_render_scalars; the functions of
csrc/tint_policy.h), the checker of tests/test_tint_cpu.py and tests/test_gpu_tint.py, written from the header's
contract on top of render_emulation.Frame, scene_emulation's composite and the scalar sampler's restatement
(scalar_emulation.sample's sums, here with the grid built once).

    pixels   first_inside >= 0 after the fluid pass and the solids pass; every other pixel is kept, scalar 0
    SURFACE  v = rho > 0 ? a_channel / rho : 0 at p_hit = eye + depth * d
    COLUMN   A = 0; for k = first_inside ... while t_k <= tfar and k < max_samples: (rho, a) = walk(eye + t_k * d),
             rho > iso: A = A + (rho > 0 ? a / rho : 0) * step
    map      u = (v - lo) / (hi - lo), clamped by fmin(fmax(u, 0), 1); x = u * (n - 1); i = min((int)x, n - 2);
             fr = x - i; col = t[i] + fr * (t[i + 1] - t[i])
    shade    w = 1 (FLAT) or ambient + diffuse * fmax(ndl, 0) of the stored normal; byte of col * w, alpha 255
Every operation is one float32 numpy operation in the contract's order.  The column marches all rays at once,
one k at a time."""
import collections

import numpy as np

import pressure_emulation as PE
import render_emulation as E
import sample_emulation as SE
import scene_emulation as SCN

F32 = np.float32
SURFACE, COLUMN = 0, 1
FLAT = 1

Tint = collections.namedtuple("Tint", ["channel", "mode", "lo", "hi", "flags"])
TintFrame = collections.namedtuple("TintFrame", SCN.SceneFrame._fields + ("scalar",))


class Walk:
    """walk(p) of a state: the scalar sampler's sums over the sampler's members in canonical order."""

    def __init__(self, p, pos, vel, mass, T):
        self.grid = SE.Grid(p, pos, vel, mass)
        self.Ts = np.asarray(T, F32).reshape(-1, 4)[PE.canonical_order(p, pos)]

    def __call__(self, points, channel):
        """(rho (m,), a_channel (m,), count (m,)) of the probes; channel None: a of all four channels, (m, 4)"""
        points = np.asarray(points, F32).reshape(-1, 3)
        m = points.shape[0]
        chans = range(4) if channel is None else [channel]
        if m == 0:
            return np.zeros(0, F32), np.zeros(0 if channel is not None else (0, 4), F32), np.zeros(0, np.int32)
        probe, idx, d2 = PE.members(self.grid, points)
        t = SE.density_terms(self.grid.p, d2, self.grid.mass[idx])
        with np.errstate(invalid="ignore", over="ignore"):
            cols = [t] + [(t * self.Ts[idx, ch]).astype(F32) for ch in chans]
        sums, count = PE.ordered_sums(probe, m, cols)
        return sums[0], (sums[1] if channel is not None else np.stack(sums[1:], 1)), count

    def density(self, points):
        return self(points, 0)[0]


def shepard(a, rho):
    """rho > 0 ? a / rho : 0; a (m,) or (m, 4)"""
    a = np.asarray(a, F32)
    if a.ndim == 2:
        return np.stack([PE.quotient(a[:, c], rho) for c in range(a.shape[1])], 1)
    return PE.quotient(a, rho)


def color_map(v, lo, hi, table):
    """(m, 3) float32 colours of the values v through the (n, 3) table"""
    v = np.asarray(v, F32).reshape(-1)
    t = np.asarray(table, F32).reshape(-1, 3)
    n = t.shape[0]
    lo, hi = F32(lo), F32(hi)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (v - lo) / (hi - lo)
        u = np.fmin(np.fmax(u, F32(0.0)), F32(1.0))
        x = (u * F32(n - 1)).astype(F32)
        i = np.minimum(x.astype(np.int32), n - 2)
        fr = (x - i.astype(F32)).astype(F32)
        return (t[i] + fr[:, None] * (t[i + 1] - t[i])).astype(F32)


def weight(normal, light, ambient, diffuse):
    """the renderer's Lambert weight of stored normals (m, 3)"""
    normal = np.asarray(normal, F32).reshape(-1, 3)
    L = E._v(light)
    with np.errstate(invalid="ignore", over="ignore"):
        ll = np.sqrt((L[0] * L[0] + L[1] * L[1]) + L[2] * L[2])
        l = L / ll
        ndl = (normal[:, 0] * l[0] + normal[:, 1] * l[1]) + normal[:, 2] * l[2]
        return (F32(ambient) + F32(diffuse) * np.fmax(ndl, F32(0.0))).astype(F32)


def pixel(col, w):
    """(m, 4) uint8 of colours (m, 3) under the weights w (m,)"""
    col = np.asarray(col, F32).reshape(-1, 3)
    rgba = np.full((col.shape[0], 4), 255, np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(3):
            rgba[:, c] = E.quantise(col[:, c] * np.asarray(w, F32))
    return rgba


def column_add(A, rho, a, iso, step):
    """one sample into the running integrals A (m,)"""
    with np.errstate(invalid="ignore", over="ignore"):
        inside = np.asarray(rho, F32) > F32(iso)
        if np.asarray(A).ndim == 2:
            inside = inside[:, None]
        return np.where(inside, A + shepard(a, rho) * F32(step), A).astype(F32)


def column_sequence(rhos, As, iso, step):
    """the accumulation of one ray over a scripted sequence of (rho, a): A after the last sample"""
    A = np.zeros(1, F32)
    for rho, a in zip(rhos, As):
        A = column_add(A, np.array([rho], F32), np.array([a], F32), iso, step)
    return A[0]


def column(walk, cam, rp, width, height, px, py, first, channel):
    """(A (m,), inside count (m,)) of the pixels (px, py), whose first inside sample is first (m,) >= 0; channel
    None: A (m, 4) of all four channels"""
    px, py = np.asarray(px, np.int64), np.asarray(py, np.int64)
    m = px.size
    A = np.zeros(m if channel is not None else (m, 4), F32)
    inside_count = np.zeros(m, np.int64)
    if m == 0:
        return A, inside_count
    step, iso = F32(rp.step), F32(rp.iso)
    eye = E._v(cam.eye)
    d, _ = E.pixel_rays(cam, width, height, px, py)
    tnear, tfar, _ = E.box_interval(eye, d, rp.box_lo, rp.box_hi)
    k = np.asarray(first, np.int64).copy()
    active = np.ones(m, bool)
    while active.any():
        idx = np.flatnonzero(active)
        with np.errstate(invalid="ignore", over="ignore"):
            t = (tnear[idx] + k[idx].astype(F32) * step).astype(F32)
            go = (t <= tfar[idx]) & (k[idx] < int(rp.max_samples))
        active[idx[~go]] = False
        idx, t = idx[go], t[go]
        if idx.size == 0:
            break
        rho, a, _ = walk(E.point_at(eye, t, d[idx]), channel)
        with np.errstate(invalid="ignore"):
            inside_count[idx] += rho > iso
        A[idx] = column_add(A[idx], rho, a, iso, step)
        k[idx] += 1
    return A, inside_count


def values(frame, walk, cam, rp, mode, width, height, pixels=None, channel=None):
    """v of the frame's fluid pixels (first_inside >= 0, in pixel order) in `mode`: (h,) of one channel, or (h, 4)
    of all four (channel None) - what tint() maps, computed once for several tints of one frame"""
    if pixels is None:
        py, px = np.divmod(np.arange(width * height, dtype=np.int64), width)
    else:
        px, py = (np.asarray(v, np.int64).reshape(-1) for v in pixels)
    h = np.flatnonzero(frame.first_inside >= 0)
    if mode == SURFACE:
        d, _ = E.pixel_rays(cam, width, height, px[h], py[h])
        rho, a, _ = walk(E.point_at(E._v(cam.eye), frame.depth[h], d), channel)
        return shepard(a, rho)
    return column(walk, cam, rp, width, height, px[h], py[h], frame.first_inside[h], channel)[0]


def tint(frame, walk, cam, rp, tp, table, width, height, pixels=None, v=None):
    """The flattened frame (a render_emulation.Frame or a scene_emulation.SceneFrame of the same pixels) with its
    fluid pixels tinted: a TintFrame.  tp: a Tint; walk: a Walk, or None when no particle is resident; v: the
    fluid pixels' values where values() has computed them already."""
    if pixels is None:
        py, px = np.divmod(np.arange(width * height, dtype=np.int64), width)
    else:
        px, py = (np.asarray(v, np.int64).reshape(-1) for v in pixels)
    n = px.size
    solid_id = frame.solid_id.copy() if hasattr(frame, "solid_id") else np.full(n, -1, np.int32)
    rgba = frame.rgba.copy()
    scalar = np.zeros(n, F32)
    h = np.flatnonzero(frame.first_inside >= 0)
    if h.size and (walk is not None or v is not None):
        if v is None:
            v = values(frame, walk, cam, rp, tp.mode, width, height, pixels, tp.channel)
        col = color_map(v, tp.lo, tp.hi, table)
        if tp.flags & FLAT:
            w = np.ones(h.size, F32)
        else:
            w = weight(frame.normal[h], rp.light, rp.ambient, rp.diffuse)
        rgba[h] = pixel(col, w)
        scalar[h] = v
    return TintFrame(rgba, frame.depth.copy(), frame.normal.copy(), frame.velocity.copy(), frame.first_inside.copy(),
                     solid_id, scalar)
