"""numpy restatement of the renderer (include/sph_hip.h: sph_hip_render), the checker of
tests/test_gpu_render.py and tests/test_render_cpu.py, written from the header's contract.

The field f is a callable: points (n, 3) float32 -> density (n,) float32.  On the device checks it
is sample_emulation.Grid(...).sample (the sampler's bits); on CPU checks, analytic fields.  Every
ray is marched at once, one sample index k at a time, with an active mask.  numpy evaluates float32
arrays operation by operation with IEEE rounding and never fuses, and np.fmin / np.fmax follow the
C99 NaN rules of fminf / fmaxf, so the bits are the device's.
"""
import collections

import numpy as np

F32 = np.float32

Frame = collections.namedtuple("Frame", ["rgba", "depth", "normal", "velocity", "first_inside"])


def _v(x):
    return np.array([float(c) for c in x], F32)


def pixel_rays(cam, width, height, px, py):
    """(direction (n, 3), ok (n,)) of pixels (px, py): ok is False where len is 0 or not finite."""
    px = np.asarray(px, np.int64)
    py = np.asarray(py, np.int64)
    a = (2 * px + 1 - width).astype(F32) / F32(width)
    b = (height - 2 * py - 1).astype(F32) / F32(height)
    fw, rt, up = _v(cam.forward), _v(cam.right), _v(cam.up)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        dc = (fw[None, :] + a[:, None] * rt[None, :]) + b[:, None] * up[None, :]
        ln = np.sqrt((dc[:, 0] * dc[:, 0] + dc[:, 1] * dc[:, 1]) + dc[:, 2] * dc[:, 2])
        ok = (ln > F32(0)) & np.isfinite(ln)
        d = (dc / ln[:, None]).astype(F32)
    return d, ok


def box_interval(eye, d, lo, hi):
    """(tnear, tfar, hit) of rays from eye along d through the box [lo, hi]."""
    eye, lo, hi = _v(eye), _v(lo), _v(hi)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        inv = F32(1.0) / d
        t0 = (lo - eye)[None, :] * inv
        t1 = (hi - eye)[None, :] * inv
        near = np.fmin(t0, t1)
        far = np.fmax(t0, t1)
        tnear = np.fmax(np.fmax(np.fmax(near[:, 0], near[:, 1]), near[:, 2]), F32(0.0))
        tfar = np.fmin(np.fmin(far[:, 0], far[:, 1]), far[:, 2])
        hit = tnear <= tfar
    return tnear.astype(F32), tfar.astype(F32), hit


def point_at(eye, t, d):
    return (_v(eye)[None, :] + t[:, None] * d).astype(F32)


def quantise(v):
    """(uint8)(fminf(fmaxf(v, 0), 1) * 255 + 0.5), NaN -> 0"""
    v = np.asarray(v, F32)
    with np.errstate(invalid="ignore"):
        return (np.fmin(np.fmax(v, F32(0.0)), F32(1.0)) * F32(255.0) + F32(0.5)).astype(np.uint8)


def render(field, cam, rp, width, height, velocity_field=None, pixels=None):
    """The frame, or the pixels (px, py) of it (flattened, in the given order).  rp has the fields of
    sph_hip_render_params (the ctypes struct will do).  velocity_field: points -> (n, 3) Shepard
    velocity, or None (velocity stays 0, as without SPH_HIP_RENDER_VELOCITY)."""
    if pixels is None:
        py, px = np.divmod(np.arange(width * height, dtype=np.int64), width)
    else:
        px, py = (np.asarray(v, np.int64).reshape(-1) for v in pixels)
    n = px.size
    step, iso, gs = F32(rp.step), F32(rp.iso), F32(rp.grad_step)
    eye = _v(cam.eye)
    d, ok = pixel_rays(cam, width, height, px, py)
    tnear, tfar, inbox = box_interval(eye, d, rp.box_lo, rp.box_hi)
    active = ok & inbox
    first = np.full(n, -1, np.int32)
    k = 0
    while active.any():
        idx = np.flatnonzero(active)
        with np.errstate(invalid="ignore", over="ignore"):
            t = (tnear[idx] + F32(k) * step).astype(F32)
            go = (t <= tfar[idx]) & (k < int(rp.max_samples))
        active[idx[~go]] = False
        idx, t = idx[go], t[go]
        if idx.size == 0:
            break
        with np.errstate(invalid="ignore"):
            inside = np.asarray(field(point_at(eye, t, d[idx])), F32) > iso
        first[idx[inside]] = k
        active[idx[inside]] = False
        k += 1

    rgba = np.tile(np.array(list(rp.background), np.uint8), (n, 1))
    depth = np.full(n, np.inf, F32)
    normal = np.zeros((n, 3), F32)
    vel = np.zeros((n, 3), F32)
    h = np.flatnonzero(first >= 0)
    if h.size:
        dh, t0, kk = d[h], tnear[h], first[h]
        ta = (t0 + np.maximum(kk - 1, 0).astype(F32) * step).astype(F32)
        tb = np.where(kk > 0, (t0 + kk.astype(F32) * step).astype(F32), t0).astype(F32)
        ref = np.flatnonzero(kk > 0)
        for _ in range(int(rp.refine)):
            if ref.size == 0:
                break
            tm = (F32(0.5) * (ta[ref] + tb[ref])).astype(F32)
            with np.errstate(invalid="ignore"):
                ins = np.asarray(field(point_at(eye, tm, dh[ref])), F32) > iso
            tb[ref] = np.where(ins, tm, tb[ref])
            ta[ref] = np.where(ins, ta[ref], tm)
        p = point_at(eye, tb, dh)
        two = F32(2.0) * gs
        g = np.zeros((h.size, 3), F32)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            for a in range(3):
                q = p.copy()
                q[:, a] = p[:, a] + gs
                fp = np.asarray(field(q), F32)
                q[:, a] = p[:, a] - gs
                fm = np.asarray(field(q), F32)
                g[:, a] = (fp - fm) / two
            gl = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
            gok = (gl > F32(0)) & np.isfinite(gl)
            nh = np.where(gok[:, None], -(g / gl[:, None]), F32(0.0)).astype(F32)
            L = _v(rp.light)
            ll = np.sqrt((L[0] * L[0] + L[1] * L[1]) + L[2] * L[2])
            l = L / ll
            ndl = (nh[:, 0] * l[0] + nh[:, 1] * l[1]) + nh[:, 2] * l[2]
            w = F32(rp.ambient) + F32(rp.diffuse) * np.fmax(ndl, F32(0.0))
            alb = _v(rp.albedo)
            for c in range(3):
                rgba[h, c] = quantise(alb[c] * w)
        rgba[h, 3] = 255
        depth[h] = tb
        normal[h] = nh
        if velocity_field is not None:
            vel[h] = np.asarray(velocity_field(p), F32).reshape(-1, 3)
    return Frame(rgba, depth, normal, vel, first)


def grid_fields(grid):
    """(density field, velocity field) of a sample_emulation.Grid"""
    return (lambda pts: grid.sample(pts, velocity=False)[0]), (lambda pts: grid.sample(pts)[1])
