"""numpy restatement of the scene renderer (include/sph_hip.h: sph_hip_render_scene; the functions of
csrc/scene_policy.h), the checker of tests/test_scene_cpu.py and tests/test_gpu_scene_render.py, written
from the header's contract and vectorised over rays.

Every operation is one float32 numpy operation, in the contract's order; np.fmin / np.fmax follow the
C99 NaN rules of fminf / fmaxf.  A solid is anything with the fields of sph_hip_obstacle (the ctypes
struct, or an obstacles.Sphere / Box / Cylinder through as_struct()).
"""
import collections

import numpy as np

import render_emulation as E

F32 = np.float32
SPHERE, BOX, CYLINDER = 0, 1, 2

SceneFrame = collections.namedtuple("SceneFrame", E.Frame._fields + ("solid_id",))


def _struct(o):
    return o if hasattr(o, "_fields_") else o.as_struct()


def _f3(v):
    return np.array([float(c) for c in v], F32)


def slab(eye_a, d_a, lo, hi):
    """(near, far) of one axis: the renderer's box slab"""
    inv = F32(1.0) / d_a
    u0 = (F32(lo) - eye_a) * inv
    u1 = (F32(hi) - eye_a) * inv
    return np.fmin(u0, u1), np.fmax(u0, u1)


def _interval(t0, t1, d):
    """(hit, inside, t, normal for the inside case) of the rules every kind shares"""
    hit = (t0 <= t1) & (t1 >= F32(0.0))
    inside = hit & (t0 < F32(0.0))
    t = np.where(inside, F32(0.0), np.fmax(t0, F32(0.0)) + F32(0.0)).astype(F32)
    return hit, inside, t, (-d).astype(F32)


def hit(o, eye, d):
    """Where rays eye + t * d (d (n, 3) float32, normalised; eye (3,) or one per ray (n, 3)) enter solid o:
    (hit (n,) bool, t (n,) float32, normal (n, 3) float32); t and normal mean nothing where hit is False."""
    o = _struct(o)
    d = np.ascontiguousarray(d, F32).reshape(-1, 3)
    n = d.shape[0]
    eye = np.asarray(eye, F32)
    eye = np.ascontiguousarray(np.broadcast_to(_f3(eye), (n, 3)) if eye.ndim == 1 else eye.reshape(n, 3))
    cen, r = _f3(o.center), F32(o.radius)
    lo, hi = _f3(o.lo), _f3(o.hi)
    normal = np.zeros((n, 3), F32)
    with np.errstate(all="ignore"):
        if o.kind == SPHERE:
            oc = eye - cen[None, :]
            b = (oc[:, 0] * d[:, 0] + oc[:, 1] * d[:, 1]) + oc[:, 2] * d[:, 2]
            c = ((oc[:, 0] * oc[:, 0] + oc[:, 1] * oc[:, 1]) + oc[:, 2] * oc[:, 2]) - r * r
            disc = b * b - c
            ok = disc >= F32(0.0)
            s = np.sqrt(np.where(ok, disc, F32(0.0)))
            t0, t1 = (-b) - s, (-b) + s
            h, inside, t, nin = _interval(t0, t1, d)
            h &= ok
            for a in range(3):
                normal[:, a] = ((eye[:, a] + t * d[:, a]) - cen[a]) / r
        elif o.kind == BOX:
            nr = np.zeros((n, 3), F32)
            fr = np.zeros((n, 3), F32)
            for a in range(3):
                nr[:, a], fr[:, a] = slab(eye[:, a], d[:, a], lo[a], hi[a])
            t0 = np.fmax(np.fmax(nr[:, 0], nr[:, 1]), nr[:, 2])
            t1 = np.fmin(np.fmin(fr[:, 0], fr[:, 1]), fr[:, 2])
            h, inside, t, nin = _interval(t0, t1, d)
            ax = np.where(nr[:, 0] == t0, 0, np.where(nr[:, 1] == t0, 1, 2))
            da = d[np.arange(n), ax]
            normal[np.arange(n), ax] = np.where(da > F32(0.0), F32(-1.0), F32(1.0))
        elif o.kind == CYLINDER:
            a = int(o.axis)
            u, w = (a + 1) % 3, (a + 2) % 3
            ou, ow = eye[:, u] - cen[u], eye[:, w] - cen[w]
            du, dw = d[:, u], d[:, w]
            qa = du * du + dw * dw
            par = qa == F32(0.0)
            in_circle = ou * ou + ow * ow < r * r
            b = ou * du + ow * dw
            c = (ou * ou + ow * ow) - r * r
            disc = b * b - qa * c
            ok = np.where(par, in_circle, disc >= F32(0.0))
            s = np.sqrt(np.where(ok & ~par, disc, F32(0.0)))
            qs = np.where(par, F32(1.0), qa)
            s0 = np.where(par, F32(-np.inf), ((-b) - s) / qs).astype(F32)
            s1 = np.where(par, F32(np.inf), ((-b) + s) / qs).astype(F32)
            c0, c1 = slab(eye[:, a], d[:, a], lo[a], hi[a])
            side = s0 >= c0
            t0 = np.where(side, s0, c0).astype(F32)
            t1 = np.fmin(s1, c1)
            h, inside, t, nin = _interval(t0, t1, d)
            h &= ok
            normal[:, u] = np.where(side, ((eye[:, u] + t * du) - cen[u]) / r, F32(0.0))
            normal[:, w] = np.where(side, ((eye[:, w] + t * dw) - cen[w]) / r, F32(0.0))
            normal[:, a] = np.where(side, F32(0.0), np.where(d[:, a] > F32(0.0), F32(-1.0), F32(1.0)))
        else:
            raise ValueError("unknown obstacle kind %r" % (o.kind,))
        normal = np.where(inside[:, None], nin, normal).astype(F32)
    return h, t.astype(F32), normal


def nearest(solids, eye, d):
    """(t (n,), normal (n, 3), id (n,) int32): the list's nearest solid per ray, -1 and +inf for none;
    list order with a strict <, so the lower index wins a tie."""
    d = np.ascontiguousarray(d, F32).reshape(-1, 3)
    n = d.shape[0]
    t = np.full(n, np.inf, F32)
    normal = np.zeros((n, 3), F32)
    sid = np.full(n, -1, np.int32)
    for i, o in enumerate(solids):
        h, ti, ni = hit(o, eye, d)
        with np.errstate(invalid="ignore"):
            take = h & (ti < t)
        t[take] = ti[take]
        normal[take] = ni[take]
        sid[take] = i
    return t, normal, sid


def shade(normal, light, albedo, ambient, diffuse):
    """(n, 4) uint8: the renderer's Lambert formula; albedo (n, 3)"""
    L = _f3(light)
    ll = np.sqrt((L[0] * L[0] + L[1] * L[1]) + L[2] * L[2])
    l = L / ll
    ndl = (normal[:, 0] * l[0] + normal[:, 1] * l[1]) + normal[:, 2] * l[2]
    w = F32(ambient) + F32(diffuse) * np.fmax(ndl, F32(0.0))
    rgba = np.full((normal.shape[0], 4), 255, np.uint8)
    for c in range(3):
        rgba[:, c] = E.quantise(albedo[:, c] * w)
    return rgba


def composite(frame, solids, cam, rp, sp, width, height, velocities=None, albedos=None, velocity=True, pixels=None):
    """The fluid pass's flattened Frame (render_emulation.render's, of the same pixels) with the solids drawn
    into it: a SceneFrame.  sp has albedo / ambient / diffuse; velocities and albedos are (len(solids), 3),
    defaulting to 0 and sp.albedo; velocity=False is a call without SPH_HIP_RENDER_VELOCITY."""
    if pixels is None:
        py, px = np.divmod(np.arange(width * height, dtype=np.int64), width)
    else:
        px, py = (np.asarray(v, np.int64).reshape(-1) for v in pixels)
    k = len(solids)
    vel_s = np.zeros((k, 3), F32) if velocities is None else np.asarray(velocities, F32).reshape(k, 3)
    alb_s = np.tile(_f3(sp.albedo), (k, 1)) if albedos is None else np.asarray(albedos, F32).reshape(k, 3)
    d, ok = E.pixel_rays(cam, width, height, px, py)
    t, normal, sid = nearest(solids, cam.eye, np.where(ok[:, None], d, F32(1.0)).astype(F32))
    with np.errstate(invalid="ignore"):
        take = ok & (sid >= 0) & (t < frame.depth)
    sid = np.where(take, sid, -1).astype(np.int32)
    rgba, depth, nrm = frame.rgba.copy(), frame.depth.copy(), frame.normal.copy()
    vel, first = frame.velocity.copy(), frame.first_inside.copy()
    i = np.flatnonzero(take)
    if i.size:
        rgba[i] = shade(normal[i], rp.light, alb_s[sid[i]], sp.ambient, sp.diffuse)
        depth[i] = t[i]
        nrm[i] = normal[i]
        vel[i] = vel_s[sid[i]] if velocity else F32(0.0)
        first[i] = -1
    return SceneFrame(rgba, depth, nrm, vel, first, sid)


def background(rp, n):
    """the fluid pass's Frame of n pixels when no particle is resident"""
    return E.Frame(np.tile(np.array(list(rp.background), np.uint8), (n, 1)), np.full(n, np.inf, F32),
                   np.zeros((n, 3), F32), np.zeros((n, 3), F32), np.full(n, -1, np.int32))


def motion_velocity(motion, tau):
    """a driven solid's velocity at the motion clock tau: the motion's while start <= tau < stop"""
    v = _f3(motion.velocity)
    on = bool((v != 0).any()) and F32(motion.start) <= F32(tau) < F32(motion.stop)
    return v if on else np.zeros(3, F32)
