"""numpy restatement of the tracers (csrc/tracer_policy.h; include/sph_hip.h: sph_hip_set_tracers) on top of
the field sampler's restatement (sample_emulation.Grid), the checker of tests/test_gpu_tracers.py and
tests/test_tracers_cpu.py.

A tracer moves as a particle does: the integrate displaces a particle by vh * (dt * sim_scale_inv), so the
advance uses that displacement step, pos_dt = dt * sim_scale_inv (one fp32 product: displacement_step).  One
advance of a tracer at x in the state S (positions, velocities, masses):
    1  (u1, c1) = sample(S, x)                      Shepard velocity and member count
    2  c1 == 0: dry - x unchanged, dry_steps += 1
    3  half = 0.5f * pos_dt; xm = x + u1 * half; (u2, c2) = sample(S, xm); u = c2 > 0 ? u2 : u1
    4  y = x + u * pos_dt; any component not finite: dry as in 2
    5  apply_walls: y < 0 -> 0, y > max -> max
    6  x = y; wet_steps += 1
numpy evaluates float32 arrays operation by operation with IEEE rounding and never fuses, so the bits are
the device's."""
import collections

import numpy as np

import sample_emulation as SE

F32 = np.float32

# x float32 (n, 3), wet and dry int32 (n,)
State = collections.namedtuple("State", ["x", "wet", "dry"])
# what each tracer did in one advance (boolean (n,) each): dry because c1 == 0, second probe without members,
# dry because y was not finite, clamped on a face [n, 3] low / high, moved (x changed)
Info = collections.namedtuple("Info", ["no_members", "midpoint_empty", "not_finite", "clamp_lo", "clamp_hi", "moved",
                                       "wet"])


def initial(points):
    x = np.array(points, F32).reshape(-1, 3)
    return State(x, np.zeros(len(x), np.int32), np.zeros(len(x), np.int32))


def displacement_step(p, dt):
    """pos_dt: the time step times the parameters' sim_scale_inv, one fp32 product (csrc/launch.h: launch_tracers;
    csrc/common_kernels.h: the integrate's pos_dt)"""
    return F32(F32(dt) * F32(p.sim_scale_inv))


def midpoint(x, u1, pos_dt):
    """step 3's probe"""
    half = F32(0.5) * F32(pos_dt)
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(x, F32) + np.asarray(u1, F32) * half).astype(F32)


def finish(state, u1, c1, u2, c2, pos_dt, apply_walls, maxv):
    """Steps 2 to 6 from the two probes' answers: (State, Info)."""
    x = np.asarray(state.x, F32)
    pos_dt = F32(pos_dt)
    have = np.asarray(c1) > 0
    second = np.asarray(c2) > 0
    u = np.where(second[:, None], np.asarray(u2, F32), np.asarray(u1, F32)).astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        y = (x + u * pos_dt).astype(F32)
    finite = np.isfinite(y).all(1)
    wet = have & finite
    maxv = np.asarray(maxv, F32).reshape(3)
    lo = np.zeros_like(y, bool)
    hi = np.zeros_like(y, bool)
    if apply_walls:
        with np.errstate(invalid="ignore"):
            lo = y < F32(0.0)
            y = np.where(lo, F32(0.0), y).astype(F32)
            hi = y > maxv[None, :]
            y = np.where(hi, maxv[None, :], y).astype(F32)
    new_x = np.where(wet[:, None], y, x).astype(F32)
    info = Info(~have, have & ~second, have & ~finite, lo & wet[:, None], hi & wet[:, None],
                (new_x.view(np.uint32) != x.view(np.uint32)).any(1), wet)
    return State(new_x, (state.wet + wet).astype(np.int32), (state.dry + ~wet).astype(np.int32)), info


def advance(p, pos, vel, mass, tracers, dt, with_info=False):
    """One advance of `tracers` (a State) in the state (pos, vel, mass) under the parameters p with the time
    step dt; the displacement step comes from p (displacement_step)."""
    n = len(tracers.x)
    pos_dt = displacement_step(p, dt)
    if np.asarray(mass).size == 0 or n == 0:
        zero3, zero = np.zeros((n, 3), F32), np.zeros(n, np.int32)
        out = finish(tracers, zero3, zero, zero3, zero, pos_dt, p.apply_walls, (p.max_x, p.max_y, p.max_z))
        return out if with_info else out[0]
    g = SE.Grid(p, pos, vel, mass)
    _, u1, c1 = g.sample(tracers.x)
    _, u2, c2 = g.sample(midpoint(tracers.x, u1, pos_dt))
    out = finish(tracers, u1, c1, u2, c2, pos_dt, p.apply_walls, (p.max_x, p.max_y, p.max_z))
    return out if with_info else out[0]
