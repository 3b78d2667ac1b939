"""numpy restatement of buoyancy (csrc/buoyancy_policy.h; include/sph_hip.h: buoyancy), the checker of
tests/test_gpu_buoyancy.py and tests/test_buoyancy_cpu.py.

    s     0, then for c = 0 .. 3: s = s + beta[c] * (T_c - reference[c])
    b     (-s) * gravity per component
    guard s == 0 or s not finite: neither row of the particle changes
    a'    a + b, then accel_end's clamp: dot = (ax*ax + ay*ay) + az*az; where dot > cfl_limit2 every component times
          cfl_limit / sqrt(dot)
    v'    v + b * dt
numpy evaluates float32 arrays operation by operation with IEEE rounding and never fuses, so the bits are the
device's.  step() composes one whole FULL step from the oracle's phases (test infrastructure), the scalars'
restatement and apply()."""
import collections

import numpy as np

import scalar_emulation as SC
from helpers import to_oracle_params

F32 = np.float32

# {beta[4], reference[4], gravity[3]}: sph_hip_buoyancy
Setting = collections.namedtuple("Setting", ["beta", "reference", "gravity"])


def setting(beta, reference=(0.0, 0.0, 0.0, 0.0), gravity=(0.0, -9.81, 0.0)):
    def pad(v):
        out = np.zeros(4, F32)
        v = np.asarray(v, F32).reshape(-1)
        out[:v.size] = v
        return out
    return Setting(pad(beta), pad(reference), np.asarray(gravity, F32).reshape(3))


def of(buoyancy):
    """The Setting of a scalars.Buoyancy that has its gravity."""
    return setting(buoyancy.beta, buoyancy.reference, buoyancy.gravity)


def excess(b, Ts):
    Ts = np.asarray(Ts, F32).reshape(-1, 4)
    s = np.zeros(Ts.shape[0], F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(4):
            s = s + b.beta[c] * (Ts[:, c] - b.reference[c])
    return s.astype(F32)


def acts(s):
    with np.errstate(invalid="ignore"):
        return (s != 0) & (np.abs(s) <= F32(3.402823466e38))


def clamp(a, cfl_limit, cfl_limit2):
    """accel_end's rule on rows a (m, 3)."""
    a = np.asarray(a, F32).reshape(-1, 3).copy()
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        dot = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
        over = dot > F32(cfl_limit2)
        scale = F32(cfl_limit) / np.sqrt(dot[over])
        a[over] = a[over] * scale[:, None]
    return a


def apply(p, b, Ts, acc, vel, dt=None):
    """The kernel on rows in any one order: Ts (n, 4), acc and vel (3n,).  Returns (acc', vel', touched)."""
    dt = F32(p.time_step if dt is None else dt)
    acc = np.asarray(acc, F32).reshape(-1, 3)
    vel = np.asarray(vel, F32).reshape(-1, 3)
    s = excess(b, Ts)
    on = acts(s)
    a2, v2 = acc.copy(), vel.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        bb = ((-s[on])[:, None] * b.gravity[None, :]).astype(F32)
        a2[on] = clamp(acc[on] + bb, p.cfl_limit, p.cfl_limit2)
        v2[on] = vel[on] + bb * dt
    return a2.reshape(-1), v2.reshape(-1), on


def step(orc, p, pos, vel, mass, T, kappa, sources=(), b=None, integrate=None):
    """One whole FULL step of a context with scalars and the buoyancy b (None: none), everything in particle
    order: the oracle's cells and densities, the scalars' step, the oracle's accelerations, apply() with the
    channels as they stood BEFORE the scalars' step, the oracle's integrate - or integrate(op, pos, vel, acc, mass),
    in place on pos and vel, where a context's integrate does more (obstacles, a load recording).  Returns
    dict(pos, vel, acc, acc_before, rho, T, touched); nothing given is changed."""
    op = to_oracle_params(p)
    pos = np.ascontiguousarray(pos, F32).copy()
    vel = np.ascontiguousarray(vel, F32).copy()
    mass = np.ascontiguousarray(mass, F32)
    T = np.asarray(T, F32).reshape(-1, 4)
    _, cs, ci = orc.full_cells(op, pos)
    rho, _ = orc.full_density(op, pos, mass, cs, ci)
    # (a channel without diffusivity is carried by selection and there is no source: the scalars' step is the identity)
    idle = not np.asarray(kappa, F32).any() and len(sources) == 0
    T_new = T.copy() if idle else SC.step(p, pos, vel, mass, rho, T, kappa, sources)
    acc = orc.full_accel(op, pos, vel, mass, rho, cs, ci)
    before = acc.copy()
    touched = np.zeros(mass.size, bool)
    if b is not None:
        acc, vel, touched = apply(p, b, T, acc, vel)
        acc, vel = np.ascontiguousarray(acc), np.ascontiguousarray(vel)
    (integrate or orc.integrate)(op, pos, vel, acc, mass)
    return dict(pos=pos, vel=vel, acc=acc, acc_before=before, rho=rho, T=T_new, touched=touched)
