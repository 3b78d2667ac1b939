"""Static analytic obstacles (include/sph_hip.h: sph_hip_set_obstacles).

`Sphere`, `Box`, `Cylinder` and `Wedge` (a box cut by one plane: the way to a slope) describe the solids
a context's particles collide with; `as_struct()` gives the C ABI's sph_hip_obstacle,
`signed_distance(points)` the numpy distance to the surface (negative inside), for placing obstacles
and checking results.  `Motion` is the constant velocity an
obstacle is driven at between two readings of the context's motion clock
(sph_hip_set_obstacle_motion); `MotionPath` is a keyframed displacement it follows instead
(sph_hip_set_obstacle_paths); `Body` makes it a free body that the fluid's own loads move
(sph_hip_set_bodies).  The collision response itself is csrc/obstacle_policy.h and runs on the GPU.
`Rotation` tilts an obstacle, or turns it at a constant angular rate, about a coordinate axis through a
pivot: the contract (csrc/obstacle_policy.h, third part), scene building and carving only - no context
takes a rotation list yet.
"""
import ctypes as C
import math

import numpy as np

SPHERE, BOX, CYLINDER, WEDGE = 0, 1, 2, 3   # SPH_HIP_OBSTACLE_* (include/sph_hip.h)
MAX_OBSTACLES = 64                # SPH_HIP_MAX_OBSTACLES


class SphObstacle(C.Structure):
    """Mirror of sph_hip_obstacle (include/sph_hip.h): 48 bytes, field order is ABI."""

    _fields_ = [("kind", C.c_int32), ("axis", C.c_int32), ("center", C.c_float * 3), ("radius", C.c_float),
                ("lo", C.c_float * 3), ("hi", C.c_float * 3)]


def _vec3(v):
    return np.array(v, np.float32).reshape(3)


def _points(points):
    return np.asarray(points, np.float64).reshape(-1, 3)


class Sphere:
    kind = SPHERE

    def __init__(self, center, radius):
        self.center, self.radius = _vec3(center), np.float32(radius)

    def as_struct(self):
        s = SphObstacle()
        s.kind = SPHERE
        s.center[:] = [float(v) for v in self.center]
        s.radius = float(self.radius)
        return s

    def signed_distance(self, points):
        d = _points(points) - self.center.astype(np.float64)
        return np.sqrt((d * d).sum(1)) - float(self.radius)

    def __repr__(self):
        return "Sphere(%s, %g)" % (list(self.center), self.radius)


class Box:
    """Axis-aligned box [lo, hi]."""

    kind = BOX

    def __init__(self, lo, hi):
        self.lo, self.hi = _vec3(lo), _vec3(hi)

    def as_struct(self):
        s = SphObstacle()
        s.kind = BOX
        s.lo[:] = [float(v) for v in self.lo]
        s.hi[:] = [float(v) for v in self.hi]
        return s

    def signed_distance(self, points):
        p = _points(points)
        lo, hi = self.lo.astype(np.float64), self.hi.astype(np.float64)
        q = np.maximum(lo - p, p - hi)                       # per axis: > 0 outside that slab
        outside = np.sqrt((np.maximum(q, 0.0) ** 2).sum(1))
        inside = np.minimum(q.max(1), 0.0)
        return outside + inside

    def __repr__(self):
        return "Box(%s, %s)" % (list(self.lo), list(self.hi))


class Cylinder:
    """Capped cylinder along `axis` (0 x, 1 y, 2 z): radius about `center` (whose axis component is
    ignored), caps at lo and hi on the axis."""

    kind = CYLINDER

    def __init__(self, axis, center, radius, lo, hi):
        if int(axis) not in (0, 1, 2):
            raise ValueError("axis must be 0, 1 or 2")
        self.axis = int(axis)
        self.center, self.radius = _vec3(center), np.float32(radius)
        self.lo, self.hi = np.float32(lo), np.float32(hi)

    def as_struct(self):
        s = SphObstacle()
        s.kind = CYLINDER
        s.axis = self.axis
        s.center[:] = [float(v) for v in self.center]
        s.radius = float(self.radius)
        s.lo[self.axis] = float(self.lo)
        s.hi[self.axis] = float(self.hi)
        return s

    def signed_distance(self, points):
        p = _points(points)
        a = self.axis
        u, w = (a + 1) % 3, (a + 2) % 3
        c = self.center.astype(np.float64)
        radial = np.hypot(p[:, u] - c[u], p[:, w] - c[w]) - float(self.radius)
        cap = np.maximum(float(self.lo) - p[:, a], p[:, a] - float(self.hi))
        q = np.stack([radial, cap], 1)
        outside = np.sqrt((np.maximum(q, 0.0) ** 2).sum(1))
        inside = np.minimum(q.max(1), 0.0)
        return outside + inside

    def __repr__(self):
        return "Cylinder(%d, %s, %g, %g, %g)" % (self.axis, list(self.center), self.radius, self.lo, self.hi)


class Wedge:
    """Axis-aligned box [lo, hi] cut by a plane: the part of the box with normal . x < offset.  `normal` is
    the outward normal of the cut face; it is normalised in float64, then rounded to fp32, which is what
    the C ABI stores (center = normal, radius = offset)."""

    kind = WEDGE

    def __init__(self, lo, hi, normal, offset):
        self.lo, self.hi = _vec3(lo), _vec3(hi)
        n = np.asarray(normal, np.float64).reshape(3)
        length = math.sqrt(float((n * n).sum()))
        if not (length > 0.0 and math.isfinite(length)):
            raise ValueError("normal must be finite and not zero")
        self.normal = (n / length).astype(np.float32)
        self.offset = np.float32(offset)

    @classmethod
    def ramp(cls, lo, hi, run, up, rising=True):
        """The box [lo, hi] cut by the plane through its lower edge (along `up`) at one end of axis `run`
        and its upper edge at the other: a slope that rises towards hi[run] (`rising`) or falls."""
        run, up = int(run), int(up)
        if run not in (0, 1, 2) or up not in (0, 1, 2) or run == up:
            raise ValueError("run and up must be two different axes out of 0, 1, 2")
        lo64, hi64 = _vec3(lo).astype(np.float64), _vec3(hi).astype(np.float64)
        length, height = hi64[run] - lo64[run], hi64[up] - lo64[up]
        n = np.zeros(3)
        n[up] = length
        n[run] = -height if rising else height
        n /= math.sqrt(float((n * n).sum()))
        foot = lo64.copy()                      # a point of the plane: the lower edge
        foot[run] = lo64[run] if rising else hi64[run]
        return cls(lo, hi, n, float((n * foot).sum()))

    def as_struct(self):
        s = SphObstacle()
        s.kind = WEDGE
        s.center[:] = [float(v) for v in self.normal]
        s.radius = float(self.offset)
        s.lo[:] = [float(v) for v in self.lo]
        s.hi[:] = [float(v) for v in self.hi]
        return s

    def signed_distance(self, points):
        """The larger of the box's distance and the plane's (float64): negative exactly inside, a lower
        bound of the distance outside."""
        p = _points(points)
        plane = p @ self.normal.astype(np.float64) - float(self.offset)
        return np.maximum(Box(self.lo, self.hi).signed_distance(p), plane)

    def __repr__(self):
        return "Wedge(%s, %s, %s, %g)" % (list(self.lo), list(self.hi), list(self.normal), self.offset)


def _wedge_from_struct(s):
    w = Wedge.__new__(Wedge)                    # the stored fields as they are: no second normalisation
    w.lo, w.hi = _vec3(list(s.lo)), _vec3(list(s.hi))
    w.normal, w.offset = _vec3(list(s.center)), np.float32(s.radius)
    return w


def from_struct(s):
    """The Sphere / Box / Cylinder / Wedge an sph_hip_obstacle describes."""
    if s.kind == SPHERE:
        return Sphere(list(s.center), s.radius)
    if s.kind == BOX:
        return Box(list(s.lo), list(s.hi))
    if s.kind == CYLINDER:
        return Cylinder(s.axis, list(s.center), s.radius, s.lo[s.axis], s.hi[s.axis])
    if s.kind == WEDGE:
        return _wedge_from_struct(s)
    raise ValueError("unknown obstacle kind %d" % s.kind)


def as_array(obstacles):
    """A ctypes array of sph_hip_obstacle for a list of obstacles (or of structs)."""
    obstacles = list(obstacles)
    arr = (SphObstacle * max(1, len(obstacles)))()
    for i, o in enumerate(obstacles):
        arr[i] = o if isinstance(o, SphObstacle) else o.as_struct()
    return arr, len(obstacles)


class SphObstacleMotion(C.Structure):
    """Mirror of sph_hip_obstacle_motion (include/sph_hip.h): 20 bytes, field order is ABI."""

    _fields_ = [("velocity", C.c_float * 3), ("start", C.c_float), ("stop", C.c_float)]


class Motion:
    """An obstacle translating at `velocity` (position units per unit of time_step) while the motion
    clock is in [start, stop], at rest before and after; stop may be math.inf."""

    def __init__(self, velocity, start=0.0, stop=math.inf):
        self.velocity = _vec3(velocity)
        self.start, self.stop = np.float32(start), np.float32(stop)

    def as_struct(self):
        s = SphObstacleMotion()
        s.velocity[:] = [float(v) for v in self.velocity]
        s.start, s.stop = float(self.start), float(self.stop)
        return s

    def moves(self):
        return bool((self.velocity != 0).any())

    def displacement(self, clock):
        """The shift at motion clock `clock`, float32[3], in the C ABI's fp32 arithmetic."""
        tau = np.float32(clock)
        s = (self.start if tau < self.start else self.stop if tau > self.stop else tau) - self.start
        with np.errstate(over="ignore"):
            return (self.velocity * np.float32(s)).astype(np.float32)

    def __eq__(self, other):
        return isinstance(other, Motion) and bytes(self.as_struct()) == bytes(other.as_struct())

    def __repr__(self):
        return "Motion(%s, %g, %g)" % (list(self.velocity), self.start, self.stop)


def motion_from_struct(s):
    return Motion(list(s.velocity), s.start, s.stop)


def as_motion_array(motions):
    """A ctypes array of sph_hip_obstacle_motion for a list of Motion, struct or None (at rest)."""
    motions = list(motions)
    arr = (SphObstacleMotion * max(1, len(motions)))()
    for i, m in enumerate(motions):
        if m is None:
            m = Motion((0.0, 0.0, 0.0))
        arr[i] = m if isinstance(m, SphObstacleMotion) else m.as_struct()
    return arr, len(motions)


MAX_PATH_KEYS = 16384             # SPH_HIP_MAX_PATH_KEYS


class SphMotionKey(C.Structure):
    """Mirror of sph_hip_motion_key (include/sph_hip.h): 16 bytes, field order is ABI."""

    _fields_ = [("t", C.c_float), ("d", C.c_float * 3)]


class SphMotionPath(C.Structure):
    """Mirror of sph_hip_motion_path (include/sph_hip.h): 16 bytes, field order is ABI."""

    _fields_ = [("first", C.c_int32), ("count", C.c_int32), ("start", C.c_float), ("cycle", C.c_int32)]


class MotionPath:
    """An obstacle following a keyframed displacement (sph_hip_set_obstacle_paths): `displacements`[k]
    (position units) at `times`[k] after the motion clock reaches `start`, linear in between, held
    before and after - or, with `cycle`, repeated with period times[-1].  times[0] is 0, times rise
    strictly, at least two keys; a cyclic path ends at the displacement it begins with."""

    def __init__(self, times, displacements, start=0.0, cycle=False):
        self.times = np.array(times, np.float32).reshape(-1)
        self.displacements = np.array(displacements, np.float32).reshape(-1, 3)
        if self.times.size != self.displacements.shape[0]:
            raise ValueError("one displacement per time")
        self.start, self.cycle = np.float32(start), bool(cycle)

    @classmethod
    def sine(cls, amplitude_xyz, period, keys=64, start=0.0):
        """One period of amplitude * sin(2 pi t / period), cyclic: `keys` segments of equal length, the
        closing key a bitwise copy of the first.  Between keys the path is linear, so it stays within
        amplitude * (2 pi / keys)**2 / 8 of the sine."""
        keys = int(keys)
        if keys < 2:
            raise ValueError("keys must be at least 2")
        amp = np.asarray(amplitude_xyz, np.float64).reshape(3)
        phase = np.arange(keys + 1, dtype=np.float64) / keys
        times = (phase * float(period)).astype(np.float32)
        disp = (np.sin(2.0 * math.pi * phase)[:, None] * amp[None, :]).astype(np.float32)
        times[0] = 0.0
        disp[-1] = disp[0]
        return cls(times, disp, start, True)

    @classmethod
    def stroke(cls, displacement_xyz, duration, start=0.0):
        """Two keys: from rest to `displacement_xyz` in `duration`, and held there."""
        return cls([0.0, duration], [(0.0, 0.0, 0.0), tuple(displacement_xyz)], start, False)

    def segment(self, clock):
        """(j, u, clamped): the segment in force at motion clock `clock`, the path time, and whether
        that time was clamped - the contract's fp32 arithmetic (csrc/obstacle_policy.h: path_segment)."""
        f = np.float32
        t = self.times
        T = t[-1]
        with np.errstate(all="ignore"):
            u = f(f(clock) - self.start)
            clamped = bool(u < 0)
            if u < 0:
                u = f(0)
            if not self.cycle:
                if u > T:
                    u, clamped = T, True
            else:
                if u >= T:
                    k = f(np.floor(f(u / T)))
                    u = f(u - f(k * T))
                if u < 0:
                    u = f(0)
                if u >= T:
                    u = f(0)
        j = int(np.searchsorted(t, u, side="right")) - 1
        return min(max(j, 0), t.size - 2), f(u), clamped

    def displacement_at(self, clock):
        """The shift at motion clock `clock`, float32[3], in the C ABI's fp32 arithmetic."""
        f = np.float32
        j, u, _ = self.segment(clock)
        t, d = self.times, self.displacements
        with np.errstate(all="ignore"):
            w = f(f(u - t[j]) / f(t[j + 1] - t[j]))
            return (d[j] + (w * (d[j + 1] - d[j]).astype(f)).astype(f)).astype(f)

    def velocity_at(self, clock):
        """The velocity of the segment in force at `clock`, float32[3]; 0 while the path time is clamped."""
        f = np.float32
        j, _, clamped = self.segment(clock)
        if clamped:
            return np.zeros(3, f)
        t, d = self.times, self.displacements
        with np.errstate(all="ignore"):
            return ((d[j + 1] - d[j]).astype(f) / f(t[j + 1] - t[j])).astype(f)

    def __eq__(self, other):
        return (isinstance(other, MotionPath) and self.times.tobytes() == other.times.tobytes() and
                self.displacements.tobytes() == other.displacements.tobytes() and
                self.start.tobytes() == other.start.tobytes() and self.cycle == other.cycle)

    def __repr__(self):
        return "MotionPath(%d keys to t = %g, start %g%s)" % (self.times.size, self.times[-1], self.start,
                                                              ", cyclic" if self.cycle else "")


def as_path_arrays(paths):
    """(ctypes array of sph_hip_motion_path, n, ctypes array of sph_hip_motion_key, n_keys) for a list of
    MotionPath or None (no path): the keys of all paths one after the other."""
    paths = list(paths)
    n_keys = sum(p.times.size for p in paths if p is not None)
    arr = (SphMotionPath * max(1, len(paths)))()
    keys = np.zeros((max(1, n_keys), 4), np.float32)
    first = 0
    for i, p in enumerate(paths):
        if p is None:
            continue
        k = p.times.size
        arr[i].first, arr[i].count, arr[i].start, arr[i].cycle = first, k, float(p.start), int(p.cycle)
        keys[first:first + k, 0] = p.times
        keys[first:first + k, 1:] = p.displacements
        first += k
    karr = (SphMotionKey * max(1, n_keys)).from_buffer_copy(keys.tobytes())
    return arr, len(paths), karr, n_keys


def paths_from_arrays(arr, n, karr):
    """The list of MotionPath / None that n sph_hip_motion_path structs over the keys `karr` describe."""
    out = []
    for i in range(n):
        s = arr[i]
        if s.count == 0:
            out.append(None)
            continue
        ks = [karr[s.first + j] for j in range(s.count)]
        out.append(MotionPath([k.t for k in ks], [list(k.d) for k in ks], s.start, s.cycle != 0))
    return out


class SphObstacleRotation(C.Structure):
    """Mirror of sph_hip_obstacle_rotation (csrc/obstacle_policy.h): 32 bytes, field order is fixed."""

    _fields_ = [("axis", C.c_int32), ("pivot", C.c_float * 3), ("angle", C.c_float), ("rate", C.c_float),
                ("start", C.c_float), ("stop", C.c_float)]


class Rotation:
    """An obstacle turned about the coordinate axis `axis` (0 x, 1 y, 2 z) through `pivot`: by `angle` radians
    (right-handed about +axis) at the motion clock's start, and on at `rate` radians per unit of time_step
    while the clock is in [start, stop]; stop may be math.inf.  The obstacle's own fields describe it in the
    frame that turns with it, which coincides with the world at angle 0."""

    def __init__(self, axis, pivot, angle=0.0, rate=0.0, start=0.0, stop=math.inf):
        if int(axis) not in (0, 1, 2):
            raise ValueError("axis must be 0, 1 or 2")
        self.axis = int(axis)
        self.pivot = _vec3(pivot)
        self.angle, self.rate = np.float32(angle), np.float32(rate)
        self.start, self.stop = np.float32(start), np.float32(stop)

    def as_struct(self):
        s = SphObstacleRotation()
        s.axis = self.axis
        s.pivot[:] = [float(v) for v in self.pivot]
        s.angle, s.rate = float(self.angle), float(self.rate)
        s.start, s.stop = float(self.start), float(self.stop)
        return s

    def posed(self):
        return bool(self.angle != 0 or self.rate != 0)

    def rotates(self):
        return bool(self.rate != 0)

    def angle_at(self, clock):
        """theta at motion clock `clock`, in the contract's fp32 arithmetic."""
        tau = np.float32(clock)
        s = np.float32((self.start if tau < self.start else self.stop if tau > self.stop else tau) - self.start)
        with np.errstate(over="ignore", invalid="ignore"):
            return np.float32(self.angle + np.float32(self.rate * s))

    def _turn(self, points, theta, sign):
        x = _points(points).copy()
        a = self.axis
        u, w = (a + 1) % 3, (a + 2) % 3
        pv = self.pivot.astype(np.float64)
        cs, sn = math.cos(float(theta)), sign * math.sin(float(theta))
        du, dw = x[:, u] - pv[u], x[:, w] - pv[w]
        x[:, u] = pv[u] + (cs * du + sn * dw)
        x[:, w] = pv[w] + (cs * dw - sn * du)
        return x

    def to_body(self, points, clock=0.0):
        """World points in the frame fixed to the solid at motion clock `clock` (float64, for building
        scenes; the contract's fp32 form is csrc/obstacle_policy.h)."""
        return self._turn(points, self.angle_at(clock), 1.0)

    def to_world(self, points, clock=0.0):
        """Points of the solid's frame in the world at motion clock `clock` (float64)."""
        return self._turn(points, self.angle_at(clock), -1.0)

    def __eq__(self, other):
        return isinstance(other, Rotation) and bytes(self.as_struct()) == bytes(other.as_struct())

    def __repr__(self):
        return "Rotation(%d, %s, %g, %g, %g, %g)" % (self.axis, list(self.pivot), self.angle, self.rate, self.start,
                                                     self.stop)


def rotation_from_struct(s):
    return Rotation(s.axis, list(s.pivot), s.angle, s.rate, s.start, s.stop)


def as_rotation_array(rotations):
    """A ctypes array of sph_hip_obstacle_rotation for a list of Rotation, struct or None (unposed: all
    zero with stop = inf)."""
    rotations = list(rotations)
    arr = (SphObstacleRotation * max(1, len(rotations)))()
    for i, r in enumerate(rotations):
        if r is None:
            r = Rotation(0, (0.0, 0.0, 0.0))
        arr[i] = r if isinstance(r, SphObstacleRotation) else r.as_struct()
    return arr, len(rotations)


class SphBody(C.Structure):
    """Mirror of sph_hip_body (include/sph_hip.h): 56 bytes, field order is ABI."""

    _fields_ = [("mass", C.c_float), ("velocity", C.c_float * 3), ("accel", C.c_float * 3), ("free_axes", C.c_uint32),
                ("travel_lo", C.c_float * 3), ("travel_hi", C.c_float * 3)]


class SphBodyState(C.Structure):
    """Mirror of sph_hip_body_state (include/sph_hip.h): 40 bytes, field order is ABI."""

    _fields_ = [("displacement", C.c_float * 3), ("velocity", C.c_float * 3), ("skipped", C.c_int64),
                ("steps", C.c_int64)]


class Body:
    """An obstacle that the fluid's loads move (sph_hip_set_bodies): `mass`, the initial `velocity`
    (position units per unit of time_step), `accel` (body force per unit mass, gravity say), `free` (which
    components may move) and the limits of its displacement, travel_lo <= 0 <= travel_hi per component -
    the stops that stand in for walls and floor.  The coupling lags one step and treats the solid as
    infinitely heavy within a step: use bodies several times heavier than the fluid they displace."""

    def __init__(self, mass, velocity=(0.0, 0.0, 0.0), accel=(0.0, 0.0, 0.0), free=(True, True, True),
                 travel_lo=(-math.inf,) * 3, travel_hi=(math.inf,) * 3):
        self.mass = np.float32(mass)
        self.velocity, self.accel = _vec3(velocity), _vec3(accel)
        self.free = tuple(bool(f) for f in free)
        if len(self.free) != 3:
            raise ValueError("free takes three values")
        self.travel_lo, self.travel_hi = _vec3(travel_lo), _vec3(travel_hi)

    @property
    def free_axes(self):
        return sum(1 << c for c in range(3) if self.free[c])

    def as_struct(self):
        s = SphBody()
        s.mass = float(self.mass)
        s.velocity[:] = [float(v) for v in self.velocity]
        s.accel[:] = [float(v) for v in self.accel]
        s.free_axes = self.free_axes
        s.travel_lo[:] = [float(v) for v in self.travel_lo]
        s.travel_hi[:] = [float(v) for v in self.travel_hi]
        return s

    def __eq__(self, other):
        return isinstance(other, Body) and bytes(self.as_struct()) == bytes(other.as_struct())

    def __repr__(self):
        return "Body(%g, %s, %s, %s, %s, %s)" % (self.mass, list(self.velocity), list(self.accel), self.free,
                                                 list(self.travel_lo), list(self.travel_hi))


def body_from_struct(s):
    """The Body an sph_hip_body describes; None for an entry that is not a body (mass == 0)."""
    if s.mass == 0:
        return None
    return Body(s.mass, list(s.velocity), list(s.accel), [bool(s.free_axes >> c & 1) for c in range(3)],
                list(s.travel_lo), list(s.travel_hi))


def as_body_array(bodies):
    """A ctypes array of sph_hip_body for a list of Body, struct or None (not a body: all zero)."""
    bodies = list(bodies)
    arr = (SphBody * max(1, len(bodies)))()
    for i, b in enumerate(bodies):
        if b is not None:
            arr[i] = b if isinstance(b, SphBody) else b.as_struct()
    return arr, len(bodies)


def inside_any(points, obstacles, rotations=None):
    """Boolean mask of the points strictly inside any of the obstacles (float64 distances); with
    `rotations` (a Rotation or None per obstacle), inside each as it stands at the motion clock's start."""
    p = _points(points)
    mask = np.zeros(p.shape[0], bool)
    obstacles = list(obstacles)
    rotations = list(rotations) if rotations else [None] * len(obstacles)
    if len(rotations) != len(obstacles):
        raise ValueError("rotations must hold one entry (a Rotation or None) per obstacle")
    for o, r in zip(obstacles, rotations):
        x = p if r is None or not r.posed() else r.to_body(p)
        mask |= o.signed_distance(x) < 0.0
    return mask
