"""Ports (include/sph_hip.h: sph_hip_set_ports): inflow emitters and outflow sinks.

Emitter and Sink describe one port each; SPH.setPorts takes a list of each, SPH.getPorts returns them with the
PortTotals.  The schedule, the lattice points, the ids and the sink test are in csrc/port_policy.h."""
import collections
import ctypes as C

import numpy as np

MAX_EMITTERS = 8               # SPH_HIP_MAX_EMITTERS
MAX_SINKS = 8                  # SPH_HIP_MAX_SINKS
MAX_EMITTER_POINTS = 65536     # SPH_HIP_MAX_EMITTER_POINTS


class SphEmitter(C.Structure):
    """Mirror of sph_hip_emitter (include/sph_hip.h): 56 bytes."""

    _fields_ = [("axis", C.c_int32), ("origin", C.c_float * 3), ("count", C.c_int32 * 2), ("spacing", C.c_float),
                ("velocity", C.c_float * 3), ("mass", C.c_float), ("first", C.c_int32), ("every", C.c_int32),
                ("layers", C.c_int32)]


class SphSink(C.Structure):
    """Mirror of sph_hip_sink (include/sph_hip.h): 24 bytes."""

    _fields_ = [("lo", C.c_float * 3), ("hi", C.c_float * 3)]


def _f3(v):
    return tuple(float(x) for x in np.asarray(v, np.float32).reshape(3))


class Emitter:
    """A lattice of count = (nu, nw) points `spacing` apart on the plane with normal `axis` through `origin`
    (the lattice axes are (axis + 1) % 3 and (axis + 2) % 3), emitted as one layer with `velocity` and `mass` in
    port step `first` and every `every`-th after it, `layers` times (-1: without limit)."""

    __slots__ = ("axis", "origin", "count", "spacing", "velocity", "mass", "first", "every", "layers")

    def __init__(self, axis, origin, count, spacing, velocity, mass, first=0, every=1, layers=-1):
        self.axis = int(axis)
        self.origin = _f3(origin)
        self.count = (int(count[0]), int(count[1]))
        self.spacing = float(np.float32(spacing))
        self.velocity = _f3(velocity)
        self.mass = float(np.float32(mass))
        self.first, self.every, self.layers = int(first), int(every), int(layers)

    @property
    def points(self):
        return self.count[0] * self.count[1]

    def _key(self):
        return tuple(getattr(self, name) for name in self.__slots__)

    def __eq__(self, other):
        return isinstance(other, Emitter) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "Emitter(%s)" % ", ".join("%s=%r" % (name, getattr(self, name)) for name in self.__slots__)

    def to_struct(self):
        e = SphEmitter()
        e.axis, e.spacing, e.mass = self.axis, self.spacing, self.mass
        e.first, e.every, e.layers = self.first, self.every, self.layers
        for c in range(3):
            e.origin[c] = self.origin[c]
            e.velocity[c] = self.velocity[c]
        e.count[0], e.count[1] = self.count
        return e


class Sink:
    """The box lo <= x < hi: particles inside it at the start of a step are removed."""

    __slots__ = ("lo", "hi")

    def __init__(self, lo, hi):
        self.lo, self.hi = _f3(lo), _f3(hi)

    def __eq__(self, other):
        return isinstance(other, Sink) and (self.lo, self.hi) == (other.lo, other.hi)

    def __hash__(self):
        return hash((self.lo, self.hi))

    def __repr__(self):
        return "Sink(lo=%r, hi=%r)" % (self.lo, self.hi)

    def to_struct(self):
        k = SphSink()
        for c in range(3):
            k.lo[c] = self.lo[c]
            k.hi[c] = self.hi[c]
        return k


def emitter_from_struct(e):
    return Emitter(e.axis, tuple(e.origin), tuple(e.count), e.spacing, tuple(e.velocity), e.mass, e.first, e.every,
                   e.layers)


def sink_from_struct(k):
    return Sink(tuple(k.lo), tuple(k.hi))


def as_emitter_array(emitters):
    """(SphEmitter array or None, n) of a list of Emitter / SphEmitter."""
    emitters = list(emitters)
    n = len(emitters)
    if n == 0:
        return None, 0
    arr = (SphEmitter * n)()
    for i, e in enumerate(emitters):
        arr[i] = e if isinstance(e, SphEmitter) else e.to_struct()
    return arr, n


def as_sink_array(sinks):
    """(SphSink array or None, n) of a list of Sink / SphSink."""
    sinks = list(sinks)
    n = len(sinks)
    if n == 0:
        return None, 0
    arr = (SphSink * n)()
    for i, k in enumerate(sinks):
        arr[i] = k if isinstance(k, SphSink) else k.to_struct()
    return arr, n


# sph_hip_get_ports' totals: emitted int64 (emitters,), removed int64 (sinks,), live and next_id ints
PortTotals = collections.namedtuple("PortTotals", ["emitted", "removed", "live", "next_id"])
