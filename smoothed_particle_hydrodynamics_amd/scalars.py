"""Carried scalars (include/sph_hip.h: sph_hip_set_scalars): four channels per particle - a temperature, a dye
concentration, a salinity - that move with the fluid and diffuse between neighbours.

SPH.setScalars gives every particle its values and every channel its diffusivity, SPH.getScalars reads them back
in particle order, SPH.setScalarSources takes a list of ScalarSource, SPH.sampleScalars and
SPH.sampleScalarLattice interpolate the channels at probes.  The arithmetic of a step is in csrc/scalar_policy.h.
SPH.setBuoyancy takes a Buoyancy: the channels then change a particle's weight (csrc/buoyancy_policy.h)."""
import ctypes as C

import numpy as np

CHANNELS = 4          # SPH_HIP_SCALAR_CHANNELS
MAX_SOURCES = 8       # SPH_HIP_MAX_SCALAR_SOURCES
HOLD, ADD = 0, 1      # SPH_HIP_SCALAR_HOLD / _ADD


class SphScalarSource(C.Structure):
    """Mirror of sph_hip_scalar_source (include/sph_hip.h): 36 bytes."""

    _fields_ = [("lo", C.c_float * 3), ("hi", C.c_float * 3), ("channel", C.c_int32), ("kind", C.c_int32),
                ("value", C.c_float)]


def _f3(v):
    return tuple(float(x) for x in np.asarray(v, np.float32).reshape(3))


class ScalarSource:
    """A box lo < x < hi (strictly inside) in which, after every step's diffusion, `channel` is set to `value`
    (kind HOLD: a heated plate, a dye injector) or raised by value * dt (kind ADD: a heater of a given power)."""

    __slots__ = ("lo", "hi", "channel", "kind", "value")

    def __init__(self, lo, hi, channel, kind, value):
        self.lo, self.hi = _f3(lo), _f3(hi)
        self.channel, self.kind = int(channel), int(kind)
        self.value = float(np.float32(value))

    @classmethod
    def hold(cls, lo, hi, channel, value):
        return cls(lo, hi, channel, HOLD, value)

    @classmethod
    def add(cls, lo, hi, channel, value):
        return cls(lo, hi, channel, ADD, value)

    def _key(self):
        return tuple(getattr(self, name) for name in self.__slots__)

    def __eq__(self, other):
        return isinstance(other, ScalarSource) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "ScalarSource(%s)" % ", ".join("%s=%r" % (name, getattr(self, name)) for name in self.__slots__)

    def to_struct(self):
        q = SphScalarSource()
        for c in range(3):
            q.lo[c] = self.lo[c]
            q.hi[c] = self.hi[c]
        q.channel, q.kind, q.value = self.channel, self.kind, self.value
        return q


def from_struct(q):
    return ScalarSource(tuple(q.lo), tuple(q.hi), q.channel, q.kind, q.value)


def as_array(sources):
    """(SphScalarSource array or None, n) of a list of ScalarSource / SphScalarSource."""
    sources = list(sources)
    n = len(sources)
    if n == 0:
        return None, 0
    arr = (SphScalarSource * n)()
    for i, q in enumerate(sources):
        arr[i] = q if isinstance(q, SphScalarSource) else q.to_struct()
    return arr, n


class SphBuoyancy(C.Structure):
    """Mirror of sph_hip_buoyancy (include/sph_hip.h): 44 bytes."""

    _fields_ = [("beta", C.c_float * 4), ("reference", C.c_float * 4), ("gravity", C.c_float * 3)]


def _pad4(v, what):
    v = np.asarray(v, np.float32).reshape(-1)
    if v.size > CHANNELS:
        raise ValueError("at most %d %s" % (CHANNELS, what))
    out = np.zeros(CHANNELS, np.float32)
    out[:v.size] = v
    return tuple(float(x) for x in out)


class Buoyancy:
    """The carried scalars change a particle's weight (include/sph_hip.h: buoyancy): with the excess
    s = sum over the channels of beta[c] * (T_c - reference[c]) a particle takes the acceleration (-s) * gravity
    on top of its own.  `beta` and `reference` are one value (channel 0) or up to four, padded with zeros;
    gravity=None takes the context's params.gravity when the setting is handed to SPH.setBuoyancy.  A positive
    beta lifts warm fluid, a negative one - a salinity - sinks it."""

    __slots__ = ("beta", "reference", "gravity")

    def __init__(self, beta, reference=(0.0, 0.0, 0.0, 0.0), gravity=None):
        self.beta = _pad4(beta, "betas")
        self.reference = _pad4(reference, "references")
        self.gravity = None if gravity is None else _f3(gravity)

    def _key(self):
        return (self.beta, self.reference, self.gravity)

    def __eq__(self, other):
        return isinstance(other, Buoyancy) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "Buoyancy(beta=%r, reference=%r, gravity=%r)" % self._key()

    def with_gravity(self, gravity):
        """This setting with `gravity` where it has none of its own."""
        return self if self.gravity is not None else Buoyancy(self.beta, self.reference, gravity)

    def to_struct(self):
        if self.gravity is None:
            raise ValueError("a Buoyancy without a gravity: give one, or hand it to SPH.setBuoyancy")
        b = SphBuoyancy()
        for c in range(CHANNELS):
            b.beta[c] = self.beta[c]
            b.reference[c] = self.reference[c]
        for a in range(3):
            b.gravity[a] = self.gravity[a]
        return b


def buoyancy_from_struct(b):
    return Buoyancy(tuple(b.beta), tuple(b.reference), tuple(b.gravity))


def pad_values(values, n=None):
    """`values`, (n,) or (n, c) with c <= 4, as float32 (n, 4) rows padded with zeros."""
    v = np.asarray(values, np.float32)
    if v.ndim == 1:
        v = v.reshape(-1, 1)
    if v.ndim != 2 or v.shape[1] > CHANNELS or v.shape[1] < 1:
        raise ValueError("scalar values are (n,) or (n, c) with 1 <= c <= %d" % CHANNELS)
    out = np.zeros((v.shape[0], CHANNELS), np.float32)
    out[:, :v.shape[1]] = v
    return out


def pad_diffusivity(diffusivity):
    """One diffusivity for every channel, or up to four of them, as float32 (4,) padded with zeros."""
    k = np.asarray(diffusivity, np.float32).reshape(-1)
    if k.size == 1:
        return np.full(CHANNELS, k[0], np.float32)
    if k.size > CHANNELS:
        raise ValueError("at most %d diffusivities" % CHANNELS)
    out = np.zeros(CHANNELS, np.float32)
    out[:k.size] = k
    return out
