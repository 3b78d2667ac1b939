"""Viscous stress (include/sph_hip.h: sph_hip_set_viscous_stress): a pairwise, momentum-conserving viscous force of a
stated dynamic viscosity.  SPH.setViscousStress(mu) sets a constant one; SPH.setViscousStress(mu, law) multiplies mu
per particle by a ViscosityLaw's factor of a carried channel (scalars.py): a table of keys, linear between them and
constant beyond its ends.  The arithmetic of a step is in csrc/viscous_policy.h."""
import ctypes as C
import math

import numpy as np

MAX_KEYS = 16         # SPH_HIP_MAX_VISCOSITY_KEYS
MAX_SWEEPS = 64       # SPH_HIP_MAX_VISCOUS_SWEEPS (SPH.setViscousSolver)


class SphViscosityLaw(C.Structure):
    """Mirror of sph_hip_viscosity_law (include/sph_hip.h): 136 bytes."""

    _fields_ = [("channel", C.c_int32), ("n_keys", C.c_int32), ("value", C.c_float * MAX_KEYS),
                ("factor", C.c_float * MAX_KEYS)]


class ViscosityLaw:
    """factor(x) of the carried channel `channel`: `values` are the keys (2 to 16 of them, strictly ascending),
    `factors` what mu is multiplied by at each (>= 0).  Below the first key and for a NaN the first factor holds,
    from the last key on the last, between two keys the straight line through them.  The library checks the rules
    when the law is handed to SPH.setViscousStress."""

    __slots__ = ("channel", "values", "factors")

    def __init__(self, channel, values, factors):
        self.channel = int(channel)
        self.values = tuple(float(np.float32(v)) for v in np.asarray(values, np.float64).reshape(-1))
        self.factors = tuple(float(np.float32(f)) for f in np.asarray(factors, np.float64).reshape(-1))
        if len(self.values) != len(self.factors):
            raise ValueError("a ViscosityLaw needs as many factors as values")
        if len(self.values) > MAX_KEYS:
            raise ValueError("a ViscosityLaw holds at most %d keys" % MAX_KEYS)

    @classmethod
    def tabulate(cls, channel, fn, lo, hi, keys=MAX_KEYS):
        """fn at `keys` evenly spaced values from lo to hi, evaluated on the host in float64."""
        x = np.linspace(float(lo), float(hi), int(keys))
        return cls(channel, x, [fn(float(v)) for v in x])

    @classmethod
    def exponential(cls, channel, reference, rate, lo, hi, keys=MAX_KEYS):
        """exp(-rate * (x - reference)): 1 at the reference, falling by the factor e per 1 / rate above it - oil that
        thins as it warms, lava that stiffens as it cools."""
        return cls.tabulate(channel, lambda x: math.exp(-float(rate) * (x - float(reference))), lo, hi, keys)

    @classmethod
    def arrhenius(cls, channel, activation, reference, lo, hi, keys=MAX_KEYS):
        """exp(activation * (1 / x - 1 / reference)), x an absolute temperature (lo > 0): 1 at the reference,
        activation = E / R in the channel's units."""
        if not float(lo) > 0.0:
            raise ValueError("an Arrhenius law needs absolute temperatures: lo > 0")
        return cls.tabulate(channel, lambda x: math.exp(float(activation) * (1.0 / x - 1.0 / float(reference))), lo, hi,
                            keys)

    def _key(self):
        return (self.channel, self.values, self.factors)

    def __eq__(self, other):
        return isinstance(other, ViscosityLaw) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "ViscosityLaw(channel=%r, values=%r, factors=%r)" % self._key()

    def factor(self, x):
        """The law at x, in float64 (the device's fp32 arithmetic is restated in tests/viscous_emulation.py)."""
        v, f = self.values, self.factors
        if not x > v[0]:
            return f[0]
        if x >= v[-1]:
            return f[-1]
        k = int(np.searchsorted(v, x, side="right")) - 1
        return f[k] + (x - v[k]) / (v[k + 1] - v[k]) * (f[k + 1] - f[k])

    def to_struct(self):
        q = SphViscosityLaw()
        q.channel, q.n_keys = self.channel, len(self.values)
        for k, (v, f) in enumerate(zip(self.values, self.factors)):
            q.value[k], q.factor[k] = v, f
        return q


def from_struct(q):
    n = int(q.n_keys)
    return ViscosityLaw(q.channel, [q.value[k] for k in range(n)], [q.factor[k] for k in range(n)])
