"""Gauges (include/sph_hip.h: sph_hip_set_gauges): fixed instruments that read the field inside the step.

PointGauge, ColumnGauge, SectionGauge, PressureGauge and PressurePatch describe one instrument each; SPH.setGauges takes a list of them,
SPH.readGauges evaluates them now, SPH.recordGauges keeps one row of readings per recorded step on the device
and SPH.getGaugeRecord returns the rows as a GaugeRecord.  The arithmetic of every reading is in
csrc/gauge_policy.h."""
import collections
import ctypes as C

import numpy as np

POINT, COLUMN, SECTION = 0, 1, 2       # SPH_HIP_GAUGE_*
PRESSURE, PRESSURE_PATCH = 4, 5        # (3 is not a kind: the library refuses it as unknown)
MAX_GAUGES = 4096                      # SPH_HIP_MAX_GAUGES
MAX_GAUGE_PROBES = 4096                # SPH_HIP_MAX_GAUGE_PROBES

# sph_hip_gauge_reading as a numpy record: 24 bytes
READING = np.dtype([("v", np.float32, (4,)), ("n", np.int32), ("k", np.int32)])


class SphGauge(C.Structure):
    """Mirror of sph_hip_gauge (include/sph_hip.h): 40 bytes."""

    _fields_ = [("kind", C.c_int32), ("axis", C.c_int32), ("origin", C.c_float * 3), ("spacing", C.c_float * 2),
                ("count", C.c_int32 * 2), ("iso", C.c_float)]


def _struct(kind, axis, origin, spacing=(0.0, 0.0), count=(0, 0), iso=0.0):
    g = SphGauge()
    g.kind, g.axis, g.iso = kind, int(axis), float(iso)
    for c in range(3):
        g.origin[c] = float(origin[c])
    for c in range(2):
        g.spacing[c] = float(spacing[c])
        g.count[c] = int(count[c])
    return g


class PointGauge(collections.namedtuple("PointGauge", ["point"])):
    """The sampler's density, Shepard velocity and member count at `point`."""
    __slots__ = ()

    def to_struct(self):
        return _struct(POINT, 0, self.point)


class ColumnGauge(collections.namedtuple("ColumnGauge", ["base", "axis", "spacing", "samples", "iso"])):
    """`samples` probes `spacing` apart up `axis` from `base`: the level of the topmost crossing of `iso`, the
    wet depth and the two densities the level was interpolated from."""
    __slots__ = ()

    def to_struct(self):
        return _struct(COLUMN, self.axis, self.base, (self.spacing, 0.0), (self.samples, 0), self.iso)


class SectionGauge(collections.namedtuple("SectionGauge", ["corner", "axis", "spacing", "shape", "iso"])):
    """A lattice of shape = (nu, nv) probes, spacing = (su, sv) apart along the two axes that are not `axis` (in
    ascending axis order), on the plane through `corner` with normal `axis`: the mass flow through it along the
    normal, its wetted area and the sum of its densities."""
    __slots__ = ()

    def to_struct(self):
        return _struct(SECTION, self.axis, self.corner, self.spacing, self.shape, self.iso)


class PressureGauge(collections.namedtuple("PressureGauge", ["point"])):
    """The Shepard-normalised pressure at `point` - the members' (rho_j - rho0) * stiffness weighted by the
    sampler's terms - with the sampler's density, the raw pressure sum and the member count."""
    __slots__ = ()

    def to_struct(self):
        return _struct(PRESSURE, 0, self.point)


class PressurePatch(collections.namedtuple("PressurePatch", ["corner", "axis", "spacing", "shape", "iso"])):
    """A sensor face or wall panel: SectionGauge's rectangle of probes on the plane through `corner` with normal
    `axis`.  Over the probes whose density exceeds `iso`: the force along the normal (the sum of their pressures
    times the area of a probe), the wetted area, the mean pressure and the sum of the densities."""
    __slots__ = ()

    def to_struct(self):
        return _struct(PRESSURE_PATCH, self.axis, self.corner, self.spacing, self.shape, self.iso)


def from_struct(g):
    o = tuple(g.origin)
    if g.kind == POINT:
        return PointGauge(o)
    if g.kind == COLUMN:
        return ColumnGauge(o, g.axis, g.spacing[0], g.count[0], g.iso)
    if g.kind == SECTION:
        return SectionGauge(o, g.axis, tuple(g.spacing), tuple(g.count), g.iso)
    if g.kind == PRESSURE:
        return PressureGauge(o)
    if g.kind == PRESSURE_PATCH:
        return PressurePatch(o, g.axis, tuple(g.spacing), tuple(g.count), g.iso)
    raise ValueError("unknown gauge kind %d" % g.kind)


def as_array(gauges):
    """(SphGauge array or None, n) of a list of PointGauge / ColumnGauge / SectionGauge / PressureGauge /
    PressurePatch / SphGauge."""
    gauges = list(gauges)
    n = len(gauges)
    if n == 0:
        return None, 0
    arr = (SphGauge * n)()
    for i, g in enumerate(gauges):
        arr[i] = g if isinstance(g, SphGauge) else g.to_struct()
    return arr, n


def _pressure_column(readings, i, gauge):
    """where gauge i keeps its pressure: a point's v[0], a patch's mean v[2].  The kind is `gauge` (a kind value
    or a PressureGauge / PressurePatch) where given, else the one SPH.readGauges / getGaugeRecord noted."""
    kind = gauge
    if kind is None:
        if readings.kinds is None:
            raise ValueError("the kinds of these readings are not known: pass the gauge")
        kind = readings.kinds[i]
    if kind == PRESSURE or isinstance(kind, PressureGauge):
        return 0
    if kind == PRESSURE_PATCH or isinstance(kind, PressurePatch):
        return 2
    raise ValueError("gauge %d is not a pressure gauge" % i)


class GaugeReadings(collections.namedtuple("GaugeReadings", ["v", "n", "k"])):
    """sph_hip_read_gauges' answer, one entry per gauge in list order: v float32 (n, 4), n and k int32 (n,).
    `kinds` (not a field) holds the gauges' kinds where SPH.readGauges made the readings."""
    kinds = None

    def pressure(self, i, gauge=None):
        """the pressure of gauge i: a PressureGauge's reading, or the mean over the wet probes of a PressurePatch"""
        return self.v[i, _pressure_column(self, i, gauge)]

    def force(self, i):
        """a pressure patch's force along its normal"""
        return self.v[i, 0]


class GaugeRecord(collections.namedtuple("GaugeRecord", ["steps", "v", "n", "k"])):
    """The rows of a gauge recording (sph_hip_get_gauge_record): steps int32 (rows,), the steps completed since
    recordGauges when each row was read (row 0: the state at the call); the raw readings v float32
    (rows, gauges, 4), n and k int32 (rows, gauges).  The helpers return the time series of gauge i.  `kinds`
    (not a field) holds the gauges' kinds where SPH.getGaugeRecord made the record."""
    kinds = None

    def level(self, i):
        """a column's free-surface level along its axis"""
        return self.v[:, i, 0]

    def depth(self, i):
        """a column's wet depth: wet probes times spacing"""
        return self.v[:, i, 1]

    def flow(self, i):
        """a section's mass flow along its normal"""
        return self.v[:, i, 0]

    def probe(self, i):
        """a point gauge's (density, velocity[3]) series"""
        return self.v[:, i, 0], self.v[:, i, 1:4]

    def pressure(self, i, gauge=None):
        """the pressure series of gauge i: a PressureGauge's reading, or the mean over the wet probes of a
        PressurePatch"""
        return self.v[:, i, _pressure_column(self, i, gauge)]

    def force(self, i):
        """a pressure patch's force along its normal: the sum of its wet probes' pressures times a probe's area"""
        return self.v[:, i, 0]
