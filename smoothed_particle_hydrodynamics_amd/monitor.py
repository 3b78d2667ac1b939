"""The step monitor's rows (include/sph_hip.h: step monitor): the layout of sph_hip_monitor_row and MonitorRecord,
what SPH.getMonitorRecord returns - the decoded arrays and the stability numbers formed from them.  The numbers are
plain float64 formulas; nothing here touches the device."""
import math

import numpy as np

SCALARS_VALID = 1        # flags bit 0: scalar_min, scalar_max, scalar_bad are valid
DIFFUSION_VALID = 2      # flags bit 1: s_max, pair_bad are valid
NO_ID = 0xFFFFFFFF       # bad_id_min where no particle was bad
QUANTUM_DEFAULT = -24

# sph_hip_monitor_row: field order is ABI, 128 bytes
ROW = np.dtype([("momentum", "<i8", (3,)), ("kinetic", "<i8"), ("mass", "<i8"),
                ("live", "<i4"), ("bad", "<i4"), ("skipped", "<i4"), ("lone", "<i4"), ("ncount_max", "<i4"),
                ("scalar_bad", "<i4"), ("pair_bad", "<i4"), ("bad_id_min", "<u4"),
                ("v2_max", "<f4"), ("a2_max", "<f4"), ("rho_max", "<f4"), ("rho_min", "<f4"), ("s_max", "<f4"),
                ("scalar_min", "<f4", (4,)), ("scalar_max", "<f4", (4,)), ("flags", "<u4")])
ROW_BYTES = 128
assert ROW.itemsize == ROW_BYTES


class MonitorRecord:
    """The rows of a step monitor: `rows` (a structured array of ROW, one per recorded step, the raw bits), `steps`
    (int32: the number of the step each row describes, from 1 at recordMonitor) and `quantum_log2` of the integer
    sums.  Every field of ROW is also an attribute (record.bad, record.v2_max, ...)."""

    def __init__(self, rows, steps, quantum_log2=QUANTUM_DEFAULT):
        self.rows = np.ascontiguousarray(rows, ROW).reshape(-1)
        self.steps = np.ascontiguousarray(steps, np.int32).reshape(-1)
        if self.rows.size != self.steps.size:
            raise ValueError("one step number per row")
        self.quantum_log2 = int(quantum_log2)

    def __len__(self):
        return self.rows.size

    def __getattr__(self, name):
        if name != "rows" and name in ROW.names:
            return self.rows[name]
        raise AttributeError(name)

    # ---- the integer sums in physical units ----------------------------------------------------------
    @property
    def quantum(self):
        return math.ldexp(1.0, self.quantum_log2)

    @property
    def momentum(self):
        """(rows, 3) float64: sum of m * v"""
        return self.rows["momentum"].astype(np.float64) * self.quantum

    @property
    def kinetic(self):
        """(rows,) float64: sum of 0.5 * m * v^2"""
        return self.rows["kinetic"].astype(np.float64) * self.quantum

    @property
    def mass(self):
        return self.rows["mass"].astype(np.float64) * self.quantum

    # ---- stability numbers ---------------------------------------------------------------------------------
    @property
    def speed_max(self):
        return np.sqrt(self.rows["v2_max"].astype(np.float64))

    @property
    def accel_max(self):
        return np.sqrt(self.rows["a2_max"].astype(np.float64))

    @staticmethod
    def _length_step(params):
        """what a unit of speed moves a particle per step, in smoothing lengths (the tracers' displacement step)"""
        return float(params.time_step) * float(params.sim_scale_inv) / float(params.h)

    def courant(self, params):
        """The displacement of the fastest particle in one step, in smoothing lengths."""
        return self.speed_max * self._length_step(params)

    def accel_number(self, params):
        """The same for the speed the largest acceleration adds in one step, sqrt(a2_max) * time_step."""
        return self.accel_max * float(params.time_step) * self._length_step(params)

    def diffusion_number(self, kappa, time_step):
        """(rows, 4) float64: dt * kappa[c] * s_max, which must stay <= 1 for the scalar pass to be a convex
        combination; NaN in the rows that carry no s_max."""
        kappa = np.asarray(kappa, np.float64).reshape(4)
        s = np.where(self.has_diffusion, self.rows["s_max"].astype(np.float64), np.nan)
        return float(time_step) * s[:, None] * kappa[None, :]

    @property
    def has_scalars(self):
        return (self.rows["flags"] & SCALARS_VALID) != 0

    @property
    def has_diffusion(self):
        return (self.rows["flags"] & DIFFUSION_VALID) != 0

    def first_bad(self):
        """The index of the first row with a bad particle, a channel that is not finite or a diffusion sum that is
        not, or None."""
        wrong = (self.rows["bad"] != 0) | (self.rows["scalar_bad"] != 0) | (self.rows["pair_bad"] != 0)
        hit = np.flatnonzero(wrong)
        return int(hit[0]) if hit.size else None

    def suggest_time_step(self, params, kappa=None, courant=0.25, diffusion=0.5):
        """The largest time step that would have kept every row's courant() and accel_number() at or under `courant`
        and, with kappa, every diffusion_number() at or under `diffusion`, for the speeds, accelerations and sums
        the rows hold; inf where nothing in them limits it."""
        per_dt = float(params.sim_scale_inv) / float(params.h)
        limit = math.inf
        if len(self):
            v = float(self.speed_max.max())
            a = float(self.accel_max.max())
            if v > 0.0:
                limit = min(limit, courant / (v * per_dt))
            if a > 0.0:
                limit = min(limit, math.sqrt(courant / (a * per_dt)))
            if kappa is not None and self.has_diffusion.any():
                k = float(np.asarray(kappa, np.float64).max())
                s = float(self.rows["s_max"][self.has_diffusion].astype(np.float64).max())
                if k > 0.0 and s > 0.0:
                    limit = min(limit, diffusion / (k * s))
        return limit
