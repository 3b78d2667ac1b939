"""Velocity gradients (include/sph_hip.h: velocity gradients): the eight quantities' names and numbers, and the host
view of the two float4 rows the device forms per particle or per probe."""
import numpy as np

# SPH_HIP_VELGRAD_*: the order of the two rows, rotation = (w_x, w_y, w_z, div), invariants = (strain, Q, |w|, valid)
QUANTITIES = ("vorticity_x", "vorticity_y", "vorticity_z", "divergence", "strain_rate", "q", "vorticity_magnitude",
              "valid")
VORTICITY_X, VORTICITY_Y, VORTICITY_Z, DIVERGENCE, STRAIN_RATE, Q, VORTICITY_MAGNITUDE, VALID = range(8)
GROUP_ROTATION, GROUP_INVARIANTS = 0, 1


def quantity_index(quantity):
    """The number 0 .. 7 of a quantity given by name or by number."""
    if isinstance(quantity, str):
        if quantity not in QUANTITIES:
            raise ValueError("quantity must be one of %s" % ", ".join(QUANTITIES))
        return QUANTITIES.index(quantity)
    q = int(quantity)
    if not 0 <= q < len(QUANTITIES):
        raise ValueError("quantity must be 0 .. 7")
    return q


class VelocityGradients:
    """The rows of n particles (getVelocityGradients) or n probes (sampleVelocityGradients; with density and count, and
    any leading shape for a lattice): .vorticity (..., 3), .divergence, .strain_rate, .q, .vorticity_magnitude and
    .valid - bool for particles, for probes the weighted share of valid particles around the probe as a float."""

    def __init__(self, rotation, invariants, density=None, count=None):
        self.rotation = np.asarray(rotation, np.float32)
        self.invariants = np.asarray(invariants, np.float32)
        self.density = density
        self.count = count

    @property
    def vorticity(self):
        return self.rotation[..., 0:3]

    @property
    def divergence(self):
        return self.rotation[..., 3]

    @property
    def strain_rate(self):
        return self.invariants[..., 0]

    @property
    def q(self):
        return self.invariants[..., 1]

    @property
    def vorticity_magnitude(self):
        return self.invariants[..., 2]

    @property
    def valid(self):
        v = self.invariants[..., 3]
        return v != 0 if self.density is None else v

    def quantity(self, quantity):
        """One of the eight by name or number, as floats."""
        i = quantity_index(quantity)
        return (self.rotation if i < 4 else self.invariants)[..., i & 3]

    def enstrophy(self, mass):
        """0.5 * sum_i m_i |w_i|^2 over the particles, a host sum in float64."""
        m = np.asarray(mass, np.float64).reshape(-1)
        w = self.vorticity_magnitude.astype(np.float64).reshape(-1)
        return float(0.5 * np.sum(m * w * w))
