"""Colour tables for SPH.renderScalars (include/sph_hip.h: scalar renderer): each an (n, 3) float32 array of
RGB rows in [0, 1], row 0 for the range's low end and row n - 1 for its high end; the device interpolates
linearly between neighbouring rows.  numpy only."""
import numpy as np

MAX_COLORS = 256   # SPH_HIP_TINT_MAX_COLORS


def _rows(n):
    n = int(n)
    if n < 2 or n > MAX_COLORS:
        raise ValueError("a colour table has 2 .. %d rows" % MAX_COLORS)
    return n


def _ramp(n, stops):
    """n rows along the piecewise-linear path through `stops` (equally spaced RGB points)"""
    n = _rows(n)
    stops = np.asarray(stops, np.float64).reshape(-1, 3)
    x = np.linspace(0.0, stops.shape[0] - 1.0, n)
    at = np.arange(stops.shape[0], dtype=np.float64)
    return np.stack([np.interp(x, at, stops[:, c]) for c in range(3)], 1).astype(np.float32)


def heat(n=256):
    """black - red - yellow - white"""
    return _ramp(n, [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)])


def gray(n=256):
    """black - white"""
    return _ramp(n, [(0, 0, 0), (1, 1, 1)])


def diverging(n=256):
    """blue - white - red, white at the middle of the range"""
    return _ramp(n, [(0.23, 0.30, 0.75), (1, 1, 1), (0.70, 0.02, 0.15)])


def dye(rgb, water=(0.25, 0.55, 0.9), n=2):
    """from the water's colour (concentration at the range's low end) to the dye's `rgb`"""
    return _ramp(n, [water, rgb])
