"""Shared helpers for the parity tests."""
import ctypes as C
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "smoothed_particle_hydrodynamics_amd",
                    "csrc")
PINS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_pins.json")


def compile_shim(source, flags, tmp_path_factory):
    """Compile an extern "C" shim over csrc/'s plain C++ headers with g++ (no HIP include path: the
    headers must compile without one) plus `flags`, and load it; skips the test where g++ is missing."""
    import pytest
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("shim")
    src, so = d / "shim.cpp", d / "libshim.so"
    src.write_text(source)
    subprocess.run([gxx, "-std=c++17", *flags, "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src),
                    "-o", str(so)], check=True)
    return C.CDLL(str(so))


def to_oracle_params(p):
    """SphParams (product) -> OracleParams (checker); the two structs have identical layout
    (asserted in test_capi.py)."""
    from oracle.oracle import OracleParams
    o = OracleParams()
    assert C.sizeof(o) == C.sizeof(p)
    C.memmove(C.byref(o), C.byref(p), C.sizeof(o))
    return o


def to_product_params(o):
    from smoothed_particle_hydrodynamics_amd import SphParams
    p = SphParams()
    assert C.sizeof(o) == C.sizeof(p)
    C.memmove(C.byref(p), C.byref(o), C.sizeof(p))
    return p


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def pin_sha(a):
    """sha() with every NaN written as the one quiet NaN: what np.array_equal(..., equal_nan=True)
    treats as equal hashes equal"""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f" and np.isnan(a).any():
        a = np.where(np.isnan(a), np.array(np.nan, a.dtype), a)
    return sha(a)


def _pin(v):
    if isinstance(v, np.ndarray):
        return pin_sha(v)
    if isinstance(v, (tuple, list)):
        return [float(x) for x in v]
    return float(v)


def reference_pins(case, run):
    """What the reference's own compiled sph.cpp computes for one test's inputs: pin_sha() of every
    array, the exact value of every number.  `run(reference)` drives the live library
    (oracle/_ref/libsphref.so) and returns {name: array, number or sequence of numbers}.  Where that
    library can be loaded, its answers are returned and must equal the pins stored for `case` in
    tests/golden/reference_pins.json; elsewhere the stored pins stand in for it.  With
    SPH_RECORD_REFERENCE_PINS=1 the live answers are written to that file instead of checked."""
    from oracle.oracle import Reference, reference_available
    with open(PINS_PATH) as f:
        stored = json.load(f)
    if not reference_available():
        assert case in stored, "no pins stored for " + case
        return stored[case]
    got = {name: _pin(v) for name, v in run(Reference()).items()}
    if os.environ.get("SPH_RECORD_REFERENCE_PINS") == "1":
        stored[case] = got
        with open(PINS_PATH, "w") as f:
            json.dump(stored, f, indent=1, sort_keys=True)
            f.write("\n")
    else:
        assert stored.get(case) == got, "the live reference disagrees with the pins stored for " + case
    return got


def live_mask(counts, cap):
    """boolean mask over the n*cap list storage selecting the stored entries"""
    return (np.arange(cap)[None, :] < counts[:, None]).ravel()


def max_rel(a, b, floor=0.0):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    den = np.maximum(np.maximum(np.abs(a), np.abs(b)), floor)
    den[den == 0] = 1.0
    return float((np.abs(a - b) / den).max()) if a.size else 0.0


def vec_rel(a, b):
    """per-particle relative error of 3-vectors: |a-b| / max(|a|,|b|)"""
    a = np.asarray(a, np.float64).reshape(-1, 3)
    b = np.asarray(b, np.float64).reshape(-1, 3)
    num = np.linalg.norm(a - b, axis=1)
    den = np.maximum(np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1))
    den[den == 0] = 1.0
    return num / den


def nonfinite_mismatch(a, b):
    """per component: True where a or b is not finite and the two are not of one class - NaN, +inf
    or -inf (a NaN's payload and sign do not count)"""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    fa, fb = np.isfinite(a), np.isfinite(b)
    same = (np.isnan(a) & np.isnan(b)) | (~fa & ~fb & (a == b))
    return (~fa | ~fb) & ~same


def finite_parts(a, b, what=""):
    """The tolerance bars' rule for non-finite values: wherever a component of either side is not
    finite, the other side's component must be of the same class (NaN, +inf, -inf).  Returns float64
    copies of a and b with those components set to 0 on both sides, so that a relative or absolute
    bar applied to them sees the finite components alone (a row finite on both sides unchanged)."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    bad = nonfinite_mismatch(a, b)
    if bad.any():
        i = int(np.flatnonzero(bad.reshape(-1))[0])
        raise AssertionError("%s: %d components differ in their non-finite class (first: component %d, %r "
                             "against %r)" % (what, int(bad.sum()), i, a.reshape(-1)[i], b.reshape(-1)[i]))
    keep = np.isfinite(a) & np.isfinite(b)
    return np.where(keep, a, 0.0), np.where(keep, b, 0.0)


def count_calls(cls, *names):
    """Wrap the methods `names` of `cls` (for the rest of the process): every call appends the
    method's name to the list returned here, then goes on to the method."""
    calls = []
    for name in names:
        def counted(self, *args, _inner=getattr(cls, name), _name=name, **kwargs):
            calls.append(_name)
            return _inner(self, *args, **kwargs)
        setattr(cls, name, counted)
    return calls


def energy_rtol(n):
    """the reference accumulates N fp32 terms serially: ~sqrt(N) * 2^-24 relative, x8 margin"""
    return 1e-6 + 8.0 * np.sqrt(float(n)) * 2.0 ** -24


def check_energy(got, want, vel_after, mass):
    """got: (ke, pe) from the device (double tree sum); want: the oracle's serial fp32 sums."""
    import pytest
    n = mass.size
    ke, pe = got
    assert ke == pytest.approx(want[0], rel=energy_rtol(n), abs=1e-30)
    assert pe == pytest.approx(want[1], rel=energy_rtol(n), abs=1e-30)
    # exact check: the same fp32 per-particle terms (reference src/sph.cpp:997-1004) summed in f64
    v = np.asarray(vel_after, np.float32).reshape(-1, 3)
    dot = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]
    term = (np.float32(0.5) * mass.astype(np.float32)) * dot
    ke64 = float(term[dot > 0].astype(np.float64).sum())
    assert ke == pytest.approx(np.float32(ke64), rel=1e-6, abs=1e-30)


NONFINITE_SCENES = ("particles", "central_x_inf", "central_z_nan")


def nonfinite_scene(case, params_for_h=None):
    """scenes.dam_break(4000, speed=0.05) - the moving dam-break without a point mass (central_mass
    = 0) - with non-finite values where the point-mass term meets them.  "particles": one particle
    with x = +inf, one with y = -inf, one with z = +inf, one with x = NaN, one NaN in all three;
    "central_x_inf" / "central_z_nan": the central position itself, for every particle.
    params_for_h(h, cells) makes the parameters: the product's default_params by default, the
    oracle's params_for_h (the same values, test_capi.py) in a CPU test, which must not load the
    product library (and with it torch) next to the reference's."""
    import math
    from smoothed_particle_hydrodynamics_amd import scenes
    n, hi = 4000, (0.1, 0.75, 1.0)
    h = np.float32(scenes.dam_break_h(n))
    cells = [int(math.ceil(1.0 / (2.0 * float(h))))] * 3
    p = (params_for_h or scenes.default_params)(float(h), cells)
    p.central_mass = 0.0
    pos = scenes.box_fill(n, (0.0, 0.0, 0.0), hi, 42).reshape(-1, 3)
    vel = scenes.box_fill(n, (-0.05,) * 3, (0.05,) * 3, 43)
    mass = np.ones(n, np.float32)
    if case == "particles":
        pos[10, 0] = np.inf
        pos[20, 1] = -np.inf
        pos[30, 2] = np.inf
        pos[40, 0] = np.nan
        pos[50] = np.nan
    elif case == "central_x_inf":
        p.central_pos[0] = np.inf
    elif case == "central_z_nan":
        p.central_pos[2] = np.nan
    else:
        raise ValueError(case)
    return p, np.ascontiguousarray(pos.reshape(-1)), vel, mass


READBACK_COUNTS = (1, 255, 256, 257, 6000)
READBACK_NONFINITE_ROWS = (10, 20, 30, 40, 50)


def readback_scene(n=6000, params_for_h=None):
    """The first n rows of the scene the read-back tests share (test_readback_cpu.py,
    test_gpu_readback.py): h = 0.1 on a 5 x 9 x 17 voxel grid (FULL grid 10 x 18 x 34: three distinct
    extents on both grids, so an index formula with two axes swapped cannot pass), no point mass, unit
    masses.  6000 positions uniform in [-0.3, 1.3) x the box's extent per axis - about three quarters lie
    outside the box and are clamped into its edge cells -, rows 100-399 snapped onto REF voxel faces, and
    the five non-finite rows of nonfinite_scene("particles"); velocities uniform in [-1, 1).  Rows that a
    smaller n does not have are simply missing.  params_for_h as in nonfinite_scene."""
    from smoothed_particle_hydrodynamics_amd import scenes
    total = READBACK_COUNTS[-1]
    cells = (5, 9, 17)
    p = (params_for_h or scenes.default_params)(0.1, cells)
    p.central_mass = 0.0
    ext = np.float32(cells) * np.float32(p.htimes2)
    pos = scenes.box_fill(total, tuple(np.float32(-0.3) * ext), tuple(np.float32(1.3) * ext), 61).reshape(-1, 3)
    edge = np.float32(1.0) / np.float32(p.htimes2inv)
    pos[100:400] = edge * np.round(pos[100:400] / edge)
    pos[10, 0] = np.inf
    pos[20, 1] = -np.inf
    pos[30, 2] = np.inf
    pos[40, 0] = np.nan
    pos[50] = np.nan
    vel = scenes.box_fill(total, (-1.0,) * 3, (1.0,) * 3, 62)
    return (p, np.ascontiguousarray(pos[:n].reshape(-1)), np.ascontiguousarray(vel[:3 * n]),
            np.ones(n, np.float32))


def grid_occupancy(pos, inv, cells):
    """Per-cell occupancy of a cells = (nx, ny, nz) grid with cell edge 1 / inv, restated in numpy: a
    bincount of (cz * ny + cy) * nx + cx with sample_emulation.cell_coord (csrc/sph_device.h
    cell_coord) per axis.  Returns (ids per particle, counts per cell)."""
    from sample_emulation import cell_coord
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    c = [cell_coord(pos[:, a], inv, cells[a]) for a in range(3)]
    ids = (c[2] * cells[1] + c[1]) * cells[0] + c[0]
    return ids, np.bincount(ids, minlength=cells[0] * cells[1] * cells[2]).astype(np.int32)
