"""ctypes binding of include/sph_hip.h.  Fails loudly when the HIP library is absent."""
import collections
import ctypes as C
import os

from .build import library_path

MODE_REF = 0
MODE_FULL = 1
MODE_FULL_FAST = 2   # FULL with tolerance-mode pair arithmetic (include/sph_hip.h)
ARITH_EXACT, ARITH_FAST = 0, 1
ABI_DIAGNOSTIC = 0x4000
# sph_hip_set_timing levels (include/sph_hip.h)
TIMING_OFF, TIMING_SUMS, TIMING_PHASES = 0, 1, 2


class SphHipError(RuntimeError):
    pass


class SphParams(C.Structure):
    """Mirror of sph_hip_params (include/sph_hip.h) = the protected constants of the
    reference's SPH class (reference src/sph.h:149-210)."""

    _fields_ = [
        ("cells_x", C.c_int32), ("cells_y", C.c_int32), ("cells_z", C.c_int32),
        ("cell_size", C.c_float),
        ("max_x", C.c_float), ("max_y", C.c_float), ("max_z", C.c_float),
        ("h", C.c_float), ("h2", C.c_float), ("hscaled", C.c_float), ("hscaled2", C.c_float),
        ("hscaled6", C.c_float), ("hscaled9", C.c_float), ("htimes2", C.c_float),
        ("htimes2inv", C.c_float), ("sim_scale", C.c_float), ("sim_scale_inv", C.c_float),
        ("kernel1", C.c_float), ("kernel2", C.c_float), ("kernel3", C.c_float),
        ("rho0", C.c_float), ("stiffness", C.c_float), ("viscosity", C.c_float),
        ("time_step", C.c_float), ("damping", C.c_float),
        ("cfl_limit", C.c_float), ("cfl_limit2", C.c_float),
        ("gravity", C.c_float * 3),
        ("grav_const", C.c_float), ("central_mass", C.c_float), ("central_pos", C.c_float * 3),
        ("softening", C.c_float),
        ("examine_count", C.c_int32),
        ("full_cells_x", C.c_int32), ("full_cells_y", C.c_int32), ("full_cells_z", C.c_int32),
        ("full_cell_inv", C.c_float),
        ("apply_gravity", C.c_int32), ("apply_walls", C.c_int32),
    ]

    def copy(self):
        other = SphParams()
        C.memmove(C.byref(other), C.byref(self), C.sizeof(SphParams))
        return other

    def as_dict(self):
        out = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            out[name] = list(v) if hasattr(v, "__len__") else v
        return out


class SphCamera(C.Structure):
    """Mirror of sph_hip_camera (include/sph_hip.h: renderer)."""

    _fields_ = [("eye", C.c_float * 3), ("forward", C.c_float * 3), ("right", C.c_float * 3),
                ("up", C.c_float * 3)]


class SphRenderParams(C.Structure):
    """Mirror of sph_hip_render_params (include/sph_hip.h: renderer)."""

    _fields_ = [
        ("box_lo", C.c_float * 3), ("box_hi", C.c_float * 3),
        ("step", C.c_float), ("iso", C.c_float), ("refine", C.c_int32), ("grad_step", C.c_float),
        ("light", C.c_float * 3), ("albedo", C.c_float * 3), ("ambient", C.c_float), ("diffuse", C.c_float),
        ("background", C.c_uint8 * 4), ("max_samples", C.c_int32),
    ]


class SphSceneParams(C.Structure):
    """Mirror of sph_hip_scene_params (include/sph_hip.h: scene renderer): 20 bytes."""

    _fields_ = [("albedo", C.c_float * 3), ("ambient", C.c_float), ("diffuse", C.c_float)]


class SphTintParams(C.Structure):
    """Mirror of sph_hip_tint_params (include/sph_hip.h: scalar renderer): 24 bytes."""

    _fields_ = [("channel", C.c_int32), ("mode", C.c_int32), ("lo", C.c_float), ("hi", C.c_float),
                ("n_colors", C.c_int32), ("flags", C.c_int32)]


from . import obstacles as _obstacles  # noqa: E402
from .obstacles import (SphBody, SphBodyState, SphMotionKey, SphMotionPath, SphObstacle,  # noqa: E402
                        SphObstacleMotion)  # (mirrors of the C structs)
from .gauges import GaugeReadings, GaugeRecord, SphGauge  # noqa: E402,F401
from .ports import PortTotals, SphEmitter, SphSink  # noqa: E402,F401
from .scalars import SphBuoyancy, SphScalarSource  # noqa: E402,F401
from .viscosity import SphViscosityLaw  # noqa: E402,F401

# every symbol include/sph_hip.h declares: name -> (restype, argtypes)
_P = C.POINTER
_ctx = C.c_void_p
PROTOTYPES = {
    "sph_hip_params_default": (C.c_int, [_P(SphParams), C.c_float, C.c_int, C.c_int, C.c_int]),
    "sph_hip_create": (C.c_int, [_P(_ctx), _P(SphParams), C.c_int, C.c_int, C.c_int]),
    "sph_hip_destroy": (None, [_ctx]),
    "sph_hip_last_error": (C.c_char_p, [_ctx]),
    "sph_hip_set_params": (C.c_int, [_ctx, _P(SphParams)]),
    "sph_hip_get_params": (C.c_int, [_ctx, _P(SphParams)]),
    "sph_hip_set_arithmetic": (C.c_int, [_ctx, C.c_int]),
    "sph_hip_get_arithmetic": (C.c_int, [_ctx]),
    "sph_hip_upload": (C.c_int, [_ctx, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sph_hip_download": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sph_hip_particle_count": (C.c_int, [_ctx]),
    "sph_hip_download_async": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, _P(C.c_int)]),
    "sph_hip_download_done": (C.c_int, [_ctx, C.c_int]),
    "sph_hip_host_register": (C.c_int, [C.c_void_p, C.c_size_t]),
    "sph_hip_host_unregister": (C.c_int, [C.c_void_p]),
    "sph_hip_step": (C.c_int, [_ctx]),
    "sph_hip_run": (C.c_int, [_ctx, C.c_int]),
    "sph_hip_voxelize": (C.c_int, [_ctx]),
    "sph_hip_find_neighbors": (C.c_int, [_ctx]),
    "sph_hip_compute_density": (C.c_int, [_ctx]),
    "sph_hip_compute_acceleration": (C.c_int, [_ctx]),
    "sph_hip_integrate": (C.c_int, [_ctx]),
    "sph_hip_synchronize": (C.c_int, [_ctx]),
    "sph_hip_get_timings": (C.c_int, [_ctx, _P(C.c_float * 6)]),
    "sph_hip_get_phase_totals": (C.c_int, [_ctx, _P(C.c_double * 6), _P(C.c_int32)]),
    "sph_hip_reset_timings": (C.c_int, [_ctx]),
    "sph_hip_set_timing": (C.c_int, [_ctx, C.c_int]),
    "sph_hip_set_timing_stride": (C.c_int, [_ctx, C.c_int]),
    "sph_hip_get_tile_stats": (C.c_int, [_ctx, _P(C.c_int32 * 20)]),
    "sph_hip_get_energy": (C.c_int, [_ctx, _P(C.c_float), _P(C.c_float)]),
    "sph_hip_get_neighbor_stats": (C.c_int, [_ctx, _P(C.c_int32), _P(C.c_int32), _P(C.c_int32)]),
    "sph_hip_download_voxels": (C.c_int, [_ctx, C.c_void_p, C.c_void_p]),
    "sph_hip_download_grid_counts": (C.c_int, [_ctx, C.c_void_p]),
    "sph_hip_download_neighbor_lists": (C.c_int, [_ctx, C.c_void_p, C.c_void_p]),
    "sph_hip_sample_points": (C.c_int, [_ctx, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sph_hip_sample_pressure_points": (C.c_int, [_ctx, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sph_hip_sample_pressure_lattice": (C.c_int, [_ctx, _P(C.c_float * 3), _P(C.c_float * 3), _P(C.c_int32 * 3),
                                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "sph_hip_sample_lattice": (C.c_int, [_ctx, _P(C.c_float * 3), _P(C.c_float * 3), _P(C.c_int32 * 3),
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "sph_hip_extract_surface": (C.c_int, [_ctx, _P(C.c_float * 3), _P(C.c_float * 3), _P(C.c_int32 * 3), C.c_float,
                                          C.c_int, _P(C.c_int32 * 2)]),
    "sph_hip_download_surface": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sph_hip_render": (C.c_int, [_ctx, _P(SphCamera), _P(SphRenderParams), C.c_int, C.c_int, C.c_int,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sph_hip_render_scene": (C.c_int, [_ctx, _P(SphCamera), _P(SphRenderParams), _P(SphSceneParams), C.c_void_p,
                                       C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "sph_hip_render_scalars": (C.c_int, [_ctx, _P(SphCamera), _P(SphRenderParams), _P(SphSceneParams), C.c_void_p,
                                         C.c_int, _P(SphTintParams), C.c_void_p, C.c_int, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "sph_hip_set_obstacles": (C.c_int, [_ctx, _P(SphObstacle), C.c_int]),
    "sph_hip_get_obstacles": (C.c_int, [_ctx, _P(SphObstacle), C.c_int]),
    "sph_hip_set_obstacle_motion": (C.c_int, [_ctx, _P(SphObstacleMotion), C.c_int]),
    "sph_hip_get_obstacle_motion": (C.c_int, [_ctx, _P(SphObstacleMotion), C.c_int, _P(C.c_float)]),
    "sph_hip_get_obstacles_now": (C.c_int, [_ctx, _P(SphObstacle), C.c_int]),
    "sph_hip_set_obstacle_paths": (C.c_int, [_ctx, _P(SphMotionPath), C.c_int, _P(SphMotionKey), C.c_int]),
    "sph_hip_get_obstacle_paths": (C.c_int, [_ctx, _P(SphMotionPath), C.c_int, _P(SphMotionKey), C.c_int,
                                             C.c_void_p]),
    "sph_hip_set_bodies": (C.c_int, [_ctx, _P(SphBody), C.c_int, C.c_int]),
    "sph_hip_get_bodies": (C.c_int, [_ctx, _P(SphBody), _P(SphBodyState), C.c_int]),
    "sph_hip_record_loads": (C.c_int, [_ctx, C.c_int, C.c_int]),
    "sph_hip_get_loads": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, _P(C.c_int32)]),
    "sph_hip_set_tracers": (C.c_int, [_ctx, C.c_int, C.c_void_p]),
    "sph_hip_get_tracers": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sph_hip_tracer_count": (C.c_int, [_ctx]),
    "sph_hip_record_tracers": (C.c_int, [_ctx, C.c_int, C.c_int]),
    "sph_hip_get_tracer_path": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "sph_hip_set_gauges": (C.c_int, [_ctx, _P(SphGauge), C.c_int]),
    "sph_hip_get_gauges": (C.c_int, [_ctx, _P(SphGauge), C.c_int]),
    "sph_hip_read_gauges": (C.c_int, [_ctx, C.c_void_p]),
    "sph_hip_record_gauges": (C.c_int, [_ctx, C.c_int, C.c_int]),
    "sph_hip_get_gauge_record": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "sph_hip_set_ports": (C.c_int, [_ctx, _P(SphEmitter), C.c_int, _P(SphSink), C.c_int]),
    "sph_hip_get_ports": (C.c_int, [_ctx, _P(SphEmitter), _P(SphSink), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                    _P(C.c_int32), _P(C.c_uint32)]),
    "sph_hip_download_live": (C.c_int, [_ctx, C.c_int, _P(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "sph_hip_set_scalars": (C.c_int, [_ctx, C.c_int, C.c_void_p, C.c_void_p]),
    "sph_hip_get_scalars": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_void_p]),
    "sph_hip_set_scalar_sources": (C.c_int, [_ctx, _P(SphScalarSource), C.c_int]),
    "sph_hip_get_scalar_sources": (C.c_int, [_ctx, _P(SphScalarSource), C.c_int]),
    "sph_hip_sample_scalars_points": (C.c_int, [_ctx, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sph_hip_sample_scalars_lattice": (C.c_int, [_ctx, _P(C.c_float * 3), _P(C.c_float * 3), _P(C.c_int32 * 3),
                                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    "sph_hip_set_buoyancy": (C.c_int, [_ctx, _P(SphBuoyancy)]),
    "sph_hip_get_buoyancy": (C.c_int, [_ctx, _P(SphBuoyancy)]),
    "sph_hip_set_cohesion": (C.c_int, [_ctx, C.c_float]),
    "sph_hip_get_cohesion": (C.c_int, [_ctx, _P(C.c_float)]),
    "sph_hip_set_xsph": (C.c_int, [_ctx, C.c_float]),
    "sph_hip_get_xsph": (C.c_int, [_ctx, _P(C.c_float)]),
    "sph_hip_set_viscous_stress": (C.c_int, [_ctx, C.c_float, _P(SphViscosityLaw)]),
    "sph_hip_get_viscous_stress": (C.c_int, [_ctx, _P(C.c_float), _P(SphViscosityLaw), _P(C.c_int)]),
    "sph_hip_set_viscous_implicit": (C.c_int, [_ctx, C.c_int]),
    "sph_hip_get_viscous_implicit": (C.c_int, [_ctx, _P(C.c_int)]),
    "sph_hip_record_monitor": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int]),
    "sph_hip_get_monitor_record": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "sph_hip_get_velocity_gradients": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "sph_hip_sample_velocity_gradients_points": (C.c_int, [_ctx, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                           C.c_void_p]),
    "sph_hip_sample_velocity_gradients_lattice": (C.c_int, [_ctx, _P(C.c_float * 3), _P(C.c_float * 3),
                                                            _P(C.c_int32 * 3), C.c_int, C.c_void_p, C.c_void_p,
                                                            C.c_void_p]),
    "sph_hip_render_velocity_gradients": (C.c_int, [_ctx, _P(SphCamera), _P(SphRenderParams), _P(SphSceneParams),
                                                    C.c_void_p, C.c_int, _P(SphTintParams), C.c_void_p, C.c_int,
                                                    C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "sph_hip_stream": (C.c_void_p, [_ctx]),
    "sph_hip_set_stream": (C.c_int, [_ctx, C.c_void_p]),
    "sph_hip_create_slab": (C.c_int, [_P(_ctx), _P(SphParams), C.c_int, C.c_int, C.c_int, C.c_int]),
    "sph_hip_slab_upload": (C.c_int, [_ctx, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int]),
    "sph_hip_slab_download": (C.c_int, [_ctx, C.c_int, _P(C.c_int32), C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sph_hip_slab_download_mass": (C.c_int, [_ctx, C.c_int, _P(C.c_int32), C.c_void_p]),
    "sph_hip_slab_export_records": (C.c_int, [_ctx, C.c_void_p, C.c_int, _P(C.c_int32)]),
    "sph_hip_slab_upload_records": (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int]),
    "sph_hip_slab_message_bytes": (C.c_size_t, [C.c_int]),
    "sph_hip_slab_pack": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int]),
    "sph_hip_slab_unpack": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int]),
    "sph_hip_slab_step_begin": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "sph_hip_slab_step_end": (C.c_int, [_ctx]),
    "sph_hip_rccl_unique_id": (C.c_int, [C.c_void_p, C.c_int]),
    "sph_hip_slab_comm_init": (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "sph_hip_slab_comm_run": (C.c_int, [_ctx, C.c_int]),
    "sph_hip_slab_comm_trim": (C.c_int, [_ctx, C.c_float, C.c_int, _P(C.c_int32)]),
    "sph_hip_slab_comm_selftest": (C.c_int, [_ctx]),
    "sph_hip_slab_comm_exchange_check": (C.c_int, [_ctx]),
    "sph_hip_slab_comm_stats": (C.c_int, [_ctx, _P(C.c_int32)]),
    "sph_hip_slab_status": (C.c_int, [_ctx, _P(C.c_int32), _P(C.c_int32), _P(C.c_int32)]),
    "sph_hip_slab_poll_errors": (C.c_int, [_ctx, _P(C.c_int32)]),
    "sph_hip_abi_version": (C.c_int, []),
    "sph_hip_selftest_sqrt": (C.c_int, [C.c_int, _P(C.c_uint64), _P(C.c_uint32)]),
}
ABI_VERSION = 7   # SPH_HIP_ABI_VERSION of the include/sph_hip.h these prototypes mirror

_LIB = None


def load_library(path=None):
    """Load libsph_hip.so and bind every entry point of include/sph_hip.h.

    There is deliberately no fallback: if the library has not been built (or cannot be
    loaded) this raises, and so does everything that depends on it.
    """
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    path = path or library_path()
    # Plumbing: when PyTorch is installed it must bring up ITS ROCm runtime before this library
    # touches HIP — two independently initialised HIP runtimes in one process leave the second
    # one without a device ("no ROCm-capable device is detected").  torch is only imported, never
    # used here; the C++ host (integration/) has no such concern.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(path):
        raise SphHipError(
            "libsph_hip.so is missing (%s): build it with "
            "`python -m smoothed_particle_hydrodynamics_amd.build`; there is no CPU fallback" % path)
    try:
        lib = C.CDLL(path)
    except OSError as exc:  # pragma: no cover - depends on the machine
        raise SphHipError("cannot load %s: %s" % (path, exc)) from exc
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.restype = restype
        fn.argtypes = argtypes
    abi = lib.sph_hip_abi_version()
    if abi & ABI_DIAGNOSTIC and os.environ.get("SPH_HIP_ALLOW_DIAGNOSTIC") != "1":
        raise SphHipError("%s is a diagnostic build (profiling hooks that cut pieces out of the "
                          "kernels: its results are garbage by design); only tools/ablate.py, with "
                          "SPH_HIP_ALLOW_DIAGNOSTIC=1, may load one" % path)
    if abi & ~ABI_DIAGNOSTIC != ABI_VERSION:
        raise SphHipError("%s has ABI version %d, this binding expects %d: rebuild it" %
                          (path, abi & ~ABI_DIAGNOSTIC, ABI_VERSION))
    _LIB = lib
    return lib


def _ptr(a):
    """A numpy array (or None) as the void* argument of an entry point."""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


OBSTACLE_SPHERE, OBSTACLE_BOX, OBSTACLE_CYLINDER, OBSTACLE_WEDGE = (   # SPH_HIP_OBSTACLE_*
    _obstacles.SPHERE, _obstacles.BOX, _obstacles.CYLINDER, _obstacles.WEDGE)
LOAD_SOLIDS = 6 + _obstacles.MAX_OBSTACLES   # SPH_HIP_LOAD_SOLIDS
LOAD_QUANTUM_LOG2 = -24                      # the default quantum of a load recording
LOAD_NAMES = tuple(["x-lo", "x-hi", "y-lo", "y-hi", "z-lo", "z-hi"] +
                   ["obstacle %d" % i for i in range(_obstacles.MAX_OBSTACLES)])


class Loads:
    """The rows of a load recording (sph_hip_get_loads), one per recorded step:
    impulse_q int64 [steps, LOAD_SOLIDS, 3], the impulse given to each solid in quanta of
    `quantum` = 2**quantum_log2; count and skipped int64 [steps, LOAD_SOLIDS], the responses summed
    and those left out (a term that was not finite or reached 2^38 quanta); names: the columns.
    Rows of several slabs add up exactly: a + b."""

    names = LOAD_NAMES

    def __init__(self, impulse_q, count, skipped, quantum_log2):
        self.impulse_q, self.count, self.skipped = impulse_q, count, skipped
        self.quantum_log2 = int(quantum_log2)

    @property
    def quantum(self):
        return 2.0 ** self.quantum_log2

    @property
    def impulse(self):
        """float64 [steps, LOAD_SOLIDS, 3], in mass * velocity units"""
        return self.impulse_q.astype("float64") * self.quantum

    def force(self, time_step):
        """the mean force on each solid during each step: impulse / time_step"""
        return self.impulse / float(time_step)

    def __add__(self, other):
        if self.quantum_log2 != other.quantum_log2 or self.impulse_q.shape != other.impulse_q.shape:
            raise ValueError("loads of different quanta or step counts do not add")
        return Loads(self.impulse_q + other.impulse_q, self.count + other.count, self.skipped + other.skipped,
                     self.quantum_log2)


# sph_hip_get_bodies' answer: bodies [Body or None per obstacle], displacement and velocity float32 (n, 3),
# skipped and steps int64 (n,); n = 0 when no bodies are set
Bodies = collections.namedtuple("Bodies", ["bodies", "displacement", "velocity", "skipped", "steps"])


# sph_hip_get_obstacle_paths' answer: paths [MotionPath or None per obstacle], the motion clock, shifts float32
# (n_obstacles, 2, 3) - D0 and D1 of the last enqueued step - or None when they were not asked for
ObstaclePaths = collections.namedtuple("ObstaclePaths", ["paths", "clock", "shifts"])


# sph_hip_get_tracers' answer, in the order given to set_tracers: position float32 (n, 3), wet_steps and
# dry_steps int32 (n,)
Tracers = collections.namedtuple("Tracers", ["position", "wet_steps", "dry_steps"])
# sph_hip_get_tracer_path's answer: steps int32 (rows,), the step numbers since record_tracers; positions
# float32 (rows, n, 3) by tracer id
TracerPath = collections.namedtuple("TracerPath", ["steps", "positions"])


class Context:
    """Owner of one sph_hip_context handle: creation, destruction, the checked call, and the
    operations that need nothing but the handle.  SPH (sph.py) and HipSlab (slab.py) derive from it."""

    def __init__(self, creator, *args):
        """creator: name of the entry point that makes the handle ("sph_hip_create",
        "sph_hip_create_slab"); it is given the handle's address, then `args`."""
        self._lib = load_library()
        self._ctx = C.c_void_p()
        rc = getattr(self._lib, creator)(C.byref(self._ctx), *args)
        if rc != 0:
            msg = self._lib.sph_hip_last_error(None).decode()
            self._ctx = C.c_void_p()
            raise SphHipError("%s failed (%d): %s" % (creator, rc, msg))

    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx:
            self._lib.sph_hip_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def call(self, name, *args):
        """Entry point `name` with the handle and `args`, checked."""
        fn = getattr(self._lib, name)
        return self.check(fn, fn(self._ctx, *args))

    def check(self, fn, rc):
        """What entry point `fn` returned: a negative value (every SPH_HIP_ERR_* is negative) raises
        SphHipError with the context's message; anything else is passed on."""
        if rc < 0:
            msg = self._lib.sph_hip_last_error(self._ctx).decode()
            raise SphHipError("%s failed (%d): %s" % (fn.__name__, rc, msg))
        return rc

    def synchronize(self):
        self.call("sph_hip_synchronize")

    def tile_stats(self):
        """dict of the last step's LDS-tile statistics (sph_hip_get_tile_stats)."""
        out = (C.c_int32 * 20)()
        self.call("sph_hip_get_tile_stats", C.byref(out))
        v = list(out)
        return {"over_level": v[0:12], "workgroups": v[12], "largest_tile": v[13],
                "untiled_density": v[14], "untiled_acceleration": v[15],
                "capacity_density": v[16], "capacity_acceleration": v[17], "wide_entries": v[18],
                "list_capacity": v[19]}

    def phase_totals(self):
        """(sum of the six phase times in ms over the steps since reset_timings(), steps)"""
        ms = (C.c_double * 6)()
        k = C.c_int32()
        self.call("sph_hip_get_phase_totals", C.byref(ms), C.byref(k))
        return list(ms), k.value

    def energy(self):
        """(kinetic, potential) energy total of the last integrate."""
        ke, pe = C.c_float(), C.c_float()
        self.call("sph_hip_get_energy", C.byref(ke), C.byref(pe))
        return ke.value, pe.value

    def reset_timings(self):
        self.call("sph_hip_reset_timings")

    def set_timing(self, level):
        """Which intervals a step times: TIMING_PHASES (default, all six), TIMING_SUMS (density +
        acceleration as one interval, in slot 2), TIMING_OFF.  Resets the collected timings."""
        self.call("sph_hip_set_timing", int(level))

    def set_timing_stride(self, every):
        """Record the timing events on every `every`-th step only (sph_hip_set_timing_stride)."""
        self.call("sph_hip_set_timing_stride", int(every))

    def set_arithmetic(self, arithmetic):
        """ARITH_EXACT / ARITH_FAST for the pair sums of a FULL-mode context (sph_hip_set_arithmetic)."""
        self.call("sph_hip_set_arithmetic", int(arithmetic))

    def set_obstacles(self, obstacles):
        """Replace the static obstacles (obstacles.Sphere / Box / Cylinder, at most 64; an empty list
        clears them).  Steps already queued keep the old list."""
        arr, n = _obstacles.as_array(obstacles)
        self.call("sph_hip_set_obstacles", arr, n)

    def get_obstacles(self, now=False):
        """The context's obstacles, in list order: as they were set, or (now=True) displaced by their
        motions and paths to the current motion clock and, free bodies, to where the device has moved them
        (sph_hip_get_obstacles_now)."""
        arr = (SphObstacle * _obstacles.MAX_OBSTACLES)()
        n = self.call("sph_hip_get_obstacles_now" if now else "sph_hip_get_obstacles", arr, _obstacles.MAX_OBSTACLES)
        return [_obstacles.from_struct(arr[i]) for i in range(n)]

    def set_obstacle_motion(self, motions):
        """Drive the obstacles (sph_hip_set_obstacle_motion): one obstacles.Motion per obstacle, None
        for one at rest; an empty list clears all motions.  Sets the motion clock to 0; steps already
        queued keep the motions and the clock they were enqueued with."""
        arr, n = _obstacles.as_motion_array(motions)
        self.call("sph_hip_set_obstacle_motion", arr, n)

    def get_obstacle_motion(self):
        """([Motion per obstacle] - empty when no motions are set -, the motion clock)."""
        arr = (SphObstacleMotion * _obstacles.MAX_OBSTACLES)()
        clock = C.c_float()
        n = self.call("sph_hip_get_obstacle_motion", arr, _obstacles.MAX_OBSTACLES, C.byref(clock))
        return [_obstacles.motion_from_struct(arr[i]) for i in range(n)], clock.value

    def set_obstacle_paths(self, paths):
        """Drive the obstacles along keyframed displacements (sph_hip_set_obstacle_paths): one
        obstacles.MotionPath per obstacle, None for one without a path; an empty list clears all paths.
        Sets the motion clock to 0; steps already queued keep the paths and the clock they were enqueued
        with.  Single contexts only, and not beside free bodies."""
        arr, n, keys, n_keys = _obstacles.as_path_arrays(paths)
        self.call("sph_hip_set_obstacle_paths", arr, n, keys, n_keys)

    def get_obstacle_paths(self, shifts=True):
        """ObstaclePaths(paths, clock, shifts): [MotionPath or None per obstacle] - empty when no paths are
        set -, the motion clock, and (shifts=True; synchronises) float32 (n_obstacles, 2, 3): the shifts D0
        and D1 the device used for each obstacle in the last enqueued step, zeros without a path."""
        import numpy as np
        arr = (SphMotionPath * _obstacles.MAX_OBSTACLES)()
        keys = (SphMotionKey * _obstacles.MAX_PATH_KEYS)()
        out = np.zeros((_obstacles.MAX_OBSTACLES, 2, 3), np.float32)
        n = self.call("sph_hip_get_obstacle_paths", arr, _obstacles.MAX_OBSTACLES, keys, _obstacles.MAX_PATH_KEYS,
                      _ptr(out) if shifts else None)
        clock = C.c_float()
        self.call("sph_hip_get_obstacle_motion", None, 0, C.byref(clock))
        n_obst = self.call("sph_hip_get_obstacles", None, 0)
        return ObstaclePaths(_obstacles.paths_from_arrays(arr, n, keys), clock.value,
                             out[:n_obst].copy() if shifts else None)

    def record_loads(self, steps, quantum_log2=LOAD_QUANTUM_LOG2):
        """Record the impulse the next `steps` steps give to every wall and obstacle
        (sph_hip_record_loads); steps = 0 stops and frees the recording."""
        self.call("sph_hip_record_loads", int(steps), int(quantum_log2))
        self._loads_quantum_log2 = int(quantum_log2)

    def get_loads(self):
        """The rows recorded so far, as a Loads (sph_hip_get_loads; synchronises)."""
        import numpy as np
        done = C.c_int32()
        self.call("sph_hip_get_loads", 0, 0, None, None, None, C.byref(done))
        n = done.value
        imp = np.zeros((n, LOAD_SOLIDS, 3), np.int64)
        cnt = np.zeros((n, LOAD_SOLIDS), np.int64)
        skp = np.zeros((n, LOAD_SOLIDS), np.int64)
        self.call("sph_hip_get_loads", 0, n, _ptr(imp), _ptr(cnt), _ptr(skp), None)
        return Loads(imp, cnt, skp, self._loads_quantum_log2)


def default_params(h=0.1, cells=(32, 32, 32)):
    """SPH::SPH()'s constants (reference src/sph.cpp:46-98) for smoothing length h."""
    lib = load_library()
    p = SphParams()
    rc = lib.sph_hip_params_default(C.byref(p), h, int(cells[0]), int(cells[1]), int(cells[2]))
    if rc != 0:
        raise SphHipError("sph_hip_params_default failed (%d)" % rc)
    return p
