"""Host-side mirror of the reference's solver interface over the HIP C ABI.

`SPH` keeps the public/protected method names of the reference class (reference
src/sph.h:20-139) so that code and tests written against the reference read the same here;
`Particle` keeps the reference container's member names and layouts (reference
src/particle.h:7-20: one object for all particles, xyz interleaved).  All computation
happens in libsph_hip.so on the GPU; this file only moves arrays and parameters.
"""
import collections
import ctypes as C
import math
import struct
import zlib

import numpy as np

from . import gauges as _G
from . import obstacles as _O
from . import ports as _P
from . import scalars as _S
from . import colormaps as _CM
from . import monitor as _M
from . import velgrad as _V
from . import viscosity as _VS
from .lib import ARITH_EXACT, ARITH_FAST, MODE_FULL, MODE_FULL_FAST, MODE_REF, Bodies, Context, SphCamera, SphRenderParams, SphSceneParams, SphTintParams, TracerPath, Tracers, _ptr, default_params

__all__ = ["SPH", "Particle", "SurfaceMesh", "Tracers", "TracerPath", "Camera", "RenderResult", "ScalarRenderResult", "write_png", "MODE_REF", "MODE_FULL", "MODE_FULL_FAST", "ARITH_EXACT", "ARITH_FAST"]


class Particle:
    """reference src/particle.h:7-20 — struct of arrays for ALL particles."""

    def __init__(self, num_particles):
        n = int(num_particles)
        self.mMass = np.zeros(n, np.float32)
        self.mDensity = np.zeros(n, np.float32)
        self.mPosition = np.zeros(3 * n, np.float32)
        self.mVelocity = np.zeros(3 * n, np.float32)
        self.mAcceleration = np.zeros(3 * n, np.float32)
        self.mNeighborCount = np.zeros(n, np.int32)


SURFACE_NORMALS, SURFACE_VELOCITY = 1, 2   # SPH_HIP_SURFACE_* (include/sph_hip.h)

# sph_hip_extract_surface's mesh: vertices (V, 3) float32, triangles (T, 3) int32, normals and
# velocity (V, 3) float32 or None where not asked for
SurfaceMesh = collections.namedtuple("SurfaceMesh", ["vertices", "triangles", "normals", "velocity"])


RENDER_VELOCITY = 1   # SPH_HIP_RENDER_VELOCITY (include/sph_hip.h)

# sph_hip_render's frame: rgba (H, W, 4) uint8, depth (H, W) float32, normal (H, W, 3) float32,
# velocity (H, W, 3) float32 or None where not asked for, first_inside (H, W) int32; solid_id (H, W) int32 -
# the obstacle a pixel shows, -1 for none - from sph_hip_render_scene (render(..., solids=True)), else None
RenderResult = collections.namedtuple("RenderResult", ["rgba", "depth", "normal", "velocity", "first_inside",
                                                       "solid_id"], defaults=[None])


# sph_hip_render_scalars' frame: RenderResult's fields (solid_id None without solids) and scalar (H, W) float32,
# the value a tinted pixel's colour stands for, 0 on every other pixel
ScalarRenderResult = collections.namedtuple("ScalarRenderResult", RenderResult._fields + ("scalar",))

TINT_SURFACE, TINT_COLUMN = 0, 1   # SPH_HIP_TINT_* (include/sph_hip.h)
TINT_FLAT = 1
TINT_MODES = {"surface": TINT_SURFACE, "column": TINT_COLUMN}


class Camera:
    """sph_hip_camera: the eye and three fp32 vectors (include/sph_hip.h: renderer).  Pixel (px, py)
    looks along forward + a * right + b * up, a and b in (-1, 1) across the image."""

    def __init__(self, eye, forward, right, up):
        self.eye, self.forward, self.right, self.up = (np.array(v, np.float32).reshape(3)
                                                       for v in (eye, forward, right, up))

    @classmethod
    def look_at(cls, eye, target, up, fov_y_deg, width, height):
        """A pinhole camera at `eye` looking at `target`, `up` giving the image's vertical, with a
        vertical field of view of fov_y_deg and square pixels: computed in float64, then rounded to
        the four fp32 vectors (unit forward; right and up scaled to the image plane's half extents)."""
        e = np.asarray(eye, np.float64).reshape(3)
        f = np.asarray(target, np.float64).reshape(3) - e
        if not np.linalg.norm(f) > 0:
            raise ValueError("eye and target coincide")
        f = f / np.linalg.norm(f)
        r = np.cross(f, np.asarray(up, np.float64).reshape(3))
        if not np.linalg.norm(r) > 0:
            raise ValueError("up is parallel to the view direction")
        r = r / np.linalg.norm(r)
        u = np.cross(r, f)
        half_h = math.tan(math.radians(float(fov_y_deg)) / 2.0)
        half_w = half_h * float(width) / float(height)
        return cls(e, f, r * half_w, u * half_h)

    def as_struct(self):
        c = SphCamera()
        for name in ("eye", "forward", "right", "up"):
            getattr(c, name)[:] = [float(v) for v in getattr(self, name)]
        return c


def _lattice(origin, spacing, shape):
    """origin, spacing and shape of a lattice call as its three C arrays, and shape as a list"""
    o = (C.c_float * 3)(*[float(v) for v in origin])
    s = (C.c_float * 3)(*[float(v) for v in spacing])
    dims = [int(v) for v in shape]
    if len(dims) != 3 or len(o) != 3 or len(s) != 3:
        raise ValueError("origin, spacing and shape take three values each")
    return o, s, (C.c_int32 * 3)(*dims), dims


class SPH(Context):
    """The reference's `SPH` (src/sph.h:15-216) with the step executed on an MI355X.

    Differences that are part of the contract:
      * the particle count and the scene are arguments (the reference fixes N = M*1024 at
        compile time and always builds its sphere scene, src/sph.cpp:59,117);
      * `mode` selects the shipped sampled search (MODE_REF) or complete neighbourhoods
        (MODE_FULL; MODE_FULL_FAST = the same neighbourhoods and order with tolerance-mode pair
        arithmetic, see include/sph_hip.h);
      * the host `Particle` mirror is refreshed by `syncParticles()` / `getParticles()`
        rather than being written by every phase.
    """

    def __init__(self, particle_count, params=None, mode=MODE_FULL, device=0, capacity=None):
        self.mParticleCount = int(particle_count)
        self.mode = mode
        self._params = params.copy() if params is not None else default_params()
        cap = int(capacity) if capacity is not None else max(1, self.mParticleCount)
        super().__init__("sph_hip_create", C.byref(self._params), cap, int(mode), int(device))
        self.mSrcParticles = Particle(self.mParticleCount)
        self._mirror_fresh = False
        self._capacity = cap
        self._ports_set = False   # some emitter or sink is set
        self._had_ports = False   # ... or was since the last upload: the mirror holds the live rows by id

    # ---- scene ------------------------------------------------------------------------------
    def setParticles(self, position, velocity, mass):
        """Fill Particle::mPosition / mVelocity / mMass (what the reference's constructor and
        initParticlePolitionsSphere do, src/sph.cpp:105-108, 361-425) and upload."""
        pos = np.ascontiguousarray(position, np.float32).reshape(-1)
        vel = np.ascontiguousarray(velocity, np.float32).reshape(-1)
        m = np.ascontiguousarray(mass, np.float32).reshape(-1)
        n = m.size
        if pos.size != 3 * n or vel.size != 3 * n:
            raise ValueError("position/velocity must hold 3 floats per particle")
        if n != self.mParticleCount:
            self.mParticleCount = n
            self.mSrcParticles = Particle(n)
        self.mSrcParticles.mPosition[:] = pos
        self.mSrcParticles.mVelocity[:] = vel
        self.mSrcParticles.mMass[:] = m
        self.call("sph_hip_upload", n, _ptr(pos), _ptr(vel), _ptr(m))
        self._mirror_fresh = False
        self._had_ports = self._ports_set   # (the lists survive an upload; the ids start over)

    def syncParticles(self):
        """Refresh the host `Particle` mirror from the device.  On a context that has had ports since its
        last upload the mirror is a new Particle of the live rows in ascending id order, with the ids in mId
        (and no mMass: the masses are the emitters' and the upload's)."""
        if self._had_ports:
            return self._sync_live()
        p = self.mSrcParticles
        self.call("sph_hip_download", _ptr(p.mPosition), _ptr(p.mVelocity), _ptr(p.mDensity),
                  _ptr(p.mAcceleration), _ptr(p.mNeighborCount))
        self._mirror_fresh = True
        return p

    # ---- public getters (reference src/sph.cpp:1172-1289) -------------------------------------
    def getParticles(self):
        if not self._mirror_fresh:
            self.syncParticles()
        return self.mSrcParticles

    def getParticleCount(self):
        """The particle count: on a context that has had ports the live count, read from the device."""
        if self._had_ports:
            self.mParticleCount = self.getPorts()[0].live
        return self.mParticleCount

    # ---- ports (sph_hip_set_ports) ---------------------------------------------------------------
    def setPorts(self, emitters=(), sinks=()):
        """Replace the emitters and sinks (ports.Emitter / ports.Sink, at most 8 of each; none clears them):
        from the next step on the sinks remove what stands inside them at the start of a step and the emitters
        append their layers (include/sph_hip.h: ports).  The schedule and the totals start at 0.  Single
        contexts only."""
        ea, ne = _P.as_emitter_array(emitters)
        sa, ns = _P.as_sink_array(sinks)
        self.call("sph_hip_set_ports", ea, ne, sa, ns)
        self._ports_set = ne > 0 or ns > 0
        self._had_ports = self._had_ports or self._ports_set
        self._mirror_fresh = False

    def getPorts(self):
        """(PortTotals(emitted, removed, live, next_id), [Emitter], [Sink]) after every step enqueued so far
        (sph_hip_get_ports; synchronises)."""
        ea = (_P.SphEmitter * _P.MAX_EMITTERS)()
        sa = (_P.SphSink * _P.MAX_SINKS)()
        emitted = np.zeros(_P.MAX_EMITTERS, np.int64)
        removed = np.zeros(_P.MAX_SINKS, np.int64)
        live, next_id = C.c_int32(), C.c_uint32()
        r = self.call("sph_hip_get_ports", ea, sa, _P.MAX_EMITTERS, _P.MAX_SINKS, _ptr(emitted), _ptr(removed),
                      C.byref(live), C.byref(next_id))
        ne, ns = r & 0xFF, r >> 8
        return (_P.PortTotals(emitted[:ne].copy(), removed[:ns].copy(), live.value, next_id.value),
                [_P.emitter_from_struct(ea[i]) for i in range(ne)], [_P.sink_from_struct(sa[i]) for i in range(ns)])

    def downloadLive(self):
        """The live particles in device order (sph_hip_download_live; synchronises): (ids uint32 [n], pos [3n],
        vel [3n], density [n], acc [3n], neighbour count [n])."""
        cap = self._capacity
        rows = C.c_int32()
        ids = np.zeros(cap, np.uint32)
        pos, vel, acc = (np.zeros(3 * cap, np.float32) for _ in range(3))
        rho = np.zeros(cap, np.float32)
        cnt = np.zeros(cap, np.int32)
        self.call("sph_hip_download_live", cap, C.byref(rows), _ptr(ids), _ptr(pos), _ptr(vel), _ptr(rho), _ptr(acc),
                  _ptr(cnt))
        n = rows.value
        return ids[:n], pos[:3 * n], vel[:3 * n], rho[:n], acc[:3 * n], cnt[:n]

    def _sync_live(self):
        ids, pos, vel, rho, acc, cnt = self.downloadLive()
        order = np.argsort(ids, kind="stable")
        p = Particle(ids.size)
        p.mId = ids[order]
        p.mPosition[:] = pos.reshape(-1, 3)[order].reshape(-1)
        p.mVelocity[:] = vel.reshape(-1, 3)[order].reshape(-1)
        p.mAcceleration[:] = acc.reshape(-1, 3)[order].reshape(-1)
        p.mDensity[:] = rho[order]
        p.mNeighborCount[:] = cnt[order]
        self.mSrcParticles = p
        self.mParticleCount = ids.size
        self._mirror_fresh = True
        return p

    def getGridCellCounts(self):
        return self._params.cells_x, self._params.cells_y, self._params.cells_z

    def getParticleBounds(self):
        return self._params.max_x, self._params.max_y, self._params.max_z

    def getInteractionRadius2(self):
        return self._params.hscaled2

    def getCellSize(self):
        return self._params.cell_size

    def getGrid(self):
        """Per-voxel occupancy: what callers take from getGrid()[i].count()
        (reference src/visualization.cpp:178-193)."""
        p = self._params
        if self.mode == MODE_REF:
            ncells = p.cells_x * p.cells_y * p.cells_z
        else:
            ncells = p.full_cells_x * p.full_cells_y * p.full_cells_z
        counts = np.zeros(ncells, np.int32)
        self.call("sph_hip_download_grid_counts", _ptr(counts))
        return counts

    def getParams(self):
        return self._params.copy()

    def _push(self):
        self.call("sph_hip_set_params", C.byref(self._params))

    def getGravity(self):
        return tuple(self._params.gravity)

    def setGravity(self, gravity):
        for c in range(3):
            self._params.gravity[c] = gravity[c]
        self._push()

    def getStiffness(self):
        return self._params.stiffness

    def setStiffness(self, stiffness):
        self._params.stiffness = stiffness
        self._push()

    def getViscosityScalar(self):
        return self._params.viscosity

    def setViscosityScalar(self, viscosity):
        self._params.viscosity = viscosity
        self._push()

    def getTimeStep(self):
        return self._params.time_step

    def setTimeStep(self, time_step):
        self._params.time_step = time_step
        self._push()

    def getDamping(self):
        return self._params.damping

    def setDamping(self, damping):
        self._params.damping = damping
        self._push()

    def getCflLimit(self):
        return self._params.cfl_limit

    def setCflLimit(self, cfl_limit):
        # reference src/sph.cpp:1237-1241: also refreshes the squared limit, in fp32
        self._params.cfl_limit = cfl_limit
        lim = np.float32(self._params.cfl_limit)
        self._params.cfl_limit2 = float(lim * lim)
        self._push()

    setObstacles, getObstacles = Context.set_obstacles, Context.get_obstacles
    setObstacleMotion, getObstacleMotion = Context.set_obstacle_motion, Context.get_obstacle_motion
    setObstaclePaths, getObstaclePaths = Context.set_obstacle_paths, Context.get_obstacle_paths
    recordLoads, getLoads = Context.record_loads, Context.get_loads

    def setBodies(self, bodies, quantum_log2=-24):
        """Make obstacles free bodies that the fluid's loads move (sph_hip_set_bodies): one obstacles.Body per
        obstacle, None for one that is not a body; an empty list clears the bodies.  quantum_log2 is the
        quantum of the load rows the bodies consume: a recording made meanwhile must use the same.  Single
        contexts only: a body needs the sum of all slabs' rows before any slab may advance it."""
        arr, n = _O.as_body_array(bodies)
        self.call("sph_hip_set_bodies", arr, n, int(quantum_log2))

    def getBodies(self):
        """The bodies and their state after every step enqueued so far, as a Bodies (sph_hip_get_bodies;
        synchronises)."""
        lst = (_O.SphBody * _O.MAX_OBSTACLES)()
        st = (_O.SphBodyState * _O.MAX_OBSTACLES)()
        n = self.call("sph_hip_get_bodies", lst, st, _O.MAX_OBSTACLES)
        return Bodies([_O.body_from_struct(lst[i]) for i in range(n)],
                      np.array([list(st[i].displacement) for i in range(n)], np.float32).reshape(n, 3),
                      np.array([list(st[i].velocity) for i in range(n)], np.float32).reshape(n, 3),
                      np.array([st[i].skipped for i in range(n)], np.int64),
                      np.array([st[i].steps for i in range(n)], np.int64))

    # ---- tracers (sph_hip_set_tracers) ------------------------------------------------------------
    def setTracers(self, points):
        """Replace the tracers with markers at `points` ((n, 3) float32; an empty list clears them): massless
        points that every step from here on advances on the device by the midpoint rule in the fluid's
        Shepard velocity (include/sph_hip.h: tracers).  Counts start at zero; a recording ends."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        self.call("sph_hip_set_tracers", pts.shape[0], _ptr(pts))

    def tracerCount(self):
        return self.call("sph_hip_tracer_count")

    def getTracers(self):
        """The tracers after every step enqueued so far, in the order given to setTracers, as a Tracers
        (sph_hip_get_tracers; synchronises)."""
        n = self.tracerCount()
        pos = np.zeros((n, 3), np.float32)
        wet = np.zeros(n, np.int32)
        dry = np.zeros(n, np.int32)
        self.call("sph_hip_get_tracers", 0, n, _ptr(pos), _ptr(wet), _ptr(dry))
        return Tracers(pos, wet, dry)

    def recordTracers(self, rows, every=1):
        """Keep the tracers' positions after the next step and every `every`-th after it, `rows` times, on
        the device (sph_hip_record_tracers); rows = 0 stops and frees the recording."""
        self.call("sph_hip_record_tracers", int(rows), int(every))

    def getTracerPath(self):
        """The rows recorded so far, as a TracerPath: steps[rows] (numbered from recordTracers, the first
        step is 1) and positions[rows, n, 3] (sph_hip_get_tracer_path; synchronises)."""
        rows = self.call("sph_hip_get_tracer_path", 0, 0, None, None)
        n = self.tracerCount()
        steps = np.zeros(rows, np.int32)
        pos = np.zeros((rows, n, 3), np.float32)
        if rows:
            self.call("sph_hip_get_tracer_path", 0, rows, _ptr(pos), _ptr(steps))
        return TracerPath(steps, pos)

    # ---- gauges (sph_hip_set_gauges) -------------------------------------------------------------
    def setGauges(self, gauges):
        """Replace the gauges with `gauges` (gauges.PointGauge / ColumnGauge / SectionGauge / PressureGauge /
        PressurePatch; an empty list clears them): fixed instruments evaluated on the device (include/sph_hip.h:
        gauges).  A recording ends."""
        arr, n = _G.as_array(gauges)
        self.call("sph_hip_set_gauges", arr, n)

    def getGauges(self):
        """The gauges as they were set, in list order."""
        n = self.call("sph_hip_get_gauges", None, 0)
        if n == 0:
            return []
        arr = (_G.SphGauge * n)()
        self.call("sph_hip_get_gauges", arr, n)
        return [_G.from_struct(arr[i]) for i in range(n)]

    def _gauge_kinds(self, n):
        arr = (_G.SphGauge * max(n, 1))()
        if n:
            self.call("sph_hip_get_gauges", arr, n)
        return tuple(int(arr[i].kind) for i in range(n))

    def readGauges(self):
        """Every gauge evaluated now, in the current state, as a GaugeReadings (sph_hip_read_gauges; synchronises;
        the simulation is not changed by the call)."""
        n = self.call("sph_hip_get_gauges", None, 0)
        out = np.zeros(n, _G.READING)
        if n:
            self.call("sph_hip_read_gauges", _ptr(out))
        got = _G.GaugeReadings(out["v"].copy(), out["n"].copy(), out["k"].copy())
        got.kinds = self._gauge_kinds(n)
        return got

    def recordGauges(self, rows, every=1):
        """Keep the gauges' readings in the state at this call and after every `every`-th step from it, `rows`
        times, on the device (sph_hip_record_gauges); rows = 0 stops and frees the recording."""
        self.call("sph_hip_record_gauges", int(rows), int(every))

    def getGaugeRecord(self):
        """The rows recorded so far, as a GaugeRecord: steps[rows] (the steps completed since recordGauges when
        the row was read) and the readings v[rows, n, 4], n[rows, n], k[rows, n] (sph_hip_get_gauge_record;
        synchronises)."""
        rows = self.call("sph_hip_get_gauge_record", 0, 0, None, None)
        n = self.call("sph_hip_get_gauges", None, 0)
        steps = np.zeros(rows, np.int32)
        out = np.zeros((rows, n), _G.READING)
        if rows:
            self.call("sph_hip_get_gauge_record", 0, rows, _ptr(out), _ptr(steps))
        got = _G.GaugeRecord(steps, out["v"].copy(), out["n"].copy(), out["k"].copy())
        got.kinds = self._gauge_kinds(n)
        return got

    # ---- slots ---------------------------------------------------------------------------------
    def step(self):
        """SPH::step() (reference src/sph.cpp:190-304)."""
        self.call("sph_hip_step")
        self._mirror_fresh = False

    def run(self, steps):
        """`steps` steps queued back to back (SPH::run's loop body, src/sph.cpp:171-181)."""
        self.call("sph_hip_run", int(steps))
        self._mirror_fresh = False

    def runToFiles(self, total_steps, outdir="out"):
        """SPH::run() (reference src/sph.cpp:149-187, 203, 232): `total_steps + 1` steps, one line
        per step in energy.txt / angularmomentum.txt / timing.txt / neighbors.txt with the
        reference's headers and column order.  Differences: times are fractional milliseconds
        (the reference truncates to int), KE/PE are summed in a fixed order in f64."""
        import os
        os.makedirs(outdir, exist_ok=True)
        with open(os.path.join(outdir, "energy.txt"), "w") as fe, \
                open(os.path.join(outdir, "angularmomentum.txt"), "w") as fl, \
                open(os.path.join(outdir, "timing.txt"), "w") as ft, \
                open(os.path.join(outdir, "neighbors.txt"), "w") as fn:
            fe.write("Step, Kinetic Energy, Potential Energy, Total Energy\n")
            fl.write("Step, Angular Momentum\n")
            ft.write("Step, Voxelize, Find Neighbors, Compute Density, Compute Pressure, "
                     "Compute Acceleration, Integrate\n")
            for s in range(int(total_steps) + 1):
                self.step()
                ke, pe = self.energy()
                fe.write("%d, %.9g, %.9g, %.9g\n" % (s, ke, pe, np.float32(ke) + np.float32(pe)))
                fl.write("%d, 0\n" % s)          # mAngularMomentumTotal is never accumulated
                ft.write("%d, %s\n" % (s, ", ".join("%.4f" % v for v in self.elapsed())))
                fn.write("%d, %d, %d\n" % self.neighborStats())

    def setArithmetic(self, arithmetic):
        self.set_arithmetic(arithmetic)
        self._mirror_fresh = False

    def getArithmetic(self):
        return self._lib.sph_hip_get_arithmetic(self._ctx)

    # ---- protected pipeline (reference src/sph.h:96-112) ----------------------------------------
    def voxelizeParticles(self):
        self.call("sph_hip_voxelize")
        self._mirror_fresh = False

    def findNeighbors(self):
        self.call("sph_hip_find_neighbors")
        self._mirror_fresh = False

    def computeDensity(self):
        self.call("sph_hip_compute_density")
        self._mirror_fresh = False

    def computeAcceleration(self):
        self.call("sph_hip_compute_acceleration")
        self._mirror_fresh = False

    def integrate(self):
        self.call("sph_hip_integrate")
        self._mirror_fresh = False

    # ---- field sampler (sph_hip_sample_points / sph_hip_sample_lattice) ---------------------------
    def sampleFields(self, points, velocity=True):
        """SPH interpolation of the current state at `points` ((n, 3) float32): (density[n],
        velocity[n, 3] or None, count[n]) as numpy arrays.  The probe sums every particle within h,
        its own included where a probe sits on one (include/sph_hip.h: field sampler); the
        simulation is not changed by the call."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n = pts.shape[0]
        rho = np.zeros(n, np.float32)
        vel = np.zeros((n, 3), np.float32) if velocity else None
        cnt = np.zeros(n, np.int32)
        self.call("sph_hip_sample_points", n, _ptr(pts), _ptr(rho), _ptr(vel), _ptr(cnt))
        return rho, vel, cnt

    def sampleLattice(self, origin, spacing, shape, velocity=True):
        """The same sums on the lattice origin + i * spacing (fp32, per axis), shape = (nx, ny, nz):
        (density[nz, ny, nx], velocity[nz, ny, nx, 3] or None, count[nz, ny, nx])."""
        o, s, d, dims = _lattice(origin, spacing, shape)
        grid = (max(dims[2], 0), max(dims[1], 0), max(dims[0], 0))
        total = grid[0] * grid[1] * grid[2]
        if total >= 2 ** 31:
            raise ValueError("a lattice of more than 2^31 - 1 points")
        rho = np.zeros(grid, np.float32)
        vel = np.zeros(grid + (3,), np.float32) if velocity else None
        cnt = np.zeros(grid, np.int32)
        self.call("sph_hip_sample_lattice", C.byref(o), C.byref(s), C.byref(d), _ptr(rho), _ptr(vel),
                  _ptr(cnt))
        return rho, vel, cnt

    def samplePressure(self, points):
        """The pressure of the current state at `points` ((n, 3) float32): (pressure[n], density[n], count[n]).
        Every particle's pressure is (rho_j - rho0) * stiffness with the density pass's rho_j of this state, not
        clamped; a probe's is their Shepard-normalised sum over the sampler's members (include/sph_hip.h:
        pressure readings).  The simulation is not changed by the call."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n = pts.shape[0]
        prs = np.zeros(n, np.float32)
        rho = np.zeros(n, np.float32)
        cnt = np.zeros(n, np.int32)
        self.call("sph_hip_sample_pressure_points", n, _ptr(pts), _ptr(prs), _ptr(rho), _ptr(cnt))
        return prs, rho, cnt

    def samplePressureLattice(self, origin, spacing, shape):
        """The same on sampleLattice's lattice, shape = (nx, ny, nz): (pressure[nz, ny, nx],
        density[nz, ny, nx], count[nz, ny, nx])."""
        o, s, d, dims = _lattice(origin, spacing, shape)
        grid = (max(dims[2], 0), max(dims[1], 0), max(dims[0], 0))
        if grid[0] * grid[1] * grid[2] >= 2 ** 31:
            raise ValueError("a lattice of more than 2^31 - 1 points")
        prs = np.zeros(grid, np.float32)
        rho = np.zeros(grid, np.float32)
        cnt = np.zeros(grid, np.int32)
        self.call("sph_hip_sample_pressure_lattice", C.byref(o), C.byref(s), C.byref(d), _ptr(prs), _ptr(rho),
                  _ptr(cnt))
        return prs, rho, cnt

    # ---- carried scalars (sph_hip_set_scalars) --------------------------------------------------
    def setScalars(self, values, diffusivity=0.0):
        """Give every particle its carried scalars: `values` is (n,) or (n, c) with c <= 4 in particle order,
        padded with zeros to four channels; `diffusivity` is one kappa for every channel or up to four of
        them (padded with zeros; a channel with kappa 0 is only carried, its bits kept).  values=None
        switches the scalars off.  From the next step on every step moves them with the fluid and diffuses
        them between neighbours (include/sph_hip.h: carried scalars), explicitly: per channel a step is a
        convex combination of a particle's value and its neighbours' while
        dt * kappa * sum_j (m_j / rho_j) * kernel3 * (h - d_ij) <= 1, and nothing polices that condition - next to
        a particle of the spray, whose density is next to nothing, it fails for any kappa > 0 and a diffusing
        channel can overflow (scenes.scalar_stable_kappa gives a kappa for the bulk).  No particle changes by a bit.  A new setParticles drops the scalars and the sources."""
        if values is None:
            self.call("sph_hip_set_scalars", 0, None, None)
            return
        v = _S.pad_values(values)
        k = _S.pad_diffusivity(diffusivity)
        self.call("sph_hip_set_scalars", v.shape[0], _ptr(v), _ptr(k))

    def getScalars(self):
        """The carried scalars after every step enqueued so far, float32 (n, 4) in particle order
        (sph_hip_get_scalars; synchronises)."""
        n = self.mParticleCount
        out = np.zeros((n, _S.CHANNELS), np.float32)
        self.call("sph_hip_get_scalars", 0, n, _ptr(out))
        return out

    def setScalarSources(self, sources):
        """Replace the scalar sources with `sources` (scalars.ScalarSource.hold / .add, at most 8; an empty
        list clears them), for the steps enqueued from now on."""
        arr, n = _S.as_array(sources)
        self.call("sph_hip_set_scalar_sources", arr, n)

    def getScalarSources(self):
        arr = (_S.SphScalarSource * _S.MAX_SOURCES)()
        n = self.call("sph_hip_get_scalar_sources", arr, _S.MAX_SOURCES)
        return [_S.from_struct(arr[i]) for i in range(n)]

    # ---- buoyancy (sph_hip_set_buoyancy) ----------------------------------------------------------
    def setBuoyancy(self, buoyancy):
        """Let the carried scalars change a particle's weight from the next enqueued step on
        (scalars.Buoyancy; include/sph_hip.h: buoyancy): a particle with the excess s = sum of beta[c] *
        (T_c - reference[c]) takes (-s) * gravity on top of its own acceleration.  A Buoyancy without a gravity
        of its own takes the context's params.gravity as it stands now.  None, or a beta of zeros, switches it
        off.  Needs setScalars first; a new setParticles, and setScalars(None), drop it."""
        if buoyancy is None:
            self.call("sph_hip_set_buoyancy", None)
            return
        b = buoyancy.with_gravity(self.getGravity()).to_struct()
        self.call("sph_hip_set_buoyancy", C.byref(b))

    def getBuoyancy(self):
        """The Buoyancy in force, or None."""
        b = _S.SphBuoyancy()
        return _S.buoyancy_from_struct(b) if self.call("sph_hip_get_buoyancy", C.byref(b)) == 1 else None

    # ---- cohesion (sph_hip_set_cohesion) ----------------------------------------------------------
    def setCohesion(self, gamma):
        """A pairwise surface tension from the next enqueued step on (include/sph_hip.h: cohesion): every particle
        takes -gamma * sum_j t_j * (r_i - r_j) on top of its own acceleration, t_j the density sum's pair term - it
        cancels inside the fluid and pulls a free surface inward.  None or 0 switches it off; a negative gamma
        pushes apart.  FULL and FULL_FAST contexts without ports; a new setParticles drops it."""
        self.call("sph_hip_set_cohesion", C.c_float(0.0 if gamma is None else float(gamma)))

    def getCohesion(self):
        """The gamma in force, 0.0 when cohesion is off."""
        g = C.c_float(0.0)
        self.call("sph_hip_get_cohesion", C.byref(g))
        return float(g.value)

    # ---- xsph (sph_hip_set_xsph) ------------------------------------------------------------------
    def setVelocitySmoothing(self, eps):
        """XSPH from the next enqueued step on (include/sph_hip.h: xsph): every particle's velocity moves by
        eps * sum_j g_ij * (v_j - v_i) towards its neighbours' weighted mean, behind the acceleration pass and in
        front of the integrate - velocity noise decays, a uniform motion and the momentum stay.  eps in [0, 1];
        None or 0 switches it off.  FULL and FULL_FAST contexts without ports; a new setParticles drops it."""
        self.call("sph_hip_set_xsph", C.c_float(0.0 if eps is None else float(eps)))

    def getVelocitySmoothing(self):
        """The eps in force, 0.0 when the smoothing is off."""
        e = C.c_float(0.0)
        self.call("sph_hip_get_xsph", C.byref(e))
        return float(e.value)

    # ---- viscous stress (sph_hip_set_viscous_stress) ------------------------------------------------
    def setViscousStress(self, mu, law=None):
        """A pairwise viscous force of the dynamic viscosity `mu` from the next enqueued step on (include/sph_hip.h:
        viscous stress): every particle takes (1 / m_i) * sum_j mu_ij * V_i * V_j * L(d_ij) * (v_j - v_i) on top of
        its own acceleration, V = m / rho and L the viscosity Laplacian - velocity differences decay, a uniform
        motion keeps its bits, and the force addends of a pair negate each other for any masses.  With a `law`
        (viscosity.ViscosityLaw) mu is multiplied per particle by the law's factor of a carried channel and a pair
        takes the mean of its two; a law needs setScalars first, and setScalars(None) drops it and keeps mu.  mu is
        finite and >= 0; None or 0 switches the term off.  The scheme is explicit: a step damps while
        dt * (1 / m_i) * sum_j mu_ij V_i V_j L <= 1 for every particle, and nothing polices that
        (scenes.viscous_stable_mu gives a mu for the bulk).  FULL and FULL_FAST contexts without ports; a new
        setParticles drops the setting."""
        q = None if law is None else C.byref(law.to_struct())
        self.call("sph_hip_set_viscous_stress", C.c_float(0.0 if mu is None else float(mu)), q)

    def getViscousStress(self):
        """(mu, law): the mu in force, 0.0 when the term is off, and its ViscosityLaw or None."""
        mu, law, have = C.c_float(0.0), _VS.SphViscosityLaw(), C.c_int(0)
        self.call("sph_hip_get_viscous_stress", C.byref(mu), C.byref(law), C.byref(have))
        return float(mu.value), (_VS.from_struct(law) if have.value else None)

    # ---- implicit viscous stress (sph_hip_set_viscous_implicit) ---------------------------------------
    def setViscousSolver(self, sweeps):
        """How the viscous stress of setViscousStress is taken from the next enqueued step on (include/sph_hip.h:
        implicit viscous stress).  None or 0: explicitly, as an acceleration - the default, bounded only while
        dt * (1 / m_i) * sum_j mu_ij V_i V_j L <= 1.  1 .. viscosity.MAX_SWEEPS: implicitly, by that many Jacobi
        sweeps of backward Euler on the same pair operator, which write the velocities: every sweep leaves a convex
        combination of a particle's own velocity and its neighbours', so no velocity component leaves the range of
        the step's velocities for ANY mu >= 0 and dt (provided no neighbour stands beyond hscaled).  The price:
        where N = dt * (1 / m_i) * sum_j mu_ij V_i V_j L >> 1 the error contracts only like N / (1 + N) per sweep,
        so too few sweeps act like a smaller mu (scenes.viscous_number gives the bulk's N); and a truncated solve
        does not conserve momentum pair by pair - the defect falls with the sweeps and vanishes at convergence (on
        scenes.shear_layer(3000, 0.5), momentum 749.5, at 5 times the bulk's limit: 1.07 after 2 sweeps, 0.064 after
        16; at 50 times 1.85 and 1.79).
        K sweeps are K + 1 launches per step.  The count takes effect only while mu != 0; setScalars(None) keeps
        it, a new setParticles drops it.  FULL and FULL_FAST contexts without ports."""
        self.call("sph_hip_set_viscous_implicit", C.c_int(0 if sweeps is None else int(sweeps)))

    def getViscousSolver(self):
        """The sweep count in force, 0 when the viscous stress is taken explicitly."""
        k = C.c_int(0)
        self.call("sph_hip_get_viscous_implicit", C.byref(k))
        return int(k.value)

    # ---- step monitor (sph_hip_record_monitor) ------------------------------------------------------
    def recordMonitor(self, rows, every=1, quantum_log2=_M.QUANTUM_DEFAULT):
        """Keep a row of stability and conservation figures for the step after this call and every `every`-th
        step from it, `rows` times, on the device (include/sph_hip.h: step monitor): peak speed and acceleration,
        the density range, neighbour counts, particles that are not finite, the carried channels' range and
        diffusion sum, and momentum, kinetic energy and mass as integer sums in quanta of 2^quantum_log2.  Queued
        steps stay queued; rows = 0 stops and frees the recording.  FULL and FULL_FAST contexts without ports."""
        self.call("sph_hip_record_monitor", int(rows), int(every), int(quantum_log2))
        self._monitor_quantum = int(quantum_log2)

    def getMonitorRecord(self):
        """The rows filled so far, as a monitor.MonitorRecord (sph_hip_get_monitor_record; synchronises)."""
        rows = self.call("sph_hip_get_monitor_record", 0, 0, None, None)
        out = np.zeros(rows, _M.ROW)
        steps = np.zeros(rows, np.int32)
        if rows:
            self.call("sph_hip_get_monitor_record", 0, rows, _ptr(out), _ptr(steps))
        return _M.MonitorRecord(out, steps, getattr(self, "_monitor_quantum", _M.QUANTUM_DEFAULT))

    def sampleScalars(self, points):
        """The carried scalars of the current state at `points` ((n, 3) float32): (channels[n, 4], density[n],
        count[n]) - the Shepard-normalised sums over the sampler's members, 0 where there are none.  The
        simulation is not changed by the call."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n = pts.shape[0]
        chan = np.zeros((n, _S.CHANNELS), np.float32)
        rho = np.zeros(n, np.float32)
        cnt = np.zeros(n, np.int32)
        self.call("sph_hip_sample_scalars_points", n, _ptr(pts), _ptr(chan), _ptr(rho), _ptr(cnt))
        return chan, rho, cnt

    def sampleScalarLattice(self, origin, spacing, shape):
        """The same on sampleLattice's lattice, shape = (nx, ny, nz): (channels[nz, ny, nx, 4],
        density[nz, ny, nx], count[nz, ny, nx])."""
        o, s, d, dims = _lattice(origin, spacing, shape)
        grid = (max(dims[2], 0), max(dims[1], 0), max(dims[0], 0))
        if grid[0] * grid[1] * grid[2] >= 2 ** 31:
            raise ValueError("a lattice of more than 2^31 - 1 points")
        chan = np.zeros(grid + (_S.CHANNELS,), np.float32)
        rho = np.zeros(grid, np.float32)
        cnt = np.zeros(grid, np.int32)
        self.call("sph_hip_sample_scalars_lattice", C.byref(o), C.byref(s), C.byref(d), _ptr(chan), _ptr(rho),
                  _ptr(cnt))
        return chan, rho, cnt

    def extractSurface(self, origin, spacing, shape, iso, normals=True, velocity=False):
        """The surface {density > iso} of the lattice sampleLattice(origin, spacing, shape) would
        give, meshed on the device (include/sph_hip.h: iso-surface extractor): a SurfaceMesh of
        numpy arrays.  The mesh stays in the context until the next extraction."""
        o, s, d, _ = _lattice(origin, spacing, shape)
        flags = (SURFACE_NORMALS if normals else 0) | (SURFACE_VELOCITY if velocity else 0)
        counts = (C.c_int32 * 2)()
        self.call("sph_hip_extract_surface", C.byref(o), C.byref(s), C.byref(d), float(iso), flags,
                  C.byref(counts))
        nv, nt = counts[0], counts[1]
        vtx = np.zeros((nv, 3), np.float32)
        tri = np.zeros((nt, 3), np.int32)
        nrm = np.zeros((nv, 3), np.float32) if normals else None
        vel = np.zeros((nv, 3), np.float32) if velocity else None
        self.call("sph_hip_download_surface", _ptr(vtx), _ptr(nrm), _ptr(vel), _ptr(tri))
        return SurfaceMesh(vtx, tri, nrm, vel)

    # ---- renderer (sph_hip_render) ------------------------------------------------------------------
    def renderParams(self, iso, step=None, refine=8, grad_step=None, box=None, light=(0.4, 0.8, 0.45),
                     albedo=(0.25, 0.55, 0.9), ambient=0.2, diffuse=0.8, background=(0, 0, 0, 255),
                     max_samples=1 << 16):
        """The sph_hip_render_params of render(...)'s arguments, defaults filled in."""
        f = np.float32
        h = f(self._params.h)
        if box is None:
            top = np.array(self.getParticleBounds(), f)
            box = (np.full(3, f(0.0) - h, f), (top + h).astype(f))
        rp = SphRenderParams()
        rp.box_lo[:] = [float(v) for v in np.asarray(box[0], f).reshape(3)]
        rp.box_hi[:] = [float(v) for v in np.asarray(box[1], f).reshape(3)]
        rp.step = float(f(0.5) * h) if step is None else float(step)
        rp.iso = float(iso)
        rp.refine = int(refine)
        rp.grad_step = float(f(0.5) * h) if grad_step is None else float(grad_step)
        rp.light[:] = [float(v) for v in light]
        rp.albedo[:] = [float(v) for v in albedo]
        rp.ambient = float(ambient)
        rp.diffuse = float(diffuse)
        rp.background[:] = [int(v) for v in background]
        rp.max_samples = int(max_samples)
        return rp

    def render(self, camera, width, height, iso, step=None, refine=8, grad_step=None, box=None,
               light=(0.4, 0.8, 0.45), albedo=(0.25, 0.55, 0.9), ambient=0.2, diffuse=0.8,
               background=(0, 0, 0, 255), velocity=False, max_samples=1 << 16, solids=False,
               solid_albedo=(0.72, 0.72, 0.72), solid_colors=None, solid_ambient=None, solid_diffuse=None):
        """Ray-march the surface {density > iso} of the current state into a width x height image on
        the device (include/sph_hip.h: renderer): a RenderResult of numpy arrays.  step and
        grad_step default to h / 2, the box to the particle bounds [0, max] grown by h on every
        side; the simulation is not changed by the call.
        solids=True draws the context's obstacles, where they stand now, into the frame with the fluid
        (include/sph_hip.h: scene renderer) and fills RenderResult.solid_id: solid_albedo for every
        solid, or solid_colors, one RGB albedo per obstacle; solid_ambient / solid_diffuse default to the
        fluid's."""
        rp, W, H, out, cam, flags = self._frame_args(camera, width, height, iso, step, refine, grad_step, box, light,
                                                     albedo, ambient, diffuse, background, velocity, max_samples)
        rgba, depth, normal, vel, first = out
        if not solids:
            self.call("sph_hip_render", C.byref(cam), C.byref(rp), W, H, flags,
                      _ptr(rgba), _ptr(depth), _ptr(normal), _ptr(vel), _ptr(first))
            return RenderResult(rgba, depth, normal, vel, first)
        sp, colors = self._scene_args(ambient, diffuse, solid_albedo, solid_colors, solid_ambient, solid_diffuse)
        solid_id = np.zeros((H, W), np.int32)
        self.call("sph_hip_render_scene", C.byref(cam), C.byref(rp), C.byref(sp), _ptr(colors),
                  0 if colors is None else colors.shape[0], W, H, flags,
                  _ptr(rgba), _ptr(depth), _ptr(normal), _ptr(vel), _ptr(first), _ptr(solid_id))
        return RenderResult(rgba, depth, normal, vel, first, solid_id)

    def _frame_args(self, camera, width, height, iso, step, refine, grad_step, box, light, albedo, ambient, diffuse,
                    background, velocity, max_samples):
        """What every frame call is given: (params, W, H, (rgba, depth, normal, velocity or None, first_inside),
        camera struct, flags)."""
        rp = self.renderParams(iso, step, refine, grad_step, box, light, albedo, ambient, diffuse, background,
                               max_samples)
        W, H = int(width), int(height)
        if W < 1 or H < 1:
            raise ValueError("width and height must be positive")
        out = (np.zeros((H, W, 4), np.uint8), np.zeros((H, W), np.float32), np.zeros((H, W, 3), np.float32),
               np.zeros((H, W, 3), np.float32) if velocity else None, np.zeros((H, W), np.int32))
        return rp, W, H, out, camera.as_struct(), RENDER_VELOCITY if velocity else 0

    @staticmethod
    def _scene_args(ambient, diffuse, solid_albedo, solid_colors, solid_ambient, solid_diffuse):
        """(scene params, per-solid albedos (n, 3) or None) of a frame with the solids drawn"""
        sp = SphSceneParams()
        sp.albedo[:] = [float(v) for v in solid_albedo]
        sp.ambient = float(ambient if solid_ambient is None else solid_ambient)
        sp.diffuse = float(diffuse if solid_diffuse is None else solid_diffuse)
        colors = None if solid_colors is None else np.ascontiguousarray(solid_colors, np.float32).reshape(-1, 3)
        return sp, colors

    # ---- scalar renderer (sph_hip_render_scalars) -----------------------------------------------------
    def renderScalars(self, camera, width, height, iso, channel, value_range, colormap=None, mode="surface",
                      flat=False, solids=False, step=None, refine=8, grad_step=None, box=None,
                      light=(0.4, 0.8, 0.45), albedo=(0.25, 0.55, 0.9), ambient=0.2, diffuse=0.8,
                      background=(0, 0, 0, 255), velocity=False, max_samples=1 << 16,
                      solid_albedo=(0.72, 0.72, 0.72), solid_colors=None, solid_ambient=None, solid_diffuse=None):
        """render(...)'s frame with every pixel that shows fluid coloured by carried channel `channel` on the
        device (include/sph_hip.h: scalar renderer): a ScalarRenderResult, render's arrays plus .scalar.
        value_range = (lo, hi) are the values mapped onto the first and last row of `colormap`, an (n, 3)
        table of RGB in [0, 1] with 2 <= n <= 256 (colormaps.heat() by default).  mode "surface" colours a
        pixel by the channel at its hit point - what sampleScalars returns there; "column" by the channel
        integrated along the ray through the fluid from the surface to the end of `box` (with a channel
        that is 1 everywhere: the fluid's thickness), which shows what lies under the surface.  Solids do
        not clip a column.  flat=True leaves the Lambert factor out (for cut views, where rays enter inside
        the fluid).  The other arguments are render's; the simulation is not changed by the call."""
        return self._render_tinted("sph_hip_render_scalars", int(channel), camera, width, height, iso, value_range,
                                   colormap, mode, flat, solids, step, refine, grad_step, box, light, albedo, ambient,
                                   diffuse, background, velocity, max_samples, solid_albedo, solid_colors,
                                   solid_ambient, solid_diffuse)

    def _render_tinted(self, entry, channel, camera, width, height, iso, value_range, colormap, mode, flat, solids,
                       step, refine, grad_step, box, light, albedo, ambient, diffuse, background, velocity,
                       max_samples, solid_albedo, solid_colors, solid_ambient, solid_diffuse):
        """The tinted frame of renderScalars and renderVelocityGradients: `entry` is the C entry point, `channel`
        what its tint params carry."""
        if mode not in TINT_MODES:
            raise ValueError("mode must be 'surface' or 'column'")
        rp, W, H, out, cam, flags = self._frame_args(camera, width, height, iso, step, refine, grad_step, box, light,
                                                     albedo, ambient, diffuse, background, velocity, max_samples)
        rgba, depth, normal, vel, first = out
        table = np.ascontiguousarray(_CM.heat() if colormap is None else colormap, np.float32)
        if table.ndim != 2 or table.shape[1] != 3:
            raise ValueError("colormap must be an (n, 3) table")
        tp = SphTintParams()
        tp.channel = channel
        tp.mode = TINT_MODES[mode]
        tp.lo, tp.hi = float(value_range[0]), float(value_range[1])
        tp.n_colors = table.shape[0]
        tp.flags = TINT_FLAT if flat else 0
        scalar = np.zeros((H, W), np.float32)
        sp, colors, solid_id = None, None, None
        if solids:
            sp, colors = self._scene_args(ambient, diffuse, solid_albedo, solid_colors, solid_ambient, solid_diffuse)
            solid_id = np.zeros((H, W), np.int32)
        self.call(entry, C.byref(cam), C.byref(rp), None if sp is None else C.byref(sp),
                  _ptr(colors), 0 if colors is None else colors.shape[0], C.byref(tp), _ptr(table), W, H, flags,
                  _ptr(rgba), _ptr(depth), _ptr(normal), _ptr(vel), _ptr(first), _ptr(solid_id), _ptr(scalar))
        return ScalarRenderResult(rgba, depth, normal, vel, first, solid_id, scalar)

    # ---- velocity gradients (sph_hip_get_velocity_gradients) ---------------------------------------------
    def getVelocityGradients(self):
        """Vorticity, divergence, strain rate, Q and |vorticity| of every particle of the current state, in particle
        order, as a velgrad.VelocityGradients (include/sph_hip.h: velocity gradients; synchronises): a weighted
        least-squares fit of the velocity over each particle's neighbours, exact on a linear field.  A particle
        with too few or nearly coplanar neighbours has .valid False and zeros.  The simulation is not changed by
        the call.  FULL and FULL_FAST contexts whose ids ports have not changed."""
        n = self.call("sph_hip_particle_count")      # (0 before the first setParticles)
        rot = np.zeros((n, 4), np.float32)
        inv = np.zeros((n, 4), np.float32)
        self.call("sph_hip_get_velocity_gradients", 0, n, _ptr(rot), _ptr(inv))
        return _V.VelocityGradients(rot, inv)

    def sampleVelocityGradients(self, points):
        """The same quantities at `points` ((n, 3) float32): a VelocityGradients with .density and .count, every
        value the Shepard-normalised sum over the sampler's members, 0 where there are none; .valid is the
        weighted share of valid particles around the probe.  Two calls, one per row."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n = pts.shape[0]
        rows = [np.zeros((n, 4), np.float32) for _ in range(2)]
        rho = np.zeros(n, np.float32)
        cnt = np.zeros(n, np.int32)
        for group in range(2):
            self.call("sph_hip_sample_velocity_gradients_points", n, _ptr(pts), group, _ptr(rows[group]), _ptr(rho),
                      _ptr(cnt))
        return _V.VelocityGradients(rows[0], rows[1], rho, cnt)

    def sampleVelocityGradientLattice(self, origin, spacing, shape):
        """The same on sampleLattice's lattice, shape = (nx, ny, nz): every field with the leading shape
        [nz, ny, nx]."""
        o, s, d, dims = _lattice(origin, spacing, shape)
        grid = (max(dims[2], 0), max(dims[1], 0), max(dims[0], 0))
        if grid[0] * grid[1] * grid[2] >= 2 ** 31:
            raise ValueError("a lattice of more than 2^31 - 1 points")
        rows = [np.zeros(grid + (4,), np.float32) for _ in range(2)]
        rho = np.zeros(grid, np.float32)
        cnt = np.zeros(grid, np.int32)
        for group in range(2):
            self.call("sph_hip_sample_velocity_gradients_lattice", C.byref(o), C.byref(s), C.byref(d), group,
                      _ptr(rows[group]), _ptr(rho), _ptr(cnt))
        return _V.VelocityGradients(rows[0], rows[1], rho, cnt)

    def renderVelocityGradients(self, camera, width, height, iso, quantity, value_range, colormap=None, mode="surface",
                                flat=False, solids=False, step=None, refine=8, grad_step=None, box=None,
                                light=(0.4, 0.8, 0.45), albedo=(0.25, 0.55, 0.9), ambient=0.2, diffuse=0.8,
                                background=(0, 0, 0, 255), velocity=False, max_samples=1 << 16,
                                solid_albedo=(0.72, 0.72, 0.72), solid_colors=None, solid_ambient=None,
                                solid_diffuse=None):
        """renderScalars' frame coloured by a velocity-gradient quantity in the place of a carried channel:
        `quantity` is a name of velgrad.QUANTITIES ("vorticity_z", "divergence", "q", ...) or its number 0 .. 7.
        The context needs no carried scalars.  Every other argument is renderScalars'."""
        return self._render_tinted("sph_hip_render_velocity_gradients", _V.quantity_index(quantity), camera, width,
                                   height, iso, value_range, colormap, mode, flat, solids, step, refine, grad_step,
                                   box, light, albedo, ambient, diffuse, background, velocity, max_samples,
                                   solid_albedo, solid_colors, solid_ambient, solid_diffuse)

    # ---- diagnostics -----------------------------------------------------------------------------
    def elapsed(self):
        """The six numbers of SPH::updateElapsed (reference src/sph.cpp:292-299), in ms."""
        ms = (C.c_float * 6)()
        self.call("sph_hip_get_timings", C.byref(ms))
        return list(ms)

    # the reference-style names of what every context can do (lib.Context)
    resetTimings, setTiming = Context.reset_timings, Context.set_timing
    setTimingStride = Context.set_timing_stride
    tileStats, phaseTotals = Context.tile_stats, Context.phase_totals

    def neighborStats(self):
        """(avg, max, min) as written to out/neighbors.txt (reference src/sph.cpp:232)."""
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self.call("sph_hip_get_neighbor_stats", C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def voxels(self):
        """(mVoxelCoords as 3 ints per particle, mVoxelIds) — REF mode."""
        n = self.mParticleCount
        coords = np.zeros(3 * n, np.int32)
        ids = np.zeros(n, np.int32)
        self.call("sph_hip_download_voxels", _ptr(coords), _ptr(ids))
        return coords, ids

    def neighborLists(self):
        """(mNeighbors, mNeighborDistancesScaled), row stride mExamineCount — REF mode."""
        m = self.mParticleCount * self._params.examine_count
        nb = np.zeros(m, np.uint32)
        nd = np.zeros(m, np.float32)
        self.call("sph_hip_download_neighbor_lists", _ptr(nb), _ptr(nd))
        return nb, nd


def write_ply(path, mesh):
    """Write a SurfaceMesh (or any object with .vertices, .triangles and an optional .normals) as
    binary little-endian PLY: x y z [nx ny nz] float per vertex, a uchar-counted int list per face."""
    v = np.ascontiguousarray(mesh.vertices, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(mesh.triangles, np.int32).reshape(-1, 3)
    n = getattr(mesh, "normals", None)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if n is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    vert = np.empty(len(v), dtype=fields)
    vert["x"], vert["y"], vert["z"] = v[:, 0], v[:, 1], v[:, 2]
    if n is not None:
        n = np.asarray(n, np.float32).reshape(-1, 3)
        vert["nx"], vert["ny"], vert["nz"] = n[:, 0], n[:, 1], n[:, 2]
    face = np.empty(len(t), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    face["n"] = 3
    face["i"] = t
    head = ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(v)]
    head += ["property float %s" % name for name, _ in fields]
    head += ["element face %d" % len(t), "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        f.write(vert.tobytes())
        f.write(face.tobytes())


def write_png(path, rgba):
    """Write an (H, W, 4) uint8 RGBA image as an 8-bit RGBA PNG (zlib and struct only; every row
    with filter 0)."""
    img = np.ascontiguousarray(rgba, np.uint8)
    if img.ndim != 3 or img.shape[2] != 4:
        raise ValueError("rgba must be (H, W, 4) uint8")
    H, W = img.shape[0], img.shape[1]
    raw = np.concatenate([np.zeros((H, 1), np.uint8), img.reshape(H, W * 4)], 1).tobytes()

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 6, 0, 0, 0)))
        f.write(chunk(b"IDAT", zlib.compress(raw, 6)))
        f.write(chunk(b"IEND", b""))
