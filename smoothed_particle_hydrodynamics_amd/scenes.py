"""Synthetic initial conditions for the SPH step.

The reference ships one scene (a rotating sphere from glibc rand(), src/sph.cpp:361-425) and
a commented-out box/dam init (src/sph.cpp:324-358).  The generators here use a counter-based
PRNG (SplitMix64 finaliser on the particle/component counter) so that any host — numpy here,
C elsewhere — produces bit-identical fp32 positions from (seed, index) without libc state.
"""
import math

import numpy as np

from .lib import default_params

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def uniform01(seed, counters):
    """24-bit uniforms in [0,1) as float32: SplitMix64 finaliser of (counter+1)*golden + seed*c."""
    with np.errstate(over="ignore"):
        z = (np.asarray(counters, np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = z + np.uint64(seed) * np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def box_fill(n, lo, hi, seed=42):
    """n points uniform in the axis-aligned box [lo, hi) (fp32), interleaved xyz."""
    idx = np.arange(3 * n, dtype=np.uint64)
    u = uniform01(seed, idx).reshape(n, 3)
    lo = np.asarray(lo, np.float32)
    ext = np.asarray(hi, np.float32) - lo
    pos = (lo + u * ext).astype(np.float32)
    return np.ascontiguousarray(pos.reshape(-1))


def dam_break_h(n, box=(1.0, 1.0, 1.0), fill=(0.1, 0.75, 1.0), neighbors=32.0):
    """Smoothing length giving ~`neighbors` particles inside radius h in the filled column."""
    vol = box[0] * fill[0] * box[1] * fill[1] * box[2] * fill[2]
    number_density = n / vol
    return (3.0 * neighbors / (4.0 * math.pi * number_density)) ** (1.0 / 3.0)


def box_fill_axis(n, lo, hi, axis, seed=42):
    """Coordinate `axis` of box_fill(n, lo, hi, seed)'s points, without the other two."""
    idx = np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(axis)
    u = uniform01(seed, idx)
    lo = np.float32(lo[axis])
    return (lo + u * (np.float32(hi[axis]) - lo)).astype(np.float32)


def box_fill_subset(ids, lo, hi, seed=42):
    """Rows `ids` of box_fill(n, lo, hi, seed) (any n > max(ids)), interleaved xyz."""
    ids = np.asarray(ids, np.uint64)
    idx = (ids[:, None] * np.uint64(3) + np.arange(3, dtype=np.uint64)[None, :]).reshape(-1)
    u = uniform01(seed, idx).reshape(-1, 3)
    lo = np.asarray(lo, np.float32)
    ext = np.asarray(hi, np.float32) - lo
    return np.ascontiguousarray((lo + u * ext).astype(np.float32).reshape(-1))


def dam_break_params(n, box=(1.0, 1.0, 1.0), fill=(0.1, 0.75, 1.0), neighbors=32.0):
    """(params, column extent) of dam_break(n, box, fill, neighbors) without any particle."""
    h = np.float32(dam_break_h(n, box, fill, neighbors))
    cells = [max(1, int(math.ceil(b / (2.0 * float(h))))) for b in box]
    p = default_params(float(h), cells)
    p.central_mass = 0.0
    return p, [box[c] * fill[c] for c in range(3)]


def dam_break(n, box=(1.0, 1.0, 1.0), fill=(0.1, 0.75, 1.0), neighbors=32.0, seed=42, speed=0.0):
    """Dam-break column modelled on the reference's commented-out init (src/sph.cpp:328-345):
    uniform random points in x<0.1*Lx, y<0.75*Ly, z<Lz, at rest, unit masses.  speed > 0: a seeded
    uniform random velocity in [-speed, speed)^3 per particle instead of rest (parity tests: with
    every particle at rest the viscous sum of src/sph.cpp:875-882 is identically zero).

    Returns (params, pos[3n], vel[3n], mass[n]).  The voxel grid (edge 2h) covers the box; the
    central point mass is switched off (it is the astrophysical part of the reference's
    default scene, not of a dam-break); everything else keeps the reference's defaults.
    """
    p, hi = dam_break_params(n, box, fill, neighbors)
    pos = box_fill(n, (0.0, 0.0, 0.0), hi, seed)
    vel = np.zeros(3 * n, np.float32)
    if speed > 0.0:
        vel = box_fill(n, (-speed,) * 3, (speed,) * 3, seed + 1)
    mass = np.ones(n, np.float32)
    return p, pos, vel, mass


def dense_block(n, lo=(1.0, 1.0, 1.0), hi=(2.2, 2.2, 2.2), seed=7, speed=0.5):
    """Reference default constants (h=0.1, 32^3 voxels) with n particles packed into a small
    block, so that the shipped sampled search actually finds neighbours (its stock sphere
    scene finds almost none).  Velocities: small uniform random."""
    p = default_params()
    pos = box_fill(n, lo, hi, seed)
    vel = (box_fill(n, (-speed,) * 3, (speed,) * 3, seed + 1)).astype(np.float32)
    mass = np.ones(n, np.float32)
    return p, pos, vel, mass


def reference_sphere(n, params=None):
    """The reference's default scene (src/sph.cpp:361-425): srand(42), rejection-sampled points
    within radius 2 of the box centre, tangential velocity 20*(dist + h/2)^-0.5 in the x-z plane,
    small random v_y.  Uses the C library's own rand()/atan2f/sinf/cosf/pow through ctypes, so on
    a glibc system the arrays are bit-identical to what `SPH::SPH()` builds with -DM=n/1024.

    Returns (params, pos[3n], vel[3n], mass[n]).  Not thread-safe (libc rand() state)."""
    import ctypes as C
    import ctypes.util
    libc = C.CDLL(ctypes.util.find_library("c") or "libc.so.6")
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libc.rand.restype = C.c_int
    for name in ("atan2f",):
        getattr(libm, name).restype = C.c_float
        getattr(libm, name).argtypes = [C.c_float, C.c_float]
    for name in ("sinf", "cosf", "sqrtf"):
        getattr(libm, name).restype = C.c_float
        getattr(libm, name).argtypes = [C.c_float]
    libm.pow.restype = C.c_double
    libm.pow.argtypes = [C.c_double, C.c_double]
    p = params.copy() if params is not None else default_params()
    f32 = np.float32
    rand_max = f32(2147483647.0)           # (float)RAND_MAX
    ext = [f32(p.cells_x) * f32(p.htimes2), f32(p.cells_y) * f32(p.htimes2),
           f32(p.cells_z) * f32(p.htimes2)]
    cells = [f32(p.cells_x), f32(p.cells_y), f32(p.cells_z)]
    centre = [f32(p.max_x) * f32(0.5), f32(p.max_y) * f32(0.5), f32(p.max_z) * f32(0.5)]
    half_h = float(f32(p.hscaled)) * 0.5   # double, as in `mHScaled*0.5`
    pos = np.zeros(3 * n, f32)
    vel = np.zeros(3 * n, f32)
    libc.srand(42)
    for i in range(n):
        while True:
            c = []
            for a in range(3):
                v = f32(libc.rand()) / rand_max
                v = v * ext[a]
                if v == cells[a]:
                    v = v - f32(0.00001)
                c.append(f32(v))
            d = [f32(c[a] - centre[a]) for a in range(3)]
            dist = f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2]))
            dist = f32(libm.sqrtf(dist))
            if not dist > f32(2.0):
                break
        pos[3 * i:3 * i + 3] = c
        phi = f32(libm.atan2f(f32(c[2] - centre[2]), f32(c[0] - centre[0])))
        amp = 20.0 * libm.pow(float(dist) + half_h, -0.5)          # double
        vel[3 * i] = f32(amp * float(f32(-libm.sinf(phi))))
        vel[3 * i + 2] = f32(amp * float(f32(libm.cosf(phi))))
        vel[3 * i + 1] = f32(f32(f32(libc.rand()) / rand_max) * f32(0.5)) - f32(0.25)
    return p, pos, vel, np.ones(n, f32)


def carve(pos, vel, mass, obstacles, rotations=None):
    """The scene without the particles that start strictly inside an obstacle (obstacles.Sphere /
    Box / Cylinder, each as its obstacles.Rotation of `rotations` poses it at the motion clock's start):
    (pos[3m], vel[3m], mass[m]), the kept rows in their order."""
    from .obstacles import inside_any
    keep = ~inside_any(np.asarray(pos, np.float32).reshape(-1, 3), obstacles, rotations)
    pos = np.ascontiguousarray(np.asarray(pos, np.float32).reshape(-1, 3)[keep].reshape(-1))
    vel = np.ascontiguousarray(np.asarray(vel, np.float32).reshape(-1, 3)[keep].reshape(-1))
    return pos, vel, np.ascontiguousarray(np.asarray(mass, np.float32)[keep])


def dam_break_pillar(n, pillar=(0.35, 0.5), radius=0.08, surge=0.7, box=(1.0, 1.0, 1.0),
                     fill=(0.1, 0.75, 1.0), neighbors=32.0, seed=42, gravity=-9.81):
    """The dam column (dam_break) with uniform gravity along -y and the walls on, released with a
    uniform velocity `surge` along +x, and a cylinder pillar along y standing downstream of it: axis
    through (x, z) = `pillar`, `radius`, from below the floor to above the box.  (With the reference's
    constants the column at rest collapses downward and does not spread along x for the first thousand
    steps and more; the surge carries it into the pillar.)  Particles that would start inside the pillar
    are dropped (carve).  Returns (params, pos, vel, mass, [Cylinder])."""
    from .obstacles import Cylinder
    p, pos, vel, mass = dam_break(n, box, fill, neighbors, seed)
    p.apply_gravity = 1
    p.apply_walls = 1
    p.gravity[0], p.gravity[1], p.gravity[2] = 0.0, gravity, 0.0
    vel.reshape(-1, 3)[:, 0] = np.float32(surge)
    obstacles = [Cylinder(1, (pillar[0], 0.0, pillar[1]), radius, -1.0, 2.0 * float(p.max_y) + 1.0)]
    pos, vel, mass = carve(pos, vel, mass, obstacles)
    return p, pos, vel, mass, obstacles


def dam_break_gate(n, lift_speed, thickness=2.0, surge=0.7, box=(1.0, 1.0, 1.0), fill=(0.1, 0.75, 1.0),
                   neighbors=32.0, seed=42, gravity=-9.81):
    """The dam column of dam_break_pillar (gravity along -y, the walls on, the surge along +x) held behind
    a gate: a Box `thickness` kernel radii thick whose upstream face stands one kernel radius from the
    column's face, from below the floor to above the column and across the whole box along z.  Its
    Motion lifts it along +y at `lift_speed` (position units per unit of time_step) until its lower edge
    is one kernel radius above the column, and stops.  Particles that would start inside the gate are
    dropped (carve).  Returns (params, pos, vel, mass, [Box], [Motion]): setObstacles, then
    setObstacleMotion."""
    from .obstacles import Box, Motion
    p, pos, vel, mass = dam_break(n, box, fill, neighbors, seed)
    p.apply_gravity = 1
    p.apply_walls = 1
    p.gravity[0], p.gravity[1], p.gravity[2] = 0.0, gravity, 0.0
    vel.reshape(-1, 3)[:, 0] = np.float32(surge)
    h = float(p.h)
    x0, top = box[0] * fill[0] + h, box[1] * fill[1]
    gate = Box((x0, -h, -h), (x0 + thickness * h, top + h, float(p.max_z) + h))
    pos, vel, mass = carve(pos, vel, mass, [gate])
    travel = top + 2.0 * h
    return p, pos, vel, mass, [gate], [Motion((0.0, lift_speed, 0.0), 0.0, travel / lift_speed)]


def dam_break_ramp(n, slope_deg=20.0, length=0.6, thickness=0.1, gap=0.25, surge=0.7, box=(1.0, 1.0, 1.0),
                   fill=(0.1, 0.75, 1.0), neighbors=32.0, seed=42, gravity=-9.81):
    """The surging dam column of dam_break_pillar (gravity along -y, the walls on, the surge along +x) running
    up a ramp: a Box `length` long and `thickness` thick across the whole box along z, whose upper upstream
    edge lies on the floor `gap` kernel radii from the column's face, tilted about z through that edge by
    `slope_deg` degrees, so that its upper face rises downstream.  Particles that would start inside it are
    dropped (carve).  Returns (params, pos, vel, mass, [Box], [Rotation]); the rotation is the contract's
    (csrc/obstacle_policy.h, third part), which no context takes yet."""
    from .obstacles import Box, Rotation
    p, pos, vel, mass = dam_break(n, box, fill, neighbors, seed)
    p.apply_gravity = 1
    p.apply_walls = 1
    p.gravity[0], p.gravity[1], p.gravity[2] = 0.0, gravity, 0.0
    vel.reshape(-1, 3)[:, 0] = np.float32(surge)
    h = float(p.h)
    x0 = box[0] * fill[0] + gap * h
    ramp = Box((x0, -thickness, -h), (x0 + length, 0.0, float(p.max_z) + h))
    tilt = Rotation(2, (x0, 0.0, 0.0), math.radians(slope_deg))
    pos, vel, mass = carve(pos, vel, mass, [ramp], [tilt])
    return p, pos, vel, mass, [ramp], [tilt]


def dam_break_beach(n, slope_deg=20.0, length=0.6, gap=0.25, surge=0.7, box=(1.0, 1.0, 1.0), fill=(0.1, 0.75, 1.0),
                    neighbors=32.0, seed=42, gravity=-9.81):
    """dam_break_ramp's set-up - the surging dam column of dam_break_pillar, gravity along -y, the walls on, the
    surge along +x - running up a beach that a context takes: a Wedge standing on the floor across the whole
    box along z, whose foot lies `gap` kernel radii from the column's face and whose face rises downstream at
    `slope_deg` degrees over `length`.  Particles that would start inside it are dropped (carve).  Returns
    (params, pos, vel, mass, [Wedge]): setObstacles."""
    from .obstacles import Wedge
    p, pos, vel, mass = dam_break(n, box, fill, neighbors, seed)
    p.apply_gravity = 1
    p.apply_walls = 1
    p.gravity[0], p.gravity[1], p.gravity[2] = 0.0, gravity, 0.0
    vel.reshape(-1, 3)[:, 0] = np.float32(surge)
    h = float(p.h)
    x0 = box[0] * fill[0] + gap * h
    rise = length * math.tan(math.radians(slope_deg))
    beach = Wedge.ramp((x0, 0.0, -h), (x0 + length, rise, float(p.max_z) + h), 0, 1)
    pos, vel, mass = carve(pos, vel, mass, [beach])
    return p, pos, vel, mass, [beach]


def wave_flume(n, stroke=0.06, period=0.4, slope_deg=15.0, box=(2.0, 0.5, 0.25), depth=0.5, gauges=4, keys=64,
               neighbors=32.0, seed=42, gravity=-9.81):
    """Still water in a long tank (gravity along -y, the walls on) filled to `depth` of its height, with a
    piston wavemaker at the upstream end and a beach at the far one.  The piston is a Box two kernel radii
    thick across the whole tank along z, from below the floor to above the tank, on a MotionPath.sine along x:
    amplitude stroke / 2, `period` on the motion clock, `keys` segments per period; its back face stays half a
    stroke inside the upstream wall at its rearmost.  The water starts at the piston's front face.  The beach is
    a Wedge.ramp standing on the floor whose face rises downstream at `slope_deg` degrees to 1.25 times the
    still water level and ends at the downstream wall (the walls are the voxel grid's: at least `box`).  `gauges` ColumnGauges stand evenly along the mid-line
    between the piston's foremost position and the beach's foot.  Particles that would start inside a solid are
    dropped (carve).  Returns (params, pos, vel, mass, [Box, Wedge], [MotionPath, None], [ColumnGauge, ...]):
    setObstacles, then setObstaclePaths, then setGauges."""
    from .gauges import ColumnGauge
    from .obstacles import Box, MotionPath, Wedge
    p, _ = dam_break_params(n, box, (1.0, depth, 1.0), neighbors)
    p.apply_gravity = 1
    p.apply_walls = 1
    p.gravity[0], p.gravity[1], p.gravity[2] = 0.0, gravity, 0.0
    h = float(p.h)
    length_x, width_z = float(p.max_x), float(p.max_z)   # the walls: the voxel grid's extent, at least `box`
    level = box[1] * depth
    back = stroke                                   # rearmost: back - stroke / 2 > 0
    piston = Box((back, -h, -h), (back + 2.0 * h, float(p.max_y) + h, width_z + h))
    rise = 1.25 * level
    length = rise / math.tan(math.radians(slope_deg))
    foot = length_x - length
    if not foot > back + 2.0 * h + stroke:
        raise ValueError("the tank is too short for this beach and stroke")
    beach = Wedge.ramp((foot, 0.0, -h), (length_x, rise, width_z + h), 0, 1)
    pos = box_fill(n, (back + 2.0 * h, 0.0, 0.0), (length_x, level, width_z), seed)
    vel = np.zeros(3 * n, np.float32)
    mass = np.ones(n, np.float32)
    pos, vel, mass = carve(pos, vel, mass, [piston, beach])
    path = MotionPath.sine((0.5 * stroke, 0.0, 0.0), period, keys)
    x0, x1 = back + 2.0 * h + 0.5 * stroke, foot
    samples = max(2, int(math.ceil(float(p.max_y) / (0.5 * h))))
    # half the sampler's density deep inside the fill (as dam_break_gauged's columns)
    number_density = n / ((length_x - back - 2.0 * h) * level * width_z)
    iso = 0.5 * number_density * float(p.kernel1) * float(p.sim_scale) ** 6 * h ** 9 * 64.0 * math.pi / 315.0
    cols = [ColumnGauge((x0 + (x1 - x0) * (g + 1) / (gauges + 1), 0.0, 0.5 * width_z), 1, 0.5 * h, samples, iso)
            for g in range(gauges)]
    return p, pos, vel, mass, [piston, beach], [path, None], cols


def stirred_tank(n, rate, depth=0.5, blade=(0.6, 0.08), start=0.0, stop=math.inf, box=(1.0, 1.0, 1.0),
                 neighbors=32.0, seed=42, gravity=-9.81):
    """A block of fluid at rest filling the tank to `depth` of its height (gravity along -y, the walls on),
    stirred by a paddle: a Box blade[0] of the tank's width long and blade[1] thick, from below the floor to
    above the fluid, centred on the vertical axis through the tank's middle and turning about it at `rate`
    radians per unit of time_step while the motion clock is in [start, stop].  Particles that would start
    inside the paddle are dropped (carve).  Returns (params, pos, vel, mass, [Box], [Rotation]); the rotation
    is the contract's (csrc/obstacle_policy.h, third part), which no context takes yet."""
    from .obstacles import Box, Rotation
    p, pos, vel, mass = dam_break(n, box, (1.0, depth, 1.0), neighbors, seed)
    p.apply_gravity = 1
    p.apply_walls = 1
    p.gravity[0], p.gravity[1], p.gravity[2] = 0.0, gravity, 0.0
    h = float(p.h)
    cx, cz = 0.5 * float(p.max_x), 0.5 * float(p.max_z)
    half, thick = 0.5 * blade[0] * float(p.max_x), 0.5 * blade[1] * float(p.max_z)
    paddle = Box((cx - half, -h, cz - thick), (cx + half, box[1] * depth + 2.0 * h, cz + thick))
    turn = Rotation(1, (cx, 0.0, cz), 0.0, rate, start, stop)
    pos, vel, mass = carve(pos, vel, mass, [paddle])
    return p, pos, vel, mass, [paddle], [turn]


def dam_break_debris(n, size=(0.12, 0.12, 0.3), gap=3.0, density_ratio=6.0, surge=0.7, box=(1.0, 1.0, 1.0),
                     fill=(0.1, 0.75, 1.0), neighbors=32.0, seed=42, gravity=-9.81):
    """The surging dam column of dam_break_pillar (gravity along -y, the walls on, the surge along +x) with a
    piece of debris downstream of it: a Box of `size` standing on the floor, centred along z, its upstream
    face `gap` kernel radii from the column's face.  It is a free body (obstacles.Body) along the surge axis
    only - the floor carries it - whose mass is `density_ratio` (at least 4: the coupling treats the solid as
    infinitely heavy within a step) times the mass of the fluid it displaces at the column's density, and
    whose travel ends one kernel radius before the downstream wall, so that it stays inside the domain.
    Returns (params, pos, vel, mass, [Box], [Body]): setObstacles, then setBodies."""
    from .obstacles import Body, Box
    if density_ratio < 4.0:
        raise ValueError("density_ratio must be at least 4")
    p, pos, vel, mass = dam_break(n, box, fill, neighbors, seed)
    p.apply_gravity = 1
    p.apply_walls = 1
    p.gravity[0], p.gravity[1], p.gravity[2] = 0.0, gravity, 0.0
    vel.reshape(-1, 3)[:, 0] = np.float32(surge)
    h = float(p.h)
    x0 = box[0] * fill[0] + gap * h
    z0 = 0.5 * (float(p.max_z) - size[2])
    debris = Box((x0, 0.0, z0), (x0 + size[0], size[1], z0 + size[2]))
    column = box[0] * fill[0] * box[1] * fill[1] * box[2] * fill[2]
    displaced = float(mass.sum()) / column * size[0] * size[1] * size[2]
    travel = float(p.max_x) - h - float(debris.hi[0])
    body = Body(density_ratio * displaced, free=(True, False, False), travel_lo=(0.0, 0.0, 0.0),
                travel_hi=(travel, 0.0, 0.0))
    pos, vel, mass = carve(pos, vel, mass, [debris])
    return p, pos, vel, mass, [debris], [body]


def tracer_lattice(lo, hi, spacing):
    """Tracer start points on the lattice lo + i * spacing per axis (fp32, unfused, x fastest), every i with
    lo + i * spacing <= hi: (n, 3) float32.  `spacing` is one value or one per axis."""
    f = np.float32
    lo = np.asarray(lo, f).reshape(3)
    hi = np.asarray(hi, f).reshape(3)
    sp = np.broadcast_to(np.asarray(spacing, f), (3,))
    if not (sp > 0).all():
        raise ValueError("spacing must be positive")
    ax = []
    for a in range(3):
        m = max(0, int(math.floor((float(hi[a]) - float(lo[a])) / float(sp[a]))) + 2)
        x = lo[a] + np.arange(m, dtype=np.int64).astype(f) * sp[a]
        ax.append(x[x <= hi[a]])
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.ascontiguousarray(np.stack([x, y, z], -1).astype(f).reshape(-1, 3))


def dam_break_dye(n, spacing=1.0, surge=0.7, box=(1.0, 1.0, 1.0), fill=(0.1, 0.75, 1.0), neighbors=32.0, seed=42,
                  gravity=-9.81):
    """The breaking dam of dam_break_pillar without the pillar - gravity along -y, the walls on, the surge
    along +x - with dye through the column: a lattice of tracers `spacing` kernel radii apart, half a spacing
    inside the column's faces.  Returns (params, pos, vel, mass, tracers[m, 3]): setParticles, then
    setTracers."""
    p, pos, vel, mass = dam_break(n, box, fill, neighbors, seed)
    p.apply_gravity = 1
    p.apply_walls = 1
    p.gravity[0], p.gravity[1], p.gravity[2] = 0.0, gravity, 0.0
    vel.reshape(-1, 3)[:, 0] = np.float32(surge)
    s = float(spacing) * float(p.h)
    top = [box[c] * fill[c] for c in range(3)]
    tracers = tracer_lattice([0.5 * s] * 3, [t - 0.5 * s for t in top], s)
    return p, pos, vel, mass, tracers


def dam_break_gauged(n, surge=0.7, box=(1.0, 1.0, 1.0), fill=(0.1, 0.75, 1.0), neighbors=32.0, seed=42, gravity=-9.81):
    """The surging dam of dam_break_dye without the dye, with the instruments of a dam-break experiment: four
    column gauges up y at x = 0.05, 0.3, 0.6 and 0.9 of the box on the mid-plane in z, h/2 between probes from
    the floor to the lid; one section across the box at x = 0.2 (normal x, h/2 between probes); one point probe
    at mid-height of the column, at its centre.  iso is half the sampler's density deep inside the column - the
    number density times the integral of the kernel over its support, kernel1 * sim_scale^6 * h^9 * 64 pi / 315 -
    and does not involve rho0.  Returns (params, pos, vel, mass, gauges): setParticles, then setGauges."""
    from .gauges import ColumnGauge, PointGauge, SectionGauge
    p, pos, vel, mass = dam_break(n, box, fill, neighbors, seed)
    p.apply_gravity = 1
    p.apply_walls = 1
    p.gravity[0], p.gravity[1], p.gravity[2] = 0.0, gravity, 0.0
    vel.reshape(-1, 3)[:, 0] = np.float32(surge)
    h = float(p.h)
    column = [box[c] * fill[c] for c in range(3)]
    bulk = n / (column[0] * column[1] * column[2]) * float(p.kernel1) * float(p.sim_scale) ** 6 * h ** 9 * 64.0 * math.pi / 315.0
    iso = 0.5 * bulk
    s = 0.5 * h
    up = min(int(math.floor(box[1] / s)) + 1, 4096)
    gauges = [ColumnGauge((f * box[0], 0.0, 0.5 * box[2]), 1, s, up, iso) for f in (0.05, 0.3, 0.6, 0.9)]
    nu = int(math.floor(box[1] / s)) + 1
    nv = int(math.floor(box[2] / s)) + 1
    while nu * nv > 4096:   # (a finer h than a section's probe limit allows: a coarser lattice over the same rectangle)
        s *= 2.0
        nu = int(math.floor(box[1] / s)) + 1
        nv = int(math.floor(box[2] / s)) + 1
    gauges.append(SectionGauge((0.2 * box[0], 0.0, 0.0), 0, (s, s), (nu, nv), iso))
    gauges.append(PointGauge((0.5 * column[0], 0.5 * column[1], 0.5 * column[2])))
    return p, pos, vel, mass, gauges


def dam_break_sensors(n, surge=0.7, box=(1.0, 1.0, 1.0), fill=(0.1, 0.75, 1.0), neighbors=32.0, seed=42, gravity=-9.81,
                      points=16):
    """The surging dam of dam_break_gauged with the pressure sensors of a dam-break experiment: `points`
    PressureGauges up the downstream wall - the wall the simulation keeps, x = params.max_x, the voxel grid's
    edge at or beyond box[0] - on the column's mid-plane in z, one kernel radius apart from half a radius above
    the floor; one PressurePatch over the lower quarter of that wall (normal x) and one on the floor under the
    column (normal y), h/2 between probes (coarser where a patch would exceed its probe limit).  iso is
    dam_break_gauged's: half the sampler's density deep inside the column.  Returns (params, pos, vel, mass,
    gauges): setParticles, then setGauges."""
    from .gauges import MAX_GAUGE_PROBES, PressureGauge, PressurePatch
    p, pos, vel, mass, gauged = dam_break_gauged(n, surge, box, fill, neighbors, seed, gravity)
    iso = gauged[0].iso
    h = float(p.h)
    column = [box[c] * fill[c] for c in range(3)]
    wall = (float(p.max_x), float(p.max_y), float(p.max_z))
    gauges = [PressureGauge((wall[0], (0.5 + i) * h, 0.5 * box[2])) for i in range(int(points))
              if (0.5 + i) * h <= wall[1]]

    def patch(corner, axis, extent):
        s = 0.5 * h
        shape = [int(math.floor(e / s)) + 1 for e in extent]
        while shape[0] * shape[1] > MAX_GAUGE_PROBES:
            s *= 2.0
            shape = [int(math.floor(e / s)) + 1 for e in extent]
        return PressurePatch(corner, axis, (s, s), tuple(shape), iso)

    gauges.append(patch((wall[0], 0.0, 0.0), 0, (0.25 * wall[1], wall[2])))     # u = y, v = z
    gauges.append(patch((0.0, 0.0, 0.0), 1, (column[0], column[2])))            # u = x, v = z
    return p, pos, vel, mass, gauges


def filling_tank(capacity, box=(1.0, 1.0, 1.0), inlet=1.0 / 3.0, speed=2.0, neighbors=32.0, gravity=-9.81):
    """An empty tank (gravity along -y, the walls on) that fills through an inlet under its lid: one Emitter with
    normal y, a square lattice `inlet` of the tank's width across, centred, one kernel radius below the lid,
    blowing downward at `speed`.  The smoothing length is the one at which `capacity` particles filling the
    whole tank would have ~`neighbors` neighbours, the lattice spacing that fluid's own; a layer enters every
    round(spacing / (speed * time_step)) steps, so that successive layers are one spacing apart.  Create the
    context with this capacity and upload the empty arrays.  Returns (params, pos, vel, mass, [Emitter], []):
    setParticles, then setPorts."""
    from .ports import Emitter
    p, _ = dam_break_params(capacity, box, (1.0, 1.0, 1.0), neighbors)
    p.apply_gravity = 1
    p.apply_walls = 1
    p.gravity[0], p.gravity[1], p.gravity[2] = 0.0, gravity, 0.0
    s = (box[0] * box[1] * box[2] / float(capacity)) ** (1.0 / 3.0)
    nu = max(1, int(math.floor(inlet * box[2] / s)))
    nw = max(1, int(math.floor(inlet * box[0] / s)))
    every = max(1, int(round(s / (speed * float(p.time_step)))))
    origin = (0.5 * (box[0] - (nw - 1) * s), box[1] - float(p.h), 0.5 * (box[2] - (nu - 1) * s))
    emitter = Emitter(1, origin, (nu, nw), s, (0.0, -speed, 0.0), 1.0, 0, every, -1)
    empty = np.zeros(0, np.float32)
    return p, empty, empty.copy(), empty.copy(), [emitter], []


def channel_flow(n, box=(2.0, 0.5, 0.5), depth=0.5, speed=1.0, neighbors=32.0, gravity=-9.81):
    """An open channel (gravity along -y, the walls on): a block of n particles at rest filling the channel's
    whole length to `depth` of its height, an inlet face upstream - one Emitter with normal x half a spacing
    from the upstream wall, a lattice over the wet cross-section, blowing along +x at `speed` - and a sink slab
    downstream: the last two kernel radii of the channel over its whole cross-section.  The lattice spacing is
    the block's own; a layer enters every round(spacing / (speed * time_step)) steps.  Returns (params, pos,
    vel, mass, [Emitter], [Sink]): setParticles, then setPorts."""
    from .ports import Emitter, Sink
    fill = (1.0, depth, 1.0)
    p, pos, vel, mass = dam_break(n, box, fill, neighbors)
    p.apply_gravity = 1
    p.apply_walls = 1
    p.gravity[0], p.gravity[1], p.gravity[2] = 0.0, gravity, 0.0
    h = float(p.h)
    s = (box[0] * box[1] * depth * box[2] / float(n)) ** (1.0 / 3.0)
    nu = max(1, int(math.floor(depth * box[1] / s)))
    nw = max(1, int(math.floor(box[2] / s)))
    every = max(1, int(round(s / (speed * float(p.time_step)))))
    emitter = Emitter(0, (0.5 * s, 0.5 * s, 0.5 * s), (nu, nw), s, (speed, 0.0, 0.0), 1.0, 0, every, -1)
    top = (float(p.max_x), float(p.max_y), float(p.max_z))
    sink = Sink((box[0] - 2.0 * h, -h, -h), (top[0] + h, top[1] + h, top[2] + h))
    return p, pos, vel, mass, [emitter], [sink]


def channel_weir(n, crest=0.6, at=0.45, ramps=(0.3, 0.2), top=0.1, box=(2.0, 0.5, 0.5), depth=0.5, speed=1.0,
                 neighbors=32.0, gravity=-9.81):
    """channel_flow's open channel with a trapezoidal weir across it, built from three solids in a row along x:
    a Wedge rising downstream over ramps[0], a Box `top` long, a Wedge falling over ramps[1]; the crest stands
    `crest` of the water's depth above the floor and the upstream foot `at` of the channel's length from the
    upstream wall; every solid reaches one kernel radius beyond the side walls.  Particles that would start
    inside the weir are dropped (carve).  Returns (params, pos, vel, mass, [Wedge, Box, Wedge], [Emitter],
    [Sink]): setParticles, setObstacles, then setPorts."""
    from .obstacles import Box, Wedge
    p, pos, vel, mass, emitters, sinks = channel_flow(n, box, depth, speed, neighbors, gravity)
    h = float(p.h)
    height = crest * depth * box[1]
    x0 = at * box[0]
    x1, x2, x3 = x0 + ramps[0], x0 + ramps[0] + top, x0 + ramps[0] + top + ramps[1]
    z0, z1 = -h, float(p.max_z) + h
    weir = [Wedge.ramp((x0, 0.0, z0), (x1, height, z1), 0, 1, rising=True), Box((x1, 0.0, z0), (x2, height, z1)),
            Wedge.ramp((x2, 0.0, z0), (x3, height, z1), 0, 1, rising=False)]
    pos, vel, mass = carve(pos, vel, mass, weir)
    return p, pos, vel, mass, weir, emitters, sinks


def scalar_stable_kappa(p, fraction=0.25):
    """A diffusivity for carried scalars that keeps a step convex deep inside a fluid at its rest spacing.  The
    explicit update is a convex combination while dt * kappa * sum_j V_j * kernel3 * (h - d_ij) <= 1
    (include/sph_hip.h: carried scalars); with volumes that tile the fluid the sum is the integral of
    kernel3 * (h - r) over the kernel's support, kernel3 * pi * h^4 / 3 in scaled lengths.  Returns the kappa for
    which the product is `fraction`.  Near a free surface volumes are larger than the bulk's: keep a margin."""
    hs = float(p.hscaled)
    total = float(p.kernel3) * math.pi * hs ** 4 / 3.0   # (densities, and so volumes, are per scaled length cubed)
    return fraction / (float(p.time_step) * total)


def heated_floor(n, depth=0.3, hot=1.0, box=(1.0, 1.0, 1.0), neighbors=32.0, seed=42, gravity=-9.81):
    """Still water `depth` of the box deep, gravity along -y and the walls on, over a heated floor: channel 0 is
    a temperature that starts at 0 and diffuses (scalar_stable_kappa), and one HOLD source - a slab one kernel
    radius thick along the whole floor, reaching a radius beyond the walls - keeps it at `hot`.  Returns (params,
    pos, vel, mass, values[n, 4], kappa[4], [ScalarSource]): setParticles, setScalars, then setScalarSources."""
    from .scalars import ScalarSource
    p, pos, vel, mass = dam_break(n, box, (1.0, depth, 1.0), neighbors, seed)
    p.apply_gravity = 1
    p.apply_walls = 1
    p.gravity[0], p.gravity[1], p.gravity[2] = 0.0, gravity, 0.0
    h = float(p.h)
    values = np.zeros((n, 4), np.float32)
    kappa = np.zeros(4, np.float32)
    kappa[0] = scalar_stable_kappa(p)
    slab = ScalarSource.hold((-h, -h, -h), (float(p.max_x) + h, h, float(p.max_z) + h), 0, hot)
    return p, pos, vel, mass, values, kappa, [slab]


def dam_break_dyed(n, surge=0.7, box=(1.0, 1.0, 1.0), fill=(0.1, 0.75, 1.0), neighbors=32.0, seed=42, gravity=-9.81):
    """The surging column of dam_break_dye with a dye concentration in place of the tracers: channel 0 is 1 in
    the column's upstream half (x below half its width) and 0 in the other, with diffusivity 0 - every particle
    carries its value unchanged, so the channel shows where the upstream water goes.  Returns (params, pos, vel,
    mass, values[n, 4], kappa[4]): setParticles, then setScalars."""
    p, pos, vel, mass, _ = dam_break_dye(n, 1.0, surge, box, fill, neighbors, seed, gravity)
    values = np.zeros((n, 4), np.float32)
    values[:, 0] = (pos.reshape(-1, 3)[:, 0] < np.float32(0.5 * box[0] * fill[0])).astype(np.float32)
    return p, pos, vel, mass, values, np.zeros(4, np.float32)


def thermal_plume(n, patch=0.3, beta=0.2, depth=0.3, hot=1.0, box=(1.0, 1.0, 1.0), neighbors=32.0, seed=42,
                  gravity=-9.81):
    """heated_floor's still tank with the HOLD slab shrunk to a square patch in the middle of the floor, `patch` of
    the tank's width and length on a side, and a Buoyancy on channel 0: water at `hot` is lighter by the fraction
    beta * hot and rises over the patch.  Returns heated_floor's tuple with the Buoyancy appended: setParticles,
    setScalars, setScalarSources, then setBuoyancy."""
    from .scalars import Buoyancy, ScalarSource
    p, pos, vel, mass, values, kappa, _ = heated_floor(n, depth, hot, box, neighbors, seed, gravity)
    h = float(p.h)
    mx, mz = 0.5 * float(p.max_x), 0.5 * float(p.max_z)
    rx, rz = 0.5 * patch * float(p.max_x), 0.5 * patch * float(p.max_z)
    plate = ScalarSource.hold((mx - rx, -h, mz - rz), (mx + rx, h, mz + rz), 0, hot)
    return p, pos, vel, mass, values, kappa, [plate], Buoyancy(beta, 0.0, tuple(p.gravity))


def lock_exchange(n, beta=-0.2, depth=0.3, box=(1.0, 1.0, 1.0), neighbors=32.0, seed=42, gravity=-9.81):
    """Still water `depth` of the box deep, gravity along -y and the walls on, with the lock just opened: channel 0
    is a salinity of 1 in the half with x below the tank's middle and 0 in the other, carried without diffusion
    (kappa = 0), and a Buoyancy with a negative beta - salt water is heavier by the fraction -beta and slumps under
    the fresh.  Returns heated_floor's tuple (no sources) with the Buoyancy appended: setParticles, setScalars,
    then setBuoyancy."""
    from .scalars import Buoyancy
    p, pos, vel, mass, values, kappa, _ = heated_floor(n, depth, 1.0, box, neighbors, seed, gravity)
    kappa[:] = 0.0
    values[:, 0] = (pos.reshape(-1, 3)[:, 0] < np.float32(0.5) * np.float32(p.max_x)).astype(np.float32)
    return p, pos, vel, mass, values, kappa, [], Buoyancy(beta, 0.0, tuple(p.gravity))


# the gamma at which the median cohesive acceleration of droplet(3000)'s shell particles is about the median
# acceleration the pressure gives them (cohesion, "The droplet")
DROPLET_GAMMA = 3.0e-6


def droplet(n, gamma=DROPLET_GAMMA, neighbors=32.0, cells=None, seed=42):
    """A blob of fluid held together by cohesion alone: n particles at rest, a cubic random fill in the middle of
    the box at the density that gives ~`neighbors` particles inside radius h, gravity and the central mass off,
    the walls on.  The box is `cells` voxels of edge 2h on a side; the smoothing length is the dam column's at
    this n (dam_break_h), the cube's edge what the density asks for.  Without cohesion the pressure - repulsive at
    every density with the reference's rho0 - blows the blob apart.  Returns (params, pos, vel, mass, gamma):
    setParticles, then setCohesion."""
    h = np.float32(dam_break_h(n, neighbors=neighbors))
    number_density = 3.0 * neighbors / (4.0 * math.pi * float(h) ** 3)
    edge = (n / number_density) ** (1.0 / 3.0)
    if cells is None:   # the blob and its own width of room around it
        cells = max(8, int(math.ceil(edge / float(h))))
    p = default_params(float(h), [cells] * 3)
    p.central_mass = 0.0
    p.apply_gravity = 0
    p.apply_walls = 1
    mid = [0.5 * float(m) for m in (p.max_x, p.max_y, p.max_z)]
    if not edge + 2.0 * float(h) < 2.0 * min(mid):
        raise ValueError("the box is too small for this blob: more cells")
    pos = box_fill(n, [m - 0.5 * edge for m in mid], [m + 0.5 * edge for m in mid], seed)
    return p, pos, np.zeros(3 * n, np.float32), np.ones(n, np.float32), float(gamma)


def dam_break_cohesive(n, gamma, surge=0.7, box=(1.0, 1.0, 1.0), fill=(0.1, 0.75, 1.0), neighbors=32.0, seed=42,
                       gravity=-9.81):
    """The surging dam of dam_break_dye without the dye - gravity along -y, the walls on, the surge along +x - with
    cohesion: the tongue that otherwise frays into single particles holds together.  Returns (params, pos, vel,
    mass, gamma): setParticles, then setCohesion."""
    p, pos, vel, mass, _ = dam_break_dye(n, 1.0, surge, box, fill, neighbors, seed, gravity)
    return p, pos, vel, mass, float(gamma)


# Monaghan's usual choice
XSPH_EPS = 0.5


def dam_break_smoothed(n, eps=XSPH_EPS, surge=0.7, box=(1.0, 1.0, 1.0), fill=(0.1, 0.75, 1.0), neighbors=32.0, seed=42,
                       gravity=-9.81):
    """The surging dam of dam_break_dye without the dye - gravity along -y, the walls on, the surge along +x - with
    XSPH velocity smoothing: the particle-scale velocity noise of the breaking column decays while the flow keeps
    its course.  Returns (params, pos, vel, mass, eps): setParticles, then setVelocitySmoothing."""
    p, pos, vel, mass, _ = dam_break_dye(n, 1.0, surge, box, fill, neighbors, seed, gravity)
    return p, pos, vel, mass, float(eps)


def noisy_block(n, amplitude, seed=42, neighbors=32.0, cells=None):
    """A resting block with velocity noise: droplet's cubic random fill in the middle of the box (gravity and the
    central mass off, the walls on, unit masses, ~`neighbors` particles inside radius h) and a seeded uniform
    random velocity in [-amplitude, amplitude)^3 per particle - mean about zero, no structure above the particle
    scale: what XSPH is there to remove.  Returns (params, pos, vel, mass)."""
    p, pos, _, mass, _ = droplet(n, 0.0, neighbors, cells, seed)
    a = float(amplitude)
    vel = box_fill(n, (-a,) * 3, (a,) * 3, seed + 1) if a > 0.0 else np.zeros(3 * n, np.float32)
    return p, pos, vel, mass


def viscous_stable_mu(p, fraction=0.25, neighbors=32.0, mass=1.0):
    """A dynamic viscosity for SPH.setViscousStress that keeps a step damping deep inside a fluid of ~`neighbors`
    particles of `mass` inside radius h.  The explicit term is a convex combination while
    dt * (1 / m_i) * sum_j mu * V_i * V_j * kernel3 * (h - d_ij) <= 1 (include/sph_hip.h: viscous stress); with
    volumes that tile the fluid that is dt * (mu / rho) * kernel3 * pi * h^4 / 3 in scaled lengths
    (scalar_stable_kappa's integral), rho the bulk density mass * 3 * neighbors / (4 pi h^3).  Returns the mu for
    which the product is `fraction`.  Near a free surface densities are lower than the bulk's: keep a margin."""
    hs = float(p.hscaled)
    rho = float(mass) * 3.0 * float(neighbors) / (4.0 * math.pi * hs ** 3)
    return scalar_stable_kappa(p, fraction) * rho


def dam_break_viscous(n, mu, surge=0.7, box=(1.0, 1.0, 1.0), fill=(0.1, 0.75, 1.0), neighbors=32.0, seed=42,
                      gravity=-9.81):
    """The surging dam of dam_break_dye without the dye - gravity along -y, the walls on, the surge along +x - as a
    thick fluid: a viscous stress of the dynamic viscosity `mu` (viscous_stable_mu gives the scale).  Returns
    (params, pos, vel, mass, mu): setParticles, then setViscousStress."""
    p, pos, vel, mass, _ = dam_break_dye(n, 1.0, surge, box, fill, neighbors, seed, gravity)
    return p, pos, vel, mass, float(mu)


def viscous_number(p, mu, neighbors=32.0, mass=1.0):
    """viscous_stable_mu's inverse: N = dt * (mu / rho) * kernel3 * pi * h^4 / 3 of the dynamic viscosity `mu` deep
    inside a fluid of ~`neighbors` particles of `mass` inside radius h.  Up to 1 the explicit term damps; beyond it
    take the term implicitly (SPH.setViscousSolver), whose error contracts like N / (1 + N) per sweep."""
    return float(mu) / viscous_stable_mu(p, 1.0, neighbors, mass)


def dam_break_honey(n, fraction=5.0, sweeps=8, surge=0.7, box=(1.0, 1.0, 1.0), fill=(0.1, 0.75, 1.0), neighbors=32.0,
                    seed=42, gravity=-9.81):
    """dam_break_viscous's dam as a fluid too thick for the explicit term: mu is `fraction` times the bulk's explicit
    limit (viscous_stable_mu(p, fraction): viscous_number gives `fraction` back), taken by `sweeps` Jacobi sweeps.
    Returns (params, pos, vel, mass, mu, sweeps): setParticles, setViscousStress(mu), then
    setViscousSolver(sweeps)."""
    p, pos, vel, mass, _ = dam_break_viscous(n, 0.0, surge, box, fill, neighbors, seed, gravity)
    return p, pos, vel, mass, viscous_stable_mu(p, float(fraction), neighbors), int(sweeps)


def shear_layer(n, speed, seed=42, neighbors=32.0, cells=None):
    """A resting block whose upper half moves: droplet's cubic random fill in the middle of the box (gravity and
    the central mass off, the walls on, unit masses) with the velocity (speed, 0, 0) for every particle above the
    block's mid-height and rest below it - a velocity jump one particle wide, which a viscous stress spreads into a
    layer while the total momentum stays.  Returns (params, pos, vel, mass)."""
    p, pos, _, mass, _ = droplet(n, 0.0, neighbors, cells, seed)
    vel = np.zeros((n, 3), np.float32)
    vel[pos.reshape(-1, 3)[:, 1] > np.float32(0.5) * np.float32(p.max_y), 0] = np.float32(speed)
    return p, pos, np.ascontiguousarray(vel.reshape(-1)), mass


def cooling_flow(n, hot=1.0, stiffening=50.0, surge=0.7, box=(1.0, 1.0, 1.0), fill=(0.1, 0.75, 1.0), neighbors=32.0,
                 seed=42, gravity=-9.81):
    """Lava over a cold floor: dam_break_dye's surging dam, warm through and through - channel 0 is a temperature
    that starts at `hot` and diffuses (scalar_stable_kappa) - over heated_floor's slab, which holds the floor at 0,
    with an exponential ViscosityLaw on the channel: the factor is 1 at `hot` and `stiffening` at 0, so the tongue's
    underside thickens as it cools while its top keeps running.  mu is chosen so that the stiffest fluid stays inside
    the explicit range (viscous_stable_mu over `stiffening`).  Returns (params, pos, vel, mass, values[n, 4],
    kappa[4], [ScalarSource], mu, ViscosityLaw): setParticles, setScalars, setScalarSources, then
    setViscousStress(mu, law)."""
    from .scalars import ScalarSource
    from .viscosity import ViscosityLaw
    p, pos, vel, mass, _ = dam_break_dye(n, 1.0, surge, box, fill, neighbors, seed, gravity)
    h = float(p.h)
    values = np.zeros((n, 4), np.float32)
    values[:, 0] = np.float32(hot)
    kappa = np.zeros(4, np.float32)
    kappa[0] = scalar_stable_kappa(p)
    slab = ScalarSource.hold((-h, -h, -h), (float(p.max_x) + h, h, float(p.max_z) + h), 0, 0.0)
    law = ViscosityLaw.exponential(0, hot, math.log(float(stiffening)) / float(hot), 0.0, hot)
    mu = viscous_stable_mu(p, 0.25, neighbors) / float(stiffening)
    return p, pos, vel, mass, values, kappa, [slab], float(mu), law


def rankine_vortex(n, omega, core, neighbors=32.0, cells=None, seed=42):
    """A still block of fluid - droplet's fill, box and constants - swirling about the vertical (y) axis through its
    middle as a Rankine vortex: solid-body rotation at the rate `omega` within the radius `core` of the axis,
    v = omega x r with omega = (0, omega, 0), and the irrotational swirl of speed omega * core^2 / r outside it.
    The vorticity is (0, 2 * omega, 0) inside the core and zero outside: what getVelocityGradients should show.
    Returns (params, pos, vel, mass)."""
    p, pos, _, mass, _ = droplet(n, 0.0, neighbors, cells, seed)
    x = pos.reshape(-1, 3).astype(np.float64)
    dx = x[:, 0] - 0.5 * float(p.max_x)
    dz = x[:, 2] - 0.5 * float(p.max_z)
    r2 = dx * dx + dz * dz
    rate = np.where(r2 < float(core) ** 2, float(omega), float(omega) * float(core) ** 2 / np.maximum(r2, 1e-300))
    vel = np.zeros((n, 3), np.float32)
    vel[:, 0] = rate * dz
    vel[:, 2] = -rate * dx
    return p, pos, np.ascontiguousarray(vel.reshape(-1)), mass


def dyed_cut_box(p):
    """The marched box (lo, hi) that cuts the tank of dam_break_dyed and heated_floor at its mid-plane z = max_z / 2:
    the renderer's default box - the domain grown by h - with its far side in z moved to the middle.  A camera
    on the +z side then looks at a section through the fluid: renderScalars(..., box=dyed_cut_box(p), flat=True)."""
    f = np.float32
    h = f(p.h)
    lo = np.full(3, f(0.0) - h, f)
    hi = (np.array([p.max_x, p.max_y, p.max_z], f) + h).astype(f)
    hi[2] = f(0.5) * f(p.max_z)
    return lo, hi
