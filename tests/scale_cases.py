"""Parameter sets off unit scale, and the probes that reach what only the general instantiations can reach.

Every kernel that sums over neighbours exists as UNIT_SCALE true and false (csrc/launch.h: unit_scale).  The
flavours here make `sample_emulation.unit_scale(p)` false in the ways a caller can:
    SCALED     sim_scale = 0.5, sim_scale_inv = 2: every distance is halved before the kernel sees it, no pair
               is dropped, every density term grows; the integrate's displacement step is 2 dt
    SHELL      hscaled = f32(0.95 h) at a scale of 1: sqrt(h2) > hscaled, so a member with d > hscaled is counted
               and adds +0.0f - a probe can have count > 0 and a density of 0
    SCALED_UP  sim_scale = 2, sim_scale_inv = 0.5 (point samplers only): most members fall outside hscaled
Plain functions, no fixtures; tests/test_gpu_off_unit_scale.py and tests/test_tracers_cpu.py use them.
"""
import collections

import numpy as np

import sample_emulation as SE

F32 = np.float32

FLAVOURS = ("SCALED", "SHELL")
POINT_FLAVOURS = ("SCALED", "SHELL", "SCALED_UP")


def apply(p, flavour):
    """The flavour's overrides on the parameters p (SphParams or OracleParams), in place."""
    if flavour == "SCALED":
        p.sim_scale, p.sim_scale_inv = 0.5, 2.0
    elif flavour == "SCALED_UP":
        p.sim_scale, p.sim_scale_inv = 2.0, 0.5
    elif flavour == "SHELL":
        p.hscaled = float(F32(0.95 * float(F32(p.h))))
    else:
        raise ValueError(flavour)
    assert not SE.unit_scale(p), flavour
    return p


def block_scene(flavour, params_for_h=None, walls=False):
    """param_cases.scene - 6 000 particles: a compressed block, a layer, a dilute spray (the particles without a
    neighbour) and particles leaving through the walls - under the flavour."""
    import param_cases
    if params_for_h is None:
        from smoothed_particle_hydrodynamics_amd import scenes
        params_for_h = scenes.default_params
    p, pos, vel, mass = param_cases.scene(params_for_h)
    if walls:
        p.apply_walls = 1
    apply(p, flavour)
    return p, pos, vel, mass


def dam_scene(flavour):
    """scenes.dam_break(20000, speed=4), gravity and walls on (the gauges', tracers' and renderers' scene), under
    the flavour."""
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dam_break(20000, speed=4.0)
    p.apply_gravity = 1
    p.apply_walls = 1
    p.gravity[0], p.gravity[1], p.gravity[2] = 0.0, -9.81, 0.0
    apply(p, flavour)
    return p, pos, vel, mass


# float32 (m, 3) each; `every` is their concatenation in this order
Probes = collections.namedtuple("Probes", ["shell", "on", "jitter", "empty", "faces", "outside"])


def every(probes):
    return np.ascontiguousarray(np.concatenate(list(probes)).astype(F32))


def span(probes, name):
    """the rows of `name` in every(probes)"""
    k = Probes._fields.index(name)
    a = sum(len(q) for q in probes[:k])
    return slice(a, a + len(probes[k]))


def shell_probes(p, pos, vel, mass, factor=0.97):
    """Probes at factor * h from a particle that has no other particle within h, along an axis, kept where the
    particle is the probe's only member: count == 1, and under SHELL (0.97 h > hscaled) a density of +0."""
    x = np.asarray(pos, F32).reshape(-1, 3)
    g = SE.Grid(p, pos, vel, mass)
    alone = np.flatnonzero(g.sample(x, velocity=False)[2] == 1)
    step = F32(factor) * F32(p.h)
    out = []
    for a in range(3):
        for s in (F32(1.0), F32(-1.0)):
            q = x[alone].copy()
            q[:, a] = q[:, a] + s * step
            d = q - x[alone]
            d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
            keep = (g.sample(q, velocity=False)[2] == 1) & (d2 < F32(p.h2)) & (q > 0).all(1)
            out.append(q[keep])
    return np.concatenate(out).astype(F32)


def probes(p, pos, vel, mass, seed=29, n_on=512, n_jitter=512, n_empty=64):
    """The probe set of one scene, derived from it: shell probes (shell_probes), probes on particle positions,
    particle positions jittered by up to h per axis, probes with no member inside the box, probes on each of the
    box's six faces, and probes just outside the box."""
    x = np.asarray(pos, F32).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    h = F32(p.h)
    top = np.array([p.max_x, p.max_y, p.max_z], F32)
    on = x[rng.choice(len(x), n_on, replace=False)]
    jitter = (x[rng.choice(len(x), n_jitter, replace=False)] + ((rng.random((n_jitter, 3)) * 2 - 1) * h).astype(F32)).astype(F32)
    g = SE.Grid(p, pos, vel, mass)
    cand = (rng.random((4096, 3)) * top).astype(F32)
    empty = cand[g.sample(cand, velocity=False)[2] == 0][:n_empty]
    assert len(empty) == n_empty, "the scene leaves no empty space"
    faces = []
    for a in range(3):
        for v in (F32(0.0), top[a]):
            q = (rng.random((32, 3)) * top).astype(F32)
            q[:, a] = v
            faces.append(q)
    out_hi = (top + F32(1e-3) + rng.random((32, 3)).astype(F32) * F32(0.01)).astype(F32)
    out_lo = (-F32(1e-3) - rng.random((32, 3)).astype(F32) * F32(0.01)).astype(F32)
    out_lo[:, 1] = (rng.random(32) * top[1]).astype(F32)          # outside on two axes, inside on the third
    return Probes(shell_probes(p, pos, vel, mass), on, jitter, empty, np.concatenate(faces), np.concatenate([out_hi, out_lo]))


def iso_of(p, pos, vel, mass, on):
    """The iso-value of a flavour: half the median of the restatement's density over the on-particle probes.  (At
    sim_scale = 0.5 every density term grows: an iso-value written for unit scale selects nothing or everything.)"""
    rho = SE.Grid(p, pos, vel, mass).sample(np.asarray(on, F32).reshape(-1, 3), velocity=False)[0]
    return float(F32(0.5) * F32(np.median(rho)))


def zero_term_members(p, pos, vel, mass, probes):
    """Per probe: how many of its members add a term of exactly zero (d * sim_scale > hscaled)."""
    probes = np.asarray(probes, F32).reshape(-1, 3)
    g = SE.Grid(p, pos, vel, mass)
    probe, idx = g.candidates(probes)
    d = probes[probe] - g.pos[idx]
    d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    member = d2 < F32(p.h2)
    t = SE.density_terms(p, d2[member], g.mass[idx[member]])
    return np.bincount(probe[member][t == 0], minlength=len(probes))


# ---- a fluid in uniform translation: what "carried" means ------------------------------------------------------
V0 = (0.375, -1.25, 0.8125)          # every component non-zero
N_CARRIED = 256


def carried_scene():
    """scenes.dam_break(20000) under SCALED with stiffness = 0, viscosity = 0, no point mass, no gravity and no
    walls - every acceleration is exactly zero -, every particle moving at V0, and the rows of N_CARRIED interior
    particles (more than h inside the column on every axis) on which tracers are put."""
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, _, mass = scenes.dam_break(20000)
    apply(p, "SCALED")
    p.stiffness = 0.0
    p.viscosity = 0.0
    p.central_mass = 0.0
    p.apply_gravity = 0
    p.apply_walls = 0
    vel = np.ascontiguousarray(np.tile(np.array(V0, F32), (mass.size, 1)).reshape(-1))
    x = pos.reshape(-1, 3)
    h = F32(p.h)
    inside = ((x > x.min(0) + h) & (x < x.max(0) - h)).all(1)
    rows = np.flatnonzero(inside)
    rows = rows[:: max(1, len(rows) // N_CARRIED)][:N_CARRIED]
    assert len(rows) == N_CARRIED
    return p, pos, vel, mass, rows


def carried_bound(p, count, x):
    """Per tracer and component, how far a tracer set on a particle may end from that particle's new position after
    one step of carried_scene: (count + 2) * 2^-23 * |v0_c| * pos_dt + 2^-23 * max|x_c| - the fp32 error of a Shepard
    quotient over `count` same-signed terms, plus the two roundings of the move (float64)."""
    pos_dt = float(F32(p.time_step) * F32(p.sim_scale_inv))
    v0 = np.abs(np.array(V0, np.float64))
    reach = np.abs(np.asarray(x, np.float64).reshape(-1, 3)).max(0)
    return (np.asarray(count, np.float64)[:, None] + 2.0) * 2.0 ** -23 * v0[None, :] * pos_dt + 2.0 ** -23 * reach[None, :]
