"""Named sets of physical constants that sit on either side of the edges the device code branches
on, and the one scene every set is run on.  tests/test_oracle_vs_reference.py pins the oracle to
the reference on each case; tests/test_gpu_param_space.py holds every mode and route to the oracle
on each case.

A case is a name and overrides applied on top of the default constants (`sph_hip_params_default`,
the oracle's `params_for_h`: the same values).  The scene's own base is the reference's defaults
without the point mass (central_mass = 0), so that the pair sums, not the point-mass term, make
most of each force; cases put the point mass back where they are about it.
"""
import math

import numpy as np

H = 0.1
CELLS = (8, 8, 8)                 # a box of 1.6 on each axis
ON_PARTICLE = (0.65, 0.65, 0.65)  # particle 0 sits here (inside the compressed block)
N_BLOCK, N_LAYER, N_SPRAY, N_WALL = 2400, 2400, 1008, 192


class Case:
    """ref_only: REF mode alone (examine_count).  position_from_force: FULL_FAST positions are held to
    what the force bar allows them (check_fast_position's fixed bar assumes a step of ~1e-3)."""

    def __init__(self, name, ref_only=False, position_from_force=False, **overrides):
        self.name = name
        self.ref_only = ref_only
        self.position_from_force = position_from_force
        self.overrides = overrides

    def __repr__(self):
        return self.name


def f32(v):
    return float(np.float32(v))


CASES = [
    # the scene's base: reference constants, no point mass
    Case("base"),
    # the reference's own point mass (1e5 at the box centre): the CFL clamp fires at the default limit
    Case("point_mass", central_mass=1e5),
    # stiffness 0: every pressure is 0, so rhoiInv = 1 and the viscous scale is the viscosity itself
    Case("stiffness_zero", stiffness=0.0),
    # stiffness x100: every pressure 100 times larger
    Case("stiffness_x100", stiffness=0.1),
    # a negative stiffness flips every pressure: the dense particles take rhoiInv = 1, the empty
    # ones 1 / p = 1e4 (a viscous scale of 100, above the 0.5 threshold of visc_keep)
    Case("stiffness_negative", stiffness=-0.001),
    # rho0 = 0: an isolated particle's pressure is exactly 0
    Case("rho0_zero", rho0=0.0),
    # rho0 above every density of the scene (the largest is 3.7e4): every pressure is negative, every
    # rhoiInv is 1
    Case("rho0_above_all", rho0=4e4),
    # no viscosity: the viscous sum is multiplied by 0 after every neighbour
    Case("viscosity_zero", viscosity=0.0),
    # a negative viscosity: the running viscous sum changes sign after every neighbour
    Case("viscosity_negative", viscosity=-0.01),
    # |mu * rhoiInv| = 0.49 for every particle (stiffness 0: no pressure, rhoiInv = 1, the force is the
    # viscous sum alone): visc_keep keeps the last 65 neighbours, fewer than the compressed block has
    Case("visc_scale_0.49", viscosity=0.49, stiffness=0.0),
    # |mu * rhoiInv| = 0.5: the first scale at which visc_keep keeps every neighbour
    Case("visc_scale_0.5", viscosity=0.5, stiffness=0.0),
    # |mu * rhoiInv| = 0.51: every neighbour, from above the threshold
    Case("visc_scale_0.51", viscosity=0.51, stiffness=0.0),
    # |mu * rhoiInv| = 1e-34 (stiffness 0 again: the force is the viscous sum alone): visc_keep keeps
    # the last neighbour only
    Case("visc_scale_below_1e-30", viscosity=1e-34, stiffness=0.0),
    # |mu * rhoiInv| = 1e-25 (stiffness 0): visc_keep's logarithm gives 1 (ceil(66.4 / 83.1)), the
    # last neighbour alone
    Case("visc_scale_1e-25", viscosity=1e-25, stiffness=0.0),
    # a small step: the integration's half kicks round differently
    Case("time_step_small", time_step=1e-5),
    # a step of 0.04: particles move by up to ~0.3 h, so the second step's neighbourhoods differ.  A
    # force within 1e-4 of 1e4 (clamped) moves a particle by up to 1 * dt^2 / 2 = 8e-4 more than the
    # oracle's: FULL_FAST positions are held to that (position_from_force), not to 1e-6 of the cell edge
    Case("time_step_large", position_from_force=True, time_step=0.04),
    # the same with the walls on: many particles cross a wall within one step
    Case("time_step_large_walls", position_from_force=True, time_step=0.04, apply_walls=1),
    # a CFL limit below most particles' force (set through SPH.setCflLimit's fp32 rule): the clamp
    # rescales most accelerations, on every route
    Case("cfl_limit_small", cfl_limit=0.007),
    # softening one fp32 step below 1e-12 without a point mass: FAST evaluates the point-mass term
    Case("softening_below_1e-12", softening=float(np.nextafter(np.float32(1e-12), np.float32(0)))),
    # softening at 1e-12 without a point mass: FAST skips the point-mass term
    Case("softening_at_1e-12", softening=f32(1e-12)),
    # softening 0, no point mass, the centre on particle 0: -G * 0 * (0 / 0) is NaN for particle 0
    Case("softening_zero_no_mass_on_particle", softening=0.0, central_pos=ON_PARTICLE),
    # softening 0 with the point mass on particle 0: 0 / 0 for that particle, huge forces next to it
    Case("softening_zero_mass_on_particle", softening=0.0, central_mass=1e5, central_pos=ON_PARTICLE),
    # G = 0 with a point mass: the term is -0 * M * g, and the FAST skip is off (M != 0)
    Case("grav_const_zero", grav_const=0.0, central_mass=1e5),
    # G = +inf without a point mass: -inf * 0 is NaN in every component of every particle
    Case("grav_const_inf", grav_const=math.inf),
    # G = -inf without a point mass: the same NaN, from the other sign
    Case("grav_const_neg_inf", grav_const=-math.inf),
    # a negative point mass pushes outwards
    Case("central_mass_negative", central_mass=-1e5),
    # walls on, damping 0: a reflected particle stops at the wall
    Case("damping_zero", damping=0.0, apply_walls=1),
    # walls on, damping 1: the reflected remainder of the step is kept whole
    Case("damping_one", damping=1.0, apply_walls=1),
    # walls on, damping 1.5: the reflection overshoots
    Case("damping_1.5", damping=1.5, apply_walls=1),
    # kernel2 * sim_scale = -2^120: the FAST pressure shift clamps at +120.  A stiffness of -2^-58 takes
    # the 2^96 back out of the pressure terms of the dense particles (negative pressure: A * B goes with
    # the stiffness squared), so that most forces stay finite
    Case("kernel2_shift_clamp_high", kernel2=-(2.0 ** 120), stiffness=-(2.0 ** -58)),
    # kernel2 * sim_scale = -1e-40 (subnormal): the FAST pressure shift clamps at -120
    Case("kernel2_shift_clamp_low", kernel2=-1e-40),
    # kernel2 = -2^-149 at a simulation scale of 1/2: the product underflows to -0 and the shift stays 0
    Case("kernel2_scale_underflow", kernel2=-(2.0 ** -149), sim_scale=0.5, sim_scale_inv=2.0),
    # hscaled = 0.95 h at sim_scale 1: sqrt(h2) > hscaled, the general instantiations run at a scale of 1
    # and the "d > hscaled" test drops the outer pairs from the density
    Case("hscaled_below_root_h2", hscaled=f32(0.95 * H)),
    # h2 = (0.95 h)^2 at sim_scale 1: sqrt(h2) < hscaled, the UNIT_SCALE instantiations, fewer neighbours
    Case("h2_below_hscaled2", h2=f32(f32(0.95 * H) ** 2)),
    # REF only, fixed at creation: the list size and the stop rule of the sampled search
    Case("examine_count_8", ref_only=True, examine_count=8),
    Case("examine_count_16", ref_only=True, examine_count=16),
    Case("examine_count_24", ref_only=True, examine_count=24),
    Case("examine_count_48", ref_only=True, examine_count=48),
    Case("examine_count_64", ref_only=True, examine_count=64),
]

FULL_CASES = [c for c in CASES if not c.ref_only]


def apply_case(p, case):
    """the case's overrides on params `p` (product SphParams or oracle OracleParams), in place"""
    for k, v in case.overrides.items():
        if k == "cfl_limit":
            # SPH.setCflLimit (reference src/sph.cpp:1237-1241): the squared limit in fp32
            lim = np.float32(v)
            p.cfl_limit = float(lim)
            p.cfl_limit2 = float(lim * lim)
        elif k in ("central_pos", "gravity"):
            arr = getattr(p, k)
            for c in range(3):
                arr[c] = v[c]
        else:
            setattr(p, k, v)
    return p


def scene(params_for_h, case=None):
    """(params, pos[3n], vel[3n], mass[n]) of the one scene, with `case` applied.  params_for_h(h,
    cells) makes the default constants: the product's default_params on the GPU, the oracle's
    params_for_h in a CPU test (which must not load the product library next to the reference's).

    6000 particles in a box of 1.6: a compressed block (~80 neighbours each), a fluid layer (~23), a
    dilute spray over the whole box (~1), and 192 particles just inside the six walls moving out;
    a seeded swirl plus noise as the velocity field; unit masses."""
    from smoothed_particle_hydrodynamics_amd import scenes
    p = params_for_h(H, CELLS)
    p.central_mass = 0.0
    box = float(np.float32(p.max_x))
    block = scenes.box_fill(N_BLOCK, (0.4, 0.4, 0.4), (0.9, 0.9, 0.9), 301).reshape(-1, 3)
    layer = scenes.box_fill(N_LAYER, (0.2, 0.15, 0.2), (1.4, 0.45, 1.4), 302).reshape(-1, 3)
    spray = scenes.box_fill(N_SPRAY, (0.02,) * 3, (box - 0.02,) * 3, 303).reshape(-1, 3)
    wall = scenes.box_fill(N_WALL, (0.1,) * 3, (box - 0.1,) * 3, 304).reshape(-1, 3)
    pos = np.concatenate([block, layer, spray, wall]).astype(np.float32)
    pos[0] = ON_PARTICLE
    n = pos.shape[0]
    c = np.float32(0.5 * box)
    noise = scenes.box_fill(n, (-1.0,) * 3, (1.0,) * 3, 305).reshape(-1, 3)
    vel = np.empty_like(pos)
    vel[:, 0] = np.float32(-3.0) * (pos[:, 2] - c) + noise[:, 0]
    vel[:, 1] = noise[:, 1]
    vel[:, 2] = np.float32(3.0) * (pos[:, 0] - c) + noise[:, 2]
    w0 = N_BLOCK + N_LAYER + N_SPRAY
    for k in range(N_WALL):
        axis, side = (k % 6) // 2, k % 2
        i = w0 + k
        pos[i, axis] = np.float32(0.001) if side == 0 else np.float32(box - 0.001)
        vel[i, axis] = np.float32(-3.0) if side == 0 else np.float32(3.0)
    if case is not None:
        apply_case(p, case)
    mass = np.ones(n, np.float32)
    return p, np.ascontiguousarray(pos.reshape(-1)), np.ascontiguousarray(vel.reshape(-1)), mass
