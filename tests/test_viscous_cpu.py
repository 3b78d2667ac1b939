"""CPU checks of the viscous stress (include/sph_hip.h: viscous stress): csrc/viscous_policy.h, compiled with g++
behind an extern "C" shim that walks a particle's candidates the way k_viscous_apply's row walk does, against the numpy
restatement tests/viscous_emulation.py bit for bit - at unit scale and off it, with unequal masses, with and without a
law; the antisymmetry of the force addends; the guards; the law; every refusal text; the prototypes and the launch
decision beside the unchanged ones; step_impl's order; the kernels' signatures; the scenes; the physics of the
restatement on scenes.shear_layer - the explicit range, the energy, the momentum; the header's code under the host's
sanitizers."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mass_cases
import pressure_emulation as PE
import sample_emulation as SE
import scalar_emulation as SC
import scale_cases
import viscous_emulation as VE
from helpers import compile_shim

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smoothed_particle_hydrodynamics_amd", "csrc")

# One particle and its candidates in the order given, every operation of the contract through the header's
# functions: what one lane of the kernel does.
WALK = r"""
#include <math.h>

#include "viscous_policy.h"
#include "launch_policy.h"

struct WalkConsts {
   float h2, hscaled, sim_scale, kernel3, cfl_limit, cfl_limit2;
   int unit;
};

// Ri: the particle's own staged row, Mi its staged viscosity; Rj (4 floats each), Mj: the candidates'.  acc: the
// particle's acceleration, changed in place if the particle is touched; c_out: the viscous acceleration
static int walk(const WalkConsts* k, float mu, int law, const float* pi, float mi, const float* Ri, float Mi, int n,
                const float* pj, const float* Rj, const float* Mj, float* acc, float* c_out)
{
   const ViscousRow ri = {Ri[0], Ri[1], Ri[2], Ri[3]};
   ViscousSum s = {0.0f, 0.0f, 0.0f};
   for (int j = 0; j < n; j++) {
      const float dx = pi[0] - pj[3 * j], dy = pi[1] - pj[3 * j + 1], dz = pi[2] - pj[3 * j + 2];
      const float d2 = dx * dx + dy * dy + dz * dz;
      if (!(d2 < k->h2)) continue;
      const float d = scalar_distance(d2, k->sim_scale, k->unit != 0);
      const ViscousRow rj = {Rj[4 * j], Rj[4 * j + 1], Rj[4 * j + 2], Rj[4 * j + 3]};
      viscous_pair(s, viscous_pair_mu(law != 0, mu, Mi, law ? Mj[j] : 0.0f), d, k->hscaled, k->kernel3, ri, rj);
   }
   const ViscousSum c = viscous_accel(s, mi);
   c_out[0] = c.x; c_out[1] = c.y; c_out[2] = c.z;
   if (!viscous_acts(ri.w, mi, c)) return 0;
   viscous_apply(c, k->cfl_limit, k->cfl_limit2, acc[0], acc[1], acc[2]);
   return 1;
}
"""

SHIM = WALK + r"""
extern "C" {
int abi() { return SPH_HIP_ABI_VERSION; }
int max_keys() { return SPH_HIP_MAX_VISCOSITY_KEYS; }
int law_bytes() { return (int)sizeof(sph_hip_viscosity_law); }
void stage(float vx, float vy, float vz, float m, float rho, float* out)
{
   const ViscousRow r = viscous_stage(vx, vy, vz, m, rho);
   out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
}
float factor(const sph_hip_viscosity_law* law, float x) { return viscous_factor(*law, x); }
float stage_mu(float mu, const sph_hip_viscosity_law* law, const float* T4)
{
   return viscous_stage_mu(mu, *law, viscous_channel(law->channel, T4[0], T4[1], T4[2], T4[3]));
}
void accel(const float* s, float m, float* out)
{
   const ViscousSum c = viscous_accel(ViscousSum{s[0], s[1], s[2]}, m);
   out[0] = c.x; out[1] = c.y; out[2] = c.z;
}
int particle(const WalkConsts* k, float mu, int law, const float* pi, float mi, const float* Ri, float Mi, int n,
             const float* pj, const float* Rj, const float* Mj, float* acc, float* c_out)
{
   return walk(k, mu, law, pi, mi, Ri, Mi, n, pj, Rj, Mj, acc, c_out);
}
static const char* text(const char* w) { return w ? w : ""; }
int is_off(float mu) { return viscous_is_off(mu) ? 1 : 0; }
const char* mu_finite_check(float mu) { return text(viscous_mu_finite_check(mu)); }
const char* mu_sign_check(float mu) { return text(viscous_mu_sign_check(mu)); }
const char* law_channel_check(const sph_hip_viscosity_law* law) { return text(viscous_law_channel_check(*law)); }
const char* law_keys_check(const sph_hip_viscosity_law* law) { return text(viscous_law_keys_check(*law)); }
const char* law_values_finite_check(const sph_hip_viscosity_law* law) { return text(viscous_law_values_finite_check(*law)); }
const char* law_ascending_check(const sph_hip_viscosity_law* law) { return text(viscous_law_ascending_check(*law)); }
const char* law_factors_finite_check(const sph_hip_viscosity_law* law) { return text(viscous_law_factors_finite_check(*law)); }
const char* law_factors_sign_check(const sph_hip_viscosity_law* law) { return text(viscous_law_factors_sign_check(*law)); }
const char* law_check(const sph_hip_viscosity_law* law) { return text(viscous_law_check(*law)); }
const char* law_scalars_check(int n_scalars) { return text(viscous_law_scalars_check(n_scalars)); }
const char* mode_check(int full_mode) { return text(viscous_mode_check(full_mode != 0)); }
const char* slab_check(int whole_grid) { return text(viscous_slab_check(whole_grid != 0)); }
const char* ports_set_check(int ports_set) { return text(viscous_ports_set_check(ports_set != 0)); }
const char* ports_check(int have, int ne, int ns) { return text(viscous_ports_check(have != 0, ne, ns)); }
void law_clean(const sph_hip_viscosity_law* law, sph_hip_viscosity_law* out) { *out = viscous_law_clean(law); }
// the launch decisions: the new one beside XSPH's, cohesion's and buoyancy's
int launches(int have, int n) { return step_launches_viscous(have != 0, n) ? 1 : 0; }
int launches_xsph(int have, int n) { return step_launches_xsph(have != 0, n) ? 1 : 0; }
int launches_cohesion(int have, int n) { return step_launches_cohesion(have != 0, n) ? 1 : 0; }
int launches_buoyancy(int have, int n_scalars, int n) { return step_launches_buoyancy(have != 0, n_scalars, n) ? 1 : 0; }
int fuse7(int hash_too, int tiled, int n, int no_fused, int n_obst, int loads, int between)
{
   return fuse_integrate(hash_too, tiled, n, no_fused, n_obst, loads, between) ? 1 : 0;
}
}
"""

CHECKS_OF_A_LAW = ("law_channel_check", "law_keys_check", "law_values_finite_check", "law_ascending_check",
                   "law_factors_finite_check", "law_factors_sign_check", "law_check")


class WalkConsts(C.Structure):
    _fields_ = [("h2", C.c_float), ("hscaled", C.c_float), ("sim_scale", C.c_float), ("kernel3", C.c_float),
                ("cfl_limit", C.c_float), ("cfl_limit2", C.c_float), ("unit", C.c_int)]


def consts_of(p):
    return WalkConsts(p.h2, p.hscaled, p.sim_scale, p.kernel3, p.cfl_limit, p.cfl_limit2, 1 if SE.unit_scale(p) else 0)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def struct_of(lw):
    from smoothed_particle_hydrodynamics_amd.viscosity import SphViscosityLaw
    q = SphViscosityLaw()
    q.channel, q.n_keys = lw.channel, lw.values.size
    for k in range(min(lw.values.size, 16)):
        q.value[k], q.factor[k] = float(lw.values[k]), float(lw.factors[k])
    return q


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    lib = compile_shim(SHIM, ["-O2", "-ffp-contract=off"], tmp_path_factory)
    V, I, F = C.c_void_p, C.c_int, C.c_float
    lib.particle.argtypes = [V, F, I, V, F, V, F, I, V, V, V, V, V]
    lib.stage.argtypes = [F, F, F, F, F, V]
    lib.stage.restype = None
    lib.factor.argtypes = [V, F]
    lib.factor.restype = F
    lib.stage_mu.argtypes = [F, V, V]
    lib.stage_mu.restype = F
    lib.accel.argtypes = [V, F, V]
    lib.accel.restype = None
    lib.law_clean.argtypes = [V, V]
    lib.law_clean.restype = None
    for name in CHECKS_OF_A_LAW:
        getattr(lib, name).argtypes = [V]
    for name, args in (("mu_finite_check", [F]), ("mu_sign_check", [F]), ("law_scalars_check", [I]), ("mode_check", [I]),
                       ("slab_check", [I]), ("ports_set_check", [I]), ("ports_check", [I, I, I])):
        getattr(lib, name).argtypes = args
    for name in CHECKS_OF_A_LAW + ("mu_finite_check", "mu_sign_check", "law_scalars_check", "mode_check", "slab_check",
                                   "ports_set_check", "ports_check"):
        getattr(lib, name).restype = C.c_char_p
    lib.is_off.argtypes = [F]
    return lib


def header_particle(policy, p, mu, pi, mi, Ri, pj, Rj, acc, Mi=None, Mj=None):
    a, c = np.ascontiguousarray(acc, F32).copy(), np.zeros(3, F32)
    k = consts_of(p)
    pj = np.ascontiguousarray(pj, F32).reshape(-1, 3)
    Rj = np.ascontiguousarray(Rj, F32).reshape(-1, 4)
    law = Mi is not None
    Mj = np.ascontiguousarray(Mj if law else np.zeros(pj.shape[0]), F32)
    touched = policy.particle(C.byref(k), float(mu), int(law), ptr(np.ascontiguousarray(pi, F32)), float(mi),
                              ptr(np.ascontiguousarray(Ri, F32)), float(Mi) if law else 0.0, pj.shape[0], ptr(pj), ptr(Rj),
                              ptr(Mj), ptr(a), ptr(c))
    return a, bool(touched), c


# ---- the header against the restatement ----------------------------------------------------------------------
COUNTS = (0, 1, 7, 8, 9, 200)
LAW = VE.law(2, [0.0, 0.25, 0.5, 1.0], [8.0, 3.0, 1.5, 1.0])


def params_of(flavour):
    from smoothed_particle_hydrodynamics_amd import scenes
    p, _, _, _ = scenes.dam_break(2001)
    if flavour != "UNIT":
        scale_cases.apply(p, flavour)
    return p


def bulk_density(p):
    """about what 32 unit masses inside the radius give"""
    return 32.0 * 3.0 / (4.0 * math.pi * float(p.hscaled) ** 3)


def mu_for(p):
    """a mu for which a seeded particle's viscous acceleration is of the order of its velocity differences over a
    step: scenes.viscous_stable_mu's formula"""
    from smoothed_particle_hydrodynamics_amd import scenes
    return float(F32(scenes.viscous_stable_mu(p, 0.25)))



def seeded_particle(rng, p, k, masses="UNIT"):
    """A particle with k candidates within 1.1 h per axis (members and non-members), velocities in [-1, 1)^3,
    densities about the bulk's, masses by mass_cases' flavour (the particle is id 0, the candidates 1 .. k), an
    acceleration in [-1, 1)^3 and channel rows in [-0.2, 1.2)."""
    h = F32(p.h)
    pi = rng.uniform(0.2, 0.8, 3).astype(F32)
    pj = (pi[None, :] + rng.uniform(-1.1, 1.1, (k, 3)).astype(F32) * h).astype(F32)
    m = mass_cases.masses(masses, p, np.zeros(3 * 201, F32))[:k + 1]          # (by id: the first k + 1 of one draw)
    rho = (bulk_density(p) * rng.uniform(0.5, 2.0, k + 1)).astype(F32)
    vel = rng.uniform(-1.0, 1.0, (k + 1, 3)).astype(F32)
    R = VE.stage(vel, m, rho)
    T = rng.uniform(-0.2, 1.2, (k + 1, 4)).astype(F32)
    acc = rng.uniform(-1.0, 1.0, 3).astype(F32)
    return pi, m[0], R[0], pj, R[1:], acc, T


def same_particle(got, want):
    return (np.array_equal(bits(got[0]), bits(want[0])) and got[1] == want[1] and np.array_equal(bits(got[2]), bits(want[2])))


@pytest.mark.parametrize("with_law", [False, True])
@pytest.mark.parametrize("masses", ["UNIT", "SPREAD", "TWO_SPECIES"])
@pytest.mark.parametrize("flavour", ["UNIT", "SCALED", "SHELL"])
def test_header_equals_the_restatement_bit_for_bit(policy, hiplib, flavour, masses, with_law):
    p = params_of(flavour)
    assert SE.unit_scale(p) == (flavour == "UNIT")
    mu = mu_for(p)
    rng = np.random.default_rng(2024)
    members_seen = negative_L = touched = 0
    for k in COUNTS:
        for row in range(16):
            pi, mi, Ri, pj, Rj, acc, T = seeded_particle(rng, p, k, masses)
            M = VE.stage_mu(mu, LAW, T) if with_law else None
            Mi, Mj = (M[0], M[1:]) if with_law else (None, None)
            want = VE.particle(p, mu, pi, mi, Ri, pj, Rj, acc, Mi, Mj)
            got = header_particle(policy, p, mu, pi, mi, Ri, pj, Rj, acc, Mi, Mj)
            assert same_particle(got, want), (k, row)
            r = pi[None, :] - pj
            d2 = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2]
            member = d2 < F32(p.h2)
            members_seen += int(member.sum())
            negative_L += int((SC.distance(SC.consts_of(p), d2[member]) > F32(p.hscaled)).sum())
            touched += int(got[1])
            if k == 0:      # no neighbour: nothing changes, c is +0
                assert not got[1] and np.array_equal(bits(got[0]), bits(acc)) and not bits(got[2]).any()
            if got[1]:
                assert np.isfinite(got[0]).all() and not np.array_equal(bits(got[0]), bits(acc))
    assert members_seen > 700 and touched > 60
    # SHELL: members beyond hscaled, whose Laplacian is negative - no extra rule
    assert (negative_L > 20) == (flavour == "SHELL")
    if masses != "UNIT":
        assert not mass_cases.uniform(mass_cases.masses(masses, p, np.zeros(30, F32)))


def test_the_stage_and_the_acceleration_are_correctly_rounded_divisions(policy):
    rng = np.random.default_rng(3)
    rho = np.concatenate([rng.uniform(1.0, 5.0e4, 200), [0.0, -0.0, -3.0, np.inf, np.nan, 1e-45, 3e38]]).astype(F32)
    m = rng.uniform(0.5, 4.0, rho.size).astype(F32)
    vel = rng.uniform(-2.0, 2.0, (rho.size, 3)).astype(F32)
    vel[0, 0] = F32(-0.0)
    want = VE.stage(vel, m, rho)
    exact = (m[:200].astype(np.float64) / rho[:200].astype(np.float64)).astype(F32)      # one rounding
    assert np.array_equal(bits(want[:200, 3]), bits(exact))
    for i in range(rho.size):
        out = np.zeros(4, F32)
        policy.stage(float(vel[i, 0]), float(vel[i, 1]), float(vel[i, 2]), float(m[i]), float(rho[i]), ptr(out))
        assert np.array_equal(bits(out), bits(want[i])), i
    # rho not > 0 (0, -0, negative, NaN): the volume is +0; inf gives m / inf = +0 too
    assert not bits(want[200:205, 3]).any()
    # c = s / m: three divisions, each the float64 quotient rounded once
    s = rng.uniform(-3.0, 3.0, (200, 3)).astype(F32)
    for i in range(200):
        out = np.zeros(3, F32)
        policy.accel(ptr(s[i]), float(m[i]), ptr(out))
        assert np.array_equal(bits(out), bits((s[i].astype(np.float64) / np.float64(m[i])).astype(F32)))
        assert np.array_equal(bits(out), bits(VE.accel(s[i], m[i:i + 1])[0]))


# ---- antisymmetry ------------------------------------------------------------------------------------------------
NB, SPEED, SEED = 3000, 0.5, 42


@pytest.fixture(scope="module")
def layer(hiplib):
    """shear_layer(3000, 0.5) with the restatement's densities (pressure_emulation.particle_density: the density
    pass's sums)"""
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.shear_layer(NB, SPEED, SEED)
    rho = PE.particle_density(p, pos, vel, mass)
    assert (rho > 0).all()                       # every particle has a neighbour
    return p, pos, vel, mass, rho


@pytest.mark.parametrize("with_law", [False, True])
@pytest.mark.parametrize("masses", mass_cases.FLAVOURS)
def test_the_force_addends_of_a_pair_negate_each_other_for_any_masses(layer, masses, with_law):
    """g_ij = (m_ij * (V_i * V_j)) * L: every factor is symmetric in i and j by bits, and v_j - v_i is the exact
    negation of v_i - v_j.  So the addend of (i, j) is the bitwise negation of (j, i)'s, whatever the masses."""
    p, pos, _, _, _ = layer
    rng = np.random.default_rng(8)
    vel = rng.uniform(-1.0, 1.0, 3 * NB).astype(F32)
    mass = mass_cases.masses(masses, p, pos)
    rho = PE.particle_density(p, pos, vel, mass)
    T = rng.uniform(-0.2, 1.2, (NB, 4)).astype(F32)
    mu = mu_for(p)
    _, info = VE.sums(p, mu, pos, vel, mass, rho, LAW if with_law else None, T, with_info=True)
    terms, pr, idx = info["terms"], info["probe"], info["idx"]
    assert info["on"].all() and terms.shape[0] > 60000
    key = np.argsort(idx * NB + pr, kind="stable")          # (j, i) in the order of (i, j)
    assert np.array_equal((idx * NB + pr)[key], pr * NB + idx)
    assert np.array_equal(bits(terms) ^ np.uint32(0x80000000), bits(terms[key]))
    assert (bits(terms) & 0x7fffffff).any(1).sum() > 60000          # and they are not zeros
    for a in range(3):
        assert math.fsum(terms[:, a].astype(np.float64)) == 0.0
    # the masses do tell: the accelerations differ from what unit masses give in nearly every row
    unit = VE.apply(p, mu, pos, vel, np.ones(NB, F32), rho, np.zeros(3 * NB, F32))[2]
    mine = VE.apply(p, mu, pos, vel, mass, rho, np.zeros(3 * NB, F32))[2]
    assert mass_cases.rows_differing(unit, mine).sum() > 0.4 * NB


# ---- guards --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["UNIT", "SCALED", "SHELL"])
def test_guards_and_switch_off(policy, hiplib, flavour):
    p = params_of(flavour)
    mu = mu_for(p)
    rng = np.random.default_rng(7)
    pi, mi, Ri, pj, Rj, acc, T = seeded_particle(rng, p, 9, "SPREAD")
    r = pi[None, :] - pj
    inside = np.flatnonzero((r * r).sum(1) < 0.5 * float(p.h2))
    assert inside.size >= 1

    def both(mu_, Ri_, Rj_, mi_=mi, pj_=pj, Mi=None, Mj=None):
        got = header_particle(policy, p, mu_, pi, mi_, Ri_, pj_, Rj_, acc, Mi, Mj)
        assert same_particle(got, VE.particle(p, mu_, pi, mi_, Ri_, pj_, Rj_, acc, Mi, Mj))
        return got

    base = both(mu, Ri, Rj)
    assert base[1]
    # a member with V_j == 0 is skipped by selection, whatever its row holds: a NaN velocity does not reach the sum
    Rz = Rj.copy()
    Rz[inside[0]] = [np.nan, np.inf, -np.nan, 0.0]
    got = both(mu, Ri, Rz)
    assert got[1] and np.isfinite(got[2]).all()
    without = both(mu, Ri, np.delete(Rj, inside[0], 0), pj_=np.delete(pj, inside[0], 0))
    assert same_particle(got, without)
    Rz[inside[0], 3] = F32(-0.0)                                     # (-0.0f == 0: skipped too)
    assert same_particle(both(mu, Ri, Rz), without)
    # V_i == 0 stores nothing, and neither does a mass that is not > 0
    R0 = Ri.copy()
    R0[3] = 0.0
    got = both(mu, R0, Rj)
    assert not got[1] and np.array_equal(bits(got[0]), bits(acc))
    for bad_mass in (0.0, -1.0, np.nan):
        got = both(mu, Ri, Rj, mi_=bad_mass)
        assert not got[1] and np.array_equal(bits(got[0]), bits(acc))
    # every neighbour moves as the particle does: every addend is g * 0, the sum is zero, nothing is stored
    Ru = Rj.copy()
    Ru[:, :3] = Ri[None, :3]
    got = both(mu, Ri, Ru)
    assert not got[1] and np.array_equal(bits(got[0]), bits(acc)) and not (bits(got[2]) & 0x7fffffff).any()
    # a NaN or infinite operand reaches the sum: c is not finite and the guard leaves the particle alone
    for col, bad in ((0, np.nan), (1, np.inf), (3, np.inf), (3, np.nan)):
        Rb = Rj.copy()
        Rb[inside[0], col] = bad
        got = both(mu, Ri, Rb)
        assert not got[1] and not np.isfinite(got[2]).all() and np.array_equal(bits(got[0]), bits(acc))
    Rn = Ri.copy()
    Rn[3] = np.nan                                                    # ... the particle's own volume too
    got = both(mu, Rn, Rj)
    assert not got[1] and np.isnan(got[2]).all()
    M = VE.stage_mu(mu, LAW, T)
    Mb = M[1:].copy()
    Mb[inside[0]] = np.inf                                            # ... and a staged viscosity
    got = both(mu, Ri, Rj, Mi=M[0], Mj=Mb)
    assert not got[1] and not np.isfinite(got[2]).all() and np.array_equal(bits(got[0]), bits(acc))
    # a candidate with a NaN position is no member
    with_nan = np.insert(pj, 4, [np.nan, pi[1], pi[2]], axis=0)
    assert same_particle(both(mu, Ri, np.insert(Rj, 4, Rj[0], axis=0), pj_=with_nan), base)
    # mu = 0 is off by bits: every g is +-0, c is zero, nothing is stored
    for zero in (0.0, -0.0):
        assert policy.is_off(zero) == 1
        got = both(zero, Ri, Rj)
        assert not got[1] and np.array_equal(bits(got[0]), bits(acc)) and not (bits(got[2]) & 0x7fffffff).any()
    assert policy.is_off(1e-45) == 0 and policy.is_off(mu) == 0


def test_a_uniform_velocity_stores_nothing_and_adding_one_keeps_the_bits(layer):
    """Velocities on a 2^-12 lattice and a uniform velocity on the same lattice: every v + u is representable, every
    difference v_j - v_i is exact and the same with and without u, so c has the same bits.  A uniform field alone
    stores nothing."""
    p, pos, _, mass, rho = layer
    mu = mu_for(p)
    rng = np.random.default_rng(12)
    q = F32(2.0 ** -12)
    v0 = (np.round(rng.uniform(-0.5, 0.5, 3 * NB) / q) * q).astype(F32)
    u = np.array([0.5, -0.25, 1.0 + 3.0 * 2.0 ** -12], F32)
    v1 = (v0.reshape(-1, 3) + u[None, :]).astype(F32)
    assert np.array_equal(v1.astype(np.float64), v0.reshape(-1, 3).astype(np.float64) + u.astype(np.float64)[None, :])
    zero = np.zeros(3 * NB, F32)
    a0, on0, c0, _ = VE.apply(p, mu, pos, v0, mass, rho, zero)
    a1, on1, c1, _ = VE.apply(p, mu, pos, v1.reshape(-1), mass, rho, zero)
    assert np.array_equal(bits(c0), bits(c1)) and np.array_equal(on0, on1) and on0.sum() > NB - 5
    assert np.array_equal(bits(a0), bits(a1)) and a0.any()
    only = np.repeat(u[None, :], NB, 0).reshape(-1)
    acc = rng.uniform(-1.0, 1.0, 3 * NB).astype(F32)
    new, on, c, _ = VE.apply(p, mu, pos, only, mass, rho, acc)
    assert not on.any() and np.array_equal(bits(new), bits(acc)) and not (bits(c) & 0x7fffffff).any()


# ---- the law ---------------------------------------------------------------------------------------------------------
def header_factor(policy, lw, x):
    q = struct_of(lw)
    return np.array([policy.factor(C.byref(q), float(v)) for v in np.asarray(x, F32).reshape(-1)], F32)


def test_the_law_below_on_between_and_above_its_keys(policy):
    lw = VE.law(1, [-1.0, 0.0, 0.5, 2.0], [4.0, 2.0, 0.0, 3.0])
    x = F32([-5.0, -1.0, np.nextafter(F32(-1.0), F32(0.0)), -0.5, 0.0, 0.25, 0.5, 1.25, np.nextafter(F32(2.0), F32(0.0)),
             2.0, 7.0, np.nan, np.inf, -np.inf])
    want = VE.factor(lw, x)
    got = header_factor(policy, lw, x)
    assert np.array_equal(bits(got), bits(want))
    # below and on the first key, NaN and -inf: f_0; on and above the last, +inf: f_{K-1}; on an inner key: its factor
    assert list(want[[0, 1, 11, 13]]) == [4.0] * 4 and list(want[[9, 10, 12]]) == [3.0] * 3
    assert want[3] == 3.0 and want[4] == 2.0 and want[5] == 1.0 and want[6] == 0.0 and want[7] == 1.5
    assert 3.99 < want[2] <= 4.0 and 2.99 < want[8] < 3.0      # (a step of one ulp off the first key rounds back to f_0)
    # -0.0f as the first factor keeps its bits where the first key is not exceeded
    neg = VE.law(0, [0.0, 1.0], [-0.0, 1.0])
    assert bits(header_factor(policy, neg, [0.0]))[0] == 0x80000000 == bits(VE.factor(neg, F32([0.0])))[0]


@pytest.mark.parametrize("keys", [2, 3, 16])
def test_the_law_with_two_and_with_sixteen_keys_and_unfused(policy, keys):
    """Seeded inputs across and beyond the table; the header's bits are the restatement's, the quotient u is the float64
    quotient rounded once, and f_k + u * (f_{k+1} - f_k) is told from a fused multiply-add on many inputs."""
    rng = np.random.default_rng(100 + keys)
    values = np.sort(rng.uniform(-1.0, 2.0, keys)).astype(F32)
    assert (np.diff(values) > 0).all()
    factors = rng.uniform(0.0, 10.0, keys).astype(F32)
    lw = VE.law(3, values, factors)
    span = float(values[-1] - values[0])
    x = np.concatenate([rng.uniform(values[0] - 0.3 * span, values[-1] + 0.3 * span, 400).astype(F32), values,
                        [np.nan, np.inf, -np.inf]]).astype(F32)
    want = VE.factor(lw, x)
    got = header_factor(policy, lw, x)
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(want[400:400 + keys], factors)               # on a key: its factor
    inner = np.flatnonzero((x > values[0]) & (x < values[-1]))
    assert inner.size > 150
    k = np.searchsorted(values, x[inner], side="right") - 1
    xk, xk1, fk, fk1 = values[k], values[k + 1], factors[k], factors[k + 1]
    u = ((x[inner] - xk).astype(np.float64) / (xk1 - xk).astype(np.float64)).astype(F32)        # one rounding
    plain = (fk + (u * (fk1 - fk)).astype(F32)).astype(F32)
    assert np.array_equal(bits(plain), bits(want[inner]))
    fused = (fk.astype(np.float64) + u.astype(np.float64) * (fk1 - fk).astype(np.float64)).astype(F32)
    assert (bits(fused) != bits(want[inner])).sum() > 20
    # the staged viscosity: mu times the factor of the law's channel, whichever channel that is
    T = rng.uniform(-1.5, 2.5, (50, 4)).astype(F32)
    q = struct_of(lw)
    for c in range(4):
        lc = VE.law(c, values, factors)
        q.channel = c
        M = VE.stage_mu(0.37, lc, T)
        assert np.array_equal(bits(M), bits((F32(0.37) * VE.factor(lc, T[:, c])).astype(F32)))
        for i in range(50):
            assert bits(np.array([policy.stage_mu(0.37, C.byref(q), ptr(T[i]))], F32))[0] == bits(M[i:i + 1])[0]


# ---- refusals ------------------------------------------------------------------------------------------------
def test_every_refusal_text(policy):
    for ok in (0.0, -0.0, 1.0, 1e-45, 3e38):
        assert policy.mu_finite_check(ok) == b"" and policy.mu_sign_check(ok) == b""
    for bad in (np.nan, np.inf, -np.inf):
        assert policy.mu_finite_check(bad) == b"a viscosity that is not finite"
    for bad in (-1e-45, -0.5, -3e38):
        assert policy.mu_finite_check(bad) == b"" and policy.mu_sign_check(bad) == b"a negative viscosity"
    assert [policy.is_off(e) for e in (0.0, -0.0, 1e-45, 1.0)] == [1, 1, 0, 0]

    def check(name, lw):
        return getattr(policy, name)(C.byref(struct_of(lw)))

    good = VE.law(0, [0.0, 1.0], [2.0, 0.0])
    full = VE.law(3, np.arange(16), np.arange(16))
    for lw in (good, full):
        for name in CHECKS_OF_A_LAW:
            assert check(name, lw) == b"", name
    cases = (
        ("law_channel_check", VE.law(-1, [0.0, 1.0], [1.0, 1.0]), b"a law channel outside 0..3"),
        ("law_channel_check", VE.law(4, [0.0, 1.0], [1.0, 1.0]), b"a law channel outside 0..3"),
        ("law_keys_check", VE.law(0, [0.0], [1.0]), b"a law with fewer than 2 or more than 16 keys"),
        ("law_keys_check", VE.law(0, [], []), b"a law with fewer than 2 or more than 16 keys"),
        ("law_values_finite_check", VE.law(0, [0.0, np.inf], [1.0, 1.0]), b"a key value that is not finite"),
        ("law_values_finite_check", VE.law(0, [np.nan, 1.0], [1.0, 1.0]), b"a key value that is not finite"),
        ("law_ascending_check", VE.law(0, [0.0, 1.0, 1.0], [1.0, 1.0, 1.0]), b"key values that are not strictly ascending"),
        ("law_ascending_check", VE.law(0, [0.0, -1.0], [1.0, 1.0]), b"key values that are not strictly ascending"),
        ("law_factors_finite_check", VE.law(0, [0.0, 1.0], [1.0, np.inf]), b"a key factor that is not finite"),
        ("law_factors_finite_check", VE.law(0, [0.0, 1.0], [np.nan, 1.0]), b"a key factor that is not finite"),
        ("law_factors_sign_check", VE.law(0, [0.0, 1.0], [1.0, -1e-45]), b"a negative key factor"),
    )
    for name, lw, text in cases:
        assert check(name, lw) == text, name
        assert check("law_check", lw) == text, name               # the composed check says the same
    too_many = struct_of(good)
    too_many.n_keys = 17
    assert policy.law_keys_check(C.byref(too_many)) == b"a law with fewer than 2 or more than 16 keys"
    # a value beyond n_keys is not looked at
    junk = struct_of(good)
    junk.value[5], junk.factor[5] = float("nan"), -1.0
    assert policy.law_check(C.byref(junk)) == b""
    cleaned = struct_of(good)
    policy.law_clean(C.byref(junk), C.byref(cleaned))
    assert bytes(cleaned) == bytes(struct_of(good))
    policy.law_clean(None, C.byref(cleaned))
    assert bytes(cleaned) == bytes(C.sizeof(cleaned))
    assert policy.law_scalars_check(5) == b"" and policy.law_scalars_check(0) == b"a viscosity law on a context without scalars"
    assert policy.mode_check(1) == b"" and policy.mode_check(0) == b"FULL and FULL_FAST contexts only"
    assert policy.slab_check(1) == b""
    assert policy.slab_check(0) == b"slab contexts (with neighbours, or that have exchanged) cannot have viscous stress"
    assert policy.ports_set_check(0) == b""
    assert policy.ports_set_check(1) == b"a context with ports cannot have viscous stress"
    for have in (0, 1):
        for ne in (0, 2):
            for ns in (0, 3):
                want = b"a context with viscous stress cannot have ports" if have and (ne or ns) else b""
                assert policy.ports_check(have, ne, ns) == want


def test_the_host_calls_refuse_in_the_headers_words():
    text = open(os.path.join(CSRC, "sph_hip.hip")).read()
    body = text[text.index("int sph_hip_set_viscous_stress("):text.index("int sph_hip_get_viscous_stress(")]
    calls = ("viscous_mu_finite_check(mu)", "viscous_mu_sign_check(mu)", "viscous_law_channel_check(*law)",
             "viscous_law_keys_check(*law)", "viscous_law_values_finite_check(*law)", "viscous_law_ascending_check(*law)",
             "viscous_law_factors_finite_check(*law)", "viscous_law_factors_sign_check(*law)",
             "viscous_law_scalars_check(ctx->n_scalars)", "viscous_mode_check(", "viscous_slab_check(",
             "viscous_ports_set_check(")
    for call in calls:
        assert re.search(r"if \(const char\* why = %s.*\) return refuse\(ctx, who, why\);" % re.escape(call), body), call
    assert [body.index(c) for c in calls] == sorted(body.index(c) for c in calls)
    assert "hipStreamSynchronize" not in body and "hipDeviceSynchronize" not in body      # the setter does not wait
    # switching it off is never refused: the law's, the context's checks and the allocation stand behind the off test
    off = body.index("if (!viscous_is_off(mu)) {")
    assert (body.index("viscous_mu_sign_check(mu)") < off < body.index("viscous_law_channel_check(")
            < body.index("dev_alloc(rows"))
    assert "!ctx->viscous_R && dev_alloc(rows" in body and "with_law && !ctx->viscous_M && dev_alloc(mus" in body
    ports = text[text.index("int sph_hip_set_ports("):]
    ports = ports[:ports.index("ports_restart(ctx)")]
    assert "viscous_ports_check(ctx->have_viscous != 0, ne, ns)) return refuse(ctx, who, why);" in ports
    upload = text[text.index("static int upload_impl("):text.index("static int all_same_mass(")]
    assert "ctx->have_viscous = 0;" in upload and "ctx->have_viscous_law = 0;" in upload
    scalars = text[text.index("int sph_hip_set_scalars("):text.index("int sph_hip_get_scalars(")]
    off_branch = scalars[scalars.index("if (!values4 || n == 0) {"):scalars.index("if (!ctx->scalar_T)")]
    assert "ctx->have_viscous_law = 0;" in off_branch and "have_viscous =" not in off_branch      # the law goes, mu stays
    # no context allocates the rows at creation: the setter is the only place of this file that names them
    assert text.count("viscous_R") == body.count("viscous_R") > 0 and text.count("viscous_M") == body.count("viscous_M") > 0


# ---- signatures ------------------------------------------------------------------------------------------------
def test_prototypes_and_abi(policy, hiplib):
    from smoothed_particle_hydrodynamics_amd import lib as L
    from smoothed_particle_hydrodynamics_amd import viscosity as VS
    assert policy.abi() == 7 and L.ABI_VERSION == 7
    assert policy.max_keys() == 16 == VS.MAX_KEYS and policy.law_bytes() == C.sizeof(VS.SphViscosityLaw) == 136
    V, I, F, Q = C.c_void_p, C.c_int, C.c_float, C.POINTER
    assert L.PROTOTYPES["sph_hip_set_viscous_stress"] == (I, [V, F, Q(VS.SphViscosityLaw)])
    assert L.PROTOTYPES["sph_hip_get_viscous_stress"] == (I, [V, Q(F), Q(VS.SphViscosityLaw), Q(I)])
    text = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    assert re.search(r"#define SPH_HIP_ABI_VERSION 7\b", text)
    section = text[text.index("---- viscous stress"):text.index("int sph_hip_set_viscous_stress(")]
    flat = section.replace("\n *", " ")
    assert re.search(r"added without a change of\s+SPH_HIP_ABI_VERSION", flat)
    assert "NOT apply the viscous stress" in re.sub(r"\s+", " ", flat)
    assert "NOTHING polices this" in flat
    assert re.search(r"\bint sph_hip_set_viscous_stress\(sph_hip_context\* ctx, float mu, "
                     r"const sph_hip_viscosity_law\* law_or_null\);", text)
    assert re.search(r"\bint sph_hip_get_viscous_stress\(sph_hip_context\* ctx, float\* mu, sph_hip_viscosity_law\* law, "
                     r"int\* have_law\);", text)
    for name in ("set_viscous_stress", "get_viscous_stress"):
        assert hasattr(hiplib, "sph_hip_" + name)
    # a null context is refused without touching the device
    assert hiplib.sph_hip_set_viscous_stress(None, 0.5, None) < 0
    assert hiplib.sph_hip_get_viscous_stress(None, None, None, None) < 0
    import smoothed_particle_hydrodynamics_amd as S
    assert callable(S.SPH.setViscousStress) and callable(S.SPH.getViscousStress) and S.ViscosityLaw is VS.ViscosityLaw
    from smoothed_particle_hydrodynamics_amd import build as B
    assert "viscous_kernels.h" in B.HEADERS and "viscous_policy.h" in B.HEADERS
    policy_text = open(os.path.join(CSRC, "viscous_policy.h")).read()
    assert "NOTHING polices this" in policy_text


def test_the_python_laws():
    from smoothed_particle_hydrodynamics_amd import ViscosityLaw
    from smoothed_particle_hydrodynamics_amd import viscosity as VS
    law = ViscosityLaw(2, [0.0, 1.0, 3.0], [4.0, 2.0, 0.0])
    q = law.to_struct()
    assert (q.channel, q.n_keys, list(q.value)[:4], list(q.factor)[:4]) == (2, 3, [0.0, 1.0, 3.0, 0.0], [4.0, 2.0, 0.0, 0.0])
    assert VS.from_struct(q) == law and hash(VS.from_struct(q)) == hash(law) and "channel=2" in repr(law)
    xs = (-1.0, 0.0, 0.5, 1.0, 2.0, 3.0, 9.0, float("nan"))
    assert [law.factor(x) for x in xs] == [4.0, 4.0, 3.0, 2.0, 1.0, 0.0, 0.0, 4.0]
    assert np.array_equal(VE.factor(VE.of(law), F32([-1.0, 0.5, 2.0, 9.0])), F32([4.0, 3.0, 1.0, 0.0]))
    with pytest.raises(ValueError):
        ViscosityLaw(0, [0.0, 1.0], [1.0])
    with pytest.raises(ValueError):
        ViscosityLaw(0, np.arange(17), np.arange(17))
    e = ViscosityLaw.exponential(1, 0.5, 2.0, 0.0, 1.0)
    assert e.channel == 1 and len(e.values) == 16 and e.values[0] == 0.0 and e.values[-1] == 1.0
    want = np.exp(-2.0 * (np.linspace(0.0, 1.0, 16) - 0.5)).astype(F32)
    assert np.array_equal(F32(e.factors), want) and abs(e.factor(0.5) - 1.0) < 2.5e-3      # (spacing^2 / 8 * f'': 0.0024)
    assert len(ViscosityLaw.exponential(0, 0.0, 1.0, 0.0, 1.0, keys=5).values) == 5
    a = ViscosityLaw.arrhenius(0, 2000.0, 1400.0, 1000.0, 1500.0, keys=8)
    want = np.exp(2000.0 * (1.0 / np.linspace(1000.0, 1500.0, 8) - 1.0 / 1400.0)).astype(F32)
    assert np.array_equal(F32(a.factors), want) and a.factors[0] > 1.0 > a.factors[-1]
    with pytest.raises(ValueError):
        ViscosityLaw.arrhenius(0, 2000.0, 1400.0, 0.0, 1500.0)


# ---- decisions -------------------------------------------------------------------------------------------------
def test_launch_decisions_and_the_order_of_a_step(policy):
    assert [policy.launches(have, n) for have in (0, 1) for n in (0, 100)] == [0, 0, 0, 1]
    # XSPH's, cohesion's and buoyancy's decisions stand as they stood, and so does fuse_integrate
    assert [policy.launches_xsph(have, n) for have in (0, 1) for n in (0, 100)] == [0, 0, 0, 1]
    assert [policy.launches_cohesion(have, n) for have in (0, 1) for n in (0, 100)] == [0, 0, 0, 1]
    cases = [(have, ns, n) for have in (0, 1) for ns in (0, 100) for n in (0, 100)]
    assert [policy.launches_buoyancy(*c) for c in cases] == [0, 0, 0, 0, 0, 0, 0, 1]
    assert policy.fuse7(1, 1, 100, 0, 0, 0, 0) == 1 and policy.fuse7(1, 1, 100, 1, 0, 0, 0) == 0
    text = open(os.path.join(CSRC, "launch.h")).read()
    step = text[text.index("int step_impl("):text.index("// the six phase times")]
    assert (step.index("launch_accel(ctx") < step.index("launch_cohesion(ctx)") < step.index("launch_viscous(ctx)")
            < step.index("launch_xsph(ctx)") < step.index("launch_buoyancy(ctx)") < step.index("launch_integrate(ctx"))
    assert "if (viscous && (rc = launch_viscous(ctx))) return rc;" in step        # nothing launched without it
    flag = "const bool viscous = step_launches_viscous(ctx->have_viscous != 0, ctx->n);"
    assert flag in step and step.index(flag) < step.index("const bool fused =")
    # a viscous step is never fused, whatever else holds: the flag stands in fuse_integrate's switch-off argument; the
    # step keeps the prehash (launch_integrate's hash_too)
    fused = step[step.index("const bool fused ="):step.index("const bool smoothing")]
    assert "ctx->no_fused_integrate != 0 || viscous," in fused
    assert re.search(r"const bool fused = !cohesive &&\s+fuse_integrate\(hash_too,", step)
    assert "loads_pending(ctx), buoyant);" in step
    assert "const bool fuse_now = fused && !smoothing;" in step
    below = step[step.index("const bool fuse_now ="):]
    assert not re.search(r"\bfused\b", below[below.index(";"):])
    assert "launch_integrate(ctx, hash_too)" in step
    # exactly one call site, and the stand-alone phase calls do not apply it
    hip = open(os.path.join(CSRC, "sph_hip.hip")).read()
    assert hip.count("launch_viscous(") == 0 and text.count("launch_viscous(ctx)") == 1
    # both launches, no synchronisation; mu and the law by value
    body = text[text.index("int launch_viscous("):text.index("// ---- xsph")]
    assert body.index("k_viscous_stage") < body.index("k_viscous_apply") and "Synchronize" not in body
    assert "ctx->viscous_mu" in body and "ctx->viscous_law," in body and "ctx->acc" in body
    assert body.count("ctx->velp[ctx->cur]") == 1          # the stage reads it; the pass never does


def test_the_kernels_signatures():
    """const everywhere but R and M for the stage and acc for the apply."""
    mine = open(os.path.join(CSRC, "viscous_kernels.h")).read()
    sig = mine[mine.index("k_viscous_stage(const float4* __restrict__ velp"):]
    sig = sig[:sig.index(")\n{")]
    assert sig.count("const ") == 5 and sig.count("*") == 7
    assert sig.endswith("float4* __restrict__ R, float* __restrict__ M")
    for name in ("velp", "posm", "rho", "meta", "Ts"):
        assert re.search(r"const \w+\* __restrict__ %s\b" % name, sig), name
    assert "float mu, sph_hip_viscosity_law law," in sig                    # by value
    assert "template <bool LAW>\n__global__ void __launch_bounds__(256)\nk_viscous_stage" in mine
    sig = mine[mine.index("k_viscous_apply(const float4* __restrict__ posm"):]
    sig = sig[:sig.index(")\n{")]
    assert sig.count("const ") == 9 and sig.count("*") == 10
    assert sig.endswith("int tiled,\n                float4* __restrict__ acc")
    for name in ("posm", "R", "M", "ncount", "cell_start", "meta", "desc", "nlist", "nlist_overflow"):
        assert re.search(r"const \w+\* __restrict__ %s\b" % name, sig), name
    assert "float mu," in sig and "PairConsts k," in sig and "CellGrid g," in sig                 # by value
    assert ("template <bool UNIT_SCALE, bool WIDE, bool LAW>\n__global__ void __launch_bounds__(TILE_THREADS)\nk_viscous_apply"
            in mine)
    assert mine.count("__shared__") == 1 and "__shared__ TileDesc sd;" in mine
    # the pair kernel reads no velocity but the staged ones, and writes its own acc only
    body = mine[mine.index("k_viscous_apply("):]
    assert "velp" not in body and body.count("acc[") == 2 and "acc[p]" in body and "acc[q]" not in mine
    assert "xcd_workgroup(blockIdx.x, gridDim.x)" in body and "scalar_workgroup_route(" in body and "scalar_lane_route(" in body
    code = "\n".join(line.split("//")[0] for line in mine.splitlines())
    assert "atomic" not in code and "#pragma unroll 1\n   for (int row = 0; row < 9; row++)" in code


# ---- the scenes --------------------------------------------------------------------------------------------------
def test_the_scenes(hiplib):
    from smoothed_particle_hydrodynamics_amd import ViscosityLaw, scenes
    from smoothed_particle_hydrodynamics_amd.scalars import HOLD
    n = 3000
    base = scenes.dam_break_dye(n)
    q, pos, vel, mass, mu = scenes.dam_break_viscous(n, 0.125)
    assert mu == 0.125 and bytes(q) == bytes(base[0])
    for got, want in zip((pos, vel, mass), base[1:4]):
        assert got.tobytes() == want.tobytes() and got.dtype == want.dtype
    assert q.apply_gravity == 1 and q.apply_walls == 1 and (vel.reshape(-1, 3)[:, 0] == F32(0.7)).all()

    p, pos, vel, mass = scenes.shear_layer(n, 0.5, seed=11)
    d = scenes.droplet(n, seed=11)
    assert bytes(p) == bytes(d[0]) and np.array_equal(pos, d[1]) and (mass == 1).all()
    assert p.apply_gravity == 0 and p.apply_walls == 1 and p.central_mass == 0.0
    v, y = vel.reshape(-1, 3), pos.reshape(-1, 3)[:, 1]
    upper = y > F32(0.5) * F32(p.max_y)
    assert vel.dtype == F32 and vel.size == 3 * n and 0.4 * n < upper.sum() < 0.6 * n
    assert (v[upper, 0] == F32(0.5)).all() and not v[~upper].any() and not v[:, 1:].any()
    assert np.array_equal(scenes.shear_layer(n, 0.5, seed=11)[2], vel)
    assert np.array_equal(scenes.shear_layer(n, 0.25, seed=11)[2], F32(0.5) * vel)
    assert not scenes.shear_layer(n, 0.0, seed=11)[2].any()

    q, pos, vel, mass, values, kappa, sources, mu, law = scenes.cooling_flow(n)
    assert bytes(q) == bytes(base[0]) and all(np.array_equal(a, c) for a, c in zip((pos, vel, mass), base[1:4]))
    assert values.shape == (n, 4) and (values[:, 0] == 1).all() and not values[:, 1:].any()
    assert kappa[0] == F32(scenes.scalar_stable_kappa(q)) and not kappa[1:].any()
    assert len(sources) == 1 and sources[0].kind == HOLD and sources[0].channel == 0 and sources[0].value == 0.0
    assert isinstance(law, ViscosityLaw) and law.channel == 0 and len(law.values) == 16
    assert abs(law.factor(1.0) - 1.0) < 1e-6 and abs(law.factor(0.0) / 50.0 - 1.0) < 1e-6       # stiffer where it is cold
    assert all(a > b for a, b in zip(law.factors, law.factors[1:]))
    assert mu > 0 and abs(mu * 50.0 / scenes.viscous_stable_mu(q, 0.25) - 1.0) < 1e-12
    # viscous_stable_mu: dt * (mu / rho) * kernel3 * pi * h^4 / 3 == fraction at the bulk density
    rho = 32.0 * 3.0 / (4.0 * math.pi * float(q.hscaled) ** 3)
    total = float(q.kernel3) * math.pi * float(q.hscaled) ** 4 / 3.0
    assert abs(float(q.time_step) * scenes.viscous_stable_mu(q, 0.25) / rho * total / 0.25 - 1.0) < 1e-9
    # no existing scene function changed its output
    assert all(np.array_equal(a, c) for a, c in zip(base[1:], scenes.dam_break_dye(n)[1:]))
    assert np.array_equal(scenes.droplet(n, seed=11)[1], d[1])


# ---- physics on the restatement ----------------------------------------------------------------------------------
PHYS_FRACTION = 0.1


def advance(p, vel, acc):
    """v + dt * a, fp32: the velocity part of one explicit step with the viscous acceleration alone"""
    return (np.asarray(vel, F32) + F32(p.time_step) * np.asarray(acc, F32)).astype(F32)


def test_the_explicit_range_the_energy_and_the_momentum(layer):
    """mu = viscous_stable_mu(p, 0.1): a tenth of the explicit limit at the bulk density, which leaves the rim of the
    block - where densities fall to a fraction of the bulk's - inside the range too; that is asserted first, on the
    reference state and on the second one.  Inside the range every v' is a convex combination of S_k's velocities, so
    the kinetic energy about the mean velocity falls, twice.  The force addends of a pair negate each other, so what is
    left of sum_i m_i c_i is the rounding of the per-particle sums: under (kmax + 4) * 2^-24 * sum_i |m_i c_i|."""
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass, rho = layer
    mu = float(F32(scenes.viscous_stable_mu(p, PHYS_FRACTION)))
    zero = np.zeros(3 * NB, F32)
    energies = [VE.kinetic_about_mean(vel, mass)]
    v = vel
    for application in range(2):
        acc, on, c, N, info = VE.apply(p, mu, pos, v, mass, rho, zero, with_info=True)
        kmax = int(info["count"].max())
        print("application %d: mu %.6g, max N_i %.4f, median N_i %.4f, touched %d, kmax %d" %
              (application, mu, N.max(), np.median(N), on.sum(), kmax))
        assert N.max() <= 1.0 and N.min() >= 0.0                      # the precondition of every claim below
        assert np.array_equal(acc.reshape(-1, 3)[on], c[on])                    # (nothing was clamped)
        assert kmax > 40 and on.sum() > (300 if application == 0 else 600)
        mc = mass.astype(np.float64)[:, None] * c.astype(np.float64)
        for a in range(3):
            total, scale = math.fsum(mc[:, a]), float(np.abs(mc[:, a]).sum())
            bound = (kmax + 4) * 2.0 ** -24 * scale
            print("  component %d: sum m c %.3e, bound %.3e, sum |m c| %.3e" % (a, total, bound, scale))
            assert abs(total) <= bound
            assert a != 0 or scale > 0
        v = advance(p, v, acc)
        energies.append(VE.kinetic_about_mean(v, mass))
        print("  kinetic energy about the mean: %.9e -> %.9e" % (energies[-2], energies[-1]))
        assert energies[-1] < energies[-2]
    # the layer spreads: particles that were at rest or at full speed now move at speeds in between
    vx = v.reshape(-1, 3)[:, 0]
    assert ((vx > 0) & (vx < F32(SPEED))).sum() > 600 and vx.min() >= 0 and vx.max() <= F32(SPEED)


# ---- sanitizers ------------------------------------------------------------------------------------------------
MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
""" + WALK + r"""
static float uni(unsigned& s) { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f; }

int main()
{
   unsigned seed = 4711u;
   double checksum = 0.0;
   int particles = 0, touched = 0, refused = 0;
   const int counts[6] = {0, 1, 7, 8, 9, 200};
   for (int rep = 0; rep < 600; rep++) {
      const int n = counts[rep % 6];
      std::vector<float> pj(3 * n), Rj(4 * n), Mj(n);      // heap rows of exactly n entries: a walk past them is caught
      const float h = 0.0576f;
      WalkConsts k;
      k.unit = rep % 3 == 0;
      k.sim_scale = rep % 3 == 1 ? 0.5f : 1.0f;
      k.h2 = h * h;
      k.hscaled = (rep % 3 == 2 ? 0.95f * h : h) * k.sim_scale;
      k.kernel3 = 45.0f / (3.14159265f * powf(k.hscaled, 6.0f));
      k.cfl_limit = 100.0f;
      k.cfl_limit2 = k.cfl_limit * k.cfl_limit;
      // a law of 2 .. 16 keys on a channel 0 .. 3; every 29th breaks a rule
      sph_hip_viscosity_law law = {};
      law.channel = rep % 4;
      law.n_keys = 2 + rep % 15;
      for (int q = 0; q < law.n_keys; q++) {
         law.value[q] = (float)q / (float)(law.n_keys - 1) + 0.01f * uni(seed);
         law.factor[q] = 4.0f * uni(seed);
      }
      if (rep % 29 == 0) law.value[1] = law.value[0];
      const int with_law = rep % 2;
      float pi[3] = {0.2f + 0.6f * uni(seed), 0.2f + 0.6f * uni(seed), 0.2f + 0.6f * uni(seed)};
      const float mi = rep % 31 == 0 ? 0.0f : 0.5f + uni(seed);
      float mu = rep % 13 == 0 ? 0.0f : 1.0e-4f * uni(seed);
      if (rep % 17 == 0) mu = __builtin_nanf("");
      if (rep % 19 == 0) mu = -1.0f;
      if (viscous_mu_finite_check(mu) || viscous_mu_sign_check(mu) || viscous_is_off(mu) ||
          (with_law && viscous_law_check(law))) {
         refused++;
         continue;
      }
      const sph_hip_viscosity_law kept = viscous_law_clean(&law);
      const ViscousRow own = viscous_stage(2.0f * uni(seed) - 1.0f, 2.0f * uni(seed) - 1.0f, 2.0f * uni(seed) - 1.0f, mi,
                                           rep % 23 == 0 ? 0.0f : 2.0e4f * (0.5f + uni(seed)));
      const float Ri[4] = {own.x, own.y, own.z, own.w};
      const float Mi = viscous_stage_mu(mu, kept, viscous_channel(kept.channel, uni(seed), uni(seed), uni(seed),
                                                                  1.5f * uni(seed)));
      for (int j = 0; j < n; j++) {
         for (int a = 0; a < 3; a++) pj[3 * j + a] = pi[a] + (2.2f * uni(seed) - 1.1f) * h;
         const ViscousRow r = viscous_stage(2.0f * uni(seed) - 1.0f, 2.0f * uni(seed) - 1.0f, 2.0f * uni(seed) - 1.0f,
                                            0.5f + uni(seed), j % 37 == 5 ? 0.0f : 2.0e4f * (0.5f + uni(seed)));
         Rj[4 * j] = r.x; Rj[4 * j + 1] = r.y; Rj[4 * j + 2] = r.z; Rj[4 * j + 3] = r.w;
         Mj[j] = viscous_stage_mu(mu, kept, 1.4f * uni(seed) - 0.2f);
      }
      if (n > 2 && rep % 7 == 0) pj[3] = __builtin_nanf("");
      if (n > 2 && rep % 11 == 0) Rj[7] = __builtin_inff();
      float acc[3] = {uni(seed), uni(seed), uni(seed)}, c[3];
      touched += walk(&k, mu, with_law, pi, mi, Ri, Mi, n, pj.data(), Rj.data(), Mj.data(), acc, c);
      particles++;
      for (int a = 0; a < 3; a++) checksum += (double)acc[a];
   }
   if (viscous_mode_check(true) || !viscous_mode_check(false) || viscous_slab_check(true) || !viscous_slab_check(false))
      return 4;
   if (viscous_ports_set_check(false) || !viscous_ports_set_check(true) || viscous_ports_check(true, 0, 0) ||
       !viscous_ports_check(true, 1, 0) || viscous_ports_check(false, 1, 1) || viscous_law_scalars_check(3) ||
       !viscous_law_scalars_check(0))
      return 5;
   printf("particles %d refused %d touched %d checksum %.6f\n", particles, refused, touched, checksum);
   return particles > 400 && refused > 50 && touched > 200 && touched < particles ? 0 : 3;
}
"""


def test_new_header_code_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    src, exe = tmp_path / "viscous_main.cpp", tmp_path / "viscous_main"
    src.write_text(MAIN)
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == "", run.stderr
    assert run.stdout.split()[0] == "particles"
