"""CPU checks of XSPH velocity smoothing (include/sph_hip.h: xsph): csrc/xsph_policy.h, compiled with g++ behind an
extern "C" shim that walks a particle's candidates the way k_xsph_apply's row walk does, against the numpy
restatement tests/xsph_emulation.py bit for bit; every refusal text; the prototypes and the launch decision beside
the unchanged ones; step_impl's order; the kernels' signatures; the scenes; the physics of the restatement on
scenes.noisy_block - momentum, energy, a uniform velocity; the header's code under the host's sanitizers."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pressure_emulation as PE
import sample_emulation as SE
import scale_cases
import xsph_emulation as XE
from helpers import compile_shim

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smoothed_particle_hydrodynamics_amd", "csrc")

# One particle and its candidates in the order given, every operation of the contract through the header's
# functions: what one lane of the kernel does.  The weight is the density pass's pair term, which only the device
# compiles (pair_math.h: density_term<INSIDE = UNIT_SCALE>); the walk restates it for the host.
WALK = r"""
#include <math.h>

#include "xsph_policy.h"
#include "launch_policy.h"

struct WalkConsts {
   float h2, hscaled, hscaled2, sim_scale, kernel1;
   int unit;
};

static float walk_term(const WalkConsts& k, float m, float d)
{
   float t = (k.hscaled2 - (d * d));
   t = (t * t * t);
   const float w = k.kernel1 * t;
   const float term = (m * w);
   return (k.unit || !(d > k.hscaled)) ? term : 0.0f;
}

// Ri: the particle's own staged row; Rj: the candidates' (4 floats each).  v_out: Ri's velocity, changed in place
// if the particle is touched; dv_out: the change
static int walk(const WalkConsts* k, float eps, const float* pi, const float* Ri, int n, const float* pj, const float* mj,
                const float* Rj, float* v_out, float* dv_out)
{
   const XsphRow ri = {Ri[0], Ri[1], Ri[2], Ri[3]};
   XsphSum s = {0.0f, 0.0f, 0.0f};
   for (int j = 0; j < n; j++) {
      const float dx = pi[0] - pj[3 * j], dy = pi[1] - pj[3 * j + 1], dz = pi[2] - pj[3 * j + 2];
      const float d2 = dx * dx + dy * dy + dz * dz;
      if (!(d2 < k->h2)) continue;
      float d = sqrtf(d2);
      if (!k->unit) d *= k->sim_scale;
      const XsphRow rj = {Rj[4 * j], Rj[4 * j + 1], Rj[4 * j + 2], Rj[4 * j + 3]};
      xsph_pair(s, walk_term(*k, mj[j], d), ri, rj);
   }
   const XsphSum dv = xsph_change(eps, s);
   dv_out[0] = dv.x; dv_out[1] = dv.y; dv_out[2] = dv.z;
   v_out[0] = ri.x; v_out[1] = ri.y; v_out[2] = ri.z;
   if (!xsph_acts(dv)) return 0;
   xsph_apply(dv, v_out[0], v_out[1], v_out[2]);
   return 1;
}
"""

SHIM = WALK + r"""
extern "C" {
int abi() { return SPH_HIP_ABI_VERSION; }
void stage(float vx, float vy, float vz, float rho, float* out)
{
   const XsphRow r = xsph_stage(vx, vy, vz, rho);
   out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
}
int particle(const WalkConsts* k, float eps, const float* pi, const float* Ri, int n, const float* pj, const float* mj,
             const float* Rj, float* v_out, float* dv_out)
{
   return walk(k, eps, pi, Ri, n, pj, mj, Rj, v_out, dv_out);
}
static const char* text(const char* w) { return w ? w : ""; }
const char* eps_check(float eps) { return text(xsph_eps_check(eps)); }
int is_off(float eps) { return xsph_is_off(eps) ? 1 : 0; }
const char* context_check(int full_mode, int whole_grid) { return text(xsph_context_check(full_mode != 0, whole_grid != 0)); }
const char* ports_set_check(int ports_set) { return text(xsph_ports_set_check(ports_set != 0)); }
const char* ports_check(int have, int ne, int ns) { return text(xsph_ports_check(have != 0, ne, ns)); }
// the launch decisions: the new one beside cohesion's and buoyancy's
int launches(int have, int n) { return step_launches_xsph(have != 0, n) ? 1 : 0; }
int launches_cohesion(int have, int n) { return step_launches_cohesion(have != 0, n) ? 1 : 0; }
int launches_buoyancy(int have, int n_scalars, int n) { return step_launches_buoyancy(have != 0, n_scalars, n) ? 1 : 0; }
int fuse7(int hash_too, int tiled, int n, int no_fused, int n_obst, int loads, int between)
{
   return fuse_integrate(hash_too, tiled, n, no_fused, n_obst, loads, between) ? 1 : 0;
}
}
"""


class WalkConsts(C.Structure):
    _fields_ = [("h2", C.c_float), ("hscaled", C.c_float), ("hscaled2", C.c_float), ("sim_scale", C.c_float),
                ("kernel1", C.c_float), ("unit", C.c_int)]


def consts_of(p):
    return WalkConsts(p.h2, p.hscaled, p.hscaled2, p.sim_scale, p.kernel1, 1 if SE.unit_scale(p) else 0)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    lib = compile_shim(SHIM, ["-O2", "-ffp-contract=off"], tmp_path_factory)
    V, I, F = C.c_void_p, C.c_int, C.c_float
    lib.particle.argtypes = [V, F, V, V, I, V, V, V, V, V]
    lib.stage.argtypes = [F, F, F, F, V]
    lib.stage.restype = None
    for name, args in (("eps_check", [F]), ("context_check", [I, I]), ("ports_set_check", [I]), ("ports_check", [I, I, I])):
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = C.c_char_p
    lib.is_off.argtypes = [F]
    return lib


def header_particle(policy, p, eps, pi, Ri, pj, mj, Rj):
    v, dv = np.zeros(3, F32), np.zeros(3, F32)
    k = consts_of(p)
    pj = np.ascontiguousarray(pj, F32).reshape(-1, 3)
    mj = np.ascontiguousarray(mj, F32)
    Rj = np.ascontiguousarray(Rj, F32).reshape(-1, 4)
    touched = policy.particle(C.byref(k), float(eps), ptr(np.ascontiguousarray(pi, F32)), ptr(np.ascontiguousarray(Ri, F32)),
                              mj.size, ptr(pj), ptr(mj), ptr(Rj), ptr(v), ptr(dv))
    return v, bool(touched), dv


# ---- the header against the restatement ----------------------------------------------------------------------
COUNTS = (0, 1, 7, 8, 9, 200)
EPS = 0.5


def params_of(flavour):
    from smoothed_particle_hydrodynamics_amd import scenes
    p, _, _, _ = scenes.dam_break(2001)
    if flavour != "UNIT":
        scale_cases.apply(p, flavour)
    return p


def seeded_particle(rng, p, k):
    """A particle with k candidates within 1.1 h per axis (members and non-members), masses in [0.5, 1.5), velocities
    in [-1, 1)^3 and inverse densities about the inverse of what 32 unit masses give."""
    h = F32(p.h)
    pi = rng.uniform(0.2, 0.8, 3).astype(F32)
    pj = (pi[None, :] + rng.uniform(-1.1, 1.1, (k, 3)).astype(F32) * h).astype(F32)
    mj = rng.uniform(0.5, 1.5, k).astype(F32)
    rinv = F32(1.0) / F32(32.0 * float(p.kernel1) * float(p.hscaled2) ** 3 * 0.2)
    R = np.concatenate([rng.uniform(-1.0, 1.0, (k + 1, 3)), rinv * rng.uniform(0.5, 2.0, (k + 1, 1))], 1).astype(F32)
    return pi, R[0], pj, mj, R[1:]


def same_particle(got, want):
    return (np.array_equal(bits(got[0]), bits(want[0])) and got[1] == want[1] and np.array_equal(bits(got[2]), bits(want[2])))


@pytest.mark.parametrize("flavour", ["UNIT", "SCALED", "SHELL"])
def test_header_equals_the_restatement_bit_for_bit(policy, hiplib, flavour):
    p = params_of(flavour)
    assert SE.unit_scale(p) == (flavour == "UNIT")
    rng = np.random.default_rng(2024)
    members_seen = zero_terms = touched = 0
    for k in COUNTS:
        for row in range(24):
            pi, Ri, pj, mj, Rj = seeded_particle(rng, p, k)
            want = XE.particle(p, EPS, pi, Ri, pj, mj, Rj)
            got = header_particle(policy, p, EPS, pi, Ri, pj, mj, Rj)
            assert same_particle(got, want), (k, row)
            r = pi[None, :] - pj
            d2 = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2]
            member = d2 < F32(p.h2)
            members_seen += int(member.sum())
            zero_terms += int((SE.density_terms(p, d2[member], mj[member]) == 0).sum())
            touched += int(got[1])
            if k == 0:      # no neighbour: nothing changes, dv is +0
                assert not got[1] and np.array_equal(bits(got[0]), bits(Ri[:3])) and not bits(got[2]).any()
            if got[1]:
                assert np.array_equal(bits(got[0]), bits(Ri[:3] + got[2])) and np.isfinite(got[0]).all()
    assert members_seen > 1000 and touched > 60
    # SHELL: members beyond hscaled, whose weight is +0.0f
    assert (zero_terms > 20) == (flavour == "SHELL")


@pytest.mark.parametrize("flavour", ["UNIT", "SCALED", "SHELL"])
def test_a_zero_sum_and_a_nan_inverse_density_store_nothing(policy, hiplib, flavour):
    p = params_of(flavour)
    rng = np.random.default_rng(7)
    pi, Ri, pj, mj, Rj = seeded_particle(rng, p, 9)
    r = pi[None, :] - pj
    inside = np.flatnonzero((r * r).sum(1) < 0.5 * float(p.h2))
    assert inside.size >= 1
    base = header_particle(policy, p, EPS, pi, Ri, pj, mj, Rj)
    assert base[1] and same_particle(base, XE.particle(p, EPS, pi, Ri, pj, mj, Rj))
    # every neighbour moves as the particle does: every addend is g * 0, the sum is zero, nothing is stored -
    # whatever the velocity's own bits are, -0.0f included
    Ru = Rj.copy()
    Ri0 = Ri.copy()
    Ri0[0] = F32(-0.0)
    Ru[:, :3] = Ri0[None, :3]
    for fn in (lambda: header_particle(policy, p, EPS, pi, Ri0, pj, mj, Ru), lambda: XE.particle(p, EPS, pi, Ri0, pj, mj, Ru)):
        v, on, dv = fn()
        assert not on and np.array_equal(bits(v), bits(Ri0[:3])) and bits(v)[0] == 0x80000000
        assert not (bits(dv) & 0x7fffffff).any()
    # a member whose inverse density is NaN (or inf: a neighbour whose density is 0) reaches the sum: dv is not finite
    # and the guard leaves the particle alone
    for bad in (np.nan, np.inf):
        Rb = Rj.copy()
        Rb[inside[0], 3] = bad
        got = header_particle(policy, p, EPS, pi, Ri, pj, mj, Rb)
        assert same_particle(got, XE.particle(p, EPS, pi, Ri, pj, mj, Rb))
        assert not got[1] and not np.isfinite(got[2]).all() and np.array_equal(bits(got[0]), bits(Ri[:3]))
    # ... and so does the particle's own
    Rn = Ri.copy()
    Rn[3] = np.nan
    got = header_particle(policy, p, EPS, pi, Rn, pj, mj, Rj)
    assert not got[1] and np.isnan(got[2]).all() and same_particle(got, XE.particle(p, EPS, pi, Rn, pj, mj, Rj))
    # a candidate with a NaN position is no member
    with_nan = np.insert(pj, 4, [np.nan, pi[1], pi[2]], axis=0)
    got = header_particle(policy, p, EPS, pi, Ri, with_nan, np.insert(mj, 4, 1.0), np.insert(Rj, 4, Rj[0], axis=0))
    assert same_particle(got, base)
    # eps = 0 is off by bits
    for zero in (0.0, -0.0):
        v, on, dv = header_particle(policy, p, zero, pi, Ri, pj, mj, Rj)
        assert not on and np.array_equal(bits(v), bits(Ri[:3])) and not (bits(dv) & 0x7fffffff).any()


def test_the_stage_is_one_correctly_rounded_division(policy):
    rng = np.random.default_rng(3)
    rho = np.concatenate([rng.uniform(1.0, 5.0e4, 200), [0.0, -0.0, np.inf, np.nan, 1e-45, 3e38]]).astype(F32)
    vel = rng.uniform(-2.0, 2.0, (rho.size, 3)).astype(F32)
    vel[0, 0] = F32(-0.0)
    want = XE.stage(vel, rho)
    exact = (1.0 / rho[:200].astype(np.float64)).astype(F32)      # float64 holds the quotient to 53 bits: one rounding
    assert np.array_equal(bits(want[:200, 3]), bits(exact))
    for i in range(rho.size):
        out = np.zeros(4, F32)
        policy.stage(float(vel[i, 0]), float(vel[i, 1]), float(vel[i, 2]), float(rho[i]), ptr(out))
        assert np.array_equal(bits(out), bits(want[i])) or (np.isnan(out[3]) and np.isnan(want[i, 3])), i
    assert np.isinf(want[200, 3]) and want[200, 3] > 0 and want[201, 3] < 0


def test_the_sum_tells_a_fused_multiply_add_from_a_multiply_and_an_add(policy, hiplib):
    """s + g * dv with the product kept exact (float64 holds the product of two float32 exactly; the float64 sum is
    then rounded once to float32, as an FMA rounds) differs from the unfused sum on many seeded particles: a
    translation unit built without -ffp-contract=off on a machine with FMA would fail the comparison above."""
    p = params_of("UNIT")
    rng = np.random.default_rng(2024)
    differ = 0
    for row in range(40):
        pi, Ri, pj, mj, Rj = seeded_particle(rng, p, 9)
        r = (pi[None, :] - pj).astype(F32)
        d2 = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2]
        member = d2 < F32(p.h2)
        g = XE.weights(p, d2[member], mj[member], Ri[3], Rj[member, 3])
        fused = np.zeros(3, F32)
        for gj, rj in zip(g, Rj[member]):
            fused = (fused.astype(np.float64) + np.float64(gj) * (rj[:3] - Ri[:3]).astype(np.float64)).astype(F32)
        _, _, dv = header_particle(policy, p, EPS, pi, Ri, pj, mj, Rj)
        differ += int((bits(XE.change(EPS, fused)) != bits(dv)).any())
    assert differ > 10


# ---- refusals ------------------------------------------------------------------------------------------------
def test_every_refusal_text(policy):
    for ok in (0.0, -0.0, 1.0, 0.5, 1e-45, float(np.nextafter(F32(1.0), F32(0.0)))):
        assert policy.eps_check(ok) == b""
    for bad in (np.nan, np.inf, -np.inf):
        assert policy.eps_check(bad) == b"an eps that is not finite"
    for bad in (-1e-45, -0.5, float(np.nextafter(F32(1.0), F32(2.0))), 2.0, 3e38):
        assert policy.eps_check(bad) == b"an eps outside [0, 1]"
    assert [policy.is_off(e) for e in (0.0, -0.0, 1e-45, 1.0)] == [1, 1, 0, 0]
    assert policy.context_check(1, 1) == b""
    assert policy.context_check(0, 1) == policy.context_check(0, 0) == b"FULL and FULL_FAST contexts only"
    assert policy.context_check(1, 0) == \
        b"slab contexts (with neighbours, or that have exchanged) cannot have velocity smoothing"
    assert policy.ports_set_check(0) == b""
    assert policy.ports_set_check(1) == b"a context with ports cannot have velocity smoothing"
    for have in (0, 1):
        for ne in (0, 2):
            for ns in (0, 3):
                want = b"a context with velocity smoothing cannot have ports" if have and (ne or ns) else b""
                assert policy.ports_check(have, ne, ns) == want


def test_the_host_calls_refuse_in_the_headers_words():
    text = open(os.path.join(CSRC, "sph_hip.hip")).read()
    body = text[text.index("int sph_hip_set_xsph("):text.index("int sph_hip_get_xsph(")]
    for call in ("xsph_eps_check(eps)", "xsph_context_check(", "xsph_ports_set_check("):
        assert re.search(r"if \(const char\* why = %s.*\) return refuse\(ctx, who, why\);" % re.escape(call), body), call
    assert "hipStreamSynchronize" not in body and "hipDeviceSynchronize" not in body      # the setter does not wait
    # switching it off is never refused: the context checks and the allocation stand behind the off test
    off = body.index("if (!xsph_is_off(eps)) {")
    assert body.index("xsph_eps_check(eps)") < off < body.index("xsph_context_check(") < body.index("dev_alloc(rows")
    assert "if (!ctx->xsph_R)" in body          # allocated at the first non-zero setting, once
    ports = text[text.index("int sph_hip_set_ports("):]
    ports = ports[:ports.index("ports_restart(ctx)")]
    assert "xsph_ports_check(ctx->have_xsph != 0, ne, ns)) return refuse(ctx, who, why);" in ports
    upload = text[text.index("static int upload_impl("):text.index("static int all_same_mass(")]
    assert "ctx->have_xsph = 0;" in upload
    # no context allocates the rows at creation: the setter is the only place of this file that names them
    assert text.count("xsph_R") == body.count("xsph_R") > 0


# ---- signatures ------------------------------------------------------------------------------------------------
def test_prototypes_and_abi(policy, hiplib):
    from smoothed_particle_hydrodynamics_amd import lib as L
    assert policy.abi() == 7 and L.ABI_VERSION == 7
    V, I, F, Q = C.c_void_p, C.c_int, C.c_float, C.POINTER
    assert L.PROTOTYPES["sph_hip_set_xsph"] == (I, [V, F])
    assert L.PROTOTYPES["sph_hip_get_xsph"] == (I, [V, Q(F)])
    text = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    assert re.search(r"#define SPH_HIP_ABI_VERSION 7\b", text)
    section = text[text.index("---- xsph"):text.index("int sph_hip_set_xsph(")]
    assert re.search(r"added without a change of\s+SPH_HIP_ABI_VERSION", section.replace("\n *", " "))
    assert "NOT apply the smoothing" in section.replace("\n *", " ").replace("  ", " ")
    assert re.search(r"\bint sph_hip_set_xsph\(sph_hip_context\* ctx, float eps\);", text)
    assert re.search(r"\bint sph_hip_get_xsph\(sph_hip_context\* ctx, float\* eps\);", text)
    for name in ("set_xsph", "get_xsph"):
        assert hasattr(hiplib, "sph_hip_" + name)
    # a null context is refused without touching the device
    assert hiplib.sph_hip_set_xsph(None, 0.5) < 0
    assert hiplib.sph_hip_get_xsph(None, None) < 0
    import smoothed_particle_hydrodynamics_amd as S
    assert callable(S.SPH.setVelocitySmoothing) and callable(S.SPH.getVelocitySmoothing)
    from smoothed_particle_hydrodynamics_amd import build as B
    assert "xsph_kernels.h" in B.HEADERS and "xsph_policy.h" in B.HEADERS


# ---- decisions -------------------------------------------------------------------------------------------------
def test_launch_decisions_and_the_order_of_a_step(policy):
    assert [policy.launches(have, n) for have in (0, 1) for n in (0, 100)] == [0, 0, 0, 1]
    # cohesion's and buoyancy's decisions stand as they stood, and so does fuse_integrate
    assert [policy.launches_cohesion(have, n) for have in (0, 1) for n in (0, 100)] == [0, 0, 0, 1]
    cases = [(have, ns, n) for have in (0, 1) for ns in (0, 100) for n in (0, 100)]
    assert [policy.launches_buoyancy(*c) for c in cases] == [0, 0, 0, 0, 0, 0, 0, 1]
    assert policy.fuse7(1, 1, 100, 0, 0, 0, 0) == 1 and policy.fuse7(1, 1, 100, 0, 0, 0, 1) == 0
    text = open(os.path.join(CSRC, "launch.h")).read()
    step = text[text.index("int step_impl("):text.index("// the six phase times")]
    assert (step.index("launch_accel(ctx") < step.index("launch_cohesion(ctx)") < step.index("launch_xsph(ctx)")
            < step.index("launch_buoyancy(ctx)") < step.index("launch_integrate(ctx"))
    assert "if (smoothing && (rc = launch_xsph(ctx))) return rc;" in step        # nothing launched without it
    assert "const bool smoothing = step_launches_xsph(ctx->have_xsph != 0, ctx->n);" in step
    # a smoothing step is never fused, whatever else holds; it keeps the prehash (launch_integrate's hash_too)
    assert "const bool fuse_now = fused && !smoothing;" in step
    below = step[step.index("const bool fuse_now ="):]
    assert "launch_accel(ctx, 0, nullptr, fuse_now)" in below and "if (fuse_now) fused_step_done(ctx, 1);" in below
    assert not re.search(r"\bfused\b", below[below.index(";"):])
    assert "launch_integrate(ctx, hash_too)" in step
    # exactly one call site, and the stand-alone phase calls do not apply it
    hip = open(os.path.join(CSRC, "sph_hip.hip")).read()
    assert hip.count("launch_xsph(") == 0 and text.count("launch_xsph(ctx)") == 1
    # both launches, no synchronisation
    body = text[text.index("int launch_xsph("):text.index("// ---- step monitor")]
    assert body.index("k_xsph_stage") < body.index("k_xsph_apply") and "Synchronize" not in body
    assert "ctx->xsph_eps" in body and "ctx->velp[ctx->cur]" in body and "ctx->acc" not in body


def test_the_kernels_signatures():
    """const everywhere but R for the stage and velp for the apply; and what the pass reads, the acceleration
    kernels take through pointers to const."""
    mine = open(os.path.join(CSRC, "xsph_kernels.h")).read()
    sig = mine[mine.index("k_xsph_stage(const float4* __restrict__ velp"):]
    sig = sig[:sig.index(")\n{")]
    assert sig.count("const ") == 3 and sig.count("*") == 4 and re.search(r"[^t] float4\* __restrict__ R$", sig)
    assert "__launch_bounds__(256)\nk_xsph_stage" in mine
    sig = mine[mine.index("k_xsph_apply(const float4* __restrict__ posm"):]
    sig = sig[:sig.index(")\n{")]
    assert sig.count("const ") == 8 and sig.count("*") == 9 and sig.endswith("int tiled, float4* __restrict__ velp")
    for name in ("posm", "R", "ncount", "cell_start", "meta", "desc", "nlist", "nlist_overflow"):
        assert re.search(r"const \w+\* __restrict__ %s\b" % name, sig), name
    assert "float eps," in sig and "PairConsts k," in sig                 # by value
    assert "template <bool UNIT_SCALE, bool WIDE>\n__global__ void __launch_bounds__(TILE_THREADS)\nk_xsph_apply" in mine
    assert mine.count("__shared__") == 1 and "__shared__ TileDesc sd;" in mine
    # the pair kernel never reads another particle's velp
    body = mine[mine.index("k_xsph_apply("):]
    assert body.count("velp[") == 2 and "velp[p]" in body and "velp[q]" not in mine
    # (what it gathers for a neighbour is its accumulator's to say: the staged rows, and pair_walk.h adds posm[q])
    pairs = mine[mine.index("struct XsphPairs {"):mine.index("k_xsph_apply(const float4* __restrict__ posm")]
    assert "velp" not in pairs and "{ return R[q]; }" in pairs
    assert "velp" not in open(os.path.join(CSRC, "pair_walk.h")).read().split("#pragma once")[1]
    tiled = open(os.path.join(CSRC, "full_tiled.h")).read()
    sig = tiled[tiled.index("k_full_accel_lists(const float4* __restrict__ posm"):]
    sig = sig[:sig.index(")\n{")]
    for name in ("posm", "rho", "ncount", "desc", "nlist", "nlist_overflow"):
        assert re.search(r"const \w+\* __restrict__ %s\b" % name, sig), name
    plain = open(os.path.join(CSRC, "full_kernels.h")).read()
    sig = plain[plain.index("k_full_accel(const float4* __restrict__ posm"):]
    sig = sig[:sig.index(")\n{")]
    assert "const float* __restrict__ rho" in sig and "const int32_t* __restrict__ ncount" in sig
    coh = open(os.path.join(CSRC, "cohesion_kernels.h")).read()
    assert "velp" not in coh[coh.index("k_cohesion_apply("):]


# ---- the scenes --------------------------------------------------------------------------------------------------
def test_the_scenes(hiplib):
    from smoothed_particle_hydrodynamics_amd import scenes
    n = 3000
    base = scenes.dam_break_dye(n)
    q, pos, vel, mass, eps = scenes.dam_break_smoothed(n)
    assert eps == scenes.XSPH_EPS == 0.5 and scenes.dam_break_smoothed(n, eps=0.25)[4] == 0.25
    assert bytes(q) == bytes(base[0])
    for got, want in zip((pos, vel, mass), base[1:4]):
        assert np.array_equal(got, want)
    assert q.apply_gravity == 1 and q.apply_walls == 1 and (vel.reshape(-1, 3)[:, 0] == F32(0.7)).all()
    coh = scenes.dam_break_cohesive(n, 0.5)
    assert all(np.array_equal(a, c) for a, c in zip((pos, vel, mass), coh[1:4]))

    amp = 0.05
    p, pos, vel, mass = scenes.noisy_block(n, amp, seed=11)
    d = scenes.droplet(n, seed=11)
    assert bytes(p) == bytes(d[0]) and np.array_equal(pos, d[1]) and (mass == 1).all()
    assert p.apply_gravity == 0 and p.apply_walls == 1 and p.central_mass == 0.0
    assert vel.dtype == F32 and vel.size == 3 * n and np.abs(vel).max() < amp and np.abs(vel).max() > 0.9 * amp
    v = vel.reshape(-1, 3).astype(np.float64)
    assert np.abs(v.mean(0)).max() < 4.0 * amp / math.sqrt(3.0 * n)           # mean about zero: four sigma
    assert abs(v.std() / (amp / math.sqrt(3.0)) - 1.0) < 0.05                    # uniform in [-amp, amp)
    again = scenes.noisy_block(n, amp, seed=11)
    assert np.array_equal(again[1], pos) and np.array_equal(again[2], vel)
    other = scenes.noisy_block(n, amp, seed=12)
    assert not np.array_equal(other[1], pos) and not np.array_equal(other[2], vel)
    assert np.array_equal(scenes.noisy_block(n, 2 * amp, seed=11)[1], pos)
    assert not scenes.noisy_block(n, 0.0, seed=11)[2].any()
    # no existing scene function changed its output
    assert all(np.array_equal(a, c) for a, c in zip(base[1:], scenes.dam_break_dye(n)[1:]))
    assert np.array_equal(scenes.droplet(n, seed=11)[1], d[1])


# ---- physics on the restatement ----------------------------------------------------------------------------------
NB, AMP, SEED = 3000, 0.05, 42
PHYS_EPS = 0.5


@pytest.fixture(scope="module")
def noisy(hiplib):
    """noisy_block(3000, 0.05) with the restatement's densities (pressure_emulation.particle_density: the density
    pass's sums) and this restatement's sums, addends and weights."""
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.noisy_block(NB, AMP, SEED)
    rho = PE.particle_density(p, pos, vel, mass)
    assert (rho > 0).all()                       # every particle has a neighbour
    s, info = XE.sums(p, pos, vel, mass, rho, with_info=True)
    return p, pos, vel, mass, rho, s, info


def test_momentum_is_conserved_to_the_sums_own_rounding(noisy):
    """Equal masses: the addend of (i, j) is the bitwise negation of (j, i)'s - the same d2, the same weight, the
    same mean of the inverse densities, the difference negated - so the exact sum of all addends is zero and what is
    left of sum_i dv_i is the rounding of the per-particle sums.  The bound: (kmax + 4) * 2^-24 * T per component, T
    the float64 sum of the absolute addends (times eps, as dv is), kmax the largest member count."""
    p, pos, vel, mass, rho, s, info = noisy
    assert (mass == mass[0]).all()
    terms, probe = info["terms"], info["probe"]
    kmax = int(info["count"].max())
    assert kmax > 40 and terms.shape[0] > 60000
    # the antisymmetry itself
    grid = SE.Grid(p, pos, vel, mass)
    pr, idx, _ = PE.members(grid, grid.pos, exclude_self=True)
    assert np.array_equal(pr, probe)
    key = np.argsort(idx * NB + pr, kind="stable")          # (j, i) in the order of (i, j)
    assert np.array_equal((idx * NB + pr)[key], pr * NB + idx)
    assert np.array_equal(bits(terms) ^ np.uint32(0x80000000), bits(terms[key]))
    for a in range(3):
        assert math.fsum(terms[:, a].astype(np.float64)) == 0.0
    dv = XE.change(PHYS_EPS, s)
    for a in range(3):
        T = PHYS_EPS * float(np.abs(terms[:, a].astype(np.float64)).sum())
        total = math.fsum(dv[:, a].astype(np.float64))
        bound = (kmax + 4) * 2.0 ** -24 * T
        moved = float(np.abs(dv[:, a].astype(np.float64)).sum())
        print("component %d: sum dv %.3e, bound %.3e, sum |dv| %.3e, T %.3e, kmax %d" % (a, total, bound, moved, T, kmax))
        assert T > 0 and moved > 1.0e3 * bound         # the case is not vacuous: the changes are far above the bound
        assert abs(total) <= bound


def test_the_kinetic_energy_about_the_mean_velocity_falls(noisy):
    """eps = 0.5 on the block; the precondition eps * max_i sum_j g_ij <= 1 makes every v' a convex combination of
    S_k's velocities, and then the kinetic energy about the mean velocity must fall strictly."""
    p, pos, vel, mass, rho, s, info = noisy
    worst = PHYS_EPS * float(info["g_sum"].max())
    print("eps * max_i sum_j g_ij = %.4f" % worst)
    assert worst <= 1.0
    new, on, _ = XE.apply(p, PHYS_EPS, pos, vel, mass, rho)
    before, after = XE.kinetic_about_mean(vel, mass), XE.kinetic_about_mean(new, mass)
    print("kinetic energy about the mean: %.6e -> %.6e" % (before, after))
    assert on.sum() > NB - 5 and before > 0
    assert after < before
    # and a second application lowers it again
    third, _, _ = XE.apply(p, PHYS_EPS, pos, new, mass, rho)
    assert XE.kinetic_about_mean(third, mass) < after


def test_a_uniform_velocity_changes_nothing(noisy):
    """Velocities on a 2^-12 lattice and a uniform velocity on the same lattice: every v + u is representable, every
    difference v_j - v_i is exact and the same with and without u, so dv has the same bits.  A uniform field alone
    stores nothing."""
    p, pos, vel, mass, rho, _, _ = noisy
    q = F32(2.0 ** -12)
    v0 = (np.round(vel / q) * q).astype(F32)
    u = np.array([0.5, -0.25, 1.0 + 3.0 * 2.0 ** -12], F32)
    v1 = (v0.reshape(-1, 3) + u[None, :]).astype(F32)
    assert np.array_equal(v1.astype(np.float64), v0.reshape(-1, 3).astype(np.float64) + u.astype(np.float64)[None, :])
    new0, on0, dv0 = XE.apply(p, PHYS_EPS, pos, v0, mass, rho)
    new1, on1, dv1 = XE.apply(p, PHYS_EPS, pos, v1.reshape(-1), mass, rho)
    assert np.array_equal(bits(dv0), bits(dv1)) and np.array_equal(on0, on1) and on0.sum() > NB - 5
    assert not np.array_equal(bits(new0), bits(v0))
    only = np.repeat(u[None, :], NB, 0).reshape(-1)
    new, on, dv = XE.apply(p, PHYS_EPS, pos, only, mass, rho)
    assert not on.any() and np.array_equal(bits(new), bits(only)) and not (bits(dv) & 0x7fffffff).any()


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
      std::vector<float> pj(3 * n), mj(n), Rj(4 * n);      // heap rows of exactly n entries: a walk past them is caught
      const float h = 0.0576f;
      WalkConsts k;
      k.unit = rep % 3 == 0;
      k.sim_scale = rep % 3 == 1 ? 0.5f : 1.0f;
      k.h2 = h * h;
      k.hscaled = (rep % 3 == 2 ? 0.95f * h : h) * k.sim_scale;
      k.hscaled2 = k.hscaled * k.hscaled;
      k.kernel1 = 315.0f / (64.0f * 3.14159265f * powf(k.hscaled, 9.0f));
      float pi[3] = {0.2f + 0.6f * uni(seed), 0.2f + 0.6f * uni(seed), 0.2f + 0.6f * uni(seed)};
      const XsphRow own = xsph_stage(2.0f * uni(seed) - 1.0f, 2.0f * uni(seed) - 1.0f, 2.0f * uni(seed) - 1.0f,
                                     rep % 23 == 0 ? 0.0f : 2.0e4f * (0.5f + uni(seed)));
      const float Ri[4] = {own.x, own.y, own.z, own.w};
      for (int j = 0; j < n; j++) {
         for (int a = 0; a < 3; a++) pj[3 * j + a] = pi[a] + (2.2f * uni(seed) - 1.1f) * h;
         mj[j] = 0.5f + uni(seed);
         const XsphRow r = xsph_stage(2.0f * uni(seed) - 1.0f, 2.0f * uni(seed) - 1.0f, 2.0f * uni(seed) - 1.0f,
                                      2.0e4f * (0.5f + uni(seed)));
         Rj[4 * j] = r.x; Rj[4 * j + 1] = r.y; Rj[4 * j + 2] = r.z; Rj[4 * j + 3] = r.w;
      }
      if (n > 2 && rep % 7 == 0) pj[3] = __builtin_nanf("");
      if (n > 2 && rep % 11 == 0) Rj[7] = __builtin_inff();
      float eps = rep % 13 == 0 ? 0.0f : uni(seed);
      if (rep % 17 == 0) eps = __builtin_nanf("");
      if (rep % 19 == 0) eps = 1.5f;
      if (xsph_eps_check(eps) || xsph_is_off(eps)) {
         refused++;
         continue;
      }
      float v[3], dv[3];
      touched += walk(&k, eps, pi, Ri, n, pj.data(), mj.data(), Rj.data(), v, dv);
      particles++;
      for (int a = 0; a < 3; a++) checksum += (double)v[a];
   }
   if (xsph_context_check(true, true) || !xsph_context_check(false, true) || !xsph_context_check(true, false)) return 4;
   if (xsph_ports_set_check(false) || !xsph_ports_set_check(true) || xsph_ports_check(true, 0, 0) ||
       !xsph_ports_check(true, 1, 0) || xsph_ports_check(false, 1, 1))
      return 5;
   printf("particles %d refused %d touched %d checksum %.6f\n", particles, refused, touched, checksum);
   return particles > 400 && refused > 50 && touched > 200 && touched < particles ? 0 : 3;
}
"""


def test_new_header_code_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    src, exe = tmp_path / "xsph_main.cpp", tmp_path / "xsph_main"
    src.write_text(MAIN)
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == "", run.stderr
    assert run.stdout.split()[0] == "particles"
