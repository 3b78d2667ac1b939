"""CPU checks of the ports (include/sph_hip.h: sph_hip_set_ports): the layouts and the binding, every refusal
text of port_check, the firing schedule, lattice points, ids and the sink test of csrc/port_policy.h (compiled
with g++ behind an extern "C" shim) against the numpy restatement tests/port_emulation.py bit for bit, the new
launch decisions next to the unchanged ones, the Python side (ports.py) and the two scenes stepped with the
oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import port_emulation as PE
from helpers import compile_shim, to_oracle_params

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = r"""
#include <stddef.h>
#include "port_policy.h"
#include "launch_policy.h"

extern "C" {
void layout(int* out)
{
   const int v[] = {(int)sizeof(sph_hip_emitter), (int)offsetof(sph_hip_emitter, axis), (int)offsetof(sph_hip_emitter, origin),
                    (int)offsetof(sph_hip_emitter, count), (int)offsetof(sph_hip_emitter, spacing),
                    (int)offsetof(sph_hip_emitter, velocity), (int)offsetof(sph_hip_emitter, mass),
                    (int)offsetof(sph_hip_emitter, first), (int)offsetof(sph_hip_emitter, every),
                    (int)offsetof(sph_hip_emitter, layers), (int)sizeof(sph_hip_sink), (int)offsetof(sph_hip_sink, lo),
                    (int)offsetof(sph_hip_sink, hi), SPH_HIP_MAX_EMITTERS, SPH_HIP_MAX_SINKS, SPH_HIP_MAX_EMITTER_POINTS,
                    SPH_HIP_ABI_VERSION, (int)sizeof(PortFiring)};
   for (unsigned i = 0; i < sizeof(v) / sizeof(v[0]); i++) out[i] = v[i];
}
const char* check(const sph_hip_emitter* e, int ne, const sph_hip_sink* k, int ns, int nx, int ny, int nz, float inv,
                  int z0, int nz_held)
{
   const PortGrid g = {nx, ny, nz, inv, z0, nz_held};
   const char* w = port_check(e, ne, k, ns, g);
   return w ? w : "";
}
int points(const sph_hip_emitter* e, float* xyz)
{
   const int n = port_points(*e);
   for (int k = 0; k < n; k++) port_point(*e, k, xyz[3 * k], xyz[3 * k + 1], xyz[3 * k + 2]);
   return n;
}
// the host's bookkeeping over `steps` port steps: per step and emitter {fired, offset, id_base}, per step m
void schedule(const sph_hip_emitter* e, int ne, int steps, uint32_t next_id, long long* table, int* m_of)
{
   long long fired[SPH_HIP_MAX_EMITTERS] = {0};
   for (int s = 0; s < steps; s++) {
      const PortFiring f = port_plan(e, ne, s, fired, next_id);
      for (int i = 0; i < ne; i++) table[(s * ne + i) * 3] = 0;
      for (int q = 0; q < f.n; q++) {
         long long* row = table + (s * ne + f.emitter[q]) * 3;
         row[0] = 1; row[1] = f.offset[q]; row[2] = f.id_base[q];
         fired[f.emitter[q]]++;
      }
      m_of[s] = f.m;
      next_id += (uint32_t)f.m;
   }
}
int fires(const sph_hip_emitter* e, long long s, long long fired) { return port_fires(*e, s, fired) ? 1 : 0; }
int ids_fit(uint32_t next_id, int m) { return port_ids_fit(next_id, m) ? 1 : 0; }
void first_sink(const sph_hip_sink* k, int ns, const float* xyz, int n, int* out)
{
   for (int i = 0; i < n; i++) out[i] = port_first_sink(k, ns, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
}
int active(int ne, int ns) { return ports_active(ne, ns) ? 1 : 0; }
int no_prehash(int sw, int ne, int ns) { return ports_no_prehash(sw != 0, ne, ns) ? 1 : 0; }
int must_tighten(int bound, int m, int cap) { return ports_must_tighten(bound, m, cap) ? 1 : 0; }
int layer_fits(int live, int m, int cap) { return ports_layer_fits(live, m, cap) ? 1 : 0; }
int fuse(int hash_too, int tiled, int n, int no_fused, int n_obst, int loads)
{
   return fuse_integrate(hash_too != 0, tiled != 0, n, no_fused != 0, n_obst, loads != 0) ? 1 : 0;
}
int moving(int n_obst, int n_moving) { return use_moving_kernels(n_obst, n_moving) ? 1 : 0; }
int bodies(int n_obst, int n_bodies) { return use_body_kernels(n_obst, n_bodies) ? 1 : 0; }
}
"""

GRID = (16, 16, 16, F32(16.0), 0, 16)   # cells of edge 1/16 over the unit cube


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    lib = compile_shim(SHIM, ["-O2", "-ffp-contract=off"], tmp_path_factory)
    V, I, F, L = C.c_void_p, C.c_int, C.c_float, C.c_longlong
    lib.layout.argtypes = [V]
    lib.layout.restype = None
    lib.check.argtypes = [V, I, V, I, I, I, I, F, I, I]
    lib.check.restype = C.c_char_p
    lib.points.argtypes = [V, V]
    lib.schedule.argtypes = [V, I, I, C.c_uint32, V, V]
    lib.schedule.restype = None
    lib.fires.argtypes = [V, L, L]
    lib.ids_fit.argtypes = [C.c_uint32, I]
    lib.first_sink.argtypes = [V, I, V, I, V]
    lib.first_sink.restype = None
    return lib


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def bits(a):
    return np.asarray(a, F32).view(np.uint32)


def P():
    from smoothed_particle_hydrodynamics_amd import ports
    return ports


def emitter(axis=0, origin=(0.5, 0.25, 0.25), count=(4, 3), spacing=0.05, velocity=(1.0, 0.0, 0.0), mass=1.0, first=0,
            every=1, layers=-1):
    return P().Emitter(axis, origin, count, spacing, velocity, mass, first, every, layers)


def check(policy, emitters=(), sinks=(), grid=GRID, ne=None, ns=None):
    ea, n_e = P().as_emitter_array(emitters)
    sa, n_s = P().as_sink_array(sinks)
    return policy.check(ea, n_e if ne is None else ne, sa, n_s if ns is None else ns, *grid).decode()


# ---- layouts and the binding ---------------------------------------------------------------------------------
def test_layouts_and_constants(policy):
    out = (C.c_int * 18)()
    policy.layout(out)
    ports = P()
    assert list(out)[:10] == [56, 0, 4, 16, 24, 28, 40, 44, 48, 52]
    assert list(out)[10:13] == [24, 0, 12]
    assert list(out)[13:17] == [8, 8, 65536, 7]
    assert out[17] == 8 + 3 * 8 * 4
    assert C.sizeof(ports.SphEmitter) == 56 and C.sizeof(ports.SphSink) == 24
    for name, off in (("axis", 0), ("origin", 4), ("count", 16), ("spacing", 24), ("velocity", 28), ("mass", 40),
                      ("first", 44), ("every", 48), ("layers", 52)):
        assert getattr(ports.SphEmitter, name).offset == off
    assert ports.SphSink.lo.offset == 0 and ports.SphSink.hi.offset == 12
    assert (ports.MAX_EMITTERS, ports.MAX_SINKS, ports.MAX_EMITTER_POINTS) == (8, 8, 65536)
    assert (PE.MAX_EMITTERS, PE.MAX_SINKS, PE.MAX_POINTS, PE.DEAD_ID) == (8, 8, 65536, 0xFFFFFFFF)


def test_prototypes_match_the_header(hiplib):
    from smoothed_particle_hydrodynamics_amd import lib as L
    ports = P()
    V, I, Q = C.c_void_p, C.c_int, C.POINTER
    assert L.PROTOTYPES["sph_hip_set_ports"] == (I, [V, Q(ports.SphEmitter), I, Q(ports.SphSink), I])
    assert L.PROTOTYPES["sph_hip_get_ports"] == (I, [V, Q(ports.SphEmitter), Q(ports.SphSink), I, I, V, V,
                                                     Q(C.c_int32), Q(C.c_uint32)])
    assert L.PROTOTYPES["sph_hip_download_live"] == (I, [V, I, Q(C.c_int32), V, V, V, V, V, V])
    text = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    assert re.search(r"#define SPH_HIP_ABI_VERSION 7\b", text) and L.ABI_VERSION == 7
    section = text[text.index("ports: inflow emitters and outflow sinks"):text.index("int sph_hip_download_live(")]
    assert re.search(r"added without a change of\s+SPH_HIP_ABI_VERSION", section.replace("\n *", " "))
    for name in ("set_ports", "get_ports", "download_live"):
        assert hasattr(hiplib, "sph_hip_" + name)
        assert re.search(r"\bint sph_hip_%s\(" % name, text)
    for name, value in (("MAX_EMITTERS", 8), ("MAX_SINKS", 8), ("MAX_EMITTER_POINTS", 65536)):
        assert re.search(r"#define SPH_HIP_%s\s+%d\b" % (name, value), text)
    # a null context is refused without touching the device
    assert hiplib.sph_hip_set_ports(None, None, 0, None, 0) < 0
    assert hiplib.sph_hip_get_ports(None, None, None, 0, 0, None, None, None, None) < 0
    assert hiplib.sph_hip_download_live(None, 0, None, None, None, None, None, None, None) < 0


# ---- port_check ----------------------------------------------------------------------------------------------
def test_port_check_refusals(policy):
    ports = P()
    ok_sink = ports.Sink((0.8, 0.0, 0.0), (1.0, 1.0, 1.0))
    assert check(policy) == ""
    assert check(policy, [emitter()], [ok_sink]) == ""
    assert check(policy, [emitter()] * 8, [ok_sink] * 8) == ""
    assert check(policy, ne=-1) == "negative count" == check(policy, ns=-1)
    assert check(policy, [emitter()] * 9) == "more than SPH_HIP_MAX_EMITTERS emitters"
    assert check(policy, sinks=[ok_sink] * 9) == "more than SPH_HIP_MAX_SINKS sinks"
    assert check(policy, ne=1) == "null emitter list"
    assert check(policy, ns=1) == "null sink list"
    for axis in (-1, 3):
        assert check(policy, [emitter(axis=axis)]) == "axis must be 0, 1 or 2"
    nan, inf = float("nan"), float("inf")
    for bad in (nan, inf, -inf):
        for kw in (dict(origin=(bad, 0.25, 0.25)), dict(origin=(0.5, 0.25, bad)), dict(spacing=bad),
                   dict(velocity=(0.0, bad, 0.0)), dict(mass=bad)):
            assert check(policy, [emitter(**kw)]) == "an emitter field that is not finite", kw
    for s in (0.0, -0.05):
        assert check(policy, [emitter(spacing=s)]) == "spacing must be > 0"
    for c in ((0, 3), (4, 0), (-1, 2)):
        assert check(policy, [emitter(count=c)]) == "count must be >= 1"
    assert check(policy, [emitter(count=(256, 257), spacing=1e-4)]) == "more than SPH_HIP_MAX_EMITTER_POINTS points in one layer"
    assert check(policy, [emitter(count=(65536, 65536), spacing=1e-7)]) == "more than SPH_HIP_MAX_EMITTER_POINTS points in one layer"
    assert check(policy, [emitter(count=(256, 256), spacing=1e-3)]) == ""
    for m in (0.0, -1.0):
        assert check(policy, [emitter(mass=m)]) == "mass must be > 0"
    assert check(policy, [emitter(first=-1)]) == "first must be >= 0"
    for e in (0, -2):
        assert check(policy, [emitter(every=e)]) == "every must be >= 1"
    assert check(policy, [emitter(layers=-2)]) == "layers must be >= -1"
    assert check(policy, [emitter(layers=0)]) == "" == check(policy, [emitter(layers=-1)])
    # corners: the origin itself, the far end of each lattice axis, below zero, the plane outside
    corner = "a lattice corner outside the cell grid"
    assert check(policy, [emitter(origin=(1.0, 0.25, 0.25))]) == corner          # x = 1.0 is cell 16 of 16
    assert check(policy, [emitter(origin=(-1e-6, 0.25, 0.25))]) == corner
    assert check(policy, [emitter(origin=(0.5, 0.9, 0.25), count=(4, 3))]) == corner     # u = y runs past 1
    assert check(policy, [emitter(origin=(0.5, 0.25, 0.95), count=(4, 3))]) == corner    # w = z runs past 1
    assert check(policy, [emitter(origin=(0.5, 0.25, 0.25), count=(4, 3))]) == ""
    assert check(policy, [emitter(axis=1, origin=(0.9, 0.5, 0.25), count=(3, 4))]) == corner   # axis 1: w = x
    assert check(policy, [emitter(axis=1, origin=(0.25, 0.5, 0.85), count=(3, 4))]) == ""      # u = z: 0.85 .. 0.95
    assert check(policy, [emitter(axis=1, origin=(0.25, 0.5, 0.86), count=(4, 3))]) == corner   # ... 1.01
    # a slab's planes: the same emitter outside the planes held
    assert check(policy, [emitter()], grid=(16, 16, 16, F32(16.0), 8, 8)) == corner    # z = 0.25 is plane 4
    assert check(policy, [emitter(origin=(0.5, 0.25, 0.6))], grid=(16, 16, 16, F32(16.0), 8, 8)) == ""
    # the second emitter is checked too
    assert check(policy, [emitter(), emitter(mass=0.0)]) == "mass must be > 0"
    # sinks
    for bad in (nan, inf, -inf):
        assert check(policy, sinks=[ports.Sink((bad, 0, 0), (1, 1, 1))]) == "a sink bound that is not finite"
        assert check(policy, sinks=[ports.Sink((0, 0, 0), (1, bad, 1))]) == "a sink bound that is not finite"
    assert check(policy, sinks=[ports.Sink((0, 0, 0), (1, 0, 1))]) == "a sink needs hi > lo on every axis"
    assert check(policy, sinks=[ports.Sink((0, 0, 2), (1, 1, 1))]) == "a sink needs hi > lo on every axis"
    assert check(policy, sinks=[ok_sink, ports.Sink((0, 0, 0), (0, 1, 1))]) == "a sink needs hi > lo on every axis"
    # a sink may reach outside the grid
    assert check(policy, sinks=[ports.Sink((-5, -5, -5), (5, 5, 5))]) == ""


# ---- lattice points, schedule and ids ------------------------------------------------------------------------
def seeded_emitters():
    rng = np.random.default_rng(20240611)
    out = []
    for count in ((1, 1), (8, 8), (64, 1), (5, 13), (65, 1), (18, 18), (256, 256), (1, 324)):
        for axis in range(3):
            o = rng.random(3).astype(F32) * F32(0.2)
            if count == (8, 8):
                o[(axis + 1) % 3] = F32(-0.0)          # a -0.0f origin along a lattice axis ...
            if count == (5, 13):
                o[axis] = F32(-0.0)                    # ... and on the plane itself
            out.append(emitter(axis, tuple(o), count, float(F32(rng.random() * 0.003 + 0.0005)),
                               tuple(rng.standard_normal(3)), float(rng.random() + 0.5)))
    return out


def test_lattice_points_are_fp32_unfused(policy):
    sizes = set()
    for e in seeded_emitters():
        s = e.to_struct()
        got = np.zeros((e.points, 3), F32)
        assert policy.points(C.byref(s), ptr(got)) == e.points
        want = PE.points_of(PE.of_emitter(e))
        assert np.array_equal(bits(got), bits(want)), e
        sizes.add(e.points)
        # the plane coordinate is the origin's, bit for bit (a -0.0f stays -0.0f)
        assert (bits(got[:, e.axis]) == bits(F32(e.origin[e.axis]))).all()
    assert {1, 64, 65, 324, 65536} <= sizes
    # the axis convention: a = axis, u = (a + 1) % 3 runs fastest, w = (a + 2) % 3
    e = emitter(1, (0.1, 0.2, 0.3), (2, 3), 0.5)
    want = [[0.1 + 0.5 * j, 0.2, 0.3 + 0.5 * i] for j in range(3) for i in range(2)]
    assert np.array_equal(PE.points_of(PE.of_emitter(e)), np.asarray(want, F32))
    # not fused: a product that rounds differently under fma
    e = emitter(0, (0.0, F32(1.0) / F32(3.0), 0.0), (1000, 1), float(F32(0.1) / F32(3.0)))
    got = np.zeros((1000, 3), F32)
    policy.points(C.byref(e.to_struct()), ptr(got))
    i = np.arange(1000, dtype=np.int64)
    fused = (np.float64(F32(1.0) / F32(3.0)) + i.astype(np.float64) * np.float64(F32(e.spacing))).astype(F32)
    assert np.array_equal(bits(got), bits(PE.points_of(PE.of_emitter(e))))
    assert (bits(got[:, 1]) != bits(fused)).any(), "the case is meant to tell an fma from a multiply and an add"


def test_schedule_and_ids(policy):
    steps = 40
    sets = [
        [emitter(count=(18, 18), first=0, every=3, layers=-1), emitter(count=(1, 1), first=5, every=1, layers=4),
         emitter(count=(65, 1), first=39, every=7, layers=1), emitter(count=(8, 8), first=40, every=1, layers=-1),
         emitter(count=(5, 13), first=2, every=11, layers=0), emitter(count=(64, 1), first=1, every=19, layers=3)],
        [emitter(count=(256, 256), spacing=1e-3, first=3, every=20, layers=2)],
        [emitter(first=f, every=e, layers=l) for f, e, l in ((0, 1, -1), (0, 1, 40), (0, 1, 39), (38, 2, -1),
                                                             (7, 8, 5), (7, 8, 4), (1, 39, -1), (0, 40, -1))],
    ]
    for emitters in sets:
        for next_id in (0, 3000, 0x7FFFFFF0):
            ne = len(emitters)
            ea, _ = P().as_emitter_array(emitters)
            table = np.zeros((steps, ne, 3), np.int64)
            m_of = np.zeros(steps, np.int32)
            policy.schedule(ea, ne, steps, next_id, ptr(table), ptr(m_of))
            em = [PE.of_emitter(e) for e in emitters]
            fired, nid = [0] * ne, next_id
            for s in range(steps):
                want, m = PE.plan(em, s, fired, nid)
                assert m == m_of[s]
                rows = {i: (off, base) for i, off, base in want}
                for i in range(ne):
                    assert policy.fires(C.byref(emitters[i].to_struct()), s, fired[i]) == (1 if i in rows else 0)
                    if i in rows:
                        assert tuple(table[s, i]) == (1,) + rows[i], (s, i)
                        fired[i] += 1
                    else:
                        assert table[s, i, 0] == 0
                nid += m
    # the first set by hand: 18 x 18 every third step from 0, the single point in steps 5..8, the late ones
    em = [PE.of_emitter(e) for e in sets[0]]
    fired, seen = [0] * 6, []
    for s in range(steps):
        rows, _ = PE.plan(em, s, fired, 0)
        for i, _, _ in rows:
            fired[i] += 1
        seen.append([i for i, _, _ in rows])
    assert fired == [14, 4, 1, 0, 0, 3]
    assert seen[0] == [0] and seen[5] == [1] and seen[6] == [0, 1] and seen[39] == [0, 2, 5] and seen[20] == [5]
    # ids: list order within a step, point k gets id_base + k
    rows, m = PE.plan(em, 6, [2, 1, 0, 0, 0, 1], 1000)
    assert rows == [(0, 0, 1000), (1, 324, 1324)] and m == 325
    # reaching the dead id is refused
    assert policy.ids_fit(0xFFFFFFFF - 324, 324) == 1 and policy.ids_fit(0xFFFFFFFF - 323, 324) == 0
    assert policy.ids_fit(0, 65536) == 1 and policy.ids_fit(0xFFFFFFFF, 1) == 0 and policy.ids_fit(0xFFFFFFFE, 1) == 1


# ---- sinks ---------------------------------------------------------------------------------------------------
def test_sink_faces_nan_and_overlap(policy):
    ports = P()
    lo, hi = np.asarray((0.25, -0.5, F32(0.1)), F32), np.asarray((0.75, 0.5, F32(0.3)), F32)
    sinks = [ports.Sink(lo, hi), ports.Sink((0.5, 0.0, 0.0), (2.0, 2.0, 2.0))]
    mid = (lo + hi) * F32(0.5)
    pts, want = [], []
    for c in range(3):
        for face, inside_at in ((lo[c], True), (hi[c], False)):
            for value, label in ((face, "on"), (np.nextafter(face, F32(-np.inf)), "below"),
                                 (np.nextafter(face, F32(np.inf)), "above")):
                q = mid.copy()
                q[c] = value
                pts.append(q)
                if face == lo[c]:
                    want.append(label != "below")
                else:
                    want.append(label == "below")
    pts = np.asarray(pts, F32)
    one = [sinks[0]]
    sa, _ = ports.as_sink_array(one)
    got = np.zeros(len(pts), np.int32)
    policy.first_sink(sa, 1, ptr(pts), len(pts), ptr(got))
    assert (got >= 0).tolist() == want
    assert np.array_equal(got, PE.first_sink([PE.of_sink(k) for k in one], pts))
    # NaN in any coordinate is never caught; infinities compare as numbers
    odd = np.asarray([[np.nan, 0.0, 0.2], [0.5, np.nan, 0.2], [0.5, 0.0, np.nan], [np.nan] * 3, [np.inf, 0.0, 0.2],
                      [-np.inf, 0.0, 0.2], mid, [0.6, 0.25, 0.2], [1.5, 1.5, 1.5], [0.3, 0.25, 0.2], [-3, -3, -3]], F32)
    sa, _ = ports.as_sink_array(sinks)
    got = np.zeros(len(odd), np.int32)
    policy.first_sink(sa, 2, ptr(odd), len(odd), ptr(got))
    assert got.tolist() == [-1, -1, -1, -1, -1, -1, 0, 0, 1, 0, -1]      # inside both counts for sink 0
    assert np.array_equal(got, PE.first_sink([PE.of_sink(k) for k in sinks], odd))
    # the other order of the same two sinks: the lowest index still wins
    sa, _ = ports.as_sink_array(sinks[::-1])
    policy.first_sink(sa, 2, ptr(odd), len(odd), ptr(got))
    assert got.tolist() == [-1, -1, -1, -1, -1, -1, 0, 0, 0, 1, -1]
    # seeded points against numpy
    rng = np.random.default_rng(5)
    cloud = (rng.random((4000, 3)) * 3.0 - 1.0).astype(F32)
    got = np.zeros(len(cloud), np.int32)
    policy.first_sink(sa, 2, ptr(cloud), len(cloud), ptr(got))
    assert np.array_equal(got, PE.first_sink([PE.of_sink(k) for k in sinks[::-1]], cloud))
    assert {-1, 0, 1} == set(got.tolist())


# ---- launch decisions ----------------------------------------------------------------------------------------
def test_launch_decisions(policy):
    assert [policy.active(*a) for a in ((0, 0), (1, 0), (0, 1), (8, 8))] == [0, 1, 1, 1]
    # a context with ports never prehashes; without ports the switch alone decides
    assert [policy.no_prehash(*a) for a in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 2, 3))] == [0, 1, 1, 1, 1]
    # the host bound: tighten when bound + m exceeds the capacity, refuse when live + m still does
    assert policy.must_tighten(3000, 324, 3324) == 0 and policy.must_tighten(3001, 324, 3324) == 1
    assert policy.must_tighten(0x7FFFFFFF, 65536, 0x7FFFFFFF) == 1
    assert policy.layer_fits(3000, 324, 3324) == 1 and policy.layer_fits(3001, 324, 3324) == 0
    assert policy.layer_fits(0, 0, 1) == 1 and policy.layer_fits(0x7FFFFFFF, 65536, 0x7FFFFFFF) == 0
    # the unchanged ones: a port context's hash_too = false keeps it off the fused integrate by itself
    assert policy.fuse(1, 1, 100, 0, 0, 0) == 1 and policy.fuse(0, 1, 100, 0, 0, 0) == 0
    assert policy.fuse(1, 0, 100, 0, 0, 0) == 0 and policy.fuse(1, 1, 0, 0, 0, 0) == 0
    assert policy.fuse(1, 1, 100, 1, 0, 0) == 0 and policy.fuse(1, 1, 100, 0, 1, 0) == 0 and policy.fuse(1, 1, 100, 0, 0, 1) == 0
    assert policy.moving(1, 1) == 1 and policy.moving(0, 1) == 0 and policy.moving(1, 0) == 0
    assert policy.bodies(1, 1) == 1 and policy.bodies(0, 1) == 0 and policy.bodies(1, 0) == 0


# ---- Python --------------------------------------------------------------------------------------------------
def test_python_round_trips(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    ports = P()
    e = ports.Emitter(2, (0.1, 0.2, 0.3), (18, 18), 0.0125, (0.0, 0.0, -1.5), 0.75, first=3, every=4, layers=9)
    s = e.to_struct()
    assert (s.axis, tuple(s.count), s.first, s.every, s.layers) == (2, (18, 18), 3, 4, 9)
    assert np.array_equal(bits(list(s.origin)), bits([0.1, 0.2, 0.3])) and bits(s.spacing) == bits(0.0125)
    assert ports.emitter_from_struct(s) == e and e.points == 324
    assert e != ports.Emitter(2, (0.1, 0.2, 0.3), (18, 18), 0.0125, (0.0, 0.0, -1.5), 0.75, first=3, every=4, layers=8)
    assert eval(repr(e), {"Emitter": ports.Emitter}) == e
    d = ports.Emitter(0, (0, 0, 0), (1, 1), 1.0, (0, 0, 0), 1.0)
    assert (d.first, d.every, d.layers) == (0, 1, -1)
    k = ports.Sink((0.0, -1.0, 0.5), (1.0, 2.0, 0.75))
    assert ports.sink_from_struct(k.to_struct()) == k and k != ports.Sink((0.0, -1.0, 0.5), (1.0, 2.0, 0.8))
    assert eval(repr(k), {"Sink": ports.Sink}) == k
    assert ports.as_emitter_array([]) == (None, 0) and ports.as_sink_array(()) == (None, 0)
    arr, n = ports.as_emitter_array([e, s])
    assert n == 2 and ports.emitter_from_struct(arr[0]) == ports.emitter_from_struct(arr[1]) == e
    arr, n = ports.as_sink_array([k, k.to_struct()])
    assert n == 2 and ports.sink_from_struct(arr[1]) == k
    t = ports.PortTotals(np.zeros(1, np.int64), np.zeros(0, np.int64), 5, 6)
    assert t._fields == ("emitted", "removed", "live", "next_id") and t.live == 5
    assert S.Emitter is ports.Emitter and S.Sink is ports.Sink and S.PortTotals is ports.PortTotals
    for name in ("setPorts", "getPorts", "downloadLive"):
        assert callable(getattr(S.SPH, name))
    # slabs refuse ports without asking the device
    from smoothed_particle_hydrodynamics_amd import slab
    for cls in (slab.HipSlab, slab.LocalSlabGroup):
        with pytest.raises(S.SphHipError, match="cannot have ports"):
            cls.set_ports(None, [e], [])
    # the restatement reads the same fields
    assert PE.of_emitter(e) == PE.Emitter(2, e.origin, (18, 18), e.spacing, e.velocity, e.mass, 3, 4, 9)
    assert PE.of_sink(k) == PE.Sink(k.lo, k.hi)


# ---- scenes --------------------------------------------------------------------------------------------------
def run_scene(oracle, scene, steps=20):
    p, pos, vel, mass, emitters, sinks = scene
    run = PE.PortRun(to_oracle_params(p), pos, vel, mass, emitters, sinks)
    for _ in range(steps):
        assert run.step(oracle)
        for a in (run.pos, run.vel, run.rho, run.acc):
            assert np.isfinite(a).all()
        assert (np.diff(run.ids.astype(np.int64)) > 0).all()
    return run


def test_filling_tank_scene(oracle, hiplib, policy):
    from smoothed_particle_hydrodynamics_amd import scenes
    ports = P()
    p, pos, vel, mass, emitters, sinks = scene = scenes.filling_tank(20000, speed=10.0)
    assert pos.size == vel.size == mass.size == 0 and sinks == [] and len(emitters) == 1
    e = emitters[0]
    assert isinstance(e, ports.Emitter) and e.axis == 1 and e.velocity == (0.0, -10.0, 0.0) and e.layers == -1
    assert p.apply_walls == 1 and p.apply_gravity == 1 and p.gravity[1] < 0
    assert e.every == max(1, int(round(e.spacing / (10.0 * p.time_step)))) and e.every <= 9
    assert abs(e.origin[1] - (1.0 - p.h)) < 1e-6                       # under the lid
    grid = (p.full_cells_x, p.full_cells_y, p.full_cells_z, F32(p.full_cell_inv), 0, p.full_cells_z)
    assert check(policy, emitters, sinks, grid) == ""
    pts = PE.points_of(PE.of_emitter(e))
    assert (pts > 0).all() and (pts < 1.0).all() and abs(float(pts[:, 0].mean()) - 0.5) < 1e-3
    run = run_scene(oracle, scene)
    layers = 1 + 19 // e.every
    assert run.layers_emitted == layers >= 2 and run.live == layers * e.points <= 20000
    assert run.emitted.tolist() == [layers * e.points] and run.next_id == run.live
    assert run.pos[:, 1].max() < e.origin[1] and run.vel[:, 1].max() < 0     # everything is on its way down
    # a slower inlet fires less often
    assert scenes.filling_tank(20000, speed=1.0)[4][0].every == int(round(e.spacing / p.time_step)) > e.every


def test_channel_flow_scene(oracle, hiplib, policy):
    from smoothed_particle_hydrodynamics_amd import scenes
    ports = P()
    p, pos, vel, mass, emitters, sinks = scene = scenes.channel_flow(6000, speed=10.0)
    assert mass.size == 6000 and pos.size == vel.size == 18000 and not vel.any()
    e, k = emitters[0], sinks[0]
    assert isinstance(e, ports.Emitter) and isinstance(k, ports.Sink) and len(emitters) == len(sinks) == 1
    assert e.axis == 0 and e.velocity == (10.0, 0.0, 0.0)
    assert e.every == max(1, int(round(e.spacing / (10.0 * p.time_step))))
    grid = (p.full_cells_x, p.full_cells_y, p.full_cells_z, F32(p.full_cell_inv), 0, p.full_cells_z)
    assert check(policy, emitters, sinks, grid) == ""
    # the sink slab is the downstream end over the whole cross-section
    assert abs(k.lo[0] - (2.0 - 2.0 * p.h)) < 1e-6 and k.hi[0] > p.max_x and k.lo[1] < 0 and k.hi[2] > p.max_z
    start_inside = int(PE.caught(PE.of_sink(k), pos).sum())
    assert start_inside > 0
    run = run_scene(oracle, scene)
    assert run.layers_emitted == 1 + 19 // e.every >= 2
    assert run.removed[0] >= start_inside >= 1
    assert run.live == 6000 + run.emitted[0] - run.removed[0]
    assert run.ids[-1] == run.next_id - 1 and run.next_id == 6000 + run.emitted[0]
