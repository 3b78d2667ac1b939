"""GPU: carried scalars (include/sph_hip.h: carried scalars).  k_scalars_stage, k_scalars_step on every route and
the two samplers against the numpy restatement tests/scalar_emulation.py, bit for bit: the restatement is fed with
the state S_k downloaded before a step and the densities downloaded after it.  The routes are set by switches
that are read at context creation, so each runs in a child process of its own (this file with a route name)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import sample_emulation as SE
import scalar_emulation as SC
from test_sample_cpu import forced_chunks, policy  # noqa: F401  (policy: the g++ shim of sample_policy.h)

pytestmark = pytest.mark.gpu

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
N = 2001            # eight workgroups of 256, the last with one live lane

# route name -> (environment, what the tile statistics must show)
ROUTES = {
    "default": {},
    "untiled": {"SPH_HIP_UNTILED": "1"},
    "lists_none": {"SPH_HIP_TILE_CAP": "256"},     # no tile of this scene fits: every workgroup is LISTS_NONE
    "lists_some": {"SPH_HIP_LIST_CAP": "16"},      # most particles have more than 16 neighbours: NLIST_NO_LIST lanes
    "wide": {"SPH_HIP_TILE_CAP": "4096"},          # above 4064: 14-bit tile indices in the entries
}
ROUTE_SWITCHES = ("SPH_HIP_UNTILED", "SPH_HIP_TILE_CAP", "SPH_HIP_LIST_CAP", "SPH_HIP_TILE_CAP_ACCEL",
                  "SPH_HIP_TILE_CAP_DENSITY", "SPH_HIP_CHUNKED", "SPH_HIP_SCALAR_ROWS")


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def block_scene():
    """2 001 seeded particles with seeded velocities, gravity and walls on; four channels with seeded values
    (-0.0f among the carried ones) and the diffusivities (0, k, 2k, k), k a tenth of the bulk's stability limit."""
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dam_break(N, speed=0.3)
    p.apply_gravity = 1
    p.apply_walls = 1
    p.gravity[0], p.gravity[1], p.gravity[2] = 0.0, -9.81, 0.0
    rng = np.random.default_rng(77)
    T = rng.uniform(-1.0, 1.0, (N, 4)).astype(F32)
    T[::7, 0] = F32(-0.0)
    k = scenes.scalar_stable_kappa(p, 0.1)
    kappa = np.array([0.0, k, 2.0 * k, k], F32)
    return p, pos, vel, mass, T, kappa


def block_sources(p):
    """a HOLD over the column's foot, an ADD over its middle, and an ADD on the HOLD's channel behind it"""
    h = float(p.h)
    top = (float(p.max_x) + h, float(p.max_y) + h, float(p.max_z) + h)
    return [SC.hold((-h, -h, -h), (top[0], 0.2, top[2]), 1, 2.5),
            SC.add((-h, 0.3, -h), (top[0], 0.5, 0.5), 2, 40.0),
            SC.add((-h, -h, 0.25), (0.05, 0.1, top[2]), 1, -8.0)]


def api_sources(sources):
    from smoothed_particle_hydrodynamics_amd import ScalarSource
    return [ScalarSource(q.lo, q.hi, q.channel, q.kind, q.value) for q in sources]


def mode_of(S, name):
    return {"full": S.MODE_FULL, "fast": S.MODE_FULL_FAST, "ref": S.MODE_REF}[name]


def checked_steps(sph, p, mass, T, kappa, sources, steps):
    """`steps` single steps, each compared with the restatement fed with the state before it and the densities
    after it; returns the scalars after the last one."""
    for k in range(steps):
        part = sph.getParticles()
        pos_k, vel_k = part.mPosition.copy(), part.mVelocity.copy()
        sph.step()
        rho = sph.getParticles().mDensity.copy()
        got = sph.getScalars()
        want = SC.step(p, pos_k, vel_k, mass, rho, T, kappa, sources)
        assert same(got, want), "step %d: %d rows differ" % (k, int((bits(got) != bits(want)).any(1).sum()))
        T = got
    return T


# ---- single steps against the restatement ----------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["full", "fast"])
def test_single_steps_equal_the_restatement(hiplib, mode):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, T, kappa = block_scene()
    with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setScalars(T, kappa)
        assert same(sph.getScalars(), T)
        out = checked_steps(sph, p, mass, T, kappa, [], 2)
        stats = sph.tileStats()
        assert stats["workgroups"] == 8 and stats["untiled_density"] == 0      # the list route
    assert same(out[:, 0], T[:, 0])                                            # kappa = 0: carried, -0.0f and all
    assert (bits(out[::7, 0]) == 0x80000000).all()
    for ch in (1, 2, 3):
        assert (bits(out[:, ch]) != bits(T[:, ch])).mean() > 0.9               # and the others diffuse


def test_both_arithmetics_give_the_same_scalars(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, T, kappa = block_scene()
    out = []
    for mode in ("full", "fast"):
        with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
            sph.setParticles(pos, vel, mass)
            sph.setScalars(T, kappa)
            sph.step()
            out.append(sph.getScalars())
    assert same(out[0], out[1])


@pytest.mark.parametrize("mode", ["full", "fast"])
def test_queued_steps_equal_single_steps(hiplib, mode):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, T, kappa = block_scene()
    src = api_sources(block_sources(p))
    out = []
    for queued in (True, False):
        with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
            sph.setParticles(pos, vel, mass)
            sph.setScalars(T, kappa)
            sph.setScalarSources(src)
            if queued:
                sph.run(5)
            else:
                for _ in range(5):
                    sph.step()
            part = sph.getParticles()
            out.append((sph.getScalars(), part.mPosition.copy()))
    assert same(out[0][0], out[1][0]) and same(out[0][1], out[1][1])
    assert not same(out[0][0][:, 1:], T[:, 1:])


# ---- routes: one child process per setting -----------------------------------------------------------------------
def route_reference():
    """The restatement's scalars after 1 and after 3 steps of the block with its sources, from states and densities
    downloaded from a context of this process (every route computes the same states)."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, T, kappa = block_scene()
    sources = block_sources(p)
    with S.SPH(N, p) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setScalars(T, kappa)
        sph.setScalarSources(api_sources(sources))
        after1 = checked_steps(sph, p, mass, T, kappa, sources, 1)
        after3 = checked_steps(sph, p, mass, after1, kappa, sources, 2)
        counts = sph.getParticles().mNeighborCount.copy()
    return after1, after3, counts


@pytest.fixture(scope="module")
def reference_scalars(hiplib):
    return route_reference()


def child(route, out_path):
    """One route, FULL and FULL_FAST: the scalars after 1 and 3 steps and the tile statistics, into out_path."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, T, kappa = block_scene()
    src = api_sources(block_sources(p))
    result = {}
    stats = {}
    for mode in ("full", "fast"):
        with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
            sph.setParticles(pos, vel, mass)
            sph.setScalars(T, kappa)
            sph.setScalarSources(src)
            sph.step()
            result[mode + "1"] = sph.getScalars()
            sph.run(2)
            result[mode + "3"] = sph.getScalars()
            result[mode + "_counts"] = sph.getParticles().mNeighborCount.copy()
            stats[mode] = sph.tileStats() if route != "untiled" else {}
    np.savez(out_path, stats=json.dumps(stats), **result)


@pytest.mark.parametrize("route", list(ROUTES))
def test_every_route_gives_the_restatements_bits(reference_scalars, route, tmp_path):
    after1, after3, counts = reference_scalars
    env = {k: v for k, v in os.environ.items() if k not in ROUTE_SWITCHES}
    env.update(ROUTES[route])
    out_path = str(tmp_path / "route.npz")
    run = subprocess.run([sys.executable, os.path.abspath(__file__), route, out_path], env=env, capture_output=True,
                         text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    got = np.load(out_path)
    stats = json.loads(str(got["stats"]))
    for mode in ("full", "fast"):
        assert same(got[mode + "1"], after1) and same(got[mode + "3"], after3), (route, mode)
        assert np.array_equal(got[mode + "_counts"], counts)
        # the setting produced the route it is there for, or the case proves nothing
        st = stats[mode]
        if route == "default":
            assert st["workgroups"] == 8 and st["untiled_density"] == 0 and st["wide_entries"] == 0
            assert counts.max() <= st["list_capacity"]                       # every lane has its list
        elif route == "lists_none":
            # every workgroup with 256 particles gave up its tile (the last one, a single particle, may keep its own)
            assert st["capacity_density"] == 256 and st["largest_tile"] > 256 and st["workgroups"] == 8
            assert st["untiled_density"] >= 7
        elif route == "lists_some":
            assert st["list_capacity"] == 16 and st["untiled_density"] == 0
            # lanes without a list (more neighbours than it holds) beside lanes with one, in every full workgroup
            assert (counts > 16).sum() > 100 and (counts <= 16).sum() > 100
        elif route == "wide":
            assert st["wide_entries"] == 1 and st["capacity_density"] == 4096 and st["untiled_density"] == 0
    if route == "untiled":
        assert "SPH_HIP_UNTILED" in ROUTES[route]        # (an untiled context keeps no tile statistics)


# ---- carry: the id indirection through the re-sorts ---------------------------------------------------------------
def test_a_carried_channel_keeps_its_bits_through_fifty_steps(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass, values, kappa = scenes.dam_break_dyed(4000)
    values[:, 3] = np.arange(4000, dtype=np.float32)        # a channel that names its row
    with S.SPH(4000, p) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setScalars(values, kappa)
        sph.run(50)
        got = sph.getScalars()
        moved = np.abs(sph.getParticles().mPosition - pos).max()
    assert same(got, values)
    assert moved > 0.01, "the column is meant to surge (moved %g)" % moved


# ---- the coupling is one way ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["full", "fast"])
def test_no_particle_changes(hiplib, mode):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, T, kappa = block_scene()
    out = []
    for scalars in (False, True):
        with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
            sph.setParticles(pos, vel, mass)
            if scalars:
                sph.setScalars(T, kappa)
                sph.setScalarSources(api_sources(block_sources(p)))
            sph.run(19)
            sph.step()
            part = sph.getParticles()
            out.append([getattr(part, nm).copy() for nm in ("mPosition", "mVelocity", "mDensity", "mAcceleration",
                                                            "mNeighborCount")] + list(sph.energy()))
    for a, b in zip(*out):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()


# ---- sources --------------------------------------------------------------------------------------------------------
def test_sources_over_five_steps(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, T, kappa = block_scene()
    sources = block_sources(p)
    with S.SPH(N, p) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setScalars(T, kappa)
        sph.setScalarSources(api_sources(sources))
        assert sph.getScalarSources() == api_sources(sources)
        out = checked_steps(sph, p, mass, T, kappa, sources, 5)
        xyz = sph.getParticles().mPosition.reshape(-1, 3)
        # the sources cleared: the next step only diffuses
        sph.setScalarSources([])
        assert sph.getScalarSources() == []
        checked_steps(sph, p, mass, out, kappa, [], 1)
    # well inside the HOLD's box and well outside the ADD's that follows it on the same channel
    held = (xyz[:, 1] < 0.15) & ~((xyz[:, 2] > 0.24) & (xyz[:, 0] < 0.06) & (xyz[:, 1] < 0.11))
    assert held.sum() > 50 and (out[held, 1] == F32(2.5)).all()          # HOLD pins what stays inside
    assert same(out[:, 0], T[:, 0])


# ---- samplers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["full", "fast"])
def test_samplers_equal_the_restatement(hiplib, mode):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, T, kappa = block_scene()
    rng = np.random.default_rng(3)
    xyz = pos.reshape(-1, 3)
    probes = np.concatenate([xyz[rng.integers(0, N, 24)] + rng.uniform(-0.5, 0.5, (24, 3)).astype(F32) * F32(p.h),
                             xyz[:8],                                                      # on particles
                             rng.uniform(0.4, 0.9, (30, 3)).astype(F32),                   # outside the fluid
                             np.array([[np.nan, 0.1, 0.1], [-5.0, 0.2, 0.2]], F32)]).astype(F32)
    assert probes.shape == (64, 3)
    origin, spacing, shape = (-0.02, 0.01, 0.03), (0.05, 0.13, 0.24), (9, 7, 5)
    with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setScalars(T, kappa)
        sph.run(3)
        part = sph.getParticles()
        pos_k, vel_k = part.mPosition.copy(), part.mVelocity.copy()
        T_k = sph.getScalars()
        chan, rho, cnt = sph.sampleScalars(probes)
        lchan, lrho, lcnt = sph.sampleScalarLattice(origin, spacing, shape)
        f_rho, _, f_cnt = sph.sampleFields(probes, velocity=False)
        # the calls change nothing
        assert same(sph.getScalars(), T_k) and same(sph.getParticles().mPosition, pos_k)
    want = SC.sample(p, pos_k, vel_k, mass, T_k, probes)
    assert same(chan, want[0]) and same(rho, want[1]) and np.array_equal(cnt, want[2])
    assert same(rho, f_rho) and np.array_equal(cnt, f_cnt)                    # the sampler's density and count
    empty = cnt == 0
    assert empty.sum() >= 20 and (cnt > 0).sum() >= 30
    assert not chan[empty].any() and not rho[empty].any()
    pts = SE.lattice_points(origin, spacing, shape)
    lwant = SC.sample(p, pos_k, vel_k, mass, T_k, pts.reshape(-1, 3))
    assert lchan.shape == (5, 7, 9, 4)
    assert same(lchan.reshape(-1, 4), lwant[0]) and same(lrho.reshape(-1), lwant[1])
    assert np.array_equal(lcnt.reshape(-1), lwant[2])
    assert (lcnt == 0).sum() > 50 and (lcnt > 0).sum() > 10 and not lchan[lcnt == 0].any()


def test_chunked_samplers_equal_the_unchunked_ones(hiplib, policy, monkeypatch):
    """SPH_HIP_SAMPLE_CHUNK: the lattice in single bricks (cut along x, y and z: the strided copy-out of 16-byte
    elements), the points in three chunks, the last one ragged - every bit as from the one chunk these calls
    take otherwise"""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass, T, kappa = block_scene()
    xyz = pos.reshape(-1, 3)
    h = F32(p.h)
    spacing = (float(h / F32(2)),) * 3
    origin = tuple(float(c) for c in xyz.min(0) - h)          # from outside the column into it
    shape = (19, 21, 11)
    cut_x = forced_chunks(policy, shape, [spacing[0] * float(F32(p.full_cell_inv))] * 3)[2]
    rng = np.random.default_rng(5)
    probes = np.concatenate([xyz[rng.integers(0, N, 500)] + rng.uniform(-0.5, 0.5, (500, 3)).astype(F32) * h,
                             rng.uniform(0.4, 0.9, (98, 3)).astype(F32),
                             np.array([[np.nan, 0.1, 0.1], [-5.0, 0.2, 0.2]], F32)]).astype(F32)
    assert len(probes) == 600                                 # chunks of 256, 256 and 88 probes

    def sampled(forced):
        monkeypatch.delenv("SPH_HIP_SAMPLE_CHUNK", raising=False)
        if forced:
            monkeypatch.setenv("SPH_HIP_SAMPLE_CHUNK", str(forced))
        with S.SPH(N, p, mode=S.MODE_FULL) as sph:      # (the switch is read when the context is created)
            sph.setParticles(pos, vel, mass)
            sph.setScalars(T, kappa)
            sph.run(3)
            return sph.sampleScalarLattice(origin, spacing, shape), sph.sampleScalars(probes)

    whole_lattice, whole_points = sampled(None)
    assert (whole_lattice[2] > 0).sum() > 100 and (whole_lattice[2] == 0).sum() > 100 and whole_lattice[0].any()
    assert (whole_points[2] > 0).sum() > 400 and (whole_points[2] == 0).sum() > 50
    lattice, _ = sampled(cut_x)
    _, points = sampled(256)
    for got, whole, what in ((lattice, whole_lattice, "lattice in chunks of %d" % cut_x), (points, whole_points, "points in chunks of 256")):
        assert same(got[0], whole[0]) and same(got[1], whole[1]) and np.array_equal(got[2], whole[2]), what


# ---- refusals on the device ------------------------------------------------------------------------------------------
def test_refusals(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import ScalarSource, scenes
    from smoothed_particle_hydrodynamics_amd.ports import Sink
    from smoothed_particle_hydrodynamics_amd.slab import HipSlab
    p, pos, vel, mass, T, kappa = block_scene()

    def refused(call, *args, text):
        with pytest.raises(S.SphHipError) as e:
            call(*args)
        assert text in str(e.value), str(e.value)

    # REF mode
    rp, rpos, rvel, rmass = scenes.dense_block(512)
    with S.SPH(512, rp, mode=S.MODE_REF) as sph:
        sph.setParticles(rpos, rvel, rmass)
        refused(sph.setScalars, np.zeros(512), 0.0, text="FULL and FULL_FAST contexts only")
    # a slab context
    with HipSlab(p, 0, p.full_cells_z // 2, 4096, 1024, has_left=False) as slab:
        v = np.zeros((16, 4), F32)
        k = np.zeros(4, F32)
        with pytest.raises(S.SphHipError, match="slab contexts"):
            slab.call("sph_hip_set_scalars", 16, v.ctypes.data, k.ctypes.data)
        with pytest.raises(S.SphHipError, match="slab contexts"):
            slab.call("sph_hip_sample_scalars_points", 1, v.ctypes.data, None, None, None)
    with S.SPH(N, p) as sph:
        sph.setParticles(pos, vel, mass)
        # nothing set yet
        refused(sph.getScalars, text="the context carries no scalars")
        refused(sph.setScalarSources, [ScalarSource.hold((0, 0, 0), (1, 1, 1), 0, 1.0)], text="the context carries no scalars")
        refused(sph.sampleScalars, np.zeros((1, 3), F32), text="the context carries no scalars")
        # a wrong n, bad values
        refused(sph.setScalars, T[:-1], kappa, text="n must equal the particle count")
        bad = T.copy()
        bad[5, 2] = np.inf
        refused(sph.setScalars, bad, kappa, text="a value that is not finite")
        refused(sph.setScalars, T, [0.0, -1.0, 0.0, 0.0], text="a diffusivity that is not finite and >= 0")
        # ports both ways
        sink = Sink((0.9, 0.9, 0.9), (1.0, 1.0, 1.0))
        sph.setPorts([], [sink])
        refused(sph.setScalars, T, kappa, text="a context with ports cannot carry scalars")
        sph.setPorts([], [])
        sph.setScalars(T, kappa)
        refused(sph.setPorts, [], [sink], text="a context that carries scalars cannot have ports")
        sph.setPorts([], [])                                   # (clearing ports is no port)
        # a refused call keeps what is set
        refused(sph.setScalars, T[:5], kappa, text="n must equal the particle count")
        refused(sph.setScalarSources, [ScalarSource((0, 0, 0), (1, 1, 1), 4, 0, 1.0)], text="channel must be 0 .. 3")
        refused(sph.setScalarSources, [ScalarSource.hold((0, 0, 0), (1, 0, 1), 0, 1.0)] * 2, text="lo must be < hi")
        refused(sph.setScalarSources, [ScalarSource.hold((0, 0, 0), (1, 1, 1), 0, 1.0)] * 9,
                text="more than SPH_HIP_MAX_SCALAR_SOURCES sources")
        assert same(sph.getScalars(), T) and sph.getScalarSources() == []
        # switched off
        sph.setScalars(None)
        refused(sph.getScalars, text="the context carries no scalars")


def test_an_upload_drops_the_scalars_and_the_sources(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import ScalarSource
    p, pos, vel, mass, T, kappa = block_scene()
    with S.SPH(N, p) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setScalars(T, kappa)
        sph.setScalarSources([ScalarSource.hold((0, 0, 0), (1, 1, 1), 0, 1.0)])
        sph.step()
        sph.setParticles(pos, vel, mass)
        with pytest.raises(S.SphHipError) as e:
            sph.getScalars()
        assert "the context carries no scalars" in str(e.value)
        assert sph.getScalarSources() == []
        sph.step()                                              # and a step launches nothing for them
        sph.setScalars(T[:, :2], kappa[:2])                     # set again: two channels, padded
        got = sph.getScalars()
        assert same(got[:, :2], T[:, :2]) and not got[:, 2:].any()


# ---- the other features beside scalars -------------------------------------------------------------------------------
def test_other_features_read_what_they_read_without_scalars(hiplib):
    """Tracers, gauges (a pressure kind among them), an obstacle on a motion path and a load recording, one short
    run each without and with scalars: the same bits."""
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass, T, kappa = block_scene()
    dt = float(p.time_step)
    tracers = scenes.tracer_lattice((0.01, 0.05, 0.1), (0.09, 0.7, 0.9), 0.04)
    gauges = [S.PointGauge((0.05, 0.3, 0.5)), S.ColumnGauge((0.05, 0.0, 0.5), 1, 0.5 * float(p.h), 40, 1000.0),
              S.PressureGauge((0.05, 0.1, 0.5))]
    obst = [O.Box((0.02, 0.0, 0.3), (0.06, 0.2, 0.6))]
    paths = [O.MotionPath.sine((0.0, 0.02, 0.03), 8.0 * dt, 16)]
    out = []
    for scalars in (False, True):
        got = []

        def start(sph):
            sph.setParticles(pos, vel, mass)
            if scalars:
                sph.setScalars(T, kappa)
                sph.setScalarSources(api_sources(block_sources(p)))

        with S.SPH(N, p) as sph:
            start(sph)
            sph.setTracers(tracers)
            sph.run(6)
            tr = sph.getTracers()
            got += [tr.position, tr.wet_steps, tr.dry_steps]
        with S.SPH(N, p) as sph:
            start(sph)
            sph.setGauges(gauges)
            sph.recordGauges(4, 2)
            sph.run(6)
            rec = sph.getGaugeRecord()
            got += [rec.v, rec.n, rec.k]
        with S.SPH(N, p) as sph:
            start(sph)
            sph.setObstacles(obst)
            sph.setObstaclePaths(paths)
            sph.recordLoads(6)
            sph.run(6)
            loads = sph.getLoads()
            got += [loads.impulse_q, loads.count, loads.skipped, sph.getParticles().mPosition.copy()]
            if scalars:
                assert not same(sph.getScalars()[:, 1:], T[:, 1:])       # (the scalars did run beside them)
        out.append(got)
    assert len(out[0]) == 10
    for a, b in zip(*out):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    assert out[0][1].sum() > 0 and np.abs(out[0][3]).sum() > 0 and out[0][7].sum() > 0     # wet tracers, readings, loads


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    child(sys.argv[1], sys.argv[2])
