"""GPU: velocity gradients (include/sph_hip.h: velocity gradients).  k_velgrad_particles and k_velgrad_unsort through the
getter, the two samplers and the renderer against the numpy restatement tests/velgrad_emulation.py (with
scalar_emulation's Shepard sums and tint_emulation's frame on top of it), bit for bit; the degenerate neighbourhoods; off
unit scale; nothing a caller can read changes; ports, refusals and empty contexts.  The chunk and route switches are
read at context creation, so each runs in a child process of its own (this file with an output path)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import render_emulation as E
import sample_emulation as SE
import scale_cases
import scene_emulation as SCN
import tint_emulation as TE
import velgrad_emulation as VE
from test_gpu_scalars import N, block_scene

pytestmark = pytest.mark.gpu

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
SWITCHES = ("SPH_HIP_SAMPLE_CHUNK", "SPH_HIP_UNTILED", "SPH_HIP_TILE_CAP", "SPH_HIP_LIST_CAP", "SPH_HIP_TILE_CAP_ACCEL",
            "SPH_HIP_TILE_CAP_DENSITY", "SPH_HIP_CHUNKED")
CHILDREN = {"chunk": {"SPH_HIP_SAMPLE_CHUNK": "256"}, "untiled": {"SPH_HIP_UNTILED": "1"},
            "small tiles": {"SPH_HIP_TILE_CAP": "256"}}
LATTICE = ((-0.02, 0.01, 0.03), (0.05, 0.13, 0.19), (7, 5, 6))      # from inside the block to three planes beyond it
FRAME = (48, 32)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def mode_of(S, name):
    return {"full": S.MODE_FULL, "fast": S.MODE_FULL_FAST}[name]


def block():
    """tests/test_gpu_scalars.py's block: 2 001 seeded particles with seeded velocities - eight workgroups, the last
    with one live lane."""
    p, pos, vel, mass, _, _ = block_scene()
    return p, pos, vel, mass


def rows_of(g):
    """a VelocityGradients of particles as (n, 8) float32"""
    return np.concatenate([g.rotation, g.invariants], 1)


def restated(p, sph, mass):
    """(pos, vel, the restatement's rows (n, 8)) of the context's current state, in particle order"""
    part = sph.getParticles()
    pos, vel = part.mPosition.copy(), part.mVelocity.copy()
    return pos, vel, VE.rows(p, pos, vel, mass)


def assert_rows(got, want, what):
    bad = np.flatnonzero((bits(got) != bits(want)).any(1))
    assert bad.size == 0, "%s: %d of %d rows differ, first %d: %r vs %r" % (what, bad.size, len(want), bad[0], got[bad[0]],
                                                                          want[bad[0]])


def probe_set(p, pos, seed=3):
    """300 seeded points: near particles, on particles, outside the fluid, one NaN, one outside the box"""
    rng = np.random.default_rng(seed)
    xyz = np.asarray(pos, F32).reshape(-1, 3)
    near = xyz[rng.integers(0, len(xyz), 200)] + rng.uniform(-0.5, 0.5, (200, 3)).astype(F32) * F32(p.h)
    probes = np.concatenate([near, xyz[:38], rng.uniform(0.4, 0.9, (60, 3)).astype(F32),
                             np.array([[np.nan, 0.1, 0.1], [-5.0, 0.2, 0.2]], F32)]).astype(F32)
    assert probes.shape == (300, 3)
    return probes


def block_iso(sph, pos):
    """half the median density at every seventh uploaded position (tests/test_gpu_render.py: iso_of)"""
    rho = sph.sampleFields(np.asarray(pos, F32).reshape(-1, 3)[::7], velocity=False)[0]
    return float(F32(0.5) * np.median(rho[rho > 0]))


def camera(p, pos):
    from smoothed_particle_hydrodynamics_amd import Camera
    x = np.asarray(pos, F32).reshape(-1, 3).astype(np.float64)
    c = 0.5 * (x.min(0) + x.max(0))
    box = max(p.max_x, p.max_y, p.max_z)
    return Camera.look_at(c + np.array([0.9, 0.7, 1.6]) * box, c, (0, 1, 0), 40, *FRAME)


# ---- the getter against the restatement --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["full", "fast"])
def test_particles_equal_the_restatement(hiplib, mode):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
        sph.setParticles(pos, vel, mass)
        for steps in (0, 3):
            if steps:
                sph.run(steps)
            pos_k, vel_k, want = restated(p, sph, mass)
            g = sph.getVelocityGradients()
            assert_rows(rows_of(g), want, "%s after %d steps" % (mode, steps))
            valid = want[:, 7] == 1.0
            assert g.valid.dtype == bool and np.array_equal(g.valid, valid) and valid.mean() > 0.95
            assert not rows_of(g)[~valid].any()
            assert (want[valid, 4] > 0).all() and (want[valid, 6] > 0).all()
            assert same(g.vorticity, want[:, 0:3]) and same(g.q, want[:, 5])
            assert g.enstrophy(mass) == 0.5 * float(np.sum(mass.astype(np.float64) * want[:, 6].astype(np.float64) ** 2))
        # after three steps the sorted order is no longer the id order: the rows went through k_velgrad_unsort
        order = VE.PE.canonical_order(p, pos_k)
        assert (order != np.arange(N)).mean() > 0.5
        # a range of rows, and either output alone
        rot = np.zeros((100, 4), F32)
        inv = np.zeros((100, 4), F32)
        sph.call("sph_hip_get_velocity_gradients", 1901, 100, rot.ctypes.data, None)
        sph.call("sph_hip_get_velocity_gradients", 1901, 100, None, inv.ctypes.data)
        assert same(rot, want[1901:, :4]) and same(inv, want[1901:, 4:])


def test_full_and_fast_agree_at_the_uploaded_state(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    out = []
    for mode in ("full", "fast"):
        with S.SPH(N, p, mode=mode_of(S, mode)) as sph:
            sph.setParticles(pos, vel, mass)
            out.append(rows_of(sph.getVelocityGradients()))
    assert same(out[0], out[1]) and (out[0][:, 7] == 1).mean() > 0.95


# ---- degenerate neighbourhoods -----------------------------------------------------------------------------------
def test_degenerate_neighbourhoods_give_zeros_at_exactly_those_ids(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = block()
    h = float(p.h)
    x = pos.reshape(-1, 3)
    assert x[:, 0].max() < 0.3                                  # the block stands at the low end of x: room beyond
    extras = np.array([[0.8, 0.8, 0.8],                                                             # a lone particle
                       [0.6, 0.2, 0.2], [0.6 + 0.3 * h, 0.2, 0.2],                                  # a pair
                       [0.7, 0.5, 0.5], [0.7 + 0.4 * h, 0.5, 0.5], [0.7, 0.5 + 0.3 * h, 0.5],       # a planar patch
                       [0.7 + 0.3 * h, 0.5 + 0.4 * h, 0.5],
                       [0.5, 0.3, 0.7], [0.5, 0.3, 0.7],                                            # a coincident pair
                       [np.nan, 0.4, 0.4]], F32)                                                    # a NaN particle
    rng = np.random.default_rng(8)
    pos2 = np.concatenate([x, extras]).astype(F32).reshape(-1)
    vel2 = np.concatenate([vel.reshape(-1, 3), rng.uniform(-1, 1, extras.shape).astype(F32)]).reshape(-1)
    mass2 = np.ones(N + len(extras), F32)
    want = VE.rows(p, pos2, vel2, mass2)
    assert not want[N:].any() and (want[:N, 7] == 1).all()      # the restatement: zeros at exactly those ids
    with S.SPH(mass2.size, p) as sph:
        sph.setParticles(pos2, vel2, mass2)
        g = sph.getVelocityGradients()
    got = rows_of(g)
    assert_rows(got, want, "block with extras")
    assert not bits(got[N:]).any() and np.array_equal(np.flatnonzero(~g.valid), np.arange(N, N + len(extras)))
    # and the block's own rows are what they are without the extras
    assert same(got[:N], VE.rows(p, pos, vel, mass))


# ---- off unit scale ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", scale_cases.FLAVOURS)
def test_off_unit_scale(hiplib, flavour):
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = scale_cases.block_scene(flavour)
    assert not SE.unit_scale(p)
    with S.SPH(mass.size, p) as sph:
        sph.setParticles(pos, vel, mass)
        sph.step()
        pos_k, vel_k, want = restated(p, sph, mass)
        got = rows_of(sph.getVelocityGradients())
    assert_rows(got, want, flavour)
    valid = want[:, 7] == 1
    assert 0.5 < valid.mean() < 0.99                            # the spray has no fit, the block and the layer have
    if flavour == "SHELL":
        xyz = pos_k.reshape(-1, 3)
        assert scale_cases.zero_term_members(p, pos_k, vel_k, mass, xyz[valid][:512]).sum() > 100


# ---- nothing changes ---------------------------------------------------------------------------------------------
def snapshot(sph):
    part = sph.syncParticles()
    rec = sph.getMonitorRecord()
    return [part.mPosition.copy(), part.mVelocity.copy(), part.mAcceleration.copy(), part.mDensity.copy(),
            part.mNeighborCount.copy(), sph.getScalars(), np.array([sph.get_obstacle_motion()[1]], F32),
            rec.rows.copy().view(np.uint8), rec.steps.copy(), np.array(sph.energy(), F32)]


def observed_context(S, mode):
    """the block with carried scalars, a moving obstacle out of the fluid's way (the motion clock runs) and a monitor
    recording"""
    from smoothed_particle_hydrodynamics_amd.obstacles import Box, Motion
    p, pos, vel, mass, T, kappa = block_scene()
    sph = S.SPH(N, p, mode=mode_of(S, mode))
    sph.setParticles(pos, vel, mass)
    sph.setScalars(T, kappa)
    sph.set_obstacles([Box((0.6, 0.0, 0.3), (0.8, 0.3, 0.6))])
    sph.set_obstacle_motion([Motion((0.01, 0.0, 0.0))])
    sph.recordMonitor(8)
    return sph, p, pos


def the_three_calls(sph, p, pos):
    cam = camera(p, pos)
    return [lambda: sph.getVelocityGradients(),
            lambda: (sph.sampleVelocityGradients(probe_set(p, pos)), sph.sampleVelocityGradientLattice(*LATTICE)),
            lambda: sph.renderVelocityGradients(cam, FRAME[0], FRAME[1], block_iso(sph, pos), "q", (-1.0, 1.0), mode="column",
                                                solids=True)]


@pytest.mark.parametrize("mode", ["full", "fast"])
def test_the_calls_change_nothing(hiplib, mode):
    import smoothed_particle_hydrodynamics_amd as S
    sph, p, pos = observed_context(S, mode)
    with sph:
        sph.run(3)
        before = snapshot(sph)
        assert before[6][0] > 0 and len(before[8]) == 3
        for k, call in enumerate(the_three_calls(sph, p, pos)):
            call()
            for a, b in zip(before, snapshot(sph)):
                assert a.tobytes() == b.tobytes(), "call %d" % k
        sph.run(3)
        got = snapshot(sph)
    twin, _, _ = observed_context(S, mode)
    with twin:
        twin.run(3)
        twin.run(3)
        want = snapshot(twin)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.tobytes() == b.tobytes(), "field %d differs from the twin that never asked" % k
    assert len(want[8]) == 6


# ---- samplers, render, and the switches in child processes -------------------------------------------------------
def observe(sph, p, pos0):
    """what a child process and its parent compare: the getter's rows, both samplers in both groups, one frame"""
    g = sph.getVelocityGradients()
    pts = sph.sampleVelocityGradients(probe_set(p, pos0))
    lat = sph.sampleVelocityGradientLattice(*LATTICE)
    fr = sph.renderVelocityGradients(camera(p, pos0), FRAME[0], FRAME[1], block_iso(sph, pos0), 5, (-4.0, 4.0), mode="column")
    return dict(rows=rows_of(g), p_rot=pts.rotation, p_inv=pts.invariants, p_rho=pts.density, p_cnt=pts.count,
                l_rot=lat.rotation, l_inv=lat.invariants, l_rho=lat.density, l_cnt=lat.count, rgba=fr.rgba,
                scalar=fr.scalar, depth=fr.depth)


def stepped_block(S):
    p, pos, vel, mass = block()
    sph = S.SPH(N, p)
    sph.setParticles(pos, vel, mass)
    sph.run(3)
    return sph, p, pos, mass


def child(out_path):
    import smoothed_particle_hydrodynamics_amd as S
    sph, p, pos, _ = stepped_block(S)
    with sph:
        out = observe(sph, p, pos)
        stats = sph.tile_stats() if not os.environ.get("SPH_HIP_UNTILED") else {}
    np.savez(out_path, capacity_density=stats.get("capacity_density", -1), **out)


@pytest.fixture(scope="module")
def stepped(hiplib):
    """the block after three steps in a context of this process: its state, the restatement's rows, what observe()
    sees - computed once and left unchanged"""
    import smoothed_particle_hydrodynamics_amd as S
    sph, p, pos0, mass = stepped_block(S)
    with sph:
        pos, vel, want = restated(p, sph, mass)
        seen = observe(sph, p, pos0)
    return p, pos0, mass, pos, vel, want, seen


def test_samplers_equal_the_shepard_restatement(stepped):
    p, pos0, mass, pos, vel, want, seen = stepped
    assert_rows(seen["rows"], want, "getter")
    probes = probe_set(p, pos0)
    pts = SE.lattice_points(*LATTICE).reshape(-1, 3)
    for group, name in ((0, "rot"), (1, "inv")):
        chan, rho, cnt = VE.sample(p, pos, vel, mass, want, probes, group)
        assert same(seen["p_" + name], chan) and same(seen["p_rho"], rho) and np.array_equal(seen["p_cnt"], cnt), name
        lchan, lrho, lcnt = VE.sample(p, pos, vel, mass, want, pts, group)
        assert seen["l_" + name].shape == (6, 5, 7, 4)
        assert same(seen["l_" + name].reshape(-1, 4), lchan) and same(seen["l_rho"].reshape(-1), lrho), name
        assert np.array_equal(seen["l_cnt"].reshape(-1), lcnt)
    cnt = seen["p_cnt"]
    assert (cnt == 0).sum() >= 50 and (cnt > 0).sum() >= 200 and not seen["p_rot"][cnt == 0].any()
    assert (seen["l_cnt"] > 0).sum() > 10 and (seen["l_cnt"] == 0).sum() > 50
    assert (seen["depth"] < np.inf).sum() > 50 and seen["scalar"].any()          # the frame shows the block
    # a sampled `valid` is the weighted share of valid members: 1 up to the quotient's rounding inside the block
    share = seen["p_inv"][cnt > 0, 3]
    assert share.max() <= 1.0 + 2.0 ** -20 and np.median(share) > 0.99


@pytest.mark.parametrize("name", list(CHILDREN))
def test_switches_in_a_child_process_give_the_same_bytes(stepped, name, tmp_path):
    seen = stepped[6]
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(CHILDREN[name])
    out_path = str(tmp_path / "child.npz")
    run = subprocess.run([sys.executable, os.path.abspath(__file__), out_path], env=env, capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    got = np.load(out_path)
    for k, v in seen.items():
        assert got[k].shape == v.shape and got[k].tobytes() == v.tobytes(), (name, k)
    if name == "small tiles":
        assert int(got["capacity_density"]) == 256


class Frames:
    """the restatement of the frames of one state: the fluid pass (and the solids over it) once per view, the fluid
    pixels' values once per view, mode and row"""

    def __init__(self, sph, p, pos, vel, mass, rows8, solids=None):
        self.sph = sph
        self.walks = [TE.Walk(p, pos, vel, mass, rows8[:, 0:4]), TE.Walk(p, pos, vel, mass, rows8[:, 4:8])]
        self.fields = E.grid_fields(self.walks[0].grid)
        self.solids = solids
        self.cache = {}

    def want(self, iso, cam, quantity, mode, lo, hi, table, flat_):
        W, H = FRAME
        if "frame" not in self.cache:
            rp = self.sph.renderParams(iso)
            fr = E.render(self.fields[0], cam, rp, W, H, velocity_field=None)
            if self.solids is not None:
                from test_gpu_scene_render import DEFAULT
                fr = SCN.composite(fr, self.solids, cam, rp, DEFAULT, W, H, None, None, False, None)
            self.cache["frame"] = (rp, fr)
        rp, fr = self.cache["frame"]
        k = (mode, quantity >> 2)
        if k not in self.cache:
            self.cache[k] = TE.values(fr, self.walks[quantity >> 2], cam, rp, mode, W, H)
        v = self.cache[k][:, quantity & 3]
        return TE.tint(fr, None, cam, rp, TE.Tint(quantity & 3, mode, lo, hi, TE.FLAT if flat_ else 0), table, W, H, v=v)


@pytest.mark.parametrize("solids", [False, True])
def test_frames_equal_the_tint_restatement(hiplib, solids):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd.obstacles import Box
    from test_gpu_render import iso_of
    from test_gpu_tint import assert_tint, flat, seeded_table
    p, pos0, vel0, mass = block()
    obst = [Box((0.3, 0.0, 0.3), (0.5, 0.3, 0.6))] if solids else None
    ranges = {TE.SURFACE: (-2.0, 3.0), TE.COLUMN: (-0.1, 0.15)}
    table = seeded_table(17)
    with S.SPH(N, p) as sph:
        sph.setParticles(pos0, vel0, mass)
        if solids:
            sph.set_obstacles(obst)
        sph.run(3)
        pos, vel, want8 = restated(p, sph, mass)
        R = Frames(sph, p, pos, vel, mass, want8, obst)
        iso = iso_of(sph, pos.reshape(-1, 3))
        cam = camera(p, pos0)
        tinted = 0
        for mode, mode_name in ((TE.SURFACE, "surface"), (TE.COLUMN, "column")):
            lo, hi = ranges[mode]
            inside = outside = False
            for quantity in (2, 3, 5):
                for flat_ in (False, True):
                    got = sph.renderVelocityGradients(cam, FRAME[0], FRAME[1], iso, quantity, (lo, hi), table, mode_name,
                                                      flat_, solids=solids)
                    want = R.want(iso, cam, quantity, mode, lo, hi, table, flat_)
                    assert_tint(flat(got), want, "%s quantity %d flat=%s solids=%s" % (mode_name, quantity, flat_, solids))
                    hit = want.first_inside >= 0
                    v = want.scalar[hit]
                    inside |= bool(((v > lo) & (v < hi)).any())
                    outside |= bool(((v < lo) | (v > hi)).any())
                    assert (want.scalar[~hit] == 0).all()
            tinted += int(hit.sum())
            assert inside and outside                           # values on the table and clamped to both of its ends
        assert tinted > 100
        if solids:
            assert (got.solid_id >= 0).sum() > 20 and not ((got.solid_id >= 0) & (got.first_inside >= 0)).any()
        # a quantity by name is the quantity by number, and the context carries no scalars
        a = sph.renderVelocityGradients(cam, FRAME[0], FRAME[1], iso, "divergence", ranges[TE.SURFACE], table)
        b = sph.renderVelocityGradients(cam, FRAME[0], FRAME[1], iso, 3, ranges[TE.SURFACE], table)
        assert a.rgba.tobytes() == b.rgba.tobytes() and a.scalar.tobytes() == b.scalar.tobytes()
        with pytest.raises(S.SphHipError, match="the context carries no scalars"):
            sph.renderScalars(cam, FRAME[0], FRAME[1], iso, 0, (0.0, 1.0))


# ---- ports, refusals, empty contexts -----------------------------------------------------------------------------
def test_a_port_context_samples_and_refuses_the_getter(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    from test_gpu_ports import block_scene as port_scene
    p, pos, vel, mass, emitters, sinks = port_scene()
    with S.SPH(mass.size, p, capacity=6000) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setPorts(emitters, sinks)
        sph.run(7)                                              # three layers emitted, some particles caught
        ids, lpos, lvel, _, _, _ = sph.downloadLive()
        o = np.argsort(ids, kind="stable")
        assert len(ids) > mass.size and not np.array_equal(ids[o], np.arange(len(ids)))
        lpos = np.ascontiguousarray(lpos.reshape(-1, 3)[o].reshape(-1))
        lvel = np.ascontiguousarray(lvel.reshape(-1, 3)[o].reshape(-1))
        lmass = np.ones(len(ids), F32)                          # (the emitter's mass is 1 too)
        want8 = VE.rows(p, lpos, lvel, lmass)
        probes = probe_set(p, lpos, seed=9)
        got = sph.sampleVelocityGradients(probes)
        for group, rows in ((0, got.rotation), (1, got.invariants)):
            chan, rho, cnt = VE.sample(p, lpos, lvel, lmass, want8, probes, group)
            assert same(rows, chan) and same(got.density, rho) and np.array_equal(got.count, cnt), group
        assert (got.count > 0).sum() > 150 and got.rotation.any()
        with pytest.raises(S.SphHipError) as e:
            sph.getVelocityGradients()
        assert ("sph_hip_get_velocity_gradients: ports have changed the particle set, the ids are no longer 0..n-1 until "
                "the next upload: use the samplers") in str(e.value)
        # the next upload lifts it
        sph.setPorts()
        sph.setParticles(pos, vel, mass)
        assert sph.getVelocityGradients().valid.any()


def test_refusals_and_empty_contexts(hiplib):
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    from smoothed_particle_hydrodynamics_amd.slab import HipSlab
    p, pos, vel, mass = block()
    buf = np.zeros((16, 4), F32)
    # REF mode
    rp, rpos, rvel, rmass = scenes.dense_block(512)
    with S.SPH(512, rp, mode=S.MODE_REF) as sph:
        sph.setParticles(rpos, rvel, rmass)
        for call in (sph.getVelocityGradients, lambda: sph.sampleVelocityGradients(np.zeros((1, 3), F32)),
                     lambda: sph.sampleVelocityGradientLattice(*LATTICE)):
            with pytest.raises(S.SphHipError, match="FULL and FULL_FAST contexts only"):
                call()
    # a slab context
    with HipSlab(p, 0, p.full_cells_z // 2, 4096, 1024, has_left=False) as slab:
        with pytest.raises(S.SphHipError, match="slab contexts .* have no velocity gradients"):
            slab.call("sph_hip_get_velocity_gradients", 0, 0, None, None)
        with pytest.raises(S.SphHipError, match="slab contexts"):
            slab.call("sph_hip_sample_velocity_gradients_points", 1, buf.ctypes.data, 0, None, None, None)
    with S.SPH(N, p) as sph:
        # nothing resident: empty rows, samples of zero, a background frame
        g = sph.getVelocityGradients()
        assert g.rotation.shape == (0, 4) and g.valid.shape == (0,)
        s = sph.sampleVelocityGradients(probe_set(p, pos))
        assert not s.rotation.any() and not s.invariants.any() and not s.density.any() and not s.count.any()
        lat = sph.sampleVelocityGradientLattice(*LATTICE)
        assert lat.rotation.shape == (6, 5, 7, 4) and not lat.rotation.any() and not lat.count.any()
        fr = sph.renderVelocityGradients(camera(p, pos), FRAME[0], FRAME[1], 1.0, "q", (0.0, 1.0))
        assert (fr.first_inside == -1).all() and not fr.scalar.any()
        sph.setParticles(pos, vel, mass)
        # ranges, groups, quantities
        for first, n in ((0, N + 1), (-1, 4), (N, 1), (5, -1)):
            with pytest.raises(S.SphHipError, match="the range leaves what the context holds"):
                sph.call("sph_hip_get_velocity_gradients", first, n, buf.ctypes.data, None)
        sph.call("sph_hip_get_velocity_gradients", N, 0, None, None)
        for group in (-1, 2):
            with pytest.raises(S.SphHipError, match="group must be 0 or 1"):
                sph.call("sph_hip_sample_velocity_gradients_points", 1, buf.ctypes.data, group, None, None, None)
        with pytest.raises(ValueError):
            sph.renderVelocityGradients(camera(p, pos), FRAME[0], FRAME[1], 1.0, 8, (0.0, 1.0))
        with pytest.raises(ValueError):
            sph.renderVelocityGradients(camera(p, pos), FRAME[0], FRAME[1], 1.0, "vorticity", (0.0, 1.0))
        from smoothed_particle_hydrodynamics_amd.lib import SphTintParams
        import ctypes as C
        tp = SphTintParams(8, 0, 0.0, 1.0, 2, 0)
        with pytest.raises(S.SphHipError, match="quantity must be 0 .. 7"):
            sph.call("sph_hip_render_velocity_gradients", None, None, None, None, 0, C.byref(tp), None, 4, 4, 0, None, None,
                     None, None, None, None, None)
        # after particles were resident and are gone again: empty once more
        sph.setParticles(pos[:0], vel[:0], mass[:0])
        assert sph.getVelocityGradients().rotation.shape == (0, 4)
        assert not sph.sampleVelocityGradients(probe_set(p, pos)).count.any()


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    child(sys.argv[1])
