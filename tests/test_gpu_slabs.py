"""GPU: the slab-decomposed FULL-mode step (what runs one-slab-per-GPU over RCCL) against the
single-context step and the oracle.  All slabs live on the one GPU of the test box and hand
their messages over by pointer (LocalSlabGroup) — kernels, message format and ghost/migrant
protocol are exactly those of the distributed run; only the transport differs (that part is
covered under gloo in test_slab_cpu.py).  Bar: bit-identical per-particle results for any
number of slabs."""
import os

import numpy as np
import pytest

from helpers import to_oracle_params

pytestmark = pytest.mark.gpu


def build_group(S, p, pos, vel, mass, world, overlap=False):
    from smoothed_particle_hydrodynamics_amd import slab as SL
    z = pos.reshape(-1, 3)[:, 2]
    cuts = SL.plan_cuts(p, z, world)
    hist = np.bincount(SL.plane_of(p, z), minlength=p.full_cells_z)
    uniform = bool((mass == mass[0]).all())
    import torch
    stream = torch.cuda.Stream()     # slabs of one process share one stream
    slabs = []
    for r in range(world):
        cap, msg = SL.slab_capacities(hist, cuts, r, slack=2.0)
        s = SL.HipSlab(p, cuts[r], cuts[r + 1], cap, msg, device=0, has_left=r > 0,
                       has_right=r + 1 < world, stream=stream)
        s.upload(*SL.split_scene(p, cuts, r, pos, vel, mass), all_masses_equal=uniform)
        slabs.append(s)
    two = overlap == "two-streams"
    return SL.LocalSlabGroup(slabs, overlap=bool(overlap),
                             exchange_stream=torch.cuda.Stream(priority=-1) if two else None), cuts


def moving_block(n=30000, speed=40.0, unequal=True):
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dense_block(n, lo=(1.0, 1.0, 1.0), hi=(2.2, 2.2, 2.8), speed=speed)
    if unequal:
        mass = (0.5 + scenes.uniform01(11, np.arange(n))).astype(np.float32)
    return p, pos, vel, mass


@pytest.mark.parametrize("overlap", [False, True, "two-streams"],
                         ids=["serial", "early-exchange", "early-exchange-2-streams"])
@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_slabs_equal_single_context_and_oracle(oracle, hiplib, world, overlap):
    """overlap=True: the messages are packed before the interior's acceleration and the integrate
    (sph_hip_slab_step_begin / _end) - what the distributed run overlaps with the transfer."""
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = moving_block()
    steps = 5
    group, cuts = build_group(S, p, pos, vel, mass, world, overlap)
    owned0 = [s.status()["owned"] for s in group.slabs]
    for _ in range(steps):
        group.step()
    got = group.gather(mass.size)
    assert (got["owner"] >= 0).all()
    for s in group.slabs:
        assert s.status()["errors"] == 0

    opos, ovel = pos.copy(), vel.copy()
    for _ in range(steps):
        ref = oracle.step(to_oracle_params(p), opos, ovel, mass, mode="full")
    assert np.array_equal(got["ncount"], ref["ncount"])
    assert np.array_equal(got["rho"], ref["rho"])
    assert np.array_equal(got["acc"], ref["acc"])
    assert np.array_equal(got["pos"], opos)
    assert np.array_equal(got["vel"], ovel)

    with S.SPH(mass.size, p) as one:
        one.setParticles(pos, vel, mass)
        one.run(steps)
        part = one.getParticles()
        assert np.array_equal(got["acc"], part.mAcceleration)
        assert np.array_equal(got["pos"], part.mPosition)

    if world > 1:
        owned1 = [s.status()["owned"] for s in group.slabs]
        assert sum(owned1) == mass.size
        assert owned0 != owned1, "the scene is meant to migrate particles across the cuts"
    for s in group.slabs:
        s.close()


@pytest.mark.parametrize("overlap", [False, True, "two-streams"],
                         ids=["serial", "early-exchange", "early-exchange-2-streams"])
def test_slabs_dam_break_uniform_mass_two_slabs(oracle, hiplib, overlap):
    """the benchmark scene (uniform masses -> fast path), 2 slabs, 3 steps"""
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dam_break(120000)
    group, cuts = build_group(S, p, pos, vel, mass, 2, overlap)
    for _ in range(3):
        group.step()
    got = group.gather(mass.size)
    opos, ovel = pos.copy(), vel.copy()
    for _ in range(3):
        ref = oracle.step(to_oracle_params(p), opos, ovel, mass, mode="full")
    for k, want in (("ncount", ref["ncount"]), ("rho", ref["rho"]), ("acc", ref["acc"]),
                    ("pos", opos), ("vel", ovel)):
        assert np.array_equal(got[k], want), k
    for s in group.slabs:
        assert s.status()["errors"] == 0
        s.close()


@pytest.mark.parametrize("fused", [True, False], ids=["fused-slab-step", "separate-kernels"])
@pytest.mark.parametrize("world", [2, 3])
def test_slabs_in_tolerance_mode_equal_the_single_context_bit_for_bit(hiplib, monkeypatch, world, fused):
    """SPH_HIP_ARITH_FAST on slab contexts (sph_hip_set_arithmetic): every fused operation is
    written out, so the slabs' results - ghost densities recomputed locally included - are the
    single FAST context's bits, with migration, early exchange on two streams, with the two parts
    of the acceleration launch doing the rest of the step and with the separate kernels
    (SPH_HIP_NO_FUSED_SLAB=1); unequal masses, moving block."""
    import smoothed_particle_hydrodynamics_amd as S
    if fused:
        monkeypatch.delenv("SPH_HIP_NO_FUSED_SLAB", raising=False)
    else:
        monkeypatch.setenv("SPH_HIP_NO_FUSED_SLAB", "1")
    p, pos, vel, mass = moving_block()
    steps = 5
    group, cuts = build_group(S, p, pos, vel, mass, world, "two-streams")
    for s in group.slabs:
        s.set_arithmetic(S.ARITH_FAST)
    owned0 = [s.status()["owned"] for s in group.slabs]
    for _ in range(steps):
        group.step()
    got = group.gather(mass.size)
    for s in group.slabs:
        assert s.status()["errors"] == 0
    with S.SPH(mass.size, p, mode=S.MODE_FULL_FAST) as one:
        one.setParticles(pos, vel, mass)
        one.run(steps)
        part = one.getParticles()
        for k, want in (("ncount", part.mNeighborCount), ("rho", part.mDensity), ("acc", part.mAcceleration),
                        ("pos", part.mPosition), ("vel", part.mVelocity)):
            assert np.array_equal(got[k], want), k
    assert owned0 != [s.status()["owned"] for s in group.slabs]
    for s in group.slabs:
        s.close()


def test_records_leave_and_enter_a_slab_on_the_device(hiplib):
    """sph_hip_slab_export_records / _upload_records: the owned particles as message records in
    device memory and back into a fresh slab - what rebalance() moves between ranks.  The second
    slab steps to the same bits as the first."""
    import torch
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import slab as SL
    p, pos, vel, mass = moving_block(20000)
    a = SL.HipSlab(p, 0, p.full_cells_z, 30000, 64, device=0, has_left=False, has_right=False)
    a.upload(np.arange(mass.size, dtype=np.uint32), pos, vel, mass, all_masses_equal=False)
    a.step()
    rec = a.export_records()
    assert rec.shape == (mass.size, 8) and rec.is_cuda
    ids = rec[:, 7].contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
    assert sorted(ids.cpu().tolist()) == list(range(mass.size))
    rows = rec[torch.argsort(ids, stable=True)].contiguous()
    da = a.download()
    order = np.argsort(da["ids"], kind="stable")
    assert np.array_equal(rows[:, 0:3].cpu().numpy(), da["pos"].reshape(-1, 3)[order])
    assert np.array_equal(rows[:, 3].cpu().numpy(), mass)
    b = SL.HipSlab(p, 0, p.full_cells_z, 30000, 64, device=0, has_left=False, has_right=False)
    b.upload_records(rows, all_masses_equal=False)
    a.step()
    b.step()
    da, db = a.download(), b.download()
    oa, ob = np.argsort(da["ids"], kind="stable"), np.argsort(db["ids"], kind="stable")
    for k in ("pos", "vel", "acc"):
        assert np.array_equal(da[k].reshape(-1, 3)[oa], db[k].reshape(-1, 3)[ob]), k
    for k in ("rho", "ncount"):
        assert np.array_equal(da[k][oa], db[k][ob]), k
    a.close()
    b.close()


def test_message_overflow_is_reported(hiplib):
    """a message buffer that is too small sets error bit 2 instead of corrupting memory"""
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import slab as SL
    p, pos, vel, mass = moving_block(20000, unequal=False)
    cuts = SL.plan_cuts(p, pos.reshape(-1, 3)[:, 2], 2)
    import torch
    stream = torch.cuda.Stream()
    slabs = []
    for r in range(2):
        s = SL.HipSlab(p, cuts[r], cuts[r + 1], 60000, 16, device=0, has_left=r > 0, has_right=r < 1,
                       stream=stream)
        s.upload(*SL.split_scene(p, cuts, r, pos, vel, mass), all_masses_equal=True)
        slabs.append(s)
    SL.LocalSlabGroup(slabs).step()
    assert any(s.status()["errors"] & 2 for s in slabs)
    for s in slabs:
        s.close()


def test_a_run_that_loses_particles_stops_loudly(hiplib):
    """Nobody has to ask: the stepping loop looks at the error bits every 16 steps without
    synchronising (sph_hip_slab_poll_errors) and raises within 32 steps of the overflow;
    waiting for the slab (sph_hip_synchronize) and downloading from it raise too."""
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import slab as SL
    p, pos, vel, mass = moving_block(20000, unequal=False)
    cuts = SL.plan_cuts(p, pos.reshape(-1, 3)[:, 2], 2)
    import torch
    stream = torch.cuda.Stream()
    slabs = []
    for r in range(2):
        s = SL.HipSlab(p, cuts[r], cuts[r + 1], 60000, 16, device=0, has_left=r > 0, has_right=r < 1,
                       stream=stream)
        s.upload(*SL.split_scene(p, cuts, r, pos, vel, mass), all_masses_equal=True)
        slabs.append(s)
    group = SL.LocalSlabGroup(slabs)
    stopped_at = None
    for step in range(40):
        try:
            group.step()
        except S.SphHipError as e:
            assert "lost particles" in str(e) and "error bits" in str(e)
            stopped_at = step
            break
    assert stopped_at is not None and stopped_at <= 2 * SL.LocalSlabGroup.CHECK_EVERY
    bad = [s for s in slabs if s.status()["errors"] & 2]
    assert bad
    with pytest.raises(S.SphHipError, match="lost particles"):
        bad[0].synchronize()
    with pytest.raises(S.SphHipError, match="lost particles"):
        bad[0].download()
    for s in slabs:
        s.close()


def test_early_exchange_reports_a_particle_it_missed(hiplib):
    """A particle deep inside a slab that jumps into the planes next to the border within one step
    was not in the early message; the next cell build must say so (error bit 8), not lose it."""
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import slab as SL
    p, pos, vel, mass = moving_block(20000, speed=0.0, unequal=False)
    cuts = SL.plan_cuts(p, pos.reshape(-1, 3)[:, 2], 2)
    pl = SL.plane_of(p, pos.reshape(-1, 3)[:, 2])
    # one particle of slab 0, five planes below the cut, flies up five cell planes per step
    i = int(np.nonzero(pl == cuts[1] - 6)[0][0])
    cell = 1.0 / float(p.full_cell_inv)
    vel = vel.copy()
    vel.reshape(-1, 3)[i, 2] = 5.0 * cell / (float(p.time_step) * float(p.sim_scale_inv))
    group, _ = build_group(S, p, pos, vel, mass, 2, overlap=True)
    group.step()
    group.step()
    assert group.slabs[0].status()["errors"] & 8
    for s in group.slabs:
        s.close()


@pytest.mark.parametrize("case", range(12))
def test_random_slab_runs_equal_single_context(hiplib, case):
    """Seeded random blocks, slab counts 2-6 (down to the thinnest slabs plan_cuts allows, whose
    border planes are the whole slab), the three exchange orders: per-particle results after 4
    steps equal the single context's, bit for bit, and nobody reports an error."""
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    rng = np.random.default_rng(500 + case)
    n = int(rng.choice([3000, 9000, 20000]))
    zlo = float(rng.uniform(0.3, 2.0))
    zhi = zlo + float(rng.uniform(1.0, 3.5))
    p, pos, vel, mass = scenes.dense_block(n, lo=(1.0, 1.2, zlo), hi=(2.0, 2.4, zhi), seed=case,
                                           speed=float(rng.choice([0.0, 10.0, 40.0])))
    if rng.random() < 0.5:
        mass = (0.5 + scenes.uniform01(case, np.arange(n))).astype(np.float32)
    world = int(rng.integers(2, 7))
    overlap = [False, True, "two-streams"][case % 3]
    group, cuts = build_group(S, p, pos, vel, mass, world, overlap)
    steps = 4
    for _ in range(steps):
        group.step()
    got = group.gather(n)
    for s in group.slabs:
        assert s.status()["errors"] == 0, "case %d: slab error bits %d" % (case, s.status()["errors"])
        s.close()
    with S.SPH(n, p) as one:
        one.setParticles(pos, vel, mass)
        one.run(steps)
        part = one.getParticles()
    what = "case %d (world %d, %s): " % (case, world, overlap)
    assert (got["owner"] >= 0).all(), what + "a particle belongs to no slab"
    assert np.array_equal(got["ncount"], part.mNeighborCount), what + "neighbour counts"
    assert np.array_equal(got["rho"], part.mDensity), what + "density"
    assert np.array_equal(got["acc"], part.mAcceleration), what + "acceleration"
    assert np.array_equal(got["pos"], part.mPosition), what + "position"
    assert np.array_equal(got["vel"], part.mVelocity), what + "velocity"


def test_native_rccl_exchange_single_rank(oracle, hiplib):
    """The library's own RCCL path as far as one GPU can take it: librccl opened with dlopen, a
    1-rank communicator, a message sent to itself through the same grouped ncclSend/ncclRecv on
    the exchange stream (selftest), and sph_hip_slab_comm_run on a slab that holds the whole grid
    (no neighbours: every launch of the overlapped step, no transfer) against the oracle."""
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import slab as SL
    p, pos, vel, mass = moving_block(20000, unequal=True)
    s = SL.HipSlab(p, 0, p.full_cells_z, 40000, 4096, device=0, has_left=False, has_right=False)
    s.upload(np.arange(mass.size, dtype=np.uint32), pos, vel, mass, all_masses_equal=False)
    try:
        ident = SL.rccl_unique_id()
    except S.SphHipError as e:
        if "cannot open librccl" in str(e):
            pytest.skip("no librccl on this box: " + str(e))
        raise
    s.comm_init(ident, 0, 1)
    s.comm_selftest()
    s.comm_exchange_check()            # (no neighbours: the empty group and the checks around it)
    s.comm_run(1)
    s.comm_run(2)                      # one at a time and in a batch: the same loop
    st = s.comm_stats()
    assert st == {"active_records": 4096, "capacity_records": 4096, "growths": 0, "steps": 3}, st
    d = s.download()
    assert s.status()["errors"] == 0
    opos, ovel = pos.copy(), vel.copy()
    for _ in range(3):
        ref = oracle.step(to_oracle_params(p), opos, ovel, mass, mode="full")
    ids = d["ids"].astype(np.int64)
    assert np.array_equal(np.sort(ids), np.arange(mass.size))
    assert np.array_equal(d["pos"].reshape(-1, 3), opos.reshape(-1, 3)[ids])
    assert np.array_equal(d["acc"].reshape(-1, 3), ref["acc"].reshape(-1, 3)[ids])
    assert np.array_equal(d["rho"], ref["rho"][ids])
    s.close()


def _gpu_rebalance_worker(rank, world, port, steps, outdir):
    """one process per slab, both on GPU 0 (gloo + host-staged messages: RCCL refuses two ranks on
    one device); everything else - HipSlab, kernels, message format, stepper - as on a node"""
    import os
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import smoothed_particle_hydrodynamics_amd as S
        from helpers import count_calls
        from smoothed_particle_hydrodynamics_amd import scenes
        from smoothed_particle_hydrodynamics_amd import slab as SL
        torch.cuda.set_device(0)
        p, pos, vel, mass = scenes.dense_block(40000, lo=(1.0, 1.0, 0.6), hi=(2.0, 2.0, 2.4), seed=17,
                                               speed=10.0)
        vel = vel.copy()
        vel.reshape(-1, 3)[:, 2] += np.float32(80.0)      # the block drifts up the slab axis
        mass = (0.5 + scenes.uniform01(19, np.arange(mass.size))).astype(np.float32)
        z = pos.reshape(-1, 3)[:, 2]
        cuts = SL.plan_cuts(p, z, world)

        def make_slab(new_cuts, r, hist):
            return SL.HipSlab(p, new_cuts[r], new_cuts[r + 1], 60000, 20000, device=0,
                              has_left=r > 0, has_right=r + 1 < world)

        slab = make_slab(cuts, rank, None)
        slab.upload(*SL.split_scene(p, cuts, rank, pos, vel, mass), all_masses_equal=False)
        stepper = SL.DistSlabStepper(slab, SL.HostStagedTransport(rank, world), make_slab=make_slab,
                                     cuts=cuts, rebalance_every=4, imbalance=1.02, trim_every=3)
        downloads = count_calls(SL.HipSlab, "download", "download_mass")
        for _ in range(steps):
            stepper.step()
        # the rebalances kept the host out of the data path: records exported, re-partitioned and
        # uploaded on the device (only the rows that change owner cross the gloo group of this
        # rehearsal), nothing downloaded
        assert downloads == []
        slab = stepper.slab
        slab.synchronize()
        d = slab.download()
        assert slab.status()["errors"] == 0
        np.savez(os.path.join(outdir, "rank%d.npz" % rank), cuts0=np.array(cuts),
                 cuts=np.array(stepper.cuts), rebalances=stepper.rebalances, active=slab.msg_active, **d)
        slab.close()
    finally:
        dist.destroy_process_group()


def test_rebalancing_and_trimmed_messages_on_the_gpu(hiplib, tmp_path):
    """Two slab processes on the one GPU, a scene that drifts along z: cuts re-evaluated every 4
    steps (records exported, rows that change owner exchanged, new slab contexts), message
    size agreed every 3 steps from what was packed (the pack kernels enforce it, the transport moves
    only that part): per-particle results after 10 steps equal the single context's, bit for bit."""
    import socket
    import torch.multiprocessing as mp
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    steps, world = 10, 2
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    mp.spawn(_gpu_rebalance_worker, args=(world, port, steps, str(tmp_path)), nprocs=world, join=True)
    p, pos, vel, mass = scenes.dense_block(40000, lo=(1.0, 1.0, 0.6), hi=(2.0, 2.0, 2.4), seed=17,
                                           speed=10.0)
    vel = vel.copy()
    vel.reshape(-1, 3)[:, 2] += np.float32(80.0)
    mass = (0.5 + scenes.uniform01(19, np.arange(mass.size))).astype(np.float32)
    with S.SPH(mass.size, p) as one:
        one.setParticles(pos, vel, mass)
        one.run(steps)
        part = one.getParticles()
    seen = np.zeros(mass.size, bool)
    for r in range(world):
        d = np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))
        ids = d["ids"].astype(np.int64)
        assert not seen[ids].any()
        seen[ids] = True
        assert np.array_equal(d["pos"].reshape(-1, 3), part.mPosition.reshape(-1, 3)[ids])
        assert np.array_equal(d["vel"].reshape(-1, 3), part.mVelocity.reshape(-1, 3)[ids])
        assert np.array_equal(d["rho"], part.mDensity[ids])
        assert np.array_equal(d["acc"].reshape(-1, 3), part.mAcceleration.reshape(-1, 3)[ids])
        assert np.array_equal(d["ncount"], part.mNeighborCount[ids])
        assert int(d["rebalances"]) >= 1 and (d["cuts"] != d["cuts0"]).any()
        assert int(d["active"]) < 20000
    assert seen.all()


@pytest.mark.parametrize("fused", [True, False], ids=["fused-slab-step", "separate-kernels"])
def test_slab_energies_add_up_when_workgroups_give_up(hiplib, monkeypatch, fused):
    """A two-part acceleration launch walks the give-up list in BOTH parts; only the part that owns
    a listed workgroup may write its energy partial sums (the other part's zeros raced with them on
    the unordered streams: round-3 advice).  8 logical slabs with tile capacities forced so small
    that most workgroups are on the give-up lists - some with lists (they fit one pass only), some
    without - early exchange on two streams: the slabs' KE / PE add up to the single context's."""
    import smoothed_particle_hydrodynamics_amd as S
    from helpers import energy_rtol
    from smoothed_particle_hydrodynamics_amd import scenes
    monkeypatch.setenv("SPH_HIP_TILE_CAP", "1024")
    monkeypatch.setenv("SPH_HIP_TILE_CAP_ACCEL", "768")
    monkeypatch.setenv("SPH_HIP_TILE_CAP_DENSITY", "896")
    if fused:
        monkeypatch.delenv("SPH_HIP_NO_FUSED_SLAB", raising=False)
    else:
        monkeypatch.setenv("SPH_HIP_NO_FUSED_SLAB", "1")
    p, pos, vel, mass = scenes.dam_break(160000, speed=0.05)
    p.central_mass = 1.0e5       # a potential energy to add up as well
    group, cuts = build_group(S, p, pos, vel, mass, 8, "two-streams")
    for _ in range(3):
        group.step()
    gave_up = sum(s.tile_stats()["untiled_acceleration"] for s in group.slabs)
    assert gave_up > 50, gave_up
    ke = sum(np.float64(s.energy()[0]) for s in group.slabs)
    pe = sum(np.float64(s.energy()[1]) for s in group.slabs)
    got = group.gather(mass.size)
    for s in group.slabs:
        assert s.status()["errors"] == 0
        s.close()
    with S.SPH(mass.size, p) as one:
        one.setParticles(pos, vel, mass)
        one.run(3)
        want = one.energy()
        part = one.getParticles()
        assert np.array_equal(got["pos"], part.mPosition) and np.array_equal(got["vel"], part.mVelocity)
    assert ke == pytest.approx(want[0], rel=energy_rtol(mass.size))
    assert pe == pytest.approx(want[1], rel=energy_rtol(mass.size))


def test_a_duplicated_halo_record_is_an_error_code_not_a_fault(hiplib):
    """What a first multi-GPU exchange is most likely to get wrong: a record delivered twice.  The
    two copies would take the same place in their cell's canonical order (one overwriting the other,
    one position keeping stale data); the cell build says so - error bit 16 - and the run stops with
    SPH_HIP_ERR_EXCHANGE instead of stepping on with a corrupted state or faulting."""
    import torch
    import smoothed_particle_hydrodynamics_amd as S
    p, pos, vel, mass = moving_block(20000, unequal=False)
    group, cuts = build_group(S, p, pos, vel, mass, 2)
    group.step()
    a, b = group.slabs
    for s in group.slabs:
        s.pack()
    a.stream.synchronize()
    # slab 0's message to the right: its first record once more behind the last one
    msg = a.send_right
    count = int(msg[:4].view(torch.int32)[0].item())
    assert 0 < count < a.msg_active
    header = 8 * 4
    rec = msg[header:].view(torch.float32).view(-1, 8)
    rec[count] = rec[0]
    msg[:4].view(torch.int32)[0] = count + 1
    group._deliver()
    for s in group.slabs:
        s.step()
    assert b.status()["errors"] & 16
    with pytest.raises(S.SphHipError, match="lost particles"):
        b.synchronize()
    for s in group.slabs:
        s.close()


def test_cell_counts_beyond_the_capacity_are_an_error_code_not_a_fault(hiplib):
    """Round 3's abort: a step that counted its particles twice sent the next cell build past the end
    of its arrays.  The build now clamps its ranges to the context's capacity and raises error bit 4.
    Provoked here the honest way: more records arrive than the slab has room for between its live
    entries and its capacity - twice, so that the counts of the build exceed the capacity."""
    import torch
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import slab as SL
    p, pos, vel, mass = moving_block(20000, unequal=False)
    cuts = SL.plan_cuts(p, pos.reshape(-1, 3)[:, 2], 2)
    stream = torch.cuda.Stream()
    slabs = []
    for r in range(2):
        own = SL.split_scene(p, cuts, r, pos, vel, mass)
        # slab 1 has room for its own particles and a handful more: the halo does not fit
        cap = own[0].size + 64 if r == 1 else 60000
        s = SL.HipSlab(p, cuts[r], cuts[r + 1], cap, 20000, device=0, has_left=r > 0, has_right=r < 1,
                       stream=stream)
        s.upload(*own, all_masses_equal=True)
        slabs.append(s)
    group = SL.LocalSlabGroup(slabs)
    with pytest.raises(S.SphHipError, match="lost particles"):
        for _ in range(3 * SL.LocalSlabGroup.CHECK_EVERY):
            group.step()
    assert slabs[1].status()["errors"] & 4
    for s in slabs:
        s.close()
