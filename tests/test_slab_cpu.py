"""Slab decomposition on CPU: planning, message flow and the torch.distributed transport
(gloo, world_size 2 and 3) with the oracle-backed FakeSlab standing in for the GPU slab.
The decomposed run must reproduce the single-domain oracle run bit for bit — including
particles that migrate across the cut."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from test_oracle_golden import box_fill  # noqa: E402


def scene(n=6000):
    pos = box_fill(n, (1.0, 1.0, 1.0), (2.2, 2.2, 2.6), 7)
    vel = box_fill(n, (-40.0,) * 3, (40.0,) * 3, 8)     # up to 0.4 cells per step: migration
    mass = (0.5 + box_fill(n, (0,) * 3, (1,) * 3, 11)[:n]).astype(np.float32)
    return pos, vel, mass


def test_plane_of_matches_oracle_cells(oracle):
    from smoothed_particle_hydrodynamics_amd.slab import plane_of
    p = oracle.params_for_h(0.1)
    pos, _, _ = scene(3000)
    pos[5] = 99.0        # far outside: clamped to the last plane
    pos[8] = -3.0
    ids, cs, ci = oracle.full_cells(p, pos)
    z_from_id = ids // (p.full_cells_x * p.full_cells_y)
    assert np.array_equal(plane_of(p, pos.reshape(-1, 3)[:, 2]), z_from_id)


def test_plan_cuts_balanced_and_valid(oracle):
    from smoothed_particle_hydrodynamics_amd.slab import plan_cuts, plane_of
    p = oracle.params_for_h(0.1)
    pos, _, _ = scene(20000)
    z = pos.reshape(-1, 3)[:, 2]
    for world in (1, 2, 3, 4):
        cuts = plan_cuts(p, z, world)
        assert cuts[0] == 0 and cuts[-1] == p.full_cells_z and len(cuts) == world + 1
        assert all(b - a >= 4 for a, b in zip(cuts, cuts[1:]))
        counts = np.histogram(plane_of(p, z), bins=cuts)[0]
        assert counts.sum() == z.size
        if world > 1:
            assert counts.max() < 1.6 * z.size / world
    with pytest.raises(ValueError):
        plan_cuts(p, z, 32)       # 64 planes cannot feed 32 slabs of >= 4 planes


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, steps, outdir, overlap):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from oracle.oracle import Oracle
        from fake_slab import FakeSlab
        from smoothed_particle_hydrodynamics_amd.slab import (DistSlabStepper, DistTransport,
                                                              plan_cuts, split_scene)
        o = Oracle()
        p = o.params_for_h(0.1)
        pos, vel, mass = scene()
        cuts = plan_cuts(p, pos.reshape(-1, 3)[:, 2], world)
        slab = FakeSlab(o, p, cuts[rank], cuts[rank + 1], 8192, rank > 0, rank + 1 < world)
        slab.upload(*split_scene(p, cuts, rank, pos, vel, mass), all_masses_equal=False)
        stepper = DistSlabStepper(slab, DistTransport(rank, world), overlap=overlap)
        assert stepper.overlap == overlap
        owned_history = []
        for _ in range(steps):
            stepper.step()
            owned_history.append(slab.status()["owned"])
        d = slab.download()
        assert slab.status()["errors"] == 0
        np.savez(os.path.join(outdir, "rank%d.npz" % rank), owned_history=owned_history, **d)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "early-exchange"])
@pytest.mark.parametrize("world", [2, 3])
def test_distributed_slabs_equal_single_domain(oracle, tmp_path, world, overlap):
    steps = 4
    port = _free_port()
    mp.spawn(_worker, args=(world, port, steps, str(tmp_path), overlap), nprocs=world, join=True)

    p = oracle.params_for_h(0.1)
    pos, vel, mass = scene()
    n = mass.size
    for _ in range(steps):
        ref = oracle.step(p, pos, vel, mass, mode="full")

    seen = np.zeros(n, bool)
    migrated = 0
    for r in range(world):
        d = np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))
        ids = d["ids"].astype(np.int64)
        assert not seen[ids].any()
        seen[ids] = True
        assert np.array_equal(d["pos"].reshape(-1, 3), pos.reshape(-1, 3)[ids])
        assert np.array_equal(d["vel"].reshape(-1, 3), vel.reshape(-1, 3)[ids])
        assert np.array_equal(d["rho"], ref["rho"][ids])
        assert np.array_equal(d["acc"].reshape(-1, 3), ref["acc"].reshape(-1, 3)[ids])
        assert np.array_equal(d["ncount"], ref["ncount"][ids])
        h = d["owned_history"]
        migrated += int(np.abs(np.diff(h)).sum())
    assert seen.all()
    assert migrated > 0, "the scene is meant to move particles across the cuts"


def drifting_scene(n=5000):
    """a block that moves up the z axis as a whole (plus some random motion): the balanced cuts
    of step 0 are far from balanced a few steps later"""
    pos = box_fill(n, (1.0, 1.0, 0.6), (2.0, 2.0, 2.2), 17)
    vel = box_fill(n, (-10.0,) * 3, (10.0,) * 3, 18)
    vel.reshape(-1, 3)[:, 2] += np.float32(90.0)        # ~0.9 cell planes per step
    mass = (0.5 + box_fill(n, (0,) * 3, (1,) * 3, 19)[:n]).astype(np.float32)
    return pos, vel, mass


def _worker_rebalance(rank, world, port, steps, outdir, overlap):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from oracle.oracle import Oracle
        from fake_slab import FakeSlab
        from helpers import count_calls
        from smoothed_particle_hydrodynamics_amd.slab import (DistSlabStepper, DistTransport,
                                                              plan_cuts, split_scene)
        o = Oracle()
        p = o.params_for_h(0.1)
        pos, vel, mass = drifting_scene()
        cuts = plan_cuts(p, pos.reshape(-1, 3)[:, 2], world)

        def make_slab(new_cuts, r, hist):
            return FakeSlab(o, p, new_cuts[r], new_cuts[r + 1], 8192, r > 0, r + 1 < world)

        slab = make_slab(cuts, rank, None)
        slab.upload(*split_scene(p, cuts, rank, pos, vel, mass), all_masses_equal=False)
        stepper = DistSlabStepper(slab, DistTransport(rank, world), overlap=overlap,
                                  make_slab=make_slab, cuts=cuts, rebalance_every=3, imbalance=1.02,
                                  trim_every=4)
        history, active = [list(cuts)], []
        downloads = count_calls(FakeSlab, "download")
        for _ in range(steps):
            stepper.step()
            history.append(list(stepper.cuts))
            active.append(stepper.slab.msg_active)
        # the rebalances went the way a HipSlab's go: records out, records in, no host download
        assert downloads == []
        d = stepper.slab.download()
        assert stepper.slab.status()["errors"] == 0
        np.savez(os.path.join(outdir, "rank%d.npz" % rank), cuts=np.array(history),
                 rebalances=stepper.rebalances, active=np.array(active), **d)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "early-exchange"])
@pytest.mark.parametrize("world", [2, 3])
def test_cut_rebalancing_and_message_trimming_keep_the_bits(oracle, tmp_path, world, overlap):
    """A scene that drifts along the slab axis: every 3 steps the ranks re-evaluate the cut planes
    from the z-plane histogram and move the particles that change owner, every 4 steps they agree
    on a smaller message size from what was actually packed.  Neither may change a single bit of
    any particle with respect to the single-domain run (cuts re-evaluated
    periodically; results independent of the rank count)."""
    steps = 10
    port = _free_port()
    mp.spawn(_worker_rebalance, args=(world, port, steps, str(tmp_path), overlap), nprocs=world,
             join=True)
    p = oracle.params_for_h(0.1)
    pos, vel, mass = drifting_scene()
    n = mass.size
    for _ in range(steps):
        ref = oracle.step(p, pos, vel, mass, mode="full")
    seen = np.zeros(n, bool)
    for r in range(world):
        d = np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))
        ids = d["ids"].astype(np.int64)
        assert not seen[ids].any()
        seen[ids] = True
        assert np.array_equal(d["pos"].reshape(-1, 3), pos.reshape(-1, 3)[ids])
        assert np.array_equal(d["vel"].reshape(-1, 3), vel.reshape(-1, 3)[ids])
        assert np.array_equal(d["rho"], ref["rho"][ids])
        assert np.array_equal(d["acc"].reshape(-1, 3), ref["acc"].reshape(-1, 3)[ids])
        assert np.array_equal(d["ncount"], ref["ncount"][ids])
        cuts = d["cuts"]
        assert int(d["rebalances"]) >= 2, "the drifting block must have moved the cuts"
        assert (cuts[-1] != cuts[0]).any() and (np.diff(cuts, axis=1) >= 4).all()
        assert d["active"][-1] < 8192 and d["active"][0] == 8192     # trimmed after step 4
        if r == 0:
            first = cuts
        assert np.array_equal(cuts, first)                           # every rank agrees
    assert seen.all()


def _worker_growth(rank, world, port, steps, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from oracle.oracle import Oracle
        from fake_slab import FakeSlab
        from helpers import count_calls
        from smoothed_particle_hydrodynamics_amd.slab import (DistSlabStepper, DistTransport,
                                                              plan_cuts, split_scene)
        o = Oracle()
        p = o.params_for_h(0.1)
        pos, vel, mass = crowding_scene()
        cuts = plan_cuts(p, pos.reshape(-1, 3)[:, 2], world)

        def make_slab(new_cuts, r, hist):
            return FakeSlab(o, p, new_cuts[r], new_cuts[r + 1], 8192, r > 0, r + 1 < world)

        slab = make_slab(cuts, rank, None)
        slab.set_timing(1)
        slab.set_timing_stride(5)
        slab.set_arithmetic(1)
        slab.upload(*split_scene(p, cuts, rank, pos, vel, mass), all_masses_equal=False)
        # the agreements travel over their own gloo group with host tensors (bench.py: the
        # control plane must not depend on the device-to-device path)
        control = dist.new_group(backend="gloo")
        stepper = DistSlabStepper(slab, DistTransport(rank, world), overlap=True, make_slab=make_slab,
                                  cuts=cuts, rebalance_every=0, control_group=control)
        stepper.CHECK_EVERY = 2
        active = []
        downloads = count_calls(FakeSlab, "download")
        for s in range(steps):
            if s == 2:
                stepper.trim_messages(slack=1.05, extra=4)      # tight on purpose
            if s == steps - 2:
                stepper.rebalance(force=True)
            stepper.step()
            active.append(stepper.slab.msg_active)
        assert downloads == []          # the rebalance moved records, as a HipSlab's does
        final = stepper.slab
        assert final is not slab and getattr(slab, "closed", False)
        assert final.settings() == {"timing": 1, "timing_stride": 5, "arithmetic": 1}
        d = final.download()
        assert final.status()["errors"] == 0
        np.savez(os.path.join(outdir, "rank%d.npz" % rank), active=np.array(active),
                 growths=stepper.message_growths, **d)
    finally:
        dist.destroy_process_group()


def crowding_scene(n=6000):
    """two blocks that run into each other across the middle of the z range: the strips next to
    the cut fill up step by step - a trimmed message has to grow before it overflows"""
    half = n // 2
    lo = box_fill(half, (1.0, 1.0, 0.4), (2.0, 2.0, 1.5), 27).reshape(-1, 3)
    hi = box_fill(n - half, (1.0, 1.0, 1.9), (2.0, 2.0, 3.0), 28).reshape(-1, 3)
    pos = np.ascontiguousarray(np.concatenate([lo, hi]).reshape(-1))
    vel = box_fill(n, (-5.0,) * 3, (5.0,) * 3, 29)
    v = vel.reshape(-1, 3)
    v[:half, 2] += np.float32(60.0)
    v[half:, 2] -= np.float32(60.0)
    mass = np.ones(n, np.float32)
    return pos, vel, mass


def test_trimmed_messages_grow_before_they_overflow_and_settings_survive_a_rebalance(oracle, tmp_path):
    """Messages trimmed tightly while the strips next to the cut are still thin; then the blocks
    meet there.  The ranks notice from asynchronously copied record counts (no device
    synchronisation), agree over the control group and go back to the allocated size before
    anything is dropped (FakeSlab asserts on an overflow); a forced rebalance late in the run
    hands the timing level, stride and arithmetic on to the new slab, and the stepper's slab -
    not the one the caller created - is the one that lives on."""
    world, steps = 2, 12
    port = _free_port()
    mp.spawn(_worker_growth, args=(world, port, steps, str(tmp_path)), nprocs=world, join=True)
    p = oracle.params_for_h(0.1)
    pos, vel, mass = crowding_scene()
    for _ in range(steps):
        ref = oracle.step(p, pos, vel, mass, mode="full")
    seen = np.zeros(mass.size, bool)
    for r in range(world):
        d = np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))
        ids = d["ids"].astype(np.int64)
        seen[ids] = True
        assert np.array_equal(d["pos"].reshape(-1, 3), pos.reshape(-1, 3)[ids])
        assert np.array_equal(d["rho"], ref["rho"][ids])
        assert int(d["growths"]) >= 1, "the crowding strips must have forced the messages to grow"
        a = d["active"]
        assert a[2] < 8192 and a[-1] == 8192, a
    assert seen.all()


def test_scene_subsets_match_the_whole_scene():
    """bench.py's ranks generate only their own slab: any coordinate axis or subset of rows of the
    counter-based scene must equal the corresponding part of the whole scene, and the parameters
    must not depend on whether particles were generated."""
    from smoothed_particle_hydrodynamics_amd import scenes
    n = 20000
    p, pos, vel, mass = scenes.dam_break(n, box=(1.0, 1.0, 3.0))
    p2, hi = scenes.dam_break_params(n, box=(1.0, 1.0, 3.0))
    assert bytes(p) == bytes(p2)
    for axis in range(3):
        a = scenes.box_fill_axis(n, (0.0, 0.0, 0.0), hi, axis)
        assert np.array_equal(a, pos.reshape(-1, 3)[:, axis])
    ids = np.array([0, 1, 17, 4096, n - 1, 12345], np.int64)
    sub = scenes.box_fill_subset(ids, (0.0, 0.0, 0.0), hi).reshape(-1, 3)
    assert np.array_equal(sub, pos.reshape(-1, 3)[ids])
    assert not vel.any() and (mass == 1.0).all()


def _worker_preflight(rank, world, port, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from smoothed_particle_hydrodynamics_amd.slab import neighbour_exchange_works
        ok = neighbour_exchange_works(rank, world, "cpu")
        # a second group, as bench.py makes for the agreement and the fallback transport
        other = dist.new_group(backend="gloo")
        verdict = torch.tensor([1 if ok else 0], dtype=torch.int32)
        dist.all_reduce(verdict, op=dist.ReduceOp.MIN, group=other)
        ok2 = neighbour_exchange_works(rank, world, "cpu", group=other)
        np.save(os.path.join(outdir, "ok%d.npy" % rank), np.array([ok, int(verdict.item()), ok2]))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_exchange_preflight_reports_a_working_path(tmp_path, world):
    """bench.py's first contact with the neighbour exchange (one small batch_isend_irecv per
    neighbour, content checked, verdicts agreed over a gloo group): on a working backend every
    rank says yes, on the default group and on a second one."""
    port = _free_port()
    mp.spawn(_worker_preflight, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        assert np.load(os.path.join(str(tmp_path), "ok%d.npy" % r)).tolist() == [1, 1, 1]
