"""GPU: every path that carries results back to a caller, against CPU references.

The asynchronous host mirror (sph_hip_download_async / sph_hip_download_done / sph_hip_host_register,
k_export and k_voxel_counts behind them), the blocking sph_hip_download with NULL pointers and after a
smaller upload, SPH.getGrid() per cell, sph_hip_get_neighbor_stats, and the calls that a context of the
wrong mode or kind must refuse.  The contract is the one written in include/sph_hip.h.

References, none of them from the code under test: the state after k steps is the oracle's, bit for bit
(REF, FULL); a FULL_FAST context, whose arithmetic is not what is under test here, is compared with its
own blocking sph_hip_download taken at the same point.  Occupancy on the REF voxel grid is
np.diff(oracle.voxelize(...)[2]) of the positions the same snapshot returned and, independently, numpy's
bincount (helpers.grid_occupancy); on the FULL grid np.diff(oracle.full_cells(...)[1]) of the positions
the last cell build saw.  tests/test_readback_cpu.py pins these references to each other.

The scene is helpers.readback_scene: a 5 x 9 x 17 voxel grid (no two extents alike on either grid), three
quarters of the particles clamped, particles on voxel faces, non-finite coordinates.  No test here waits,
sleeps, retries or depends on which of two outcomes a race has."""
import ctypes as C

import numpy as np
import pytest

from helpers import READBACK_COUNTS, grid_occupancy, readback_scene, to_oracle_params

pytestmark = pytest.mark.gpu

MODES = ("ref", "full", "fast")
NAMES = ("pos", "vel", "rho", "acc", "ncount", "vox")     # the six arrays of a mirror, in argument order
STATE = NAMES[:5]                                          # those of a blocking download
SENTINEL = np.uint32(0xA5C3F00D)                           # (as a float: -3.4e-16, a value no scene here holds)
ERR_INVALID = -1                                           # SPH_HIP_ERR_INVALID
RED_THREADS = 256                                          # csrc/common_kernels.h


def mode_id(mode):
    import smoothed_particle_hydrodynamics_amd as S
    return {"ref": S.MODE_REF, "full": S.MODE_FULL, "fast": S.MODE_FULL_FAST}[mode]


def make_sph(mode, p, pos, vel, mass, capacity=None):
    import smoothed_particle_hydrodynamics_amd as S
    sph = S.SPH(mass.size, p, mode=mode_id(mode), capacity=capacity)
    sph.setParticles(pos, vel, mass)
    return sph


def ref_cells(p):
    return (p.cells_x, p.cells_y, p.cells_z)


def full_cells(p):
    return (p.full_cells_x, p.full_cells_y, p.full_cells_z)


def words(name, n, p=None):
    if name == "vox":
        return p.cells_x * p.cells_y * p.cells_z
    return {"pos": 3 * n, "vel": 3 * n, "rho": n, "acc": 3 * n, "ncount": n}[name]


def sentinel_buffers(n, p, rows=None):
    """the six arrays as uint32 words, every word the sentinel; rows > n: room past the end that a
    download of n particles must leave alone"""
    return {k: np.full(words(k, n if rows is None else rows, p), SENTINEL, np.uint32) for k in NAMES}


def untouched(a):
    return bool((a == SENTINEL).all())


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def request(sph, buf, want=NAMES):
    """sph_hip_download_async for the arrays named in `want` (NULL for the others): *started"""
    started = C.c_int(-7)
    sph.call("sph_hip_download_async", *[ptr(buf[k]) if k in want else None for k in NAMES], C.byref(started))
    return started.value


def blocking(sph, buf, want=STATE):
    sph.call("sph_hip_download", *[ptr(buf[k]) if k in want else None for k in STATE])


def bits(a):
    """the words of a, every NaN written as the one quiet NaN (x86 and the GPU make different payloads)"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.float32)
    if a.dtype.kind == "f":
        a = np.where(np.isnan(a), np.float32(np.nan), a).astype(np.float32)
    return np.ascontiguousarray(a).view(np.uint32)


def assert_state(buf, want, n, what, names=STATE):
    """the first n rows of the named arrays in buf are bit for bit the state `want`"""
    for k in names:
        m = words(k, n)
        assert np.array_equal(bits(buf[k][:m]), bits(want[k])), "%s: %s differs" % (what, k)


def assert_occupancy(oracle, p, buf, pos, what):
    """buf's voxel counts are the REF-grid occupancy of positions pos: the oracle's and numpy's"""
    got = buf["vox"].view(np.int32)
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1)
    assert got.sum() == pos.size // 3, what + ": occupancy does not sum to the particle count"
    assert np.array_equal(got, np.diff(oracle.voxelize(to_oracle_params(p), pos)[2])), what + ": occupancy (oracle)"
    assert np.array_equal(got, grid_occupancy(pos, p.htimes2inv, ref_cells(p))[1]), what + ": occupancy (numpy)"


_ORACLE_STATES = {}


def oracle_state(oracle, mode, n, k):
    """the oracle's state of readback_scene(n) after k steps, REF or FULL (k = 0: the upload; rho, acc and
    ncount then missing).  Computed once per (mode, n), step by step, and never changed afterwards."""
    assert mode in ("ref", "full")
    states = _ORACLE_STATES.setdefault((mode, n), [])
    p, pos, vel, mass = readback_scene(n)
    if not states:
        states.append(dict(pos=pos, vel=vel))
    while len(states) <= k:
        a, b = states[-1]["pos"].copy(), states[-1]["vel"].copy()
        r = oracle.step(to_oracle_params(p), a, b, mass, mode=mode)
        states.append(dict(pos=a, vel=b, rho=r["rho"], acc=r["acc"], ncount=r["ncount"]))
        for v in states[-1].values():
            v.setflags(write=False)
    return states[k]


_FAST_STATES = {}


def fast_state(n, k):
    """FULL_FAST: the blocking download of a fresh context that ran k steps of readback_scene(n) (the FAST
    arithmetic gives the same bits on every route: test_gpu_full_fast.py); read-only, like the oracle's states"""
    if (n, k) not in _FAST_STATES:
        p, pos, vel, mass = readback_scene(n)
        with make_sph("fast", p, pos, vel, mass) as sph:
            sph.run(k)
            part = sph.getParticles()
            _FAST_STATES[(n, k)] = dict(pos=part.mPosition.copy(), vel=part.mVelocity.copy(), rho=part.mDensity.copy(),
                                        acc=part.mAcceleration.copy(), ncount=part.mNeighborCount.copy())
            for v in _FAST_STATES[(n, k)].values():
                v.setflags(write=False)
    return _FAST_STATES[(n, k)]


def state_now(oracle, sph, mode, n, k):
    """what the context must hold after k steps: the oracle's state, or (FULL_FAST) its own blocking
    download, taken now"""
    if mode != "fast":
        return oracle_state(oracle, mode, n, k)
    buf = sentinel_buffers(n, sph.getParams())
    blocking(sph, buf)
    return {name: buf[name].view(np.int32 if name == "ncount" else np.float32) for name in STATE}


# ---- 1. a snapshot is a picture of its moment ---------------------------------------------------------

@pytest.mark.parametrize("n", READBACK_COUNTS)
@pytest.mark.parametrize("mode", MODES)
def test_snapshot_is_of_the_steps_queued_before_it(oracle, hiplib, mode, n):
    """k steps, a request for all six arrays, at once m more steps, then the wait: every array is the state
    after k steps whatever the m steps did meanwhile, the occupancy is that of the snapshot's own positions
    on the REF voxel grid (in FULL mode too), and a blocking download afterwards is the state after k + m"""
    k, m = 2, 3
    p, pos, vel, mass = readback_scene(n)
    with make_sph(mode, p, pos, vel, mass) as sph:
        sph.run(k)
        want = state_now(oracle, sph, mode, n, k)
        buf = sentinel_buffers(n, p)
        assert request(sph, buf) == 1
        sph.run(m)
        assert sph.call("sph_hip_download_done", 1) == 1
        assert_state(buf, want, n, "mirror after %d steps" % k)
        assert_occupancy(oracle, p, buf, buf["pos"].view(np.float32), "mirror")
        assert_occupancy(oracle, p, buf, want["pos"], "mirror")
        late = sentinel_buffers(n, p)
        blocking(sph, late)
        want_late = fast_state(n, k + m) if mode == "fast" else oracle_state(oracle, mode, n, k + m)
        assert_state(late, want_late, n, "blocking download after %d steps" % (k + m))
        assert not np.array_equal(bits(late["pos"]), bits(buf["pos"]))      # the m steps did move the particles
        assert sph.call("sph_hip_download_done", 0) == 1


# ---- 2. any pointer may be NULL -----------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_null_subsets_write_only_what_was_asked_for(oracle, hiplib, mode):
    """each of the six arrays alone, and none at all: the request starts, the array asked for is right and
    every other keeps its sentinel; the same subsets of the blocking download"""
    n, k = 6000, 2
    p, pos, vel, mass = readback_scene(n)
    with make_sph(mode, p, pos, vel, mass) as sph:
        sph.run(k)
        want = state_now(oracle, sph, mode, n, k)
        for asked in [(name,) for name in NAMES] + [()]:
            buf = sentinel_buffers(n, p)
            assert request(sph, buf, asked) == 1, asked
            assert sph.call("sph_hip_download_done", 1) == 1
            for name in NAMES:
                if name not in asked:
                    assert untouched(buf[name]), "a request for %r wrote %s" % (asked, name)
            if asked == ("vox",):
                assert_occupancy(oracle, p, buf, want["pos"], "voxel counts alone")
            else:
                assert_state(buf, want, n, "mirror of %r" % (asked,), asked)
        for asked in [(name,) for name in STATE] + [()]:
            buf = sentinel_buffers(n, p)
            blocking(sph, buf, asked)
            for name in NAMES:
                if name not in asked:
                    assert untouched(buf[name]), "a download of %r wrote %s" % (asked, name)
            assert_state(buf, want, n, "download of %r" % (asked,), asked)


# ---- 3. a request while one is travelling is dropped --------------------------------------------------

# Steps queued in front of request A, so that A is still on its way when request B is made.  Measured on an
# MI355X with phaseTotals() over 100 step() calls of readback_scene(6000): 75.5 us of GPU time per step in
# REF mode, 70.7 us in FULL, 72.1 us in FULL_FAST, so 800 steps are 57 ms of it in the fastest mode.  That is
# the work queued, not the work still waiting when the request is made: the host needs 55 - 73 us to enqueue
# a step of run(), no less than the GPU needs to execute it, and when run(800) returns 2.2 ms (REF), 3.4 ms
# (FULL) and 3.9 ms (FULL_FAST) of it are left.  The margin the drop rests on is therefore those 2 - 4 ms plus
# request A's own export kernel, event and six copies on a second stream, against the microseconds between
# two host calls: a factor of several hundred, not the ten thousand that 50 ms would give.  A longer queue
# does not widen it.  Should A ever have arrived, the test fails; it cannot pass without the drop.
QUEUED_STEPS = 800


@pytest.mark.parametrize("mode", MODES)
def test_request_while_one_travels_is_dropped_and_touches_nothing(oracle, hiplib, mode):
    """request A behind QUEUED_STEPS steps, q = done(no wait), request B into other arrays.  Asserted are
    the implications of the contract, not an outcome: q == 1 implies B started; B dropped implies its
    arrays keep every sentinel word and A's hold the state A was asked at; B started implies B's arrays
    hold a complete state.  With the queue above A is still travelling, so the drop is what happens: the
    test fails, rather than pass without it, if A had already arrived.  Both sets of arrays are page-locked,
    as the header asks of a host that wants the copy to be asynchronous."""
    n, k = 6000, QUEUED_STEPS
    p, pos, vel, mass = readback_scene(n)
    a, b = sentinel_buffers(n, p), sentinel_buffers(n, p)
    pinned = []
    try:
        for arr in list(a.values()) + list(b.values()):
            assert hiplib.sph_hip_host_register(ptr(arr), arr.nbytes) == 0
            pinned.append(arr)
        with make_sph(mode, p, pos, vel, mass) as sph:
            sph.run(k)
            started_a = request(sph, a)
            q = sph.call("sph_hip_download_done", 0)
            started_b = request(sph, b)
            assert started_a == 1
            assert sph.call("sph_hip_download_done", 1) == 1
            sph.synchronize()
            if q == 1:
                assert started_b == 1
            want = fast_state(n, k) if mode == "fast" else oracle_state(oracle, mode, n, k)
            if started_b == 0:
                for name in NAMES:
                    assert untouched(b[name]), "the dropped request wrote " + name
                assert_state(a, want, n, "request A")
                assert_occupancy(oracle, p, a, want["pos"], "request A")
            else:
                assert_state(b, want, n, "request B")
                assert_occupancy(oracle, p, b, want["pos"], "request B")
            assert q == 0 and started_b == 0, "request A had arrived before B was made: lengthen the queue"
    finally:
        for arr in pinned:
            hiplib.sph_hip_host_unregister(ptr(arr))


# ---- 4. destroy with a copy in flight -----------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_destroy_waits_for_the_copy_in_flight(oracle, hiplib, mode):
    """a request, then sph_hip_destroy at once: the context drains its copy stream before it frees the
    staging, so the arrays (alive until after the destroy) hold the complete snapshot"""
    n, k = 6000, 2
    p, pos, vel, mass = readback_scene(n)
    buf = sentinel_buffers(n, p)
    sph = make_sph(mode, p, pos, vel, mass)
    try:
        sph.run(k)
        want = state_now(oracle, sph, mode, n, k)
        assert request(sph, buf) == 1
    finally:
        sph.close()
    assert_state(buf, want, n, "mirror after destroy")
    assert_occupancy(oracle, p, buf, want["pos"], "mirror after destroy")


# ---- 5. page-locked against pageable ------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_page_locked_arrays_get_the_same_bytes(oracle, hiplib, mode):
    n, k = 6000, 2
    p, pos, vel, mass = readback_scene(n)
    pageable, locked = sentinel_buffers(n, p), sentinel_buffers(n, p)
    pinned = []
    try:
        for arr in locked.values():
            assert hiplib.sph_hip_host_register(ptr(arr), arr.nbytes) == 0
            pinned.append(arr)
        with make_sph(mode, p, pos, vel, mass) as sph:
            sph.run(k)
            want = state_now(oracle, sph, mode, n, k)
            for buf in (pageable, locked):
                assert request(sph, buf) == 1
                assert sph.call("sph_hip_download_done", 1) == 1
        assert_state(locked, want, n, "page-locked mirror")
        assert_occupancy(oracle, p, locked, want["pos"], "page-locked mirror")
        for name in NAMES:
            assert np.array_equal(locked[name], pageable[name]), name
    finally:
        for arr in pinned:
            assert hiplib.sph_hip_host_unregister(ptr(arr)) == 0


def test_host_register_refuses_null_and_empty(hiplib):
    arr = np.zeros(64, np.float32)
    assert hiplib.sph_hip_host_register(None, arr.nbytes) == ERR_INVALID
    assert hiplib.sph_hip_host_register(ptr(arr), 0) == ERR_INVALID
    assert hiplib.sph_hip_host_unregister(None) == ERR_INVALID


# ---- 6. a smaller upload into the same context --------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_smaller_upload_reads_back_its_own_rows_only(oracle, hiplib, mode):
    """6000 particles and a step, then 257 into the same context and a step: the blocking download and the
    mirror return exactly the 257 rows, the occupancy sums to 257, and arrays sized for 6000 keep their
    sentinel past row 257"""
    big, n = 6000, 257
    p, pos, vel, mass = readback_scene(big)
    with make_sph(mode, p, pos, vel, mass) as sph:
        sph.step()
        sph.synchronize()
        _, pos, vel, mass = readback_scene(n)
        sph.setParticles(pos, vel, mass)
        sph.step()
        assert sph.call("sph_hip_particle_count") == n
        want = fast_state(n, 1) if mode == "fast" else oracle_state(oracle, mode, n, 1)
        down, mirror = sentinel_buffers(n, p, rows=big), sentinel_buffers(n, p, rows=big)
        blocking(sph, down)
        assert request(sph, mirror) == 1
        assert sph.call("sph_hip_download_done", 1) == 1
        for what, buf in (("download", down), ("mirror", mirror)):
            assert_state(buf, want, n, what + " after the smaller upload")
            for name in STATE:
                assert untouched(buf[name][words(name, n, p):]), "%s wrote %s past row %d" % (what, name, n)
        assert untouched(down["vox"])
        assert mirror["vox"].view(np.int32).sum() == n
        assert_occupancy(oracle, p, mirror, want["pos"], "mirror after the smaller upload")


# ---- 7. getGrid() per cell ----------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_get_grid_per_cell(oracle, hiplib, mode):
    """SPH.getGrid() (sph_hip_download_grid_counts) cell by cell: after step() the occupancy of the
    positions that entered the step, after a stand-alone voxelizeParticles() that of the current ones - on
    the FULL grid (FULL, FULL_FAST) against oracle.full_cells, on the voxel grid (REF) against
    oracle.voxelize; and against numpy's bincount on either"""
    n = 6000
    p, pos, vel, mass = readback_scene(n)
    op = to_oracle_params(p)

    def occupancy(x):
        x = np.ascontiguousarray(x, np.float32)
        if mode == "ref":
            return np.diff(oracle.voxelize(op, x)[2]), grid_occupancy(x, p.htimes2inv, ref_cells(p))[1]
        return np.diff(oracle.full_cells(op, x)[1]), grid_occupancy(x, p.full_cell_inv, full_cells(p))[1]

    with make_sph(mode, p, pos, vel, mass) as sph:
        sph.step()
        entered = state_now(oracle, sph, mode, n, 1)["pos"]
        sph.step()
        for want in occupancy(entered):
            got = sph.getGrid()
            assert got.sum() == n and np.array_equal(got, want), "getGrid() after step()"
        now = state_now(oracle, sph, mode, n, 2)["pos"]
        assert not np.array_equal(occupancy(now)[0], occupancy(entered)[0])     # the step did change the occupancy
        sph.voxelizeParticles()
        for want in occupancy(now):
            got = sph.getGrid()
            assert got.sum() == n and np.array_equal(got, want), "getGrid() after voxelizeParticles()"


# ---- 8. neighbour statistics --------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["ref", "full"])
def test_neighbor_stats_on_the_shared_scene(oracle, hiplib, mode):
    n = 6000
    p, pos, vel, mass = readback_scene(n)
    with make_sph(mode, p, pos, vel, mass) as sph:
        sph.step()
        want = oracle.neighbor_stats(oracle_state(oracle, mode, n, 1)["ncount"])
        assert sph.neighborStats() == want
        assert want[1] > 0 and want[2] == 0


def test_neighbor_stats_min_starts_at_34(oracle, hiplib):
    """FULL mode on a block so dense that every particle has more than 34 neighbours: min is the start
    value of the reference's running minimum (src/sph.cpp:206), not the smallest count"""
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dense_block(12000, hi=(1.5, 1.5, 1.5))
    opos, ovel = pos.copy(), vel.copy()
    ref = oracle.step(to_oracle_params(p), opos, ovel, mass, mode="full")
    assert ref["ncount"].min() > 34
    want = oracle.neighbor_stats(ref["ncount"])
    assert want == (int(ref["ncount"].astype(np.int64).sum()) // mass.size, int(ref["ncount"].max()), 34)
    with make_sph("full", p, pos, vel, mass) as sph:
        sph.step()
        assert sph.neighborStats() == want


@pytest.mark.parametrize("mode", ["ref", "full"])
def test_neighbor_stats_of_one_particle(oracle, hiplib, mode):
    p, pos, vel, mass = readback_scene(1)
    with make_sph(mode, p, pos, vel, mass) as sph:
        sph.step()
        assert sph.neighborStats() == (0, 0, 0) == oracle.neighbor_stats(oracle_state(oracle, mode, 1, 1)["ncount"])


@pytest.mark.parametrize("scene", ["dense_block", "tail_decides"])
def test_neighbor_stats_stride_loop_second_trip(oracle, hiplib, scene):
    """REF mode, 1024 * RED_THREADS + 257 particles, one step: the reduction is launched with at most 1024
    workgroups, so 257 threads go round its grid-stride loop a second time.  "dense_block": the particles of
    scenes.dense_block.  "tail_decides": the same, but the first 1024 * RED_THREADS rows moved onto a lattice
    wider than h, where nothing has a neighbour, and the last 257 shrunk into voxel (1, 1, 1), which they
    have to themselves - the maximum then comes from the second trip alone (among
    262 401 particles of the dense block, 257 more or fewer rarely change sum / n, max or min)."""
    from smoothed_particle_hydrodynamics_amd import scenes
    head = 1024 * RED_THREADS
    n = head + 257
    p, pos, vel, mass = scenes.dense_block(n)
    if scene == "tail_decides":
        i = np.arange(head)
        lattice = np.stack([i % 64, (i // 64) % 64, i // 4096], 1).astype(np.float32) * np.float32(0.1001)
        pos.reshape(-1, 3)[:head] = lattice + np.float32([0.55, 0.003, 0.003])
        pos.reshape(-1, 3)[head:] = np.float32(0.27) + np.float32(0.05) * (pos.reshape(-1, 3)[head:] - np.float32(1.0))
    opos, ovel = pos.copy(), vel.copy()
    ref = oracle.step(to_oracle_params(p), opos, ovel, mass, mode="ref")
    want = oracle.neighbor_stats(ref["ncount"])
    if scene == "tail_decides":
        assert ref["ncount"][:head].max() == 0 and want[1] > 0
        assert oracle.neighbor_stats(ref["ncount"][:head]) != want
    else:
        assert want[0] > 0 and want[1] > want[0]
    with make_sph("ref", p, pos, vel, mass) as sph:
        sph.step()
        assert sph.neighborStats() == want
        assert np.array_equal(sph.getParticles().mNeighborCount, ref["ncount"])


# ---- 9. what a context of the wrong mode or kind refuses ----------------------------------------------

def last_error(hiplib, ctx):
    return hiplib.sph_hip_last_error(ctx._ctx).decode()


@pytest.mark.parametrize("mode", ["full", "fast"])
def test_ref_only_downloads_are_refused_by_a_full_context(hiplib, mode):
    n = 257
    p, pos, vel, mass = readback_scene(n)
    with make_sph(mode, p, pos, vel, mass) as sph:
        sph.step()
        coords, ids = np.full(3 * n, SENTINEL, np.uint32), np.full(n, SENTINEL, np.uint32)
        assert hiplib.sph_hip_download_voxels(sph._ctx, ptr(coords), ptr(ids)) == ERR_INVALID
        assert "sph_hip_download_voxels" in last_error(hiplib, sph)
        assert untouched(coords) and untouched(ids)
        nb = np.full(n * p.examine_count, SENTINEL, np.uint32)
        nd = np.full(n * p.examine_count, SENTINEL, np.uint32)
        assert hiplib.sph_hip_download_neighbor_lists(sph._ctx, ptr(nb), ptr(nd)) == ERR_INVALID
        assert "sph_hip_download_neighbor_lists" in last_error(hiplib, sph)
        assert untouched(nb) and untouched(nd)


def test_whole_grid_downloads_are_refused_by_a_slab_context(hiplib):
    """a slab context (the lower half of the planes) refuses sph_hip_download and sph_hip_download_async,
    writes nothing, and leaves *started == 0"""
    from smoothed_particle_hydrodynamics_amd.lib import Context
    n = 257
    p, _, _, _ = readback_scene(n)
    with Context("sph_hip_create_slab", C.byref(p), n, 0, 0, p.full_cells_z // 2) as slab:
        buf = sentinel_buffers(n, p)
        assert hiplib.sph_hip_download(slab._ctx, *[ptr(buf[k]) for k in STATE]) == ERR_INVALID
        assert "sph_hip_download" in last_error(hiplib, slab)
        started = C.c_int(-7)
        assert hiplib.sph_hip_download_async(slab._ctx, *[ptr(buf[k]) for k in NAMES], C.byref(started)) == ERR_INVALID
        assert "sph_hip_download_async" in last_error(hiplib, slab)
        assert started.value == 0
        assert hiplib.sph_hip_download_done(slab._ctx, 1) == 1
        for name in NAMES:
            assert untouched(buf[name]), name
