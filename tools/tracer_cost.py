"""What tracers (include/sph_hip.h: sph_hip_set_tracers) cost per step: the 4M-particle FULL_FAST dam column
(scenes.dam_break) with tracers on every 16th and on every 4th particle position, in upload order - the
unordered probes of profiles/sample_cost.txt - with

    parent     the library of the parent commit (--parent PATH: libsph_hip.so built from it), which has no tracers
    none       this tree's library, no tracer set: the same kernels as the parent's (tools/kernel_isa_diff.py)
    unsorted   this tree's library with tracers, SPH_HIP_TRACER_SORT=0: the slots stay in upload order
    sorted     the same tracers, SPH_HIP_TRACER_SORT=<--cadence>: the slots re-sorted by cell at that cadence

One child process per measurement (a library is loaded, and the switch read, once per process), the variants
taking turns --rounds times in one session; this process never opens the GPU, and every child runs under its own
time limit (--child-timeout).  A child runs --warmup steps (the mixing), then --reps windows of --steps steps queued
back to back, each timed with a host clock around the window and a synchronise.  Reported: the best and the median
window per variant over all rounds in ms per step, the ratios to the parent, the cost of a tracer-step in ns
(median minus the median without tracers, over the tracer count), and the two conditions: `none` against the
spread of the parent's own windows, `sorted` against `unsorted` and the spread of the unsorted windows.

    timeout -k 10 1100 python tools/tracer_cost.py --parent /path/to/parent/libsph_hip.so \
        --out profiles/tracer_cost.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sph_hip_set_tracers", "sph_hip_get_tracers", "sph_hip_tracer_count", "sph_hip_record_tracers",
               "sph_hip_get_tracer_path")


def child(args):
    sys.path.insert(0, ROOT)
    from smoothed_particle_hydrodynamics_amd import lib as B
    if args.child == "parent":
        for name in NEW_SYMBOLS:          # the parent's library does not export them
            B.PROTOTYPES.pop(name)
    import numpy as np

    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dam_break(args.particles)
    windows, wet = [], 0
    with S.SPH(mass.size, p, mode=S.MODE_FULL_FAST) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setTiming(S.TIMING_OFF)
        if args.stride > 0:
            sph.setTracers(pos.reshape(-1, 3)[::args.stride])
        sph.run(args.warmup)
        sph.synchronize()
        for _ in range(args.reps):
            t0 = time.perf_counter()
            sph.run(args.steps)
            sph.synchronize()
            windows.append((time.perf_counter() - t0) / args.steps * 1e3)
        if args.stride > 0:
            t = sph.getTracers()
            assert np.isfinite(t.position).all()
            assert (t.wet_steps + t.dry_steps == args.warmup + args.reps * args.steps).all()
            wet = int(t.wet_steps.sum())
        assert np.isfinite(sph.getParticles().mPosition).all()
    print("RESULT " + json.dumps({"windows": windows, "wet": wet}), flush=True)


def measure(variant, stride, args):
    env = dict(os.environ)
    env.pop("SPH_HIP_LIBRARY", None)
    env.pop("SPH_HIP_TRACER_SORT", None)
    if variant == "parent":
        env["SPH_HIP_LIBRARY"] = os.path.abspath(args.parent)
    if variant == "unsorted":
        env["SPH_HIP_TRACER_SORT"] = "0"
    if variant == "sorted":
        env["SPH_HIP_TRACER_SORT"] = str(args.cadence)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", variant, "--stride", str(stride),
           "--particles", str(args.particles), "--warmup", str(args.warmup), "--steps", str(args.steps),
           "--reps", str(args.reps)]
    out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=args.child_timeout).stdout
    line = [ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="libsph_hip.so built from the parent commit")
    ap.add_argument("--particles", type=int, default=4 * 1024 * 1024)
    ap.add_argument("--strides", type=int, nargs="+", default=[16, 4], help="a tracer on every n-th particle")
    ap.add_argument("--cadence", type=int, default=16, help="SPH_HIP_TRACER_SORT of the sorted variant")
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child-timeout", type=float, default=240.0)
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--child", default=None, choices=["parent", "none", "unsorted", "sorted"], help=argparse.SUPPRESS)
    ap.add_argument("--stride", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    runs = ([("parent", 0)] if args.parent else []) + [("none", 0)]
    for s in args.strides:
        runs += [("unsorted", s), ("sorted", s)]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("tracer cost: %d-particle dam column, FULL_FAST; %d rounds, the variants taking turns; per child %d warm-up "
        "steps, then %d windows of %d steps; sorted = SPH_HIP_TRACER_SORT=%d" %
        (args.particles, args.rounds, args.warmup, args.reps, args.steps, args.cadence))
    windows = {r: [] for r in runs}
    wet = {}
    for _ in range(args.rounds):
        for r in runs:
            got = measure(r[0], r[1], args)      # a child that fails ends the run: nothing more is started
            windows[r] += got["windows"]
            wet[r] = got["wet"]
    base = runs[0]
    med = {r: statistics.median(windows[r]) for r in runs}
    total_steps = args.warmup + args.reps * args.steps
    for r in runs:
        count = args.particles // r[1] if r[1] else 0
        name = "%-8s %9d tracers" % (r[0], count)
        extra = ""
        if count:
            extra = "   %6.3f ns per tracer-step, %4.1f %% of tracer-steps wet" % (
                (med[r] - med[("none", 0)]) * 1e6 / count, 100.0 * wet[r] / (count * total_steps))
        say("%s best %8.4f ms/step %6.3fx   median %8.4f ms/step %6.3fx   (windows %.4f .. %.4f)%s" %
            (name, min(windows[r]), min(windows[r]) / min(windows[base]), med[r], med[r] / med[base],
             min(windows[r]), max(windows[r]), extra))
    say("for comparison, the sampler (profiles/sample_cost.txt): 0.17 ns per coherent probe, 2.36 ns per unordered "
        "probe; a tracer-step is two probes with velocity")
    if args.parent:
        pw = windows[("parent", 0)]
        spread = max(pw) - min(pw)
        diff = med[("none", 0)] - med[("parent", 0)]
        say("condition 1, no tracers: this tree's median minus the parent's %+.4f ms/step; the parent's own windows "
            "spread %.4f ms/step: %s" % (diff, spread, "within" if abs(diff) <= spread else "OUTSIDE"))
    for s in args.strides:
        uw = windows[("unsorted", s)]
        spread = max(uw) - min(uw)
        gain = med[("unsorted", s)] - med[("sorted", s)]
        say("condition 2, every %d-th: unsorted median minus sorted median %+.4f ms/step; the unsorted windows spread "
            "%.4f ms/step: the sort %s" % (s, gain, spread, "PAYS" if gain > spread else "does not pay"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
