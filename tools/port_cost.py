"""What ports (include/sph_hip.h: sph_hip_set_ports) cost per step: the 4M-particle FULL_FAST dam column
(scenes.dam_break) with

    parent       the library of the parent commit (--parent PATH: libsph_hip.so built from it), which has no ports
    none         this tree's library, no ports: the same kernels as the parent's (tools/kernel_isa_diff.py) and the
                 same launches
    no_prehash   this tree's library with SPH_HIP_NO_PREHASH=1: the unfused route a port context takes - the cell
                 build hashes, a separate integrate kernel - without the port launch
    ports        this tree's library with one sink that catches nothing and one emitter whose `first` lies beyond
                 the run: the same route plus k_ports_apply over every particle, every step

ports - no_prehash is the kernel, no_prehash - none the price of the unfused route.  The floor of the kernel is
the 16 bytes per particle it must read.

One child process per measurement (a library is loaded once per process), the variants taking turns --rounds times
in one session; this process never opens the GPU, and every child runs under its own time limit (--child-timeout).
A child runs --warmup steps, then --reps windows of --steps steps queued back to back, each timed with a host
clock around the window and a synchronise.  Reported: the best and the median window per variant over all rounds
in ms per step, the ratios to the first variant, and the differences of the medians, as measured.

    timeout -k 10 1100 python tools/port_cost.py --parent /path/to/parent/libsph_hip.so \
        --out profiles/port_cost.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sph_hip_set_ports", "sph_hip_get_ports", "sph_hip_download_live")
HBM_MEASURED = 6.29e12   # bytes per second, a float4 copy on the MI355X


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
    windows = []
    total = args.warmup + args.reps * args.steps
    with S.SPH(mass.size, p, mode=S.MODE_FULL_FAST) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setTiming(S.TIMING_OFF)
        if args.child == "ports":
            h = float(p.h)
            sph.setPorts([S.Emitter(1, (0.5, 0.9, 0.5), (1, 1), h, (0.0, -1.0, 0.0), 1.0, first=total + 1000)],
                         [S.Sink((-3.0, -3.0, -3.0), (-2.0, -2.0, -2.0))])
        sph.run(args.warmup)
        sph.synchronize()
        for _ in range(args.reps):
            t0 = time.perf_counter()
            sph.run(args.steps)
            sph.synchronize()
            windows.append((time.perf_counter() - t0) / args.steps * 1e3)
        if args.child == "ports":
            t, _, _ = sph.getPorts()
            assert t.emitted.tolist() == [0] and t.removed.tolist() == [0] and t.live == args.particles
            assert np.isfinite(sph.downloadLive()[1]).all()
        else:
            assert np.isfinite(sph.getParticles().mPosition).all()
    print("RESULT " + json.dumps({"windows": windows}), flush=True)


def measure(variant, args):
    env = dict(os.environ)
    env.pop("SPH_HIP_LIBRARY", None)
    env.pop("SPH_HIP_NO_PREHASH", None)
    if variant == "parent":
        env["SPH_HIP_LIBRARY"] = os.path.abspath(args.parent)
    if variant == "no_prehash":
        env["SPH_HIP_NO_PREHASH"] = "1"
    cmd = [sys.executable, os.path.abspath(__file__), "--child", variant, "--particles", str(args.particles),
           "--warmup", str(args.warmup), "--steps", str(args.steps), "--reps", str(args.reps)]
    out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=args.child_timeout).stdout
    line = [ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="libsph_hip.so built from the parent commit")
    ap.add_argument("--particles", type=int, default=4 * 1024 * 1024)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child-timeout", type=float, default=240.0)
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--child", default=None, choices=["parent", "none", "no_prehash", "ports"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    runs = (["parent"] if args.parent else []) + ["none", "no_prehash", "ports"]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("port cost: %d-particle dam column, FULL_FAST; %d rounds, the variants taking turns; per child %d warm-up "
        "steps, then %d windows of %d steps" % (args.particles, args.rounds, args.warmup, args.reps, args.steps))
    windows = {r: [] for r in runs}
    for _ in range(args.rounds):
        for r in runs:
            windows[r] += measure(r, args)["windows"]      # a child that fails ends the run: nothing more is started
    base = runs[0]
    med = {r: statistics.median(windows[r]) for r in runs}
    for r in runs:
        say("%-10s best %8.4f ms/step %6.3fx   median %8.4f ms/step %6.3fx   (windows %.4f .. %.4f)" %
            (r, min(windows[r]), min(windows[r]) / min(windows[base]), med[r], med[r] / med[base], min(windows[r]),
             max(windows[r])))
    if args.parent:
        pw = windows["parent"]
        say("no ports against the parent: this tree's median %.4f minus the parent's %.4f = %+.4f ms/step (the parent's "
            "own windows spread %.4f ms/step).  The condition is structural, not this timing: the kernels that exist in "
            "the parent are the same code (tools/kernel_isa_diff.py), and without ports a step enqueues the parent's "
            "launches." % (med["none"], med["parent"], med["none"] - med["parent"], max(pw) - min(pw)))
    nw = windows["none"]
    say("the unfused route: no_prehash minus none = %+.4f ms/step (the windows without ports spread %.4f ms/step)" %
        (med["no_prehash"] - med["none"], max(nw) - min(nw)))
    floor_us = 16.0 * args.particles / HBM_MEASURED * 1e6
    say("the kernel: ports minus no_prehash = %+.4f ms/step = %.1f us; its floor, the 16 bytes per particle it must read, "
        "is %.1f MB = %.1f us at the %.2f TB/s a float4 copy reaches" %
        (med["ports"] - med["no_prehash"], (med["ports"] - med["no_prehash"]) * 1e3, 16.0 * args.particles / 1e6, floor_us,
         HBM_MEASURED / 1e12))
    say("a port context against one without: ports minus none = %+.4f ms/step (%.3fx)" %
        (med["ports"] - med["none"], med["ports"] / med["none"]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
