"""What the step monitor (include/sph_hip.h: step monitor) costs: the 4M-particle FULL_FAST dam column
(scenes.dam_break), six variants taking turns in child processes (tools/cohesion_cost.py's protocol):
    parent     the library of the parent commit (--parent PATH: libsph_hip.so built from it)
    none       this tree's library without a recording: the same kernels and the same launches as the parent's
               (tools/kernel_isa_diff.py shows only the k_monitor_* kernels and their descriptors as new)
    every1     a recording with every = 1: k_monitor_particles and k_monitor_finish behind every step
    every10    a recording with every = 10: the same behind every tenth step
    scalars    carried scalars (one diffusing channel, a tenth of the bulk's stability limit) without a recording ...
    scalars1   ... and with every = 1: k_monitor_pairs behind the scalar pass as well
Each child builds the scene, warms up, and times windows of queued steps between two synchronisations; the variants
take turns over several rounds and every window is kept; the recording holds a row for every step of a child, so
every timed step of `every1` is a recorded one.  Reported: best and median ms/step per variant; `none` beside `parent`
with the parent's own window spread (the condition: a context without a recording enqueues the parent's launches);
the particle kernel and the fold (`every1` minus `none`) beside the bytes it streams, 72 per particle; and the pair
kernel (`scalars1` minus `scalars`, less the particle kernel) beside cohesion's +0.26 ms.

    timeout -k 10 1100 python tools/monitor_cost.py --parent /path/to/parent/libsph_hip.so \
        --out profiles/monitor_cost.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sph_hip_record_monitor", "sph_hip_get_monitor_record")
VARIANTS = ("parent", "none", "every1", "every10", "scalars", "scalars1")
EVERY = {"every1": 1, "every10": 10, "scalars1": 1}
STREAMED_BYTES = 72            # posm, velp, acc (16 each), rho, ncount (4 each) ... and T by id with scalars (+16)
HBM_BYTES_PER_MS = 8.0e9        # 8 TB/s peak, in bytes per millisecond
COHESION_MS = 0.26             # k_cohesion_apply alone


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
    n = mass.size
    windows = []
    total = args.warmup + args.reps * args.steps
    with S.SPH(n, p, mode=S.MODE_FULL_FAST) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setTiming(S.TIMING_OFF)
        if args.child in ("scalars", "scalars1"):
            T = np.zeros((n, 4), np.float32)
            T[:, 0] = pos.reshape(-1, 3)[:, 1]
            sph.setScalars(T, [scenes.scalar_stable_kappa(p, 0.1), 0.0, 0.0, 0.0])
        every = EVERY.get(args.child)
        if every:
            sph.recordMonitor(total // every + 1, every=every)
        sph.run(args.warmup)
        sph.synchronize()
        for _ in range(args.reps):
            t0 = time.perf_counter()
            sph.run(args.steps)
            sph.synchronize()
            windows.append((time.perf_counter() - t0) / args.steps * 1e3)
        part = sph.getParticles()
        assert np.isfinite(part.mPosition).all()
        neighbours = float(part.mNeighborCount.mean())
        rows, said = 0, ""
        if every:
            rec = sph.getMonitorRecord()
            rows = len(rec)
            assert rows == (total - 1) // every + 1 and (rec.live == n).all() and (rec.bad == 0).all()
            # what the rows say about the run that was timed
            said = "courant %.3g, accel number %.3g" % (rec.courant(p).max(), rec.accel_number(p).max())
            if rec.has_diffusion.any():
                kappa = [scenes.scalar_stable_kappa(p, 0.1), 0.0, 0.0, 0.0]
                worst = rec.diffusion_number(kappa, p.time_step)[:, 0]
                first = rec.first_bad()
                said += ", diffusion number %.3g .. %.3g, first bad row %s" % (
                    np.nanmin(worst), np.nanmax(worst), "none" if first is None else
                    "%d (step %d: scalar_bad %d, pair_bad %d)" % (first, rec.steps[first], rec.scalar_bad[first],
                                                                    rec.pair_bad[first]))
    print("RESULT " + json.dumps({"windows": windows, "neighbours": neighbours, "rows": rows, "said": said}), flush=True)


def measure(variant, args):
    env = dict(os.environ)
    env.pop("SPH_HIP_LIBRARY", None)
    if variant == "parent":
        env["SPH_HIP_LIBRARY"] = os.path.abspath(args.parent)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", variant, "--particles", str(args.particles),
           "--warmup", str(args.warmup), "--steps", str(args.steps), "--reps", str(args.reps)]
    run = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
    if run.returncode != 0:             # a child that fails ends the run, with what it said
        sys.exit("child %s ended with status %d\n%s%s" % (variant, run.returncode, run.stdout, run.stderr))
    line = [ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")][-1]
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
    ap.add_argument("--child", default=None, choices=list(VARIANTS), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    runs = [r for r in VARIANTS if args.parent or r != "parent"]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("step monitor cost: %d-particle dam column, FULL_FAST; %d rounds, the variants taking turns; per child %d "
        "warm-up steps, then %d windows of %d steps" % (args.particles, args.rounds, args.warmup, args.reps, args.steps))
    windows = {r: [] for r in runs}
    neighbours, rows, said = {}, {}, {}
    for _ in range(args.rounds):
        for r in runs:
            got = measure(r, args)      # a child that fails ends the run: nothing more is started
            windows[r] += got["windows"]
            neighbours[r] = got["neighbours"]
            rows[r] = got["rows"]
            said[r] = got["said"]
    med = {r: statistics.median(windows[r]) for r in runs}
    base = runs[0]
    for r in runs:
        say("%-8s best %8.4f ms/step %6.3fx   median %8.4f ms/step %6.3fx   (windows %.4f .. %.4f)   rows %d" %
            (r, min(windows[r]), min(windows[r]) / min(windows[base]), med[r], med[r] / med[base], min(windows[r]),
             max(windows[r]), rows[r]))
    if args.parent:
        pw = windows["parent"]
        spread = max(pw) - min(pw)
        diff = med["none"] - med["parent"]
        say("no recording, beside the parent (structural: no existing kernel differs, the same launches): this tree's "
            "median %.4f, the parent's %.4f, %+.4f ms/step; the parent's own windows spread %.4f ms/step: %s" %
            (med["none"], med["parent"], diff, spread, "inside it" if abs(diff) <= spread else "OUTSIDE it"))
    particles = med["every1"] - med["none"]
    byte_ms = args.particles * STREAMED_BYTES / HBM_BYTES_PER_MS
    say("k_monitor_particles and k_monitor_finish (every = 1 minus no recording): median %+.4f ms/step, best %+.4f "
        "ms/step; %d bytes streamed per particle are %.4f ms at 8 TB/s: %.1f times its byte time" %
        (particles, min(windows["every1"]) - min(windows["none"]), STREAMED_BYTES, byte_ms, particles / byte_ms))
    say("every = 10 minus no recording: median %+.4f ms/step (a tenth of the above is %+.4f)" %
        (med["every10"] - med["none"], particles / 10.0))
    with_pairs = med["scalars1"] - med["scalars"]
    say("with scalars, every = 1 minus no recording: median %+.4f ms/step; less the particle kernel, k_monitor_pairs "
        "alone %+.4f ms/step beside k_cohesion_apply's %+.2f" % (with_pairs, with_pairs - particles, COHESION_MS))
    for r in runs:
        if said[r]:
            say("the rows of %s: %s" % (r, said[r]))
    say("neighbours per particle at the end of a run: " + ", ".join("%s %.2f" % (r, neighbours[r]) for r in runs))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
