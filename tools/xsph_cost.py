"""What XSPH velocity smoothing (include/sph_hip.h: xsph) costs: the 4M-particle FULL_FAST dam column
(scenes.dam_break), four variants taking turns in child processes (tools/cohesion_cost.py's protocol):
    parent    the library of the parent commit (--parent PATH: libsph_hip.so built from it), no smoothing
    none      this tree's library, no smoothing: the same kernels as the parent's
              (tools/kernel_isa_diff.py shows only k_xsph_stage, k_xsph_apply and their descriptors as new)
    unfused   the same with SPH_HIP_NO_FUSED_INTEGRATE=1: the separate integrate kernel, which a smoothing step takes
    xsph      this tree's library with eps = --eps: every step gives up the fused integrate and runs k_xsph_stage and
              k_xsph_apply.  The pair kernel's gathers do not depend on the velocities, its store does: a particle
              whose change is zero is not stored, and the column at rest would store nothing.  So every variant
              starts from the column with a seeded velocity noise of --speed per component (scenes.dam_break's
              speed), small enough that the column keeps its neighbour count over the run (reported per variant);
              the run ends with an error unless the smoothing left less velocity noise than the plain run.
Each child builds the scene, warms up, and times windows of queued steps between two synchronisations; the variants
take turns over several rounds and every window is kept.  Reported: best and median ms/step per variant; `none`
beside `parent` with the parent's own window spread (a structural statement - a context without the smoothing
enqueues the parent's launches - with the two times recorded beside it); what giving up the fused integrate costs
(`unfused` minus `none`); and the kernel pair alone (`xsph` minus `unfused`) beside what it gathers: 32 bytes per
neighbour, where cohesion's kernel gathers 16 and costs +0.257 ms (profiles/cohesion_cost.txt) and the scalar pass
gathers 36 and costs +0.74 ms.

    timeout -k 10 1100 python tools/xsph_cost.py --parent /path/to/parent/libsph_hip.so \
        --out profiles/xsph_cost.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sph_hip_set_xsph", "sph_hip_get_xsph")
VARIANTS = ("parent", "none", "unfused", "xsph")
GATHER_BYTES = 32              # posm[q] and R[q] per neighbour
COHESION_GATHER_BYTES = 16     # posm[q]: cohesion's kernel
COHESION_MS = 0.2569           # profiles/cohesion_cost.txt: k_cohesion_apply alone, median
SCALAR_GATHER_BYTES = 36       # posm[q], Ts[q], Vs[q]: the scalar pass
SCALAR_PASS_MS = 0.74


def child(args):
    sys.path.insert(0, ROOT)
    from smoothed_particle_hydrodynamics_amd import lib as B
    if args.child == "parent":
        for name in NEW_SYMBOLS:          # the parent's library does not export them
            B.PROTOTYPES.pop(name)
    import numpy as np

    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dam_break(args.particles, speed=args.speed)
    n = mass.size
    windows = []
    with S.SPH(n, p, mode=S.MODE_FULL_FAST) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setTiming(S.TIMING_OFF)
        if args.child == "xsph":
            sph.setVelocitySmoothing(args.eps)
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
        speed = float(np.sqrt((part.mVelocity.astype(np.float64) ** 2).mean()))
        if args.child == "xsph":
            assert sph.getVelocitySmoothing() != 0.0
    print("RESULT " + json.dumps({"windows": windows, "neighbours": neighbours, "speed": speed}), flush=True)


def measure(variant, args):
    env = dict(os.environ)
    for name in ("SPH_HIP_LIBRARY", "SPH_HIP_NO_FUSED_INTEGRATE"):
        env.pop(name, None)
    if variant == "parent":
        env["SPH_HIP_LIBRARY"] = os.path.abspath(args.parent)
    if variant == "unfused":
        env["SPH_HIP_NO_FUSED_INTEGRATE"] = "1"
    cmd = [sys.executable, os.path.abspath(__file__), "--child", variant, "--particles", str(args.particles),
           "--warmup", str(args.warmup), "--steps", str(args.steps), "--reps", str(args.reps), "--eps", str(args.eps),
           "--speed", str(args.speed)]
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
    ap.add_argument("--eps", type=float, default=0.5)
    ap.add_argument("--speed", type=float, default=0.01, help="the velocity noise every variant starts from")
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

    say("xsph cost: %d-particle dam column, FULL_FAST, velocity noise %.3g, eps = %.3g; %d rounds, the variants taking "
        "turns; per child %d warm-up steps, then %d windows of %d steps" %
        (args.particles, args.speed, args.eps, args.rounds, args.warmup, args.reps, args.steps))
    windows = {r: [] for r in runs}
    neighbours, speed = {}, {}
    for _ in range(args.rounds):
        for r in runs:
            got = measure(r, args)      # a child that fails ends the run: nothing more is started
            windows[r] += got["windows"]
            neighbours[r] = got["neighbours"]
            speed[r] = got["speed"]
    if not speed["xsph"] < speed["none"]:
        sys.exit("the smoothing did not act: rms velocity component %g with it, %g without" % (speed["xsph"], speed["none"]))
    med = {r: statistics.median(windows[r]) for r in runs}
    base = runs[0]
    for r in runs:
        say("%-8s best %8.4f ms/step %6.3fx   median %8.4f ms/step %6.3fx   (windows %.4f .. %.4f)" %
            (r, min(windows[r]), min(windows[r]) / min(windows[base]), med[r], med[r] / med[base], min(windows[r]),
             max(windows[r])))
    if args.parent:
        pw = windows["parent"]
        say("no smoothing, beside the parent (structural: no existing kernel differs, the same launches): this tree's "
            "median %.4f, the parent's %.4f, %+.4f ms/step; the parent's own windows spread %.4f ms/step" %
            (med["none"], med["parent"], med["none"] - med["parent"], max(pw) - min(pw)))
    say("giving up the fused integrate (SPH_HIP_NO_FUSED_INTEGRATE=1 minus the default): median %+.4f ms/step, best "
        "%+.4f ms/step" % (med["unfused"] - med["none"], min(windows["unfused"]) - min(windows["none"])))
    kernel = med["xsph"] - med["unfused"]
    say("k_xsph_stage and k_xsph_apply alone (xsph minus SPH_HIP_NO_FUSED_INTEGRATE=1): median %+.4f ms/step, best %+.4f "
        "ms/step; %d bytes gathered per neighbour" % (kernel, min(windows["xsph"]) - min(windows["unfused"]), GATHER_BYTES))
    say("neighbours per particle at the end of a run: " + ", ".join("%s %.2f" % (r, neighbours[r]) for r in runs))
    say("rms velocity component at the end of a run: " + ", ".join("%s %.4g" % (r, speed[r]) for r in runs))
    say("beside cohesion's kernel (%d bytes per neighbour, +%.3f ms/step): %.2f of its gathered bytes, %.2f of its time" %
        (COHESION_GATHER_BYTES, COHESION_MS, GATHER_BYTES / COHESION_GATHER_BYTES, kernel / COHESION_MS))
    say("beside the scalar pass (%d bytes per neighbour, +%.2f ms/step): %.2f of its gathered bytes, %.2f of its time" %
        (SCALAR_GATHER_BYTES, SCALAR_PASS_MS, GATHER_BYTES / SCALAR_GATHER_BYTES, kernel / SCALAR_PASS_MS))
    say("smoothing on, whole step: median %+.4f ms/step over the default route without it" % (med["xsph"] - med["none"]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
