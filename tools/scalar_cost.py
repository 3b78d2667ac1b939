"""What carried scalars (include/sph_hip.h: carried scalars) cost: the 4M-particle FULL_FAST dam column
(scenes.dam_break) with

    parent   the library of the parent commit (--parent PATH: libsph_hip.so built from it), no scalars
    none     this tree's library, no scalars: the same kernels as the parent's (tools/kernel_isa_diff.py), and a
             step launches nothing new
    lists    this tree's library with four channels set, diffusivities (0, k, 2k, k) and two sources: every step
             runs k_scalars_stage and k_scalars_step, the lanes walking their neighbour lists (the default route)
    rows     the same with SPH_HIP_SCALAR_ROWS=1: every lane walks the nine cell rows as k_particle_density does

One child process per measurement (a library is loaded, and the route switch read, once per process), the variants
taking turns --rounds times in one session; this process never opens the GPU, and every child runs under its own
time limit (--child-timeout).  A child runs --warmup steps, then --reps windows of --steps steps queued back to
back, each timed with a host clock around the window and a synchronise.  Reported: the best and the median window
per variant in ms per step; the condition - `none` against `parent`, within the spread of the parent's own windows;
and the added ms per step of the two routes over `none`, as measured (no bar is fixed for them).

    timeout -k 10 1100 python tools/scalar_cost.py --parent /path/to/parent/libsph_hip.so \
        --out profiles/scalar_cost.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sph_hip_set_scalars", "sph_hip_get_scalars", "sph_hip_set_scalar_sources", "sph_hip_get_scalar_sources",
               "sph_hip_sample_scalars_points", "sph_hip_sample_scalars_lattice")
VARIANTS = ("parent", "none", "lists", "rows")


def child(args):
    sys.path.insert(0, ROOT)
    from smoothed_particle_hydrodynamics_amd import lib as B
    if args.child == "parent":
        for name in NEW_SYMBOLS:          # the parent's library does not export them
            B.PROTOTYPES.pop(name)
    import numpy as np

    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import ScalarSource, scenes
    p, pos, vel, mass = scenes.dam_break(args.particles)
    n = mass.size
    windows = []
    changed, finite = 0.0, 1.0
    with S.SPH(n, p, mode=S.MODE_FULL_FAST) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setTiming(S.TIMING_OFF)
        if args.child in ("lists", "rows"):
            values = np.zeros((n, 4), np.float32)
            values[:, 0] = np.arange(n, dtype=np.float32)
            values[:, 1:] = (pos.reshape(-1, 3)[:, 1:2] > 0.4).astype(np.float32)
            # (a small diffusivity: the column is a random fill that relaxes, and next to a particle of its spray,
            # whose density is next to nothing and whose volume m / rho is huge, no step is convex - DESIGN.md 26)
            k = scenes.scalar_stable_kappa(p, 0.01)
            sph.setScalars(values, [0.0, k, 2.0 * k, k])
            sph.setScalarSources([ScalarSource.hold((-1.0, -1.0, -1.0), (2.0, 0.05, 2.0), 1, 1.0),
                                  ScalarSource.add((-1.0, 0.6, -1.0), (2.0, 2.0, 2.0), 2, 5.0)])
        sph.run(args.warmup)
        sph.synchronize()
        for _ in range(args.reps):
            t0 = time.perf_counter()
            sph.run(args.steps)
            sph.synchronize()
            windows.append((time.perf_counter() - t0) / args.steps * 1e3)
        if args.child in ("lists", "rows"):
            got = sph.getScalars()
            assert np.array_equal(got[:, 0], values[:, 0])          # the carried channel: its row numbers
            changed = float((got[:, 1] != values[:, 1]).mean())
            finite = float(np.isfinite(got).all(1).mean())
            assert changed > 0.01
        assert np.isfinite(sph.getParticles().mPosition).all()
    print("RESULT " + json.dumps({"windows": windows, "changed": changed, "finite": finite}), flush=True)


def measure(variant, args):
    env = dict(os.environ)
    env.pop("SPH_HIP_LIBRARY", None)
    env.pop("SPH_HIP_SCALAR_ROWS", None)
    if variant == "parent":
        env["SPH_HIP_LIBRARY"] = os.path.abspath(args.parent)
    if variant == "rows":
        env["SPH_HIP_SCALAR_ROWS"] = "1"
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

    say("scalar cost: %d-particle dam column, FULL_FAST; %d rounds, the variants taking turns; per child %d warm-up "
        "steps, then %d windows of %d steps; scalars: four channels, diffusivities (0, k, 2k, k), two sources" %
        (args.particles, args.rounds, args.warmup, args.reps, args.steps))
    windows = {r: [] for r in runs}
    changed, finite = {}, {}
    for _ in range(args.rounds):
        for r in runs:
            got = measure(r, args)      # a child that fails ends the run: nothing more is started
            windows[r] += got["windows"]
            changed[r] = got["changed"]
            finite[r] = got["finite"]
    med = {r: statistics.median(windows[r]) for r in runs}
    base = runs[0]
    for r in runs:
        say("%-8s best %8.4f ms/step %6.3fx   median %8.4f ms/step %6.3fx   (windows %.4f .. %.4f)" %
            (r, min(windows[r]), min(windows[r]) / min(windows[base]), med[r], med[r] / med[base], min(windows[r]),
             max(windows[r])))
    if args.parent:
        pw = windows["parent"]
        spread = max(pw) - min(pw)
        diff = med["none"] - med["parent"]
        side = "within" if abs(diff) <= spread else "OUTSIDE, this tree faster" if diff < 0 else "OUTSIDE, this tree slower"
        say("condition, no scalars: this tree's median %.4f minus the parent's %.4f = %+.4f ms/step; the parent's own "
            "windows spread %.4f ms/step: %s" % (med["none"], med["parent"], diff, spread, side))
    nw = windows["none"]
    for r, what in (("lists", "the list route (default)"), ("rows", "the row walk (SPH_HIP_SCALAR_ROWS=1)")):
        say("scalars on, %s: median minus the median without scalars %+.4f ms/step, best minus best %+.4f ms/step (the "
            "windows without scalars spread %.4f ms/step); %.1f %% of the particles changed a diffusing channel, %.4f %% "
            "of the rows are finite at the end" %
            (what, med[r] - med["none"], min(windows[r]) - min(nw), max(nw) - min(nw), 100.0 * changed[r], 100.0 * finite[r]))
    say("the list route %s the row walk by %.4f ms/step (medians)" %
        ("beats" if med["lists"] < med["rows"] else "DOES NOT beat", abs(med["rows"] - med["lists"])))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
