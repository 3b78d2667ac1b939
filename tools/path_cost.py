"""What a motion path (include/sph_hip.h: sph_hip_set_obstacle_paths) costs per step: the 4M-particle FULL_FAST
dam column of scenes.dam_break_pillar - walls on, the pillar in place, so every variant integrates in a kernel
of its own behind the acceleration pass - with

    parent   the library of the parent commit (--parent PATH: libsph_hip.so built from it), which has no
             paths: k_integrate_obst
    static   this tree's library, the pillar static: k_integrate_obst, the same code as the parent's
             (tools/kernel_isa_diff.py)
    motion   this tree's library with the pillar on a Motion across the surge (--velocity, position units
             per unit of time_step, along +z): k_integrate_obst_moving
    path     this tree's library with the pillar on a 64-key cyclic sine along z of the amplitude that gives
             the Motion's peak speed: k_paths_eval (one wave) + k_integrate_obst_path

One child process per measurement (a library is loaded once per process), each under its own time limit, the
variants taking turns --rounds times in one session; this process never opens the GPU.  A child runs --warmup
steps, then --reps windows of --steps steps queued back to back, each timed with a host clock around the
window and a synchronise.  Reported: the best and the median window per variant over all rounds, in ms per
step, the ratios to the first variant, and path minus motion in microseconds per step - the expectation is the
time of one single-wave launch.

    timeout -k 10 1100 python tools/path_cost.py --parent /path/to/parent/libsph_hip.so \
        --out profiles/path_cost.txt
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sph_hip_set_obstacle_paths", "sph_hip_get_obstacle_paths")
VARIANTS = ["parent", "static", "motion", "path"]
NAMES = {"parent": "parent library", "static": "this tree, pillar static", "motion": "this tree, pillar on a Motion",
         "path": "this tree, pillar on a 64-key sine"}


def child(args):
    sys.path.insert(0, ROOT)
    from smoothed_particle_hydrodynamics_amd import lib as B
    if args.child == "parent":
        for name in NEW_SYMBOLS:          # the parent's library does not export them
            B.PROTOTYPES.pop(name)
    import numpy as np

    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    from smoothed_particle_hydrodynamics_amd.obstacles import Motion, MotionPath
    p, pos, vel, mass, obst = scenes.dam_break_pillar(args.particles)
    windows = []
    with S.SPH(mass.size, p, mode=S.MODE_FULL_FAST) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setObstacles(obst)
        sph.setTiming(S.TIMING_OFF)
        if args.child == "motion":
            sph.setObstacleMotion([Motion((0.0, 0.0, args.velocity))])
        elif args.child == "path":
            period = 200.0 * float(p.time_step)
            sph.setObstaclePaths([MotionPath.sine((0.0, 0.0, args.velocity * period / (2.0 * math.pi)), period, 64)])
        sph.run(args.warmup)
        sph.synchronize()
        for _ in range(args.reps):
            t0 = time.perf_counter()
            sph.run(args.steps)
            sph.synchronize()
            windows.append((time.perf_counter() - t0) / args.steps * 1e3)
        clock = sph.getObstacleMotion()[1] if args.child in ("motion", "path") else 0.0
        x = sph.getParticles().mPosition
        assert np.isfinite(x).all()
    print("RESULT " + json.dumps({"windows": windows, "clock": clock}), flush=True)


def measure(variant, args):
    env = dict(os.environ)
    env.pop("SPH_HIP_LIBRARY", None)
    if variant == "parent":
        env["SPH_HIP_LIBRARY"] = os.path.abspath(args.parent)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", variant, "--particles", str(args.particles),
           "--warmup", str(args.warmup), "--steps", str(args.steps), "--reps", str(args.reps),
           "--velocity", str(args.velocity)]
    out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=args.child_timeout).stdout
    line = [ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="libsph_hip.so built from the parent commit")
    ap.add_argument("--particles", type=int, default=4 * 1024 * 1024)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--velocity", type=float, default=0.2)
    ap.add_argument("--child-timeout", type=float, default=240.0)
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--child", default=None, choices=VARIANTS, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    variants = [v for v in VARIANTS if v != "parent" or args.parent]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("path cost: %d-particle dam_break_pillar (walls, 1 cylinder), FULL_FAST; %d rounds, the variants taking "
        "turns; per child %d warm-up steps, then %d windows of %d steps; peak pillar speed %g along z" %
        (args.particles, args.rounds, args.warmup, args.reps, args.steps, args.velocity))
    windows = {v: [] for v in variants}
    clocks = {}
    for _ in range(args.rounds):
        for v in variants:
            r = measure(v, args)      # a child that fails ends the run: nothing more is started
            windows[v] += r["windows"]
            clocks[v] = r["clock"]
    base = variants[0]
    best0, med0 = min(windows[base]), statistics.median(windows[base])
    for v in variants:
        best, med = min(windows[v]), statistics.median(windows[v])
        say("%-36s best %8.4f ms/step %6.3fx   median %8.4f ms/step %6.3fx   (windows %.4f .. %.4f)" %
            (NAMES[v], best, best / best0, med, med / med0, min(windows[v]), max(windows[v])))
    say("motion clock after %d steps: motion %.6f, path %.6f" %
        (args.warmup + args.reps * args.steps, clocks["motion"], clocks["path"]))
    say("path - motion: %.2f us/step (median), %.2f us/step (best)" %
        ((statistics.median(windows["path"]) - statistics.median(windows["motion"])) * 1e3,
         (min(windows["path"]) - min(windows["motion"])) * 1e3))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
