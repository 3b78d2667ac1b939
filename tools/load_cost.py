"""What a load recording (include/sph_hip.h: sph_hip_record_loads) costs per step: the 4M-particle
FULL_FAST dam column of scenes.dam_break_pillar - walls on, the pillar in place, so every variant
integrates in a kernel of its own behind the acceleration pass - with

    parent         the library of the parent commit (--parent PATH: libsph_hip.so built from it), which
                   has no recording: k_integrate_obst
    recording off  this tree's library, nothing recorded: k_integrate_obst, the same code as the parent's
    recording on   this tree's library with a row per step: k_integrate_loads

One child process per measurement (a library is loaded once per process), the variants taking turns
--rounds times in one session; this process never opens the GPU.  A child runs --warmup steps, then
--reps windows of --steps steps queued back to back, each timed with a host clock around the window and
a synchronise; every variant steps through the same states.  Reported: the best and the median window
per variant over all rounds, in ms per step, and the ratios to the parent.

    timeout -k 10 1100 python tools/load_cost.py --parent /path/to/parent/libsph_hip.so \
        --out profiles/load_cost.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sph_hip_record_loads", "sph_hip_get_loads")


def child(args):
    sys.path.insert(0, ROOT)
    from smoothed_particle_hydrodynamics_amd import lib as B
    if args.child == "parent":
        for name in NEW_SYMBOLS:          # the parent's library does not export them
            B.PROTOTYPES.pop(name)
    import numpy as np

    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass, obst = scenes.dam_break_pillar(args.particles)
    windows = []
    with S.SPH(mass.size, p, mode=S.MODE_FULL_FAST) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setObstacles(obst)
        sph.setTiming(S.TIMING_OFF)
        if args.child == "on":
            sph.recordLoads(args.warmup + args.reps * args.steps)
        sph.run(args.warmup)
        sph.synchronize()
        for _ in range(args.reps):
            t0 = time.perf_counter()
            sph.run(args.steps)
            sph.synchronize()
            windows.append((time.perf_counter() - t0) / args.steps * 1e3)
        responses = skipped = -1
        if args.child == "on":
            loads = sph.getLoads()
            assert loads.count.shape[0] == args.warmup + args.reps * args.steps
            responses, skipped = int(loads.count.sum()), int(loads.skipped.sum())
        x = sph.getParticles().mPosition
        assert np.isfinite(x).all()
    print("RESULT " + json.dumps({"windows": windows, "responses": responses, "skipped": skipped}), flush=True)


def measure(variant, args):
    env = dict(os.environ)
    env.pop("SPH_HIP_LIBRARY", None)
    if variant == "parent":
        env["SPH_HIP_LIBRARY"] = os.path.abspath(args.parent)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", variant, "--particles", str(args.particles),
           "--warmup", str(args.warmup), "--steps", str(args.steps), "--reps", str(args.reps)]
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
    ap.add_argument("--child-timeout", type=float, default=240.0)
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--child", default=None, choices=["parent", "off", "on"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    variants = (["parent"] if args.parent else []) + ["off", "on"]
    names = {"parent": "parent library", "off": "this tree, recording off", "on": "this tree, recording on"}
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("load recording cost: %d-particle dam_break_pillar (walls, 1 cylinder), FULL_FAST; %d rounds, the variants "
        "taking turns; per child %d warm-up steps, then %d windows of %d steps" %
        (args.particles, args.rounds, args.warmup, args.reps, args.steps))
    windows = {v: [] for v in variants}
    responses = skipped = 0
    for _ in range(args.rounds):
        for v in variants:
            r = measure(v, args)      # a child that fails ends the run: nothing more is started
            windows[v] += r["windows"]
            if v == "on":
                responses, skipped = r["responses"], r["skipped"]
    base = variants[0]
    best0, med0 = min(windows[base]), statistics.median(windows[base])
    for v in variants:
        best, med = min(windows[v]), statistics.median(windows[v])
        say("%-26s best %8.4f ms/step %6.3fx   median %8.4f ms/step %6.3fx   (windows %.4f .. %.4f)" %
            (names[v], best, best / best0, med, med / med0, min(windows[v]), max(windows[v])))
    say("recorded: %d responses in %d steps, %d skipped" % (responses, args.warmup + args.reps * args.steps, skipped))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
