"""What a free body (include/sph_hip.h: sph_hip_set_bodies) costs per step: the 4M-particle FULL_FAST dam column
of scenes.dam_break_pillar - walls on, the pillar in place, so every variant integrates in a kernel of its own
behind the acceleration pass - with

    parent   the library of the parent commit (--parent PATH: libsph_hip.so built from it), which has no
             bodies: k_integrate_obst
    static   this tree's library, no body set: k_integrate_obst, the same code as the parent's
             (tools/kernel_isa_diff.py)
    body     this tree's library with the pillar a heavy body (--mass-ratio times the fluid a pillar of the
             column's height displaces), free along the surge axis: k_bodies_advance, one wave, and
             k_integrate_bodies, which records every wall and obstacle response into an internal row

One child process per measurement (a library is loaded once per process), the variants taking turns
--rounds times in one session; this process never opens the GPU, and every child runs under its own time
limit (--child-timeout).  A child runs --warmup steps, then --reps windows of --steps steps queued back to
back, each timed with a host clock around the window and a synchronise.  Reported: the best and the median
window per variant over all rounds, in ms per step, and the ratios to the parent.  A body-to-parent ratio
above 1.05 is flagged.

    timeout -k 10 1100 python tools/body_cost.py --parent /path/to/parent/libsph_hip.so \
        --out profiles/body_cost.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sph_hip_set_bodies", "sph_hip_get_bodies")


def child(args):
    sys.path.insert(0, ROOT)
    from smoothed_particle_hydrodynamics_amd import lib as B
    if args.child == "parent":
        for name in NEW_SYMBOLS:          # the parent's library does not export them
            B.PROTOTYPES.pop(name)
    import numpy as np

    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    from smoothed_particle_hydrodynamics_amd.obstacles import Body
    p, pos, vel, mass, obst = scenes.dam_break_pillar(args.particles)
    windows = []
    with S.SPH(mass.size, p, mode=S.MODE_FULL_FAST) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setObstacles(obst)
        sph.setTiming(S.TIMING_OFF)
        if args.child == "body":
            # the fluid a pillar as tall as the column displaces, at the column's density
            displaced = mass.size / (0.1 * 0.75 * 1.0) * 3.141592653589793 * float(obst[0].radius) ** 2 * 0.75
            sph.setBodies([Body(args.mass_ratio * displaced, free=(True, False, False), travel_lo=(0.0, 0.0, 0.0),
                                travel_hi=(0.4, 0.0, 0.0))])
        sph.run(args.warmup)
        sph.synchronize()
        for _ in range(args.reps):
            t0 = time.perf_counter()
            sph.run(args.steps)
            sph.synchronize()
            windows.append((time.perf_counter() - t0) / args.steps * 1e3)
        moved, skipped = 0.0, 0
        if args.child == "body":
            got = sph.getBodies()
            moved, skipped = float(got.displacement[0, 0]), int(got.skipped[0])
            assert int(got.steps[0]) == args.warmup + args.reps * args.steps
        x = sph.getParticles().mPosition
        assert np.isfinite(x).all()
    print("RESULT " + json.dumps({"windows": windows, "moved": moved, "skipped": skipped}), flush=True)


def measure(variant, args):
    env = dict(os.environ)
    env.pop("SPH_HIP_LIBRARY", None)
    if variant == "parent":
        env["SPH_HIP_LIBRARY"] = os.path.abspath(args.parent)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", variant, "--particles", str(args.particles),
           "--warmup", str(args.warmup), "--steps", str(args.steps), "--reps", str(args.reps),
           "--mass-ratio", str(args.mass_ratio)]
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
    ap.add_argument("--mass-ratio", type=float, default=8.0)
    ap.add_argument("--child-timeout", type=float, default=240.0)
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--child", default=None, choices=["parent", "static", "body"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    variants = (["parent"] if args.parent else []) + ["static", "body"]
    names = {"parent": "parent library", "static": "this tree, static pillar", "body": "this tree, pillar a body"}
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("free body cost: %d-particle dam_break_pillar (walls, 1 cylinder), FULL_FAST; %d rounds, the variants "
        "taking turns; per child %d warm-up steps, then %d windows of %d steps; the body %g times the fluid it displaces" %
        (args.particles, args.rounds, args.warmup, args.reps, args.steps, args.mass_ratio))
    windows = {v: [] for v in variants}
    moved, skipped = 0.0, 0
    for _ in range(args.rounds):
        for v in variants:
            r = measure(v, args)      # a child that fails ends the run: nothing more is started
            windows[v] += r["windows"]
            if v == "body":
                moved, skipped = r["moved"], r["skipped"]
    base = variants[0]
    best0, med0 = min(windows[base]), statistics.median(windows[base])
    for v in variants:
        best, med = min(windows[v]), statistics.median(windows[v])
        say("%-26s best %8.4f ms/step %6.3fx   median %8.4f ms/step %6.3fx   (windows %.4f .. %.4f)" %
            (names[v], best, best / best0, med, med / med0, min(windows[v]), max(windows[v])))
    say("the body's displacement after %d steps: %.6g (responses skipped: %d)" %
        (args.warmup + args.reps * args.steps, moved, skipped))
    ratio = statistics.median(windows["body"]) / med0
    say("body / %s (median): %.3fx%s" % (names[base], ratio, "  ABOVE 1.05x" if ratio > 1.05 else ""))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
