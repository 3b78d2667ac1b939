"""What the wedge kind (include/sph_hip.h: SPH_HIP_OBSTACLE_WEDGE) costs the obstacle route per step, on
bench.py's 4M dam column at rest (FULL_FAST) behind tools/obstacle_cost.py's first sphere, box and cylinder:

  (a) a library built from the parent commit (--parent-lib), on that three-obstacle list
  (b) this tree's library on the same list - the wedge branch is compiled in and never taken
  (c) this tree's library with one floor ramp (obstacles.Wedge.ramp) added to the list

Every measurement is a child process of its own (the library is chosen by SPH_HIP_LIBRARY before the package
loads it), under its own `timeout`; the variants take turns for --rounds rounds, and the first child that
fails ends the run: nothing is started after it.  A child warms up, then times --windows windows of --steps
steps queued back to back with a host clock around each.  Per variant: the median, lowest and highest window.
The condition on (b): its median may exceed (a)'s by no more than (a)'s own spread (highest - lowest window)
in this session.  (c) is recorded, not bounded.

    python tools/wedge_cost.py --parent-lib PATH/libsph_hip.so --out profiles/wedge_cost.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(args):
    import numpy as np

    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import obstacles as O
    from smoothed_particle_hydrodynamics_amd import scenes
    from tools.obstacle_cost import obstacle_field
    p, pos, vel, mass = scenes.dam_break(args.particles)
    obst = obstacle_field(3)
    if args.ramp:
        obst.append(O.Wedge.ramp((0.3, 0.0, -0.1), (0.9, 0.25, 1.1), 0, 1))
    with S.SPH(args.particles, p, mode=S.MODE_FULL_FAST) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setObstacles(obst)
        sph.setTiming(S.TIMING_OFF)
        sph.run(args.warmup)
        sph.synchronize()
        windows = []
        for _ in range(args.windows):
            t0 = time.perf_counter()
            sph.run(args.steps)
            sph.synchronize()
            windows.append((time.perf_counter() - t0) / args.steps * 1e3)
        assert np.isfinite(sph.getParticles().mPosition).all()
    print(json.dumps({"windows_ms": windows}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=4 * 1024 * 1024)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds a child may take")
    ap.add_argument("--parent-lib", default=None, help="libsph_hip.so built from the parent commit")
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--ramp", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        ap.error("--parent-lib must name a library built from the parent commit")
    variants = [("a parent library, sphere + box + cylinder", args.parent_lib, False),
                ("b this tree, the same list", None, False),
                ("c this tree, the list + one ramp", None, True)]
    got = {name: [] for name, _, _ in variants}
    for r in range(args.rounds):
        for name, lib, ramp in variants:
            env = dict(os.environ)
            env.pop("SPH_HIP_LIBRARY", None)
            if lib:
                env["SPH_HIP_LIBRARY"] = os.path.abspath(lib)
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child",
                   "--particles", str(args.particles), "--warmup", str(args.warmup), "--steps", str(args.steps),
                   "--windows", str(args.windows)] + (["--ramp"] if ramp else [])
            run = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT)
            if run.returncode != 0:
                print(run.stdout + run.stderr)
                print("round %d, %s: exit status %d - nothing more is started" % (r, name, run.returncode))
                return 1
            got[name] += json.loads(run.stdout.strip().splitlines()[-1])["windows_ms"]
            print("round %d  %-44s %s" % (r, name, " ".join("%.4f" % w for w in got[name][-args.windows:])), flush=True)
    lines = ["wedge cost: %d-particle dam column at rest, FULL_FAST, %d rounds x %d windows of %d steps after %d warm-up,"
             % (args.particles, args.rounds, args.windows, args.steps, args.warmup),
             "one child process per variant and round, the variants taking turns; ms/step",
             "%-46s %9s %9s %9s" % ("variant", "median", "lowest", "highest")]
    med = {}
    for name, _, _ in variants:
        w = got[name]
        med[name] = statistics.median(w)
        lines.append("%-46s %9.4f %9.4f %9.4f" % (name, med[name], min(w), max(w)))
    a, b, c = (name for name, _, _ in variants)
    spread = max(got[a]) - min(got[a])
    ok = med[b] - med[a] <= spread
    lines.append("(b) - (a) medians: %+.4f ms/step; (a)'s own spread: %.4f ms/step: %s" %
                 (med[b] - med[a], spread, "within it" if ok else "NOT within it"))
    lines.append("(c) - (b) medians: %+.4f ms/step (recorded, not bounded)" % (med[c] - med[b]))
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
