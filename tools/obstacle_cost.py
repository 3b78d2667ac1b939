"""What static obstacles (include/sph_hip.h: sph_hip_set_obstacles) cost per step on bench.py's 4M dam
column at rest (FULL_FAST, as bench.py's headline): 0, 1, 8 and 64 obstacles downstream of the column,
plus the obstacle-free step on the unfused route (SPH_HIP_NO_FUSED_INTEGRATE=1: a k_integrate launch
behind the acceleration pass, the route a context with obstacles takes) - the difference between that
row and the 0 row is what an obstacle-aware fused route could save at most.

Per case: one context, --warmup steps, then the mean of --steps steps queued back to back and timed with
a host clock around them (best of --reps).  One process; it starts no GPU children.

    timeout -k 10 900 python tools/obstacle_cost.py --out profiles/obstacle_cost.txt
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import smoothed_particle_hydrodynamics_amd as S  # noqa: E402
from smoothed_particle_hydrodynamics_amd import obstacles as O  # noqa: E402
from smoothed_particle_hydrodynamics_amd import scenes  # noqa: E402


def obstacle_field(k, seed=3):
    """k obstacles (cycling sphere, box, cylinder) in x in [0.2, 0.95] - downstream of the column"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(k):
        c = (rng.uniform(0.2, 0.95), rng.uniform(0.05, 0.9), rng.uniform(0.05, 0.95))
        s = rng.uniform(0.02, 0.06)
        if i % 3 == 0:
            out.append(O.Sphere(c, s))
        elif i % 3 == 1:
            out.append(O.Box((c[0] - s, c[1] - s, c[2] - s), (c[0] + s, c[1] + s, c[2] + s)))
        else:
            out.append(O.Cylinder(1, c, s, -1.0, 2.0))
    return out


def time_case(n, k, warmup, steps, reps, unfused=False):
    p, pos, vel, mass = scenes.dam_break(n)
    if unfused:
        os.environ["SPH_HIP_NO_FUSED_INTEGRATE"] = "1"
    try:
        sph = S.SPH(n, p, mode=S.MODE_FULL_FAST)
    finally:
        os.environ.pop("SPH_HIP_NO_FUSED_INTEGRATE", None)
    with sph:
        sph.setParticles(pos, vel, mass)
        sph.setObstacles(obstacle_field(k))
        sph.setTiming(S.TIMING_OFF)
        sph.run(warmup)
        sph.synchronize()
        best = float("inf")
        for _ in range(reps):
            t0 = time.perf_counter()
            sph.run(steps)
            sph.synchronize()
            best = min(best, (time.perf_counter() - t0) / steps * 1e3)
        x = sph.getParticles().mPosition
        assert np.isfinite(x).all()
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=4 * 1024 * 1024)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    os.environ.pop("SPH_HIP_NO_FUSED_INTEGRATE", None)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n = args.particles
    say("obstacle cost: %d-particle dam column at rest, FULL_FAST, best of %d x %d steps after %d warm-up"
        % (n, args.reps, args.steps, args.warmup))
    base = time_case(n, 0, args.warmup, args.steps, args.reps)
    say("%-34s %8.4f ms/step  %5.3fx" % ("0 obstacles (fused integrate)", base, 1.0))
    unf = time_case(n, 0, args.warmup, args.steps, args.reps, unfused=True)
    say("%-34s %8.4f ms/step  %5.3fx" % ("0 obstacles, unfused integrate", unf, unf / base))
    for k in (1, 8, 64):
        t = time_case(n, k, args.warmup, args.steps, args.reps)
        say("%-34s %8.4f ms/step  %5.3fx" % ("%d obstacle%s" % (k, "" if k == 1 else "s"), t, t / base))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
