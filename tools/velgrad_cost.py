"""What the velocity-gradient pass (include/sph_hip.h: velocity gradients) costs: the 4M-particle FULL_FAST dam column
(scenes.dam_break), three variants taking turns in child processes of one session (tools/cohesion_cost.py's protocol).
Every variant is one public call that synchronises, repeated on the same warmed-up state:
    build     sph_hip_voxelize: the cell build every call below runs first, alone
    density   sph_hip_sample_pressure_points with one probe: the cell build, k_particle_density's stand-alone call, and
              a one-probe sampler launch
    velgrad   sph_hip_sample_velocity_gradients_points with one probe, group 0: the cell build, k_velgrad_particles, and
              the same one-probe sampler launch
Each child builds the scene, steps the warm-up, and times windows of repeated calls between two readings of the clock;
the variants take turns over several rounds and every window is kept.  Reported: best and median ms/call per variant;
the pass with the cell build (velgrad) and without it (velgrad minus build), beside k_particle_density likewise
(density minus build), their ratio, and the mean neighbour count.  The pass walks the same rows as the density
kernel and gathers 16 more bytes (velp[q]) for members only.

    timeout -k 10 500 python tools/velgrad_cost.py --out profiles/velgrad_cost.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("build", "density", "velgrad")


def child(args):
    sys.path.insert(0, ROOT)
    import numpy as np

    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dam_break(args.particles)
    n = mass.size
    probe = np.ascontiguousarray(pos.reshape(-1, 3)[n // 2:n // 2 + 1], np.float32)
    out4 = np.zeros((1, 4), np.float32)
    out1 = np.zeros(1, np.float32)
    cnt = np.zeros(1, np.int32)
    windows = []
    with S.SPH(n, p, mode=S.MODE_FULL_FAST) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setTiming(S.TIMING_OFF)
        sph.run(args.warmup)
        sph.synchronize()

        def call():
            if args.child == "build":
                sph.call("sph_hip_voxelize")
                sph.synchronize()
            elif args.child == "density":
                sph.call("sph_hip_sample_pressure_points", 1, probe.ctypes.data, out1.ctypes.data, None, cnt.ctypes.data)
            else:
                sph.call("sph_hip_sample_velocity_gradients_points", 1, probe.ctypes.data, 0, out4.ctypes.data, None,
                         cnt.ctypes.data)

        for _ in range(3):      # the first call allocates
            call()
        for _ in range(args.reps):
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call()
            windows.append((time.perf_counter() - t0) / args.calls * 1e3)
        part = sph.getParticles()
        assert np.isfinite(part.mPosition).all()
        neighbours = float(part.mNeighborCount.mean())
        if args.child == "velgrad":
            assert cnt[0] > 0 and np.isfinite(out4).all()
    print("RESULT " + json.dumps({"windows": windows, "neighbours": neighbours}), flush=True)


def measure(variant, args):
    env = dict(os.environ)
    env.pop("SPH_HIP_LIBRARY", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", variant, "--particles", str(args.particles), "--warmup",
           str(args.warmup), "--calls", str(args.calls), "--reps", str(args.reps)]
    run = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
    if run.returncode != 0:             # a child that fails ends the run, with what it said
        sys.exit("child %s ended with status %d\n%s%s" % (variant, run.returncode, run.stdout, run.stderr))
    line = [ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=4 * 1024 * 1024)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child-timeout", type=float, default=240.0)
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--child", default=None, choices=list(VARIANTS), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("velocity-gradient cost: %d-particle dam column, FULL_FAST; %d rounds, the variants taking turns; per child %d "
        "warm-up steps, then %d windows of %d calls" % (args.particles, args.rounds, args.warmup, args.reps, args.calls))
    windows = {r: [] for r in VARIANTS}
    neighbours = {}
    for _ in range(args.rounds):
        for r in VARIANTS:
            got = measure(r, args)      # a child that fails ends the run: nothing more is started
            windows[r] += got["windows"]
            neighbours[r] = got["neighbours"]
    med = {r: statistics.median(windows[r]) for r in VARIANTS}
    best = {r: min(windows[r]) for r in VARIANTS}
    for r in VARIANTS:
        say("%-8s best %8.4f ms/call   median %8.4f ms/call   (windows %.4f .. %.4f)" %
            (r, best[r], med[r], min(windows[r]), max(windows[r])))
    say("the pass with its cell build: median %.4f ms/call, best %.4f" % (med["velgrad"], best["velgrad"]))
    pass_med, pass_best = med["velgrad"] - med["build"], best["velgrad"] - best["build"]
    rho_med, rho_best = med["density"] - med["build"], best["density"] - best["build"]
    say("k_velgrad_particles alone (velgrad minus build): median %+.4f ms, best %+.4f ms" % (pass_med, pass_best))
    say("k_particle_density alone (density minus build):  median %+.4f ms, best %+.4f ms" % (rho_med, rho_best))
    say("the pass over the density kernel: median %.2fx, best %.2fx (both minus the build; each with a one-probe sampler "
        "launch)" % (pass_med / rho_med, pass_best / rho_best))
    say("neighbours per particle at the end of a run: " + ", ".join("%s %.2f" % (r, neighbours[r]) for r in VARIANTS))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
