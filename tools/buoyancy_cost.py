"""What buoyancy (include/sph_hip.h: buoyancy) costs: the 4M-particle FULL_FAST dam column (scenes.dam_break) with
carried scalars - four channels, diffusivities (0, k, 2k, k), two sources, as tools/scalar_cost.py sets them - and

    parent    the library of the parent commit (--parent PATH: libsph_hip.so built from it), scalars, no buoyancy
    none      this tree's library, scalars, no buoyancy: the same kernels as the parent's
              (tools/kernel_isa_diff.py), and a step launches what the parent's launches
    unfused   the same with SPH_HIP_NO_FUSED_INTEGRATE=1: the separate integrate kernel, which a buoyant step takes
    buoyancy  this tree's library with a Buoyancy on the carried channel 0 (1 above y = 0.4, 0 below; beta 0.05):
              every step gives up the fused integrate and runs k_buoyancy_apply

One child process per measurement (a library is loaded, and the route switch read, once per process), the variants
taking turns --rounds times in one session; this process never opens the GPU, and every child runs under its own
time limit (--child-timeout).  A child runs --warmup steps, then --reps windows of --steps steps queued back to
back, each timed with a host clock around the window and a synchronise.  Reported: the best and the median window
per variant in ms per step; `none` beside `parent` (a structural condition - no existing kernel differs and a step
without buoyancy enqueues the parent's launches - with the two times recorded beside it); what giving up the fused
integrate costs (`unfused` minus `none`); and the kernel alone (`buoyancy` minus `unfused`) beside its traffic floor
of 80 bytes per particle at --copy-gbs, the float4-copy rate DESIGN.md section 22 records.  No bar is fixed.

    timeout -k 10 1100 python tools/buoyancy_cost.py --parent /path/to/parent/libsph_hip.so \
        --out profiles/buoyancy_cost.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sph_hip_set_buoyancy", "sph_hip_get_buoyancy")
VARIANTS = ("parent", "none", "unfused", "buoyancy")
BYTES_PER_PARTICLE = 80        # three 16-byte loads and two 16-byte stores per lane


def child(args):
    sys.path.insert(0, ROOT)
    from smoothed_particle_hydrodynamics_amd import lib as B
    if args.child == "parent":
        for name in NEW_SYMBOLS:          # the parent's library does not export them
            B.PROTOTYPES.pop(name)
    import numpy as np

    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import Buoyancy, ScalarSource, scenes
    p, pos, vel, mass = scenes.dam_break(args.particles)
    n = mass.size
    windows = []
    with S.SPH(n, p, mode=S.MODE_FULL_FAST) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setTiming(S.TIMING_OFF)
        values = np.zeros((n, 4), np.float32)
        values[:, 0] = (pos.reshape(-1, 3)[:, 1] > 0.4).astype(np.float32)
        values[:, 1:] = values[:, 0:1]
        k = scenes.scalar_stable_kappa(p, 0.01)      # (small: tools/scalar_cost.py says why)
        sph.setScalars(values, [0.0, k, 2.0 * k, k])
        sph.setScalarSources([ScalarSource.hold((-1.0, -1.0, -1.0), (2.0, 0.05, 2.0), 1, 1.0),
                              ScalarSource.add((-1.0, 0.6, -1.0), (2.0, 2.0, 2.0), 2, 5.0)])
        if args.child == "buoyancy":
            sph.setBuoyancy(Buoyancy(0.05, 0.0, (0.0, -9.81, 0.0)))
        sph.run(args.warmup)
        sph.synchronize()
        for _ in range(args.reps):
            t0 = time.perf_counter()
            sph.run(args.steps)
            sph.synchronize()
            windows.append((time.perf_counter() - t0) / args.steps * 1e3)
        got = sph.getScalars()
        assert np.array_equal(got[:, 0], values[:, 0])          # the carried channel
        assert np.isfinite(sph.getParticles().mPosition).all()
        if args.child == "buoyancy":
            assert sph.getBuoyancy() is not None
    print("RESULT " + json.dumps({"windows": windows, "lifted": float(values[:, 0].mean())}), flush=True)


def measure(variant, args):
    env = dict(os.environ)
    for name in ("SPH_HIP_LIBRARY", "SPH_HIP_SCALAR_ROWS", "SPH_HIP_NO_FUSED_INTEGRATE"):
        env.pop(name, None)
    if variant == "parent":
        env["SPH_HIP_LIBRARY"] = os.path.abspath(args.parent)
    if variant == "unfused":
        env["SPH_HIP_NO_FUSED_INTEGRATE"] = "1"
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
    ap.add_argument("--copy-gbs", type=float, default=6290.0,
                    help="the float4-copy rate in GB/s the traffic floor is priced at (DESIGN.md section 22: 6.29 TB/s)")
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

    say("buoyancy cost: %d-particle dam column, FULL_FAST, scalars on in every variant (four channels, diffusivities "
        "(0, k, 2k, k), two sources); %d rounds, the variants taking turns; per child %d warm-up steps, then %d windows "
        "of %d steps" % (args.particles, args.rounds, args.warmup, args.reps, args.steps))
    windows = {r: [] for r in runs}
    lifted = 0.0
    for _ in range(args.rounds):
        for r in runs:
            got = measure(r, args)      # a child that fails ends the run: nothing more is started
            windows[r] += got["windows"]
            lifted = got["lifted"]
    med = {r: statistics.median(windows[r]) for r in runs}
    base = runs[0]
    for r in runs:
        say("%-8s best %8.4f ms/step %6.3fx   median %8.4f ms/step %6.3fx   (windows %.4f .. %.4f)" %
            (r, min(windows[r]), min(windows[r]) / min(windows[base]), med[r], med[r] / med[base], min(windows[r]),
             max(windows[r])))
    if args.parent:
        pw = windows["parent"]
        say("no buoyancy, beside the parent (structural: no existing kernel differs, the same launches): this tree's "
            "median %.4f, the parent's %.4f, %+.4f ms/step; the parent's own windows spread %.4f ms/step" %
            (med["none"], med["parent"], med["none"] - med["parent"], max(pw) - min(pw)))
    say("giving up the fused integrate (SPH_HIP_NO_FUSED_INTEGRATE=1 minus the default): median %+.4f ms/step, best "
        "%+.4f ms/step" % (med["unfused"] - med["none"], min(windows["unfused"]) - min(windows["none"])))
    kernel = med["buoyancy"] - med["unfused"]
    say("k_buoyancy_apply alone (buoyancy minus SPH_HIP_NO_FUSED_INTEGRATE=1): median %+.4f ms/step, best %+.4f ms/step; "
        "%.1f %% of the particles carry an excess and are stored" %
        (kernel, min(windows["buoyancy"]) - min(windows["unfused"]), 100.0 * lifted))
    mb = BYTES_PER_PARTICLE * args.particles / 1e6
    say("traffic floor: %d bytes per particle, %.1f MB, at %.0f GB/s %.4f ms" %
        (BYTES_PER_PARTICLE, mb, args.copy_gbs, mb / args.copy_gbs))
    say("buoyancy on, whole step: median %+.4f ms/step over the default route without it" % (med["buoyancy"] - med["none"]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
