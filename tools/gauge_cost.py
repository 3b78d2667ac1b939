"""What gauges (include/sph_hip.h: sph_hip_set_gauges) cost per step: the 4M-particle FULL_FAST dam column
(scenes.dam_break) with

    parent     the library of the parent commit (--parent PATH: libsph_hip.so built from it), which has no gauges
    none       this tree's library, no gauge set: the same kernels as the parent's (tools/kernel_isa_diff.py)
    set        this tree's library with the gauges set and no recording: a step launches nothing for them
    recorded   the same gauges with a recording of every step

The gauges: 16 columns of 256 probes up y through the column (h/2 apart, on a 4 x 4 lattice in x and z), 4 sections
of 32 x 32 probes with normal x across it (h/2 apart) and 64 points inside it: 8 256 probes per evaluation.

One child process per measurement (a library is loaded once per process), the variants taking turns --rounds times
in one session; this process never opens the GPU, and every child runs under its own time limit (--child-timeout).
A child runs --warmup steps, then --reps windows of --steps steps queued back to back, each timed with a host
clock around the window and a synchronise.  Reported: the best and the median window per variant over all rounds
in ms per step, the ratios to the parent, and the two conditions: `none` and `set` against the spread of the
parent's own windows; the cost of the recorded set per step and per probe, as measured.

    timeout -k 10 1100 python tools/gauge_cost.py --parent /path/to/parent/libsph_hip.so \
        --out profiles/gauge_cost.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sph_hip_set_gauges", "sph_hip_get_gauges", "sph_hip_read_gauges", "sph_hip_record_gauges",
               "sph_hip_get_gauge_record")
COLUMNS, COLUMN_PROBES, SECTIONS, SECTION_SIDE, POINTS = 16, 256, 4, 32, 64
PROBES = COLUMNS * COLUMN_PROBES + SECTIONS * SECTION_SIDE * SECTION_SIDE + POINTS


def gauge_set(p, n):
    import math

    from smoothed_particle_hydrodynamics_amd.gauges import ColumnGauge, PointGauge, SectionGauge
    h = float(p.h)
    s = 0.5 * h
    # half the sampler's density deep inside the column (scenes.dam_break_gauged)
    iso = 0.5 * n / (0.1 * 0.75 * 1.0) * float(p.kernel1) * float(p.sim_scale) ** 6 * h ** 9 * 64.0 * math.pi / 315.0
    gauges = []
    for i in range(4):
        for j in range(4):
            gauges.append(ColumnGauge((0.0125 + 0.025 * i, 0.0, 0.125 + 0.25 * j), 1, s, COLUMN_PROBES, iso))
    for i in range(SECTIONS):
        gauges.append(SectionGauge((0.02 + 0.02 * i, 0.1 + 0.1 * i, 0.1 + 0.2 * i), 0, (s, s), (SECTION_SIDE, SECTION_SIDE), iso))
    for i in range(POINTS):
        gauges.append(PointGauge((0.01 + 0.08 * (i % 8) / 8.0, 0.05 + 0.65 * (i // 8) / 8.0, 0.03 + 0.9 * ((i * 37) % 64) / 64.0)))
    assert len(gauges) == COLUMNS + SECTIONS + POINTS
    return gauges


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
    windows, wet = [], 0
    total = args.warmup + args.reps * args.steps
    with S.SPH(mass.size, p, mode=S.MODE_FULL_FAST) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setTiming(S.TIMING_OFF)
        if args.child in ("set", "recorded"):
            sph.setGauges(gauge_set(p, args.particles))
        if args.child == "recorded":
            sph.recordGauges(total)
        sph.run(args.warmup)
        sph.synchronize()
        for _ in range(args.reps):
            t0 = time.perf_counter()
            sph.run(args.steps)
            sph.synchronize()
            windows.append((time.perf_counter() - t0) / args.steps * 1e3)
        if args.child == "recorded":
            rec = sph.getGaugeRecord()
            assert rec.steps.tolist() == list(range(total)) and np.isfinite(rec.v).all()
            wet = int(rec.n[:, :COLUMNS + SECTIONS].sum())
        if args.child == "set":
            assert len(sph.getGaugeRecord().steps) == 0
        assert np.isfinite(sph.getParticles().mPosition).all()
    print("RESULT " + json.dumps({"windows": windows, "wet": wet}), flush=True)


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
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child-timeout", type=float, default=240.0)
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--child", default=None, choices=["parent", "none", "set", "recorded"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    runs = (["parent"] if args.parent else []) + ["none", "set", "recorded"]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("gauge cost: %d-particle dam column, FULL_FAST; %d rounds, the variants taking turns; per child %d warm-up "
        "steps, then %d windows of %d steps; the gauges: %d columns x %d probes, %d sections x %d, %d points = %d probes" %
        (args.particles, args.rounds, args.warmup, args.reps, args.steps, COLUMNS, COLUMN_PROBES, SECTIONS,
         SECTION_SIDE * SECTION_SIDE, POINTS, PROBES))
    windows = {r: [] for r in runs}
    wet = 0
    for _ in range(args.rounds):
        for r in runs:
            got = measure(r, args)      # a child that fails ends the run: nothing more is started
            windows[r] += got["windows"]
            wet = got["wet"] or wet
    base = runs[0]
    med = {r: statistics.median(windows[r]) for r in runs}
    for r in runs:
        say("%-9s best %8.4f ms/step %6.3fx   median %8.4f ms/step %6.3fx   (windows %.4f .. %.4f)" %
            (r, min(windows[r]), min(windows[r]) / min(windows[base]), med[r], med[r] / med[base], min(windows[r]),
             max(windows[r])))
    if args.parent:
        pw = windows["parent"]
        spread = max(pw) - min(pw)
        for r in ("none", "set"):
            diff = med[r] - med["parent"]
            say("condition, %s: this tree's median %.4f minus the parent's %.4f = %+.4f ms/step; the parent's own windows "
                "spread %.4f ms/step: %s" % ("no gauges" if r == "none" else "gauges set, no recording", med[r],
                                             med["parent"], diff, spread, "within" if abs(diff) <= spread else "OUTSIDE"))
    cost = med["recorded"] - med["none"]
    nw = windows["none"]
    say("recorded every step: median minus the median without gauges %+.4f ms/step (the windows without gauges spread "
        "%.4f ms/step) = %.3f ns per probe over %d probes; %d wet probes counted over the run" %
        (cost, max(nw) - min(nw), cost * 1e6 / PROBES, PROBES, wet))
    say("for comparison, the sampler (profiles/sample_cost.txt): 0.17 ns per coherent probe, 2.36 ns per unordered "
        "probe; a gauge is one wave, %d waves in %d workgroups per evaluation" %
        (COLUMNS + SECTIONS + POINTS, (COLUMNS + SECTIONS + POINTS + 3) // 4))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
