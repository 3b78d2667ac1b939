"""What pressure readings (include/sph_hip.h: pressure readings) cost: the 4M-particle FULL_FAST dam column
(scenes.dam_break) with

    parent        the library of the parent commit (--parent PATH: libsph_hip.so built from it), no gauges
    none          this tree's library, no gauge set: the same kernels as the parent's (tools/kernel_isa_diff.py)
    set           this tree's library with tools/gauge_cost.py's field gauges set and no recording: a step launches
                  nothing for them
    parent_field  the parent's library with tools/gauge_cost.py's field gauges, recorded every step
    field         this tree's library with the same field gauges recorded: k_gauges_read alone, nothing new launched
    pressure      this tree's library with 64 pressure points and 4 patches of 32 x 32 probes, recorded every step:
                  k_gauges_pressure behind every step's density pass

and, in a child of its own, samplePressureLattice beside sampleLattice on a 128^3 lattice over the column, with the
density kernel's share (a one-probe samplePressure against a one-probe sampleFields: both run the cell build, the
first also k_particle_density over every particle).

One child process per measurement (a library is loaded once per process), the stepping variants taking turns
--rounds times in one session; this process never opens the GPU, and every child runs under its own time limit
(--child-timeout).  A stepping child runs --warmup steps, then --reps windows of --steps steps queued back to back,
each timed with a host clock around the window and a synchronise.  Reported: the best and the median window per
variant in ms per step, and the conditions - `none` and `set` against `parent`, within the spread of the parent's
own windows (they launch nothing new), and `field` against `parent_field` (the one existing kernel whose code
changed, k_gauges_read) with the side it falls on; the cost of the recorded pressure set per step and per probe,
as measured (no bar is fixed for it).

    timeout -k 10 1100 python tools/pressure_cost.py --parent /path/to/parent/libsph_hip.so \
        --out profiles/pressure_cost.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sph_hip_sample_pressure_points", "sph_hip_sample_pressure_lattice")
POINTS, PATCHES, PATCH_SIDE = 64, 4, 32
PROBES = POINTS + PATCHES * PATCH_SIDE * PATCH_SIDE
LATTICE = 128
STEPPING = ("parent", "none", "set", "parent_field", "field", "pressure")


def pressure_set(p, n):
    import math

    from smoothed_particle_hydrodynamics_amd.gauges import PressureGauge, PressurePatch
    h = float(p.h)
    s = 0.5 * h
    # half the sampler's density deep inside the column (scenes.dam_break_gauged); half of that again on the walls
    iso = 0.5 * n / (0.1 * 0.75 * 1.0) * float(p.kernel1) * float(p.sim_scale) ** 6 * h ** 9 * 64.0 * math.pi / 315.0
    gauges = [PressureGauge((0.0, 0.01 + 0.7 * i / POINTS, 0.03 + 0.9 * ((i * 37) % 64) / 64.0)) for i in range(POINTS)]
    side = (PATCH_SIDE, PATCH_SIDE)
    gauges.append(PressurePatch((0.0, 0.1, 0.1), 0, (s, s), side, 0.5 * iso))        # the wall behind the column
    gauges.append(PressurePatch((0.0, 0.3, 0.6), 0, (s, s), side, 0.5 * iso))
    gauges.append(PressurePatch((0.01, 0.0, 0.2), 1, (0.08 / (PATCH_SIDE - 1), s), side, 0.5 * iso))   # the floor
    gauges.append(PressurePatch((0.05, 0.4, 0.3), 0, (s, s), side, iso))             # a face inside the column
    assert len(gauges) == POINTS + PATCHES
    return gauges


def child_lattice(args):
    import numpy as np

    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dam_break(args.particles)
    origin, shape = (0.0, 0.0, 0.0), (LATTICE, LATTICE, LATTICE)
    spacing = (0.1 / (LATTICE - 1), 0.75 / (LATTICE - 1), 1.0 / (LATTICE - 1))
    one = np.array([[0.05, 0.3, 0.5]], np.float32)
    out = {}
    with S.SPH(mass.size, p, mode=S.MODE_FULL_FAST) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setTiming(S.TIMING_OFF)
        sph.run(args.warmup)
        sph.synchronize()
        calls = {"sampleLattice (density and count)": lambda: sph.sampleLattice(origin, spacing, shape, velocity=False),
                 "sampleLattice (with velocity)": lambda: sph.sampleLattice(origin, spacing, shape),
                 "samplePressureLattice": lambda: sph.samplePressureLattice(origin, spacing, shape),
                 "sampleFields, one probe": lambda: sph.sampleFields(one, velocity=False),
                 "samplePressure, one probe": lambda: sph.samplePressure(one)}
        for name, call in calls.items():
            call()                                   # (the first call allocates)
            times = []
            for _ in range(args.reps + 1):
                t0 = time.perf_counter()
                call()
                times.append((time.perf_counter() - t0) * 1e3)
            out[name] = times
        prs, rho, cnt = sph.samplePressureLattice(origin, spacing, shape)
        assert np.isfinite(prs).all() and cnt.any()
    print("RESULT " + json.dumps(out), flush=True)


def child(args):
    sys.path.insert(0, ROOT)
    from smoothed_particle_hydrodynamics_amd import lib as B
    if args.child.startswith("parent"):
        for name in NEW_SYMBOLS:          # the parent's library does not export them
            B.PROTOTYPES.pop(name)
    if args.child == "lattice":
        return child_lattice(args)
    import numpy as np

    import gauge_cost
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dam_break(args.particles)
    windows, wet = [], 0
    total = args.warmup + args.reps * args.steps
    with S.SPH(mass.size, p, mode=S.MODE_FULL_FAST) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setTiming(S.TIMING_OFF)
        if args.child in ("parent_field", "field", "set"):
            sph.setGauges(gauge_cost.gauge_set(p, args.particles))
        if args.child == "pressure":
            sph.setGauges(pressure_set(p, args.particles))
        if args.child not in ("parent", "none", "set"):
            sph.recordGauges(total)
        sph.run(args.warmup)
        sph.synchronize()
        for _ in range(args.reps):
            t0 = time.perf_counter()
            sph.run(args.steps)
            sph.synchronize()
            windows.append((time.perf_counter() - t0) / args.steps * 1e3)
        if args.child == "set":
            assert len(sph.getGaugeRecord().steps) == 0
        elif args.child not in ("parent", "none"):
            rec = sph.getGaugeRecord()
            assert rec.steps.tolist() == list(range(total)) and np.isfinite(rec.v).all()
            wet = int(rec.n[:, POINTS:].sum()) if args.child == "pressure" else int(rec.n.sum())
        assert np.isfinite(sph.getParticles().mPosition).all()
    print("RESULT " + json.dumps({"windows": windows, "wet": wet}), flush=True)


def measure(variant, args):
    env = dict(os.environ)
    env.pop("SPH_HIP_LIBRARY", None)
    if variant.startswith("parent"):
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
    ap.add_argument("--child", default=None, choices=list(STEPPING) + ["lattice"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    runs = [r for r in STEPPING if args.parent or not r.startswith("parent")]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("pressure cost: %d-particle dam column, FULL_FAST; %d rounds, the variants taking turns; per child %d warm-up "
        "steps, then %d windows of %d steps; the pressure set: %d points, %d patches x %d = %d probes; the field set: "
        "tools/gauge_cost.py's %d probes" %
        (args.particles, args.rounds, args.warmup, args.reps, args.steps, POINTS, PATCHES, PATCH_SIDE * PATCH_SIDE, PROBES,
         16 * 256 + 4 * 1024 + 64))
    windows = {r: [] for r in runs}
    wet = 0
    for _ in range(args.rounds):
        for r in runs:
            got = measure(r, args)      # a child that fails ends the run: nothing more is started
            windows[r] += got["windows"]
            if r == "pressure":
                wet = got["wet"] or wet
    med = {r: statistics.median(windows[r]) for r in runs}
    base = runs[0]
    for r in runs:
        say("%-12s best %8.4f ms/step %6.3fx   median %8.4f ms/step %6.3fx   (windows %.4f .. %.4f)" %
            (r, min(windows[r]), min(windows[r]) / min(windows[base]), med[r], med[r] / med[base], min(windows[r]),
             max(windows[r])))
    if args.parent:
        for r, against, what in (("none", "parent", "no gauges"), ("set", "parent", "field gauges set, no recording"),
                                 ("field", "parent_field", "field gauges recorded (k_gauges_read changed)")):
            pw = windows[against]
            spread = max(pw) - min(pw)
            diff = med[r] - med[against]
            side = "within" if abs(diff) <= spread else "OUTSIDE, this tree faster" if diff < 0 else "OUTSIDE, this tree slower"
            say("condition, %s: this tree's median %.4f minus the parent's %.4f = %+.4f ms/step; the parent's own windows "
                "spread %.4f ms/step: %s" % (what, med[r], med[against], diff, spread, side))
    cost = med["pressure"] - med["none"]
    nw = windows["none"]
    say("pressure set recorded every step: median minus the median without gauges %+.4f ms/step (the windows without "
        "gauges spread %.4f ms/step) = %.3f ns per probe over %d probes, %d trips of the longest wave; %d wet patch "
        "probes counted over the run" % (cost, max(nw) - min(nw), cost * 1e6 / PROBES, PROBES,
                                         PATCH_SIDE * PATCH_SIDE // 64, wet))
    lat = measure("lattice", args)
    best = {k: min(v) for k, v in lat.items()}
    for name, times in lat.items():
        say("%-36s best %9.3f ms   median %9.3f ms   (%d calls)" % (name, min(times), statistics.median(times), len(times)))
    share = best["samplePressure, one probe"] - best["sampleFields, one probe"]
    say("%d^3 lattice: samplePressureLattice %.3f ms beside sampleLattice %.3f ms (density and count) and %.3f ms (with "
        "velocity); the density kernel's share, one-probe samplePressure minus one-probe sampleFields: %.3f ms of it" %
        (LATTICE, best["samplePressureLattice"], best["sampleLattice (density and count)"],
         best["sampleLattice (with velocity)"], share))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
