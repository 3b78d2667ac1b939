"""A/B of library builds on ONE box, in windows (tools/ab_variants.py gives one figure per child; this
gives the spread a difference has to be set against, laid out as profiles/gauge_cost.txt).

    tools/build_variant.sh a_parent HEAD ; tools/build_variant.sh b_new WORK
    python tools/ab_windows.py [particles] [rounds]

Every library under build/variants/*.so, taking turns, one child process per library and round: the
dam column, FULL_FAST, 200 warm-up steps, 4 windows of 50 steps (wall time of sph.run, synchronised),
then 10 instrumented steps for the density / acceleration launch times (HIP events).  The first
library in name order is the parent the others are compared with."""
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, WINDOWS, STEPS = 200, 4, 50


def child(n):
    sys.path.insert(0, ROOT)
    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dam_break(n)
    with S.SPH(n, p, mode=S.MODE_FULL_FAST) as sph:
        sph.setParticles(pos, vel, mass)
        sph.run(WARM)
        sph.synchronize()
        win = []
        for _ in range(WINDOWS):
            t0 = time.perf_counter()
            sph.run(STEPS)
            sph.synchronize()
            win.append((time.perf_counter() - t0) / STEPS * 1e3)
        sph.setTiming(S.TIMING_PHASES)
        for _ in range(10):
            sph.step()
        sph.synchronize()
        t, k = sph.phaseTotals()
    print(json.dumps({"windows_ms": win, "density_us": t[2] / k * 1e3, "accel_us": t[4] / k * 1e3,
                      "build_us": t[0] / k * 1e3}), flush=True)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4 * 1024 * 1024
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    libs = sorted(glob.glob(os.path.join(ROOT, "build", "variants", "*.so")))
    res = {os.path.basename(so)[:-3]: {"win": [], "accel": [], "density": []} for so in libs}
    for _ in range(rounds):
        for so in libs:
            env = dict(os.environ, SPH_HIP_LIBRARY=so)
            out = subprocess.run([sys.executable, __file__, "--one", str(n)], env=env, timeout=300,
                                 capture_output=True, text=True, check=True)
            r = json.loads(out.stdout.strip().splitlines()[-1])
            name = os.path.basename(so)[:-3]
            res[name]["win"] += r["windows_ms"]
            res[name]["accel"].append(r["accel_us"])
            res[name]["density"].append(r["density_us"])
            print("# %-16s windows %s  accel %.1f us  density %.1f us" % (
                name, " ".join("%.4f" % w for w in r["windows_ms"]), r["accel_us"], r["density_us"]), flush=True)
    print("%d-particle dam column, FULL_FAST; %d rounds, the variants taking turns; per child %d warm-up steps, "
          "then %d windows of %d steps, then 10 instrumented steps (launch times by HIP events)" % (
              n, rounds, WARM, WINDOWS, STEPS))
    names = list(res)
    base = res[names[0]]
    bmed, bbest = statistics.median(base["win"]), min(base["win"])
    spread = max(base["win"]) - min(base["win"])
    for name in names:
        w = res[name]["win"]
        print("%-16s best %8.4f ms/step %6.3fx   median %8.4f ms/step %6.3fx   (windows %.4f .. %.4f)   "
              "acceleration pass median %6.1f us (%s)   density pass median %6.1f us" % (
                  name, min(w), min(w) / bbest, statistics.median(w), statistics.median(w) / bmed, min(w), max(w),
                  statistics.median(res[name]["accel"]), " ".join("%.1f" % a for a in res[name]["accel"]),
                  statistics.median(res[name]["density"])))
    for name in names[1:]:
        d = statistics.median(res[name]["win"]) - bmed
        print("%s: median %.4f minus %s's %.4f = %+.4f ms/step; %s's own windows spread %.4f ms/step: %s" % (
            name, statistics.median(res[name]["win"]), names[0], bmed, d, names[0], spread,
            "a gain beyond the spread" if d < -spread else "a loss beyond the spread" if d > spread else "within"))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--one":
        child(int(sys.argv[2]))
    else:
        main()
