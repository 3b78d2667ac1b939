"""What the field sampler costs per probe on the 4M dam column (bench.py's C3 scene), next to what the
density pass costs per particle in the same process (phaseTotals(), FULL_FAST as bench.py runs it).

  * lattices of 64^3, 128^3 and 256^3 points spanning the particles' bounding box, on the default
    route (sample_policy.h) and with SPH_HIP_SAMPLE_TILED=1 (a second context, created after the
    variable is set: the LDS tile wherever it fits);
  * lattices h/4 and h/2 apart on every axis inside the column (4M and 2M points), the same two ways;
  * 1M random points in the bounding box (sph_hip_sample_points).

Each case is timed two ways, median of --reps calls: "device" = the call with every output NULL
(cell build + sampling kernels + the final synchronise, nothing copied), from which the cell build
alone (sph_hip_voxelize + synchronise, timed the same way) is subtracted to give the kernels' ns per
probe; "end to end" = sampleLattice / sampleFields with density and velocity copied to numpy.
One process; it starts no GPU children.

    timeout -k 10 600 python tools/sample_cost.py --out profiles/sample_cost.txt
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import smoothed_particle_hydrodynamics_amd as S  # noqa: E402
from smoothed_particle_hydrodynamics_amd import scenes  # noqa: E402

F32 = np.float32


def median_ms(fn, reps):
    fn()   # warm: scratch allocation, first launch of each kernel
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed (%d)" % (what, rc))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=4 * 1024 * 1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20, help="timed steps for the density pass's cost")
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    os.environ.pop("SPH_HIP_SAMPLE_UNTILED", None)
    os.environ.pop("SPH_HIP_SAMPLE_TILED", None)

    p, pos, vel, mass = scenes.dam_break(args.particles)
    n = mass.size
    lo, hi = pos.reshape(-1, 3).min(0), pos.reshape(-1, 3).max(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sph = S.SPH(n, p, mode=S.MODE_FULL_FAST, device=0)
    sph.setParticles(pos, vel, mass)
    lib, ctx = sph._lib, sph._ctx
    sph.run(10)
    sph.synchronize()
    sph.resetTimings()
    for _ in range(args.steps):
        sph.step()
    sph.synchronize()
    ms, k = sph.phaseTotals()
    density_ns = ms[2] / k / n * 1e6
    say("scene: dam column, %d particles, h = %.6g, FULL cell edge %.6g; bounding box %s .. %s" %
        (n, p.h, 1.0 / p.full_cell_inv, np.round(lo, 4).tolist(), np.round(hi, 4).tolist()))
    say("density pass (FULL_FAST, %d steps): %.4f ms per step = %.1f ps per particle" %
        (k, ms[2] / k, density_ns * 1e3))

    def build():
        check(lib.sph_hip_voxelize(ctx), "voxelize")
        check(lib.sph_hip_synchronize(ctx), "synchronize")

    build_ms = median_ms(build, args.reps)
    say("cell build alone (sph_hip_voxelize + synchronise): %.3f ms" % build_ms)

    other = None
    results = []
    try:
        h = F32(p.h)
        cases = [("lattice %d^3" % m, (m, m, m), tuple(float(v) for v in lo),
                  tuple(float(v) for v in (hi - lo) / F32(m - 1))) for m in (64, 128, 256)]
        inside = (0.002, 0.05, 0.1)
        cases += [("inside, h/4", (64, 256, 256), inside, (float(h / F32(4)),) * 3),
                  ("inside, h/2", (32, 256, 256), inside, (float(h / F32(2)),) * 3)]
        for name, shape, origin, spacing in cases:
            o, s, d = (C.c_float * 3)(*origin), (C.c_float * 3)(*spacing), (C.c_int32 * 3)(*shape)
            cells = [round(v * float(F32(p.full_cell_inv)), 3) for v in spacing]
            for route in ("default", "tiled"):
                if route == "tiled" and other is None:
                    os.environ["SPH_HIP_SAMPLE_TILED"] = "1"
                    other = S.SPH(n, p, mode=S.MODE_FULL_FAST, device=0)
                    os.environ.pop("SPH_HIP_SAMPLE_TILED", None)
                    other.setParticles(sph.getParticles().mPosition, sph.getParticles().mVelocity, mass)
                c = sph if route == "default" else other

                def device():
                    check(c._lib.sph_hip_sample_lattice(c._ctx, C.byref(o), C.byref(s), C.byref(d), None, None, None),
                          "sample_lattice")

                dev_ms = median_ms(device, args.reps)
                e2e_ms = median_ms(lambda: c.sampleLattice(origin, spacing, shape), max(3, args.reps // 2))
                probes = shape[0] * shape[1] * shape[2]
                r = {"case": name, "route": route, "spacing_cells": cells, "probes": probes,
                     "device_ms": round(dev_ms, 3), "kernel_ns_per_probe": round((dev_ms - build_ms) / probes * 1e6, 4),
                     "end_to_end_ms": round(e2e_ms, 3)}
                results.append(r)
        rng = np.random.default_rng(1)
        pts = (lo + rng.random((args.points, 3)) * (hi - lo)).astype(F32)

        def device_points():
            check(lib.sph_hip_sample_points(ctx, args.points, pts.ctypes.data_as(C.c_void_p), None, None, None),
                  "sample_points")

        dev_ms = median_ms(device_points, args.reps)
        e2e_ms = median_ms(lambda: sph.sampleFields(pts), max(3, args.reps // 2))
        results.append({"case": "%d random points" % args.points, "route": "points", "probes": args.points,
                        "device_ms": round(dev_ms, 3),
                        "kernel_ns_per_probe": round((dev_ms - build_ms) / args.points * 1e6, 4),
                        "end_to_end_ms": round(e2e_ms, 3)})
    finally:
        if other is not None:
            other.close()
        sph.close()

    say("")
    say("%-22s %-8s %-22s %10s %12s %16s %14s %10s" % ("case", "route", "spacing (cells)", "probes", "device ms",
                                                        "kernel ns/probe", "end-to-end ms", "vs density"))
    for r in results:
        say("%-22s %-8s %-22s %10d %12.3f %16.4f %14.3f %9.2fx" % (
            r["case"], r["route"], str(r.get("spacing_cells", "")), r["probes"], r["device_ms"],
            r["kernel_ns_per_probe"], r["end_to_end_ms"], r["kernel_ns_per_probe"] / density_ns))
    say("")
    say(json.dumps({"density_ns_per_particle": round(density_ns, 5), "build_ms": round(build_ms, 3),
                    "cases": results}))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
