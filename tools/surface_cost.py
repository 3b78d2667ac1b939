"""What the iso-surface extractor costs on the 4M dam column (bench.py's C3 scene), next to the field
sampler's end-to-end cost for the same lattice in the same process (FULL_FAST, as bench.py runs it).

  * lattices of 128^3 and 256^3 points spanning the particles' bounding box, and h/4 apart inside
    the column, each with and without normals (velocity is not asked for);
  * iso = half the median of the positive densities of a 64^3 lattice over the bounding box,
    after 10 steps.

Device time is split three ways from phases timed the same way (median of --reps calls, each ended
by a synchronise): the cell build alone (sph_hip_voxelize), the cell build plus the sampling of the
whole lattice (sph_hip_sample_lattice with every output NULL), and the whole extraction
(sph_hip_extract_surface); meshing = extraction - sampling, sampling = sampling - build.  The
extraction samples its slabs' halo planes once more, so "meshing" includes that re-sampling and
the per-slab synchronisation.  "end to end" is SPH.extractSurface (mesh copied to numpy) against
SPH.sampleLattice (density, velocity and count copied to numpy).
One process; it starts no GPU children.

    timeout -k 10 600 python tools/surface_cost.py --out profiles/surface_cost.txt
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
    fn()   # warm: scratch and mesh allocation, first launch of each kernel
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
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    os.environ.pop("SPH_HIP_SURFACE_PLANES", None)
    os.environ.pop("SPH_HIP_SAMPLE_TILED", None)

    p, pos, vel, mass = scenes.dam_break(args.particles)
    n = mass.size
    lo, hi = pos.reshape(-1, 3).min(0), pos.reshape(-1, 3).max(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sph = S.SPH(n, p, mode=S.MODE_FULL_FAST, device=0)
    results = []
    try:
        sph.setParticles(pos, vel, mass)
        lib, ctx = sph._lib, sph._ctx
        sph.run(10)
        # half the median density of the fluid on a coarse lattice over the bounding box
        m = 64
        coarse = sph.sampleLattice(tuple(float(v) for v in lo), tuple(float(v) for v in (hi - lo) / F32(m - 1)),
                                   (m, m, m), velocity=False)[0]
        iso = float(F32(0.5) * np.median(coarse[coarse > 0]))
        say("scene: dam column, %d particles, h = %.6g; bounding box %s .. %s; iso = %.6g" %
            (n, p.h, np.round(lo, 4).tolist(), np.round(hi, 4).tolist(), iso))

        def build():
            check(lib.sph_hip_voxelize(ctx), "voxelize")
            check(lib.sph_hip_synchronize(ctx), "synchronize")

        build_ms = median_ms(build, args.reps)
        say("cell build alone (sph_hip_voxelize + synchronise): %.3f ms" % build_ms)
        h = F32(p.h)
        cases = [("lattice %d^3" % m, (m, m, m), tuple(float(v) for v in lo),
                  tuple(float(v) for v in (hi - lo) / F32(m - 1))) for m in (128, 256)]
        cases += [("inside, h/4", (64, 256, 256), (0.002, 0.05, 0.1), (float(h / F32(4)),) * 3)]
        for name, shape, origin, spacing in cases:
            o, s, d = (C.c_float * 3)(*origin), (C.c_float * 3)(*spacing), (C.c_int32 * 3)(*shape)

            def sample():
                check(lib.sph_hip_sample_lattice(ctx, C.byref(o), C.byref(s), C.byref(d), None, None, None),
                      "sample_lattice")

            sample_ms = median_ms(sample, args.reps)
            sample_e2e = median_ms(lambda: sph.sampleLattice(origin, spacing, shape), max(3, args.reps // 2))
            for normals in (False, True):
                counts = (C.c_int32 * 2)()

                def extract():
                    check(lib.sph_hip_extract_surface(ctx, C.byref(o), C.byref(s), C.byref(d), C.c_float(iso),
                                                      1 if normals else 0, C.byref(counts)), "extract_surface")

                ext_ms = median_ms(extract, args.reps)
                e2e = median_ms(lambda: sph.extractSurface(origin, spacing, shape, iso, normals=normals),
                                max(3, args.reps // 2))
                samp = sample_ms - build_ms
                mesh = ext_ms - sample_ms
                results.append({"case": name, "normals": normals, "points": shape[0] * shape[1] * shape[2],
                                "V": counts[0], "T": counts[1], "build_ms": round(build_ms, 3),
                                "sampling_ms": round(samp, 3), "meshing_ms": round(mesh, 3),
                                "meshing_vs_sampling": round(mesh / samp, 3), "extract_device_ms": round(ext_ms, 3),
                                "extract_end_to_end_ms": round(e2e, 3), "sample_end_to_end_ms": round(sample_e2e, 3),
                                "e2e_ratio": round(e2e / sample_e2e, 3)})
    finally:
        sph.close()

    say("")
    say("%-14s %-7s %10s %9s %9s %8s %9s %9s %7s %10s %10s %10s %7s" % (
        "case", "normals", "points", "V", "T", "build", "sampling", "meshing", "m/s", "extract", "ext e2e",
        "sample e2e", "e2e/s"))
    for r in results:
        say("%-14s %-7s %10d %9d %9d %8.3f %9.3f %9.3f %7.3f %10.3f %10.3f %10.3f %7.3f" % (
            r["case"], "yes" if r["normals"] else "no", r["points"], r["V"], r["T"], r["build_ms"],
            r["sampling_ms"], r["meshing_ms"], r["meshing_vs_sampling"], r["extract_device_ms"],
            r["extract_end_to_end_ms"], r["sample_end_to_end_ms"], r["e2e_ratio"]))
    say("(ms; m/s = meshing / sampling, target <= 0.2; e2e/s = extractSurface / sampleLattice end to end, "
        "target <= 0.25 with normals on 256^3)")
    say("")
    say(json.dumps({"build_ms": round(build_ms, 3), "cases": results}))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
