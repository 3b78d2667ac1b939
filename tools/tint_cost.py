"""What tinting the fluid by a carried channel adds to a rendered frame (include/sph_hip.h:
sph_hip_render_scalars, SURFACE and COLUMN, against sph_hip_render) on the 4M-particle scenes.dam_break_dyed
column (FULL_FAST), at rest and --steps steps in.

  * 1280 x 720, a camera framing the box, step = grad_step = h / 2, refine = 8,
    iso = half the median density the sampler gives at every 7th particle;
  * the same context and the same state for all calls of a row: sph_hip_render, sph_hip_render_scalars
    SURFACE, sph_hip_render_scalars COLUMN, then sph_hip_render again (what two runs of one call differ by).

Per state: warm up, then the median of --reps frames of each call, each timed with a host clock around the
synchronising call with every output NULL (the device's frame: cell build, occupancy map, march, shade, and
for the scalar calls the stage, the table upload, the memset and the tint kernel).  One process; it starts no
GPU children.  The per-kernel split comes from a run of its own under rocprofv3:

    timeout -k 10 900 python tools/tint_cost.py --out profiles/tint_cost.txt
    timeout -k 10 900 rocprofv3 --kernel-trace --stats -d /tmp/rp -- python tools/tint_cost.py --reps 3
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import smoothed_particle_hydrodynamics_amd as S  # noqa: E402
from scene_render_cost import median_ms  # noqa: E402
from smoothed_particle_hydrodynamics_amd import colormaps, scenes  # noqa: E402
from smoothed_particle_hydrodynamics_amd.lib import SphTintParams  # noqa: E402

F32 = np.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=4 * 1024 * 1024)
    ap.add_argument("--steps", type=int, default=100, help="steps between the two states")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--frames", default=None, help="write the tinted frames as PNG into this directory")
    args = ap.parse_args()
    W, H = 1280, 720
    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    p, pos, vel, mass, values, kappa = scenes.dam_break_dyed(args.particles)
    box = np.array([p.max_x, p.max_y, p.max_z], np.float64)
    c = 0.5 * box
    cam = S.Camera.look_at(c + np.array([1.1, 0.6, 1.5]) * box.max(), c, (0, 1, 0), 45, W, H)
    table = colormaps.dye((0.9, 0.1, 0.2), n=16)
    with S.SPH(mass.size, p, mode=S.MODE_FULL_FAST, device=0) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setScalars(values, kappa)
        sph.setTiming(S.TIMING_OFF)
        lib, ctx = sph._lib, sph._ctx
        for state, steps in (("at rest", 0), ("%d steps in" % args.steps, args.steps)):
            if steps:
                sph.run(steps)
            spos = sph.syncParticles().mPosition.reshape(-1, 3)
            rho = sph.sampleFields(spos[::7], velocity=False)[0]
            iso = float(F32(0.5) * np.median(rho[rho > 0]))
            camS, rp = cam.as_struct(), sph.renderParams(iso)

            def fluid():
                if lib.sph_hip_render(ctx, C.byref(camS), C.byref(rp), W, H, 0, None, None, None, None, None) != 0:
                    raise RuntimeError(lib.sph_hip_last_error(ctx).decode())

            def tinted(mode, hi):
                tp = SphTintParams(0, mode, 0.0, hi, table.shape[0], 0)

                def frame():
                    if lib.sph_hip_render_scalars(ctx, C.byref(camS), C.byref(rp), None, None, 0, C.byref(tp),
                                                  table.ctypes.data_as(C.c_void_p), W, H, 0, None, None, None, None,
                                                  None, None, None) != 0:
                        raise RuntimeError(lib.sph_hip_last_error(ctx).decode())
                return frame

            ms_fluid = median_ms(fluid, args.reps)
            ms_surface = median_ms(tinted(0, 1.0), args.reps)
            ms_column = median_ms(tinted(1, 0.1), args.reps)
            ms_fluid2 = median_ms(fluid, args.reps)
            fr = sph.renderScalars(cam, W, H, iso, 0, (0.0, 0.1), table, "column")
            hits = int((fr.first_inside >= 0).sum())
            if args.frames:
                os.makedirs(args.frames, exist_ok=True)
                S.write_png(os.path.join(args.frames, "dyed_column_%d.png" % steps), fr.rgba)
                S.write_png(os.path.join(args.frames, "dyed_surface_%d.png" % steps),
                            sph.renderScalars(cam, W, H, iso, 0, (0.0, 1.0), table).rgba)
            results.append({"state": state, "particles": int(mass.size), "fluid_pixels": hits,
                            "render_ms": round(ms_fluid, 3), "render_again_ms": round(ms_fluid2, 3),
                            "surface_ms": round(ms_surface, 3), "column_ms": round(ms_column, 3),
                            "surface_added_ms": round(ms_surface - ms_fluid, 3),
                            "column_added_ms": round(ms_column - ms_fluid, 3),
                            "column_max": float(fr.scalar.max())})
            say("%-13s %8d particles: sph_hip_render %8.3f ms (again %8.3f)  SURFACE %8.3f ms (%+.3f)  COLUMN %8.3f ms "
                "(%+.3f)  fluid pixels %d" % (state, mass.size, ms_fluid, ms_fluid2, ms_surface, ms_surface - ms_fluid,
                                              ms_column, ms_column - ms_fluid, hits))
    say("(%dx%d, every output NULL, median of %d frames per call, one context)" % (W, H, args.reps))
    say(json.dumps(results))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
