"""What drawing the solids adds to a rendered frame (include/sph_hip.h: sph_hip_render_scene against
sph_hip_render) on two scenes with solids in them: scenes.dam_break_pillar at 4M particles and
scenes.dam_break_debris (FULL_FAST, as the scenes set gravity and walls).

  * 1280 x 720, a camera framing the box, step = grad_step = h / 2, refine = 8,
    iso = half the median density the sampler gives at every 7th particle;
  * the same context, the same state, the same process: sph_hip_render, then sph_hip_render_scene.

Per scene: warm up, then the median of --reps frames of each entry point, each timed with a host clock
around the synchronising call with every output NULL (the device's frame: cell build, occupancy map,
march, shade, and for the scene call the list upload and k_scene_solids).  --frames DIR writes each
scene's frame with solids as PNG there.  One process; it starts no GPU children.  The solids kernel
alone comes from a run of its own under rocprofv3:

    timeout -k 10 900 python tools/scene_render_cost.py --out profiles/scene_render_cost.txt --frames /tmp/frames
    timeout -k 10 900 rocprofv3 --kernel-trace --stats -d /tmp/rp -- python tools/scene_render_cost.py --reps 3
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
from smoothed_particle_hydrodynamics_amd.lib import SphSceneParams  # noqa: E402

F32 = np.float32


def median_ms(fn, reps):
    fn()   # warm: scratch allocation, first launch of each kernel
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=4 * 1024 * 1024, help="of the pillar scene")
    ap.add_argument("--debris-particles", type=int, default=1024 * 1024)
    ap.add_argument("--steps", type=int, default=100, help="steps before the frames are taken")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--frames", default=None, help="write the frames as PNG into this directory")
    args = ap.parse_args()
    W, H = 1280, 720
    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    cases = [("pillar", scenes.dam_break_pillar(args.particles)), ("debris", scenes.dam_break_debris(args.debris_particles))]
    for name, scene in cases:
        p, pos, vel, mass, obst = scene[:5]
        box = np.array([p.max_x, p.max_y, p.max_z], np.float64)
        c = 0.5 * box
        cam = S.Camera.look_at(c + np.array([1.1, 0.6, 1.5]) * box.max(), c, (0, 1, 0), 45, W, H)
        with S.SPH(mass.size, p, mode=S.MODE_FULL_FAST, device=0) as sph:
            sph.setParticles(pos, vel, mass)
            sph.setObstacles(obst)
            if name == "debris":
                sph.setBodies(scene[5])
            sph.setTiming(S.TIMING_OFF)
            sph.run(args.steps)
            spos = sph.syncParticles().mPosition.reshape(-1, 3)
            rho = sph.sampleFields(spos[::7], velocity=False)[0]
            iso = float(F32(0.5) * np.median(rho[rho > 0]))
            lib, ctx = sph._lib, sph._ctx
            camS, rp = cam.as_struct(), sph.renderParams(iso)
            sp = SphSceneParams()
            sp.albedo[:] = [0.72, 0.72, 0.72]
            sp.ambient, sp.diffuse = 0.2, 0.8

            def fluid():
                if lib.sph_hip_render(ctx, C.byref(camS), C.byref(rp), W, H, 0, None, None, None, None, None) != 0:
                    raise RuntimeError(lib.sph_hip_last_error(ctx).decode())

            def scene_frame():
                if lib.sph_hip_render_scene(ctx, C.byref(camS), C.byref(rp), C.byref(sp), None, 0, W, H, 0, None, None,
                                            None, None, None, None) != 0:
                    raise RuntimeError(lib.sph_hip_last_error(ctx).decode())

            ms_fluid = median_ms(fluid, args.reps)
            ms_scene = median_ms(scene_frame, args.reps)
            ms_fluid2 = median_ms(fluid, args.reps)      # again: what two runs of the same call differ by
            fr = sph.render(cam, W, H, iso, solids=True)
            solid = int((fr.solid_id >= 0).sum())
            if args.frames:
                os.makedirs(args.frames, exist_ok=True)
                S.write_png(os.path.join(args.frames, "%s_solids.png" % name), fr.rgba)
            results.append({"scene": name, "particles": int(mass.size), "steps": args.steps, "solid_pixels": solid,
                            "fluid_pixels": int((fr.first_inside >= 0).sum()), "render_ms": round(ms_fluid, 3),
                            "render_again_ms": round(ms_fluid2, 3), "render_scene_ms": round(ms_scene, 3),
                            "added_ms": round(ms_scene - ms_fluid, 3)})
            say("%-7s %8d particles, step %d: sph_hip_render %8.3f ms (again %8.3f)  sph_hip_render_scene %8.3f ms  "
                "added %+.3f ms  solid pixels %d" % (name, mass.size, args.steps, ms_fluid, ms_fluid2, ms_scene,
                                                     ms_scene - ms_fluid, solid))
    say("(%dx%d, every output NULL, median of %d frames per entry point, one context per scene)" % (W, H, args.reps))
    say(json.dumps(results))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
