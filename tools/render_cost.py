"""What a rendered frame costs (include/sph_hip.h: sph_hip_render) on bench.py's 4M dam: the column at
rest and the breaking dam at step 510 (FULL_FAST, gravity and walls on, as bench.py runs it).

  * 1280 x 720, a camera framing the box, step = grad_step = h / 2, refine = 8,
    iso = half the median density the sampler gives at every 7th particle;
  * with and without velocity, on the default route and with SPH_HIP_RENDER_NOSKIP=1 (a context of
    its own, the switch is read at creation).

Per case: warm up, then the median of --reps frames, each timed with a host clock around the
synchronising call with every output NULL (the device's frame: cell build, occupancy map, march,
shade), and the same end to end through SPH.render (rgba, depth, normal, first_inside copied to
numpy).  --frames DIR writes each case's frame as PNG there.  One process; it starts no GPU children.
The per-kernel split comes from a run of its own under rocprofv3:

    timeout -k 10 900 python tools/render_cost.py --out profiles/render_cost.txt --frames /tmp/frames
    timeout -k 10 900 rocprofv3 --kernel-trace --stats -d /tmp/rp -- python tools/render_cost.py --reps 3
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
    fn()   # warm: scratch and occupancy allocation, first launch of each kernel
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=4 * 1024 * 1024)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--steps", type=int, default=510, help="steps of the breaking dam")
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--frames", default=None, help="write the frames as PNG into this directory")
    args = ap.parse_args()
    os.environ.pop("SPH_HIP_RENDER_NOSKIP", None)
    W, H = 1280, 720
    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    p, pos, vel, mass = scenes.dam_break(args.particles)
    p.apply_gravity = 1
    p.apply_walls = 1
    p.gravity[0], p.gravity[1], p.gravity[2] = 0.0, -9.81, 0.0
    box = np.array([p.max_x, p.max_y, p.max_z], np.float64)
    c = 0.5 * box
    cam = S.Camera.look_at(c + np.array([1.1, 0.6, 1.5]) * box.max(), c, (0, 1, 0), 45, W, H)
    say("scene: dam, %d particles, h = %.6g; %dx%d, camera framing the box, step = grad_step = h/2, refine = 8"
        % (mass.size, p.h, W, H))
    # the two states: at rest and after --steps steps, each rendered on both routes
    sph = S.SPH(mass.size, p, mode=S.MODE_FULL_FAST, device=0)
    states = []
    try:
        sph.setParticles(pos, vel, mass)
        sph.setTiming(S.TIMING_OFF)
        part = sph.syncParticles()
        states.append(("column at rest", part.mPosition.copy(), part.mVelocity.copy()))
        sph.run(args.steps)
        part = sph.syncParticles()
        states.append(("dam, step %d" % args.steps, part.mPosition.copy(), part.mVelocity.copy()))
    finally:
        sph.close()
    for name, spos, svel in states:
        for noskip in (False, True):
            if noskip:
                os.environ["SPH_HIP_RENDER_NOSKIP"] = "1"
            sph = S.SPH(mass.size, p, mode=S.MODE_FULL_FAST, device=0)
            os.environ.pop("SPH_HIP_RENDER_NOSKIP", None)
            try:
                sph.setParticles(spos, svel, mass)
                rho = sph.sampleFields(spos.reshape(-1, 3)[::7], velocity=False)[0]
                iso = float(F32(0.5) * np.median(rho[rho > 0]))
                lib, ctx = sph._lib, sph._ctx
                for velocity in (False, True):
                    camS, rp = cam.as_struct(), sph.renderParams(iso)

                    def frame():
                        rc = lib.sph_hip_render(ctx, C.byref(camS), C.byref(rp), W, H, 1 if velocity else 0,
                                                None, None, None, None, None)
                        if rc != 0:
                            raise RuntimeError(lib.sph_hip_last_error(ctx).decode())

                    ms = median_ms(frame, args.reps)
                    e2e = median_ms(lambda: sph.render(cam, W, H, iso, velocity=velocity), max(3, args.reps // 3))
                    fr = sph.render(cam, W, H, iso, velocity=velocity)
                    hits = int((fr.first_inside >= 0).sum())
                    route = "noskip" if noskip else "default"
                    if args.frames:
                        os.makedirs(args.frames, exist_ok=True)
                        S.write_png(os.path.join(args.frames, "%s_%s%s.png" % (
                            name.replace(" ", "_").replace(",", ""), route, "_vel" if velocity else "")), fr.rgba)
                    results.append({"state": name, "route": route, "velocity": velocity, "hit_pixels": hits,
                                    "frame_ms": round(ms, 3), "ns_per_pixel": round(ms * 1e6 / (W * H), 2),
                                    "ns_per_hit_pixel": round(ms * 1e6 / max(hits, 1), 2),
                                    "end_to_end_ms": round(e2e, 3)})
                    r = results[-1]
                    say("%-16s %-8s vel=%-5s hits %7d  frame %8.3f ms  %7.2f ns/pixel  e2e %8.3f ms" % (
                        name, route, velocity, hits, ms, r["ns_per_pixel"], e2e))
            finally:
                sph.close()
    say("(frame: sph_hip_render with every output NULL, median of %d; target <= 16.7 ms for the column at rest)"
        % args.reps)
    say(json.dumps(results))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
