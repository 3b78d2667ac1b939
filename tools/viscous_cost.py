"""What the viscous stress (include/sph_hip.h: viscous stress) costs: the 4M-particle FULL_FAST dam column
(scenes.dam_break), the variants taking turns in child processes (tools/xsph_cost.py's protocol):
    parent    the library of the parent commit (--parent PATH: libsph_hip.so built from it), no setting
    none      this tree's library, no setting: the same kernels as the parent's
              (tools/kernel_isa_diff.py shows only k_viscous_stage, k_viscous_apply and their descriptors as new)
    unfused   the same with SPH_HIP_NO_FUSED_INTEGRATE=1: the separate integrate kernel, which a viscous step takes
    mu        this tree's library with a constant mu: every step gives up the fused integrate and runs
              k_viscous_stage<false> and k_viscous_apply<.., false>: 32 bytes gathered per neighbour in two streams
    scalars   mu beside carried scalars that nothing reads (one channel, diffusivity 0): what the scalar pass, which a
              law needs, costs by itself
    law       mu with a 16-key law on that channel: k_viscous_stage<true> and k_viscous_apply<.., true>, 36 bytes per
              neighbour in three streams; law minus scalars is the law form of the kernel pair
    xsph      this tree's library with XSPH at eps 0.5 and no viscous stress: the yardstick, a kernel pair of the same
              skeleton that gathers the same 32 bytes, measured in the same session
The pair kernel's gathers do not depend on the velocities, its store does: a particle whose viscous acceleration is
zero is not stored, and the column at rest would store nothing.  So every variant starts from the column with a seeded
velocity noise of --speed per component (scenes.dam_break's speed), small enough that the column keeps its neighbour
count over the run (reported per variant); the run ends with an error unless the viscous variants left less velocity
noise than the plain run.  mu is scenes.viscous_stable_mu at --fraction of the bulk's explicit limit.
Each child builds the scene, warms up, and times windows of queued steps between two synchronisations; the variants
take turns over several rounds and every window is kept.  Reported: best and median ms/step per variant; `none` beside
`parent` with the parent's own window spread (a structural statement - a context without the setting enqueues the
parent's launches - with the two times recorded beside it); what giving up the fused integrate costs (`unfused` minus
`none`); the kernel pair alone, constant (`mu` minus `unfused`) and with a law (`law` minus `scalars` plus that), beside
XSPH's pair (`xsph` minus `unfused`).

    timeout -k 10 1100 python tools/viscous_cost.py --parent /path/to/parent/libsph_hip.so \
        --out profiles/viscous_cost.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sph_hip_set_viscous_stress", "sph_hip_get_viscous_stress")
VARIANTS = ("parent", "none", "unfused", "mu", "scalars", "law", "xsph")
VISCOUS = ("mu", "scalars", "law")
GATHER_BYTES = 32              # posm[q] and R[q] per neighbour
LAW_GATHER_BYTES = 36          # and M[q]


def child(args):
    sys.path.insert(0, ROOT)
    from smoothed_particle_hydrodynamics_amd import lib as B
    if args.child == "parent":
        for name in NEW_SYMBOLS:          # the parent's library does not export them
            B.PROTOTYPES.pop(name)
    import numpy as np

    import smoothed_particle_hydrodynamics_amd as S
    from smoothed_particle_hydrodynamics_amd import scenes
    p, pos, vel, mass = scenes.dam_break(args.particles, speed=args.speed)
    n = mass.size
    mu = scenes.viscous_stable_mu(p, args.fraction)
    windows = []
    with S.SPH(n, p, mode=S.MODE_FULL_FAST) as sph:
        sph.setParticles(pos, vel, mass)
        sph.setTiming(S.TIMING_OFF)
        if args.child in ("scalars", "law"):
            # a temperature that falls with the height, carried and not diffused
            y = pos.reshape(-1, 3)[:, 1]
            sph.setScalars((1.0 - y / max(float(y.max()), 1e-30)).astype(np.float32), 0.0)
        if args.child in ("mu", "scalars"):
            sph.setViscousStress(mu)
        if args.child == "law":
            # the factor is 1 at the top and a half at the foot: never above the constant variant's mu
            sph.setViscousStress(mu, S.ViscosityLaw.exponential(0, 0.0, 0.6931471805599453, 0.0, 1.0))
        if args.child == "xsph":
            sph.setVelocitySmoothing(args.eps)
        sph.run(args.warmup)
        sph.synchronize()
        for _ in range(args.reps):
            t0 = time.perf_counter()
            sph.run(args.steps)
            sph.synchronize()
            windows.append((time.perf_counter() - t0) / args.steps * 1e3)
        part = sph.getParticles()
        assert np.isfinite(part.mPosition).all()
        neighbours = float(part.mNeighborCount.mean())
        speed = float(np.sqrt((part.mVelocity.astype(np.float64) ** 2).mean()))
        if args.child in VISCOUS:
            got_mu, got_law = sph.getViscousStress()
            assert got_mu != 0.0 and (got_law is not None) == (args.child == "law")
    print("RESULT " + json.dumps({"windows": windows, "neighbours": neighbours, "speed": speed, "mu": mu}), flush=True)


def measure(variant, args):
    env = dict(os.environ)
    for name in ("SPH_HIP_LIBRARY", "SPH_HIP_NO_FUSED_INTEGRATE"):
        env.pop(name, None)
    if variant == "parent":
        env["SPH_HIP_LIBRARY"] = os.path.abspath(args.parent)
    if variant == "unfused":
        env["SPH_HIP_NO_FUSED_INTEGRATE"] = "1"
    cmd = [sys.executable, os.path.abspath(__file__), "--child", variant, "--particles", str(args.particles),
           "--warmup", str(args.warmup), "--steps", str(args.steps), "--reps", str(args.reps), "--eps", str(args.eps),
           "--speed", str(args.speed), "--fraction", str(args.fraction)]
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
    ap.add_argument("--eps", type=float, default=0.5, help="the yardstick's XSPH setting")
    ap.add_argument("--fraction", type=float, default=0.1, help="mu as a fraction of the bulk's explicit limit")
    ap.add_argument("--speed", type=float, default=0.01, help="the velocity noise every variant starts from")
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

    windows = {r: [] for r in runs}
    neighbours, speed, mu = {}, {}, 0.0
    for k in range(args.rounds):
        for r in runs:
            got = measure(r, args)      # a child that fails ends the run: nothing more is started
            print("round %d %-8s median %.4f ms/step" % (k + 1, r, statistics.median(got["windows"])), flush=True)
            windows[r] += got["windows"]
            neighbours[r] = got["neighbours"]
            speed[r] = got["speed"]
            mu = got["mu"]
    say("viscous stress cost: %d-particle dam column, FULL_FAST, velocity noise %.3g, mu = %.6g (%.3g of the bulk's "
        "explicit limit); %d rounds, the variants taking turns; per child %d warm-up steps, then %d windows of %d steps" %
        (args.particles, args.speed, mu, args.fraction, args.rounds, args.warmup, args.reps, args.steps))
    for r in VISCOUS:
        if not speed[r] < speed["none"]:
            sys.exit("the term did not act in `%s`: rms velocity component %g with it, %g without" %
                     (r, speed[r], speed["none"]))
    med = {r: statistics.median(windows[r]) for r in runs}
    best = {r: min(windows[r]) for r in runs}
    base = runs[0]
    for r in runs:
        say("%-8s best %8.4f ms/step %6.3fx   median %8.4f ms/step %6.3fx   (windows %.4f .. %.4f)" %
            (r, best[r], best[r] / best[base], med[r], med[r] / med[base], best[r], max(windows[r])))
    if args.parent:
        pw = windows["parent"]
        say("no setting, beside the parent (structural: no existing kernel differs, the same launches): this tree's "
            "median %.4f, the parent's %.4f, %+.4f ms/step; the parent's own windows spread %.4f ms/step" %
            (med["none"], med["parent"], med["none"] - med["parent"], max(pw) - min(pw)))
    say("giving up the fused integrate (SPH_HIP_NO_FUSED_INTEGRATE=1 minus the default): median %+.4f ms/step, best "
        "%+.4f ms/step" % (med["unfused"] - med["none"], best["unfused"] - best["none"]))
    pair = med["mu"] - med["unfused"]
    say("k_viscous_stage and k_viscous_apply alone, constant mu (mu minus SPH_HIP_NO_FUSED_INTEGRATE=1): median %+.4f "
        "ms/step, best %+.4f ms/step; %d bytes gathered per neighbour in two streams" %
        (pair, best["mu"] - best["unfused"], GATHER_BYTES))
    say("the scalar pass a law needs (scalars minus mu): median %+.4f ms/step" % (med["scalars"] - med["mu"]))
    law_pair = pair + med["law"] - med["scalars"]
    say("the kernel pair with a law (that plus law minus scalars): median %+.4f ms/step, %+.4f over the constant form; "
        "%d bytes gathered per neighbour in three streams" % (law_pair, med["law"] - med["scalars"], LAW_GATHER_BYTES))
    yard = med["xsph"] - med["unfused"]
    say("the yardstick, k_xsph_stage and k_xsph_apply in the same session (xsph minus SPH_HIP_NO_FUSED_INTEGRATE=1): "
        "median %+.4f ms/step, %d bytes per neighbour in two streams; the constant-mu pair takes %.2f of its time, the "
        "law pair %.2f" % (yard, GATHER_BYTES, pair / yard, law_pair / yard))
    say("neighbours per particle at the end of a run: " + ", ".join("%s %.2f" % (r, neighbours[r]) for r in runs))
    say("rms velocity component at the end of a run: " + ", ".join("%s %.4g" % (r, speed[r]) for r in runs))
    say("a constant mu, whole step: median %+.4f ms/step over the default route without it; with a law and its scalars "
        "%+.4f" % (med["mu"] - med["none"], med["law"] - med["none"]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
