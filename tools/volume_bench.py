#!/usr/bin/env python3
"""Measures the volume kernel: A, the built-in kernel (vrh_render_volume), against B, the volume example's
lambda as a hipcc user kernel, on one frame.

    python tools/volume_bench.py [--reps 5] [--out profiles/volume/bench.json]

Workload: 1920 x 1080, a procedural 256^3 volume (linear / clamp) as R8 and as R32F, a 256-entry linear
transfer function, the view_all camera, dt = box extent / 512.  Per format one run of
build/tests/volume_user_kernel (tests/cpp/volume_user_kernel.hip `bench`), under its own time limit: after a
warm-up of both kernels it alternates A and B `reps` times, times every frame from issue to completion and
reports the medians; the steps are vrh_volume_last_stats' of the built-in frame (the lambda renders the same
bits, which the program checks).  A run that fails or times out ends the measurement: nothing further is
started.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "tests", "volume_user_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--timeout", type=int, default=150, help="seconds per format")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume", "bench.json"))
    args = ap.parse_args()
    if not os.path.exists(EXE):
        sys.exit("volume_bench: %s is not built (make -C visionaray_amd)" % EXE)
    results = []
    for fmt in ("r8", "r32f"):
        cmd = ["timeout", "-k", "10", str(args.timeout), EXE, "bench", fmt, str(args.n), str(args.width), str(args.height), str(args.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("volume_bench: %s ended with status %d: %s" % (fmt, r.returncode, (r.stdout + r.stderr).strip()))
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        if not rec["same_bits"]:
            sys.exit("volume_bench: %s: the lambda and the built-in kernel render different frames" % fmt)
        results.append(rec)
        print(json.dumps(rec), flush=True)
    out = {"workload": {"width": args.width, "height": args.height, "volume": "%d^3 procedural, linear / clamp" % args.n,
                        "transfunc": "256 entries, linear / clamp", "camera": "view_all of [-1, 1]^3, fovy 45 degrees",
                        "dt": "box extent / 512", "opacity_cutoff": 0.999},
           "method": "warm-up of both, then %d alternated frames of A (built-in kernel) and B (the example's lambda as a "
                     "user kernel), wall time from issue to completion, medians" % args.reps,
           "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
