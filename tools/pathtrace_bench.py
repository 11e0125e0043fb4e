#!/usr/bin/env python3
"""Throughput of the built-in path tracer next to the whitted kernel: hf1M at 1920x1080, whitted_spec
materials, 10 bounces, one frame per launch and 8 frames per launch.  Reports rays / kernel_ms from
vrh_last_frame_stats (median over the timed launches) as one JSON line.  Run it under a timeout:

    timeout 300 python tools/pathtrace_bench.py [--scene hf1M] [--launches 5] [--bounces 10]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import visionaray_amd as va  # noqa: E402
from oracle import oracle as O  # noqa: E402
from visionaray_amd import scenes  # noqa: E402


def measure(ctx, dev, k, cams, W, H, launches, warmup=2):
    rt = va.hip_buffer_rt(ctx, W, H * len(cams))
    ms, rays = [], 0
    for i in range(warmup + launches):
        va.render_batch(ctx, dev, rt, cams, k, frame_num=1 + i * len(cams))
        st = ctx.last_frame_stats()
        if i >= warmup:
            ms.append(st["kernel_ms"])
            rays = st["rays"]
    med = statistics.median(ms)
    return {"kernel_ms": round(med, 4), "rays": int(rays), "mrays_per_s": round(rays / med / 1e3, 1),
            "frames_per_launch": len(cams)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="hf1M")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--bounces", type=int, default=10)
    args = ap.parse_args()
    W, H = args.width, args.height
    ctx = va.Context(0)
    prims = scenes.primitives(args.scene)
    prims["geom_id"] = np.arange(len(prims), dtype=np.uint32) % 3
    dev = va.hip_index_bvh(ctx, va.build_index_bvh(prims), va.face_normals(prims))
    cam, _, _ = scenes.scene_camera(args.scene, W, H)
    basis = cam.basis(W, H)
    O.build()
    m, lt, amb, bg = O.whitted_spec()
    sh = va.shading(ctx, m.view(va.PLASTIC_DTYPE), lt.view(va.POINT_LIGHT_DTYPE))
    kernels = {
        "pathtracing": va.pathtracing_kernel(dev, sh, bg=bg, ambient=(1.0, 1.0, 1.0, 1.0), num_bounces=args.bounces),
        "whitted": va.whitted_kernel(dev, sh, bg=bg, ambient=amb, num_bounces=4),
    }
    out = {"scene": args.scene, "W": W, "H": H, "bounces": args.bounces}
    for name, k in kernels.items():
        out[name] = {"f1": measure(ctx, dev, k, [basis], W, H, args.launches),
                     "f8": measure(ctx, dev, k, [basis] * 8, W, H, args.launches)}
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
