#!/usr/bin/env python3
"""The path tracer's plastic instance next to its generic instance (tagged material records) on the SAME
materials: bench.py's scene (hf1M at 1920x1080), 32 frames in flight per launch (vrh_render_batch) and
hipEvent kernel time (vrh_last_frame_stats), whitted_spec's plastics, 10 bounces.  The two are launched
alternately; reports the median kernel time per frame of each, and checks that both rendered the same
bits.  One JSON line.  Run it under a timeout:

    timeout 300 python tools/pathtrace_generic_ab.py [--scene hf1M] [--launches 5] [--frames 32]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="hf1M")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--bounces", type=int, default=10)
    args = ap.parse_args()
    W, H, F = args.width, args.height, args.frames
    ctx = va.Context(0)
    prims = scenes.primitives(args.scene)
    prims["geom_id"] = np.arange(len(prims), dtype=np.uint32) % 3
    dev = va.hip_index_bvh(ctx, va.build_index_bvh(prims), va.face_normals(prims))
    cam, _, _ = scenes.scene_camera(args.scene, W, H)
    cams = [cam.basis(W, H)] * F
    O.build()
    m, lt, _, bg = O.whitted_spec()
    m, lt = m.view(va.PLASTIC_DTYPE), lt.view(va.POINT_LIGHT_DTYPE)
    kw = dict(bg=bg, ambient=(1.0, 1.0, 1.0, 1.0), num_bounces=args.bounces)
    kernels = {"plastic": va.pathtracing_kernel(dev, va.shading(ctx, m, lt), **kw),
               "generic": va.pathtracing_kernel(dev, va.generic_shading(ctx, m, lt), **kw)}
    rt = va.hip_buffer_rt(ctx, W, H * F, flags=va._capi.VRH_RT_COLOR)
    ms = {name: [] for name in kernels}
    rays, first = {}, {}
    for i in range(1 + args.launches):                       # launch 0 of each: warm-up
        for name, k in kernels.items():
            va.render_batch(ctx, dev, rt, cams, k, frame_num=1)
            st = ctx.last_frame_stats()
            if i == 0:
                first[name] = rt.download()["color"][:W * H].copy()
            else:
                ms[name].append(st["kernel_ms"])
            rays[name] = int(st["rays"])
    out = {"scene": args.scene, "W": W, "H": H, "bounces": args.bounces, "frames_per_launch": F, "launches": args.launches,
           "same_bits": bool(np.array_equal(first["plastic"].view(np.uint32), first["generic"].view(np.uint32)))}
    for name in kernels:
        med = statistics.median(ms[name])
        out[name] = {"kernel_ms_per_frame": round(med / F, 4), "kernel_ms_launches": [round(x, 3) for x in ms[name]],
                     "rays": rays[name], "mrays_per_s": round(rays[name] / med / 1e3, 1)}
    out["generic_over_plastic"] = round(out["generic"]["kernel_ms_per_frame"] / out["plastic"]["kernel_ms_per_frame"], 4)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
