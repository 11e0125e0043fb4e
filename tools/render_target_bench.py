#!/usr/bin/env python3
"""Measures the resolve pass of formatted render targets (visionaray_amd/csrc/vrh_resolve.hip): the same frame
into a plain target and into a formatted one, on the same build and card.

    python tools/render_target_bench.py [--frames 24] [--out profiles/render_target/bench.json]

At 1920 x 1080, after a warm-up, medians over `frames` frames of each leg:
    hf1M primary        vrh_render             plain | RGBA8
    hf1M AO             vrh_render             plain | RGBA8
    hf1M AO             vrh_render_view        plain | RGBA8 + DEPTH24_STENCIL8
    256^3 volume frame  vrh_render_volume      plain | RGBA8      (the workload of profiles/volume/bench.json, R8)
The traversal frames are timed by the runtime's hipEvent pair around the launch (vrh_last_frame_stats kernel_ms,
which covers a formatted target's resolve pass); the volume frame has no such pair and is timed on the host from
issue to completion, as tools/volume_bench.py does.  There is no bar: the ratio formatted / plain is recorded.
The resolve alone is also timed: `batch` back-to-back vrh_rt_resolve calls on the stream, host time / batch, with
the bytes it moves per second (read: 16 B staging colour, + 8 B prim id and t with depth; written: the formatted
pixel, + 4 B depth).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import visionaray_amd as va  # noqa: E402
from visionaray_amd import buildinfo, scenes  # noqa: E402

CF, DF = va.color_format, va.depth_format


def median_kernel_ms(ctx, frame, n, warmup):
    out = []
    for i in range(warmup + n):
        frame()
        ms = ctx.last_frame_stats()["kernel_ms"]
        if i >= warmup:
            out.append(ms)
    return statistics.median(out)


def median_wall_ms(ctx, frame, n, warmup):
    out = []
    for i in range(warmup + n):
        ctx.sync()
        t0 = time.perf_counter()
        frame()
        ctx.sync()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def look_at(eye):
    eye = np.asarray(eye, np.float64)
    f = -eye / np.linalg.norm(eye)
    s = np.cross(f, (0.0, 1.0, 0.0))
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    m = np.eye(4)
    m[0, :3], m[1, :3], m[2, :3] = s, u, -f
    m[:3, 3] = -m[:3, :3] @ eye
    return m.astype(np.float32)


def perspective(fovy, aspect, zn, zf):
    f = 1.0 / np.tan(fovy / 2.0)
    m = np.zeros((4, 4))
    m[0, 0], m[1, 1], m[2, 2], m[2, 3], m[3, 2] = f / aspect, f, (zf + zn) / (zn - zf), 2.0 * zf * zn / (zn - zf), -1.0
    return m.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_target", "bench.json"))
    args = ap.parse_args()
    if args.frames < 20:
        sys.exit("render_target_bench: at least 20 frames")
    W, H = args.width, args.height
    px = W * H
    ctx = va.Context(0)
    prims = scenes.primitives("hf1M")
    dev = va.hip_index_bvh(ctx, va.build_index_bvh(prims), scenes.normals_for(prims))
    cam, _, _ = scenes.scene_camera("hf1M", W, H)
    basis = cam.basis(W, H)
    fovy = float(np.float32(45.0) * np.float32(va.DEGREES_TO_RADIANS))
    view, proj = look_at(basis.eye[:]), perspective(fovy, W / H, 0.001, 1000.0)
    vcam = va.view_camera(view, proj, W, H)
    results = []

    def leg(name, entry, plain_frame, fmt_frame, fmt, timer):
        plain_ms = timer(ctx, plain_frame, args.frames, args.warmup)
        fmt_ms = timer(ctx, fmt_frame, args.frames, args.warmup)
        rec = {"frame": name, "entry_point": entry, "format": fmt, "plain_ms": round(plain_ms, 4), "formatted_ms": round(fmt_ms, 4),
               "ratio": round(fmt_ms / plain_ms, 4), "timer": "hipEvent" if timer is median_kernel_ms else "host, issue to completion"}
        results.append(rec)
        print(json.dumps(rec), flush=True)

    plain = va.hip_buffer_rt(ctx, W, H)
    rgba8 = va.hip_buffer_rt(ctx, W, H, color_format=CF.rgba8)
    rgba8d = va.hip_buffer_rt(ctx, W, H, color_format=CF.rgba8, depth_format=DF.depth24_stencil8)
    primary, ao = va.closest_hit_kernel(dev), va.ao_kernel(dev)
    leg("hf1M primary", "vrh_render", lambda: va.render(ctx, dev, plain, basis, primary), lambda: va.render(ctx, dev, rgba8, basis, primary),
        "RGBA8", median_kernel_ms)
    leg("hf1M AO", "vrh_render", lambda: va.render(ctx, dev, plain, basis, ao), lambda: va.render(ctx, dev, rgba8, basis, ao),
        "RGBA8", median_kernel_ms)
    leg("hf1M AO", "vrh_render_view", lambda: va.render_view(ctx, dev, plain, vcam, ao), lambda: va.render_view(ctx, dev, rgba8d, vcam, ao),
        "RGBA8 + DEPTH24_STENCIL8", median_kernel_ms)

    # the resolve alone, on the frames the last legs left in the staging buffers
    resolve = []
    for name, rt, desc, rd, wr in (("RGBA8", rgba8, va.resolve_desc(), 16, 4),
                                   ("RGBA8 + DEPTH24_STENCIL8", rgba8d, va.resolve_desc(view=view, proj=proj), 24, 8)):
        times = []
        for i in range(args.warmup + args.frames):
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(args.batch):
                rt.resolve(desc)
            ctx.sync()
            if i >= args.warmup:
                times.append((time.perf_counter() - t0) * 1e3 / args.batch)
        ms = statistics.median(times)
        rec = {"format": name, "resolve_ms": round(ms, 5), "bytes_per_pixel": rd + wr, "gbytes_per_s": round(px * (rd + wr) / (ms * 1e-3) / 1e9, 1),
               "timer": "host time of %d back-to-back passes / %d" % (args.batch, args.batch)}
        resolve.append(rec)
        print(json.dumps(rec), flush=True)

    # the volume frame of profiles/volume/bench.json (tests/cpp/volume_user_kernel.hip bench<uint8_t>)
    n = 256
    g = np.arange(n, dtype=np.float32)
    s = (np.sin(np.float32(5.0) * g / n + np.float32(2.0))[:, None, None] * np.sin(np.float32(7.0) * g / n + np.float32(1.0))[None, :, None]
         * np.sin(np.float32(9.0) * g / n)[None, None, :])
    voxels = ((0.5 + 0.5 * s) * 255.0).astype(np.uint8)
    u = np.arange(256, dtype=np.float32) / np.float32(255.0)
    tf = va.transfunc(np.stack([u, 1.0 - u, 0.5 + 0.5 * np.sin(20.0 * u), 0.02 * u * u], axis=1).astype(np.float32),
                      va.tex_filter.linear, va.tex_address.clamp)
    vol = va.volume(ctx, voxels, va.tex_filter.linear, va.tex_address.clamp, tf)
    vcamera = va.camera()
    vcamera.perspective(fovy, np.float32(W) / np.float32(H), 0.001, 1000.0)
    r = float(np.sqrt(12.0) * 0.5)
    vcamera.look_at((0.0, 0.0, r + r / float(np.arctan(fovy))), (0.0, 0.0, 0.0))
    kern = va.volume_kernel(vol, ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), dt=2.0 / 512.0)
    sched = va.hip_sched(ctx, async_frames=False)
    sp_plain = va.make_sched_params(va.pixel_sampler.uniform_type, vcamera, plain)
    sp_fmt = va.make_sched_params(va.pixel_sampler.uniform_type, vcamera, rgba8)
    leg("256^3 volume (R8)", "vrh_render_volume", lambda: sched.frame(kern, sp_plain), lambda: sched.frame(kern, sp_fmt), "RGBA8", median_wall_ms)

    out = {"workload": {"width": W, "height": H, "scene": "hf1M, the benchmark's camera; the matrix camera looks from the same eye",
                        "volume": "256^3 procedural R8, linear / clamp, 256-entry transfer function, view_all, dt = 2 / 512"},
           "method": "medians over %d frames after %d warm-up frames per leg" % (args.frames, args.warmup),
           "kernel_source_sha256": buildinfo.kernel_source_sha256(), "frames": results, "resolve_alone": resolve}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    for o in (plain, rgba8, rgba8d, vol, dev):
        o.close()
    ctx.close()


if __name__ == "__main__":
    main()
