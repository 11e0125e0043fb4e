#!/usr/bin/env python3
"""Measures the multi-volume kernel (vrh_render_multi_volume) through the Python API.

    python tools/multi_volume_bench.py [--reps 5] [--out profiles/multi_volume/bench.json]

Workload A: the multi-volume example's scene at 1920 x 1080 -- the Marschner-Lobb signal (201^3), the heart (256^3)
and the mandelbulb (256^3) as float volumes, linear / clamp, their 5-entry nearest / clamp transfer functions,
rotations by pi / 4 about x / y / z, translations 2.5 i, the example's material, the light at the eye, dt = 0.007.
After a warm-up frame, `reps` synchronous frames are timed from issue to completion; the median is reported with
the frame's loop iterations (vrh_volume_last_stats) per second.  Outside the timed region the host build of the
same loop (vrh_multi_volume_count_host; the same steps and alpha, checked) renders the frame once and counts the
volume samples and the share of them that are shaded.

Workload B, for scale: one 256^3 float volume (the heart), identity transform, a 256-entry linear transfer
function whose alphas stay below shade_alpha (no sample is shaded), dt = 0.01, through the multi-volume kernel
and through the single-volume kernel (vrh_render_volume), alternated `reps` times after a warm-up of both; the
two render the same bits (checked), and the ratio of the medians is recorded as measured.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import visionaray_amd as va  # noqa: E402

UNIT_BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
TF = np.asarray([
    [0.0, 0.2, 0.8, 0.005], [1.0, 0.8, 0.0, 0.01], [0.0, 1.0, 0.0, 0.50], [1.0, 0.8, 0.0, 0.01], [1.0, 1.0, 1.0, 0.005],
    [1.0, 0.0, 0.0, 1.0], [1.0, 0.0, 0.0, 0.2], [1.0, 0.0, 0.0, 0.2], [1.0, 0.0, 0.0, 0.2], [1.0, 1.0, 1.0, 0.002],
    [1.0, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 0.50], [1.0, 1.0, 1.0, 0.50], [1.0, 1.0, 1.0, 0.50], [0.0, 0.0, 1.0, 0.002]],
    np.float32).reshape(3, 5, 4)


def grid(n, scale, offset):
    a = (np.arange(n, dtype=np.float32) / np.float32(n)) * np.float32(scale) - np.float32(offset)
    return np.meshgrid(a, a, a, indexing="ij")            # z, y, x


def marschner_lobb(n):
    z, y, x = grid(n, 2.0, 1.0)
    pi = np.float32(np.pi)
    rho = np.cos(2 * pi * np.float32(6.0) * np.cos(pi * np.sqrt(x * x + y * y) / 2))
    return ((1 - np.sin(pi * z / 2) + np.float32(0.25) * (1 + rho)) / np.float32(2.5)).astype(np.float32)


def heart(n):
    z, y, x = grid(n, 4.0, 2.0)
    s = x * x + np.float32(2.25) * (y * y) + z * z - 1
    return (s * s * s - (x * x) * (z * z * z) - np.float32(9.0 / 80.0) * (y * y) * (z * z * z)).astype(np.float32)


def mandelbulb(n):
    z0, y0, x0 = grid(n, 3.0, 1.5)
    px, py, pz = x0.copy(), y0.copy(), z0.copy()
    inside = np.zeros(px.shape, bool)
    alive = np.ones(px.shape, bool)
    for _ in range(8):
        r = np.sqrt(px * px + py * py + pz * pz)
        theta, phi = np.arctan2(np.sqrt(px * px + py * py), pz) * 8, np.arctan2(py, px) * 8
        rn = r ** 8
        px, py, pz = rn * np.sin(theta) * np.cos(phi) + x0, rn * np.sin(theta) * np.sin(phi) + y0, rn * np.cos(theta)
        with np.errstate(over="ignore", invalid="ignore"):
            out = alive & ~(px * px + py * py + pz * pz <= 2.0)
        inside |= out
        alive &= ~out
        px[~alive], py[~alive], pz[~alive] = 0, 0, 0
    return inside.astype(np.float32)


def rotation(axis, angle):
    m = np.eye(4, dtype=np.float32)
    c, s = np.float32(np.cos(angle)), np.float32(np.sin(angle))
    a, b = [(1, 2), (2, 0), (0, 1)][axis]
    m[a, a], m[a, b], m[b, a], m[b, b] = c, -s, s, c
    return m


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the volumes' side lengths")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_volume", "bench.json"))
    args = ap.parse_args()
    W, H = args.width, args.height
    sizes = [int(201 * args.scale), int(256 * args.scale), int(256 * args.scale)]
    ctx = va.Context(0)
    sched = va.hip_sched(ctx, async_frames=False)
    rt = va.hip_buffer_rt(ctx, W, H)
    cam = va.camera()
    cam.perspective(45.0 * va.DEGREES_TO_RADIANS, W / H, 0.001, 1000.0)
    eye = (2.5, 1.0, 11.0)
    cam.look_at(eye, (2.5, 0.0, 0.0), (0.0, 1.0, 0.0))
    sp = va.make_sched_params(va.pixel_sampler.uniform_type, cam, rt)

    # A: the example's scene
    data = [marschner_lobb(sizes[0]), heart(sizes[1]), mandelbulb(sizes[2])]
    vols = [va.volume(ctx, data[i], va.tex_filter.linear, va.tex_address.clamp, va.transfunc(TF[i], va.tex_filter.nearest, va.tex_address.clamp))
            for i in range(3)]
    transforms = []
    for i in range(3):
        m = rotation(i, np.pi / 4)
        m[0, 3] = 2.5 * i
        transforms.append(m)
    material = va.plastic(ca=(0.2,) * 3, ka=1.0, cd=(0.8,) * 3, kd=1.0, cs=(0.8,) * 3, ks=1.0, exp=128.0)
    kern = va.multi_volume_kernel(vols, [UNIT_BOX] * 3, transforms, [material] * 3, va.point_light(eye))
    sched.frame(kern, sp)                                      # warm-up
    ms = sorted(timed(lambda: sched.frame(kern, sp)) for _ in range(args.reps))
    st = ctx.volume_last_stats()
    color = rt.download()["color"]
    med = ms[len(ms) // 2]
    # not timed: the host build of the same header takes the device's steps bit for bit and counts what the device
    # does not -- the volume samples and how many of them are shaded
    tfs = [va.transfunc(TF[i], va.tex_filter.nearest, va.tex_address.clamp) for i in range(3)]
    host = va.multi_volume_render_host(data, tfs, kern.entries, cam.basis(W, H), kern.desc)
    if host["stats"]["steps"] != st["steps"] or not np.array_equal(host["color"][:, 3].view(np.uint32), color[:, 3].view(np.uint32)):
        sys.exit("multi_volume_bench: the host build and the device disagree on the example's frame")
    cutoff = np.float32(va.api.float_not_below(0.999))              # what the kernel compares with
    example = {"ms_per_frame": med, "ms_all": ms, "rays": st["rays"], "steps": st["steps"], "capped": st["capped"],
               "steps_per_second": st["steps"] / (med * 1e-3), "hit_pixels": int((color[:, 3] > 0).sum()),
               "cutoff_pixels": int((color[:, 3] >= cutoff).sum()), "samples": host["samples"],
               "shaded_samples": host["shaded_samples"], "share_of_samples_shaded": host["shaded_samples"] / max(host["samples"], 1)}
    print(json.dumps({"example": example}), flush=True)

    # B: one unshaded volume through both kernels
    ramp = np.linspace(0.0, 1.0, 256, dtype=np.float32)
    tf = va.transfunc(np.stack([ramp, 1 - ramp, np.float32(0.5) + 0 * ramp, np.float32(0.08) * ramp], axis=1), va.tex_filter.linear,
                      va.tex_address.clamp)
    one = va.volume(ctx, np.clip(data[1] / np.float32(64.0), 0.0, 1.0), va.tex_filter.linear, va.tex_address.clamp, tf)
    cam.look_at((1.5, 1.2, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    single = va.volume_kernel(one, UNIT_BOX, dt=0.01)
    multi = va.multi_volume_kernel([one], [UNIT_BOX], [np.eye(4, dtype=np.float32)], [material], va.point_light(eye), dt=0.01)
    sched.frame(single, sp)
    want, want_steps = rt.download()["color"], ctx.volume_last_stats()["steps"]
    sched.frame(multi, sp)
    got, got_steps = rt.download()["color"], ctx.volume_last_stats()["steps"]
    same = bool(np.array_equal(want.view(np.uint32), got.view(np.uint32)) and want_steps == got_steps)
    a, b = [], []
    for _ in range(args.reps):
        a.append(timed(lambda: sched.frame(single, sp)))
        b.append(timed(lambda: sched.frame(multi, sp)))
    a.sort(), b.sort()
    scale = {"same_bits": same, "steps": got_steps, "single_volume_kernel_ms": a[len(a) // 2], "multi_volume_kernel_ms": b[len(b) // 2],
             "ratio_multi_over_single": b[len(b) // 2] / a[len(a) // 2], "single_all": a, "multi_all": b}
    print(json.dumps({"one_volume": scale}), flush=True)
    if not same:
        sys.exit("multi_volume_bench: the two kernels render different frames of the one-volume scene")

    out = {"workload": {"width": W, "height": H, "volumes": "Marschner-Lobb %d^3, heart %d^3, mandelbulb %d^3, float, linear / clamp" % tuple(sizes),
                        "transfuncs": "the example's three, 5 entries, nearest / clamp", "dt": 0.007, "shade_alpha": 0.1,
                        "camera": "eye (2.5, 1, 11) looking at (2.5, 0, 0), fovy 45 degrees", "opacity_cutoff": 0.999},
           "method": "warm-up, then %d synchronous frames timed from issue to completion, median; the one-volume scene alternates "
                     "the two kernels" % args.reps,
           "example": example, "one_volume": scale}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
