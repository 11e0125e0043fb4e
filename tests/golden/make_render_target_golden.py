#!/usr/bin/env python3
"""Fixtures of formatted render targets: tests/golden/rt_pixels.npz and tests/golden/rt_frame.npz.

Compiles tests/golden/render_target_ref.cpp (our own program over the reference tree's headers: its
detail::pixel_access::store / blend, detail::depth_transform, simple_buffer_rt::clear_* and simple_sched with
camera matrices) with g++ into oracle/_ref/ and runs it.  Runs only where the reference tree exists; nothing in
build(), smoke(), bench.py or the tests calls it.

    python tests/golden/make_render_target_golden.py [--ref /path/to/reference]

rt_pixels.npz (the pixel pipeline; every input a function of SEED): N pixels go through
    clear(colour, depth), store, blend frame 1, blend frame 2, blend frame 3, blend frame 4, store
(blend of frame f: 1 / f, 1 - 1 / f) in every colour format x depth format; the file holds the inputs of the six
steps (colour, hit, t, isect_pos) and the raw buffers after the clear and after every step.  The colour buffers
do not depend on the depth format nor the depth buffers on the colour format -- the generator checks that over
all twelve targets and stores each once.  The camera is the identity (view = proj = 1): the pixel's ray is then
(u, v, -1) + t (0, 0, 1) exactly, so isect_pos = (., ., t - 1) and the tests reproduce the reference's depth from t.
The colours include 0, 1, values below 0 and above 1, k / 255 and its two float neighbours, and products
rgb * a just below and above k / 255; the depths include 0, 1 and k / 16777215 and its neighbours.

rt_frame.npz (a whole frame): simple_sched<basic_ray<float>> with make_sched_params(uniform_type, view, proj, rt)
over a random triangle BVH built by the reference's builder, image 61 x 45, kernel colour = a function of the
prim id, into <PF_RGBA8, PF_DEPTH24_STENCIL8> and <PF_RGB8, PF_DEPTH32F>: the triangles, the matrices, the raw
buffers, and the prim id / t of every pixel.  Every triangle lies between the near and far planes, so no depth is
non-finite (checked).

Both files are self-contained and written with fixed zip timestamps, so a second run reproduces them byte for
byte; the seeds are recorded in them.
"""
import argparse
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import visionaray_amd as va  # noqa: E402
from make_pathtrace_golden import save_npz  # noqa: E402

BIN = os.path.join(ROOT, "oracle", "_ref", "render_target_ref")
SEED = 20
N = 128
STEPS = [(0, 1), (1, 1), (1, 2), (1, 3), (1, 4), (0, 5)]     # (blend, frame_num)
CLEAR_COLOR, CLEAR_DEPTH = (0.25, 0.5, 0.75, 0.5), 1.0
FRAME_SEED, W, H = 21, 61, 45
MAX_BYTES = 65961            # the largest of the ptm_*.npz fixtures
COLOR_BYTES = (16, 16, 4, 3)  # RGBA32F, RGB32F (vector<3, float> is 16 bytes), RGBA8, RGB8
f32 = np.float32


def compile_generator(ref):
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.run(["g++", "-std=c++14", "-O2", "-msse4.1", "-ffp-contract=off", "-w", "-I" + os.path.join(ref, "include"),
                    os.path.join(HERE, "render_target_ref.cpp"), "-o", BIN], check=True)


def neighbours(x):
    x = f32(x)
    return [np.nextafter(x, f32(-1e9)), x, np.nextafter(x, f32(1e9))]


def draw_step(rng):
    """colours (N, 4), hit (N,), t (N,) of one step"""
    special = [0.0, 1.0, -0.5, 1.7, -0.0, 0.999999, 1.000001, 0.5]
    for k in rng.integers(1, 255, 6):
        special += neighbours(f32(k) / f32(255.0))
    color = rng.uniform(-0.25, 1.25, (N, 4)).astype(f32)
    pick = rng.random((N, 4)) < 0.4
    color[pick] = rng.choice(np.asarray(special, f32), int(pick.sum()))
    # alpha: often exactly 1 (so the RGB formats see the special values), else in and beyond [0, 1]
    color[rng.random(N) < 0.35, 3] = 1.0
    # products rgb * a just below and above k / 255
    for i in rng.choice(N, N // 4, replace=False):
        a = f32(rng.uniform(0.3, 1.0))
        for c in range(3):
            target = rng.choice(neighbours(f32(rng.integers(1, 255)) / f32(255.0)))
            q = f32(target / a)
            color[i, c] = rng.choice(neighbours(q))
        color[i, 3] = a
    hit = rng.random(N) < 0.75
    depth = rng.uniform(0.0, 1.0, N).astype(f32)
    sp = [0.0, 1.0, 0.5] + [y for k in rng.integers(1, 16777215, 8) for y in neighbours(f32(k) / f32(16777215.0))]
    pick = rng.random(N) < 0.4
    depth[pick] = np.clip(rng.choice(np.asarray(sp, f32), int(pick.sum())), 0.0, 1.0)
    t = (depth * f32(2.0)).astype(f32)                  # depth = ((t - 1) + 1) * 0.5
    return color, hit, t


def make_pixels():
    rng = np.random.default_rng(SEED)
    colors, hits, ts, poss = [], [], [], []
    blob = struct.pack("<3I5f", 0x58505452, N, len(STEPS), *CLEAR_COLOR, CLEAR_DEPTH)
    for blend, frame in STEPS:
        color, hit, t = draw_step(rng)
        pos = rng.uniform(-1.0, 1.0, (N, 3)).astype(f32)
        pos[:, 2] = t - f32(1.0)                          # the identity camera's ray: z = -1 + 1 * t
        colors.append(color); hits.append(hit); ts.append(t); poss.append(pos)
        blob += struct.pack("<2I", blend, frame) + color.tobytes() + hit.astype(np.uint32).tobytes() + pos.tobytes()
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        open(src, "wb").write(blob)
        subprocess.run([BIN, "pixels", src, dst], check=True)
        raw = open(dst, "rb").read()
    S = len(STEPS) + 1
    off = 0
    col = {}
    dep = {}
    for cf in range(4):
        for df in range(3):
            c = np.zeros((S, N * COLOR_BYTES[cf]), np.uint8)
            z = np.zeros((S, N), np.uint32)
            for s in range(S):
                c[s] = np.frombuffer(raw, np.uint8, N * COLOR_BYTES[cf], off); off += N * COLOR_BYTES[cf]
                if df:
                    z[s] = np.frombuffer(raw, np.uint32, N, off); off += N * 4
            if cf == 1:
                c = c.reshape(S, N, 16)[:, :, :12].reshape(S, -1)     # the fourth word is unspecified
            assert cf not in col or np.array_equal(col[cf], c), "colour depends on the depth format"
            col[cf] = c
            if df:
                assert df not in dep or np.array_equal(dep[df], z), "depth depends on the colour format"
                dep[df] = z
    assert off == len(raw)
    arrays = {"seed": np.uint32([SEED]), "steps": np.uint32(STEPS), "clear_color": f32(CLEAR_COLOR), "clear_depth": f32([CLEAR_DEPTH]),
              "in_color": np.stack(colors), "in_hit": np.stack(hits).astype(np.uint8), "in_t": np.stack(ts), "in_pos": np.stack(poss),
              "out_rgba32f": col[0].view(np.uint32).reshape(S, N, 4), "out_rgb32f": col[1].view(np.uint32).reshape(S, N, 3),
              "out_rgba8": col[2].reshape(S, N, 4), "out_rgb8": col[3].reshape(S, N, 3),
              "out_depth32f": dep[1], "out_depth24s8": dep[2]}
    assert np.isfinite(dep[1].view(f32)).all()
    path = os.path.join(HERE, "rt_pixels.npz")
    save_npz(path, **arrays)
    return path


def look_at(eye, center, up):
    f = center - eye
    f = f / np.linalg.norm(f)
    s = np.cross(f, up)
    s = s / np.linalg.norm(s)
    u = np.cross(s, f)
    m = np.eye(4)
    m[0, :3], m[1, :3], m[2, :3] = s, u, -f
    m[:3, 3] = -m[:3, :3] @ eye
    return m.astype(f32)


def perspective(fovy, aspect, zn, zf):
    f = 1.0 / np.tan(fovy / 2.0)
    m = np.zeros((4, 4))
    m[0, 0], m[1, 1] = f / aspect, f
    m[2, 2], m[2, 3] = (zf + zn) / (zn - zf), 2.0 * zf * zn / (zn - zf)
    m[3, 2] = -1.0
    return m.astype(f32)


def make_frame():
    rng = np.random.default_rng(FRAME_SEED)
    n = 300
    c = rng.uniform(-0.9, 0.9, (n, 3))
    size = 10.0 ** rng.uniform(-1.2, -0.5, (n, 1))
    e1, e2 = rng.standard_normal((n, 3)) * size, rng.standard_normal((n, 3)) * size
    prims = va.make_triangles(c - 0.5 * (e1 + e2), e1, e2)
    d = rng.standard_normal(3)
    eye = 3.2 * d / np.linalg.norm(d)
    view = look_at(eye, np.zeros(3), np.array([0.0, 1.0, 0.0]))
    proj = perspective(0.8, W / H, 0.25, 12.0)          # everything within [-2, 2]^3 lies between the planes
    vcm, pcm = view.T.reshape(16).copy(), proj.T.reshape(16).copy()     # column-major
    blob = struct.pack("<4I", 0x52465452, W, H, n) + vcm.tobytes() + pcm.tobytes() + np.ascontiguousarray(prims).tobytes()
    with tempfile.TemporaryDirectory() as dd:
        src, dst = os.path.join(dd, "in.bin"), os.path.join(dd, "out.bin")
        open(src, "wb").write(blob)
        subprocess.run([BIN, "frame", src, dst], check=True)
        raw = open(dst, "rb").read()
    P = W * H
    off = 0
    rgba8 = np.frombuffer(raw, np.uint8, P * 4, off).reshape(P, 4); off += P * 4
    d24 = np.frombuffer(raw, np.uint32, P, off); off += P * 4
    rgb8 = np.frombuffer(raw, np.uint8, P * 3, off).reshape(P, 3); off += P * 3
    d32 = np.frombuffer(raw, np.uint32, P, off); off += P * 4
    pid = np.frombuffer(raw, np.uint32, P, off); off += P * 4
    t = np.frombuffer(raw, np.uint32, P, off); off += P * 4
    assert off == len(raw)
    hit = pid != 0xFFFFFFFF
    assert hit.any() and (~hit).any(), "the frame needs pixels that hit and pixels that miss"
    assert np.isfinite(d32.view(f32)).all() and (d32.view(f32)[hit] < 1.0).all() and (d32.view(f32)[hit] > 0.0).all()
    arrays = {"seed": np.uint32([FRAME_SEED]), "size": np.uint32([W, H]), "view": vcm, "proj": pcm,
              "prims": np.ascontiguousarray(prims).view(np.uint32).reshape(n, 16),
              "rgba8": rgba8, "depth24s8": d24, "rgb8": rgb8, "depth32f": d32, "prim_id": pid, "t": t}
    path = os.path.join(HERE, "rt_frame.npz")
    save_npz(path, **arrays)
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    if not os.path.exists(os.path.join(args.ref, "include", "visionaray", "detail", "pixel_access.h")):
        sys.exit("make_render_target_golden: the reference tree is not here")
    compile_generator(args.ref)
    for path in (make_pixels(), make_frame()):
        size = os.path.getsize(path)
        assert size <= MAX_BYTES, (path, size)
        print(os.path.basename(path), size, "bytes")


if __name__ == "__main__":
    main()
