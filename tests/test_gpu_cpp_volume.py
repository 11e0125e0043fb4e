"""GPU: one scene -- the procedural 32^3 volume of examples/volume_hip.cpp in the box [-1, 1]^3 with the
example's parameters -- through three routes: the C++ header API's built-in kernel (examples/volume_hip),
the volume example's lambda as a hipcc user kernel (tests/cpp/volume_user_kernel.hip, which also runs the
built-in) and the Python API.  All render the same colour bits: the hashes are equal."""
import json
import os
import subprocess

import numpy as np
import pytest

import visionaray_amd as va

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, "build", "examples", "volume_hip")
USER = os.path.join(ROOT, "build", "tests", "volume_user_kernel")
N, W, H = 32, 160, 90


def color_hash(color):
    bits = np.ascontiguousarray(color, np.float32).view(np.uint32).ravel().astype(np.uint64)
    with np.errstate(over="ignore"):
        return "%016x" % int((bits * (2 * np.arange(bits.size, dtype=np.uint64) + 1)).sum(dtype=np.uint64))


def python_frame(ctx):
    z, y, x = np.meshgrid(*(np.arange(N, dtype=np.uint64),) * 3, indexing="ij")
    k = ((x * 73856093) ^ (y * 19349663) ^ (z * 83492791)) & 0xFFFFFFFF & 1023
    voxels = k.astype(np.float32) / np.float32(1023.0)
    tf = va.transfunc([[0.0, 0.0, 0.0, 0.0], [0.9, 0.2, 0.1, 0.01], [0.1, 0.8, 0.3, 0.04], [0.2, 0.3, 1.0, 0.12]],
                      va.tex_filter.linear, va.tex_address.clamp)
    vol = va.volume(ctx, voxels, va.tex_filter.linear, va.tex_address.clamp, tf)
    cam = va.camera()
    cam.perspective(np.float32(45.0) * np.float32(va.DEGREES_TO_RADIANS), np.float32(W) / np.float32(H), 0.001, 1000.0)
    cam.look_at((1.5, 1.2, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    rt = va.hip_buffer_rt(ctx, W, H)
    va.hip_sched(ctx, async_frames=False).frame(va.volume_kernel(vol, ((-1, -1, -1), (1, 1, 1))),
                                                va.make_sched_params(va.pixel_sampler.uniform_type, cam, rt))
    color = rt.download()["color"]
    st = ctx.volume_last_stats()
    rt.close(), vol.close()
    return color, st


def test_three_routes_render_one_frame(ctx):
    color, st = python_frame(ctx)
    assert st["capped"] == 0 and st["rays"] == W * H and st["steps"] > 100 * 1000
    assert np.any(color[:, 3] >= 0.999) and np.any(color[:, 3] == 0.0), "rays that end by the cutoff, and misses"
    want = color_hash(color)
    r = subprocess.run([EXAMPLE, str(N), str(W), str(H)], check=True, capture_output=True, text=True, timeout=120)
    ex = json.loads(r.stdout.strip().splitlines()[-1])
    assert ex["color_hash"] == want and ex["steps"] == st["steps"] and ex["rays"] == st["rays"] and ex["capped"] == 0
    r = subprocess.run([USER, str(N), str(W), str(H)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    uk = json.loads(r.stdout.strip().splitlines()[-1])
    assert uk["builtin_hash"] == want and uk["lambda_hash"] == want and uk["steps"] == st["steps"]
