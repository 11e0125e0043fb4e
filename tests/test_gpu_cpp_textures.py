"""GPU: tests/cpp/textured_standalone.cpp (hip_shading::set_textures through the C++ header API with the
types of visionaray_hip/standalone.h; built by visionaray_amd/Makefile) renders the frame the Python API
renders from the same scene, textures and camera: the colour hashes are equal."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import visionaray_amd as va
from visionaray_amd import _capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "tests", "textured_standalone")


def fnv1a(data):
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def test_cpp_set_textures_renders_the_python_frame(ctx):
    r = subprocess.run([EXE], check=True, capture_output=True, text=True, timeout=120)
    out = json.loads(r.stdout.strip().splitlines()[-1])
    grid, W, H = 16, out["W"], out["H"]
    prims = np.zeros(2 * grid * grid, va.TRIANGLE_DTYPE)
    _capi.check("vrh_gen_heightfield", grid, prims.ctypes.data_as(C.c_void_p))
    prims["geom_id"] = np.arange(len(prims), dtype=np.uint32) % 3
    dev = va.hip_index_bvh(ctx, va.build_index_bvh(prims), va.face_normals(prims))
    materials = np.concatenate([
        np.atleast_1d(va.plastic((0.2, 0.2, 0.2), 1.0, (0.8, 0.3, 0.2), 1.0, (1.0, 1.0, 1.0), 0.4, 32.0)),
        np.atleast_1d(va.plastic((0.1, 0.1, 0.1), 0.5, (0.2, 0.7, 0.3), 0.9, (0.9, 0.9, 0.9), 0.2, 8.0)),
        np.atleast_1d(va.plastic((0.05, 0.05, 0.1), 1.0, (0.3, 0.3, 0.9), 0.7, (1.0, 0.8, 0.6), 0.6, 64.5))])
    sh = va.shading(ctx, materials, np.atleast_1d(va.point_light((0.0, 2.0, 0.0), (1.0, 1.0, 1.0), 1.0, 1.0, 0.0, 0.0)))
    i = np.arange(16)
    checker = np.where((((i + i // 4) & 1) != 0)[:, None], 255, 40 + 60 * np.arange(4)[None, :]).astype(np.uint8).reshape(4, 4, 4)
    small = ((17 * np.arange(16) + 30) & 255).astype(np.uint8).reshape(2, 2, 4)
    textures = [va.texture(checker, va.tex_filter.linear, va.tex_address.wrap),
                va.texture(small, va.tex_filter.nearest, (va.tex_address.mirror, va.tex_address.clamp)), None]
    v = np.stack([prims["v1"], prims["v1"] + prims["e1"], prims["v1"] + prims["e2"]], axis=1).astype(np.float32)
    tc = np.stack([v[:, :, 0] * np.float32(3.0), v[:, :, 2] * np.float32(3.0)], axis=2).reshape(-1, 2)
    sh.set_textures(tc, textures)
    cam = va.camera()
    cam.perspective(np.float32(45.0) * np.float32(va.DEGREES_TO_RADIANS), np.float32(W) / np.float32(H), 0.001, 1000.0)
    cam.look_at((0.0, 0.9, 1.4), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    rt = va.hip_buffer_rt(ctx, W, H)
    k = va.simple_kernel(dev, sh, bg=(0.1, 0.2, 0.3, 1.0), ambient=(1.0, 1.0, 1.0, 0.3))
    va.hip_sched(ctx).frame(k, va.make_sched_params(va.pixel_sampler.uniform_type, cam, rt))
    got = rt.download()
    assert (got["prim_id"] != 0xFFFFFFFF).any()
    assert fnv1a(np.ascontiguousarray(got["color"]).tobytes()) == out["color_hash"]
    sh.set_textures(None, None)
    va.hip_sched(ctx).frame(k, va.make_sched_params(va.pixel_sampler.uniform_type, cam, rt))
    assert fnv1a(np.ascontiguousarray(rt.download()["color"]).tobytes()) != out["color_hash"]
