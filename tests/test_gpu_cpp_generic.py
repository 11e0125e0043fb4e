"""GPU: generic primitives through the C++ header layer.  examples/generic_primitive_hip.cpp (built on
visionaray_hip/standalone.h by visionaray_amd/Makefile) renders the reference example's scene through
hip_sched::frame; its buffer hashes are compared with the reference's frames of tests/golden/gp_example.npz (prim id
and t in all four kernels, primary and AO colour, AO masks) and, for the simple / whitted colour, with the Python
API's frames of the same scene.  tests/cpp/generic_user_kernel.hip: a generic view never reaches a user kernel's walk."""
import json
import os
import subprocess

import numpy as np
import pytest

import gp_cases as G
import visionaray_amd as va
from visionaray_amd import _capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, "build", "examples", "generic_primitive_hip")
USER = os.path.join(ROOT, "build", "tests", "generic_user_kernel")


def fnv1a(a):
    h = 1469598103934665603
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def example_camera():
    """the generator's camera of gp_example (make_generic_primitive_golden.py example_scene) and the sphere's y"""
    f = np.float32
    s = G.spec()["gp_example"]
    fovy = f(f(45.0) * f(va.DEGREES_TO_RADIANS))
    r = f(np.sqrt(f(12.0)) * f(0.5))
    eye_z = f(f(1.0) + f(r + f(r / np.arctan(fovy))))
    cam = va.camera()
    cam.perspective(float(fovy), np.float32(G.W) / np.float32(G.H), 0.001, 1000.0)
    cam.look_at((0.0, 0.0, float(eye_z)), (0.0, 0.0, 1.0))
    b = cam.basis(G.W, G.H)
    basis = np.float32([list(b.eye), list(b.cam_u), list(b.cam_v), list(b.cam_w)])
    assert G.same_bits(basis, G.fixture("gp_example")["camera"])          # the fixture's camera, bit for bit
    return np.float32([s["sphere_y"], 0.0, 0.0, eye_z, 0.0, 0.0, 1.0, fovy])


def test_example_renders_the_reference_frames(ctx, tmp_path):
    cam_file = tmp_path / "camera.bin"
    example_camera().tofile(str(cam_file))
    r = subprocess.run([EXAMPLE, str(cam_file)], check=True, capture_output=True, text=True, timeout=120)
    out = json.loads(r.stdout.strip().splitlines()[-1])
    a, s = G.fixture("gp_example"), G.spec()["gp_example"]
    assert out["hits"] == int((a["prim_id"] != G.MISS).sum())
    for kind in G.KERNELS:
        assert out[kind]["prim_id"] == fnv1a(a["prim_id"]), kind
        assert out[kind]["t"] == fnv1a(a["t"]), kind
    hit = a["prim_id"] != G.MISS
    primary = np.where(hit[:, None], np.float32(1.0), np.float32(s["bg"])[None, :]).astype(np.float32)
    assert out["primary"]["color"] == fnv1a(primary)
    assert out["ao"]["color"] == fnv1a(a["ao_color"]) and out["ao"]["occ"] == fnv1a(a["occ"])
    # simple / whitted colour: the Python API's frames of the fixture (held to the reference in tests/test_gpu_generic.py)
    dev = va.hip_index_bvh(ctx, G.host_bvh("gp_example"), a["normals"])
    sh = G.shading_of(ctx, a)
    for kind in ("simple", "whitted"):
        got = G.render(ctx, dev, G.camera_of(a["camera"]), G.kernel(kind, dev, sh, s))
        assert out[kind]["color"] == fnv1a(got["color"]), kind


def test_example_default_arguments_render_the_scene():
    r = subprocess.run([EXAMPLE], check=True, capture_output=True, text=True, timeout=120)
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["W"] == G.W and out["H"] == G.H and out["hits"] > 100


def test_generic_view_is_never_walked_by_a_user_kernel():
    r = subprocess.run([USER], check=True, capture_output=True, text=True, timeout=120)
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["checked_ref_status"] == _capi.VRH_ERR_UNSUPPORTED
    assert out["declined_status"] == _capi.VRH_ERR_UNSUPPORTED and out["names_generic"] == 1
    assert out["wrong_pixels"] == 0                    # every call was declined: misses, never a record read as the wrong kind
    assert out["builtin_hits"] > 100 and out["centre_prim"] == 2
