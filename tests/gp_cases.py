"""Mixed triangle / sphere scenes (VRH_PRIM_GENERIC80), shared by tests/test_generic_build.py (CPU) and
tests/test_gpu_generic.py / tests/test_gpu_cpp_generic.py (GPU): the fixtures tests/golden/gp_<case>.npz
(tests/golden/make_generic_primitive_golden.py: the reference's own trees and frames) and the small scenes
of the identity tests."""
import ctypes as C
import functools
import json
import os

import numpy as np

import visionaray_amd as va
from visionaray_amd import _capi

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["gp_example", "gp_soup", "gp_inside"]
MISS = 0xFFFFFFFF
W, H = 60, 44


@functools.lru_cache(maxsize=None)
def spec():
    with open(os.path.join(HERE, "golden", "generic_primitive.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def fixture(case):
    """the arrays of a fixture (read-only; loaded once per process), `prims` as GENERIC_DTYPE records"""
    with np.load(os.path.join(HERE, "golden", case + ".npz")) as z:
        a = {k: z[k] for k in z.files}
    a["records"] = np.ascontiguousarray(a["prims"]).view(va.GENERIC_DTYPE).reshape(-1)
    for v in a.values():
        v.setflags(write=False)
    return a


def host_bvh(case):
    """the fixture's records under the reference's own nodes and indices"""
    a = fixture(case)
    nodes = np.ascontiguousarray(a["nodes"]).view(va.BVH_NODE_DTYPE).reshape(-1)
    return va.index_bvh(a["records"], nodes, a["indices"], tree_depth(nodes))


def tree_depth(nodes):
    depth, todo = 0, [(0, 0)]
    while todo:
        i, d = todo.pop()
        depth = max(depth, d)
        if nodes[i]["num_prims"] == 0:
            todo += [(int(nodes[i]["first"]), d + 1), (int(nodes[i]["first"]) + 1, d + 1)]
    return depth


def camera_of(basis, w=W, h=H):
    """vrh_camera from the recorded basis (eye, u, v, w rows): the bits the reference's frames were traced with"""
    cam = _capi.vrh_camera()
    b = np.asarray(basis, np.float32)
    cam.eye[:], cam.cam_u[:], cam.cam_v[:], cam.cam_w[:] = (list(map(float, r)) for r in b)
    cam.width, cam.height = w, h
    return cam


def shading_of(ctx, a):
    return va.shading(ctx, np.ascontiguousarray(a["materials"]).view(va.PLASTIC_DTYPE).reshape(-1),
                      np.ascontiguousarray(a["lights"]).view(va.POINT_LIGHT_DTYPE).reshape(-1))


KERNELS = ["primary", "ao", "simple", "whitted"]


def kernel(kind, dev, sh, s):
    """the built-in kernel `kind` with the parameters of the spec record `s` (generic_primitive.json's fields)"""
    bg, amb = tuple(s["bg"]), tuple(s["ambient"])
    if kind == "primary":
        return va.closest_hit_kernel(dev, bg=bg)
    if kind == "ao":
        return va.ao_kernel(dev, samples=s["ao_samples"], radius=s["ao_radius"], eps=s["ao_eps"], bg=bg)
    if kind == "simple":
        return va.simple_kernel(dev, sh, bg=bg, ambient=amb)
    assert kind == "whitted"
    return va.whitted_kernel(dev, sh, bg=bg, ambient=amb, num_bounces=s["bounces"], epsilon=s["eps"])


def render(ctx, dev, cam, k, w=W, h=H):
    rt = va.hip_buffer_rt(ctx, w, h)
    va.render(ctx, dev, rt, cam, k)
    ctx.sync()
    out = rt.download()
    rt.close()
    return out


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def random_mixed(seed, nt, ns):
    """(triangles, spheres) with prim ids 0 .. nt - 1 and nt .. nt + ns - 1, geom_id = prim_id % 4, in [-1, 1]^3"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.9, 0.9, (nt, 3))
    size = 10.0 ** rng.uniform(-1.0, -0.4, (nt, 1))
    f1, f2 = rng.standard_normal((nt, 3)) * size, rng.standard_normal((nt, 3)) * size
    ids = np.arange(nt + ns, dtype=np.uint32)
    tris = va.make_triangles(c - 0.5 * (f1 + f2), f1, f2, prim_id=ids[:nt], geom_id=ids[:nt] % 4)
    sph = va.make_spheres(rng.uniform(-0.9, 0.9, (ns, 3)), 10.0 ** rng.uniform(-1.4, -0.8, ns), prim_id=ids[nt:], geom_id=ids[nt:] % 4)
    return tris, sph


def outside_camera(w=W, h=H):
    cam = va.camera()
    cam.perspective(0.8, np.float32(w) / np.float32(h), 0.001, 1000.0)
    cam.look_at((1.9, 1.4, 2.3), (0.0, 0.0, 0.0))
    return cam.basis(w, h)


def build(prims):
    """vrh_build_bvh as (nodes as (n, 8) u32, indices, depth)"""
    b = va.build_index_bvh(prims)
    return b.nodes.view(np.uint32).reshape(-1, 8), b.indices, b.max_depth


def build_status(prims):
    """the raw status of vrh_build_bvh on `prims` (GENERIC_DTYPE)"""
    n = len(prims)
    nodes = np.zeros(2 * n, va.BVH_NODE_DTYPE)
    idx = np.zeros(n, np.uint32)
    nn, depth = C.c_uint32(0), C.c_uint32(0)
    return _capi.lib().vrh_build_bvh(prims.ctypes.data_as(C.c_void_p), n, _capi.VRH_PRIM_GENERIC80, nodes.ctypes.data_as(C.c_void_p),
                                     C.byref(nn), idx.ctypes.data_as(C.c_void_p), C.byref(depth))
