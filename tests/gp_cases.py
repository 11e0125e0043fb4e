"""Mixed triangle / sphere scenes (VRH_PRIM_GENERIC80), shared by tests/test_generic_build.py (CPU) and
tests/test_gpu_generic.py / tests/test_gpu_cpp_generic.py (GPU): the fixtures tests/golden/gp_<case>.npz
(tests/golden/make_generic_primitive_golden.py: the reference's own trees and frames) and the small scenes
of the identity tests.

Also the randomized sweep of the generic instances against the oracle's VO_GENERIC mode: sweep_case(seed) draws
scene, camera, image size, kernel, shading, frame number and launch option from the seed alone.  The fixture
maker draws gp_sweep from the same generator (sweep_scene, sweep_shading, sweep_camera), tests/test_oracle_generic.py
checks the sweep's coverage on the oracle's frames (CPU) and tests/test_gpu_fuzz_generic.py renders it (GPU).

DEPTH_LIMIT: the deepest generic BVH each kernel's launch plan accepts at default options (the whole stack in
LDS, no overflow block), as tests/cpp/launch_plan_check.cpp limits prints them."""
import ctypes as C
import functools
import json
import os

import numpy as np

import visionaray_amd as va
from visionaray_amd import _capi

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["gp_example", "gp_soup", "gp_inside", "gp_sweep"]
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


# ---- the randomized sweep ---------------------------------------------------------------------------------

def random_plastics(rng, n):
    """plastics with a diffuse part in every channel"""
    return np.stack([va.plastic(ca=rng.uniform(0.0, 0.3, 3), ka=rng.uniform(0.3, 1.0), cd=rng.uniform(0.2, 0.9, 3),
                                kd=rng.uniform(0.5, 1.0), cs=rng.uniform(0.3, 1.0, 3), ks=rng.uniform(0.2, 0.8),
                                exp=float(rng.choice([8.0, 16.0, 32.0, 64.5]))) for _ in range(n)])


def sweep_scene(rng, nt, ns, spread=1.0, min_size=1e-3):
    """(generic records, triangles, spheres): nt triangles whose sizes span min_size .. 0.3 (about 5 % slivers, as
    tests/test_gpu_fuzz.py::_scene draws them) and ns spheres of radius min_size .. 0.2 with centres in
    [-spread, spread]^3 (they overlap each other and the triangles), interleaved at random in prim order,
    geom_id = prim_id % 4"""
    order = rng.permutation(np.concatenate([np.zeros(nt, np.uint8), np.ones(ns, np.uint8)]))
    ids = np.arange(nt + ns, dtype=np.uint32)
    c = rng.uniform(-spread, spread, (nt, 3))
    size = 10.0 ** rng.uniform(np.log10(min_size), np.log10(0.3), (nt, 1))
    e1 = rng.standard_normal((nt, 3)) * size
    e2 = rng.standard_normal((nt, 3)) * size
    sliver = rng.random(nt) < 0.05                           # nearly degenerate: e2 ~ parallel to e1
    k = int(sliver.sum())
    e2[sliver] = e1[sliver] * rng.uniform(0.5, 2.0, (k, 1)) + 1e-6 * rng.standard_normal((k, 3))
    tris = va.make_triangles(c - 0.5 * (e1 + e2), e1, e2, prim_id=ids[order == 0], geom_id=ids[order == 0] % 4)
    sph = va.make_spheres(rng.uniform(-spread, spread, (ns, 3)), (10.0 ** rng.uniform(np.log10(min_size), np.log10(0.2), ns)).astype(np.float32),
                          prim_id=ids[order == 1], geom_id=ids[order == 1] % 4)
    return va.make_generic(tris, sph, order), tris, sph


def sweep_shading(rng):
    """(four plastics by geom_id, one to three point lights)"""
    mats = random_plastics(rng, 4)
    lights = []
    for _ in range(int(rng.integers(1, 4))):
        d = rng.standard_normal(3)
        pos = d / np.linalg.norm(d) * rng.uniform(1.5, 4.0)
        lights.append(va.point_light(tuple(float(x) for x in pos), cl=tuple(rng.uniform(0.5, 1.0, 3)), kl=float(rng.uniform(0.5, 1.0)),
                                     constant_att=1.0, linear_att=float(rng.uniform(0.0, 0.2)), quadratic_att=float(rng.uniform(0.0, 0.1))))
    return mats, np.stack(lights)


def sweep_camera(rng, w, h, inside=None):
    """tests/test_gpu_fuzz.py::_camera: outside the cloud, or inside it in a quarter of the cases; `inside` = True
    draws again until the eye is inside"""
    from test_gpu_fuzz import _camera
    while True:
        cam = _camera(rng, w, h)
        # (an inside eye is drawn from [-0.5, 0.5]^3, an outside one at a distance of 1.5 or more)
        if inside is None or (float(np.abs(np.float64(cam.basis(w, h).eye[:])).max()) <= 0.5) == inside:
            return cam


def sphere_ids(prims):
    """is_sphere by prim_id of a list of generic records"""
    n = len(prims)
    rows = prims["type"] == va.GENERIC_TYPE_SPHERE
    ids = np.ascontiguousarray(prims["data"]).view(np.uint32).reshape(n, 16)[:, 1]
    out = np.zeros(n, bool)
    out[ids[rows]] = True
    return out


def mixed_leaves(nodes, indices, prims):
    """the number of leaves that hold both kinds (nodes as (n, 8) u32 rows)"""
    rows = prims["type"] == va.GENERIC_TYPE_SPHERE
    nodes = np.ascontiguousarray(nodes).view(np.uint32).reshape(-1, 8)
    mixed = 0
    for first, count in zip(nodes[:, 3], nodes[:, 7]):
        if count:
            kinds = rows[indices[first:first + count]]
            mixed += int(kinds.any() and not kinds.all())
    return mixed


BG = (0.1, 0.2, 0.3, 1.0)
AMBIENT = (1.0, 1.0, 1.0, 1.0)
AO_EPS = 1e-3
SWEEP_SEEDS = list(range(32))
# the seed of sweep case i is SWEEP_BASE + i.  A base is refused when the oracle's frames miss a coverage condition
# of tests/test_oracle_generic.py (never a condition relaxed).  Refused bases: 9000 .. 9029, each for a case with more
# than 7 primitives and 63 pixels whose frame has no miss or no hit, or whose AO rays are all occluded or all free
# (the first such case of each base: 18 24 11 12 14 20 5 6 7 9 1 7 3 2 1 0 2 1 0 9 5 9 3 2 1 0 9 29 9 25).
SWEEP_BASE = 9030
# what a seed fixes instead of drawing it: (triangles, spheres), (width, height) (None: drawn), launch option
SWEEP_COUNTS = {4: (None, 0), 10: (None, 0),           # no spheres
                6: (0, None), 11: (0, None),           # no triangles
                8: (3, 2), 13: (2, 1), 15: (4, 3),     # fewer than 8 primitives: a single leaf, or a tree 1 or 2 deep
                16: (1, 0), 17: (0, 1)}                # a single primitive of each kind
SWEEP_IMAGES = {9: (5, None), 14: (None, 3), 19: (1, 1), 22: (7, 6), 28: (1, None)}
# (every option of the list at least once; AO -- seeds 1, 5, 9 .. -- and whitted -- 3, 7, 11 .. -- at 256 threads)
SWEEP_OPTIONS = {1: ("block_threads", 256), 3: ("block_threads", 256), 5: ("ao_gate", 2), 7: ("pop_on_miss", 2),
                 12: ("descent_cap", 2), 18: ("refill_min", 32), 21: ("wide_anyhit", 2), 23: ("scalar_fetch", 2),
                 24: ("xcd_queues", 3), 25: ("ao_cut", 2), 26: ("exact_minmax", 1), 29: ("block_threads", 128),
                 30: ("wide_anyhit", 1)}


@functools.lru_cache(maxsize=None)
def sweep_case(i):
    """sweep case i as a dict: prims (generic records), tris, normals (by prim_id; a sphere's row stays 0), is_sphere
    (by prim_id), W, H, cam (the va.camera), camera (its vrh_camera basis), kind (KERNELS[i % 4]), spec (the parameter record
    kernel() takes, plus frame_num), materials, lights, option ((name, value) or None)"""
    rng = np.random.default_rng(SWEEP_BASE + i)
    nt, ns = int(rng.integers(0, 3001)), int(rng.integers(0, 2001))
    fixed = SWEEP_COUNTS.get(i, (None, None))
    nt, ns = (nt if fixed[0] is None else fixed[0]), (ns if fixed[1] is None else fixed[1])
    # (a handful of primitives: large ones near the origin, where every camera looks)
    prims, tris, sph = sweep_scene(rng, nt, ns, 0.3, 0.1) if nt + ns < 8 else sweep_scene(rng, nt, ns)
    w, h = int(rng.integers(1, 141)), int(rng.integers(1, 91))
    fixed = SWEEP_IMAGES.get(i, (None, None))
    w, h = (w if fixed[0] is None else fixed[0]), (h if fixed[1] is None else fixed[1])
    cam = sweep_camera(rng, w, h)
    mats, lights = sweep_shading(rng)
    spec = dict(bg=list(BG), ambient=list(AMBIENT), ao_samples=int(rng.choice([1, 2, 3, 5, 8, 32])),
                ao_radius=float(np.float32(10.0 ** rng.uniform(-2.0, 0.0))), ao_eps=AO_EPS, bounces=int(rng.integers(1, 6)),
                eps=float(rng.choice([1e-3, 1e-4])), frame_num=int(rng.integers(0, 50)))
    normals = np.zeros((nt + ns, 4), np.float32)
    if nt:
        normals[tris["prim_id"]] = va.face_normals(tris)
    out = dict(prims=prims, tris=tris, normals=normals, is_sphere=sphere_ids(prims), W=w, H=h, cam=cam, camera=cam.basis(w, h), kind=KERNELS[i % 4],
               spec=spec, materials=mats, lights=lights, option=SWEEP_OPTIONS.get(i))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def oracle_scene(O, name, prims, nodes, indices, normals, depth):
    """the oracle's Scene over generic records"""
    return O.Scene(name, O.VO_GENERIC, np.ascontiguousarray(prims), np.ascontiguousarray(nodes).view(O.NODE_DTYPE).reshape(-1),
                   np.ascontiguousarray(indices, np.uint32), np.ascontiguousarray(normals, np.float32), depth)


def oracle_camera(cam, w, h):
    """the oracle's camera tuple of a vrh_camera basis or of a fixture's (eye, u, v, w) rows"""
    if hasattr(cam, "cam_u"):
        cam = [cam.eye[:], cam.cam_u[:], cam.cam_v[:], cam.cam_w[:]]
    b = np.asarray(cam, np.float32)
    return (b[0], b[1], b[2], b[3], w, h)


def oracle_frame(O, sc, cam, kind, s, materials, lights):
    """the oracle's frame of kernel `kind` with the parameters of the spec record `s` (kernel()'s counterpart)"""
    m = np.ascontiguousarray(materials).view(np.float32).reshape(-1).view(O.PLASTIC_DTYPE)
    lt = np.ascontiguousarray(lights).view(np.float32).reshape(-1).view(O.POINT_LIGHT_DTYPE)
    bg, frame = tuple(s["bg"]), s.get("frame_num", 0)
    if kind == "primary":
        return O.render(sc, cam, mode=O.VO_MODE_PRIMARY, bg=bg)
    if kind == "ao":
        return O.render(sc, cam, mode=O.VO_MODE_AO, samples=s["ao_samples"], radius=s["ao_radius"], eps=s["ao_eps"], bg=bg,
                        frame_num=frame)
    mode = O.VO_MODE_SIMPLE if kind == "simple" else O.VO_MODE_WHITTED
    return O.render(sc, cam, mode=mode, materials=m, lights=lt, ambient=tuple(s["ambient"]), bg=bg, num_bounces=s["bounces"],
                    eps=s["eps"])


RTOL, ATOL = 1e-5, 1e-7        # tests/test_gpu_fuzz_shading.py


def assert_frame(out, ref, kind, samples=8, label=""):
    """every pixel of `out` against the oracle's frame under the bars above"""
    assert np.array_equal(out["prim_id"], ref["prim_id"]), f"prim_id: {int((out['prim_id'] != ref['prim_id']).sum())} pixels differ"
    assert same_bits(out["t"], ref["t"]), f"t: {int((out['t'].view(np.uint32) != ref['t'].view(np.uint32)).sum())} pixels differ"
    if kind in ("primary", "ao"):
        if kind == "primary" or samples <= 8:                  # (more than 8 samples: the kernel leaves the mask buffer alone)
            assert np.array_equal(out["occ"], ref["occ"]), f"occ: {int((out['occ'] != ref['occ']).sum())} pixels differ"
        assert same_bits(out["color"], ref["color"]), "colour"
        return
    miss = ref["prim_id"] == MISS
    assert same_bits(out["color"][miss], ref["color"][miss])
    hit = ~miss
    rel = np.abs(out["color"][hit] - ref["color"][hit]) / np.maximum(np.abs(ref["color"][hit]), 1e-30)
    print(label, kind, "max rel diff %.3g" % (float(rel.max()) if hit.any() else 0.0))
    np.testing.assert_allclose(out["color"], ref["color"], rtol=RTOL, atol=ATOL)       # every pixel, the misses again


# the deepest generic BVH the launch plan accepts per kernel at default options (64 threads per block: 256 bytes of LDS
# per stack entry, entries in fours, 160 KiB per CU less the AO kernel's per-wave area / whitted's bounce surface)
DEPTH_LIMIT = {"primary": 640, "ao": 628, "simple": 640, "whitted": 628}


@functools.lru_cache(maxsize=None)
def sweep_reference(i):
    """(the oracle's Scene of sweep case i over the oracle's own tree, the oracle's frame of the case's kernel);
    computed once per process, read-only"""
    from oracle import oracle as O
    O.build()
    c = sweep_case(i)
    nodes, idx, depth = O.build_bvh(c["prims"], O.VO_GENERIC)
    sc = oracle_scene(O, "sweep%d" % i, c["prims"], nodes, idx, c["normals"], depth)
    ref = oracle_frame(O, sc, oracle_camera(c["camera"], c["W"], c["H"]), c["kind"], c["spec"], c["materials"], c["lights"])
    for a in [sc.nodes, sc.indices] + [v for v in ref.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return sc, ref
