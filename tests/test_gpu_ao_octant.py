"""GPU: the AO kernel's octant step (vrh_device.h OCTANT_STEP, vrh_octant.h).

The step fetches the near and the far planes of each axis from the piece of the 4-wide record that the sign of the
ray's inverse direction names, and forms tn / tf without sorting.  Every AO frame stays bit-identical to the oracle
(the C restatement of ao/main.cpp:183-246) -- colour bits, prim id, occlusion mask, t bits -- and traces the oracle's
number of rays, at 64x48:

  * room24 from inside: a closed axis-aligned room (the cube's six walls, normals inward) with an axis-aligned
    block on its floor (normals outward); the leaf boxes are flat on one axis;
  * hf16, a 16x16 heightfield;
  * soup60, 60 random triangles whose normals are set to the six axis directions in turn: the cosine-weighted AO
    rays about +x fill the four octants with dx > 0, and so on, so one frame's AO rays cover the eight octants (the
    oracle's frame is checked for hits with open and occluded samples under each of the six normals);
  * comb31 (tests/deep_cases.py), a tree of depth 30, deeper than the LDS part of the stack: the overflow-stack instance;
  * soup60_inverted: the soup's tree with one leaf box inverted on x, which build_quads refuses (no 4-wide records):
    its AO rays walk the binary records, which sort the box's planes as the oracle does;
  * frame numbers 0, 1 and 3, each as a one-frame launch and as the first of a batch of 4;
  * LDS stack entries (VRH_OPT_STACK_CAP) 1 and 8: 4-wide rays without room restart on the binary records.

The counting instance's box-test and primitive-test totals equal those of the parent commit's library over the same
views (frame 3), recorded from a run of that library in profiles/octant/counts.json -- not from the code under test.
"""
import functools
import json
import os

import numpy as np
import pytest

import visionaray_amd as va
from visionaray_amd import scenes

import deep_cases as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 64, 48
MISS = 0xFFFFFFFF
FIELDS = ("prim_id", "t", "occ", "color")
VIEWS = ("room24", "hf16", "soup60", "comb31", "soup60_inverted")
FRAMES = (0, 1, 3)
BATCH = 4
UP = (0.0, 1.0, 0.0)
RADIUS = {"room24": 1.0, "hf16": 0.3}            # AO radius (default 0.1): the room's and the terrain's occluders are farther
AXES = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.float32)


def soup(n):
    """n small random triangles in [-1, 1]^3 (a fixed draw); normal k is axis direction k mod 6"""
    rng = np.random.RandomState(60)
    v1 = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    e1 = rng.uniform(-0.6, 0.6, (n, 3)).astype(np.float32)
    e2 = rng.uniform(-0.6, 0.6, (n, 3)).astype(np.float32)
    prims = va.make_triangles(v1, e1, e2)
    normals = np.zeros((n, 4), np.float32)
    normals[:, :3] = AXES[np.arange(n) % 6]
    return prims, normals


def room(lo=(-0.6, -1.0, -0.7), hi=(-0.2, -0.5, -0.3)):
    """the six walls of [-1, 1]^3 with normals into the room, the six faces of the block [lo, hi] with normals out of it"""
    v1, e1, e2, nrm = [], [], [], []
    for bmin, bmax, sign in (((-1.0,) * 3, (1.0,) * 3, -1.0), (lo, hi, 1.0)):
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            for side in (0, 1):
                o = np.array(bmin, np.float32)
                o[a] = (bmin, bmax)[side][a]
                eb, ec, n = np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(4, np.float32)
                eb[b], ec[c] = bmax[b] - bmin[b], bmax[c] - bmin[c]
                n[a] = sign * (1.0 if side else -1.0)
                v1 += [o, o]; e1 += [eb, eb + ec]; e2 += [eb + ec, ec]; nrm += [n, n]
    return va.make_triangles(np.array(v1), np.array(e1), np.array(e2)), np.array(nrm, np.float32)


@functools.lru_cache(maxsize=None)
def host_scene(view):
    """(prims, nodes, indices, depth, normals, (eye, center)) of a view, read-only"""
    from oracle import oracle as O
    O.build()
    if view == "comb31":
        c = D.case(view)
        eye, center, _ = c.cameras["oblique"]
        return c.prims, c.nodes, c.indices, c.depth, c.normals, (eye, center)
    if view.startswith("soup"):
        prims, normals = soup(60)
        eye, center = (0.4, 1.5, 2.6), (0.0, 0.0, 0.0)
    elif view == "room24":
        prims, normals = room()
        eye, center = (0.7, 0.5, 0.8), (-0.8, -0.9, -0.9)             # from inside towards the block's corner
    else:
        prims = scenes.primitives(view)
        normals = scenes.normals_for(prims)
        eye, center = scenes.spec(view)[2], (0.0, 0.0, 0.0)
    nodes, idx, depth = O.build_bvh(prims.view(O.TRI_DTYPE), O.VO_TRI)
    nodes = nodes.view(va.BVH_NODE_DTYPE).copy()
    if view == "soup60_inverted":
        leaf = int(np.flatnonzero(nodes["num_prims"] != 0)[-1])
        lo, hi = nodes["bbox_min"][leaf, 0].copy(), nodes["bbox_max"][leaf, 0].copy()
        assert lo < hi
        nodes["bbox_min"][leaf, 0], nodes["bbox_max"][leaf, 0] = hi, lo
    for a in (prims, nodes, idx, normals):
        a.setflags(write=False)
    return prims, nodes, idx, int(depth), normals, (eye, center)


def camera(view):
    eye, center = host_scene(view)[5]
    cam = va.camera()
    cam.perspective(float(np.float32(45.0) * np.float32(va.DEGREES_TO_RADIANS)), float(np.float32(W) / np.float32(H)),
                    0.001, 1000.0)
    cam.look_at(tuple(float(x) for x in eye), tuple(float(x) for x in center), UP)
    return cam


@functools.lru_cache(maxsize=None)
def reference(view, frame):
    """the oracle's frame over the same tree (computed once per process, read-only)"""
    from oracle import oracle as O
    O.build()
    prims, nodes, idx, depth, normals, _ = host_scene(view)
    sc = O.Scene(view, O.VO_TRI, prims.view(O.TRI_DTYPE), nodes.view(O.NODE_DTYPE), idx, normals, depth)
    b = camera(view).basis(W, H)
    cam = tuple(np.array(x[:], np.float32) for x in (b.eye, b.cam_u, b.cam_v, b.cam_w)) + (W, H)
    ref = O.render(sc, cam, mode=O.VO_MODE_AO, radius=RADIUS.get(view, 0.1), frame_num=frame)
    for k in FIELDS:
        ref[k].setflags(write=False)
    return ref


_devices = {}


def device(ctx, view):
    if view not in _devices:
        prims, nodes, idx, depth, normals, _ = host_scene(view)
        d = va.hip_index_bvh(ctx, va.index_bvh(prims.view(va.TRIANGLE_DTYPE), nodes.view(va.BVH_NODE_DTYPE), idx, depth), normals)
        assert (d.info["wide_records"] > 0) == (view != "soup60_inverted")       # build_quads refuses the inverted box
        _devices[view] = d
    return _devices[view]


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, ref, what, lo=0):
    for k in FIELDS:
        a = _bits(got[k])[lo:lo + W * H]
        assert np.array_equal(a.reshape(-1), _bits(ref[k]).reshape(-1)), f"{what}: {k}"


def one_frame(ctx, view, frame, count=False):
    rt = va.hip_buffer_rt(ctx, W, H)
    va.hip_sched(ctx).frame(va.ao_kernel(device(ctx, view), radius=RADIUS.get(view, 0.1), count_tests=count), va.make_sched_params(camera(view), rt),
                            frame_num=frame)
    out = rt.download()
    rt.close()
    return out, ctx.last_frame_stats()


def batch(ctx, view, frame):
    rt = va.hip_buffer_rt(ctx, W, BATCH * H)
    d = device(ctx, view)
    va.render_batch(ctx, d, rt, [camera(view).basis(W, H)] * BATCH, va.ao_kernel(d, radius=RADIUS.get(view, 0.1)), None, frame_num=frame)
    out = rt.download()
    rt.close()
    return out, ctx.last_frame_stats()


def check_launches(ctx, view, frame, what):
    got, st = one_frame(ctx, view, frame)
    same(got, reference(view, frame), f"{what}, one frame")
    assert int(st["rays"]) == reference(view, frame)["rays"], f"{what}, one frame: rays"
    got, st = batch(ctx, view, frame)
    for f in range(BATCH):
        same(got, reference(view, frame + f), f"{what}, frame {f} of the batch", lo=f * W * H)
    assert int(st["rays"]) == sum(reference(view, frame + f)["rays"] for f in range(BATCH)), f"{what}, batch: rays"


def counts(ctx, view):
    """the counting instance's frame 3 and its (box_tests, prim_tests)"""
    got, st = one_frame(ctx, view, 3, count=True)
    return got, [int(st["box_tests"]), int(st["prim_tests"])]


def test_the_views_exercise_the_step():
    """not vacuous: every view has hits with open and occluded samples; the soup has them under each of the six axis
    normals; the room is closed and its leaves are flat; the comb is deeper than the LDS part of the stack"""
    for view in VIEWS:
        ref = reference(view, 3)
        hit = ref["prim_id"] != MISS
        assert hit.any(), view
        assert (ref["occ"][hit] != 0).any() and (ref["occ"][hit] != 0xFF).any(), view
    normals = host_scene("soup60")[4]
    ref = reference("soup60", 3)
    hit = ref["prim_id"] != MISS
    mixed = hit & (ref["occ"] != 0) & (ref["occ"] != 0xFF)
    assert {tuple(int(x) for x in normals[p, :3]) for p in np.unique(ref["prim_id"][mixed])} == {tuple(int(x) for x in a) for a in AXES}
    assert (reference("room24", 3)["prim_id"] != MISS).all()                # closed: no primary ray leaves the room
    nodes = host_scene("room24")[1]
    leaves = nodes[nodes["num_prims"] != 0]
    assert ((leaves["bbox_min"][:, :3] == leaves["bbox_max"][:, :3]).sum(axis=1) == 1).any()     # flat on one axis
    assert host_scene("comb31")[3] == 30


@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("view", VIEWS)
def test_frames_equal_the_oracle(ctx, view, frame):
    check_launches(ctx, view, frame, f"{view} frame {frame}")
    if view == "comb31":
        assert ctx.last_frame_stats()["stack_depth"] >= 30


@pytest.mark.parametrize("cap", [1, 8])
@pytest.mark.parametrize("view", ["room24", "hf16", "soup60", "comb31"])
def test_stack_caps_restart_on_the_binary_records(ctx, view, cap):
    ctx.set_option("stack_cap", cap)
    try:
        check_launches(ctx, view, 3, f"{view} stack_cap {cap}")
    finally:
        ctx.set_option("stack_cap", 0)


@pytest.mark.parametrize("view", VIEWS)
def test_counted_tests_equal_the_parents(ctx, view):
    with open(os.path.join(ROOT, "profiles", "octant", "counts.json")) as f:
        parent = json.load(f)["parent"]
    got, c = counts(ctx, view)
    print(f"{view}: box_tests {c[0]} prim_tests {c[1]}, parent {parent[view]}")
    same(got, reference(view, 3), "counting instance")
    assert c[0] > 0 and c[1] > 0
    assert c == parent[view]
