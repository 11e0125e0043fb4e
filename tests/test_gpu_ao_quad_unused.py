"""GPU: the AO kernel's 4-wide step without its link compares (vrh_device.h NEVER_HIT_UNUSED).

The default build uploads every unused entry of a 4-wide record as a point box at +inf (vrh_quad.cpp), which no
finite ray passes, and the AO kernel's step no longer compares the entries' links with QUAD_NONE.  Every AO frame
stays bit-identical to the oracle (the C restatement of ao/main.cpp:183-246) -- prim id, t bits, occlusion masks,
colour bits:

  * scenes of 3, 5 and 7 triangles under hand-made trees of one triangle per leaf, split in halves: the root
    record of the first has 3 children, the others' lower records 2 (tests/cpp/quad_unused_check.cpp has the same
    trees on the host), at 72x40;
  * hf200 at 72x40 (whole tiles) and 75x43 (partial tiles on both edges);
  * radii 0.002, 0.1, 8.0, and inf, whose rays walk the binary records;
  * LDS stack entries (VRH_OPT_STACK_CAP) 0 (auto), 1, 8 and 12; the entry cut (VRH_OPT_AO_CUT) 0 (auto) and 2 (off);
  * one frame, and three frames in flight.

The counting instance keeps counting four box tests per record (the tests are still made), so its box-test and
primitive-test counts equal the parent commit's.  PARENT_COUNTS was recorded from a run of the parent commit's
library over these views (one frame, frame number 3, default stack and cut), not from the code under test.
"""
import functools

import numpy as np
import pytest

import visionaray_amd as va
from visionaray_amd import scenes

pytestmark = pytest.mark.gpu

MISS = 0xFFFFFFFF
FIELDS = ("prim_id", "t", "occ", "color")
VIEWS = {"tri3": ("tri3", 72, 40), "tri5": ("tri5", 72, 40), "tri7": ("tri7", 72, 40),
         "hf200_72x40": ("hf200", 72, 40), "hf200_75x43": ("hf200", 75, 43)}
RADII = [0.002, 0.1, 8.0, float("inf")]
CAPS = [0, 1, 8, 12]
CUTS = [0, 2]
FRAME0 = 2                                   # three frames in flight: 2, 3, 4; one frame: 3
EYE, CENTER, UP = (0.4, 1.5, 1.9), (-0.5, 0.0, -0.5), (0.0, 1.0, 0.0)

# (box_tests, prim_tests) of the counting instance of the PARENT commit's library, one frame (frame number 3), default
# stack capacity and cut
PARENT_COUNTS = {
    ("tri3", 0.002): (37292, 2037),
    ("tri3", 0.1): (37292, 2253),
    ("tri3", 8.0): (37292, 2394),
    ("tri3", float("inf")): (22640, 2394),
    ("tri5", 0.002): (42470, 2397),
    ("tri5", 0.1): (42946, 2549),
    ("tri5", 8.0): (45062, 3219),
    ("tri5", float("inf")): (44884, 3219),
    ("tri7", 0.002): (45952, 3080),
    ("tri7", 0.1): (47060, 3264),
    ("tri7", 8.0): (50076, 3940),
    ("tri7", float("inf")): (48290, 3942),
    ("hf200_72x40", 0.002): (407270, 62002),
    ("hf200_72x40", 0.1): (473190, 68237),
    ("hf200_72x40", 8.0): (551362, 68941),
    ("hf200_72x40", float("inf")): (538592, 68886),
    ("hf200_75x43", 0.002): (458462, 69784),
    ("hf200_75x43", 0.1): (536102, 77130),
    ("hf200_75x43", 8.0): (629322, 77870),
    ("hf200_75x43", float("inf")): (615076, 77853),
}


def tiny_prims(n):
    """a floor triangle and n - 1 small tilted ones hovering 0.03 .. 0.2 above it"""
    p = np.zeros(n, va.TRIANGLE_DTYPE)
    p["prim_id"] = np.arange(n, dtype=np.uint32)
    p["v1"][0, :3] = (-2.0, 0.0, -2.0)
    p["e1"][0, :3] = (0.0, 0.0, 4.0)
    p["e2"][0, :3] = (4.0, 0.0, 0.0)
    for i in range(1, n):
        p["v1"][i, :3] = (-1.4 + 0.22 * i, 0.03 * i, -1.3 + 0.2 * i)
        p["e1"][i, :3] = (0.05, 0.02 * (i % 3), 0.5)
        p["e2"][i, :3] = (0.5, 0.03, -0.04 * i)
    return p


def tiny_tree(p):
    """one triangle per leaf, leaves [lo, hi) split in halves, children adjacent; every box the exact float32
    bounds of its triangles, so every child's box lies inside its parent's"""
    v = np.stack([p["v1"][:, :3], p["v1"][:, :3] + p["e1"][:, :3], p["v1"][:, :3] + p["e2"][:, :3]], axis=1).astype(np.float32)
    nodes = [None]
    depth = [0]

    def fill(k, lo, hi, d):
        depth[0] = max(depth[0], d)
        bmin, bmax = v[lo:hi].min(axis=(0, 1)), v[lo:hi].max(axis=(0, 1))
        if hi - lo == 1:
            nodes[k] = (bmin, lo, bmax, 1)
            return
        fc = len(nodes)
        nodes.extend([None, None])
        nodes[k] = (bmin, fc, bmax, 0)
        mid = lo + (hi - lo) // 2
        fill(fc, lo, mid, d + 1)
        fill(fc + 1, mid, hi, d + 1)

    fill(0, 0, len(p), 0)
    out = np.zeros(len(nodes), va.BVH_NODE_DTYPE)
    for k, (bmin, first, bmax, count) in enumerate(nodes):
        out[k] = (bmin, first, bmax, count)
    return out, np.arange(len(p), dtype=np.uint32), depth[0]


def camera(name, w, h):
    if name == "hf200":
        return scenes.scene_camera(name, w, h)[0]
    cam = va.camera()
    cam.perspective(float(np.float32(45.0) * np.float32(va.DEGREES_TO_RADIANS)), float(np.float32(w) / np.float32(h)),
                    0.001, 1000.0)
    cam.look_at(EYE, CENTER, UP)
    return cam


def oracle_camera(cam, w, h):
    b = cam.basis(w, h)
    return tuple(np.array(x[:], np.float32) for x in (b.eye, b.cam_u, b.cam_v, b.cam_w)) + (w, h)


@functools.lru_cache(maxsize=None)
def host_scene(name):
    """(prims, nodes, indices, depth, normals) of a scene: the library's builder for hf200, the hand-made trees"""
    if name == "hf200":
        prims = scenes.primitives(name)
        bvh = va.build_index_bvh(prims)
        return prims, bvh.nodes, bvh.indices, bvh.max_depth, scenes.normals_for(prims)
    prims = tiny_prims(int(name[3:]))
    nodes, idx, depth = tiny_tree(prims)
    return prims, nodes, idx, depth, va.face_normals(prims)


_devices = {}


def device(ctx, name):
    if name not in _devices:
        prims, nodes, idx, depth, nrm = host_scene(name)
        d = va.hip_index_bvh(ctx, va.index_bvh(prims, nodes, idx, depth), nrm)
        assert d.info["wide_records"] > 0
        if name != "hf200":
            # leaves minus one inner nodes, every second level skipped: 1, 2 and 4 records
            assert d.info["wide_records"] == {3: 1, 5: 2, 7: 4}[len(prims)]
        _devices[name] = d
    return _devices[name]


@functools.lru_cache(maxsize=None)
def reference(view, radius, frame):
    """the oracle's frame over the same tree (computed once per process, read-only)"""
    from oracle import oracle as O
    O.build()
    name, w, h = VIEWS[view]
    prims, nodes, idx, depth, nrm = host_scene(name)
    sc = O.Scene(name, O.VO_TRI, prims.view(O.TRI_DTYPE), nodes.view(O.NODE_DTYPE), idx, nrm, depth)
    ref = O.render(sc, oracle_camera(camera(name, w, h), w, h), mode=O.VO_MODE_AO, radius=radius, frame_num=frame)
    for k in FIELDS:
        ref[k].setflags(write=False)
    return ref


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, ref, what, lo=0, n=None):
    for k in FIELDS:
        a = _bits(got[k])
        a = a[lo:lo + n] if n else a
        assert np.array_equal(a.reshape(-1), _bits(ref[k]).reshape(-1)), f"{what}: {k}"


def one_frame(ctx, d, view, radius, count=False):
    name, w, h = VIEWS[view]
    rt = va.hip_buffer_rt(ctx, w, h)
    va.hip_sched(ctx).frame(va.ao_kernel(d, radius=radius, count_tests=count), va.make_sched_params(camera(name, w, h), rt),
                            frame_num=FRAME0 + 1)
    out = rt.download()
    rt.close()
    return out


def three_frames(ctx, d, view, radius):
    name, w, h = VIEWS[view]
    rt = va.hip_buffer_rt(ctx, w, 3 * h)
    va.render_batch(ctx, d, rt, [camera(name, w, h).basis(w, h)] * 3, va.ao_kernel(d, radius=radius), None, frame_num=FRAME0)
    out = rt.download()
    rt.close()
    return out


def counts(ctx, view, radius):
    """the counting instance's frame and its (box_tests, prim_tests)"""
    got = one_frame(ctx, device(ctx, VIEWS[view][0]), view, radius, count=True)
    st = ctx.last_frame_stats()
    return got, (int(st["box_tests"]), int(st["prim_tests"]))


def test_the_views_exercise_the_step():
    """not vacuous: every view has hits; at radius 0.1 and above samples are occluded and open on every view"""
    for view in VIEWS:
        for radius in RADII:
            ref = reference(view, radius, FRAME0 + 1)
            assert (ref["prim_id"] != MISS).any(), (view, radius)
            if radius >= 0.1:
                occ = ref["occ"][ref["prim_id"] != MISS]
                assert (occ != 0).any() and (occ != 0xFF).any(), (view, radius)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("view", list(VIEWS))
def test_frames_equal_the_oracle(ctx, view, radius):
    name, w, h = VIEWS[view]
    d = device(ctx, name)
    refs = [reference(view, radius, FRAME0 + f) for f in range(3)]
    for cap in CAPS:
        for cut in CUTS:
            ctx.set_option("stack_cap", cap)
            ctx.set_option("ao_cut", cut)
            try:
                one = one_frame(ctx, d, view, radius)
                three = three_frames(ctx, d, view, radius)
            finally:
                ctx.set_option("stack_cap", 0)
                ctx.set_option("ao_cut", 0)
            same(one, refs[1], f"cap {cap} cut {cut}, one frame")
            for f in range(3):
                same(three, refs[f], f"cap {cap} cut {cut}, frame {f} of 3 in flight", lo=f * w * h, n=w * h)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("view", list(VIEWS))
def test_counted_tests_equal_the_parents(ctx, view, radius):
    got, c = counts(ctx, view, radius)
    print(f"{view} radius {radius}: box_tests {c[0]} prim_tests {c[1]}, parent {PARENT_COUNTS[(view, radius)]}")
    same(got, reference(view, radius, FRAME0 + 1), "counting instance")
    assert c[0] > 0 and c[1] > 0
    assert c == PARENT_COUNTS[(view, radius)]
