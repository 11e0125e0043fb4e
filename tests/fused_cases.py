"""GPU cases of the fused 4-wide records, run by tests/test_gpu_ao_fused.py in a process of its own that loads
libvrh_fused.so (the build with the fused step compiled in, VRH_FUSED_STEP); not collected by name.

The AO kernel over the fused records (vrh_fused_slab.h: boxes widened at upload, one fma per slab distance, every
leaf verified against its exact box) leaves every AO frame bit-identical to the oracle -- prim id, t bits, colour
bits, occlusion masks.

Views: hf24 at 72x40 and 75x43 under the camera of test_gpu_ao_handout.py (empty, single-hit, full and partial
tiles), hf200 at 320x180.  Radii 0.002, 0.1, 8.0 and inf (no 4-wide rays).  One frame and three frames in flight,
each with 1 and with 8 LDS stack entries (restarts on the binary records mix with the verification).  The whole
set at the derived widening and with VRH_OPT_FUSED_WIDEN at 1/8 and 1/2 of the scene extent, where the counting
instance must report rejected leaves.  Further: the byte-mask intersector on hf64, eight cases of
test_gpu_fuzz.py's generator at a widening of 1/8, and a tree that fails the nesting check (no fused records).

Every verification case prints the counting instance's checks and rejects before it asserts.
"""
import functools
import os
import sys

import numpy as np
import pytest

import visionaray_amd as va
from visionaray_amd import scenes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_ao_handout as handout  # noqa: E402
import test_gpu_fuzz as fuzz  # noqa: E402
import test_gpu_mask as mask_tests  # noqa: E402

pytestmark = pytest.mark.gpu

VIEWS = {"hf24_72x40": ("hf24", 72, 40), "hf24_75x43": ("hf24", 75, 43), "hf200_320x180": ("hf200", 320, 180)}
RADII = [0.002, 0.1, 8.0, float("inf")]
WIDEN = {"derived": 0, "eighth": 3, "half": 1}          # VRH_OPT_FUSED_WIDEN: the extent x 2^-value
FRAME0 = 2                                              # three frames in flight: 2, 3, 4; one frame: 3


def upload(ctx, bvh, normals, widen):
    """the scene uploaded under the widening option (read by vrh_scene_upload only)"""
    ctx.set_option("fused_widen", widen)
    try:
        return va.hip_index_bvh(ctx, bvh, normals)
    finally:
        ctx.set_option("fused_widen", 0)


_devices = {}


def device(ctx, name, widen):
    if (name, widen) not in _devices:
        prims = scenes.primitives(name)
        d = upload(ctx, va.build_index_bvh(prims), scenes.normals_for(prims), widen)
        assert d.info["wide_records"] > 0
        assert d.info["fused_records"] == d.info["wide_records"]        # the builder's trees nest
        # the records again, and the exact leaf boxes: two float4 per leaf-ordered primitive
        assert d.info["fused_bytes"] == 128 * d.info["wide_records"] + 32 * d.info["num_indices"]
        _devices[(name, widen)] = d
    return _devices[(name, widen)]


def view_camera(view):
    name, w, h = VIEWS[view]
    if name == "hf24":
        return handout.camera(w, h)
    return scenes.scene_camera(name, w, h)[0]


@functools.lru_cache(maxsize=None)
def _oracle_scene(name):
    from oracle import oracle as O
    O.build()
    return O.make_scene(name)


@functools.lru_cache(maxsize=None)
def reference(view, radius, frame):
    """the oracle's frame (computed once per process, read-only)"""
    from oracle import oracle as O
    name, w, h = VIEWS[view]
    ref = O.render(_oracle_scene(name), handout.oracle_camera(view_camera(view), w, h), mode=O.VO_MODE_AO,
                   radius=radius, frame_num=frame)
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref


def one_frame(ctx, d, view, radius, count=False):
    _, w, h = VIEWS[view]
    rt = va.hip_buffer_rt(ctx, w, h)
    va.hip_sched(ctx).frame(va.ao_kernel(d, radius=radius, count_tests=count), va.make_sched_params(view_camera(view), rt),
                            frame_num=FRAME0 + 1)
    out = rt.download()
    rt.close()
    return out


def three_frames(ctx, d, view, radius):
    _, w, h = VIEWS[view]
    rt = va.hip_buffer_rt(ctx, w, 3 * h)
    va.render_batch(ctx, d, rt, [view_camera(view).basis(w, h)] * 3, va.ao_kernel(d, radius=radius), None, frame_num=FRAME0)
    out = rt.download()
    rt.close()
    return out


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("view", list(VIEWS))
@pytest.mark.parametrize("widen", list(WIDEN))
def test_frames_equal_the_oracle(ctx, widen, view, radius):
    name, w, h = VIEWS[view]
    d = device(ctx, name, WIDEN[widen])
    refs = [reference(view, radius, FRAME0 + f) for f in range(3)]
    assert (refs[1]["prim_id"] != handout.MISS).any()
    for cap in (1, 8):
        ctx.set_option("stack_cap", cap)
        try:
            handout.check(one_frame(ctx, d, view, radius), refs[1])
            got = three_frames(ctx, d, view, radius)
        finally:
            ctx.set_option("stack_cap", 0)
        for f in range(3):
            handout.check(got, refs[f], rows=(f * w * h, (f + 1) * w * h))


def counted(ctx, widen, view, radius):
    """the counting instance's frame of a case: equal to the oracle's too; its verification counts"""
    d = device(ctx, VIEWS[view][0], WIDEN[widen])
    handout.check(one_frame(ctx, d, view, radius, count=True), reference(view, radius, FRAME0 + 1))
    st = ctx.last_handout_stats()
    print(f"{widen} {view} radius {radius}: checks {st['fused_checks']} rejects {st['fused_rejects']} "
          f"of {st['ao_handout_rays']} AO rays, occluded samples {int(np.unpackbits(reference(view, radius, FRAME0 + 1)['occ']).sum())}")
    assert st["fused_rejects"] <= st["fused_checks"]
    return st


@pytest.mark.parametrize("widen", list(WIDEN))
def test_verification_runs_and_decides(ctx, widen):
    """Over the whole set of views and radii: leaves are checked against their exact boxes; at the exaggerated
    widenings some must be rejected.  (Measured, checks / rejects summed over the set: derived 948,663 / 335,
    eighth 56,676,376 / 56,589,295, half 496,283 / 492,838 -- at a half, most rays fill the LDS part of the stack
    and restart on the binary records.  With the test after a hit instead (measured and since removed), no widening
    gives a reject on these views: a ray that hits a triangle crosses the leaf's box, which contains it.)"""
    checks = rejects = 0
    for view in VIEWS:
        for radius in RADII:
            st = counted(ctx, widen, view, radius)
            if radius == float("inf"):
                assert st["fused_checks"] == 0          # a radius beyond FLT_MAX walks the binary records
            checks += st["fused_checks"]
            rejects += st["fused_rejects"]
    print(f"{widen}: checks {checks} rejects {rejects}")
    if WIDEN[widen] == 0:
        assert checks > 0
    else:
        assert rejects > 0


@pytest.mark.parametrize("widen", list(WIDEN))
def test_byte_mask_intersector(ctx, golden, widen):
    g, ref, tc, mask = mask_tests.case_inputs(golden, "mask_hf64_160x90")
    d = device(ctx, g["scene"], WIDEN[widen])
    m = va.hit_mask(ctx, tc, mask)
    cam = scenes.scene_camera(g["scene"], g["W"], g["H"])[0]
    rt = va.hip_buffer_rt(ctx, g["W"], g["H"])
    va.render_batch(ctx, d, rt, [cam.basis(g["W"], g["H"])], va.with_hit_mask(va.ao_kernel(d), m))
    mask_tests.assert_equal_frame(rt.download(), ref)
    rt.close()
    m.close()


@pytest.mark.parametrize("seed", [0, 1, 4, 5, 8, 9, 12, 13])       # the generator's AO cases (triangles, seed % 4 < 2)
def test_fuzz_cases_at_an_eighth(ctx, oracle_mod, seed):
    O = oracle_mod
    rng = np.random.default_rng(1000 + seed)
    prims = fuzz._scene(rng, "tri")
    bvh = va.build_index_bvh(prims)
    nrm = va.face_normals(prims)
    d = upload(ctx, bvh, nrm, 3)
    assert d.info["fused_records"] == d.info["wide_records"]
    W, H = int(rng.integers(9, 140)), int(rng.integers(7, 90))
    samples, radius = int(rng.integers(1, 9)), float(np.float32(10.0 ** rng.uniform(-2.0, 0.0)))
    kern = va.ao_kernel(d, samples=samples, radius=radius)
    osc = O.Scene(f"fused{seed}", O.VO_TRI, prims, bvh.nodes, bvh.indices, nrm, bvh.max_depth)
    frame0 = int(rng.integers(0, 50))
    cams = [fuzz._camera(rng, W, H) for _ in range(3)]
    bases = [c.basis(W, H) for c in cams]
    refs = [O.render(osc, fuzz._ocam(b, W, H), mode=O.VO_MODE_AO, samples=samples, radius=radius, frame_num=frame0 + f)
            for f, b in enumerate(bases)]
    rt = va.hip_buffer_rt(ctx, W, H)
    va.hip_sched(ctx).frame(kern, va.make_sched_params(cams[0], rt), frame_num=frame0)
    fuzz._same(rt.download(), refs[0])
    rt.close()
    rtb = va.hip_buffer_rt(ctx, W, 3 * H)
    va.render_batch(ctx, d, rtb, bases, kern, frame_num=frame0)
    got = rtb.download()
    rtb.close()
    for f in range(3):
        fuzz._same(got, refs[f], f * W * H, W * H)
    d.close()


def test_tree_that_fails_the_nesting_check(ctx, oracle_mod):
    """hf24's tree with one bound of a child of the root one ulp outside the root's box: the 4-wide records stand
    (the skipped levels still nest), the fused ones are refused, the frame is the oracle's over the same tree"""
    O = oracle_mod
    sc = _oracle_scene("hf24")
    nodes = sc.nodes.copy()
    v = nodes.view(va.BVH_NODE_DTYPE)
    assert v["num_prims"][0] == 0 and v["first"][0] == 1
    v["bbox_max"][1][0] = np.nextafter(v["bbox_max"][0][0], np.float32(np.inf))
    d = upload(ctx, va.index_bvh(sc.prims.view(va.TRIANGLE_DTYPE), v, sc.indices, sc.max_depth), sc.normals, 0)
    assert d.info["wide_records"] > 0 and d.info["fused_records"] == 0 and d.info["fused_bytes"] == 0
    osc = O.Scene("hf24_unnested", O.VO_TRI, sc.prims, nodes, sc.indices, sc.normals, sc.max_depth)
    w, h = 72, 40
    ref = O.render(osc, handout.oracle_camera(handout.camera(w, h), w, h), mode=O.VO_MODE_AO, frame_num=3)
    assert (ref["occ"] != 0).any()
    handout.check(handout.frame(ctx, d, 8, 3), ref)
    d.close()
