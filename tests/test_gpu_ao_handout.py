"""GPU: the AO kernel's hand-out path (vrh_kernels.hip start_ao / ao_ray: idle lanes take new AO rays --
hit record and normal fetched first, the disk sample searched four candidates at a time, the basis
formed afterwards, then the tile's cut entries) leaves every AO frame bit-identical.

Every comparison is against the oracle's AO masks and colour bits (the C restatement of
ao/main.cpp:183-246).  The scene is hf24 (1,152 triangles) at 72x40 -- 9 x 5 whole tiles -- under a
camera pitched up so that the terrain's far edge crosses the image: some tiles have no hit (no hand-out),
some one (hand-outs of one slot), some all 64; 75x43 adds partial tiles at the right edge and the bottom.
"""
import functools

import numpy as np
import pytest

import deep_cases as D
import visionaray_amd as va
from visionaray_amd import scenes

pytestmark = pytest.mark.gpu

NAME, W, H = "hf24", 72, 40
EYE, CENTER, UP = (0.3, 0.9, 1.4), (0.0, 0.35, 0.0), (0.0, 1.0, 0.0)
MISS = 0xFFFFFFFF


def camera(w, h):
    cam = va.camera()
    cam.perspective(float(np.float32(45.0) * np.float32(va.DEGREES_TO_RADIANS)), float(np.float32(w) / np.float32(h)),
                    0.001, 1000.0)
    cam.look_at(EYE, CENTER, UP)
    return cam


def oracle_camera(cam, w, h):
    b = cam.basis(w, h)
    return tuple(np.array(x[:], np.float32) for x in (b.eye, b.cam_u, b.cam_v, b.cam_w)) + (w, h)


@functools.lru_cache(maxsize=None)
def reference(samples=8, frame=0, w=W, h=H):
    """the oracle's frame (computed once per process, read-only)"""
    from oracle import oracle as O
    O.build()
    ref = O.render(_oracle_scene(), oracle_camera(camera(w, h), w, h), mode=O.VO_MODE_AO, samples=samples, frame_num=frame)
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def _oracle_scene():
    from oracle import oracle as O
    O.build()
    return O.make_scene(NAME)


@pytest.fixture(scope="module")
def dev(ctx):
    prims = scenes.primitives(NAME)
    d = va.hip_index_bvh(ctx, va.build_index_bvh(prims), scenes.normals_for(prims))
    assert d.info["wide_records"] > 0          # AO rays walk the 4-wide records and start at a cut
    return d


def check(got, ref, samples=8, rows=None):
    """prim ids, t bits, colour bits and -- where a byte holds them -- the occlusion masks"""
    n0, n1 = rows if rows else (0, len(ref["prim_id"]))
    assert np.array_equal(got["prim_id"][n0:n1], ref["prim_id"])
    assert np.array_equal(got["t"][n0:n1].view(np.uint32), ref["t"].view(np.uint32))
    assert np.array_equal(got["color"][n0:n1].view(np.uint32), ref["color"].view(np.uint32))
    if samples <= 8:
        assert np.array_equal(got["occ"][n0:n1], ref["occ"])


def frame(ctx, d, samples=8, frame_num=0, w=W, h=H):
    rt = va.hip_buffer_rt(ctx, w, h)
    va.hip_sched(ctx).frame(va.ao_kernel(d, samples=samples), va.make_sched_params(camera(w, h), rt), frame_num=frame_num)
    out = rt.download()
    rt.close()
    return out


def test_view_has_empty_single_hit_and_full_tiles():
    hit = (reference()["prim_id"] != MISS).reshape(H, W)
    counts = {int(hit[y:y + 8, x:x + 8].sum()) for y in range(0, H, 8) for x in range(0, W, 8)}
    assert {0, 1, 64} <= counts
    occ = reference()["occ"][hit.ravel()]
    assert (occ != 0).any() and (occ == 0).any()          # occluded and open samples both occur


@pytest.mark.parametrize("frame_num", [0, 3, 2 ** 32 - 1])
@pytest.mark.parametrize("samples", [1, 5, 8, 32])
def test_samples_and_frame_numbers(ctx, dev, samples, frame_num):
    check(frame(ctx, dev, samples, frame_num), reference(samples, frame_num), samples)


def test_partial_tiles(ctx, dev):
    w, h = 75, 43
    check(frame(ctx, dev, 8, 3, w, h), reference(8, 3, w, h))


def test_three_frames_in_flight(ctx, dev):
    basis = camera(W, H).basis(W, H)
    rt = va.hip_buffer_rt(ctx, W, 3 * H)
    va.render_batch(ctx, dev, rt, [basis] * 3, va.ao_kernel(dev), None, frame_num=2)
    got = rt.download()
    rt.close()
    for f in range(3):
        check(got, reference(8, 2 + f), rows=(f * W * H, (f + 1) * W * H))


@pytest.mark.parametrize("cut", [1, 2])            # VRH_OPT_AO_CUT: on, off
@pytest.mark.parametrize("refill", [1, 64])        # hand-outs of single lanes, of whole waves
def test_refill_threshold_and_cut(ctx, dev, refill, cut):
    ctx.set_option("refill_min", refill)
    ctx.set_option("ao_cut", cut)
    try:
        check(frame(ctx, dev, 8, 3), reference(8, 3))
        check(frame(ctx, dev, 5, 0), reference(5, 0), 5)
    finally:
        ctx.set_option("refill_min", 0)
        ctx.set_option("ao_cut", 0)


def test_share_instance(ctx, dev):
    """one frame with tail sharing: idle waves start a sibling's AO rays from its records and cut"""
    ctx.set_option("ao_share", 1)
    try:
        check(frame(ctx, dev, 8, 3), reference(8, 3))
        assert ctx.last_frame_stats()["block_threads"] == 256
    finally:
        ctx.set_option("ao_share", 0)


def test_two_bvh_list(ctx):
    """the BVH-list instance: the terrain's triangles split over two BVHs by prim id"""
    from oracle import oracle as O
    O.build()
    sc = _oracle_scene()
    members, osc = [], []
    for k in (0, 1):
        p = sc.prims[sc.prims["prim_id"] % 2 == k]
        nodes, idx, depth = O.build_bvh(p, O.VO_TRI)
        osc.append(O.Scene(NAME, O.VO_TRI, p, nodes, idx, sc.normals if k == 0 else None, depth))
        members.append(va.hip_index_bvh(ctx, va.index_bvh(p.view(va.TRIANGLE_DTYPE), nodes.view(va.BVH_NODE_DTYPE), idx, depth)))
    lst = va.hip_index_bvh.scene_list(ctx, members, sc.normals)
    for m in members:
        m.close()
    assert lst.info["num_bvhs"] == 2
    ref = O.render(osc, oracle_camera(camera(W, H), W, H), mode=O.VO_MODE_AO, frame_num=3)
    assert (ref["occ"] != 0).any()
    check(frame(ctx, lst, 8, 3), ref)
    lst.close()


def test_depth_30_comb_runs_the_overflow_stack_instance(ctx):
    """a BVH deeper than 20 keeps 20 stack entries in LDS and the rest in the overflow block
    (tests/deep_cases.py comb31, its oblique camera, 160x90)"""
    c = D.case("comb31")
    assert c.depth == 30
    d = va.hip_index_bvh(ctx, va.index_bvh(c.prims, c.nodes, c.indices, c.depth), c.normals)
    assert d.info["max_depth"] == 30
    eye, center, up = c.cameras["oblique"]
    cam = va.camera()
    cam.perspective(float(np.float32(45.0) * np.float32(va.DEGREES_TO_RADIANS)), float(np.float32(D.W) / np.float32(D.H)),
                    0.001, 1000.0)
    cam.look_at(eye, center, up)
    rt = va.hip_buffer_rt(ctx, D.W, D.H)
    va.hip_sched(ctx).frame(va.ao_kernel(d), va.make_sched_params(cam, rt))
    assert ctx.last_frame_stats()["stack_depth"] >= 30
    ref = D.reference("comb31", "oblique")
    assert (ref["occ"] != 0).any()
    check(rt.download(), ref)
    rt.close()
    d.close()


def test_counting_instance_reports_the_hand_out(ctx, dev):
    """VRH_KERNEL_COUNT_TESTS: the same frame, plus where the waves' time went and the hand-outs' shape"""
    rt = va.hip_buffer_rt(ctx, W, H)
    va.hip_sched(ctx).frame(va.ao_kernel(dev, count_tests=True), va.make_sched_params(camera(W, H), rt), frame_num=3)
    check(rt.download(), reference(8, 3))
    rt.close()
    st = ctx.last_handout_stats()
    ao_rays = 8 * int((reference(8, 3)["prim_id"] != MISS).sum())
    assert st["ao_handout_rays"] == ao_rays
    assert 0 < st["ao_handout_events"] <= st["ao_handout_slot_runs"] <= ao_rays
    assert st["ao_handout_slot_runs"] >= ao_rays // 8                  # a run holds at most a slot's 8 rays
    assert 0 < st["ao_handout_ticks"] < st["loop_ticks"] and 0 < st["step_ticks"] < st["loop_ticks"]
    assert st["ao_handout_ticks"] + st["primary_handout_ticks"] + st["step_ticks"] <= st["loop_ticks"]
