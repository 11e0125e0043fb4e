"""GPU: the AO kernel's 4-wide any-hit step keeps its pushes in the LDS part of the stack.

An AO ray that descends the 4-wide records pushes a record's other hit entries without a test against
the LDS capacity: it asks for LDS room first (stack_t::room_lds) and, where that fails, restarts on the
binary records, whose walk keeps the checked push and the overflow block.  Both walks reach the same
leaves, so every frame stays bit-identical to the oracle (the C restatement of ao/main.cpp:183-246) at
every LDS capacity: 1 (the smallest VRH_OPT_STACK_CAP accepts: no record's hits ever fit, every 4-wide
ray restarts), 8 (rays with several pending entries restart) and the default.  hfstack32x24 stacks 24
terrain layers, so an AO ray holds several pending entries; the large radius keeps the root's children
as the entry cut, the small one cuts deep.
"""
import functools

import numpy as np
import pytest

import visionaray_amd as va
from visionaray_amd import scenes

pytestmark = pytest.mark.gpu

SCENES = ["hfstack32x24", "hf64"]
SIZES = [(72, 40), (75, 43)]          # whole 8x8 tiles; partial tiles on both edges
RADII = [0.1, 1.0]
FRAMES = [0, 5]
CAPS = [1, 8, 0]                      # LDS stack entries: the smallest accepted, 8, the default (auto)
FIELDS = ("color", "occ", "prim_id", "t")
MISS = 0xFFFFFFFF


@pytest.fixture(scope="module")
def devs(ctx, oracle_mod):
    out = {}
    for name in SCENES:
        _, prims = oracle_mod.gen_prims(name)          # hfstack is the oracle's (a test-only scene)
        prims = prims.view(va.TRIANGLE_DTYPE).copy()
        assert oracle_mod.scene_spec(name)[2] == scenes.spec("hf64")[2]      # _frames: one camera for both
        out[name] = va.hip_index_bvh(ctx, va.build_index_bvh(prims), va.face_normals(prims))
        assert out[name].info["wide_records"] > 0
        assert out[name].info["max_depth"] > 8          # caps 1 and 8 run the overflow-stack instances
    yield out
    for d in out.values():
        d.close()


@functools.lru_cache(maxsize=None)
def _oracle_scene(O, name):
    return O.make_scene(name)


@functools.lru_cache(maxsize=None)
def _reference(O, name, W, H, radius, frame_num):
    """one oracle frame, computed once and shared (read-only)"""
    ref = O.render(_oracle_scene(O, name), O.scene_camera(name, W, H), mode=O.VO_MODE_AO, samples=8, radius=radius,
                   frame_num=frame_num)
    for k in FIELDS:
        ref[k].setflags(write=False)
    return ref


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, ref, what, lo=0, n=None):
    """bit for bit; lo, n: pixels lo .. lo + n of `got` (one frame of a launch of several)"""
    for k in FIELDS:
        a = _bits(got[k])
        a = a[lo:lo + n] if n else a
        assert np.array_equal(a.reshape(-1), _bits(ref[k]).reshape(-1)), f"{what}: {k}"


def _frames(ctx, dev, name, W, H, radius, frame_num, cap, count=False):
    """the one-frame launch and a launch of 3 frames in flight at the LDS capacity `cap`"""
    cam, _, _ = scenes.scene_camera("hf64", W, H)      # the heightfields' camera (bit-identical to the oracle's)
    ctx.set_option("stack_cap", cap)
    try:
        k = va.ao_kernel(dev, samples=8, radius=radius, count_tests=count)
        rt = va.hip_buffer_rt(ctx, W, H)
        va.hip_sched(ctx).frame(k, va.make_sched_params(cam, rt), frame_num=frame_num)
        one = rt.download()
        stats = ctx.last_frame_stats()
        rt.close()
        if count:
            return one, stats
        rtb = va.hip_buffer_rt(ctx, W, H * 3)
        va.render_batch(ctx, dev, rtb, [cam.basis(W, H)] * 3, k, frame_num=frame_num)
        three = rtb.download()
        rtb.close()
        return one, three
    finally:
        ctx.set_option("stack_cap", 0)


@pytest.mark.parametrize("frame_num", FRAMES)
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", SCENES)
def test_every_stack_size_matches_the_oracle(ctx, oracle_mod, devs, name, size, radius, frame_num):
    O = oracle_mod
    W, H = size
    dev = devs[name]
    refs = [_reference(O, name, W, H, radius, frame_num + f) for f in range(3)]
    assert (refs[0]["prim_id"] != MISS).any() and (refs[0]["occ"] != 0).any()
    first = None
    for cap in CAPS:
        one, three = _frames(ctx, dev, name, W, H, radius, frame_num, cap)
        _same(one, refs[0], f"cap {cap}, one frame")
        for f in range(3):
            _same(three, refs[f], f"cap {cap}, frame {f} of 3 in flight", lo=f * W * H, n=W * H)
        # ... and equal across stack sizes (as each equals the oracle; stated on its own)
        if first is None:
            first = (one, three)
        else:
            _same(one, first[0], f"cap {cap} against cap {CAPS[0]}, one frame")
            _same(three, first[1], f"cap {cap} against cap {CAPS[0]}, 3 frames in flight")


@pytest.mark.parametrize("cap", [1, 8])
def test_a_small_stack_runs_the_restart(ctx, oracle_mod, devs, cap):
    """Restarted rays test boxes again on the binary records, so the counting instance's box_tests at a
    small LDS capacity must differ from the default capacity's on the same frame (hfstack32x24, 75x43,
    radius 1.0, frame 5).  The counting instance holds its whole stack in LDS; it is told the LDS entries of
    the uncounted launch it stands for (launch_plan::quad_lds) and restarts where that launch does.
    Measured: capacity 1 725,880, capacity 8 789,940, default 672,678 box tests.  (Before the 4-wide walk
    kept to the LDS part the three were equal, 672,678: a full LDS part overflowed into the global block,
    and the restart ran only when the whole stack was full.)"""
    name, (W, H), radius, frame_num = "hfstack32x24", SIZES[1], 1.0, 5
    dev = devs[name]
    ref = _reference(oracle_mod, name, W, H, radius, frame_num)
    small, st_small = _frames(ctx, dev, name, W, H, radius, frame_num, cap, count=True)
    auto, st_auto = _frames(ctx, dev, name, W, H, radius, frame_num, 0, count=True)
    _same(small, ref, f"counting instance, cap {cap}")
    _same(auto, ref, "counting instance, default cap")
    print(f"box_tests: cap {cap}: {st_small['box_tests']} (stack {st_small['stack_depth']}), "
          f"default: {st_auto['box_tests']} (stack {st_auto['stack_depth']})")
    assert st_small["box_tests"] > 0 and st_auto["box_tests"] > 0
    assert st_small["box_tests"] != st_auto["box_tests"]


def test_a_non_finite_radius_matches_the_oracle(ctx, oracle_mod, devs):
    """radius inf: tn < radius no longer implies tn < FLT_MAX, so these AO rays keep the full test"""
    name, (W, H), frame_num = "hfstack32x24", SIZES[1], 0
    dev = devs[name]
    ref = _reference(oracle_mod, name, W, H, float("inf"), frame_num)
    assert (ref["prim_id"] != MISS).any() and (ref["occ"] != 0).any()
    for cap in CAPS:
        one, three = _frames(ctx, dev, name, W, H, float("inf"), frame_num, cap)
        _same(one, ref, f"radius inf, cap {cap}, one frame")
        _same(three, ref, f"radius inf, cap {cap}, frame 0 of 3 in flight", lo=0, n=W * H)
