"""GPU: the built-in pathtracing::kernel (VRH_KERNEL_PATHTRACING) against the reference's own frames.

tests/golden/pt_*.npz hold frames of the reference's pathtracing::kernel (tests/golden/pathtrace_ref.cpp,
run by make_pathtrace_golden.py) with random_sampler<float> seeded per pixel as hip_sched seeds it.
With ks = 0 (`diffuse`) no powf is reached and the GPU frame is bit-identical; with the plastics of
whitted_spec the colour is within the fixture's rtol_spec (derived from the reference alone: twice the
response of a frame to powf moving by one float) on at least 99 % of the hit pixels.
EPI 4 has no overflow-stack instance (like the whitted kernel): the deep-BVH case (depth 89 with the whole
stack in LDS, depth 999 refused on the host) and the randomized sweep against the oracle's path-tracing mode
are in tests/test_gpu_fuzz_pathtracing.py.
"""
import functools
import json
import os
import sys

import numpy as np
import pytest

import visionaray_amd as va
from visionaray_amd import _capi, scenes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_multi_hit import camera_of, product_scene  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MISS = 0xFFFFFFFF
with open(os.path.join(HERE, "golden", "pathtrace.json")) as _f:
    PT = json.load(_f)
DIFFUSE = [(c, f) for c in ("pt_cornell12_diffuse", "pt_hfstack_diffuse", "pt_hf64_vertex_diffuse") for f in PT[c]["frames"]]
PLASTIC = ["pt_cornell12_plastic2", "pt_cornell12_plastic"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def primary_of(name, W, H):
    """the oracle's closest hit of the shading scene (computed once per scene and size)"""
    from oracle import oracle as O
    ref = O.render(O.make_shade_scene(name), O.scene_camera(name, W, H), mode=O.VO_MODE_PRIMARY)
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref


def setup(ctx, O, g):
    """device scene, path-tracing kernel and camera of a fixture record"""
    dev = product_scene(ctx, O, g["scene"])
    m, lt, _, bg = O.whitted_spec()
    m = m.copy()
    if g["materials"] == "diffuse":
        m["ks"] = 0.0
    sh = va.shading(ctx, m.view(va.PLASTIC_DTYPE), lt.view(va.POINT_LIGHT_DTYPE))
    binding = va.normals_per_vertex_binding if g["binding"] == "vertex" else va.normals_per_face_binding
    k = va.pathtracing_kernel(dev, sh, binding=binding, bg=bg, ambient=g["ambient"], num_bounces=g["bounces"],
                              epsilon=g["eps"])
    return dev, k, camera_of(O, g["scene"], g["W"], g["H"])


def frame(ctx, dev, k, cam, W, H, frame_num=0, shard=None, rt=None):
    rt = rt or va.hip_buffer_rt(ctx, W, H)
    va.render(ctx, dev, rt, cam, k, shard=shard, frame_num=frame_num)
    return rt.download()


def check_primary(out, g):
    ref = primary_of(g["scene"], g["W"], g["H"])
    assert np.array_equal(out["prim_id"], ref["prim_id"])
    assert np.array_equal(bits(out["t"]), bits(ref["t"]))
    return out["prim_id"] != MISS


@pytest.mark.parametrize("case,fr", DIFFUSE)
def test_diffuse_frames_are_bit_identical(ctx, oracle_mod, case, fr):
    g = PT[case]
    dev, k, cam = setup(ctx, oracle_mod, g)
    out = frame(ctx, dev, k, cam, g["W"], g["H"], frame_num=fr)
    st = ctx.last_frame_stats()
    ref = np.load(os.path.join(HERE, "golden", case + ".npz"))["color_f%d" % fr]
    hit = check_primary(out, g)
    differ = np.any(bits(out["color"]) != bits(ref), axis=1)
    assert not differ.any(), f"{int(differ.sum())} of {differ.size} pixels differ from the reference frame"
    assert st["rays"] == g["rays"][str(fr)]
    assert st["hits"] == int(hit.sum()) and hit.any()


def test_jittered_blend_accumulation_is_bit_identical(ctx, oracle_mod):
    g = PT["pt_cornell12_blend"]
    dev, k, cam = setup(ctx, oracle_mod, g)
    ref = np.load(os.path.join(HERE, "golden", "pt_cornell12_blend.npz"))
    rt = va.hip_buffer_rt(ctx, g["W"], g["H"])
    rt.clear_color_buffer((0.0, 0.0, 0.0, 0.0))
    first = g["first_frame"]
    for n in range(first, first + g["num_frames"]):
        va.render_sampled(ctx, dev, rt, cam, k, va.pixel_sampler.jittered_blend_type, frame_num=n)
        if n == first:
            assert np.array_equal(bits(rt.download()["color"]), bits(ref["color_first"]))
    assert np.array_equal(bits(rt.download()["color"]), bits(ref["color_last"]))


@pytest.mark.parametrize("case", PLASTIC)
def test_plastic_frames_within_derived_tolerance(ctx, oracle_mod, case):
    g = PT[case]
    dev, k, cam = setup(ctx, oracle_mod, g)
    out = frame(ctx, dev, k, cam, g["W"], g["H"], frame_num=g["frames"][0])
    ref = np.load(os.path.join(HERE, "golden", case + ".npz"))["color_f%d" % g["frames"][0]]
    hit = check_primary(out, g)
    assert np.array_equal(bits(out["color"][~hit]), bits(ref[~hit]))
    got, want = out["color"][hit].astype(np.float64), ref[hit].astype(np.float64)
    rel = np.abs(got - want) / np.where(want == 0.0, 1.0, np.abs(want))
    rel[(want == 0.0) & (got != 0.0)] = np.inf          # a zero channel must stay exactly zero
    ok = np.all(rel <= g["rtol_spec"], axis=1)
    nz = rel[np.isfinite(rel)]
    print(f"{case}: {ok.mean():.5f} of {ok.size} hit pixels within rtol_spec {g['rtol_spec']:.3e}; "
          f"max rel {nz.max():.3e}, bit-identical {np.mean(np.all(bits(out['color'][hit]) == bits(ref[hit]), axis=1)):.4f}")
    assert ok.mean() >= 0.99, f"only {ok.mean():.4f} of the hit pixels are within rtol_spec {g['rtol_spec']:.3e}"


def test_zero_bounces_is_background(ctx, oracle_mod):
    g = dict(PT["pt_cornell12_diffuse"], bounces=0)
    dev, k, cam = setup(ctx, oracle_mod, g)
    out = frame(ctx, dev, k, cam, g["W"], g["H"])
    hit = check_primary(out, g)
    assert hit.any() and (~hit).any()
    assert np.array_equal(out["color"], np.tile(np.float32(g["bg"]), (g["W"] * g["H"], 1)))


def test_one_bounce_is_black_on_hits(ctx, oracle_mod):
    g = dict(PT["pt_cornell12_diffuse"], bounces=1)
    dev, k, cam = setup(ctx, oracle_mod, g)
    out = frame(ctx, dev, k, cam, g["W"], g["H"])
    hit = check_primary(out, g)
    assert np.array_equal(out["color"][hit], np.tile(np.float32([0, 0, 0, 1]), (int(hit.sum()), 1)))
    assert np.array_equal(out["color"][~hit], np.tile(np.float32(g["bg"]), (int((~hit).sum()), 1)))


def test_frame_number_selects_the_random_numbers(ctx, oracle_mod):
    g = PT["pt_cornell12_diffuse"]
    dev, k, cam = setup(ctx, oracle_mod, g)
    a = frame(ctx, dev, k, cam, g["W"], g["H"], frame_num=0)
    b = frame(ctx, dev, k, cam, g["W"], g["H"], frame_num=0)
    c = frame(ctx, dev, k, cam, g["W"], g["H"], frame_num=1)
    assert np.array_equal(bits(a["color"]), bits(b["color"]))
    hit = a["prim_id"] != MISS
    assert np.any(bits(a["color"][hit]) != bits(c["color"][hit]))
    assert np.array_equal(a["prim_id"], c["prim_id"])


@pytest.mark.parametrize("occ", [0, 1])
def test_frames_in_flight_equal_single_frames(ctx, oracle_mod, occ):
    g = PT["pt_hfstack_diffuse"]
    W, H = g["W"], g["H"]
    dev, k, cam = setup(ctx, oracle_mod, g)
    ctx.set_option("waves_per_simd", occ)
    try:
        singles = [frame(ctx, dev, k, cam, W, H, frame_num=5 + f) for f in range(3)]
        three = va.hip_buffer_rt(ctx, W, 3 * H)
        va.render_batch(ctx, dev, three, [cam] * 3, k, frame_num=5)
        got = three.download()
    finally:
        ctx.set_option("waves_per_simd", 0)
    n = W * H
    assert np.any(bits(singles[0]["color"]) != bits(singles[1]["color"]))
    for f in range(3):
        for key in ("prim_id", "t", "color"):
            assert np.array_equal(bits(got[key][f * n:(f + 1) * n]), bits(singles[f][key])), (f, key)


def test_shard_and_scissor_draw_the_whole_image_numbers(ctx, oracle_mod):
    g = PT["pt_hf64_vertex_diffuse"]          # 60 x 44: partial tiles on both edges
    W, H = g["W"], g["H"]
    dev, k, cam = setup(ctx, oracle_mod, g)
    whole = frame(ctx, dev, k, cam, W, H, frame_num=3)
    fill = np.float32([0.25, 0.5, 0.75, 0.125])

    def prefilled():
        rt = va.hip_buffer_rt(ctx, W, H)
        rt.clear_color_buffer(tuple(float(x) for x in fill))     # side buffers: miss
        return rt

    rows = np.arange(W * H) // W
    cols = np.arange(W * H) % W
    # shard 1 of 3, unpacked: the bands (8 rows) b with b % 3 == 1
    part = frame(ctx, dev, k, cam, W, H, frame_num=3, shard=_capi.vrh_shard(1, 3, 0, 0), rt=prefilled())
    mine = (rows // _capi.VRH_BAND_ROWS) % 3 == 1
    # a scissor box that cuts through 8x8 tiles
    box = (5, 3, 43, 30)
    cam2 = camera_of(oracle_mod, g["scene"], W, H)
    cam2.scissor[:] = list(box)
    cut = frame(ctx, dev, k, cam2, W, H, frame_num=3, rt=prefilled())
    inside = (cols >= box[0]) & (cols < box[2]) & (rows >= box[1]) & (rows < box[3])
    for got, sel in ((part, mine), (cut, inside)):
        assert sel.any() and (~sel).any()
        for key in ("prim_id", "t", "color"):
            assert np.array_equal(bits(got[key][sel]), bits(whole[key][sel])), key
        assert np.array_equal(got["color"][~sel], np.tile(fill, (int((~sel).sum()), 1)))
        assert np.all(got["prim_id"][~sel] == MISS)


def _refused(code, fn, *args, **kw):
    with pytest.raises(va.VrhError) as e:
        fn(*args, **kw)
    assert e.value.code == code, str(e.value)
    assert _capi.lib().vrh_last_error().decode() != ""


def test_refusals(ctx, oracle_mod):
    O = oracle_mod
    g = PT["pt_cornell12_diffuse"]
    W, H = g["W"], g["H"]
    dev, k, cam = setup(ctx, O, g)
    rt = va.hip_buffer_rt(ctx, W, H)
    UNS, INV = _capi.VRH_ERR_UNSUPPORTED, _capi.VRH_ERR_INVALID
    _refused(UNS, va.render_sampled, ctx, dev, rt, cam, k, va.pixel_sampler.ssaa4_type)
    _refused(UNS, va.render_view, ctx, dev, rt, va.view_camera(np.eye(4), np.eye(4), W, H), k)
    _refused(UNS, va.render_view, ctx, dev, rt, va.view_camera(np.eye(4), np.eye(4), W, H), k,
             va.pixel_sampler.jittered_type)
    # spheres
    sph = va.make_spheres([[0, 0, 0]], [1.0])
    sdev = va.hip_index_bvh(ctx, va.build_index_bvh(sph))
    ks = va.pathtracing_kernel(sdev, k.shade)
    _refused(UNS, va.render, ctx, sdev, rt, cam, ks)
    # scene lists
    lst = va.hip_index_bvh.scene_list(ctx, [dev, dev], va.face_normals(O.gen_prims(g["scene"])[1].view(va.TRIANGLE_DTYPE)))
    _refused(UNS, va.render, ctx, lst, rt, cam, va.pathtracing_kernel(lst, k.shade))
    # test counting with a sampler
    kc = va.pathtracing_kernel(dev, k.shade, count_tests=True)
    _refused(UNS, va.render_sampled, ctx, dev, rt, cam, kc, va.pixel_sampler.jittered_type, frame_num=1)
    # a hit mask
    m = va.hit_mask(ctx, np.zeros((3 * 12, 2), np.float32), np.ones((2, 2), np.uint8))
    km = va.with_hit_mask(va.pathtracing_kernel(dev, k.shade), m)
    _refused(UNS, va.render, ctx, dev, rt, cam, km)
    # no shading
    kn = va.pathtracing_kernel(dev, k.shade)
    kn.desc.shading = None
    _refused(INV, va.render, ctx, dev, rt, cam, kn)
    # render groups
    (grp,) = va.render_group.local([ctx])
    try:
        _refused(UNS, va.render_sharded, [grp], [dev], [k], rt, [cam])
    finally:
        grp.close()
    # nothing above rendered: the target still runs a frame
    assert (frame(ctx, dev, k, cam, W, H, rt=rt)["prim_id"] != MISS).any()


def test_hip_sched_frame_accumulates_like_render_sampled(ctx, oracle_mod):
    """hip_sched.frame(pathtracing_kernel, sched_params(jittered_blend ...)): the bits of the blend fixture"""
    g = PT["pt_cornell12_blend"]
    W, H = g["W"], g["H"]
    dev, k, _ = setup(ctx, oracle_mod, g)
    cam, _, _ = scenes.scene_camera(g["scene"], W, H)
    rt = va.hip_buffer_rt(ctx, W, H)
    rt.clear_color_buffer((0.0, 0.0, 0.0, 0.0))
    sched = va.hip_sched(ctx)
    try:
        sp = va.make_sched_params(va.pixel_sampler.jittered_blend_type, cam, rt)
        for n in range(g["first_frame"], g["first_frame"] + g["num_frames"]):
            sched.frame(k, sp, frame_num=n)
        got = rt.download()["color"]
    finally:
        ctx.set_option("async_frames", 0)
    ref = np.load(os.path.join(HERE, "golden", "pt_cornell12_blend.npz"))["color_last"]
    assert np.array_equal(bits(got), bits(ref))


def test_counting_variant_renders_the_same_frame(ctx, oracle_mod):
    """VRH_KERNEL_COUNT_TESTS (one-frame launches): the same bits, with box / primitive tests counted"""
    g = PT["pt_hf64_vertex_diffuse"]
    dev, k, cam = setup(ctx, oracle_mod, g)
    plain = frame(ctx, dev, k, cam, g["W"], g["H"], frame_num=1)
    kc = va.pathtracing_kernel(dev, k.shade, binding=va.normals_per_vertex_binding, bg=tuple(g["bg"]),
                               ambient=g["ambient"], num_bounces=g["bounces"], epsilon=g["eps"], count_tests=True)
    counted = frame(ctx, dev, kc, cam, g["W"], g["H"], frame_num=1)
    st = ctx.last_frame_stats()
    for key in ("prim_id", "t", "color"):
        assert np.array_equal(bits(counted[key]), bits(plain[key])), key
    assert st["rays"] == g["rays"]["1"]
    assert st["box_tests"] > 0 and st["prim_tests"] > 0


def test_cpp_example_accumulates_like_the_python_layer(ctx, tmp_path):
    """examples/pathtrace_hip.cpp (make_hip_pathtracing_kernel + jittered_blend_type through hip_backend.h):
    its PFM image holds the bits of the same frames issued through the Python layer"""
    import subprocess
    exe = os.path.join(os.path.dirname(HERE), "build", "examples", "pathtrace_hip")
    W, H, frames, bounces = 96, 64, 3, 4
    out = tmp_path / "pt.pfm"
    r = subprocess.run([exe, "64", str(W), str(H), str(frames), str(bounces), str(out)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    raw = out.read_bytes()
    head = b"PF\n%d %d\n-1.0\n" % (W, H)
    assert raw.startswith(head)
    img = np.frombuffer(raw, np.float32, W * H * 3, len(head)).reshape(W * H, 3)

    prims = scenes.primitives("hf64")
    prims["geom_id"] = np.arange(len(prims), dtype=np.uint32) % 3
    dev = va.hip_index_bvh(ctx, va.build_index_bvh(prims), va.face_normals(prims))
    m = np.zeros(3, va.PLASTIC_DTYPE)
    m[0] = ((0.0, 0.0, 0.0), 1.0, (0.8, 0.3, 0.2), 1.0, (1.0, 1.0, 1.0), 0.4, 32.0)
    m[1] = ((0.0, 0.0, 0.0), 1.0, (0.2, 0.7, 0.3), 0.9, (0.9, 0.9, 0.9), 0.2, 8.0)
    m[2] = ((0.0, 0.0, 0.0), 1.0, (0.3, 0.3, 0.9), 0.7, (1.0, 0.8, 0.6), 0.6, 64.5)
    lt = np.zeros(1, va.POINT_LIGHT_DTYPE)
    lt[0] = ((0.0, 2.0, 0.0), (1.0, 1.0, 1.0), 1.0, 1.0, 0.0, 0.0)
    sh = va.shading(ctx, m, lt)
    k = va.pathtracing_kernel(dev, sh, bg=(0.1, 0.2, 0.3, 1.0), ambient=(1.0, 1.0, 1.0, 1.0), num_bounces=bounces)
    cam, _, _ = scenes.scene_camera("hf64", W, H)
    rt = va.hip_buffer_rt(ctx, W, H)
    rt.clear_color_buffer((0.0, 0.0, 0.0, 0.0))
    rays = 0
    for n in range(1, frames + 1):
        va.render_sampled(ctx, dev, rt, cam.basis(W, H), k, va.pixel_sampler.jittered_blend_type, frame_num=n)
        rays += ctx.last_frame_stats()["rays"]
    got = rt.download()["color"]
    assert info["rays"] == rays
    assert np.array_equal(bits(img), bits(got[:, :3]))
    assert (got[:, 3] == 1.0).any()
