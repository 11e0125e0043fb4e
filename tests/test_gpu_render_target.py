"""GPU: formatted render targets (vrh_rt_alloc_formatted: RGBA8 / RGB8 / RGB32F / RGBA32F colour, DEPTH32F /
DEPTH24_STENCIL8 depth) and their resolve kernel (visionaray_amd/csrc/vrh_resolve.hip), bit for bit.

The resolve alone is held to the reference's own buffers (tests/golden/rt_pixels.npz, rt_frame.npz); frames are
held to the same frame in a plain target (the staging buffers) and to vrh_rt_resolve_host of it -- the host build
of the kernel's text, which tests/test_render_target_fixtures.py holds to the reference on the CPU.
"""
import os
import sys

import numpy as np
import pytest

import visionaray_amd as va
from visionaray_amd import _capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mv_cases as MC  # noqa: E402
import rt_cases as RC  # noqa: E402
import vol_cases as VC  # noqa: E402

pytestmark = pytest.mark.gpu
W, H = 61, 45
PS = va.pixel_sampler
ALL_FORMATS = [(c, d) for c in RC.COLOR_FORMATS for d in RC.DEPTH_FORMATS]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_formatted(got, want):
    assert sorted(got) == sorted(want)
    for k in got:
        a, b = got[k], want[k]
        if a.dtype == np.float32:
            a, b = bits(a), bits(b)
        bad = np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))
        assert bad.size == 0, f"{k}: {bad.size} pixels differ, first {bad[0]}: {got[k][bad[0]]} != {want[k][bad[0]]}"


def same_staging(fmt_rt, plain_rt):
    a, b = fmt_rt.download(occ=False), plain_rt.download(occ=False)
    assert np.array_equal(a["prim_id"], b["prim_id"])
    assert np.array_equal(bits(a["t"]), bits(b["t"])) and np.array_equal(bits(a["color"]), bits(b["color"]))
    return a


def resolve_host(rt, staging, desc, before=None):
    before = before or {}
    return va.rt_resolve_host(rt.color_format, rt.depth_format, rt.w, rt.h, staging["color"], desc, prim_id=staging["prim_id"],
                              t=staging["t"], color_out=before.get("color"), depth_out=before.get("depth"))


# ---- the resolve alone ---------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(1, 1), (3, 1), (61, 45), (64, 8)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cf_name,df_name", ALL_FORMATS)
def test_resolve_steps_match_reference(ctx, cf_name, df_name, size):
    """the reference's pixel pipeline step by step: clear, store, blend frames 1-4, store"""
    w, h = size
    n = w * h
    rt = va.hip_buffer_rt(ctx, w, h, color_format=RC.COLOR_FORMATS[cf_name], depth_format=RC.DEPTH_FORMATS[df_name], formatted=True)
    fx = RC.pixels_fixture()
    rt.clear_color_buffer(tuple(float(x) for x in fx["clear_color"]))
    if df_name != "none":
        rt.clear_depth_buffer(float(fx["clear_depth"][0]))
    assert RC.same(rt.download_formatted(), RC.expected(0, cf_name, df_name, n), cf_name, df_name), "clear"
    assert np.array_equal(bits(rt.color()), bits(np.tile(fx["clear_color"], (n, 1)))), "the staging colour is cleared too"
    for step in range(len(fx["steps"])):
        color, prim_id, t = RC.step_inputs(step, n)
        rt.upload(color=color, prim_id=prim_id, t=t)
        rt.resolve(RC.step_desc(step, depth=df_name != "none"))
        assert RC.same(rt.download_formatted(), RC.expected(step + 1, cf_name, df_name, n), cf_name, df_name), f"step {step}"
    rt.close()


BOXES = [(1, 1, 4, 3), (3, 2, 60, 44), (5, 0, 6, 45), (0, 7, 61, 8), (7, 7, 7, 7), (9, 3, 2, 40), (58, 40, 99, 99), (2, 0, 63, 45)]


@pytest.mark.parametrize("cf_name,df_name", [("rgba8", "depth24s8"), ("rgb8", "depth32f"), ("rgb32f", "none"), ("rgba32f", "depth32f"),
                                             ("rgba8", "none")])
def test_resolve_scissor_boxes(ctx, cf_name, df_name):
    """odd left / right edges, a single column, a single row, empty boxes, a box clipped by the image: store and
    blend write the box exactly as the host twin does and leave every other pixel as it was"""
    n = W * H
    rt = va.hip_buffer_rt(ctx, W, H, color_format=RC.COLOR_FORMATS[cf_name], depth_format=RC.DEPTH_FORMATS[df_name])
    rng = np.random.default_rng(11)
    for k, box in enumerate(BOXES):
        color, prim_id, t = RC.step_inputs(k % 6, n)
        before = rt.download_formatted()
        if k == 0:      # arbitrary earlier contents
            c = before["color"]
            before["color"] = rng.integers(0, 256, c.shape).astype(np.uint8) if c.dtype == np.uint8 else rng.uniform(0, 1, c.shape).astype(np.float32)
            if df_name != "none":
                before["depth"] = RC.expected(3, "rgba8", df_name, n)["depth"].view(before["depth"].dtype)
            rt.upload_formatted(**before)
        desc = va.resolve_desc(blend=k % 2 == 1, s=0.25, d=0.75, scissor=box,
                               **(dict(view=RC.IDENTITY, proj=RC.IDENTITY) if df_name != "none" else {}))
        rt.upload(color=color, prim_id=prim_id, t=t)
        rt.resolve(desc)
        want = resolve_host(rt, {"color": color, "prim_id": prim_id, "t": t}, desc, before)
        same_formatted(rt.download_formatted(), want)
        x0, y0, x1, y1 = box[0], box[1], min(box[2], W), min(box[3], H)
        outside = np.ones((H, W), bool)
        outside[y0:y1, x0:x1] = False
        outside = outside.reshape(-1)
        for key in want:
            assert np.array_equal(want[key][outside], before[key][outside]), "the twin leaves the outside untouched"
    rt.close()


# ---- frames ------------------------------------------------------------------------------------------------

def look_at(eye, center, up=(0.0, 1.0, 0.0)):
    eye, center, up = (np.asarray(v, np.float64) for v in (eye, center, up))
    f = (center - eye) / np.linalg.norm(center - eye)
    s = np.cross(f, up) / np.linalg.norm(np.cross(f, up))
    u = np.cross(s, f)
    m = np.eye(4)
    m[0, :3], m[1, :3], m[2, :3] = s, u, -f
    m[:3, 3] = -m[:3, :3] @ eye
    return m.astype(np.float32)


def perspective(fovy, aspect, zn, zf):
    f = 1.0 / np.tan(fovy / 2.0)
    m = np.zeros((4, 4))
    m[0, 0], m[1, 1], m[2, 2], m[2, 3], m[3, 2] = f / aspect, f, (zf + zn) / (zn - zf), 2.0 * zf * zn / (zn - zf), -1.0
    return m.astype(np.float32)


class Scene:
    pass


@pytest.fixture(scope="module")
def scene(ctx, oracle_mod):
    """a few hundred random triangles (tests/test_gpu_fuzz.py's kind of scene), a pinhole and a matrix camera, and
    a shading for the shading kernels"""
    O = oracle_mod
    s = Scene()
    rng = np.random.default_rng(4242)
    n = 400
    c = rng.uniform(-1.0, 1.0, (n, 3))
    size = 10.0 ** rng.uniform(-1.5, -0.5, (n, 1))
    e1, e2 = rng.standard_normal((n, 3)) * size, rng.standard_normal((n, 3)) * size
    prims = va.make_triangles(c - 0.5 * (e1 + e2), e1, e2)
    prims["geom_id"] = np.arange(n, dtype=np.uint32) % 3
    fn = va.face_normals(prims)
    bvh = va.build_index_bvh(prims)
    s.dev = va.hip_index_bvh(ctx, bvh, fn)
    s.oracle_scene = O.Scene("rt_scene", O.VO_TRI, prims, bvh.nodes, bvh.indices, fn, bvh.max_depth)
    s.dev.set_vertex_normals(O.vertex_normals(fn))
    cam = va.camera()
    cam.perspective(0.9, np.float32(W) / np.float32(H), 0.001, 1000.0)
    cam.look_at((2.0, 1.2, 2.4), (0.0, 0.0, 0.0))
    s.basis = cam.basis(W, H)
    s.view, s.proj = look_at((2.0, 1.2, 2.4), (0.0, 0.0, 0.0)), perspective(0.9, W / H, 0.2, 20.0)
    s.vcam = va.view_camera(s.view, s.proj, W, H)
    m, lt, amb, bg = O.shade_spec()
    s.shade = va.shading(ctx, m.view(va.PLASTIC_DTYPE), lt.view(va.POINT_LIGHT_DTYPE))
    s.amb, s.bg = amb, bg
    yield s
    s.shade.close()
    s.dev.close()


def kernel_of(s, name):
    if name == "primary":
        return va.closest_hit_kernel(s.dev)
    if name == "ao":
        return va.ao_kernel(s.dev, samples=4, radius=0.3)
    if name == "simple":
        return va.simple_kernel(s.dev, s.shade, bg=s.bg, ambient=s.amb)
    if name == "whitted":
        return va.whitted_kernel(s.dev, s.shade, bg=s.bg, ambient=s.amb, num_bounces=3, epsilon=1e-3)
    if name == "multi_hit":
        return va.multi_hit_kernel(s.dev, s.shade, max_hits=4)
    assert name == "pathtracing"
    return va.pathtracing_kernel(s.dev, s.shade, bg=s.bg, ambient=s.amb, num_bounces=3, epsilon=1e-3)


def pair(ctx, cf, df, multi_hit=False):
    rts = va.hip_buffer_rt(ctx, W, H, color_format=cf, depth_format=df), va.hip_buffer_rt(ctx, W, H)
    for rt in rts:
        if multi_hit:
            rt.alloc_multi_hit(4)
    return rts


@pytest.mark.parametrize("kernel", ["primary", "ao", "simple", "whitted", "multi_hit", "pathtracing"])
@pytest.mark.parametrize("cf_name", ["rgba8", "rgb8", "rgb32f"])
def test_vrh_render_into_a_formatted_target(ctx, scene, kernel, cf_name):
    frt, prt = pair(ctx, RC.COLOR_FORMATS[cf_name], RC.DF.none, kernel == "multi_hit")
    k = kernel_of(scene, kernel)
    for rt in (frt, prt):
        va.render(ctx, scene.dev, rt, scene.basis, k, frame_num=3)
    staging = same_staging(frt, prt)
    assert (staging["prim_id"] != RC.MISS).any() and (staging["prim_id"] == RC.MISS).any()
    same_formatted(frt.download_formatted(), resolve_host(frt, staging, va.resolve_desc()))
    frt.close(), prt.close()


def test_vrh_render_scissor_box(ctx, scene):
    """the resolve covers the frame's scissor box only"""
    frt = va.hip_buffer_rt(ctx, W, H, color_format=RC.CF.rgba8)
    cam = type(scene.basis).from_buffer_copy(scene.basis)
    cam.scissor[:] = [5, 3, 50, 41]
    before = {"color": np.full((W * H, 4), 0x5A, np.uint8)}
    frt.upload_formatted(**before)
    va.render(ctx, scene.dev, frt, cam, kernel_of(scene, "ao"))
    got, staging = frt.download_formatted(), frt.download()
    want = resolve_host(frt, staging, va.resolve_desc(scissor=(5, 3, 50, 41)), before)
    same_formatted(got, want)
    assert (got["color"].reshape(H, W, 4)[:3] == 0x5A).all() and (got["color"].reshape(H, W, 4)[:, 50:] == 0x5A).all()
    frt.close()


@pytest.mark.parametrize("kernel", ["ao", "pathtracing"])
def test_render_sampled_jittered(ctx, scene, kernel):
    frt, prt = pair(ctx, RC.CF.rgba8, RC.DF.none)
    for rt in (frt, prt):
        va.render_sampled(ctx, scene.dev, rt, scene.basis, kernel_of(scene, kernel), PS.jittered_type, frame_num=5)
    staging = same_staging(frt, prt)
    same_formatted(frt.download_formatted(), resolve_host(frt, staging, va.resolve_desc()))
    frt.close(), prt.close()


@pytest.mark.parametrize("cf_name", ["rgba8", "rgb8", "rgb32f"])
def test_render_sampled_jittered_blend_accumulates_in_the_formatted_buffer(ctx, scene, cf_name):
    """four frames of jittered_blend: each frame's sample is in the staging buffers (= the jittered sampler's frame
    in a plain target), and is blended onto the formatted buffer's quantised contents with 1 / f, 1 - 1 / f"""
    frt, prt = pair(ctx, RC.COLOR_FORMATS[cf_name], RC.DF.none)
    k = kernel_of(scene, "ao")
    frt.clear_color_buffer((0.2, 0.4, 0.6, 0.8))
    state = frt.download_formatted()
    for f in range(1, 5):
        va.render_sampled(ctx, scene.dev, frt, scene.basis, k, PS.jittered_blend_type, frame_num=f)
        va.render_sampled(ctx, scene.dev, prt, scene.basis, k, PS.jittered_type, frame_num=f)
        staging = same_staging(frt, prt)
        s = np.float32(1.0) / np.float32(f)
        state = resolve_host(frt, staging, va.resolve_desc(blend=True, s=float(s), d=float(np.float32(1.0) - s)), state)
        same_formatted(frt.download_formatted(), state)
    frt.close(), prt.close()


@pytest.mark.parametrize("sampler", ["uniform", "jittered", "jittered_blend"])
@pytest.mark.parametrize("cf_name,df_name", [("rgba8", "depth24s8"), ("rgba32f", "depth32f"), ("rgb8", "depth32f"), ("rgb32f", "depth24s8")])
def test_render_view_writes_depth(ctx, scene, oracle_mod, cf_name, df_name, sampler):
    frt, prt = pair(ctx, RC.COLOR_FORMATS[cf_name], RC.DEPTH_FORMATS[df_name])
    k = kernel_of(scene, "ao" if sampler != "jittered" else "primary")
    frt.clear_color_buffer((0.0, 0.0, 0.0, 0.0))
    frt.clear_depth_buffer(1.0)
    state = frt.download_formatted()
    for f in ((1, 2) if sampler == "jittered_blend" else (7,)):
        va.render_view(ctx, scene.dev, frt, scene.vcam, k, getattr(PS, sampler + "_type"), frame_num=f)
        va.render_view(ctx, scene.dev, prt, scene.vcam, k, PS.uniform_type if sampler == "uniform" else PS.jittered_type, frame_num=f)
        staging = same_staging(frt, prt)
        s = np.float32(1.0) / np.float32(f)
        blend = sampler == "jittered_blend"
        desc = va.resolve_desc(blend=blend, s=float(s) if blend else 1.0, d=float(np.float32(1.0) - s) if blend else 0.0,
                               view=scene.view, proj=scene.proj, jitter=sampler != "uniform", frame_num=f)
        state = resolve_host(frt, staging, desc, state)
        same_formatted(frt.download_formatted(), state)
    # independently of the twin, which shares its ray with the kernel: the frame's prim ids and t are the oracle's for this
    # sampler and frame number, and the stored depth is that of the hit point recomputed in doubles from the documented
    # jitter draws -- the un-jittered pixel centre's depth is not
    ocam = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, -1), W, H)
    ref = oracle_mod.render_sampled(scene.oracle_scene, ocam, "uniform" if sampler == "uniform" else "jittered", mode=oracle_mod.VO_MODE_PRIMARY,
                                    frame_num=f, matrices=(scene.view.T.reshape(16), scene.proj.T.reshape(16)))
    assert np.array_equal(staging["prim_id"], ref["prim_id"]) and np.array_equal(bits(staging["t"]), bits(ref["t"]))
    if sampler != "jittered_blend":
        got = state["depth"].astype(np.float64) if df_name == "depth32f" else (state["depth"] >> 8).astype(np.float64) / 16777215.0
        atol = RC.DEPTH_ATOL + (0.0 if df_name == "depth32f" else 1.0 / 16777215.0)
        want = RC.depth_in_doubles(scene.view, scene.proj, W, H, ref["prim_id"], ref["t"], jitter=sampler == "jittered", frame_num=f)
        assert np.max(np.abs(got - want)) <= atol, float(np.max(np.abs(got - want)))
        if sampler == "jittered":
            centre = RC.depth_in_doubles(scene.view, scene.proj, W, H, ref["prim_id"], ref["t"])
            hit = ref["prim_id"] != RC.MISS         # (a miss stores 1.0 whatever the ray)
            assert np.mean(np.abs(got - centre)[hit] > atol) > 0.25, "the check tells the jittered ray from the pixel centre's"
    depth = state["depth"] if df_name == "depth32f" else (state["depth"] >> 8).astype(np.float64) / 16777215.0
    hit = staging["prim_id"] != RC.MISS
    assert hit.any() and np.all(depth[hit] < 1.0) and np.all(depth[hit] > 0.0)
    if sampler != "jittered_blend":
        assert np.all(depth[~hit] == 1.0)
    frt.close(), prt.close()


def test_render_view_matches_the_reference_frame(ctx):
    """rt_frame.npz: the reference's simple_sched frame with camera matrices, its colour re-derived from the prim id"""
    fx = RC.frame_fixture()
    w, h = (int(x) for x in fx["size"])
    prims = np.ascontiguousarray(fx["prims"]).view(va.TRIANGLE_DTYPE).reshape(-1)
    dev = va.hip_index_bvh(ctx, va.build_index_bvh(prims), va.face_normals(prims))
    vcam = va.view_camera(fx["view"], fx["proj"], w, h)
    for cf, df, ck, dk in ((RC.CF.rgba8, RC.DF.depth24_stencil8, "rgba8", "depth24s8"), (RC.CF.rgb8, RC.DF.depth32f, "rgb8", "depth32f")):
        rt = va.hip_buffer_rt(ctx, w, h, color_format=cf, depth_format=df)
        va.render_view(ctx, dev, rt, vcam, va.closest_hit_kernel(dev))
        got = rt.download_formatted()
        st = rt.download()
        assert np.array_equal(st["prim_id"], fx["prim_id"]) and np.array_equal(bits(st["t"]), fx["t"])
        assert np.array_equal(bits(got["depth"]), fx[dk]), "the depth buffer is the reference's"
        # the built-in kernel's colour is not the generator's: put the generator's in and resolve again
        rt.upload(color=RC.prim_color(st["prim_id"]))
        rt.resolve(va.resolve_desc(view=fx["view"], proj=fx["proj"]))
        got = rt.download_formatted()
        assert np.array_equal(got["color"], fx[ck]) and np.array_equal(bits(got["depth"]), fx[dk])
        rt.close()
    dev.close()


def test_volume_frames_into_rgba8(ctx):
    F = VC.load_frame("vol_example")
    tf, k, cam, filt, addr = VC.frame_objects(F)
    vol = va.volume(ctx, F["voxels"], filt, addr, tf)
    frt = va.hip_buffer_rt(ctx, cam.width, cam.height, color_format=RC.CF.rgba8)
    prt = va.hip_buffer_rt(ctx, cam.width, cam.height)
    try:
        for rt in (frt, prt):
            sp = va.make_sched_params(PS.uniform_type, VC.fixed_camera(cam), rt)
            va.hip_sched(ctx, async_frames=False).frame(va.api._volume_kernel(vol, k), sp)
        staging = same_staging(frt, prt)
        assert np.array_equal(bits(staging["color"]), bits(F["color"]))
        same_formatted(frt.download_formatted(), resolve_host(frt, staging, va.resolve_desc()))
    finally:
        frt.close(), prt.close(), vol.close()


def test_multi_volume_frames_into_rgba8(ctx):
    """a frame with a scissor box: the pixels outside keep what the clear left, in all buffers"""
    F = MC.load_frame("mv_example")
    vox, tfs, filters, addresses, entries, k, cam = MC.frame_objects(F)
    vols = [va.volume(ctx, vox[i], filters[i], addresses[i], tfs[i]) for i in range(len(vox))]
    kern = va.api._multi_volume_kernel(vols, entries, k)
    frt = va.hip_buffer_rt(ctx, cam.width, cam.height, color_format=RC.CF.rgba8)
    prt = va.hip_buffer_rt(ctx, cam.width, cam.height)
    box = (3, 2, cam.width - 5, cam.height - 1)
    try:
        for rt in (frt, prt):
            rt.clear_color_buffer((0.5, 0.25, 1.0, 1.0))
            sp = va.make_sched_params(PS.uniform_type, VC.fixed_camera(cam), rt)
            sp.scissor_box = box
            va.hip_sched(ctx, async_frames=False).frame(kern, sp)
        staging = same_staging(frt, prt)
        cleared = va.rt_resolve_host(RC.CF.rgba8, RC.DF.none, cam.width, cam.height, np.tile(np.float32([0.5, 0.25, 1.0, 1.0]), (len(staging["t"]), 1)),
                                     va.resolve_desc())
        want = resolve_host(frt, staging, va.resolve_desc(scissor=box), cleared)
        same_formatted(frt.download_formatted(), want)
        assert (want["color"] != cleared["color"]).any()
    finally:
        frt.close(), prt.close()
        for v in vols:
            v.close()


# ---- ordering ------------------------------------------------------------------------------------------------

def test_asynchronous_frames_on_two_lanes(ctx, scene):
    """two formatted targets rendered alternately, then one twice in a row, on two frame lanes: every resolve runs
    after its own frame and before the next frame into the target, so the result is the synchronous run's"""
    k = kernel_of(scene, "ao")

    def run(async_on):
        a = va.hip_buffer_rt(ctx, W, H, color_format=RC.CF.rgba8)
        b = va.hip_buffer_rt(ctx, W, H, color_format=RC.CF.rgb8, depth_format=RC.DF.depth24_stencil8)
        ctx.set_option("async_frames", 2 if async_on else 0)
        try:
            for f in range(1, 4):
                va.render_sampled(ctx, scene.dev, a, scene.basis, k, PS.jittered_blend_type, frame_num=f)
                va.render_view(ctx, scene.dev, b, scene.vcam, k, PS.jittered_blend_type, frame_num=f)
            va.render_sampled(ctx, scene.dev, a, scene.basis, k, PS.jittered_blend_type, frame_num=4)
            va.render_sampled(ctx, scene.dev, a, scene.basis, k, PS.jittered_blend_type, frame_num=5)
            out = a.download_formatted(), b.download_formatted(), a.download(), b.download()
        finally:
            ctx.set_option("async_frames", 0)
        a.close(), b.close()
        return out

    sync, asyn = run(False), run(True)
    for x, y in zip(sync[:2], asyn[:2]):
        same_formatted(y, x)
    for x, y in zip(sync[2:], asyn[2:]):
        for key in ("color", "prim_id", "t"):
            assert np.array_equal(bits(x[key]), bits(y[key]))


# ---- refusals ------------------------------------------------------------------------------------------------

def snapshot(rt):
    return rt.download_formatted(), rt.download()


def unchanged(rt, snap):
    now = snapshot(rt)
    return all(a[k].tobytes() == b[k].tobytes() for a, b in zip(now, snap) for k in a)


def marked(ctx, w, h, cf, df):
    rt = va.hip_buffer_rt(ctx, w, h, color_format=cf, depth_format=df)
    n = w * h
    rng = np.random.default_rng(5)
    rt.upload(color=rng.uniform(0, 1, (n, 4)).astype(np.float32), prim_id=rng.integers(0, 99, n).astype(np.uint32),
              t=rng.uniform(0, 9, n).astype(np.float32), occ=rng.integers(0, 256, n).astype(np.uint8))
    f = rt.download_formatted()
    rt.upload_formatted(**{k: rng.integers(0, 255, v.shape).astype(v.dtype) for k, v in f.items()})
    return rt


def refused(call, code, *words):
    with pytest.raises(va.VrhError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_refusals_leave_the_target_untouched(ctx, scene):
    U = _capi.VRH_ERR_UNSUPPORTED
    ao = kernel_of(scene, "ao")
    rt = marked(ctx, W, H, RC.CF.rgba8, RC.DF.none)
    snap = snapshot(rt)
    refused(lambda: va.render_sampled(ctx, scene.dev, rt, scene.basis, ao, PS.ssaa_type(4)), U, "ssaa", "formatted")
    refused(lambda: va.render_view(ctx, scene.dev, rt, scene.vcam, ao, PS.ssaa_type(2)), U, "ssaa", "formatted")
    refused(lambda: va.render(ctx, scene.dev, rt, scene.basis, ao, shard=_capi.vrh_shard(0, 1, 0, 0)), U, "shard")
    refused(lambda: va.unshard(ctx, W, H, 1, rt, kernel=ao), U, "formatted", "unshard")
    (g,) = va.render_group.local([ctx])
    refused(lambda: g.render(scene.dev, ao, rt, [scene.basis]), U, "formatted", "render group")
    g.close()
    assert unchanged(rt, snap)
    rt.close()

    tall = marked(ctx, W, 2 * H, RC.CF.rgb8, RC.DF.none)
    snap = snapshot(tall)
    refused(lambda: va.render_batch(ctx, scene.dev, tall, [scene.basis, scene.basis], ao), U, "batch", "formatted")
    assert unchanged(tall, snap)
    tall.close()

    drt = marked(ctx, W, H, RC.CF.rgba8, RC.DF.depth24_stencil8)
    snap = snapshot(drt)
    refused(lambda: va.render(ctx, scene.dev, drt, scene.basis, ao), U, "depth", "vrh_render_view")
    refused(lambda: va.render_sampled(ctx, scene.dev, drt, scene.basis, ao, PS.jittered_type), U, "depth", "vrh_render_view")
    assert unchanged(drt, snap)
    drt.close()


def test_depth_targets_are_refused_by_the_volume_kernels(ctx):
    U = _capi.VRH_ERR_UNSUPPORTED
    F = VC.load_frame("vol_example")
    tf, k, cam, filt, addr = VC.frame_objects(F)
    vol = va.volume(ctx, F["voxels"], filt, addr, tf)
    drt = marked(ctx, cam.width, cam.height, RC.CF.rgba8, RC.DF.depth32f)
    snap = snapshot(drt)
    sp = va.make_sched_params(PS.uniform_type, VC.fixed_camera(cam), drt)
    refused(lambda: va.hip_sched(ctx, async_frames=False).frame(va.api._volume_kernel(vol, k), sp), U, "vrh_render_volume", "depth")
    M = MC.load_frame("mv_example")
    vox, tfs, filters, addresses, entries, mk, mcam = MC.frame_objects(M, cam.width, cam.height)
    vols = [va.volume(ctx, vox[i], filters[i], addresses[i], tfs[i]) for i in range(len(vox))]
    sp = va.make_sched_params(PS.uniform_type, VC.fixed_camera(mcam), drt)
    refused(lambda: va.hip_sched(ctx, async_frames=False).frame(va.api._multi_volume_kernel(vols, entries, mk), sp), U,
            "vrh_render_multi_volume", "depth")
    ok = unchanged(drt, snap)
    drt.close(), vol.close()
    for v in vols:
        v.close()
    assert ok
