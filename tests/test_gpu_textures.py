"""GPU: diffuse maps (vrh_shading_set_textures) in the simple, whitted and path-tracing kernels against the
reference's own textured frames.

tests/golden/tex_*.npz hold frames of the reference's simple::kernel, whitted::kernel and
pathtracing::kernel with the textured parameter pack (tests/golden/textured_ref.cpp, run by
make_textured_golden.py), each with its scene, materials, lights, texture coordinates, textures and camera.
Bars: hits and t bit-exact everywhere; the path-traced frames that reach no powf (matte, emissive, mirror,
plastic with ks = 0) bit-identical; simple / whitted radiance within the project's 1e-5 relative (a texture
factor is an exact multiply on the diffuse term); the path tracer with ks > 0 within the fixture's rtol
(twice the response of the reference's frame to powf moving by one float), tests/pt_cases.py check_frame's
bar.  Without a fixture: dummy textures and 1x1 textures of 255 render the bits of the untextured shading.
"""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest

import visionaray_amd as va
from visionaray_amd import _capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tex_cases as TC  # noqa: E402
from pt_cases import check_frame  # noqa: E402
from test_textures import write_textured_obj  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MISS = 0xFFFFFFFF
RTOL = 1e-5          # tests/test_gpu_shading.py, tests/test_gpu_whitted.py
with open(os.path.join(HERE, "golden", "textured.json")) as _f:
    TEX = json.load(_f)
EXACT = ["tex_simple_face", "tex_whitted_vertex", "tex_path_diffuse", "tex_path_generic"]   # one per kernel family


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def fixture(case):
    with np.load(os.path.join(HERE, "golden", case + ".npz")) as z:
        arrs = {k: z[k] for k in z.files}
    for a in arrs.values():
        a.setflags(write=False)
    return arrs


def camera_of(basis, W, H):
    cam = _capi.vrh_camera()
    cam.eye[:], cam.cam_u[:], cam.cam_v[:], cam.cam_w[:] = (list(map(float, r)) for r in basis)
    cam.width, cam.height = W, H
    return cam


class fixed_camera:
    """a camera whose pinhole basis is the fixture's (hip_sched.frame asks a camera for its basis)"""

    def __init__(self, cam):
        self.cam = cam

    def basis(self, w, h):
        assert (w, h) == (self.cam.width, self.cam.height)
        return self.cam


def textures_of(z, kind="fixture"):
    out = []
    for i, (w, h, f, ax, ay) in enumerate(z["tex_params"]):
        if kind == "dummy":
            out.append(None)
        elif kind == "ones":
            # Mirror axes become Wrap: on one texel Mirror maps odd periods to 0 / 1 - frac < 0, the linear
            # filter then extrapolates, and (1 - x) * 255 + x * 255 rounds below 255 for about a sixth of
            # the coordinates -- in the reference too (the 1x1 mirror configurations of tex2d_samples.npz,
            # which vrh_tex2d_host equals bit for bit), so such a texture is not white there either
            wrap = lambda a: va.tex_address.wrap if int(a) == va.tex_address.mirror else int(a)  # noqa: E731
            out.append(va.texture(np.full((1, 1, 4), 255, np.uint8), int(f), (wrap(ax), wrap(ay))))
        else:
            out.append(None if w == 0 or h == 0 else va.texture(z["tex%d" % i], int(f), (int(ax), int(ay))))
    return out


def setup(ctx, case, textures="fixture"):
    """device scene, shading (textured unless textures is None), kernel, camera of a fixture"""
    g, z = TEX[case], fixture(case)
    prims = np.ascontiguousarray(z["prims"]).view(va.TRIANGLE_DTYPE).reshape(-1)
    dev = va.hip_index_bvh(ctx, va.build_index_bvh(prims), z["normals"])
    if "vertex_normals" in z:
        dev.set_vertex_normals(z["vertex_normals"])
    lights = np.ascontiguousarray(z["lights"]).view(va.POINT_LIGHT_DTYPE).reshape(-1)
    if g["generic"]:
        sh = va.generic_shading(ctx, np.ascontiguousarray(z["materials"]).view(va.MATERIAL_DTYPE).reshape(-1))
    else:
        m = np.ascontiguousarray(z["materials"][:, 1:14]).view(va.PLASTIC_DTYPE).reshape(-1)
        sh = va.shading(ctx, m, lights)
    if textures is not None:
        sh.set_textures(z["tex_coords"], textures_of(z, textures))
    binding = va.normals_per_vertex_binding if g["binding"] == "vertex" else va.normals_per_face_binding
    kw = dict(binding=binding, bg=tuple(g["bg"]), ambient=tuple(g["ambient"]))
    if g["algo"] == "simple":
        k = va.simple_kernel(dev, sh, **kw)
    elif g["algo"] == "whitted":
        k = va.whitted_kernel(dev, sh, num_bounces=g["bounces"], epsilon=g["eps"], **kw)
    else:
        k = va.pathtracing_kernel(dev, sh, num_bounces=g["bounces"], epsilon=g["eps"], **kw)
    return dev, sh, k, camera_of(z["camera"], g["W"], g["H"])


def frame(ctx, k, cam, frame_num=0, sampler=None, rt=None):
    """one frame through hip_sched.frame"""
    rt = rt or va.hip_buffer_rt(ctx, cam.width, cam.height)
    sp = va.make_sched_params(sampler or va.pixel_sampler.uniform_type, fixed_camera(cam), rt)
    va.hip_sched(ctx).frame(k, sp, frame_num=frame_num)
    return rt.download()


def check_primary(out, z):
    assert np.array_equal(out["prim_id"], z["prim_id"])
    assert np.array_equal(bits(out["t"]), bits(z["t"]))
    return out["prim_id"] != MISS


@pytest.mark.parametrize("case", ["tex_simple_face", "tex_simple_vertex", "tex_whitted_face", "tex_whitted_vertex"])
def test_simple_and_whitted_frames(ctx, case):
    g, z = TEX[case], fixture(case)
    dev, sh, k, cam = setup(ctx, case)
    out = frame(ctx, k, cam)
    hit = check_primary(out, z)
    ref = z["color_f0"]
    assert hit.any()
    assert np.array_equal(bits(out["color"][~hit]), bits(ref[~hit]))
    rel = np.abs(out["color"].astype(np.float64) - ref) / np.where(ref == 0.0, 1.0, np.abs(ref))
    print(f"{case}: max rel {rel.max():.3e}, bit-identical pixels {np.mean(np.all(bits(out['color']) == bits(ref), axis=1)):.4f}")
    np.testing.assert_allclose(out["color"], ref, rtol=RTOL, atol=0.0)
    # the textures matter: the untextured shading renders another frame
    sh.set_textures(None, None)
    plain = frame(ctx, k, cam)
    assert np.array_equal(plain["prim_id"], out["prim_id"]) and not np.array_equal(bits(plain["color"]), bits(out["color"]))


@pytest.mark.parametrize("case,fr", [(c, f) for c in ("tex_path_diffuse", "tex_path_generic", "tex_path_generic_vertex")
                                     for f in TEX[c]["frames"]])
def test_powf_free_path_frames_are_bit_identical(ctx, case, fr):
    g, z = TEX[case], fixture(case)
    dev, sh, k, cam = setup(ctx, case)
    out = frame(ctx, k, cam, frame_num=fr)
    st = ctx.last_frame_stats()
    hit = check_primary(out, z)
    ref = z["color_f%d" % fr]
    differ = np.any(bits(out["color"]) != bits(ref), axis=1)
    assert not differ.any(), f"{int(differ.sum())} of {differ.size} pixels differ from the reference frame (first {int(np.argmax(differ))})"
    assert st["rays"] == g["rays"][str(fr)]
    assert st["hits"] == int(hit.sum()) and hit.any()


def test_jittered_blend_accumulation_is_bit_identical(ctx):
    g, z = TEX["tex_path_blend"], fixture("tex_path_blend")
    dev, sh, k, cam = setup(ctx, "tex_path_blend")
    rt = va.hip_buffer_rt(ctx, g["W"], g["H"])
    rt.clear_color_buffer((0.0, 0.0, 0.0, 0.0))
    first, rays = g["first_frame"], 0
    for n in range(first, first + g["num_frames"]):
        frame(ctx, k, cam, frame_num=n, sampler=va.pixel_sampler.jittered_blend_type, rt=rt)
        rays += ctx.last_frame_stats()["rays"]
        if n == first:
            assert np.array_equal(bits(rt.download()["color"]), bits(z["color_first"]))
    out = rt.download()
    check_primary(out, z)
    assert np.array_equal(bits(out["color"]), bits(z["color_last"]))
    assert rays == g["rays_total"]


def test_specular_plastic_within_derived_tolerance(ctx):
    g, z = TEX["tex_path_plastic"], fixture("tex_path_plastic")
    dev, sh, k, cam = setup(ctx, "tex_path_plastic")
    out = frame(ctx, k, cam, frame_num=g["frames"][0])
    ref = {"prim_id": z["prim_id"], "t": z["t"], "color": z["color_f%d" % g["frames"][0]]}
    assert g["rtol"] > 0.0 and not g["powf_free"] and g["unstable"] == 0.0
    worst = check_frame(out, ref, {"rtol": g["rtol"]}, False, "tex_path_plastic")
    print(f"tex_path_plastic: largest relative difference {worst:.3e}, rtol {g['rtol']:.3e}")


@pytest.mark.parametrize("case", EXACT)
def test_dummies_and_white_texels_render_the_untextured_bits(ctx, case):
    dev, sh, k, cam = setup(ctx, case, textures=None)
    plain = frame(ctx, k, cam, frame_num=3)
    rays = ctx.last_frame_stats()["rays"]
    assert (plain["prim_id"] != MISS).any()
    z = fixture(case)
    for kind in ("dummy", "ones"):
        sh.set_textures(z["tex_coords"], textures_of(z, kind))
        out = frame(ctx, k, cam, frame_num=3)
        for key in ("prim_id", "t", "color"):
            assert np.array_equal(bits(out[key]), bits(plain[key])), (kind, key)
        assert ctx.last_frame_stats()["rays"] == rays
    # textures, then detached: the untextured bits return
    sh.set_textures(z["tex_coords"], textures_of(z))
    tex = frame(ctx, k, cam, frame_num=3)
    assert not np.array_equal(bits(tex["color"]), bits(plain["color"]))
    sh.set_textures(None, [])
    back = frame(ctx, k, cam, frame_num=3)
    assert np.array_equal(bits(back["color"]), bits(plain["color"]))


def test_three_frames_in_flight_equal_their_single_renders(ctx):
    case = "tex_path_generic"
    g, z = TEX[case], fixture(case)
    dev, sh, k, cam = setup(ctx, case)
    W, H = g["W"], g["H"]
    cams = []
    for i in range(3):
        c = camera_of(z["camera"], W, H)
        c.eye[0] += 0.05 * i
        c.eye[1] -= 0.03 * i
        cams.append(c)
    rt = va.hip_buffer_rt(ctx, W, 3 * H)
    va.render_batch(ctx, dev, rt, cams, k, frame_num=5)
    batch = rt.download()
    assert ctx.last_frame_stats()["frames"] == 3
    for i in range(3):
        one = frame(ctx, k, cams[i], frame_num=5 + i)
        for key in ("prim_id", "t", "color"):
            assert np.array_equal(bits(batch[key][i * W * H:(i + 1) * W * H]), bits(one[key])), (i, key)
    assert not np.array_equal(bits(batch["color"][:W * H]), bits(batch["color"][W * H:2 * W * H]))


@pytest.mark.parametrize("case", ["tex_whitted_face", "tex_path_generic"])
def test_shard_equals_the_owned_bands(ctx, case):
    g = TEX[case]
    dev, sh, k, cam = setup(ctx, case)
    W, H = g["W"], g["H"]
    full = frame(ctx, k, cam)
    rt = va.hip_buffer_rt(ctx, W, H)
    rt.clear_color_buffer((7.0, 7.0, 7.0, 7.0))
    va.render(ctx, dev, rt, cam, k, shard=_capi.vrh_shard(1, 3, 0, 0))
    part = rt.download()
    rows = np.arange(H)
    owned = np.repeat((rows // _capi.VRH_BAND_ROWS) % 3 == 1, W)
    assert owned.any() and (~owned).any()
    assert np.array_equal(bits(part["color"][owned]), bits(full["color"][owned]))
    assert np.array_equal(part["prim_id"][owned], full["prim_id"][owned])
    assert np.all(part["color"][~owned] == 7.0)


def test_errors(ctx):
    case = "tex_simple_face"
    g, z = TEX[case], fixture(case)
    dev, sh, k, cam = setup(ctx, case, textures=None)
    texs, tc = textures_of(z), z["tex_coords"]

    def code(fn):
        with pytest.raises(va.VrhError) as e:
            fn()
        return e.value.code

    INV, UNS = _capi.VRH_ERR_INVALID, _capi.VRH_ERR_UNSUPPORTED
    assert code(lambda: sh.set_textures(tc, texs[:-1])) == INV                     # count mismatch
    assert code(lambda: sh.set_textures(tc[:-1], texs)) == INV                     # not three per triangle
    real = next(t for t in texs if t is not None)
    for field, value in (("format", 3), ("filter", 2), ("width", 32769)):
        descs = (_capi.vrh_texture_desc * len(texs))()
        for d, t in zip(descs, texs):
            if t is not None:
                t._fill(d)
        i = texs.index(real)
        setattr(descs[i], field, value)
        tcc = np.ascontiguousarray(tc)
        assert _capi.lib().vrh_shading_set_textures(ctx.handle, sh.handle, tcc.ctypes.data_as(C.c_void_p), len(tcc), descs,
                                                    len(texs)) == INV, field
    descs[texs.index(real)].width = real.width
    descs[texs.index(real)].address[0] = 3
    assert _capi.lib().vrh_shading_set_textures(ctx.handle, sh.handle, tcc.ctypes.data_as(C.c_void_p), len(tcc), descs,
                                                len(texs)) == INV
    descs[texs.index(real)].address[0] = 0
    descs[texs.index(real)].width, descs[texs.index(real)].height = 32768, 16384      # 2^29 texels
    assert _capi.lib().vrh_shading_set_textures(ctx.handle, sh.handle, tcc.ctypes.data_as(C.c_void_p), len(tcc), descs,
                                                len(texs)) == INV
    for bad in (np.nan, np.inf, 2.0 ** 20 + 1.0):
        t2 = tc.copy()
        t2[5, 1] = bad
        assert code(lambda: sh.set_textures(t2, texs)) == INV
    # a failed call leaves the shading untextured and usable
    plain = frame(ctx, k, cam)
    assert (plain["prim_id"] != MISS).any()
    # fewer coordinate triples than the scene has primitives
    sh.set_textures(tc[:3 * (len(tc) // 3 - 1)], texs)
    assert code(lambda: frame(ctx, k, cam)) == INV
    sh.set_textures(tc, texs)
    frame(ctx, k, cam)
    # multi_hit, a hit mask and test counting take no textured shading
    rt = va.hip_buffer_rt(ctx, cam.width, cam.height)
    rt.alloc_multi_hit(4)
    mk = va.multi_hit_kernel(dev, sh, max_hits=4, binding=va.normals_per_face_binding)
    assert code(lambda: va.render(ctx, dev, rt, cam, mk)) == UNS
    mask = va.hit_mask(ctx, tc, np.ones((4, 4), np.uint8))
    assert code(lambda: va.render(ctx, dev, rt, cam, va.with_hit_mask(k, mask))) == UNS
    ck = va.simple_kernel(dev, sh, binding=va.normals_per_face_binding, count_tests=True)
    assert code(lambda: va.render(ctx, dev, rt, cam, ck)) == UNS
    # the primary and AO kernels ignore a shading
    va.render(ctx, dev, rt, cam, va.closest_hit_kernel(dev))


def test_obj_end_to_end(ctx, tmp_path):
    path, px = write_textured_obj(str(tmp_path))
    m = va.load_obj(path)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        texs = m.load_textures()
    dev = va.hip_index_bvh(ctx, va.build_index_bvh(m.primitives), m.geometric_normals)
    lights = np.stack([va.point_light((0.3, 0.4, 2.0), kl=1.5)]).reshape(-1)
    W, H = 40, 28
    cam = va.camera()
    cam.perspective(0.9, np.float32(W) / np.float32(H), 0.001, 100.0)
    cam.look_at((0.5, 0.5, 1.6), (0.5, 0.5, 0.0))

    def render(textures):
        sh = va.shading(ctx, m.materials, lights)
        if textures is not None:
            sh.set_textures(m.tex_coords, textures)
        k = va.simple_kernel(dev, sh, bg=(0.1, 0.2, 0.3, 1.0), ambient=(1.0, 1.0, 1.0, 0.2))
        rt = va.hip_buffer_rt(ctx, W, H)
        va.hip_sched(ctx).frame(k, va.make_sched_params(va.pixel_sampler.uniform_type, cam, rt))
        return rt.download()

    loaded = render(texs)
    by_hand = [None] * len(m.materials)
    for i, name in enumerate(m.material_names):
        if name in ("checker", "again"):
            by_hand[i] = va.texture(px, va.tex_filter.linear, va.tex_address.wrap)
    hand = render(by_hand)
    assert (loaded["prim_id"] != MISS).any()
    for key in ("prim_id", "t", "color"):
        assert np.array_equal(bits(loaded[key]), bits(hand[key])), key
    assert not np.array_equal(bits(render(None)["color"]), bits(loaded["color"]))
