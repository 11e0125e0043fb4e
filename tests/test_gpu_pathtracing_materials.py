"""GPU: VRH_KERNEL_PATHTRACING over tagged materials (vrh_shading_create_generic: plastic, matte, mirror,
emissive by the hit's record) against the reference's own frames.

tests/golden/ptm_*.npz hold frames of the reference's pathtracing::kernel over
generic_material<plastic, matte, mirror, emissive> (tests/golden/generic_material_ref.cpp, run by
make_generic_material_golden.py), each with its scene, materials and camera.  matte, mirror and emissive
never reach powf: the GPU frame is bit-identical.  ptm_room_plastic has a plastic with ks > 0: within
the fixture's rtol (twice the response of the reference's frame to powf moving by one float) on at least
99 % of the hit pixels, tests/pt_cases.py check_frame's bar.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import visionaray_amd as va
from visionaray_amd import _capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pt_cases import check_frame  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MISS = 0xFFFFFFFF
with open(os.path.join(HERE, "golden", "pathtrace_materials.json")) as _f:
    PTM = json.load(_f)
BITS = [(c, f) for c in ("ptm_room_emitter", "ptm_room_vertex", "ptm_soup_env") for f in PTM[c]["frames"]]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def fixture(case):
    """the arrays of a fixture (loaded once, read-only)"""
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


def scene_of(ctx, z):
    prims = np.ascontiguousarray(z["prims"]).view(va.TRIANGLE_DTYPE).reshape(-1)
    dev = va.hip_index_bvh(ctx, va.build_index_bvh(prims), z["normals"])
    if "vertex_normals" in z:
        dev.set_vertex_normals(z["vertex_normals"])
    return dev


def setup(ctx, case, materials=None, **over):
    """device scene, path-tracing kernel over the fixture's (or the given) tagged materials, camera"""
    g, z = dict(PTM[case], **over), fixture(case)
    dev = scene_of(ctx, z)
    m = np.ascontiguousarray(z["materials"]).view(va.MATERIAL_DTYPE).reshape(-1) if materials is None else materials
    sh = va.generic_shading(ctx, m)
    binding = va.normals_per_vertex_binding if g["binding"] == "vertex" else va.normals_per_face_binding
    k = va.pathtracing_kernel(dev, sh, binding=binding, bg=tuple(g["bg"]), ambient=tuple(g["ambient"]),
                              num_bounces=g["bounces"], epsilon=g["eps"])
    return dev, k, camera_of(z["camera"], g["W"], g["H"])


def frame(ctx, dev, k, cam, frame_num=0, shard=None, rt=None):
    rt = rt or va.hip_buffer_rt(ctx, cam.width, cam.height)
    va.render(ctx, dev, rt, cam, k, shard=shard, frame_num=frame_num)
    return rt.download()


def check_primary(out, z):
    assert np.array_equal(out["prim_id"], z["prim_id"])
    assert np.array_equal(bits(out["t"]), bits(z["t"]))
    return out["prim_id"] != MISS


@pytest.mark.parametrize("case,fr", BITS)
def test_powf_free_frames_are_bit_identical(ctx, case, fr):
    g, z = PTM[case], fixture(case)
    dev, k, cam = setup(ctx, case)
    out = frame(ctx, dev, k, cam, frame_num=fr)
    st = ctx.last_frame_stats()
    hit = check_primary(out, z)
    ref = z["color_f%d" % fr]
    differ = np.any(bits(out["color"]) != bits(ref), axis=1)
    assert not differ.any(), f"{int(differ.sum())} of {differ.size} pixels differ from the reference frame (first {int(np.argmax(differ))})"
    assert st["rays"] == g["rays"][str(fr)]
    assert st["hits"] == int(hit.sum()) and hit.any()
    light = np.any(ref[:, :3] != 0.0, axis=1)
    assert (hit & light).any() and ((~hit).any() or (hit & ~light).any())


def test_jittered_blend_accumulation_is_bit_identical(ctx):
    g, z = PTM["ptm_room_blend"], fixture("ptm_room_blend")
    dev, k, cam = setup(ctx, "ptm_room_blend")
    rt = va.hip_buffer_rt(ctx, g["W"], g["H"])
    rt.clear_color_buffer((0.0, 0.0, 0.0, 0.0))
    first, rays = g["first_frame"], 0
    for n in range(first, first + g["num_frames"]):
        va.render_sampled(ctx, dev, rt, cam, k, va.pixel_sampler.jittered_blend_type, frame_num=n)
        rays += ctx.last_frame_stats()["rays"]
        if n == first:
            assert np.array_equal(bits(rt.download()["color"]), bits(z["color_first"]))
    out = rt.download()
    check_primary(out, z)                     # the last frame's (jittered) first hits
    assert np.array_equal(bits(out["color"]), bits(z["color_last"]))
    assert rays == g["rays_total"]


def test_plastic_among_the_kinds_within_derived_tolerance(ctx):
    g, z = PTM["ptm_room_plastic"], fixture("ptm_room_plastic")
    dev, k, cam = setup(ctx, "ptm_room_plastic")
    out = frame(ctx, dev, k, cam, frame_num=g["frames"][0])
    ref = {"prim_id": z["prim_id"], "t": z["t"], "color": z["color_f%d" % g["frames"][0]]}
    assert g["rtol"] > 0.0 and not g["powf_free"]
    worst = check_frame(out, ref, {"rtol": g["rtol"]}, False, "ptm_room_plastic")
    print(f"ptm_room_plastic: largest relative difference {worst:.3e}, rtol {g['rtol']:.3e}")


def test_all_emissive_is_the_radiance_after_one_ray(ctx):
    g, z = PTM["ptm_soup_env"], fixture("ptm_soup_env")
    m = np.stack([va.emissive(ce=(0.25, 0.5, 0.75), ls=3.0)] * len(g["materials"]))
    dev, k, cam = setup(ctx, "ptm_soup_env", materials=m)
    out = frame(ctx, dev, k, cam)
    hit = check_primary(out, z)
    assert hit.any() and (~hit).any()
    want = np.float32([np.float32(0.25) * np.float32(3.0), np.float32(0.5) * np.float32(3.0), np.float32(0.75) * np.float32(3.0), 1.0])
    assert np.array_equal(bits(out["color"][hit]), bits(np.tile(want, (int(hit.sum()), 1))))
    assert ctx.last_frame_stats()["rays"] == g["W"] * g["H"]


def test_all_mirror_closed_box_is_black_and_every_path_alive(ctx):
    """The plain box of the example (emissive_box: no triangle cuts a wall, so no origin offset along the
    next direction can carry a path outside; the fixtures' rooms do lose a few mirror paths that way, in
    the reference too: 15828 of 15840 rays in ptm_room_emitter's room).  The reference traces 6 * pixels
    rays here as well."""
    prims, four = emissive_box()
    W, H = 60, 44
    m = np.stack([va.mirror(cr=(0.9, 0.8, 0.7), kr=0.95, ior=(0.2, 0.9, 1.1), absorption=(3.9, 2.4, 2.2))] * len(four))
    dev = va.hip_index_bvh(ctx, va.build_index_bvh(prims), va.face_normals(prims))
    k = va.pathtracing_kernel(dev, va.generic_shading(ctx, m), bg=(0.1, 0.2, 0.3, 1.0), ambient=(0.0, 0.0, 0.0, 1.0),
                              num_bounces=6)
    out = frame(ctx, dev, k, box_camera(W, H).basis(W, H))
    n = W * H
    assert np.array_equal(bits(out["color"]), bits(np.tile(np.float32([0, 0, 0, 1]), (n, 1))))
    assert ctx.last_frame_stats()["rays"] == 6 * n


def test_generic_shading_of_plastics_renders_the_plastic_shading_bits(ctx, oracle_mod):
    """pt_cornell12_plastic's scene and settings: both paths call the device's powf, no tolerance"""
    from test_gpu_multi_hit import camera_of as scene_camera, product_scene
    O = oracle_mod
    with open(os.path.join(HERE, "golden", "pathtrace.json")) as f:
        g = json.load(f)["pt_cornell12_plastic"]
    dev = product_scene(ctx, O, g["scene"])
    m, lt, _, bg = O.whitted_spec()
    m, lt = m.view(va.PLASTIC_DTYPE), lt.view(va.POINT_LIGHT_DTYPE)
    cam = scene_camera(O, g["scene"], g["W"], g["H"])
    kw = dict(bg=bg, ambient=g["ambient"], num_bounces=g["bounces"], epsilon=g["eps"])
    plain = frame(ctx, dev, va.pathtracing_kernel(dev, va.shading(ctx, m, lt), **kw), cam, frame_num=g["frames"][0])
    rays = ctx.last_frame_stats()["rays"]
    lifted = va.generic_materials(m)
    assert lifted.dtype == va.MATERIAL_DTYPE and np.all(lifted["kind"] == va.MATERIAL_PLASTIC)
    gen = frame(ctx, dev, va.pathtracing_kernel(dev, va.generic_shading(ctx, lifted, lt), **kw), cam, frame_num=g["frames"][0])
    assert (plain["prim_id"] != MISS).any()
    for key in ("prim_id", "t", "color"):
        assert np.array_equal(bits(gen[key]), bits(plain[key])), key
    assert ctx.last_frame_stats()["rays"] == rays


@pytest.mark.parametrize("occ", [0, 1])
def test_frames_in_flight_equal_single_frames(ctx, occ):
    g = PTM["ptm_room_emitter"]
    W, H = g["W"], g["H"]
    dev, k, cam = setup(ctx, "ptm_room_emitter")
    ctx.set_option("waves_per_simd", occ)
    try:
        singles = [frame(ctx, dev, k, cam, frame_num=5 + f) for f in range(3)]
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


def test_shard_and_scissor_draw_the_whole_image_numbers(ctx):
    g = PTM["ptm_room_vertex"]               # 60 x 44: partial tiles on both edges
    W, H = g["W"], g["H"]
    dev, k, cam = setup(ctx, "ptm_room_vertex")
    whole = frame(ctx, dev, k, cam, frame_num=3)
    fill = np.float32([0.25, 0.5, 0.75, 0.125])

    def prefilled():
        rt = va.hip_buffer_rt(ctx, W, H)
        rt.clear_color_buffer(tuple(float(x) for x in fill))     # side buffers: miss
        return rt

    rows = np.arange(W * H) // W
    cols = np.arange(W * H) % W
    # shard 1 of 3, unpacked: the bands (8 rows) b with b % 3 == 1
    part = frame(ctx, dev, k, cam, frame_num=3, shard=_capi.vrh_shard(1, 3, 0, 0), rt=prefilled())
    mine = (rows // _capi.VRH_BAND_ROWS) % 3 == 1
    # a scissor box that cuts through 8x8 tiles
    box = (5, 3, 43, 30)
    cam2 = camera_of(fixture("ptm_room_vertex")["camera"], W, H)
    cam2.scissor[:] = list(box)
    cut = frame(ctx, dev, k, cam2, frame_num=3, rt=prefilled())
    inside = (cols >= box[0]) & (cols < box[2]) & (rows >= box[1]) & (rows < box[3])
    for got, sel in ((part, mine), (cut, inside)):
        assert sel.any() and (~sel).any()
        for key in ("prim_id", "t", "color"):
            assert np.array_equal(bits(got[key][sel]), bits(whole[key][sel])), key
        assert np.array_equal(got["color"][~sel], np.tile(fill, (int((~sel).sum()), 1)))
        assert np.all(got["prim_id"][~sel] == MISS)


def test_counting_variant_renders_the_same_frame(ctx):
    g = PTM["ptm_room_vertex"]
    dev, k, cam = setup(ctx, "ptm_room_vertex")
    plain = frame(ctx, dev, k, cam, frame_num=0)
    kc = va.pathtracing_kernel(dev, k.shade, binding=va.normals_per_vertex_binding, bg=tuple(g["bg"]),
                               ambient=tuple(g["ambient"]), num_bounces=g["bounces"], epsilon=g["eps"], count_tests=True)
    counted = frame(ctx, dev, kc, cam, frame_num=0)
    st = ctx.last_frame_stats()
    for key in ("prim_id", "t", "color"):
        assert np.array_equal(bits(counted[key]), bits(plain[key])), key
    assert st["rays"] == g["rays"]["0"]
    assert st["box_tests"] > 0 and st["prim_tests"] > 0


def _refused(code, fn, *args, **kw):
    with pytest.raises(va.VrhError) as e:
        fn(*args, **kw)
    assert e.value.code == code, str(e.value)
    assert _capi.lib().vrh_last_error().decode() != ""


def test_refusals(ctx):
    g, z = PTM["ptm_room_vertex"], fixture("ptm_room_vertex")
    W, H = g["W"], g["H"]
    dev, k, cam = setup(ctx, "ptm_room_vertex")
    rt = va.hip_buffer_rt(ctx, W, H)
    UNS, INV = _capi.VRH_ERR_UNSUPPORTED, _capi.VRH_ERR_INVALID
    _refused(UNS, va.render, ctx, dev, rt, cam, va.simple_kernel(dev, k.shade))
    _refused(UNS, va.render, ctx, dev, rt, cam, va.whitted_kernel(dev, k.shade))
    mh = va.hip_buffer_rt(ctx, W, H)
    mh.alloc_multi_hit(4)
    _refused(UNS, va.render, ctx, dev, mh, cam, va.multi_hit_kernel(dev, k.shade, max_hits=4))
    # an unknown kind, at creation
    bad = np.ascontiguousarray(z["materials"]).view(va.MATERIAL_DTYPE).reshape(-1).copy()
    bad["kind"][1] = 7
    _refused(INV, va.generic_shading, ctx, bad)
    # what the path tracer refuses stays refused with a generic shading
    _refused(UNS, va.render_sampled, ctx, dev, rt, cam, k, va.pixel_sampler.ssaa4_type)
    # nothing above rendered: the target still runs a frame
    out = frame(ctx, dev, k, cam, rt=rt)
    assert np.array_equal(bits(out["color"]), bits(z["color_f0"]))


def test_cpp_example_renders_the_python_layers_frames(ctx, tmp_path):
    """examples/pathtrace_emissive_hip.cpp (hip_shading over vrh_material records, make_hip_pathtracing_kernel,
    jittered_blend_type): its PFM image holds the bits of the same frames issued through the Python layer"""
    exe = os.path.join(os.path.dirname(HERE), "build", "examples", "pathtrace_emissive_hip")
    W, H, frames, bounces = 96, 64, 3, 5
    out = tmp_path / "box.pfm"
    r = subprocess.run([exe, str(W), str(H), str(frames), str(bounces), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    raw = out.read_bytes()
    head = b"PF\n%d %d\n-1.0\n" % (W, H)
    assert raw.startswith(head)
    img = np.frombuffer(raw, np.float32, W * H * 3, len(head)).reshape(W * H, 3)

    prims, m = emissive_box()
    dev = va.hip_index_bvh(ctx, va.build_index_bvh(prims), va.face_normals(prims))
    k = va.pathtracing_kernel(dev, va.generic_shading(ctx, m), bg=(0.1, 0.2, 0.3, 1.0), ambient=(0.0, 0.0, 0.0, 0.0),
                              num_bounces=bounces)
    cam = box_camera(W, H)
    rt = va.hip_buffer_rt(ctx, W, H)
    rt.clear_color_buffer((0.0, 0.0, 0.0, 0.0))
    rays = 0
    for n in range(1, frames + 1):
        va.render_sampled(ctx, dev, rt, cam.basis(W, H), k, va.pixel_sampler.jittered_blend_type, frame_num=n)
        rays += ctx.last_frame_stats()["rays"]
    got = rt.download()["color"]
    assert info["rays"] == rays
    assert np.array_equal(bits(img), bits(got[:, :3]))
    assert np.mean(np.any(got[:, :3] != 0.0, axis=1)) > 0.5      # lit by the ceiling quad alone: ambient is 0


def box_camera(W, H):
    """the camera of examples/pathtrace_emissive_hip.cpp"""
    cam = va.camera()
    cam.perspective(float(np.float32(60.0) * np.float32(va.DEGREES_TO_RADIANS)), np.float32(W) / np.float32(H), 0.001, 1000.0)
    cam.look_at((0.0, 0.0, 0.9), (0.0, -0.1, -1.0), (0.0, 1.0, 0.0))
    return cam


def emissive_box():
    """the scene of examples/pathtrace_emissive_hip.cpp: the box [-1, 1]^3, six quads of two triangles;
    geom 0 matte white (floor, back, front), 1 matte red (left), 2 mirror (right), 3 emissive (a ceiling
    quad below the matte ceiling)"""
    def quad(a, b, c, d, geom):
        a, b, c, d = (np.float32(x) for x in (a, b, c, d))
        return [(a, b - a, c - a, geom), (a, c - a, d - a, geom)]

    t = []
    t += quad((-1, -1, -1), (1, -1, -1), (1, -1, 1), (-1, -1, 1), 0)          # floor
    t += quad((-1, 1, -1), (-1, 1, 1), (1, 1, 1), (1, 1, -1), 0)              # ceiling
    t += quad((-1, -1, -1), (-1, 1, -1), (1, 1, -1), (1, -1, -1), 0)          # back
    t += quad((-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1), 0)              # front
    t += quad((-1, -1, -1), (-1, -1, 1), (-1, 1, 1), (-1, 1, -1), 1)          # left
    t += quad((1, -1, -1), (1, 1, -1), (1, 1, 1), (1, -1, 1), 2)              # right
    t += quad((-0.8, 0.99, -0.8), (-0.8, 0.99, 0.8), (0.8, 0.99, 0.8), (0.8, 0.99, -0.8), 3)   # light
    prims = va.make_triangles([x[0] for x in t], [x[1] for x in t], [x[2] for x in t],
                              geom_id=np.uint32([x[3] for x in t]))
    m = np.stack([va.matte(cd=(0.8, 0.8, 0.8), kd=1.0), va.matte(cd=(0.8, 0.2, 0.2), kd=1.0),
                  va.mirror(cr=(1.0, 1.0, 1.0), kr=0.9, ior=(0.2, 0.9, 1.1), absorption=(3.9, 2.4, 2.2)),
                  va.emissive(ce=(1.0, 0.9, 0.8), ls=8.0)])
    return prims, m
