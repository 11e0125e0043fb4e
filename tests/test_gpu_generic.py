"""GPU: mixed triangle / sphere scenes (VRH_PRIM_GENERIC80) in primary visibility, AO, simple and whitted.

Against the reference's own frames (tests/golden/gp_*.npz, make_generic_primitive_golden.py): prim id and the
bits of t on every pixel in all four kernels, AO masks and AO colour bit for bit, simple / whitted radiance
within the bar tests/test_gpu_shading.py holds those kernels to (1e-5 relative: the device powf; the sphere
normal adds correctly rounded subtractions and divisions only).  Against the existing kinds: a generic list of
triangles only equals the TRI64 upload on every buffer, spheres only the SPHERE48 upload in primary visibility.
Everything the generic instances do not cover is refused with VRH_ERR_UNSUPPORTED and leaves the target alone.
"""
import numpy as np
import pytest

import deep_cases
import gp_cases as G
import visionaray_amd as va
from visionaray_amd import _capi

pytestmark = pytest.mark.gpu
RTOL = 1e-5          # tests/test_gpu_shading.py


def upload(ctx, bvh, tri_normals_of=None):
    """device BVH with the face normals of the list's triangles at their prim ids (a sphere's row stays 0)"""
    normals = np.zeros((len(bvh.prims), 4), np.float32)
    if tri_normals_of is not None and len(tri_normals_of):
        normals[tri_normals_of["prim_id"]] = va.face_normals(tri_normals_of)
    return va.hip_index_bvh(ctx, bvh, normals)


@pytest.fixture(scope="module")
def frames(ctx):
    """frames(case) -> {kernel: buffers} of a fixture under the reference's own tree, rendered once"""
    cache = {}

    def get(case):
        if case not in cache:
            a, s = G.fixture(case), G.spec()[case]
            dev = va.hip_index_bvh(ctx, G.host_bvh(case), a["normals"])
            sh = G.shading_of(ctx, a)
            cam = G.camera_of(a["camera"])
            cache[case] = {k: G.render(ctx, dev, cam, G.kernel(k, dev, sh, s)) for k in G.KERNELS}
            assert dev.info["prim_kind"] == _capi.VRH_PRIM_GENERIC80 and dev.info["num_prims"] == len(a["records"])
        return cache[case]
    return get


@pytest.mark.parametrize("case", G.CASES)
@pytest.mark.parametrize("kind", G.KERNELS)
def test_hits_match_the_reference(frames, case, kind):
    a, out = G.fixture(case), frames(case)[kind]
    assert np.array_equal(out["prim_id"], a["prim_id"])
    assert G.same_bits(out["t"], a["t"])


@pytest.mark.parametrize("case", G.CASES)
def test_primary_and_ao_frames_match_bit_for_bit(frames, case):
    a, f = G.fixture(case), frames(case)
    hit = a["prim_id"] != G.MISS
    bg = np.float32(G.spec()[case]["bg"])
    assert G.same_bits(f["primary"]["color"], np.where(hit[:, None], np.float32(1.0), bg[None, :]).astype(np.float32))
    assert np.array_equal(f["ao"]["occ"], a["occ"])
    assert G.same_bits(f["ao"]["color"], a["ao_color"])
    assert a["occ"].any() and (a["occ"][hit] == 0).any()


@pytest.mark.parametrize("case", G.CASES)
@pytest.mark.parametrize("kind", ["simple", "whitted"])
def test_radiance_matches_the_reference(frames, case, kind):
    a, out = G.fixture(case), frames(case)[kind]
    ref = a[kind + "_color"]
    miss = a["prim_id"] == G.MISS
    assert G.same_bits(out["color"][miss], ref[miss])
    print(case, kind, "max rel diff", float(np.max(np.abs(out["color"] - ref) / np.maximum(np.abs(ref), 1e-30))))
    np.testing.assert_allclose(out["color"], ref, rtol=RTOL, atol=0.0)
    if kind == "whitted":
        assert a["whitted_cross"].any()


def four_frames(ctx, dev, cam, mats_lights, w=G.W, h=G.H):
    s = dict(bg=(0.1, 0.2, 0.3, 1.0), ambient=(1.0, 1.0, 1.0, 1.0), ao_samples=8, ao_radius=0.3, ao_eps=1e-3, bounces=3, eps=1e-3)
    sh = G.shading_of(ctx, mats_lights)
    return {k: G.render(ctx, dev, cam, G.kernel(k, dev, sh, s), w, h) for k in G.KERNELS}


def assert_same_frames(a, b, kinds=G.KERNELS):
    for k in kinds:
        for buf in ("color", "prim_id", "t", "occ"):
            assert G.same_bits(a[k][buf], b[k][buf]), (k, buf)
        assert (a[k]["prim_id"] != G.MISS).any()


@pytest.mark.parametrize("n", [300, 1])
def test_triangles_only_equal_the_tri64_upload(ctx, n):
    tris, _ = G.random_mixed(11, n, 0)
    if n == 1:
        tris = va.make_triangles([[-1.0, -1.0, 0.0]], [[2.5, 0.0, 0.0]], [[0.0, 2.5, 0.0]])
    ml = G.fixture("gp_soup")
    cam = G.outside_camera()
    plain = four_frames(ctx, upload(ctx, va.build_index_bvh(tris), tris), cam, ml)
    gen = four_frames(ctx, upload(ctx, va.build_index_bvh(va.make_generic(tris, None)), tris), cam, ml)
    assert_same_frames(plain, gen)
    if n > 1:
        assert (plain["primary"]["prim_id"] == G.MISS).any() and plain["ao"]["occ"].any()


@pytest.mark.parametrize("n", [300, 1])
def test_spheres_only_equal_the_sphere48_upload(ctx, n):
    _, sph = G.random_mixed(12, 0, n)
    if n == 1:
        sph = va.make_spheres([[0.0, 0.0, 0.0]], [0.7])
    cam = G.outside_camera()
    k = lambda dev: va.closest_hit_kernel(dev)                                 # noqa: E731
    dev_p, dev_g = upload(ctx, va.build_index_bvh(sph)), upload(ctx, va.build_index_bvh(va.make_generic(None, sph)))
    a, b = G.render(ctx, dev_p, cam, k(dev_p)), G.render(ctx, dev_g, cam, k(dev_g))
    assert_same_frames({"primary": a}, {"primary": b}, ["primary"])
    assert (a["prim_id"] == G.MISS).any()


def centre_scene(order):
    """One leaf of four primitives: a far triangle (0), a triangle (1) and a sphere (2) that the centre ray of a 9 x 9
    image from (0, 0, 5) along -z both meets at t = 4 exactly, a far sphere (3).  `order`: the leaf order."""
    tris = va.make_triangles([[-1, -1, -3], [-1, -1, 1]], [[4, 0, 0]] * 2, [[0, 4, 0]] * 2, prim_id=[0, 1])
    sph = va.make_spheres([[0, 0, 0], [0, 0, -6]], [1.0, 0.5], prim_id=[2, 3])
    prims = va.make_generic(tris, sph)                   # list positions = prim ids
    nodes = np.zeros(1, va.BVH_NODE_DTYPE)
    nodes[0]["bbox_min"], nodes[0]["bbox_max"] = [-1, -1, -6.5], [3, 3, 1]
    nodes[0]["first"], nodes[0]["num_prims"] = 0, 4
    return va.index_bvh(prims, nodes, np.array(order, np.uint32), 0), tris


@pytest.mark.parametrize("order,winner", [([0, 1, 2, 3], 1), ([0, 2, 1, 3], 2), ([3, 2, 0, 1], 2), ([1, 3, 2, 0], 1)])
def test_equal_t_resolves_in_leaf_order(ctx, order, winner):
    bvh, tris = centre_scene(order)
    cam = va.camera()
    cam.perspective(0.5, 1.0, 0.001, 1000.0)
    cam.look_at((0.0, 0.0, 5.0), (0.0, 0.0, 0.0))
    dev = upload(ctx, bvh, tris)
    out = G.render(ctx, dev, cam.basis(9, 9), va.closest_hit_kernel(dev), 9, 9)
    centre = 4 * 9 + 4
    assert out["t"][centre] == np.float32(4.0)
    assert out["prim_id"][centre] == winner


def comb(depth):
    """a comb of `depth` levels as TRI64 and as GENERIC80 under the same tree, and the axial camera: a ray crosses
    every leaf box, so the walk holds a pushed leaf per level"""
    tris, bvh = deep_cases.comb_bvh(depth + 1, deep_cases.PITCH)
    gen = va.index_bvh(va.make_generic(tris, None), bvh.nodes, bvh.indices, depth)
    cam = va.camera()
    L = depth * deep_cases.PITCH
    cam.perspective(0.8, np.float32(G.W) / np.float32(G.H), 0.001, 1000.0)
    cam.look_at((L + 1.0, 0.2, 0.2), (0.0, 0.2, 0.2))
    return tris, bvh, gen, cam.basis(G.W, G.H)


def test_comb_40_deep_equals_tri64_or_is_refused(ctx):
    """(40 levels are within every kernel's LDS limit, gp_cases.DEPTH_LIMIT: the frames must render)"""
    tris, bvh, gen, cam = comb(40)
    ml = G.fixture("gp_soup")
    plain = four_frames(ctx, upload(ctx, bvh, tris), cam, ml)
    dev = upload(ctx, gen, tris)
    assert dev.info["max_depth"] == 40 < min(G.DEPTH_LIMIT.values())
    got = four_frames(ctx, dev, cam, ml)
    assert_same_frames(plain, got)


DEEP_SPEC = dict(bg=(0.1, 0.2, 0.3, 1.0), ambient=(1.0, 1.0, 1.0, 1.0), ao_samples=8, ao_radius=0.3, ao_eps=1e-3, bounces=3, eps=1e-3)


@pytest.mark.parametrize("kind", G.KERNELS)
def test_comb_at_the_lds_depth_limit_renders(ctx, oracle_mod, kind):
    """the deepest tree the launch plan accepts for this kernel (tests/test_launch_plan.py pins the number): the
    whole stack in LDS, all of a CU's 160 KiB in primary visibility and simple.  Against the oracle's frame and against
    the TRI64 upload of the same tree."""
    depth = G.DEPTH_LIMIT[kind]
    tris, bvh, gen, cam = comb(depth)
    ml = G.fixture("gp_soup")
    dev = upload(ctx, gen, tris)
    assert dev.info["max_depth"] == depth
    sh = G.shading_of(ctx, ml)
    got = G.render(ctx, dev, cam, G.kernel(kind, dev, sh, DEEP_SPEC))
    normals = np.zeros((len(tris), 4), np.float32)
    normals[tris["prim_id"]] = va.face_normals(tris)
    sc = G.oracle_scene(oracle_mod, "comb%d" % depth, gen.prims, bvh.nodes, bvh.indices, normals, depth)
    ref = G.oracle_frame(oracle_mod, sc, G.oracle_camera(cam, G.W, G.H), kind, DEEP_SPEC, ml["materials"], ml["lights"])
    assert (ref["prim_id"] != G.MISS).any() and (ref["prim_id"] == G.MISS).any()
    G.assert_frame(got, ref, kind, 8, "comb%d" % depth)
    plain_dev = upload(ctx, bvh, tris)
    plain = G.render(ctx, plain_dev, cam, G.kernel(kind, plain_dev, sh, DEEP_SPEC))
    assert_same_frames({kind: plain}, {kind: got}, [kind])


@pytest.mark.parametrize("kind", G.KERNELS)
def test_comb_one_level_past_the_lds_depth_limit_is_refused(ctx, kind):
    depth = G.DEPTH_LIMIT[kind] + 1
    tris, bvh, gen, cam = comb(depth)
    dev = upload(ctx, gen, tris)
    assert dev.info["max_depth"] == depth
    sh = G.shading_of(ctx, G.fixture("gp_soup"))
    rt = va.hip_buffer_rt(ctx, G.W, G.H)
    mark = np.full((G.W * G.H, 4), 7.0, np.float32)
    rt.upload(color=mark, prim_id=np.full(G.W * G.H, 12345, np.uint32))
    with pytest.raises(va.VrhError) as e:
        va.render(ctx, dev, rt, cam, G.kernel(kind, dev, sh, DEEP_SPEC))
    assert e.value.code == _capi.VRH_ERR_UNSUPPORTED and "LDS" in str(e.value)
    ctx.sync()
    out = rt.download()
    assert G.same_bits(out["color"], mark) and (out["prim_id"] == 12345).all()


@pytest.mark.parametrize("where", ["outside", "inside"])
def test_sphere_normal_feeds_ao_and_shading_vs_oracle(ctx, oracle_mod, where):
    """One sphere of radius 0.7 and one triangle that pierces it, 33 x 17 pixels, all four kernels against the oracle.
    From outside the sphere's normal (isect_pos - center) / radius faces the viewer on every sphere hit.  From inside
    the sphere the reference's ray / sphere test (math/intersect.h:186-221) returns the nearer root, which lies behind
    the origin and is rejected (t < 0): no ray that starts inside meets the sphere, as in the fixture gp_inside, so an
    outward normal that faces away from the viewer cannot arise -- the camera inside sees the triangle through the
    sphere, and the assertion on the normal's side holds over the sphere hits there are (none)."""
    w, h = 33, 17
    tris = va.make_triangles([[-0.2, -0.2, 0.35]], [[1.3, 0.0, 0.0]], [[0.0, 1.3, 0.1]], prim_id=[0], geom_id=[1])
    sph = va.make_spheres([[0.0, 0.0, 0.0]], [0.7], prim_id=[1], geom_id=[2])
    gen = va.make_generic(tris, sph)
    bvh = va.build_index_bvh(gen)
    cam = va.camera()
    cam.perspective(0.9, np.float32(w) / np.float32(h), 0.001, 1000.0)
    if where == "outside":
        cam.look_at((1.9, 1.4, 2.3), (0.0, 0.0, 0.0))
    else:
        cam.look_at((0.1, 0.05, -0.3), (0.3, 0.3, 1.0))
    cam = cam.basis(w, h)
    ml = G.fixture("gp_soup")
    spec = dict(DEEP_SPEC, ao_radius=2.0, bounces=4)
    dev = upload(ctx, bvh, tris)
    sh = G.shading_of(ctx, ml)
    normals = np.zeros((2, 4), np.float32)
    normals[0] = va.face_normals(tris)[0]
    sc = G.oracle_scene(oracle_mod, "sphere_normal", gen, bvh.nodes, bvh.indices, normals, bvh.max_depth)
    ocam = G.oracle_camera(cam, w, h)
    ref = None
    for kind in G.KERNELS:
        frame = G.oracle_frame(oracle_mod, sc, ocam, kind, spec, ml["materials"], ml["lights"])
        G.assert_frame(G.render(ctx, dev, cam, G.kernel(kind, dev, sh, spec), w, h), frame, kind, 8, where)
        ref = frame if kind == "ao" else ref
    # the side of the sphere's normal, from the oracle's hits: n = (pos - center) / radius, view = -dir
    eye, cu, cv, cw = (np.float64(a) for a in ocam[:4])
    y, x = np.divmod(np.arange(w * h), w)
    d = cu[None] * (2.0 * (x + 0.5) / w - 1.0)[:, None] + cv[None] * (2.0 * (y + 0.5) / h - 1.0)[:, None] + cw[None]
    d /= np.linalg.norm(d, axis=1)[:, None]
    on_sphere = ref["prim_id"] == 1
    n = (eye[None] + d * np.float64(ref["t"])[:, None]) / 0.7
    facing = -(n * d).sum(axis=1)
    assert (ref["prim_id"] == 0).any()
    if where == "outside":
        assert on_sphere.sum() > 30 and (facing[on_sphere] > 0.0).all() and ref["occ"][ref["prim_id"] == 0].any()
    else:
        assert np.linalg.norm(eye) < 0.7 and not on_sphere.any() and (facing[on_sphere] < 0.0).all()


def test_tree_deeper_than_the_lds_stack_is_refused_and_leaves_the_target_untouched(ctx):
    """the generic instances keep the whole stack in LDS: a comb 699 deep needs 700 entries x 64 lanes x 4 bytes, more
    than a CU's 160 KiB, in every kernel"""
    tris, bvh = deep_cases.comb_bvh(700, deep_cases.PITCH)
    gen = va.index_bvh(va.make_generic(tris, None), bvh.nodes, bvh.indices, 699)
    dev = upload(ctx, gen, tris)
    assert dev.info["max_depth"] == 699
    cam = G.outside_camera()
    sh = G.shading_of(ctx, G.fixture("gp_soup"))
    s = dict(bg=(0.1, 0.2, 0.3, 1.0), ambient=(1.0, 1.0, 1.0, 1.0), ao_samples=8, ao_radius=0.3, ao_eps=1e-3, bounces=3, eps=1e-3)
    rt = va.hip_buffer_rt(ctx, G.W, G.H)
    mark = np.full((G.W * G.H, 4), 7.0, np.float32)
    rt.upload(color=mark, prim_id=np.full(G.W * G.H, 12345, np.uint32))
    for kind in G.KERNELS:
        with pytest.raises(va.VrhError) as e:
            va.render(ctx, dev, rt, cam, G.kernel(kind, dev, sh, s))
        assert e.value.code == _capi.VRH_ERR_UNSUPPORTED and "LDS" in str(e.value), kind
    ctx.sync()
    out = rt.download()
    assert G.same_bits(out["color"], mark) and (out["prim_id"] == 12345).all()


def test_bad_type_index_is_refused_at_upload(ctx):
    tris, sph = G.random_mixed(5, 6, 6)
    g = va.make_generic(tris, sph)
    bvh = va.build_index_bvh(g)
    bvh.prims = g.copy()
    bvh.prims["type"][3] = 3
    with pytest.raises(va.VrhError) as e:
        va.hip_index_bvh(ctx, bvh)
    assert e.value.code == _capi.VRH_ERR_INVALID


def test_unsupported_uses_are_refused_and_leave_the_target_untouched(ctx):
    tris, sph = G.random_mixed(21, 40, 40)
    g = va.make_generic(tris, sph, np.arange(80) % 2)
    dev = upload(ctx, va.build_index_bvh(g), tris)
    ml = G.fixture("gp_soup")
    sh = G.shading_of(ctx, ml)
    cam = G.outside_camera()
    rt = va.hip_buffer_rt(ctx, G.W, G.H)
    mark = np.full((G.W * G.H, 4), 7.0, np.float32)
    rt.upload(color=mark, prim_id=np.full(G.W * G.H, 12345, np.uint32))
    prim, ao = va.closest_hit_kernel(dev), va.ao_kernel(dev)
    simple = va.simple_kernel(dev, sh)

    def refused(call, *args, **kw):
        with pytest.raises(va.VrhError) as e:
            call(*args, **kw)
        assert e.value.code == _capi.VRH_ERR_UNSUPPORTED, str(e.value)
        assert "generic" in str(e.value)

    # frames in flight
    rt2 = va.hip_buffer_rt(ctx, G.W, 2 * G.H)
    refused(va.render_batch, ctx, dev, rt2, [cam, cam], prim)
    # BVH lists
    refused(va.hip_index_bvh.scene_list, ctx, [dev, dev])
    # pixel-sampler passes and camera matrices
    refused(va.render_sampled, ctx, dev, rt, cam, prim, va.pixel_sampler.jittered_type)
    # shards (render groups render shards)
    refused(va.render, ctx, dev, rt, cam, prim, shard=_capi.vrh_shard(0, 2, 0, 0))
    refused(va.render, ctx, dev, rt, cam, ao, shard=_capi.vrh_shard(0, 1, 1, 0))
    # multi_hit, the path tracer, textures, hit masks, test counting
    rt.alloc_multi_hit(4)
    refused(va.render, ctx, dev, rt, cam, va.multi_hit_kernel(dev, sh, max_hits=4, binding=va.normals_per_face_binding))
    refused(va.render, ctx, dev, rt, cam, va.pathtracing_kernel(dev, sh))
    refused(va.render, ctx, dev, rt, cam, va.pathtracing_kernel(dev, va.generic_shading(ctx, [va.matte()] * 4)))
    tsh = G.shading_of(ctx, ml)
    tex = va.texture(np.full((2, 2, 4), 255, np.uint8))
    tsh.set_textures(np.zeros((3 * 80, 2), np.float32), [tex] * len(tsh.materials))
    refused(va.render, ctx, dev, rt, cam, va.simple_kernel(dev, tsh))
    mask = va.hit_mask(ctx, np.zeros((3 * 80, 2), np.float32), np.ones((2, 2), np.uint8))
    refused(va.render, ctx, dev, rt, cam, va.with_hit_mask(va.closest_hit_kernel(dev), mask))
    refused(va.render, ctx, dev, rt, cam, va.closest_hit_kernel(dev, count_tests=True))
    refused(va.render, ctx, dev, rt, cam, va.ao_kernel(dev, count_tests=True))
    # per-vertex normals
    refused(dev.set_vertex_normals, np.zeros((3 * 80, 4), np.float32))
    refused(va.render, ctx, dev, rt, cam, va.simple_kernel(dev, sh, binding=va.normals_per_vertex_binding))
    # the LBVH build
    refused(va.hip_index_bvh.gpu_build, ctx, g)
    ctx.sync()
    out = rt.download()
    assert G.same_bits(out["color"], mark) and (out["prim_id"] == 12345).all()
    # and the supported kernels still render into it
    va.render(ctx, dev, rt, cam, simple)
    ctx.sync()
    assert (rt.download()["prim_id"] != 12345).all()
