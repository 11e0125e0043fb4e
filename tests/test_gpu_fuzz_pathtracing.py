"""GPU: randomized sweep and edge cases of the built-in path tracer against the oracle's path-tracing mode.

The oracle (oracle/vrh_oracle.c VO_MODE_PATHTRACING) is a second, independent statement of
pathtracing::kernel, pinned to the reference by tests/test_oracle_pathtracing.py.  The sweep's cases
and bars are those of tests/pt_cases.py: prim_id and t bit-identical everywhere; a case that cannot
reach powf has bit-identical colours and the oracle's ray total in all four render paths (one frame
per launch, three frames in flight, the jittered sampler, two jittered_blend frames onto a random
target); any other case keeps misses bit-identical and zero channels zero and has at least 99 % of
its hit pixels within rtol = 2 * sens, derived from the oracle alone.

Then the cases fixed frames cannot reach: every launch option on one closed-room case, a BVH of depth
89 (whole stack in LDS) and the host-side refusal of depth 999, GPU-built trees, tiny and partial
images, a path killed by pdf <= 0, and a seed that is 0 modulo the generator's modulus.

With num_bounces 0 the reference traces no ray; the kernel still traces the primary ray that fills
prim_id / t, so its ray count is one per pixel there.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import visionaray_amd as va
from visionaray_amd import _capi, scenes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pt_cases as P  # noqa: E402
from test_gpu_parity import comb_bvh  # noqa: E402
from test_oracle_pathtracing import room_case, wrapping_frames  # noqa: E402

pytestmark = pytest.mark.gpu
MISS = 0xFFFFFFFF
OPTION_CASE = 5           # a closed room that cannot reach powf, 10 bounces, 112 x 12, per-vertex normals


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def vrh_cam(ocam):
    eye, u, v, w, W, H = ocam
    F3 = C.c_float * 3
    return _capi.vrh_camera(F3(*eye), F3(*u), F3(*v), F3(*w), W, H)


def lights():
    lt = np.zeros(1, va.POINT_LIGHT_DTYPE)          # the path tracer is lit by the environment alone
    lt[0] = ((0.0, 2.0, 0.0), (1.0, 1.0, 1.0), 1.0, 1.0, 0.0, 0.0)
    return lt


def device_scene(ctx, O, prims, bvh=None):
    prims = np.ascontiguousarray(prims).view(va.TRIANGLE_DTYPE)
    fn = va.face_normals(prims)
    dev = va.hip_index_bvh(ctx, bvh if bvh is not None else va.build_index_bvh(prims), fn)
    dev.set_vertex_normals(O.vertex_normals(fn))
    return dev


def kernel_of(ctx, dev, materials, per_vertex, bg, ambient, num_bounces, eps):
    sh = va.shading(ctx, np.ascontiguousarray(materials).view(va.PLASTIC_DTYPE), lights())
    binding = va.normals_per_vertex_binding if per_vertex else va.normals_per_face_binding
    return va.pathtracing_kernel(dev, sh, binding=binding, bg=bg, ambient=ambient, num_bounces=num_bounces, epsilon=eps)


def setup_case(ctx, O, seed):
    case = P.draw_case(seed)
    dev = device_scene(ctx, O, case["prims"])
    k = kernel_of(ctx, dev, case["materials"], case["per_vertex"], case["bg"], case["ambient"], case["num_bounces"],
                  case["eps"])
    return case, dev, k, [c.basis(case["W"], case["H"]) for c in case["cams"]]


def expected_rays(case, ref):
    return ref["rays"] if case["num_bounces"] > 0 else case["W"] * case["H"]


def run_paths(ctx, O, seed, case, dev, k, bases, paths=("single", "flight", "jittered", "blend")):
    """renders the case's frames and applies the sweep's bar to each; returns the largest relative difference"""
    W, H, fn, free = case["W"], case["H"], case["frame_num"], case["powf_free"]
    worst = 0.0
    if "single" in paths:
        rt = va.hip_buffer_rt(ctx, W, H)
        va.render(ctx, dev, rt, bases[0], k, frame_num=fn)
        ref, tol = P.reference(O, seed, "single")
        worst = max(worst, P.check_frame(rt.download(), ref, tol, free, f"seed {seed} single"))
        if free:
            assert ctx.last_frame_stats()["rays"] == expected_rays(case, ref)
    if "flight" in paths:
        rt = va.hip_buffer_rt(ctx, W, 3 * H)
        va.render_batch(ctx, dev, rt, bases, k, frame_num=fn)
        got, rays, n = rt.download(), 0, W * H
        for f in range(3):
            ref, tol = P.reference(O, seed, "flight%d" % f)
            part = {key: got[key][f * n:(f + 1) * n] for key in ("prim_id", "t", "color")}
            worst = max(worst, P.check_frame(part, ref, tol, free, f"seed {seed} flight {f}"))
            rays += expected_rays(case, ref)
        if free:
            assert ctx.last_frame_stats()["rays"] == rays
    if "jittered" in paths:
        rt = va.hip_buffer_rt(ctx, W, H)
        rt.upload(color=case["init"])
        va.render_sampled(ctx, dev, rt, bases[0], k, va.pixel_sampler.jittered_type, frame_num=fn)
        ref, tol = P.reference(O, seed, "jittered")
        worst = max(worst, P.check_frame(rt.download(), ref, tol, free, f"seed {seed} jittered"))
        if free:
            assert ctx.last_frame_stats()["rays"] == expected_rays(case, ref)
    if "blend" in paths:
        rt = va.hip_buffer_rt(ctx, W, H)
        rt.upload(color=case["init"])
        ref, tol = P.reference(O, seed, "blend")
        for n, want in ((case["blend_first"], ref["rays_first"]), (case["blend_first"] + 1, ref["rays"])):
            va.render_sampled(ctx, dev, rt, bases[0], k, va.pixel_sampler.jittered_blend_type, frame_num=n)
            if free:
                assert ctx.last_frame_stats()["rays"] == (want if case["num_bounces"] > 0 else W * H)
        worst = max(worst, P.check_frame(rt.download(), ref, tol, free, f"seed {seed} blend"))
    return worst


@pytest.mark.parametrize("seed", P.SEEDS)
def test_random_cases_vs_oracle(ctx, oracle_mod, seed):
    case, dev, k, bases = setup_case(ctx, oracle_mod, seed)
    worst = run_paths(ctx, oracle_mod, seed, case, dev, k, bases)
    if not case["powf_free"]:
        print(f"seed {seed}: largest relative difference over all frames {worst:.3e}")


# ---- launch options: "Results never depend on these" (vrh.h) -------------------------------------------

OPTIONS = {
    "block64": {"block_threads": 64}, "block128": {"block_threads": 128}, "block256": {"block_threads": 256},
    "occ1": {"waves_per_simd": 1}, "occ5": {"waves_per_simd": 5}, "occ8": {"waves_per_simd": 8},
    "blocks_per_cu1": {"blocks_per_cu": 1},
    "queues2": {"xcd_queues": 2}, "queues3": {"xcd_queues": 3}, "queues4": {"xcd_queues": 4, "cluster_tiles": 5},
    "descent_cap1": {"descent_cap": 1}, "pop_on_miss2": {"pop_on_miss": 2}, "scalar_fetch2": {"scalar_fetch": 2},
    "exact_minmax1": {"exact_minmax": 1}, "stack_cap4": {"stack_cap": 4}, "stack_cap8": {"stack_cap": 8},
    "pair_layout1": {"pair_layout": 1},           # read when a scene is uploaded: the case uploads after setting it
}


@pytest.mark.parametrize("name", sorted(OPTIONS))
def test_launch_options_do_not_change_the_frames(ctx, oracle_mod, name):
    """one frame, frames in flight and a sampler pass of a closed-room case under each launch option"""
    try:
        for key, v in OPTIONS[name].items():
            ctx.set_option(key, v)
        case, dev, k, bases = setup_case(ctx, oracle_mod, OPTION_CASE)
        assert case["powf_free"] and case["family"] == "room" and case["num_bounces"] >= 10
        ref, _ = P.reference(oracle_mod, OPTION_CASE, "single")
        assert int(ref["nrays"].max()) == case["num_bounces"]        # paths run to num_bounces
        run_paths(ctx, oracle_mod, OPTION_CASE, case, dev, k, bases, paths=("single", "flight", "jittered"))
    finally:
        for key in OPTIONS[name]:
            ctx.set_option(key, 0)


# ---- deep trees ------------------------------------------------------------------------------------------

def comb_setup(ctx, O, n):
    tris, bvh = comb_bvh(n)
    dev = device_scene(ctx, O, tris, bvh)
    m, _, _, bg = O.whitted_spec()
    m = m.copy()
    m["ks"] = 0.0
    k = kernel_of(ctx, dev, m, False, bg, (0.6, 1.1, 0.3, 0.8), 6, 1e-3)
    fn = va.face_normals(tris)
    osc = O.Scene("comb%d" % n, O.VO_TRI, tris.view(O.TRI_DTYPE), bvh.nodes.view(O.NODE_DTYPE), bvh.indices, fn,
                  bvh.max_depth, O.vertex_normals(fn))
    W, H = 64, 8
    cam = va.camera()
    cam.perspective(1.0, np.float32(W) / np.float32(H), 0.001, 1000.0)
    # from between the teeth 87 and 88 back along the comb: every level's leaf lies behind its sibling, so the
    # stack grows to the tree's depth before tooth 87 is found, and bounces go back and forth between teeth
    cam.look_at((43.75, 0.1, 0.1), (0.0, 0.12, 0.11), (0.0, 1.0, 0.0))
    basis = cam.basis(W, H)
    return dev, k, osc, m, bg, basis, P._ocam(basis, W, H)


def comb_check(ctx, O, dev, k, osc, m, bg, basis, ocam):
    W, H = ocam[4], ocam[5]
    ref = O.render_pathtracing(osc, ocam, O.VO_NORMALS_PER_FACE, m, (0.6, 1.1, 0.3, 0.8), bg, 6, 1e-3, frame_num=11)
    assert int(ref["nrays"].max()) >= 3 and (ref["prim_id"] != MISS).any()
    rt = va.hip_buffer_rt(ctx, W, H)
    va.render(ctx, dev, rt, basis, k, frame_num=11)
    P.check_frame(rt.download(), ref, None, True, "comb")
    assert ctx.last_frame_stats()["rays"] == ref["rays"]


def test_deep_tree_whole_stack_in_lds_and_refusal(ctx, oracle_mod):
    O = oracle_mod
    deep = comb_setup(ctx, O, 90)
    assert deep[0].info["max_depth"] == 89
    comb_check(ctx, O, *deep)
    # depth 999: more LDS stack than a CU has, and this kernel has no overflow-stack instance.  Refused on
    # the host before any launch.
    dev, k, _, _, _, basis, ocam = comb_setup(ctx, O, 1000)
    rt = va.hip_buffer_rt(ctx, ocam[4], ocam[5])
    with pytest.raises(va.VrhError) as e:
        va.render(ctx, dev, rt, basis, k, frame_num=11)
    assert e.value.code == _capi.VRH_ERR_UNSUPPORTED, str(e.value)
    assert _capi.lib().vrh_last_error().decode() != ""
    comb_check(ctx, O, *deep)                    # the context still renders


# ---- GPU-built trees ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["hf64", "soup"])
def test_gpu_built_scene(ctx, oracle_mod, name):
    O = oracle_mod
    if name == "soup":
        prims = np.ascontiguousarray(P.draw_case(0)["prims"]).copy()
    else:
        prims = scenes.primitives(name).copy()
    prims["geom_id"] = np.arange(len(prims), dtype=np.uint32) % 3
    fn = va.face_normals(prims)
    dev = va.hip_index_bvh.gpu_build(ctx, prims, fn)
    assert dev.info["gpu_built"] == 1
    dev.set_vertex_normals(O.vertex_normals(fn))
    nodes, idx = dev.download_bvh()
    m, _, _, bg = O.whitted_spec()
    m = m.copy()
    m["ks"] = 0.0
    W, H = 60, 44
    k = kernel_of(ctx, dev, m, True, bg, (0.9, 0.8, 1.2, 1.0), 5, 1e-3)
    osc = O.Scene(name, O.VO_TRI, prims.view(O.TRI_DTYPE), nodes.view(O.NODE_DTYPE), idx, fn, dev.info["max_depth"],
                  O.vertex_normals(fn))
    ocam = O.scene_camera("hf64", W, H)
    ref = O.render_pathtracing(osc, ocam, O.VO_NORMALS_PER_VERTEX, m, (0.9, 0.8, 1.2, 1.0), bg, 5, 1e-3, frame_num=2)
    assert (ref["prim_id"] != MISS).any() and int(ref["nrays"].max()) >= 3
    rt = va.hip_buffer_rt(ctx, W, H)
    va.render(ctx, dev, rt, vrh_cam(ocam), k, frame_num=2)
    P.check_frame(rt.download(), ref, None, True, name)
    assert ctx.last_frame_stats()["rays"] == ref["rays"]


# ---- small and partial images ------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", [(1, 1), (8, 8), (9, 1)])
def test_small_images(ctx, oracle_mod, W, H):
    O = oracle_mod
    sc, ocam, m, bg = room_case(O, W, H)
    dev = device_scene(ctx, O, sc.prims)
    amb = (0.7, 1.3, 0.2, 0.9)
    k = kernel_of(ctx, dev, m, True, bg, amb, 5, 1e-3)
    fn = 0xFFFFFFF0                                   # frame_num * W * H wraps but for 1 x 1
    for sampler, stype in ((None, None), ("jittered", va.pixel_sampler.jittered_type)):
        ref = O.render_pathtracing(sc, ocam, O.VO_NORMALS_PER_VERTEX, m, amb, bg, 5, 1e-3, frame_num=fn, sampler=sampler)
        assert (ref["prim_id"] != MISS).any()
        rt = va.hip_buffer_rt(ctx, W, H)
        if stype is None:
            va.render(ctx, dev, rt, vrh_cam(ocam), k, frame_num=fn)
        else:
            va.render_sampled(ctx, dev, rt, vrh_cam(ocam), k, stype, frame_num=fn)
        P.check_frame(rt.download(), ref, None, True, f"{W}x{H} {sampler}")
        assert ctx.last_frame_stats()["rays"] == ref["rays"]


def test_scissor_box_with_the_jittered_sampler(ctx, oracle_mod):
    O = oracle_mod
    W, H, box = 60, 44, (5, 3, 43, 30)
    sc, ocam, m, bg = room_case(O, W, H)
    dev = device_scene(ctx, O, sc.prims)
    amb = (0.7, 1.3, 0.2, 0.9)
    k = kernel_of(ctx, dev, m, False, bg, amb, 5, 1e-3)
    args = (sc, ocam, O.VO_NORMALS_PER_FACE, m, amb, bg, 5, 1e-3)
    fill = (0.25, 0.5, 0.75, 0.125)
    whole = O.render_pathtracing(*args, frame_num=9, sampler="jittered")
    ref = O.render_pathtracing(*args, frame_num=9, sampler="jittered", scissor=box, init=fill)
    cam = vrh_cam(ocam)
    cam.scissor[:] = list(box)
    rt = va.hip_buffer_rt(ctx, W, H)
    rt.clear_color_buffer(fill)
    va.render_sampled(ctx, dev, rt, cam, k, va.pixel_sampler.jittered_type, frame_num=9)
    got = rt.download()
    y, x = np.arange(W * H) // W, np.arange(W * H) % W
    inside = (x >= box[0]) & (x < box[2]) & (y >= box[1]) & (y < box[3])
    assert np.array_equal(bits(got["color"][inside]), bits(whole["color"][inside]))
    assert np.array_equal(got["color"][~inside], np.tile(np.float32(fill), (int((~inside).sum()), 1)))
    assert np.array_equal(bits(got["color"]), bits(ref["color"]))
    assert np.array_equal(got["prim_id"][inside], ref["prim_id"][inside]) and np.all(got["prim_id"][~inside] == MISS)
    assert ctx.last_frame_stats()["rays"] == ref["rays"]


# ---- branches of the bounce ----------------------------------------------------------------------------------

def test_paths_killed_by_a_non_positive_pdf(ctx, oracle_mod):
    """a purely specular material of exponent 0: many half vectors face away from the viewer (pdf <= 0), and
    pow(x, 0) = 1 exactly, so which paths die and how many rays are traced does not depend on powf"""
    O = oracle_mod
    W, H = 40, 30
    sc, ocam, m, bg = room_case(O, W, H, specular_exp=0.0)
    dev = device_scene(ctx, O, sc.prims)
    k = kernel_of(ctx, dev, m, False, bg, (1.0, 1.0, 1.0, 1.0), 2, 1e-3)
    ref = O.render_pathtracing(sc, ocam, O.VO_NORMALS_PER_FACE, m, (1.0, 1.0, 1.0, 1.0), bg, 2, 1e-3, frame_num=4)
    died = (ref["prim_id"] != MISS) & (ref["nrays"] == 1)
    assert died.any() and ((ref["prim_id"] != MISS) & (ref["nrays"] == 2)).any()
    rt = va.hip_buffer_rt(ctx, W, H)
    va.render(ctx, dev, rt, vrh_cam(ocam), k, frame_num=4)
    got = rt.download()
    assert np.array_equal(got["prim_id"], ref["prim_id"]) and np.array_equal(bits(got["t"]), bits(ref["t"]))
    assert np.array_equal(got["color"][died], np.tile(np.float32([0, 0, 0, 1]), (int(died.sum()), 1)))
    # with two bounces every path's first sample decides alone whether a second ray is traced
    assert ctx.last_frame_stats()["rays"] == ref["rays"]


def test_seed_zero_modulo_the_modulus_and_a_wrapping_frame_number(ctx, oracle_mod):
    O = oracle_mod
    W, H = 9, 7
    sc, ocam, m, bg = room_case(O, W, H)
    p = 3 * W + 4
    dev = device_scene(ctx, O, sc.prims)
    amb = (0.7, 1.3, 0.2, 0.9)
    k = kernel_of(ctx, dev, m, False, bg, amb, 6, 1e-3)
    frames = []
    for n in wrapping_frames(W, H, p):
        ref = O.render_pathtracing(sc, ocam, O.VO_NORMALS_PER_FACE, m, amb, bg, 6, 1e-3, frame_num=n)
        rt = va.hip_buffer_rt(ctx, W, H)
        va.render(ctx, dev, rt, vrh_cam(ocam), k, frame_num=n)
        frames.append(rt.download())
        P.check_frame(frames[-1], ref, None, True, f"frame {n}")
        assert ctx.last_frame_stats()["rays"] == ref["rays"]
    assert frames[0]["color"][p, :3].any()
    assert np.array_equal(bits(frames[0]["color"][p]), bits(frames[1]["color"][p]))
