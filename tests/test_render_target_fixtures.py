"""CPU: the host build of the formatted render targets' resolve pass (vrh_rt_resolve_host, the text of
include/visionaray_hip/detail/vrh_pixel.h that the resolve kernel compiles too) against the reference.

rt_pixels.npz holds the reference's pixel_access::store / blend / depth_transform / clear_* on a sequence of steps,
rt_frame.npz a whole simple_sched frame with camera matrices (tests/golden/make_render_target_golden.py).  Every
comparison is bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

import visionaray_amd as va

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import rt_cases as RC  # noqa: E402


def u8(*hexes):
    return np.frombuffer(bytes.fromhex("".join(hexes)), np.uint8)


def test_known_answers_of_the_reference():
    """what the reference stores for (0.3, 1.7, -0.2, 0.5), its depth words, and its unit test's RGB32F answer
    (test/unittests/render_target.cpp: 0.4 stored with alpha 0.4 reads 0.16)"""
    c = np.float32([[0.3, 1.7, -0.2, 0.5]])
    d = va.resolve_desc()
    assert np.array_equal(va.rt_resolve_host(RC.CF.rgba8, RC.DF.none, 1, 1, c, d)["color"].reshape(-1), u8("4cff007f"))
    assert np.array_equal(va.rt_resolve_host(RC.CF.rgb8, RC.DF.none, 1, 1, c, d)["color"].reshape(-1), u8("26d800"))
    got = va.rt_resolve_host(RC.CF.rgb32f, RC.DF.none, 1, 1, c, d)["color"]
    assert np.array_equal(got[0, :3].view(np.uint32), np.float32([0.15, 0.85, -0.1]).view(np.uint32))
    assert got[0, 3] == 0.0
    assert np.array_equal(va.rt_resolve_host(RC.CF.rgba32f, RC.DF.none, 1, 1, c, d)["color"].view(np.uint32), c.view(np.uint32))
    got = va.rt_resolve_host(RC.CF.rgb32f, RC.DF.none, 1, 1, np.float32([[0.4, 0.4, 0.4, 0.4]]), d)["color"]
    assert np.array_equal(got[0, :3], np.float32([0.4, 0.4, 0.4]) * np.float32(0.4))
    assert abs(float(got[0, 0]) - 0.16) < 1e-7
    # depth: a miss stores 1.0 = ffffff00; the depth 0x3f77b6e2 stores f7b6e100 (identity camera: depth = t / 2)
    ident = RC.step_desc(0)
    miss = va.rt_resolve_host(RC.CF.rgba8, RC.DF.depth24_stencil8, 1, 1, c, ident, prim_id=np.uint32([RC.MISS]), t=np.float32([-1]))
    assert miss["depth"][0] == 0xFFFFFF00
    depth = np.uint32([0x3F77B6E2]).view(np.float32)
    hit = va.rt_resolve_host(RC.CF.rgba8, RC.DF.depth24_stencil8, 1, 1, c, ident, prim_id=np.uint32([7]), t=depth * np.float32(2))
    assert hit["depth"][0] == 0xF7B6E100
    hit = va.rt_resolve_host(RC.CF.rgba8, RC.DF.depth32f, 1, 1, c, ident, prim_id=np.uint32([7]), t=depth * np.float32(2))
    assert hit["depth"].view(np.uint32)[0] == 0x3F77B6E2


def test_unorm_get_is_the_references():
    """blend with s = 0, d = 1 stores what get read: u -> float(double(float(u)) / 255.0) -> u again for every byte"""
    n = 256
    buf = np.stack([np.arange(n, dtype=np.uint8)] * 4, axis=1)
    zero = np.zeros((n, 4), np.float32)
    d = va.resolve_desc(blend=True, s=0.0, d=1.0)
    got = va.rt_resolve_host(RC.CF.rgba8, RC.DF.none, n, 1, zero, d, color_out=buf)["color"]
    assert np.array_equal(got, buf)
    # RGB formats read alpha 1: the stored rgb is the read rgb times (0 * 0 + 1 * 1)
    got = va.rt_resolve_host(RC.CF.rgb8, RC.DF.none, n, 1, zero, d, color_out=buf[:, :3])["color"]
    assert np.array_equal(got, buf[:, :3])


@pytest.mark.parametrize("df_name", list(RC.DEPTH_FORMATS))
@pytest.mark.parametrize("cf_name", list(RC.COLOR_FORMATS))
def test_pixel_pipeline_matches_reference_step_by_step(cf_name, df_name):
    fx = RC.pixels_fixture()
    cf, df = RC.COLOR_FORMATS[cf_name], RC.DEPTH_FORMATS[df_name]
    n = fx["in_color"].shape[1]
    # the clears: a constant frame that misses everywhere stores the clear colour and depth 1.0
    assert float(fx["clear_depth"][0]) == 1.0
    clear = np.tile(fx["clear_color"], (n, 1))
    state = va.rt_resolve_host(cf, df, n, 1, clear, RC.step_desc(0), prim_id=np.full(n, RC.MISS, np.uint32), t=np.full(n, -1, np.float32))
    assert RC.same(state, RC.expected(0, cf_name, df_name, n), cf_name, df_name), "clear"
    for step in range(len(fx["steps"])):
        color, prim_id, t = RC.step_inputs(step, n)
        state = va.rt_resolve_host(cf, df, n, 1, color, RC.step_desc(step), prim_id=prim_id, t=t, color_out=state["color"],
                                   depth_out=state.get("depth"))
        assert RC.same(state, RC.expected(step + 1, cf_name, df_name, n), cf_name, df_name), f"step {step}"


@pytest.mark.parametrize("df_name", ["depth32f", "depth24s8"])
def test_depth_taken_from_the_staging_t_buffer(df_name):
    """matrix_cam 0 (a user kernel's launch leaves result.depth in t): the fixture's depths, given as they are, go
    through the same store and blend as the depths the matrix camera's ray gives"""
    fx = RC.pixels_fixture()
    df = RC.DEPTH_FORMATS[df_name]
    n = fx["in_color"].shape[1]
    state = RC.expected(0, "rgba8", df_name, n)
    for step in range(len(fx["steps"])):
        color, prim_id, t = RC.step_inputs(step, n)
        one = np.float32(1.0)
        depth = np.where(prim_id != RC.MISS, ((t - one) + one) * np.float32(0.5), one).astype(np.float32)    # depth_transform of (., ., t - 1)
        state = va.rt_resolve_host(RC.CF.rgba8, df, n, 1, color, RC.step_desc(step, depth=False), t=depth, color_out=state["color"],
                                   depth_out=state["depth"].view(np.float32 if df_name == "depth32f" else np.uint32))
        assert RC.same(state, RC.expected(step + 1, "rgba8", df_name, n), "rgba8", df_name), f"step {step}"


@pytest.mark.parametrize("jitter", [False, True])
def test_depth_against_doubles(jitter):
    """the twin's depth -- its own matrix_ray and jitter draws -- against a recomputation in numpy doubles from what
    include/vrh.h documents; with the jittered sampler the pixel centre's ray does not pass"""
    fx = RC.frame_fixture()
    w, h = 61, 45
    view, proj = fx["view"].reshape(4, 4).T, fx["proj"].reshape(4, 4).T
    rng = np.random.default_rng(9)
    t = rng.uniform(2.0, 4.5, w * h).astype(np.float32)
    prim_id = np.where(rng.random(w * h) < 0.8, 5, RC.MISS).astype(np.uint32)
    d = va.resolve_desc(view=fx["view"], proj=fx["proj"], jitter=jitter, frame_num=11)
    got = va.rt_resolve_host(RC.CF.rgba8, RC.DF.depth32f, w, h, np.zeros((w * h, 4), np.float32), d, prim_id=prim_id, t=t)["depth"]
    want = RC.depth_in_doubles(view, proj, w, h, prim_id, t, jitter=jitter, frame_num=11)
    assert np.max(np.abs(got - want)) <= RC.DEPTH_ATOL
    if jitter:
        centre = RC.depth_in_doubles(view, proj, w, h, prim_id, t)
        assert np.mean(np.abs(got - centre)[prim_id != RC.MISS] > RC.DEPTH_ATOL) > 0.25


def test_whole_frame_matches_reference(oracle_mod):
    """the reference's simple_sched frame with camera matrices: prim_id / t from the oracle's matrix camera, the
    colour the generator's function of prim_id, resolved by the twin with the twin's own ray"""
    O = oracle_mod
    fx = RC.frame_fixture()
    W, H = (int(x) for x in fx["size"])
    prims = np.ascontiguousarray(fx["prims"]).view(va.TRIANGLE_DTYPE).reshape(-1)
    nodes, idx, depth = O.build_bvh(prims, O.VO_TRI)
    sc = O.Scene("rt_frame", O.VO_TRI, prims, nodes, idx, O.face_normals(prims), depth)
    cam = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, -1), W, H)
    out = O.render_sampled(sc, cam, "uniform", mode=O.VO_MODE_PRIMARY, matrices=(fx["view"], fx["proj"]))
    assert np.array_equal(out["prim_id"], fx["prim_id"])
    assert np.array_equal(out["t"].view(np.uint32), fx["t"])
    d = va.resolve_desc(view=fx["view"], proj=fx["proj"])
    color = RC.prim_color(out["prim_id"])
    a = va.rt_resolve_host(RC.CF.rgba8, RC.DF.depth24_stencil8, W, H, color, d, prim_id=out["prim_id"], t=out["t"])
    assert np.array_equal(a["color"], fx["rgba8"]) and np.array_equal(a["depth"], fx["depth24s8"])
    b = va.rt_resolve_host(RC.CF.rgb8, RC.DF.depth32f, W, H, color, d, prim_id=out["prim_id"], t=out["t"])
    assert np.array_equal(b["color"], fx["rgb8"]) and np.array_equal(b["depth"].view(np.uint32), fx["depth32f"])


def test_scissor_box_leaves_the_rest_untouched():
    W, H = 7, 5
    rng = np.random.default_rng(3)
    color = rng.uniform(0, 1, (W * H, 4)).astype(np.float32)
    before = rng.integers(0, 256, (W * H, 4)).astype(np.uint8)
    full = va.rt_resolve_host(RC.CF.rgba8, RC.DF.none, W, H, color, va.resolve_desc())["color"]
    for box in [(1, 1, 4, 3), (3, 0, 4, 5), (2, 2, 2, 2), (5, 4, 99, 99)]:
        got = va.rt_resolve_host(RC.CF.rgba8, RC.DF.none, W, H, color, va.resolve_desc(scissor=box), color_out=before)["color"]
        x0, y0, x1, y1 = box[0], box[1], min(box[2], W), min(box[3], H)
        inside = np.zeros((H, W), bool)
        inside[y0:y1, x0:x1] = True
        inside = inside.reshape(-1)
        assert np.array_equal(got[inside], full[inside]) and np.array_equal(got[~inside], before[~inside])


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_pixel_edge_check_program(flags, tmp_path):
    """tests/cpp/pixel_edge_check.cpp: a stand-alone program over the shared header -- NaN / inf / huge colours and
    depths, w = 0 in the depth transform, 1 x 1 images, empty boxes -- plain and under the address and
    undefined-behaviour sanitizers"""
    exe = str(tmp_path / "pixel_edge_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "include"),
                    os.path.join(HERE, "cpp", "pixel_edge_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pixel_edge_check ok" in r.stdout
