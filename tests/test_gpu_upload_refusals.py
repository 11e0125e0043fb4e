"""GPU: malformed trees are refused at vrh_scene_upload, on the host (vrh_upload.cpp prepare_scene) before any device
call is made, and the context uploads and renders a valid tree afterwards -- under both pair layouts, which reach
prepare_scene as options of the context.  Face normals whose rows a prim_id would overrun are refused the same way by
vrh_scene_upload and vrh_scene_build."""
import numpy as np
import pytest

import visionaray_amd as va
from visionaray_amd import _capi, scenes

pytestmark = pytest.mark.gpu


def _malformed(b):
    """(name, index_bvh, part of the message) of three malformed copies of the host BVH b"""
    inner = np.flatnonzero(b.nodes["num_prims"] == 0)
    leaves = np.flatnonzero(b.nodes["num_prims"] != 0)
    cycle = b.nodes.copy()
    cycle["first"][inner[-1]] = 1                      # a deep inner node points back at the root's pair
    past = b.nodes.copy()
    past["num_prims"][leaves[0]] += len(b.indices)
    return [("cycle", va.index_bvh(b.prims, cycle, b.indices, b.max_depth), "not a tree"),
            ("even node count", va.index_bvh(b.prims, b.nodes[:-1].copy(), b.indices, b.max_depth), "node count must be odd"),
            ("leaf range past the indices", va.index_bvh(b.prims, past, b.indices, b.max_depth), "malformed node pair")]


@pytest.mark.parametrize("layout", [1, 2])
def test_refusals_then_a_valid_upload_renders(ctx, oracle_mod, layout):
    O = oracle_mod
    name, W, H = "hf64", 64, 32
    prims = scenes.primitives(name)
    b = va.build_index_bvh(prims)
    ctx.set_option("pair_layout", layout)
    try:
        for what, bad, text in _malformed(b):
            with pytest.raises(va.VrhError) as e:
                va.hip_index_bvh(ctx, bad, scenes.normals_for(prims))
            assert e.value.code == _capi.VRH_ERR_INVALID, what
            assert text in str(e.value), what
        dev = va.hip_index_bvh(ctx, b, scenes.normals_for(prims))
    finally:
        ctx.set_option("pair_layout", 0)
    cam, _, _ = scenes.scene_camera(name, W, H)
    rt = va.hip_buffer_rt(ctx, W, H)
    va.hip_sched(ctx).frame(va.ao_kernel(dev), va.make_sched_params(va.pixel_sampler.uniform_type, cam, rt))
    got = rt.download()
    rt.close()
    dev.close()
    ref = O.render(O.make_scene(name), O.scene_camera(name, W, H), mode=O.VO_MODE_AO)
    assert (ref["prim_id"] != 0xFFFFFFFF).any() and ref["occ"].any()
    assert np.array_equal(got["prim_id"], ref["prim_id"])
    assert np.array_equal(got["t"].view(np.uint32), ref["t"].view(np.uint32))
    assert np.array_equal(got["occ"], ref["occ"].astype(np.uint8))


def _primary(ctx, dev, cam, W, H):
    rt = va.hip_buffer_rt(ctx, W, H)
    va.hip_sched(ctx).frame(va.closest_hit_kernel(dev), va.make_sched_params(cam, rt))
    got = rt.download()
    rt.close()
    return got


def test_face_normals_need_prim_ids_below_num_prims(ctx, oracle_mod):
    """Face normals are num_prims rows read as normals[prim_id]: vrh_scene_upload and vrh_scene_build refuse them, on
    the host, when a prim_id is not below num_prims; the same primitives without normals upload / build and render
    primary visibility; download_bvh is for GPU-built scenes only; and the context renders a valid AO scene after."""
    O = oracle_mod
    name, W, H = "hf64", 64, 32
    good = scenes.primitives(name)
    n = len(good)
    cam, _, _ = scenes.scene_camera(name, W, H)
    ocam = O.scene_camera(name, W, H)
    seen = O.render(O.make_scene(name), ocam, mode=O.VO_MODE_PRIMARY)["prim_id"]
    prims = good.copy()
    # the triangle that covers the most pixels gets an id past the normals; the geometry is unchanged
    prims["prim_id"][np.bincount(seen[seen != 0xFFFFFFFF]).argmax()] = n + 5
    nrm = scenes.normals_for(good)
    b = va.build_index_bvh(prims)

    with pytest.raises(va.VrhError) as e:
        va.hip_index_bvh(ctx, b, nrm)
    assert e.value.code == _capi.VRH_ERR_INVALID and f"prim_id {n + 5}" in str(e.value) and "vrh_scene_upload" in str(e.value)
    up = va.hip_index_bvh(ctx, b)
    assert up.info["max_prim_id"] == n + 5
    ref = O.render(O.Scene(name, O.VO_TRI, prims, b.nodes, b.indices, None, b.max_depth), ocam, mode=O.VO_MODE_PRIMARY)
    assert (ref["prim_id"] == n + 5).any()
    got = _primary(ctx, up, cam, W, H)
    assert np.array_equal(got["prim_id"], ref["prim_id"])
    assert np.array_equal(got["t"].view(np.uint32), ref["t"].view(np.uint32))
    with pytest.raises(va.VrhError) as e:
        up.download_bvh()
    assert e.value.code == _capi.VRH_ERR_UNSUPPORTED and "GPU-built" in str(e.value)
    up.close()

    for _ in range(3):
        with pytest.raises(va.VrhError) as e:
            va.hip_index_bvh.gpu_build(ctx, prims, nrm)
        assert e.value.code == _capi.VRH_ERR_INVALID and f"prim_id {n + 5}" in str(e.value) and "vrh_scene_build" in str(e.value)
    built = va.hip_index_bvh.gpu_build(ctx, prims)
    assert built.info["max_prim_id"] == n + 5
    nodes, idx = built.download_bvh()
    ref = O.render(O.Scene(name, O.VO_TRI, prims, nodes.view(O.NODE_DTYPE), idx, None, built.info["max_depth"]), ocam,
                   mode=O.VO_MODE_PRIMARY)
    got = _primary(ctx, built, cam, W, H)
    assert (ref["prim_id"] == n + 5).any()
    assert np.array_equal(got["prim_id"], ref["prim_id"])
    assert np.array_equal(got["t"].view(np.uint32), ref["t"].view(np.uint32))
    built.close()

    dev = va.hip_index_bvh.gpu_build(ctx, good, nrm)
    nodes, idx = dev.download_bvh()
    rt = va.hip_buffer_rt(ctx, W, H)
    va.hip_sched(ctx).frame(va.ao_kernel(dev), va.make_sched_params(cam, rt))
    got = rt.download()
    rt.close()
    ref = O.render(O.Scene(name, O.VO_TRI, good, nodes.view(O.NODE_DTYPE), idx, nrm, dev.info["max_depth"]), ocam,
                   mode=O.VO_MODE_AO)
    dev.close()
    assert (ref["prim_id"] != 0xFFFFFFFF).any() and ref["occ"].any()
    assert np.array_equal(got["prim_id"], ref["prim_id"])
    assert np.array_equal(got["t"].view(np.uint32), ref["t"].view(np.uint32))
    assert np.array_equal(got["occ"], ref["occ"].astype(np.uint8))
