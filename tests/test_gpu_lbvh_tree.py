"""GPU: vrh_scene_build against its CPU reference (tests/lbvh_ref.py), on the edge cases of tests/lbvh_cases.py.

Tree: gpu_build + download_bvh must give the reference's tree -- the index array, every first and num_prims bit
for bit, every box as a float value (signed zeros compare equal) -- and the scene info its node count, max_depth
(which sizes the traversal's per-lane stack), id maxima and index count.
Frame: one frame over the built scene (AO with per-face normals for triangles, primary visibility for spheres)
must equal the oracle traversing the downloaded tree, bit for bit.  The permuted case also renders simple::kernel
with per-face normals, where a mix-up of a primitive's index and its prim_id shows as a wrong normal.
List: two GPU-built scenes in one scene list, one of them a single-leaf root (the re-based LEAF|0 root).
"""
import os
import sys
from functools import lru_cache

import numpy as np
import pytest

import visionaray_amd as va

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lbvh_cases as LC  # noqa: E402
import lbvh_ref as LR  # noqa: E402

pytestmark = pytest.mark.gpu


@lru_cache(maxsize=None)
def _reference(name, max_leaf):
    return LR.lbvh_reference(LC.BY_NAME[name].prims, max_leaf)


def _build(ctx, prims, max_leaf, normals=True):
    nrm = LC.normals_by_id(prims) if normals and prims.dtype == va.TRIANGLE_DTYPE else None
    return va.hip_index_bvh.gpu_build(ctx, prims, nrm, max_leaf=max_leaf)


def _same_frame(got, ref):
    for k in ("prim_id", "occ"):
        assert np.array_equal(got[k], ref[k]), f"{k}: {int((got[k] != ref[k]).sum())} pixels differ"
    for k in ("t", "color"):
        a, b = got[k].view(np.uint32), ref[k].view(np.uint32)
        assert np.array_equal(a, b), f"{k}: {int((a != b).any(axis=-1).sum() if a.ndim > 1 else (a != b).sum())} pixels differ"


def _frame(ctx, case, scene):
    W, H = case.size
    kern = va.ao_kernel(scene, radius=case.radius, eps=case.eps) if case.ao else va.closest_hit_kernel(scene)
    rt = va.hip_buffer_rt(ctx, W, H)
    va.hip_sched(ctx).frame(kern, va.make_sched_params(case.camera(), rt))
    got = rt.download()
    rt.close()
    return got


@pytest.mark.parametrize("name,max_leaf", LC.PARAMS)
def test_built_tree_equals_the_reference(ctx, name, max_leaf):
    prims = LC.BY_NAME[name].prims
    ref = _reference(name, max_leaf)
    dev = _build(ctx, prims, max_leaf)
    nodes, idx = dev.download_bvh()
    info = dict(dev.info)
    dev.close()
    assert idx.dtype == np.uint32 and idx.tobytes() == ref.indices.tobytes()
    assert len(nodes) == len(ref.nodes)
    for k in ("first", "num_prims"):
        bad = np.flatnonzero(nodes[k] != ref.nodes[k])
        assert len(bad) == 0, f"{k} differs at nodes {bad[:8]} ({len(bad)} of {len(nodes)})"
    for k in ("bbox_min", "bbox_max"):
        bad = np.flatnonzero((nodes[k] != ref.nodes[k]).any(1))
        assert len(bad) == 0, f"{k} differs at nodes {bad[:8]}: {nodes[k][bad[:2]]} vs {ref.nodes[k][bad[:2]]}"
    want = {"num_nodes": len(ref.nodes), "max_depth": ref.max_depth, "max_prim_id": ref.max_prim_id,
            "max_geom_id": ref.max_geom_id, "num_indices": len(prims), "gpu_built": 1}
    assert {k: info[k] for k in want} == want


@pytest.mark.parametrize("name,max_leaf", LC.PARAMS)
def test_frame_over_the_built_tree_equals_the_oracle(ctx, oracle_mod, name, max_leaf):
    case = LC.BY_NAME[name]
    prims = case.prims
    dev = _build(ctx, prims, max_leaf)
    nodes, idx = dev.download_bvh()
    got = _frame(ctx, case, dev)
    depth = dev.info["max_depth"]
    dev.close()
    ref = LC.oracle_frame(oracle_mod, case, prims, nodes, idx, depth)
    assert (ref["prim_id"] != 0xFFFFFFFF).any()
    _same_frame(got, ref)


def test_permuted_prim_ids_pick_their_own_normals(ctx, oracle_mod):
    """simple::kernel with per-face normals over the case whose prim_id is the reversed index and whose geom_id is
    random: normals are read by prim_id, materials by geom_id.  prim_id and t bit-exact, radiance within the
    shading kernels' 1e-5 (device powf; tests/test_gpu_shading.py), misses bit-exact -- and the oracle's frame with
    the normals in index order is far outside that, so the comparison can tell the two apart."""
    O = oracle_mod
    case = LC.BY_NAME["permuted_tri"]
    prims = case.prims
    W, H = case.size
    m, lt, amb, bg = O.shade_spec()
    sh = va.shading(ctx, m.view(va.PLASTIC_DTYPE), lt.view(va.POINT_LIGHT_DTYPE))
    ocam = case.ocam()
    for max_leaf in case.max_leafs:
        dev = _build(ctx, prims, max_leaf)
        nodes, idx = dev.download_bvh()
        rt = va.hip_buffer_rt(ctx, W, H)
        va.hip_sched(ctx).frame(va.simple_kernel(dev, sh, bg=bg, ambient=amb), va.make_sched_params(case.camera(), rt))
        got = rt.download()
        rt.close()
        frames = []
        for nrm in (LC.normals_by_id(prims), va.face_normals(prims)):
            osc = O.Scene(case.name, O.VO_TRI, prims, nodes.view(O.NODE_DTYPE), idx, nrm, dev.info["max_depth"])
            frames.append(O.render_simple(osc, ocam, O.VO_NORMALS_PER_FACE))
        dev.close()
        ref, wrong = frames
        hit = ref["prim_id"] != 0xFFFFFFFF
        assert hit.any() and not hit.all()
        seen = len(prims) - 1 - np.unique(ref["prim_id"][hit])                     # prim_id -> index
        assert len(np.unique(prims["geom_id"][seen])) > 1
        assert (np.abs(ref["color"] - wrong["color"]).max(1) > 1e-2).sum() > hit.sum() // 4
        assert np.array_equal(got["prim_id"], ref["prim_id"])
        assert np.array_equal(got["t"].view(np.uint32), ref["t"].view(np.uint32))
        assert np.array_equal(got["color"][~hit].view(np.uint32), ref["color"][~hit].view(np.uint32))
        np.testing.assert_allclose(got["color"], ref["color"], rtol=1e-5, atol=1e-7)


def test_list_of_two_built_scenes_one_a_single_leaf_root(ctx, oracle_mod):
    O = oracle_mod
    case = LC.LIST_CASE
    members = LC.list_members()
    normals = LC.normals_by_id(case.prims)
    devs, osc = [], []
    for k, (prims, max_leaf) in enumerate(members):
        dev = _build(ctx, prims, max_leaf, normals=False)
        nodes, idx = dev.download_bvh()
        ref = LR.lbvh_reference(prims, max_leaf)
        assert idx.tobytes() == ref.indices.tobytes() and len(nodes) == len(ref.nodes)
        assert all(np.array_equal(nodes[f], ref.nodes[f]) for f in ("first", "num_prims", "bbox_min", "bbox_max"))
        devs.append(dev)
        osc.append(O.Scene(case.name, O.VO_TRI, prims, nodes.view(O.NODE_DTYPE), idx, normals if k == 0 else None,
                           dev.info["max_depth"]))
    assert devs[1].info["num_nodes"] == 1 and devs[1].info["max_depth"] == 0          # the single-leaf root
    assert devs[1].info["max_prim_id"] == 302
    lst = va.hip_index_bvh.scene_list(ctx, devs, normals)
    got = _frame(ctx, case, lst)
    ref = O.render(osc, case.ocam(), mode=O.VO_MODE_AO, radius=case.radius, eps=case.eps)
    hit = ref["prim_id"] != 0xFFFFFFFF
    assert (ref["prim_id"][hit] >= 300).any() and (ref["prim_id"][hit] < 300).any()    # both members are seen
    assert (ref["occ"][hit] != 0).any() and (ref["occ"][hit] != 0xFF).any()
    _same_frame(got, ref)
    lst.close()
    for d in devs:
        d.close()
