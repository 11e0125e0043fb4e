"""GPU BVH construction: vrh_scene_build builds a linear BVH on the device.

The tree is not the reference's binned-SAH tree, so the bar is:
  * structure: a valid reference-layout index BVH (root at 0, child pairs at odd indices, every
    primitive in exactly one leaf, leaves <= max_leaf, every box exactly the union of its children /
    of its primitives' reference bounds);
  * traversal on it is bit-exact against the oracle traversing the SAME (downloaded) tree;
  * quality gate: sah_cost (statistics.h) within a bound of the reference SAH tree's;
  * results against the reference frame (SAH tree): closest-hit t identical on >= 99.9 % of
    pixels (differences only where box rounding or equal-t ties differ between trees).
"""
import os
import sys

import numpy as np
import pytest

import visionaray_amd as va
from visionaray_amd import scenes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lbvh_ref import check_structure  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("name,W,H", [("cornell12", 128, 128), ("hf64", 160, 90), ("hf200", 320, 180),
                                      ("sph5000", 256, 144)])
@pytest.mark.parametrize("max_leaf", [1, 4])
def test_gpu_built_tree_traversal_matches_oracle(ctx, oracle_mod, name, W, H, max_leaf):
    O = oracle_mod
    prims = scenes.primitives(name)
    nrm = scenes.normals_for(prims)
    dev = va.hip_index_bvh.gpu_build(ctx, prims, nrm, max_leaf=max_leaf)
    assert dev.info["gpu_built"] == 1
    nodes, idx = dev.download_bvh()
    check_structure(nodes, idx, prims, max_leaf)
    cam, _, _ = scenes.scene_camera(name, W, H)
    ao = prims.dtype == va.TRIANGLE_DTYPE
    kern = va.ao_kernel(dev) if ao else va.closest_hit_kernel(dev)
    rt = va.hip_buffer_rt(ctx, W, H)
    va.hip_sched(ctx).frame(kern, va.make_sched_params(cam, rt))
    got = rt.download()
    kind = O.VO_TRI if ao else O.VO_SPHERE
    depth = dev.info["max_depth"]
    osc = O.Scene(name, kind, prims.view(O.TRI_DTYPE if ao else O.SPHERE_DTYPE), nodes.view(O.NODE_DTYPE), idx,
                  None if nrm is None else nrm, depth)
    ref = O.render(osc, O.scene_camera(name, W, H), mode=O.VO_MODE_AO if ao else O.VO_MODE_PRIMARY)
    assert np.array_equal(got["prim_id"], ref["prim_id"])
    assert np.array_equal(got["t"].view(np.uint32), ref["t"].view(np.uint32))
    assert np.array_equal(got["occ"], ref["occ"])
    assert np.array_equal(got["color"].view(np.uint32), ref["color"].view(np.uint32))


@pytest.mark.parametrize("name", ["hf1M", "sph1M"])
def test_gpu_built_tree_quality_and_reference_agreement(ctx, golden, name):
    g = golden[name]
    prims = scenes.primitives(name)
    dev = va.hip_index_bvh.gpu_build(ctx, prims, scenes.normals_for(prims))
    nodes, idx = dev.download_bvh()
    assert len(nodes) == dev.info["num_nodes"] and len(idx) == len(prims)
    ref_sah = np.uint32(int(golden["sah_cost_bits"][name], 16)).view(np.float32)
    ratio = va.sah_cost(nodes) / float(ref_sah)
    print(f"{name}: LBVH sah_cost {ratio:.3f}x the reference SAH tree")
    assert ratio < 1.25, f"LBVH sah_cost {ratio:.3f}x the reference SAH tree"
    cam, W, H = scenes.scene_camera(name)
    rt = va.hip_buffer_rt(ctx, W, H)
    va.hip_sched(ctx).frame(va.closest_hit_kernel(dev), va.make_sched_params(cam, rt))
    got = rt.download()
    ref = np.load(os.path.join(HERE, "golden", name + ".npz"))
    pix = ref["pixels"]
    same_t = got["t"][pix].view(np.uint32) == ref["t"].view(np.uint32)
    assert same_t.mean() >= 0.999, f"t differs on {(~same_t).sum()} of {len(pix)} sampled pixels"
    assert (got["prim_id"][pix] != 0xFFFFFFFF).sum() == (ref["prim_id"] != 0xFFFFFFFF).sum() or same_t.mean() >= 0.999
