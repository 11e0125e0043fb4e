"""CPU: the deep-BVH scenes of tests/deep_cases.py exercise the walk -- conditions on the oracle's
frames alone, so a scene that stops doing so fails here and not silently in the GPU comparison
(tests/test_gpu_user_deep.py).

Measured on the oracle (160 x 90): the comb's oblique camera for n = 24 .. 41 shows every one of the n
prim ids and 1,500 - 1,900 hit pixels with a non-zero occlusion mask; sah200_1.2 is 24 deep with 2,785
hit pixels on 23 prims, the deepest hit leaf at depth 19; sah120_1.5 is 28 deep with 1,933 hit pixels
on 11 prims, the deepest hit leaf at depth 22.
"""
import numpy as np
import pytest

import deep_cases as D


@pytest.mark.parametrize("n", [24, 25, 28, 32, 33, 41])
def test_comb_oblique_camera_sees_every_leaf_and_occlusion(n):
    ref = D.reference(f"comb{n}", "oblique")
    hit = ref["prim_id"] != D.MISS
    seen = np.unique(ref["prim_id"][hit])
    occluded = int((ref["occ"][hit] != 0).sum())
    print(f"comb{n}: {seen.size} prims, {int(hit.sum())} hit pixels, {occluded} occluded")
    assert D.case(f"comb{n}").depth == n - 1
    assert np.array_equal(seen, np.arange(n)), "every triangle of the comb is some pixel's closest hit"
    assert occluded >= 1000


@pytest.mark.parametrize("n", [24, 25, 28, 32])
def test_comb_axial_camera_crosses_every_leaf_box(n):
    """The camera looks down the x axis from the deep end, at (0.2, 0.2) of the triangles' yz box: every
    triangle behind the nearest one (prim n - 1, the deepest leaf) projects inside it, so the rays
    that hit anything hit that one -- a triangle 0.4 wide at distance 1 under 45 degrees, about 900
    pixels -- after their walk has passed the box of every other leaf.  (The hypotenuse runs through
    the centre of projection, so a pixel on it may fall to a triangle behind.)"""
    ref = D.reference(f"comb{n}", "axial")
    hit = ref["prim_id"] != D.MISS
    nearest = int((ref["prim_id"] == n - 1).sum())
    print(f"comb{n} axial: {int(hit.sum())} hit pixels, {nearest} on prim {n - 1}")
    assert int(hit.sum()) >= 500
    assert nearest >= 0.9 * hit.sum()


@pytest.mark.parametrize("name", sorted(D.SAH))
def test_sah_scenes_are_deep_and_hit_deep_leaves(name):
    c = D.case(name)
    ref = D.reference(name)
    hit = ref["prim_id"] != D.MISS
    seen = np.unique(ref["prim_id"][hit])
    deepest = int(D.leaf_depth_of_prims(c)[seen].max())
    leaf_sizes = c.nodes["num_prims"][c.nodes["num_prims"] > 0]
    print(f"{name}: depth {c.depth}, {int(hit.sum())} hit pixels, {seen.size} prims, deepest hit leaf {deepest}, "
          f"largest leaf {int(leaf_sizes.max())}")
    assert 24 <= c.depth <= 31
    assert int(hit.sum()) >= 1000
    assert seen.size >= 10
    assert deepest >= 18
    assert leaf_sizes.max() > 1, "leaves of several primitives"
