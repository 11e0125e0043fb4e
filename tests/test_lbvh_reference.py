"""CPU: the reference of the GPU LBVH build (tests/lbvh_ref.py) is pinned before the GPU tests lean on it.

  * its tree passes the structural bar of a reference-layout index BVH on every shared case;
  * its hierarchy, written top-down over the keys (code, position), equals a literal restatement of the kernel's
    Karras search (direction, lmax doubling, the two binary searches, delta with the index tie-break) written here
    independently: same ranges, same splits, same child kinds, on every case and on random arrays of heavily
    duplicated codes;
  * every case's camera gives the frame tests something to compare: hit and miss pixels, and for the AO (triangle)
    cases occluded and unoccluded samples.  The all-identical sets may fill the image; none needs to.
"""
import os
import sys

import numpy as np
import pytest

import visionaray_amd as va

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lbvh_cases as LC  # noqa: E402
import lbvh_ref as LR  # noqa: E402

LEAF = LR.LEAF


def _clz32(x):
    return 32 - int(x).bit_length()


def karras(codes):
    """k_karras of vrh_lbvh.hip, statement for statement, for every node i in [0, n - 1):
    (first, last, gamma, left, right)"""
    n = len(codes)
    codes = [int(c) for c in codes]

    def delta(i, j):
        if j < 0 or j >= n:
            return -1
        a, b = codes[i], codes[j]
        if a == b:
            return 32 + _clz32(i ^ j)
        return _clz32(a ^ b)

    out = []
    for i in range(n - 1):
        d = 1 if delta(i, i + 1) - delta(i, i - 1) >= 0 else -1
        dmin = delta(i, i - d)
        lmax = 2
        while delta(i, i + lmax * d) > dmin:
            lmax *= 2
        l, t = 0, lmax // 2
        while t >= 1:
            if delta(i, i + (l + t) * d) > dmin:
                l += t
            t //= 2
        j = i + l * d
        dnode = delta(i, j)
        s, t = 0, l
        while True:
            t = (t + 1) >> 1
            if delta(i, i + (s + t) * d) > dnode:
                s += t
            if t <= 1:
                break
        gamma = i + s * d + min(d, 0)
        first, last = min(i, j), max(i, j)
        left = (LEAF | gamma) if first == gamma else gamma
        right = (LEAF | (gamma + 1)) if last == gamma + 1 else gamma + 1
        out.append((first, last, gamma, left, right))
    return out


def _agree(codes):
    first, last, gamma, child, parent, order = LR.hierarchy_topdown(codes)
    top = [(int(first[i]), int(last[i]), int(gamma[i]), int(child[i, 0]), int(child[i, 1])) for i in range(len(first))]
    assert top == karras(codes)
    return len(top)


@pytest.mark.parametrize("name", [c.name for c in LC.CASES] + [LC.LIST_CASE.name])
def test_topdown_hierarchy_equals_the_karras_search(name):
    prims = LC.BY_NAME[name].prims
    codes = LR.lbvh_reference(prims, 1).codes
    m = _agree(codes)
    dup = len(codes) - len(np.unique(codes))
    print(f"{name}: {m} hierarchy nodes, {dup} duplicated codes: top-down == Karras")


def test_topdown_hierarchy_equals_the_karras_search_on_duplicated_codes():
    rng = np.random.default_rng(77)
    for k in range(60):
        n = int(rng.integers(2, 200))
        distinct = int(rng.integers(1, 12))
        pool = rng.integers(0, 1 << 30, distinct, dtype=np.uint32)
        if k % 3 == 0:
            pool = (np.uint32(1) << rng.integers(0, 30, distinct).astype(np.uint32)) | np.uint32(k % 2)
        _agree(np.sort(pool[rng.integers(0, distinct, n)]))


@pytest.mark.parametrize("name,max_leaf", LC.PARAMS)
def test_reference_tree_is_a_valid_bvh(name, max_leaf):
    prims = LC.BY_NAME[name].prims
    tree = LR.lbvh_reference(prims, max_leaf)
    ml = LR.effective_max_leaf(max_leaf)
    LR.check_structure(tree.nodes, tree.indices, prims, ml)
    n = len(prims)
    assert len(tree.nodes) == 1 + 2 * tree.num_visible
    if n <= ml:
        assert len(tree.nodes) == 1 and tree.max_depth == 0 and tree.nodes["num_prims"][0] == n
    else:
        # depth of the emitted tree, walked from the root: the deepest inner node (root 1) is max_depth
        deepest, st = 0, [(0, 1)]
        while st:
            k, d = st.pop()
            if tree.nodes["num_prims"][k] == 0:
                deepest = max(deepest, d)
                st += [(int(tree.nodes["first"][k]), d + 1), (int(tree.nodes["first"][k]) + 1, d + 1)]
        assert tree.max_depth == deepest
    assert tree.max_prim_id == int(prims["prim_id"].max()) and tree.max_geom_id == int(prims["geom_id"].max())


def test_case_list_covers_the_edges():
    ns = {len(c.prims) for c in LC.CASES}
    assert {1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 37, 300} <= ns and max(ns) <= 4100
    assert {ml for _, ml in LC.PARAMS} == {0, 1, 2, 3, 4, 8, 64, 100}
    rel = set()
    for name, ml in LC.PARAMS:
        n, e = len(LC.BY_NAME[name].prims), LR.effective_max_leaf(ml)
        rel.add("n == max_leaf" if n == e else "n == max_leaf + 1" if n == e + 1 else "n < max_leaf" if n < e else "")
    assert {"n == max_leaf", "n == max_leaf + 1", "n < max_leaf"} <= rel
    kinds = {c.prims.dtype for c in LC.CASES}
    assert kinds == {va.TRIANGLE_DTYPE, va.SPHERE_DTYPE}
    assert all(c.size[0] <= 96 and c.size[1] <= 64 for c in LC.CASES + [LC.LIST_CASE])
    p = LC.BY_NAME["permuted_tri"].prims
    assert np.array_equal(np.sort(p["prim_id"]), np.arange(len(p))) and (p["prim_id"] != np.arange(len(p))).all()
    assert len(np.unique(p["geom_id"])) > 1
    assert np.isinf(LC.BY_NAME["inf_sph"].prims["radius"]).sum() == 1
    for name in ("same37_sph", "same300_sph", "same_box_tri"):
        assert len(np.unique(LR.lbvh_reference(LC.BY_NAME[name].prims, 1).codes)) == 1
    lo, hi = LR.prim_bounds(LC.BY_NAME["lattice_tri"].prims)
    u = ((lo + hi) * np.float32(0.5) + np.float32(2.0)) * np.float32(256.0)
    assert np.array_equal(u, np.round(u)) and u.min() == 0 and u.max() == 1024


@pytest.mark.parametrize("name", [c.name for c in LC.CASES] + [LC.LIST_CASE.name])
def test_case_camera_sees_hits_misses_and_occlusion(oracle_mod, name):
    O = oracle_mod
    case = LC.BY_NAME[name]
    prims = case.prims
    for max_leaf in case.max_leafs:
        tree = LR.lbvh_reference(prims, max_leaf)
        ref = LC.oracle_frame(O, case, prims, tree.nodes, tree.indices, tree.max_depth)
        hit = ref["prim_id"] != 0xFFFFFFFF
        line = f"{name}/{max_leaf}: {int(hit.sum())} hit, {int((~hit).sum())} miss"
        assert hit.any() and not hit.all(), line
        if case.ao:
            occ = ref["occ"][hit]
            line += f", {int((occ != 0).sum())} pixels with occluded, {int((occ != 0xFF).sum())} with unoccluded samples"
            assert (occ != 0).any() and (occ != 0xFF).any(), line
        print(line)


def test_gpu_build_checks_the_normals_shape():
    """hip_index_bvh.gpu_build refuses normals that are not (len(prims), 4) before it touches the context"""
    prims = LC.BY_NAME["n5_tri"].prims
    for bad in (np.zeros((4, 4), np.float32), np.zeros((6, 4), np.float32), np.zeros((5, 3), np.float32),
                np.zeros(20, np.float32)):
        with pytest.raises(ValueError, match="normals"):
            va.hip_index_bvh.gpu_build(None, prims, bad)
