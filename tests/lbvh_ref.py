"""CPU reference of the GPU LBVH build (visionaray_amd/csrc/vrh_lbvh.hip), in numpy float32.

The library is compiled without FMA contraction and with correctly rounded fp32 division, so every
step of the build is bit-predictable: primitive bounds, the Morton quantization, the stable sort,
the hierarchy over the keys (code, sorted position), the collapse to leaves of <= max_leaf
primitives and the emitted reference-layout node array.  lbvh_reference() returns what
vrh_scene_build + vrh_scene_download_bvh must return, to the bit (boxes as float values).

The hierarchy is written top-down here (split a key range at the highest differing bit); the
kernel finds the same ranges bottom-up with Karras' search.  tests/test_lbvh_reference.py holds a
literal restatement of that search and checks the two against each other on every shared case.

check_structure / prim_bounds are the structural bar of a reference-layout index BVH, shared by
test_gpu_bvh_build.py, test_lbvh_reference.py and test_gpu_lbvh_tree.py.
"""
from dataclasses import dataclass

import numpy as np

import visionaray_amd as va

LEAF = 0x80000000
F32 = np.float32


def prim_bounds(prims):
    """(lo, hi), each (n, 3) float32, the way the reference's get_bounds computes them."""
    if prims.dtype == va.TRIANGLE_DTYPE:
        v1 = prims["v1"][:, :3]
        a, b, c = v1, v1 + prims["e1"][:, :3], v1 + prims["e2"][:, :3]
        return np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
    c, r = prims["center"][:, :3], prims["radius"][:, None]
    return c - r, c + r


def check_structure(nodes, idx, prims, max_leaf):
    """A valid reference-layout index BVH: idx a permutation, every primitive in exactly one leaf of
    <= max_leaf primitives, every box exactly the union of its primitives' / children's boxes,
    children as pairs at odd indices, 2 * inner + 1 nodes."""
    n = len(prims)
    assert np.array_equal(np.sort(idx), np.arange(n, dtype=np.uint32))
    lo, hi = prim_bounds(prims)
    bmin, bmax = nodes["bbox_min"], nodes["bbox_max"]
    leaf = nodes["num_prims"] != 0
    assert (nodes["num_prims"][leaf] <= max_leaf).all()
    covered = np.zeros(n, np.int64)
    for k in np.nonzero(leaf)[0]:
        f, c = nodes["first"][k], nodes["num_prims"][k]
        sel = idx[f:f + c]
        covered[f:f + c] += 1
        assert np.array_equal(bmin[k], lo[sel].min(0)) and np.array_equal(bmax[k], hi[sel].max(0))
    assert (covered == 1).all()
    inner = np.nonzero(~leaf)[0]
    fc = nodes["first"][inner]
    assert (fc % 2 == 1).all() and (fc + 1 < len(nodes)).all()
    assert np.array_equal(bmin[inner], np.minimum(bmin[fc], bmin[fc + 1]))
    assert np.array_equal(bmax[inner], np.maximum(bmax[fc], bmax[fc + 1]))
    assert len(np.unique(fc)) == len(fc) and len(nodes) == 2 * len(inner) + 1


def effective_max_leaf(max_leaf):
    """vrh_scene_build: 0 means 4, the rest is clamped to 1..64"""
    return 4 if max_leaf == 0 else max(1, min(int(max_leaf), 64))


def _expand10(v):
    """10 bits -> every third bit"""
    v = v.astype(np.uint64)
    for mul, mask in ((0x00010001, 0xFF0000FF), (0x00000101, 0x0F00F00F), (0x00000011, 0xC30C30C3),
                      (0x00000005, 0x49249249)):
        v = ((v * np.uint64(mul)) & np.uint64(0xFFFFFFFF)) & np.uint64(mask)
    return v.astype(np.uint32)


def morton_codes(lo, hi):
    """30-bit codes of the primitives' centroids, quantized against the centroid bounds of the
    primitives whose six bounds are finite, one scale (the largest extent) for all axes."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        cen = (lo + hi) * F32(0.5)
        ok = np.isfinite(lo).all(1) & np.isfinite(hi).all(1)
        if ok.any():
            cmin, cmax = cen[ok].min(0), cen[ok].max(0)
        else:
            cmin, cmax = np.full(3, np.inf, F32), np.full(3, -np.inf, F32)
        d = cmax - cmin
        ext = np.fmax(np.fmax(d[0], d[1]), d[2])
        if ext > 0:
            u = (cen - cmin) / ext
        else:
            u = np.full_like(cen, 0.5)
        u = np.where(np.isfinite(u), np.fmin(np.fmax(u, F32(0.0)), F32(1.0)), F32(0.5)).astype(F32)
        q = np.minimum((u * F32(1024.0)).astype(np.uint32), np.uint32(1023))
    assert cen.dtype == F32 and u.dtype == F32
    return (_expand10(q[:, 0]) << np.uint32(2)) | (_expand10(q[:, 1]) << np.uint32(1)) | _expand10(q[:, 2])


def hierarchy_topdown(codes):
    """The binary radix tree over the keys (codes[p] << 32) | p of the sorted codes, top-down: the
    node over [f, l] splits at the highest bit in which key[f] and key[l] differ, gamma is the last
    position on f's side; the root is node 0, an inner left child node gamma, an inner right child
    node gamma + 1.  Returns (first, last, gamma, child, parent, order): per node its range, split,
    two children (LEAF | position, or node index) and parent (-1 for the root), and the nodes in an
    order that lists every parent before its children."""
    n = len(codes)
    m = n - 1
    keys = [(int(c) << 32) | p for p, c in enumerate(codes)]
    first = np.full(m, -1, np.int64)
    last = np.full(m, -1, np.int64)
    gamma = np.full(m, -1, np.int64)
    child = np.zeros((m, 2), np.int64)
    parent = np.full(m, -1, np.int64)
    order = []
    if m <= 0:
        return first, last, gamma, child, parent, order
    karr = np.array(keys, dtype=np.uint64)
    stack = [(0, 0, n - 1, -1)]
    while stack:
        i, f, l, par = stack.pop()
        assert first[i] == -1, "a hierarchy index was given to two nodes"
        b = (keys[f] ^ keys[l]).bit_length() - 1
        g = int(np.searchsorted(karr, np.uint64((keys[l] >> b) << b), side="left")) - 1
        assert f <= g < l
        first[i], last[i], gamma[i], parent[i] = f, l, g, par
        order.append(i)
        for side, (cf, cl, ci) in enumerate(((f, g, g), (g + 1, l, g + 1))):
            if cf == cl:
                child[i, side] = LEAF | cf
            else:
                child[i, side] = ci
                stack.append((ci, cf, cl, i))
    assert len(order) == m
    return first, last, gamma, child, parent, order


@dataclass
class Tree:
    nodes: np.ndarray           # va.BVH_NODE_DTYPE, the reference layout
    indices: np.ndarray         # uint32: the sorted original indices
    max_depth: int
    max_prim_id: int
    max_geom_id: int
    max_leaf: int               # the effective one
    codes: np.ndarray           # sorted Morton codes
    num_visible: int


def lbvh_reference(prims, max_leaf):
    """What vrh_scene_build(prims, max_leaf) must build: see the module docstring."""
    n = len(prims)
    ml = effective_max_leaf(max_leaf)
    with np.errstate(invalid="ignore", over="ignore"):
        lo, hi = prim_bounds(prims)
    lo, hi = np.ascontiguousarray(lo, F32), np.ascontiguousarray(hi, F32)
    codes = morton_codes(lo, hi)
    idx = np.argsort(codes, kind="stable").astype(np.uint32)
    codes = codes[idx]
    slo, shi = lo[idx], hi[idx]                              # bounds in sorted order
    mpid, mgid = int(prims["prim_id"].max()), int(prims["geom_id"].max())

    def union(f, l):
        return np.fmin.reduce(slo[f:l + 1], axis=0), np.fmax.reduce(shi[f:l + 1], axis=0)

    if n <= ml:
        nodes = np.zeros(1, va.BVH_NODE_DTYPE)
        nodes["bbox_min"][0], nodes["bbox_max"][0] = union(0, n - 1)
        nodes["first"][0], nodes["num_prims"][0] = 0, n
        return Tree(nodes, idx, 0, mpid, mgid, ml, codes, 0)

    first, last, gamma, child, parent, order = hierarchy_topdown(codes)
    size = last - first + 1
    vis = size > ml
    slot = np.cumsum(vis) - vis                              # rank among the visible, by hierarchy index
    V = int(vis.sum())
    assert vis[0] and slot[0] == 0
    nodes = np.zeros(1 + 2 * V, va.BVH_NODE_DTYPE)
    nodes["first"][0] = 1
    where = {0: 0}                                           # visible hierarchy node -> emitted node
    for j in order:
        if not vis[j]:
            continue
        s = int(slot[j])
        for side in range(2):
            k = 2 * s + 1 + side
            c = int(child[j, side])
            if c & LEAF:
                p = c & ~LEAF
                nodes["first"][k], nodes["num_prims"][k] = p, 1
                nodes["bbox_min"][k], nodes["bbox_max"][k] = union(p, p)
            elif vis[c]:
                nodes["first"][k], nodes["num_prims"][k] = 2 * int(slot[c]) + 1, 0
                where[c] = k
            else:
                nodes["first"][k], nodes["num_prims"][k] = first[c], size[c]
                nodes["bbox_min"][k], nodes["bbox_max"][k] = union(first[c], last[c])
    for j in reversed(order):                                # children before parents
        if vis[j]:
            k, fc = where[j], 2 * int(slot[j]) + 1
            nodes["bbox_min"][k] = np.fmin(nodes["bbox_min"][fc], nodes["bbox_min"][fc + 1])
            nodes["bbox_max"][k] = np.fmax(nodes["bbox_max"][fc], nodes["bbox_max"][fc + 1])
    depth = 0
    for j in np.nonzero(vis)[0]:
        d, a = 1, int(j)
        while parent[a] >= 0:
            a = int(parent[a])
            d += 1
        depth = max(depth, d)
    return Tree(nodes, idx, depth, mpid, mgid, ml, codes, V)
