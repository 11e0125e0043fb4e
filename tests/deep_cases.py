"""Deep BVHs for the user-kernel walk (include/visionaray_hip/hip_kernels.h), shared by
tests/test_oracle_deep.py (CPU: the conditions on the oracle's frames alone) and
tests/test_gpu_user_deep.py (GPU: tests/cpp/user_kernels.hip `deep` against the oracle).

The user walk keeps its traversal stack in LDS: 24 entries per thread (VRH_USER_LDS_STACK) unless a
deeper BVH was registered, 32 (VRH_USER_STACK) at the most.  A BVH of depth d needs d + 1 entries.  The
scenes here sit on both sides of both numbers.

Family A, comb<n>: the hand-built comb of depth n - 1 (comb_bvh): n triangles of size 0.4 in the yz
plane at x = k * pitch, the inner node of level k holding the leaf of triangle k and the inner node of
level k + 1.  pitch = 0.05, so the AO rays of radius 0.1 reach the neighbours.  Two cameras at the deep
end: `oblique` sees every triangle; `axial` looks down the x axis, so a ray crosses every leaf box, the
near child is the inner node at every level, and the walk holds one pushed leaf per level: n - 1 live
entries, the stack's last one when the launch gives depth + 1.

Family B, sah<n>_<q>: n triangles v1 = (s_k, 0, 0), e1 = (0, s_k / 2, 0), e2 = (0, 0, s_k / 2) with
s_k = float32(q ** -k), built by the oracle's binned-SAH builder (the library's builder gives the same
tree, tests/test_capi.py): geometrically shrinking primitives make the builder peel a few off per
level, and its leaves hold several primitives, which the comb's never do.

A scene goes to the test program as files (write_scene) and to the oracle as the same arrays
(reference), with the lambda's parameters: AO, 8 samples, radius 0.1, eps 1e-3, frame 0.
"""
import functools
import os
from dataclasses import dataclass

import numpy as np

import visionaray_amd as va

W, H = 160, 90
MISS = 0xFFFFFFFF
PITCH = 0.05
SAH = {"sah200_1.2": (200, 1.2, 150), "sah120_1.5": (120, 1.5, 90)}      # name: (n, q, camera scale s_k)


def comb_bvh(n, pitch=0.5):
    """Hand-built 'comb' index BVH of depth n-1 over n triangles along x (valid reference layout):
    inner node at level k has children (leaf: triangle k, inner: level k+1)."""
    xs = np.arange(n, dtype=np.float32) * np.float32(pitch)
    tris = va.make_triangles(np.stack([xs, np.zeros(n), np.zeros(n)], 1), np.tile([[0.0, 0.4, 0.0]], (n, 1)),
                             np.tile([[0.0, 0.0, 0.4]], (n, 1)))
    nodes = np.zeros(2 * n - 1, va.BVH_NODE_DTYPE)

    def box(lo, hi):
        return [xs[lo], 0.0, 0.0], [xs[hi - 1], 0.4, 0.4]

    inner = 0                       # node index of the inner node for level k
    for k in range(n - 1):
        c = 2 * k + 1
        nodes[inner]["bbox_min"], nodes[inner]["bbox_max"] = box(k, n)
        nodes[inner]["first"], nodes[inner]["num_prims"] = c, 0
        nodes[c]["bbox_min"], nodes[c]["bbox_max"] = box(k, k + 1)
        nodes[c]["first"], nodes[c]["num_prims"] = k, 1
        inner = c + 1
    nodes[inner]["bbox_min"], nodes[inner]["bbox_max"] = box(n - 1, n)
    nodes[inner]["first"], nodes[inner]["num_prims"] = n - 1, 1
    return tris, va.index_bvh(tris, nodes, np.arange(n, dtype=np.uint32), n - 1)


@dataclass(frozen=True)
class Case:
    name: str
    prims: np.ndarray
    nodes: np.ndarray
    indices: np.ndarray
    normals: np.ndarray
    depth: int
    cameras: dict          # name: (eye, center, up), float32 triples


def _f32(*xs):
    return tuple(float(np.float32(x)) for x in xs)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case(name):
    """comb<n> or one of SAH"""
    from oracle import oracle as O
    O.build()
    up = (0.0, 1.0, 0.0)
    if name.startswith("comb"):
        n = int(name[4:])
        prims, bvh = comb_bvh(n, PITCH)
        nodes, indices, depth = bvh.nodes, bvh.indices, n - 1
        L = (n - 1) * PITCH
        cams = {"oblique": (_f32(L + 0.8, 0.9, 1.1), _f32(L / 2, 0.2, 0.2), up),
                "axial": (_f32(L + 1.0, 0.2, 0.2), _f32(0.0, 0.2, 0.2), up)}
    else:
        n, q, ck = SAH[name]
        s = np.array([q ** -k for k in range(n)], np.float64).astype(np.float32)
        z = np.zeros(n, np.float32)
        prims = va.make_triangles(np.stack([s, z, z], 1), np.stack([z, s / 2, z], 1), np.stack([z, z, s / 2], 1))
        nodes, indices, depth = O.build_bvh(prims, O.VO_TRI)
        c = float(s[ck])
        cams = {"oblique": (_f32(-0.6 * c, 0.9 * c, 1.3 * c), _f32(0.4 * c, 0.1 * c, 0.1 * c), up)}
    normals = O.face_normals(prims)
    _frozen(prims, nodes, indices, normals)
    return Case(name, prims, nodes, indices, normals, int(depth), cams)


@functools.lru_cache(maxsize=None)
def reference(name, camera="oblique"):
    """the oracle's AO frame of case `name` (read-only arrays; computed once per process)"""
    from oracle import oracle as O
    c = case(name)
    eye, center, up = c.cameras[camera]
    fovy = np.float32(45.0) * np.float32(1.74532925199432957692369076849e-02)
    u, v, w = O.camera_basis(eye, center, up, float(fovy), float(np.float32(W) / np.float32(H)))
    ref = O.render(O.Scene(name, O.VO_TRI, c.prims, c.nodes, c.indices, c.normals, c.depth),
                   (np.array(eye, np.float32), u, v, w, W, H))
    _frozen(*(a for a in ref.values() if isinstance(a, np.ndarray)))
    return ref


def write_scene(path, name, camera="oblique"):
    """the files of `user_kernels deep`: nodes.bin, prims.bin, indices.bin, normals.bin, cam.bin"""
    c = case(name)
    os.makedirs(path, exist_ok=True)
    assert c.nodes.dtype.itemsize == 32 and c.prims.dtype.itemsize == 64 and c.normals.shape[1] == 4
    for fn, a in (("nodes", c.nodes), ("prims", c.prims), ("indices", c.indices.astype(np.uint32)),
                  ("normals", c.normals.astype(np.float32))):
        np.ascontiguousarray(a).tofile(os.path.join(path, fn + ".bin"))
    np.array(c.cameras[camera], np.float32).tofile(os.path.join(path, "cam.bin"))
    return path


def leaf_depth_of_prims(c):
    """depth of the leaf that holds each prim_id (root: depth 0)"""
    out = np.full(len(c.prims), -1, np.int64)
    todo = [(0, 0)]
    while todo:
        i, d = todo.pop()
        first, num = int(c.nodes[i]["first"]), int(c.nodes[i]["num_prims"])
        if num == 0:
            todo += [(first, d + 1), (first + 1, d + 1)]
        else:
            out[c.prims["prim_id"][c.indices[first:first + num]]] = d
    assert (out >= 0).all() and out.max() == c.depth
    return out
