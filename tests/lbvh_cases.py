"""Shared inputs of the LBVH tree tests (test_lbvh_reference.py on the CPU, test_gpu_lbvh_tree.py on the GPU).

Every case is a small seeded primitive set that puts the GPU build (vrh_lbvh.hip) on a path the
fixed scenes do not reach -- a single-leaf root, the smallest Karras ranges, equal Morton codes,
wave and block edges, degenerate centroid extents, ids that differ from the index, non-finite
bounds -- with the max_leaf values to build it with and a camera under which the frame has hit
and miss pixels (and, for the triangle cases, which render AO, occluded and unoccluded samples;
test_lbvh_reference.py holds the cameras to that).
"""
import itertools
import os
import sys
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import visionaray_amd as va

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_fuzz import _ocam, _scene  # noqa: E402

F32 = np.float32


@dataclass(frozen=True)
class Case:
    name: str
    make: object                # () -> primitives
    max_leafs: tuple            # the max_leaf values to build with (0 -> 4, > 64 -> 64)
    eye: tuple
    center: tuple
    size: tuple = (96, 64)      # image
    fovy: float = 45.0          # degrees
    radius: float = 0.1         # AO radius (triangle cases)
    eps: float = 1e-3           # AO ray offset

    @property
    def prims(self):
        return _prims(self.name)

    @property
    def ao(self):
        return self.prims.dtype == va.TRIANGLE_DTYPE

    def camera(self):
        W, H = self.size
        cam = va.camera()
        cam.perspective(float(F32(self.fovy) * F32(va.DEGREES_TO_RADIANS)), float(F32(W) / F32(H)), 0.001, 1000.0)
        cam.look_at(self.eye, self.center, (0.0, 1.0, 0.0))
        return cam

    def ocam(self):
        W, H = self.size
        return _ocam(self.camera().basis(W, H), W, H)


# ---- generators ---------------------------------------------------------------------------------

def _rng(tag):
    return np.random.default_rng([20240917, sum(ord(c) * (k + 1) for k, c in enumerate(tag))])


def _tris(rng, centers, size):
    """random triangles of edge length ~size about the given centres"""
    centers = np.asarray(centers, np.float64).reshape(-1, 3)
    e1 = rng.standard_normal(centers.shape) * size
    e2 = rng.standard_normal(centers.shape) * size
    return va.make_triangles(centers - (e1 + e2) / 3.0, e1, e2)


def _boxed_tris(c, h, flip):
    """triangles whose bounds are exactly c -/+ h on the axes where h > 0 (c, h: (n, 3) float32 with c - h and c + h
    exact), so that their centroid is exactly c; flip picks one of two shapes"""
    c, h = np.asarray(c, F32), np.asarray(h, F32)
    n = len(c)
    v1 = c - h
    e1 = np.zeros((n, 3), F32)
    e2 = np.zeros((n, 3), F32)
    two = F32(2.0) * h
    f = np.asarray(flip, bool)
    # shape 0: corners (-,-,-) (+,-,+) (-,+,0); shape 1: corners (-,-,-) (+,+,0) (0,-,+)
    e1[:, 0] = two[:, 0]
    e1[:, 1] = np.where(f, two[:, 1], 0)
    e1[:, 2] = np.where(f, h[:, 2], two[:, 2])
    e2[:, 0] = np.where(f, h[:, 0], 0)
    e2[:, 1] = np.where(f, 0, two[:, 1])
    e2[:, 2] = np.where(f, two[:, 2], h[:, 2])
    return va.make_triangles(v1, e1, e2)


def _random(kind, n, size):
    def make():
        rng = _rng(f"{kind}{n}")
        c = rng.uniform(-1.0, 1.0, (n, 3))
        if kind == "tri":
            return _tris(rng, c, size)
        return va.make_spheres(c, (size * rng.uniform(0.4, 1.6, n)).astype(F32))
    return make


def _same_spheres(n):
    def make():
        return va.make_spheres(np.tile(F32([0.25, -0.125, 0.5]), (n, 1)), np.full(n, 0.375, F32))
    return make


def _same_box_tris():
    """50 triangles, 25 shapes twice over, all with the bounds [0, 1]^3: identical centroids (every code comes from
    u = 0.5) but not coplanar, so that AO rays find occluders"""
    corners = np.array(list(itertools.product((0.0, 1.0), repeat=3)), F32)
    shapes = [t for t in itertools.combinations(range(8), 3)
              if (corners[list(t)].min(0) == 0).all() and (corners[list(t)].max(0) == 1).all()]
    rng = _rng("samebox")
    pick = [shapes[k] for k in rng.permutation(len(shapes))[:25]] * 2
    a, b, c = (corners[[t[k] for t in pick]] for k in range(3))
    return va.make_triangles(a, b - a, c - a)


def _clusters():
    """500 triangles spread over 3 centroids (concentric, of many sizes) beside 20 isolated ones"""
    rng = _rng("clusters")
    cen = F32([[-0.625, 0.25, 0.375], [0.5, -0.375, -0.25], [0.125, 0.625, -0.5]])
    which = rng.integers(0, 3, 500)
    h = (2.0 ** rng.integers(-9, -2, (500, 3))).astype(F32)           # powers of two: c -/+ h is exact
    t = _boxed_tris(cen[which], h, rng.random(500) < 0.5)
    iso = _tris(rng, rng.uniform(-1.0, 1.0, (20, 3)), 0.15)
    out = np.concatenate([t, iso])[rng.permutation(520)]
    out["prim_id"] = np.arange(520, dtype=np.uint32)
    return out


def _planar():
    """400 triangles whose centroids have z = 0.25 exactly (their z ranges are 0.25 -/+ h): one extent is zero"""
    rng = _rng("planar")
    c = np.concatenate([rng.uniform(-1.0, 1.0, (400, 2)), np.full((400, 1), 0.25)], 1).astype(F32)
    h = np.concatenate([rng.uniform(0.02, 0.12, (400, 2)), 2.0 ** rng.integers(-5, -2, (400, 1))], 1).astype(F32)
    return _boxed_tris(c, h, rng.random(400) < 0.5)


def _collinear():
    """300 spheres centred on the x axis: two extents are zero"""
    rng = _rng("collinear")
    c = np.zeros((300, 3))
    c[:, 0] = rng.uniform(-1.0, 1.0, 300)
    return va.make_spheres(c, (10.0 ** rng.uniform(-2.5, -1.0, 300)).astype(F32))


def _lattice():
    """1000 triangles whose centroids are -2 + k / 256, k in 0..1024 per axis: exactly on the cell lattice k / 1024
    of the extent 4, both ends included, so that every quantization falls on a cell boundary"""
    rng = _rng("lattice")
    k = rng.integers(0, 1025, (1000, 3))
    k[0], k[1] = 0, 1024
    c = (F32(-2.0) + k.astype(F32) / F32(256.0)).astype(F32)
    return _boxed_tris(c, np.full((1000, 3), 0.0625, F32), rng.random(1000) < 0.5)


def _deep():
    """32 clusters of 60 triangles at scale 1e-4 in a scene of extent 1e3.  Each cluster shares one Morton cell, so
    the hierarchy under it is decided by the index tie-break alone; the clusters sit in the cells 2^L (L = 0..9) of
    each axis, at the origin and in the far corner, so that their codes are 0, the 30 single bits and all ones: one
    cluster splits off per Morton bit -- the deepest tree 30-bit codes give.  The camera looks at the origin's."""
    rng = _rng("deep")
    cell = 1000.0 / 1024.0
    cc = [(0.0, 0.0, 0.0), (1000.0, 1000.0, 1000.0)]
    for axis in range(3):
        for L in range(10):
            p = [0.0, 0.0, 0.0]
            p[axis] = (2.0 ** L + 0.5) * cell
            cc.append(tuple(p))
    c = np.repeat(np.array(cc), 60, 0) + rng.uniform(-1e-4, 1e-4, (1920, 3))
    return _tris(rng, c, 1e-4)


def _fuzz(seed, kind):
    def make():
        return _scene(np.random.default_rng(seed), kind)
    return make


def _permuted():
    """prim_id the reversed index, geom_id random in 0..2 (the shading tests' three materials)"""
    rng = _rng("permuted")
    t = _tris(rng, rng.uniform(-1.0, 1.0, (300, 3)), 0.25)
    t["prim_id"] = np.arange(300, dtype=np.uint32)[::-1]
    t["geom_id"] = rng.integers(0, 3, 300)
    return t


def _inf_sphere():
    """200 spheres, one of radius inf: non-finite bounds, a NaN centroid"""
    rng = _rng("inf")
    s = va.make_spheres(rng.uniform(-1.0, 1.0, (200, 3)), (10.0 ** rng.uniform(-2.0, -0.8, 200)).astype(F32))
    s["radius"][77] = np.inf
    return s


# n == max_leaf: n1/1, n2/2, n3/3, n4/4 and /0, n64/64 and /100; n == max_leaf + 1: n2/1, n3/2, n4/3, n5/0 and /4,
# n65/64 and /100; n < max_leaf: n1/4, n2/0, n3/8, n5/8, n63/64, same37/64, same_box/100
CASES = [
    Case("n1_sph", _random("sph", 1, 0.5), (1, 4), (0.0, 0.0, 4.0), (0.0, 0.0, 0.0), (33, 27)),
    Case("n2_tri", _random("tri", 2, 0.8), (1, 2, 0), (0.0, 0.0, 4.0), (0.0, 0.0, 0.0), (40, 30), radius=2.0),
    Case("n3_sph", _random("sph", 3, 0.4), (1, 2, 3, 8), (0.0, 0.0, 4.0), (0.0, 0.0, 0.0), (47, 31)),
    Case("n4_tri", _random("tri", 4, 0.8), (1, 3, 4, 0), (0.0, 0.0, 4.0), (0.0, 0.0, 0.0), (64, 48), radius=2.0),
    Case("n5_tri", _random("tri", 5, 0.8), (0, 2, 4, 8), (0.0, 0.0, 4.0), (0.0, 0.0, 0.0), (64, 48), radius=2.0),
    Case("n63_tri", _random("tri", 63, 0.4), (1, 8, 64), (0.0, 0.0, 4.0), (0.0, 0.0, 0.0), radius=1.0),
    Case("n64_sph", _random("sph", 64, 0.15), (3, 64, 100), (0.0, 0.0, 4.0), (0.0, 0.0, 0.0), (95, 63)),
    Case("n65_tri", _random("tri", 65, 0.4), (2, 64, 100), (0.0, 0.0, 4.0), (0.0, 0.0, 0.0), radius=1.0),
    Case("n255_sph", _random("sph", 255, 0.1), (1, 4), (0.0, 0.0, 4.0), (0.0, 0.0, 0.0), (81, 57)),
    Case("n256_tri", _random("tri", 256, 0.3), (0, 8), (0.0, 0.0, 4.0), (0.0, 0.0, 0.0), radius=0.5),
    Case("n257_tri", _random("tri", 257, 0.3), (1, 64), (0.0, 0.0, 4.0), (0.0, 0.0, 0.0), radius=0.5),
    Case("n257_sph", _random("sph", 257, 0.1), (3,), (0.0, 0.0, 4.0), (0.0, 0.0, 0.0), (73, 41)),
    Case("same37_sph", _same_spheres(37), (1, 4, 64), (0.25, -0.125, 3.0), (0.25, -0.125, 0.5), (48, 32)),
    Case("same300_sph", _same_spheres(300), (1, 8, 100), (2.0, 1.0, 2.5), (0.25, -0.125, 0.5), (45, 35)),
    Case("same_box_tri", _same_box_tris, (1, 3, 100), (2.5, 1.8, 3.0), (0.5, 0.5, 0.5), (64, 48), radius=1.0),
    Case("clusters_tri", _clusters, (1, 2, 64), (0.0, 0.0, 4.0), (0.0, 0.0, 0.0), radius=0.3),
    Case("planar_tri", _planar, (1, 4), (0.0, 0.0, 4.0), (0.0, 0.0, 0.0), radius=0.3),
    Case("collinear_sph", _collinear, (1, 3), (0.0, 0.3, 3.0), (0.0, 0.0, 0.0), (96, 33)),
    Case("lattice_tri", _lattice, (1, 4), (0.0, 0.0, 8.0), (0.0, 0.0, 0.0), radius=0.5),
    Case("deep_tri", _deep, (1, 4), (3e-4, 2e-4, 6e-4), (0.0, 0.0, 0.0), radius=2e-4, eps=1e-6),
    Case("fuzz_tri_a", _fuzz(31, "tri"), (0, 1), (0.0, 0.0, 4.0), (0.0, 0.0, 0.0)),
    Case("fuzz_tri_b", _fuzz(41, "tri"), (4,), (0.0, 0.0, 4.0), (0.0, 0.0, 0.0)),
    Case("fuzz_sph", _fuzz(39, "sph"), (2, 8), (0.0, 0.0, 4.0), (0.0, 0.0, 0.0), (91, 61)),
    Case("permuted_tri", _permuted, (1, 4), (0.0, 0.0, 4.0), (0.0, 0.0, 0.0), radius=0.5),
    Case("inf_sph", _inf_sphere, (1, 4), (0.0, 0.0, 4.0), (0.0, 0.0, 0.0), (64, 40)),
]
BY_NAME = {c.name: c for c in CASES}
PARAMS = [(c.name, ml) for c in CASES for ml in c.max_leafs]


@lru_cache(maxsize=None)
def _prims(name):
    p = BY_NAME[name].make()
    p.flags.writeable = False
    return p


def list_members():
    """The two members of the scene-list case: 300 triangles (prim ids 0..299), and three more (300..302) that a
    max_leaf of 4 leaves as a single-leaf root.  Returns [(prims, max_leaf), ...] and the list's camera case."""
    rng = _rng("list")
    a = _tris(rng, rng.uniform(-1.0, 1.0, (300, 3)), 0.25)
    b = _tris(rng, rng.uniform(-0.6, 0.6, (3, 3)), 0.9)
    b["prim_id"] = np.arange(300, 303, dtype=np.uint32)
    return [(a, 1), (b, 4)]


LIST_CASE = Case("list_tri", lambda: np.concatenate([m for m, _ in list_members()]), (1,), (0.0, 0.0, 4.0),
                 (0.0, 0.0, 0.0), (80, 50), radius=0.5)
BY_NAME[LIST_CASE.name] = LIST_CASE


def normals_by_id(prims):
    """face normals as the kernels read them: row prim_id (va.face_normals is in index order)"""
    out = np.zeros((int(prims["prim_id"].max()) + 1, 4), F32)
    out[prims["prim_id"]] = va.face_normals(prims)
    return out


def oracle_frame(O, case, prims, nodes, indices, max_depth):
    """The case's frame by the oracle over the given tree: AO with per-face normals for triangles, primary
    visibility for spheres"""
    ao = prims.dtype == va.TRIANGLE_DTYPE
    osc = O.Scene(case.name, O.VO_TRI if ao else O.VO_SPHERE, prims, np.ascontiguousarray(nodes).view(O.NODE_DTYPE),
                  np.ascontiguousarray(indices), normals_by_id(prims) if ao else None, max_depth)
    return O.render(osc, case.ocam(), mode=O.VO_MODE_AO if ao else O.VO_MODE_PRIMARY, radius=case.radius, eps=case.eps)
