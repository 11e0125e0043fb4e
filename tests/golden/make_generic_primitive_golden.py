#!/usr/bin/env python3
"""Fixtures of mixed triangle / sphere scenes (VRH_PRIM_GENERIC80): tests/golden/gp_<case>.npz and
tests/golden/generic_primitive.json.

Compiles tests/golden/generic_primitive_ref.cpp (the reference's own builder, closest_hit / any_hit,
simple::kernel and whitted::kernel over generic_primitive<basic_triangle<3, float>, basic_sphere<float>>,
from the reference tree's headers) with g++ into oracle/_ref/ and runs it.  Runs only where the reference
tree exists; nothing in build(), smoke(), bench.py or the tests calls it.

    python tests/golden/make_generic_primitive_golden.py [--ref /path/to/reference]

Cases, each a function of its seed alone, 60 x 44 pixels (partial 8 x 8 tiles on both edges):
  gp_example  the reference example's scene (src/examples/generic_primitive: two pyramids of 6 triangles, two
              spheres, four plastics, one light at (0, 10, 10), 4 bounces, epsilon 1e-4) from the example's own
              camera, view_all() of its box [-1, 1] x [-1, 1] x [0, 2] at 45 degrees (camera.inl:79-87);
              the seed is the animation frame: the moving sphere's y after seed - 100 of the example's steps
              (y = -0.5, then y += 0.2f * 0.1f per frame, in float)
  gp_soup     150 random triangles and 150 random spheres, interleaved in prim order, geom_id = prim_id % 4
  gp_inside   the camera inside one large sphere that encloses a few triangles and small spheres: the large
              sphere's nearer root is behind the origin (t < 0, rejected), so its pixels miss
  gp_sweep    the scene generator of the randomized GPU sweep (tests/gp_cases.py sweep_scene / sweep_shading /
              sweep_camera) at fewer primitives: 160 triangles with sizes from 1e-3 to 0.3, some of them slivers,
              120 spheres of radius 1e-3 to 0.2 that overlap, the camera inside the cloud, one to three lights
Every .npz is self-contained: the 80-byte records (20 u32 words), the reference's nodes and indices, normals
(one row per prim_id; a sphere's row is never read and stays 0), plastic materials (13 floats), lights (10
floats), the camera basis (eye, u, v, w), and per pixel prim_id / t (primary), occ / ao_color (AO, the
deterministic sample spec of oracle/ref_harness.cpp, the normal through get_surface), simple_color,
whitted_color, and whitted_cross (1 where a path reflects from a sphere onto a triangle or the reverse).

A seed is refused -- and the next one tried, never a condition relaxed -- unless: at least one leaf holds both
kinds; each kind is the closest hit on at least 5 % of the pixels; some pixels miss; some AO rays are
occluded; some pixel's whitted path reflects across kinds; every colour is finite.  The seed used and the
seeds refused are recorded, and so is the number of colour channels that are denormals (the example's plastics
with exponent 128 and pure diffuse colours have some: a blinn term below FLT_MIN in a channel without a
diffuse part -- the tests' relative bar applies to them as to every other value).

The .npz files are written with fixed zip timestamps, so a second run reproduces them byte for byte.
"""
import argparse
import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import visionaray_amd as va  # noqa: E402
from gp_cases import random_plastics, sweep_camera, sweep_scene, sweep_shading  # noqa: E402
from make_pathtrace_golden import save_npz  # noqa: E402

BIN = os.path.join(ROOT, "oracle", "_ref", "generic_primitive_ref")
W, H = 60, 44
MISS = 0xFFFFFFFF
BG = (0.1, 0.2, 0.3, 1.0)
AMBIENT = (1.0, 1.0, 1.0, 1.0)
AO_SAMPLES, AO_EPS = 8, 1e-3
MIN_SHARE = 0.05
# case, first seed
CASES = [("gp_example", 100), ("gp_soup", 200), ("gp_inside", 300), ("gp_sweep", 400)]


def compile_generator(ref):
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.run(["g++", "-std=c++14", "-O2", "-msse4.1", "-ffp-contract=off", "-w",
                    "-I" + os.path.join(ref, "include"), os.path.join(HERE, "generic_primitive_ref.cpp"), "-o", BIN],
                   check=True)


def camera_basis(eye, center, fovy):
    cam = va.camera()
    cam.perspective(float(fovy), np.float32(W) / np.float32(H), 0.001, 1000.0)
    cam.look_at(tuple(float(x) for x in eye), tuple(float(x) for x in center))
    b = cam.basis(W, H)
    return np.float32([list(b.eye), list(b.cam_u), list(b.cam_v), list(b.cam_w)])


def example_scene(seed):
    """src/examples/generic_primitive/main.cpp generate_frame() at animation frame seed - 100"""
    f = np.float32
    y = f(-0.5)
    for _ in range(seed - 100 + 1):
        y = f(y + f(f(0.2) * f(0.1)))
    p1 = [[(-1, -1, 1), (1, -1, 1), (0, 1, 0)], [(1, -1, 1), (1, -1, -1), (0, 1, 0)], [(1, -1, -1), (-1, -1, -1), (0, 1, 0)],
          [(-1, -1, -1), (-1, -1, 1), (0, 1, 0)], [(1, -1, 1), (-1, -1, 1), (1, -1, -1)], [(-1, -1, 1), (-1, -1, -1), (1, -1, -1)]]
    a, b, c, d, top = (0.3, 0.3, 0.7), (0.7, 0.3, 0.7), (0.7, 0.3, 0.3), (0.3, 0.3, 0.3), (0.5, 0.7, 0.5)
    p2 = [[a, b, top], [b, c, top], [c, d, top], [d, a, top], [b, a, c], [a, d, c]]
    v = np.array(p1 + p2, dtype=f)                      # the example's double literals, rounded to float as vec3(...) does
    tris = va.make_triangles(v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0], prim_id=np.arange(12), geom_id=[0] * 6 + [1] * 6)
    sph = va.make_spheres([[f(-0.7), y, f(0.8)], [f(1.0), f(0.8), f(-0.0)]], [f(0.5), f(0.3)], prim_id=[12, 13], geom_id=[2, 3])
    prims = va.make_generic(tris, sph)
    mats = np.stack([va.plastic(ca=(0, 0, 0), ka=1, cd=(0, 1, 1), kd=1, cs=(0.2, 0.4, 0.4), ks=1, exp=16.0),
                     va.plastic(ca=(0, 0, 0), ka=1, cd=(1, 0, 0), kd=1, cs=(0.5, 0.2, 0.2), ks=1, exp=128.0),
                     va.plastic(ca=(0, 0, 0), ka=1, cd=(0, 0, 1), kd=1, cs=(1, 1, 1), ks=1, exp=128.0),
                     va.plastic(ca=(0, 0, 0), ka=1, cd=(1, 1, 1), kd=1, cs=(1, 1, 1), ks=1, exp=32.0)])
    lights = np.stack([va.point_light((0.0, 10.0, 10.0), cl=(1, 1, 1), kl=1.0)])
    # camera::view_all(aabb((-1, -1, 0), (1, 1, 2))), camera.inl:79-87, in float
    fovy = f(f(45.0) * f(va.DEGREES_TO_RADIANS))
    r = f(np.sqrt(f(12.0)) * f(0.5))
    eye = (0.0, 0.0, float(f(f(1.0) + f(r + f(r / np.arctan(fovy))))))
    basis = camera_basis(eye, (0.0, 0.0, 1.0), float(fovy))
    return prims, tris, mats, lights, basis, dict(bounces=4, eps=1e-4, ao_radius=0.5, sphere_y=float(y))


def random_tris(rng, n, spread, lo, hi):
    c = rng.uniform(-spread, spread, (n, 3))
    size = 10.0 ** rng.uniform(lo, hi, (n, 1))
    f1, f2 = rng.standard_normal((n, 3)) * size, rng.standard_normal((n, 3)) * size
    return c - 0.5 * (f1 + f2), f1, f2


def soup_scene(seed):
    rng = np.random.default_rng(seed)
    nt, ns = 150, 150
    order = rng.permutation(np.concatenate([np.zeros(nt, np.uint8), np.ones(ns, np.uint8)]))
    ids = np.arange(nt + ns, dtype=np.uint32)
    v1, e1, e2 = random_tris(rng, nt, 0.9, -1.0, -0.4)
    tris = va.make_triangles(v1, e1, e2, prim_id=ids[order == 0], geom_id=ids[order == 0] % 4)
    sph = va.make_spheres(rng.uniform(-0.9, 0.9, (ns, 3)), 10.0 ** rng.uniform(-1.4, -0.8, ns), prim_id=ids[order == 1],
                          geom_id=ids[order == 1] % 4)
    prims = va.make_generic(tris, sph, order)
    lights = np.stack([va.point_light((0.5, 3.0, 2.5), cl=(1, 1, 1), kl=1.0),
                       va.point_light((-2.5, 1.0, 0.5), cl=(1.0, 0.8, 0.6), kl=0.7, constant_att=1.0, linear_att=0.1, quadratic_att=0.05)])
    d = rng.standard_normal(3)
    basis = camera_basis(3.0 * d / np.linalg.norm(d), (0.0, 0.0, 0.0), rng.uniform(0.7, 0.9))
    return prims, tris, random_plastics(rng, 4), lights, basis, dict(bounces=4, eps=1e-3, ao_radius=0.3)


def inside_scene(seed):
    rng = np.random.default_rng(seed)
    nt, ns = 10, 8
    v1, e1, e2 = random_tris(rng, nt, 1.2, -0.5, -0.1)
    tris = va.make_triangles(v1, e1, e2, prim_id=np.arange(1, 1 + nt), geom_id=np.arange(1, 1 + nt) % 3)
    centers = np.concatenate([[[0.0, 0.0, 0.0]], rng.uniform(-1.2, 1.2, (ns, 3))])
    radii = np.concatenate([[3.0], 10.0 ** rng.uniform(-0.8, -0.4, ns)])
    sid = np.concatenate([[0], np.arange(1 + nt, 1 + nt + ns)]).astype(np.uint32)
    sph = va.make_spheres(centers, radii, prim_id=sid, geom_id=sid % 3)
    order = np.concatenate([[1], np.zeros(nt, np.uint8), np.ones(ns, np.uint8)])
    prims = va.make_generic(tris, sph, order)
    lights = np.stack([va.point_light(tuple(rng.uniform(-0.5, 0.5, 3)), cl=(1, 1, 1), kl=1.0, constant_att=1.0, linear_att=0.2,
                                      quadratic_att=0.1)])
    eye = rng.uniform(-1.8, 1.8, 3)
    while not 1.6 < np.linalg.norm(eye) < 2.4:          # inside the large sphere, outside the cluster
        eye = rng.uniform(-1.8, 1.8, 3)
    basis = camera_basis(eye, rng.uniform(-0.3, 0.3, 3), rng.uniform(0.8, 1.1))
    return prims, tris, random_plastics(rng, 3), lights, basis, dict(bounces=3, eps=1e-3, ao_radius=0.5)


def sweep_fixture_scene(seed):
    rng = np.random.default_rng(seed)
    prims, tris, _ = sweep_scene(rng, 160, 120)
    b = sweep_camera(rng, W, H, inside=True).basis(W, H)
    basis = np.float32([list(b.eye), list(b.cam_u), list(b.cam_v), list(b.cam_w)])
    mats, lights = sweep_shading(rng)
    return prims, tris, mats, lights, basis, dict(bounces=int(rng.integers(2, 6)), eps=float(rng.choice([1e-3, 1e-4])),
                                                  ao_radius=float(np.float32(10.0 ** rng.uniform(-1.0, 0.0))))


SCENES = {"gp_example": example_scene, "gp_soup": soup_scene, "gp_inside": inside_scene, "gp_sweep": sweep_fixture_scene}


def run_ref(prims, normals, mats, lights, basis, spec):
    hdr = struct.pack("<8I", 0x50475246, W, H, len(prims), len(mats), len(lights), spec["bounces"], AO_SAMPLES)
    hdr += struct.pack("<3f4f4f", spec["eps"], spec["ao_radius"], AO_EPS, *BG, *AMBIENT) + np.ascontiguousarray(basis, np.float32).tobytes()
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "scene.bin"), os.path.join(d, "out.bin")
        with open(src, "wb") as f:
            f.write(hdr + np.ascontiguousarray(mats).tobytes() + np.ascontiguousarray(lights).tobytes()
                    + np.ascontiguousarray(prims).tobytes() + np.ascontiguousarray(normals, np.float32).tobytes())
        subprocess.run([BIN, src, dst], check=True)
        raw = open(dst, "rb").read()
    n, npx = len(prims), W * H
    nn = int(np.frombuffer(raw, np.uint32, 1)[0])
    off = 4
    out = {}

    def take(name, dtype, count, shape):
        nonlocal off
        out[name] = np.frombuffer(raw, dtype, count, off).reshape(shape).copy()
        off += count * np.dtype(dtype).itemsize
    take("nodes", np.uint32, nn * 8, (nn, 8))
    take("indices", np.uint32, n, (n,))
    take("prim_id", np.uint32, npx, (npx,))
    take("t", np.float32, npx, (npx,))
    take("occ", np.uint8, npx, (npx,))
    take("ao_color", np.float32, npx * 4, (npx, 4))
    take("simple_color", np.float32, npx * 4, (npx, 4))
    take("whitted_color", np.float32, npx * 4, (npx, 4))
    take("whitted_cross", np.uint8, npx, (npx,))
    assert off == len(raw)
    return out


def try_seed(case, seed):
    """(json record, npz arrays) of a case at one seed, or the reason the seed is refused"""
    prims, tris, mats, lights, basis, spec = SCENES[case](seed)
    n = len(prims)
    normals = np.zeros((n, 4), np.float32)
    normals[tris["prim_id"]] = va.face_normals(tris)      # a sphere's row is never read
    ref = run_ref(prims, normals, mats, lights, basis, spec)
    is_sphere = np.zeros(n, bool)
    sph_rows = prims["type"] == va.GENERIC_TYPE_SPHERE
    ids = np.ascontiguousarray(prims["data"]).view(np.uint32).reshape(n, 16)[:, 1]
    is_sphere[ids[sph_rows]] = True
    nodes = ref["nodes"]
    mixed = 0
    for first, count in zip(nodes[:, 3], nodes[:, 7]):
        if count:
            kinds = sph_rows[ref["indices"][first:first + count]]
            mixed += int(kinds.any() and not kinds.all())
    pid = ref["prim_id"]
    hit = pid != MISS
    share_s = float(np.mean(hit & is_sphere[np.where(hit, pid, 0)]))
    share_t = float(np.mean(hit & ~is_sphere[np.where(hit, pid, 0)]))
    if mixed == 0:
        return "no leaf holds both kinds"
    if share_s < MIN_SHARE or share_t < MIN_SHARE:
        return "closest-hit shares: triangles %.3f, spheres %.3f" % (share_t, share_s)
    if hit.all():
        return "no pixel misses"
    if not ref["occ"].any():
        return "no AO ray is occluded"
    if not ref["whitted_cross"].any():
        return "no whitted path reflects across kinds"
    if not all(np.isfinite(ref[k]).all() for k in ("ao_color", "simple_color", "whitted_color")):
        return "a non-finite colour"
    denormals = {k: int(((np.abs(ref[k]) < np.finfo(np.float32).tiny) & (ref[k] != 0.0)).sum()) for k in ("simple_color", "whitted_color")}
    arrays = dict(ref)
    arrays.update(prims=np.ascontiguousarray(prims).view(np.uint32).reshape(n, 20), normals=normals,
                  materials=np.ascontiguousarray(mats).view(np.float32).reshape(len(mats), 13),
                  lights=np.ascontiguousarray(lights).view(np.float32).reshape(len(lights), 10), camera=basis)
    rec = {"seed": seed, "W": W, "H": H, "num_prims": n, "num_spheres": int(sph_rows.sum()), "num_nodes": len(nodes),
           "bounces": spec["bounces"], "eps": spec["eps"], "ao_samples": AO_SAMPLES, "ao_radius": spec["ao_radius"], "ao_eps": AO_EPS,
           "bg": list(BG), "ambient": list(AMBIENT), "mixed_leaves": mixed, "triangle_share": share_t, "sphere_share": share_s,
           "miss_share": float(np.mean(~hit)), "occluded_rays": int(np.unpackbits(ref["occ"]).sum()),
           "cross_pixels": int(ref["whitted_cross"].sum()), "denormal_channels": denormals}
    if "sphere_y" in spec:
        rec["sphere_y"] = spec["sphere_y"]
    return rec, arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    if not os.path.exists(os.path.join(args.ref, "include", "visionaray", "generic_primitive.h")):
        sys.exit("make_generic_primitive_golden: the reference tree is not here")
    compile_generator(args.ref)
    out = {}
    for case, seed0 in CASES:
        refused = []
        for seed in range(seed0, seed0 + 50):
            got = try_seed(case, seed)
            if not isinstance(got, str):
                break
            refused.append([seed, got])
            print(case, "seed", seed, "refused:", got, flush=True)
        else:
            sys.exit(case + ": no usable seed")
        rec, arrays = got
        rec["refused_seeds"] = refused
        path = os.path.join(HERE, case + ".npz")
        save_npz(path, **arrays)
        rec["bytes"] = os.path.getsize(path)
        out[case] = rec
        print(case, json.dumps(rec), flush=True)
    with open(os.path.join(HERE, "generic_primitive.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
