#!/usr/bin/env python3
"""Fixtures of the texture support: tests/golden/tex2d_samples.npz, tests/golden/tex_<case>.npz and
tests/golden/textured.json.

Compiles tests/golden/textured_ref.cpp (the reference's own tex2D and its simple / whitted / pathtracing
kernels with the textured parameter pack, from the reference tree's headers) with g++ into oracle/_ref/
and runs it.  Runs only where the reference tree exists; nothing in build(), smoke(), bench.py or the tests
calls it.

    python tests/golden/make_textured_golden.py [--ref /path/to/reference]

tex2d_samples.npz: direct tex2D calls over the configurations and coordinates of tests/tex_cases.py.  Per
configuration `<key>` the packed RGBA8 samples (`<key>`, u32, 0 where dropped) and the kept flags
(`<key>_kept`, packed bits); `dropped` holds the number of dropped coordinates per configuration in
tex_cases.configs() order.  The driver stores the texels between guard texels and every configuration is
sampled twice, with guard bytes 0 and 255: a coordinate whose two results differ read outside the array
(undefined in the reference) and is dropped.  None of the random coordinates may be dropped.

Frames (60 x 44, partial 8 x 8 tiles on both edges): the rooms and soups of
make_generic_material_golden.py (geom_id = prim_id % materials) with random texture coordinates in
[-2.5, 3.5] and one texture per material -- sizes of tex_cases.SIZES, mixed filters and address modes, one
dummy.  Every frame is rendered twice with the two guard bytes; a seed whose two renders differ is refused,
as is one with a non-finite colour (a mirror path with dot(n, wi) == 0).  Each .npz is self-contained.
Bars: the path-traced cases without a specular plastic never reach powf (checked: the frame does not move
when powf moves by one float) and are compared bit for bit; `tex_path_plastic` gets rtol = 2 * sens as
make_pathtrace_golden.py derives it; simple / whitted radiance keeps the project's 1e-5.
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
import tex_cases as TC  # noqa: E402
import visionaray_amd as va  # noqa: E402
from make_generic_material_golden import BG, DARK, ENV, EPS, MAX_RTOL, MAX_UNSTABLE, MISS, H, W, draw_scene, rel_diff  # noqa: E402
from make_pathtrace_golden import save_npz  # noqa: E402
from oracle import oracle as O  # noqa: E402

BIN = os.path.join(ROOT, "oracle", "_ref", "textured_ref")
MAGIC = 0x54585246
GUARDS = (0, 255)
ALGO = {"simple": 0, "whitted": 1, "path": 2}

P5 = ("plastic", "plastic", "plastic", "plastic", "plastic")
D5 = ("diffuse", "diffuse", "diffuse", "diffuse", "diffuse")
G5 = ("matte", "emissive", "mirror", "diffuse", "matte")
# case, algorithm, family, materials, generic, ambient, lights, bounces, binding, frames or ("blend", first, count), first seed
CASES = [
    ("tex_simple_face", "simple", "room", P5, False, (0.6, 0.7, 0.8, 0.5), 3, 3, "face", [0], 1100),
    ("tex_simple_vertex", "simple", "soup", P5, False, (0.6, 0.7, 0.8, 0.5), 2, 3, "vertex", [0], 1200),
    ("tex_whitted_face", "whitted", "room", P5, False, (0.6, 0.7, 0.8, 0.5), 2, 3, "face", [0], 1300),
    ("tex_whitted_vertex", "whitted", "soup", P5, False, (0.6, 0.7, 0.8, 0.5), 3, 3, "vertex", [0], 1400),
    ("tex_path_diffuse", "path", "soup", D5, False, ENV, 0, 4, "face", [0, 1], 1500),
    ("tex_path_generic", "path", "room", G5, True, DARK, 0, 10, "face", [0], 1600),
    ("tex_path_generic_vertex", "path", "room", G5, True, DARK, 0, 5, "vertex", [0], 1700),
    ("tex_path_blend", "path", "room", G5, True, DARK, 0, 5, "face", ("blend", 1, 4), 1800),
    ("tex_path_plastic", "path", "soup", P5, False, ENV, 0, 4, "face", [0], 1900),
]


def compile_generator(ref):
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.run(["g++", "-std=c++14", "-O2", "-msse4.1", "-ffp-contract=off", "-fno-builtin-powf", "-w",
                    "-I" + os.path.join(ref, "include"), os.path.join(HERE, "textured_ref.cpp"), "-o", BIN, "-ldl"],
                   check=True)


def run_bin(payload):
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(src, "wb") as f:
            f.write(payload)
        subprocess.run([BIN, src, dst], check=True)
        return open(dst, "rb").read()


# ---- tex2D samples ---------------------------------------------------------------------------------

def sample_ref(texels, filt, ax, ay, coords, guard):
    h, w = texels.shape[:2]
    raw = run_bin(struct.pack("<9I", MAGIC, 0, w, h, filt, ax, ay, len(coords), guard) + texels.tobytes() + coords.tobytes())
    return np.frombuffer(raw, np.float32).reshape(len(coords), 4)


def pack_samples(vals):
    """the reference's normalised floats back to the 8-bit values they came from (exact table look-up)"""
    table = TC.unorm8_table()
    k = np.searchsorted(table, vals)
    assert np.array_equal(table[np.clip(k, 0, 255)], vals), "a tex2D result that is no unorm_to_float<8> value"
    k = k.astype(np.uint32)
    return k[:, 0] | k[:, 1] << 8 | k[:, 2] << 16 | k[:, 3] << 24


def make_samples():
    arrays, dropped = {}, []
    for (w, h, f, ax, ay) in TC.configs():
        texels, coords = TC.texels(w, h), TC.coords(w, h)
        a, b = (sample_ref(texels, f, ax, ay, coords, g) for g in GUARDS)
        kept = np.all(a.view(np.uint32) == b.view(np.uint32), axis=1)
        assert kept[:TC.NUM_RANDOM].all(), "a random coordinate read outside the array"
        packed = pack_samples(np.where(kept[:, None], a, np.float32(0.0)))
        key = TC.config_key(w, h, f, ax, ay)
        arrays[key] = np.where(kept, packed, 0).astype(np.uint32)
        arrays[key + "_kept"] = np.packbits(kept)
        dropped.append(int((~kept).sum()))
        print(key, "coords", len(coords), "dropped", dropped[-1], flush=True)
    arrays["dropped"] = np.asarray(dropped, np.uint32)
    path = os.path.join(HERE, "tex2d_samples.npz")
    save_npz(path, **arrays)
    print("tex2d_samples.npz", os.path.getsize(path), "bytes", flush=True)


# ---- frames ----------------------------------------------------------------------------------------

def plastic_record(rng, specular):
    return va.generic_materials(va.plastic(ca=rng.uniform(0.0, 1.0, 3), ka=rng.uniform(0.0, 1.0), cd=rng.uniform(0.2, 0.9, 3),
                                           kd=rng.uniform(0.4, 1.0), cs=rng.uniform(0.3, 1.0, 3),
                                           ks=rng.uniform(0.3, 0.8) if specular else 0.0, exp=32.0))[0]


def draw_case(seed, family, kinds, num_lights):
    """(triangles, material records, camera basis, lights, tex coords, texture list) of a case: a function of
    the seed alone.  A texture is (W, H, filter, address x, address y, texels); W = H = 0 is the dummy."""
    base = tuple("matte" if k in ("plastic", "diffuse") else k for k in kinds)
    prims, mats, basis = draw_scene(seed, family, base)
    rng = np.random.default_rng(seed + 77777)
    mats = mats.copy()
    for i, k in enumerate(kinds):
        if k in ("plastic", "diffuse"):
            mats[i] = plastic_record(rng, k == "plastic")
    lights = np.zeros(num_lights, va.POINT_LIGHT_DTYPE)
    for i in range(num_lights):
        lights[i] = va.point_light(rng.uniform(-0.8, 0.8, 3) if family == "room" else rng.uniform(-3.0, 3.0, 3),
                                   cl=rng.uniform(0.5, 1.0, 3), kl=rng.uniform(0.5, 1.0), constant_att=1.0,
                                   linear_att=rng.uniform(0.0, 0.2), quadratic_att=rng.uniform(0.0, 0.1))
    tc = rng.uniform(-2.5, 3.5, (3 * len(prims), 2)).astype(np.float32)
    dummy = int(rng.integers(0, len(kinds)))
    textures = []
    for i in range(len(kinds)):
        if i == dummy:
            textures.append((0, 0, 1, 0, 0, np.zeros((0, 0, 4), np.uint8)))
            continue
        w, h = TC.SIZES[(i + seed) % len(TC.SIZES)]
        ax, ay = TC.ADDRESS[int(rng.integers(0, len(TC.ADDRESS)))]
        textures.append((w, h, int(rng.integers(0, 2)), ax, ay, TC.texels(w, h, seed + i)))
    return prims, mats, basis, lights, tc, textures


def run_frame(algo, generic, prims, normals, per_vertex, mats, basis, lights, tc, textures, ambient, bounces, first_frame,
              accum, pow_shift, guard):
    """One run of the generator: (colour snapshots, first prim ids, first t, signatures, rays per pixel, total)"""
    hdr = struct.pack("<2I10Ii3I", MAGIC, 1, W, H, len(prims), int(per_vertex), len(mats), int(generic), ALGO[algo], bounces,
                      first_frame, accum, pow_shift, len(lights), len(textures), guard)
    hdr += struct.pack("<f4f4f", EPS, *BG, *ambient) + np.ascontiguousarray(basis, np.float32).tobytes()
    lt = np.zeros((len(lights), 10), np.float32)
    for i, l in enumerate(lights):
        lt[i] = list(l["position"]) + list(l["cl"]) + [l["kl"], l["constant_att"], l["linear_att"], l["quadratic_att"]]
    body = np.ascontiguousarray(mats).tobytes() + lt.tobytes() + np.ascontiguousarray(prims).tobytes() \
        + np.ascontiguousarray(normals, np.float32).tobytes() + np.ascontiguousarray(tc, np.float32).tobytes()
    for (w, h, f, ax, ay, texels) in textures:
        body += struct.pack("<5I", w, h, f, ax, ay) + texels.tobytes()
    raw = run_bin(hdr + body)
    n = W * H
    snaps = 2 if accum > 1 else 1
    colors = [np.frombuffer(raw, np.float32, n * 4, k * n * 16).reshape(n, 4).copy() for k in range(snaps)]
    off = snaps * n * 16
    pid = np.frombuffer(raw, np.uint32, n, off).copy()
    t = np.frombuffer(raw, np.float32, n, off + 4 * n).copy()
    sig = np.frombuffer(raw, np.uint64, n, off + 8 * n).copy()
    rays = np.frombuffer(raw, np.uint32, n, off + 16 * n).copy()
    total = int(np.frombuffer(raw, np.uint64, 1, off + 20 * n)[0])
    assert len(raw) == off + 20 * n + 8
    return colors, pid, t, sig, rays, total


def same_run(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a[0], b[0])) \
        and all(np.array_equal(a[i], b[i]) for i in (1, 3, 4)) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))


def try_seed(seed, algo, family, kinds, generic, ambient, num_lights, bounces, binding, frames):
    prims, mats, basis, lights, tc, textures = draw_case(seed, family, kinds, num_lights)
    fn = va.face_normals(prims)
    per_vertex = binding == "vertex"
    normals = O.vertex_normals(fn) if per_vertex else fn
    powf_free = algo == "path" and "plastic" not in kinds
    arrays = {"prims": np.ascontiguousarray(prims).view(np.uint32).reshape(len(prims), 16), "normals": fn,
              "materials": np.ascontiguousarray(mats).view(np.uint32).reshape(len(mats), 16), "camera": basis,
              "lights": np.ascontiguousarray(lights).view(np.float32).reshape(len(lights), 10), "tex_coords": tc,
              "tex_params": np.asarray([t[:5] for t in textures], np.uint32)}
    for i, t in enumerate(textures):
        arrays["tex%d" % i] = t[5]
    if per_vertex:
        arrays["vertex_normals"] = normals
    rec = {"algo": algo, "family": family, "seed": seed, "W": W, "H": H, "binding": binding, "materials": list(kinds),
           "generic": generic, "bounces": bounces, "eps": EPS, "ambient": list(ambient), "bg": list(BG), "num_prims": len(prims),
           "num_lights": num_lights, "powf_free": powf_free}
    blend = isinstance(frames, tuple)
    runs = [(frames[1], frames[2])] if blend else [(fr, 0) for fr in frames]
    if blend:
        rec.update(sampler="jittered_blend", first_frame=frames[1], num_frames=frames[2])
    else:
        rec.update(sampler="uniform", frames=list(frames), rays={})
    sens, unstable = 0.0, 0.0

    def go(first, accum, shift, guard):
        return run_frame(algo, generic, prims, normals, per_vertex, mats, basis, lights, tc, textures, ambient, bounces, first,
                         accum, shift, guard)

    for first, accum in runs:
        A = go(first, accum, 0, GUARDS[0])
        if not same_run(A, go(first, accum, 0, GUARDS[1])):
            return "a texel read outside its array (the two guard colours give two frames)"
        colors, pid, t, sig, rays, total = A
        if not all(np.isfinite(c).all() for c in colors):
            return "a non-finite colour"
        hit = pid != MISS
        if family == "soup" and not (hit.any() and (~hit).any()):
            return "no pixel that hits or none that misses"
        if algo == "path":
            B, Cc = go(first, accum, +1, GUARDS[0]), go(first, accum, -1, GUARDS[0])
            if powf_free:
                if not (same_run(A, B) and same_run(A, Cc)):
                    return "a powf-free case whose frame moves with powf"
                lightf = np.any(colors[0][:, :3] != 0.0, axis=1)
                if not (lightf.any() and (~lightf).any()):
                    return "no lit path or none that is dark"
            else:
                last = colors[-1]
                lit = last[:, 3] == 1.0
                stable = (sig == B[3]) & (sig == Cc[3])
                unstable = max(unstable, float(np.sum(lit & ~stable)) / max(1, int(np.sum(lit))))
                sel = stable & hit
                sens = max(sens, rel_diff(last[sel], B[0][-1][sel]), rel_diff(last[sel], Cc[0][-1][sel]))
                # the issue asks for a seed at which no pixel changes its path
                if unstable > 0.0 or not 2.0 * sens <= MAX_RTOL:
                    return "unstable share %.4f, rtol %.3e" % (unstable, 2.0 * sens)
        if blend:
            arrays["color_first"], arrays["color_last"] = colors
            rec["rays_total"] = total
        else:
            arrays["color_f%d" % first] = colors[0]
            rec["rays"][str(first)] = total
        arrays["prim_id"], arrays["t"], arrays["rays_px"] = pid, t, rays.astype(np.uint16)
        rec["hit_share"] = float(hit.mean())
    rec.update(sens=sens, rtol=2.0 * sens, unstable=unstable)
    return rec, arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--only", default="", help="samples | frames")
    args = ap.parse_args()
    if not os.path.exists(os.path.join(args.ref, "include", "visionaray", "texture", "texture.h")):
        sys.exit("make_textured_golden: the reference tree is not here")
    O.build()
    compile_generator(args.ref)
    if args.only != "frames":
        make_samples()
    if args.only == "samples":
        return
    out = {}
    for case, algo, family, kinds, generic, ambient, num_lights, bounces, binding, frames, seed0 in CASES:
        refused = []
        for seed in range(seed0, seed0 + 50):
            got = try_seed(seed, algo, family, kinds, generic, ambient, num_lights, bounces, binding, frames)
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
        print(case, json.dumps({k: v for k, v in rec.items() if k not in ("bg", "ambient")}), flush=True)
    with open(os.path.join(HERE, "textured.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
