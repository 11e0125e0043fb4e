#!/usr/bin/env python3
"""Fixtures of the built-in path tracer: tests/golden/pt_<case>.npz and tests/golden/pathtrace.json.

Compiles tests/golden/pathtrace_ref.cpp (the reference's own pathtracing::kernel, from the reference
tree's headers) with g++ into oracle/_ref/ and runs it on the scenes of oracle.gen_prims (geom ids
i % 3, face and vertex normals as the shading tests' product_scene).  Runs only where the reference
tree exists; nothing in build(), smoke(), bench.py or the tests calls it.

    python tests/golden/make_pathtrace_golden.py [--ref /path/to/reference]

Materials: `diffuse` = whitted_spec()'s three plastics with ks = 0 (prob_diff is exactly 1: no powf is
reached, the GPU frame must be bit-identical), `plastic` = whitted_spec()'s plastics unchanged.
Ambient (the environment light) is (1, 1, 1, 1), bg whitted_spec()'s.

Tolerance of the plastic cases (derived from the reference alone): each is rendered with the C
library's powf (A), with every powf result one float up (B) and one float down (C).  A pixel is
stable when its path signature (hit prim ids in order + number of rays) is the same in A, B and C;
sens = the largest relative colour difference A-B / A-C over stable pixels; rtol_spec = 2 * sens (two
powf implementations each within one ulp of the true value are at most two apart, and the response
is linear at that scale).  A case whose unstable share exceeds 0.25 % is refused.

The .npz files are written with fixed zip timestamps, so a second run reproduces them byte for byte.
"""
import argparse
import io
import json
import os
import struct
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402

BIN = os.path.join(ROOT, "oracle", "_ref", "pathtrace_ref")
EPS = 1e-3
AMBIENT = (1.0, 1.0, 1.0, 1.0)
PLASTIC_ULPS = 1          # the documented bound of the device powf this tolerance rests on
MAX_UNSTABLE = 0.0025
SIZE_LIMIT = 1 << 20

# case, scene, W, H, binding, materials, bounces, frames (uniform sampler) or ("blend", first, count)
CASES = [
    ("pt_cornell12_diffuse", "cornell12", 64, 64, "face", "diffuse", 4, [0, 2]),
    ("pt_hfstack_diffuse", "hfstack32x24", 96, 64, "face", "diffuse", 10, [0]),
    ("pt_hf64_vertex_diffuse", "hf64", 60, 44, "vertex", "diffuse", 3, [0, 1]),
    ("pt_cornell12_blend", "cornell12", 64, 64, "face", "diffuse", 4, ("blend", 1, 4)),
    ("pt_cornell12_plastic2", "cornell12", 64, 64, "face", "plastic", 2, [0]),
    ("pt_cornell12_plastic", "cornell12", 64, 64, "face", "plastic", 4, [0]),
]


def compile_generator(ref):
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.run(["g++", "-std=c++14", "-O2", "-msse4.1", "-ffp-contract=off", "-fno-builtin-powf", "-w",
                    "-I" + os.path.join(ref, "include"), os.path.join(HERE, "pathtrace_ref.cpp"), "-o", BIN, "-ldl"],
                   check=True)


def materials_of(kind):
    m, _, _, bg = O.whitted_spec()
    m = m.copy()
    if kind == "diffuse":
        m["ks"] = 0.0
    return m, bg


def scene_of(name):
    sc = O.make_shade_scene(name)          # geom_id = i % 3, face normals, vertex normals
    return sc.prims, sc.normals, sc.vertex_normals


def run_ref(scene, W, H, binding, mat_kind, bounces, first_frame, accum, pow_shift):
    """One run of the generator on a named scene: see run_ref_arrays."""
    prims, fn, vn = scene_of(scene)
    m, bg = materials_of(mat_kind)
    eye, u, v, w, _, _ = O.scene_camera(scene, W, H)
    per_vertex = binding == "vertex"
    return run_ref_arrays(prims, vn if per_vertex else fn, per_vertex, m, (eye, u, v, w), W, H, AMBIENT, bg, EPS,
                          bounces, first_frame, accum, pow_shift)


def run_ref_arrays(prims, normals, per_vertex, m, camera, W, H, ambient, bg, eps, bounces, first_frame, accum,
                   pow_shift):
    """One run of the generator: (colour snapshots, signatures, rays per pixel, closest_hit calls).
    prims: 64-byte triangle records; normals: float4 rows, one per triangle (three with per_vertex);
    m: plastic records (ca, ka, cd, kd, cs, ks, exp); camera: (eye, cam_u, cam_v, cam_w)."""
    hdr = struct.pack("<9Ii", 0x50545246, W, H, len(prims), int(per_vertex), len(m), bounces, first_frame, accum, pow_shift)
    hdr += struct.pack("<f4f4f", eps, *bg, *ambient)
    hdr += b"".join(np.asarray(a, np.float32).tobytes() for a in camera)
    mats = np.zeros((len(m), 13), np.float32)
    for i, r in enumerate(m):
        mats[i] = list(r["ca"]) + [r["ka"]] + list(r["cd"]) + [r["kd"]] + list(r["cs"]) + [r["ks"], r["exp"]]
    normals = np.ascontiguousarray(normals, np.float32)
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "scene.bin"), os.path.join(d, "out.bin")
        with open(src, "wb") as f:
            f.write(hdr + mats.tobytes() + np.ascontiguousarray(prims).tobytes() + normals.tobytes())
        subprocess.run([BIN, src, dst], check=True)
        raw = open(dst, "rb").read()
    n = W * H
    snaps = 2 if accum > 1 else 1
    colors = [np.frombuffer(raw, np.float32, n * 4, k * n * 16).reshape(n, 4).copy() for k in range(snaps)]
    off = snaps * n * 16
    sig = np.frombuffer(raw, np.uint64, n, off).copy()
    rays = np.frombuffer(raw, np.uint32, n, off + 8 * n).copy()
    total = int(np.frombuffer(raw, np.uint64, 1, off + 12 * n)[0])
    assert len(raw) == off + 12 * n + 8
    return colors, sig, rays, total


def save_npz(path, **arrays):
    """np.savez_compressed with fixed member timestamps (byte-for-byte reproducible)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    assert os.path.getsize(path) < SIZE_LIMIT, path


def rel_diff(a, b):
    """largest |a - b| / |a| over the rgb channels; channels that are 0 in a must be 0 in b"""
    a, b = a[:, :3].astype(np.float64), b[:, :3].astype(np.float64)
    zero = a == 0.0
    assert np.all(b[zero] == 0.0), "a channel that is 0 with libm's powf is not 0 with the moved powf"
    nz = ~zero
    return float(np.max(np.abs(a[nz] - b[nz]) / np.abs(a[nz]))) if nz.any() else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    if not os.path.exists(os.path.join(args.ref, "include", "visionaray", "detail", "pathtracing.inl")):
        sys.exit("make_pathtrace_golden: the reference tree is not here")
    O.build()
    compile_generator(args.ref)
    out = {}
    for case, scene, W, H, binding, mat, bounces, frames in CASES:
        _, bg = materials_of(mat)
        rec = {"scene": scene, "W": W, "H": H, "binding": binding, "materials": mat, "bounces": bounces, "eps": EPS,
               "ambient": list(AMBIENT), "bg": [float(x) for x in bg]}
        arrays = {}
        if isinstance(frames, tuple):
            _, first, count = frames
            colors, _, _, total = run_ref(scene, W, H, binding, mat, bounces, first, count, 0)
            arrays["color_first"], arrays["color_last"] = colors
            rec.update(sampler="jittered_blend", first_frame=first, num_frames=count, rays_total=total)
        else:
            rec.update(sampler="uniform", frames=frames, rays={})
            for fr in frames:
                colors, sig, rays, total = run_ref(scene, W, H, binding, mat, bounces, fr, 0, 0)
                arrays["color_f%d" % fr] = colors[0]
                rec["rays"][str(fr)] = total
                if mat == "plastic":
                    up, sig_up, _, _ = run_ref(scene, W, H, binding, mat, bounces, fr, 0, +PLASTIC_ULPS)
                    dn, sig_dn, _, _ = run_ref(scene, W, H, binding, mat, bounces, fr, 0, -PLASTIC_ULPS)
                    hit = rays > 0
                    lit = colors[0][:, 3] == 1.0            # to_rgba(dst): the primary ray hit
                    stable = (sig == sig_up) & (sig == sig_dn)
                    unstable_share = float(np.sum(lit & ~stable)) / max(1, int(np.sum(lit)))
                    if unstable_share > MAX_UNSTABLE:
                        sys.exit("%s: %.4f of the hit pixels change their path when powf moves by one float "
                                 "(cap %.4f): lower the bounce count or use another scene" % (case, unstable_share, MAX_UNSTABLE))
                    sel = stable & hit
                    sens = max(rel_diff(colors[0][sel], up[0][sel]), rel_diff(colors[0][sel], dn[0][sel]))
                    rec.update(powf_ulps=PLASTIC_ULPS, sens=sens, rtol_spec=2.0 * sens, unstable_share=unstable_share)
        save_npz(os.path.join(HERE, case + ".npz"), **arrays)
        rec["bytes"] = os.path.getsize(os.path.join(HERE, case + ".npz"))
        out[case] = rec
        print(case, json.dumps({k: v for k, v in rec.items() if k not in ("bg", "ambient")}), flush=True)
    with open(os.path.join(HERE, "pathtrace.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
