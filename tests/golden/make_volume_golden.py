#!/usr/bin/env python3
"""Fixtures of the volume support: tests/golden/tex3d_samples.npz, tests/golden/vol_<case>.npz and
tests/golden/volume.json.

Compiles tests/golden/volume_ref.cpp (the reference's own tex3D / tex1D and the loop of its volume example
with scalar float rays, from the reference tree's headers) with g++ into oracle/_ref/ and runs it.  Runs only
where the reference tree exists; nothing in build(), smoke(), bench.py or the tests calls it.

    python tests/golden/make_volume_golden.py [--ref /path/to/reference] [--only samples|frames]

tex3d_samples.npz: direct tex3D / tex1D calls over the configurations and coordinates of tests/vol_cases.py.
Per configuration `<key>` the float bits of the samples (u32, 0 where dropped) and the kept flags
(`<key>_kept`, packed bits).  Every configuration is sampled twice, its arrays between guard texels of 0 and
of the format's largest value: a coordinate whose two results differ read outside the array (undefined in
the reference) and is dropped.  None of the random coordinates may be dropped; volume.json records the
dropped edge coordinates per configuration.

Frames (60 x 44, partial 8 x 8 tiles on both edges): each .npz is self-contained -- voxels, transfer
function, box, kernel parameters, camera basis, and the reference's colour, hit, tnear and steps per pixel
with their total.  Every frame is rendered with both guards; a seed is refused (and recorded) if the two
renders differ, a channel is not finite, the frame lacks a hitting or a missing pixel (except the two
eye-relative cases), fewer than 5 % of the hit pixels end by the cutoff or by tfar (the two linear 16^3 /
4096-entry cases), or the longest ray reaches the device's step limit.
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
import vol_cases as VC  # noqa: E402
import visionaray_amd as va  # noqa: E402
from make_pathtrace_golden import save_npz  # noqa: E402

BIN = os.path.join(ROOT, "oracle", "_ref", "volume_ref")
MAGIC = 0x564F4C52
GUARDS = (0, 1)
W, H = VC.FRAME_W, VC.FRAME_H
NEAREST, LINEAR = 0, 1
WRAP, MIRROR, CLAMP = 0, 1, 2
R8, R16, R32F = 0, 1, 2

# case -> volume (W, H, D), format, filter, address; transfer function size, filter, address, alpha scale; box; dt;
# flips; view ("out": eye outside looking at the box, "inside", "behind"); check of the 5 % shares; first seed
CASES = {
    "vol_example": dict(dims=(2, 2, 2), fmt=R32F, filt=NEAREST, addr=(CLAMP,) * 3, tf=(4, LINEAR, CLAMP, 0.08),
                        box=((-1, -1, -1), (1, 1, 1)), dt=0.01, flip=(False, True, True), view="out", shares=False, seed=100,
                        example=True),
    "vol_r8_wrap": dict(dims=(5, 7, 3), fmt=R8, filt=LINEAR, addr=(WRAP,) * 3, tf=(16, LINEAR, CLAMP, 0.05),
                        box=((-1, -1, -1), (1, 1, 1)), dt=0.01, flip=(False, True, True), view="out", shares=False, seed=200),
    "vol_r16_mirror": dict(dims=(6, 4, 9), fmt=R16, filt=LINEAR, addr=(MIRROR,) * 3, tf=(16, LINEAR, WRAP, 0.12),
                           box=((-1, -1, -1), (1, 1, 1)), dt=0.01, flip=(False, True, True), view="out", shares=False, seed=300),
    "vol_r32f_16": dict(dims=(16, 16, 16), fmt=R32F, filt=LINEAR, addr=(CLAMP,) * 3, tf=(256, LINEAR, CLAMP, 0.06),
                        box=((-1, -1, -1), (1, 1, 1)), dt=0.01, flip=(False, True, True), view="out", shares=True, seed=400),
    "vol_tf1": dict(dims=(5, 7, 3), fmt=R8, filt=NEAREST, addr=(CLAMP, WRAP, MIRROR), tf=(1, NEAREST, CLAMP, 0.03),
                    box=((-1, -1, -1), (1, 1, 1)), dt=0.01, flip=(False, True, True), view="out", shares=False, seed=500),
    "vol_tf4096": dict(dims=(16, 16, 16), fmt=R8, filt=LINEAR, addr=(CLAMP,) * 3, tf=(4096, LINEAR, CLAMP, 0.06),
                       box=((-1, -1, -1), (1, 1, 1)), dt=0.01, flip=(False, True, True), view="out", shares=True, seed=600),
    "vol_box": dict(dims=(6, 4, 9), fmt=R32F, filt=LINEAR, addr=(CLAMP, MIRROR, WRAP), tf=(64, LINEAR, MIRROR, 0.9),
                    box=((0.5, -2.0, 1.0), (3.5, -0.5, 2.0)), dt=0.07, flip=(True, False, True), view="out", shares=False, seed=700),
    "vol_inside": dict(dims=(6, 4, 9), fmt=R16, filt=LINEAR, addr=(CLAMP,) * 3, tf=(32, LINEAR, CLAMP, 0.04),
                       box=((-1, -1, -1), (1, 1, 1)), dt=0.01, flip=(False, True, True), view="inside", shares=False, seed=800),
    "vol_behind": dict(dims=(5, 7, 3), fmt=R8, filt=LINEAR, addr=(MIRROR, CLAMP, WRAP), tf=(8, NEAREST, WRAP, 0.05),
                       box=((-1, -1, -1), (1, 1, 1)), dt=0.01, flip=(False, True, True), view="behind", shares=False, seed=900),
}


def compile_generator(ref):
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.run(["g++", "-std=c++14", "-O2", "-msse4.1", "-ffp-contract=off", "-w",
                    "-I" + os.path.join(ref, "include"), os.path.join(HERE, "volume_ref.cpp"), "-o", BIN], check=True)


def run_bin(payload):
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(src, "wb") as f:
            f.write(payload)
        subprocess.run([BIN, src, dst], check=True)
        return open(dst, "rb").read()


# ---- samples ---------------------------------------------------------------------------------------

def make_samples():
    arrays, dropped = {}, {}
    for (w, h, d, fmt, f, a) in VC.configs():
        vox, c = VC.voxels(w, h, d, fmt), VC.coords(w, h, d)
        runs = [np.frombuffer(run_bin(struct.pack("<12I", MAGIC, 0, w, h, d, fmt, f, a[0], a[1], a[2], len(c), g) + vox.tobytes()
                                      + c.tobytes()), np.uint32) for g in GUARDS]
        kept = runs[0] == runs[1]
        assert kept[:VC.NUM_RANDOM].all(), "a random coordinate read outside the array"
        key = VC.config_key(w, h, d, fmt, f, a)
        arrays[key] = np.where(kept, runs[0], 0).astype(np.uint32)
        arrays[key + "_kept"] = np.packbits(kept)
        dropped[key] = np.flatnonzero(~kept).tolist()
    for (n, f, a) in VC.tf_configs():
        tf, c = VC.transfunc(n), VC.tf_coords(n)
        runs = [np.frombuffer(run_bin(struct.pack("<7I", MAGIC, 1, n, f, a, len(c), g) + tf.tobytes() + c.tobytes()),
                              np.uint32).reshape(len(c), 4) for g in GUARDS]
        kept = np.all(runs[0] == runs[1], axis=1)
        assert kept[:VC.NUM_RANDOM].all(), "a random coordinate read outside the transfer function"
        key = VC.tf_key(n, f, a)
        arrays[key] = np.where(kept[:, None], runs[0], 0).astype(np.uint32)
        arrays[key + "_kept"] = np.packbits(kept)
        dropped[key] = np.flatnonzero(~kept).tolist()
    path = os.path.join(HERE, "tex3d_samples.npz")
    save_npz(path, **arrays)
    print("tex3d_samples.npz", os.path.getsize(path), "bytes,", sum(len(v) for v in dropped.values()), "edge coordinates dropped",
          flush=True)
    return dropped


# ---- frames ----------------------------------------------------------------------------------------

def draw_camera(rng, case):
    lo, hi = (np.asarray(b, np.float64) for b in case["box"])
    centre, radius = (lo + hi) / 2, float(np.linalg.norm(hi - lo)) / 2
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    cam = va.camera()
    cam.perspective(45.0 * va.DEGREES_TO_RADIANS, W / H, 0.001, 1000.0)
    if case["view"] == "inside":
        eye = centre + (hi - lo) * rng.uniform(-0.2, 0.2, 3)
        cam.look_at(eye, eye + d, (0.0, 1.0, 0.0))
    elif case["view"] == "behind":
        eye = centre + d * radius * 2.5
        cam.look_at(eye, eye + d + rng.uniform(-0.1, 0.1, 3), (0.0, 1.0, 0.0))
    else:
        eye = centre + d * radius * rng.uniform(1.9, 2.4)
        cam.look_at(eye, centre + rng.uniform(-0.15, 0.15, 3) * radius, (0.0, 1.0, 0.0))
    return cam.basis(W, H)


def run_frame(case, vox, tf, kd, basis, guard):
    n, tf_filter, tf_address, _ = case["tf"]
    w, h, d = case["dims"]
    hdr = struct.pack("<2I", MAGIC, 2) + struct.pack(
        "<16I16fd12f", W, H, w, h, d, case["fmt"], case["filt"], *case["addr"], n, tf_filter, tf_address, guard,
        1 if case.get("example") else 0, 0, *kd.box_min, *kd.box_max, *kd.coord_sign, *kd.coord_offset, *kd.coord_extent,
        kd.dt, case["cutoff"], *basis.eye, *basis.cam_u, *basis.cam_v, *basis.cam_w)
    raw = run_bin(hdr + vox.tobytes() + tf.tobytes())
    px = W * H
    assert len(raw) == px * 28 + 8
    return (np.frombuffer(raw, np.float32, px * 4).reshape(px, 4).copy(), np.frombuffer(raw, np.uint32, px, px * 16).copy(),
            np.frombuffer(raw, np.float32, px, px * 20).copy(), np.frombuffer(raw, np.uint32, px, px * 24).copy(),
            int(np.frombuffer(raw, np.uint64, 1, px * 28)[0]))


def try_seed(name, case, seed):
    rng = np.random.default_rng(seed)
    w, h, d = case["dims"]
    n, tf_filter, tf_address, alpha = case["tf"]
    vox, tf = VC.voxels(w, h, d, case["fmt"], seed), VC.transfunc(n, seed, alpha)
    case["cutoff"] = 0.999
    kd = va.volume_kernel_desc(case["box"], case["dt"], case["cutoff"], case["flip"])
    basis = draw_camera(rng, case)
    A, B = (run_frame(case, vox, tf, kd, basis, g) for g in GUARDS)
    if not (all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(A[:4], B[:4])) and A[4] == B[4]):
        return "a texel read outside its array (the two guards give two frames)"
    color, hit, tnear, steps, total = A
    if not np.isfinite(color).all():
        return "a channel that is not finite"
    hits = hit != 0
    if case["view"] == "out" and not (hits.any() and (~hits).any()):
        return "no pixel that hits or none that misses"
    cut = hits & (color[:, 3] >= case["cutoff"])
    if case["shares"] and not (cut.sum() >= 0.05 * hits.sum() and (hits & ~cut).sum() >= 0.05 * hits.sum()):
        return "fewer than 5 %% of the hit pixels end by the cutoff or by tfar (%d of %d cut)" % (cut.sum(), hits.sum())
    cap = VC.device_cap(kd.box_min[:], kd.box_max[:], kd.dt)
    if not int(steps.max()) < cap:
        return "the longest ray reaches the device's step limit"
    arrays = {"voxels": vox, "transfunc": tf, "vol_params": np.asarray([case["fmt"], case["filt"], *case["addr"]], np.uint32),
              "tf_params": np.asarray([tf_filter, tf_address], np.uint32),
              "kernel": np.asarray([*kd.box_min, *kd.box_max, *kd.coord_sign, *kd.coord_offset, *kd.coord_extent, kd.dt], np.float32),
              "cutoff": np.asarray([case["cutoff"]], np.float64),
              "camera": np.asarray([*basis.eye, *basis.cam_u, *basis.cam_v, *basis.cam_w], np.float32),
              "color": color, "hit": hit.astype(np.uint8), "tnear": tnear, "steps_px": steps.astype(np.uint16)
              if steps.max() < 65536 else steps, "total_steps": np.asarray([total], np.uint64)}
    rec = {"seed": seed, "W": W, "H": H, "dims": list(case["dims"]), "format": case["fmt"], "tf_size": n, "view": case["view"],
           "dt": case["dt"], "hits": int(hits.sum()), "cut": int(cut.sum()), "to_tfar": int((hits & ~cut).sum()),
           "max_steps": int(steps.max()), "cap": cap, "total_steps": total, "negative_tnear": int((hits & (tnear < 0)).sum())}
    return rec, arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--only", default="", help="samples | frames")
    args = ap.parse_args()
    if not os.path.exists(os.path.join(args.ref, "include", "visionaray", "texture", "texture.h")):
        sys.exit("make_volume_golden: the reference tree is not here")
    compile_generator(args.ref)
    json_path = os.path.join(HERE, "volume.json")
    out = json.load(open(json_path)) if os.path.exists(json_path) else {}
    if args.only != "frames":
        out["dropped_edge_coordinates"] = make_samples()
    if args.only != "samples":
        frames = {}
        for name, case in CASES.items():
            refused = []
            for seed in range(case["seed"], case["seed"] + 50):
                got = try_seed(name, case, seed)
                if not isinstance(got, str):
                    break
                refused.append([seed, got])
                print(name, "seed", seed, "refused:", got, flush=True)
            else:
                sys.exit(name + ": no usable seed")
            rec, arrays = got
            rec["refused_seeds"] = refused
            path = os.path.join(HERE, name + ".npz")
            save_npz(path, **arrays)
            rec["bytes"] = os.path.getsize(path)
            frames[name] = rec
            print(name, json.dumps(rec), flush=True)
        out["frames"] = frames
    with open(json_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
