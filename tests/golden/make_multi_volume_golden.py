#!/usr/bin/env python3
"""Fixtures of the multi-volume kernel: tests/golden/mv_<case>.npz and tests/golden/multi_volume.json.

Compiles tests/golden/multi_volume_ref.cpp (the loop of the reference's multi-volume example with scalar float
rays over the reference's own tex3D, tex1D, intersect, matrix, plastic<float>::shade, shade_record and
point_light, from the reference tree's headers) with g++ into oracle/_ref/ and runs it.  Runs only where the
reference tree exists; nothing in build(), smoke(), bench.py or the tests calls it.

    python tests/golden/make_multi_volume_golden.py [--ref /path/to/reference]

Frames are 60 x 44 (partial 8 x 8 tiles on both edges), volumes at most 16^3; each .npz is self-contained (layout:
tests/mv_cases.py).  Every case is rendered with the C library's powf (A, with both texel guards of
volume_ref.cpp), with every powf result one float up (B) and one float down (C).  Alpha, steps, hit and tmin
must be identical in A, B and C -- shading multiplies rgb only -- or the generator stops: the bars of the
tests rest on it.  The largest relative rgb difference between the three runs is recorded per case.

A seed is refused (and recorded) when the two guards give two frames, a channel is not finite, the longest
ray reaches the device's step limit, or the case lacks what it is there for (`need` below); no condition is
ever relaxed.
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
import mv_cases as MC  # noqa: E402
import vol_cases as VC  # noqa: E402
import visionaray_amd as va  # noqa: E402
from make_pathtrace_golden import save_npz  # noqa: E402

BIN = os.path.join(ROOT, "oracle", "_ref", "multi_volume_ref")
MAGIC = 0x4D564F4C
W, H = MC.FRAME_W, MC.FRAME_H
NEAREST, LINEAR = 0, 1
WRAP, MIRROR, CLAMP = 0, 1, 2
R8, R16, R32F = 0, 1, 2
UNIT_BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
PI = float(np.float32(3.14159265358979323846))

# the example's transfer functions (multi_volume/main.cpp:61-84)
EXAMPLE_TF = np.asarray([
    [0.0, 0.2, 0.8, 0.005], [1.0, 0.8, 0.0, 0.01], [0.0, 1.0, 0.0, 0.50], [1.0, 0.8, 0.0, 0.01], [1.0, 1.0, 1.0, 0.005],
    [1.0, 0.0, 0.0, 1.0], [1.0, 0.0, 0.0, 0.2], [1.0, 0.0, 0.0, 0.2], [1.0, 0.0, 0.0, 0.2], [1.0, 1.0, 1.0, 0.002],
    [1.0, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 0.50], [1.0, 1.0, 1.0, 0.50], [1.0, 1.0, 1.0, 0.50], [0.0, 0.0, 1.0, 0.002]],
    np.float32).reshape(3, 5, 4)
EXAMPLE_MATERIAL = dict(ca=(0.2, 0.2, 0.2), ka=1.0, cd=(0.8, 0.8, 0.8), kd=1.0, cs=(0.8, 0.8, 0.8), ks=1.0, exp=128.0)
AXES = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))


def vol(dims, fmt, filt, addr, tf, axis, angle, scaling, translation, box=UNIT_BOX, flip=(False, True, True), material=None,
        constant=None):
    """tf: (size, filter, address, alpha scale) or an (N, 4) array with (filter, address); constant: (axis, upto, value)
    fills the voxels below `upto` along `axis` with one value (a region whose gradient is 0)"""
    return dict(dims=dims, fmt=fmt, filt=filt, addr=addr, tf=tf, axis=axis, angle=angle, scaling=scaling, translation=translation,
                box=box, flip=flip, material=material, constant=constant)


# case -> volumes, kernel constants, view and what the case must show
CASES = {
    "mv_example": dict(
        example=True, dt=0.007, shade_alpha=0.1, delta=0.01, seed=100, view=("at", (2.5, 0.0, 0.0), 9.0), light="eye",
        volumes=[vol((9, 9, 9), R32F, LINEAR, (CLAMP,) * 3, (EXAMPLE_TF[i], NEAREST, CLAMP), AXES[i], PI / 4.0, (1.0, 1.0, 1.0),
                     (2.5 * i, 0.0, 0.0), material=EXAMPLE_MATERIAL, constant=(0, 4, 0.05) if i == 1 else None) for i in range(3)],
        need=("hit_and_miss", "shaded", "zero_gradient")),
    "mv_formats": dict(
        dt=0.02, shade_alpha=0.1, delta=0.01, seed=200, view=("at", (0.4, 0.1, 0.0), 6.5), light="near",
        volumes=[vol((5, 7, 3), R8, NEAREST, (CLAMP, WRAP, MIRROR), (16, LINEAR, CLAMP, 0.16), (1.0, 1.0, 0.0), 0.6, (1.0, 1.0, 1.0),
                     (-0.6, 0.0, 0.0)),
                 vol((6, 4, 9), R16, LINEAR, (MIRROR,) * 3, (64, LINEAR, WRAP, 0.12), (0.0, 1.0, 1.0), -0.9, (1.5, 0.7, 1.0),
                     (0.5, 0.2, 0.1), box=((-1.0, -0.5, -1.0), (0.5, 1.0, 1.0)), flip=(True, False, True)),
                 vol((16, 16, 16), R32F, LINEAR, (CLAMP,) * 3, (256, NEAREST, MIRROR, 0.2), (1.0, 0.0, 1.0), 1.2, (1.0, 1.0, 1.0),
                     (1.3, -0.2, 0.4))],
        need=("hit_and_miss", "shaded", "two_volumes", "shares")),
    "mv_unshaded": dict(
        dt=0.02, shade_alpha=0.1, delta=0.01, seed=300, view=("at", (0.5, 0.0, 0.0), 6.0), light="near",
        volumes=[vol((6, 4, 9), R16, LINEAR, (CLAMP,) * 3, (32, LINEAR, CLAMP, 0.09), (0.0, 0.0, 1.0), 0.5, (1.0, 1.0, 1.0),
                     (0.0, 0.0, 0.0)),
                 vol((5, 7, 3), R8, LINEAR, (CLAMP, MIRROR, CLAMP), (8, NEAREST, CLAMP, 0.09), (1.0, 0.0, 0.0), 0.8, (1.0, 1.2, 0.8),
                     (1.1, 0.3, 0.0))],
        need=("hit_and_miss", "two_volumes", "unshaded")),
    "mv_inside": dict(
        dt=0.02, shade_alpha=0.1, delta=0.01, seed=400, view=("inside",), light="near",
        volumes=[vol((6, 4, 9), R32F, LINEAR, (CLAMP,) * 3, (32, LINEAR, CLAMP, 0.15), (0.0, 1.0, 0.0), 0.4, (1.0, 1.0, 1.0),
                     (0.0, 0.0, 0.0)),
                 vol((5, 7, 3), R8, LINEAR, (CLAMP,) * 3, (16, LINEAR, CLAMP, 0.3), (1.0, 0.0, 0.0), 0.3, (0.5, 0.5, 0.5),
                     "behind")],
        need=("shaded", "negative_tmin")),
    "mv_gap": dict(
        dt=0.02, shade_alpha=0.1, delta=0.01, seed=500, view=("along", 7.0), light="near",
        volumes=[vol((5, 7, 3), R16, LINEAR, (CLAMP,) * 3, (16, LINEAR, CLAMP, 0.05), (0.0, 0.0, 1.0), 0.3, (1.0, 1.0, 1.0),
                     (0.0, 0.0, 0.0)),
                 vol((6, 4, 9), R32F, LINEAR, (CLAMP,) * 3, (16, LINEAR, CLAMP, 0.25), (0.0, 1.0, 0.0), 0.2, (1.0, 1.0, 1.0),
                     "row")],
        need=("hit_and_miss", "shaded", "no_volume")),
}


def compile_generator(ref):
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.run(["g++", "-std=c++14", "-O2", "-msse4.1", "-ffp-contract=off", "-fno-builtin-powf", "-w",
                    "-I" + os.path.join(ref, "include"), os.path.join(HERE, "multi_volume_ref.cpp"), "-o", BIN, "-ldl"], check=True)


def run_bin(payload):
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(src, "wb") as f:
            f.write(payload)
        subprocess.run([BIN, src, dst], check=True)
        return open(dst, "rb").read()


def draw_material(rng):
    return dict(ca=tuple(rng.uniform(0.0, 0.3, 3)), ka=1.0, cd=tuple(rng.uniform(0.2, 1.0, 3)), kd=float(rng.uniform(0.5, 1.0)),
                cs=tuple(rng.uniform(0.0, 1.0, 3)), ks=float(rng.uniform(0.1, 1.0)), exp=float(rng.choice([4.0, 16.0, 128.0])))


def draw_scene(case, seed):
    """the volumes' arrays and placements, the camera and the light of a seed"""
    rng = np.random.default_rng(seed)
    view = case["view"]
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    cam = va.camera()
    cam.perspective(45.0 * va.DEGREES_TO_RADIANS, W / H, 0.001, 1000.0)
    if view[0] == "at":
        centre = np.asarray(view[1])
        if case.get("example"):
            d = np.asarray([0.15, 0.25, 1.0]) / np.linalg.norm([0.15, 0.25, 1.0])
        eye = centre + d * view[2] * rng.uniform(0.95, 1.1)
        cam.look_at(eye, centre + rng.uniform(-0.1, 0.1, 3), (0.0, 1.0, 0.0))
    elif view[0] == "inside":
        eye = rng.uniform(-0.3, 0.3, 3)
        cam.look_at(eye, eye + d, (0.0, 1.0, 0.0))
    else:
        eye = -d * view[1]
        cam.look_at(eye, rng.uniform(-0.1, 0.1, 3), (0.0, 1.0, 0.0))
    vols = []
    for i, v in enumerate(case["volumes"]):
        w, h, dd = v["dims"]
        vox = VC.voxels(w, h, dd, v["fmt"], seed + i)
        if v["fmt"] == R32F:
            vox = np.clip(vox, 0.0, 1.0).astype(np.float32)
        if v["constant"] is not None:
            axis, upto, value = v["constant"]
            sl = [slice(None)] * 3
            sl[2 - axis] = slice(0, upto)
            vox[tuple(sl)] = value
        if isinstance(v["tf"][0], np.ndarray):
            tf, tf_filter, tf_address = v["tf"]
        else:
            n, tf_filter, tf_address, alpha = v["tf"]
            tf = VC.transfunc(n, seed + i, alpha)
        tr = v["translation"]
        if tr == "behind":            # wholly behind the eye: its box (half-size 0.5) lies 3 back along the view
            tr = tuple(eye - d * 3.0)
        elif tr == "row":             # behind the first volume along the view, with a gap between the two
            tr = tuple(d * 3.6)
        vols.append(dict(v, voxels=np.ascontiguousarray(vox), transfunc=np.ascontiguousarray(tf, np.float32), tf_filter=tf_filter,
                         tf_address=tf_address, translation=tuple(float(np.float32(x)) for x in tr),
                         material=v["material"] or draw_material(rng)))
    if case["light"] == "eye":
        light = va.point_light(eye)
    else:
        light = va.point_light(eye + rng.uniform(-1.0, 1.0, 3), cl=tuple(rng.uniform(0.6, 1.0, 3)), kl=float(rng.uniform(0.8, 1.2)),
                               constant_att=1.0, linear_att=0.05, quadratic_att=0.01)
    look_at = np.asarray([*cam.eye, *cam.center, *cam.up, cam.fovy, cam.aspect], np.float32)
    return vols, cam.basis(W, H), light, look_at


def run_frame(case, vols, basis, light, guard, pow_shift):
    lw = np.frombuffer(np.asarray(light).tobytes(), np.float32)
    payload = struct.pack("<6Ii I4fd10f12f", MAGIC, W, H, len(vols), guard, 1 if case.get("example") else 0, pow_shift, 0,
                          case["dt"], case["shade_alpha"], case["delta"], 0.0, case["cutoff"], *lw,
                          *basis.eye, *basis.cam_u, *basis.cam_v, *basis.cam_w)
    for v in vols:
        k = va.volume_kernel_desc(v["box"], 1.0, 1.0, v["flip"])
        m = v["material"]
        w, h, d = v["dims"]
        payload += struct.pack("<12I15f10f13f", w, h, d, v["fmt"], v["filt"], *v["addr"], len(v["transfunc"]), v["tf_filter"],
                               v["tf_address"], 0, *k.box_min, *k.box_max, *k.coord_sign, *k.coord_offset, *k.coord_extent,
                               *v["axis"], v["angle"], *v["scaling"], *v["translation"],
                               *m["ca"], m["ka"], *m["cd"], m["kd"], *m["cs"], m["ks"], m["exp"])
        payload += v["voxels"].tobytes() + v["transfunc"].tobytes()
    raw = run_bin(payload)
    n, px = len(vols), W * H
    assert len(raw) == n * 64 + px * 28 + 48
    o = n * 64
    return dict(minv=np.frombuffer(raw, np.float32, n * 16).reshape(n, 16).copy(),
                color=np.frombuffer(raw, np.float32, px * 4, o).reshape(px, 4).copy(),
                hit=np.frombuffer(raw, np.uint32, px, o + px * 16).copy(), tmin=np.frombuffer(raw, np.float32, px, o + px * 20).copy(),
                steps=np.frombuffer(raw, np.uint32, px, o + px * 24).copy(),
                counters=np.frombuffer(raw, np.uint64, 6, o + px * 28).copy())


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_frame(a, b, rgb):
    return (np.array_equal(bits(a["color"][:, 3]), bits(b["color"][:, 3])) and np.array_equal(a["hit"], b["hit"])
            and np.array_equal(bits(a["tmin"]), bits(b["tmin"])) and np.array_equal(a["steps"], b["steps"])
            and np.array_equal(a["counters"], b["counters"]) and (not rgb or np.array_equal(bits(a["color"]), bits(b["color"]))))


def world_distance(vols, A, basis):
    """D of the hang guard: from the eye to the farthest world-space box corner"""
    far = 0.0
    for i, v in enumerate(vols):
        m = A["minv"][i].astype(np.float64).reshape(4, 4).T            # [row, col]
        lin, b = np.linalg.inv(m[:3, :3]), m[:3, 3]
        lo, hi = (np.asarray(x, np.float64) for x in v["box"])
        for c in range(8):
            p = np.where([(c >> a) & 1 for a in range(3)], hi, lo)
            far = max(far, float(np.linalg.norm(lin @ (p - b) - np.asarray(basis.eye[:], np.float64))))
    return far


def try_seed(name, case, seed):
    vols, basis, light, look_at = draw_scene(case, seed)
    case["cutoff"] = 0.999
    A, A1 = (run_frame(case, vols, basis, light, g, 0) for g in (0, 1))
    if not same_frame(A, A1, True):
        return "a texel read outside its array (the two guards give two frames)"
    up, down = (run_frame(case, vols, basis, light, 0, s) for s in (1, -1))
    # the analysis the bars rest on: powf reaches rgb only
    assert same_frame(A, up, False) and same_frame(A, down, False), name + ": alpha, steps, hit or tmin move with powf"
    color, hit, tmin, steps, counters = A["color"], A["hit"] != 0, A["tmin"], A["steps"], [int(c) for c in A["counters"]]
    if not all(np.isfinite(r["color"]).all() for r in (A, up, down)):
        return "a channel that is not finite"
    for v in vols:
        m = v["material"]
        if not (np.all(np.asarray(m["cd"]) * m["kd"] > 0.0) and np.all(v["transfunc"] >= 0.0)):
            return "a material without a diffuse part in a channel, or a negative transfer-function colour"
    cap = 2 * int(np.ceil(2.0 * world_distance(vols, A, basis) / float(np.float32(case["dt"])))) + 8
    if not int(steps.max()) < cap:
        return "the longest ray reaches the device's step limit"
    total, multi, none, shaded, zero_grad, cut = counters
    need = case["need"]
    if "hit_and_miss" in need and not (hit.any() and (~hit).any()):
        return "no pixel that hits or none that misses"
    if "shaded" in need and shaded < 500:
        return "fewer than 500 shaded samples"
    if "zero_gradient" in need and zero_grad < 50:
        return "fewer than 50 samples with alpha >= shade_alpha and a zero gradient"
    if "two_volumes" in need and multi < 500:
        return "fewer than 500 steps inside two or more volumes"
    if "no_volume" in need and none < 500:
        return "fewer than 500 steps inside no volume"
    if "unshaded" in need and (shaded or zero_grad or not all(np.all(v["transfunc"][:, 3] < case["shade_alpha"]) for v in vols)):
        return "a sample that reaches shade_alpha"
    if "unshaded" in need and not (same_frame(A, up, True) and same_frame(A, down, True)):
        return "an unshaded frame that moves with powf"
    if "negative_tmin" in need and not (hit.all() and np.all(tmin < 0) and multi + none < total):
        return "a pixel whose march does not start behind the eye"
    if "shares" in need and not (cut >= 0.05 * hit.sum() and hit.sum() - cut >= 0.05 * hit.sum()):
        return "fewer than 5 %% of the hit rays end by the cutoff or by tmax (%d of %d cut)" % (cut, hit.sum())
    ref = np.abs(color[:, :3].astype(np.float64))
    sens = 0.0
    for other in (up, down):
        diff = np.abs(other["color"][:, :3].astype(np.float64) - color[:, :3].astype(np.float64))
        assert np.all(diff[ref == 0.0] == 0.0), "a channel that is 0 with libm's powf is not 0 with the moved powf"
        sens = max(sens, float((diff[ref > 0.0] / ref[ref > 0.0]).max()) if (ref > 0.0).any() else 0.0)
    n = len(vols)
    entries = np.zeros((n, 44), np.float32)
    for i, v in enumerate(vols):
        k = va.volume_kernel_desc(v["box"], 1.0, 1.0, v["flip"])
        m = v["material"]
        entries[i] = [*k.box_min, *k.box_max, *k.coord_sign, *k.coord_offset, *k.coord_extent, *A["minv"][i],
                      *m["ca"], m["ka"], *m["cd"], m["kd"], *m["cs"], m["ks"], m["exp"]]
    arrays = {"vol_params": np.asarray([[v["fmt"], v["filt"], *v["addr"]] for v in vols], np.uint32),
              "tf_params": np.asarray([[v["tf_filter"], v["tf_address"]] for v in vols], np.uint32), "entries": entries,
              "kernel": np.asarray([case["dt"], case["shade_alpha"], case["delta"]], np.float32),
              "cutoff": np.asarray([case["cutoff"]], np.float64), "light": np.frombuffer(np.asarray(light).tobytes(), np.float32),
              "camera": np.asarray([*basis.eye, *basis.cam_u, *basis.cam_v, *basis.cam_w], np.float32), "look_at": look_at,
              "color": color, "hit": hit.astype(np.uint8), "tmin": tmin, "steps_px": steps.astype(np.uint16) if steps.max() < 65536 else steps,
              "total_steps": np.asarray([total], np.uint64), "counters": A["counters"]}
    for i, v in enumerate(vols):
        arrays["voxels_%d" % i], arrays["transfunc_%d" % i] = v["voxels"], v["transfunc"]
    rec = {"seed": seed, "W": W, "H": H, "volumes": n, "dt": case["dt"], "hits": int(hit.sum()), "cut": cut, "to_tmax": int(hit.sum()) - cut,
           "max_steps": int(steps.max()), "cap": cap, "total_steps": total, "steps_in_two_or_more": multi, "steps_in_none": none,
           "shaded_samples": shaded, "zero_gradient_samples": zero_grad, "negative_tmin": int((hit & (tmin < 0)).sum()),
           "powf_rgb_sensitivity": sens}
    return rec, arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    if not os.path.exists(os.path.join(args.ref, "include", "visionaray", "texture", "texture.h")):
        sys.exit("make_multi_volume_golden: the reference tree is not here")
    compile_generator(args.ref)
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
    with open(os.path.join(HERE, "multi_volume.json"), "w") as f:
        json.dump({"frames": frames}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
