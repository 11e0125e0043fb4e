#!/usr/bin/env python3
"""What generic primitives (VRH_PRIM_GENERIC80) cost on one MI355X: ms / frame at 1920 x 1080, written to
profiles/generic/bench.json.

    python tools/generic_bench.py [--frames 20] [--warmup 3] [--repeats 3] [--out profiles/generic/bench.json]
                                  [--headline this.jsonl] [--headline-parent parent.jsonl]

Scenes and kernels:
  hf1M   as TRI64 and as GENERIC80 with all triangles: primary, AO, whitted.  The ratio is the price of the type test
         alone (plus what the generic instances give up: the overflow stack, 8 / 6 waves per SIMD).
  sph1M  as SPHERE48 and as GENERIC80 with all spheres: primary.
  mixed  a 512 x 512 heightfield with 100,000 spheres of radius 0.002-0.006 resting on it, GENERIC80: primary, AO, whitted.
Each figure: `--repeats` rounds, each the wall time of `--frames` synchronous frames after `--warmup` untimed ones,
divided by the frames; the minimum, the median and all rounds are kept.  The uploads alternate inside a round, so a
drift of the clocks falls on both sides of a ratio.  Ratios are of the medians, GENERIC80 / plain.

--headline / --headline-parent: files of `python bench.py --gpus 1` result lines (one per repeat) of this commit and
of the parent commit, taken in the same session on the same machine; they are copied into the output with the parent's
spread (max - min) as the margin and the verdict `this median >= parent median - margin`.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def headline(path):
    with open(path) as f:
        rows = [json.loads(ln) for ln in f if ln.strip().startswith("{")]
    return [r["value"] for r in rows], (rows[0]["unit"] if rows else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generic", "bench.json"))
    ap.add_argument("--headline")
    ap.add_argument("--headline-parent")
    a = ap.parse_args()
    import numpy as np
    import visionaray_amd as va
    from visionaray_amd import scenes

    ctx = va.Context(0)
    W, H = 1920, 1080
    m = np.zeros(3, va.PLASTIC_DTYPE)
    m[0] = ((0.2, 0.2, 0.2), 1.0, (0.8, 0.3, 0.2), 1.0, (1.0, 1.0, 1.0), 0.4, 32.0)
    m[1] = ((0.1, 0.1, 0.1), 0.5, (0.2, 0.7, 0.3), 0.9, (0.9, 0.9, 0.9), 0.2, 8.0)
    m[2] = ((0.05, 0.05, 0.1), 1.0, (0.3, 0.3, 0.9), 0.7, (1.0, 0.8, 0.6), 0.6, 64.5)
    lt = np.zeros(2, va.POINT_LIGHT_DTYPE)
    lt[0] = ((0.5, 2.0, 1.5), (1.0, 1.0, 1.0), 1.0, 1.0, 0.0, 0.0)
    lt[1] = ((-1.5, 1.0, 0.5), (1.0, 0.8, 0.6), 0.7, 1.0, 0.1, 0.05)
    sh = va.shading(ctx, m, lt)
    bg, amb = (0.1, 0.2, 0.3, 1.0), (0.4, 0.4, 0.4, 0.5)
    sched = va.hip_sched(ctx, async_frames=False)          # timed: frame() returns when the frame is done
    rt = va.hip_buffer_rt(ctx, W, H)

    def kernels(dev, names):
        k = {"primary": va.closest_hit_kernel(dev, bg=bg), "ao": va.ao_kernel(dev, samples=8, radius=0.1, eps=1e-3, bg=bg),
             "whitted": va.whitted_kernel(dev, sh, bg=bg, ambient=amb, num_bounces=4, epsilon=1e-3)}
        return {n: k[n] for n in names}

    def device(prims, tri_rows):
        """upload with the triangles' face normals at their prim ids"""
        normals = np.zeros((len(prims), 4), np.float32)
        if tri_rows is not None and len(tri_rows):
            normals[tri_rows["prim_id"]] = va.face_normals(tri_rows)
        return va.hip_index_bvh(ctx, va.build_index_bvh(prims), normals)

    def timed(k, sp):
        for _ in range(a.warmup):
            sched.frame(k, sp)
        t0 = time.perf_counter()
        for _ in range(a.frames):
            sched.frame(k, sp)
        return (time.perf_counter() - t0) * 1e3 / a.frames

    def measure(cam, sides, names):
        """sides: {label: device BVH}; -> {kernel: {label: {rounds, min, median}}}, the sides alternating per round"""
        sp = va.make_sched_params(va.pixel_sampler.uniform_type, cam, rt)
        ks = {lab: kernels(dev, names) for lab, dev in sides.items()}
        rounds = {n: {lab: [] for lab in sides} for n in names}
        for _ in range(a.repeats):
            for n in names:
                for lab in sides:
                    rounds[n][lab].append(timed(ks[lab][n], sp))
        return {n: {lab: {"ms_per_frame_rounds": v, "min": min(v), "median": statistics.median(v)} for lab, v in by.items()}
                for n, by in rounds.items()}

    def ratios(res, plain, generic="GENERIC80"):
        return {n: r[generic]["median"] / r[plain]["median"] for n, r in res.items()}

    out = {"what": "ms / frame at 1920 x 1080 on one MI355X, synchronous frames", "frames": a.frames, "warmup": a.warmup,
           "repeats": a.repeats}

    tris = scenes.primitives("hf1M")
    tris["geom_id"] = np.arange(len(tris), dtype=np.uint32) % 3
    cam, _, _ = scenes.scene_camera("hf1M", W, H)
    res = measure(cam, {"TRI64": device(tris, tris), "GENERIC80": device(va.make_generic(tris, None), tris)}, ["primary", "ao", "whitted"])
    out["hf1M"] = {"primitives": len(tris), "ms": res, "ratio_generic_over_tri64": ratios(res, "TRI64")}
    del tris

    sph = scenes.primitives("sph1M")
    cam, _, _ = scenes.scene_camera("sph1M", W, H)
    res = measure(cam, {"SPHERE48": device(sph, None), "GENERIC80": device(va.make_generic(None, sph), None)}, ["primary"])
    out["sph1M"] = {"primitives": len(sph), "ms": res, "ratio_generic_over_sphere48": ratios(res, "SPHERE48")}
    del sph

    grid = 512
    hf = np.zeros(2 * grid * grid, va.TRIANGLE_DTYPE)
    va._capi.check("vrh_gen_heightfield", grid, hf.ctypes.data_as(__import__("ctypes").c_void_p))
    hf["geom_id"] = np.arange(len(hf), dtype=np.uint32) % 3
    rng = np.random.default_rng(1)
    pick = rng.integers(0, len(hf), 100000)
    radius = rng.uniform(0.002, 0.006, len(pick)).astype(np.float32)
    centre = (hf["v1"][pick, :3] + (hf["e1"][pick, :3] + hf["e2"][pick, :3]) / np.float32(3.0)).astype(np.float32)
    centre[:, 1] += radius                                   # resting on the surface (y is up)
    ids = np.arange(len(hf), len(hf) + len(pick), dtype=np.uint32)
    sp_ = va.make_spheres(centre, radius, prim_id=ids, geom_id=ids % 3)
    cam, _, _ = scenes.scene_camera("hf1M", W, H)
    res = measure(cam, {"GENERIC80": device(va.make_generic(hf, sp_), hf)}, ["primary", "ao", "whitted"])
    out["mixed_hf512_100k_spheres"] = {"triangles": len(hf), "spheres": len(sp_), "ms": res}

    if a.headline and a.headline_parent:
        this, unit = headline(a.headline)
        parent, _ = headline(a.headline_parent)
        margin = max(parent) - min(parent)
        out["headline_bench_py"] = {"unit": unit, "this_commit": this, "parent_commit": parent, "margin_parent_spread": margin,
                                    "this_median": statistics.median(this), "parent_median": statistics.median(parent),
                                    "within_parent_spread": statistics.median(this) >= statistics.median(parent) - margin}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k.startswith("headline") or k in ("what",)}))
    for k in ("hf1M", "sph1M"):
        print(k, json.dumps({x: y for x, y in out[k].items() if x.startswith("ratio")}))


if __name__ == "__main__":
    main()
