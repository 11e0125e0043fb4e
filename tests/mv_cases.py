"""Shared by the multi-volume tests and tests/golden/make_multi_volume_golden.py: the fixture frames
tests/golden/mv_<case>.npz and the objects built from them.

A fixture holds, for n volumes: `voxels_<i>` (D, H, W), `transfunc_<i>` (N, 4), `vol_params` (n, 5: format, filter,
address x y z), `tf_params` (n, 2: filter, address), `entries` (n, 44 floats: the words of vrh_multi_volume_entry --
box min / max, coordinate sign / offset / extent, the inverse transform as the reference's inverse() returned
it, the plastic record), `kernel` (dt, shade_alpha, gradient_delta), `cutoff` (the double), `light` (10 floats),
`camera` (eye, cam_u, cam_v, cam_w), `look_at` (the camera it was made from: eye, center, up, fovy, aspect), and the reference's `color`, `hit`, `tmin`, `steps_px`, `total_steps` and
`counters` (total steps, steps inside two or more volumes, steps inside none, shaded samples, samples with
alpha >= shade_alpha and a zero gradient, rays ended by the cutoff).
"""
import ctypes as C
import os

import numpy as np

FRAMES = ["mv_example", "mv_formats", "mv_unshaded", "mv_inside", "mv_gap"]
FRAME_W, FRAME_H = 60, 44
RTOL = 1e-5                      # the project's bar for plastic::shade on the device (tests/test_gpu_shading.py)
HERE = os.path.dirname(os.path.abspath(__file__))


def load_frame(name):
    with np.load(os.path.join(HERE, "golden", name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def entries_of(words):
    """vrh_multi_volume_entry array of an (n, 44) float32 array"""
    from visionaray_amd import _capi
    w = np.ascontiguousarray(words, np.float32)
    assert w.ndim == 2 and w.shape[1] * 4 == C.sizeof(_capi.vrh_multi_volume_entry)
    return (_capi.vrh_multi_volume_entry * len(w)).from_buffer_copy(w.tobytes())


def camera_of(words, width=FRAME_W, height=FRAME_H):
    from visionaray_amd import _capi
    cam = _capi.vrh_camera()
    c = [float(x) for x in words]
    cam.eye[:], cam.cam_u[:], cam.cam_v[:], cam.cam_w[:] = c[0:3], c[3:6], c[6:9], c[9:12]
    cam.width, cam.height = width, height
    return cam


def kernel_of(kernel, cutoff, light):
    import visionaray_amd as va
    from visionaray_amd import _capi
    k = _capi.vrh_multi_volume_kernel_desc()
    k.dt, k.shade_alpha, k.gradient_delta = (float(x) for x in kernel)
    k.opacity_cutoff = va.api.float_not_below(float(cutoff))            # the fixture holds the example's double
    k.light = _capi.vrh_point_light.from_buffer_copy(np.ascontiguousarray(light, np.float32).tobytes())
    return k


def frame_objects(F, width=FRAME_W, height=FRAME_H):
    """(voxels, transfuncs, filters, addresses, entries, kernel descriptor, camera) of a fixture"""
    import visionaray_amd as va
    n = len(F["entries"])
    vox = [F["voxels_%d" % i] for i in range(n)]
    tfs = [va.transfunc(F["transfunc_%d" % i], int(F["tf_params"][i][0]), int(F["tf_params"][i][1])) for i in range(n)]
    filters = [int(F["vol_params"][i][1]) for i in range(n)]
    addresses = [tuple(int(a) for a in F["vol_params"][i][2:5]) for i in range(n)]
    return (vox, tfs, filters, addresses, entries_of(F["entries"]), kernel_of(F["kernel"], F["cutoff"][0], F["light"]),
            camera_of(F["camera"], width, height))


def check_frame(got, F, name, exact_rgb=False):
    """the bars: alpha, hit, tmin (and steps where given) bit for bit, rgb to RTOL -- bit for bit where no sample
    is shaded"""
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)      # noqa: E731
    hit = np.asarray(F["hit"]).astype(bool)
    assert np.array_equal(got["prim_id"] == 0, hit) and np.all(got["prim_id"][~hit] == 0xFFFFFFFF), name
    assert np.array_equal(bits(got["t"][hit]), bits(np.asarray(F["tmin"])[hit])) and np.all(got["t"][~hit] == -1.0), name
    if "steps_px" in got:
        assert np.array_equal(got["steps_px"], np.asarray(F["steps_px"]).astype(np.uint32)), name
    want = np.asarray(F["color"])
    bad = np.flatnonzero(bits(got["color"][:, 3]) != bits(want[:, 3]))
    assert bad.size == 0, f"{name}: alpha differs at {bad.size} pixels, first {bad[0]}: {got['color'][bad[0]]} != {want[bad[0]]}"
    if exact_rgb:
        bad = np.flatnonzero(np.any(bits(got["color"]) != bits(want), axis=1))
        assert bad.size == 0, f"{name}: {bad.size} pixels differ, first {bad[0]}: {got['color'][bad[0]]} != {want[bad[0]]}"
        return 0.0
    g, w = got["color"][:, :3].astype(np.float64), want[:, :3].astype(np.float64)
    rel = np.abs(g - w) / np.where(w != 0.0, np.abs(w), 1.0)
    rel[(w == 0.0) & (g == 0.0)] = 0.0
    worst = float(rel.max())
    print(f"{name}: largest relative rgb difference {worst:.3e}")
    assert np.all(np.abs(g - w) <= RTOL * np.abs(w)), f"{name}: rgb off by {worst:.3e} relative (bar {RTOL})"
    return worst
