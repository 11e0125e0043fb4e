"""Shared by the formatted render target tests: the fixtures of tests/golden/make_render_target_golden.py
(rt_pixels.npz: the reference's pixel pipeline step by step; rt_frame.npz: a whole reference frame), laid out on
images of any size, and the descriptors of their steps."""
import functools
import os

import numpy as np

import visionaray_amd as va

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MISS = 0xFFFFFFFF
CF = va.color_format
DF = va.depth_format
COLOR_FORMATS = {"rgba32f": CF.rgba32f, "rgb32f": CF.rgb32f, "rgba8": CF.rgba8, "rgb8": CF.rgb8}
DEPTH_FORMATS = {"none": DF.none, "depth32f": DF.depth32f, "depth24s8": DF.depth24_stencil8}
IDENTITY = np.eye(4, dtype=np.float32).reshape(16)


@functools.lru_cache(maxsize=None)
def pixels_fixture():
    return dict(np.load(os.path.join(GOLDEN, "rt_pixels.npz")))


@functools.lru_cache(maxsize=None)
def frame_fixture():
    return dict(np.load(os.path.join(GOLDEN, "rt_frame.npz")))


def tile(a, n):
    """the fixture's N pixel cases laid out on n pixels: pixel i is case i % N"""
    return a[np.arange(n) % len(a)]


def step_inputs(step, n):
    """staging colour, prim_id and t of n pixels for step `step` of the pixel fixture (the identity camera's ray
    of any pixel is (u, v, -1) + t (0, 0, 1), so the fixture's isect_pos.z = t - 1 is the ray's at the fixture's t)"""
    fx = pixels_fixture()
    hit = tile(fx["in_hit"][step], n) != 0
    prim_id = np.where(hit, np.arange(n, dtype=np.uint32) % 1000, MISS).astype(np.uint32)
    t = np.where(hit, tile(fx["in_t"][step], n), np.float32(-1.0)).astype(np.float32)
    return np.ascontiguousarray(tile(fx["in_color"][step], n)), prim_id, t


def step_desc(step, scissor=(0, 0, 0, 0), depth=True):
    """the vrh_resolve_desc of step `step`: store, or blend with 1 / frame_num, 1 - 1 / frame_num computed as the
    runtime does (float32)"""
    blend, frame = (int(x) for x in pixels_fixture()["steps"][step])
    s = np.float32(1.0) / np.float32(frame)
    d = np.float32(1.0) - s
    mats = dict(view=IDENTITY, proj=IDENTITY) if depth else {}
    return va.resolve_desc(blend=bool(blend), s=float(s) if blend else 1.0, d=float(d) if blend else 0.0, scissor=scissor,
                           frame_num=frame, **mats)


def expected(snapshot, cf_name, df_name, n):
    """the reference's buffers after snapshot `snapshot` (0: after the clears, k: after step k - 1) on n pixels, in
    the layout of hip_buffer_rt.download_formatted (RGB32F: three words compared)"""
    fx = pixels_fixture()
    out = {"color": tile(fx["out_" + cf_name][snapshot], n)}
    if df_name != "none":
        out["depth"] = tile(fx["out_" + df_name][snapshot], n)
    return out


def same(got, want, cf_name, df_name):
    """bit-for-bit comparison of download_formatted / rt_resolve_host output with expected()"""
    c = got["color"]
    if cf_name in ("rgba32f", "rgb32f"):
        c = c.view(np.uint32)[:, :want["color"].shape[1]]
    if not np.array_equal(c, want["color"]):
        return False
    if df_name != "none" and not np.array_equal(got["depth"].view(np.uint32), want["depth"]):
        return False
    return True


def prim_color(pid):
    """tests/golden/render_target_ref.cpp prim_color"""
    pid = pid.astype(np.uint32)

    def ch(v):
        return (v % np.uint32(37)).astype(np.float32) / np.float32(32.0) - np.float32(0.0625)
    c = np.stack([ch(pid * np.uint32(7) + np.uint32(1)), ch(pid * np.uint32(11) + np.uint32(5)), ch(pid * np.uint32(13) + np.uint32(9)),
                  (pid % np.uint32(5) + np.uint32(1)).astype(np.float32) / np.float32(4.0)], axis=1)
    c[pid == MISS] = np.float32([0.1, 0.2, 0.3, 1.0])
    return c.astype(np.float32)


def depth_in_doubles(view, proj, w, h, prim_id, t, jitter=False, frame_num=0):
    """The depth of every pixel written independently of vrh_pixel.h, in numpy doubles: the jitter draws as include/vrh.h
    states them for vrh_pixel_sampler (counter c = p * 2 + 0x632BE5AB + n * 0x68E31DA4, U the Appendix-A hash, jy = U(c) - 0.5,
    jx = U(c + 1) - 0.5), the ray of vrh_view_camera, (z + 1) / 2 of the hit point under proj * view.  view / proj: 4 x 4
    [row, col].  Agrees with the float32 arithmetic of the kernel to rounding (DEPTH_RTOL), not to the bit."""
    def uniform01(k):
        a = k.astype(np.uint32)
        a = (a ^ np.uint32(61)) ^ (a >> np.uint32(16))
        a = a + (a << np.uint32(3))
        a = a ^ (a >> np.uint32(4))
        a = a * np.uint32(0x27D4EB2D)
        a = a ^ (a >> np.uint32(15))
        return (a >> np.uint32(8)).astype(np.float64) / 16777216.0
    view, proj = np.asarray(view, np.float64), np.asarray(proj, np.float64)
    p = np.arange(w * h, dtype=np.uint64)
    x, y = (p % w).astype(np.float64), (p // w).astype(np.float64)
    if jitter:
        c = (p * 2 + 0x632BE5AB + (frame_num * 0x68E31DA4)) & 0xFFFFFFFF
        y = y + uniform01(c) - 0.5
        x = x + uniform01((c + 1) & 0xFFFFFFFF) - 0.5
    u, v = 2.0 * (x + 0.5) / w - 1.0, 2.0 * (y + 0.5) / h - 1.0
    inv = np.linalg.inv(view) @ np.linalg.inv(proj)
    near = inv @ np.stack([u, v, -np.ones_like(u), np.ones_like(u)])
    far = inv @ np.stack([u, v, np.ones_like(u), np.ones_like(u)])
    ori, far = near[:3] / near[3], far[:3] / far[3]
    d = (far - ori) / np.linalg.norm(far - ori, axis=0)
    pos = ori + d * np.asarray(t, np.float64)
    clip = proj @ (view @ np.vstack([pos, np.ones_like(u)]))
    depth = (clip[2] / clip[3] + 1.0) * 0.5
    return np.where(np.asarray(prim_id) == MISS, 1.0, depth)


# float32 against doubles: the depth of a hit at distance t from a camera with near plane zn moves by about
# (t / zn) ulps of t per ulp of the ray -- the tests' cameras (t <= 6, zn >= 0.2) stay well below this
DEPTH_ATOL = 2e-5
