"""Shared inputs of the volume tests and of tests/golden/make_volume_golden.py: the volumes, transfer
functions, filters, address modes and coordinates of tests/golden/tex3d_samples.npz, all derived from the
integer hashes of tex_cases.py (the same arrays on every machine and numpy version).

A tex3D configuration is (W, H, D, format, filter, (address x, y, z)); its key in the fixture is
config_key().  The three axes are mapped independently (map_tex_coord per axis), so the address triples put
every mode on every axis rather than crossing all 27.  Its coordinates are NUM_RANDOM points uniform in
[-2.5, 3.5]^3, then per axis that axis' edge list with the other two coordinates random, then the three
edge lists zipped.  A tex1D configuration is (N, filter, address), key tf_key().
"""
import numpy as np

from tex_cases import MAX_COORD, edge_values, uniform01, wang  # noqa: F401

SIZES = [(1, 1, 1), (2, 2, 2), (5, 7, 3), (6, 4, 9), (16, 16, 16)]      # (W, H, D): distinct dimensions catch swapped strides
FORMATS = [0, 1, 2]                                                     # R8, R16, R32F
DTYPES = {0: np.uint8, 1: np.uint16, 2: np.float32}
FILTERS = [0, 1]                                                        # nearest, linear
ADDRESS = [(0, 0, 0), (1, 1, 1), (2, 2, 2), (0, 1, 2), (2, 0, 1), (1, 2, 0)]   # wrap 0, mirror 1, clamp 2
TF_SIZES = [1, 2, 4, 256, 4096]
TF_ADDRESS = [0, 1, 2]
NUM_RANDOM = 128
FRAME_W, FRAME_H = 60, 44
MAX_STEPS = 65536


def configs():
    return [(w, h, d, fmt, f, a) for (w, h, d) in SIZES for fmt in FORMATS for f in FILTERS for a in ADDRESS]


def config_key(w, h, d, fmt, f, a):
    return "%dx%dx%d_t%d_f%d_a%d%d%d" % (w, h, d, fmt, f, a[0], a[1], a[2])


def tf_configs():
    return [(n, f, a) for n in TF_SIZES for f in FILTERS for a in TF_ADDRESS]


def tf_key(n, f, a):
    return "tf%d_f%d_a%d" % (n, f, a)


def voxels(w, h, d, fmt, seed=0):
    """(D, H, W) voxels: every byte / 16-bit value, or floats in [-0.3, 1.3) (the transfer function's
    coordinate: outside [0, 1] too)"""
    n = w * h * d
    k = np.arange(n, dtype=np.uint64) + ((seed * 7919 + w * 131 + h * 17 + d) << 14) + (fmt << 10)
    if fmt == 0:
        v = (wang(wang(k)) >> 11).astype(np.uint8)
    elif fmt == 1:
        v = (wang(wang(k)) >> 9).astype(np.uint16)
    else:
        v = uniform01(wang(k)) * np.float32(1.6) - np.float32(0.3)
    return np.ascontiguousarray(v.reshape(d, h, w))


def transfunc(n, seed=0, alpha=1.0):
    """(N, 4) float32 entries in [0, 1), the alpha channel scaled by `alpha`"""
    k = np.arange(n * 4, dtype=np.uint64) + ((seed * 6151 + n) << 13)
    t = uniform01(wang(k)).reshape(n, 4).copy()
    t[:, 3] *= np.float32(alpha)
    return np.ascontiguousarray(t.astype(np.float32))


def _random(count, base):
    k = np.arange(count, dtype=np.uint64) + base
    return uniform01(k) * np.float32(6.0) - np.float32(2.5)


def coords(w, h, d, seed=0):
    """(n, 3) float32 coordinates of a W x H x D volume: NUM_RANDOM random ones first"""
    base = (seed * 104729 + w * 1009 + h * 31 + d) << 12
    parts = [_random(NUM_RANDOM * 3, base).reshape(NUM_RANDOM, 3)]
    edges = [edge_values(n) for n in (w, h, d)]
    for axis in range(3):
        e = edges[axis]
        c = _random(len(e) * 3, base + 4096 * (axis + 1)).reshape(len(e), 3)
        c[:, axis] = e
        parts.append(c)
    m = max(len(e) for e in edges)
    parts.append(np.stack([np.resize(e, m) for e in edges], axis=1))
    return np.ascontiguousarray(np.concatenate(parts).astype(np.float32))


def tf_coords(n, seed=0):
    """float32 coordinates of an N-entry transfer function: NUM_RANDOM random ones, then the edge list"""
    base = (seed * 15485863 + n) << 11
    return np.ascontiguousarray(np.concatenate([_random(NUM_RANDOM, base), edge_values(n)]).astype(np.float32))


FRAMES = ["vol_example", "vol_r8_wrap", "vol_r16_mirror", "vol_r32f_16", "vol_tf1", "vol_tf4096", "vol_box", "vol_inside",
          "vol_behind"]
EYE_RELATIVE = ("vol_inside", "vol_behind")          # the eye inside the box / the box behind the eye
BOTH_ENDINGS = ("vol_r32f_16", "vol_tf4096")         # >= 5 % of the hit pixels end by the cutoff, >= 5 % by tfar


def load_frame(name):
    """the arrays of tests/golden/<name>.npz"""
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def frame_objects(F, width=FRAME_W, height=FRAME_H):
    """(transfunc, vrh_volume_kernel_desc, vrh_camera, filter, address) of a frame fixture, the camera for a
    width x height image of the same view"""
    import visionaray_amd as va
    from visionaray_amd import _capi
    tf = va.transfunc(F["transfunc"], int(F["tf_params"][0]), int(F["tf_params"][1]))
    k = _capi.vrh_volume_kernel_desc()
    v = [float(x) for x in F["kernel"]]
    k.box_min[:], k.box_max[:], k.coord_sign[:], k.coord_offset[:], k.coord_extent[:] = v[0:3], v[3:6], v[6:9], v[9:12], v[12:15]
    k.dt = v[15]
    k.opacity_cutoff = va.api.float_not_below(float(F["cutoff"][0]))     # the fixture holds the example's double
    cam = _capi.vrh_camera()
    c = [float(x) for x in F["camera"]]
    cam.eye[:], cam.cam_u[:], cam.cam_v[:], cam.cam_w[:] = c[0:3], c[3:6], c[6:9], c[9:12]
    cam.width, cam.height = width, height
    return tf, k, cam, int(F["vol_params"][1]), tuple(int(a) for a in F["vol_params"][2:5])


class fixed_camera:
    """a camera whose basis is given (hip_sched::frame asks sparams.cam for it)"""

    def __init__(self, basis):
        self._basis = basis

    def basis(self, width, height):
        assert (width, height) == (self._basis.width, self._basis.height)
        return type(self._basis).from_buffer_copy(self._basis)       # the caller sets its scissor box


def device_cap(box_min, box_max, dt):
    """the device's step limit 2 * ceil(diagonal / dt) + 8 (include/vrh.h vrh_render_volume), in doubles"""
    e = np.asarray(box_max, np.float32).astype(np.float64) - np.asarray(box_min, np.float32).astype(np.float64)
    return 2 * int(np.ceil(np.sqrt(np.sum(e * e)) / float(np.float32(dt)))) + 8
