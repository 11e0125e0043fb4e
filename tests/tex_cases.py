"""Shared inputs of the texture tests and of tests/golden/make_textured_golden.py: the textures, filters,
address-mode pairs and coordinates of tests/golden/tex2d_samples.npz, all derived from integer hashes (no
library random generator: the same arrays on every machine and numpy version).

A configuration is (W, H, filter, address x, address y); its key in the fixture is config_key().  Its
coordinates are 256 points uniform in [-3, 3]^2 followed by the edge list of the x axis crossed with
the edge list of the y axis.
"""
import numpy as np

SIZES = [(1, 1), (2, 2), (5, 3), (16, 16), (64, 37)]          # (W, H)
FILTERS = [0, 1]                                              # nearest, linear
ADDRESS = [(0, 0), (1, 1), (2, 2), (0, 2), (1, 0)]            # wrap 0, mirror 1, clamp 2: (x, y)
NUM_RANDOM = 256
MAX_COORD = float(2 ** 20)


def wang(a):
    """the project's counter hash (vrh_sampler.h wang), vectorised over uint32"""
    a = np.asarray(a, dtype=np.uint64) & 0xFFFFFFFF
    a = (a ^ 61) ^ (a >> 16)
    a = (a + (a << 3)) & 0xFFFFFFFF
    a = a ^ (a >> 4)
    a = (a * 0x27D4EB2D) & 0xFFFFFFFF
    a = a ^ (a >> 15)
    return a.astype(np.uint32)


def uniform01(k):
    return (wang(k) >> 8).astype(np.float32) * np.float32(1.0 / 16777216.0)


def configs():
    return [(w, h, f, ax, ay) for (w, h) in SIZES for f in FILTERS for (ax, ay) in ADDRESS]


def config_key(w, h, f, ax, ay):
    return "%dx%d_f%d_a%d%d" % (w, h, f, ax, ay)


def texels(w, h, seed=0):
    """(H, W, 4) uint8 texels of the W x H texture"""
    n = w * h * 4
    k = np.arange(n, dtype=np.uint64) + ((seed * 7919 + w * 131 + h) << 12)
    return (wang(wang(k)) >> 11).astype(np.uint8).reshape(h, w, 4)


def edge_values(n):
    """the edge list of an axis of n texels, float32, duplicates removed (0.0 and -0.0 both kept)"""
    one = np.float32(1.0)
    vals = [0.0, -0.0, 1.0, -1.0, 2.0, 1e-8, -1e-8, -1e-30, float(np.nextafter(one, np.float32(0.0))),
            MAX_COORD - 0.7, -(MAX_COORD - 0.7)]
    for k in sorted({0, 1, n // 2, n - 1, n}):
        q = np.float32(k) / np.float32(n)
        vals += [float(q), float(np.nextafter(q, np.float32(-4.0))), float(np.nextafter(q, np.float32(4.0))),
                 float((np.float32(k) + np.float32(0.5)) / np.float32(n))]
    out, seen = [], set()
    for v in np.asarray(vals, np.float32):
        b = int(v.view(np.uint32))
        if b not in seen:
            seen.add(b)
            out.append(v)
    return np.asarray(out, np.float32)


def coords(w, h, seed=0):
    """(n, 2) float32 coordinates of a W x H texture: NUM_RANDOM random ones, then the edge cross"""
    base = (seed * 104729 + w * 1009 + h) << 10
    k = np.arange(NUM_RANDOM * 2, dtype=np.uint64) + base
    rnd = (uniform01(k) * np.float32(6.0) - np.float32(3.0)).reshape(NUM_RANDOM, 2)
    ex, ey = edge_values(w), edge_values(h)
    gx, gy = np.meshgrid(ex, ey, indexing="ij")
    edge = np.stack([gx.ravel(), gy.ravel()], axis=1)
    return np.ascontiguousarray(np.concatenate([rnd, edge]).astype(np.float32))


def unorm8_table():
    """unorm_to_float<8>: float(double(float(k)) / 255.0)"""
    return (np.arange(256, dtype=np.float32).astype(np.float64) / 255.0).astype(np.float32)
