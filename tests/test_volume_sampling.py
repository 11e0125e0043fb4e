"""CPU: the shared volume samplers (include/visionaray_hip/detail/vrh_volume.h) through vrh_tex3d_host and
vrh_tex1d_host against the reference's own tex3D / tex1D.

tests/golden/tex3d_samples.npz holds direct calls of the reference (tests/golden/volume_ref.cpp, run by
make_volume_golden.py) over the volumes, formats, filters, address modes and coordinates of
tests/vol_cases.py.  Coordinates at which the reference read outside its array (found there with guard texels
of two values) are marked dropped: on those the sampler must still return a value from inside the array.
Everything else is compared bit for bit.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import visionaray_amd as va

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vol_cases as VC  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@functools.lru_cache(maxsize=None)
def samples():
    with np.load(os.path.join(HERE, "golden", "tex3d_samples.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def dropped():
    with open(os.path.join(HERE, "golden", "volume.json")) as f:
        return json.load(f)["dropped_edge_coordinates"]


def kept_flags(key, n):
    kept = np.unpackbits(samples()[key + "_kept"])[:n].astype(bool)
    assert kept[:VC.NUM_RANDOM].all(), "the fixture kept every random coordinate"
    assert np.flatnonzero(~kept).tolist() == dropped()[key], "volume.json lists the dropped coordinates"
    return kept


@pytest.mark.parametrize("cfg", VC.configs(), ids=lambda c: VC.config_key(*c))
def test_tex3d_host_equals_the_reference(cfg):
    w, h, d, fmt, f, a = cfg
    key = VC.config_key(*cfg)
    coords = VC.coords(w, h, d)
    kept = kept_flags(key, len(coords))
    got = va.tex3d_host(VC.voxels(w, h, d, fmt), coords, f, a).view(np.uint32)
    want = samples()[key]
    bad = np.flatnonzero(kept & (got != want))
    assert bad.size == 0, f"{key}: {bad.size} samples differ, first at {coords[bad[0]]}: {got[bad[0]]:08x} != {want[bad[0]]:08x}"


@pytest.mark.parametrize("cfg", VC.tf_configs(), ids=lambda c: VC.tf_key(*c))
def test_tex1d_host_equals_the_reference(cfg):
    n, f, a = cfg
    key = VC.tf_key(*cfg)
    coords = VC.tf_coords(n)
    kept = kept_flags(key, len(coords))
    got = va.transfunc(VC.transfunc(n), f, a).tex1d(coords).view(np.uint32)
    want = samples()[key]
    bad = np.flatnonzero(kept & np.any(got != want, axis=1))
    assert bad.size == 0, f"{key}: {bad.size} samples differ, first at {coords[bad[0]]}"


@pytest.mark.parametrize("fmt", VC.FORMATS)
def test_dropped_samples_read_inside_the_array(fmt):
    """On the coordinates the fixture dropped the sample must come from the array: a volume of one value
    samples to that value's result whatever the filter interpolates."""
    for (w, h, d, cfmt, f, a) in VC.configs():
        if cfmt != fmt:
            continue
        key = VC.config_key(w, h, d, cfmt, f, a)
        idx = dropped()[key]
        if not idx:
            continue
        coords = VC.coords(w, h, d)[idx]
        const = np.full((d, h, w), {0: 200, 1: 50000, 2: 0.75}[fmt], VC.DTYPES[fmt])
        want = va.tex3d_host(const, np.full((1, 3), 0.5, np.float32), 0, a)[0]
        got = va.tex3d_host(const, coords, f, a)
        # (1 - x) * c + x * c may round one ulp off c at each of the three lerp levels: the float format keeps
        # what the filter returns, the unorm formats truncate and must land within one step
        if fmt == 2:
            assert np.all(np.abs(got - want) <= 4 * np.spacing(np.float32(want))), key
        else:
            step = np.float32(1.0 / (255.0 if fmt == 0 else 65535.0))
            assert np.all(np.abs(got - want) <= step * np.float32(1.001)), key


def test_unorm16_normalisation_over_all_values():
    """unorm_to_float<16> = float(double(float(k)) / 65535.0) (math/detail/unorm.inl:26-31) on all 65536 inputs,
    through a nearest sample of a volume that holds every value once"""
    vox = np.arange(65536, dtype=np.uint16).reshape(16, 16, 256)
    z, y, x = np.meshgrid(np.arange(16), np.arange(16), np.arange(256), indexing="ij")
    coords = np.stack([(x.ravel() + 0.5) / 256.0, (y.ravel() + 0.5) / 16.0, (z.ravel() + 0.5) / 16.0], axis=1).astype(np.float32)
    got = va.tex3d_host(vox, coords, va.tex_filter.nearest, va.tex_address.clamp)
    want = (np.arange(65536, dtype=np.float32).astype(np.float64) / 65535.0).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_unorm8_normalisation_over_all_values():
    vox = np.arange(256, dtype=np.uint8).reshape(1, 1, 256)
    coords = np.stack([(np.arange(256) + 0.5) / 256.0, np.full(256, 0.5), np.full(256, 0.5)], axis=1).astype(np.float32)
    got = va.tex3d_host(vox, coords, va.tex_filter.nearest, va.tex_address.clamp)
    want = (np.arange(256, dtype=np.float32).astype(np.float64) / 255.0).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_volume_edge_check_program(flags, tmp_path):
    """tests/cpp/volume_edge_check.cpp: a stand-alone program over the shared header -- coordinates that map to
    index N, the index clamp, NaN box clips and the step limit -- plain and under the address and
    undefined-behaviour sanitizers"""
    exe = str(tmp_path / "volume_edge_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "include"),
                    os.path.join(HERE, "cpp", "volume_edge_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "volume_edge_check ok" in r.stdout
