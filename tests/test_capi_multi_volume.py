"""CPU: the multi-volume part of the C-ABI (include/vrh.h) -- the ctypes structures have the sizes a C compiler
gives them, and every documented refusal of vrh_render_multi_volume is made without a device: the entries, the
kernel descriptor and the hang guard are checked before any object is looked at, and
vrh_multi_volume_render_host shares those checks."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import visionaray_amd as va
from visionaray_amd import _capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mv_cases as MC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = ["vrh_multi_volume_entry", "vrh_multi_volume_kernel_desc"]
UNIT_BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


def test_ctypes_struct_sizes_match_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "vrh.h"\nint main(void) {\n'
                   + "".join('  printf("%s %%zu\\n", sizeof(%s));\n' % (s, s) for s in STRUCTS)
                   + '  printf("max %u\\n", VRH_MULTI_VOLUME_MAX);\n  return 0;\n}\n')
    exe = str(tmp_path / "sizes")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = dict(line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    for s in STRUCTS:
        assert int(out[s]) == C.sizeof(getattr(_capi, s)), s
    assert C.sizeof(_capi.vrh_multi_volume_entry) == 44 * 4 and C.sizeof(_capi.vrh_multi_volume_kernel_desc) == 14 * 4
    assert int(out["max"]) == _capi.VRH_MULTI_VOLUME_MAX == 32


def scene(n=1, eye=(0.0, 0.0, 5.0)):
    """n unit boxes in a row along x, a camera at `eye` looking down -z, the example's kernel constants"""
    transforms = [np.eye(4, dtype=np.float32) for _ in range(n)]
    for i, t in enumerate(transforms):
        t[0, 3] = 0.1 * i
    entries = va.multi_volume_entries([UNIT_BOX] * n, [va.matrix_inverse(t) for t in transforms], [va.plastic()] * n)
    cam = MC.camera_of([*eye, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, -1.0], 8, 8)
    return entries, cam, va.multi_volume_kernel_desc(va.point_light(eye))


def device_call(entries, n, cam, k):
    """vrh_render_multi_volume without a context, volumes or target: (status, message)"""
    rc = _capi.lib().vrh_render_multi_volume(None, None, entries, n, None, C.byref(cam), C.byref(k))
    return rc, _capi.lib().vrh_last_error().decode()


def host_call(entries, n, cam, k):
    """vrh_multi_volume_render_host without volume descriptors: (status, message)"""
    rc = _capi.lib().vrh_multi_volume_render_host(None, None, entries, n, C.byref(cam), C.byref(k), None, None, None, None, None)
    return rc, _capi.lib().vrh_last_error().decode()


def refused(entries, n, cam, k, what):
    for call in (device_call, host_call):
        rc, msg = call(entries, n, cam, k)
        assert rc == _capi.VRH_ERR_INVALID and what in msg, f"{call.__name__}: status {rc} ({msg}), expected '{what}'"


def test_valid_descriptors_reach_the_object_checks():
    for n in (1, 3, 32):
        entries, cam, k = scene(n)
        rc, msg = device_call(entries, n, cam, k)
        assert rc == _capi.VRH_ERR_INVALID and "null context" in msg, msg
        rc, msg = host_call(entries, n, cam, k)
        assert rc == _capi.VRH_ERR_INVALID and "null volume" in msg, msg


@pytest.mark.parametrize("n", [0, 33, 1000])
def test_volume_count(n):
    entries, cam, k = scene(1)
    many = (_capi.vrh_multi_volume_entry * 40)(*[entries[0]] * 40)
    refused(many, n, cam, k, "1 to 32")


def test_null_entries_and_descriptors():
    entries, cam, k = scene(1)
    refused(None, 1, cam, k, "null entries")
    assert _capi.lib().vrh_render_multi_volume(None, None, entries, 1, None, None, C.byref(k)) == _capi.VRH_ERR_INVALID
    assert _capi.lib().vrh_render_multi_volume(None, None, entries, 1, None, C.byref(cam), None) == _capi.VRH_ERR_INVALID


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_transform_not_finite(bad):
    for at in (0, 5, 12, 15):
        entries, cam, k = scene(2)
        entries[1].transform_inv[at] = bad
        refused(entries, 2, cam, k, "volume 1: a transform that is not finite")


def test_transform_singular():
    entries, cam, k = scene(2)
    entries[0].transform_inv[:] = [1.0, 2.0, 3.0, 0.0, 2.0, 4.0, 6.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]      # two parallel columns
    refused(entries, 2, cam, k, "volume 0: a transform whose 3 x 3 part is singular")
    entries, cam, k = scene(1)
    entries[0].transform_inv[:] = [0.0] * 15 + [1.0]
    refused(entries, 1, cam, k, "singular")


def test_entry_fields():
    entries, cam, k = scene(1)
    entries[0].box_min[1] = 2.0
    refused(entries, 1, cam, k, "min > max")
    entries, cam, k = scene(1)
    entries[0].coord_sign[2] = 0.5
    refused(entries, 1, cam, k, "coordinate sign")
    entries, cam, k = scene(1)
    entries[0].coord_extent[0] = 0.0
    refused(entries, 1, cam, k, "coordinate extent")
    entries, cam, k = scene(1)
    entries[0].material.exp = float("nan")
    refused(entries, 1, cam, k, "material")


def test_kernel_fields():
    entries, cam, k = scene(1)
    k.shade_alpha = float("nan")
    refused(entries, 1, cam, k, "shade_alpha")
    entries, cam, k = scene(1)
    k.gradient_delta = float("inf")
    refused(entries, 1, cam, k, "gradient_delta")
    entries, cam, k = scene(1)
    k.light.position[0] = float("nan")
    refused(entries, 1, cam, k, "light")


@pytest.mark.parametrize("dt,what", [(float("nan"), "dt is not finite"), (float("inf"), "dt is not finite"), (0.0, "dt <= 0"),
                                     (-0.01, "dt <= 0")])
def test_hang_guard_dt(dt, what):
    entries, cam, k = scene(2)
    k.dt = dt
    refused(entries, 2, cam, k, what)


def test_hang_guard_distance():
    """D is the distance from the eye to the farthest world-space box corner: the unit box at the origin, scaled by
    2 in world space (transform_inv scales by 1/2), seen from (0, 0, 5): the corner (+-2, +-2, -2), D = sqrt(57)"""
    entries, cam, k = scene(1)
    entries[0].transform_inv[:] = [float(x) for x in np.diag([0.5, 0.5, 0.5, 1.0]).astype(np.float32).T.ravel()]
    D = float(np.sqrt(57.0))
    k.dt = float(np.float32(2.0 * D / 65536.0 * 0.999))
    refused(entries, 1, cam, k, "more than 65536 steps")
    k.dt = float(np.float32(2.0 * D / 65536.0 * 1.001))
    assert "null context" in device_call(entries, 1, cam, k)[1]
    # the unscaled box would pass with this dt: the guard looks at world space
    entries, cam, k2 = scene(1)
    k2.dt = float(np.float32(2.0 * np.sqrt(38.0) / 65536.0 * 1.001))
    assert "null context" in device_call(entries, 1, cam, k2)[1]
    # t + dt > t must hold up to D: an eye 2^21 away with dt = 1 (2 D / dt would pass, D * 2^-20 does not)
    entries, cam, k = scene(1, eye=(0.0, 0.0, float(2 ** 21)))
    k.dt = 1.0
    refused(entries, 1, cam, k, "below 2^-20")
    # the farthest corner over all volumes counts
    entries, cam, k = scene(2)
    entries[1].transform_inv[12] = -1000.0                 # volume 1 sits 1000 along x
    k.dt = 0.007
    refused(entries, 2, cam, k, "more than 65536 steps")


def test_host_entry_checks_the_volume_descriptors():
    entries, cam, k = scene(1)
    vd, _vox = va.volume_desc(np.zeros((2, 2, 2), np.float32))
    tf = va.transfunc(np.zeros((2, 4), np.float32))
    td = tf.desc()
    vd.format = 7
    rc = _capi.lib().vrh_multi_volume_render_host(C.byref(vd), C.byref(td), entries, 1, C.byref(cam), C.byref(k), None, None, None, None, None)
    assert rc == _capi.VRH_ERR_INVALID and "volume 0: unknown volume format" in _capi.lib().vrh_last_error().decode()


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_multi_volume_edge_check_program(flags, tmp_path):
    """tests/cpp/multi_volume_edge_check.cpp: a stand-alone program over the shared header -- the split samplers
    against tex3d / tex1d, directions with zero components, tmax == tmin, a ray that enters no box, 32 volumes,
    gradient coordinates outside [0, 1] under every address mode -- plain and under the address and
    undefined-behaviour sanitizers"""
    exe = str(tmp_path / "multi_volume_edge_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "multi_volume_edge_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "multi_volume_edge_check ok" in r.stdout


def test_python_layer_refusals():
    with pytest.raises(ValueError):
        va.multi_volume_kernel([], [UNIT_BOX], [np.eye(4)], [va.plastic()], va.point_light((0.0, 0.0, 0.0)))
    with pytest.raises(TypeError):
        va.multi_volume_entries([UNIT_BOX], [np.eye(4)], [np.zeros(5, np.float32)])
