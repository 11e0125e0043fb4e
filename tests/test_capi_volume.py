"""CPU: the volume part of the C-ABI (include/vrh.h) -- the ctypes structures have the sizes a C compiler gives
them, and every documented refusal is made without a device (the descriptors are checked before a context
is looked at; the host entry points share the checks of the device ones)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import visionaray_amd as va
from visionaray_amd import _capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vol_cases as VC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = ["vrh_volume_desc", "vrh_transfunc_desc", "vrh_volume_kernel_desc", "vrh_volume_stats"]


def test_ctypes_struct_sizes_match_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "vrh.h"\nint main(void) {\n'
                   + "".join('  printf("%s %%zu\\n", sizeof(%s));\n' % (s, s) for s in STRUCTS) + "  return 0;\n}\n")
    exe = str(tmp_path / "sizes")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = dict(line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    for s in STRUCTS:
        assert int(out[s]) == C.sizeof(getattr(_capi, s)), s
    assert _capi.VRH_VOLUME_MAX_STEPS == 65536 and (_capi.VRH_VOL_R8, _capi.VRH_VOL_R16, _capi.VRH_VOL_R32F) == (0, 1, 2)


def refused(fn, *args):
    rc = getattr(_capi.lib(), fn)(*args)
    msg = _capi.lib().vrh_last_error().decode()
    assert rc == _capi.VRH_ERR_INVALID, f"{fn}: status {rc} ({msg})"
    return msg


def create(vd, td):
    """vrh_volume_create without a context: a valid pair of descriptors gets as far as the context check"""
    out = C.c_void_p()
    msg = refused("vrh_volume_create", None, C.byref(vd), C.byref(td), C.byref(out))
    assert not out.value
    return msg


def good():
    vd, vox = va.volume_desc(np.zeros((3, 4, 5), np.float32), va.tex_filter.linear, va.tex_address.clamp)
    tf = va.transfunc(np.zeros((4, 4), np.float32))
    return vd, vox, tf, tf.desc()


def test_valid_descriptors_reach_the_context_check():
    vd, _vox, _tf, td = good()
    assert "null context" in create(vd, td)


@pytest.mark.parametrize("field,value,what", [("format", 3, "volume format"), ("filter", 2, "filter"), ("address", 3, "address mode")])
def test_unknown_volume_enum(field, value, what):
    vd, _vox, _tf, td = good()
    if field == "address":
        for a in range(3):
            vd2, _v2, _t2, _d2 = good()
            vd2.address[a] = value
            assert what in create(vd2, td)
    else:
        setattr(vd, field, value)
        assert what in create(vd, td)
    out = np.zeros(1, np.float32)
    c = np.zeros(3, np.float32)
    if field != "address":
        assert what in refused("vrh_tex3d_host", C.byref(vd), c.ctypes.data_as(C.c_void_p), 1, out.ctypes.data_as(C.c_void_p))


@pytest.mark.parametrize("field,value,what", [("filter", 2, "filter"), ("address", 3, "address mode")])
def test_unknown_transfunc_enum(field, value, what):
    vd, _vox, _tf, td = good()
    setattr(td, field, value)
    assert what in create(vd, td)
    out, c = np.zeros(4, np.float32), np.zeros(1, np.float32)
    assert what in refused("vrh_tex1d_host", C.byref(td), c.ctypes.data_as(C.c_void_p), 1, out.ctypes.data_as(C.c_void_p))


def test_dimensions():
    vd, _vox, _tf, td = good()
    for f in ("width", "height", "depth"):
        vd2, _v2, _t2, _d2 = good()
        setattr(vd2, f, _capi.VRH_TEX_MAX_DIM + 1)
        assert "dimension above" in create(vd2, td)
        setattr(vd2, f, 0)
        assert "dimension of 0" in create(vd2, td)
    # 2^29 voxels: refused by the count before a voxel is read (the pointer holds 60 floats)
    vd.width, vd.height, vd.depth = 1024, 1024, 512
    assert "2^28" in create(vd, td)
    vd, _vox, _tf, td = good()
    td.size = _capi.VRH_TEX_MAX_DIM + 1
    assert "size above" in create(vd, td)
    td.size = 0
    assert "size 0" in create(vd, td)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_values_that_are_not_finite(bad):
    vox = np.zeros((3, 4, 5), np.float32)
    vox[1, 2, 3] = bad
    vd, _keep = va.volume_desc(vox)
    tf = va.transfunc(np.zeros((4, 4), np.float32))
    assert "not finite" in create(vd, tf.desc())
    rgba = np.zeros((4, 4), np.float32)
    rgba[2, 1] = bad
    vd, _vox, _tf, _td = good()
    tf = va.transfunc(rgba)
    assert "entry 2 is not finite" in create(vd, tf.desc())


def test_voxel_above_the_coordinate_limit():
    vox = np.zeros((3, 4, 5), np.float32)
    vox[0, 0, 1] = -(_capi.VRH_TEX_MAX_COORD + 1.0)
    vd, _keep = va.volume_desc(vox)
    tf = va.transfunc(np.zeros((4, 4), np.float32))
    assert "2^20" in create(vd, tf.desc())
    vox[0, 0, 1] = _capi.VRH_TEX_MAX_COORD            # the limit itself is fine
    vd, _keep = va.volume_desc(vox)
    assert "null context" in create(vd, tf.desc())
    # the integer formats have no such limit
    vd, _keep = va.volume_desc(np.full((2, 2, 2), 65535, np.uint16))
    assert "null context" in create(vd, tf.desc())


def host_render(k, cam):
    vd, _vox, _tf, td = good()
    return refused("vrh_volume_render_host", C.byref(vd), C.byref(td), C.byref(cam), C.byref(k), None, None, None, None, None)


def example_view():
    F = VC.load_frame("vol_example")
    _tf, k, cam, _f, _a = VC.frame_objects(F, 8, 8)
    return k, cam


@pytest.mark.parametrize("dt,what", [(np.nan, "not finite"), (np.inf, "not finite"), (0.0, "dt <= 0"), (-0.01, "dt <= 0")])
def test_hang_guard_dt(dt, what):
    k, cam = example_view()
    k.dt = dt
    assert what in host_render(k, cam)
    # the device entry point makes the same check before it looks at its context, volume or target
    assert what in refused("vrh_render_volume", None, None, None, C.byref(cam), C.byref(k))


def test_hang_guard_step_too_small_for_the_eye_distance():
    k, cam = example_view()
    far = np.sqrt(sum(max(abs(cam.eye[a] - k.box_min[a]), abs(cam.eye[a] - k.box_max[a])) ** 2 for a in range(3)))
    k.dt = float(np.float32(far * 2.0 ** -20 * 0.99))
    assert "2^-20" in host_render(k, cam)
    # far away from a small box the same bound applies although the box itself would take few steps
    k, cam = example_view()
    cam.eye[0] = 1.0e6
    k.dt = 0.5
    assert "2^-20" in host_render(k, cam)


def test_hang_guard_too_many_steps():
    k, cam = example_view()
    diagonal = np.sqrt(12.0)
    k.dt = float(np.float32(diagonal / 65536 * 0.99))
    assert "65536 steps" in host_render(k, cam)
    k.dt = float(np.float32(diagonal / 65536 * 1.01))
    vd, _vox, _tf, td = good()
    st = _capi.vrh_volume_stats()
    _capi.check("vrh_volume_render_host", C.byref(vd), C.byref(td), C.byref(cam), C.byref(k), None, None, None, None, C.byref(st))
    assert st.rays == 64 and st.capped == 0


def test_kernel_parameters():
    for field, value, what in [("coord_sign", 0.5, "sign"), ("coord_sign", 0.0, "sign"), ("coord_extent", 0.0, "extent"),
                               ("coord_extent", np.nan, "extent"), ("coord_offset", np.inf, "offset"), ("box_min", np.nan, "box"),
                               ("box_min", 2.0, "box")]:
        k, cam = example_view()
        getattr(k, field)[1] = value
        assert what in host_render(k, cam), field


def test_python_wrappers_refuse_before_the_library():
    with pytest.raises(TypeError):
        va.volume_desc(np.zeros((2, 2), np.float32))
    with pytest.raises(TypeError):
        va.volume_desc(np.zeros((2, 2, 2), np.float64))
    with pytest.raises(TypeError):
        va.transfunc(np.zeros((4, 3), np.float32))


def test_hip_sched_refuses_what_the_volume_kernel_does_not_take():
    """non-uniform sampler, camera matrices and shards raise before any device call"""
    class _rt:
        def width(self):
            return 8

        def height(self):
            return 8

    sched = va.hip_sched.__new__(va.hip_sched)
    k = va.volume_kernel(None, ((-1, -1, -1), (1, 1, 1)))
    cam = va.camera()
    with pytest.raises(ValueError, match="uniform"):
        sched.frame(k, va.make_sched_params(va.pixel_sampler.jittered_type, cam, _rt()))
    with pytest.raises(ValueError, match="matrices"):
        sched.frame(k, va.make_sched_params(np.eye(4), np.eye(4), _rt()))
    with pytest.raises(ValueError, match="shards"):
        sched.frame(k, va.make_sched_params(cam, _rt()), shard=(0, 2, False))
