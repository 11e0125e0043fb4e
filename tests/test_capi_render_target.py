"""CPU: the formatted render targets' entry points (include/vrh.h vrh_rt_alloc_formatted ... vrh_rt_resolve_host) --
the structures' layouts, and every refusal that is decided before a context is used, with its error text.  No device
is needed."""
import ctypes as C

import numpy as np
import pytest

import visionaray_amd as va
from visionaray_amd import _capi

INVALID = _capi.VRH_ERR_INVALID


def call(fn, *args):
    rc = getattr(_capi.lib(), fn)(*args)
    return rc, _capi.lib().vrh_last_error().decode()


def test_structure_layouts():
    assert C.sizeof(_capi.vrh_rt_format) == 8
    d = _capi.vrh_resolve_desc
    assert C.sizeof(d) == 176
    assert (d.blend.offset, d.s.offset, d.d.offset, d.scissor.offset, d.matrix_cam.offset) == (0, 4, 8, 12, 28)
    assert (d.view.offset, d.proj.offset, d.jitter.offset, d.frame_num.offset, d.px_off.offset) == (32, 96, 160, 164, 168)
    assert (_capi.VRH_CF_RGBA32F, _capi.VRH_CF_RGB32F, _capi.VRH_CF_RGBA8, _capi.VRH_CF_RGB8) == (0, 1, 2, 3)
    assert (_capi.VRH_DF_NONE, _capi.VRH_DF_DEPTH32F, _capi.VRH_DF_DEPTH24_STENCIL8) == (0, 1, 2)


def test_alloc_refuses_bad_formats_before_the_context_is_used():
    out = C.c_void_p(0x1234)
    rc, msg = call("vrh_rt_alloc_formatted", None, 8, 8, 0, None, C.byref(out))
    assert rc == INVALID and "null format" in msg
    for cf, df, word in ((4, 0, "colour format 4"), (0, 3, "depth format 3"), (0xFFFFFFFF, 0, "colour format")):
        fmt = _capi.vrh_rt_format(cf, df)
        rc, msg = call("vrh_rt_alloc_formatted", None, 8, 8, 0, C.byref(fmt), C.byref(out))
        assert rc == INVALID and word in msg, msg
    fmt = _capi.vrh_rt_format(_capi.VRH_CF_RGBA8, 0)
    rc, msg = call("vrh_rt_alloc_formatted", None, 8, 8, 0, C.byref(fmt), C.byref(out))
    assert rc == INVALID and "vrh_rt_alloc_formatted" in msg             # a null context
    assert out.value == 0x1234, "nothing is handed out"


def test_null_targets_are_refused():
    d = va.resolve_desc()
    for fn, args in (("vrh_rt_get_formatted", (None, None, None, None)), ("vrh_rt_download_formatted", (None, None, None, None)),
                     ("vrh_rt_upload_formatted", (None, None, None, None)), ("vrh_rt_clear_depth", (None, None, C.c_float(1.0))),
                     ("vrh_rt_resolve", (None, None, C.byref(d)))):
        rc, msg = call(fn, *args)
        assert rc == INVALID and fn in msg, (fn, msg)


def resolve_host(fmt, w, h, color, pid, t, desc, co, do):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)     # noqa: E731
    return call("vrh_rt_resolve_host", None if fmt is None else C.byref(fmt), w, h, p(color), p(pid), p(t),
                None if desc is None else C.byref(desc), p(co), p(do))


def test_resolve_host_descriptor_checks():
    color, co = np.zeros((4, 4), np.float32), np.full((4, 4), 7, np.uint8)
    pid, t, do = np.zeros(4, np.uint32), np.zeros(4, np.float32), np.full(4, 9, np.uint32)
    rgba8 = _capi.vrh_rt_format(_capi.VRH_CF_RGBA8, _capi.VRH_DF_NONE)
    d24 = _capi.vrh_rt_format(_capi.VRH_CF_RGBA8, _capi.VRH_DF_DEPTH24_STENCIL8)
    ok = va.resolve_desc()
    cases = [
        ((None, 2, 2, color, None, None, ok, co, None), "null format"),
        ((_capi.vrh_rt_format(9, 0), 2, 2, color, None, None, ok, co, None), "unknown colour format 9"),
        ((_capi.vrh_rt_format(0, 7), 2, 2, color, None, None, ok, co, None), "unknown depth format 7"),
        ((rgba8, 0, 2, color, None, None, ok, co, None), "image size"),
        ((rgba8, 1 << 16, 1 << 16, color, None, None, ok, co, None), "image size"),
        ((rgba8, 2, 2, None, None, None, ok, co, None), "null colour"),
        ((rgba8, 2, 2, color, None, None, ok, None, None), "null colour"),
        ((rgba8, 2, 2, color, None, None, None, co, None), "null descriptor"),
        ((rgba8, 2, 2, color, None, None, va.resolve_desc(), co, None), None),
        ((d24, 2, 2, color, None, t, va.resolve_desc(view=np.eye(4), proj=np.eye(4)), co, do), "prim_id"),
        ((d24, 2, 2, color, pid, t, va.resolve_desc(view=np.eye(4), proj=np.eye(4)), co, None), "depth array"),
        ((d24, 2, 2, color, None, None, ok, co, do), "needs t"),
    ]
    bad_blend, bad_jitter = va.resolve_desc(), va.resolve_desc()
    bad_blend.blend, bad_jitter.jitter = 2, 5
    cases += [((rgba8, 2, 2, color, None, None, bad_blend, co, None), "blend"), ((rgba8, 2, 2, color, None, None, bad_jitter, co, None), "jitter")]
    for args, word in cases:
        co[...] = 7
        do[...] = 9
        rc, msg = resolve_host(*args)
        if word is None:
            assert rc == _capi.VRH_OK and (co == 0).all()
            continue
        assert rc == INVALID and word in msg and "vrh_rt_resolve_host" in msg, (word, msg)
        assert (co == 7).all() and (do == 9).all(), "a refusal writes nothing"


def test_python_mirror_checks_sizes():
    with pytest.raises(ValueError):
        va.rt_resolve_host(va.color_format.rgba8, va.depth_format.none, 3, 2, np.zeros((5, 4), np.float32), va.resolve_desc())
    with pytest.raises(ValueError):
        va.rt_resolve_host(va.color_format.rgba8, va.depth_format.depth32f, 3, 2, np.zeros((6, 4), np.float32),
                           va.resolve_desc(view=np.eye(4), proj=np.eye(4)), prim_id=np.zeros(5, np.uint32), t=np.zeros(6, np.float32))
    with pytest.raises(ValueError):
        va.hip_buffer_rt(None, 4, 4, wrap=(1, 0, 0, 0), color_format=va.color_format.rgb8)
