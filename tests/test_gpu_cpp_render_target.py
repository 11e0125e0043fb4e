"""GPU: formatted render targets through the C++ header layer.  tests/cpp/render_target_user.hip (built by
visionaray_amd/Makefile with hipcc) renders into hip_buffer_rt<PF_RGBA8, PF_UNSPECIFIED> and <PF_RGBA32F, PF_DEPTH32F>
through hip_sched::frame, with built-in kernels and with a user lambda; every frame's formatted buffers are held, bit
for bit, to vrh_rt_resolve_host of the staging buffers the same frame left."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import visionaray_amd as va

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rt_cases as RC  # noqa: E402
from test_gpu_render_target import look_at, perspective  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
USER = os.path.join(ROOT, "build", "tests", "render_target_user")


def load(d, name, n, cf, df):
    raw = open(os.path.join(d, name + ".staging"), "rb").read()
    st = {"color": np.frombuffer(raw, np.float32, n * 4).reshape(n, 4), "prim_id": np.frombuffer(raw, np.uint32, n, n * 16),
          "t": np.frombuffer(raw, np.float32, n, n * 20)}
    raw = open(os.path.join(d, name + ".formatted"), "rb").read()
    cb = 4 if cf == RC.CF.rgba8 else 16
    fm = {"color": np.frombuffer(raw, np.uint8 if cf == RC.CF.rgba8 else np.float32, n * 4).reshape(n, 4)}
    if df != RC.DF.none:
        fm["depth"] = np.frombuffer(raw, np.float32, n, n * cb)
    assert len(raw) == n * cb + (n * 4 if df != RC.DF.none else 0)
    return st, fm


def same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a) and sorted(a) == sorted(b)


def test_formatted_targets_through_hip_sched(ctx, tmp_path):
    view, proj = look_at((0.3, 0.2, 3.0), (0.0, 0.0, 0.0)), perspective(0.8, 61 / 45, 0.5, 10.0)
    mats = np.concatenate([view.T.reshape(16), proj.T.reshape(16)]).astype(np.float32)
    mats.tofile(str(tmp_path / "matrices.bin"))
    r = subprocess.run([USER, str(tmp_path), str(tmp_path / "matrices.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    w, h = out["width"], out["height"]
    n = w * h
    assert out["pinhole_depth_refused"] == 1 and out["names_depth"] == 1 and out["frames_refused"] == 1 and out["names_batch"] == 1
    assert out["has_depth_ptr"] == 1 and out["formatted_differs"] == 1
    for name in ("rgba8_builtin", "rgba8_user"):
        st, fm = load(tmp_path, name, n, RC.CF.rgba8, RC.DF.none)
        assert (st["color"][:, 0] != st["color"][0, 0]).any(), name
        assert same(fm, va.rt_resolve_host(RC.CF.rgba8, RC.DF.none, w, h, st["color"], va.resolve_desc())), name
    # the user kernel's scissor box: the pixels outside keep the cleared colour
    st, fm = load(tmp_path, "rgba8_user_box", n, RC.CF.rgba8, RC.DF.none)
    cleared = va.rt_resolve_host(RC.CF.rgba8, RC.DF.none, w, h, np.tile(np.float32([1.0, 0.5, 0.25, 1.0]), (n, 1)), va.resolve_desc())
    want = va.rt_resolve_host(RC.CF.rgba8, RC.DF.none, w, h, st["color"], va.resolve_desc(scissor=(5, 3, 50, 40)), color_out=cleared["color"])
    assert same(fm, want) and (want["color"] != cleared["color"]).any()
    # depth through camera matrices with the built-in kernel; the refused user frame leaves the target as it was
    st, fm = load(tmp_path, "depth32f_builtin", n, RC.CF.rgba32f, RC.DF.depth32f)
    want = va.rt_resolve_host(RC.CF.rgba32f, RC.DF.depth32f, w, h, st["color"], va.resolve_desc(view=mats[:16], proj=mats[16:]),
                              prim_id=st["prim_id"], t=st["t"])
    assert same(fm, want)
    hit = st["prim_id"] != RC.MISS
    assert hit.any() and (~hit).any() and np.all(fm["depth"][~hit] == 1.0) and np.all(fm["depth"][hit] < 1.0)
    builtin_st, builtin_fm = st, fm
    # the user lambda through camera matrices: its result's isect_pos = ori + dir * t becomes the depth, which the launch
    # leaves in the staging t buffer; the same ray and hit as the built-in kernel's, so the same depth buffer
    st, fm = load(tmp_path, "depth32f_user", n, RC.CF.rgba32f, RC.DF.depth32f)
    user_desc = va.resolve_desc()                            # matrix_cam 0: the staging t is the depth
    assert same(fm, va.rt_resolve_host(RC.CF.rgba32f, RC.DF.depth32f, w, h, st["color"], user_desc, t=st["t"]))
    assert fm["depth"].tobytes() == builtin_fm["depth"].tobytes(), "the user kernel's depth is the built-in kernel's"
    # ... and blended by jittered_blend, frame 2, onto it: the launch runs the jittered ray, the resolve blends
    st2, fm2 = load(tmp_path, "depth32f_user_blend2", n, RC.CF.rgba32f, RC.DF.depth32f)
    half = va.resolve_desc(blend=True, s=0.5, d=0.5)
    assert same(fm2, va.rt_resolve_host(RC.CF.rgba32f, RC.DF.depth32f, w, h, st2["color"], half, t=st2["t"], color_out=fm["color"],
                                        depth_out=fm["depth"]))
    assert st2["t"].tobytes() != st["t"].tobytes(), "the jittered ray"
    # jittered_blend of the user lambda into RGBA8: each frame's sample in the staging buffer, the quantised buffer accumulates
    state = {"color": np.zeros((n, 4), np.uint8)}
    samples = []
    for f in (1, 2, 3):
        st, fm = load(tmp_path, "rgba8_user_blend%d" % f, n, RC.CF.rgba8, RC.DF.none)
        s = np.float32(1.0) / np.float32(f)
        state = va.rt_resolve_host(RC.CF.rgba8, RC.DF.none, w, h, st["color"], va.resolve_desc(blend=True, s=float(s), d=float(np.float32(1.0) - s)),
                                   color_out=state["color"])
        assert same(fm, state), f
        samples.append(st["color"].tobytes())
    assert len(set(samples)) == 3, "three different jittered samples"
    st3, fm3 = load(tmp_path, "rgba8_after_refusal", n, RC.CF.rgba8, RC.DF.none)
    assert same(fm3, state) and st3["color"].tobytes() == samples[-1]
    st, fm = st2, fm2
    st2, fm2 = load(tmp_path, "depth32f_after_refusal", n, RC.CF.rgba32f, RC.DF.depth32f)
    assert same(st2, st) and same(fm2, fm)
