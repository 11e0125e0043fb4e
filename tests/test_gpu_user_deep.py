"""GPU: user kernels (include/visionaray_hip/hip_kernels.h) on BVHs around and beyond the depth of
their LDS traversal stack -- `user_kernels deep` (tests/cpp/user_kernels.hip) on the scenes of
tests/deep_cases.py against the oracle's frames of the same bytes, bit for bit.

A launch gives 24 stack entries per thread (VRH_USER_LDS_STACK) unless a deeper BVH was registered,
32 (VRH_USER_STACK) at the most, and a BVH of depth d needs d + 1.  By the route the kernel's
hip_bvh_ref was made:

    depth            ref                    checked                view
    23               exact, 24 entries      exact, 24 entries      exact, 24 entries
    24 .. 31         exact, d + 1 entries   exact, d + 1 entries   VRH_ERR_UNSUPPORTED at download()
    32 and deeper    checked_ref's host error, no launch           VRH_ERR_UNSUPPORTED at download()

Before checked_ref registered the depth it accepts, `checked` at 24 .. 31 rendered a frame of misses,
and before the device recorded a declined walk, so did every `view` cell but the first -- with exit
status 0 either way.  An error case here is a reported error: the device side of a declined walk is an
early return, nothing faults.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import deep_cases as D
from visionaray_amd import _capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "tests", "user_kernels")
VARIANT_BINS = ["uk_defer", "uk_share", "uk_cut", "uk_oca"]
SHORT, WHOLE = 24, 32          # VRH_USER_LDS_STACK, VRH_USER_STACK
CRASHED = (134, 139, -6, -11)


def _deep(tmp_path, binary, name, camera, route, grid=0):
    """one `deep` process: (exit status, the JSON lines it printed, its output directory)"""
    assert os.path.exists(binary), "run __graft_entry__.build() (make -C visionaray_amd cpp_tests)"
    scene = D.write_scene(str(tmp_path / "scene"), name, camera)
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([binary, "deep", str(grid), str(D.W), str(D.H), str(out), scene, route],
                       capture_output=True, text=True, timeout=120)
    recs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    print(r.returncode, r.stdout, r.stderr)
    assert r.returncode not in CRASHED, r.stderr
    return r, recs, out


def _assert_exact(out, name, camera):
    ref = D.reference(name, camera)
    got = {"prim_id": np.fromfile(out / "prim_id.bin", np.uint32), "t": np.fromfile(out / "t.bin", np.float32),
           "occ": np.fromfile(out / "occ.bin", np.uint8),
           "color": np.fromfile(out / "color.bin", np.float32).reshape(-1, 4)}
    for k in ("prim_id", "occ"):
        assert np.array_equal(got[k], ref[k]), f"{k}: {int((got[k] != ref[k]).sum())} pixels differ from the oracle"
    for k in ("t", "color"):
        assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), f"{k}: bits differ from the oracle"
    assert (ref["prim_id"] != D.MISS).any()


def _assert_rendered(run, name, camera, entries):
    r, recs, out = run
    assert r.returncode == 0, r.stdout + r.stderr
    rec = next(x for x in recs if "max_depth" in x)
    assert rec["max_depth"] == D.case(name).depth
    assert rec["stack_entries"] == entries
    _assert_exact(out, name, camera)
    return rec


def _assert_unsupported(run, launched):
    """a reported VRH_ERR_UNSUPPORTED: exit status 3, the status in the JSON line, no frame written"""
    r, recs, out = run
    assert r.returncode == 3, f"exit status {r.returncode}: {r.stdout}{r.stderr}"
    rec = next(x for x in recs if "error_status" in x)
    assert rec["error_status"] == _capi.VRH_ERR_UNSUPPORTED, rec
    assert not (out / "prim_id.bin").exists()
    assert not any("max_depth" in x for x in recs)
    if launched is None:
        assert rec["stack_entries"] == 0, "checked_ref rejects the BVH before any launch"
    else:
        assert rec["stack_entries"] == launched
        assert str(launched) in rec["what"] and "depth" in rec["what"], rec["what"]
    return rec


# ---- the default build ------------------------------------------------------------------------------

@pytest.mark.parametrize("camera", ["oblique", "axial"])
@pytest.mark.parametrize("route", ["ref", "checked", "view"])
def test_comb_that_fits_the_short_stack_renders_by_every_route(tmp_path, route, camera):
    """depth 23: the deepest BVH the 24-entry stack holds; the axial camera's walk holds 23 entries"""
    _assert_rendered(_deep(tmp_path, BIN, "comb24", camera, route), "comb24", camera, SHORT)


@pytest.mark.parametrize("camera", ["oblique", "axial"])
@pytest.mark.parametrize("route", ["ref", "checked"])
@pytest.mark.parametrize("n", [25, 28, 32])
def test_comb_deeper_than_the_short_stack_renders_through_registered_routes(tmp_path, n, route, camera):
    """depth 24, 27, 31: ref() and checked_ref() register the depth, the launch gives depth + 1 entries
    and the axial camera's walk sits on the last of them"""
    _assert_rendered(_deep(tmp_path, BIN, f"comb{n}", camera, route), f"comb{n}", camera, n)


@pytest.mark.parametrize("camera", ["oblique", "axial"])
@pytest.mark.parametrize("n", [25, 28, 32])
def test_comb_deeper_than_the_short_stack_unregistered_is_an_error(tmp_path, n, camera):
    rec = _assert_unsupported(_deep(tmp_path, BIN, f"comb{n}", camera, "view"), SHORT)
    assert str(n - 1) in rec["what"]


@pytest.mark.parametrize("route", ["ref", "checked", "view"])
@pytest.mark.parametrize("name", sorted(D.SAH))
def test_sah_built_deep_trees(tmp_path, name, route):
    """depth 24 and 28 from the SAH builder, leaves of several primitives"""
    depth = D.case(name).depth
    assert SHORT <= depth < WHOLE
    run = _deep(tmp_path, BIN, name, "oblique", route)
    if route == "view":
        _assert_unsupported(run, SHORT)
    else:
        _assert_rendered(run, name, "oblique", depth + 1)


@pytest.mark.parametrize("route", ["ref", "checked", "view"])
@pytest.mark.parametrize("n", [33, 41])
def test_comb_deeper_than_the_whole_stack_is_an_error_by_every_route(tmp_path, n, route):
    """depth 32, 40: checked_ref rejects the BVH on the host before any launch; the unchecked view is
    launched with the short stack, declined on the device and reported"""
    _assert_unsupported(_deep(tmp_path, BIN, f"comb{n}", "oblique", route), SHORT if route == "view" else None)


def test_stack_grows_within_one_process(tmp_path):
    """hf64 through ref() with the short stack, then the first ref() of a comb 27 deep: the next launch
    gives 28 entries (the registry, and the launch choices cached per stack size) and its frame is exact"""
    rec = _assert_rendered(_deep(tmp_path, BIN, "comb28", "oblique", "grow", grid=64), "comb28", "oblique", 28)
    assert rec["first_stack_entries"] == SHORT


def test_declined_walk_is_reported_once_and_the_context_recovers(tmp_path):
    """comb 27 deep through the unregistered view: VRH_ERR_UNSUPPORTED at download(), nothing more at the
    next sync(); then the same view through checked_ref on the same context and target: exact"""
    rec = _assert_rendered(_deep(tmp_path, BIN, "comb28", "oblique", "recover", grid=64), "comb28", "oblique", 28)
    assert rec["first_error_status"] == _capi.VRH_ERR_UNSUPPORTED
    assert rec["first_stack_entries"] == SHORT


# ---- the opt-in walks: always the whole 32-entry stack -------------------------------------------------

@pytest.mark.parametrize("binary", VARIANT_BINS)
def test_variant_builds_render_a_deep_comb(tmp_path, binary):
    """comb 27 deep, oblique camera.  The hit / miss answers decide every compared output, so the
    shared walk's free choice of which hit it reports does not matter here."""
    b = os.path.join(ROOT, "build", "tests", binary)
    _assert_rendered(_deep(tmp_path, b, "comb28", "oblique", "ref"), "comb28", "oblique", WHOLE)


@pytest.mark.parametrize("binary", VARIANT_BINS)
def test_variant_builds_report_a_comb_deeper_than_the_stack(tmp_path, binary):
    b = os.path.join(ROOT, "build", "tests", binary)
    rec = _assert_unsupported(_deep(tmp_path, b, "comb41", "oblique", "view"), WHOLE)
    assert "40" in rec["what"]


def test_declined_walk_word_of_a_context(ctx):
    """vrh_ctx_user_declined: one word per context, host-readable, zero while no walk was declined"""
    lib = _capi.lib()
    hw, dw, hw2, dw2 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert lib.vrh_ctx_user_declined(ctx.handle, C.byref(hw), C.byref(dw)) == _capi.VRH_OK
    assert lib.vrh_ctx_user_declined(ctx.handle, C.byref(hw2), None) == _capi.VRH_OK
    assert hw.value and dw.value and hw2.value == hw.value
    assert C.c_uint32.from_address(hw.value).value == 0
