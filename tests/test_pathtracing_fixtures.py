"""CPU: the path-tracing fixtures (tests/golden/pathtrace.json, pt_*.npz) and the kernel-kind constant."""
import json
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
CASES = {
    "pt_cornell12_diffuse": ("cornell12", 64, 64, "face", "diffuse", 4),
    "pt_hfstack_diffuse": ("hfstack32x24", 96, 64, "face", "diffuse", 10),
    "pt_hf64_vertex_diffuse": ("hf64", 60, 44, "vertex", "diffuse", 3),
    "pt_cornell12_blend": ("cornell12", 64, 64, "face", "diffuse", 4),
    "pt_cornell12_plastic2": ("cornell12", 64, 64, "face", "plastic", 2),
    "pt_cornell12_plastic": ("cornell12", 64, 64, "face", "plastic", 4),
}
FRAMES = {"pt_cornell12_diffuse": [0, 2], "pt_hfstack_diffuse": [0], "pt_hf64_vertex_diffuse": [0, 1],
          "pt_cornell12_plastic2": [0], "pt_cornell12_plastic": [0]}


def load():
    with open(os.path.join(GOLDEN, "pathtrace.json")) as f:
        return json.load(f)


def test_every_case_is_listed_with_its_settings():
    pt = load()
    assert set(pt) == set(CASES)
    for case, (scene, W, H, binding, mat, bounces) in CASES.items():
        g = pt[case]
        assert (g["scene"], g["W"], g["H"], g["binding"], g["materials"], g["bounces"]) == (scene, W, H, binding, mat, bounces)
        assert g["ambient"] == [1.0, 1.0, 1.0, 1.0]
    b = pt["pt_cornell12_blend"]
    assert (b["sampler"], b["first_frame"], b["num_frames"]) == ("jittered_blend", 1, 4)


def test_fixture_files_hold_the_frames_and_stay_small():
    pt = load()
    for case, g in pt.items():
        path = os.path.join(GOLDEN, case + ".npz")
        assert os.path.getsize(path) < (1 << 20)
        with np.load(path) as z:
            names = ["color_first", "color_last"] if case == "pt_cornell12_blend" else ["color_f%d" % f for f in FRAMES[case]]
            assert sorted(z.files) == sorted(names)
            for n in names:
                assert z[n].shape == (g["W"] * g["H"], 4) and z[n].dtype == np.float32
                assert np.isfinite(z[n]).all()
        if case != "pt_cornell12_blend":
            assert g["frames"] == FRAMES[case]
            assert all(g["rays"][str(f)] >= g["W"] * g["H"] for f in g["frames"])


def test_plastic_cases_carry_a_derived_tolerance():
    pt = load()
    for case in ("pt_cornell12_plastic2", "pt_cornell12_plastic"):
        g = pt[case]
        assert g["rtol_spec"] > 0.0 and g["rtol_spec"] == 2.0 * g["sens"]
        assert 0.0 <= g["unstable_share"] <= 0.0025
        assert g["powf_ulps"] >= 1


def test_kernel_kind_constant_is_5_in_header_and_binding():
    from visionaray_amd import _capi
    with open(os.path.join(ROOT, "include", "vrh.h")) as f:
        m = re.search(r"VRH_KERNEL_PATHTRACING\s*=\s*(\d+)", f.read())
    assert m and int(m.group(1)) == 5
    assert _capi.VRH_KERNEL_PATHTRACING == 5
