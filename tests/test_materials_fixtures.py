"""CPU: the fixtures of the path tracer over tagged materials (tests/golden/pathtrace_materials.json,
ptm_*.npz; written by tests/golden/make_generic_material_golden.py from the reference's own kernel) are
what tests/test_gpu_pathtracing_materials.py expects: the cases and their settings, self-contained
arrays, finite frames, and tolerances within the project's caps."""
import json
import os

import numpy as np
import pytest

import visionaray_amd as va

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
MAX_UNSTABLE, MAX_RTOL = 0.0025, 1e-2          # tests/pt_cases.py
MISS = 0xFFFFFFFF
with open(os.path.join(GOLDEN, "pathtrace_materials.json")) as _f:
    PTM = json.load(_f)

ROOM4 = ["matte", "emissive", "mirror", "matte"]
DARK, ENV = [0.0, 0.0, 0.0, 1.0], [1.0, 1.0, 1.0, 1.0]
# case: materials, ambient, bounces, binding, frames (None: jittered_blend, 4 frames)
CASES = {
    "ptm_room_emitter": (ROOM4, DARK, 10, "face", [0, 1]),
    "ptm_room_vertex": (ROOM4, DARK, 5, "vertex", [0]),
    "ptm_soup_env": (["matte", "mirror", "emissive"], ENV, 4, "face", [0]),
    "ptm_room_blend": (ROOM4, DARK, 5, "face", None),
    "ptm_room_plastic": (["matte", "emissive", "mirror", "plastic", "matte"], ENV, 4, "face", [0]),
}
KIND = {"plastic": va.MATERIAL_PLASTIC, "matte": va.MATERIAL_MATTE, "mirror": va.MATERIAL_MIRROR,
        "emissive": va.MATERIAL_EMISSIVE}


def test_the_json_lists_the_cases_with_their_settings():
    assert set(PTM) == set(CASES)
    for case, (mats, ambient, bounces, binding, frames) in CASES.items():
        g = PTM[case]
        assert (g["W"], g["H"]) == (60, 44), case          # partial 8 x 8 tiles on both edges
        assert g["materials"] == mats and g["ambient"] == ambient and g["bounces"] == bounces, case
        assert g["binding"] == binding, case
        assert 112 <= g["num_prims"] <= 312 or g["family"] == "soup" and 100 <= g["num_prims"] <= 300, case
        if frames is None:
            assert g["sampler"] == "jittered_blend" and g["num_frames"] == 4 and g["rays_total"] > 0, case
        else:
            assert g["sampler"] == "uniform" and g["frames"] == frames, case
            assert sorted(g["rays"]) == sorted(str(f) for f in frames), case
        assert g["powf_free"] == ("plastic" not in mats), case


@pytest.mark.parametrize("case", sorted(CASES))
def test_fixture_files_are_small_self_contained_and_finite(case):
    g = PTM[case]
    path = os.path.join(GOLDEN, case + ".npz")
    assert os.path.getsize(path) < (1 << 20) and os.path.getsize(path) == g["bytes"]
    with np.load(path) as z:
        a = {k: z[k] for k in z.files}
    n = g["W"] * g["H"]
    assert a["prims"].shape == (g["num_prims"], 16) and a["prims"].dtype == np.uint32
    prims = np.ascontiguousarray(a["prims"]).view(va.TRIANGLE_DTYPE).reshape(-1)
    assert np.array_equal(prims["prim_id"], np.arange(len(prims)))
    assert np.array_equal(prims["geom_id"], np.arange(len(prims)) % len(g["materials"]))
    assert a["normals"].shape == (len(prims), 4) and a["camera"].shape == (4, 3)
    assert ("vertex_normals" in a) == (g["binding"] == "vertex")
    if g["binding"] == "vertex":
        assert a["vertex_normals"].shape == (3 * len(prims), 4)
    mats = np.ascontiguousarray(a["materials"]).view(va.MATERIAL_DTYPE).reshape(-1)
    assert [int(k) for k in mats["kind"]] == [KIND[k] for k in g["materials"]]
    if "plastic" in g["materials"]:
        p = mats[g["materials"].index("plastic")]["params"]
        assert p[11] > 0.0 and p[12] == 32.0                 # ks > 0, exp 32
    frames = ["color_first", "color_last"] if g["sampler"] == "jittered_blend" else ["color_f%d" % f for f in g["frames"]]
    for f in frames:
        assert a[f].shape == (n, 4) and a[f].dtype == np.float32 and np.isfinite(a[f]).all(), f
    assert a["prim_id"].shape == (n,) and a["t"].shape == (n,)
    hit = a["prim_id"] != MISS
    assert np.all(a["t"][hit] > 0.0) and np.all(a["t"][~hit] == -1.0)
    last = a[frames[-1]]
    assert np.all(last[hit, 3] == 1.0)
    # both populations: pixels that hit and pixels that miss, or in a closed room paths that end on an
    # emitter (light in the pixel) and paths that do not
    light = np.any(a[frames[0]][:, :3] != 0.0, axis=1)
    if g["family"] == "soup":
        assert hit.any() and (~hit).any()
        assert np.array_equal(last[~hit], np.tile(np.float32(g["bg"]), (int((~hit).sum()), 1)))
    else:
        assert hit.all() and light.any() and (~light).any()


def test_tolerances_are_within_the_caps():
    for case, g in PTM.items():
        assert 0.0 <= g["unstable"] <= MAX_UNSTABLE, case
        assert 0.0 <= g["rtol"] <= MAX_RTOL and g["rtol"] == 2.0 * g["sens"], case
        if g["powf_free"]:
            assert g["sens"] == 0.0 and g["rtol"] == 0.0 and g["unstable"] == 0.0, case
        else:
            assert g["sens"] > 0.0, case
