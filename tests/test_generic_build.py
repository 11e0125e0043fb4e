"""CPU: vrh_build_bvh over generic primitives (VRH_PRIM_GENERIC80: triangles and spheres in one list).

The fixtures tests/golden/gp_*.npz hold the reference's own build<index_bvh<generic_primitive<...>>> of their
records (tests/golden/make_generic_primitive_golden.py); the host builder must give those trees byte for byte.
"""
import numpy as np
import pytest

import gp_cases
import visionaray_amd as va
from visionaray_amd import _capi


@pytest.mark.parametrize("case", gp_cases.CASES)
def test_build_matches_the_reference_tree(case):
    a = gp_cases.fixture(case)
    nodes, indices, depth = gp_cases.build(a["records"])
    assert gp_cases.same_bits(nodes, a["nodes"])
    assert gp_cases.same_bits(indices, a["indices"])
    assert depth == gp_cases.tree_depth(a["nodes"].view(va.BVH_NODE_DTYPE).reshape(-1))


def test_fixture_records_have_the_documented_layout():
    for case in gp_cases.CASES:
        a = gp_cases.fixture(case)
        r = a["records"]
        assert r.dtype.itemsize == 80 and set(np.unique(r["type"])) == {1, 2}
        assert gp_cases.spec()[case]["num_spheres"] == int((r["type"] == 2).sum())
        assert not a["prims"][:, 17:].any()                         # padding after the type index


def test_single_kind_lists_build_the_single_kind_trees():
    tris, sph = gp_cases.random_mixed(7, 300, 300)
    for plain, generic in ((tris, va.make_generic(tris, None)), (sph, va.make_generic(None, sph))):
        pn, pi, pd = gp_cases.build(plain)
        gn, gi, gd = gp_cases.build(generic)
        assert gp_cases.same_bits(pn, gn) and gp_cases.same_bits(pi, gi) and pd == gd
    one = va.make_generic(tris[:1], None)
    assert gp_cases.build(one)[0].shape == (1, 8)


def test_make_generic_interleaves_in_prim_order():
    tris, sph = gp_cases.random_mixed(3, 3, 2)
    g = va.make_generic(tris, sph, order=[1, 0, 0, 1, 0])
    assert list(g["type"]) == [2, 1, 1, 2, 1]
    assert bytes(g["data"][1]) == tris[0].tobytes() and bytes(g["data"][3][:48]) == sph[1].tobytes()
    assert not g["data"][0][48:].any()
    with pytest.raises(ValueError):
        va.make_generic(tris, sph, order=[0, 0, 0, 0, 1])


@pytest.mark.parametrize("bad", [0, 3])
def test_unknown_type_index_is_invalid(bad):
    tris, sph = gp_cases.random_mixed(5, 6, 6)
    g = va.make_generic(tris, sph)
    assert gp_cases.build_status(g) == _capi.VRH_OK
    g["type"][7] = bad
    assert gp_cases.build_status(g) == _capi.VRH_ERR_INVALID


def test_record_layout_and_upload_relayout_under_sanitizers(tmp_path):
    """tests/cpp/generic_record_check.cpp: a stand-alone host program under ASan / UBSan over a fixture's records"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, recs = tmp_path / "generic_record_check", tmp_path / "records.bin"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(root, "tests", "cpp", "generic_record_check.cpp"), "-o", str(exe)], check=True)
    gp_cases.fixture("gp_soup")["records"].tofile(str(recs))
    r = subprocess.run([str(exe), str(recs)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "generic record ok: 150 triangles, 150 spheres"
