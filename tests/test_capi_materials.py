"""CPU: the tagged material record of the C ABI (vrh_material, include/vrh.h), its Python dtype and
constructors, the OBJ loader's generic materials (emissive where the MTL file has a Ke), and the C++
layer over generic_material lists (syntax only: no device here)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import visionaray_amd as va
from visionaray_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROP_IN = os.path.join(ROOT, "tests", "cpp", "drop_in_generic_material.cpp")


def test_material_record_size_and_offsets(tmp_path):
    """the documented layout, asked of the C compiler: 64 bytes, kind at 0, parameters from 4 on"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vrh.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(vrh_material),\n'
                   '  offsetof(vrh_material, kind), offsetof(vrh_material, u), offsetof(vrh_material, u.plastic.exp),\n'
                   '  offsetof(vrh_material, u.matte.cd), offsetof(vrh_material, u.matte.kd), offsetof(vrh_material, u.mirror.kr),\n'
                   '  offsetof(vrh_material, u.mirror.ior), offsetof(vrh_material, u.mirror.absorption),\n'
                   '  offsetof(vrh_material, u.emissive.ce), offsetof(vrh_material, u.emissive.ls)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [64, 0, 4, 4 + 4 * 12, 4 + 4 * 4, 4 + 4 * 7, 4 + 4 * 3, 4 + 4 * 4, 4 + 4 * 7, 4, 4 + 4 * 3]
    assert C.sizeof(_capi.vrh_material) == 64 and _capi.vrh_material.params.offset == 4
    assert (_capi.VRH_MATERIAL_PLASTIC, _capi.VRH_MATERIAL_MATTE, _capi.VRH_MATERIAL_MIRROR, _capi.VRH_MATERIAL_EMISSIVE) == (0, 1, 2, 3)
    header = open(os.path.join(ROOT, "include", "vrh.h")).read()
    for name, value in (("PLASTIC", 0), ("MATTE", 1), ("MIRROR", 2), ("EMISSIVE", 3)):
        assert re.search(r"VRH_MATERIAL_%s = %d\b" % (name, value), header)


def test_material_dtype_and_constructors():
    d = va.MATERIAL_DTYPE
    assert d.itemsize == 64 and d.fields["kind"][1] == 0 and d.fields["params"][1] == 4
    assert d.fields["params"][0].shape == (15,) and d.fields["params"][0].base == np.float32
    m = va.matte(ca=(0.1, 0.2, 0.3), ka=0.4, cd=(0.5, 0.6, 0.7), kd=0.8)
    assert m["kind"] == va.MATERIAL_MATTE
    assert np.array_equal(m["params"], np.float32([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8] + [0] * 7))
    r = va.mirror(cr=(1, 2, 3), kr=4, ior=(5, 6, 7), absorption=(8, 9, 10))
    assert r["kind"] == va.MATERIAL_MIRROR and np.array_equal(r["params"], np.float32(list(range(1, 11)) + [0] * 5))
    assert np.array_equal(va.mirror(ior=1.5, absorption=2.0)["params"][4:10], np.float32([1.5] * 3 + [2.0] * 3))
    e = va.emissive(ce=(1, 2, 3), ls=4)
    assert e["kind"] == va.MATERIAL_EMISSIVE and np.array_equal(e["params"], np.float32([1, 2, 3, 4] + [0] * 11))
    # a plastic record is lifted with its 13 floats unchanged
    p = va.plastic(ca=(0.1, 0.2, 0.3), ka=0.4, cd=(0.5, 0.6, 0.7), kd=0.8, cs=(0.9, 1.0, 1.1), ks=1.2, exp=13.0)
    g = va.generic_materials([p, m, np.stack([r, e])])
    assert g.dtype == d and [int(k) for k in g["kind"]] == [0, 1, 2, 3]
    assert g["params"][0, :13].tobytes() == p.tobytes() and np.all(g["params"][0, 13:] == 0.0)
    assert g[1] == m and g[2] == r and g[3] == e


OBJ = """mtllib box.mtl
v 0 0 0
v 1 0 0
v 0 1 0
v 0 0 1
usemtl lamp
f 1 2 3
usemtl wall
f 1 2 4
usemtl faint
f 1 3 4
"""
MTL = """newmtl lamp
Ka 0.1 0.1 0.1
Kd 0.2 0.3 0.4
Ks 0.5 0.5 0.5
Ke 4.0 3.0 2.0
Ns 10
newmtl wall
Ka 0.3 0.2 0.1
Kd 0.6 0.5 0.4
Ks 0.9 0.8 0.7
Ns 20
newmtl faint
Kd 0.5 0.5 0.5
Ke 0 0 1e-30
"""


def test_obj_generic_materials_turn_ke_into_emissive(tmp_path):
    (tmp_path / "box.obj").write_text(OBJ)
    (tmp_path / "box.mtl").write_text(MTL)
    mod = va.load_obj(tmp_path / "box.obj")
    assert mod.material_names == ["lamp", "wall", "faint"]
    # vrh_obj_get_data: the unchanged plastic array (Ke is not part of it)
    assert mod.materials.dtype == va.PLASTIC_DTYPE and len(mod.materials) == 3
    want = np.zeros(3, va.PLASTIC_DTYPE)
    want[0] = ((0.1, 0.1, 0.1), 1.0, (0.2, 0.3, 0.4), 1.0, (0.5, 0.5, 0.5), 1.0, 10.0)
    want[1] = ((0.3, 0.2, 0.1), 1.0, (0.6, 0.5, 0.4), 1.0, (0.9, 0.8, 0.7), 1.0, 20.0)
    assert mod.materials[:2].tobytes() == want[:2].tobytes()
    g = mod.generic_materials
    assert g.dtype == va.MATERIAL_DTYPE and len(g) == 3
    assert g[0] == va.emissive(ce=(4.0, 3.0, 2.0), ls=1.0)
    assert g[1]["kind"] == va.MATERIAL_PLASTIC
    assert g[1] == va.generic_materials(mod.materials[1:2])[0]
    # length(Ke) > 0 in float: (1e-30)^2 underflows to 0, so the reference keeps this one plastic
    assert g[2]["kind"] == va.MATERIAL_PLASTIC and g[2] == va.generic_materials(mod.materials[2:3])[0]
    assert [int(p["geom_id"]) for p in mod.primitives] == [0, 1, 2]


def test_obj_padding_materials_are_plastic(tmp_path):
    (tmp_path / "plain.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    mod = va.load_obj(tmp_path / "plain.obj")
    assert len(mod.generic_materials) == len(mod.materials) == 1
    assert mod.generic_materials[0] == va.generic_materials(mod.materials)[0]


def test_generic_material_program_compiles_standalone():
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-DVRH_DROP_IN_STANDALONE",
                    "-I", os.path.join(ROOT, "include"), DROP_IN], check=True)
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "pathtrace_emissive_hip.cpp")], check=True)


@pytest.mark.skipif(not os.path.isdir("/root/reference/include"), reason="reference headers absent")
def test_generic_material_drop_in_compiles_against_reference_headers():
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-w", "-I/root/reference/include",
                    "-I", os.path.join(ROOT, "include"), DROP_IN], check=True)
