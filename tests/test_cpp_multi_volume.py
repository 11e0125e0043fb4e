"""The C++ header layer of the multi-volume kernel (include/visionaray_hip), on the CPU: examples/multi_volume_hip.cpp
compiles against visionaray_hip/standalone.h alone and, where the reference's headers exist, against the
reference's own aabb / mat4 / plastic<float> / point_light<float> (the drop-in build); standalone.h's matrix
helpers give the example's transforms."""
import os
import subprocess

import numpy as np
import pytest

import visionaray_amd as va

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "examples", "multi_volume_hip.cpp")


def test_example_compiles_standalone():
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), SRC], check=True)


@pytest.mark.skipif(not os.path.isdir("/root/reference/include"), reason="reference headers absent")
def test_example_compiles_against_reference_headers():
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-w", "-DVRH_TEST_REFERENCE_HEADERS", "-I/root/reference/include",
                    "-I", os.path.join(ROOT, "include"), SRC], check=True)


def test_standalone_transforms_invert_to_the_fixtures_matrices(tmp_path):
    """t * r * s built with standalone.h's rotate / scale / translate and inverted by vrh_matrix_inverse: the
    bits of the inverse transforms the reference computed for mv_example"""
    src = tmp_path / "transforms.cpp"
    src.write_text("""#include <visionaray_hip/standalone.h>
#include <cstdio>
using namespace visionaray;
int main()
{
    for (int i = 0; i < 3; ++i)
    {
        vec3 axis(i == 0 ? 1.0f : 0.0f, i == 1 ? 1.0f : 0.0f, i == 2 ? 1.0f : 0.0f);
        mat4 r = rotate(mat4::identity(), axis, constants::pi<float>() / 4.0f);
        mat4 s = scale(mat4::identity(), vec3(1.0f, 1.0f, 1.0f));
        mat4 t = translate(mat4::identity(), vec3(i * 2.5f, 0.0f, 0.0f));
        mat4 m = t * r * s;
        for (int k = 0; k < 16; ++k) printf("%a ", m.data()[k]);
        printf("\\n");
    }
    return 0;
}
""")
    exe = str(tmp_path / "transforms")
    # hip_backend.h's inline functions call into libvrh: link against the in-tree library
    lib = os.path.join(ROOT, "visionaray_amd", "_lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                    "-L" + lib, "-lvrh", "-Wl,-rpath," + lib], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import mv_cases as MC
    F = MC.load_frame("mv_example")
    for i in range(3):
        m = np.asarray([float.fromhex(w) for w in out[i].split()], np.float32)
        assert np.array_equal(va.matrix_inverse(m).view(np.uint32), F["entries"][i][15:31].view(np.uint32)), i
