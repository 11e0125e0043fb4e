"""hip_shading::set_textures of the C++ header API (include/visionaray_hip/hip_backend.h) compiles with the
minimal texture_ref of visionaray_hip/standalone.h and, where the reference's headers exist, with the
reference's own texture_ref objects -- tests/cpp/textured_standalone.cpp, syntax only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "textured_standalone.cpp")


def test_set_textures_compiles_standalone():
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), SRC], check=True)


@pytest.mark.skipif(not os.path.isdir("/root/reference/include"), reason="reference headers absent")
def test_set_textures_compiles_against_reference_headers():
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-w", "-DVRH_TEST_REFERENCE_HEADERS", "-I/root/reference/include",
                    "-I", os.path.join(ROOT, "include"), SRC], check=True)
