"""CPU: tests/cpp/drop_in_render_target.cpp, an application that keeps hip_buffer_rt<CF, DF> in the reference's
other pixel formats, compiles against the reference's headers with the reference's pixel_format values (where
they exist) and against include/ alone; a format outside the supported set does not compile."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "drop_in_render_target.cpp")


@pytest.mark.skipif(not os.path.isdir("/root/reference/include"), reason="reference headers absent")
def test_render_target_drop_in_compiles_against_reference_headers():
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-w", "-I/root/reference/include", "-I", os.path.join(ROOT, "include"), SRC],
                   check=True)


def test_render_target_drop_in_compiles_standalone():
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-DVRH_DROP_IN_STANDALONE", "-I", os.path.join(ROOT, "include"),
                    SRC], check=True)


@pytest.mark.parametrize("cf,df,word", [("5", "0", "colour format"), ("12", "33", "depth format")])
def test_other_formats_do_not_compile(tmp_path, cf, df, word):
    src = tmp_path / "bad_format.cpp"
    src.write_text("#include <visionaray_hip/standalone.h>\nvisionaray::hip_buffer_rt<%s, %s> rt;\nint main() { return 0; }\n" % (cf, df))
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode != 0 and "hip_buffer_rt" in r.stderr and word in r.stderr
