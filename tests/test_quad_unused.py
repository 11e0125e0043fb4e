"""The never-hit boxes of unused 4-wide entries (vrh_quad.cpp build_quads, vrh_device.h NEVER_HIT_UNUSED) on the CPU --
tests/cpp/quad_unused_check.cpp, host code built with AddressSanitizer and UBSan as a program of its own: every
unused entry of hand-made trees' records is the point box at +inf with link QUAD_NONE, no admitted ray passes one
under either form of the entry test without the link compare, every entry gives what the compared records gave,
and the inverted box the records must not use does pass."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_unused_entries_never_pass(tmp_path):
    exe = tmp_path / "quad_unused_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "quad_unused_check.cpp"),
                    os.path.join(ROOT, "visionaray_amd", "csrc", "vrh_quad.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = r.stdout.splitlines()
    assert got[-1] == "ok", got
    m = re.match(r"records: (\d+) with 2, (\d+) with 3, (\d+) with 4 children, (\d+) unused entries, (\d+) wrong", got[0])
    assert m, got[0]
    two, three, four, unused, wrong = map(int, m.groups())
    assert two > 0 and three > 0 and four > 0 and unused == 2 * two + three and wrong == 0
    m = re.match(r"rays: (\d+) generated, (\d+) not admitted by finite_ray, (\d+) admitted with a zero reciprocal; "
                 r"unused entries: (\d+) tests, (\d+) pass; used entries: (\d+) tests, (\d+) pass; (\d+) differ", got[1])
    assert m, got[1]
    rays, refused, zero_inv, unused_tests, unused_pass, used_tests, used_pass, differ = map(int, m.groups())
    assert rays >= 10 ** 4 and 0 < refused < rays and zero_inv > 0
    assert unused_tests >= 10 ** 6 and unused_pass == 0
    assert 0 < used_pass < used_tests          # not vacuous: the used entries do pass and fail over the sweep
    assert differ == 0
    m = re.match(r"inverted box: (\d+) passes", got[2])
    assert m and int(m.group(1)) > 0, got[2]
