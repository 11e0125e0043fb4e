"""The octant form of the AO kernel's 4-wide entry test (include/visionaray_hip/detail/vrh_octant.h) and its
precondition (vrh_quad.cpp build_quads), on the CPU -- host code built as programs of their own, plainly and with
AddressSanitizer and UBSan.

tests/cpp/quad_octant_check.cpp: over more than a million random boxes and finite rays, the same number in each of
the eight octants, and over the edge cases (flat boxes, the origin on a plane, differences that underflow, inv at
+-FLT_MAX and +-FLT_MIN, the never-hit box, radius 0 and FLT_MAX) the octant form gives the pass / fail, the tn and the
tf of quad_entry<true>, +0 and -0 counting as equal.

tests/cpp/quad_precondition_check.cpp: build_quads gives every fixture scene its records, and none to a tree with
one inverted box or one NaN bound."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visionaray_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def build_and_run(tmp_path, name, sources, flags):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall"] + flags
                   + ["-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", name + ".cpp")]
                   + [os.path.join(CSRC, f) for f in sources] + ["-pthread", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]        # the sanitizers stayed silent, too
    got = r.stdout.splitlines()
    assert got[-1] == "ok", got
    return got


@pytest.mark.parametrize("flags", [[], SANITIZE], ids=["plain", "asan_ubsan"])
def test_octant_entry_equals_the_sorting_entry(tmp_path, flags):
    got = build_and_run(tmp_path, "quad_octant_check", [], flags)
    m = re.match(r"random: (\d+) cases, (\d+) per octant, (\d+) pass, (\d+) differ, (\d+) differ from the mirror", got[0])
    assert m, got[0]
    cases, per_octant, passed, differ, mirror = map(int, m.groups())
    assert cases >= 10 ** 6 and cases == 8 * per_octant and 0 < passed < cases and differ == 0 and mirror == 0
    m = re.match(r"edges: (\d+) cases, (\d+) pass, (\d+) differ, (\d+) differ from the mirror, (\d+) zeros of the other sign, "
                 r"(\d+) rays left out; never-hit box: (\d+) cases, (\d+) pass, (\d+) differ, (\d+) with a NaN distance", got[1])
    assert m, got[1]
    cases, passed, differ, mirror, zeros, left_out, never, never_pass, never_differ, never_nan = map(int, m.groups())
    assert cases > 10 ** 5 and 0 < passed < cases and differ == 0 and mirror == 0
    assert zeros > 0                    # not vacuous: the two forms do return zeros of opposite signs
    assert left_out < cases // 20
    assert never > 0 and never_pass == 0 and never_differ == 0 and never_nan > 0


@pytest.mark.parametrize("flags", [[], SANITIZE], ids=["plain", "asan_ubsan"])
def test_build_quads_refuses_boxes_that_are_not_ordered(tmp_path, flags):
    got = build_and_run(tmp_path, "quad_precondition_check", ["vrh_quad.cpp", "vrh_build.cpp", "vrh_scenes.cpp"], flags)
    m = re.match(r"fixture scenes: (\d+) of (\d+) accepted, (\d+) used entries \((\d+) flat axes\), (\d+) unused, (\d+) wrong", got[0])
    assert m, got[0]
    accepted, scenes, used, flat, unused, wrong = map(int, m.groups())
    assert accepted == scenes == 5 and used > 10 ** 4 and flat > 0 and unused > 0 and wrong == 0
    m = re.match(r"one inverted box or one NaN bound: (\d+) trees, (\d+) refused", got[1])
    assert m and int(m.group(1)) == 27 and int(m.group(2)) == 27, got[1]
