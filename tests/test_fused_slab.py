"""The fused slab test of the AO kernel's 4-wide step (include/visionaray_hip/detail/vrh_fused_slab.h) on the
CPU -- tests/cpp/fused_slab_check.cpp, host code built with AddressSanitizer and UBSan: over seeded ray / box
cases the fused test on the widened box never fails where the exact test passes on the exact box, a widened box
contains its exact box, the +inf entry never passes, and build_quads refuses the fused records for a tree with
one child bound one ulp outside its parent."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fused_test_on_widened_boxes_is_conservative(tmp_path):
    exe = tmp_path / "fused_slab_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "fused_slab_check.cpp"),
                    os.path.join(ROOT, "visionaray_amd", "csrc", "vrh_quad.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = r.stdout.splitlines()
    assert got[-1] == "ok", got
    m = re.match(r"cases: (\d+) generated, (\d+) eligible, (\d+) exact passes, (\d+) of them fail the fused test on "
                 r"the exact box \([\d.]+ %\), (\d+) fail it on the widened box", got[0])
    assert m, got[0]
    generated, eligible, passes, plain_fail, widened_fail = map(int, m.groups())
    assert generated >= 10 ** 6 and passes >= 10 ** 6
    assert widened_fail == 0
    # not vacuous: on the exact boxes the fused test does lose leaves the exact test keeps
    assert plain_fail * 100 >= passes, (plain_fail, passes)
    assert got[2] == "widened boxes: 0 not containing their exact box; +inf entry: 0 passes", got[2]
    assert got[3] == "upload: nested tree gets fused records", got[3]
    assert got[4] == "upload: widening option applies", got[4]
    assert got[5] == "upload: one ulp outside the parent keeps the exact records only", got[5]
