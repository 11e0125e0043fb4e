"""The launch plan of vrh_render (visionaray_amd/csrc/vrh_launch.h: which render_unified_kernel instance a
frame runs, its block, LDS stack and tuning values) on the CPU, against a stated model of the occupancy
query -- tests/cpp/launch_plan_check.cpp (host code, g++).

Its named cases must equal tests/golden/launch_plan.txt, recorded from a line-by-line transcript of the
decision as vrh_render made it before it became plan_launch; the last line of the file is the program's
sweep of the whole input space (its in-program assertions, the number of keys with an instance and a
digest of every decision).  A deliberate change of a default changes the file with it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_plan_matches_the_recorded_decisions(tmp_path):
    exe = tmp_path / "launch_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "tests", "cpp", "launch_plan_check.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    got = r.stdout.splitlines()
    with open(os.path.join(ROOT, "tests", "golden", "launch_plan.txt")) as f:
        want = f.read().splitlines()
    assert got[-1].startswith("sweep ok: ") and " keys=114 " in got[-1], got[-1]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
