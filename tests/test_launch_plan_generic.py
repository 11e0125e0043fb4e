"""The generic-primitive axis of the launch plan (vrh_launch.h: launch_inputs::generic, generic_instance_exists)
on the CPU -- tests/cpp/launch_plan_generic_check.cpp (host code, g++): its sweep with `generic` set asserts in
the program; the named cases it prints with `generic` unset must be lines of the recorded
tests/golden/launch_plan.txt (the existing test compares the whole file)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_generic_launch_plans(tmp_path):
    exe = tmp_path / "launch_plan_generic_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "tests", "cpp", "launch_plan_generic_check.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    got = r.stdout.splitlines()
    assert got[-1].startswith("generic sweep ok: "), got[-1]
    # primary visibility, AO, simple, whitted: the one-frame step loop, one register budget each
    assert " keys=4" in got[-1], got[-1]
    with open(os.path.join(ROOT, "tests", "golden", "launch_plan.txt")) as f:
        recorded = set(f.read().splitlines())
    named = got[:-1]
    assert len(named) == 28
    for line in named:
        assert line in recorded, line
