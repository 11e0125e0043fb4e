"""The generic-primitive axis of the launch plan (vrh_launch.h: launch_inputs::generic, generic_instance_exists)
on the CPU -- tests/cpp/launch_plan_generic_check.cpp (host code, g++): its sweep with `generic` set asserts in
the program; the named cases it prints with `generic` unset must be lines of the recorded
tests/golden/launch_plan.txt (the existing test compares the whole file).  With the argument `limits` it prints
the deepest generic BVH each kernel's plan accepts at default options (and asserts that every shallower one is
accepted and every deeper one refused for LDS): the constants of tests/gp_cases.py DEPTH_LIMIT, at which
tests/test_gpu_generic.py renders."""
import os
import subprocess

import gp_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compiled(tmp_path):
    exe = tmp_path / "launch_plan_generic_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "tests", "cpp", "launch_plan_generic_check.cpp"),
                    "-o", str(exe)], check=True)
    return exe


def test_generic_depth_limits_are_the_recorded_ones(tmp_path):
    r = subprocess.run([str(compiled(tmp_path)), "limits"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr         # includes: one deeper is refused for LDS
    got = {k: int(v) for k, v in (line.split() for line in r.stdout.splitlines())}
    assert got == G.DEPTH_LIMIT
    # the arithmetic behind them: 64 lanes x 4 bytes per entry, entries in fours, of a CU's 160 KiB less the AO
    # kernel's per-wave area (552 words) / whitted's bounce surface (12 words per lane)
    assert got["primary"] == got["simple"] == 160 * 1024 // 256
    assert got["ao"] == (160 * 1024 - 552 * 4) // 256 // 4 * 4 and got["whitted"] == (160 * 1024 - 12 * 64 * 4) // 256 // 4 * 4


def test_generic_launch_plans(tmp_path):
    exe = compiled(tmp_path)
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
