"""The launch plan of vrh_render (visionaray_amd/csrc/vrh_launch.h: which render_unified_kernel instance a
frame runs, its block, LDS stack and tuning values) on the CPU, against a stated model of the occupancy
query -- tests/cpp/launch_plan_check.cpp (host code, g++), one section per argument.

Its named cases must equal tests/golden/launch_plan.txt, recorded from a line-by-line transcript of the
decision as vrh_render made it before it became plan_launch; the last line of the file is the program's
sweep of the plain flavour's input space (its in-program assertions, the number of keys with an instance and a
digest of every decision).  A deliberate change of a default changes the file with it.

The textured and the generic-primitive flavour have a sweep each (sections `textured`, `generic`); the named
cases those sections print, with nothing of the flavour set, must be lines of launch_plan.txt.  Section
`flavours` runs the three sweeps and checks the whole key domain against what they produced:
tests/golden/launch_plan_flavours.txt (the textured and generic digests cover the refusals' texts too; like
launch_plan.txt they change only with a deliberate change of the plan).  Section `limits` prints the deepest generic-primitive BVH each
kernel's plan accepts at default options (and asserts that every shallower one is accepted and every deeper one
refused for LDS): the constants of tests/gp_cases.py DEPTH_LIMIT, at which tests/test_gpu_generic.py renders."""
import os
import subprocess

import pytest

import gp_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return f.read().splitlines()


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("launch_plan") / "launch_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "tests", "cpp", "launch_plan_check.cpp"),
                    "-o", str(exe)], check=True)

    def run(*section):
        r = subprocess.run([str(exe), *section], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr         # includes the program's own assertions
        return r.stdout.splitlines()
    return run


def test_launch_plan_matches_the_recorded_decisions(check):
    got = check()
    want = golden("launch_plan.txt")
    assert got[-1].startswith("sweep ok: ") and " keys=114 " in got[-1], got[-1]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w


def test_textured_launch_plans(check):
    got = check("textured")
    assert got[-1].startswith("textured sweep ok: "), got[-1]
    # simple, whitted: one frame; path, path_generic: one frame, frames in flight, the sampler pass -- all uncapped
    assert " keys=8 " in got[-1], got[-1]
    recorded = set(golden("launch_plan.txt"))
    named = got[:-1]
    assert len(named) == 20
    for line in named:
        assert line in recorded, line


def test_generic_launch_plans(check):
    got = check("generic")
    assert got[-1].startswith("generic sweep ok: "), got[-1]
    # primary visibility, AO, simple, whitted: the one-frame step loop, one register budget each
    assert " keys=4 " in got[-1], got[-1]
    recorded = set(golden("launch_plan.txt"))
    named = got[:-1]
    assert len(named) == 28
    for line in named:
        assert line in recorded, line


def test_generic_depth_limits_are_the_recorded_ones(check):
    got = {k: int(v) for k, v in (line.split() for line in check("limits"))}      # includes: one deeper is refused for LDS
    assert got == G.DEPTH_LIMIT
    # the arithmetic behind them: 64 lanes x 4 bytes per entry, entries in fours, of a CU's 160 KiB less the AO
    # kernel's per-wave area (552 words) / whitted's bounce surface (12 words per lane)
    assert got["primary"] == got["simple"] == 160 * 1024 // 256
    assert got["ao"] == (160 * 1024 - 552 * 4) // 256 // 4 * 4 and got["whitted"] == (160 * 1024 - 12 * 64 * 4) // 256 // 4 * 4


def test_every_flavour_decides_as_recorded_and_the_key_domain_holds_exactly_the_produced_instances(check):
    got = check("flavours")
    want = golden("launch_plan_flavours.txt")
    assert got == want
    # the plain sweep is the one of launch_plan.txt; every sweep's decisions, refusals' texts included, are the recorded ones
    assert got[0] == golden("launch_plan.txt")[-1]
    assert [line.split(" sweep ok: ")[0] for line in got[1:3]] == ["textured", "generic"]
    assert [line.split(" keys=")[1].split()[0] for line in got[:3]] == ["114", "8", "4"]
    # key_index(key_at(i)) == i over the folded domain; an instance exists for exactly the produced keys; none outside
    assert got[3] == "key domain ok: keys=18432 instances=126"
