"""The AO disk sample (include/visionaray_hip/detail/vrh_sampler.h ao_disk_sample, the search the AO
kernel's hand-out path runs four candidates at a time) on the CPU, against a sequential restatement of
the rejection loop -- tests/cpp/ao_sample_check.cpp (host code, g++): 2^20 seeded triples, pinned samples
whose first accepted candidate lies in a later group, and the grouped selection under every forced accept
pattern ("none of 16" included)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_grouped_disk_sample_equals_the_sequential_search(tmp_path):
    exe = tmp_path / "ao_sample_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "ao_sample_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    got = r.stdout.splitlines()
    assert got[-1] == "ok", got
    assert got[0].startswith("triples: 1048576 compared") and got[0].endswith("none: 0"), got[0]
    assert got[1] == "pins: 10 checked, 2 with index >= 8", got[1]
    assert got[2].startswith("patterns: 65536 accept masks"), got[2]
