"""The host half of vrh_scene_upload (visionaray_amd/csrc/vrh_upload.cpp prepare_scene) on the CPU --
tests/cpp/scene_prepare_check.cpp, host code built with AddressSanitizer and UBSan as a program of its own.

Identity: every output array (as an FNV-1a-64 hash) and scalar of small trees of each primitive kind, under both pair
layouts, never-hit unused entries on and off and fused records off / on, equals tests/golden/scene_prepare.txt.  That
file was recorded from the body of vrh_scene_upload as it stood before prepare_scene was split from it (compiled next to
the new unit, which it equalled byte for byte on every array), not from the new unit.  Refusals: every malformed input
is refused with VRH_ERR_INVALID and the message the same file holds, recorded the same way.  Properties: END flags, the
layout-1 permutation, the comb's depth, no records over a non-finite bound, the generic sphere flag."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visionaray_amd", "csrc")

# the messages no other test sees, and which defect of two is reported: spelled out here as well as in the golden file
MESSAGES = {
    "even_node_count": "vrh_scene_upload: node count must be odd (root + child pairs)",
    "root_first_not_1": "vrh_scene_upload: root children must be nodes 1,2",
    "leaf_range_past_indices": "vrh_scene_upload: malformed node pair 3",
    "inner_first_0": "vrh_scene_upload: malformed node pair 0",
    "root_leaf_past_indices": "vrh_scene_upload: malformed root node",
    "pair_with_two_parents": "vrh_scene_upload: BVH is not a tree (a node pair is reached twice)",
    "cycle_to_ancestor": "vrh_scene_upload: BVH is not a tree (a node pair is reached twice)",
    "index_out_of_range": "vrh_scene_upload: index out of range",
    "generic_type_0": "vrh_scene_upload: generic primitive 5 has type index 0 (1 triangle, 2 sphere)",
    "generic_type_3": "vrh_scene_upload: generic primitive 31 has type index 3 (1 triangle, 2 sphere)",
    "unknown_kind": "vrh_scene_upload: unknown prim_kind",
    "zero_nodes": "vrh_scene_upload: empty BVH",
    "zero_prims": "vrh_scene_upload: empty BVH",
    "even_node_count_and_index_out_of_range": "vrh_scene_upload: node count must be odd (root + child pairs)",
    "cycle_and_index_out_of_range": "vrh_scene_upload: BVH is not a tree (a node pair is reached twice)",
    "generic_type_and_malformed_pair": "vrh_scene_upload: generic primitive 2 has type index 9 (1 triangle, 2 sphere)",
}


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = tmp_path_factory.mktemp("scene_prepare") / "scene_prepare_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "scene_prepare_check.cpp")]
                   + [os.path.join(CSRC, f) for f in ("vrh_upload.cpp", "vrh_quad.cpp", "vrh_build.cpp", "vrh_scenes.cpp")]
                   + ["-pthread", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]        # the sanitizers stayed silent, too
    got = r.stdout.splitlines()
    assert got[-1] == "ok", got[-3:]
    return got


def test_outputs_and_refusals_equal_the_recorded_ones(output):
    with open(os.path.join(ROOT, "tests", "golden", "scene_prepare.txt")) as f:
        want = f.read().splitlines()
    got = output[:-2]
    assert len(want) == 128 + 19 and sum(l.startswith("refused ") for l in want) == 19
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)


def test_every_refusal_is_invalid_with_its_message(output):
    refused = dict(re.match(r"refused (\S+): (.*)", l).groups() for l in output if l.startswith("refused "))
    assert len(refused) == 19
    for name, text in refused.items():
        assert text.startswith("1 vrh_scene_upload: "), (name, text)          # VRH_ERR_INVALID
    for name, text in MESSAGES.items():
        assert refused[name] == "1 " + text


def test_properties_were_checked_on_something(output):
    m = re.match(r"checked: (\d+) runs, (\d+) refusals, (\d+) END flags set, (\d+) clear, (\d+) layout-1 links, "
                 r"(\d+) child-0 pairs, (\d+) generic sphere records, (\d+) generic triangle records, (\d+) mixed leaves, "
                 r"(\d+) non-finite runs, (\d+) with 4-wide records, (\d+) with fused records, (\d+) failures", output[-2])
    assert m, output[-2]
    (runs, refusals, end_set, end_clear, links, child0, spheres, tris, mixed, nonfinite, quads, fused, failures) = map(int, m.groups())
    assert runs == 128 and refusals == 19 and failures == 0
    assert end_set > 0 and end_clear > 0 and links > 0 and child0 > 0
    assert spheres > 0 and tris > 0 and mixed > 0
    assert nonfinite == 16 and 0 < fused < quads < runs
