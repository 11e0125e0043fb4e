"""GPU: examples/multi_volume_hip.cpp -- the multi-volume example on visionaray_hip/standalone.h through
make_hip_multi_volume_kernel and hip_sched::frame -- reproduces tests/golden/mv_example.npz when it is given the
fixture's three stand-in volumes and camera in place of its procedural ones: the transforms, transfer functions,
materials, light and constants are the program's own.  Alpha, prim_id and t bit for bit, rgb to rtol 1e-5, the step
total equal."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mv_cases as MC  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, "build", "examples", "multi_volume_hip")


def test_example_reproduces_the_fixture(ctx, tmp_path):
    F = MC.load_frame("mv_example")
    W, H = MC.FRAME_W, MC.FRAME_H
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    payload = struct.pack("<2I", W, H) + np.ascontiguousarray(F["look_at"], np.float32).tobytes()
    for i in range(3):
        v = F["voxels_%d" % i]
        payload += struct.pack("<3I", v.shape[2], v.shape[1], v.shape[0]) + np.ascontiguousarray(v, np.float32).tobytes()
    src.write_bytes(payload)
    r = subprocess.run([EXAMPLE, "--volumes", str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = dst.read_bytes()
    px = W * H
    assert len(raw) == px * 24 + 16
    got = {"color": np.frombuffer(raw, np.float32, px * 4).reshape(px, 4), "prim_id": np.frombuffer(raw, np.uint32, px, px * 16),
           "t": np.frombuffer(raw, np.float32, px, px * 20)}
    rays, steps = (int(x) for x in np.frombuffer(raw, np.uint64, 2, px * 24))
    assert rays == px and steps == int(F["total_steps"][0])
    MC.check_frame(got, F, "multi_volume_hip")         # colour, and prim_id / t as hip_buffer_rt::download hands them out
    assert np.all(got["color"][~F["hit"].astype(bool)] == 0.0)


def test_example_renders_its_procedural_scene(ctx):
    """the program's own scene at a quarter of the volumes' side lengths: hits, misses, steps"""
    r = subprocess.run([EXAMPLE, "96", "64", "", "0.25"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    import json
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["rays"] == 96 * 64 and rec["capped"] == 0 and rec["steps"] > 96 * 64
