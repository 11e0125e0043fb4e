"""GPU: the fused 4-wide records of the AO kernel (vrh_fused_slab.h).  They measured slower than the exact records
(DESIGN.md section 8), so the default library is built without them and libvrh_fused.so with them
(VRH_FUSED_STEP): the cases of tests/fused_cases.py -- every frame bit-identical to the oracle -- run
in one child process that loads that library; the default library shows that it has no fused records."""
import os
import re
import subprocess
import sys

import pytest

import visionaray_amd as va
from visionaray_amd import scenes

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FUSED_LIB = os.path.join(os.path.dirname(HERE), "visionaray_amd", "_lib", "libvrh_fused.so")


def test_fused_library_renders_the_oracles_frames():
    assert os.path.exists(FUSED_LIB), "build() makes libvrh_fused.so"
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-s", "-p", "no:cacheprovider", "-m", "gpu",
                        os.path.join(HERE, "fused_cases.py")], env={**os.environ, "VRH_LIB": FUSED_LIB},
                       cwd=os.path.dirname(HERE), capture_output=True, text=True, timeout=600)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == 51 and "failed" not in r.stdout.splitlines()[-1]


def test_default_library_has_no_fused_records(ctx):
    prims = scenes.primitives("hf24")
    ctx.set_option("fused_step", 1)
    try:
        d = va.hip_index_bvh(ctx, va.build_index_bvh(prims), scenes.normals_for(prims))
    finally:
        ctx.set_option("fused_step", 0)
    assert d.info["wide_records"] > 0 and d.info["fused_records"] == 0 and d.info["fused_bytes"] == 0
    d.close()
