import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (HIP device); run with -m gpu")
    config.addinivalue_line("markers", "slow: long-running CPU test")


@pytest.fixture(scope="session")
def golden():
    import json
    with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as f:
        return json.load(f)


@pytest.fixture(scope="session")
def golden_arrays():
    """golden_arrays(case): the arrays of tests/golden/<case>.npz and of its part files
    <case>.<array>.npz (make_golden.py's save_fixture splits a fixture too large for one file)."""
    import glob

    import numpy as np

    def load(case):
        d = os.path.join(ROOT, "tests", "golden")
        arrs = {}
        for path in [os.path.join(d, case + ".npz")] + sorted(glob.glob(os.path.join(d, case + ".*.npz"))):
            with np.load(path) as z:
                arrs.update({k: z[k] for k in z.files})
        return arrs
    return load


@pytest.fixture(scope="session")
def oracle_mod():
    from oracle import oracle as O
    O.build()
    return O


@pytest.fixture(scope="session")
def ctx():
    """HIP context on device 0.  GPU tests must run the native path: no skip, no fallback."""
    import visionaray_amd as va
    n = va.device_count()
    assert n > 0, "gpu-marked test but no HIP device is visible"
    c = va.Context(0)
    yield c
    c.close()
