import os
import sys

import numpy as np
import pytest

# torch's CPU FFT (MKL) picks a code path by processor, and the paths round float32 transforms differently: the CPU
# oracle and the goldens it is pinned to (tests/golden/make_golden.py) both take MKL's processor-independent path, so
# they agree to the tests' tolerances on any x86 host.  (Read when MKL first runs, so set before any test imports torch.)
os.environ["MKL_CBWR"] = "COMPATIBLE"

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


class _Golden(dict):
    """The arrays of a golden split in two files, read like np.load's NpzFile."""
    @property
    def files(self):
        return list(self)


def load_golden(name):
    """tests/golden/<name>.npz; where <name>_out.npz exists (make_golden.py's SPLIT: input frames too large to rewrite),
    its arrays -- the reference's outputs -- take the place of <name>.npz's own."""
    g = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    out = os.path.join(GOLDEN, name + "_out.npz")
    if not os.path.exists(out):
        return g
    with g, np.load(out, allow_pickle=False) as o:
        merged = _Golden((k, g[k]) for k in g.files)
        merged.update((k, o[k]) for k in o.files)
    return merged


@pytest.fixture(scope="session")
def golden():
    return load_golden
