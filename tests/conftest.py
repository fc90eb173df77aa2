import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
# torch's intra-op thread count the CPU goldens were written with (oracle/make_golden.py: torch.set_num_threads(8)).  The CPU kernels
# split their reductions by it, so a bit-exact oracle-vs-golden comparison holds only at this count, whatever the host's core count.
# (It still needs a CPU whose fp32 kernels round like those of the one the goldens were written on.)
GOLDEN_THREADS = 8


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden_dir():
    return GOLDEN


@pytest.fixture
def golden_threads():
    """Run the test with torch at GOLDEN_THREADS intra-op threads (restored afterwards)."""
    import torch
    prev = torch.get_num_threads()
    torch.set_num_threads(GOLDEN_THREADS)
    yield
    torch.set_num_threads(prev)
