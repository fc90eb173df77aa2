"""Writes tests/golden/dpmpp_2m_ref.npz: the float64 Heun solution at n = 96 (191 evaluations of the CPU oracle's float32 EDMPrecond,
about 20 s) of the model case of tests/dpmpp_2m.py - the reference the solvers' discretisation errors are measured against in
tests/test_dpmpp_2m_cpu.py and tools/solver_tradeoff.py.  Stored so that the CPU suite does not repeat those evaluations.

    python tools/make_golden_dpmpp_2m.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dex_tts_amd.edm import ablation_tables  # noqa: E402
from tests import dpmpp_2m as R  # noqa: E402

N_REF = 96


def main():
    net32, z, _ = R.model_case()
    sig = ablation_tables(N_REF, "euler", "edm", "linear", "none").sigma.numpy()
    ref = R.heun(R.f64_around(net32), z, sig).numpy()
    path = os.path.join(ROOT, "tests", "golden", R.GOLDEN)
    np.savez_compressed(path, heun96=ref.astype(np.float32), n=np.int64(N_REF))
    print(f"{path}: {os.path.getsize(path)} bytes, |ref|max {np.abs(ref).max():.3f}")


if __name__ == "__main__":
    main()
