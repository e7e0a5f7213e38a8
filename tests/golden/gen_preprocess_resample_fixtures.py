"""Regenerates tests/golden/preprocess_resample_fixtures.npz: the outputs of tests/resample_ref.py
(the numpy / scipy restatement of the reference's resampling step) on its seeded cases, recorded
with scipy 1.15.3 -- per data case the clamped float64 resize and cmax, the largest magnitude
among the input and every intermediate of the float64 separable form; per segmentation case the
order-1 and order-0 results and the packed tie mask; and the end-to-end case.  The generator
asserts that the clamp sets at least 10 % of every data case's outputs, that the separable form
equals scipy's zoom to 1e-12 cmax, and that no tie mask covers more than 5 % of its case.  Run
from the repository root: python tests/golden/gen_preprocess_resample_fixtures.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import resample_ref as ref  # noqa: E402

if __name__ == "__main__":
    out = ref.build_fixtures()
    path = os.path.join(HERE, "preprocess_resample_fixtures.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")
