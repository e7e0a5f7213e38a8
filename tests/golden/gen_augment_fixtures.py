"""Regenerates tests/golden/augment_fixtures.npz: the outputs of tests/augment_ref.py (the numpy /
scipy restatement of batchgenerators' train-time transforms) on its seeded cases, recorded with
scipy 1.15.3 -- prefiltered volumes per axis and boundary mode, spatial transforms with their
segmentations and tie masks, low-resolution round trips, blurs, contrast, gamma and one whole
pipeline.  float64, so that the GPU tests need no scipy.  Run from the repository root:
python tests/golden/gen_augment_fixtures.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import augment_ref as ref  # noqa: E402

if __name__ == "__main__":
    out = ref.build_fixtures()
    path = os.path.join(HERE, "augment_fixtures.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")
