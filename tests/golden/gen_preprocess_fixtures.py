"""Regenerates tests/golden/preprocess_fixtures.npz: scipy.ndimage.binary_fill_holes (recorded
with scipy 1.15.3) of the hole-fill cases of tests/preprocess_ref.py -- the filled masks as
packed bits, and for the mid-size ellipsoid case its bounding box, voxel count and the SHA-256
of the packed mask.  Run from the repository root:  python tests/golden/gen_preprocess_fixtures.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import preprocess_ref as ref  # noqa: E402

if __name__ == "__main__":
    out = ref.build_fixtures()
    path = os.path.join(HERE, "preprocess_fixtures.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")
