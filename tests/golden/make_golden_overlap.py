"""Golden vectors for the overlap suppression tests (tests/test_overlap.py, tests/test_overlap_gpu.py): the lists of
tests/overlap_cases.py through the REAL reference's DiscardOverlappingBlobs (oracle/_ref; only the .npz travels)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import pyoracle as po  # noqa: E402
from overlap_cases import CASES  # noqa: E402

R = po.load("ref")
out = {}
for name, (c, d, s, sep, ml, ms, crit, scale) in CASES.items():
    out[name + "_c"], out[name + "_d"], out[name + "_s"] = R.discard_overlapping_blobs(c, d, s, sep, ml, ms, crit, scale)
np.savez_compressed(os.path.join(HERE, "overlap.npz"), **out)
print("wrote overlap.npz:", len(out), "arrays; kept counts:", {name: len(out[name + "_d"]) for name in CASES})
