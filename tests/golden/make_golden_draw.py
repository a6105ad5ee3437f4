"""Golden images for tests/test_draw*.py, recorded from the REAL reference program (oracle/_ref/filter_mrc_ref, built by
`make -C oracle ref_cli`): for every case of draw_cases.CLI_CASES the image of -out and the text files the run writes
(blob and extrema lists).  For the blob cases the lists of the reference's BlobDogD itself (oracle/_ref/libvisfd_ref.so,
`make -C oracle ref`) are recorded as well, in detection order and with every digit: the program draws from them, and its
text files round them.  Inputs are not stored: draw_cases.cli_inputs rebuilds them.  A case whose reference run does not
exit 0 is left out and named; at most one may be.

The reference runs on ONE thread (OMP_NUM_THREADS=1).  Its blob detector collects each scale's candidates per thread and
appends the threads' lists as they finish (feature.hpp:212-346), so with several threads the order of its lists -- and with
it the picture of `-blob ... -out`, which pairs the unsorted coordinates with the sorted diameters and scores
(handlers.cpp:876-950) -- changes from run to run.  On one thread the order is the raster order within each scale."""
import os
import subprocess
import sys
import tempfile

os.environ["OMP_NUM_THREADS"] = "1"   # before anything loads an OpenMP runtime: see above

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import draw_cases as DC  # noqa: E402
import volgen  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import pyoracle  # noqa: E402

REF_CLI = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "filter_mrc_ref")


def main():
    out, left_out = {}, []
    with tempfile.TemporaryDirectory() as d:
        for name in sorted(DC.CLI_CASES):
            r = subprocess.run(DC.cli_command(name, REF_CLI, d), cwd=d, capture_output=True, text=True)
            if r.returncode != 0:
                left_out.append(name)
                continue
            out[name + "/out"] = volgen.read_mrc(os.path.join(d, "out.rec"))
            for f in DC.WRITTEN.get(name, []):
                path = os.path.join(d, f)
                out[name + "/" + f] = np.array(open(path).read() if os.path.exists(path) else "")
    R = pyoracle.load("ref")
    for name, spec in DC.BLOB_DETECT.items():
        if name in left_out:
            continue
        img, mask, _, w = DC.cli_inputs(name)
        diam = volgen.cli_blob_diameters(*spec["ladder"], 1.0) / np.float32(w)
        mins, maxs = R.blob_dog(img, R.diameters_to_sigmas(diam), mask, None, 0.02, R.ratio_from_threshold(0.03),
                                spec["minima_threshold"], spec["maxima_threshold"], False)
        for tag, rows in (("minima", mins), ("maxima", maxs)):
            rows = rows.copy()
            rows[:, 3] = R.sigmas_to_diameters(np.ascontiguousarray(rows[:, 3]))   # x, y, z, diameter (voxels), score
            out[name + "/" + tag + "_exact"] = rows
    assert len(left_out) <= 1, left_out
    path = os.path.join(HERE, "draw.npz")
    np.savez_compressed(path, **out)
    print("wrote draw.npz: %d cases, %d bytes; left out (reference did not exit 0): %s"
          % (len(DC.CLI_CASES) - len(left_out), os.path.getsize(path), left_out or "none"))


if __name__ == "__main__":
    main()
