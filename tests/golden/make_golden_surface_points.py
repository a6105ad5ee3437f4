"""Golden PLY text for tests/test_surface_points_gpu.py, written by the REAL reference program (oracle/_ref/filter_mrc_ref):
-load-progress ... -connect ... -normals-file on the synthetic thick sheet of surface_points_cases.program_scenario().  The
input image and the six tensor files are written here (and again, from the same function, by the test); the .npz holds the
PLY text, the command line and a checksum of the files the text belongs to."""
import os
import subprocess
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import surface_points_cases as SC  # noqa: E402
import volgen  # noqa: E402

REF_CLI = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "filter_mrc_ref")


def write_files(where):
    """in.rec and prog_tensor_0..5.rec into the directory; -> the CRC32 of their voxels"""
    image, tensors = SC.program_scenario()
    volgen.write_mrc(os.path.join(where, "in.rec"), image, voxel_width=1.0)
    open(os.path.join(where, "prog_info.txt"), "w").close()   # -save-progress's record of its command line: nothing to add
    crc = zlib.crc32(image.tobytes())
    for c, t in enumerate(tensors):
        volgen.write_mrc(os.path.join(where, "prog_tensor_%d.rec" % c), t, voxel_width=1.0)
        crc = zlib.crc32(t.tobytes(), crc)
    return crc


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        crc = write_files(d)
        r = subprocess.run([REF_CLI] + SC.PROGRAM_ARGS, cwd=d, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        ply = open(os.path.join(d, "n.ply"), "rb").read()
    np.savez_compressed(os.path.join(HERE, "surface_points.npz"), ply=np.frombuffer(ply, np.uint8), crc=np.int64(crc),
                        args=np.array(SC.PROGRAM_ARGS))
    print("wrote surface_points.npz: %d bytes of PLY, %d lines" % (len(ply), ply.count(b"\n")))
