"""Golden vectors for tests/test_intensity.py and tests/test_intensity_gpu.py, recorded from the REAL reference program
(oracle/_ref/filter_mrc_ref, built by `make -C oracle ref_cli`): for every case of tests/intensity_cases.py what the program
wrote to -out and the dmin, dmax, dmean of that file's header; for the cases that follow a filter, also what the filter
alone wrote (the image the tail starts from).  Inputs, masks and outputs only."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import intensity_cases as ic  # noqa: E402
import volgen  # noqa: E402

REF_CLI = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "filter_mrc_ref")


def header_stats(path):
    with open(path, "rb") as f:
        return np.frombuffer(f.read(1024), "<f4")[19:22].copy()


def filter_flags(flags):
    """the flags of the filter a case runs before its tail (none: [])"""
    return list(flags[:2]) if flags and flags[0] == "-gauss" else []


def main():
    inputs = ic.inputs()
    out = {}
    for name in ("dyadic", "dyadic_sel", "wide"):
        out["in/" + name] = inputs[name][0]
        if inputs[name][1] is not None:
            out["mask/" + name] = inputs[name][1]
    env = dict(os.environ, OMP_NUM_THREADS="1")
    with tempfile.TemporaryDirectory() as d:
        for name, (vol, mask) in inputs.items():
            volgen.write_mrc(os.path.join(d, name + ".rec"), vol, voxel_width=ic.voxel_width(name))
            if mask is not None:
                volgen.write_mrc(os.path.join(d, name + "_mask.rec"), mask, voxel_width=ic.voxel_width(name))
        for case in ic.CASES:
            name, input_name, use_mask, flags = case
            runs = [("out/" + name, case)]
            if filter_flags(flags):
                runs.append(("filtered/" + name, (name, input_name, use_mask, filter_flags(flags))))
            for key, c in runs:
                args = ic.command(c, REF_CLI, input_name + ".rec", input_name + "_mask.rec", "out.rec")
                p = subprocess.run(args, cwd=d, capture_output=True, text=True, timeout=120, env=env)
                assert p.returncode == 0, (args, p.stderr[-2000:])
                out[key] = volgen.read_mrc(os.path.join(d, "out.rec"))
                if key.startswith("out/"):
                    out["header/" + name] = header_stats(os.path.join(d, "out.rec"))
                os.remove(os.path.join(d, "out.rec"))
    path = os.path.join(HERE, "intensity.npz")
    np.savez_compressed(path, **out)
    print("wrote intensity.npz: %d bytes, %d arrays" % (os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
