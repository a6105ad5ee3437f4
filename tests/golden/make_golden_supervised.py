"""Golden results for the supervised blob thresholds (tests/test_supervised.py, tests/test_supervised_gpu.py): what the
reference's own filter_mrc (oracle/_ref/filter_mrc_ref, built by oracle/Makefile) does with the cases of
tests/supervised_cases.py.  Run in the build container; only supervised.npz travels -- numbers and text, no program."""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import supervised_cases as sc  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "filter_mrc_ref")
out = {}
for name, case in sc.CASES.items():
    with tempfile.TemporaryDirectory() as tmp:
        res = sc.run_program(REF, case["files"], case["args"], case["out"], tmp)
    out[name + "/kinds"] = json.dumps({fname: kind for fname, (kind, _) in case["files"].items()})
    for fname, (kind, data) in case["files"].items():
        out["%s/file/%s" % (name, fname)] = np.array(data) if kind == "text" else np.asarray(data, np.float32)
    out[name + "/returncode"] = np.int64(res["returncode"])
    out[name + "/has_kept"] = np.bool_(res["kept"] is not None)
    out[name + "/kept"] = np.array(res["kept"] or "")
    out[name + "/block"] = np.array(res["block"])
    out[name + "/remaining"] = np.array(json.dumps(res["remaining"]))
    n_kept = len((res["kept"] or "").strip().split("\n")) if res["kept"] else 0
    print("%-28s exit %d, %3d lines kept, block of %2d lines: %s" % (
        name, res["returncode"], n_kept, len(res["block"].split("\n")), " | ".join(res["remaining"])))
np.savez_compressed(os.path.join(HERE, "supervised.npz"), **out)
print("wrote supervised.npz:", len(out), "entries")
