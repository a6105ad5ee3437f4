"""bench.py's output contract on a small volume (GPU): one JSON line with the fields the driver reads; with --full the
roofline objects and the CPU baseline; --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def run_bench(*args, timeout=900):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + [str(a) for a in args], capture_output=True,
                       text=True, cwd=ROOT, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    """A plain run: the headline fields only, `--steps` timed steps, and with --dump-outputs the outputs of the last timed
    step as float .npy files (at most 64 MB), identical from run to run."""
    dumps = []
    for tag in ("a", "b"):
        out = run_bench("--size", 128, "--steps", 3, "--warmup", 1, "--dump-outputs", tmp_path / tag)
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "stages_ms", "roofline_pipeline"):
            assert key in out, key
        assert out["steps"] == 3 and out["modes"]["tolerance"]["steps"] == 3 and set(out["modes"]) == {"tolerance"}
        assert out["unit"] == "Mvoxels/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
        assert abs(out["value"] - 128 ** 3 / (out["ms_per_step"] * 1e-3) / 1e6) <= 1e-3 * out["value"]
        for key in ("cpu_baseline", "roofline", "roofline_gauss", "roofline_2048", "copy_gbs"):
            assert key not in out, key
        files = sorted(os.listdir(tmp_path / tag))
        assert files == sorted(n + ".npy" for n in ("gauss", "blob_minima", "blob_maxima", "membrane_threshold",
                                                     "membrane_saliency", "vote_tensor")), files
        assert sum(os.path.getsize(tmp_path / tag / f) for f in files) <= 64 << 20
        arrays = {f: np.load(tmp_path / tag / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert len(arrays["blob_minima.npy"]) == out["results"]["minima"] and arrays["vote_tensor.npy"].shape[0] == 6
        assert arrays["membrane_threshold.npy"][0] == out["results"]["threshold"] and np.abs(arrays["gauss.npy"]).max() > 0
        dumps.append(arrays)
    for f in dumps[0]:
        assert np.array_equal(dumps[0][f], dumps[1][f]), f


@pytest.mark.gpu
def test_bench_prints_one_json_line_with_the_contract_fields():
    out = run_bench("--size", 128, "--steps", 1, "--warmup", 1, "--no-2048", "--cpu-sample", 48, "--full")
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in out, key
    assert out["unit"] == "Mvoxels/s" and out["n_gpus"] == 1 and out["steps"] == 1 and out["higher_is_better"] is True
    assert out["scaling"] == "weak" and out["vs_baseline"] is None and out["dtype"] == "f32" and out["data"] == "synthetic"
    assert "workload" in out["config"] and "model" not in out["config"]
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert abs(out["value"] - 128 ** 3 / (out["ms_per_step"] * 1e-3) / 1e6) <= 1e-3 * out["value"]
    rf = out["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in rf, key
    # `roofline` describes the DOMINANT kernel of the step (tensor voting: a VALU-bound stencil priced in TFLOP/s against the
    # FP32 vector peak); the HBM-bound kernel BASELINE.json names is `roofline_gauss`
    assert rf["bound"] == "valu" and rf["unit"] == "TFLOP/s" and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    assert "tv_box_kernel" in rf["kernel"] and 0 < rf["share_of_step"] <= 1.0
    rg = out["roofline_gauss"]
    assert rg["bound"] == "hbm" and rg["unit"] == "GB/s" and abs(rg["frac"] - rg["achieved"] / rg["peak"]) < 1e-3
    assert abs(rg["frac_of_copy"] - rg["achieved"] / out["copy_gbs"]) < 1e-3 and rg["tolerance_mode"]["bound"] == "hbm"
    assert out["config"]["mode"] == "tolerance" and set(out["modes"]) == {"tolerance", "exact"}
    assert out["modes"]["exact"]["results"]["minima"] == out["modes"]["tolerance"]["results"]["minima"]   # indices: exact in both
    assert out["modes"]["exact"]["results"]["maxima"] == out["modes"]["tolerance"]["results"]["maxima"]
    cb = out["cpu_baseline"]
    for key in ("value", "unit", "cores", "kind", "sample", "cpu_model", "omp"):
        assert key in cb, key
    assert cb["kind"] in ("reference", "port") and cb["cores"] >= 1 and cb["value"] > 0
    # the best of three OpenMP teams -- every host thread, 64, the per-GPU share of 16 -- each bound close, each in
    # a process of its own; all of them listed
    assert cb["omp"]["OMP_PROC_BIND"] == "close" and len(cb["teams"]) >= 1
    assert max(t["cores"] for t in cb["teams"]) == os.cpu_count() and cb["value"] == max(t["value"] for t in cb["teams"])
    assert set(out["roofline_tv"]) == {"exact", "tolerance"} and out["roofline_tv"]["exact"]["bound"] == "valu"
    assert out["roofline_pass"]["bound"] == "hbm" and "ridge_score_kernel" in out["roofline_ridge"]
    rr = out["roofline_ridge"]   # the eigen kernels against the FP64 vector peak
    for k in ("ridge_score_kernel", "ridge_directions_kernel", "tensor_saliency_kernel"):
        assert rr[k]["fp64_flop_per_voxel"] > 0 and 0 < rr[k]["frac_fp64"] < 1
        assert abs(rr[k]["frac_fp64"] - rr[k]["achieved_fp64_tflops"] / rr["peak_tflops_fp64_vector"]) < 2e-3
    rp = out["roofline_pipeline"]   # the BASELINE metric's own "% HBM roofline"
    assert rp["algorithmic_bytes_per_voxel"] == 336.0 and set(rp["stages"]) == {"gauss", "blob_dog", "membrane_tv"}
    assert abs(rp["frac"] - rp["achieved"] / rp["peak"]) < 1e-3
    assert abs(rp["achieved"] - 336.0 * 128 ** 3 / (out["ms_per_step"] * 1e-3) / 1e9) <= 0.02 * rp["achieved"] + 0.1
