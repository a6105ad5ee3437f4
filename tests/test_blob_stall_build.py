"""The two blob-stage kernels changed for their stalls, cross-compiled for gfx950 (hipcc needs no GPU) and judged by the code
object's metadata and the device assembly alone:

  - blob_candidates_kernel (csrc/blob.hip): no scratch, at most 80 VGPRs (six waves per SIMD: three workgroups of eight waves
    per CU) and at most 32 KiB of LDS (eight waves x 512 parked indices);
  - pair_yx_kernel (csrc/gauss_pair.hip): no scratch at any half-width, at most 128 VGPRs up to H = 8 (four workgroups per CU,
    as its LDS allows there) and 168 beyond, LDS within 64 KiB;
  - the phase stamps (-DVH_BLOB_STAMPS, -DVH_PAIR_STAMPS: development builds of tools/build_variant.py) compile, read the
    shader clock, and leave nothing of themselves in the normal build."""
import os
import re
import subprocess

import pytest

from visfd_amd import build as B
from test_log_pair_build import kernel_resources

CLOCK = "s_memtime"


def _asm(tmp_path, src, flags, tag):
    s = str(tmp_path / ("%s_%s.s" % (os.path.splitext(src)[0], tag)))
    cmd = [B.HIPCC] + B.FLAGS + list(flags) + ["--cuda-device-only", "-S", "-x", "hip", os.path.join(B.CSRC, src), "-o", s]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return open(s).read()


def _one(res, kern, h=None):
    pat = r"%d%s" % (len(kern), kern) + (r"ILi%dE" % h if h is not None else "")
    hits = [(n, v) for n, v in res.items() if re.search(pat, n)]
    assert len(hits) == 1, (kern, h, sorted(res))
    return hits[0]


@pytest.mark.parametrize("stamps", [False, True], ids=["normal", "stamps"])
def test_candidate_sweep_resources(tmp_path, stamps):
    asm = _asm(tmp_path, "blob.hip", ["-DVH_BLOB_STAMPS"] if stamps else [], "stamps" if stamps else "normal")
    name, v = _one(kernel_resources(asm), "blob_candidates_kernel")
    assert v["private_segment_fixed_size"] == 0, (name, v)
    assert v["vgpr_count"] <= 80, (name, v)
    assert v["group_segment_fixed_size"] <= 32 * 1024, (name, v)
    assert (CLOCK in asm) == stamps
    assert ("g_blob_stamps" in asm) == stamps


@pytest.mark.parametrize("stamps", [False, True], ids=["normal", "stamps"])
def test_pair_yx_resources(tmp_path, stamps):
    asm = _asm(tmp_path, "gauss_pair.hip", B.PAIR_FLAGS + (["-DVH_PAIR_STAMPS"] if stamps else []), "stamps" if stamps else "normal")
    res = kernel_resources(asm)
    for h in (6, 7, 8, 9, 10):
        name, v = _one(res, "pair_yx_kernel", h)
        assert v["private_segment_fixed_size"] == 0, (name, v)
        assert v["group_segment_fixed_size"] <= 64 * 1024, (name, v)
        if not stamps:   # (the stamp build keeps five 64-bit sums per lane: a development build, no occupancy promised)
            assert v["vgpr_count"] <= (128 if h <= 8 else 168), (name, v)
            assert h > 8 or 4 * v["group_segment_fixed_size"] <= 160 * 1024, (name, v)
    assert (CLOCK in asm) == stamps
    assert ("g_pair_stamps" in asm) == stamps
