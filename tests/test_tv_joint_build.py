"""csrc/tv_box.hip cross-compiled for gfx950 (hipcc needs no GPU): the flagship instantiation of the tolerance-mode voting
kernel, tv_box_kernel<0, true> (exponent 4, folded saliencies: the 17-instruction vote with the square-root table), keeps
the resources its speed rests on -- 80 VGPRs (six waves per SIMD), no more scratch memory than the kernel had before
(profiles/tv_joint_resources.txt records that figure) and, at the flagship window h = 12, three workgroups per CU."""
import os
import re
import subprocess

from test_log_pair_build import kernel_resources
from visfd_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 160 * 1024
NT = 512            # csrc/tv_common.hpp: box_tile
NW = NT // 64
HCAP = 36           # csrc/tv_box.hip: hit entries per (wave, sub-patch, stream)


def box_row(h):     # csrc/tv_common.hpp: tv_box_row
    sp = 2 * h + 1 + 3
    while (sp & 7) != 4:
        sp += 1
    return sp


def box_slice(h):   # csrc/tv_common.hpp: tv_box_slice
    return (2 * h + 1 + 6) * box_row(h) + 8


def tol_kernel(res):
    hits = [(n, v) for n, v in res.items() if re.search(r"13tv_box_kernelILi0ELb1EE", n)]
    assert len(hits) == 1, sorted(res)
    return hits[0]


def recorded_parent_scratch():
    text = open(os.path.join(ROOT, "profiles", "tv_joint_resources.txt")).read()
    m = re.search(r"^parent\s+tv_box_kernel<0,true>.*?private_segment_fixed_size\s+(\d+)", text, re.M)
    assert m, "profiles/tv_joint_resources.txt has no parent line for tv_box_kernel<0,true>"
    return int(m.group(1))


def test_tolerance_kernel_resources(tmp_path):
    s = str(tmp_path / "tv_box.s")
    flags = dict((src, extra) for src, _stem, extra in B.TV_VARIANT)["tv_box.hip"]
    cmd = [B.HIPCC] + B.FLAGS + flags + ["--cuda-device-only", "-S", "-x", "hip", os.path.join(B.CSRC, "tv_box.hip"), "-o", s]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    name, v = tol_kernel(kernel_resources(open(s).read()))
    assert v["vgpr_count"] <= 80, (name, v)
    assert recorded_parent_scratch() == 8
    assert v["private_segment_fixed_size"] <= recorded_parent_scratch(), (name, v)
    # dev_tv_box's LDS at h = 12: two table slices and the row stretches of a pass, and its bound on the static part
    h = 12
    dynamic = 2 * 16 * box_slice(h) + 4 * (2 * h + 4) * NW
    host_static = 16 * (NT + 1) + 8 * NT + 8 * NW * 2 * 2 * HCAP + 1536
    assert v["group_segment_fixed_size"] <= host_static, (name, v, host_static)
    assert LDS_PER_CU // (dynamic + host_static) >= 3, (dynamic, host_static)
    assert 3 * (dynamic + v["group_segment_fixed_size"]) <= LDS_PER_CU
