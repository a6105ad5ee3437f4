"""csrc/gauss_pair.hip cross-compiled for gfx950 (hipcc needs no GPU): both kernels of the pair route, at every half-width
they are instantiated for, must fit their registers -- the code object's metadata reports no scratch memory for any of
them.  (A spilled ring is what made the single sweep lose at H = 9 and 10, csrc/gauss.hip: fused_applies.)"""
import os
import re
import subprocess

from visfd_amd import build as B

HALFWIDTHS = (6, 7, 8, 9, 10)


def kernel_resources(asm):
    """{kernel name: {vgpr_count, private_segment_fixed_size, group_segment_fixed_size}} from the amdhsa metadata notes of
    a device assembly listing."""
    out = {}
    for entry in re.split(r"\n  - \.", asm[asm.index("amdhsa.kernels:"):])[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry)
        if not name:
            continue
        out[name.group(1)] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, entry).group(1))
                              for k in ("vgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    return out


def compile_resources(tmp_path):
    s = str(tmp_path / "gauss_pair.s")
    cmd = [B.HIPCC] + B.FLAGS + B.PAIR_FLAGS + ["--cuda-device-only", "-S", "-x", "hip",
                                               os.path.join(B.CSRC, "gauss_pair.hip"), "-o", s]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return kernel_resources(open(s).read())


def test_pair_kernels_use_no_scratch(tmp_path):
    res = compile_resources(tmp_path)
    for kern in ("pair_z_kernel", "pair_yx_kernel"):
        for h in HALFWIDTHS:
            hits = [(n, v) for n, v in res.items() if re.search(r"%d%sILi%dE" % (len(kern), kern, h), n)]
            assert len(hits) == 1, (kern, h, sorted(res))
            name, v = hits[0]
            assert v["private_segment_fixed_size"] == 0, "%s uses %d bytes of scratch per lane" % (name, v["private_segment_fixed_size"])
            # the occupancy each kernel's launch bounds name: four waves per SIMD for the Z march, three for the Y/X kernel
            assert v["vgpr_count"] <= (128 if kern == "pair_z_kernel" else 168), (name, v)
            assert v["group_segment_fixed_size"] <= 64 * 1024, (name, v)
    assert all(v["group_segment_fixed_size"] == 0 for n, v in res.items() if "pair_z_kernel" in n)
