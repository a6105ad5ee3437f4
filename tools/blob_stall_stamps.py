"""Development aid: run the two blob-stage kernels that carry phase stamps (csrc/gauss_pair.hip: -DVH_PAIR_STAMPS,
csrc/blob.hip: -DVH_BLOB_STAMPS; libraries built by tools/build_variant.py and loaded through VISFD_HIP_LIB) once per
half-width at n^3.  The stamped library prints the shares of a wave's time to stderr after every launch; the record is
profiles/blob_stall_stamps.txt.

    python tools/build_variant.py pair_stamps gauss_pair.hip -DVH_PAIR_STAMPS
    VISFD_HIP_LIB=visfd_amd/_variants/pair_stamps.so python tools/blob_stall_stamps.py pair 1024 6,8,10
    python tools/build_variant.py scan_stamps blob.hip -DVH_BLOB_STAMPS
    VISFD_HIP_LIB=visfd_amd/_variants/scan_stamps.so python tools/blob_stall_stamps.py scan 1024 6,8,10"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visfd_amd import api  # noqa: E402

what = sys.argv[1]
n = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
hs = [int(h) for h in (sys.argv[3] if len(sys.argv) > 3 else "6,8,10").split(",")]
delta = 0.02
ratio = api.ratio_from_threshold(0.03)
dev = torch.device("cuda:0")
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
ctx = api.Context(0, stream.cuda_stream)
src = torch.randn((n, n, n), device=dev)
for h in hs:
    sigma = (h + 0.5) / (ratio * (1 + 0.5 * delta))
    sys.stderr.write("== %s, H = %d, %d^3\n" % (what, h, n))
    sys.stderr.flush()
    if what == "pair":
        dst = torch.empty_like(src)
        ctx.set_option("log_pair", 2)
        for _ in range(2):   # (the second call is the one to read: the first loads the code object)
            ctx.log_dev(src, dst, (sigma,) * 3, delta, ratio)
        torch.cuda.synchronize()
        del dst
    else:
        # three scales inside one half-width: one scan of the middle LoG volume
        sig = np.array([sigma * 0.995, sigma, sigma * 1.005], np.float32)
        for _ in range(2):
            mins, maxs = ctx.blob_dog_dev(src, sig, None, None, delta, ratio, cap=1 << 23)
        sys.stderr.write("   (%d minima, %d maxima)\n" % (len(mins), len(maxs)))
ctx.close()
