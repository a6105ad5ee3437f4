"""Development aid: time one unmasked LoG scale at n^3 for the half-widths the pair route (csrc/gauss_pair.hip) is
instantiated for, on that route (log_pair = 2) and on the one it replaces (log_pair = 0: two single sweeps up to H = 8, two
Gaussians of three launches each beyond), in alternating launches, with HIP events on the context's stream.  The table
kPairWins in csrc/gauss_pair.hip is filled from this; the record is profiles/log_pair_time.txt.

    python tools/log_pair_time.py [n] [h,h,...] [reps] > profiles/log_pair_time.txt"""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visfd_amd import api  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
hs = [int(h) for h in (sys.argv[2] if len(sys.argv) > 2 else "6,7,8,9,10").split(",")]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
delta = 0.02
ratio = api.ratio_from_threshold(0.03)
dev = torch.device("cuda:0")
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
ctx = api.Context(0, stream.cuda_stream)
src = torch.randn((n, n, n), device=dev)
dst = torch.empty_like(src)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
print("one LoG scale at %d^3, ms per call (the first call of each route is dropped); routes alternate call by call" % n)
for h in hs:
    sigma = ((h + 0.5) / (ratio * (1 + 0.5 * delta)),) * 3
    ts, sums = {0: [], 2: []}, {}
    for rep in range(reps + 1):
        for mode in (0, 2):
            ctx.set_option("log_pair", mode)
            e0.record()
            ctx.log_dev(src, dst, sigma, delta, ratio)
            e1.record()
            torch.cuda.synchronize()
            if rep:
                ts[mode].append(e0.elapsed_time(e1))
            sums[mode] = float(dst.double().sum())
    med = {m: sorted(v)[len(v) // 2] for m, v in ts.items()}
    spread = max(max(v) - min(v) for v in ts.values())
    assert sums[0] == sums[2] or (math.isnan(sums[0]) and math.isnan(sums[2])), sums
    for mode, name in ((0, "current"), (2, "pair   ")):
        print("h=%2d %s: %s" % (h, name, " ".join("%.3f" % t for t in ts[mode])))
    print("h=%2d medians %.3f -> %.3f ms (%+.3f), largest min-to-max spread %.3f ms, checksum %.9g" % (
        h, med[0], med[2], med[2] - med[0], spread, sums[2]))
ctx.set_option("log_pair", 1)
ctx.close()
