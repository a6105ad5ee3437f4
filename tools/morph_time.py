"""Development aid: time grayscale morphology (csrc/morph.hip) at n^3 with HIP events on the context's stream, next to a
device copy of the same volume.

    python tools/morph_time.py [n] [reps]

Cases: flat balls R = 2, 5, 10 (dilate, erode, open) and the soft element R = 5, rmax = 7, bmax = 50 (dilate, erode).
Flat cases run twice: on the library's own choice and with the option morph_general (the general element walk).
Each line: the case, the element's entry count, the kernel that ran (as the library reports it), the median and range of `reps` timed calls (after
one warm-up call) and the ratio of the median to the device copy's."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visfd_amd import api  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
dev = torch.device("cuda:0")
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
ctx = api.Context(0, stream.cuda_stream)
gen = torch.Generator(device=dev)
gen.manual_seed(1)
src = torch.randn((n, n, n), device=dev, generator=gen)
dst = torch.empty_like(src)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(fn):
    ts = []
    for _ in range(reps + 1):
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts = sorted(ts[1:])
    return ts[len(ts) // 2], ts[0], ts[-1]


copy_ms, _, _ = timed(lambda: dst.copy_(src))
print("n=%d  device copy %.3f ms" % (n, copy_ms))
names = {api.MORPH_DILATE: "dilate", api.MORPH_ERODE: "erode", api.MORPH_OPEN: "open"}
cases = [(r, 0.0, 0.0, op) for r in (2, 5, 10) for op in (api.MORPH_DILATE, api.MORPH_ERODE, api.MORPH_OPEN)]
cases += [(5, 7, 50, op) for op in (api.MORPH_DILATE, api.MORPH_ERODE)]
for r, rmax, bmax, op in cases:
    d, b = api.sphere_structure(r, rmax, bmax)
    for general in ((0, 1) if not b.view("u4").any() else (0,)):
        with ctx.options(morph_general=general):
            med, lo, hi = timed(lambda: ctx.morph_sphere_dev(op, src, dst, r, rmax, bmax))
            kernel = {api.MORPH_PATH_GENERAL: "morph_kernel", api.MORPH_PATH_XRUNS: "morph_runs_kernel"}[ctx.morph_last_path()]
        print("%-6s R=%-2g rmax=%-2g bmax=%-2g entries=%-5d %-18s %9.3f ms (%.3f..%.3f)  x%.1f copy" % (
            names[op], r, rmax, bmax, len(b), kernel, med, lo, hi, med / copy_ms))
ctx.close()
