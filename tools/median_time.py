"""Development aid: time the median filter (csrc/median.hip) at n^3 with HIP events on the context's stream, next to a
device copy of the same volume.

    python tools/median_time.py [n] [reps] [--general-max-entries N]

Cases: balls of radius 1, 2, 3 and 5 voxels on signed noise, without a mask and with one that keeps 75 % of the voxels, on
the library's own choice (the LDS-tiled kernel) and with the option median_general (the walk in global memory); the
tiled kernel also on the same noise shifted to be all positive, where the keys of a neighbourhood share their leading bits
and the selection skips them, and on a constant volume, where no bit is left to decide (the cost of everything but the
selection rounds).  --general-max-entries leaves out general-walk cases whose footprint has more entries
than N (that walk reads every neighbour from global memory once per decided bit).
Each line: the case, the footprint's entry count, the kernel that ran (as the library reports it), the median and range of
`reps` timed calls (after one warm-up call) and the ratio of the median to the device copy's.
There is no reference time to set beside these: the reference's median loop does not terminate for any footprint beyond
the centre voxel."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visfd_amd import api  # noqa: E402

argv = sys.argv[1:]
general_max = 1 << 30
if "--general-max-entries" in argv:
    k = argv.index("--general-max-entries")
    general_max = int(argv[k + 1])
    del argv[k:k + 2]
n = int(argv[0]) if len(argv) > 0 else 1024
reps = int(argv[1]) if len(argv) > 1 else 3
dev = torch.device("cuda:0")
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
ctx = api.Context(0, stream.cuda_stream)
gen = torch.Generator(device=dev)
gen.manual_seed(1)
src = torch.randn((n, n, n), device=dev, generator=gen)
pos = src + 100.0
const = torch.full_like(src, 3.0)
mask = (torch.rand((n, n, n), device=dev, generator=gen) < 0.75).float()
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
print("n=%d  device copy %.3f ms" % (n, copy_ms), flush=True)
kernels = {api.MEDIAN_PATH_GENERAL: "median_general_kernel", api.MEDIAN_PATH_TILED: "median_tiled_kernel"}
for r in (1, 2, 3, 5):
    entries = len(api.median_footprint(r))
    for general in (0, 1):
        for data, vol in (("signed", src), ("positive", pos), ("constant", const)):
            for m in (None, mask):
                if general and (entries > general_max or data != "signed"):
                    continue
                with ctx.options(median_general=general):
                    med, lo, hi = timed(lambda: ctx.median_sphere_dev(vol, dst, r, mask=m))
                    kernel = kernels[ctx.median_last_path()]
                print("R=%-2g entries=%-4d %-8s mask=%-4s %-22s %10.3f ms (%.3f..%.3f)  x%.1f copy" % (
                    r, entries, data, "75%" if m is not None else "none", kernel, med, lo, hi, med / copy_ms), flush=True)
ctx.close()
