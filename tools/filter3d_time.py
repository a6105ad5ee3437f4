"""Development aid: time the general 3-D filter (csrc/filter3d.hip) at n^3 with HIP events on the context's stream, next
to a device copy of the same volume.

    python tools/filter3d_time.py [n] [reps]

Cases: spherical generalised-Gaussian windows (exponent 3, width h / 2) of half-width h = 2, 5 and 12, normalised, without
and with a mask of zeros and ones, each on the library's own choice of kernel and with the option filter3d_general; then LocalFluctuations with exponent 2 (separable Gaussians) against exponent 6 (two
dense passes) at the same radius.  Each line: the case, the table's non-zero entries, the median and range of `reps` timed
calls (after one warm-up call), non-zero taps per second, and the fraction of the arithmetic floor reached: one multiply
and one add per non-zero tap and voxel (two of each with a mask: the weight times the mask, the denominator) on
64 FP32 lanes per CU and clock at the nominal 2400 MHz.

What a timed call holds besides the kernels: for the h rows, the comparison of the table with the one already on the
device (a memcmp; the table is built before the timed region and sent during the warm-up call); for the two fluctuation
rows, the whole entry point, which builds its table on the host on every call (one exp and one pow per entry) before it
queues its kernels -- the tool prints that share separately as "host table"."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visfd_amd import api  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
dev = torch.device("cuda:0")
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
ctx = api.Context(0, stream.cuda_stream)
gen = torch.Generator(device=dev)
gen.manual_seed(1)
src = torch.randn((n, n, n), device=dev, generator=gen)
mask = (torch.rand((n, n, n), device=dev, generator=gen) > 0.2).float()
dst = torch.empty_like(src)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
props = torch.cuda.get_device_properties(0)
CLOCK_MHZ = 2400.0   # the peak engine clock of the MI355X: the floor is nominal, not what the run clocked at
lanes_per_s = props.multi_processor_count * 64 * CLOCK_MHZ * 1e6


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
print("n=%d  %s  %d CUs, floor at %.0f MHz  device copy %.3f ms" % (n, props.name, props.multi_processor_count,
                                                                   CLOCK_MHZ, copy_ms), flush=True)
KERNEL = {api.FILTER3D_PATH_GENERAL: "general", api.FILTER3D_PATH_TILED: "tiled"}
for h in (2, 5, 12):
    table, _ = api.gengauss3d_table((h / 2.0,) * 3, 3.0, (h, h, h))
    nnz = int((table != 0).sum())
    for m in (None, mask):
        for general in (0, 1):
            with ctx.options(filter3d_general=general):
                med, lo, hi = timed(lambda: ctx.filter3d_dev(src, dst, table, m, True))
                kernel = KERNEL[ctx.filter3d_last_path()]
            floor_ms = nnz * n ** 3 * (2 if m is None else 4) / lanes_per_s * 1e3
            print("h=%-2d entries=%-5d of %-5d %-8s %-7s %9.3f ms (%.3f..%.3f) %7.1f Gtap/s %5.1f%% of the floor  x%.0f copy" % (
                h, nnz, table.size, "unmasked" if m is None else "masked", kernel, med, lo, hi, nnz * n ** 3 / med / 1e6,
                100 * floor_ms / med, med / copy_ms), flush=True)
radius = (6.0, 6.0, 6.0)
for exponent in (2.0, 6.0):
    sg, r = api.fluctuation_sigmas(radius, exponent, -1.0, 0.03)
    hw = api.gengauss3d_halfwidths(sg, exponent, r)
    med, lo, hi = timed(lambda: ctx.local_fluctuations_gen_dev(src, dst, sg, r, None, True, exponent))
    t0 = time.perf_counter()
    api.gengauss3d_table(sg, exponent, hw)
    host_ms = (time.perf_counter() - t0) * 1e3
    print("fluct radius=6 exponent=%g window=%s %-30s %10.3f ms (%.3f..%.3f)  host table %.3f ms of it" % (
        exponent, hw, "separable Gaussians" if exponent == 2.0 else "dense generalised Gaussian", med, lo, hi,
        0.0 if exponent == 2.0 else host_ms), flush=True)
ctx.close()
