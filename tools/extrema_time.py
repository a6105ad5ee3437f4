"""Development aid: time the plateau-aware extrema search (csrc/extrema.hip) on device volumes, next to a device copy
of the same volume and to the reference program on a 256^3 crop.

    python tools/extrema_time.py [sizes, default 512,1024] [reps, default 3]

Inputs per size n: (a) blurred Gaussian noise n^3 and (b) its 8-level quantisation; connectivity 3, minima and maxima,
three requests: counts only (capacities 0: every kernel up to the first list pass and one read of the two counts, nothing
sorted or copied), the lists, and the lists with the label image.  visfd_hip_find_extrema_dev is called directly, with
list arrays allocated once before the timing, so the figures are the library's.  Each line: the median and range of `reps`
calls after one warm-up call -- wall-clock time of the whole call, which returns with the stream idle and, for the lists,
includes their copy to the host and the host's sorting -- the list lengths, and the ratio of the median to the device
copy's.  The last lines: the seconds the reference program (oracle/_ref/filter_mrc_ref, when it has been built) takes for
the same request on the 256^3 corner of each input."""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from visfd_amd import api  # noqa: E402

sizes = [int(s) for s in sys.argv[1].split(",")] if len(sys.argv) > 1 else [512, 1024]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
dev = torch.device("cuda:0")
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
ctx = api.Context(0, stream.cuda_stream)
REF_CLI = os.path.join(ROOT, "oracle", "_ref", "filter_mrc_ref")


def timed(fn):
    ts = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    ts = sorted(ts[1:])
    return ts[len(ts) // 2], ts[0], ts[-1]


def inputs(n):
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    v = torch.randn((1, 1, n, n, n), device=dev, generator=gen)
    for _ in range(2):
        v = F.avg_pool3d(F.pad(v, (1, 1, 1, 1, 1, 1), mode="replicate"), 3, 1)
    v = v[0, 0].contiguous()
    lo, hi = float(v.min()), float(v.max())
    q = torch.clamp(torch.floor((v - lo) / (hi - lo) * 7.999999), 0, 7).contiguous()
    return v, q


crops = {}
for n in sizes:
    smooth, quant = inputs(n)
    dst = torch.empty_like(smooth)
    copy_ms, _, _ = timed(lambda: dst.copy_(smooth))
    del dst
    print("n=%d  device copy %.3f ms" % (n, copy_ms), flush=True)
    labels = torch.zeros((n, n, n), dtype=torch.int32, device=dev)
    L = api.load_library()
    for name, vol in (("blurred noise", smooth), ("8 levels", quant)):
        cnt = [C.c_int64(), C.c_int64()]

        def call(lists, caps, lab):
            tail = []
            for k in range(2):
                tail += [a.ctypes.data if a is not None else None for a in lists[k]] + [caps[k], C.byref(cnt[k])]
            rc = L.visfd_hip_find_extrema_dev(ctx._h, vol.data_ptr(), None, n, n, n, 1, 1, float("inf"), -float("inf"), 3, 1,
                                              *(tail + [lab]))
            assert rc == 0, L.visfd_hip_last_error()

        none = [(None, None, None)] * 2
        call(none, (0, 0), None)
        caps = (max(cnt[0].value, 1), max(cnt[1].value, 1))
        lists = [(np.empty(c, np.int64), np.empty(c, np.float32), np.empty(c, np.int64)) for c in caps]
        for what, fn in (("counts only", lambda: call(none, (0, 0), None)), ("lists", lambda: call(lists, caps, None)),
                         ("lists + labels", lambda: call(lists, caps, labels.data_ptr()))):
            med, lo, hi = timed(fn)
            print("n=%-5d %-14s %-15s %10.3f ms (%.3f..%.3f)  x%.1f copy   minima %d maxima %d" % (
                n, name, what, med, lo, hi, med / copy_ms, cnt[0].value, cnt[1].value), flush=True)
        crops.setdefault(name, vol[:256, :256, :256].contiguous().cpu().numpy())
    del smooth, quant, labels
ctx.close()

if os.path.exists(REF_CLI):
    import volgen
    with tempfile.TemporaryDirectory() as d:
        for name, vol in crops.items():
            volgen.write_mrc(os.path.join(d, "in.rec"), vol, voxel_width=1.0)
            t0 = time.perf_counter()
            r = subprocess.run([REF_CLI, "-in", "in.rec", "-w", "1", "-find-minima", "min.txt", "-find-maxima", "max.txt", "-out",
                                "out.rec"], cwd=d, capture_output=True, text=True)
            print("reference program, %s, %s crop: %.2f s (exit %d)" % (name, "x".join(map(str, vol.shape)),
                                                                         time.perf_counter() - t0, r.returncode), flush=True)
else:
    print("reference program not built: no comparison")
