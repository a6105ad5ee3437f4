"""Times DiscardOverlappingBlobs (csrc/discard_overlap.hip against csrc/blob_post.cpp) and writes
profiles/discard_overlap_time.txt:

    python tools/discard_overlap_time.py [--out profiles/discard_overlap_time.txt] [--quick]

Lists: random integer centres in a cubic volume, diameters uniform in a range, normal scores; min_radial_separation_ratio 1,
both volume limits off, scale 6, SORT_DECREASING_MAGNITUDE.  Per shape (blobs, volume, diameters):
  host     visfd_hip_discard_overlapping_blobs, the sequential walk: one run
  staged   visfd_hip_discard_overlapping_blobs_ctx on host arrays: copies up, the device work, the kept list down; median of
           3 after one warm-up, a host clock around the call
  device   visfd_hip_discard_overlapping_blobs_dev on device arrays (fresh copies of the list each run, made outside the
           clock); median of 3 after one warm-up
  phases   option discard_overlap_time, stream events inside one more _dev call: the reduction with its wait | ranking and
           records | buckets | the rounds with their waits | compaction
The kept lists of the three are compared bit for bit.

The second table decides filter_mrc's DISCARD_OVERLAP_MIN_BLOBS: for a growing list of the first shape's density, the host
walk against ONE staged call in a fresh process, context creation included (what a command-line run pays)."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(10 ** 5, 512, 8.0, 24.0), (10 ** 6, 1024, 8.0, 24.0), (10 ** 6, 1024, 3.0, 3.0), (4 * 10 ** 6, 1024, 3.0, 8.0)]
QUICK = [(2000, 64, 8.0, 24.0), (20000, 128, 3.0, 3.0)]

CHILD = r"""
import sys, time
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tools")
from visfd_amd import api
from discard_overlap_time import blobs
api.load_library()
n = int(sys.argv[2])
c, d, s = blobs(n, max(16, int(round(512 * (n / 1e5) ** (1 / 3.0)))), 8.0, 24.0)
t0 = time.perf_counter()
ctx = api.Context(0)
t1 = time.perf_counter()
got = ctx.discard_overlapping_blobs(c, d, s, 1.0)
t2 = time.perf_counter()
ctx.close()
t3 = time.perf_counter()
want = api.discard_overlapping_blobs(c, d, s, 1.0)
t4 = time.perf_counter()
assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, want))
print("%.3f %.3f %.3f %.3f %d" % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3, len(want[1])))
"""


def blobs(n, box, d_lo, d_hi, seed=1):
    rng = np.random.default_rng(seed)
    c = np.floor(rng.uniform(0, box, (n, 3))).astype(np.float32)
    d = rng.uniform(d_lo, d_hi, n).astype(np.float32) if d_hi > d_lo else np.full(n, d_lo, np.float32)
    return c, d, rng.normal(0, 50, n).astype(np.float32)


def same(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "discard_overlap_time.txt"))
    ap.add_argument("--quick", action="store_true", help="small lists: a rehearsal of the tool itself")
    a = ap.parse_args()
    import torch
    from visfd_amd import api
    ctx = api.Context(0)
    dev = torch.device("cuda", 0)
    rows = ["%9s %7s %9s | %10s | %10s %10s | %8s %6s | %s" % ("blobs", "volume", "diameters", "host ms", "staged ms", "device ms",
                                                              "kept", "rounds", "phases ms: reduce rank buckets rounds compact")]
    for n, box, d_lo, d_hi in (QUICK if a.quick else SHAPES):
        c, d, s = blobs(n, box, d_lo, d_hi)
        t0 = time.perf_counter()
        want = api.discard_overlapping_blobs(c, d, s, 1.0)
        host_ms = (time.perf_counter() - t0) * 1e3

        def staged():
            t0 = time.perf_counter()
            got = ctx.discard_overlapping_blobs(c, d, s, 1.0)
            return (time.perf_counter() - t0) * 1e3, got

        def device():
            tc, td, ts = (torch.from_numpy(x).to(dev) for x in (c, d, s))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            k = ctx.discard_overlapping_blobs_dev(tc, td, ts, 1.0)
            ms = (time.perf_counter() - t0) * 1e3
            return ms, (tc[:k].cpu().numpy(), td[:k].cpu().numpy(), ts[:k].cpu().numpy())

        times = {}
        for name, fn in (("staged", staged), ("device", device)):
            fn()
            runs = [fn() for _ in range(3)]
            assert all(same(got, want) for _, got in runs), name + " and host disagree"
            times[name] = float(np.median([ms for ms, _ in runs]))
        last = ctx.discard_overlapping_blobs_last()
        assert last["path"] == api.DISCARD_OVERLAP_PATH_DEVICE, last
        with ctx.options(discard_overlap_time=1):
            device()
            ph = ctx.discard_overlapping_blobs_last_times()
        rows.append("%9d %6d^3 %4g-%-4g | %10.1f | %10.2f %10.2f | %8d %6d | %s" % (
            n, box, d_lo, d_hi, host_ms, times["staged"], times["device"], len(want[1]), last["rounds"],
            " ".join("%.2f" % ph[k] for k in ("reduce", "rank", "buckets", "rounds", "compact"))))
        print(rows[-1], flush=True)
    ctx.close()
    cross = ["%9s | %10s %10s %10s %12s | %10s | %8s" % ("blobs", "context ms", "call ms", "close ms", "device sum", "host ms", "kept")]
    for n in ([2 ** 10, 2 ** 12] if a.quick else [2 ** k for k in range(10, 19)]):
        out = subprocess.check_output([sys.executable, "-c", CHILD, ROOT, str(n)], text=True).split()
        t_ctx, t_call, t_close, t_host = (float(x) for x in out[:4])
        cross.append("%9d | %10.1f %10.1f %10.1f %12.1f | %10.1f | %8d" % (n, t_ctx, t_call, t_close, t_ctx + t_call + t_close,
                                                                         t_host, int(out[4])))
        print(cross[-1], flush=True)
    text = ("DiscardOverlappingBlobs, %s; ratio 1, scale 6, random integer centres%s\n" % (
        torch.cuda.get_device_name(0), " (--quick: a rehearsal, not a measurement)" if a.quick else "") +
        "\n".join(rows) + "\n\n" +
        "one staged call in a fresh process (diameters 8-24, the density of the first shape), against the host walk of the same list:\n" +
        "\n".join(cross) + "\n")
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
