"""Times the image statistics and the intensity maps on a 1024^3 volume (csrc/intensity.hip) and writes
profiles/intensity_time.txt:

    python tools/intensity_time.py [--n 1024] [--out profiles/intensity_time.txt]

Per line: the pass, its time (median of 5 after one warm-up, HIP events on the context's stream), the bytes it must
move, and the time of a device-to-device copy that moves the same bytes (torch, same stream discipline).  Then the
host loops of -cl (float sums in scan order) on the same volume, from a numpy restatement of their arithmetic, as an
order of magnitude for what the command-line program spends there."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intensity_time.txt"))
    a = ap.parse_args()
    import torch
    from visfd_amd import api
    n = a.n
    ctx = api.Context(0)
    g = torch.Generator(device="cuda").manual_seed(1)
    src = (torch.randint(-2000, 2001, (n, n, n), generator=g, device="cuda", dtype=torch.int32).float() / 8.0).contiguous()
    out = src.clone()
    mask = (torch.rand((n, n, n), generator=g, device="cuda") < 0.7).float()
    torch.cuda.synchronize()
    vox = n ** 3

    def timed(fn, reps=5):
        fn()
        ctx.synchronize()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    def copy_ms(nbytes):
        x = torch.empty(nbytes // 8, dtype=torch.float32, device="cuda")   # a copy reads and writes: half the bytes each way
        y = torch.empty_like(x)
        return timed(lambda: y.copy_(x))

    rows = []

    def row(name, ms, nbytes):
        rows.append("%-46s %9.3f ms  %6.1f GB moved  %8.1f GB/s   copy of the same bytes %9.3f ms" % (
            name, ms, nbytes / 1e9, nbytes / ms / 1e6, copy_ms(nbytes)))

    row("image_stats, no mask", timed(lambda: ctx.image_stats(src)), 4 * vox)
    row("image_stats, mask", timed(lambda: ctx.image_stats(src, mask)), 8 * vox)
    p2 = api.intensity(api.MAP_THRESH2, (-100.0, 150.25))
    row("-thresh2 (reads in, writes out)", timed(lambda: ctx.intensity_map(p2, out, src)), 8 * vox)
    row("-thresh2 in place", timed(lambda: ctx.intensity_map(p2, out, out)), 8 * vox)

    def full_tail():
        st = ctx.image_stats(out, mask)
        p = api.intensity(api.MAP_RESCALE, (0.5, 1.0), invert_ave=st["sum"] / st["count"], masked_value=0.0, stats_mask=True)
        s2 = ctx.intensity_map(p, out, None, mask, want_stats=True)
        ctx.intensity_map(api.intensity(rescale01=(s2["min"], s2["max"], 0.0, 1.0)), out)

    row("-invert -rescale -mask -rescale-min-max (3 passes)", timed(full_tail), (8 + 12 + 8) * vox)
    # the host loops of -cl: two float sums in scan order per statistic
    h = src.cpu().numpy().reshape(-1)
    t0 = time.perf_counter()
    ave = np.add.accumulate(h, dtype=np.float32)[-1] / np.float32(h.size)
    d = h - ave
    np.multiply(d, d, out=d)
    sd = np.sqrt(np.add.accumulate(d, dtype=np.float32)[-1] / np.float32(h.size))
    cl_s = time.perf_counter() - t0
    rows.append("-cl host sums in scan order (numpy restatement)  %9.3f s  (ave %g, stddev %g)" % (cl_s, ave, sd))
    text = "intensity maps and statistics, %d^3 float32 (%s)\n" % (n, torch.cuda.get_device_name(0)) + "\n".join(rows) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
