"""Times the exact distance maps on a 1024^3 volume (csrc/distance.hip) and writes profiles/distance_time.txt:

    python tools/distance_time.py [--n 1024] [--out profiles/distance_time.txt]

Per line: the call, its time (median of 5 after one warm-up, wall clock around the call and a wait for the context's
stream; the upload of the point list is inside), the algorithmic bytes, the rate they give, and the time of a
device-to-device copy that moves the same bytes, measured in the same run.

Algorithmic bytes: what a three-pass separable transform over an int32 volume has to move, per voxel --
    row pass       4 written, plus 4 read per input array it looks at (the image; the seed flags when points lie inside)
    y and z pass   4 read + 4 written each
    float root     4 read + 4 written (distance_to_points only)
-- so 28 B/voxel for distance_to_points (32 with points inside the image) and 24 B/voxel for distance_from_points
with an image and no mask.  The kernels move more than that: the row pass sweeps its line twice (one more write and
read), the seed flags are filled before they are read, and the envelope passes push to and pop from stacks in workspace.
The yardstick is the copy; the file states the ratio."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distance_time.txt"))
    a = ap.parse_args()
    import torch
    from visfd_amd import api
    n = a.n
    ctx = api.Context(0)
    g = torch.Generator(device="cuda").manual_seed(1)
    src = (torch.rand((n, n, n), generator=g, device="cuda") < 0.3).float().contiguous()   # a 30 % selection
    dst = torch.zeros((n, n, n), device="cuda")
    torch.cuda.synchronize()
    vox = n ** 3
    rng = np.random.default_rng(2)

    def inside(k):
        return rng.integers(0, n, (k, 3)).astype(np.int32)

    outside8 = np.array([[-3, 40, 2], [n, 5, 5], [n // 2, -2, n + 3], [-1, -1, -1], [n + 7, n + 7, n + 7], [5, n, 9],
                         [-20, n // 3, n // 2], [n // 4, n // 4, -9]], np.int32)

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

    rows, ratios, times = [], {}, {}

    def row(name, ms, nbytes):
        c = copy_ms(nbytes)
        ratios[name] = ms / c
        times[name] = ms
        rows.append("%-52s %9.3f ms  %6.1f GB algorithmic  %8.1f GB/s   copy of the same bytes %9.3f ms   (%.1f x the copy)" % (
            name, ms, nbytes / 1e9, nbytes / ms / 1e6, c, ms / c))

    for k, label in ((1, "1 point"), (1000, "10^3 points"), (1000000, "10^6 points inside")):
        pts = inside(k)
        row("distance_to_points, %s" % label, timed(lambda: ctx.distance_to_points(dst, pts, 2.5)), 32 * vox)
    row("distance_to_points, 8 points outside the image", timed(lambda: ctx.distance_to_points(dst, outside8, 2.5)), 28 * vox)
    q = inside(1000)
    row("distance_from_points, 30 % selected, 10^3 points", timed(lambda: ctx.distance_from_points(src, q, 0.5, 1.5, 2.5)), 24 * vox)
    q8 = np.concatenate([q, outside8])
    row("  ... and 8 more points outside the image", timed(lambda: ctx.distance_from_points(src, q8, 0.5, 1.5, 2.5)), 28 * vox)
    one, million = times["distance_to_points, 1 point"], times["distance_to_points, 10^6 points inside"]
    note = ("1 point -> 10^6 points inside the image: %.2f x the time (the list's upload and scatter; the passes are the same)"
            % (million / one))
    ws = "workspace held after these calls: %.2f GB" % (ctx.workspace_bytes() / 1e9)
    formula = ("algorithmic bytes per voxel: row pass 4 written + 4 read per input array (image; seed flags when points lie\n"
               "inside), y and z pass 4 read + 4 written each, float root 4 read + 4 written: 32 (28 without points inside)\n"
               "for distance_to_points, 24 for distance_from_points with an image and no mask (+ 4 for the reduction over the\n"
               "selected voxels that points outside the image cost)\n")
    text = ("exact distance maps, %d^3 float32 (%s)\n" % (n, torch.cuda.get_device_name(0)) + formula + "\n".join(rows) + "\n" +
            note + "\n" + ws + "\n")
    print(text)
    with open(a.out, "w") as f:
        f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
