#!/usr/bin/env python3
"""Wall time of LabelConnected on synthetic curved sheets: everything on the host (api.label_connected) against the
device-seeded call (visfd_hip_label_connected_device_seeds: seeds searched on the device, flood on the host), and
the device's seed search alone.

    python tools/connect_time.py [--sizes 256 512] [--repeat 2] [--out profiles/connect_time.txt]

The volume holds two wavy sheets (a sphere-like shell and a corrugated plane) with a Gaussian profile plus a little
noise, so that a few per cent of the voxels pass the threshold and the saliency has many local maxima, as a voted
membrane has.  The call is the command line's: directions with standardisation, connectivity 1; no tensor (its tests
cost the same on both paths)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from visfd_amd import api   # noqa: E402


def sheets(n, seed=3):
    rng = np.random.default_rng(seed)
    ax = np.arange(n, dtype=np.float32)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij", sparse=True)
    c = np.float32(n / 2)
    r = np.sqrt((z - c) ** 2 + (y - c) ** 2 + (x - c) ** 2)
    d1 = r - np.float32(0.3 * n) - 2 * np.sin(x / 9) * np.cos(y / 7)
    d2 = (z - np.float32(0.9 * n)) - 3 * np.sin(x / 11 + y / 13)
    sal = np.exp(-0.5 * (d1 / 1.2) ** 2) + np.exp(-0.5 * (d2 / 1.2) ** 2)
    sal = (sal + 0.05 * rng.random(sal.shape, dtype=np.float32)).astype(np.float32)
    # directions: the shell's radial unit vector, the plane's z axis, with the arbitrary sign an eigenvector has
    direction = np.empty((n, n, n, 3), np.float32)
    rr = np.maximum(r, 1e-3)
    direction[..., 0] = (x - c) / rr
    direction[..., 1] = (y - c) / rr
    direction[..., 2] = (z - c) / rr
    plane = np.broadcast_to(np.abs(d2) < np.abs(d1), sal.shape)
    direction[plane] = (0.0, 0.0, 1.0)
    direction *= np.where(rng.random(sal.shape) < 0.5, np.float32(-1), np.float32(1))[..., None]
    return sal, direction


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256])
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = api.Context(0)
    lines = []
    for n in a.sizes:
        sal, direction = sheets(n)
        thr = 0.6
        share = float((sal >= thr).mean())
        kw = dict(threshold_saliency=thr, threshold_vector_saliency=-2.0, threshold_vector_neighbor=0.5,
                  consider_dot_product_sign=False, standardize_directions=True, connectivity=1)
        best = {"host": np.inf, "ctx": np.inf, "seeds": np.inf}
        for _ in range(a.repeat):
            d0 = direction.copy()
            t = time.perf_counter()
            want = api.label_connected(sal, direction=d0, **kw)
            best["host"] = min(best["host"], time.perf_counter() - t)
            d1 = direction.copy()
            t = time.perf_counter()
            got = api.label_connected(sal, direction=d1, seeds_ctx=ctx, **kw)
            best["ctx"] = min(best["ctx"], time.perf_counter() - t)
            where, seeds = ctx.label_connected_device_seeds_last()
            assert where == api.CONNECT_SEEDS_DEVICE
            assert got[1] == want[1] and np.array_equal(got[0], want[0]) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32))
            t = time.perf_counter()
            ctx.find_maxima_only(sal, threshold=thr, connectivity=1)
            best["seeds"] = min(best["seeds"], time.perf_counter() - t)
        lines.append("%d^3  %.1f%% of the voxels pass, %d seeds, %d clusters:  host %.3f s   device-seeded %.3f s  (%.2fx)   "
                     "device seed search alone, staging included %.3f s" % (
                         n, 100 * share, seeds, want[1], best["host"], best["ctx"], best["host"] / best["ctx"], best["seeds"]))
        print(lines[-1], flush=True)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
