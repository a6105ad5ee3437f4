#!/usr/bin/env python3
"""Wall time of the surface points (`-normals-file`): the host entry visfd_hip_surface_points against the context entries
visfd_hip_surface_points_ctx (host arrays, upload included) and _dev (resident device tensors), on the volume of
tools/connect_time.py (two wavy sheets; saliency with a Gaussian profile, unit normals).

    python tools/surface_points_time.py [--sizes 256 512] [--repeat 3] [--out profiles/surface_points_time.txt]

The cluster is the set of voxels whose saliency passes a threshold, as one label: 0.6 (the protocol's threshold: sheets
some 2.5 voxels thick) and 0.1 (some 5 voxels thick: longer walks).  One warm-up call of each entry, then the median of
`--repeat` calls by the host clock around the whole call (each returns with the stream idle).  The points of every context
call are compared with the host entry's, bit for bit.  Then one more _dev call under the option surface_points_time for the
per-stage split (events on the stream for the kernels, the host clock for the host finish), the walk kernel's rate in
steps per second, and the select sweep's time against the time its algorithmic bytes (label and mask read once, one bit
per voxel written) would take at the device's HBM rate."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from connect_time import sheets   # noqa: E402
from visfd_amd import api   # noqa: E402

STAGES = ("select+compact", "walk", "ridge gather", "host finish+copies")
HBM_BYTES_PER_S = 8.0e12   # MI355X, nominal


def standardized(n, direction):
    """sheets() gives every voxel's normal a random sign, as an eigenvector has; -connect standardises them before the export.
    Here: every normal turned away from the image's centre.  (With random signs a walk that steps from a voxel into a
    neighbour of the opposite sign steps back again, for ever: the reference's loop, and the host entry's, do not end on such
    an input, and the device path only ends it by its cap.)"""
    ax = np.arange(n, dtype=np.float32) - np.float32(n / 2)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij", sparse=True)
    dot = direction[..., 0] * x + direction[..., 1] * y + direction[..., 2] * z
    return direction * np.where(dot < 0, np.float32(-1), np.float32(1))[..., None]


def timed(f, repeat):
    f()   # warm-up: workspace, code objects
    runs, out = [], None
    for _ in range(repeat):
        t = time.perf_counter()
        out = f()
        runs.append(time.perf_counter() - t)
    return statistics.median(runs), runs, out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256])
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = api.Context(0)
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)
    for n in a.sizes:
        sal, direction = sheets(n)
        direction = standardized(n, direction)
        planar = torch.from_numpy(np.ascontiguousarray(np.moveaxis(direction, 3, 0))).cuda()
        dsal = torch.from_numpy(sal).cuda()
        for thr in (0.6, 0.1):
            cluster = (sal >= np.float32(thr)).astype(np.float32)
            dcl = torch.from_numpy(cluster).cuda()
            kw = dict(select_cluster=1, curve_ds=0.2, find_ridge=True, max_distance_to_feature=1.3)
            # every timed call is ONE call of its entry at a capacity that fits (the program's host path calls twice)
            kw["capacity"] = len(api.surface_points_host(sal, direction, voxel2cluster=cluster, **kw)[0]) + 1
            th, rh, want = timed(lambda: api.surface_points_host(sal, direction, voxel2cluster=cluster, **kw), a.repeat)
            tc, rc, got = timed(lambda: ctx.surface_points(sal, direction, voxel2cluster=cluster, **kw), a.repeat)
            last = ctx.surface_points_last()
            assert last[0] == api.SURFACE_POINTS_PATH_DEVICE, last
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), "host-array face"
            td, rd, got = timed(lambda: ctx.surface_points_dev(dsal, planar, voxel2cluster=dcl, **kw), a.repeat)
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), "device-array face"
            say("%d^3, cluster = saliency >= %.1f: %d selected voxels, %d points, longest walk %d steps" % (
                n, thr, last[2], last[3], last[4]))
            fmt = lambda r: " ".join("%.3f" % v for v in r)
            say("    host entry (one call: count and fill at a capacity that fits)   median %.3f s   runs %s" % (th, fmt(rh)))
            say("    _ctx entry, host arrays, upload included                        median %.3f s   runs %s   (%.1fx)" % (
                tc, fmt(rc), th / tc))
            say("    _dev entry, device arrays resident                              median %.3f s   runs %s   (%.1fx)" % (
                td, fmt(rd), th / td))
            with ctx.options(surface_points_time=1):
                ctx.surface_points_dev(dsal, planar, voxel2cluster=dcl, **kw)
                ms = ctx.surface_points_last_times()
                steps = ctx.surface_points_last()[5]
            say("    _dev stages (ms): " + ", ".join("%s %.2f" % s for s in zip(STAGES, ms)))
            say("    walk kernel: %d steps in %.2f ms = %.3g steps/s" % (steps, ms[1], steps / (ms[1] * 1e-3)))
            sweep = (4.0 + 1.0 / 8.0) * sal.size + 8.0 * last[2]   # no mask here: the label read, a bit written, the list written
            say("    select+compact: %.0f MB algorithmic (label image, selection bits, index list) = %.3f ms at %.0f TB/s; the stage "
                "(sweep, scan, list from the bits) took %.2f ms = %.2f of that rate" % (
                    sweep / 1e6, sweep / HBM_BYTES_PER_S * 1e3, HBM_BYTES_PER_S / 1e12, ms[0],
                    sweep / HBM_BYTES_PER_S * 1e3 / ms[0]))
            del dcl
        del planar, dsal
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
