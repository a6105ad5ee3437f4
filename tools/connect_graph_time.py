#!/usr/bin/env python3
"""Wall time of LabelConnected as a graph problem (visfd_hip_label_connected_graph[_dev|_host]) against the flood, on the
volumes and by the protocol of tools/connect_time.py: two wavy sheets, best of `--repeat` runs, wall time of the whole
call from numpy arrays (the _dev face: from resident device tensors), results compared in every run by the contract of
the graph entries (the flood's labels and labelled directions, the input's directions elsewhere).

    python tools/connect_graph_time.py [--sizes 256 512] [--repeat 2] [--out profiles/connect_graph_time.txt]

Per size and volume: the host flood (api.label_connected), the device-seeded flood (visfd_hip_label_connected_device_seeds),
the serial host walk, the host-array face and the device-array face of the graph entry, the path each graph call took,
and the stages of one more call of each face under the option connect_time (which waits for the stream at every stage).

Two volumes.  "protocol" is tools/connect_time.py's as it stands: its second sheet is a corrugated plane whose normals
are all the z axis, so its outward sum is zero up to rounding and the call carries the OUTWARD reason -- it measures the
hand-over to the flood.  "fanned" has the same saliency and the plane's normals fanned out from a point two image
heights below it, so every outward sum is decisive and the call stays on the device."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from connect_time import sheets   # noqa: E402
from visfd_amd import api   # noqa: E402

STAGES = ("seed search", "classify+compact", "host vector test", "edges+union-find", "clusters", "directions+last pass",
          "copies in", "copies out")
PATHS = {0: "device", 1: "host graph", 2: "flood"}


def fanned(n, sal, direction, seed=3):
    """the plane's normals (exactly the z axis, up to sign, in sheets()) replaced by unit vectors away from (c, c, -1.1 n)"""
    d = direction.copy()
    plane = (np.abs(d[..., 2]) == 1.0) & (d[..., 0] == 0.0) & (d[..., 1] == 0.0)
    ax = np.arange(n, dtype=np.float32)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij", sparse=True)
    c = np.float32(n / 2)
    v = np.stack(np.broadcast_arrays(x - c, y - c, z + np.float32(1.1 * n)), -1).astype(np.float32)
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    d[plane] = v[plane] * d[..., 2][plane][:, None]      # keep each voxel's arbitrary sign
    return d


def contract_ok(want, d_flood, d_in, got_labels, got_k, d_got):
    if got_k != want[1] or not np.array_equal(got_labels, want[0]):
        return False
    labelled = want[0] != -1
    expect = np.where(labelled[..., None], d_flood.view(np.uint32), d_in.view(np.uint32))
    return np.array_equal(d_got.view(np.uint32), expect)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256])
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = api.Context(0)
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)
    for n in a.sizes:
        sal, direction = sheets(n)
        thr = 0.6
        kw = dict(threshold_saliency=thr, threshold_vector_saliency=-2.0, threshold_vector_neighbor=0.5,
                  consider_dot_product_sign=False, standardize_directions=True, connectivity=1)
        for volume, d_in in (("protocol", direction), ("fanned", fanned(n, sal, direction))):
            names = ("flood", "seeded", "walk", "graph", "graph_dev")
            runs = {k: [] for k in names}
            paths = {}
            dsal = torch.from_numpy(sal).cuda()
            dlab = torch.empty(sal.shape, dtype=torch.int64, device="cuda")
            for _ in range(a.repeat):
                d0 = d_in.copy()
                t = time.perf_counter()
                want = api.label_connected(sal, direction=d0, **kw)
                runs["flood"].append(time.perf_counter() - t)
                d1 = d_in.copy()
                t = time.perf_counter()
                got = api.label_connected(sal, direction=d1, seeds_ctx=ctx, **kw)
                runs["seeded"].append(time.perf_counter() - t)
                assert got[1] == want[1] and np.array_equal(got[0], want[0]) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32))
                d2 = d_in.copy()
                t = time.perf_counter()
                got = api.label_connected_graph(sal, direction=d2, **kw)
                runs["walk"].append(time.perf_counter() - t)
                paths["walk"] = api.label_connected_graph_last()
                assert contract_ok(want, d0, d_in, got[0], got[1], d2), "host walk"
                d3 = d_in.copy()
                t = time.perf_counter()
                got = ctx.label_connected_graph(sal, direction=d3, **kw)
                runs["graph"].append(time.perf_counter() - t)
                paths["graph"] = ctx.label_connected_graph_last()
                assert contract_ok(want, d0, d_in, got[0], got[1], d3), "host-array face"
                dd = torch.from_numpy(d_in).cuda()
                torch.cuda.synchronize()
                t = time.perf_counter()
                k, _, _, _ = ctx.label_connected_graph_dev(dsal, dlab, direction=dd, **kw)      # returns with the stream idle
                runs["graph_dev"].append(time.perf_counter() - t)
                paths["graph_dev"] = ctx.label_connected_graph_last()
                assert contract_ok(want, d0, d_in, dlab.cpu().numpy(), k, dd.cpu().numpy()), "device-array face"
            say("%d^3 %s: %.1f%% of the voxels pass, %d clusters, %d valid voxels, %d candidates of the vector test" % (
                n, volume, 100 * float((sal >= thr).mean()), want[1], paths["graph"][2], paths["graph"][3]))
            for k_, label in zip(names, ("host flood", "device-seeded flood (parent's call)", "host walk (no device)",
                                         "graph entry, host arrays", "graph entry, device arrays resident")):
                p = paths.get(k_)
                say("    %-38s best %.3f s   runs %s%s" % (label, min(runs[k_]), " ".join("%.3f" % v for v in runs[k_]),
                                                          "" if p is None else "   path: %s, reasons %d" % (PATHS[p[0]], p[1])))
            ctx.set_option("connect_time", 1)
            d4 = d_in.copy()
            ctx.label_connected_graph(sal, direction=d4, **kw)
            say("    stages, host arrays (ms):   " + ", ".join("%s %.1f" % s for s in zip(STAGES, ctx.label_connected_graph_last_times())))
            dd = torch.from_numpy(d_in).cuda()
            ctx.label_connected_graph_dev(dsal, dlab, direction=dd, **kw)
            say("    stages, device arrays (ms): " + ", ".join("%s %.1f" % s for s in zip(STAGES, ctx.label_connected_graph_last_times())))
            ctx.set_option("connect_time", 0)
            del dd, dsal, dlab
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
