#!/usr/bin/env python3
"""Wall time of the graph entry of LabelConnected with the option connect_settle, on the volumes and by the
protocol of tools/connect_time.py and tools/connect_graph_time.py: best of `--repeat` runs, wall time of the whole call from
numpy arrays, every timed result compared with the other side's by the contract of the graph entries.

    python tools/connect_settle_time.py --part protocol|links|weights|sheet [--size 512] [--repeat 2] [--out FILE]

  protocol   filter_mrc's call on both volumes ("protocol": the corrugated sheet whose outward sum is zero up to rounding;
             "fanned": every sum decisive): the device-seeded flood, which is what cluster() called before, against the
             graph entry with the option on; the spread between the repeated runs of each
  links      option on against option off: one must-link group of 2 locations, and 8 groups of 8 (fanned volume)
  weights    option on against option off under random voxel weights (fanned volume)
  sheet      option on against option off on the corrugated sheet (protocol volume)

Each part is one process, so that a caller can give each its own time limit; --out appends."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from connect_graph_time import PATHS, contract_ok, fanned   # noqa: E402
from connect_time import sheets   # noqa: E402
from visfd_amd import api   # noqa: E402

KW = dict(threshold_saliency=0.6, threshold_vector_saliency=-2.0, threshold_vector_neighbor=0.5,
          consider_dot_product_sign=False, standardize_directions=True, connectivity=1)
BITS = {8: "must-link", 16: "weights", 32: "outward"}


def bits(b):
    return "+".join(name for bit, name in BITS.items() if b & bit) or "none"


def timed(call, d_in):
    d = d_in.copy()
    t = time.perf_counter()
    got = call(d)
    return time.perf_counter() - t, got, d


def line(label, runs, extra=""):
    return "    %-44s best %.3f s   runs %s   spread %.3f s%s" % (label, min(runs), " ".join("%.3f" % v for v in runs),
                                                               max(runs) - min(runs), extra)


def on_off(ctx, say, title, sal, d_in, repeat, **more):
    """the graph entry, host arrays, option off then on, in every run; the two results compared"""
    runs, last = {0: [], 1: []}, {}
    for _ in range(repeat):
        res = {}
        for opt in (0, 1):
            with ctx.options(connect_settle=opt):
                dt, got, d = timed(lambda d: ctx.label_connected_graph(sal, direction=d, **KW, **more), d_in)
                last[opt] = ctx.label_connected_graph_last()[:2] + (ctx.label_connected_graph_last_settled(),)
            runs[opt].append(dt)
            res[opt] = (got, d)
        (g0, d0), (g1, d1) = res[0], res[1]
        assert contract_ok(g0, d0, d_in, g1[0], g1[1], d1), title
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(g0[2:], g1[2:])), title
    say("%s: %d clusters" % (title, res[1][0][1]))
    for opt in (0, 1):
        p, r, s = last[opt]
        say(line("connect_settle=%d" % opt, runs[opt], "   path: %s, reasons %d, settled %s" % (PATHS[p], r, bits(s))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=("protocol", "links", "weights", "sheet"))
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.size
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)
    ctx = api.Context(0)
    sal, direction = sheets(n)
    if a.part == "protocol":
        for volume, d_in in (("protocol", direction), ("fanned", fanned(n, sal, direction))):
            runs = {"seeded": [], "settle": []}
            for _ in range(a.repeat):
                dt, want, d0 = timed(lambda d: api.label_connected(sal, direction=d, seeds_ctx=ctx, **KW), d_in)
                runs["seeded"].append(dt)
                with ctx.options(connect_settle=1):
                    dt, got, d1 = timed(lambda d: ctx.label_connected_graph(sal, direction=d, **KW), d_in)
                    p, r = ctx.label_connected_graph_last()[:2]
                    s = ctx.label_connected_graph_last_settled()
                runs["settle"].append(dt)
                assert contract_ok(want, d0, d_in, got[0], got[1], d1), volume
            say("%d^3 %s volume, filter_mrc's call: %d clusters" % (n, volume, want[1]))
            say(line("device-seeded flood (cluster() before)", runs["seeded"]))
            say(line("graph entry, connect_settle=1", runs["settle"], "   path: %s, reasons %d, settled %s" % (PATHS[p], r, bits(s))))
    elif a.part == "links":
        d_in = fanned(n, sal, direction)
        c = n / 2.0
        shell = lambda k: (c + 0.3 * n * np.cos(0.7 * k), c + 0.3 * n * np.sin(0.7 * k), c)      # on the shell's equator
        plane = lambda k: (c + 0.2 * n * np.cos(1.3 * k), c + 0.2 * n * np.sin(1.3 * k), 0.9 * n)
        on_off(ctx, say, "%d^3 fanned volume, one group of 2 locations" % n, sal, d_in, a.repeat, must_link=[[shell(0), plane(0)]])
        groups = [[(shell if (g + l) % 2 else plane)(8 * g + l) for l in range(8)] for g in range(8)]
        on_off(ctx, say, "%d^3 fanned volume, 8 groups of 8 locations" % n, sal, d_in, a.repeat, must_link=groups)
    elif a.part == "weights":
        w = np.random.default_rng(5).uniform(0.5, 2.0, sal.shape).astype(np.float32)
        on_off(ctx, say, "%d^3 fanned volume, random voxel weights" % n, sal, fanned(n, sal, direction), a.repeat, voxel_weights=w)
    else:
        on_off(ctx, say, "%d^3 protocol volume (corrugated sheet, outward sum in doubt)" % n, sal, direction, a.repeat)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
