"""Times FindSpheres (csrc/find_spheres.hip) and writes profiles/find_spheres_time.txt:

    python tools/find_spheres_time.py [--out profiles/find_spheres_time.txt] [--quick]

Spheres: centres uniform in a 1024^3 box, diameters uniform in [4, 12] voxels; queries uniform in the box.  Per point of the
grid n_spheres in {10^4, 10^6, 10^7} x n_crds in {10^2, 10^4}:
  device   visfd_hip_find_spheres_dev on device arrays: both preparation launches, the wait for their flag word, the
           search; median of 5 after one warm-up, a host clock around the call and a wait for the context's stream
  staged   visfd_hip_find_spheres on host arrays: the same plus the copies up and down
  host     visfd_hip_find_spheres_host, the walk over the pairs (one run; above 2 * 10^9 pairs a subset of the queries
           is walked and the time scaled to all of them, marked "~")
  table    a C++ restatement of what the reference does for the same lists -- allocate a table of 1024^3 entries of 8
           bytes (its Integer is size_t on this path), zero it, paint every sphere, read the queries off -- compiled by
           this tool with g++ -O3 and run once per list; tool-only, nothing of it is shipped
Rates are nominal pairs (n_crds * n_spheres) per second.  "copy" is a device-to-device copy of the record array
(16 bytes per sphere), the least a single batch of queries can cost; the file gives copy / device.

The second table decides filter_mrc's FIND_SPHERES_MIN_PAIRS: for 200 training points and a growing blob list, the host
walk against ONE staged device call in a fresh process, context creation included (what a command-line run pays)."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BOX = 1024

TABLE_CPP = r"""
// what FindSpheres of the reference does, restated: a table over the box, every sphere painted in list order
#include <chrono>
#include <cmath>
#include <cstdio>
#include <vector>
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb");
  long ns, nq;
  if (!f || fread(&ns, 8, 1, f) != 1 || fread(&nq, 8, 1, f) != 1) return 2;
  std::vector<float> c(3 * ns), d(ns), q(3 * nq);
  if (fread(c.data(), 4, 3 * ns, f) != (size_t)(3 * ns) || fread(d.data(), 4, ns, f) != (size_t)ns ||
      fread(q.data(), 4, 3 * nq, f) != (size_t)(3 * nq)) return 2;
  fclose(f);
  const long N = BOXSIZE;
  auto t0 = std::chrono::steady_clock::now();
  std::vector<size_t> table((size_t)N * N * N);
  for (size_t i = 0; i < table.size(); i++) table[i] = 0;
  for (long i = 0; i < ns; i++) {
    const int ix = (int)c[3 * i], iy = (int)c[3 * i + 1], iz = (int)c[3 * i + 2];
    int R = (int)std::ceil(d[i] / 2 - 0.5);
    if (R < 0) R = 0;
    int Rsqr = (int)std::ceil((d[i] / 2) * (d[i] / 2) - 0.5);
    if (Rsqr < 0) Rsqr = 0;
    for (int jz = -R; jz <= R; jz++)
      for (int jy = -R; jy <= R; jy++)
        for (int jx = -R; jx <= R; jx++) {
          if (jx * jx + jy * jy + jz * jz > Rsqr) continue;
          const long x = ix + jx, y = iy + jy, z = iz + jz;
          if (x < 0 || x >= N || y < 0 || y >= N || z < 0 || z >= N) continue;
          table[((size_t)z * N + y) * N + x] = (size_t)i + 1;
        }
  }
  unsigned long long sum = 0;
  for (long k = 0; k < nq; k++) sum += table[(((size_t)(int)q[3 * k + 2]) * N + (int)q[3 * k + 1]) * N + (int)q[3 * k]];
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  printf("%.3f %llu\n", ms, sum);
  return 0;
}
"""

CHILD = r"""
import sys, time
import numpy as np
sys.path.insert(0, sys.argv[1])
from visfd_amd import api
api.load_library()
n_blobs, n_training = int(sys.argv[2]), int(sys.argv[3])
rng = np.random.default_rng(3)
c = rng.uniform(0, 1024, (n_blobs, 3)).astype(np.float32)
d = rng.uniform(4, 12, n_blobs).astype(np.float32)
q = (c[rng.integers(0, n_blobs, n_training)] + 0.3).astype(np.float32)   # training points lie in blobs
t0 = time.perf_counter()
ctx = api.Context(0)
t1 = time.perf_counter()
ids = ctx.find_spheres(q, c, d)
t2 = time.perf_counter()
ctx.close()
t3 = time.perf_counter()
h0 = time.perf_counter()
want = api.find_spheres_host(q, c, d)
h1 = time.perf_counter()
assert np.array_equal(ids, want)
print("%.3f %.3f %.3f %.3f" % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (h1 - h0) * 1e3))
"""


def lists(n_spheres, n_crds, seed=1):
    rng = np.random.default_rng(seed)
    c = rng.uniform(0, BOX, (n_spheres, 3)).astype(np.float32)
    d = rng.uniform(4, 12, n_spheres).astype(np.float32)
    q = rng.uniform(0, BOX, (n_crds, 3)).astype(np.float32)
    return q, c, d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "find_spheres_time.txt"))
    ap.add_argument("--quick", action="store_true", help="a small grid and a small table: a rehearsal of the tool itself")
    a = ap.parse_args()
    import torch
    from visfd_amd import api
    ctx = api.Context(0)
    dev = torch.device("cuda", 0)
    box = 64 if a.quick else BOX
    grid_s = [10 ** 3, 10 ** 4] if a.quick else [10 ** 4, 10 ** 6, 10 ** 7]
    grid_q = [10, 100] if a.quick else [10 ** 2, 10 ** 4]
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "table_paint")
    with open(exe + ".cpp", "w") as f:
        f.write(TABLE_CPP.replace("BOXSIZE", str(box)))
    subprocess.check_call(["g++", "-O3", "-o", exe, exe + ".cpp"])

    def timed(fn, reps=5):
        fn()
        ctx.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    rows = ["%10s %8s | %11s %12s | %11s | %13s %12s | %12s | %11s %13s" % (
        "n_spheres", "n_crds", "device ms", "pairs/s", "staged ms", "host ms", "pairs/s", "table ms", "copy ms", "copy/device")]
    for ns in grid_s:
        table_ms = {}
        for nq in grid_q:
            q, c, d = lists(ns, nq)
            q, c = q * (box / BOX), c * (box / BOX)
            tq, tc, td = (torch.from_numpy(x).to(dev) for x in (q, c, d))
            ids = torch.empty(nq, dtype=torch.int64, device=dev)
            dev_ms = timed(lambda: ctx.find_spheres_dev(tq, tc, td, ids=ids))
            got = ids.cpu().numpy()
            staged_ms = timed(lambda: ctx.find_spheres(q, c, d))
            pairs = float(ns) * nq
            sub = nq if pairs <= 2e9 else max(1, int(2e9 // ns))
            t0 = time.perf_counter()
            want = api.find_spheres_host(q[:sub], c, d)
            host_ms = (time.perf_counter() - t0) * 1e3 * (nq / sub)
            assert np.array_equal(got[:sub], want), "device and host disagree"
            with open(os.path.join(tmp, "lists.bin"), "wb") as f:
                np.array([ns, nq], np.int64).tofile(f)
                c.tofile(f)
                d.tofile(f)
                q.tofile(f)
            out = subprocess.check_output([exe, os.path.join(tmp, "lists.bin")], text=True).split()
            table_ms[nq] = float(out[0])
            assert int(out[1]) == int(got.sum()), "the table painting and the device disagree"
            x = torch.empty(4 * ns, dtype=torch.float32, device=dev)
            y = torch.empty_like(x)
            copy_ms = timed(lambda: y.copy_(x))
            rows.append("%10d %8d | %11.3f %12.3g | %11.3f | %12.1f%s %12.3g | %12.1f | %11.4f %13.4f" % (
                ns, nq, dev_ms, pairs / dev_ms * 1e3, staged_ms, host_ms, "~" if sub < nq else " ", pairs / host_ms * 1e3,
                table_ms[nq], copy_ms, copy_ms / dev_ms))
            print(rows[-1], flush=True)
    cross = ["%10s %10s %12s | %10s %10s %10s %12s | %10s" % ("n_blobs", "n_training", "pairs", "context ms", "call ms",
                                                                "close ms", "device sum", "host ms")]
    for nb in ([10 ** 3, 10 ** 4] if a.quick else [10 ** 3, 10 ** 4, 10 ** 5, 10 ** 6, 10 ** 7]):
        out = subprocess.check_output([sys.executable, "-c", CHILD, ROOT, str(nb), "200"], text=True).split()
        t_ctx, t_call, t_close, t_host = (float(x) for x in out)
        cross.append("%10d %10d %12.3g | %10.1f %10.1f %10.1f %12.1f | %10.1f" % (nb, 200, nb * 200.0, t_ctx, t_call, t_close,
                                                                               t_ctx + t_call + t_close, t_host))
        print(cross[-1], flush=True)
    text = ("FindSpheres, %s, box %d^3, diameters 4...12 voxels%s\n" % (torch.cuda.get_device_name(0), box,
                                                                      " (--quick: a rehearsal, not a measurement)" if a.quick else "") +
            "\n".join(rows) + "\n\n" +
            "one staged call in a fresh process (training points inside blobs), against the host walk of the same lists:\n" +
            "\n".join(cross) + "\n")
    print(text)
    with open(a.out, "w") as f:
        f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
