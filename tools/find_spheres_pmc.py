"""The search kernel of csrc/find_spheres.hip under rocprofv3: its own time and its VALU counters (development aid).

    rocprofv3 --kernel-trace --output-format csv -d OUT/trace -- python tools/find_spheres_pmc.py run
    rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_BUSY_CU_CYCLES GRBM_GUI_ACTIVE --output-format csv -d OUT/pmc -- \
        python tools/find_spheres_pmc.py run
    python tools/find_spheres_pmc.py collect OUT        # -> OUT/summary.txt

`run` searches 10^7 spheres x 10^4 points (the lists of tools/find_spheres_time.py) three times on device arrays.
`collect` prints, per launch of search_kernel, the traced time and the counters, and what they give: pairs per second
by kernel time, VALU instructions per pair (SQ_INSTS_VALU counts wave instructions: x 64 lanes / pairs), the clock
GRBM_GUI_ACTIVE / kernel time, and the VALU issue rate per SIMD.  Counters are collected in a run of their own; the traced time comes from the other run."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NS, NQ = 10 ** 7, 10 ** 4


def run():
    import numpy as np
    import torch
    from visfd_amd import api
    rng = np.random.default_rng(1)
    c = rng.uniform(0, 1024, (NS, 3)).astype(np.float32)
    d = rng.uniform(4, 12, NS).astype(np.float32)
    q = rng.uniform(0, 1024, (NQ, 3)).astype(np.float32)
    dev = torch.device("cuda", 0)
    ctx = api.Context(0)
    tq, tc, td = (torch.from_numpy(x).to(dev) for x in (q, c, d))
    ids = torch.empty(NQ, dtype=torch.int64, device=dev)
    for _ in range(3):
        ctx.find_spheres_dev(tq, tc, td, ids=ids)
        ctx.synchronize()
    print("covered queries:", int((ids > 0).sum()))
    ctx.close()


def collect(out):
    pairs = float(NS) * NQ
    lines = []
    times = []
    for f in glob.glob(os.path.join(out, "trace", "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "search_kernel" in r["Kernel_Name"]:
                times.append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    for t in times:
        lines.append("search_kernel, traced: %.3f ms  -> %.3g pairs/s" % (t, pairs / t * 1e3))
    counters = {}
    for f in glob.glob(os.path.join(out, "pmc", "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "search_kernel" in r["Kernel_Name"]:
                counters.setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
    for name in sorted(counters):
        v = counters[name]
        lines.append("search_kernel, %-22s per launch %.6g (launches %d)" % (name, sum(v) / len(v), len(v)))
    if "SQ_INSTS_VALU" in counters:
        v = counters["SQ_INSTS_VALU"]
        lines.append("VALU instructions per pair: %.2f (wave instructions x 64 lanes / %.3g pairs)" % (sum(v) / len(v) * 64 / pairs, pairs))
    if "GRBM_GUI_ACTIVE" in counters and times:
        v = counters["GRBM_GUI_ACTIVE"]
        t = sorted(times)[len(times) // 2]
        cyc = sum(v) / len(v)
        lines.append("GRBM_GUI_ACTIVE / traced time: %.3f GHz summed, %.3f GHz if the counter adds the chip's 8 XCDs (cycles of the "
                     "counters run over the median time of the trace run)" % (cyc / (t * 1e6), cyc / 8 / (t * 1e6)))
        if "SQ_INSTS_VALU" in counters:
            w = sum(counters["SQ_INSTS_VALU"]) / len(counters["SQ_INSTS_VALU"])
            lines.append("VALU wave instructions per SIMD and cycle: %.3f of the 0.25 a 16-lane SIMD can issue for 64-lane waves "
                         "(1024 SIMDs, cycles per XCD as above)" % (w / 1024 / (cyc / 8)))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(os.path.join(out, "summary.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "collect":
        collect(sys.argv[2])
    else:
        run()
