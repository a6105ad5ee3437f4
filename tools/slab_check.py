"""Z-slab pipeline versus the single-volume pipeline, both on the GPU, bit for bit.

Launch with one process per rank:
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 \
        --master-port 29533 tools/slab_check.py [--matrix]
--matrix runs the case list of matrix() instead (uneven splits, tight and wide ghosts, thin slabs, the peak-height
background, the host-memory faces, a plateau at the threshold, tolerance mode, refusals, a fraction that selects no
voxel; the transport's self-test on the first handle) and prints "SLAB-OK world=N
cases=..." when every case passed.
With at least as many GPUs as ranks every rank takes its own GPU and halos travel over RCCL
("nccl"); on a one-GPU box the ranks share cuda:0 and halos are staged through gloo.  Every rank
runs the slab stages; rank 0 additionally runs the whole volume and compares the gathered owned
planes and the merged blob lists.  Prints "SLAB-OK ..." on success, exits non-zero otherwise.
"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import volgen  # noqa: E402
from visfd_amd import api, pipeline, slab  # noqa: E402


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    local = int(os.environ.get("LOCAL_RANK", rank))
    ngpu = torch.cuda.device_count()
    own_gpu = ngpu >= world
    dev_index = local if own_gpu else 0
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if own_gpu:
        dist.init_process_group("nccl", device_id=dev)
    else:
        dist.init_process_group("gloo")
    shape, sigma, tv_ratio, fraction, ghost = (48, 36, 44), 1.2, 2.0, 0.15, 6
    blob_sigmas = np.array([1.0, 1.25, 1.55, 1.9], np.float32)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ctx = api.Context(dev_index, stream.cuda_stream)
    full = torch.from_numpy(volgen.membrane_volume(shape, seed=55))

    # the library's own slab handle: the C entry points of csrc/slab.hip (RCCL with one GPU per rank, torch-backed
    # callbacks when the ranks share a card); SLAB_PY=1 keeps the Python orchestration of visfd_amd/slab.py instead
    if os.environ.get("SLAB_PY"):
        L = slab.SlabLayout(shape[0], rank, world, ghost=ghost)
    else:
        L = slab.make_slab(ctx, rank, world, shape[0], ghost)
    lshape = (L.nz_local,) + tuple(shape[1:])
    src = torch.full(lshape, float("nan"), device=dev)      # ghosts must come from the exchange
    L.owned(src).copy_(full[L.z0:L.z1])
    sal = torch.zeros(lshape, device=dev)
    dirs = torch.zeros((3,) + lshape, device=dev)
    ten = torch.zeros((6,) + lshape, device=dev)
    if os.environ.get("SLAB_PY"):
        # Python orchestration: a context on a stream of its own would race with torch's halo copies -- must be refused
        # (the C path orders its transfer stream against the context's stream itself)
        other = api.Context(dev_index)
        try:
            slab.membrane_detect_slab(other, L, src, sal, dirs, ten, sigma, tv_ratio, 4, fraction)
            refused = False
        except RuntimeError as e:
            refused = "current stream" in str(e)
        other.close()
        if not refused:
            print("SLAB-MISMATCH: a context on its own stream was accepted", flush=True)
            sys.exit(1)
    thr = slab.membrane_detect_slab(ctx, L, src, sal, dirs, ten, sigma, tv_ratio, 4, fraction)
    host_bad = []
    if isinstance(L, api.Slab):
        # the host-memory face of the same stage (what filter_mrc -slab calls): owned planes in, owned planes out
        import math
        sal_h, ten_h, thr_h = L.membrane_detect_host(
            full[L.z0:L.z1].numpy(), sigma, api.ratio_from_threshold(0.03), api.DECREASING_EIVALS, fraction,
            float(np.float32(tv_ratio) * np.float32(sigma)), 4, math.sqrt(2.0), want_tensor=True)
        ctx.synchronize()
        if np.float32(thr_h) != np.float32(thr):
            host_bad.append("host-face threshold differs on rank %d" % rank)
        if not np.array_equal(sal_h.view(np.uint32), L.owned(sal).cpu().numpy().view(np.uint32)):
            host_bad.append("host-face saliency differs on rank %d" % rank)
        if not np.array_equal(ten_h.view(np.uint32), np.moveaxis(L.owned(ten).cpu().numpy(), 0, -1).view(np.uint32)):
            host_bad.append("host-face tensor differs on rank %d" % rank)
    src2 = torch.full(lshape, float("nan"), device=dev)
    L.owned(src2).copy_(full[L.z0:L.z1])
    mins, maxs = slab.blob_detect_slab(ctx, L, src2, blob_sigmas, 0.03, 0.02, -5.0, 5.0, False)
    ctx.synchronize()
    # a list capacity far too small on ONE rank only: that rank's retry is local (the ghost planes are in place), so the
    # other ranks are not held up and the merged lists are the same
    src3 = torch.full(lshape, float("nan"), device=dev)
    L.owned(src3).copy_(full[L.z0:L.z1])
    mins_c, maxs_c = slab.blob_detect_slab(ctx, L, src3, blob_sigmas, 0.03, 0.02, -5.0, 5.0, False, cap=(2 if rank == world - 1 else 1 << 22))
    ctx.synchronize()
    for name, a, b in (("minima", mins, mins_c), ("maxima", maxs, maxs_c)):
        if a.shape != b.shape or not np.array_equal(volgen.sort_blobs(a, True).view(np.uint32), volgen.sort_blobs(b, True).view(np.uint32)):
            host_bad.append("blob %s differ after a capacity retry on rank %d" % (name, rank))

    part = dict(z0=L.z0, z1=L.z1, thr=np.float32(thr), sal=L.owned(sal).cpu().numpy(),
                ten=L.owned(ten).cpu().numpy(), mins=mins, maxs=maxs, host_bad=host_bad)
    parts = [None] * world
    dist.all_gather_object(parts, part)

    bad = []
    if rank == 0:
        vol = full.to(dev)
        fsal = torch.zeros(shape, device=dev)
        fdirs = torch.zeros((3,) + shape, device=dev)
        ften = torch.zeros((6,) + shape, device=dev)
        fthr = pipeline.membrane_detect(ctx, vol, fsal, fdirs, ften, sigma, tv_ratio, 4, fraction)
        fmins, fmaxs = pipeline.blob_detect(ctx, vol, blob_sigmas, 0.03, 0.02, None, -5.0, 5.0, False)
        ctx.synchronize()
        fsal, ften = fsal.cpu().numpy(), ften.cpu().numpy()
        if not np.abs(ften).max() > 0:
            bad.append("vote tensor is all zero")
        for p in parts:
            bad.extend(p["host_bad"])
            z0, z1 = p["z0"], p["z1"]
            if np.float32(p["thr"]) != np.float32(fthr):
                bad.append("threshold differs on planes %d..%d" % (z0, z1))
            if not np.array_equal(p["sal"].view(np.uint32), fsal[z0:z1].view(np.uint32)):
                bad.append("saliency differs on planes %d..%d" % (z0, z1))
            if not np.array_equal(p["ten"].view(np.uint32), ften[:, z0:z1].view(np.uint32)):
                bad.append("vote tensor differs on planes %d..%d" % (z0, z1))
            for name, got, want, asc in (("minima", p["mins"], fmins, True), ("maxima", p["maxs"], fmaxs, False)):
                a, b = volgen.sort_blobs(got, asc), volgen.sort_blobs(want, asc)
                if a.shape != b.shape or not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
                    bad.append("%s differ (%d vs %d)" % (name, len(a), len(b)))
        if not bad:
            print("SLAB-OK world=%d backend=%s path=%s minima=%d maxima=%d thr=%.6g" %
                  (world, dist.get_backend(), "python" if os.environ.get("SLAB_PY") else "c-abi", len(fmins), len(fmaxs), fthr),
                  flush=True)
        else:
            print("SLAB-MISMATCH: " + "; ".join(bad), flush=True)
    flag = [bool(bad)]
    dist.broadcast_object_list(flag, src=0)
    if hasattr(L, "close"):
        L.close()
    ctx.close()
    dist.destroy_process_group()
    sys.exit(1 if flag[0] else 0)


# ---- the case matrix (--matrix) ---------------------------------------------------------------------------------------
# Depths of the stages below at truncate 0.03 (ratio 2.6482): ridge floor(1.2 * ratio) + 1 = 4 (sigma 2.0: 6), vote
# h_tv = floor(sigma_tv * sqrt 2) = 3 at tv ratio 2.0 (6 at 3.6), background floor(2.0 * ratio) = 5, blob halo 6 for
# sigma 1.9 and 5 for sigma 1.4954885 (the float window: a double-precision restatement gives 4).
BLOB4 = np.array([1.0, 1.25, 1.55, 1.9], np.float32)
BLOB_SEAM = np.array([1.0, 1.2, 1.4954885], np.float32)
TOLERANCE = dict(tv_fma=1, gauss_fma=1, eig_f32=1)     # bench.py's MODE_OPTS["tolerance"]
EXACT = dict(tv_fma=0, gauss_fma=0, eig_f32=0)
PV = 0.005                                             # tests/test_tolerance_modes.py: the per-voxel bound


def _cases(world):
    """(name, nz, ghost, options): every case gets a fresh slab handle; ghosts start as NaN."""
    uneven = {2: 47, 3: 50, 4: 47}[world]
    return [
        ("uneven", dict(nz=uneven, ghost=9, selftest=True)),
        ("tight", dict(nz=12 * world + 1, ghost=5, blobs=BLOB_SEAM, seam_blob=True)),       # ghost = blob depth 5
        ("tight-wide", dict(nz=12 * world + 1, ghost=11, blobs=BLOB_SEAM, seam_blob=True)),
        ("tight-tv", dict(nz=8 * world + 3, ghost=6, tv_ratio=3.6)),                         # ghost = h_tv = blob depth 6
        ("tight-gauss", dict(nz=8 * world + 2, ghost=6, sigma=2.0, tv_ratio=1.0)),           # ghost = h_gauss + 1 = 6
        ("thin", dict(nz=6 * world, ghost=6)),                    # slabs exactly 6 planes: the middle ranks' vote-split else
        ("background", dict(nz=10 * world + 1, ghost=5, sigma_bg=2.0, blobs=None)),          # ghost = h_bg = 5
        ("host-faces", dict(nz=11 * world + 2, ghost=9, host=True)),
        ("plateau", dict(nz=12 * world + 1, ghost=6, plateau=True)),
        ("tolerance", dict(nz=uneven, ghost=9, opts=TOLERANCE, blobs=None)),
        ("refusals", dict(nz=10 * world + 1, ghost=4, refusals=True, blobs=None)),
        ("no-voxel", dict(nz=10 * world + 1, ghost=4, no_voxel=True, blobs=None)),
    ]


def _volume(nz, seed, seam_z=None, plateau=False):
    vol = volgen.membrane_volume((nz, 36, 44), seed=seed)
    if seam_z is not None:   # a dark blob (radius ~2) whose centre lies on the first plane of a rank
        z, y, x = np.meshgrid(np.arange(nz), np.arange(36), np.arange(44), indexing="ij")
        vol -= (3000.0 * np.exp(-((z - seam_z) ** 2 + (y - 20) ** 2 + (x - 30) ** 2) / (2 * 1.4 ** 2))).astype(np.float32)
    if plateau:              # a constant block across the middle ranks: its ridge scores are one long run of equal values
        vol[nz // 4:3 * nz // 4] = np.float32(1000.0)
    return np.ascontiguousarray(vol, np.float32)


def _run_case(ctx, dev, rank, world, name, c, O):
    """This rank's part of one case -> dict of owned planes / lists / flags (gathered on rank 0)."""
    import math
    nz, ghost = c["nz"], c["ghost"]
    sigma, tv_ratio = c.get("sigma", 1.2), c.get("tv_ratio", 2.0)
    sigma_bg, blobs = c.get("sigma_bg", 0.0), c.get("blobs", BLOB4)
    ratio = api.ratio_from_threshold(0.03)
    sigma_tv = float(np.float32(tv_ratio) * np.float32(sigma))
    seam_z = slab.SlabLayout(nz, 1, world, 0).z0 if c.get("seam_blob") else None
    full = _volume(nz, 55 + nz, seam_z, c.get("plateau", False))
    fraction = 0.15
    if c.get("plateau"):
        # the cut in the middle of the run of equal scores (the oracle's scores are the exact kernels' bit for bit)
        _, hess = O.calc_hessian(full, sigma, ratio, None, want_grad=False)
        raw, _ = O.hessian_saliency(hess, api.DECREASING_EIVALS)
        top = raw.max()
        run = int((raw == raw[nz // 2, 18, 22]).sum())
        assert run >= 1000 and raw[nz // 2, 18, 22] != top
        above = int((raw > raw[nz // 2, 18, 22]).sum())
        fraction = float(np.float32((above + run // 2) / raw.size))
    L = slab.make_slab(ctx, rank, world, nz, ghost)
    out = dict(z0=L.z0, z1=L.z1, fraction=fraction, seam_z=seam_z)
    lshape = (L.nz_local, 36, 44)
    if c.get("selftest"):
        # the exchange routine of the halos with this rank as its own peer, and the select's sum over the ranks
        try:
            L.selftest(1 << 12)
            out["selftest_bad"] = None
        except api.VisfdHipError as e:
            out["selftest_bad"] = str(e)

    def fresh():
        t = torch.full(lshape, float("nan"), device=dev)
        L.owned(t).copy_(torch.from_numpy(full[L.z0:L.z1]))
        return t
    with ctx.options(**c.get("opts", EXACT)):
        if c.get("refusals"):
            # every window deeper than the ghost zone is refused on every rank before anything is exchanged ...
            flags = []
            for what, call in (
                    ("blob", lambda: L.blob_dog(fresh(), BLOB4, 0.02, ratio, -5.0, 5.0)),
                    ("background", lambda: L.membrane_detect(fresh(), torch.zeros(lshape, device=dev), torch.zeros((3,) + lshape, device=dev),
                                                             torch.zeros((6,) + lshape, device=dev), torch.zeros(lshape, device=dev), sigma,
                                                             ratio, api.DECREASING_EIVALS, fraction, sigma_tv, 4, math.sqrt(2.0), False,
                                                             2.0, torch.zeros(lshape, device=dev))),
                    ("ridge", lambda: L.membrane_detect(fresh(), torch.zeros(lshape, device=dev), torch.zeros((3,) + lshape, device=dev),
                                                        torch.zeros((6,) + lshape, device=dev), torch.zeros(lshape, device=dev), 1.6,
                                                        ratio, api.DECREASING_EIVALS, fraction, sigma_tv, 4, math.sqrt(2.0))),
                    ("gauss-host", lambda: L.gauss_host(full[L.z0:L.z1], (1.0, 1.0, 2.0), (2, 2, 5), True))):
                try:
                    call()
                    flags.append(what + ": accepted")
                except api.VisfdHipError as e:
                    if "ghost depth too small" not in str(e):
                        flags.append(what + ": " + str(e))
            out["refusal_bad"] = flags
            ctx.synchronize()
            # ... and the same handle then runs a stage that fits (the membrane stage needs 4 planes)
        if c.get("no_voxel"):
            # best_fraction 1.0 of far fewer than 2^24 voxels: the float product is n itself, the rank one past the last voxel.
            # Round 0's pick finds that out on every rank from the same summed counters; the error comes once all three
            # rounds and their sums have been queued, so the ranks' collectives stay matched and the handle stays usable
            try:
                L.membrane_detect(fresh(), torch.zeros(lshape, device=dev), torch.zeros((3,) + lshape, device=dev),
                                  torch.zeros((6,) + lshape, device=dev), torch.zeros(lshape, device=dev), sigma, ratio,
                                  api.DECREASING_EIVALS, 1.0, sigma_tv, 4, math.sqrt(2.0))
                out["refusal_bad"] = ["fraction 1.0: accepted"]
            except api.VisfdHipError as e:
                out["refusal_bad"] = [] if e.code == 1 and "selects no voxel" in str(e) else ["fraction 1.0: " + str(e)]
            ctx.synchronize()
        src, sal = fresh(), torch.zeros(lshape, device=dev)
        dirs, ten = torch.zeros((3,) + lshape, device=dev), torch.zeros((6,) + lshape, device=dev)
        bg = torch.full(lshape, float("nan"), device=dev) if sigma_bg > 0 else None
        thr = L.membrane_detect(src, sal, dirs, ten, torch.empty(lshape, device=dev), sigma, ratio, api.DECREASING_EIVALS, fraction,
                                sigma_tv, 4, math.sqrt(2.0), False, sigma_bg, bg, True)
        ctx.synchronize()
        out.update(thr=np.float32(thr), sal=L.owned(sal).cpu().numpy(), ten=L.owned(ten).cpu().numpy())
        if sigma_bg > 0:   # the host-memory face of the same stage
            sal_h, ten_h, thr_h = L.membrane_detect_host(full[L.z0:L.z1], sigma, ratio, api.DECREASING_EIVALS, fraction, sigma_tv, 4,
                                                         math.sqrt(2.0), want_tensor=True, sigma_background=sigma_bg)
            out.update(thr_h=np.float32(thr_h), sal_h=sal_h, ten_h=np.ascontiguousarray(np.moveaxis(ten_h, -1, 0)))
        if blobs is not None:
            mins, maxs = slab.blob_detect_slab(ctx, L, fresh(), blobs, 0.03, 0.02, -5.0, 5.0, False)
            ctx.synchronize()
            out.update(mins=mins, maxs=maxs)
        if c.get("host"):
            for key, sg, nrm in (("g_aniso", (1.0, 1.6, 2.2), True), ("g_aniso0", (1.0, 1.6, 2.2), False), ("g_iso", (2.0, 2.0, 2.0), True)):
                hw = api.gauss_halfwidths(sg, ratio)
                out[key], out[key + "_A"] = L.gauss_host(full[L.z0:L.z1], sg, hw, nrm)
            out["hmins"], out["hmaxs"] = L.blob_dog_host(full[L.z0:L.z1], blobs, 0.02, ratio, -5.0, 5.0)
    L.close()
    return out, full


def _single_volume(ctx, dev, name, c, full, parts, O):
    """Rank 0: the whole volume on one GPU (and, in exact mode, the CPU oracle) against the gathered parts -> problems."""
    bad = []
    nz = c["nz"]
    sigma, tv_ratio = c.get("sigma", 1.2), c.get("tv_ratio", 2.0)
    sigma_bg, blobs = c.get("sigma_bg", 0.0), c.get("blobs", BLOB4)
    fraction = parts[0]["fraction"]
    ratio = api.ratio_from_threshold(0.03)
    opts = c.get("opts", EXACT)
    tol = opts is TOLERANCE
    vol = torch.from_numpy(full).to(dev)
    shape = full.shape
    fsal, fdirs, ften = torch.zeros(shape, device=dev), torch.zeros((3,) + shape, device=dev), torch.zeros((6,) + shape, device=dev)
    with ctx.options(**opts):
        fthr = np.float32(pipeline.membrane_detect(ctx, vol, fsal, fdirs, ften, sigma, tv_ratio, 4, fraction, sigma_background=sigma_bg))
        fmins = fmaxs = None
        if blobs is not None:
            fmins, fmaxs = pipeline.blob_detect(ctx, vol, blobs, 0.03, 0.02, None, -5.0, 5.0, False)
        ctx.synchronize()
    fsal, ften = fsal.cpu().numpy(), ften.cpu().numpy()
    if not np.abs(ften).max() > 0:
        bad.append("vote tensor is all zero")

    def same(a, b):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))

    def close(a, b, what):
        a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
        scale = float(np.abs(b64).max())
        err = float(np.abs(a64 - b64).max())
        if err > 1e-5 * scale:
            bad.append("%s: max|a-b| %g > 1e-5 * %g" % (what, err, scale))
        sig = np.abs(b64) > 1e-3 * scale
        over = float((np.abs(a64 - b64)[sig] > 1e-5 * np.abs(b64[sig])).mean()) if sig.any() else 0.0
        if over > PV:
            bad.append("%s: %.4f of the significant voxels beyond 1e-5 of their value" % (what, over))

    for p in parts:
        z0, z1 = p["z0"], p["z1"]
        where = "planes %d..%d" % (z0, z1)
        if p.get("selftest_bad"):
            bad.append("self-test on %s: %s" % (where, p["selftest_bad"]))
        if p.get("refusal_bad"):
            bad.append("refusals on %s: %s" % (where, "; ".join(p["refusal_bad"])))
        if p["thr"] != fthr:
            bad.append("threshold %r differs from the single volume's %r on %s" % (float(p["thr"]), float(fthr), where))
        if tol:
            close(p["ten"], ften[:, z0:z1], "tolerance-mode vote tensor on " + where)
            close(p["sal"], fsal[z0:z1], "tolerance-mode post-vote saliency on " + where)
        else:
            if not same(p["sal"], fsal[z0:z1]):
                bad.append("post-vote saliency differs on " + where)
            if not same(p["ten"], ften[:, z0:z1]):
                bad.append("vote tensor differs on " + where)
        if "thr_h" in p and not (p["thr_h"] == p["thr"] and same(p["sal_h"], p["sal"]) and same(p["ten_h"], p["ten"])):
            bad.append("host face of the background stage differs from the device face on " + where)
        if "g_iso" in p:
            for key, sg, nrm in (("g_aniso", (1.0, 1.6, 2.2), True), ("g_aniso0", (1.0, 1.6, 2.2), False), ("g_iso", (2.0, 2.0, 2.0), True)):
                hw = api.gauss_halfwidths(sg, ratio)
                gd = torch.empty_like(vol)
                A = ctx.gauss_dev(vol, gd, sg, hw, None, nrm)
                ctx.synchronize()
                want, A_o = O.gauss_hw(full, sg, hw, None, nrm)
                if not (same(p[key], gd.cpu().numpy()[z0:z1]) and same(p[key], want[z0:z1])):
                    bad.append("host-face Gaussian %s differs on %s" % (key, where))
                if not (np.float32(p[key + "_A"]) == np.float32(A) == np.float32(A_o)):
                    bad.append("host-face Gaussian %s: A differs" % key)
            hm, hx = p["hmins"], p["hmaxs"]
            own = lambda rows: rows[(rows[:, 2] >= z0) & (rows[:, 2] < z1)]
            for what, got, want, asc in (("minima", hm, fmins, True), ("maxima", hx, fmaxs, False)):
                if not same(volgen.sort_blobs(got, asc), volgen.sort_blobs(own(want), asc)):
                    bad.append("host-face blob %s differ on %s (%d vs %d)" % (what, where, len(got), len(own(want))))
        if blobs is not None:
            for what, got, want, asc in (("minima", p["mins"], fmins, True), ("maxima", p["maxs"], fmaxs, False)):
                if not same(volgen.sort_blobs(got, asc), volgen.sort_blobs(want, asc)):
                    bad.append("blob %s differ (%d vs %d)" % (what, len(got), len(want)))
    if blobs is not None and len(fmins) + len(fmaxs) < 5:
        bad.append("too few blobs (%d) for the comparison to mean anything" % (len(fmins) + len(fmaxs)))
    if parts[0]["seam_z"] is not None:
        sz = parts[0]["seam_z"]
        if not any(int(r[2]) == sz and abs(r[0] - 30) <= 1 and abs(r[1] - 20) <= 1 for r in fmins):
            bad.append("no minimum found on the seam plane %d" % sz)
    if not tol and sigma_bg == 0:
        # the CPU oracle: the blob lists bit for bit; the threshold within the tolerance the single-volume suite allows for the
        # eigenvalue stage (tests/test_gpu_parity.py)
        _, hess = O.calc_hessian(full, sigma, ratio, None, want_grad=False)
        raw, _ = O.hessian_saliency(hess, api.DECREASING_EIVALS)
        thr_o = O.threshold_fraction(raw.copy(), fraction)
        if abs(float(fthr) - float(thr_o)) > 1e-5 * float(np.abs(raw).max()):
            bad.append("threshold %r vs oracle %r" % (float(fthr), float(thr_o)))
        if blobs is not None:
            a, b = O.blob_dog(full, blobs, None, None, 0.02, ratio, -5.0, 5.0, False)
            if not (same(volgen.sort_blobs(a, True), volgen.sort_blobs(fmins, True)) and
                    same(volgen.sort_blobs(b, False), volgen.sort_blobs(fmaxs, False))):
                bad.append("single-volume blob lists differ from the oracle's")
    return ["%s: %s" % (name, b) for b in bad]


def matrix():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    local = int(os.environ.get("LOCAL_RANK", rank))
    own_gpu = torch.cuda.device_count() >= world
    dev_index = local if own_gpu else 0
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if own_gpu:
        dist.init_process_group("nccl", device_id=dev)
    else:
        dist.init_process_group("gloo")
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ctx = api.Context(dev_index, stream.cuda_stream)
    from oracle import pyoracle as po
    O = po.load("oracle")
    bad, names = [], []
    for name, c in _cases(world):
        out, full = _run_case(ctx, dev, rank, world, name, c, O)
        parts = [None] * world
        dist.all_gather_object(parts, out)
        if rank == 0:
            problems = _single_volume(ctx, dev, name, c, full, parts, O)
            bad.extend(problems)
            print("case %-12s nz=%d ghost=%d planes=%s thr=%.6g %s" % (
                name, c["nz"], c["ghost"], [p["z1"] - p["z0"] for p in parts], float(parts[0]["thr"]),
                "ok" if not problems else "MISMATCH"), flush=True)
        names.append(name)
    if rank == 0:
        if not bad:
            print("SLAB-OK world=%d cases=%s" % (world, ",".join(names)), flush=True)
        else:
            print("SLAB-MISMATCH: " + "; ".join(bad), flush=True)
    flag = [bool(bad)]
    dist.broadcast_object_list(flag, src=0)
    ctx.close()
    dist.destroy_process_group()
    sys.exit(1 if flag[0] else 0)


if __name__ == "__main__":
    if "--matrix" in sys.argv:
        matrix()
    else:
        main()
