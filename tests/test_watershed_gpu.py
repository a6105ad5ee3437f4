"""Watershed on the GPU (csrc/watershed.hip) through the C ABI, the C++ drop-in, and filter_mrc's flags against the
reference program itself.  Every comparison is exact: label images voxel for voxel, lists element for element with scores
as bit patterns, output files byte for byte.

The kernels are held to the sequential flood.  tests/test_watershed.py holds both statements of it -- the heapq
restatement (tests/watershed_np.py) and the library's host flood (visfd_hip_watershed_host) -- to the reference program's
recorded output.  Here the heapq restatement is the reference for a selection on every shape, and the host flood, which is
a hundred times faster, for the full crossing of the options (one reference per volume and option set, computed once)."""
import ctypes as C
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

import extrema_cases as EC
import volgen
import watershed_cases as WC
import watershed_np
from conftest import GOLDEN, ROOT, assert_bits_equal

pytestmark = pytest.mark.gpu

INF = float("inf")
ODD = (23, 50, 37)        # nz, ny, nx: odd, unequal, no multiple of a tile
THIN = (40, 33, 1)
WIDE = (9, 10, 130)       # crosses the 64-wide tile edge twice
CUBE = (64, 64, 64)
SHAPES = {"37x50x23": ODD, "nx1": THIN, "130x10x9": WIDE}


@pytest.fixture(scope="module")
def api():
    from visfd_amd import api
    return api


@pytest.fixture(scope="module")
def ctx(api):
    c = api.Context(0)
    yield c
    c.close()


def same(got, want, what):
    for k, name in enumerate(("labels", "basin index", "basin score")):
        assert_bits_equal(got[k], want[k], "%s %s" % (what, name))


def check(ctx, api, src, mask=None, what="", reference=None, **kw):
    """One call through the host face against the sequential flood (the library's on the host, unless a reference is given);
    -> (the reference's result, the call's statistics)."""
    want = reference or api.watershed_host(src, mask, **kw)
    got = ctx.watershed(src, mask, **kw)
    same(got, want, what)
    stats = ctx.watershed_last_stats()
    assert stats[0] == api.WATERSHED_PATH_DEVICE and stats[3] == len(want[1]), (what, stats)
    return want, stats


def levels(src, mask, thr, from_min):
    """L: the number of distinct eligible values."""
    v = src[mask != 0] if mask is not None else src.reshape(-1)
    if thr is not None:
        v = v[v <= thr] if from_min else v[v >= thr]
    return len(np.unique(v))          # -0 and +0 are one value for numpy too


def rounds_within_bound(stats, src, mask, thr, from_min, what):
    """The dependency depth of the propagation: per distinct value, the joins first and then the plateau components, so
    2 L rounds, plus the seed round and the final round that changes nothing."""
    L = levels(src, mask, thr, from_min)
    assert 1 <= stats[1] <= 2 * L + 4, (what, "label rounds", stats[1], "distinct values", L)


def crossed(thr_min, thr_max):
    for from_min, c, show, thr in itertools.product((True, False), (1, 2, 3), (True, False), (False, True)):
        t = (thr_min if from_min else thr_max) if thr else None
        yield ("%s c%d %s %s" % ("min" if from_min else "max", c, "show" if show else "hide", "thr" if thr else "nothr"),
               dict(start_from_minima=from_min, connectivity=c, show_boundaries=show, halt_threshold=t))


def masks_for(shape, seed):
    return {"nomask": None, "random": EC.random_mask(shape, seed), "walled": EC.walled_volume(shape, seed + 1)[1]}


@pytest.mark.parametrize("shape", list(SHAPES.values()), ids=list(SHAPES))
def test_smooth_noise_all_options(ctx, api, shape):
    src = EC.smooth_noise(shape, 51)
    basins = boundaries = 0
    for mname, mask in masks_for(shape, 52).items():
        for what, kw in crossed(0.5, -0.5):
            w, _ = check(ctx, api, src, mask, what="smooth %s %s" % (mname, what), **kw)
            basins += len(w[1])
            boundaries += int((w[0] == 0).sum())
    assert basins > 500 and boundaries > 1000


@pytest.mark.parametrize("shape", list(SHAPES.values()), ids=list(SHAPES))
def test_quantised_noise_all_options_and_rounds(ctx, api, shape):
    src = EC.quantised_noise(shape, 53)          # 8 levels, 0 .. 7: the thresholds sit exactly on a level
    most = 0
    for mname, mask in masks_for(shape, 54).items():
        for what, kw in crossed(4.0, 3.0):
            w, stats = check(ctx, api, src, mask, what="quantised %s %s" % (mname, what), **kw)
            rounds_within_bound(stats, src, mask, kw["halt_threshold"], kw["start_from_minima"], what)
            most = max(most, stats[1])
            if kw["halt_threshold"] is not None:
                assert (w[0][(mask != 0) if mask is not None else slice(None)] == -1).any()    # undefined voxels
    assert most >= 3


@pytest.mark.parametrize("shape", list(SHAPES.values()), ids=list(SHAPES))
def test_against_the_heapq_restatement(ctx, api, shape):
    """The independent statement itself as the reference: a selection of the options on every shape and volume kind."""
    mask = EC.random_mask(shape, 55)
    for name, src, thr in (("smooth", EC.smooth_noise(shape, 56), 0.5), ("quantised", EC.quantised_noise(shape, 57), 4.0)):
        for c, from_min, masked, show in ((3, True, True, True), (1, False, False, True), (2, True, False, False)):
            t = None if c == 1 else (thr if from_min else -thr)
            kw = dict(connectivity=c, start_from_minima=from_min, show_boundaries=show)
            want = watershed_np.watershed(src, mask if masked else None, None, INF if t is None else t, **kw)
            check(ctx, api, src, mask if masked else None, what="%s c%d vs heapq" % (name, c), reference=want,
                  halt_threshold=t, **kw)


@pytest.mark.parametrize("c", [1, 2, 3])
def test_cube_64(ctx, api, c):
    mask = EC.random_mask(CUBE, 58)
    q = EC.quantised_noise(CUBE, 59)
    for from_min in (True, False):
        check(ctx, api, EC.smooth_noise(CUBE, 60), None, connectivity=c, start_from_minima=from_min, what="64^3 smooth")
        thr = 4.0 if from_min else 3.0
        _, stats = check(ctx, api, q, mask, connectivity=c, start_from_minima=from_min, halt_threshold=thr,
                         what="64^3 quantised")
        rounds_within_bound(stats, q, mask, thr, from_min, "64^3 quantised")
    check(ctx, api, q, None, connectivity=c, show_boundaries=False, what="64^3 quantised hide")


@pytest.mark.parametrize("from_min", [True, False], ids=["min", "max"])
def test_binary_constant_and_tied_images(ctx, api, from_min):
    b = EC.binary_volume((30, 41, 52), 61)
    for c in (1, 3):
        w, stats = check(ctx, api, b, None, connectivity=c, start_from_minima=from_min, what="binary c%d" % c)
        rounds_within_bound(stats, b, None, None, from_min, "binary")
        assert len(w[1]) >= 1 and (w[0] > 0).sum() > b.size // 2
        w, stats = check(ctx, api, b, EC.random_mask(b.shape, 62), connectivity=c, start_from_minima=from_min,
                         halt_threshold=0.0 if from_min else 1.0, what="binary thr c%d" % c)
        rounds_within_bound(stats, b, EC.random_mask(b.shape, 62), 0.0 if from_min else 1.0, from_min, "binary thr")
    const = np.full((9, 20, 70), -1.25, np.float32)
    w, stats = check(ctx, api, const, None, start_from_minima=from_min, what="constant")
    assert len(w[1]) == 1 and (w[0] == 1).all() and stats[1] <= 6
    w, _ = check(ctx, api, const, None, start_from_minima=from_min, halt_threshold=-2.0 if from_min else -1.0,
                 label_undefined=-5, what="constant, nothing eligible")
    assert len(w[1]) == 0 and (w[0] == -5).all()
    ties = EC.tie_volume((17, 22, 39))
    for c in (1, 3):
        w, _ = check(ctx, api, ties, None, connectivity=c, start_from_minima=from_min, what="ties c%d" % c)
        assert len(w[1]) > 20        # equal scores: the seeds' order decides who wins a tie


@pytest.mark.parametrize("shape", [CUBE, (21, 30, 45)], ids=["64", "45x30x21"])
@pytest.mark.parametrize("from_min", [True, False], ids=["min", "max"])
def test_serpentine_plateau(ctx, api, shape, from_min):
    """A plateau of about nx*ny*nz/4 voxels, one voxel wide: sweeping through it voxel by voxel would take that many rounds;
    with the flaw (one voxel of 7 at the path's far end) the path is no maximum any more and floods from its end."""
    for flaw in (False, True):
        path = EC.serpentine(shape, flaw=flaw)
        assert int((path == 5).sum()) > path.size // 5
        for c in (1, 3):
            what = "serpentine%s c%d" % (" flawed" if flaw else "", c)
            w, stats = check(ctx, api, path, None, connectivity=c, start_from_minima=from_min, what=what)
            rounds_within_bound(stats, path, None, None, from_min, what)
            thr = 5.0 if from_min else 0.0
            _, stats = check(ctx, api, path, None, connectivity=c, start_from_minima=from_min, show_boundaries=False,
                             halt_threshold=thr, what=what + " hide")
            rounds_within_bound(stats, path, None, thr, from_min, what + " hide")


def test_long_monotone_ramps(ctx, api):
    """One chain of down pointers as long as the image, towards a minimum at either end: the worst case of the link
    compression (the serpentine is a plateau, not a ramp)."""
    n = 20000
    for shape in ((1, 1, n), (1, n, 1), (2, 5, n // 10)):
        ramp = np.arange(n, dtype=np.float32).reshape(shape)
        for src in (ramp, -ramp):
            for from_min in (True, False):
                w, stats = check(ctx, api, src, None, connectivity=1, start_from_minima=from_min, what="ramp %r" % (shape,))
                assert len(w[1]) == 1 and (w[0] == 1).all() and stats[1] <= 3


def test_special_values_and_nans(ctx, api):
    raw = EC.special_volume((18, 25, 31), 63)
    src = WC.no_nans(raw)
    assert np.isnan(raw).any() and np.isinf(src).any() and (np.signbit(src) & (src == 0)).any()
    mask = EC.random_mask(src.shape, 64)
    for c, masked, from_min in itertools.product((1, 2, 3), (False, True), (True, False)):
        for thr in (None, 0.0, -0.0, INF, -INF, 2.0, -2.0):
            check(ctx, api, src, mask if masked else None, connectivity=c, start_from_minima=from_min, halt_threshold=thr,
                  what="special c%d thr %r" % (c, thr))
    # an unmasked NaN: refused, and the labels are untouched
    L = api.load_library()
    lab = np.full(raw.shape, 77, np.int32)
    n = C.c_int64(-7)
    nz, ny, nx = raw.shape
    for m in (None, mask):
        rc = L.visfd_hip_watershed(ctx._h, raw.ctypes.data, None if m is None else m.ctypes.data, None, nx, ny, nz, INF, 1, 3, 1,
                                   0, -1, lab.ctypes.data, None, None, 0, C.byref(n))
        assert rc == 1 and "is NaN" in L.visfd_hip_last_error().decode() and (lab == 77).all()
    # with every NaN masked out the call goes through
    hide = np.where(np.isnan(raw), 0, 1).astype(np.float32)
    check(ctx, api, raw, hide, connectivity=3, what="NaNs masked out")


def test_host_option_gives_the_same_bytes(ctx, api):
    src = EC.quantised_noise(ODD, 65)
    mask = EC.random_mask(ODD, 66)
    kw = dict(halt_threshold=4.0, connectivity=2, label_boundary=-3, label_undefined=-9)
    dev = ctx.watershed(src, mask, **kw)
    assert ctx.watershed_last_stats()[0] == api.WATERSHED_PATH_DEVICE
    with ctx.options(watershed_host=1):
        host = ctx.watershed(src, mask, **kw)
        stats = ctx.watershed_last_stats()
        assert stats[0] == api.WATERSHED_PATH_HOST and stats[1:3] == (0, 0) and stats[3] == len(dev[1])
    same(dev, host, "option watershed_host")
    assert dev[0].tobytes() == host[0].tobytes()
    assert (dev[0][mask == 0] == -1).all() and (dev[0] == -9).any() and (dev[0] == -3).any()
    check(ctx, api, src, mask, what="back on the device", **kw)


def test_markers_through_both_faces(ctx, api):
    import torch
    src = EC.quantised_noise(ODD, 67)
    mask = EC.random_mask(ODD, 68)
    for name, masked, kw in (("several", False, dict(connectivity=1)),
                             ("repeated", True, dict(connectivity=3, halt_threshold=5.0)),
                             ("masked", True, dict(connectivity=2, start_from_minima=False, halt_threshold=2.0))):
        markers = WC.rounded_markers(WC.marker_volume(name, ODD, mask))
        m = mask if masked else None
        want = watershed_np.watershed(src, m, markers, kw.get("halt_threshold", INF),
                                      **{k: v for k, v in kw.items() if k != "halt_threshold"})
        got = ctx.watershed(src, m, markers, **kw)
        same(got, want, "markers %s, host face" % name)
        assert ctx.watershed_last_stats()[0] == api.WATERSHED_PATH_HOST
        lab = torch.full(ODD, -5, dtype=torch.int32, device="cuda")
        lists = ctx.watershed_dev(torch.from_numpy(src).cuda(), lab, None if m is None else torch.from_numpy(m).cuda(),
                                  torch.from_numpy(markers).cuda(), **kw)
        same((lab.cpu().numpy(),) + tuple(lists), want, "markers %s, device face" % name)


def test_device_face_and_context_state(ctx, api, oracle):
    import torch
    src = EC.quantised_noise(ODD, 69)
    mask = EC.random_mask(ODD, 70)
    kw = dict(halt_threshold=4.0, connectivity=2)
    want = api.watershed_host(src, mask, **kw)
    ds, dm = torch.from_numpy(src).cuda(), torch.from_numpy(mask).cuda()

    def dev_call():
        lab = torch.full(ODD, -5, dtype=torch.int32, device="cuda")
        lists = ctx.watershed_dev(ds, lab, dm, **kw)
        return (lab.cpu().numpy(),) + tuple(lists)

    got = dev_call()
    same(got, want, "device face")
    assert (got[0][mask == 0] == -1).all()         # written everywhere: voxels with mask == 0 hold -1
    same(dev_call(), want, "device face, second call")
    with ctx.options(morph_general=1, gauss_3pass=1, tv_fma=1, eig_f32=1):
        same(dev_call(), want, "under other stages' options")
    g, _ = ctx.gauss_ratio(src, (1.5, 1.5, 1.5), 2.5)
    assert_bits_equal(g, oracle.gauss_ratio(src, (1.5, 1.5, 1.5), 2.5)[0], "gauss in between")
    ctx.dilate_sphere(src, 2.0, mask=mask)
    ctx.find_extrema(src, mask)
    same(dev_call(), want, "after a Gaussian, a dilation and an extrema search")
    check(ctx, api, EC.smooth_noise(CUBE, 71), None, what="larger volume in between")   # grows the slots
    same(dev_call(), want, "after a larger volume")
    ctx.debug_poison_workspace()
    same(dev_call(), want, "after the workspace was poisoned")
    ctx.debug_poison_workspace()
    same(ctx.watershed(src, mask, show_boundaries=False, **kw), api.watershed_host(src, mask, show_boundaries=False, **kw),
         "host face after the workspace was poisoned")
    assert ds.cpu().numpy().tobytes() == src.tobytes() and dm.cpu().numpy().tobytes() == mask.tobytes()   # inputs untouched


def test_pending_blob_job_is_not_disturbed(ctx, api):
    import torch
    src = torch.from_numpy(volgen.blob_volume((40, 48, 56), 72)).cuda()
    sig = np.array([1.5, 1.9, 2.4, 3.0, 3.7], np.float32)
    want = ctx.blob_dog_dev(src, sig, None, None, 0.02, 2.5)
    q = EC.quantised_noise((40, 48, 56), 73)
    job = ctx.blob_dog_begin_dev(src, sig, None, None, 0.02, 2.5)
    assert ctx.blob_jobs_pending() == 1
    check(ctx, api, q, None, connectivity=3, what="with a blob job pending")
    lab = torch.empty(q.shape, dtype=torch.int32, device="cuda")
    lists = ctx.watershed_dev(torch.from_numpy(q).cuda(), lab, connectivity=3)
    got = ctx.blob_dog_end(job)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    same((lab.cpu().numpy(),) + tuple(lists), api.watershed_host(q, connectivity=3), "device face with a blob job pending")


def test_capacity_protocol(ctx, api):
    L = api.load_library()
    src = EC.smooth_noise(ODD, 74)
    want = api.watershed_host(src, connectivity=3)
    nb = len(want[1])
    assert nb > 50
    nz, ny, nx = src.shape

    def raw(cap, idx, sc, lab):
        n = C.c_int64(-7)
        rc = L.visfd_hip_watershed(ctx._h, src.ctypes.data, None, None, nx, ny, nz, INF, 1, 3, 1, 0, -1, lab.ctypes.data,
                                   None if idx is None else idx.ctypes.data, None if sc is None else sc.ctypes.data, cap,
                                   C.byref(n))
        return rc, n.value

    lab = np.full(src.shape, 77, np.int32)
    rc, n = raw(0, None, None, lab)                     # count only: labels written, no lists
    assert rc == 0 and n == nb
    assert_bits_equal(lab, want[0], "count-only labels")
    lab[:] = 77
    idx, sc = np.full(nb, -5, np.int64), np.full(nb, -5, np.float32)
    rc, n = raw(nb - 1, idx, sc, lab)
    assert rc == 4 and n == nb                          # VISFD_HIP_ECAPACITY with the needed count
    assert (lab == 77).all() and (idx == -5).all() and (sc == -5).all()   # nothing else written
    rc, n = raw(nb, idx, sc, lab)                       # the retry
    assert rc == 0 and n == nb
    same((lab, idx, sc), want, "retry")
    idx[:] = -5
    rc, n = raw(nb + 7, idx, None, lab)                 # one list only
    assert rc == 0 and np.array_equal(idx, want[1])


# ---- the C++ drop-in ---------------------------------------------------------------------------------------------------
def _read_records(path):
    out = {}
    data = open(str(path), "rb").read()
    pos = 0
    while pos < len(data):
        tag = data[pos:pos + 32].split(b"\0")[0].decode()
        n = struct.unpack_from("<q", data, pos + 32)[0]
        out[tag] = np.frombuffer(data, np.float64, n, pos + 40).copy()
        pos += 40 + 8 * n
    return out


def test_cpp_shim_watershed(api, tmp_path):
    exe = str(tmp_path / "shim_watershed_check")
    libdir = os.path.join(ROOT, "visfd_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "shim_watershed_check.cpp"), "-o", exe, "-L" + libdir, "-lvisfd_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    shape = (14, 19, 23)
    nz, ny, nx = shape
    src = EC.quantised_noise(shape, 75)
    mask = EC.random_mask(shape, 76)
    markers = WC.rounded_markers(WC.marker_volume("several", shape, mask))
    with open(str(tmp_path / "in.bin"), "wb") as f:
        f.write(struct.pack("<iii", nx, ny, nz))
        f.write(src.tobytes())
        f.write(mask.tobytes())
        f.write(markers.astype(np.float32).tobytes())
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "shim watershed check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    R = _read_records(tmp_path / "out.bin")

    def crds(index):
        return np.stack([index % nx, (index // nx) % ny, index // (nx * ny)], 1).astype(np.float64).reshape(-1)

    w = api.watershed_host(src)                                  # every default; the 9s are all overwritten
    assert R["default_n"][0] == len(w[1]) > 3 and np.array_equal(R["default_labels"].reshape(shape), w[0])
    w = api.watershed_host(src, mask, start_from_minima=False, connectivity=3)      # +inf from maxima: no threshold
    assert R["maxima_n"][0] == len(w[1]) > 3 and np.array_equal(R["maxima_labels"].reshape(shape), w[0])
    assert np.array_equal(R["maxima_crds"], crds(w[1])) and np.array_equal(R["maxima_scores"], w[2].astype(np.float64))
    for tag, show in (("hidden", False), ("shown", True)):
        w = api.watershed_host(src, mask, halt_threshold=3.0, connectivity=2, show_boundaries=show, label_boundary=-4,
                               label_undefined=-7)
        assert np.array_equal(R[tag + "_labels"].reshape(shape), w[0])
        assert (w[0] == -7).any() and (w[0] == -4).any() == show
    assert np.array_equal(R["hidden_crds"], crds(w[1]))
    w = api.watershed_host(src, mask, markers, halt_threshold=5.0, connectivity=1)
    seeds = len(np.unique(markers[(markers > 0) & (mask != 0)]))        # markers on voxels with mask == 0 seed nothing
    assert R["markers_n"][0] == len(w[1]) == seeds >= 3 and np.array_equal(R["markers_labels"].reshape(shape), w[0])
    assert np.array_equal(R["markers_crds"], crds(w[1])) and np.array_equal(R["markers_scores"], w[2].astype(np.float64))


# ---- filter_mrc against the reference program ------------------------------------------------------------------------
CLI = os.path.join(ROOT, "visfd_amd", "cli", "filter_mrc")
REF_CLI = os.path.join(ROOT, "oracle", "_ref", "filter_mrc_ref")
BLOB = os.path.join(GOLDEN, "test_blob_detect.rec")
BLOB_MASK = os.path.join(GOLDEN, "test_blob_detect_mask.rec")


@pytest.fixture(scope="module")
def ref_cli():
    if not os.path.exists(REF_CLI):
        pytest.skip("oracle/_ref/filter_mrc_ref not built (needs the reference sources at build time)")
    return REF_CLI


def both_programs(ref_cli, tmp_path, args, out="out.rec"):
    """Runs both programs with the same flags in directories of their own; -> their output images, which must be equal."""
    res = []
    for tag, exe in (("mine", CLI), ("ref", ref_cli)):
        d = tmp_path / tag
        d.mkdir(exist_ok=True)
        r = subprocess.run([exe] + [str(a) for a in args] + ["-out", out], cwd=str(d), capture_output=True, text=True)
        assert r.returncode == 0, (tag, r.stderr[-2000:])
        res.append((d / out).read_bytes())
    assert res[0] == res[1], " ".join(map(str, args))
    return volgen.read_mrc(str(tmp_path / "mine" / out))


def cli_cases(mask, t_min, t_max, markers):
    return [
        ["-watershed", "minima"],
        ["-watershed", "maxima"],
        ["-watershed", "min", "-neighbor-connectivity", 1, "-mask", mask],
        ["-watershed", "max", "-neighbor-connectivity", 2, "-mask", mask, "-mask-out", 3],
        ["-watershed", "minima", "-watershed-threshold", t_min, "-neighbor-connectivity", 1],
        ["-watershed-threshold", t_max, "-watershed", "maxima", "-mask", mask],       # the threshold survives -watershed
        ["-watershed", "maxima", "-watershed-threshold", t_max, "-watershed-hide-boundaries", "-undefined-out", 7],
        ["-watershed", "minima", "-watershed-threshold", t_min, "-watershed-boundary", 5, "-undefined-out", "max"],
        ["-watershed-hide-boundaries", "-neighbor-connectivity", 2],                   # minima by default
        ["-watershed", "minima", "-markers", markers, "-mask", mask, "-neighbor-connectivity", 1],
        ["-watershed", "maxima", "-markers", markers, "-watershed-threshold", t_max],
    ]


@pytest.fixture(scope="module")
def blob_markers(tmp_path_factory):
    v = volgen.read_mrc(BLOB)
    m = WC.marker_volume("several", v.shape, volgen.read_mrc(BLOB_MASK))
    path = str(tmp_path_factory.mktemp("markers") / "markers.rec")
    volgen.write_mrc(path, m, voxel_width=1.0)
    return path


@pytest.mark.parametrize("k", range(11))
def test_cli_watershed_equals_reference_program_blob_file(ref_cli, tmp_path, blob_markers, k):
    v = volgen.read_mrc(BLOB)
    t_min, t_max = float(np.quantile(v, 0.7)), float(np.quantile(v, 0.3))
    out = both_programs(ref_cli, tmp_path, ["-in", BLOB] + cli_cases(BLOB_MASK, t_min, t_max, blob_markers)[k])
    assert len(np.unique(out)) >= 3     # the marked cases hold few basins: a basin, undefined or boundary, and the mask


@pytest.fixture(scope="module")
def volumes_128(tmp_path_factory):
    d = tmp_path_factory.mktemp("v128")
    shape = (128, 128, 128)
    volgen.write_mrc(str(d / "q.rec"), EC.quantised_noise(shape, 77, passes=3), voxel_width=1.0)
    volgen.write_mrc(str(d / "s.rec"), EC.smooth_noise(shape, 78, passes=3), voxel_width=1.0)
    volgen.write_mrc(str(d / "m.rec"), EC.random_mask(shape, 79, keep=0.9), voxel_width=1.0)
    return str(d / "q.rec"), str(d / "s.rec"), str(d / "m.rec")


@pytest.mark.parametrize("k", range(4))
def test_cli_watershed_equals_reference_program_128(ref_cli, tmp_path, volumes_128, k):
    q, s, m = volumes_128
    flags = [["-in", q, "-watershed", "minima", "-watershed-threshold", 4, "-mask", m],
             ["-in", q, "-watershed", "maxima", "-neighbor-connectivity", 1, "-watershed-hide-boundaries"],
             ["-in", s, "-watershed", "minima", "-neighbor-connectivity", 2],
             ["-in", s, "-watershed", "maxima", "-watershed-threshold", 0.5, "-mask", m]][k]
    out = both_programs(ref_cli, tmp_path, ["-w", 1] + flags)
    assert out.max() > 20


def test_cli_scenario_of_the_reference_test_script(ref_cli, tmp_path):
    """tests/test_watershed.sh of the reference on this repository's fixtures: the blurred image segmented from its minima,
    its negative from its maxima; the two segmentations find the same number of basins, which is the largest label of the
    image."""
    base = ["-w", 19.2, "-mask", BLOB_MASK]
    (tmp_path / "ref").mkdir()
    for args in (["-in", BLOB, "-out", "gauss.rec", "-gauss", 120], ["-in", "gauss.rec", "-out", "inv.rec", "-invert"]):
        r = subprocess.run([ref_cli] + [str(a) for a in base + args], cwd=str(tmp_path / "ref"), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]     # the two inputs, made by the reference program (-invert is its own)
    gauss, inv = str(tmp_path / "ref" / "gauss.rec"), str(tmp_path / "ref" / "inv.rec")
    a = both_programs(ref_cli, tmp_path, base + ["-in", gauss, "-watershed", "minima"], out="ws_min.rec")
    b = both_programs(ref_cli, tmp_path, base + ["-in", inv, "-watershed", "maxima"], out="ws_max.rec")
    r = subprocess.run([CLI] + [str(x) for x in base + ["-in", gauss, "-watershed", "minima"]], cwd=str(tmp_path / "mine"),
                       capture_output=True, text=True)
    n = int(r.stderr.split("Number of basins found: ")[1].split()[0])
    mask = volgen.read_mrc(BLOB_MASK)
    assert n > 0 and a[mask != 0].max() == n and b[mask != 0].max() == n
