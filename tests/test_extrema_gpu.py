"""Local minima and maxima on the GPU (csrc/extrema.hip) against the numpy restatement (tests/extrema_np.py, which
tests/test_extrema.py holds to the reference program's recorded output), through the C ABI; the C++ drop-in; and
filter_mrc's flags against the reference program itself.  Every comparison is exact: lists element for element with
scores as bit patterns, label images voxel for voxel, text files byte for byte."""
import ctypes as C
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

import extrema_cases as EC
import extrema_np
import volgen
from conftest import GOLDEN, ROOT, assert_bits_equal

pytestmark = pytest.mark.gpu

INF = float("inf")
ODD = (23, 50, 37)       # nz, ny, nx: odd, unequal, no multiple of a tile
CUBE = (64, 64, 64)
KINDS = [("min", True, False), ("max", False, True), ("both", True, True)]


@pytest.fixture(scope="module")
def ctx():
    from visfd_amd import api
    c = api.Context(0)
    yield c
    c.close()


def same_lists(got, want, what):
    for k, name in enumerate(("index", "score", "nvoxels")):
        assert got[k].shape == want[k].shape, (what, name, got[k].shape, want[k].shape)
        assert_bits_equal(got[k], want[k], "%s %s" % (what, name))


def check(ctx, src, mask=None, labels0=None, what="", **kw):
    """One call through the host face, lists and label image, against the restatement; returns the restatement's result."""
    want = extrema_np.find_extrema(src, mask, labels=labels0, **kw)
    mins, maxs, lab = ctx.find_extrema(src, mask, want_labels=True, labels=labels0, **kw)
    same_lists(mins, want["min"], what + " minima")
    same_lists(maxs, want["max"], what + " maxima")
    assert_bits_equal(lab, want["labels"], what + " labels")
    return want


def crossed(thresholds):
    for (kind, fmin, fmax), c, masked, borders, thr in itertools.product(KINDS, (1, 2, 3), (False, True), (True, False),
                                                                         (False, True)):
        lo, hi = thresholds if thr else (INF, -INF)
        yield ("%s c%d %s %s %s" % (kind, c, "mask" if masked else "nomask", "borders" if borders else "noborders",
                                    "thr" if thr else "nothr"), masked,
               dict(find_minima=fmin, find_maxima=fmax, minima_threshold=lo, maxima_threshold=hi, connectivity=c,
                    allow_borders=borders))


@pytest.mark.parametrize("shape", [ODD, (40, 33, 1)], ids=["37x50x23", "nx1"])
def test_smooth_noise_all_options(ctx, shape):
    src = EC.smooth_noise(shape, 21)
    mask = EC.random_mask(shape, 22)
    listed = 0
    for what, masked, kw in crossed((-0.6, 0.6)):
        w = check(ctx, src, mask if masked else None, what=what, **kw)
        listed += len(w["min"][0]) + len(w["max"][0])
    assert listed > 1000


@pytest.mark.parametrize("shape", [ODD, (40, 33, 1)], ids=["37x50x23", "nx1"])
def test_quantised_noise_all_options(ctx, shape):
    src = EC.quantised_noise(shape, 23)
    mask = EC.random_mask(shape, 24)
    big = 0
    for what, masked, kw in crossed((1.0, 5.0)):
        w = check(ctx, src, mask if masked else None, what=what, **kw)
        big = max([big] + list(w["min"][2]) + list(w["max"][2]))
    assert big > (20 if shape == ODD else 3)     # plateaus of many voxels among the extrema


@pytest.mark.parametrize("c", [1, 2, 3])
def test_cube_64(ctx, c):
    for src in (EC.smooth_noise(CUBE, 25), EC.quantised_noise(CUBE, 26)):
        check(ctx, src, None, connectivity=c, what="64^3 c%d" % c)
        check(ctx, src, EC.random_mask(CUBE, 27), connectivity=c, allow_borders=False, what="64^3 mask c%d" % c)


@pytest.mark.parametrize("kind,fmin,fmax", KINDS)
def test_binary_and_constant_images(ctx, kind, fmin, fmax):
    b = EC.binary_volume((30, 41, 52), 28)
    for c in (1, 3):
        w = check(ctx, b, None, find_minima=fmin, find_maxima=fmax, connectivity=c, what="binary " + kind)
        assert max(list(w["min"][2]) + list(w["max"][2])) > b.size // 8     # plateaus that span the volume
    const = np.full((9, 20, 70), -1.25, np.float32)
    w = check(ctx, const, None, find_minima=fmin, find_maxima=fmax, what="constant " + kind)
    # one plateau, both a minimum and a maximum: the label rule puts the maximum first
    assert [len(w["min"][0]), len(w["max"][0])] == [int(fmin), int(fmax)]
    assert (w["labels"] == (1 if fmax else 0)).all()
    w = check(ctx, const, None, find_minima=fmin, find_maxima=fmax, allow_borders=False, what="constant noborders " + kind)
    assert len(w["min"][0]) + len(w["max"][0]) == 0 and not w["labels"].any()


@pytest.mark.parametrize("shape", [CUBE, (21, 30, 45)], ids=["64", "45x30x21"])
def test_serpentine_plateau(ctx, shape):
    """One plateau of about nx*ny*nz/4 voxels, one voxel wide: a maximum -- and no maximum once a single voxel at its far
    end touches a higher value, which every member of the plateau has to learn."""
    path = EC.serpentine(shape)
    npath = int((path == 5).sum())
    assert npath > path.size // 5
    for c in (1, 3):
        w = check(ctx, path, None, connectivity=c, what="serpentine c%d" % c)
        if c == 1:
            assert list(w["max"][2]) == [npath] and list(w["max"][0]) == [0]
        w = check(ctx, EC.serpentine(shape, flaw=True), None, connectivity=c, what="flawed serpentine c%d" % c)
        if c == 1:
            assert list(w["max"][2]) == [1] and w["max"][1][0] == 7     # only the flaw itself is a maximum
            assert not (w["labels"][path == 5]).any()


@pytest.mark.parametrize("borders", [True, False])
def test_walled_in_voxels(ctx, borders):
    src, mask = EC.walled_volume((20, 27, 34), 29)
    labels0 = np.full(src.shape, -77, np.int32)      # voxels with mask == 0 keep what the label image held
    for kind, fmin, fmax in KINDS:
        w = check(ctx, src, mask, labels0, find_minima=fmin, find_maxima=fmax, allow_borders=borders, what="walled " + kind)
        assert (w["labels"][mask == 0] == -77).all()
    # a walled-in voxel is a minimum and a maximum when borders are allowed, nothing when they are not
    w = extrema_np.find_extrema(src, mask, allow_borders=borders)
    both = set(w["min"][0]) & set(w["max"][0])
    assert (len(both) >= 4) if borders else (len(both) == 0)


def test_special_values(ctx):
    src = EC.special_volume((18, 25, 31), 30)
    assert np.isnan(src).any() and np.isinf(src).any() and (np.signbit(src) & (src == 0)).any()
    mask = EC.random_mask(src.shape, 31)
    for c, masked, borders in itertools.product((1, 2, 3), (False, True), (True, False)):
        # thresholds exactly on extremal values: 0 (the +-0 plateaus), +-inf, the outer levels
        for lo, hi in ((INF, -INF), (0.0, 0.0), (-0.0, -0.0), (-INF, INF), (-2.0, 2.0), (float("nan"), float("nan"))):
            check(ctx, src, mask if masked else None, connectivity=c, allow_borders=borders, minima_threshold=lo,
                  maxima_threshold=hi, what="special c%d thr %r %r" % (c, lo, hi))


def test_labels_under_failing_thresholds(ctx):
    """A maximum that fails its threshold carries the label of the listed maximum before it in raster order (0 if there
    is none); when only minima are sought, a plateau that is also a maximum gets 0."""
    src = EC.quantised_noise(ODD, 32)
    w = check(ctx, src, None, minima_threshold=1.0, maxima_threshold=6.0, what="failing thresholds")
    free = extrema_np.find_extrema(src)
    assert 0 < len(w["max"][0]) < len(free["max"][0])
    failed = sorted(set(free["max"][0]) - set(w["max"][0]))
    lab = w["labels"].reshape(-1)
    assert any(lab[i] > 0 for i in failed) and any(lab[i] == 0 for i in failed)
    for kind, fmin, fmax in KINDS:
        check(ctx, src, EC.random_mask(ODD, 33), find_minima=fmin, find_maxima=fmax, minima_threshold=2.0,
              maxima_threshold=5.0, allow_borders=False, what="failing thresholds " + kind)
    walled, mask = EC.walled_volume((12, 13, 14), 34)
    w = check(ctx, walled, mask, find_maxima=False, what="minima only, walled")
    both = set(extrema_np.find_extrema(walled, mask)["max"][0]) & set(w["min"][0])
    assert both and all(w["labels"].reshape(-1)[i] == 0 for i in both)


def test_tie_ordering(ctx):
    src = EC.tie_volume((17, 22, 39))
    for kind, fmin, fmax in KINDS:
        w = check(ctx, src, None, find_minima=fmin, find_maxima=fmax, what="ties " + kind)
        if fmin:
            pits = w["min"][0][w["min"][1] == -3]
            assert len(pits) > 20 and (np.diff(pits) > 0).all()          # equal scores: earlier root first
        if fmax:
            peaks = w["max"][0][w["max"][1] == 3]
            assert len(peaks) > 20 and (np.diff(peaks) < 0).all()        # the reverse for maxima: later root first


def _raw(ctx, name, src_ptr, shape, caps, labels=None, find=(1, 1)):
    from visfd_amd import api
    L = api.load_library()
    nz, ny, nx = shape
    lists = [(np.zeros(max(c, 1), np.int64), np.zeros(max(c, 1), np.float32), np.zeros(max(c, 1), np.int64)) for c in caps]
    n = [C.c_int64(-1), C.c_int64(-1)]
    tail = []
    for k in range(2):
        tail += [a.ctypes.data if caps[k] else None for a in lists[k]] + [caps[k], C.byref(n[k])]
    rc = getattr(L, name)(ctx._h, src_ptr, None, nx, ny, nz, find[0], find[1], INF, -INF, 3, 1, *(tail + [labels]))
    return rc, [int(x.value) for x in n], lists


def test_capacity_protocol(ctx):
    src = EC.smooth_noise(ODD, 35)
    want = extrema_np.find_extrema(src)
    counts = [len(want["min"][0]), len(want["max"][0])]
    assert min(counts) > 50
    rc, n, _ = _raw(ctx, "visfd_hip_find_extrema", src.ctypes.data, src.shape, (0, 0))       # count only
    assert rc == 0 and n == counts
    lab = np.full(src.shape, 123456, np.int32)
    rc, n, lists = _raw(ctx, "visfd_hip_find_extrema", src.ctypes.data, src.shape, (counts[0], counts[1] - 1), lab.ctypes.data)
    assert rc == 4 and n == counts                       # VISFD_HIP_ECAPACITY with the needed counts
    assert (lab == 123456).all() and not lists[0][0].any() and not lists[1][0].any()   # nothing else written
    rc, n, lists = _raw(ctx, "visfd_hip_find_extrema", src.ctypes.data, src.shape, (n[0], n[1] + 5), lab.ctypes.data)
    assert rc == 0 and n == counts                       # the retry
    same_lists([a[:n[0]] for a in lists[0]], want["min"], "retry minima")
    same_lists([a[:n[1]] for a in lists[1]], want["max"], "retry maxima")
    assert_bits_equal(lab, want["labels"], "retry labels")
    rc, n, lists = _raw(ctx, "visfd_hip_find_extrema", src.ctypes.data, src.shape, (0, counts[1]))   # one list only
    assert rc == 0 and n == counts
    same_lists([a[:n[1]] for a in lists[1]], want["max"], "maxima alone")
    rc, n, _ = _raw(ctx, "visfd_hip_find_extrema", src.ctypes.data, src.shape, (0, 0), find=(0, 1))
    assert rc == 0 and n == [0, counts[1]]


def test_device_face_and_context_state(ctx, oracle):
    import torch
    src = EC.quantised_noise(ODD, 36)
    mask = EC.random_mask(ODD, 37)
    kw = dict(minima_threshold=2.0, maxima_threshold=4.0, connectivity=2, allow_borders=False)
    want = extrema_np.find_extrema(src, mask, **kw)
    host = ctx.find_extrema(src, mask, want_labels=True, **kw)
    ds, dm = torch.from_numpy(src).cuda(), torch.from_numpy(mask).cuda()

    def dev_call():
        lab = torch.full(ODD, -5, dtype=torch.int32, device="cuda")
        mins, maxs = ctx.find_extrema_dev(ds, dm, labels=lab, **kw)
        return mins, maxs, lab.cpu().numpy()

    def same(got, what):
        same_lists(got[0], want["min"], what + " minima")
        same_lists(got[1], want["max"], what + " maxima")
        lab = got[2].copy()
        assert (lab[mask == 0] == -5).all()        # the device face leaves masked voxels alone too
        lab[mask == 0] = 0
        assert_bits_equal(lab, want["labels"], what + " labels")

    same_lists(host[0], want["min"], "host minima")
    assert_bits_equal(host[2], want["labels"], "host labels")
    same(dev_call(), "device face")
    same(dev_call(), "device face, second call")
    # other stages' options do not reach this one, and other stages in between leave nothing behind
    with ctx.options(morph_general=1, gauss_3pass=1, tv_fma=1, eig_f32=1):
        same(dev_call(), "under other stages' options")
    g, _ = ctx.gauss_ratio(src, (1.5, 1.5, 1.5), 2.5)
    assert_bits_equal(g, oracle.gauss_ratio(src, (1.5, 1.5, 1.5), 2.5)[0], "gauss in between")
    ctx.dilate_sphere(src, 2.0, mask=mask)
    same(dev_call(), "after a Gaussian and a dilation")
    big = EC.smooth_noise(CUBE, 38)                 # a larger volume grows the slots, a smaller one reuses them
    check(ctx, big, None, what="larger volume in between")
    same(dev_call(), "after a larger volume")
    ctx.debug_poison_workspace()
    same(dev_call(), "after the workspace was poisoned")
    assert ds.cpu().numpy().tobytes() == src.tobytes() and dm.cpu().numpy().tobytes() == mask.tobytes()   # inputs untouched


def test_pending_blob_job_is_not_disturbed(ctx):
    import torch
    src = torch.from_numpy(volgen.blob_volume((40, 48, 56), 39)).cuda()
    sig = np.array([1.5, 1.9, 2.4, 3.0, 3.7], np.float32)
    want = ctx.blob_dog_dev(src, sig, None, None, 0.02, 2.5)
    q = EC.quantised_noise((40, 48, 56), 40)
    job = ctx.blob_dog_begin_dev(src, sig, None, None, 0.02, 2.5)
    assert ctx.blob_jobs_pending() == 1
    check(ctx, q, None, what="with a blob job pending")
    mins, maxs = ctx.find_extrema_dev(torch.from_numpy(q).cuda())
    got = ctx.blob_dog_end(job)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    same_lists(mins, extrema_np.find_extrema(q)["min"], "device face with a blob job pending")


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


def test_cpp_shim_extrema(tmp_path):
    exe = str(tmp_path / "shim_extrema_check")
    libdir = os.path.join(ROOT, "visfd_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "shim_extrema_check.cpp"), "-o", exe, "-L" + libdir, "-lvisfd_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    shape = (14, 19, 23)
    nz, ny, nx = shape
    src = EC.quantised_noise(shape, 41)
    mask = EC.random_mask(shape, 42)
    with open(str(tmp_path / "in.bin"), "wb") as f:
        f.write(struct.pack("<iii", nx, ny, nz))
        f.write(src.tobytes())
        f.write(mask.tobytes())
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "shim extrema check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    R = _read_records(tmp_path / "out.bin")

    def crds(index):
        return np.stack([index % nx, (index // nx) % ny, index // (nx * ny)], 1).astype(np.float64).reshape(-1)

    w = extrema_np.find_minima(src, mask, labels=np.full(shape, 9, np.int32))
    assert np.array_equal(R["minima_crds"], crds(w["min"][0]))
    assert np.array_equal(R["minima_scores"], w["min"][1].astype(np.float64))
    assert np.array_equal(R["minima_nvoxels"], w["min"][2]) and len(w["min"][0]) > 5
    assert np.array_equal(R["minima_labels"].reshape(shape), w["labels"])
    w = extrema_np.find_maxima(src, None, connectivity=1, allow_borders=False)
    assert np.array_equal(R["maxima_crds"], crds(w["max"][0])) and len(w["max"][0]) > 5
    assert np.array_equal(R["maxima_scores"], w["max"][1].astype(np.float64))
    assert np.array_equal(R["maxima_nvoxels"], w["max"][2])
    assert np.array_equal(R["maxima_labels"].reshape(shape), w["labels"])
    w = extrema_np.find_extrema(src, mask, True, True, 1.0, 5.0, 2, True)
    for side in ("min", "max"):
        assert np.array_equal(R["both_%s_index" % side], w[side][0]) and len(w[side][0]) > 0
        assert np.array_equal(R["both_%s_scores" % side], w[side][1].astype(np.float64))
        assert np.array_equal(R["both_%s_nvoxels" % side], w[side][2])
    assert np.array_equal(R["both_labels"].reshape(shape), w["labels"])
    w = extrema_np.find_extrema(src, mask, False, True, INF, 4.0, 3, True)
    assert np.array_equal(R["maxonly_crds"], crds(w["max"][0])) and len(w["max"][0]) > 0
    assert np.array_equal(R["maxonly_scores"], w["max"][1].astype(np.float64))
    assert np.array_equal(R["maxonly_nvoxels"], w["max"][2])


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


@pytest.fixture(scope="module")
def quantised_256(tmp_path_factory):
    """A 256^3 quantised volume and a mask for it, as MRC files."""
    d = tmp_path_factory.mktemp("q256")
    shape = (256, 256, 256)
    volgen.write_mrc(str(d / "q.rec"), EC.quantised_noise(shape, 43, passes=3), voxel_width=1.0)
    volgen.write_mrc(str(d / "m.rec"), EC.random_mask(shape, 44, keep=0.9), voxel_width=1.0)
    return str(d / "q.rec"), str(d / "m.rec")


def cli_cases(mask, lo, hi):
    return [
        ["-find-minima", "min.txt"],
        ["-find-maxima", "max.txt"],
        ["-find-minima", "min.txt", "-find-maxima", "max.txt"],
        ["-find-minima", "min.txt", "-find-maxima", "max.txt", "-mask", mask],
        ["-find-minima", "min.txt", "-find-maxima", "max.txt", "-neighbor-connectivity", 1],
        ["-find-maxima", "max.txt", "-neighbor-connectivity", 2, "-mask", mask, "-mask-out", 7],
        ["-find-minima", "min.txt", "-find-maxima", "max.txt", "-ignore-boundary-extrema"],
        ["-find-minima", "min.txt", "-ignore-boundary-extrema", "-mask", mask, "-neighbor-connectivity", 1],
        ["-find-minima", "min.txt", "-find-maxima", "max.txt", "-minima-threshold", lo, "-maxima-threshold", hi],
        ["-find-maxima", "max.txt", "-maxima-threshold", hi, "-boundary-extrema", "-mask", mask],
    ]


def both_programs(ref_cli, tmp_path, args):
    res = []
    for tag, exe in (("mine", CLI), ("ref", ref_cli)):
        d = tmp_path / tag
        d.mkdir(exist_ok=True)
        r = subprocess.run([exe] + [str(a) for a in args] + ["-out", "out.rec"], cwd=str(d), capture_output=True, text=True)
        assert r.returncode == 0, (tag, r.stderr[-2000:])
        res.append(d)
    mine, ref = res
    listed = 0
    for f in ("min.txt", "max.txt"):
        a, b = mine / f, ref / f
        assert a.exists() == b.exists(), f                       # no file for an empty list, in both programs
        if b.exists():
            assert a.read_bytes() == b.read_bytes(), f
            listed += b.read_bytes().count(b"\n")
    assert_bits_equal(volgen.read_mrc(str(mine / "out.rec")), volgen.read_mrc(str(ref / "out.rec")), " ".join(map(str, args)))
    return listed


@pytest.mark.parametrize("k", range(10))
def test_cli_extrema_equals_reference_program_blob_file(ref_cli, tmp_path, k):
    v = volgen.read_mrc(BLOB)
    lo, hi = float(np.quantile(v, 0.2)), float(np.quantile(v, 0.8))
    flags = cli_cases(BLOB_MASK, lo, hi)[k]
    assert both_programs(ref_cli, tmp_path, ["-in", BLOB] + flags) > 0
    if k == 2:   # the voxel width scales the coordinates in the text files
        both_programs(ref_cli, tmp_path, ["-in", BLOB, "-w", 19.6] + flags)


@pytest.mark.parametrize("k", range(10))
def test_cli_extrema_equals_reference_program_256(ref_cli, tmp_path, quantised_256, k):
    vol, mask = quantised_256
    flags = cli_cases(mask, 1, 6)[k]
    assert both_programs(ref_cli, tmp_path, ["-in", vol, "-w", 1] + flags) > 0
