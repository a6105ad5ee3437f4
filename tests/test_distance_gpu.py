"""The exact distance maps on the GPU (csrc/distance.hip): distance_sq, distance_to_points and distance_from_points bit for
bit against the numpy restatement (tests/distance_np.py) on both paths -- the separable transform and the brute-force walks
-- through the ctypes ABI and the torch device face, the argument errors, and filter_mrc's -distance-points and
-distance-to-voxels against what the reference program wrote (tests/golden/distance.npz)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import distance_cases as dc
import distance_np as dn
import volgen
from conftest import ROOT, assert_bits_equal, golden

pytestmark = pytest.mark.gpu

F = np.float32
CLI = os.path.join(ROOT, "visfd_amd", "cli", "filter_mrc")
POISON = 0xdeadbeef   # what dst holds before a call: it must survive exactly where mask == 0

# one voxel and single lines, one past a wave of 64 on each axis, several waves and workgroups
SHAPES = [(1, 1, 1), (1, 1, 130), (1, 130, 1), (130, 1, 1), (3, 5, 65), (3, 65, 5), (65, 3, 5), (20, 23, 70)]
LONG = [(1, 1, 4200), (1, 4200, 1), (4200, 1, 1)]   # dsq reaches 4199^2 > 2^24: (float)dsq rounds


@pytest.fixture(scope="module")
def ctx():
    from visfd_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def api():
    from visfd_amd import api
    return api


def both_paths(ctx, api, run, want, what):
    """`run()` on the transform and on the brute-force walks: the path that ran and the restatement's bits"""
    for general in (0, 1):
        with ctx.options(distance_general=general):
            got = run()
            path = ctx.distance_last_path()
        assert path == (api.DISTANCE_PATH_GENERAL if general else api.DISTANCE_PATH_TRANSFORM), (what, general)
        assert_bits_equal(np.asarray(got), want, "%s general=%d" % (what, general))


def seed_sets(shape):
    """name -> keyword arguments of distance_sq (src, mask, lo, hi, points)"""
    nz, ny, nx = shape
    rng = np.random.default_rng(sum(shape))
    zeros = np.zeros(shape, F)
    corner = zeros.copy()
    corner[0, 0, 0] = 1
    faces = zeros.copy()   # the two opposite faces of the longest axis: long parabolas in between
    ax = int(np.argmax(shape))
    faces[tuple(slice(None) if a != ax else 0 for a in range(3))] = 1
    faces[tuple(slice(None) if a != ax else -1 for a in range(3))] = 1
    pair = zeros.copy()    # two seeds equidistant from the voxels between them (the line's middle for an odd distance)
    lo_idx, hi_idx = [0, 0, 0], [0, 0, 0]
    hi_idx[ax] = shape[ax] - 1 - (shape[ax] % 2)   # an even distance apart: the middle voxel is tied exactly
    pair[tuple(lo_idx)] = 1
    pair[tuple(hi_idx)] = 1
    sparse = (rng.random(shape) < 0.002).astype(F)
    dense = (rng.random(shape) < 0.3).astype(F)
    values = rng.integers(0, 10, shape).astype(F)
    values.reshape(-1)[::7] = np.nan
    mask = (rng.random(shape) < 0.7).astype(F)
    z, y, x = np.nonzero(dense)
    listed = np.stack([x, y, z], 1)
    z, y, x = np.nonzero(sparse)
    few = np.stack([x, y, z], 1)
    near, far = [[-3, 40, 2]], [[10 ** 6, 0, 0], [0, -(10 ** 9), 5]]
    sel = dict(lo=0.5, hi=1.5)
    return {
        "none": dict(),
        "none_image": dict(src=zeros, **sel),
        "corner": dict(src=corner, **sel),
        "every": dict(src=zeros + 1, **sel),
        "faces": dict(src=faces, **sel),
        "pair": dict(src=pair, **sel),
        "sparse": dict(src=sparse, **sel),
        "dense": dict(src=dense, **sel),
        "interval_mask": dict(src=values, mask=mask, lo=3.0, hi=6.0),
        "listed": dict(points=listed),
        "listed_few": dict(points=few),
        "both": dict(src=values, mask=mask, lo=8.5, hi=20.0, points=few),
        "outside_near": dict(points=near),
        "outside_far": dict(points=far),
        "outside_all": dict(src=sparse, points=near + far + [[nx, ny, nz], [-1, -1, -1], [nx // 2, -2, nz + 3]], **sel),
        "outside_many": dict(points=np.stack([np.arange(300) - 150, np.full(300, -1), np.arange(300) % 7], 1)),
    }


@functools.lru_cache(maxsize=None)
def wanted(shape, name):
    """the restatement, computed once per shape and seed set (its separable form: tests/test_distance.py holds it equal to
    the brute-force formula, which takes too long on the larger shapes)"""
    return dn.distance_sq_separable(shape, **seed_sets(shape)[name])


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_distance_sq_matches_restatement_on_both_paths(ctx, api, shape):
    for name, kw in seed_sets(shape).items():
        want = wanted(shape, name)
        assert want.dtype == np.int32
        both_paths(ctx, api, lambda: ctx.distance_sq(shape, **kw), want, "%s %s" % (shape, name))
    assert (wanted(shape, "none") == dn.cap_of(shape)).all() and (wanted(shape, "outside_far") == dn.cap_of(shape)).all()


@pytest.mark.parametrize("shape", LONG, ids=str)
def test_exact_beyond_two_to_the_24(ctx, api, shape):
    """one seed at the origin of a line of 4200 voxels: dsq = i^2 up to 4199^2 > 2^24, where (float)dsq rounds (4097^2)"""
    n = max(shape)
    sq = (np.arange(n, dtype=np.int64) ** 2).astype(np.int32).reshape(shape)
    assert sq.max() > 2 ** 24 and int(F(4097 ** 2)) != 4097 ** 2
    both_paths(ctx, api, lambda: ctx.distance_sq(shape, points=[[0, 0, 0]]), sq, "dsq %s" % (shape,))
    src = np.zeros(shape, F)
    src.reshape(-1)[0] = 1
    both_paths(ctx, api, lambda: ctx.distance_sq(src=src, lo=1.0, hi=1.0), sq, "dsq from an image %s" % (shape,))
    for w in (1.0, 1.3):
        want = np.sqrt(sq.astype(F) * (F(w) * F(w)))
        assert want.dtype == F
        both_paths(ctx, api, lambda: ctx.distance_to_points(np.zeros(shape, F), [[0, 0, 0]], w), want, "float %s w=%g" % (shape, w))


@pytest.mark.parametrize("shape", [(3, 5, 65), (20, 23, 70)], ids=str)
@pytest.mark.parametrize("face", ["numpy", "torch"])
def test_distance_to_points_keeps_dst_where_mask_is_zero(ctx, api, shape, face):
    rng = np.random.default_rng(5)
    mask = (rng.random(shape) < 0.6).astype(F)
    pts = [[2, 1, 0], [-3, 40, 2], [shape[2] - 1, shape[1] - 1, shape[0] - 1], [10 ** 6, 0, 0]]
    w = 1.3
    poisoned = np.full(shape, POISON, np.uint32).view(F)
    want = dn.distance_to_points(poisoned, pts, w, mask)
    want_nomask = dn.distance_to_points(poisoned, pts, w, None)

    def run(m):
        if face == "numpy":
            return ctx.distance_to_points(poisoned, pts, w, mask=m)
        import torch
        dst = torch.from_numpy(poisoned.copy()).cuda()
        dm = None if m is None else torch.from_numpy(m).cuda()
        out = ctx.distance_to_points(dst, pts, w, mask=dm)
        ctx.synchronize()
        assert out is dst
        return dst.cpu().numpy()

    both_paths(ctx, api, lambda: run(mask), want, "masked %s" % face)
    got = run(mask)
    assert np.all(got.view(np.uint32)[mask == 0] == POISON) and not np.any(got.view(np.uint32)[mask != 0] == POISON)
    both_paths(ctx, api, lambda: run(None), want_nomask, "unmasked %s" % face)


def test_distance_sq_on_device_tensors(ctx, api):
    import torch
    shape = (20, 23, 70)
    kw = seed_sets(shape)["both"]
    dev = dict(kw, src=torch.from_numpy(kw["src"]).cuda(), mask=torch.from_numpy(kw["mask"]).cuda())

    def run():
        out = ctx.distance_sq(**dev)
        ctx.synchronize()
        assert out.dtype == torch.int32 and out.is_cuda
        return out.cpu().numpy()

    both_paths(ctx, api, run, wanted(shape, "both"), "device tensors")


@pytest.mark.parametrize("shape", [(3, 5, 65), (20, 23, 70)], ids=str)
def test_distance_from_points(ctx, api, shape):
    nz, ny, nx = shape
    rng = np.random.default_rng(17)
    src = rng.integers(0, 10, shape).astype(F)
    mask = (rng.random(shape) < 0.7).astype(F)
    inside = np.stack([rng.integers(0, nx, 40), rng.integers(0, ny, 40), rng.integers(0, nz, 40)], 1)
    border = [[0, 0, 0], [nx - 1, 0, 0], [0, ny - 1, nz - 1], [nx - 1, ny - 1, nz - 1]]
    outside = [[-1, 0, 0], [nx, ny, nz], [-3, 40, 2], [5, -200, 1], [10 ** 6, 0, 0], [2, 3, -(2 ** 31)]]
    pts = np.concatenate([inside, border, outside]).astype(np.int64)
    nan_src = src.copy()
    nan_src.reshape(-1)[::3] = np.nan
    import torch
    for what, s, m, lo, hi, w in [("interval", src, None, 3.0, 6.0, 2.5), ("mask", src, mask, 3.0, 6.0, 1.3),
                                  ("one value", src, mask, 9.0, 9.0, 1.0), ("empty", src, None, 100.0, 200.0, 2.5),
                                  ("nan", nan_src, mask, -np.inf, np.inf, 1.3), ("no points", src, None, 3.0, 6.0, 1.0)]:
        p = pts[:0] if what == "no points" else pts
        want = dn.distance_from_points(s, p, lo, hi, w, m)
        assert want.dtype == F and want.shape == (len(p),)
        if what == "empty":
            assert_bits_equal(want, np.full(len(p), np.sqrt(F(dn.cap_of(shape)) * (F(w) * F(w))), F), "cap's distance")
        both_paths(ctx, api, lambda: ctx.distance_from_points(s, p, lo, hi, w, mask=m), want, "%s %s" % (shape, what))
        ds, dm = torch.from_numpy(s).cuda(), None if m is None else torch.from_numpy(m).cuda()
        both_paths(ctx, api, lambda: ctx.distance_from_points(ds, p, lo, hi, w, mask=dm), want, "%s %s device" % (shape, what))


def test_argument_errors_leave_the_context_usable(ctx, api):
    shape = (3, 5, 65)
    want = wanted(shape, "both")
    kw = seed_sets(shape)["both"]
    L, h = ctx._L, ctx._h
    dsq = np.empty(shape, np.int32)
    pts = np.zeros((1, 3), np.int32)
    one = np.zeros(8, F)

    def ok():
        assert_bits_equal(ctx.distance_sq(**kw), want, "after an error")

    # nx + ny + nz > 46340: (nx + ny + nz)^2 overflows the reference's int (nothing is read or allocated before the check)
    for dims in [(46339, 1, 1), (1, 46339, 1), (1, 1, 46339), (20000, 20000, 6341)]:
        assert sum(dims) == 46341
        rc = L.visfd_hip_distance_sq(h, None, None, dims[0], dims[1], dims[2], 0.0, 0.0, pts.ctypes.data, 1, dsq.ctypes.data)
        assert rc == 1 and b"46340" in L.visfd_hip_last_error()
        rc = L.visfd_hip_distance_to_points(h, one.ctypes.data, None, dims[0], dims[1], dims[2], pts.ctypes.data, 1, 1.0)
        assert rc == 1
        rc = L.visfd_hip_distance_from_points(h, one.ctypes.data, None, dims[0], dims[1], dims[2], 0.0, 1.0, pts.ctypes.data, 1,
                                              1.0, one.ctypes.data)
        assert rc == 1
        ok()
    with pytest.raises(api.VisfdHipError) as e:
        ctx.distance_sq((1, 1, 46339), points=pts)
    assert e.value.code == 1
    # dst overlapping mask
    buf = np.ones(2 * 3 * 5 * 65, F)
    dst, mask = buf[:975].reshape(shape), buf[974:974 + 975].reshape(shape)
    assert L.visfd_hip_distance_to_points(h, dst.ctypes.data, mask.ctypes.data, 65, 5, 3, pts.ctypes.data, 1, 1.0) == 1
    assert L.visfd_hip_distance_to_points(h, dst.ctypes.data, dst.ctypes.data, 65, 5, 3, pts.ctypes.data, 1, 1.0) == 1
    assert b"overlaps" in L.visfd_hip_last_error()
    ok()
    import torch
    t = torch.ones(2 * 975, device="cuda")
    assert L.visfd_hip_distance_to_points_dev(h, t.data_ptr(), t.data_ptr() + 4 * 974, 65, 5, 3, pts.ctypes.data, 1, 1.0) == 1
    ok()
    # npoints < 0
    assert L.visfd_hip_distance_sq(h, None, None, 65, 5, 3, 0.0, 0.0, pts.ctypes.data, -1, dsq.ctypes.data) == 1
    assert L.visfd_hip_distance_to_points(h, dst.ctypes.data, None, 65, 5, 3, pts.ctypes.data, -1, 1.0) == 1
    assert L.visfd_hip_distance_from_points(h, dst.ctypes.data, None, 65, 5, 3, 0.0, 1.0, pts.ctypes.data, -5, 1.0,
                                            one.ctypes.data) == 1
    assert b"points" in L.visfd_hip_last_error()
    ok()
    # points missing although counted; non-positive dimensions
    assert L.visfd_hip_distance_sq(h, None, None, 65, 5, 3, 0.0, 0.0, None, 2, dsq.ctypes.data) == 1
    assert L.visfd_hip_distance_sq(h, None, None, 65, 0, 3, 0.0, 0.0, None, 0, dsq.ctypes.data) == 1
    ok()
    # the largest size allowed passes its checks (a line of 46338 voxels: cap = 46340^2 < 2^31)
    line = ctx.distance_sq((1, 1, 46338), points=[[46337, 0, 0]])
    assert line[0, 0, 0] == 46337 ** 2 and line[0, 0, -1] == 0


def test_workspace_counts_the_stacks(ctx, api):
    """the envelope passes' stacks live in context workspace: 8 bytes per entry, [entry][lane] per wave"""
    ctx.trim()
    before = ctx.workspace_bytes()
    shape = (20, 23, 70)
    with ctx.options(distance_general=0):
        ctx.distance_sq(shape, points=[[1, 2, 3]])
    nz, ny, nx = shape
    xchunks = (nx + 63) // 64
    stack = 8 * 64 * max(nz * xchunks * ny, ny * xchunks * nz)
    assert ctx.workspace_bytes() - before >= stack + 4 * nz * ny * nx


# ---- filter_mrc -------------------------------------------------------------------------------------------------------
def header_stats(path):
    with open(path, "rb") as f:
        return np.frombuffer(f.read(1024), "<f4")[19:22].copy()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("distance_cli")
    for name, body in dc.POINT_FILES.items():
        (d / name).write_text(body)
    return d


@pytest.mark.parametrize("name", list(dc.CASES))
def test_cli_reproduces_the_reference(name, files):
    case = dc.CASES[name]
    gold = golden("distance")
    vol, mask = dc.inputs()[case["input"]]
    sub = files / name
    sub.mkdir()
    for pf in dc.POINT_FILES:
        (sub / pf).write_text(dc.POINT_FILES[pf])
    volgen.write_mrc(str(sub / "in.rec"), vol, voxel_width=case["w"])
    volgen.write_mrc(str(sub / "mask.rec"), mask, voxel_width=case["w"])
    args = dc.command(case, CLI, "in.rec", "mask.rec", "out.rec")
    r = subprocess.run(args, cwd=str(sub), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (args, r.stderr[-2000:])
    assert_bits_equal(volgen.read_mrc(str(sub / "out.rec")), gold["out/" + name], name)
    assert_bits_equal(header_stats(str(sub / "out.rec")), gold["header/" + name], name + " header (dmin, dmax, dmean)")
    if dc.writes_distances(case):
        assert (sub / dc.DIST).read_bytes() == gold["dist/" + name].tobytes(), name
    else:
        assert not (sub / dc.DIST).exists()


@pytest.mark.parametrize("flags,message", [
    (["-distance-points"], "Error: The -distance-points argument must be followed by a file name.\n"),
    (["-distance-to-voxels", "queries.txt", "dist.txt", "3"],
     "Error: The -distance-to-voxels argument must be followed by two file names and two numbers:\n"
     "       InFile OutFile BrightnessSelectMin BrightnessSelectMax\n"),
    (["-distance-to-voxels"],
     "Error: The -distance-to-voxels argument must be followed by two file names and two numbers:\n"
     "       InFile OutFile BrightnessSelectMin BrightnessSelectMax\n"),
])
def test_cli_missing_operands_carry_the_reference_messages(flags, message, files):
    r = subprocess.run([CLI, "-in", "in.rec", "-out", "out.rec"] + flags, cwd=str(files), capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and message in r.stderr, r.stderr


@pytest.mark.parametrize("flags", [["-distance-points", "phys.txt"], ["-distance-to-voxels", "queries.txt", "dist.txt", "3", "6"]])
def test_cli_rejects_the_flags_under_slab(flags, files):
    r = subprocess.run([CLI, "-in", "in.rec", "-out", "out.rec", "-slab", "0", "1", "-"] + flags, cwd=str(files),
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "-slab" in r.stderr and flags[0] in r.stderr, r.stderr
