"""The median filter on the GPU (csrc/median.hip): MedianSphere and Median with arbitrary footprints, bit for bit against
the numpy restatement of the contract (tests/median_np.py), on both kernels, through the ctypes ABI, the torch device face
and the C++ drop-in, and against what the reference program wrote for the footprints it completes."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import median_np
from conftest import GOLDEN, ROOT, assert_bits_equal, golden

pytestmark = pytest.mark.gpu

F = np.float32
POISON = 0xdeadbeef            # what dst holds before a call: it must survive exactly where mask == 0
TILE_PLUS_ONE = (5, 5, 65)     # one voxel more than the tiled kernel's 64 x 4 x 4 outputs along each axis
R_TILED_MAX, R_DECLINED = 5.0, 6.0   # the largest ball the tiled kernel's 64 KiB of LDS takes, and the first it declines


def special_volume(shape, seed):
    """Noise with +0 / -0 patches side by side, qNaN, a signalling-NaN bit pattern, +-inf, denormals and the two bit
    patterns with the extreme keys (0x7fffffff, 0xffffffff)."""
    rng = np.random.default_rng(seed)
    a = rng.normal(0.0, 10.0, shape).astype(F)
    flat = a.reshape(-1)
    n = flat.size
    idx = rng.permutation(n)
    k = max(1, n // 40)
    q = max(1, k // 4)
    flat[idx[0:k]] = 0.0
    flat[idx[k:2 * k]] = -0.0
    flat[idx[2 * k:2 * k + q]] = np.nan
    u = flat.view(np.uint32)
    u[idx[3 * k:3 * k + q]] = 0x7f800001   # signalling NaN
    u[idx[4 * k:4 * k + q]] = 0xffc00123   # negative quiet NaN with a payload
    flat[idx[5 * k:5 * k + q]] = np.inf
    flat[idx[6 * k:6 * k + q]] = -np.inf
    u[idx[7 * k:7 * k + q]] = 0x00000005   # denormal
    u[idx[8 * k:8 * k + q]] = 0x80400000   # negative denormal
    u[idx[9 * k:9 * k + q]] = 0x7fffffff   # the largest key
    u[idx[10 * k:10 * k + q]] = 0xffffffff  # the smallest key
    nz, ny, nx = shape
    zs = slice(0, max(1, nz // 2))
    a[zs, : max(1, ny // 2), : max(1, nx // 2)] = 0.0
    a[zs, : max(1, ny // 2), max(1, nx // 2):] = -0.0
    return a


def mask_for(shape, seed):
    return (np.random.default_rng(seed).random(shape) > 0.25).astype(F)


def poisoned(shape):
    return np.full(shape, POISON, np.uint32).view(F)


@pytest.fixture(scope="module")
def ctx():
    from visfd_amd import api
    c = api.Context(0)
    yield c
    c.close()


def both_paths(ctx, run, tiled_takes_it, want, mask, what):
    """`run()` on the library's own choice and on the general walk: the kernel that ran, the restatement's bits, and the
    poison where mask == 0."""
    from visfd_amd import api
    for general in (0, 1):
        with ctx.options(median_general=general):
            got = run()
            path = ctx.median_last_path()
        assert path == (api.MEDIAN_PATH_TILED if tiled_takes_it and not general else api.MEDIAN_PATH_GENERAL), (what, general)
        assert_bits_equal(got, want, "%s general=%d" % (what, general))
        if mask is not None:
            assert np.all(got.view(np.uint32)[mask == 0] == POISON), what


RADII = [0.0, 1.0, 1.5, 2.0, 2.5, 3.0, R_TILED_MAX, R_DECLINED]   # 1 .. 3: the entry counts compiled into the tiled kernel
CASES = [(s, r) for s in [(1, 40, 37), (5, 1, 64), (6, 9, 1), TILE_PLUS_ONE, (20, 23, 70)] for r in RADII] + [((3, 3, 3), 4.0)]


@pytest.mark.parametrize("shape,radius", CASES)
@pytest.mark.parametrize("with_mask", [False, True])
def test_sphere_matches_restatement_on_both_kernels(ctx, shape, radius, with_mask):
    src = special_volume(shape, seed=sum(shape) * 10 + int(2 * radius))
    mask = mask_for(shape, 11) if with_mask else None
    dst0 = poisoned(shape)
    want = median_np.median_sphere(src, radius, mask=mask, dst=dst0)
    both_paths(ctx, lambda: ctx.median_sphere(src, radius, mask=mask, dst=dst0), radius <= R_TILED_MAX, want, mask,
               "%s r=%g mask=%s" % (shape, radius, with_mask))


def test_special_values_reach_the_output(ctx):
    """The salted patterns do come out of the filter: zeros of both signs, and a NaN where NaNs are the majority."""
    src = special_volume((20, 23, 70), seed=5)
    out = ctx.median_sphere(src, 1.0)
    z = out[out == 0]
    assert np.signbit(z).any() and (~np.signbit(z)).any()
    nan = np.full((4, 5, 66), np.nan, F)
    nan.view(np.uint32)[:, :, ::2] = 0xffc00123
    assert_bits_equal(ctx.median_sphere(nan, 1.5), median_np.median_sphere(nan, 1.5), "all NaN")


TABLES = {
    "asymmetric": [(0, 0, 0), (1, 0, 0), (2, 1, 0), (0, -1, 3), (3, 2, -1), (-1, 0, 0)],
    "duplicates": [(0, 0, 0)] * 3 + [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, 1, 0), (0, 0, -2)],
    "no_centre": [(1, 0, 0), (2, 0, 0), (1, 1, 0), (1, 1, 0)],          # the bounding box does not hold the centre either
    "far": [(16, 0, 0), (-16, 3, 0), (0, 0, 0), (0, -16, 16)],          # the offset limit: beyond the tiled kernel's budget
}


@pytest.mark.parametrize("name", sorted(TABLES))
def test_table_matches_restatement_on_both_kernels(ctx, name):
    shape = (9, 14, 70)
    d = np.array(TABLES[name], np.int32)
    src = special_volume(shape, seed=61)
    mask = mask_for(shape, 62)
    if name == "no_centre":
        mask[:, :, 40:] = 0.0
        mask[:, ::2, 39] = 1.0          # voxels whose every neighbour is masked or outside: they get +0.0f
    dst0 = poisoned(shape)
    for m in (None, mask):
        want = median_np.median_table(src, d, mask=m, dst=dst0)
        both_paths(ctx, lambda: ctx.median_table(src, d, mask=m, dst=dst0), name != "far", want, m, name)
    if name == "no_centre":
        want = median_np.median_table(src, d, mask=mask, dst=dst0)
        assert ((want.view(np.uint32) == 0) & (mask != 0))[:, ::2, 39].all()


def test_device_face_equals_host_face(ctx):
    import torch
    from visfd_amd import api
    shape = (17, 26, 31)
    src = special_volume(shape, seed=31)
    mask = mask_for(shape, 32)
    dst0 = poisoned(shape)
    ts, tm = torch.from_numpy(src).cuda(), torch.from_numpy(mask).cuda()
    d = np.array(TABLES["asymmetric"], np.int32)
    for general in (0, 1):
        with ctx.options(median_general=general):
            for m, tmk in ((None, None), (mask, tm)):
                td = torch.from_numpy(dst0.copy()).cuda()
                ctx.median_sphere_dev(ts, td, 2.5, mask=tmk)
                ctx.synchronize()
                assert_bits_equal(td.cpu().numpy(), ctx.median_sphere(src, 2.5, mask=m, dst=dst0), "dev sphere")
                td = torch.from_numpy(dst0.copy()).cuda()
                ctx.median_table_dev(ts, td, d, mask=tmk)
                ctx.synchronize()
                assert_bits_equal(td.cpu().numpy(), ctx.median_table(src, d, mask=m, dst=dst0), "dev table")


def test_bad_arguments_are_einval(ctx):
    import torch
    from visfd_amd import api
    shape = (6, 7, 8)
    src = special_volume(shape, seed=71)
    ts = torch.from_numpy(src).cuda()
    td = torch.empty_like(ts)
    flat_buf = torch.zeros(2 * src.size, device="cuda")
    a = flat_buf[: src.size].view(shape)
    b = flat_buf[src.size // 2: src.size // 2 + src.size].view(shape)
    calls = [
        lambda: ctx.median_sphere_dev(ts, ts, 2.0),                 # src == dst
        lambda: ctx.median_sphere_dev(a, b, 2.0),                   # dst overlapping src
        lambda: ctx.median_sphere_dev(ts, b, 2.0, mask=a),          # dst overlapping the mask
        lambda: ctx.median_table_dev(a, b, [(0, 0, 0)]),
        lambda: ctx.median_sphere_dev(ts, td, 17.0),                # beyond the radius limit
        lambda: ctx.median_sphere(src, 17.0),
        lambda: ctx.median_sphere(src, -1.0),
        lambda: ctx.median_table(src, np.zeros((0, 3), np.int32)),  # an empty table
        lambda: ctx.median_table(src, [(17, 0, 0)]),                # an offset beyond 16
        lambda: ctx.median_table(src, np.zeros((32769, 3), np.int32)),
    ]
    for k, call in enumerate(calls):
        with pytest.raises(api.VisfdHipError) as e:
            call()
        assert e.value.code == 1, (k, e.value)                      # VISFD_HIP_EINVAL
    ok = ctx.median_table(src, np.zeros((32768, 3), np.int32))      # the largest table: 32768 times the centre
    assert_bits_equal(ok, src, "32768 copies of the centre")


def test_footprint_survives_other_stages_and_poisoned_workspace(ctx):
    """One context: median, then morphology (its own table slot), then every slot overwritten, then the same median."""
    from visfd_amd import api
    shape = (12, 13, 70)
    src = special_volume(shape, seed=81)
    mask = mask_for(shape, 82)
    first = ctx.median_sphere(src, 2.5, mask=mask)
    assert_bits_equal(first, median_np.median_sphere(src, 2.5, mask=mask), "first call")
    ctx.morph_sphere(api.MORPH_DILATE, src, 3.0)
    assert_bits_equal(ctx.median_sphere(src, 2.5, mask=mask), first, "after morphology")
    ctx.debug_poison_workspace()
    assert_bits_equal(ctx.median_sphere(src, 2.5, mask=mask), first, "after the poisoned workspace")
    ctx.trim()
    assert_bits_equal(ctx.median_sphere(src, 2.5, mask=mask), first, "after trim")


def _read_records(path):
    out = {}
    with open(path, "rb") as f:
        while True:
            tag = f.read(32)
            if len(tag) < 32:
                break
            n, = struct.unpack("<q", f.read(8))
            out[tag.split(b"\0")[0].decode()] = np.frombuffer(f.read(4 * n), F).copy()
    return out


def test_cpp_shim_median(tmp_path):
    exe = str(tmp_path / "shim_median_check")
    libdir = os.path.join(ROOT, "visfd_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "shim_median_check.cpp"), "-o", exe, "-L" + libdir, "-lvisfd_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    shape = (14, 19, 23)
    nz, ny, nx = shape
    src = special_volume(shape, seed=41)
    mask = mask_for(shape, 42)
    dest0 = poisoned(shape)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<iii", nx, ny, nz))
        for a in (src, mask, dest0):
            f.write(np.ascontiguousarray(a, F).tobytes())
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "shim median check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    R = {k: v.reshape(shape) for k, v in _read_records(tmp_path / "out.bin").items()}
    fp = np.array([(0, 0, 0), (2, -1, 0), (2, -1, 0), (-1, 0, 1), (0, 3, -2)], np.int32)
    want = {
        "sphere": median_np.median_sphere(src, 2.5, dst=dest0),
        "sphere_mask": median_np.median_sphere(src, 1.5, mask=mask, dst=dest0),
        "sphere_mask_report": median_np.median_sphere(src, 2.0, mask=mask, dst=dest0),
        "table": median_np.median_table(src, fp, dst=dest0),
        "table_mask": median_np.median_table(src, fp, mask=mask, dst=dest0),
    }
    assert sorted(R) == sorted(want)
    for k, w in want.items():
        assert_bits_equal(R[k], w, k)


def test_library_equals_reference_program_golden(ctx):
    """The footprints the reference's own program completes (radius 0 and 0.5, with a mask), as recorded in
    tests/golden/median.npz; the program fills the masked voxels with 0, so dst starts as zeros here."""
    sys.path.insert(0, GOLDEN)
    import make_golden_median as G
    g = golden("median")
    src, mask = G.volume(int(g["seed"]))
    assert_bits_equal(src, g["src"], "volume rebuilt from its seed")
    for r in G.RADII:
        both_paths_plain = []
        for general in (0, 1):
            with ctx.options(median_general=general):
                both_paths_plain.append(ctx.median_sphere(src, r, mask=mask, dst=np.zeros_like(src)))
        assert_bits_equal(both_paths_plain[0], g["out/%g" % r], "radius %g" % r)
        assert_bits_equal(both_paths_plain[1], g["out/%g" % r], "radius %g, general walk" % r)
