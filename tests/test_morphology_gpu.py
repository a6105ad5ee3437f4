"""Grayscale morphology on the GPU (csrc/morph.hip): the six sphere ops and Dilate / Erode with an arbitrary element,
bit for bit against a numpy restatement of lib/visfd/morphology.hpp (tests/morph_np.py), through the ctypes ABI, the
torch device face, the C++ drop-in and the filter_mrc flags against the reference's own program."""
import os
import struct
import subprocess

import numpy as np
import pytest

import morph_np
import volgen
from conftest import GOLDEN, ROOT, assert_bits_equal

pytestmark = pytest.mark.gpu

OPS = ["dilate", "erode", "open", "close", "white", "black"]
ELEMENTS = {
    "flat": (2.5, 0.0, 0.0),
    "rim": (1.5, 2.6, 40.0),
    "corner": (2.2, 0.0, 3.0),
}


def special_volume(shape, seed):
    """Noise with +0 / -0 patches side by side, qNaN, a signalling-NaN bit pattern, +-inf and denormals."""
    rng = np.random.default_rng(seed)
    a = rng.normal(0.0, 10.0, shape).astype(np.float32)
    flat = a.reshape(-1)
    n = flat.size
    idx = rng.permutation(n)
    k = max(1, n // 40)
    flat[idx[0:k]] = 0.0
    flat[idx[k:2 * k]] = -0.0
    flat[idx[2 * k:2 * k + max(1, k // 4)]] = np.nan
    u = flat.view(np.uint32)
    u[idx[3 * k:3 * k + max(1, k // 4)]] = 0x7f800001   # signalling NaN
    u[idx[4 * k:4 * k + max(1, k // 4)]] = 0xffc00123   # negative quiet NaN with a payload
    flat[idx[5 * k:5 * k + max(1, k // 4)]] = np.inf
    flat[idx[6 * k:6 * k + max(1, k // 4)]] = -np.inf
    u[idx[7 * k:7 * k + max(1, k // 4)]] = 0x00000005   # denormal
    u[idx[8 * k:8 * k + max(1, k // 4)]] = 0x80400000   # negative denormal
    # a block of +0 next to a block of -0 (flat erosion: the first zero in element order decides the sign)
    nz, ny, nx = shape
    zs = slice(0, max(1, nz // 2))
    a[zs, : max(1, ny // 2), : max(1, nx // 2)] = 0.0
    a[zs, : max(1, ny // 2), max(1, nx // 2):] = -0.0
    return a


def mask_for(shape, seed):
    rng = np.random.default_rng(seed)
    m = (rng.random(shape) > 0.2).astype(np.float32)
    return m


def assert_nan_aware(got, want, what):
    """Bitwise outside the restatement's NaN positions; NaN where it has NaN (tests/test_gpu_parity.py practice)."""
    wn = np.isnan(want)
    assert np.array_equal(np.isnan(got), wn), what
    assert_bits_equal(np.where(wn, 0, got).astype(np.float32), np.where(wn, 0, want).astype(np.float32), what)


@pytest.fixture(scope="module")
def ctx():
    from visfd_amd import api
    c = api.Context(0)
    yield c
    c.close()


SHAPES = [((1, 40, 37), 2.5), ((5, 1, 64), 2.5), ((3, 3, 3), 4.0), ((58, 70, 64), None)]


@pytest.mark.parametrize("shape,r_override", SHAPES)
@pytest.mark.parametrize("element", sorted(ELEMENTS))
@pytest.mark.parametrize("with_mask", [False, True])
def test_sphere_ops_match_restatement(ctx, shape, r_override, element, with_mask):
    radius, rmax, bmax = ELEMENTS[element]
    if r_override is not None:
        radius = r_override if element != "rim" else min(radius, r_override)
    src = special_volume(shape, seed=sum(shape) * 10 + len(element))
    dst0 = np.random.default_rng(7).normal(0, 5, shape).astype(np.float32)   # the top-hats read dst; masked voxels keep it
    mask = mask_for(shape, 11) if with_mask else None
    for op, name in enumerate(OPS):
        got = ctx.morph_sphere(op, src, radius, rmax, bmax, mask=mask, dst=dst0)
        want = morph_np.sphere_op(op, src, radius, rmax, bmax, mask=mask, dst=dst0)
        what = "%s %s %s mask=%s" % (name, element, shape, with_mask)
        if name in ("white", "black"):
            assert_nan_aware(got, want, what)
        else:
            assert_bits_equal(got, want, what)
            if mask is not None:
                assert_bits_equal(got[mask == 0], dst0[mask == 0], what + " (masked voxels untouched)")


def test_table_ops_match_restatement(ctx):
    shape = (21, 30, 33)
    src = special_volume(shape, seed=5)
    mask = mask_for(shape, 6)
    rng = np.random.default_rng(8)
    d = rng.integers(-3, 4, (40, 3)).astype(np.int32)
    d[5] = (40, 0, 0)                    # an entry that always falls outside the image
    b = rng.normal(0, 2, 40).astype(np.float32)
    b[::7] = -0.0
    b[3::9] = 0.0
    for dilate in (True, False):
        for m in (None, mask):
            got = (ctx.dilate if dilate else ctx.erode)(src, d, b, mask=m)
            want = morph_np.dilate_erode(src, d, b, dilate, mask=m)
            assert_bits_equal(got, want, "table dilate=%s mask=%s" % (dilate, m is not None))
    # an empty element: every written voxel is -inf / +inf, as the reference's running value starts
    assert np.all(ctx.dilate(src, np.zeros((0, 3), np.int32), np.zeros(0, np.float32)) == -np.inf)


@pytest.mark.parametrize("radius", [1, 2, 5, 8, 10, 13])
def test_xrun_path_equals_general_kernel(ctx, radius):
    """The flat X-run kernel against the general element walk (option morph_general) on 256 x 256 x 128 with +0 / -0
    patches, NaN, inf and denormals, with and without a mask: dilate, erode (the zero-sign fix-up) and open.  Radius 13 is
    above the X-run cap and must take the general kernel either way."""
    from visfd_amd import api
    shape = (128, 256, 256)
    src = special_volume(shape, seed=21)
    mask = mask_for(shape, 22)
    want_path = api.MORPH_PATH_XRUNS if radius <= 10 else api.MORPH_PATH_GENERAL
    for m in (None, mask):
        for op in (api.MORPH_DILATE, api.MORPH_ERODE, api.MORPH_OPEN):
            fast = ctx.morph_sphere(op, src, radius, mask=m)
            assert ctx.morph_last_path() == want_path
            with ctx.options(morph_general=1):
                general = ctx.morph_sphere(op, src, radius, mask=m)
                assert ctx.morph_last_path() == api.MORPH_PATH_GENERAL
            assert_bits_equal(fast, general, "R=%d op=%d mask=%s" % (radius, op, m is not None))
    if radius == 2:   # the zero patches did reach the fix-up: both signs of zero come out of the erosion
        ero = ctx.morph_sphere(api.MORPH_ERODE, src, radius)
        z = ero[ero == 0]
        assert np.signbit(z).any() and (~np.signbit(z)).any()


def test_table_entry_selects_xruns_for_run_elements(ctx):
    """The arbitrary-element entry point takes the X-run kernel for flat elements of symmetric X-runs in any order, and the
    general kernel otherwise; results equal the restatement either way."""
    from visfd_amd import api
    shape = (20, 27, 70)
    src = special_volume(shape, seed=51)
    d, b = api.sphere_structure(3.0)
    perm = np.random.default_rng(52).permutation(len(b))
    keep = ~((d[:, 0] == 1) & (d[:, 1] == 0) & (d[:, 2] == 0))
    cases = [(d, b, api.MORPH_PATH_XRUNS), (d[perm], b[perm], api.MORPH_PATH_XRUNS),
             (d[keep], b[keep], api.MORPH_PATH_GENERAL),                  # row (0, 0) without dx = 1: not a run
             (d, np.where(np.arange(len(b)) == 3, np.float32(-0.0), b).astype(np.float32), api.MORPH_PATH_GENERAL)]
    for dd, bb, path in cases:
        for dilate in (True, False):
            got = (ctx.dilate if dilate else ctx.erode)(src, dd, bb)
            assert ctx.morph_last_path() == path
            assert_bits_equal(got, morph_np.dilate_erode(src, dd, bb, dilate), "table path %d dilate=%s" % (path, dilate))


def test_device_face_equals_host_face(ctx):
    import torch
    from visfd_amd import api
    shape = (17, 26, 31)
    src = special_volume(shape, seed=31)
    mask = mask_for(shape, 32)
    dst0 = np.random.default_rng(33).normal(0, 5, shape).astype(np.float32)
    ts, tm = torch.from_numpy(src).cuda(), torch.from_numpy(mask).cuda()
    for op in range(6):
        for m, tmk in ((None, None), (mask, tm)):
            td = torch.from_numpy(dst0.copy()).cuda()
            ctx.morph_sphere_dev(op, ts, td, 2.2, 0.0, 0.0, mask=tmk)
            ctx.synchronize()
            assert_bits_equal(td.cpu().numpy(), ctx.morph_sphere(op, src, 2.2, mask=m, dst=dst0), "dev op %d" % op)
    d, b = api.sphere_structure(2.0, 3.0, 10.0)
    td = torch.from_numpy(dst0.copy()).cuda()
    ctx.erode_dev(ts, td, d, b, mask=tm)
    ctx.synchronize()
    assert_bits_equal(td.cpu().numpy(), ctx.erode(src, d, b, mask=mask, dst=dst0), "dev table erode")
    with pytest.raises(api.VisfdHipError):
        ctx.dilate_sphere_dev(ts, ts, 2.0)                # src == dst is refused
    flat_buf = torch.zeros(2 * src.size, device="cuda")
    a = flat_buf[: src.size].view(shape)
    b_ = flat_buf[src.size // 2: src.size // 2 + src.size].view(shape)
    with pytest.raises(api.VisfdHipError):
        ctx.dilate_sphere_dev(a, b_, 2.0)                 # dst overlapping src
    with pytest.raises(api.VisfdHipError):
        ctx.dilate_sphere_dev(ts, b_, 2.0, mask=a)        # dst overlapping the mask


def _read_records(path):
    out = {}
    with open(path, "rb") as f:
        while True:
            tag = f.read(32)
            if len(tag) < 32:
                break
            n, = struct.unpack("<q", f.read(8))
            out[tag.split(b"\0")[0].decode()] = np.frombuffer(f.read(4 * n), np.float32).copy()
    return out


def test_cpp_shim_morphology(tmp_path):
    exe = str(tmp_path / "shim_morph_check")
    libdir = os.path.join(ROOT, "visfd_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "shim_morph_check.cpp"), "-o", exe, "-L" + libdir, "-lvisfd_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    shape = (14, 19, 23)
    nz, ny, nx = shape
    src = special_volume(shape, seed=41)
    mask = mask_for(shape, 42)
    dest0 = np.random.default_rng(43).normal(0, 5, shape).astype(np.float32)   # NOT a copy of src
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<iii", nx, ny, nz))
        for a in (src, mask, dest0):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "shim morph check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    R = {k: v.reshape(shape) for k, v in _read_records(tmp_path / "out.bin").items()}
    sf_d = np.array([(0, 0, 0), (2, -1, 0), (-1, 0, 1), (0, 3, -2)], np.int32)
    sf_b = np.array([0.0, -1.5, 0.25, -0.0], np.float32)
    want = {
        "dilate": morph_np.sphere_op(0, src, 2.5, dst=dest0),
        "erode_mask": morph_np.sphere_op(1, src, 2.5, mask=mask, dst=dest0),
        "open": morph_np.sphere_op(2, src, 2.5, dst=dest0),
        "close_mask": morph_np.sphere_op(3, src, 2.5, mask=mask, dst=dest0),
        "white": morph_np.sphere_op(4, src, 2.5, dst=dest0),
        "black_mask": morph_np.sphere_op(5, src, 2.5, mask=mask, dst=dest0),
        "dilate_soft_mask": morph_np.sphere_op(0, src, 2.0, 3.5, 50.0, mask=mask, dst=dest0),
        "dilate_table": morph_np.dilate_erode(src, sf_d, sf_b, True, dst=dest0),
        "erode_table_mask": morph_np.dilate_erode(src, sf_d, sf_b, False, mask=mask, dst=dest0),
    }
    for k, w in want.items():
        if k in ("white", "black_mask"):
            assert_nan_aware(R[k], w, k)
        else:
            assert_bits_equal(R[k], w, k)
    # WhiteTopHatSphere is dest -= open(src): with dest != src the result is dest0 - open, not src - open
    opened = morph_np.sphere_op(2, src, 2.5)
    with np.errstate(all="ignore"):
        assert_nan_aware(R["white"], dest0 - opened, "white top-hat subtracts from dest")


# ---------------------------------------------------------------------------------- filter_mrc against the reference program
CLI = os.path.join(ROOT, "visfd_amd", "cli", "filter_mrc")
REF_CLI = os.path.join(ROOT, "oracle", "_ref", "filter_mrc_ref")


@pytest.fixture(scope="module")
def ref_cli():
    if not os.path.exists(REF_CLI):
        pytest.skip("oracle/_ref/filter_mrc_ref not built (needs the reference sources at build time)")
    return REF_CLI


def both(ref_cli, tmp_path, args, out_name="out.rec"):
    """The same command line through both programs in separate directories; returns the two directories."""
    dirs = []
    for tag, exe in (("mine", CLI), ("ref", ref_cli)):
        d = tmp_path / tag
        d.mkdir(exist_ok=True)
        r = subprocess.run([exe] + [str(a) for a in args] + ["-out", out_name], cwd=str(d), capture_output=True, text=True)
        assert r.returncode == 0, (tag, r.stderr[-2000:])
        dirs.append(d)
    return dirs


BLOB = os.path.join(GOLDEN, "test_blob_detect.rec")
BLOB_MASK = os.path.join(GOLDEN, "test_blob_detect_mask.rec")


@pytest.mark.parametrize("flags", [
    ["-dilate", 60, "-w", 19.6],
    ["-dilation", 45, "-w", 19.6, "-mask", BLOB_MASK],
    ["-erode", 60, "-w", 19.6],
    ["-erosion", 3, "-w", 1, "-mask", BLOB_MASK, "-mask-out", 7],
    ["-open", 50, "-w", 19.6],
    ["-opening", 2.5, "-w", 1, "-mask", BLOB_MASK],
    ["-close", 50, "-w", 19.6],
    ["-closing", 2, "-w", 1, "-bin", 2],
    ["-top-hat-white", 60, "-w", 19.6],
    ["-top-hat-white", 2, "-w", 1, "-mask", BLOB_MASK, "-mask-out", 7],
    ["-top-hat-black", 60, "-w", 19.6],
    ["-top-hat-black", 3, "-w", 1, "-mask", BLOB_MASK],
    ["-dilate-binary-soft", 40, 70, 20, "-w", 19.6],
    ["-dilation-binary-soft", 2, 3, 5, "-w", 1, "-mask", BLOB_MASK],
    ["-erode-binary-soft", 50, 30, 8, "-w", 19.6],
    ["-erosion-binary-soft", 2.5, 3.5, 4, "-w", 1, "-bin", 2],
])
def test_cli_morphology_equals_reference_program(ref_cli, tmp_path, flags):
    mine, ref = both(ref_cli, tmp_path, ["-in", BLOB] + flags)
    a, b = volgen.read_mrc(str(mine / "out.rec")), volgen.read_mrc(str(ref / "out.rec"))
    assert_bits_equal(a, b, " ".join(map(str, flags)))


@pytest.mark.parametrize("flags", [
    ["-dilate", 2.5], ["-erode", 2.5], ["-open", 2], ["-close", 2], ["-top-hat-white", 2], ["-top-hat-black", 2],
    ["-erode-binary-soft", 2, 0, 3], ["-dilate-binary-soft", 1.5, 2.5, 30],
])
def test_cli_morphology_special_values_equal_reference_program(ref_cli, tmp_path, flags):
    """A 96^3 volume with +-0 patches, NaN and inf: bitwise, except that NaN results only need to be NaN (their payloads
    are the arithmetic unit's business)."""
    vol = special_volume((96, 96, 96), seed=77)
    path = str(tmp_path / "special.rec")
    volgen.write_mrc(path, vol, voxel_width=1.0)
    mine, ref = both(ref_cli, tmp_path, ["-in", path, "-w", 1] + flags)
    a, b = volgen.read_mrc(str(mine / "out.rec")), volgen.read_mrc(str(ref / "out.rec"))
    assert_nan_aware(a, b, " ".join(map(str, flags)))
