"""The general 3-D filter on the GPU (csrc/filter3d.hip) against the numpy restatement tests/filter3d_np.py -- itself
checked against the reference program's golden outputs in test_filter3d.py -- and against those goldens directly.
Every comparison is bitwise."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import filter3d_cases as FC
import filter3d_np as FN
import volgen
from conftest import GOLDEN, ROOT, assert_bits_equal

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "visfd_amd", "cli", "filter_mrc")
REF_CLI = os.path.join(ROOT, "oracle", "_ref", "filter_mrc_ref")
GOLD = os.path.join(GOLDEN, "filter3d.npz")


@pytest.fixture(scope="module")
def ctx():
    from visfd_amd import api
    c = api.Context(0)
    yield c
    c.close()


def random_table(hw, seed):
    """Distinct signed weights: a symmetric table would hide index and order errors."""
    rng = np.random.default_rng(seed)
    shape = (2 * hw[2] + 1, 2 * hw[1] + 1, 2 * hw[0] + 1)
    t = rng.uniform(0.05, 1.0, shape) * rng.choice([-1.0, 1.0], shape)
    return t.astype(np.float32)


def make_mask(shape, form, seed):
    if form == "none":
        return None
    rng = np.random.default_rng(seed)
    m = np.ones(shape, np.float32)
    nz, ny, nx = shape
    m[:, : max(1, ny // 5), :] = 0                       # a block
    m[nz // 2:, ny // 2:, nx // 3: nx // 3 + 7] = 0
    m[rng.random(shape) < 0.1] = 0
    if form == "weighted":                               # values in (0, 2] and zeros
        m = (m * (2.0 - 1.99 * rng.random(shape))).astype(np.float32)
    return m


# (shape (nz, ny, nx), half-widths (hx, hy, hz)): one plane; one row; a window wider than the image on every axis; two
# workgroups per axis with remainders; flat axes in the window, where workgroups with their whole window inside the image
# exist (the loop without bounds tests, the constant denominator); the same with a window in z.
PARITY = [
    ((1, 40, 37), (2, 3, 1)),
    ((5, 1, 64), (2, 1, 3)),
    ((3, 3, 3), (4, 4, 4)),
    ((19, 21, 70), (3, 2, 4)),
    ((9, 40, 130), (1, 6, 0)),
    ((12, 20, 200), (2, 2, 2)),
]


@pytest.mark.parametrize("form", ["none", "block", "weighted"])
@pytest.mark.parametrize("shape,hw", PARITY)
def test_filter3d_matches_restatement(ctx, shape, hw, form):
    k = PARITY.index((shape, hw))
    src = volgen.noise_volume(shape, seed=40 + k, mean=3.0, sd=50.0)
    table = random_table(hw, 60 + k)
    mask = make_mask(shape, form, 80 + k)
    for normalize in (False, True):
        want, want_den = FN.apply(src, table, hw, mask, normalize, want_den=True)
        what = "%s h=%s mask=%s normalize=%d" % (shape, hw, form, normalize)
        got, den = ctx.filter3d(src, table, mask, normalize, want_den=True)
        assert_bits_equal(got, want, what)
        assert_bits_equal(den, want_den, what + " (denominator)")
        assert_bits_equal(ctx.filter3d(src, table, mask, normalize), want, what + " (no denominator asked for)")
        with ctx.options(filter3d_general=1):
            got, den = ctx.filter3d(src, table, mask, normalize, want_den=True)
            assert_bits_equal(got, want, what + " (general kernel)")
            assert_bits_equal(den, want_den, what + " (general kernel, denominator)")
            assert_bits_equal(ctx.filter3d(src, table, mask, normalize), want, what + " (general kernel, no denominator)")


# A volume of several workgroups per axis with windows up to h = 12 (15625 entries).  The restatement costs one array
# operation per entry, so it runs on three blocks of receivers, each cut out with its window (the cut keeps every sender
# a block has, and a cut's face that is the image's face skips the same senders): the origin corner and the far corner,
# and a block inside the volume across x = 64, the seam between a workgroup whose window leaves the image (x 0..63) and
# one that holds its whole window for every h <= 12 (x 64..127, y 28..35, z 16..23: the tiled kernel's eight planes): the
# first counts its denominator, the second takes the constant; the general kernel tests its senders in the first and not
# in the second.  The two kernels are compared on the whole volume, and the option's effect is read back.
WIDE_SHAPE = (40, 72, 200)
WIDE_BLOCKS = [(0, 1, 0, 4, 62, 66), (39, 40, 70, 72, 197, 200), (19, 21, 31, 33, 62, 66)]


@pytest.fixture(scope="module")
def wide_inputs():
    src = volgen.noise_volume(WIDE_SHAPE, seed=101, mean=3.0, sd=50.0)
    mask = make_mask(WIDE_SHAPE, "weighted", 102)
    src.setflags(write=False)
    mask.setflags(write=False)
    return src, mask


@pytest.mark.parametrize("form", ["none", "weighted"])
@pytest.mark.parametrize("h", [1, 3, 5, 8, 12])
def test_filter3d_wide_windows(ctx, wide_inputs, h, form):
    src, mask = wide_inputs
    mask = None if form == "none" else mask
    hw = (h, h, h)
    table = random_table(hw, 110 + h)
    from visfd_amd import api
    got, den = ctx.filter3d(src, table, mask, True, want_den=True)
    assert ctx.filter3d_last_path() == api.FILTER3D_PATH_TILED
    with ctx.options(filter3d_general=1):
        got_g, den_g = ctx.filter3d(src, table, mask, True, want_den=True)
        assert ctx.filter3d_last_path() == api.FILTER3D_PATH_GENERAL
    assert_bits_equal(got, got_g, "h=%d mask=%s: tiled against general" % (h, form))
    assert_bits_equal(den, den_g, "h=%d mask=%s: tiled against general (denominator)" % (h, form))
    for z0, z1, y0, y1, x0, x1 in WIDE_BLOCKS:
        lo = [max(0, a - h) for a in (z0, y0, x0)]
        cut = tuple(slice(l, min(n, b + h)) for l, b, n in zip(lo, (z1, y1, x1), WIDE_SHAPE))
        want, want_den = FN.apply(src[cut], table, hw, None if mask is None else mask[cut], True, want_den=True)
        inner = tuple(slice(a - l, b - l) for a, b, l in zip((z0, y0, x0), (z1, y1, x1), lo))
        block = (slice(z0, z1), slice(y0, y1), slice(x0, x1))
        what = "h=%d mask=%s block %s" % (h, form, (z0, z1, y0, y1, x0, x1))
        assert_bits_equal(got[block], want[inner], what)
        assert_bits_equal(den[block], want_den[inner], what + " (denominator)")


@pytest.mark.parametrize("form", ["none", "weighted"])
def test_filter3d_window_the_tiled_kernel_refuses(ctx, wide_inputs, form):
    """h = (40, 40, 0): two patches of 144 x 84 floats are more than 48 KB, so the general kernel runs, asked or not."""
    from visfd_amd import api
    src, mask = wide_inputs
    mask = None if form == "none" else mask
    hw = (40, 40, 0)
    table = random_table(hw, 120)
    table[0, 30:50, 30:50] *= 8                       # keeps the denominator away from 0
    got, den = ctx.filter3d(src, table, mask, True, want_den=True)
    assert ctx.filter3d_last_path() == api.FILTER3D_PATH_GENERAL
    cut = (slice(3, 4), slice(0, 72), slice(0, 200))   # no window in z: one plane is a whole problem
    want, want_den = FN.apply(src[cut], table, hw, None if mask is None else mask[cut], True, want_den=True)
    assert_bits_equal(got[cut], want, "h=%s mask=%s" % (hw, form))
    assert_bits_equal(den[cut], want_den, "h=%s mask=%s (denominator)" % (hw, form))
    with ctx.options(filter3d_general=1):
        assert_bits_equal(ctx.filter3d(src, table, mask, True), got, "h=%s: the option changes nothing" % (hw,))
        assert ctx.filter3d_last_path() == api.FILTER3D_PATH_GENERAL


def test_table_is_sent_again_for_another_row_length(ctx):
    """The sender offsets on the device belong to one nx and ny: the same table on another image must not reuse them."""
    hw = (2, 1, 1)
    table = random_table(hw, 131)
    with ctx.options(filter3d_general=1):     # the kernel that reads them
        for shape in ((6, 12, 200), (6, 14, 196), (6, 12, 200)):
            src = volgen.noise_volume(shape, seed=132)
            assert_bits_equal(ctx.filter3d(src, table, None, False), FN.apply(src, table, hw, None, False), str(shape))


def test_filter3d_device_face(ctx):
    import torch
    shape, hw = (12, 20, 200), (2, 2, 2)
    src = volgen.noise_volume(shape, seed=7)
    table = random_table(hw, 8)
    mask = make_mask(shape, "weighted", 9)
    want, want_den = FN.apply(src, table, hw, mask, True, want_den=True)
    s, m = torch.from_numpy(src).cuda(), torch.from_numpy(mask).cuda()
    d, den = torch.empty_like(s), torch.empty_like(s)
    ctx.filter3d_dev(s, d, table, m, True, den)
    ctx.synchronize()
    assert_bits_equal(d.cpu().numpy(), want, "device face")
    assert_bits_equal(den.cpu().numpy(), want_den, "device face (denominator)")


def test_unmasked_denominator_equals_mask_of_ones(ctx):
    """The constant denominator of workgroups inside the image and the sum over a mask of ones give the same bits, in
    both kernels.  (12, 20, 200) with h = 2: workgroup x 64..127, y 4..15 is inside for planes 2..9 of the general kernel
    and planes 8..9 of no tiled workgroup, so 24 planes give the tiled kernel an inside workgroup too (z 8..15)."""
    shape, hw = (24, 20, 200), (2, 2, 2)
    src = volgen.noise_volume(shape, seed=11)
    table = np.abs(random_table(hw, 12))
    for general in (0, 1):
        with ctx.options(filter3d_general=general):
            a, da = ctx.filter3d(src, table, None, True, want_den=True)
            b, db = ctx.filter3d(src, table, np.ones(shape, np.float32), True, want_den=True)
        assert_bits_equal(a, b, "normalised, unmasked against a mask of ones")
        assert_bits_equal(da, db, "denominator, unmasked against a mask of ones")
        assert len(np.unique(da[8:16, 4:16, 70:120])) == 1    # one number inside


def test_zero_entries_are_dropped_exactly(ctx):
    """A spherical support zeroes the corners of its cube: the kernel leaves those entries out, the restatement adds
    their zero products; an explicit -0.0f entry too."""
    width, m, hw = (2.1, 2.1, 2.1), 3.0, (5, 5, 5)
    table = FN.gengauss3d_table(width, m, hw)[0].copy()
    assert (table == 0).sum() > table.size // 3
    table[5, 5, 3] = -0.0
    table[1:4, 5, 5] *= -1
    shape = (14, 24, 130)
    src = volgen.noise_volume(shape, seed=13, mean=0.0)
    for mask in (None, make_mask(shape, "weighted", 14)):
        got, den = ctx.filter3d(src, table, mask, True, want_den=True)
        want, want_den = FN.apply(src, table, hw, mask, True, want_den=True)
        assert_bits_equal(got, want, "table with zero entries")
        assert_bits_equal(den, want_den, "table with zero entries (denominator)")


@pytest.mark.parametrize("name", sorted(FC.CASES))
def test_named_filters_match_reference_golden(ctx, name):
    from visfd_amd import api
    g = np.load(GOLD)
    src, mask = FC.inputs(name)
    p = FC.CASES[name][3]
    if p[0] == "ggauss":
        _, width, m, ratio, norm = p
        hw = api.gengauss3d_halfwidths(width, m, ratio)
        got, A = ctx.apply_ggauss(src, width, m, hw, mask, norm)
        t, Aw = FN.gengauss3d_table(width, m, hw)
        want = FN.apply(src, t, hw, mask, norm)
        assert np.float32(A) == Aw
    elif p[0] == "dogg":
        _, wa, wb, m, n, ratio = p
        got, A, B = ctx.apply_dogg(src, wa, wb, m, n, ratio, 0.03, mask)
        t, hw, Aw, Bw = FN.dogg3d_table(wa, wb, m, n, ratio)
        want = FN.apply(src, t, hw, mask, False)
        assert (np.float32(A), np.float32(B)) == (Aw, Bw)
    else:
        _, radius, exponent, ratio, norm = p
        sg, r = api.fluctuation_sigmas(radius, exponent, ratio, 0.03)
        got = ctx.local_fluctuations_gen(src, sg, r, mask, norm, exponent)
        want = FN.local_fluctuations(src, sg, exponent, r, mask, norm)
    assert_bits_equal(got, want, name + " against the restatement")
    assert_bits_equal(got, g[name + "/out"], name + " against the reference program")


def test_dogg_with_mask_writes_zero_outside(ctx):
    src, _ = FC.inputs("dogg")
    mask = make_mask(src.shape, "block", 21)
    got, A, B = ctx.apply_dogg(src, (1.2,) * 3, (2.0,) * 3, 2.0, 4.0, 2.5, 0.03, mask)
    t, hw, _, _ = FN.dogg3d_table((1.2,) * 3, (2.0,) * 3, 2.0, 4.0, 2.5)
    assert_bits_equal(got, FN.apply(src, t, hw, mask, False), "DoGG with a mask")
    assert not got[mask == 0].any()


def test_fluctuations_gen_exponent_2_is_the_separable_path(ctx):
    from visfd_amd import api
    src = volgen.noise_volume((17, 21, 36), seed=31)
    mask = volgen.block_mask(src.shape, seed=32)
    sg, r = api.fluctuation_sigmas((3.0, 5.0, 2.5), 2.0, 2.5, 0.03)
    for m in (None, mask):
        assert_bits_equal(ctx.local_fluctuations_gen(src, sg, r, m, True, 2.0), ctx.local_fluctuations(src, sg, r, m, True),
                          "exponent 2")
    with pytest.raises(api.VisfdHipError):
        ctx.local_fluctuations(src, sg, r, None, True, 6.0)      # the Gaussian entry still refuses


def test_filter3d_refusals(ctx):
    from visfd_amd import api
    L = ctx._L
    src = volgen.noise_volume((6, 8, 70), seed=41)
    dst = np.empty_like(src)
    mask = np.ones_like(src)
    table = random_table((1, 1, 1), 42)
    tp, hw = table.ctypes.data_as(api._fp), api._i3((1, 1, 1))

    def call(s, d, m, h=hw, den=None):
        return L.visfd_hip_filter3d(ctx._h, api._np(s), api._np(d), api._np(m), 70, 8, 6, tp, h, 0, api._np(den))
    assert call(src, dst, mask) == 0
    assert call(src, src, None) == 1                                     # dst overlaps src
    assert "in place" in L.visfd_hip_last_error().decode()
    assert call(src, mask, mask) == 1                                    # dst overlaps mask
    assert "overlaps mask" in L.visfd_hip_last_error().decode()
    assert call(src, dst, None, den=dst) == 1                            # the denominator is its own array
    assert call(src, dst, None, api._i3((1, -1, 1))) == 1                # negative half-widths
    assert "negative" in L.visfd_hip_last_error().decode()
    with pytest.raises(api.VisfdHipError):
        ctx.apply_ggauss(src, (1.0, 1.0, 1.0), 3.0, (1, 1, -2))
    with pytest.raises(api.VisfdHipError):
        ctx.local_fluctuations_gen(src, (-1.0, 1.0, 1.0), 2.0, None, True, 6.0)
    import torch
    s = torch.from_numpy(src).cuda()
    two = torch.empty(2 * s.numel(), dtype=torch.float32, device="cuda")
    with pytest.raises(api.VisfdHipError):                               # partial overlap on the device face
        ctx.filter3d_dev(two[:s.numel()].view(s.shape), two[10:10 + s.numel()].view(s.shape), table)
    with pytest.raises(api.VisfdHipError):
        ctx.filter3d_dev(s, s, table)


def test_table_capacity_too_small():
    from visfd_amd import api
    L = api.load_library()
    n = C.c_int64()
    small = np.zeros(26, np.float32)
    rc = L.visfd_hip_gengauss3d_table(api._f3((1.0, 1.0, 1.0)), 3.0, api._i3((1, 1, 1)), small.ctypes.data_as(api._fp), 26,
                                      C.byref(n), None)
    assert rc == 4 and n.value == 27


def test_poisoned_workspace_changes_nothing(ctx):
    shape, hw = (9, 40, 130), (1, 6, 0)
    src = volgen.noise_volume(shape, seed=51)
    table = random_table(hw, 52)
    mask = make_mask(shape, "weighted", 53)
    a = ctx.filter3d(src, table, mask, True)
    ctx.debug_poison_workspace()
    b = ctx.filter3d(src, table, mask, True)       # the table in the workspace was forgotten and is sent again
    assert_bits_equal(a, b, "after poisoning the workspace")
    ctx.trim()
    assert_bits_equal(ctx.filter3d(src, table, mask, True), a, "after trimming the workspace")
    sg = (1.4, 1.4, 1.4)
    f = ctx.local_fluctuations_gen(src, sg, 1.5, mask, True, 6.0)
    ctx.debug_poison_workspace()
    assert_bits_equal(ctx.local_fluctuations_gen(src, sg, 1.5, mask, True, 6.0), f, "fluctuations after poisoning")


def _read_records(path):
    out = {}
    raw = open(path, "rb").read()
    pos = 0
    while pos < len(raw):
        tag = raw[pos:pos + 32].split(b"\0")[0].decode()
        (n,) = struct.unpack("<q", raw[pos + 32:pos + 40])
        out[tag] = np.frombuffer(raw, "<f4", n, pos + 40).copy()
        pos += 40 + 4 * n
    return out


def test_cpp_shim_filter3d(tmp_path):
    exe = str(tmp_path / "shim_filter3d_check")
    libdir = os.path.join(ROOT, "visfd_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "shim_filter3d_check.cpp"), "-o", exe, "-L" + libdir, "-lvisfd_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    shape = (11, 17, 70)
    nz, ny, nx = shape
    src = volgen.noise_volume(shape, seed=61)
    mask = make_mask(shape, "block", 62)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<3i", nx, ny, nz))
        f.write(src.tobytes())
        f.write(mask.tobytes())
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "shim filter3d check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    R = _read_records(tmp_path / "out.bin")
    vol = lambda k: R[k].reshape(shape)   # noqa: E731
    width, hw = (2.2, 1.1, 0.6), (4, 2, 1)
    t, A = FN.gengauss3d_table(width, 1.5, hw)
    assert_bits_equal(R["table"].reshape(t.shape), t, "shim table")
    assert_bits_equal(vol("ggauss_norm"), FN.apply(src, t, hw, None, True), "shim Apply, normalised")
    assert_bits_equal(vol("ggauss_mask_norm"), FN.apply(src, t, hw, mask, True), "shim Apply, mask, normalised")
    raw, den = FN.apply(src, t, hw, mask, False, want_den=True)
    assert_bits_equal(vol("ggauss_mask_raw"), raw, "shim Apply with a denominator")
    assert_bits_equal(vol("ggauss_mask_den"), den, "shim Apply: the denominator")
    q = np.zeros((5, 1, 3), np.float32)
    for jz in range(-2, 3):
        for jx in range(-1, 2):
            q[jz + 2, 0, jx + 1] = np.float32(np.float32(0.25 * jz) - np.float32(0.5 * jx)) + np.float32(0.125)
    own = FN.apply(src, q, (1, 0, 2), None, False)
    assert_bits_equal(vol("own_table"), own, "shim: a copied table")
    assert_bits_equal(vol("own_table_moved"), own, "shim: a moved table")   # + 1 - 1 is exact for these entries
    tot = np.float32(0)
    sq = np.float32(0)
    for v in q.reshape(-1):
        tot = np.float32(tot + v)
        sq = np.float32(sq + np.float32(v * v))
    n15 = np.float32(15)
    assert_bits_equal(R["sums"], np.array([tot, sq, tot / n15, sq / n15], np.float32), "shim: Sum, SumSqr, Average, AverageSqr")
    t3 = (t * np.float32(3)).astype(np.float32)
    tot = np.float32(0)
    for v in t3.reshape(-1):
        tot = np.float32(tot + v)
    assert_bits_equal(R["renormalized"].reshape(t.shape), (t3 / tot).astype(np.float32), "shim: MultiplyScalar, Normalize")
    sg = (1.4, 1.4, 1.4)
    assert_bits_equal(vol("fluct_m6_mask"), FN.local_fluctuations(src, sg, 6.0, 1.5, mask, True), "shim LocalFluctuations")
    from visfd_amd import api
    sg4, r4 = api.fluctuation_sigmas((3.0, 3.0, 3.0), 4.0, 1.3, 0.03)
    assert_bits_equal(vol("fluct_radius_m4"), FN.local_fluctuations(src, sg4, 4.0, r4, None, True),
                      "shim LocalFluctuationsByRadius")


def _run_cli(exe, args, cwd):
    r = subprocess.run([exe] + [str(a) for a in args], cwd=str(cwd), capture_output=True, text=True)
    assert r.returncode == 0, (exe, r.stderr[-2000:])
    return r.stderr


def _write_inputs(name, d):
    src, mask = FC.inputs(name)
    volgen.write_mrc(str(d / "in.rec"), src, voxel_width=1.0)
    args = ["-in", "in.rec", "-w", 1, "-out", "out.rec"] + FC.CASES[name][2]
    if mask is not None:
        volgen.write_mrc(str(d / "mask.rec"), mask, voxel_width=1.0)
        args += ["-mask", "mask.rec"]
    return args


@pytest.mark.parametrize("name", sorted(FC.CASES))
def test_cli_matches_reference_golden(tmp_path, name):
    """Every new flag spelling (-ggauss, -ggauss-aniso, -dogg, -dogg-aniso, -exponent, -gauss-exponent, -exponents,
    -gdog-exponents, -fluct with an exponent) through filter_mrc: the reference program's bits and its A / B."""
    g = np.load(GOLD)
    err = _run_cli(CLI, _write_inputs(name, tmp_path), tmp_path)
    assert_bits_equal(volgen.read_mrc(str(tmp_path / "out.rec")), g[name + "/out"], name)
    if FC.CASES[name][3][0] != "fluct":
        assert " Filter Used:\n" in err
        for k, letter in enumerate("AB"[: 2 if FC.CASES[name][3][0] == "dogg" else 1]):
            assert (" %s = %s\n" % (letter, "%g" % g[name + "/AB"][k])) in err, err


@pytest.mark.parametrize("name", ["ggauss_aniso", "dogg_threshold", "fluct_m6_mask"])
def test_cli_equals_reference_program(tmp_path, name):
    if not os.path.exists(REF_CLI):
        pytest.skip("oracle/_ref/filter_mrc_ref not built (needs the reference sources at build time)")
    outs = []
    for tag, exe in (("mine", CLI), ("ref", REF_CLI)):
        d = tmp_path / tag
        d.mkdir()
        _run_cli(exe, _write_inputs(name, d), d)
        outs.append(volgen.read_mrc(str(d / "out.rec")))
    assert_bits_equal(outs[0], outs[1], name)


def test_cli_dogg_with_mask_warns_and_writes_zero(tmp_path):
    src, _ = FC.inputs("dogg")
    mask = make_mask(src.shape, "block", 71)
    volgen.write_mrc(str(tmp_path / "in.rec"), src, voxel_width=1.0)
    volgen.write_mrc(str(tmp_path / "mask.rec"), mask, voxel_width=1.0)
    err = _run_cli(CLI, ["-in", "in.rec", "-w", 1, "-out", "out.rec", "-mask", "mask.rec", "-dogg", 1.2, 2.0, "-exponents",
                         2, 4, "-truncate", 2.5], tmp_path)
    assert err.count("the reference program crashes") == 1
    out = volgen.read_mrc(str(tmp_path / "out.rec"))
    t, hw, _, _ = FN.dogg3d_table((1.2,) * 3, (2.0,) * 3, 2.0, 4.0, 2.5)
    assert_bits_equal(out, FN.apply(src, t, hw, mask, False), "-dogg -mask")
    assert not out[mask == 0].any()
