"""Two-level morphology on the GPU (csrc/morph_levels.hip): flat balls on images of at most two levels as a threshold on
the exact distance map.  Parity is bitwise against the general element walk of the same library (option morph_general),
the fall-backs against the numpy restatement of the reference (tests/morph_np.py), radii beyond the element cap against
the definition (tests/morph_levels_np.py, which tests/test_morph_levels.py ties to the element walk)."""
import os
import subprocess

import numpy as np
import pytest

import morph_levels_np as ml
import morph_np
import volgen
from conftest import GOLDEN, ROOT, assert_bits_equal

pytestmark = pytest.mark.gpu

EINVAL = 1   # VISFD_HIP_EINVAL


@pytest.fixture(scope="module")
def ctx():
    from visfd_amd import api
    c = api.Context(0)
    yield c
    c.close()


def assert_nan_aware(got, want, what):
    wn = np.isnan(want)
    assert np.array_equal(np.isnan(got), wn), what
    assert_bits_equal(np.where(wn, 0, got).astype(np.float32), np.where(wn, 0, want).astype(np.float32), what)


def parity(ctx, shape, radius, op, levels, pattern, with_mask, seed):
    """One call on the levels path against the same call on the element walk."""
    from visfd_amd import api
    src = ml.level_image(shape, levels, pattern, seed)
    mask = None
    if with_mask:
        mask, src = ml.mask_with_garbage(src, seed + 1)
    dst0 = np.random.default_rng(seed + 2).normal(0, 5, shape).astype(np.float32)
    what = "%s %s R=%g levels=%s %s mask=%s" % (ml.OPS[op], shape, radius, levels, pattern, with_mask)
    with ctx.options(morph_levels=2):
        got = ctx.morph_sphere(op, src, radius, mask=mask, dst=dst0)
        assert ctx.morph_last_path() == api.MORPH_PATH_LEVELS, what
    with ctx.options(morph_general=1):
        want = ctx.morph_sphere(op, src, radius, mask=mask, dst=dst0)
        assert ctx.morph_last_path() == api.MORPH_PATH_GENERAL, what
    if ml.OPS[op] in ("white", "black"):
        assert_nan_aware(got, want, what)
    else:
        assert_bits_equal(got, want, what)
    if mask is not None:
        assert_bits_equal(got[mask == 0], dst0[mask == 0], what + " (masked voxels keep dst)")


@pytest.mark.parametrize("radius", [0, 0.5, 1, 2.5, 4])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 40, 37), (5, 1, 64), (3, 3, 3)])
def test_levels_path_equals_element_walk_small(ctx, shape, radius):
    """Every op, level set, seed pattern and mask state at the small shapes."""
    for op in range(6):
        for li, levels in enumerate(ml.LEVEL_SETS):
            for pi, pattern in enumerate(ml.PATTERNS):
                for with_mask in (False, True):
                    parity(ctx, shape, radius, op, levels, pattern, with_mask, seed=100 * li + 10 * pi + op)


@pytest.mark.parametrize("ri,radius", list(enumerate([2.5, 13, 30.2])))
def test_levels_path_equals_element_walk_long_rows(ctx, ri, radius):
    """(40, 70, 300): x runs past 256 lanes and ends inside a chunk of 64.  The full product of ops, level sets, seed
    patterns and mask states would take most of a minute at radius 30.2 on the element walk's side, so each radius takes
    24 combinations: every op with every seed pattern, the level sets and the mask state rotating through them, and the
    three radii rotating differently."""
    shape = (40, 70, 300)
    for k in range(24):
        op, pi = k % 6, k // 6
        levels = ml.LEVEL_SETS[(k + pi + 2 * ri) % 6]
        with_mask = (k + pi + ri) % 2 == 1
        parity(ctx, shape, radius, op, levels, ml.PATTERNS[pi], with_mask, seed=1000 + 100 * ri + k)


FALLBACK_SHAPE = (9, 20, 70)


def _fallback_images():
    shape = FALLBACK_SHAPE
    two = ml.level_image(shape, (0.0, 1.0), "half", 7)
    three = two.copy()
    three[2, 3, 4] = 2.0
    with_nan = two.copy()
    with_nan[8, 19, 69] = np.nan          # the last voxel: met by the sweep's tail
    zeros = np.where(ml.seeds(shape, "half", 8), np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    return {"three levels": three, "nan": with_nan, "signed zeros": zeros}


@pytest.mark.parametrize("name", ["three levels", "nan", "signed zeros"])
def test_ineligible_images_fall_back(ctx, name):
    from visfd_amd import api
    src = _fallback_images()[name]
    mask, src_m = ml.mask_with_garbage(src, 9)
    # the same ineligible voxel must stay visible under the mask
    mask[2, 3, 4] = mask[8, 19, 69] = 1.0
    src_m[2, 3, 4], src_m[8, 19, 69] = src[2, 3, 4], src[8, 19, 69]
    with ctx.options(morph_levels=2):
        for m, s in ((None, src), (mask, src_m)):
            for op in (api.MORPH_DILATE, api.MORPH_ERODE, api.MORPH_OPEN):
                got = ctx.morph_sphere(op, s, 2.5, mask=m)
                assert ctx.morph_last_path() != api.MORPH_PATH_LEVELS, name
                want = morph_np.sphere_op(op, s, 2.5, mask=m)
                what = "%s op %d mask=%s" % (name, op, m is not None)
                if name == "nan":
                    assert_nan_aware(got, want, what)
                else:
                    assert_bits_equal(got, want, what)


def test_census_merges_the_waves_patterns(ctx):
    """Images whose tiles of 1024 voxels each hold one level, so that no wave sees more than one pattern: two levels
    are eligible, a third one or the other zero is met only where the waves put their patterns into the record."""
    from visfd_amd import api
    shape = FALLBACK_SHAPE                      # 12600 voxels: twelve whole tiles and a part
    idx = np.arange(int(np.prod(shape))).reshape(shape)
    tiles = idx // 4096                          # 0, 1, 2, 3
    images = {
        "two": (np.where(tiles % 2 == 0, 0.0, 1.0), True),
        "three": (np.choose(np.minimum(tiles, 2), [0.0, 1.0, 2.0]), False),
        "zeros": (np.where(tiles % 2 == 0, 0.0, -0.0), False),
    }
    with ctx.options(morph_levels=2):
        for name, (img, eligible) in images.items():
            src = img.astype(np.float32)
            for op in (api.MORPH_DILATE, api.MORPH_ERODE):
                got = ctx.morph_sphere(op, src, 2.5)
                assert (ctx.morph_last_path() == api.MORPH_PATH_LEVELS) == eligible, name
                assert_bits_equal(got, morph_np.sphere_op(op, src, 2.5), "%s op %d" % (name, op))


def test_ineligible_calls_fall_back(ctx):
    from visfd_amd import api
    src = ml.level_image(FALLBACK_SHAPE, (0.0, 1.0), "half", 7)
    for opts, bmax in (({"morph_levels": 2}, 3.0), ({"morph_levels": 0}, 0.0), ({"morph_levels": 2, "morph_general": 1}, 0.0)):
        with ctx.options(**opts):
            for op in (api.MORPH_DILATE, api.MORPH_ERODE, api.MORPH_CLOSE):
                got = ctx.morph_sphere(op, src, 2.5, 0.0, bmax)
                assert ctx.morph_last_path() != api.MORPH_PATH_LEVELS, (opts, bmax)
                assert_bits_equal(got, morph_np.sphere_op(op, src, 2.5, 0.0, bmax), "%s bmax=%g op %d" % (opts, bmax, op))
    # the distance transform's limit: nx + ny + nz = 46343
    shape = (1, 1, 46341)
    row = ml.level_image(shape, (0.0, 1.0), "sparse", 11)
    with ctx.options(morph_levels=2):
        for op in (api.MORPH_DILATE, api.MORPH_ERODE):
            got = ctx.morph_sphere(op, row, 2.5)
            assert ctx.morph_last_path() != api.MORPH_PATH_LEVELS
            assert_bits_equal(got, morph_np.sphere_op(op, row, 2.5), "long row op %d" % op)
        ok = ml.level_image((1, 1, 46338), (0.0, 1.0), "sparse", 11)   # 46340: the last eligible sum
        got = ctx.morph_sphere(api.MORPH_DILATE, ok, 2.5)
        assert ctx.morph_last_path() == api.MORPH_PATH_LEVELS
        assert_bits_equal(got, morph_np.sphere_op(0, ok, 2.5), "row of 46338")


def test_default_mode_takes_the_path_beyond_the_xrun_cap(ctx):
    from visfd_amd import api
    assert ctx.get_option("morph_levels") == int(os.environ.get("VISFD_HIP_MORPH_LEVELS", "1"))
    shape = (20, 30, 70)
    two = ml.level_image(shape, (0.0, 1.0), "sparse", 21)
    noise = np.random.default_rng(22).normal(0, 1, shape).astype(np.float32)
    with ctx.options(morph_levels=1):
        got = ctx.morph_sphere(api.MORPH_DILATE, two, 13)
        assert ctx.morph_last_path() == api.MORPH_PATH_LEVELS
        with ctx.options(morph_levels=0):
            assert_bits_equal(got, ctx.morph_sphere(api.MORPH_DILATE, two, 13), "mode 1 at radius 13")
            assert ctx.morph_last_path() == api.MORPH_PATH_GENERAL
        ctx.morph_sphere(api.MORPH_DILATE, noise, 13)
        assert ctx.morph_last_path() == api.MORPH_PATH_GENERAL
        ctx.morph_sphere(api.MORPH_DILATE, two, 4)       # below R0 = 5: the X-run kernel, without a census
        assert ctx.morph_last_path() == api.MORPH_PATH_XRUNS
        ctx.morph_sphere(api.MORPH_DILATE, two, 5)
        assert ctx.morph_last_path() == api.MORPH_PATH_LEVELS


@pytest.mark.parametrize("radius", [129, 200.5])
def test_radii_beyond_the_element_cap(ctx, radius):
    from visfd_amd import api
    shape = (6, 9, 300)
    # level 1 at scattered voxels with x < 40 and in a corner; eroded: its complement, so that the spreading level is
    # the scattered one both times and the far end of the rows lies beyond the radius
    ones = ml.seeds(shape, "sparse", 31) | ml.seeds(shape, "corner", 31)[:, :, ::-1]
    ones[:, :, 40:] = False
    dst0 = np.random.default_rng(33).normal(0, 5, shape).astype(np.float32)
    with ctx.options(morph_levels=2):
        for op in (api.MORPH_DILATE, api.MORPH_ERODE):
            src = np.where(ones == (op == api.MORPH_DILATE), np.float32(1.0), np.float32(0.0)).astype(np.float32)
            mask, src_m = ml.mask_with_garbage(src, 32)
            got = ctx.morph_sphere(op, src_m, radius, mask=mask, dst=dst0)
            assert ctx.morph_last_path() == api.MORPH_PATH_LEVELS
            want = ml.levels_op(op, src_m, radius, mask=mask, dst=dst0)
            assert_bits_equal(got, want, "R=%g op %d" % (radius, op))
            assert len(np.unique(got[mask != 0])) == 2, "the radius reaches every voxel: the case shows nothing"
        noise = np.random.default_rng(34).normal(0, 1, shape).astype(np.float32)
        for mode in (2, 1, 0):
            with ctx.options(morph_levels=mode):
                with pytest.raises(api.VisfdHipError) as e:
                    ctx.morph_sphere(api.MORPH_DILATE, noise, radius)
                assert e.value.code == EINVAL


def test_device_face_equals_host_face(ctx):
    import torch
    shape = (17, 26, 31)
    src = ml.level_image(shape, (-0.0, 1.0), "sparse", 41)
    mask, src_m = ml.mask_with_garbage(src, 42)
    dst0 = np.random.default_rng(43).normal(0, 5, shape).astype(np.float32)
    from visfd_amd import api
    with ctx.options(morph_levels=2):
        for op in range(6):
            for m, s in ((None, src), (mask, src_m)):
                td, ts = torch.from_numpy(dst0.copy()).cuda(), torch.from_numpy(s).cuda()
                tmk = None if m is None else torch.from_numpy(m).cuda()
                ctx.morph_sphere_dev(op, ts, td, 3.0, mask=tmk)
                ctx.synchronize()
                assert ctx.morph_last_path() == api.MORPH_PATH_LEVELS
                want = ctx.morph_sphere(op, s, 3.0, mask=m, dst=dst0)
                assert ctx.morph_last_path() == api.MORPH_PATH_LEVELS
                if op >= 4:
                    assert_nan_aware(td.cpu().numpy(), want, "dev op %d" % op)
                else:
                    assert_bits_equal(td.cpu().numpy(), want, "dev op %d" % op)
        # tensors that do not start on a 16-byte boundary: the census' one-float sweep
        n = src.size
        buf_s, buf_m = torch.zeros(n + 1, device="cuda"), torch.zeros(n + 3, device="cuda")
        ts, tm = buf_s[1:].view(shape), buf_m[3:].view(shape)
        ts.copy_(torch.from_numpy(src_m))
        tm.copy_(torch.from_numpy(mask))
        td = torch.from_numpy(dst0.copy()).cuda()
        ctx.morph_sphere_dev(api.MORPH_ERODE, ts, td, 3.0, mask=tm)
        ctx.synchronize()
        assert ctx.morph_last_path() == api.MORPH_PATH_LEVELS
        assert_bits_equal(td.cpu().numpy(), ctx.morph_sphere(api.MORPH_ERODE, src_m, 3.0, mask=mask, dst=dst0), "unaligned")


CLI = os.path.join(ROOT, "visfd_amd", "cli", "filter_mrc")
REF_CLI = os.path.join(ROOT, "oracle", "_ref", "filter_mrc_ref")
BLOB_MASK = os.path.join(GOLDEN, "test_blob_detect_mask.rec")


@pytest.fixture(scope="module")
def ref_cli():
    if not os.path.exists(REF_CLI):
        pytest.skip("oracle/_ref/filter_mrc_ref not built (needs the reference sources at build time)")
    return REF_CLI


@pytest.mark.parametrize("flags", [["-dilate", 3], ["-erode", 13], ["-open", 4], ["-close", 4]])
def test_cli_on_a_mask_image_equals_reference_program(ref_cli, tmp_path, flags):
    """A 0/1 image (22 x 32 x 27) through both programs; this one with the levels path wherever it is eligible."""
    img = volgen.read_mrc(BLOB_MASK)
    assert set(np.unique(img).tolist()) == {0.0, 1.0}
    outs = []
    for tag, exe, env in (("mine", CLI, dict(os.environ, VISFD_HIP_MORPH_LEVELS="2")), ("ref", ref_cli, None)):
        d = tmp_path / tag
        d.mkdir()
        r = subprocess.run([exe, "-in", BLOB_MASK, "-w", "1"] + [str(a) for a in flags] + ["-out", "out.rec"], cwd=str(d),
                           capture_output=True, text=True, env=env)
        assert r.returncode == 0, (tag, r.stderr[-2000:])
        outs.append(d / "out.rec")
    assert_bits_equal(volgen.read_mrc(str(outs[0])), volgen.read_mrc(str(outs[1])), " ".join(map(str, flags)))
