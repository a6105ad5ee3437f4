"""Two-level morphology (csrc/morph_levels.hip), the parts that need no GPU: the flat ball as a threshold on the squared
length of an offset, and the definition the GPU path is tested against (tests/morph_levels_np.py) bit for bit against
the numpy restatement of the reference's element walk (tests/morph_np.py)."""
import numpy as np
import pytest

import morph_levels_np as ml
import morph_np
from conftest import assert_bits_equal

SQRT2 = np.float32(np.sqrt(2.0))
# the float32 on either side of the real square root of 2 (the lower one is float32(sqrt(2.0)), the value an offset of
# squared length 2 is compared with), and the one below them
SQRT2_NEIGHBOURS = [float(np.nextafter(SQRT2, np.float32(0))), float(SQRT2), float(np.nextafter(SQRT2, np.float32(2)))]
KNOWN_T = {0: 0, 0.5: 0, 1: 1, 2.5: 6, 4: 16, 10: 100, 13: 169, 13.5: 182, 30.2: 912}


@pytest.mark.parametrize("radius", [0, 0.5, 0.99, 1] + SQRT2_NEIGHBOURS + [2.5, 4, 10, 13, 13.5, 30.2])
def test_flat_ball_is_a_threshold_on_the_squared_length(radius):
    from visfd_amd import api
    d, b = api.sphere_structure(radius)
    assert not b.view(np.uint32).any()
    dsq = (d.astype(np.int64) ** 2).sum(axis=1)
    t = api.flat_ball_dsq_max(radius)
    assert t == int(dsq.max())
    assert t == ml.t_max(radius)
    if radius in KNOWN_T:
        assert t == KNOWN_T[radius]
    # membership is exactly d^2 <= t: the element holds every offset of the cube that passes, and no other
    R = int(np.ceil(radius))
    g = np.arange(-R, R + 1, dtype=np.int64)
    cube = g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2
    assert int((cube <= t).sum()) == len(b) and int(dsq.max()) <= t


def test_threshold_steps_at_the_rounded_root():
    from visfd_amd import api
    assert SQRT2_NEIGHBOURS[1] < 2.0 ** 0.5 < SQRT2_NEIGHBOURS[2]
    assert [api.flat_ball_dsq_max(r) for r in SQRT2_NEIGHBOURS] == [1, 2, 2]


@pytest.mark.parametrize("radius", [128.5, 1000])
def test_flat_ball_threshold_beyond_the_element_cap(radius):
    from visfd_amd import api
    assert api.flat_ball_dsq_max(radius) == ml.t_max(radius)
    with pytest.raises(api.VisfdHipError):
        api.sphere_structure(radius)


def test_flat_ball_threshold_rejects_bad_radii():
    from visfd_amd import api
    for r in (-1.0, float("nan"), float("inf")):
        with pytest.raises(api.VisfdHipError):
            api.flat_ball_dsq_max(r)
    assert api.flat_ball_dsq_max(3.0e38) == 1 << 62   # saturates


CASES = [((1, 1, 1), 4.0), ((3, 3, 3), 4.0), ((9, 20, 70), 2.5), ((9, 20, 70), 13.0)]


def _assert_nan_aware(got, want, what):
    wn = np.isnan(want)
    assert np.array_equal(np.isnan(got), wn), what
    assert_bits_equal(np.where(wn, 0, got).astype(np.float32), np.where(wn, 0, want).astype(np.float32), what)


@pytest.mark.parametrize("levels", ml.LEVEL_SETS, ids=lambda lv: "/".join("%g" % v for v in lv).replace("-0", "m0"))
@pytest.mark.parametrize("shape,radius", CASES)
def test_definition_equals_the_element_walk(shape, radius, levels):
    """levels_op against morph_np.sphere_op: six ops, with and without a mask.  The image mixes a block with scattered
    voxels so that at radius 13 neither level swallows the other."""
    src = ml.level_image(shape, levels, "block", seed=3)
    src[ml.seeds(shape, "sparse", seed=4)] = levels[-1]
    dst0 = np.random.default_rng(5).normal(0, 5, shape).astype(np.float32)
    mask, src_m = ml.mask_with_garbage(src, seed=6)
    for m, s in ((None, src), (mask, src_m)):
        for op, name in enumerate(ml.OPS):
            got = ml.levels_op(op, s, radius, mask=m, dst=dst0)
            want = morph_np.sphere_op(op, s, radius, mask=m, dst=dst0)
            what = "%s %s R=%g levels=%s mask=%s" % (name, shape, radius, levels, m is not None)
            if name in ("white", "black"):
                _assert_nan_aware(got, want, what)
            else:
                assert_bits_equal(got, want, what)
