"""The device-face methods of visfd_amd.api.Context that no other test calls, against the host face of the same
operation.  The two faces share one private marshal, so these cases catch a device face that parts from the host face -- a
wrong symbol suffix, a wrong pointer converter, a wrong destination -- and not an argument out of place in the shared
marshal, which moves both alike: the host face is held against the oracle elsewhere.  One (6, 9, 70) volume with a mask:
nx = 70 crosses one 64-wide tile edge."""
import ctypes as C

import numpy as np
import pytest

import volgen
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

SHAPE = (6, 9, 70)


@pytest.fixture(scope="module")
def ctx():
    from visfd_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def vol():
    return volgen.membrane_volume(SHAPE, seed=7), volgen.block_mask(SHAPE, seed=8)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _host(ctx, t):
    ctx.synchronize()   # the device face is asynchronous on the context's stream
    return t.cpu().numpy()


def test_local_fluctuations_gen_dev(ctx, vol):
    src, mask = vol
    want = ctx.local_fluctuations_gen(src, (1.0, 1.2, 0.8), 2.0, mask=mask, normalize=True, exponent=1.5)
    dst = _dev(np.zeros_like(src))
    assert ctx.local_fluctuations_gen_dev(_dev(src), dst, (1.0, 1.2, 0.8), 2.0, mask=_dev(mask), normalize=True,
                                          exponent=1.5) is None
    assert_bits_equal(_host(ctx, dst), want, "local_fluctuations_gen_dev")
    assert np.any(want != 0)


def test_apply_ggauss_dev(ctx, vol):
    src, mask = vol
    want, A = ctx.apply_ggauss(src, (1.5, 1.2, 1.0), 1.5, (3, 2, 2), mask=mask)
    dst = _dev(np.zeros_like(src))
    assert ctx.apply_ggauss_dev(_dev(src), dst, (1.5, 1.2, 1.0), 1.5, (3, 2, 2), mask=_dev(mask)) == A
    assert_bits_equal(_host(ctx, dst), want, "apply_ggauss_dev")
    assert np.any(want != 0)


def test_apply_dogg_dev(ctx, vol):
    src, mask = vol
    want, A, B = ctx.apply_dogg(src, (1, 1, 1), (1.6, 1.6, 1.6), 2.0, 2.0, mask=mask)
    dst = _dev(np.zeros_like(src))
    assert ctx.apply_dogg_dev(_dev(src), dst, (1, 1, 1), (1.6, 1.6, 1.6), 2.0, 2.0, mask=_dev(mask)) == (A, B)
    assert_bits_equal(_host(ctx, dst), want, "apply_dogg_dev")
    assert np.any(want != 0)


TABLE = (np.array([(0, 0, 0), (1, 0, 0), (-2, 1, 0), (0, -1, 1)], np.int32), np.array([0.0, -1.5, 2.0, 0.5], np.float32))


def test_morph_table_dev(ctx, vol):
    from visfd_amd import api
    src, mask = vol
    want = ctx.morph_table(api.MORPH_ERODE, src, TABLE[0], TABLE[1], mask=mask)
    dst = _dev(src)
    assert ctx.morph_table_dev(api.MORPH_ERODE, _dev(src), dst, TABLE[0], TABLE[1], mask=_dev(mask)) is None
    assert_bits_equal(_host(ctx, dst), want, "morph_table_dev")
    assert np.any(want != src)


def test_dilate_dev(ctx, vol):
    src, mask = vol
    want = ctx.dilate(src, TABLE[0], TABLE[1], mask=mask)
    dst = _dev(src)
    ctx.dilate_dev(_dev(src), dst, TABLE[0], TABLE[1], mask=_dev(mask))
    assert_bits_equal(_host(ctx, dst), want, "dilate_dev")
    assert np.any(want != src)


def test_membrane_stage_dev_is_membrane_detect_dev(ctx, vol):
    """pipeline.membrane_detect runs the stage through membrane_stage_dev on its own tensors and expects what
    membrane_detect_dev computes: the same scores, vote tensor, directions (over zeros) and threshold."""
    import torch
    from visfd_amd import api
    src, mask = vol
    ratio = api.ratio_from_threshold(0.03)
    got, want = [], []
    for out in (got, want):
        out += [torch.zeros(SHAPE, device="cuda:0"), torch.zeros((3,) + SHAPE, device="cuda:0"),
                torch.zeros((6,) + SHAPE, device="cuda:0")]
    tsrc, tmask = _dev(src), _dev(mask)
    thr = ctx.membrane_stage_dev(tsrc, got[0], got[1], got[2], torch.empty(SHAPE, device="cuda:0"), 1.0, ratio,
                                 api.DECREASING_EIVALS, 0.1, 2.0, 4, 2.0 ** 0.5, tmask)
    thr_want = ctx.membrane_detect_dev(tsrc, want[0], 1.0, ratio, api.DECREASING_EIVALS, 0.1, 0.0, 2.0, 4, 2.0 ** 0.5,
                                       mask=tmask, dirs=want[1], tensor=want[2])
    ctx.synchronize()
    assert thr == thr_want
    for g, w, what in zip(got, want, ("scores", "directions", "vote tensor")):
        assert_bits_equal(_host(ctx, g), _host(ctx, w), "membrane_stage_dev " + what)
        assert np.any(_host(ctx, w) != 0), what


@pytest.mark.parametrize("name,n,option", [("label_connected_graph", 8, "connect_time"),
                                           ("surface_points", 4, "surface_points_time")])
def test_last_times_readers(ctx, vol, name, n, option):
    """<name>_last_times() against a direct call of the same C entry after a timed call: this checks the few lines of the
    reader (the symbol it forms, the n floats it reads, the tuple it returns) and nothing else."""
    src, mask = vol
    sal = (src.max() - src).astype(np.float32)
    with ctx.options(**{option: 1}):
        if name == "label_connected_graph":
            ctx.label_connected_graph(sal, float(np.median(sal)), mask=mask)
        else:
            dirs = np.zeros(SHAPE + (3,), np.float32)
            dirs[..., 2] = 1
            ctx.surface_points(sal, dirs, mask=mask)
        got = getattr(ctx, name + "_last_times")()
        raw = (C.c_float * n)()
        assert getattr(ctx._L, "visfd_hip_%s_last_times" % name)(ctx._h, raw) == 0
    assert isinstance(got, tuple) and len(got) == n
    assert_bits_equal(np.array(got, np.float32), np.array(tuple(raw), np.float32), name + "_last_times")
