"""The top-fraction saliency cut without a GPU: the numpy reference (tests/select_np.py) against the oracle and the
compiled reference on every case of tests/select_cases.py, and the Python walk of visfd_amd/slab.py -- the k formula,
_pick_descending across three rounds, _key_to_float -- on the same cases, whole and cut into uneven shards whose
histograms are summed by hand.  Thresholds are compared as numbers (the reference does not define which of -0 and +0 it
returns), thresholded fields bit for bit."""
import types

import numpy as np
import pytest
import torch

import select_cases as SC
import select_np
from conftest import assert_bits_equal
from oracle_ops import OracleOps
from visfd_amd import slab

f32 = np.float32
WORLD1 = types.SimpleNamespace(world=1)


def _both_sides(lib, case):
    """One case through a compiled restatement (in place) against select_np."""
    thr, want = select_np.threshold_fraction(case.values, case.mask, case.fraction)
    got = case.values.copy()
    t = lib.threshold_fraction(got, case.fraction, case.mask)
    assert f32(t) == thr, (case.name, t, thr)
    assert_bits_equal(got, want, case.name)


@pytest.mark.parametrize("group", SC.GROUPS)
def test_oracle_equals_numpy(oracle, group):
    for case in SC.cases_of(group):
        _both_sides(oracle, case)


@pytest.mark.parametrize("group", SC.GROUPS)
def test_reference_equals_numpy(ref, group):
    for case in SC.cases_of(group):
        _both_sides(ref, case)


def _walk(ops, case):
    sal = torch.from_numpy(case.values)
    mask = None if case.mask is None else torch.from_numpy(case.mask)
    return slab.distributed_threshold_fraction(ops, sal, case.fraction, WORLD1, mask)


@pytest.mark.parametrize("group", SC.GROUPS)
def test_python_walk(oracle, group):
    ops = OracleOps()
    for case in SC.cases_of(group):
        thr, _ = select_np.threshold_fraction(case.values, case.mask, case.fraction)
        assert f32(_walk(ops, case)) == thr, case.name


class ShardedOps:
    """select_histogram_dev over a volume cut into uneven shards: one histogram per shard, summed here by hand (what the
    all-reduce does between ranks)."""

    def __init__(self, parts):
        self.ops, self.parts = OracleOps(), int(parts)

    def bounds(self, n):
        cuts = [0]
        for r in range(self.parts):      # shard r is (r + 1) / (1 + 2 + ... + parts) of the volume
            cuts.append(cuts[-1] + n * (r + 1) * 2 // (self.parts * (self.parts + 1)))
        cuts[-1] = n
        return cuts

    def select_histogram_dev(self, sal, rnd, prefix, mask=None):
        cuts = self.bounds(sal.numel())
        total, count = np.zeros(2048, np.uint64), 0
        for a, b in zip(cuts[:-1], cuts[1:]):
            if a == b:
                continue
            h, n = self.ops.select_histogram_dev(sal[a:b], rnd, prefix, None if mask is None else mask[a:b])
            total += h
            count += n
        whole, n = self.ops.select_histogram_dev(sal, rnd, prefix, mask)
        assert np.array_equal(total, whole) and count == n
        assert np.array_equal(whole, select_np.round_histogram(sal.numpy(), None if mask is None else mask.numpy(), rnd, prefix))
        return total, count


@pytest.mark.parametrize("parts", [2, 3, 5])
@pytest.mark.parametrize("group", SC.GROUPS)
def test_python_walk_over_shards(oracle, group, parts):
    ops = ShardedOps(parts)
    for case in SC.cases_of(group):
        thr, _ = select_np.threshold_fraction(case.values, case.mask, case.fraction)
        assert f32(_walk(ops, case)) == thr, case.name


@pytest.mark.parametrize("case", SC.REFUSALS, ids=[c.name for c in SC.REFUSALS])
def test_refusals(oracle, case):
    with pytest.raises(ValueError):
        select_np.threshold_fraction(case.values, case.mask, case.fraction)
    for ops in (OracleOps(), ShardedOps(3)):
        with pytest.raises(ValueError, match="selects no voxel"):
            _walk(ops, case)


@pytest.mark.parametrize("n", SC.BIG)
def test_above_2_24(oracle, n):
    """float32(n) != n: the k of the reference's float product, not the exact one."""
    v = SC.big_field(n)
    ops = OracleOps()
    for f in SC.BIG_FRACTIONS[n]:
        case = SC.Case("n=%d/f=%.9g" % (n, f), v, None, f)
        thr, want = select_np.threshold_fraction(v, None, f)
        k, ke = select_np.rank_k(n, f), SC._exact_k(n, f)
        if k != ke:     # the case tells the two products apart: the entry the exact product picks holds another value
            assert np.partition(v, n - 1 - ke)[n - 1 - ke] != thr
        got = v.copy()
        assert f32(oracle.threshold_fraction(got, f)) == thr
        assert_bits_equal(got, want, case.name)
        assert f32(_walk(ops, case)) == thr
    assert f32(_walk(ShardedOps(3), case)) == thr


def test_reference_above_2_24(ref):
    n = SC.BIG[1]
    v = SC.big_field(n)
    thr, want = select_np.threshold_fraction(v, None, 0.5)
    assert f32(ref.threshold_fraction(v, 0.5)) == thr
    assert_bits_equal(v, want, "n=%d" % n)


def test_keys_and_their_inverse():
    """order_key is monotone over every kind of float, and slab._key_to_float inverts it bit for bit."""
    v = np.array([-np.inf, -3e38, -1.5, -1e-38, -1e-45, -0.0, 0.0, 1e-45, 1e-38, 1.5, 3e38, np.inf], f32)
    key = select_np.order_key(v)
    assert (np.diff(key.astype(np.int64)) > 0).all()
    for c in SC.CASES[::9]:
        for x, k in zip(c.values[:64], select_np.order_key(c.values[:64])):
            back = f32(slab._key_to_float(int(k)))
            assert back.tobytes() == x.tobytes() or (np.isnan(back) and np.isnan(x))
