"""What a context carries BETWEEN calls: workspace slots shared by unrelated stages (freed and reallocated when a later
call needs more), the tables kept inside slots (vote table, structuring element, median footprint, filter entries),
visfd_hip_trim, the option table, and blob jobs that are begun, left pending while other calls of the same context run, and
ended later.

A. a blob job times everything that may happen between its halves: the lists of the oracle, bit for bit;
B. job lifetime through the C ABI: refused arguments, capacity retries, destroy / close with a live job, stale handles;
C. no stage depends on what its slots held before: one context, every stage, oversized slots, three orders, with the
   workspace poisoned (visfd_hip_debug_poison_workspace) before every call, trimmed before every third, or left alone;
   tables of equal size one after the other, and a table slot that grows;
D. every field of the option struct answers to its name.

References: the CPU oracle (and tests/morph_np.py for morphology), bit for bit, for every stage whose arithmetic is plain
IEEE float; the suite's 1e-5 of the field's scale (conftest.assert_close_rel, per-voxel bound of test_tolerance_modes.py)
for the tolerance modes.  Stages that go through device libm (the eigen solver) or have no oracle entry (vote weight sums,
checked against a direct sum in test_tolerance_modes.py) are deterministic on the device: their reference for
state-independence is the same call on a FRESH context, bit for bit, with the oracle at the suite's 1e-5 where it has the
stage."""
import ctypes as C

import numpy as np
import pytest

import filter3d_np
import median_np
import morph_np
import volgen
from conftest import assert_bits_equal, assert_close_rel
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

TOL, PV = 1e-5, 0.005     # tests/test_tolerance_modes.py
BLOB_SHAPE = (40, 44, 48)
BLOB_SIG = np.array([1.2, 1.5, 1.9, 2.4, 3.0, 3.7], np.float32)
EINVAL, ECAPACITY = 1, 4


@pytest.fixture
def ctx():
    """A fresh context per test: every slot has the size this test's own calls gave it."""
    from visfd_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _empty(shape, fill=None):
    import torch
    t = torch.empty(tuple(shape), device="cuda:0") if fill is None else torch.full(tuple(shape), float(fill), device="cuda:0")
    torch.cuda.synchronize()   # the context runs on a stream of its own
    return t


def _host(ctx, t):
    ctx.synchronize()
    return t.cpu().numpy()


def _same_lists(got, want, what):
    assert_bits_equal(volgen.sort_blobs(got[0], True), volgen.sort_blobs(want[0], True), "minima, " + what)
    assert_bits_equal(volgen.sort_blobs(got[1], False), volgen.sort_blobs(want[1], False), "maxima, " + what)


# ============================================================================================ A. between the halves
@pytest.fixture(scope="module")
def blob_case(oracle):
    src = volgen.blob_volume(BLOB_SHAPE, seed=31, nblobs=60)
    want = oracle.blob_dog(src, BLOB_SIG, None, None, 0.02, 2.5)
    assert len(want[0]) + len(want[1]) > 40
    return src, want


class _Job:
    """begin ... end around a with-block: an exception inside the block aborts the job instead of running into `end`."""

    def __init__(self, ctx, src, begin_opts=None, end_opts=None):
        self.ctx, self.src, self.begin_opts, self.end_opts = ctx, src, begin_opts or {}, end_opts or {}

    def __enter__(self):
        assert self.ctx.blob_jobs_pending() == 0
        with self.ctx.options(**self.begin_opts):
            self.job = self.ctx.blob_dog_begin_dev(self.src, BLOB_SIG, None, None, 0.02, 2.5)
        assert self.ctx.blob_jobs_pending() == 1
        return self

    def __exit__(self, etype, e, tb):
        if etype is not None:
            self.ctx.blob_dog_abort(self.job)
            return False
        with self.ctx.options(**self.end_opts):
            self.got = self.ctx.blob_dog_end(self.job)
        assert self.ctx.blob_jobs_pending() == 0
        return False


def _between_nothing(ctx, oracle):
    pass


def _between_trim(ctx, oracle):
    ctx.trim()
    assert ctx.workspace_bytes() == 0
    assert ctx.blob_jobs_pending() == 1


def _between_poison(ctx, oracle):
    before = ctx.workspace_bytes()
    ctx.debug_poison_workspace()
    assert ctx.workspace_bytes() == before and before > 0


def _between_other_blob(ctx, oracle):
    """a one-call detector of the same size, other source: launches into the same buffer sets and counters"""
    other = volgen.blob_volume(BLOB_SHAPE, seed=77, nblobs=40)
    _same_lists(ctx.blob_dog_dev(_dev(other), BLOB_SIG, None, None, 0.02, 2.5), oracle.blob_dog(other, BLOB_SIG, None, None, 0.02, 2.5),
                "the one-call detector between the halves")


def _between_stages(ctx, oracle):
    """morphology (flat r = 2: X-run kernel; r = 13: element walk), a masked Gaussian, a radix select, exact and tolerance-
    mode voting with half-widths no earlier call of the context had: each checked, all between the halves"""
    from visfd_amd import api
    shape = (22, 26, 30)
    src = volgen.noise_volume(shape, seed=5)
    mask = volgen.block_mask(shape, seed=6)
    for r in (2.0, 13.0):
        d = _empty(shape)
        ctx.dilate_sphere_dev(_dev(src), d, r)
        assert_bits_equal(_host(ctx, d), morph_np.sphere_op(api.MORPH_DILATE, src, r), "dilate r=%g between the halves" % r)
    d = _empty(shape)
    ctx.gauss_dev(_dev(src), d, (1.5, 1.5, 1.5), (3, 3, 3), _dev(mask))
    assert_bits_equal(_host(ctx, d), oracle.gauss_hw(src, (1.5, 1.5, 1.5), (3, 3, 3), mask)[0], "masked Gaussian between the halves")
    sal, dirs = _sparse_field(shape, 9)
    s = _dev(sal)
    want = sal.copy()
    thr_o = oracle.threshold_fraction(want, 0.3)
    assert np.float32(ctx.threshold_fraction_dev(s, 0.3)) == np.float32(thr_o)
    assert_bits_equal(_host(ctx, s), want, "threshold_fraction_dev between the halves")
    dp = _dev(np.moveaxis(dirs, -1, 0))
    for sigma_tv, fma in ((5.0, 0), (4.3, 1)):     # h = 7 and h = 6
        ten = _empty((6,) + shape)
        with ctx.options(tv_fma=fma):
            ctx.tv_dense_stick_dev(s, dp, ten, sigma_tv, 4, 2.0 ** 0.5)
        got = np.moveaxis(_host(ctx, ten), 0, -1)
        ref = oracle.tv_dense_stick(want, dirs, sigma_tv, 4, 2.0 ** 0.5)
        if fma:
            assert_close_rel(got, ref, TOL, "tv_fma between the halves", pervoxel=PV)
        else:
            assert_bits_equal(got, ref, "exact voting between the halves")


@pytest.mark.parametrize("begin_opts,end_opts,between", [
    ({}, {}, _between_nothing),
    ({}, {}, _between_trim),
    ({}, {}, _between_poison),
    ({"blob_test_cap": 8}, {}, _between_nothing),
    ({"blob_test_cap": 24}, {}, _between_nothing),
    ({}, {"blob_test_cap": 8}, _between_nothing),
    ({}, {"blob_test_cap": 24}, _between_nothing),
    ({"blob_test_cap": 8}, {}, _between_trim),
    ({"blob_test_cap": 8}, {}, _between_poison),
    ({}, {}, _between_other_blob),
    ({"blob_test_cap": 24}, {}, _between_other_blob),
    ({}, {}, _between_stages),
], ids=lambda v: v.__name__[9:] if callable(v) else ("-".join("%s%d" % (k[-3:], x) for k, x in v.items()) or "std"))
def test_blob_job_survives_what_happens_between_its_halves(ctx, oracle, blob_case, begin_opts, end_opts, between):
    """An option scope that ends (or begins) between the halves, trim, poison, another detector call, other stages: a
    pending scan keeps the buffers and capacities of its launch, and whatever frees or overwrites them collects it first."""
    src_h, want = blob_case
    with _Job(ctx, _dev(src_h), begin_opts, end_opts) as j:
        between(ctx, oracle)
    _same_lists(j.got, want, "job with %s / %s around %s" % (begin_opts, end_opts, between.__name__))


@pytest.mark.parametrize("begin_opts", [{}, {"blob_test_cap": 8}], ids=["plain", "cap8"])
def test_blob_job_survives_growth_of_the_candidate_slot_by_a_membrane_stage(ctx, oracle, blob_case, begin_opts):
    """A membrane stage with dir = NULL takes 3n floats in WS_TVAUX, the slot of the scans' candidate codes: on 208^3 that is
    more than the 96 MiB the job's three buffer sets took, so the slot is freed and reallocated between the halves.  (The
    capacities `end` compares the counts with used to be recomputed from the grown slot: with `begin` under a small
    blob_test_cap, overflows of the pending scales then went unseen and their lists came back cut short.)"""
    from visfd_amd import api
    src_h, want = blob_case
    n = 208
    import torch
    g = torch.Generator(device="cuda:0").manual_seed(11)
    big = torch.randn((n, n, n), device="cuda:0", generator=g) * 100.0 + 1000.0
    sal = _empty((n, n, n))
    with _Job(ctx, _dev(src_h), begin_opts) as j:
        before = ctx.workspace_bytes()
        assert 3 * 4 * n ** 3 > 3 * (1 << 22) * 8
        thr = ctx.membrane_detect_dev(big, sal, 1.5, api.ratio_from_threshold(0.03), api.DECREASING_EIVALS, 0.05, 0.0, 3.0)
        ctx.synchronize()
        assert thr > 0 and ctx.workspace_bytes() > before + 3 * 4 * n ** 3 - 3 * (1 << 22) * 8
        assert bool(torch.isfinite(sal).all()) and int((sal != 0).sum()) > 0
    _same_lists(j.got, want, "job around a membrane stage that grows WS_TVAUX, begin under %s" % begin_opts)


def test_blob_job_survives_growth_of_the_survivor_slot_by_a_larger_blob_call(ctx, oracle, blob_case):
    """The one large case: a one-call detector on 528 x 512 x 512 between the halves needs more than 2^20 survivors per set
    (nvox / 128), so WS_CAND -- where the small job's pending survivors are -- is freed and reallocated.  The large call's
    own lists equal those of the same call on a fresh context."""
    import torch
    from visfd_amd import api
    src_h, want = blob_case
    shape = (528, 512, 512)
    assert shape[0] * shape[1] * shape[2] // 128 > 1 << 20
    g = torch.Generator(device="cuda:0").manual_seed(3)
    big = torch.randn(shape, device="cuda:0", generator=g) * 100.0 + 1000.0
    torch.cuda.synchronize()
    sig3 = np.array([2.0, 2.5, 3.1], np.float32)
    with _Job(ctx, _dev(src_h)) as j:
        got_big = ctx.blob_dog_dev(big, sig3, None, None, 0.02, 2.5, cap=1 << 20)
        assert len(got_big[0]) > 0 and len(got_big[1]) > 0
    _same_lists(j.got, want, "small job around a detector call that grows WS_CAND")
    ctx.trim()
    fresh = api.Context(0)
    try:
        want_big = fresh.blob_dog_dev(big, sig3, None, None, 0.02, 2.5, cap=1 << 20)
    finally:
        fresh.close()
    _same_lists(got_big, want_big, "the large call itself vs a fresh context")


@pytest.mark.parametrize("first_ends_first", [True, False])
def test_two_blob_jobs_of_one_context(ctx, oracle, blob_case, first_ends_first):
    src_h, want = blob_case
    other_h = volgen.blob_volume(BLOB_SHAPE, seed=77, nblobs=40)
    want2 = oracle.blob_dog(other_h, BLOB_SIG, None, None, 0.02, 2.5)
    a = ctx.blob_dog_begin_dev(_dev(src_h), BLOB_SIG, None, None, 0.02, 2.5)
    try:
        b = ctx.blob_dog_begin_dev(_dev(other_h), BLOB_SIG, None, None, 0.02, 2.5)
    except Exception:
        ctx.blob_dog_abort(a)
        raise
    assert ctx.blob_jobs_pending() == 2
    try:
        got = {}
        for k in ((0, 1) if first_ends_first else (1, 0)):
            got[k] = ctx.blob_dog_end((a, b)[k])
    finally:
        ctx.blob_dog_abort(a)
        ctx.blob_dog_abort(b)
    assert ctx.blob_jobs_pending() == 0
    _same_lists(got[0], want, "first of two jobs")
    _same_lists(got[1], want2, "second of two jobs")


# ============================================================================================ B. job lifetime
def _raw_begin(L, h, src):
    job = C.c_void_p()
    nz, ny, nx = src.shape
    rc = L.visfd_hip_blob_dog_begin_dev(h, C.c_void_p(src.data_ptr()), None, nx, ny, nz, BLOB_SIG.ctypes.data_as(C.POINTER(C.c_float)),
                                        len(BLOB_SIG), None, 0.02, 2.5, float("inf"), float("-inf"), 0, C.byref(job))
    assert rc == 0 and job.value
    return job


def _raw_end(L, job, cap, null_counts=False):
    from visfd_amd import api
    amin, amax = np.empty(max(cap, 1), api._BLOB_DTYPE), np.empty(max(cap, 1), api._BLOB_DTYPE)
    nmin, nmax = C.c_int64(-1), C.c_int64(-1)
    rc = L.visfd_hip_blob_dog_end(job, amin.ctypes.data_as(C.POINTER(api.Blob)), cap, None if null_counts else C.byref(nmin),
                                  amax.ctypes.data_as(C.POINTER(api.Blob)), cap, C.byref(nmax))
    return rc, amin, amax, nmin.value, nmax.value


def test_blob_job_lifetime_through_the_c_abi(ctx, oracle, blob_case):
    from visfd_amd import api
    L = api.load_library()
    src_h, want = blob_case
    src = _dev(src_h)
    # a refused argument: `end` owned the job before it looked at its arguments, so the job is gone, and the handle is dead
    job = _raw_begin(L, ctx._h, src)
    assert ctx.blob_jobs_pending() == 1
    assert _raw_end(L, job, 1 << 16, null_counts=True)[0] == EINVAL
    assert ctx.blob_jobs_pending() == 0
    L.visfd_hip_blob_dog_abort(job)            # nothing to do, and nothing dereferenced
    assert _raw_end(L, job, 1 << 16)[0] == EINVAL
    # too little room: the job stays, the counts come back, the retry delivers the oracle's lists
    job = _raw_begin(L, ctx._h, src)
    rc, _, _, nmin, nmax = _raw_end(L, job, 3)
    assert rc == ECAPACITY and (nmin, nmax) == (len(want[0]), len(want[1])) and ctx.blob_jobs_pending() == 1
    rc, amin, amax, nmin, nmax = _raw_end(L, job, max(nmin, nmax))
    assert rc == 0 and ctx.blob_jobs_pending() == 0
    _same_lists((api._blobs_to_rows(amin, nmin)[0], api._blobs_to_rows(amax, nmax)[0]), want, "after a capacity retry")
    assert _raw_end(L, job, 1 << 16)[0] == EINVAL      # ended: no longer live
    # abort twice
    job = _raw_begin(L, ctx._h, src)
    L.visfd_hip_blob_dog_abort(job)
    assert ctx.blob_jobs_pending() == 0
    L.visfd_hip_blob_dog_abort(job)
    L.visfd_hip_blob_dog_abort(None)
    assert L.visfd_hip_blob_jobs_pending(None) == 0
    # destroy with a live job: the job goes with its context
    h2 = C.c_void_p()
    assert L.visfd_hip_create(0, None, C.byref(h2)) == 0
    job = _raw_begin(L, h2, src)
    assert L.visfd_hip_blob_jobs_pending(h2) == 1
    assert L.visfd_hip_destroy(h2) == 0
    assert _raw_end(L, job, 1 << 16)[0] == EINVAL
    L.visfd_hip_blob_dog_abort(job)
    # the context of this test is none the worse for any of it
    _same_lists(ctx.blob_dog_dev(src, BLOB_SIG, None, None, 0.02, 2.5), want, "one call afterwards")


def test_context_close_with_a_live_blob_job(oracle, blob_case):
    from visfd_amd import api
    src = _dev(blob_case[0])
    c = api.Context(0)
    job = c.blob_dog_begin_dev(src, BLOB_SIG, None, None, 0.02, 2.5)
    assert c.blob_jobs_pending() == 1
    c.close()
    with pytest.raises(ValueError):
        c.blob_dog_end(job)
    c.blob_dog_abort(job)
    c.blob_dog_abort(job)
    c2 = api.Context(0)
    try:
        _same_lists(c2.blob_dog_dev(src, BLOB_SIG, None, None, 0.02, 2.5), blob_case[1], "a new context afterwards")
    finally:
        c2.close()


# ============================================================================================ C. slots hold anything
def _sparse_field(shape, seed, frac=0.06):
    rng = np.random.default_rng(seed)
    sal = np.zeros(shape, np.float32)
    pick = rng.random(shape) < frac
    sal[pick] = rng.uniform(1.0, 1e6, int(pick.sum())).astype(np.float32)
    d = rng.standard_normal(shape + (3,)).astype(np.float32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True).astype(np.float32)
    return sal, np.ascontiguousarray(d, np.float32)


S4, SODD = (20, 24, 28), (19, 22, 27)          # nx % 4 == 0 and not
BIG = (56, 72, 88)                             # every slot larger than the small shapes need
RATIO = 2.6482     # ~ ratio_from_threshold(0.03); any value serves, both sides get the same


class _Call:
    """One stage call.  run(ctx, shape) -> list of arrays; want(oracle, shape) -> the same list from the oracle, or None:
    then the reference is run() on a fresh context.  mode: "bits", or "rel" (tolerance modes: the suite's 1e-5 / per-voxel
    bound against the oracle)."""

    def __init__(self, name, run, want=None, mode="bits", small=S4, big=BIG):
        self.name, self.run, self.want, self.mode, self.small, self.big = name, run, want, mode, small, big


def _src(shape, seed=1):
    return volgen.membrane_volume(shape, seed=seed)


def _mask(shape):
    return volgen.block_mask(shape, seed=302)


def _calls():
    from visfd_amd import api
    calls = []

    def add(*a, **k):
        calls.append(_Call(*a, **k))

    # ---- Gaussians: single sweep (host face, nx % 4 == 0; device face, odd nx), three passes, masked, tolerance mode
    add("gauss_sweep_host", lambda c, s: list(c.gauss_hw(_src(s), (2, 2, 2), (5, 5, 5))),
        lambda o, s: list(o.gauss_hw(_src(s), (2, 2, 2), (5, 5, 5))))

    def gauss_dev(c, s, mask=False, hw=(3, 3, 3), sg=(1.2, 1.2, 1.2)):
        d = _empty(s)
        A = c.gauss_dev(_dev(_src(s)), d, sg, hw, _dev(_mask(s)) if mask else None)
        return [_host(c, d), A]
    add("gauss_sweep_dev_odd", gauss_dev, lambda o, s: list(o.gauss_hw(_src(s), (1.2, 1.2, 1.2), (3, 3, 3))), small=SODD, big=(55, 71, 87))

    def gauss_3pass(c, s):
        with c.options(gauss_3pass=1):
            return list(c.gauss_hw(_src(s), volgen.ANISO_SIGMA, volgen.ANISO_HW))
    add("gauss_3pass_aniso", gauss_3pass, lambda o, s: list(o.gauss_hw(_src(s), volgen.ANISO_SIGMA, volgen.ANISO_HW)))
    add("gauss_masked_dev", lambda c, s: gauss_dev(c, s, True, (4, 3, 2), (1.6, 1.2, 0.9)),
        lambda o, s: list(o.gauss_hw(_src(s), (1.6, 1.2, 0.9), (4, 3, 2), _mask(s))), small=SODD, big=(55, 71, 87))

    def gauss_fma(c, s):
        with c.options(gauss_fma=1):
            return [c.gauss_hw(_src(s), (2, 2, 2), (5, 5, 5))[0]]
    add("gauss_fma", gauss_fma, lambda o, s: [o.gauss_hw(_src(s), (2, 2, 2), (5, 5, 5))[0]], mode="rel")
    # ---- LoG, blobs
    add("log_host", lambda c, s: list(c.log(_src(s), (1.5, 1.5, 1.5), 0.02, RATIO)), lambda o, s: list(o.log(_src(s), (1.5, 1.5, 1.5), 0.02, RATIO)))
    bs = np.array([1.2, 1.5, 1.9, 2.4, 3.0], np.float32)

    def blobs(f, s):
        a = f(volgen.blob_volume(s, seed=31, nblobs=20), bs, None, None, 0.02, 2.5)
        return [volgen.sort_blobs(a[0], True), volgen.sort_blobs(a[1], False)]
    add("blob_one_call_host", lambda c, s: blobs(c.blob_dog, s), lambda o, s: blobs(o.blob_dog, s))
    # ---- Hessian and ridges (the eigen solver goes through device libm: fresh-context bits)
    add("hessian_host", lambda c, s: list(c.calc_hessian(_src(s), 1.5, RATIO, _mask(s))), lambda o, s: list(o.calc_hessian(_src(s), 1.5, RATIO, _mask(s))))

    def ridge_fused(c, s):
        sal, dirs = _empty(s), _empty((3,) + s, 0.0)
        c.ridge_saliency_dev(_dev(_src(s)), sal, dirs, 1.5, RATIO, api.DECREASING_EIVALS)
        return [_host(c, sal), _host(c, dirs)]
    add("ridge_fused_dev", ridge_fused)

    def ridge_two_step(c, s):
        sal, sm, dirs, m = _empty(s), _empty(s), _empty((3,) + s, 7.0), _dev(_mask(s))
        c.ridge_scores_dev(_dev(_src(s)), sal, sm, 1.5, RATIO, api.INCREASING_EIVALS, m)
        thr = c.threshold_fraction_dev(sal, 0.1, m)
        c.ridge_directions_dev(sm, sal, dirs, 1.5, api.INCREASING_EIVALS)
        return [_host(c, sal), _host(c, dirs), _host(c, sm), np.float32(thr)]
    add("ridge_two_step_dev", ridge_two_step)
    # ---- radix select
    def thr_host(f, s):
        sal = _sparse_field(s, 4, 0.5)[0]
        return [np.float32(f(sal, 0.2)), sal]
    add("threshold_host", lambda c, s: thr_host(c.threshold_fraction, s), lambda o, s: thr_host(o.threshold_fraction, s))

    def thr_dev(c, s):
        t = _dev(_sparse_field(s, 4, 0.5)[0])
        thr = c.threshold_fraction_dev(t, 0.2, _dev(_mask(s)))
        return [np.float32(thr), _host(c, t)]

    def thr_masked_o(o, s):
        sal = _sparse_field(s, 4, 0.5)[0]
        return [np.float32(o.threshold_fraction(sal, 0.2, _mask(s))), sal]
    add("threshold_masked_dev", thr_dev, thr_masked_o, small=SODD, big=(55, 71, 87))
    # ---- voting: two (sigma_tv, cutoff) that share h = 4 (the vote table's cache key has all three), masks on senders and
    #      receivers, the kernels of tv_box.hip, tv_tiled.hip (tv_exact_tiled), the tolerance mode and tv.hip (h = 34)
    def tv_host(c, s, sigma_tv, cutoff, opts, masked=True):
        sal, dirs = _sparse_field(s, 8)
        m = _mask(s) if masked else None
        with c.options(**opts):
            return [c.tv_dense_stick(sal, dirs, sigma_tv, 4, cutoff, m, m)]

    def tv_o(o, s, sigma_tv, cutoff, masked=True):
        sal, dirs = _sparse_field(s, 8)
        m = _mask(s) if masked else None
        return [o.tv_dense_stick(sal, dirs, sigma_tv, 4, cutoff, m, m)]
    assert api.tv_tables(3.2, 2.0 ** 0.5)[0] == api.tv_tables(3.0, 1.5)[0] == 4 and api.tv_tables(24.1, 2.0 ** 0.5)[0] == 34
    add("tv_exact_a", lambda c, s: tv_host(c, s, 3.2, 2.0 ** 0.5, {}), lambda o, s: tv_o(o, s, 3.2, 2.0 ** 0.5))
    add("tv_exact_b_same_h", lambda c, s: tv_host(c, s, 3.0, 1.5, {}, False), lambda o, s: tv_o(o, s, 3.0, 1.5, False))
    add("tv_exact_tiled", lambda c, s: tv_host(c, s, 3.0, 1.5, {"tv_exact_tiled": 1}), lambda o, s: tv_o(o, s, 3.0, 1.5))

    def tv_fma_dev(c, s):
        sal, dirs = _sparse_field(s, 8)
        ten = _empty((6,) + s)
        with c.options(tv_fma=1):
            c.tv_dense_stick_dev(_dev(sal), _dev(np.moveaxis(dirs, -1, 0)), ten, 3.2, 4, 2.0 ** 0.5)
        return [np.ascontiguousarray(np.moveaxis(_host(c, ten), 0, -1))]
    add("tv_fma_dev", tv_fma_dev, lambda o, s: tv_o(o, s, 3.2, 2.0 ** 0.5, False), mode="rel")
    add("tv_h34", lambda c, s: tv_host(c, s, 24.1, 2.0 ** 0.5, {}, False), lambda o, s: tv_o(o, s, 24.1, 2.0 ** 0.5, False),
        small=(9, 37, 30), big=(10, 44, 40))

    def wsum(c, s):
        m = _mask(s)
        return [c.tv_weight_sum(_sparse_field(s, 8, 0.2)[0], 3.0, 1.5, m, m)]
    add("tv_weight_sum", wsum)
    # ---- morphology: open with a flat ball (X-run kernel), dilate with a soft element, twice in a row (the second call
    #      finds its element in the slot)
    add("morph_open_flat", lambda c, s: [c.open_sphere(_src(s), 2.0, mask=_mask(s))],
        lambda o, s: [morph_np.sphere_op(api.MORPH_OPEN, _src(s), 2.0, mask=_mask(s))])

    def soft(c, s):
        out = []
        for _ in range(2):
            d = _empty(s)
            c.dilate_sphere_dev(_dev(_src(s)), d, 2.0, 3.0, 50.0)
            out.append(_host(c, d))
        return out
    add("morph_dilate_soft_twice", soft, lambda o, s: [morph_np.sphere_op(api.MORPH_DILATE, _src(s), 2.0, 3.0, 50.0)] * 2)
    # ---- the other two tables a context keeps in a slot: the median's footprint and the general filter's entries
    add("median_sphere_masked", lambda c, s: [c.median_sphere(_src(s), 1.5, mask=_mask(s))],
        lambda o, s: [median_np.median_sphere(_src(s), 1.5, mask=_mask(s))])
    table = np.random.default_rng(41).standard_normal((3, 5, 3)).astype(np.float32)     # hw = (1, 2, 1)
    add("filter3d_masked_norm", lambda c, s: [c.filter3d(_src(s), table, _mask(s), True)],
        lambda o, s: [filter3d_np.apply(_src(s), table, None, _mask(s), True)])
    # ---- binning, fluctuations
    def binning(c, s):
        half = tuple(n // 2 for n in s)
        b, u = _empty(half), _empty(s)
        c.bin_array3d_dev(_dev(_src(s)), b)
        c.unbin_array3d_dev(b, u)
        return [_host(c, b), _host(c, u)]

    def binning_o(o, s):
        b = o.bin_array3d(_src(s), tuple(n // 2 for n in s))
        return [b, o.unbin_array3d(b, s)]
    add("bin_unbin_dev", binning, binning_o)

    def fluct(c, s):
        d = _empty(s)
        c.local_fluctuations_dev(_dev(_src(s)), d, (2.0, 2.0, 2.0), RATIO, _dev(_mask(s)))
        return [_host(c, d)]
    add("fluctuations_dev", fluct, lambda o, s: [o.local_fluctuations(_src(s), (2.0, 2.0, 2.0), RATIO, _mask(s))])
    # ---- the whole membrane stage, host face
    def membrane(c, s, sigma_b):
        sal, ten, dirs, thr = c.membrane_detect(_src(s), 1.5, RATIO, api.DECREASING_EIVALS, 0.2, 0.0, 3.0, 4, 2.0 ** 0.5, _mask(s),
                                                want_tensor=True, want_dir=True, sigma_background=sigma_b)
        return [sal, ten, dirs, np.float32(thr)]
    add("membrane_host", lambda c, s: membrane(c, s, 0.0))
    add("membrane_host_background", lambda c, s: membrane(c, s, 3.0))
    return calls


def _check(call, got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        tag = "%s, output %d" % (what, i)
        if call.mode == "rel":
            assert_close_rel(g, w, TOL, tag, pervoxel=PV)
        elif isinstance(w, np.ndarray) and w.ndim:
            assert_bits_equal(g, w, tag)
        else:
            assert np.float32(g).tobytes() == np.float32(w).tobytes(), (tag, g, w)


PERMUTATION_SEEDS = (20261, 20262, 20263)


def test_stages_do_not_depend_on_what_their_slots_held(ctx, oracle):
    from visfd_amd import api
    calls = _calls()
    want = {}
    for k in calls:
        if k.want is not None:
            want[k.name] = k.want(oracle, k.small)
        else:     # no oracle form with the device's bits: the same call on a context that has seen nothing else
            fresh = api.Context(0)
            try:
                want[k.name] = k.run(fresh, k.small)
            finally:
                fresh.close()
    # the stages with device libm against the oracle at the suite's 1e-5 of the field's scale (test_saliency_direction_threshold)
    _, hess = oracle.calc_hessian(_src(S4), 1.5, RATIO, None, want_grad=False)
    assert_close_rel(want["ridge_fused_dev"][0], oracle.hessian_saliency(hess, po.ORDER_DECREASING)[0], 1e-5, "fresh-context ridge scores vs the oracle")
    # 1. large shapes first: every slot ends up larger than the small shapes need
    for k in calls:
        k.run(ctx, k.big)
    grown = ctx.workspace_bytes()
    assert grown > 0
    # 2. the small shapes in three fixed orders
    compared = 0
    for variant, seed in zip(("poison before every call", "trim before every third call", "left alone"), PERMUTATION_SEEDS):
        order = np.random.default_rng(seed).permutation(len(calls))
        for pos, i in enumerate(order):
            k = calls[int(i)]
            if variant.startswith("poison"):
                ctx.debug_poison_workspace()
            elif variant.startswith("trim") and pos % 3 == 0:
                ctx.trim()
                assert ctx.workspace_bytes() == 0
            _check(k, k.run(ctx, k.small), want[k.name], "%s (%s, position %d)" % (k.name, variant, pos))
            compared += 1
        if variant.startswith("poison"):
            assert ctx.workspace_bytes() >= grown, "poisoning frees nothing"
    assert compared == 3 * len(calls) and len(calls) >= 15
    # 3. right after a trim
    ctx.trim()
    assert ctx.workspace_bytes() == 0
    _check(calls[0], calls[0].run(ctx, calls[0].small), want[calls[0].name], calls[0].name + " right after trim")
    assert ctx.workspace_bytes() > 0


# ---- the tables kept in slots: a hit is decided by content, and a slot that is reallocated forgets what it held
TAB_SHAPE = (8, 12, 70)      # one workgroup row and a ragged edge in x
CROSS = np.array([(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.int32)
CROSS_B = CROSS.copy()
CROSS_B[1] = (1, 1, 0)       # as many entries, the same bounding box, one offset moved
CROSS_HEIGHTS = np.array([0.0, -0.5, -0.25, -1.0, -0.75, -2.0, -1.5], np.float32)


def _tab_inputs():
    return volgen.noise_volume(TAB_SHAPE, seed=17), volgen.block_mask(TAB_SHAPE, seed=18)


def test_a_table_of_the_same_size_is_not_taken_for_the_one_in_the_slot(ctx):
    """A, B, A with tables of equal entry count and bounding box that differ in one offset (morphology, median) or one
    weight (general filter): every call gets its own table's result, bit for bit against the numpy restatements."""
    from visfd_amd import api
    src, mask = _tab_inputs()
    assert (CROSS.min(0) == CROSS_B.min(0)).all() and (CROSS.max(0) == CROSS_B.max(0)).all() and len(CROSS) == len(CROSS_B)
    ta = np.random.default_rng(43).standard_normal((3, 5, 3)).astype(np.float32)     # hw = (1, 2, 1)
    tb = ta.copy()
    tb[2, 1, 0] += np.float32(0.5)
    want_morph = [morph_np.dilate_erode(src, e, CROSS_HEIGHTS, True, mask) for e in (CROSS, CROSS_B)]
    want_median = [median_np.median_table(src, e, mask=mask) for e in (CROSS, CROSS_B)]
    want_f3d = [filter3d_np.apply(src, t, None, mask, True) for t in (ta, tb)]
    for w in (want_morph, want_median, want_f3d):
        assert w[0].tobytes() != w[1].tobytes(), "the two tables must give different images"
    for pos, k in enumerate((0, 1, 0)):
        what = "%s (call %d)" % ("AB"[k], pos)
        assert_bits_equal(ctx.morph_table(api.MORPH_DILATE, src, (CROSS, CROSS_B)[k], CROSS_HEIGHTS, mask), want_morph[k], "morph_table " + what)
        assert_bits_equal(ctx.median_table(src, (CROSS, CROSS_B)[k], mask), want_median[k], "median_table " + what)
        assert_bits_equal(ctx.filter3d(src, (ta, tb)[k], mask, True), want_f3d[k], "filter3d " + what)


def test_a_table_slot_that_had_to_grow_forgets_the_table_it_held(ctx):
    """7 entries, then the 257 of the radius-4 ball (the slot is freed and reallocated), then the 7 again: all three right,
    for the median's footprint and for the structuring element."""
    from visfd_amd import api
    src, mask = _tab_inputs()
    ball, _ = morph_np.sphere_structure(4.0)
    assert len(ball) == 257 and (ball == median_np.footprint(4.0)).all()
    heights = (-0.125 * np.abs(ball).sum(axis=1)).astype(np.float32)
    want_median = {7: median_np.median_table(src, CROSS, mask=mask), 257: median_np.median_table(src, ball, mask=mask)}
    want_morph = {7: morph_np.dilate_erode(src, CROSS, CROSS_HEIGHTS, True, mask), 257: morph_np.dilate_erode(src, ball, heights, True, mask)}
    for pos, n in enumerate((7, 257, 7)):
        d, b = (CROSS, CROSS_HEIGHTS) if n == 7 else (ball, heights)
        before = ctx.workspace_bytes()
        assert_bits_equal(ctx.median_table(src, d, mask), want_median[n], "median_table, %d entries (call %d)" % (n, pos))
        assert_bits_equal(ctx.morph_table(api.MORPH_DILATE, src, d, b, mask), want_morph[n], "morph_table, %d entries (call %d)" % (n, pos))
        if pos == 1:
            assert ctx.workspace_bytes() >= before + 2 * 4 * 4 * (257 - 7), "both table slots grew"
        if pos == 2:
            assert ctx.workspace_bytes() == before, "slots only grow"


# ============================================================================================ D. options
def test_every_option_field_is_reachable_by_name(ctx):
    """The fields of struct visfd_hip_options, read out of common.hpp: each answers to its name with the default written
    there (unless the environment gives another), takes a value of its own and gives it back; no other name is known."""
    import os
    import re
    from conftest import ROOT
    from visfd_amd import api
    text = open(os.path.join(ROOT, "visfd_amd", "csrc", "common.hpp")).read()
    body = re.search(r"struct visfd_hip_options \{(.*?)\n\};", text, re.S).group(1)
    fields = re.findall(r"^\s*(?:int|int64_t)\s+(\w+)\s*=\s*(-?\d+)\s*;", body, re.M)
    assert len(fields) >= 30 and len(set(n for n, _ in fields)) == len(fields)
    assert len(fields) == len(re.findall(r"^\s*\w+\s+\w+\s*(?:=[^;]*)?;", body, re.M)), "a member line the pattern does not read"
    for name, default in fields:
        if "VISFD_HIP_" + name.upper() not in os.environ:
            assert ctx.get_option(name) == int(default), name
    for i, (name, _) in enumerate(fields):      # a value per field: two names on one field would show
        ctx.set_option(name, 1000 + i)
    for i, (name, _) in enumerate(fields):
        assert ctx.get_option(name) == 1000 + i, name
    for name, default in fields:
        ctx.set_option(name, int(default))
        assert ctx.get_option(name) == int(default), name
    for call in (lambda: ctx.get_option("no_such_option"), lambda: ctx.set_option("no_such_option", 1),
                 lambda: ctx.get_option("gauss_3pas"), lambda: ctx.get_option("")):
        with pytest.raises(api.VisfdHipError) as e:
            call()
        assert e.value.code == EINVAL
