"""The order-free restatement of LabelConnected (tests/connect_graph_np.py) against the sequential
flood in csrc/connect.cpp (api.label_connected), on the CPU.  A device path for the clustering may only be built on a
definition that this file has checked (none is built yet), so the comparison is bit for bit: labels, cluster count,
seed positions, sizes, seed saliencies and the rewritten directions.

Cases: the five calls of tests/test_connect.py::cases on its 28 x 34 x 40 tensor-voting outputs, and around them
connectivity 1 / 2 / 3, a mask, minima mode (the negated saliency), thresholds switched off (< -1), the dot product's
sign considered or not, directions that were standardised before, quantised saliency (plateau seeds), and two small
random images (3 x 3 x 3, 3 x 5 x 70) where every voxel's stencil is clamped.

Share of the cases that report no fallback reason: 26 of 34 (the rule is two thirds).  The eight that do all report
the halo reason and nothing else.  Six of them standardise raw eigenvector directions: the sign of an eigenvector is
arbitrary, a quarter to a third of the seeds of a voted surface face against their cluster's anchor, and then the directions
that the flood leaves on the UNLABELLED voxels around a cluster (the halo) depend on which basin reached them last.
The other two start from directions that an earlier call standardised and still have a handful of halo voxels whose
labelled neighbours disagree.  In all eight everything but the halo agrees with the flood, and the halo does differ
(a few hundred of ~3300 halo voxels for raw eigenvectors), which is what the reason predicts.  filter_mrc's own
-connect call is one of them.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import connect_graph_np as cg
import test_connect as tc
import volgen
from visfd_amd import api

N_CASES, N_CLEAN = 34, 26


def _variants(post):
    base = tc.cases(post)
    thr = base[0]["threshold_saliency"]
    out = [("base%d" % i, dict(c)) for i, c in enumerate(base)]
    for conn in (2, 3):
        for i in (0, 2, 3):
            out.append(("base%d conn%d" % (i, conn), dict(base[i], connectivity=conn)))
    for i in (0, 1, 2, 3):
        out.append(("base%d mask" % i, dict(base[i], mask=True)))
    for i in (0, 3, 4):       # minima mode: the same surfaces are the minima of the negated saliency
        c = dict(base[i], start_from_saliency_maxima=False, _negate=True, tensor_is_positive_definite_near_target=False)
        c["threshold_saliency"] = -c["threshold_saliency"]
        out.append(("base%d minima" % i, c))
    for signs in (True, False):
        for conn in (1, 3):
            out.append(("off signs=%d conn%d" % (signs, conn), dict(
                threshold_saliency=thr, use="vt", threshold_vector_saliency=-2.0, threshold_vector_neighbor=-2.0,
                threshold_tensor_saliency=-2.0, threshold_tensor_neighbor=-2.0, consider_dot_product_sign=signs,
                connectivity=conn)))
    out.append(("base2 signed", dict(base[2], consider_dot_product_sign=True)))
    out.append(("base3 unsigned", dict(base[3], consider_dot_product_sign=False)))
    out.append(("base3 unsigned conn3 mask", dict(base[3], consider_dot_product_sign=False, connectivity=3, mask=True)))
    out.append(("base3 no standardize v only", dict(base[3], use="v")))
    # directions that a first call has standardised: every seed agrees with its anchor, the halo is settled
    for i in (2, 4):
        out.append(("base%d standardised before" % i, dict(base[i], _prestandardise=True)))
    out.append(("base4 standardised before conn2", dict(base[4], _prestandardise=True, connectivity=2)))
    out.append(("plateaus", dict(base[0], _quantise=True)))
    out.append(("plateaus conn3 vt", dict(base[3], _quantise=True, connectivity=3)))
    out.append(("plateaus minima", dict(base[0], _quantise=True, _negate=True, start_from_saliency_maxima=False,
                                         threshold_saliency=-thr, connectivity=2)))
    return out


def _small(shape, seed, **kw):
    rng = np.random.default_rng(seed)
    sal = rng.random(shape).astype(np.float32)
    ten = rng.normal(0, 1, shape + (6,)).astype(np.float32)
    ten[..., :3] = np.abs(ten[..., :3]) + 1
    d = rng.normal(0, 1, shape + (3,)).astype(np.float32)
    return sal, ten, d, dict(threshold_saliency=0.4, use="vt", threshold_vector_saliency=0.2, threshold_vector_neighbor=0.3,
                             threshold_tensor_saliency=-0.5, threshold_tensor_neighbor=0.2, **kw)


def _call(fn, sal, ten, direction, case):
    """-> (labels, n, seeds, sizes, seed saliencies, directions after the call or None, reasons or None)"""
    kw = {k: v for k, v in case.items() if not k.startswith("_")}
    use = kw.pop("use", "")
    mask = volgen.block_mask(sal.shape, seed=9) if kw.pop("mask", False) else None
    d = direction.copy() if "v" in use else None
    t = ten if "t" in use else None
    if fn is api.label_connected:
        labels, k, cm, cs, csal = fn(sal, mask=mask, direction=d, tensor=t, **kw)
        return labels, k, cm, cs, csal, d, None
    g = fn(sal, mask=mask, direction=d, tensor=t, **kw)
    return g["labels"], g["n_clusters"], g["seeds"], g["sizes"], g["seed_saliencies"], g["direction"], g["reasons"]


def _inputs(post, ten, direction, case):
    sal = post
    if case.get("_quantise"):
        sal = (np.round(sal / sal.max() * 12) / 12 * sal.max()).astype(np.float32)
    if case.get("_negate"):
        sal = -sal
    if case.get("_prestandardise"):
        first = dict(case, sort_by_size=True)
        direction = _call(api.label_connected, sal, ten, direction, first)[5]
    return np.ascontiguousarray(sal), ten, direction


@pytest.fixture(scope="module")
def results(oracle):
    post, ten, direction = tc.tv_outputs(oracle)
    jobs = [(name, case) + _inputs(post, ten, direction, case) for name, case in _variants(post)]
    for name, shape, seed, kw in (("3x3x3", (3, 3, 3), 1, dict(connectivity=3, consider_dot_product_sign=True)),
                                  ("3x5x70", (70, 5, 3), 2, dict(connectivity=2, consider_dot_product_sign=False))):
        sal, t, d, case = _small(shape, seed, **kw)
        jobs.append((name, case, sal, t, d))
    out = []
    for name, case, sal, t, d in jobs:
        host = _call(api.label_connected, sal, t, d, case)
        graph = _call(cg.label_connected_graph, sal, t, d, case)
        out.append((name, host, graph))
    return out


def _differences(host, graph, halo_too=True):
    bad = []
    if host[1] != graph[1]:
        bad.append("n_clusters %d vs %d" % (host[1], graph[1]))
    if not np.array_equal(host[0], graph[0]):
        bad.append("labels at %d voxels" % int((host[0] != graph[0]).sum()))
    for a, b, what in zip(host[2:5], graph[2:5], ("seed positions", "sizes", "seed saliencies")):
        if a.shape != b.shape or not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
            bad.append(what)
    if host[5] is not None:
        ne = (host[5].view(np.uint32) != graph[5].view(np.uint32)).any(-1)
        if not halo_too:
            ne &= host[0] >= 1      # labelled voxels (and masked ones, which no path touches); label_undefined is -1
        if ne.any():
            bad.append("directions at %d voxels" % int(ne.sum()))
    return bad


def test_clean_cases_are_equal_bit_for_bit(results):
    failures = [(name, _differences(h, g)) for name, h, g in results if g[6] == 0 and _differences(h, g)]
    assert not failures, failures
    assert sum(h[1] > 0 for _, h, g in results if g[6] == 0) >= 20      # clusters were found, not empty images compared


def test_share_of_clean_cases(results):
    clean = [name for name, h, g in results if g[6] == 0]
    flagged = [(name, cg.reason_names(g[6])) for name, h, g in results if g[6]]
    print("clean %d of %d; flagged: %s" % (len(clean), len(results), flagged))
    assert len(results) == N_CASES and len(clean) == N_CLEAN, flagged
    assert 3 * len(clean) >= 2 * len(results)


def test_halo_cases_differ_only_in_the_halo(results):
    """A call that only reports the halo reason still has the flood's labels, lists and labelled directions; the
    directions of the unlabelled voxels are where the pop order shows, and with raw eigenvectors it does show (the
    reason is sufficient, not necessary: directions standardised before may come out alike all the same)."""
    seen = 0
    for name, h, g in results:
        if g[6] != cg.HALO:
            continue
        seen += 1
        assert h[1] > 0, name
        assert not _differences(h, g, halo_too=False), (name, _differences(h, g, halo_too=False))
        if "standardised before" not in name:
            assert _differences(h, g), name + ": the halo reason was reported but nothing depends on the order"
    assert seen >= 3


def test_raw_eigenvector_directions_always_meet_the_halo(results):
    """filter_mrc's -connect call (base2) standardises raw eigenvectors: it is not a clean case."""
    by_name = {name: g for name, h, g in results}
    assert by_name["base2"][6] & cg.HALO and by_name["base4"][6] & cg.HALO
    assert by_name["base4 standardised before"][6] == 0


def _twisted_band(n=24, radius=7.5, half_width=2.5):
    """A Moebius band around the z axis through the image centre: in the half plane of azimuth a the band is the segment
    of half-width `half_width` through (radius, 0) tilted by a / 2.  Saliency falls off with the in-plane distance to that
    segment, the direction is the segment's normal, continuous in a on [0, 2 pi) and therefore reversed across a = 0."""
    c = (n - 1) / 2.0
    z, y, x = np.meshgrid(np.arange(n) - c, np.arange(n) - c, np.arange(n) - c, indexing="ij")
    a = np.arctan2(y, x) % (2 * np.pi)
    rho = np.hypot(x, y)
    rx, ry = np.cos(a), np.sin(a)
    cw, sw = np.cos(a / 2), np.sin(a / 2)
    u, v = rho - radius, z                                     # in-plane coordinates about the band's centre line
    t = np.clip(u * cw + v * sw, -half_width, half_width)
    d2 = (u - t * cw) ** 2 + (v - t * sw) ** 2
    sal = np.exp(-d2 / 2.0).astype(np.float32)
    direction = np.ascontiguousarray(np.stack([-sw * rx, -sw * ry, cw], -1).astype(np.float32))
    return sal, direction


def test_constructed_fallback_reasons():
    """Ordinary inputs on which the flood's order decides: a band whose normals cannot be oriented, voxel weights, a
    must-link.  The restatement names the reason; the host path is their only definition and runs as ever."""
    sal, direction = _twisted_band()
    kw = dict(threshold_saliency=float(np.exp(-0.5)), connectivity=3, consider_dot_product_sign=False,
              standardize_directions=True, threshold_vector_saliency=-2.0)
    g = cg.label_connected_graph(sal, direction=direction, **kw)
    assert g["reasons"] & cg.UNBALANCED, cg.reason_names(g["reasons"])
    assert g["n_clusters"] == 1                       # one band, all of it in one component
    labels, k, _, sizes, _ = api.label_connected(sal, direction=direction.copy(), **kw)
    assert k == 1 and sizes[0] == g["sizes"][0] and np.array_equal(labels, g["labels"])
    w = np.ones(sal.shape, np.float32)
    assert cg.label_connected_graph(sal, voxel_weights=w, **kw)["reasons"] & cg.WEIGHTS
    ml = [[(4.0, 12.0, 12.0), (19.0, 12.0, 12.0)]]
    assert cg.label_connected_graph(sal, must_link=ml, **kw)["reasons"] & cg.MUST_LINK
    half = sal.copy()
    half[:, :, 12:] = 0                               # an open half band can be oriented
    g = cg.label_connected_graph(half, direction=direction, **kw)
    assert not g["reasons"] & cg.UNBALANCED and g["n_clusters"] >= 1


def test_seed_search_restated(oracle):
    """find_seeds against the clusters' seeds on an image that is nothing but plateaus, masked and not"""
    rng = np.random.default_rng(3)
    sal = rng.integers(0, 4, (9, 10, 11)).astype(np.float32)
    for mask in (None, volgen.block_mask(sal.shape, seed=9)):
        for conn in (1, 2, 3):
            for from_max in (True, False):
                kw = dict(threshold_saliency=2.0 if from_max else 1.0, connectivity=conn, mask=mask,
                          start_from_saliency_maxima=from_max, sort_by_size=False)
                labels, k, cm, cs, csal = api.label_connected(sal, **kw)
                g = cg.label_connected_graph(sal, **kw)
                assert g["reasons"] == 0 and g["n_clusters"] == k and np.array_equal(labels, g["labels"])
                assert np.array_equal(cm, g["seeds"]) and np.array_equal(cs, g["sizes"]) and np.array_equal(csal, g["seed_saliencies"])


# ---- the seed search on the device (csrc/connect_seeds.hip): what can be said without a GPU ------------------------------------------
NEW_SYMBOLS = ["visfd_hip_label_connected_device_seeds", "visfd_hip_label_connected_device_seeds_last"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_header_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "visfd_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = ctypes.CDLL(api.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(L, name) and name in api.exported_symbols(), name
    for macro, value in (("VISFD_HIP_CONNECT_SEEDS_DEVICE", api.CONNECT_SEEDS_DEVICE),
                         ("VISFD_HIP_CONNECT_SEEDS_HOST", api.CONNECT_SEEDS_HOST)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), code), macro
    # the _ex arguments after the context
    assert api._SIGS[NEW_SYMBOLS[0]][1][1:] == api._SIGS["visfd_hip_label_connected_ex"][1]
    # the names a device implementation of the flood would take stay free
    for name in ("visfd_hip_label_connected_gpu", "visfd_hip_label_connected_dev", "visfd_hip_label_connected_last_path"):
        assert not hasattr(L, name) and not re.search(r"\b%s\s*\(" % name, code), name


def test_device_seed_entry_refuses_a_null_context():
    """Without a GPU no context can be created, so the entry can only be refused here; the host entry is unchanged and
    keeps its argument checks, now made before anything is computed."""
    L = api.load_library()
    s = np.zeros((4, 4, 4), np.float32)
    lab = np.zeros((4, 4, 4), np.int64)
    n = ctypes.c_int64(0)
    tail = (s.ctypes.data, lab.ctypes.data, None, 4, 4, 4, 0.5, None, 0.0, 0.0, 1, None, 0.0, 0.0, 1, 1, -1, 1, 0, 1,
            ctypes.byref(n), None, None, None, 0, None, None, None, 0, None)
    assert L.visfd_hip_label_connected_device_seeds(None, *tail) == 1
    assert L.visfd_hip_label_connected_device_seeds_last(None, None, None) == 1
    assert L.visfd_hip_label_connected_ex(*tail) == 0 and n.value == 0
    bad = list(tail)
    bad[3] = 2                                          # nx = 2: refused as ever, with the same message
    assert L.visfd_hip_label_connected_ex(*bad) == 1 and b"at least 3 voxels" in L.visfd_hip_last_error()
    bad = list(tail)
    bad[15] = 0                                         # connectivity 0
    assert L.visfd_hip_label_connected_ex(*bad) == 1
    bad = list(tail)
    bad[3:6] = [1 << 11, 1 << 10, 1 << 10]              # 2^31 voxels: refused before a voxel is read
    assert L.visfd_hip_label_connected_ex(*bad) == 1 and b"too large" in L.visfd_hip_last_error()
