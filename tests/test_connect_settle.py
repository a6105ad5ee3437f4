"""The option connect_settle of the graph entries of LabelConnected, on the CPU: the must-link rule and
the weighted moments restated in numpy on top of tests/connect_graph_np.py, held to the flood (api.label_connected) by the
contract of tests/connect_graph_contract.py on every case of tests/connect_settle_cases.py -- before any GPU time is
spent on the device's form of the same rule.  What the GPU file expects of each case (the device path and the bits it
settles, or the one reason for a hand-over) is derived here from the restatement, so those assertions are known to be
satisfiable; two mutants of the rule show that the cases can tell a wrong rule from the right one."""
import ctypes
import os
import re

import numpy as np
import pytest

import connect_graph_contract as cc
import connect_graph_np as cg
import connect_settle_cases as sc
import test_connect as tc

F = np.float32
LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dot3(a, b):
    return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2]))


def _decider(n_i, n_j, ri, rj, how):
    """connect.cpp's contact test -> (rule, value): rule 0 match iff value > 0, 1 iff value < 0, 2 iff value <= 0"""
    d = _dot3(n_i, n_j)
    if how == 0:
        return 0, d
    if how == 1:
        return 1, d
    r = (np.asarray(ri) - np.asarray(rj)).astype(F)
    length = np.sqrt(F(F(F(r[0] * r[0]) + F(r[1] * r[1])) + F(r[2] * r[2])))
    r = r * F(1.0 / float(length)) if length > 0 else np.array([1, 0, 0], F)
    a, b = _dot3(n_i, r), _dot3(n_j, r)
    if np.arcsin(np.abs(a)) < F(np.pi / 4) and np.arcsin(np.abs(b)) < F(np.pi / 4):
        return 0, d
    return 2, F(a * b)


def settle_np(sal, mask, d_in, t, kw, at_zero="raise", tie="lowest"):
    """The graph call with must-links, weights and any outward sum settled without the flood -> dict(got = the six results
    the contract checks, reasons, settled).  at_zero, tie: the mutants."""
    kw = dict(kw)
    must_link = kw.pop("must_link", None)
    how_lists = kw.pop("must_link_directions", None)
    W = kw.pop("voxel_weights", None)
    g = cg.label_connected_graph(sal, mask=mask, direction=None if d_in is None else d_in.copy(), tensor=t, **kw)
    reasons = g["reasons"] & ~(cg.OUTWARD | cg.HALO)      # the provisional clusters' outward sums are not what counts
    done = (cg.MUST_LINK if must_link else 0) | (cg.WEIGHTS if W is not None else 0)
    shape = sal.shape
    nz, ny, nx = shape
    n = sal.size
    undefined = kw.get("label_undefined", -1)
    standardize = d_in is not None and kw.get("standardize_directions", False) and not kw.get("consider_dot_product_sign", True)
    unmasked = np.ones(n, bool) if mask is None else mask.ravel() != 0
    final = g["labels"].ravel()
    live = unmasked & (final != undefined)
    nc = g["n_clusters"]
    # back from the final numbers to the provisional ones (connect_graph_np.py sorts by the float of the integer sizes)
    perm = np.arange(nc)
    if kw.get("sort_by_size", True) and nc:
        perm = np.lexsort((np.arange(nc), g["sizes"].astype(F)))[::-1]
    prov = np.full(n, -1, np.int64)
    prov[live] = perm[final[live] - 1]
    anchor = np.zeros(nc, np.int64)      # the voxel of each provisional cluster's lowest-ranked valid seed
    for rank_in_final, xyz in enumerate(g["seeds"].astype(np.int64)):
        anchor[perm[rank_in_final]] = (xyz[2] * ny + xyz[1]) * nx + xyz[0]
    Vf = None
    if d_in is not None:
        V_in = d_in.reshape(n, 3)
        Vf = g["direction"].reshape(n, 3).copy()      # oriented to the anchor, then flipped outwards per provisional cluster
        if standardize:
            for k in range(nc):
                if np.any(np.signbit(Vf[anchor[k]]) != np.signbit(V_in[anchor[k]])):      # undo that flip
                    Vf[prov == k] *= F(-1)

    cur = np.arange(nc)
    q = np.ones(nc, np.int64)
    if must_link:
        live_idx = np.flatnonzero(live)
        lz, ly, lx = np.unravel_index(live_idx, shape)
        for grp, locs in enumerate(must_link):
            prev = None
            for l, crd in enumerate(locs):
                crd32 = np.asarray(crd, F)
                if np.any(~(np.abs(crd32) < 2.0 ** 20)):
                    reasons |= cg.LIMITS
                    continue
                want = np.floor(crd32.astype(np.float64) + 0.5).astype(np.int64)
                reach = sum(max(abs(int(w)), abs(int(w) - (m - 1))) ** 2 for w, m in zip(want, (nx, ny, nz)))
                if reach >= 2 ** 33:
                    reasons |= cg.LIMITS
                    continue
                assert len(live_idx), "no voxel clustered"
                r2 = (want[0] - lx) ** 2 + (want[1] - ly) ** 2 + (want[2] - lz) ** 2
                pos = int(np.argmin(r2)) if tie == "lowest" else len(r2) - 1 - int(np.argmin(r2[::-1]))
                i = int(live_idx[pos])
                if prev is not None and cur[prov[i]] != cur[prov[prev]]:
                    j = prev
                    keep, gone = sorted((cur[prov[i]], cur[prov[j]]))
                    negate = False
                    if standardize:
                        ri = (i % nx, (i // nx) % ny, i // (nx * ny))
                        rj = (j % nx, (j // nx) % ny, j // (nx * ny))
                        how = 2 if how_lists is None else int(how_lists[grp][l])
                        rule, v = _decider(Vf[i] * F(q[prov[i]]), Vf[j] * F(q[prov[j]]), ri, rj, how)
                        if at_zero == "raise":
                            if v == 0 or v != v:
                                reasons |= cg.ZERO_DOT
                            negate = not (v > 0 if rule == 0 else v < 0 if rule == 1 else v <= 0)
                        else:       # the mutant: <= where the rule has <, and no hand-over
                            negate = (v <= 0) if rule == 0 else (v >= 0)
                    members = cur == gone
                    cur[members] = keep
                    if negate:
                        q[members] *= -1
                prev = i
    if reasons & ~(cg.MUST_LINK | cg.WEIGHTS):
        return dict(got=None, reasons=reasons, settled=0)

    # the survivors in rank order
    kept = np.flatnonzero(cur == np.arange(nc))
    number = np.full(nc, -1, np.int64)
    number[kept] = np.arange(len(kept))
    m = len(kept)
    idx = np.flatnonzero(live)                     # raster order
    k = number[cur[prov[idx]]]
    z, y, x = np.unravel_index(idx, shape)
    if Vf is not None and standardize:
        Vf[idx] = Vf[idx] * q[prov[idx]].astype(F)[:, None]
    w = None if W is None else W.ravel()[idx]
    sizes = np.zeros(m, LD)
    flip = np.zeros(m, bool)
    doubtful = False
    with np.errstate(all="ignore"):
        for c in range(m):
            sel = k == c
            sizes[c] = np.cumsum(w[sel].astype(LD))[-1] if w is not None else LD(int(sel.sum()))
            if not standardize:
                continue
            crd = [a[sel] for a in (x, y, z)]
            if w is not None:
                com = [np.cumsum((a.astype(F) * w[sel]).astype(LD))[-1] / sizes[c] for a in crd]
            else:
                com = [np.cumsum(a.astype(LD))[-1] / sizes[c] for a in crd]
            r = np.stack([(a.astype(LD) - cm).astype(F) for a, cm in zip(crd, com)], 1)
            nrm = Vf[idx[sel]]
            term = (r[:, 0] * nrm[:, 0] + r[:, 1] * nrm[:, 1]) + r[:, 2] * nrm[:, 2]
            delta = term.astype(LD) * (w[sel].astype(LD) if w is not None else LD(1))
            total = np.cumsum(delta)[-1]
            flip[c] = total < 0
            if w is None and np.any(term != 0):      # the device's guard (connect_graph.hip, stage (e))
                B = float(np.max(np.abs(r).sum(1).astype(F) * np.abs(nrm).max(1)))
                if not abs(float(total)) > float(sel.sum()) * 2.0 ** -20 * B:
                    doubtful = True
    if doubtful:
        done |= cg.OUTWARD
    fsizes = sizes.astype(F)
    perm2 = np.arange(m)
    if kw.get("sort_by_size", True) and m:
        perm2 = np.lexsort((np.arange(m), fsizes))[::-1]
    inv2 = np.empty(m, np.int64)
    inv2[perm2] = np.arange(m)
    labels = g["labels"].ravel().copy()
    labels[idx] = inv2[k] + 1
    a = anchor[kept][perm2] if m else np.zeros(0, np.int64)
    seeds = np.stack([a % nx, (a // nx) % ny, a // (nx * ny)], 1).astype(F).reshape(-1, 3)
    seed_sal = sal.ravel()[anchor[kept]] if m else np.zeros(0, F)
    d_out = None
    if d_in is not None:
        d_out = d_in.reshape(n, 3).copy()
        if standardize:
            d_out[idx] = Vf[idx] * np.where(flip[k], F(-1), F(1))[:, None]
        d_out = d_out.reshape(shape + (3,))
    return dict(got=(labels.reshape(shape), m, seeds, fsizes, seed_sal, d_out), reasons=reasons, settled=done)


def _run(job, **mutant):
    name, sal, ten, d, case, expect = job
    kw, mask, d_in, t = cc.split(sal, ten, d, case)
    return settle_np(sal, mask, d_in, t, kw, **mutant)


def _hold(job, **mutant):
    name, sal, ten, d, case, expect = job
    res = _run(job, **mutant)
    if expect["path"] == "flood":
        assert res["reasons"] & ~(cg.MUST_LINK | cg.WEIGHTS) == expect["reasons"], (name, cg.reason_names(res["reasons"]))
        return
    assert res["reasons"] & ~(cg.MUST_LINK | cg.WEIGHTS | cg.OUTWARD | cg.HALO) == 0, (name, cg.reason_names(res["reasons"]))
    assert res["settled"] == expect["settled"], (name, cg.reason_names(res["settled"]), cg.reason_names(expect["settled"]))
    cc.check(name, res["got"], sal, ten, d, case)


_CASES = sc.all_cases()


@pytest.mark.parametrize("job", _CASES, ids=[j[0] for j in _CASES])
def test_restated_rule_equals_the_flood(job):
    _hold(job)


def test_tensor_voting_volume_with_must_links_and_weights(oracle):
    """test_connect.py's must-link and voxel-weight calls on the tensor-voting outputs: seven islands, two groups of three"""
    post, ten, direction = tc.tv_outputs(oracle)
    for i, case in enumerate(tc.must_link_cases(post)):
        bits = (cg.MUST_LINK if "must_link" in case else 0) | (cg.WEIGHTS if "voxel_weights" in case else 0)
        res = _run(("tc must-link %d" % i, post, ten, direction, case, None))
        print("tc must-link %d" % i, cg.reason_names(res["reasons"]), cg.reason_names(res["settled"]))
        if res["got"] is None:      # a structural reason: the flood's business with or without the option
            assert not res["reasons"] & (cg.OUTWARD | cg.LIMITS)
            continue
        assert res["settled"] & ~cg.OUTWARD == bits
        cc.check("tc must-link %d" % i, res["got"], post, ten, direction, case)


def _trips(**mutant):
    """the must-link cases on which the mutant's results, wherever it produces any, are not the flood's"""
    tripped = []
    for name, sal, ten, d, case, expect in sc.must_link_cases():
        res = _run((name, sal, ten, d, case, expect), **mutant)
        if res["got"] is None:
            continue
        try:
            cc.check(name, res["got"], sal, ten, d, case)
        except AssertionError:
            tripped.append(name)
    return tripped


def test_a_wrong_rule_is_caught():
    assert _trips(at_zero="le"), "no case tells D <= 0 from D < 0"
    assert "ml tie" in _trips(tie="highest")


def test_symbol_option_and_binding():
    from visfd_amd import api
    header = open(os.path.join(ROOT, "include", "visfd_hip.h")).read()
    assert re.search(r"^ \*   connect_settle\s", header, re.M), "the option is missing from the header's list"
    assert "int visfd_hip_label_connected_graph_last_settled(visfd_hip_ctx*, unsigned* settled);" in header
    lib = api.load_library()
    fn = lib.visfd_hip_label_connected_graph_last_settled
    bits = ctypes.c_uint(7)
    assert fn(None, ctypes.byref(bits)) != 0 and bits.value == 7      # a null context is refused, nothing written
    assert lib.visfd_hip_abi_version() == 10
    assert callable(api.Context.label_connected_graph_last_settled)
    assert "connect_settle" in open(os.path.join(ROOT, "visfd_amd", "csrc", "context.hip")).read()
