"""A literal numpy restatement of the reference's supervised blob thresholds, the oracle of tests/test_supervised*.py:

  find_spheres_table     FindSpheres as lib/visfd/visfd_utils.hpp:271-359 does it: an integer table spanning the queries'
                         bounding box, every sphere painted into it in list order, the queries read off it (small boxes only)
  find_spheres_pairs     the same answer without the table (chunked over the spheres), for lists a table cannot hold
  choose_threshold_1d    visfd_utils.hpp:373-516
  choose_interval        _ChooseThresholdInterval, feature_implementation.hpp:136-275
  sort_blobs, find_blob_scores, choose_blob_score_thresholds[_multi], discard_blobs_by_score_supervised

Arithmetic types follow the reference: float32 where it computes in Scalar = float, float64 where a double literal enters."""
import math

import numpy as np

F = np.float32
DO_NOT_SORT, SORT_DECREASING, SORT_INCREASING, SORT_DECREASING_MAGNITUDE, SORT_INCREASING_MAGNITUDE = range(5)


def sphere_R_Rsqr(diameter):
    """visfd_utils.hpp:324-327: diameter/2 in float, "- 0.5" and ceil in double, SQR a float product."""
    r = F(diameter) / F(2)
    R = max(0, int(math.ceil(float(r) - 0.5)))
    Rsqr = max(0, int(math.ceil(float(F(r * r)) - 0.5)))
    return R, Rsqr


def _trunc(a):
    return np.trunc(np.asarray(a, np.float32).reshape(-1, 3)).astype(np.int64)


def find_spheres_table(crds, sphere_crds, sphere_diameters):
    q, c = _trunc(crds), _trunc(sphere_crds)
    assert (q >= 0).all()
    size = [0, 0, 0]
    crds = np.asarray(crds, np.float32).reshape(-1, 3)
    for i in range(len(crds)):                     # image_size[d] = (int)(crd + 1) wherever image_size[d] <= crd
        for d in range(3):
            if size[d] <= crds[i, d]:
                size[d] = int(F(crds[i, d]) + F(1))
    table = np.zeros((size[2], size[1], size[0]), np.int64)
    for i in range(len(c)):
        R, Rsqr = sphere_R_Rsqr(sphere_diameters[i])
        j = np.arange(-R, R + 1)
        jz, jy, jx = np.meshgrid(j, j, j, indexing="ij")
        ok = jx * jx + jy * jy + jz * jz <= Rsqr
        x, y, z = c[i, 0] + jx, c[i, 1] + jy, c[i, 2] + jz
        ok &= (x >= 0) & (x < size[0]) & (y >= 0) & (y < size[1]) & (z >= 0) & (z < size[2])
        table[z[ok], y[ok], x[ok]] = i + 1
    return np.array([table[p[2], p[1], p[0]] for p in q], np.int64).reshape(-1)


def find_spheres_pairs(crds, sphere_crds, sphere_diameters, chunk=4096):
    """max over the containing spheres of index + 1, with the R test AND the Rsqr test, pair by pair"""
    q, c = _trunc(crds), _trunc(sphere_crds)
    rr = np.array([sphere_R_Rsqr(d) for d in sphere_diameters], np.int64).reshape(-1, 2)
    ids = np.zeros(len(q), np.int64)
    for s0 in range(0, len(c), chunk):
        cc, R, Rsqr = c[s0:s0 + chunk], rr[s0:s0 + chunk, 0], rr[s0:s0 + chunk, 1]
        d = np.abs(q[:, None, :] - cc[None, :, :])
        inside = (d <= R[None, :, None]).all(axis=2) & ((d * d).sum(axis=2) <= Rsqr[None, :])
        idx = np.where(inside, np.arange(s0 + 1, s0 + 1 + len(cc))[None, :], 0).max(axis=1, initial=0)
        ids = np.maximum(ids, idx)
    return ids


def _order(keys, ascending):
    """std::sort of (key, index) tuples, or through reverse iterators: the exact reverse of the ascending order"""
    order = sorted(range(len(keys)), key=lambda i: (keys[i], i))
    return order if ascending else order[::-1]


def choose_threshold_1d(scores, accepted, lower_bound=True):
    s = [F(x) for x in scores]
    N = len(s)
    order = _order(s, lower_bound)
    s_sorted, a_sorted = [s[i] for i in order], [bool(accepted[i]) for i in order]
    Nn = sum(1 for a in a_sorted if not a)
    SGN = F(1.0) if lower_bound else F(-1.0)
    counts, m = [], Nn
    for i in range(-1, N):
        if i >= 0:
            m += 1 if a_sorted[i] else -1
        counts.append(m)
    best = min(counts)
    at_min = [i - 1 for i, m in enumerate(counts) if m == best]
    it = at_min[len(at_min) // 2]
    if it == -1:
        return F(-SGN * F(np.inf))
    if it == N - 1:
        return F(SGN * F(np.inf))
    return F(0.5 * float(F(s_sorted[it] + s_sorted[it + 1])))


def choose_interval(scores, accepted):
    """-> (lower, upper, false positives, negatives, false negatives, positives)"""
    s = [F(x) for x in scores]
    acc = [bool(a) for a in accepted]
    N = len(s)

    def mistakes(lo, hi):
        return sum(1 for i in range(N) if acc[i] != (s[i] >= lo and s[i] <= hi))
    lo1 = choose_threshold_1d(s, acc, True)
    keep = [i for i in range(N) if s[i] >= lo1]
    hi1 = choose_threshold_1d([s[i] for i in keep], [acc[i] for i in keep], False)
    hi2 = choose_threshold_1d(s, acc, False)
    keep = [i for i in range(N) if s[i] <= hi2]
    lo2 = choose_threshold_1d([s[i] for i in keep], [acc[i] for i in keep], True)
    lo, hi = (lo1, hi1) if mistakes(lo1, hi1) <= mistakes(lo2, hi2) else (lo2, hi2)
    inside = [s[i] >= lo and s[i] <= hi for i in range(N)]
    fp = sum(1 for i in range(N) if inside[i] and not acc[i])
    fn = sum(1 for i in range(N) if not inside[i] and acc[i])
    return F(lo), F(hi), fp, sum(1 for a in acc if not a), fn, sum(1 for a in acc if a)


def sort_blobs(crds, diameters, scores, criteria, ascending=True):
    c, d, s = np.asarray(crds, np.float32).reshape(-1, 3), np.asarray(diameters, np.float32), np.asarray(scores, np.float32)
    if criteria == DO_NOT_SORT:
        return c, d, s
    if criteria in (SORT_INCREASING, SORT_INCREASING_MAGNITUDE):
        ascending = not ascending
    keys = [F(abs(x)) if criteria in (SORT_DECREASING_MAGNITUDE, SORT_INCREASING_MAGNITUDE) else F(x) for x in s]
    order = _order(keys, ascending)
    return c[order], d[order], s[order]


def find_blob_scores(training_crds, crds, diameters, scores, criteria=SORT_DECREASING_MAGNITUDE, find=find_spheres_pairs):
    c, d, s = sort_blobs(crds, diameters, scores, criteria, True)
    ids = find(training_crds, c, d)
    out = np.full(len(ids), -np.inf, np.float32)
    out[ids > 0] = s[ids[ids > 0] - 1]
    return out, ids


class EmptyTrainingSet(Exception):
    pass


def choose_blob_score_thresholds_multi(blob_lists, training_pos, training_neg, criteria=SORT_DECREASING_MAGNITUDE,
                                       find=find_spheres_pairs):
    scores, accepted = [], []
    for (c, d, s), pos, neg in zip(blob_lists, training_pos, training_neg):
        pos, neg = np.asarray(pos, np.float32).reshape(-1, 3), np.asarray(neg, np.float32).reshape(-1, 3)
        t = np.concatenate([pos, neg])
        ts, ids = find_blob_scores(t, c, d, s, criteria, find)
        for i in range(len(t)):
            if ids[i] != 0:
                scores.append(ts[i])
                accepted.append(i < len(pos))
    if not any(not a for a in accepted):
        raise EmptyTrainingSet("negative")
    if not any(accepted):
        raise EmptyTrainingSet("positive")
    return choose_interval(scores, accepted)


def choose_blob_score_thresholds(crds, diameters, scores, pos, neg, criteria=SORT_DECREASING_MAGNITUDE, find=find_spheres_pairs):
    return choose_blob_score_thresholds_multi([(crds, diameters, scores)], [pos], [neg], criteria, find)


def discard_blobs_by_score_supervised(crds, diameters, scores, pos, neg, criteria=SORT_DECREASING_MAGNITUDE,
                                      find=find_spheres_pairs):
    r = choose_blob_score_thresholds(crds, diameters, scores, pos, neg, criteria, find)
    c, d, s = np.asarray(crds, np.float32).reshape(-1, 3), np.asarray(diameters, np.float32), np.asarray(scores, np.float32)
    keep = (s >= r[0]) & (s <= r[1])
    return (c[keep], d[keep], s[keep]) + r
