"""DiscardOverlappingBlobs (lib/visfd/feature.hpp:720-913) as an order-free statement, in numpy, over all pairs:

    keep(i) = not exists k < i :  keep(k)  and  share(i, k)  and  crit(i, k)          (i, k: positions in the sorted list)

  crit    the discard criterion, expression by expression in the reference's number types (float32; float64 where M_PI
          enters)
  share   the two blobs reach a common cell of the occupancy table: with C = (int)floor((x - bmin) / scale) per axis and
          R = (int)ceil((d / 2) / scale) + 1, a cell c with 0 <= c < tsz on every axis, |c - C_i|^2 <= R_i^2 and
          |c - C_k|^2 <= R_k^2
  bounds  bmin = (int)min_i(c - ceil(d / 2)), bmax = max(-1, (int)max_i(c + ceil(d / 2))) (truncation; the reference's
          loop starts bmax at -1 and never lowers it), tsz = (1 + bmax - bmin) / scale

Nothing here walks a grid in list order: the ranking is a stable sort, crit and share are matrices, and keep is read off
them.  The switches of `discard_overlapping_blobs` turn the statement into the mutants tests/test_overlap.py uses to show
that its cases can tell them apart."""
import math

import numpy as np

F = np.float32
DO_NOT_SORT, SORT_DECREASING, SORT_INCREASING, SORT_DECREASING_MAGNITUDE, SORT_INCREASING_MAGNITUDE = range(5)


def rank(scores, criteria, reverse_ties=True):
    """order[position] = original index, best first (SortBlobs with ascending_order = false): (key, index) tuples ascending,
    or the exact reverse of that order for the two decreasing criteria -- equal keys then go to the LARGER index first.
    reverse_ties=False is the mutant that sends them to the smaller one."""
    s = np.asarray(scores, F)
    n = len(s)
    if criteria == DO_NOT_SORT:
        return np.arange(n)
    key = np.abs(s) if criteria in (SORT_DECREASING_MAGNITUDE, SORT_INCREASING_MAGNITUDE) else s
    order = np.argsort(key, kind="stable")            # -0 == +0: the index decides, as std::pair's < does
    if criteria in (SORT_DECREASING, SORT_DECREASING_MAGNITUDE):
        order = order[::-1] if reverse_ties else np.argsort(-key.astype(np.float64), kind="stable")
    return order


def bounds_formula(crds, diameters):
    c, d = np.asarray(crds, F).reshape(-1, 3), np.asarray(diameters, F)
    reff = np.ceil(d / F(2))[:, None]
    # the loop's bmax starts at -1 and only ever grows: a list that lies below -1 on an axis keeps -1 there
    return np.trunc((c - reff).min(0)).astype(np.int64), np.maximum(np.trunc((c + reff).max(0)).astype(np.int64), -1)


def bounds_sequential(crds, diameters):
    """the reference's loop, statement by statement (feature.hpp:756-768)"""
    c, d = np.asarray(crds, F).reshape(-1, 3), np.asarray(diameters, F)
    bmin, bmax = [0, 0, 0], [-1, -1, -1]
    for i in range(len(d)):
        reff = F(math.ceil(d[i] / F(2)))
        for a in range(3):
            x = c[i, a]
            if F(x - reff) < F(bmin[a]) or bmin[a] > bmax[a]:
                bmin[a] = int(F(x - reff))
            if F(x + reff) > F(bmax[a]) or bmin[a] > bmax[a]:
                bmax[a] = int(F(x + reff))
    return np.array(bmin, np.int64), np.array(bmax, np.int64)


def sphere_overlap(rij, Ri, Rj):
    """CalcSphereOverlap (visfd_utils.hpp:95-118) on float32 arrays"""
    Ri, Rj = np.minimum(Ri, Rj), np.maximum(Ri, Rj)
    D = np.float64
    with np.errstate(all="ignore"):
        inside = (((4 * math.pi / 3) * Ri.astype(D)) * Ri.astype(D) * Ri.astype(D)).astype(F)
        inv = 0.5 * (1.0 / rij.astype(D))
        xi = (inv * (rij * rij + Ri * Ri - Rj * Rj).astype(D)).astype(F)
        xj = (inv * (rij * rij + Rj * Rj - Ri * Ri).astype(D)).astype(F)
        qi, qj = xi / Ri, xj / Rj
        ti = Ri * Ri * Ri * (F(2) - qi * (F(3) - qi * qi))
        tj = Rj * Rj * Rj * (F(2) - qj * (F(3) - qj * qj))
        lens = ((math.pi / 3) * (ti + tj).astype(D)).astype(F)
    return np.where(rij <= Ri, inside, lens)


def crit_matrix(c, d, ratio, max_large, max_small):
    """crit[i, k] for the sorted list (blob_post.cpp, the body of the loop over a cell's entries)"""
    x, y, z = c[:, 0], c[:, 1], c[:, 2]
    dx, dy, dz = x[:, None] - x[None, :], y[:, None] - y[None, :], z[:, None] - z[None, :]
    rik = np.sqrt(dx * dx + dy * dy + dz * dz)
    r = d / F(2)
    ri, rk = np.broadcast_arrays(r[:, None], r[None, :])
    out = rik < (ri + rk) * F(ratio)
    with np.errstate(all="ignore"):
        vol = sphere_overlap(rik, ri, rk)
        v = ((4 * math.pi / 3) * (r * r * r).astype(np.float64)).astype(F)
        vi, vk = np.broadcast_arrays(v[:, None], v[None, :])
        v_large, v_small = np.where(vk > vi, vk, vi), np.where(vk > vi, vi, vk)
        out = out | (vol / v_small > F(max_small)) | (vol / v_large > F(max_large))
    return out


def cells(c, d, bmin, scale):
    C = np.floor((c - bmin.astype(F)[None, :]) / F(scale)).astype(np.int64)
    R = np.ceil((d / F(2)) / F(scale)).astype(np.int64) + 1
    return C, R


def _ball(R):
    j = np.arange(-R, R + 1)
    J = np.stack(np.meshgrid(j, j, j, indexing="ij"), -1).reshape(-1, 3)
    return J[(J * J).sum(1) <= R * R]


def share_pairs(C, R, tsz, ii, kk):
    """share(i, k) for the listed pairs: the cells of the smaller ball, one by one"""
    out = np.zeros(len(ii), bool)
    small = np.where(R[ii] <= R[kk], ii, kk)
    large = np.where(R[ii] <= R[kk], kk, ii)
    for Rs in np.unique(R[small]):
        J = _ball(int(Rs))
        sel = np.nonzero(R[small] == Rs)[0]
        step = max(1, 2000000 // len(J))
        for a in range(0, len(sel), step):
            q = sel[a:a + step]
            cell = C[small[q]][:, None, :] + J[None, :, :]
            ok = ((cell >= 0) & (cell < tsz[None, None, :])).all(2)
            far = cell - C[large[q]][:, None, :]
            ok &= (far * far).sum(2) <= (R[large[q]] ** 2)[:, None]
            out[q] = ok.any(1)
    return out


def share_table(C, R, tsz):
    """share as a matrix, through every blob's set of table cells (for small tables)"""
    g = np.stack(np.meshgrid(*[np.arange(t) for t in tsz], indexing="ij"), -1).reshape(-1, 3)
    n = len(R)
    out = np.zeros((n, n), bool)
    for a in range(0, len(g), 4096):
        far = g[None, a:a + 4096, :] - C[:, None, :]
        M = ((far * far).sum(2) <= (R * R)[:, None]).astype(np.float32)
        out |= (M @ M.T) > 0
    return out


def conflict_matrix(c, d, ratio, max_large, max_small, scale, cell_rule=True):
    """conf[i, k] = share(i, k) and crit(i, k), for all pairs of the sorted list, and (tsz, C, R)"""
    n = len(d)
    bmin, bmax = bounds_formula(c, d)
    tsz = (1 + bmax - bmin) // scale if n else np.zeros(3, np.int64)   # non-negative numerators for finite inputs
    crit = crit_matrix(c, d, ratio, max_large, max_small)
    if (tsz <= 0).any():
        return np.zeros((n, n), bool), tsz, None, None
    C, R = cells(c, d, bmin, scale)
    if not cell_rule:
        return crit, tsz, C, R
    if int(np.prod(tsz)) * n <= 4000000:
        return crit & share_table(C, R, tsz), tsz, C, R
    far = C[:, None, :] - C[None, :, :]
    pre = (far * far).sum(2) <= (R[:, None] + R[None, :]) ** 2     # necessary: spares the enumeration, decides nothing
    ii, kk = np.nonzero(np.tril(crit & pre, -1))
    ok = share_pairs(C, R, tsz, ii, kk)
    conf = np.zeros((n, n), bool)
    conf[ii[ok], kk[ok]] = True
    return conf | conf.T, tsz, C, R


def keep_from(conf, predecessors_only=True):
    n = len(conf)
    if predecessors_only:
        keep = np.zeros(n, bool)
        for i in range(n):
            keep[i] = not (conf[i, :i] & keep[:i]).any()
        return keep
    keep = np.ones(n, bool)       # the mutant: any kept blob counts, also those further down the list
    for i in range(n):
        row = conf[i] & keep
        row[i] = False
        keep[i] = not row.any()
    return keep


def rounds_of(conf):
    """Jacobi rounds until every blob is decided: discarded with a kept conflicting predecessor, kept with no undecided
    one left.  The length of the longest dependency chain."""
    low = np.tril(conf, -1)
    n = len(conf)
    kept, gone = np.zeros(n, bool), np.zeros(n, bool)
    rounds = 0
    while not (kept | gone).all():
        und = ~(kept | gone)
        hit = (low & kept[None, :]).any(1)
        wait = (low & und[None, :]).any(1)
        gone, kept = gone | (und & hit), kept | (und & ~hit & ~wait)
        rounds += 1
    return rounds, kept


def discard_overlapping_blobs(crds, diameters, scores, min_sep, max_large=np.inf, max_small=np.inf,
                              criteria=SORT_DECREASING_MAGNITUDE, scale=6, cell_rule=True, predecessors_only=True,
                              reverse_ties=True, info=None):
    c, d, s = np.asarray(crds, F).reshape(-1, 3), np.asarray(diameters, F), np.asarray(scores, F)
    order = rank(s, criteria, reverse_ties)
    c, d, s = c[order], d[order], s[order]
    if len(d) == 0:
        return c, d, s
    conf, tsz, _, _ = conflict_matrix(c, d, min_sep, max_large, max_small, scale, cell_rule)
    keep = keep_from(conf, predecessors_only)
    if info is not None:
        info["rounds"], kept2 = rounds_of(conf)
        assert np.array_equal(kept2, keep_from(conf))
        info["tsz"] = tsz
    return c[keep], d[keep], s[keep]
