"""LabelConnected (connect.hpp:168-1427) restated without its priority queue: what csrc/connect.cpp computes, written
as a property of each voxel and its neighbours.  numpy only.

  valid voxel      unmasked, passes the saliency threshold, the tensor test and the vector test (19-point stencil)
  compatible edge  two valid neighbours whose neighbour tests pass in both directions
  cluster          a connected component of (valid voxels, compatible edges) that holds a valid seed; provisional
                   number = order of its lowest-ranked valid seed; final number by size
  directions       every compatible edge carries the sign of dot(v_i, v_j); in a balanced component the labelled voxels
                   get the unique consistent orientation in which the lowest-ranked valid seed keeps its direction,
                   then the outward flip of the whole cluster
  halo             the flood also turns the direction of every UNLABELLED unmasked voxel it reaches through a passing
                   neighbour test towards the voxel that reached it, and leaves it so (connect.hpp: the flip on
                   queueing, connect.cpp "newcomers follow the voxel that reached them").  Which voxel reached it last,
                   and in which basin's orientation, is the pop order's business; the result is order-free only when
                   every labelled voxel that reaches it agrees and every valid seed of the component shares the
                   anchor's orientation.

Where the flood's pop order can matter the function says so in `reasons` (a bit set) and its other results mean
nothing; csrc/connect.cpp is then the only definition.

Written for test volumes of some 10^4 to 10^5 voxels: the plateaus of the seed search and the components are joined by
union-finds in Python dicts, one step per equal or compatible neighbour pair (a second for 28 x 34 x 40); a 256^3 image
would take hours.
"""
import math

import numpy as np

from visfd_amd import api

ASYMMETRIC, ZERO_DOT, UNBALANCED, MUST_LINK, WEIGHTS, OUTWARD, LIMITS, HALO = (1 << k for k in range(8))
REASON_NAMES = {ASYMMETRIC: "asymmetric edge", ZERO_DOT: "zero dot product", UNBALANCED: "unbalanced signs",
                MUST_LINK: "must-link", WEIGHTS: "voxel weights", OUTWARD: "outward sum near zero", LIMITS: "limits",
                HALO: "halo direction depends on the pop order"}
OUTWARD_GUARD = 2.0 ** -20      # |sum| must exceed count * max|term| * this for its sign to be taken

F = np.float32


def reason_names(bits):
    return [n for b, n in REASON_NAMES.items() if bits & b]


def neighbour_offsets(connectivity):
    """(dx, dy, dz) of the forward half of connect.hpp:219-250's neighbourhood (raster order after the centre)."""
    r = int(math.floor(math.sqrt(connectivity)))
    out = []
    for dz in range(0, r + 1):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if dx * dx + dy * dy + dz * dz > connectivity or (dz, dy, dx) <= (0, 0, 0):
                    continue
                out.append((dx, dy, dz))
    return out


def _pairs(shape, off, idx):
    """linear indices (i, j = i + off) of all in-image pairs"""
    nz, ny, nx = shape
    dx, dy, dz = off

    def sl(n, d):
        return (slice(max(0, -d), n - max(0, d)), slice(max(0, d), n - max(0, -d)))
    (zi, zj), (yi, yj), (xi, xj) = sl(nz, dz), sl(ny, dy), sl(nx, dx)
    return idx[zi, yi, xi].ravel(), idx[zj, yj, xj].ravel()


def _trace_product(a, b):
    """the value the reference's TraceProductSym3 returns (connect.cpp header), operand order kept; a, b [..., 6]"""
    a0, a1, a2 = a[..., 0], a[..., 1], a[..., 2]
    b0, b1, b2 = b[..., 0], b[..., 1], b[..., 2]
    return a0 * b0 + a0 * b1 + a1 * b2 + a1 * b0 + a1 * b1 + a2 * b2 + a2 * b1 + a2 * b2 + a0 * b0


def _frobenius(a):
    return np.sqrt(_trace_product(a, a))


def _dot3(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def hessian_fd(S):
    """visfd_utils.hpp:528-616 for every voxel: flat (xx, yy, zz, xy, yz, xz), stencil moved inwards at the faces"""
    nz, ny, nx = S.shape
    cz, cy, cx = (np.clip(np.arange(n), 1, n - 2) for n in (nz, ny, nx))

    def s(dx, dy, dz):
        return S[np.ix_(cz + dz, cy + dy, cx + dx)]
    c = s(0, 0, 0)
    two = F(2)
    H = np.empty(S.shape + (6,), F)
    H[..., 0] = s(1, 0, 0) + s(-1, 0, 0) - two * c
    H[..., 1] = s(0, 1, 0) + s(0, -1, 0) - two * c
    H[..., 2] = s(0, 0, 1) + s(0, 0, -1) - two * c
    q = lambda v: (0.25 * v.astype(np.float64)).astype(F)
    H[..., 3] = q(s(1, 1, 0) + s(-1, -1, 0) - s(1, -1, 0) - s(-1, 1, 0))
    H[..., 4] = q(s(0, 1, 1) + s(0, -1, -1) - s(0, 1, -1) - s(0, -1, 1))
    H[..., 5] = q(s(1, 0, 1) + s(-1, 0, -1) - s(-1, 0, 1) - s(1, 0, -1))
    return H


def find_seeds(S, M, seek_minima, threshold, connectivity):
    """connect.cpp find_extrema: plateau-aware extrema, the first voxel of each plateau in raster order, ranked"""
    threshold = F(threshold)
    if not seek_minima and threshold == np.inf:
        threshold = F(-np.inf)
    shape = S.shape
    n = S.size
    idx = np.arange(n, dtype=np.int64).reshape(shape)
    Sf = S.ravel()
    ok = np.ones(n, bool) if M is None else (M.ravel() != 0)
    lower = np.zeros(n, bool)      # has a lower existing neighbour
    higher = np.zeros(n, bool)
    eq_pairs = []
    for off in neighbour_offsets(connectivity):
        i, j = _pairs(shape, off, idx)
        both = ok[i] & ok[j]
        i, j = i[both], j[both]
        vi, vj = Sf[i], Sf[j]
        lower[i[vj < vi]] = True
        higher[i[vj > vi]] = True
        lower[j[vi < vj]] = True
        higher[j[vi > vj]] = True
        e = vi == vj
        eq_pairs.append(np.stack([i[e], j[e]], 1))
    parent = {}

    def find(a):
        r = a
        while parent.get(r, r) != r:
            r = parent[r]
        while parent.get(a, a) != r:
            parent[a], a = r, parent[a]
        return r
    for a, b in np.concatenate(eq_pairs, 0).tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)       # the root is the first voxel in raster order
    for a in list(parent):
        r = find(a)
        if r != a:
            lower[r] |= lower[a]
            higher[r] |= higher[a]
    is_root = ok.copy()
    for a in parent:
        if find(a) != a:
            is_root[a] = False
    if seek_minima:
        cand = np.flatnonzero(is_root & ~lower & (Sf <= threshold))
    else:
        cand = np.flatnonzero(is_root & ~higher & (Sf >= threshold))
    score = Sf[cand]
    order = np.lexsort((np.arange(len(cand)), score))       # ascending (score, raster rank)
    if not seek_minima:
        order = order[::-1]
    return cand[order], score[order]


class _Parity:
    """union-find over voxel indices with the relative sign of each voxel to its parent"""

    def __init__(self):
        self.parent, self.par = {}, {}

    def find(self, a):
        path = []
        while self.parent.get(a, a) != a:
            path.append(a)
            a = self.parent[a]
        # compress: parity to the root is the XOR along the path
        acc = 0
        for v in reversed(path):
            acc ^= self.par[v]
            self.parent[v], self.par[v] = a, acc
        return a

    def root_parity(self, a):
        r = self.find(a)
        return r, (self.par.get(a, 0) if a != r else 0)

    def union(self, a, b, sign):
        """False when a and b are already joined with the other relative sign"""
        ra, pa = self.root_parity(a)
        rb, pb = self.root_parity(b)
        if ra == rb:
            return (pa ^ pb) == sign
        if ra > rb:
            ra, rb, pa, pb = rb, ra, pb, pa
        self.parent[rb], self.par[rb] = ra, pa ^ pb ^ sign
        return True


def label_connected_graph(saliency, threshold_saliency, mask=None, direction=None, tensor=None,
                          threshold_vector_saliency=-np.inf, threshold_vector_neighbor=-np.inf,
                          consider_dot_product_sign=True, threshold_tensor_saliency=-np.inf,
                          threshold_tensor_neighbor=-np.inf, tensor_is_positive_definite_near_target=True, connectivity=1,
                          label_undefined=-1, sort_by_size=True, standardize_directions=False,
                          start_from_saliency_maxima=True, voxel_weights=None, must_link=None, must_link_directions=None):
    """api.label_connected's arguments -> dict(labels, n_clusters, seeds, sizes, seed_saliencies, direction, reasons,
    valid, n_valid).  `direction` is NOT rewritten in place; the standardised copy is returned (None without one)."""
    S = np.ascontiguousarray(saliency, F)
    shape = S.shape
    nz, ny, nx = shape
    n = S.size
    reasons = 0
    if must_link:
        reasons |= MUST_LINK
    if voxel_weights is not None:
        reasons |= WEIGHTS
    if connectivity > 3 or n >= 2 ** 31 - 2:
        reasons |= LIMITS
    M = None if mask is None else np.ascontiguousarray(mask, F)
    V = None if direction is None else np.ascontiguousarray(direction, F).reshape(n, 3)
    T = None if tensor is None else np.ascontiguousarray(tensor, F).reshape(n, 6)
    from_max = bool(start_from_saliency_maxima)
    signs = bool(consider_dot_product_sign)
    standardize = V is not None and bool(standardize_directions) and not signs
    thr, tvs, tvn = F(threshold_saliency), F(threshold_vector_saliency), F(threshold_vector_neighbor)
    tts, ttn = F(threshold_tensor_saliency), F(threshold_tensor_neighbor)
    if not signs:
        tvs = F(0) if tvs < 0 else tvs
        tvn = F(0) if tvn < 0 else tvn
    SIGN = F(-1) if from_max else F(1)
    idx = np.arange(n, dtype=np.int64).reshape(shape)
    Sf = S.ravel()
    unmasked = np.ones(n, bool) if M is None else (M.ravel() != 0)

    with np.errstate(all="ignore"):
        # ---- valid voxels (connect.hpp:445-570)
        valid = unmasked & ~((Sf * SIGN) > (thr * SIGN))
        if T is not None or V is not None:
            H = hessian_fd(S).reshape(n, 6)
            if bool(tensor_is_positive_definite_near_target) == from_max:
                H = H * F(-1)
        if T is not None:
            valid &= ~(_trace_product(H, T) < tts * _frobenius(H) * _frobenius(T))
        if V is not None:
            order = 1 if from_max else 0          # VISFD_HIP_DECREASING_EIVALS : _INCREASING_
            e0 = api.principal_directions_host(np.ascontiguousarray(H), order)      # row 0 of ConvertFlatSym2Evects3
            if signs:
                valid &= ~(_dot3(e0, V) < tvs * np.sqrt(_dot3(e0, e0)) * np.sqrt(_dot3(V, V)))
            else:
                d = _dot3(e0, V)
                valid &= ~(d * d < (tvs * tvs) * _dot3(e0, e0) * _dot3(V, V))

        # ---- seeds
        seed, seed_score = find_seeds(S, M, not from_max, thr, connectivity)
        nseeds = len(seed)

        # ---- edges: both directed tests of every pair in the forward half-neighbourhood (connect.hpp:625-672)
        def passes(i, j):       # the test as the flood evaluates it when i is popped and looks at j
            ok = unmasked[j].copy()
            if T is not None:
                ti, tj = T[i], T[j]
                ok &= ~(_trace_product(ti, tj) < ttn * _frobenius(ti) * _frobenius(tj))
                if V is not None:
                    vi, vj = V[i], V[j]
                    if signs:      # quirk kept: the signed form uses the tensor threshold
                        ok &= ~(_dot3(vi, vj) < ttn * np.sqrt(_dot3(vi, vi)) * np.sqrt(_dot3(vj, vj)))
                    else:
                        d = _dot3(vi, vj)
                        ok &= ~(d * d < (tvn * tvn) * _dot3(vi, vi) * _dot3(vj, vj))
            return ok
        uf = _Parity()
        edges = []              # (i, j, sign) of the compatible edges
        reach = []              # (from, to, dot) where a valid voxel's test towards a non-valid unmasked voxel passes
        for off in neighbour_offsets(connectivity):
            i, j = _pairs(shape, off, idx)
            any_valid = valid[i] | valid[j]
            i, j = i[any_valid], j[any_valid]
            fwd, bwd = passes(i, j), passes(j, i)
            dots = _dot3(V[i], V[j]) if V is not None else np.zeros(len(i), F)
            both = valid[i] & valid[j]
            if np.any(both & (fwd != bwd)):
                reasons |= ASYMMETRIC
            e = both & fwd & bwd
            if standardize and np.any(e & (dots == 0)):
                reasons |= ZERO_DOT
            edges.append((i[e], j[e], (dots[e] < 0).astype(np.int8)))
            a = valid[i] & ~valid[j] & fwd
            b = valid[j] & ~valid[i] & bwd
            reach.append((np.concatenate([i[a], j[b]]), np.concatenate([j[a], i[b]]), np.concatenate([dots[a], dots[b]])))
        ei = np.concatenate([e[0] for e in edges])
        ej = np.concatenate([e[1] for e in edges])
        es = np.concatenate([e[2] for e in edges])
        for a, b, s in zip(ei.tolist(), ej.tolist(), es.tolist()):
            if not uf.union(a, b, s if standardize else 0):
                reasons |= UNBALANCED

        # ---- components with a valid seed, numbered by their lowest-ranked valid seed
        vox = np.flatnonzero(valid)
        rp = [uf.root_parity(v) for v in vox.tolist()]
        root = np.full(n, -1, np.int64)
        par = np.zeros(n, np.int8)           # sign relative to the component's root
        root[vox] = [r for r, _ in rp]
        par[vox] = [p for _, p in rp]
        anchor = {}                          # root -> rank of the lowest-ranked valid seed
        for rank, c in enumerate(seed.tolist()):
            if valid[c]:
                anchor.setdefault(int(root[c]), rank)
        deepest = sorted(anchor.values())    # provisional cluster k <- seed rank
        prov_of_root = {r: k for k, r in enumerate(sorted(anchor, key=anchor.get))}
        n_clusters = len(deepest)
        prov = np.full(n, -1, np.int64)
        if n_clusters:
            lut_keys = np.array(list(prov_of_root.keys()), np.int64)
            lut_vals = np.array(list(prov_of_root.values()), np.int64)
            srt = np.argsort(lut_keys)
            lut_keys, lut_vals = lut_keys[srt], lut_vals[srt]
            pos = np.searchsorted(lut_keys, root[vox])
            pos[pos >= len(lut_keys)] = 0
            hit = lut_keys[pos] == root[vox]
            prov[vox[hit]] = lut_vals[pos[hit]]
        live = prov >= 0
        sizes = np.bincount(prov[live], minlength=n_clusters).astype(np.int64)

        # ---- standardised directions
        Vout = None if V is None else V.copy()
        detail = {}
        if standardize:
            # sign of every labelled voxel relative to its cluster's anchor seed
            anchor_par = np.zeros(n_clusters, np.int8)
            for k, rank in enumerate(deepest):
                anchor_par[k] = par[seed[rank]]
            rel = np.zeros(n, np.int8)
            rel[live] = par[live] ^ anchor_par[prov[live]]
            # every valid seed of a labelled component must share the anchor's orientation, or the basins' own
            # orientations (which the halo sees) differ from the final one
            detail["seeds_against_anchor"] = int(sum(1 for c in seed.tolist() if live[c] and rel[c]))
            if detail["seeds_against_anchor"]:
                reasons |= HALO
            flip = np.where(rel == 1, F(-1), F(1))
            Vout[live] = Vout[live] * flip[live, None]
            # the halo: unlabelled voxels reached through a passing test turn towards the voxel that reached them
            src = np.concatenate([r[0] for r in reach])
            dst = np.concatenate([r[1] for r in reach])
            dts = np.concatenate([r[2] for r in reach])
            keep = live[src]
            src, dst, dts = src[keep], dst[keep], dts[keep]
            sgn = np.sign(dts) * np.where(rel[src] == 1, F(-1), F(1))
            if np.any(sgn == 0):
                reasons |= ZERO_DOT
            neg = np.zeros(n, bool)
            posi = np.zeros(n, bool)
            neg[dst[sgn < 0]] = True
            posi[dst[sgn > 0]] = True
            detail["halo"], detail["halo_disputed"] = int((neg | posi).sum()), int((neg & posi).sum())
            if detail["halo_disputed"]:
                reasons |= HALO
            # a discarded seed is waiting in the queue until it is popped; a voxel of equal saliency may reach it before
            is_seed = np.zeros(n, bool)
            is_seed[seed] = True
            if np.any(is_seed[dst] & (Sf[dst] == Sf[src])):
                reasons |= HALO
            Vout[neg & ~posi] *= F(-1)
            # outward orientation (connect.hpp:1186-1289): sign of sum (r - r_com) . n per cluster
            z, y, x = np.unravel_index(np.flatnonzero(live), shape)
            k = prov[live]
            LD = np.longdouble
            com = np.stack([np.bincount(k, c, n_clusters) for c in (x, y, z)], 1).astype(LD) / sizes.astype(LD)[:, None]
            r = (np.stack([x, y, z], 1).astype(LD) - com[k]).astype(F)
            term = _dot3(r, Vout[live])
            live_idx = np.flatnonzero(live)
            for c in range(n_clusters):
                t = term[k == c].astype(np.float64)
                total = math.fsum(t.tolist())
                bound = len(t) * float(np.max(np.abs(t))) * OUTWARD_GUARD
                if bound > 0 and not abs(total) > bound:       # all terms zero: the sum is an exact zero, no flip
                    reasons |= OUTWARD
                if total < 0:
                    Vout[live_idx[k == c]] *= F(-1)

        # ---- final numbers, labels, per-cluster outputs
        perm = np.arange(n_clusters)
        if sort_by_size and n_clusters:
            perm = np.lexsort((np.arange(n_clusters), sizes.astype(F)))[::-1]     # (float size, id) descending
        inv = np.empty(n_clusters, np.int64)
        inv[perm] = np.arange(n_clusters)
        labels = np.full(n, nseeds + 1, np.int64)
        labels[unmasked] = label_undefined
        labels[live] = inv[prov[live]] + 1
        deepest = np.array(deepest, np.int64)
        cm_idx = seed[deepest[perm]] if n_clusters else np.zeros(0, np.int64)
        seeds_xyz = np.stack([cm_idx % nx, (cm_idx // nx) % ny, cm_idx // (nx * ny)], 1).astype(F).reshape(-1, 3)
        seed_sal = Sf[seed[deepest]] if n_clusters else np.zeros(0, F)
    return dict(labels=labels.reshape(shape), n_clusters=n_clusters, seeds=seeds_xyz, sizes=sizes.astype(F),
                seed_saliencies=seed_sal, direction=None if Vout is None else Vout.reshape(shape + (3,)), reasons=reasons,
                valid=valid.reshape(shape), n_valid=int(valid.sum()), n_seeds=nseeds, detail=detail)
