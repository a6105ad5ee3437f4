"""A numpy float32 restatement of visfd_hip_surface_points (connect.cpp; reference handlers.cpp:2039-2309): all selected
voxels walk at once, one vectorised statement per statement of the host loop, every operand float32 (numpy rounds each
operation to float32 and never contracts).  The 3x3 eigen solve of the ridge snap goes through
visfd_hip_diagonalize_sym3_f32_host.  `mutant` breaks one thing on purpose (tests/test_surface_points.py):
    "fma"    the step r += ds * drds with one rounding
    "order"  the weighted sums forward entries first
    "rint"   round half to even instead of half away from zero"""
import numpy as np

from connect_graph_np import hessian_fd

F = np.float32


def roundf(x):
    """C's roundf on float32 arrays: halves away from zero, exact"""
    t = np.trunc(x)
    d = x - t                                     # exact
    return (t + np.where(np.abs(d) >= F(0.5), np.sign(x), F(0)).astype(F)).astype(F)


def _length3(v):
    return np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])


def _inside(p, shape):
    nz, ny, nx = shape
    return (p[:, 0] >= 0) & (p[:, 0] < nx) & (p[:, 1] >= 0) & (p[:, 1] < ny) & (p[:, 2] >= 0) & (p[:, 2] < nz)


def surface_points(saliency, direction, voxel2cluster=None, mask=None, select_cluster=1, voxel_width=(1, 1, 1), curve_ds=0.2,
                   find_ridge=True, max_distance_to_feature=1.3, mutant=None, want_steps=False):
    S, V, C, M = saliency, direction, voxel2cluster, mask
    shape = S.shape
    nz, ny, nx = shape
    vw = np.asarray(voxel_width, F)
    rnd = (lambda x: np.rint(x).astype(F)) if mutant == "rint" else roundf
    Sf, Vf = S.ravel(), V.reshape(-1, 3)
    Mf = None if M is None else M.ravel()
    sel = np.ones(S.size, bool) if M is None else (Mf != 0)
    if C is None:
        idx = np.flatnonzero(sel)
        xyz = np.stack([(idx % nx).astype(F) * vw[0], ((idx // nx) % ny).astype(F) * vw[1], (idx // (nx * ny)).astype(F) * vw[2]], 1)
        return (xyz.astype(F), Vf[idx].copy()) + ((0,) if want_steps else ())
    Cf = C.ravel()
    idx = np.flatnonzero(sel & (Cf == F(select_cluster)))
    n = len(idx)
    start = np.stack([idx % nx, (idx // nx) % ny, idx // (nx * ny)], 1).astype(F)
    Sc, Cc = Sf[idx], Cf[idx]
    xyz = start.copy()
    cn = idx.copy()
    longest = 0
    ds = F(curve_ds)

    def member(r):
        """the loop test at the positions r: -> (passes, voxel index where it does)"""
        p = rnd(r).astype(np.int64)
        ok = _inside(p, shape)
        c = np.where(ok, (p[:, 2] * ny + p[:, 1]) * nx + p[:, 0], 0)
        if Mf is not None:
            ok &= Mf[c] != 0
        ok &= Cf[c] == Cc
        return ok, c

    def step(r, c, sign):
        v = Vf[c]
        drds = v / _length3(v)[:, None]
        if mutant == "fma":
            return (r.astype(np.float64) + sign * np.float64(ds) * drds.astype(np.float64)).astype(F)
        return (r + ds * drds).astype(F) if sign > 0 else (r - ds * drds).astype(F)

    if n and ds > 0:
        with np.errstate(all="ignore"):
            # forward: entry 0 is the voxel itself
            fS, fR, fW, fA = [], [], [], []
            s, r, c, alive = F(0), start.copy(), idx.copy(), np.ones(n, bool)
            while alive.any():
                fS.append(s); fR.append(r.copy()); fW.append(Sf[c]); fA.append(alive.copy())
                r = step(r, c, +1)
                s = F(s + ds)
                ok, c2 = member(r)
                alive = alive & ok
                c = np.where(alive, c2, c)
            bS, bR, bW, bA = [], [], [], []
            s, r, c, alive = F(0), start.copy(), idx.copy(), np.ones(n, bool)
            while True:
                r = step(r, c, -1)
                s = F(s - ds)
                ok, c2 = member(r)
                alive = alive & ok
                if not alive.any():
                    break
                c = np.where(alive, c2, c)
                bS.append(s); bR.append(r.copy()); bW.append(Sf[c]); bA.append(alive.copy())
            longest = max(len(fS) - 1, len(bS))
            # the joined list, most negative s first; a lane's entries are contiguous in it
            jS = bS[::-1] + fS
            jR = np.stack(bR[::-1] + fR, 0)            # [entry][lane][3]
            jW = np.stack(bW[::-1] + fW, 0)
            jA = np.stack(bA[::-1] + fA, 0)
            jSv = np.asarray(jS, F)
            order = range(len(jS))
            if mutant == "order":
                order = list(range(len(bS), len(jS))) + list(range(len(bS)))
            sum_s, sum_w = np.zeros(n, F), np.zeros(n, F)
            for e in order:
                a = jA[e]
                sum_s = np.where(a, sum_s + jW[e] * jSv[e], sum_s).astype(F)
                sum_w = np.where(a, sum_w + jW[e], sum_w).astype(F)
            ave = sum_s / sum_w
            lo = jA.argmax(0)                          # the lane's first entry
            size = jA.sum(0)
            i = np.zeros(n, np.int64)                  # relative to lo
            done = np.zeros(n, bool)
            for k in range(1, len(jS)):
                run = ~done & (i + 1 < size)
                i = np.where(run, i + 1, i)
                e = lo + i
                hit = run & (jSv[e - 1] <= ave) & (ave <= jSv[e])
                done |= hit | ~run
            e = lo + i
            lanes = np.arange(n)
            has_next = i + 1 < size
            e1 = np.where(has_next, e + 1, e)
            ri, rj = jR[e, lanes], jR[e1, lanes]
            si, sj = jSv[e], jSv[e1]
            t = (ave - si) / (sj - si)
            xyz = np.where(has_next[:, None], ri + (rj - ri) * t[:, None], ri).astype(F)
            p = rnd(ri).astype(np.int64)
            cn = (p[:, 2] * ny + p[:, 1]) * nx + p[:, 0]
    with np.errstate(all="ignore"):
        v = Vf[cn]
        normal = (v / _length3(v)[:, None]).astype(F)
        normal = (normal * Sc[:, None]).astype(F)
    if find_ridge and n:
        from visfd_amd import api
        p0 = rnd(xyz)
        pi = p0.astype(np.int64)
        assert _inside(pi, shape).all(), "a walked point rounds outside the image: the host entry reads out of range here"
        H6 = hessian_fd(S).reshape(-1, 6)[(pi[:, 2] * ny + pi[:, 1]) * nx + pi[:, 0]]
        g = np.stack([np.clip(pi[:, 0], 1, nx - 2), np.clip(pi[:, 1], 1, ny - 2), np.clip(pi[:, 2], 1, nz - 2)], 1)
        at = lambda dx, dy, dz: S[g[:, 2] + dz, g[:, 1] + dy, g[:, 0] + dx]
        half = lambda a: (0.5 * a.astype(np.float64)).astype(F)
        grad = np.stack([half(at(1, 0, 0) - at(-1, 0, 0)), half(at(0, 1, 0) - at(0, -1, 0)), half(at(0, 0, 1) - at(0, 0, -1))], 1)
        H = np.empty((n, 3, 3), F)
        H[:, 0, 0], H[:, 1, 1], H[:, 2, 2] = H6[:, 0], H6[:, 1], H6[:, 2]
        H[:, 0, 1] = H[:, 1, 0] = H6[:, 3]
        H[:, 1, 2] = H[:, 2, 1] = H6[:, 4]
        H[:, 0, 2] = H[:, 2, 0] = H6[:, 5]
        ev, E = api.diagonalize_sym3_f32_host(H, 3)    # DECREASING_ABS
        e0 = E[:, 0, :]
        with np.errstate(all="ignore"):
            g1 = (grad[:, 0] * e0[:, 0] + grad[:, 1] * e0[:, 1] + grad[:, 2] * e0[:, 2]).astype(F)
            keep = g1 != 0
            neg = g1 < 0
            g1 = np.where(neg, -g1, g1)
            e0 = np.where(neg[:, None], -e0, e0)
            dist = np.where(ev[:, 0] != 0, g1 / ev[:, 0], F(np.inf)).astype(F)
            if F(max_distance_to_feature) > 0:
                keep &= ~(np.abs(dist) > F(max_distance_to_feature))
            snapped = (p0 - dist[:, None] * e0).astype(F)
            size3 = np.asarray([nx, ny, nz], F)
            keep &= ~((snapped < 0) | (size3 < snapped)).any(1)
            xyz = (snapped * vw).astype(F)
        xyz, normal = xyz[keep], normal[keep]
    return (np.ascontiguousarray(xyz, F), np.ascontiguousarray(normal, F)) + ((longest,) if want_steps else ())
