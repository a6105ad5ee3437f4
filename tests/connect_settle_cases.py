"""Constructed calls for the option connect_settle of the graph entries of LabelConnected: must-links,
voxel weights and outward sums in doubt.  Shared by tests/test_connect_settle.py (CPU: the rule restated in numpy against
the flood) and tests/test_connect_settle_gpu.py (the device path against the flood).  Not a test file.

Shapes are (nz, ny, nx); they are the smallest that still cross a 64 x 8 x 8 tile of the seed search in each axis: 70 x 9 x 9,
9 x 12 x 9 and 9 x 9 x 12 voxels in (x, y, z), and 3 x 5 x 70.  Every case is a tuple (name, saliency, tensor, direction,
case, expect): `case` is a call as tests/connect_graph_contract.py splits it; `expect` says what the device path has to
report with the option on: the bits it settles, or the one reason it hands the call over for."""
import numpy as np

import connect_graph_np as cg

F = np.float32
X70, Y12, Z12, THIN = (9, 9, 70), (9, 12, 9), (12, 9, 9), (70, 5, 3)
_CALL = dict(use="v", consider_dot_product_sign=False, standardize_directions=True, threshold_vector_saliency=-2.0,
             connectivity=1, threshold_saliency=0.5)


def settled(*bits):
    return dict(path="device", settled=sum(bits))


def handed_over(reason):
    return dict(path="flood", reasons=reason)


def sheets(shape, zs, seed=3, top=None, normals="fan", holes=()):
    """Flat sheets of valid voxels, one voxel thick, at the planes zs; sheet k's saliency lies in (top[k], top[k] + 1), so
    the seed ranks, and with them the provisional cluster numbers, follow `top` (default: the first sheet ranks first).
    normals: "fan" = unit vectors away from a point 40 voxels below the image, each with a random sign (a cluster's
    outward sum is then far from zero however its sheets are oriented), or one vector per sheet, with random signs too.
    holes: (sheet, x, y, radius squared): the voxels of that sheet nearer than that to (x, y) are cut out."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    sal = np.zeros(shape, F)
    top = list(range(len(zs), 0, -1)) if top is None else top
    for k, z in enumerate(zs):
        sal[z] = top[k] + rng.random((ny, nx)).astype(F)
    yy, xx = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    for k, x0, y0, r2 in holes:
        sal[zs[k]][(xx - x0) ** 2 + (yy - y0) ** 2 < r2] = 0
    z, y, x = np.meshgrid(np.arange(nz) + 40.0, np.arange(ny) - ny / 2 + 0.3, np.arange(nx) - nx / 2 + 0.3, indexing="ij")
    d = np.stack([x, y, z], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    if normals != "fan":
        for k, zk in enumerate(zs):
            d[zk] = np.asarray(normals[k])
    d *= np.where(rng.random(shape) < 0.5, -1.0, 1.0)[..., None]
    return sal, np.ascontiguousarray(d.astype(F))


def corrugated(shape, nz_sign=1.0):
    """z = 3 on even x, z = 4 on odd x, normals all along z: every term of the outward sum is +-0.5 (an even number of
    columns: the sum is an exact zero) or a rounding of it (an odd number: the centre of mass is not representable)"""
    rng = np.random.default_rng(8)
    nz, ny, nx = shape
    sal = np.zeros(shape, F)
    v = 1 + rng.random((ny, nx)).astype(F)
    sal[3, :, 0::2] = v[:, 0::2]
    sal[4, :, 1::2] = v[:, 1::2]
    d = np.zeros(shape + (3,), F)
    d[..., 2] = nz_sign
    return sal, d


def must_link_cases():
    out = []
    sal, d = sheets(X70, (2, 5))
    far = [[(5.0, 4.0, 2.0), (60.0, 4.0, 5.0)]]         # the contact line lies across the normals: both angles small
    near = [[(30.0, 4.0, 2.0), (30.0, 4.0, 5.0)]]       # along them: the auto rule takes its other branch
    for how, tag in ((0, "same"), (1, "opposite"), (2, "auto")):
        out.append(("ml across %s" % tag, sal, None, d, dict(_CALL, must_link=far, must_link_directions=[[how, how]]),
                    settled(cg.MUST_LINK)))
    out.append(("ml along auto", sal, None, d, dict(_CALL, must_link=near), settled(cg.MUST_LINK)))
    # at 80 degrees to the normals: dz = 3 against a lateral step of 17
    out.append(("ml 80 degrees auto", sal, None, d, dict(_CALL, must_link=[[(20.0, 4.0, 2.0), (37.0, 4.0, 5.0)]]),
                settled(cg.MUST_LINK)))
    out.append(("ml off grid and outside", sal, None, d,
                dict(_CALL, must_link=[[(11.5, 3.5, 1.5), (-6.0, 20.0, 7.5)]]), settled(cg.MUST_LINK)))
    out.append(("ml inside one cluster", sal, None, d, dict(_CALL, must_link=[[(3.0, 2.0, 2.0), (66.0, 7.0, 2.0)]]),
                settled(cg.MUST_LINK)))
    # a tie across clusters: from (30, 4, 3) the lower sheet is cut out to a lateral distance of 2 (1 + 4), the upper one
    # to 1 (4 + 1); the lowest voxel index is the lower sheet's, the cluster of the second location: nothing merges
    tie_sal, tie_d = sheets(X70, (2, 5), holes=((0, 30, 4, 4), (1, 30, 4, 1)))
    out.append(("ml tie", tie_sal, None, tie_d, dict(_CALL, must_link=[[(30.0, 4.0, 3.0), (3.0, 2.0, 2.0)]]),
                settled(cg.MUST_LINK)))
    sal3, d3 = sheets(Z12, (2, 5, 8))
    out.append(("ml chain of three", sal3, None, d3,
                dict(_CALL, must_link=[[(1.0, 1.0, 2.0), (7.0, 7.0, 5.0), (4.0, 4.0, 8.0)]]), settled(cg.MUST_LINK)))
    sal3y, d3y = sheets(Y12, (1, 4, 7))
    out.append(("ml two groups", sal3y, None, d3y,
                dict(_CALL, must_link=[[(1.0, 1.0, 1.0), (7.0, 10.0, 4.0)], [(2.0, 3.0, 4.0), (6.0, 6.0, 7.0)]],
                     must_link_directions=[[2, 1], [0, 0]]), settled(cg.MUST_LINK)))
    # the third sheet is absorbed and negated by the second (opposite), then both by the first through a voxel of the third
    out.append(("ml absorbed twice", sal3, None, d3,
                dict(_CALL, must_link=[[(7.0, 1.0, 5.0), (2.0, 6.0, 8.0)], [(5.0, 5.0, 8.0), (1.0, 7.0, 2.0)]],
                     must_link_directions=[[1, 1], [0, 0]]), settled(cg.MUST_LINK)))
    thin_sal, thin_d = sheets(THIN, (10, 13, 66))
    out.append(("ml thin", thin_sal, None, thin_d,
                dict(_CALL, must_link=[[(1.0, 2.0, 10.0), (1.0, 3.0, 66.0)]]), settled(cg.MUST_LINK)))
    perp_sal, perp_d = sheets(X70, (2, 5), normals=((0.0, 0.0, 1.0), (1.0, 0.0, 0.0)))
    # exactly perpendicular contacts: the side the flood takes depends on the polarities its basins happen to have, which
    # differ from pair to pair
    for tag, how, pair in (("same", 0, far[0]), ("opposite", 1, [(12.0, 2.0, 2.0), (44.0, 6.0, 5.0)]),
                           ("same again", 0, [(33.0, 7.0, 5.0), (51.0, 1.0, 2.0)]),
                           ("opposite again", 1, [(66.0, 3.0, 2.0), (25.0, 5.0, 5.0)])):
        out.append(("ml perpendicular " + tag, perp_sal, None, perp_d,
                    dict(_CALL, must_link=[pair], must_link_directions=[[how, how]]), handed_over(cg.ZERO_DOT)))
    out.append(("ml a million voxels away", sal, None, d,
                dict(_CALL, must_link=[[(5.0, 4.0, 2.0), (1.0e6, 4.0, 5.0)]]), handed_over(cg.LIMITS)))
    return out


def weight_cases():
    out = []
    rng = np.random.default_rng(12)
    sal, d = sheets(X70, (2, 5), holes=((0, 20, 4, 30),))      # the first sheet is cut in two: three clusters
    w = rng.uniform(0.5, 2.0, sal.shape).astype(F)
    out.append(("w random", sal, None, d, dict(_CALL, voxel_weights=w), settled(cg.WEIGHTS)))
    w = np.ones(sal.shape, F)
    w[5] = 0.01                                                  # the larger sheet weighs less: the ranking turns over
    out.append(("w ranking inverted", sal, None, d, dict(_CALL, voxel_weights=w), settled(cg.WEIGHTS)))
    w = (2.0 ** rng.integers(-20, 21, sal.shape)).astype(F)
    out.append(("w 2^-20 to 2^20", sal, None, d, dict(_CALL, voxel_weights=w), settled(cg.WEIGHTS)))
    w = rng.uniform(0.5, 2.0, sal.shape).astype(F)
    w[5] = 0
    out.append(("w one cluster of zeros", sal, None, d, dict(_CALL, voxel_weights=w), settled(cg.WEIGHTS)))
    out.append(("w unsorted saliency only", sal, None, None,
                dict(threshold_saliency=0.5, connectivity=1, sort_by_size=False, voxel_weights=w), settled(cg.WEIGHTS)))
    return out


def outward_cases():
    call = dict(_CALL, connectivity=3)
    out = []
    for name, shape, sign in (("even columns", X70, 1.0), ("odd columns", Y12, 1.0), ("even columns facing down", X70, -1.0)):
        sal, d = corrugated(shape, sign)
        out.append(("outward " + name, sal, None, d, call, settled(cg.OUTWARD)))
    return out


def combined_case():
    """a corrugated sheet and a flat one, all normals along z, joined by a must-link, under weights"""
    sal, d = corrugated(X70)
    rng = np.random.default_rng(4)
    sal[7] = 3 + rng.random(sal.shape[1:]).astype(F)
    w = rng.uniform(0.5, 2.0, sal.shape).astype(F)
    case = dict(_CALL, connectivity=3, voxel_weights=w, must_link=[[(10.0, 4.0, 7.0), (50.4, 2.6, 3.0)]],
                must_link_directions=[[0, 0]])
    return ("combined", sal, None, d, case, settled(cg.MUST_LINK, cg.WEIGHTS))


def all_cases():
    return must_link_cases() + weight_cases() + outward_cases() + [combined_case()]
