"""Inputs of the surface-points tests (visfd_hip_surface_points and its device forms): small volumes with a sheet-like
cluster, its saliency and its normals.  Every case is a dict: saliency [nz, ny, nx], direction [nz, ny, nx, 3], cluster (the
labels as floats, or None), mask (or None), and the call's parameters.  Sheets are 7 voxels thick and the step is 0.2, so a
walk takes at most some 40 steps per direction: far below the device's default cap of 256, above the cap of 8 that one GPU
test sets."""
import numpy as np

F = np.float32


def sheet(shape, normal=(0.05, 0.08, 1.0), centre=None, half=3.5, seed=0, noise=0.05, sigma=2.0):
    """A planar sheet |d| <= half around `centre` (x, y, z; default the middle of the image) with unit normal ~ `normal`:
    the saliency is a Gaussian profile of the distance d to the mid-plane plus a little noise, the directions are the normal
    plus noise, normalised in float; -> saliency, direction, d."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    n0 = np.asarray(normal, np.float64)
    n0 /= np.linalg.norm(n0)
    c = np.array([(nx - 1) / 2, (ny - 1) / 2, (nz - 1) / 2]) if centre is None else np.asarray(centre, np.float64)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    d = (x - c[0]) * n0[0] + (y - c[1]) * n0[1] + (z - c[2]) * n0[2]
    sal = (np.exp(-d * d / (2 * sigma * sigma)) + 0.02 * rng.random(shape)).astype(F)
    v = (n0[None, None, None, :] + noise * rng.standard_normal(shape + (3,))).astype(F)
    v /= np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])[..., None]
    return sal, np.ascontiguousarray(v, F), d


def case(shape, **kw):
    p = dict(select_cluster=1, voxel_width=(1.0, 1.0, 1.0), curve_ds=0.2, find_ridge=True, max_distance_to_feature=1.3)
    geo = {k: kw.pop(k) for k in ("normal", "centre", "half", "seed", "noise") if k in kw}
    sal, v, d = sheet(shape, **geo)
    half = geo.get("half", 3.5)
    cluster = np.where(np.abs(d) <= half, F(1), F(0)).astype(F)
    mask = None
    edit = kw.pop("edit", None)
    p.update(kw)
    c = dict(saliency=sal, direction=v, cluster=cluster, mask=mask, d=d, **p)
    if edit:
        edit(c)
    del c["d"]
    for k in ("saliency", "direction", "cluster", "mask"):
        if c[k] is not None:
            c[k] = np.ascontiguousarray(c[k], F)
            c[k].setflags(write=False)
    return c


def _mask_cut(c):
    rng = np.random.default_rng(5)
    m = (c["d"] <= 1.2).astype(F)
    m[rng.random(m.shape) < 0.03] = 0      # and a few holes
    c["mask"] = m


def _two_clusters(c):
    c["cluster"] = np.where(np.abs(c["d"]) <= 3.5, np.where(c["d"] < 0, F(1), F(2)), F(0)).astype(F)


def _one_voxel(c):
    cl = np.zeros_like(c["cluster"])
    cl[5] = 1
    c["cluster"] = cl


def _non_unit(c):
    rng = np.random.default_rng(6)
    c["direction"] = c["direction"] * (10.0 ** rng.uniform(-1, 1, c["cluster"].shape)).astype(F)[..., None]


def _zero_column(c):
    s = c["saliency"].copy()
    s[:, 5:10, 10:15] = 0
    c["saliency"] = s


def _axis_exact(c):
    v = np.zeros_like(c["direction"])
    v[..., 2] = 1
    c["direction"] = v


def _plain_mask(c):
    rng = np.random.default_rng(7)
    c["cluster"] = None
    c["mask"] = (rng.random(c["saliency"].shape) < 0.3).astype(F)


def _plain(c):
    c["cluster"] = None


def _zero_direction(c):
    v = c["direction"].copy()
    nz, ny, nx = c["cluster"].shape
    v[nz // 2, ny // 2, nx // 2] = 0
    v[nz // 2, 3, 4] = 0
    c["direction"] = v


BASE = (12, 40, 70)
FACE = (14, 15, 17)   # nz, ny, nx


def _faces():
    out = {}
    nz, ny, nx = FACE
    mid = [(nx - 1) / 2, (ny - 1) / 2, (nz - 1) / 2]
    for axis, name in enumerate("xyz"):
        for side, at in (("lo", 1.0), ("hi", (nx, ny, nz)[axis] - 2.0)):
            normal = [0.06, 0.06, 0.06]
            normal[axis] = 1.0
            centre = list(mid)
            centre[axis] = at
            out["face_%s_%s" % (name, side)] = (lambda normal=tuple(normal), centre=tuple(centre):
                                                case(FACE, normal=normal, centre=centre, seed=11 + axis))
    return out


# name -> builder; every one of these is inside the bit contract (finite, non-zero directions)
CASES = {
    "sheet": lambda: case(BASE),
    "sheet_long_rows": lambda: case((9, 33, 130), seed=1),
    "sheet_thin_image": lambda: case((5, 3, 300), seed=2),
    "tilted": lambda: case(BASE, normal=(0.3, 0.2, 1.0), seed=3),
    "mask_cut": lambda: case(BASE, edit=_mask_cut),
    "two_clusters_1": lambda: case(BASE, edit=_two_clusters),
    "two_clusters_2": lambda: case(BASE, edit=_two_clusters, select_cluster=2),
    "one_voxel_ds1": lambda: case(BASE, edit=_one_voxel, curve_ds=1.0),
    "one_voxel": lambda: case(BASE, edit=_one_voxel),
    "non_unit": lambda: case(BASE, edit=_non_unit),
    "zero_saliency_column": lambda: case(BASE, edit=_zero_column),
    "axis_half_steps": lambda: case(BASE, edit=_axis_exact, curve_ds=0.5),
    "ds_zero": lambda: case(BASE, curve_ds=0.0),
    "no_cluster": lambda: case((6, 7, 21), edit=_plain),
    "no_cluster_masked": lambda: case((6, 7, 21), edit=_plain_mask, voxel_width=(1.5, 2.0, 0.75)),
    "no_ridge": lambda: case(BASE, find_ridge=False),
    "no_ridge_anisotropic": lambda: case(BASE, find_ridge=False, voxel_width=(1.5, 2.0, 0.75)),
    "maxd_off": lambda: case(BASE, max_distance_to_feature=-1.0),
    "maxd_small": lambda: case(BASE, max_distance_to_feature=0.4),
    "anisotropic": lambda: case(BASE, voxel_width=(1.5, 2.0, 0.75)),
    "absent_cluster": lambda: case((6, 7, 21), select_cluster=3),
}
CASES.update(_faces())
# The ridge snap starts from the ROUNDED walked position, so the last bits of a walk show only without it: the walks again
CASES.update({
    "tilted_no_ridge": lambda: case(BASE, normal=(0.3, 0.2, 1.0), seed=3, find_ridge=False),
    "long_rows_no_ridge": lambda: case((9, 33, 130), seed=1, find_ridge=False),
    "thin_image_no_ridge": lambda: case((5, 3, 300), seed=2, find_ridge=False),
    "mask_cut_no_ridge": lambda: case(BASE, edit=_mask_cut, find_ridge=False),
    "two_clusters_no_ridge": lambda: case(BASE, edit=_two_clusters, select_cluster=2, find_ridge=False),
    "non_unit_no_ridge": lambda: case(BASE, edit=_non_unit, find_ridge=False),
    "zero_saliency_no_ridge": lambda: case(BASE, edit=_zero_column, find_ridge=False),
    "one_voxel_no_ridge": lambda: case(BASE, edit=_one_voxel, find_ridge=False),
    "axis_half_steps_no_ridge": lambda: case(BASE, edit=_axis_exact, curve_ds=0.5, find_ridge=False),
})
CASES.update({k + "_no_ridge": (lambda f=f: dict(f(), find_ridge=False)) for k, f in _faces().items()})

# outside the bit contract: two zero-length directions inside the cluster
ZERO_DIRECTION = lambda: case(BASE, edit=_zero_direction)


# ---- the program scenario (tests/golden/make_golden_surface_points.py, tests/test_surface_points_gpu.py) -------------------
PROGRAM_SHAPE = (16, 10, 12)
PROGRAM_ARGS = ["-w", "1", "-in", "in.rec", "-membrane", "minima", "2", "-tv", "3", "-tv-angle-exponent", "4", "-bin", "1",
                "-load-progress", "prog", "-connect", "0.3", "-connect-angle", "30", "-normals-file", "n.ply",
                "-select-cluster", "1", "-out", "labels.rec"]


def program_scenario():
    """A thick sheet as vote tensors: T = a(d) n n^T with a = 1 / (1 + (d / 3)^2) (above the -connect threshold of 0.3 for
    |d| < 4.6: nine voxels) and normals n that wobble by a hash of the voxel's coordinates.  Only +, -, *, / and sqrt of
    doubles and integer arithmetic, so every machine builds the same bits.  -> (input image, [six tensor images])."""
    nz, ny, nx = PROGRAM_SHAPE
    z, y, x = np.meshgrid(np.arange(nz, dtype=np.int64), np.arange(ny, dtype=np.int64), np.arange(nx, dtype=np.int64),
                          indexing="ij")
    n0 = np.array([0.2, 0.1, 1.0])
    n0 = n0 / np.sqrt((n0 * n0).sum())
    d = (x - 5.5) * n0[0] + (y - 4.5) * n0[1] + (z - 7.5) * n0[2]
    a = 1.0 / (1.0 + (d / 3.0) * (d / 3.0))
    h = lambda k: (((x * 73856093) ^ (y * 19349663) ^ (z * 83492791) ^ (k * 2654435761)) % 1021) / 1021.0 - 0.5
    n = np.stack([n0[0] + 0.1 * h(1), n0[1] + 0.1 * h(2), n0[2] + 0.1 * h(3)], -1)
    n = n / np.sqrt((n * n).sum(-1))[..., None]
    pairs = ((0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (0, 2))
    tensors = [(a * n[..., i] * n[..., j]).astype(F) for i, j in pairs]
    image = (100.0 - 60.0 * a).astype(F)
    return image, tensors


_BUILT = {}


def get(name):
    """The case, built once (its arrays are read-only)."""
    if name not in _BUILT:
        _BUILT[name] = CASES[name]()
    return _BUILT[name]


def call_args(c):
    """The keyword arguments of api.surface_points_host / Context.surface_points for a case."""
    return dict(voxel2cluster=c["cluster"], mask=c["mask"], select_cluster=c["select_cluster"], voxel_width=c["voxel_width"],
                curve_ds=c["curve_ds"], find_ridge=c["find_ridge"], max_distance_to_feature=c["max_distance_to_feature"])
