"""numpy restatement of the exact distance maps (visfd_amd/csrc/distance.hip; the reference's HandleDistanceToPoints and
HandleDistancePointsToFeature, bin/filter_mrc/handlers_unsupported.cpp:1393-1550):

    cap    = (nx + ny + nz)^2
    dsq(v) = min(cap, min over seeds s of |v - s|^2)            integers
    out    = sqrtf((float)dsq * (w * w))                         every step rounded to float

in two forms: the brute-force formula, chunked, and a separable min-plus form.  Arrays are (nz, ny, nx); points are
(n, 3) integer rows x, y, z and may lie anywhere."""
import numpy as np

MAX_DIM_SUM = 46340


def cap_of(shape):
    nz, ny, nx = shape
    return (nx + ny + nz) ** 2


def selection(src, mask, lo, hi):
    """the voxels -distance-to-voxels measures to: mask != 0 and lo <= src <= hi in float (a NaN is never selected)"""
    with np.errstate(invalid="ignore"):
        sel = (src >= np.float32(lo)) & (src <= np.float32(hi))
    if mask is not None:
        sel &= ~(mask == 0)
    return sel


def seeds_of(shape, points=None, src=None, mask=None, lo=-np.inf, hi=np.inf):
    """every seed as (n, 3) int64 rows x, y, z: the selected voxels, then the listed points"""
    rows = [np.zeros((0, 3), np.int64)]
    if src is not None:
        z, y, x = np.nonzero(selection(src, mask, lo, hi))
        rows.append(np.stack([x, y, z], 1).astype(np.int64))
    if points is not None and len(points):
        rows.append(np.asarray(points, np.int64).reshape(-1, 3))
    return np.concatenate(rows)


def point_dsq(shape, queries, seeds, chunk=1 << 22):
    """min(cap, squared distance from each query (n, 3) to the nearest seed (m, 3)), int64, by brute force in chunks"""
    cap = cap_of(shape)
    q = np.asarray(queries, np.int64).reshape(-1, 3)
    s = np.asarray(seeds, np.int64).reshape(-1, 3)
    best = np.full(len(q), cap, np.int64)
    if len(s) == 0 or len(q) == 0:
        return best
    # python integers beyond int64 cannot arise: clip the seeds to where they still cannot beat cap
    far = 2 * MAX_DIM_SUM
    s = np.clip(s, -far, far + max(shape))
    step = max(1, chunk // len(q))
    for k in range(0, len(s), step):
        d = q[:, None, :] - s[None, k:k + step, :]
        best = np.minimum(best, (d * d).sum(2).min(1))
    return best


def distance_sq_brute(shape, points=None, src=None, mask=None, lo=-np.inf, hi=np.inf):
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    vox = np.stack([x.ravel(), y.ravel(), z.ravel()], 1)
    return point_dsq(shape, vox, seeds_of(shape, points, src, mask, lo, hi)).reshape(shape).astype(np.int32)


def _minplus(g, axis, big):
    """D(i) = min_j g(j) + (i - j)^2 along `axis`; entries equal to `big` mean "nothing" and stay out of every sum"""
    g = np.moveaxis(g, axis, 0)
    n = g.shape[0]
    out = np.full_like(g, big)
    i = np.arange(n).reshape((n,) + (1,) * (g.ndim - 1))
    for j in range(n):
        cand = np.where(g[j] == big, big, g[j] + (i - j) ** 2)
        out = np.minimum(out, cand)
    return np.moveaxis(out, 0, axis)


def distance_sq_separable(shape, points=None, src=None, mask=None, lo=-np.inf, hi=np.inf):
    """the same map: seeds inside the image through three min-plus passes, the others by the formula"""
    nz, ny, nx = shape
    cap = cap_of(shape)
    s = seeds_of(shape, points, src, mask, lo, hi)
    ins = (s[:, 0] >= 0) & (s[:, 0] < nx) & (s[:, 1] >= 0) & (s[:, 1] < ny) & (s[:, 2] >= 0) & (s[:, 2] < nz)
    g = np.full(shape, cap, np.int64)
    g[s[ins, 2], s[ins, 1], s[ins, 0]] = 0
    for axis in (2, 1, 0):
        g = _minplus(g, axis, cap)
    if (~ins).any():
        z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        vox = np.stack([x.ravel(), y.ravel(), z.ravel()], 1)
        g = np.minimum(g, point_dsq(shape, vox, s[~ins]).reshape(shape))
    return g.astype(np.int32)


def root(dsq, voxel_width):
    """sqrtf((float)dsq * (w * w)) with every step rounded to float"""
    w = np.float32(voxel_width)
    return np.sqrt(np.asarray(dsq).astype(np.float32) * np.float32(w * w)).astype(np.float32)


def distance_to_points(dst, points, voxel_width, mask=None):
    """-distance-points: dst with the distance written where mask != 0"""
    d = root(distance_sq_brute(dst.shape, points), voxel_width)
    if mask is None:
        return d
    return np.where(mask == 0, dst, d).astype(np.float32)


def distance_from_points(src, points, lo, hi, voxel_width, mask=None):
    """-distance-to-voxels: one float per point"""
    s = seeds_of(src.shape, None, src, mask, lo, hi)
    return root(point_dsq(src.shape, points, s), voxel_width)


def integer_points(crds, voxel_width, in_voxels):
    """The handlers' conversion of a coordinate file's float rows to integer points, literally: the float coordinate
    minus 1 (voxel files) or divided by the float voxel width of its axis, plus 0.5 in double, floor, int."""
    c = np.asarray(crds, np.float32).reshape(-1, 3)
    if in_voxels:
        c = c - np.float32(1.0)
    else:
        c = c / np.asarray(voxel_width, np.float32).reshape(-1)[None, :]
    return np.floor(c.astype(np.float64) + 0.5).astype(np.int64)


def format_distances(values):
    """`ostream << float << endl` per value: %g with 6 digits"""
    return "".join("%g\n" % float(v) for v in values)


def read_points_text(text):
    """A coordinate file (bin/filter_mrc/file_io.hpp:85-214, :413-493) -> ((n, 3) float32, in_voxels): 3 to 5 numbers
    per line, '#' starts a comment, words are skipped; parentheses anywhere (IMOD's notation) mean the file is in voxels.
    The reader itself turns the coordinates of a line with parentheses into floor(x) - 1 (IMOD counts from 1); the
    handlers subtract 1 once more from every line of such a file (integer_points) -- both are the reference's."""
    rows, in_voxels = [], False
    for line in text.splitlines():
        line = line.split("#")[0]
        parens = "(" in line or ")" in line
        in_voxels = in_voxels or parens
        nums = []
        for tok in line.replace("(", " ").replace(")", " ").replace(",", " ").split():
            try:
                nums.append(float(tok))
            except ValueError:
                pass
        if nums:
            assert 3 <= len(nums) <= 5, line
            rows.append([np.floor(np.float32(x)) - np.float32(1.0) for x in nums[:3]] if parens else nums[:3])
    return np.asarray(rows, np.float32).reshape(-1, 3), in_voxels


def bin_volume(v, b):
    """BinArray3D: averages of b x b x b blocks, trailing voxels dropped (exact for the small integers of the cases)"""
    nz, ny, nx = (s // b for s in v.shape)
    v = v[:nz * b, :ny * b, :nx * b].reshape(nz, b, ny, b, nx, b).astype(np.float64)
    return (v.sum((1, 3, 5)) / b ** 3).astype(np.float32)


def split_flags(flags):
    """-> (bin, point files, (dist file, A, B) or None, the flags that are left: the tail's)"""
    b, files, voxels, rest, i = 1, [], None, [], 0
    while i < len(flags):
        if flags[i] == "-bin":
            b = int(flags[i + 1]); i += 2
        elif flags[i] == "-distance-points":
            files.append(flags[i + 1]); i += 2
        elif flags[i] == "-distance-to-voxels":
            files.append(flags[i + 1])
            voxels = (flags[i + 2], np.float32(float(flags[i + 3])), np.float32(float(flags[i + 4]))); i += 5
        else:
            rest.append(flags[i]); i += 1
    return b, files, voxels, rest


def run_case(case, vol, mask, point_files, tail):
    """What filter_mrc writes for a case of tests/distance_cases.py: (image, text of the distance file or None).
    `tail(tomo_in, filtered, mask, flags)` is the restatement of the program's tail (tests/intensity_np.py)."""
    b, files, voxels, rest = split_flags(case["flags"])
    w = np.float32(case["w"])
    mask = mask if case["mask"] else None
    if b > 1:
        vol = bin_volume(vol, b)
        mask = None if mask is None else bin_volume(mask, b)
        w = np.float32(w * np.float32(b))
    pts = [np.zeros((0, 3), np.int64)]
    for name in files:
        crds, in_voxels = read_points_text(point_files[name])
        pts.append(integer_points(crds, [w, w, w], in_voxels))
    pts = np.concatenate(pts)
    if voxels is None:
        return tail(vol, distance_to_points(vol, pts, w, mask), mask, rest), None
    return tail(vol, vol, mask, rest), format_distances(distance_from_points(vol, pts, voxels[1], voxels[2], w, mask))
