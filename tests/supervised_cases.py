"""The cases of the supervised blob thresholds, shared by tests/golden/make_golden_supervised.py (which records what the
reference program does with them), tests/test_supervised.py and tests/test_supervised_gpu.py.

A command-line case is a set of small text files plus the arguments of filter_mrc; everything is run inside a scratch
directory with relative file names, so that neither stderr nor the files mention a path.  The golden stores, per case, the
numbers of every input file, the exit status, the kept list as text and the block of stderr that belongs to the
supervised step."""
import json
import os
import subprocess

import numpy as np

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
IMAGE = os.path.join(GOLDEN, "test_blob_detect.rec")        # 22 x 32 x 27 voxels
MASK = os.path.join(GOLDEN, "test_blob_detect_mask.rec")
BOX = (22, 32, 27)

# the diameters of the unit sweeps: below and at the sizes where R or Rsqr step, float neighbours of such sizes, and
# negative ones, whose R is 0 (the centre voxel alone) while their Rsqr = ceil((d/2)^2 - 0.5) grows with |d|
DIAMETERS = [-1.0, 0.0, 0.4, 0.5, 1.0, 2.0, 2.0000002, 3.0, 4.9999995, 5.0, -1.5, -2.0, -3.0, -10.0]


def gpu_scene(n=50000, nq=300):
    """The scene of tests/test_supervised_gpu.py: n spheres and nq queries in a 60^3 box (the first 261 spheres and 40
    queries in a dense corner, the last 30 queries beyond every sphere), and inside[k, i]: sphere i holds query k, by the
    restatement's pair test with both the R and the Rsqr test, chunked."""
    import supervised_np as sn
    rng = np.random.default_rng(11)
    c = rng.uniform(-6, 66, (n, 3)).astype(F)
    d = rng.choice(np.array(DIAMETERS + [6.5, 9, 13.2, -6.5], F), n)
    c[:261] = rng.uniform(0, 24, (261, 3)).astype(F)
    q = rng.uniform(-0.99, 60, (nq, 3)).astype(F)
    q[:40] = rng.uniform(-0.99, 24, (40, 3)).astype(F)
    if nq > 270:
        q[270:] = rng.uniform(74, 90, (nq - 270, 3)).astype(F)
    qi, ci = sn._trunc(q), sn._trunc(c)
    lut = {float(x): sn.sphere_R_Rsqr(x) for x in np.unique(d)}
    R = np.array([lut[float(x)][0] for x in d], np.int64)
    Rsqr = np.array([lut[float(x)][1] for x in d], np.int64)
    inside = np.zeros((nq, n), bool)
    for s0 in range(0, n, 5000):
        dd = np.abs(qi[:, None, :] - ci[None, s0:s0 + 5000, :])
        inside[:, s0:s0 + 5000] = (dd <= R[None, s0:s0 + 5000, None]).all(2) & ((dd * dd).sum(2) <= Rsqr[None, s0:s0 + 5000])
    for a in (c, d, q, inside):
        a.setflags(write=False)
    return dict(c=c, d=d, q=q, inside=inside)


def scene_expected(scene, n_crds, n_spheres):
    ins = scene["inside"][:n_crds, :n_spheres]
    return np.where(ins, np.arange(1, n_spheres + 1)[None, :], 0).max(axis=1, initial=0).astype(np.int64).reshape(n_crds)


# ---- unit scenes ----------------------------------------------------------------------------------------------------------
def squares3(n):
    """non-negative (a, b, c) with a^2 + b^2 + c^2 == n, or None"""
    m = int(n ** 0.5) + 1
    for a in range(m + 1):
        for b in range(a, m + 1):
            c2 = n - a * a - b * b
            if c2 < b * b:
                break
            c = int(round(c2 ** 0.5))
            if c * c == c2:
                return a, b, c
    return None


def boundary_scene():
    """One sphere per diameter of the sweep (twice: a centre inside the box and a negative one), and queries at squared
    distances Rsqr and Rsqr + 1 from each centre wherever three squares give that number."""
    import supervised_np as sn
    c, d, q = [], [], []
    for k, dia in enumerate(DIAMETERS + [7.0, 8.6, 12.0, -7.0]):
        for centre in ((16 * k + 6.3, 6.9, 7.2), (16 * k + 6.3, -2.5, 40.1)):
            c.append(centre)
            d.append(dia)
            ci = [int(x) for x in centre]      # truncation toward zero
            _, Rsqr = sn.sphere_R_Rsqr(dia)
            for target in (Rsqr, Rsqr + 1, max(Rsqr - 1, 0)):
                abc = squares3(target)
                if abc is None:
                    continue
                for perm in ((0, 1, 2), (2, 0, 1)):
                    for sign in (1, -1):
                        p = [ci[0] + sign * abc[perm[0]], ci[1] + abc[perm[1]], ci[2] - sign * abc[perm[2]]]
                        if min(p) >= 0:
                            q.append([p[0] + 0.5, p[1] + 0.25, p[2] + 0.9])
    return np.array(q, F), np.array(c, F), np.array(d, F)


_ok_q, _ok_c, _ok_d = np.array([[3, 3, 3]], F), np.array([[3, 3, 3], [4, 4, 4]], F), np.array([2, 3], F)


def _with(which, row, col, value):
    q, c, d = _ok_q.copy(), _ok_c.copy(), _ok_d.copy()
    a = {"q": q, "c": c, "d": d}[which]
    if a.ndim == 2:
        a[row, col] = value
    else:
        a[row] = value
    return q, c, d


EINVAL_CASES = {
    "negative_query": _with("q", 0, 1, -1.0),
    "nan_query": _with("q", 0, 2, np.nan),
    "inf_query": _with("q", 0, 0, np.inf),
    "nan_centre": _with("c", 1, 0, np.nan),
    "inf_centre": _with("c", 0, 2, -np.inf),
    "nan_diameter": _with("d", 0, 0, np.nan),
    "inf_diameter": _with("d", 1, 0, np.inf),
    "radius_46341": _with("d", 1, 0, 92682.0),     # R = ceil(46341 - 0.5) = 46341 > 46340
}
VALID_EDGE_CASES = {
    "query_minus_half": _with("q", 0, 0, -0.5),    # truncates to 0
    "radius_46340": _with("d", 1, 0, 92680.0),     # R = ceil(46340 - 0.5) = 46340
}


def random_blobs(seed, n, box=BOX, signs="mixed", ties=False, dmin=2.0, dmax=7.0):
    """centres on voxels inside the box, diameters in voxels, scores: -> (crds, diameters, scores) float32"""
    rng = np.random.default_rng(seed)
    c = np.stack([rng.integers(0, box[k], n) for k in range(3)], 1).astype(F)
    d = rng.uniform(dmin, dmax, n).astype(F)
    s = rng.uniform(10, 100, n)
    if ties:
        s = np.round(s / 10) * 10
    if signs == "minima":
        s = -s
    elif signs == "mixed":
        s = s * rng.choice([-1, 1], n)
    return c, d, s.astype(F)


def training_points(seed, blobs, n_pos, n_neg, cut, noise=0.0, outside=0, jitter=0.45, by="abs"):
    """points inside blobs: positives in blobs with key >= cut, negatives in the others (a fraction `noise` of the labels
    is swapped), plus `outside` points per set far from every blob"""
    rng = np.random.default_rng(seed)
    c, d, s = blobs
    key = np.abs(s) if by == "abs" else s
    good, bad = np.flatnonzero(key >= cut), np.flatnonzero(key < cut)

    def pick(idx, n):
        if len(idx) == 0 or n == 0:
            return np.zeros((0, 3), F)
        i = rng.choice(idx, n)
        return (c[i] + rng.uniform(0, jitter, (n, 3))).astype(F)
    pos, neg = pick(good, n_pos), pick(bad, n_neg)
    k = int(noise * min(len(pos), len(neg)))
    if k:
        pos[:k], neg[:k] = neg[:k].copy(), pos[:k].copy()
    far = np.array([[500, 600, 700]], F) + rng.uniform(0, 50, (outside, 3)).astype(F)
    return np.concatenate([pos, far[: outside // 2 + outside % 2]]), np.concatenate([neg, far[outside // 2 + outside % 2:]])


def unit_scene(name):
    """-> ((crds, diameters, scores), positives, negatives) for the library-level tests"""
    if name == "mixed_ties":
        b = random_blobs(3, 60, signs="mixed", ties=True)
        p, n = training_points(4, b, 12, 12, 55, noise=0.2)
    elif name == "overlap_priority":
        b = random_blobs(5, 120, box=(10, 10, 10), signs="mixed", ties=True, dmin=3, dmax=9)
        p, n = training_points(6, b, 15, 15, 50, noise=0.1)
    elif name == "outside_dropped":
        b = random_blobs(7, 40, signs="maxima")
        p, n = training_points(8, b, 8, 8, 60, outside=7, by="raw")
    elif name == "minima":
        b = random_blobs(9, 30, signs="minima")
        p, n = training_points(10, b, 9, 9, 45)
    elif name == "interval":     # negatives below AND above the positives: the two passes may disagree
        b = random_blobs(11, 80, signs="maxima", ties=True)
        c, d, s = b
        rng = np.random.default_rng(12)
        mid = np.flatnonzero((s >= 40) & (s <= 70))
        out = np.flatnonzero((s < 40) | (s > 70))
        p = (c[rng.choice(mid, 14)] + 0.2).astype(F)
        n = (c[rng.choice(out, 14)] + 0.2).astype(F)
    else:
        raise KeyError(name)
    return b, p, n


UNIT_SCENES = ["mixed_ties", "overlap_priority", "outside_dropped", "minima", "interval"]


# ---- command-line cases ---------------------------------------------------------------------------------------------------
def _blob_rows(blobs, w):
    c, d, s = blobs
    return np.concatenate([c * F(w), (d * F(w))[:, None], s[:, None]], 1).astype(F)


def _case(blobs, pos, neg, w=1.0, extra=(), imod=False, n_files=1, in_image=True):
    """a -discard-blobs ... -auto-thresh score -supervised case; coordinates and diameters are given in voxels and written
    in physical units (imod: the training files in IMOD's 1-based voxel notation instead)"""
    files = {"blobs.txt": ("blobs", _blob_rows(blobs, w))}
    if imod:
        files["pos.txt"] = ("imod", (np.floor(pos) + 1).astype(F))
        files["neg.txt"] = ("imod", (np.floor(neg) + 1).astype(F))
    else:
        files["pos.txt"] = ("points", (pos * F(w)).astype(F))
        files["neg.txt"] = ("points", (neg * F(w)).astype(F))
    args = ["-in", "IMAGE", "-w", "%g" % w, "-discard-blobs", "blobs.txt", "kept.txt", "-auto-thresh", "score", "-supervised",
            "pos.txt", "neg.txt"] + list(extra)
    return dict(files=files, args=args, out="kept.txt")


def _multi_case(sets, w=1.0):
    files, meta = {}, []
    for k, (blobs, pos, neg) in enumerate(sets):
        files["blobs%d.txt" % k] = ("blobs", _blob_rows(blobs, w))
        files["pos%d.txt" % k] = ("points", pos.astype(F))      # used as read: voxels
        files["neg%d.txt" % k] = ("points", neg.astype(F))
        meta.append("pos%d.txt neg%d.txt blobs%d.txt" % (k, k, k))
    files["meta.txt"] = ("text", "# positives  negatives  blobs\n" + "\n".join(meta) + "\n")
    return dict(files=files, args=["-in", "IMAGE", "-w", "%g" % w, "-supervised-multi", "meta.txt"], out=None)


def _build_cases():
    cases = {}

    def add(name, seed, n, signs, cut, npos=10, nneg=10, ties=False, noise=0.0, outside=0, by="abs", **kw):
        b = random_blobs(seed, n, signs=signs, ties=ties, **{k: kw.pop(k) for k in ("box", "dmin", "dmax") if k in kw})
        p, q = training_points(seed + 1000, b, npos, nneg, cut, noise=noise, outside=outside, by=by)
        cases[name] = _case(b, p, q, **kw)
        return b, p, q
    add("minima_5", 21, 5, "minima", 50, npos=4, nneg=4)
    add("maxima_12", 22, 12, "maxima", 50)
    add("mixed_ties_60", 23, 60, "mixed", 55, ties=True, noise=0.2)
    add("mixed_ties_sign_wins", 24, 40, "mixed", 45, ties=True, box=(8, 8, 8), dmin=3, dmax=8)
    add("overlap_priority", 25, 150, "mixed", 50, ties=True, npos=20, nneg=20, box=(12, 12, 12), dmin=3, dmax=9, noise=0.1)
    add("outside_dropped", 26, 40, "maxima", 60, outside=7, by="raw")
    add("noisy_labels", 27, 100, "maxima", 50, npos=25, nneg=25, noise=0.3, by="raw")
    add("n400", 28, 400, "mixed", 50, npos=30, nneg=30, ties=True, noise=0.15, box=(60, 60, 60))
    add("imod_pixel", 29, 50, "minima", 50, imod=True)
    add("w2", 30, 50, "maxima", 50, w=2.0)
    add("w19_6", 31, 30, "mixed", 50, w=19.6)
    add("bin2_voxel_files", 32, 50, "maxima", 50, imod=True, extra=["-bin", "2"])
    add("diameters_override", 33, 60, "mixed", 50, extra=["-diameters", "5.5"], w=2.0)
    add("with_separation", 34, 120, "maxima", 50, extra=["-blob-separation", "0.9"], box=(14, 14, 14), npos=15, nneg=15)
    add("with_mask", 35, 80, "minima", 50, extra=["-mask", "MASK"])
    add("with_mask_and_separation", 36, 100, "mixed", 50, extra=["-mask", "MASK", "-radial-separation", "0.8"], ties=True)
    add("radii_range", 37, 80, "maxima", 50, extra=["-spheres-nonmax-radii-range", "3", "6"])
    add("score_range", 38, 80, "maxima", 50, extra=["-sphere-nonmax-score-range", "20", "90"], by="raw")
    add("minima_threshold_first", 39, 80, "mixed", 50, extra=["-score-upper-bound", "-15"])
    # only positives / only negatives lie inside blobs: the reference's two error texts
    b = random_blobs(40, 30, signs="maxima")
    p, q = training_points(1040, b, 6, 0, 0, outside=8)
    cases["only_positives_inside"] = _case(b, p, q)
    p, q = training_points(1041, b, 0, 6, 1000, outside=8)
    cases["only_negatives_inside"] = _case(b, p, q)
    # edge points: -0.5 truncates to 0, x.9 to x
    c = np.array([[0, 0, 0], [5, 5, 5], [9, 3, 4], [14, 20, 8], [3, 25, 20], [18, 9, 15]], F)
    d = np.array([2, 3, 2.5, 4, 3, 1], F)
    s = np.array([30, 80, 55, 20, 95, 60], F)
    p = np.array([[5.9, 5.9, 5.9], [3.9, 25.9, 20.9], [18.9, 9.9, 15.9], [9.5, 3.2, 4.9]], F)
    q = np.array([[-0.5, -0.5, -0.5], [14.9, 20.9, 8.9], [15.9, 21.9, 9.9]], F)
    cases["edge_points"] = _case((c, d, s), p, q)
    # negatives below and above the positives: lower-first and upper-first give different intervals
    for k, seed in enumerate((41, 42, 43)):
        b = random_blobs(seed, 90, signs="maxima", ties=True)
        rng = np.random.default_rng(seed + 500)
        mid, out = np.flatnonzero((b[2] >= 40) & (b[2] <= 70)), np.flatnonzero((b[2] < 40) | (b[2] > 70))
        p = (b[0][rng.choice(mid, 12)] + 0.2).astype(F)
        q = (b[0][rng.choice(out, 12 + 3 * k)] + 0.2).astype(F)
        cases["interval_%d" % k] = _case(b, p, q)
    # one flag without the other does nothing
    b = random_blobs(44, 20, signs="maxima")
    p, q = training_points(1044, b, 5, 5, 50)
    full = _case(b, p, q)
    cases["auto_thresh_alone"] = dict(full, args=[a for a in full["args"] if a not in ("-supervised", "pos.txt", "neg.txt")])
    cases["supervised_alone"] = dict(full, args=[a for a in full["args"] if a not in ("-auto-thresh", "score")])
    # several images at once
    sets = []
    for seed in (45, 46, 47):
        b = random_blobs(seed, 40 + seed, signs="maxima", ties=True)
        sets.append((b,) + training_points(seed + 1000, b, 8, 8, 50, noise=0.15, outside=2, by="raw"))
    cases["multi_2"] = _multi_case(sets[:2])
    cases["multi_3"] = _multi_case(sets)
    cases["multi_w2"] = _multi_case(sets[1:], w=2.0)
    # -blob with thresholds as ratios of the extreme score
    cases["blob_maxima_ratio"] = dict(files={}, out="blobs.txt", args=["-in", "IMAGE", "-w", "19.6", "-blob", "maxima", "blobs.txt",
                                                                         "160", "280", "1.05", "-maxima-ratio", "0.4"])
    cases["blob_minima_ratio"] = dict(files={}, out="blobs.txt", args=["-in", "IMAGE", "-w", "19.6", "-blob", "minima", "blobs.txt",
                                                                         "160", "280", "1.05", "-minima-ratio", "0.5"])
    return cases


CASES = _build_cases()
# what this program needs a GPU for whatever the list sizes: binning and blob detection run on the device
NEEDS_GPU = ["bin2_voxel_files", "blob_maxima_ratio", "blob_minima_ratio"]
CPU_CLI_CASES = [n for n in CASES if n not in NEEDS_GPU]
# on the GPU: three cases through the device search, and the three above
GPU_CLI_CASES = ["mixed_ties_60", "overlap_priority", "multi_3"]


def write_files(case_files, directory):
    for fname, (kind, data) in case_files.items():
        with open(os.path.join(directory, fname), "w") as f:
            if kind == "text":
                f.write(data)
            elif kind == "imod":
                for x, y, z in data:
                    f.write("Pixel (%g, %g, %g) = 1\n" % (x, y, z))
            else:
                for row in data:
                    f.write(" ".join("%.9g" % v for v in row) + "\n")


def supervised_block(stderr):
    """the lines of the supervised step: from its first line to the last "blobs remaining" (the end of stderr when the step
    stopped the program, or printed thresholds only); the line that names the search route is not part of it"""
    lines = [ln for ln in stderr.split("\n") if not ln.startswith("  (find_spheres:")]
    start = None
    nonmax = any("discarding blobs in files" in ln for ln in lines)           # a -discard-blobs run
    multi = not nonmax and any(ln.startswith(" -- Attempting to allocate space for one more image") for ln in lines)   # -supervised-multi
    for i, ln in enumerate(lines):
        if (nonmax and "discarding blobs based on score using training data" in ln) or \
                (multi and (ln.startswith("-- Sorting blobs") or ln.startswith(" -- Attempting to allocate space for one"))):
            start = i
            break
    if start is None:
        return ""
    end = max([i for i, ln in enumerate(lines) if "blobs remaining" in ln and i > start], default=len(lines) - 1)
    return "\n".join(lines[start:end + 1]).rstrip("\n")


def run_program(exe, files, args, out, directory, env=None):
    write_files(files, directory)
    argv = [IMAGE if a == "IMAGE" else MASK if a == "MASK" else a for a in args]
    r = subprocess.run([exe] + argv, cwd=directory, capture_output=True, text=True, env=env)
    kept = None
    if out and os.path.exists(os.path.join(directory, out)):
        kept = open(os.path.join(directory, out)).read()
    return dict(returncode=r.returncode, stderr=r.stderr, block=supervised_block(r.stderr), kept=kept,
                remaining=[ln for ln in r.stderr.split("\n") if "blobs remaining" in ln])


def golden_files(g, name):
    """the input files of a case as the golden recorded them"""
    kinds = json.loads(str(g[name + "/kinds"]))
    return {fname: (kind, str(g["%s/file/%s" % (name, fname)]) if kind == "text" else g["%s/file/%s" % (name, fname)])
            for fname, kind in kinds.items()}


def run_case(exe, g, name, directory, env=None):
    case = CASES[name]
    return run_program(exe, golden_files(g, name), case["args"], case["out"], directory, env)


def assert_case_matches(g, name, res):
    assert res["returncode"] == int(g[name + "/returncode"]), (name, res["stderr"][-2000:])
    want_kept = str(g[name + "/kept"]) if bool(g[name + "/has_kept"]) else None
    assert res["kept"] == want_kept, name
    assert res["block"] == str(g[name + "/block"]), name
    assert res["remaining"] == json.loads(str(g[name + "/remaining"])), name
