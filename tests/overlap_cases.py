"""The lists the overlap suppression is tested on (tests/test_overlap.py, tests/test_overlap_gpu.py,
tests/golden/make_golden_overlap.py): name -> (crds, diameters, scores, min_sep, max_large, max_small, criteria, scale).
No list has more than 2000 blobs, so the all-pairs statement (tests/overlap_np.py) and the golden file stay small."""
import numpy as np

F = np.float32
INF = np.inf
DO_NOT_SORT, DEC, INC, DEC_MAG, INC_MAG = range(5)


def random_blobs(seed, n, extent=120.0, ties=False):
    """the generator of tests/test_blob_post.py, restated: integer voxel centres, diameters uniform in [3, 22)"""
    rng = np.random.default_rng(seed)
    crds = np.floor(rng.uniform(0, extent, (n, 3))).astype(F)
    diam = rng.uniform(3.0, 22.0, n).astype(F)
    score = (rng.normal(0, 50, n)).astype(F)
    if ties:
        score = np.round(score / 25).astype(F) * 25
    return crds, diam, score


def chain(m=48):
    """m blobs in a row, each conflicting with its neighbours only, in decreasing order of |score|: blob i is decided in
    round i + 1, every second one is kept"""
    i = np.arange(m)
    c = np.stack([5 + 6 * i, np.full(m, 7), np.full(m, 9)], 1).astype(F)
    s = ((m - i) * np.where(i % 2 == 0, 1, -1)).astype(F)
    return c, np.full(m, 10, F), s


def _cases():
    out = {}
    # the eight lists of tests/test_blob_post.py
    for k, (seed, n, extent, ties, sep, ml, ms, crit, scale) in enumerate([
            (1, 400, 120.0, False, 1.0, INF, INF, DEC_MAG, 6), (2, 400, 120.0, True, 0.8, INF, INF, DEC_MAG, 6),
            (3, 300, 90.0, False, 0.0, 0.3, INF, INC, 6), (4, 300, 90.0, True, 0.0, INF, 0.5, DEC, 4),
            (5, 500, 60.0, False, 1.5, 0.2, 0.6, INC_MAG, 6), (6, 40, 20.0, False, 1.0, INF, INF, DEC_MAG, 6),
            (7, 5, 4.0, False, 1.0, INF, INF, DEC_MAG, 6), (8, 1, 50.0, False, 1.0, INF, INF, DEC_MAG, 6)]):
        out["post%d" % k] = random_blobs(seed, n, extent, ties) + (sep, ml, ms, crit, scale)
    out["chain48"] = chain(48) + (1.0, INF, INF, DEC_MAG, 6)
    for n in (1, 2, 63, 64, 65, 257):
        out["n%d" % n] = random_blobs(20 + n, n, 12.0 + 6.0 * n ** (1 / 3.0)) + (1.0, INF, INF, DEC_MAG, 6)
    # ties: a handful of distinct scores, all four criteria (and the list left as it is)
    for crit in (DO_NOT_SORT, DEC, INC, DEC_MAG, INC_MAG):
        out["ties_crit%d" % crit] = random_blobs(40, 200, 60.0, True) + (0.9, INF, INF, crit, 6)
    rng = np.random.default_rng(41)
    c, d, _ = random_blobs(41, 150, 50.0)
    s = rng.choice(np.array([0.0, -0.0, 1.0, -1.0], F), 150)
    for crit in (DEC, INC, DEC_MAG, INC_MAG):
        out["zeros_crit%d" % crit] = (c, d, s, 1.0, INF, INF, crit, 6)
    # negative, fractional coordinates; diameters down to 0: centre cells below 0 and past the table's end
    rng = np.random.default_rng(42)
    c = rng.uniform(-70.0, 25.0, (300, 3)).astype(F)
    d = rng.uniform(0.0, 18.0, 300).astype(F)
    d[::7] = 0.0
    d[1] = 0.0
    c[0], c[1] = -90.5, 45.9      # the extreme centres, diameter 0: bmin = -90 and C = -1; bmax = 45 and C = tsz
    out["negative"] = (c, d, rng.normal(0, 5, 300).astype(F), 1.0, INF, INF, DEC_MAG, 6)
    out["negative_volume"] = (c, np.maximum(d, F(0.5)), rng.normal(0, 5, 300).astype(F), 0.0, 0.25, 0.5, INC, 5)
    # the whole list below -1 on every axis: the reference's bmax stays at the -1 it starts from, and the table is larger
    c = np.floor(rng.uniform(-90.0, -20.0, (200, 3))).astype(F)
    out["below_zero"] = (c, rng.uniform(3.0, 22.0, 200).astype(F), rng.normal(0, 5, 200).astype(F), 1.0, INF, INF, DEC_MAG, 6)
    # a table of 1 cell and of 0 cells (nothing collides there)
    c = np.floor(rng.uniform(0, 3, (10, 3))).astype(F)
    out["tsz1"] = (c, np.full(10, 4, F), rng.normal(0, 5, 10).astype(F), 1.0, INF, INF, DEC_MAG, 6)
    out["tsz0"] = (c, np.full(10, 1, F), rng.normal(0, 5, 10).astype(F), 1.0, INF, INF, DEC_MAG, 6)
    out["scale1"] = random_blobs(43, 100, 30.0) + (1.0, INF, INF, DEC_MAG, 1)
    out["scale50"] = random_blobs(44, 300, 200.0) + (1.0, INF, INF, DEC_MAG, 50)
    c, d, s = random_blobs(45, 300, 150.0)
    d = np.where(rng.random(300) < 0.9, F(2), F(60)).astype(F)
    out["mixed"] = (c, d, s, 1.0, INF, INF, DEC_MAG, 6)
    out["mixed_volume"] = (c, d, s, 0.0, 0.1, 0.9, DEC, 6)
    # one row of cells holds more blobs than a wave has lanes, and almost everything goes
    out["dense"] = random_blobs(46, 2000, 20.0) + (1.0, INF, INF, DEC_MAG, 6)
    # the cell rule decides: pairs that meet the criterion without sharing a cell
    out["cells_a"] = random_blobs(3, 300, 90.0) + (0.0, 0.3, INF, DEC_MAG, 6)
    out["cells_b"] = random_blobs(4, 300, 90.0) + (0.0, INF, 0.5, DEC_MAG, 4)
    out["cells_c"] = random_blobs(47, 400, 120.0) + (1.6, INF, INF, DEC_MAG, 2)
    return out


CASES = _cases()


def write_blob_file(path, crds, diameters, scores):
    """a blob list as filter_mrc reads it (x y z diameter score per line), every float32 exactly"""
    with open(path, "w") as f:
        for (x, y, z), d, sc in zip(crds, diameters, scores):
            f.write("%.9g %.9g %.9g %.9g %.9g\n" % (x, y, z, d, sc))


def run_discard_blobs(cli, image, workdir, case, min_blobs=None, tag="out"):
    """filter_mrc -discard-blobs on the list of a case (voxel width 1, ratio from the case; magnitude order, scale 6) ->
    (bytes of the output file, stderr).  min_blobs: the value of VISFD_HIP_DISCARD_OVERLAP_MIN_BLOBS, None leaves it unset."""
    import os
    import subprocess
    c, d, s, sep = case[:4]
    src, out = os.path.join(workdir, "blobs_in.txt"), os.path.join(workdir, tag + ".txt")
    write_blob_file(src, c, d, s)
    env = dict(os.environ)
    env.pop("VISFD_HIP_DISCARD_OVERLAP_MIN_BLOBS", None)
    if min_blobs is not None:
        env["VISFD_HIP_DISCARD_OVERLAP_MIN_BLOBS"] = str(min_blobs)
    r = subprocess.run([cli, "-in", image, "-w", "1", "-discard-blobs", src, out, "-blob-separation", "%.9g" % sep],
                       capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    return open(out, "rb").read(), r.stderr
