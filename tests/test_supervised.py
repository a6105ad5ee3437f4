"""The supervised blob thresholds without a GPU: the host walk of FindSpheres and the threshold logic (csrc/find_spheres.hip,
csrc/blob_post.cpp) against the literal numpy restatement (tests/supervised_np.py), which paints the reference's table;
the argument errors; the C++ drop-ins (tests/shim_supervised_check.cpp, also as a stand-alone program under
-fsanitize=address,undefined); and filter_mrc's -auto-thresh / -supervised / -supervised-multi runs, text for text and exit
status for exit status against what the reference program did (tests/golden/supervised.npz).  Every list here is below the
program's FIND_SPHERES_MIN_PAIRS, so the search walks the pairs on the host."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import supervised_cases as sc
import supervised_np as sn
from conftest import ROOT, golden

F = np.float32
CLI = os.path.join(ROOT, "visfd_amd", "cli", "filter_mrc")


@pytest.fixture(scope="module")
def api():
    from visfd_amd import api
    api.load_library()
    return api


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(CLI):
        from visfd_amd import build
        build.build(verbose=False)
    return CLI


# ---- FindSpheres, host walk -------------------------------------------------------------------------------------------------
def _sweep_diameters():
    ds = [F(x) for x in sc.DIAMETERS]
    for k in range(0, 161):
        x = F(k * 0.25)
        ds += [x, np.nextafter(x, F(0)), np.nextafter(x, F(1e9)), -x, np.nextafter(-x, F(0)), np.nextafter(-x, F(-1e9))]
    rng = np.random.default_rng(1)
    ds += [F(v) for v in rng.uniform(0, 92680, 5000)] + [F(92680.0)]
    ds += [F(v) for v in rng.uniform(-50, 0, 2000)] + [F(-92680.0)]
    return ds


def test_one_number_per_sphere_decides_both_tests():
    """What lets a record carry one number: with R >= 1, (R + 1)^2 > Rsqr, so a point beyond R on one axis is beyond Rsqr;
    with R = 0 -- every diameter up to 1, all negative ones -- Rsqr does NOT imply the R test (it grows with |d|), and the
    record's number is 0.  Swept over the unit diameters, every float near a step of R or Rsqr up to +-40, random ones
    over the whole valid range and negative ones."""
    gap = 0
    for d in _sweep_diameters():
        R, Rsqr = sn.sphere_R_Rsqr(d)
        if R >= 1:
            assert (R + 1) ** 2 > Rsqr, d
            assert R * R <= Rsqr + 2 * R, d   # and R is not far beyond: the sphere reaches R - 1 at least on an axis
        else:
            assert d <= 1
            gap += int(Rsqr >= 1)             # here a point one voxel off the centre passes the Rsqr test alone
    assert gap > 1000


def test_host_walk_applies_both_tests_for_every_diameter(api):
    """the library's record against the restatement's two tests: per diameter of the sweep one sphere, and the points
    around its centre and just inside and beyond R on an axis and on the diagonals"""
    ds = _sweep_diameters()
    ds = ds[:len(sc.DIAMETERS) + 966:3] + ds[-7200::40] + ds[-2001:]    # a third of the steps, a sample of the random ones, every negative one
    offs = np.array([(x, y, z) for x in range(-3, 4) for y in range(-3, 4) for z in range(-3, 4)], np.int64)
    for d in ds:
        R, _ = sn.sphere_R_Rsqr(d)
        c = np.array([[R + 50.5, R + 50.25, R + 50.75]], F)
        ring = np.array([(R, 0, 0), (R + 1, 0, 0), (0, -R, 0), (0, -R - 1, 0), (0, 0, R), (0, 0, R + 1), (R, 1, 0), (R, R, 0)], np.int64)
        q = (np.trunc(c).astype(np.int64) + np.concatenate([offs, ring])).astype(F) + F(0.5)
        q = q[(q >= 0).all(axis=1)]
        want = sn.find_spheres_pairs(q, c, [d])
        assert np.array_equal(api.find_spheres_host(q, c, np.array([d], F)), want), d
        assert want[len(offs) // 2] == 1                      # the centre voxel is always inside


def test_negative_diameter_holds_its_centre_voxel_only(api):
    """d = -3 has R = 0 and Rsqr = ceil(2.25 - 0.5) = 2; d = -10 has R = 0 and Rsqr = 25: the painted table holds one voxel"""
    q = np.array([[3, 3, 3], [4, 3, 3], [3, 4, 4], [3, 3, 8], [9, 9, 9]], F)
    for d, rsqr in ((-3.0, 2), (-10.0, 25), (-1.5, 1)):
        assert sn.sphere_R_Rsqr(d) == (0, rsqr)
        c, dd = np.array([[3.9, 3.2, 3.5]], F), np.array([d], F)
        assert list(sn.find_spheres_table(q, c, dd)) == [1, 0, 0, 0, 0]
        assert list(api.find_spheres_host(q, c, dd)) == [1, 0, 0, 0, 0]


def test_gpu_scene_restatement_agrees_with_the_painted_table():
    """the answer the GPU tests share comes from the pair walk; on the dense corner the table painting gives the same"""
    scene = sc.gpu_scene(261, 40)
    n, nq = 261, 40
    q = scene["q"][:nq].copy()
    q[0] = 25.5   # the table is sized by the queries themselves: one beyond the rest keeps (int)-0.99 = 0 inside it
    want = sn.find_spheres_pairs(q, scene["c"][:n], scene["d"][:n])
    assert np.array_equal(sn.find_spheres_table(q, scene["c"][:n], scene["d"][:n]), want)
    assert np.array_equal(want[1:], sc.scene_expected(scene, nq, n)[1:])
    assert (want > 0).sum() > 10 and (want == 0).sum() > 2


@pytest.mark.parametrize("seed", range(6))
def test_host_walk_equals_the_painted_table(api, seed):
    rng = np.random.default_rng(seed)
    for _ in range(40):
        ns, nq = int(rng.integers(0, 40)), int(rng.integers(1, 30))
        c = rng.uniform(-5, 16, (ns, 3)).astype(F)          # centres negative and beyond the queries' box included
        d = rng.choice(np.array(sc.DIAMETERS + [7.3, 11.0, -4.0, -7.5], F), ns)
        d[::5] = rng.uniform(-50, 0, len(d[::5])).astype(F)
        q = rng.uniform(-0.99, 12, (nq, 3)).astype(F)
        q[0] = [12.5, 12.25, 12.9]                          # sizes the table: every other query lies inside it
        want = sn.find_spheres_table(q, c, d)
        assert np.array_equal(sn.find_spheres_pairs(q, c, d), want)
        assert np.array_equal(api.find_spheres_host(q, c, d), want)


def test_host_walk_at_the_boundary_of_every_sphere(api):
    q, c, d = sc.boundary_scene()
    want = sn.find_spheres_pairs(q, c, d)
    assert (want > 0).sum() > 40 and (want == 0).sum() > 20
    assert np.array_equal(api.find_spheres_host(q, c, d), want)
    # one sphere at a time, against the painted table (a second query sizes the table beyond the sphere)
    for i in range(0, len(c), 2):
        near = np.abs(q - c[i]).max(axis=1) < 9
        qq = np.concatenate([q[near], [[c[i][0] + 12, 20, 20]]]).astype(F)
        assert np.array_equal(api.find_spheres_host(qq, c[i:i + 1], d[i:i + 1]), sn.find_spheres_table(qq, c[i:i + 1], d[i:i + 1]))


def test_truncation_and_priority(api):
    c = np.array([[5.9, 5.9, 5.9], [5.1, 5.1, 5.1], [-0.9, 0.9, 0.5]], F)      # all three truncate toward zero
    d = np.array([1, 1, 1], F)                                                  # R = 0, Rsqr = 0: the centre voxel alone
    q = np.array([[5.99, 5.0, 5.5], [-0.5, -0.5, 0.99], [6.0, 5, 5], [0, 1, 0]], F)
    assert list(api.find_spheres_host(q, c, d)) == [2, 3, 0, 0]                 # the LAST sphere that holds the point wins
    assert list(api.find_spheres_host(q, c[:1], d[:1])) == [1, 0, 0, 0]
    assert list(api.find_spheres_host(q, c[:0], d[:0])) == [0, 0, 0, 0]
    assert len(api.find_spheres_host(q[:0], c, d)) == 0


@pytest.mark.parametrize("name", sorted(sc.EINVAL_CASES))
def test_refused_values(api, name):
    q, c, d = sc.EINVAL_CASES[name]
    with pytest.raises(api.VisfdHipError) as e:
        api.find_spheres_host(q, c, d)
    assert e.value.code == 1


def test_accepted_edge_values_and_null_arrays(api):
    for name, (q, c, d) in sc.VALID_EDGE_CASES.items():
        assert np.array_equal(api.find_spheres_host(q, c, d), sn.find_spheres_pairs(q, c, d)), name
    L = api.load_library()
    q, c, d = (np.ascontiguousarray(a) for a in sc.VALID_EDGE_CASES["query_minus_half"])
    ids = np.full(1, 77, np.int64)
    P = lambda a: a.ctypes.data   # noqa: E731
    assert L.visfd_hip_find_spheres_host(None, 1, P(c), P(d), 2, P(ids)) == 1
    assert L.visfd_hip_find_spheres_host(P(q), 1, None, P(d), 2, P(ids)) == 1
    assert L.visfd_hip_find_spheres_host(P(q), 1, P(c), None, 2, P(ids)) == 1
    assert L.visfd_hip_find_spheres_host(P(q), 1, P(c), P(d), 2, None) == 1
    assert L.visfd_hip_find_spheres_host(P(q), 1, P(c), P(d), 1 << 31, P(ids)) == 1
    assert L.visfd_hip_find_spheres_host(P(q), -1, P(c), P(d), 2, P(ids)) == 1
    assert ids[0] == 77
    assert L.visfd_hip_find_spheres_host(None, 0, None, None, 0, None) == 0
    assert L.visfd_hip_find_spheres_host(P(q), 1, None, None, 0, P(ids)) == 0 and ids[0] == 0
    # the context faces refuse a null context before anything else
    assert L.visfd_hip_find_spheres(None, P(q), 1, P(c), P(d), 2, P(ids)) == 1
    assert L.visfd_hip_find_spheres_dev(None, P(q), 1, P(c), P(d), 2, P(ids)) == 1
    assert L.visfd_hip_find_spheres_last_path(None, None) == 1


# ---- ChooseThreshold1D and the interval -------------------------------------------------------------------------------------
@pytest.mark.parametrize("ties", [False, True])
def test_choose_threshold_1d_every_labeling(api, ties):
    """all 2^N labelings for N <= 8, both directions, scores distinct or with ties (also across the two labels)"""
    rng = np.random.default_rng(3 + ties)
    for N in range(0, 9):
        scores = rng.choice(np.array([-2.5, -1, 0, 0.5, 3], F), N) if ties else rng.permutation(np.arange(N)).astype(F) * F(1.7) - F(3)
        for labels in itertools.product([False, True], repeat=N):
            for lower in (True, False):
                got = api.choose_threshold_1d(scores, labels, lower)
                want = sn.choose_threshold_1d(scores, labels, lower)
                assert F(got) == want or (np.isnan(got) and np.isnan(want)), (scores, labels, lower, got, want)


def test_midpoint_is_rounded_as_the_reference_rounds_it(api):
    """0.5 * (a + b): the sum is rounded to float before the double product.  Within one binade that gives the float a
    double sum would give; where the float sum overflows it does not: the threshold is +inf, as in the reference"""
    s = np.array([16777216.0, 16777218.0], F)
    assert api.choose_threshold_1d(s, [False, True], True) == float(F(0.5 * float(F(s[0] + s[1]))))
    s = np.array([3.0000002, 3.0000005], F)
    assert F(api.choose_threshold_1d(s, [False, True], True)) == sn.choose_threshold_1d(s, [False, True], True)
    big = np.array([3e38, 3.2e38], F)     # the float sum overflows, as in the reference
    assert api.choose_threshold_1d(big, [False, True], True) == np.inf


@pytest.mark.parametrize("name", sc.UNIT_SCENES)
def test_supervised_functions_equal_the_restatement(api, name):
    blobs, pos, neg = sc.unit_scene(name)
    for criteria in (sn.SORT_DECREASING_MAGNITUDE, sn.SORT_DECREASING, sn.SORT_INCREASING, sn.SORT_INCREASING_MAGNITUDE):
        t = np.concatenate([pos, neg])
        got_s, got_i = api.find_blob_scores(t, *blobs, criteria=criteria)
        want_s, want_i = sn.find_blob_scores(t, *blobs, criteria=criteria, find=sn.find_spheres_pairs)
        assert np.array_equal(got_i, want_i) and np.array_equal(got_s, want_s), (name, criteria)
        want = sn.discard_blobs_by_score_supervised(*blobs, pos, neg, criteria=criteria)
        got = api.discard_blobs_by_score_supervised(*blobs, pos, neg, criteria=criteria)
        for a, b in zip(got[:3], want[:3]):
            assert np.array_equal(a, b), (name, criteria)
        assert (F(got[3]), F(got[4])) == (want[3], want[4]), (name, criteria)
        assert tuple(got[5][k] for k in ("false_positives", "negatives", "false_negatives", "positives")) == want[5:]
        lo, hi, rep = api.choose_blob_score_thresholds(*blobs, pos, neg, criteria=criteria)
        assert (lo, hi, rep) == got[3:]
    # the overlapping scene with the painted table as the search: priority as the reference decides it
    if name == "overlap_priority":
        big = np.array([[12, 12, 12]], F)
        ts, ids = sn.find_blob_scores(np.concatenate([pos, neg, big]), *blobs, find=sn.find_spheres_table)
        got_s, got_i = api.find_blob_scores(np.concatenate([pos, neg, big]), *blobs)
        assert np.array_equal(ids, got_i) and np.array_equal(ts, got_s)


def test_interval_passes_can_disagree(api):
    """negatives on both sides of the positives: lower-first and upper-first choose different intervals somewhere in this
    sweep, and "<=" keeps the lower-first one on equal mistakes"""
    rng = np.random.default_rng(9)
    differ = 0
    for _ in range(300):
        n = int(rng.integers(4, 14))
        s = rng.choice(np.arange(8, dtype=F), n)
        acc = (s >= 3) & (s <= 5)
        flip = rng.random(n) < 0.25
        acc = acc ^ flip
        if acc.all() or not acc.any():
            continue
        # through the C ABI: one blob per datum, each training point at its blob's centre; positives come first there
        so, ao = np.concatenate([s[acc], s[~acc]]), np.concatenate([acc[acc], acc[~acc]])
        lo1 = sn.choose_threshold_1d(so, ao, True)
        hi2 = sn.choose_threshold_1d(so, ao, False)
        want = sn.choose_interval(so, ao)
        c = np.stack([np.arange(n) * 10, np.zeros(n), np.zeros(n)], 1).astype(F)
        d = np.full(n, 2, F)
        lo, hi, rep = api.choose_blob_score_thresholds(c, d, s, c[acc], c[~acc], criteria=sn.SORT_DECREASING)
        assert (F(lo), F(hi)) == want[:2], (s, acc)
        assert (rep["false_positives"], rep["negatives"], rep["false_negatives"], rep["positives"]) == want[2:]
        # the kept interval is that of one pass; count the draws where the other pass's first threshold is not in it
        differ += int((lo1, hi2) != (want[0], want[1]))
    assert differ > 10


def test_multi_concatenates_the_sets_in_order(api):
    sets = [sc.unit_scene(n) for n in ("mixed_ties", "minima", "outside_dropped")]
    want = sn.choose_blob_score_thresholds_multi([s[0] for s in sets], [s[1] for s in sets], [s[2] for s in sets])
    lo, hi, rep = api.choose_blob_score_thresholds_multi([s[0] for s in sets], [s[1] for s in sets], [s[2] for s in sets])
    assert (F(lo), F(hi)) == want[:2]
    assert (rep["false_positives"], rep["negatives"], rep["false_negatives"], rep["positives"]) == want[2:]
    one = api.choose_blob_score_thresholds_multi([sets[0][0]], [sets[0][1]], [sets[0][2]])
    assert one == api.choose_blob_score_thresholds(*sets[0][0], sets[0][1], sets[0][2])


def test_empty_training_sets_carry_the_reference_messages(api):
    g = golden("supervised")
    blobs, pos, neg = sc.unit_scene("minima")
    far = np.array([[900, 900, 900]], F)
    for p, n, case in ((pos, far, "only_positives_inside"), (far, neg, "only_negatives_inside"), (pos, neg[:0], "only_positives_inside")):
        with pytest.raises(api.VisfdHipError) as e:
            api.choose_blob_score_thresholds(*blobs, p, n)
        assert e.value.code == 1
        text = str(e.value).split(": ", 1)[1]
        assert text.startswith("Error: Empty list of ")
        assert text.rstrip("\n") in str(g[case + "/block"]), case    # the reference's own words, as its program printed them


# ---- ABI, header, shim ------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["visfd_hip_find_spheres_host", "visfd_hip_find_spheres", "visfd_hip_find_spheres_dev",
               "visfd_hip_find_spheres_last_path", "visfd_hip_choose_threshold_1d", "visfd_hip_find_blob_scores",
               "visfd_hip_choose_blob_score_thresholds", "visfd_hip_choose_blob_score_thresholds_multi",
               "visfd_hip_discard_blobs_by_score_supervised"]


def test_abi_header_and_binding_agree(api):
    text = open(os.path.join(ROOT, "include", "visfd_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = ctypes.CDLL(api.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(L, name) and name in api.exported_symbols(), name
    for macro, value in (("VISFD_HIP_FIND_SPHERES_PATH_DEVICE", api.FIND_SPHERES_PATH_DEVICE),
                         ("VISFD_HIP_FIND_SPHERES_PATH_HOST", api.FIND_SPHERES_PATH_HOST),
                         ("VISFD_HIP_FIND_SPHERES_MAX_R", api.FIND_SPHERES_MAX_R)):
        assert int(re.search(r"#define %s (\d+)" % macro, code).group(1)) == value
    hpp = open(os.path.join(ROOT, "include", "visfd_hip.hpp")).read()
    for fn in ("FindSpheres", "ChooseThreshold1D", "FindBlobScores", "ChooseBlobScoreThresholds", "ChooseBlobScoreThresholdsMulti",
               "DiscardBlobsByScoreSupervised"):
        assert re.search(r"inline \w+ %s\(" % fn, hpp), fn
    # the option is in the table: a context would take VISFD_HIP_FIND_SPHERES_HOST from the environment
    assert "VH_OPT(find_spheres_host)" in open(
        os.path.join(ROOT, "visfd_amd", "csrc", "context.hip")).read()


def _scene_file(path, blobs, pos, neg):
    c, d, s = blobs
    with open(path, "w") as f:
        f.write("%d %d %d\n" % (len(d), len(pos), len(neg)))
        for i in range(len(d)):
            f.write("%.9g %.9g %.9g %.9g %.9g\n" % (c[i][0], c[i][1], c[i][2], d[i], s[i]))
        for p in list(pos) + list(neg):
            f.write("%.9g %.9g %.9g\n" % tuple(p))


def _expected_shim_output(blobs, pos, neg):
    def fmt(x):
        return "%.9g" % x
    c, d, s = blobs
    lines = ["find_spheres: " + " ".join(str(i) for i in sn.find_spheres_pairs(pos, c, d))]
    t = np.concatenate([pos, neg])
    ts, ids = sn.find_blob_scores(t, c, d, s)
    keep = ids > 0
    lines.append("blob_scores: " + " ".join(fmt(x) + ("+" if i < len(pos) else "-") for i, x in enumerate(ts) if keep[i]))
    acc = [i < len(pos) for i in range(len(t)) if keep[i]]
    lines.append("threshold_1d: %s %s" % (fmt(sn.choose_threshold_1d(ts[keep], acc, True)), fmt(sn.choose_threshold_1d(ts[keep], acc, False))))
    r = sn.choose_blob_score_thresholds(c, d, s, pos, neg)
    lines.append("thresholds: %s %s" % (fmt(r[0]), fmt(r[1])))
    h = len(d) // 2
    m = sn.choose_blob_score_thresholds_multi([(c, d, s), (c[:h], d[:h], s[:h])], [pos, pos], [neg, neg])
    lines.append("thresholds_multi: %s %s" % (fmt(m[0]), fmt(m[1])))
    k = sn.discard_blobs_by_score_supervised(c, d, s, pos, neg)
    lines.append("kept: " + " ".join(",".join(fmt(v) for v in (k[0][i][0], k[0][i][1], k[0][i][2], k[1][i], k[2][i])) for i in range(len(k[1]))))
    sort = "-- Sorting blobs according to their scores... done --\n"
    table = (" -- Attempting to allocate space for one more image.       --\n"
             " -- (If this crashes your computer, find a computer with   --\n"
             " --  more RAM and use \"ulimit\", OR use a smaller image.)   --\n")

    def report(x):
        return ("  examining training data to determine optimal thresholds\n"
                "  threshold lower bound: %s\n  threshold upper bound: %s\n"
                "  number of false positives: %d (out of %d negatives)\n"
                "  number of false negatives: %d (out of %d positives)\n\n" % (("%g" % x[0]), ("%g" % x[1]), x[2], x[3], x[4], x[5]))
    progress = (table + sort + table + sort + table + report(r) + sort + table + sort + table + report(m) + sort + table + report(r) +
                "  allocating another blob list copy.\n")
    return "\n".join(lines) + "\nprogress:\n" + progress


@pytest.mark.parametrize("sanitize", [False, True])
def test_cpp_drop_ins(api, tmp_path, sanitize):
    """tests/shim_supervised_check.cpp with its own main, under -Wall -Werror; once more with the address and
    undefined-behaviour sanitizers, as a stand-alone program (the sanitizer's runtime is linked into the program)"""
    exe = str(tmp_path / "shim_supervised_check")
    libdir = os.path.dirname(api.LIB_PATH)
    cmd = ["g++", "-std=c++11", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "shim_supervised_check.cpp"), "-L" + libdir, "-lvisfd_hip", "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ)
    if sanitize:
        env["ASAN_OPTIONS"] = "detect_leaks=0"   # the HIP runtime the library links keeps its allocations until exit
    for name in ("mixed_ties", "overlap_priority", "outside_dropped"):
        blobs, pos, neg = sc.unit_scene(name)
        scene = str(tmp_path / (name + ".txt"))
        _scene_file(scene, blobs, pos, neg)
        r = subprocess.run([exe, scene], capture_output=True, text=True, env=env)
        assert r.returncode == 0, (name, r.returncode, r.stdout[-500:], r.stderr[-3000:])
        assert r.stdout == _expected_shim_output(blobs, pos, neg), name


# ---- filter_mrc -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.CPU_CLI_CASES)
def test_cli_equals_the_reference_program(cli, name, tmp_path):
    g = golden("supervised")
    sc.assert_case_matches(g, name, sc.run_case(cli, g, name, str(tmp_path)))


def test_golden_holds_every_case_and_the_cases_it_was_made_from():
    g = golden("supervised")
    for name, case in sc.CASES.items():
        assert name + "/returncode" in g.files, name
        for fname, (kind, data) in case["files"].items():
            stored = g["%s/file/%s" % (name, fname)]
            assert (str(stored) == data) if kind == "text" else np.array_equal(stored, np.asarray(data, F)), (name, fname)
    errors = [n for n in sc.CASES if int(g[n + "/returncode"]) != 0]
    assert sorted(errors) == ["only_negatives_inside", "only_positives_inside"]
    shrunk = [n for n in sc.CPU_CLI_CASES if len(json_list(g, n)) == 2 and json_list(g, n)[0] != json_list(g, n)[1]]
    assert len(shrunk) >= 20


def json_list(g, name):
    import json
    return json.loads(str(g[name + "/remaining"]))


def test_cli_route_override_names_the_search(cli, tmp_path):
    """VISFD_HIP_FIND_SPHERES_MIN_PAIRS: a huge value keeps the host walk and the program says so; the results are the golden's"""
    g = golden("supervised")
    env = dict(os.environ, VISFD_HIP_FIND_SPHERES_MIN_PAIRS="1e30")
    res = sc.run_case(cli, g, "mixed_ties_60", str(tmp_path), env=env)
    assert "  (find_spheres: host search)\n" in res["stderr"]
    sc.assert_case_matches(g, "mixed_ties_60", res)


IN = ["-in", sc.IMAGE]
ARG_ERRORS = [
    ("auto_thresh_word", IN + ["-auto-thresh", "size"], "Error: The -auto-thresh argument must be followed by \"score\"\n"),
    ("auto_thresh_nothing", IN + ["-auto-thresh"], "Error: The -auto-thresh argument must be followed by \"score\"\n"),
    ("supervised_one_file", IN + ["-supervised", "a.txt"], "Error: The -supervised argument must be followed by two file names:\n"
                                                             "       FILE_POS.txt  FILE_NEG.txt\n"),
    ("supervised_multi_nothing", IN + ["-supervised-multi"], "Error: The -supervised-multi argument must be followed a file name."),
    ("radii_range_negative", IN + ["-spheres-nonmax-radii-range", "-1", "3"],
     "Error: The -spheres-nonmax-radii-range argument must be followed by a number number.\n"),
    ("score_range_one", IN + ["-sphere-nonmax-score-range", "3"],
     "Error: The -sphere-nonmax-score-range argument must be followed by two numbers.\n"),
    ("ratio_under_slab", IN + ["-blob", "minima", "b.txt", "100", "200", "1.1", "-minima-ratio", "0.5", "-slab", "0", "1", "id"],
     "Error: -slab takes absolute score thresholds only"),
]


@pytest.mark.parametrize("name,args,message", ARG_ERRORS, ids=[a[0] for a in ARG_ERRORS])
def test_cli_argument_errors(cli, name, args, message, tmp_path):
    r = subprocess.run([cli] + args, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 1 and message in r.stderr, r.stderr


def test_cli_multi_refusals(cli, tmp_path):
    """the reference's two refusals of -supervised-multi, and the one deviation: not together with -supervised"""
    g = golden("supervised")
    files = sc.golden_files(g, "multi_2")
    base = sc.CASES["multi_2"]["args"]
    r = sc.run_program(cli, files, base + ["-discard-blobs", "blobs0.txt", "out.txt"], None, str(tmp_path))
    assert r["returncode"] == 1 and "Error: This program is too stupid to automatically discard blobs from multiple\n" in r["stderr"]
    r = sc.run_program(cli, files, base + ["-mask", "MASK"], None, str(tmp_path))
    assert r["returncode"] == 1 and "Error: You may not use the \"-supervised-multi\" argument simultaneously with\n" in r["stderr"]
    r = sc.run_program(cli, files, base + ["-supervised", "pos0.txt", "neg0.txt"], None, str(tmp_path))
    assert r["returncode"] == 1 and "Error: -supervised-multi does not combine with -supervised" in r["stderr"]
    bad = dict(files, **{"meta.txt": ("text", "pos0.txt neg0.txt\n")})
    r = sc.run_program(cli, bad, base, None, str(tmp_path))
    assert r["returncode"] == 1 and "Expected 3 file names in every line in this file:" in r["stderr"] and "line: 1" in r["stderr"]
