"""The contract of the graph entries of LabelConnected (include/visfd_hip.h: visfd_hip_label_connected_graph[_dev|_host]),
derived from the restatement in connect_graph_np.py and the flood (api.label_connected), and the calls the CPU and the GPU
tests both make.  Not a test file.

  labels, count, seed positions, sizes, seed saliencies     the flood's bits
  direction of a labelled voxel                               the flood's bits (= the restatement's where it has no reason)
  direction of every other voxel (unlabelled or masked)       the INPUT's bits
  reasons                                                     the restatement's, HALO masked off; none: the graph path
  valid voxels, candidates of the host's vector test          the restatement's counts with and without the directions

Restated and flooded results are kept per call name, so that the CPU tests and the GPU tests of one session compute each
reference once."""
import numpy as np

import connect_graph_np as cg
import test_connect as tc
import test_connect_graph as tg
import volgen
from visfd_amd import api

SHAPES = [(3, 3, 3), (70, 5, 3), (20, 20, 70), (70, 20, 9), (9, 70, 20)]      # (nz, ny, nx)
_memo = {}


def mask_for(shape):
    """block_mask cuts boxes of 4 x 5 x 6 voxels; thinner images get a sprinkle"""
    if min(shape) > 6:
        return volgen.block_mask(shape, seed=9)
    return (np.random.default_rng(9).random(shape) > 0.2).astype(np.float32)


def split(sal, ten, direction, case):
    """a call of the test files' kind -> (keyword arguments, mask, direction as passed in or None, tensor or None)"""
    kw = {k: v for k, v in case.items() if not k.startswith("_")}
    use = kw.pop("use", "")
    mask = mask_for(sal.shape) if kw.pop("mask", False) else None
    return kw, mask, (direction if "v" in use else None), (ten if "t" in use else None)


def reference(name, sal, ten, direction, case):
    """-> (flood result (labels, n, seeds, sizes, saliencies, directions after), reasons the contract expects, valid voxels,
    candidates of the vector test: the voxels that pass mask, threshold and tensor test, which is what the restatement
    calls valid when it is given no directions; 0 for a call without directions)"""
    if name not in _memo:
        kw, mask, d_in, t = split(sal, ten, direction, case)
        d = None if d_in is None else d_in.copy()
        flood = api.label_connected(sal, mask=mask, direction=d, tensor=t, **kw) + (d,)
        g = cg.label_connected_graph(sal, mask=mask, direction=None if d_in is None else d_in.copy(), tensor=t, **kw)
        candidates = 0 if d_in is None else cg.label_connected_graph(sal, mask=mask, direction=None, tensor=t, **kw)["n_valid"]
        _memo[name] = (flood, g["reasons"] & ~cg.HALO, g["n_valid"], candidates)
    return _memo[name]


def check(name, got, sal, ten, direction, case):
    """got = (labels, n, seeds, sizes, saliencies, directions after the call) of a graph entry on the call's inputs"""
    flood = reference(name, sal, ten, direction, case)[0]
    kw, mask, d_in, _ = split(sal, ten, direction, case)
    assert got[1] == flood[1], (name, "n_clusters", got[1], flood[1])
    assert np.array_equal(got[0], flood[0]), (name, "labels differ at", int((got[0] != flood[0]).sum()), "voxels")
    for x, y, what in zip(got[2:5], flood[2:5], ("seed positions", "sizes", "seed saliencies")):
        assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)), (name, what)
    if d_in is None:
        assert got[5] is None
        return
    labelled = flood[0] != kw.get("label_undefined", -1)
    if mask is not None:
        labelled &= mask != 0
    want = np.where(labelled[..., None], flood[5].view(np.uint32), d_in.view(np.uint32))
    ne = (got[5].view(np.uint32) != want).any(-1)
    assert not ne.any(), (name, "directions: %d labelled and %d other voxels differ" % (int((ne & labelled).sum()),
                                                                                       int((ne & ~labelled).sum())))


def tv_jobs(post, ten, direction):
    """every call of test_connect.py and every variant of test_connect_graph.py on the tensor-voting outputs, and its two
    small volumes: (name, sal, ten, direction, case); the last 34 are the calls of test_connect_graph.py"""
    jobs = [("tc case %d" % i, post, ten, direction, c) for i, c in enumerate(tc.cases(post))]
    jobs += [("tc must-link %d" % i, post, ten, direction, c) for i, c in enumerate(tc.must_link_cases(post))]
    for name, case in tg._variants(post):
        jobs.append((("tg " + name,) + tg._inputs(post, ten, direction, case) + (case,)))
    for name, shape, seed, kw in (("tg 3x3x3", (3, 3, 3), 1, dict(connectivity=3, consider_dot_product_sign=True)),
                                  ("tg 3x5x70", (70, 5, 3), 2, dict(connectivity=2, consider_dot_product_sign=False))):
        sal, t, d, case = tg._small(shape, seed, **kw)
        jobs.append((name, sal, t, d, case))
    return jobs


N_TG = 34


# ---- the small shapes: fixed generator seeds -------------------------------------------------------------------------------
SHAPE_SEED = 41


def field(shape, seed=SHAPE_SEED, about_centre=False):
    """Random saliency and tensors as tg._small has them.  The directions are the unit vectors away from a point beyond the
    image's first corner plus a fifth of noise, each with the arbitrary sign of an eigenvector: neighbours then agree up to
    that sign, so a component can be oriented (random directions cannot: every cycle is a coin toss, and around the centre
    of a radial field opposite neighbours face each other), and a cluster's outward sum is far from zero.
    about_centre: the point is the image's centre, and the larger shapes get components that cannot be oriented."""
    rng = np.random.default_rng(seed)
    sal = rng.random(shape).astype(np.float32)
    ten = rng.normal(0, 1, shape + (6,)).astype(np.float32)
    ten[..., :3] = np.abs(ten[..., :3]) + 1
    z, y, x = np.meshgrid(*(np.arange(n) + (0.3 - (n - 1) / 2.0 if about_centre else 0.6 * n + 3.3) for n in shape), indexing="ij")
    d = np.stack([x, y, z], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    d += 0.2 * rng.normal(0, 1, d.shape)
    d *= np.where(rng.random(shape) < 0.5, -1.0, 1.0)[..., None]
    return sal, ten, np.ascontiguousarray(d.astype(np.float32))


def shape_jobs(shape, conn):
    """signs on and off; the saliency as it is and in five levels (plateaus, seeds and components across every tile and
    workgroup edge); mask on for connectivity 2; minima for connectivity 3; one call on the saliency alone; for
    connectivity 3 one call more, on directions about the image's centre (the fall-back's share)"""
    sal, ten, d = field(shape)
    flat = (np.floor(sal * 5) / 5).astype(np.float32)
    tag = "%dx%dx%d conn%d" % (shape[2], shape[1], shape[0], conn)
    jobs = []
    for signs in (True, False):
        case = dict(threshold_saliency=0.4, use="vt", threshold_vector_saliency=0.2, threshold_vector_neighbor=0.3,
                    threshold_tensor_saliency=-0.5, threshold_tensor_neighbor=0.2, connectivity=conn,
                    consider_dot_product_sign=signs, standardize_directions=not signs)
        jobs.append(("%s signs%d" % (tag, signs), sal, ten, d, case))
        jobs.append(("%s signs%d levels" % (tag, signs), flat, ten, d,
                     dict(case, mask=conn == 2, start_from_saliency_maxima=conn != 3,
                          threshold_saliency=0.4 if conn != 3 else 0.6)))
    jobs.append(("%s saliency only" % tag, flat, None, None, dict(threshold_saliency=0.8, connectivity=conn, sort_by_size=False)))
    if conn == 3:
        jobs.append(("%s about the centre" % tag, sal, ten, field(shape, about_centre=True)[2],
                     dict(jobs[2][4], threshold_saliency=0.5)))
    return jobs


def run_host_walk(sal, ten, direction, case):
    kw, mask, d_in, t = split(sal, ten, direction, case)
    d = None if d_in is None else d_in.copy()
    return api.label_connected_graph(sal, mask=mask, direction=d, tensor=t, **kw) + (d,)
