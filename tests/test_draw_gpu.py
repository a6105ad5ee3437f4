"""DrawSpheres and DrawRegions on the GPU (csrc/draw.hip) against the numpy restatement tests/draw_np.py -- itself checked
against the reference program's golden images in test_draw.py -- and, through the command line, against those goldens
directly.  Every comparison is bitwise."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import draw_cases as DC
import draw_np as DN
import volgen
from conftest import GOLDEN, ROOT, assert_bits_equal

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "visfd_amd", "cli", "filter_mrc")
REF_CLI = os.path.join(ROOT, "oracle", "_ref", "filter_mrc_ref")
GOLD = os.path.join(GOLDEN, "draw.npz")
EINVAL = 1


@pytest.fixture(scope="module")
def ctx():
    from visfd_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


# ---- DrawSpheres ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(DC.SPHERE_CASES))
def test_draw_spheres_matches_restatement(ctx, name):
    kw = DC.SPHERE_CASES[name]()
    want, want_outside = DN.draw_spheres(**kw)
    got, outside = ctx.draw_spheres(want_outside=True, **kw)
    assert_bits_equal(got, want, name)
    assert outside == want_outside


def test_draw_order_decides():
    """Three mutually overlapping spheres: the list order shows in the image, so a kernel that ignored it could not pass."""
    a, _ = DN.draw_spheres(**DC.SPHERE_CASES["order_forward"]())
    b, _ = DN.draw_spheres(**DC.SPHERE_CASES["order_reversed"]())
    assert (a != b).sum() > 50


@pytest.mark.parametrize("name", ["rescale_offset", "normalize_weighted_mask", "foreground_normalize", "many_writers"])
def test_draw_spheres_device_face_in_place(ctx, torch, name):
    """The device face with dst == background, and with a separate dst: the same bits, the background left alone."""
    kw = DC.SPHERE_CASES[name]()
    want, want_outside = DN.draw_spheres(**kw)
    bg = torch.from_numpy(kw.pop("background")).cuda()
    mask = kw.pop("mask", None)
    mask = None if mask is None else torch.from_numpy(mask).cuda()
    dst = torch.full_like(bg, float("nan"))
    keep = bg.clone()
    assert ctx.draw_spheres_dev(dst, bg, mask=mask, **kw) == want_outside
    ctx.synchronize()
    assert_bits_equal(dst.cpu().numpy(), want, name + " (device face)")
    assert_bits_equal(bg.cpu().numpy(), keep.cpu().numpy(), name + " (background untouched)")
    ctx.draw_spheres_dev(bg, bg, mask=mask, **kw)
    ctx.synchronize()
    assert_bits_equal(bg.cpu().numpy(), want, name + " (in place)")


def test_draw_spheres_same_image_on_every_run(ctx):
    kw = DC.SPHERE_CASES["many_writers"]()
    first = ctx.draw_spheres(**kw)
    for _ in range(3):
        assert_bits_equal(ctx.draw_spheres(**kw), first, "repeat")


def _raw_spheres(ctx, dst, background, centers, diameters=None, n=None):
    from visfd_amd import api
    nz, ny, nx = dst.shape
    c = np.ascontiguousarray(centers, np.float32)
    d = None if diameters is None else np.ascontiguousarray(diameters, np.float32)
    return ctx._L.visfd_hip_draw_spheres(ctx._h, api._np(dst), None, api._np(background), nx, ny, nz,
                                         c.ctypes.data_as(api._fp), None if d is None else d.ctypes.data_as(api._fp), None,
                                         None, c.shape[0] if n is None else n, 0.0, 1.0, 0, 0, None)


@pytest.mark.parametrize("name", sorted(DC.REFUSED_SPHERES))
def test_draw_spheres_refuses(ctx, name):
    kw = DC.REFUSED_SPHERES[name]
    bg = DC.image((6, 7, 8), 30)
    with pytest.raises(DN.Refused):
        DN.draw_spheres(bg, **kw)
    dst = np.full_like(bg, 123.0)
    assert _raw_spheres(ctx, dst, bg, kw["centers"], kw.get("diameters")) == EINVAL
    assert (dst == 123.0).all(), "a refused call wrote to dst"


def test_draw_spheres_refuses_null_background_and_long_lists(ctx):
    bg = DC.image((6, 7, 8), 30)
    dst = np.full_like(bg, 123.0)
    c = np.zeros((1, 3), np.float32)
    assert _raw_spheres(ctx, dst, None, c) == EINVAL
    assert _raw_spheres(ctx, dst, bg, c, n=2 ** 31 - 1) == EINVAL      # the list is not read before its length is refused
    assert (dst == 123.0).all()


# ---- DrawRegions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(DC.REGION_CASES))
def test_draw_regions_matches_restatement(ctx, torch, name):
    image, regions, mask, subtract = DC.REGION_CASES[name]()
    want = DN.draw_regions(image, regions, mask, subtract)
    assert_bits_equal(ctx.draw_regions(image, regions, mask, subtract), want, name)
    d = torch.from_numpy(image.copy()).cuda()
    ctx.draw_regions_dev(d, regions, None if mask is None else torch.from_numpy(mask).cuda(), subtract)
    ctx.synchronize()
    assert_bits_equal(d.cpu().numpy(), want, name + " (device face)")


def test_draw_regions_cases_do_what_their_names_say():
    im, r, m, s = DC.REGION_CASES["fill_hidden_nonzero"]()
    assert (DN.draw_regions(im, r, m, s) == 1).sum() > 1000        # filled with ones although a masked voxel is not 0
    im, r, m, s = DC.REGION_CASES["fill_visible_nonzero"]()
    assert_bits_equal(DN.draw_regions(im, r, m, s), im)            # not filled, and nothing positive to subtract from
    im, r, m, s = DC.REGION_CASES["negative_without_subtract"]()
    positive = [x for x in r if not x[2] < 0]
    assert_bits_equal(DN.draw_regions(im, r, m, s), DN.draw_regions(im, positive, m, s))
    im, r, m, s = DC.REGION_CASES["inverted_rect"]()
    assert_bits_equal(DN.draw_regions(im, r, m, s), im)


def test_draw_regions_refuses(ctx):
    from visfd_amd import api
    im = DC.image((6, 7, 8), 31)
    for bad in ([(DN.SPHERE, (float("nan"), 1, 1, 2), 1.0)], [(DN.SPHERE, (1, 1, 1, float("inf")), 1.0)],
                [(DN.SPHERE, (1, 1, 1, 40000.0), 1.0)], [(7, (1, 1, 1, 1, 1, 1), 1.0)]):
        with pytest.raises(DN.Refused):
            DN.draw_regions(im, bad)
        with pytest.raises(api.VisfdHipError) as e:
            ctx.draw_regions(im, bad)
        assert e.value.code == EINVAL


# ---- context hygiene -----------------------------------------------------------------------------------------------------
def test_draw_trim_draw(ctx):
    kw = DC.SPHERE_CASES["foreground_normalize"]()
    want, _ = DN.draw_spheres(**kw)
    assert_bits_equal(ctx.draw_spheres(**kw), want, "before trim")
    assert ctx.workspace_bytes() > 0
    ctx.trim()
    assert ctx.workspace_bytes() == 0, "visfd_hip_trim must release the owner volume and the sphere tables"
    assert_bits_equal(ctx.draw_spheres(**kw), want, "after trim")
    ctx.debug_poison_workspace()
    assert_bits_equal(ctx.draw_spheres(**kw), want, "after poisoning the workspace")
    im, r, m, s = DC.REGION_CASES["fill_with_ones_masked"]()
    ctx.debug_poison_workspace()
    assert_bits_equal(ctx.draw_regions(im, r, m, s), DN.draw_regions(im, r, m, s), "regions after poisoning")


def test_draw_between_two_gaussians(ctx):
    src = volgen.noise_volume((12, 14, 16), seed=77)
    first, _ = ctx.gauss_ratio(src, (1.5, 1.5, 1.5), 2.5)
    kw = DC.SPHERE_CASES["rescale_offset"]()
    assert_bits_equal(ctx.draw_spheres(**kw), DN.draw_spheres(**kw)[0], "draw between Gaussians")
    im, r, m, s = DC.REGION_CASES["with_mask"]()
    assert_bits_equal(ctx.draw_regions(im, r, m, s), DN.draw_regions(im, r, m, s), "regions between Gaussians")
    again, _ = ctx.gauss_ratio(src, (1.5, 1.5, 1.5), 2.5)
    assert_bits_equal(again, first, "Gaussian after a draw")


# ---- the command line ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("name", sorted(DC.CLI_CASES))
def test_program_matches_reference_goldens(gold, name, tmp_path):
    """Our filter_mrc on the command line the reference program was recorded with: the same image, the same list files."""
    d = str(tmp_path)
    r = subprocess.run(DC.cli_command(name, CLI, d), cwd=d, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert_bits_equal(volgen.read_mrc(os.path.join(d, "out.rec")), gold[name + "/out"], name)
    for f in DC.WRITTEN.get(name, []):
        path = os.path.join(d, f)
        assert (open(path).read() if os.path.exists(path) else "") == str(gold[name + "/" + f]), f


def test_thinning_needs_its_diameter(gold, tmp_path):
    """Without -diameters the extrema list is the unthinned one (longer than the recorded thinned list)."""
    d = str(tmp_path)
    cmd = [a for a in DC.cli_command("maxima_thinned", CLI, d)]
    k = cmd.index("-diameters")
    r = subprocess.run(cmd[:k] + cmd[k + 2:], cwd=d, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    full = open(os.path.join(d, "extrema.txt")).read().splitlines()
    thinned = str(gold["maxima_thinned/extrema.txt"]).splitlines()
    assert 0 < len(thinned) < len(full)


# The three -draw-spheres command lines of the reference's own shell tests (tests/test_blob_detection.sh:35,
# tests/test_watershed.sh:14 and :83), on this repository's fixtures, next to the reference program.
SCRIPT_FORMS = {
    "blob_detection_35": (19.6, True, ["-draw-spheres", "list.txt", "-background", "0", "-foreground", "1", "-sphere-radii", "0"]),
    "watershed_14": (1.0, False, ["-draw-spheres", "list.txt", "-diameters", "3", "-foreground", "1", "-background", "0",
                                  "-spheres-shell-ratio", "1"]),
    "watershed_83": (19.6, True, ["-draw-spheres", "list.txt", "-foreground", "1", "-background", "0", "-spheres-shell-ratio", "1"]),
}


@pytest.mark.parametrize("name", sorted(SCRIPT_FORMS))
def test_program_next_to_reference_program(name, tmp_path):
    if not os.path.exists(REF_CLI):
        pytest.skip("oracle/_ref/filter_mrc_ref not built (make -C oracle ref_cli needs the reference's sources)")
    w, masked, flags = SCRIPT_FORMS[name]
    rng = np.random.default_rng(sorted(SCRIPT_FORMS).index(name) + 40)
    rows = np.concatenate([rng.random((9, 3)) * [22, 32, 27] * 1.2 - 2, rng.random((9, 1)) * 9, rng.standard_normal((9, 1))], 1)
    with open(tmp_path / "list.txt", "w") as f:
        f.write(DC.rows_text([tuple(r) for r in rows], w))
    blob = os.path.join(GOLDEN, "test_blob_detect.rec")
    common = ["-in", blob, "-w", repr(w)] + (["-mask", os.path.join(GOLDEN, "test_blob_detect_mask.rec")] if masked else [])
    images = []
    for prog, out in ((CLI, "ours.rec"), (REF_CLI, "ref.rec")):
        r = subprocess.run([prog] + common + ["-out", out] + flags, cwd=str(tmp_path), capture_output=True, text=True)
        assert r.returncode == 0, (prog, r.stderr[-2000:])
        images.append(volgen.read_mrc(str(tmp_path / out)))
    assert (images[1] != 0).any()
    assert_bits_equal(images[0], images[1], name)


# ---- the C++ drop-in -------------------------------------------------------------------------------------------------------
def _read_records(path):
    import struct
    out = {}
    with open(path, "rb") as f:
        while True:
            tag = f.read(32)
            if len(tag) < 32:
                break
            n, = struct.unpack("<q", f.read(8))
            out[tag.split(b"\0")[0].decode()] = np.frombuffer(f.read(4 * n), np.float32).copy()
    return out


def test_shim_draws_with_the_reference_signatures(tmp_path):
    import struct
    exe = str(tmp_path / "shim_draw_check")
    libdir = os.path.join(ROOT, "visfd_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "shim_draw_check.cpp"), "-o", exe, "-L" + libdir, "-lvisfd_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    shape = (10, 12, 14)
    image, mask = DC.image(shape, 90), DC.weighted_mask(shape, 91)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<iii", shape[2], shape[1], shape[0]))
        f.write(image.tobytes())
        f.write(mask.tobytes())
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "shim draw check ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    R = _read_records(tmp_path / "out.bin")
    c = np.array([[4.2, 5.0, 6.9], [9.0, 8.0, 3.0], [-0.7, 3.0, 4.0], [30.0, 3.0, 4.0], [7.5, 6.1, 7.0]], np.float32)
    d = np.array([7, 0, 5, 6, 6], np.float32)
    th = np.array([1, 1, 9, 1, 0], np.float32)
    s = np.array([1.5, -2.0, 3.0, 4.0, 5.5], np.float32)
    assert_bits_equal(R["defaults"].reshape(shape), DN.draw_spheres(image, c)[0], "default arguments")
    assert_bits_equal(R["all_arguments"].reshape(shape), DN.draw_spheres(image, c, d, th, s, mask, 0.25, 0.5, True, True)[0],
                      "every argument")
    assert_bits_equal(R["in_place"].reshape(shape), DN.draw_spheres(image, c, d, background_offset=1.0)[0], "in place")
    regions = [(DN.SPHERE, (6, 6, 5, 3.5), -1.0), (DN.RECT, (0, -1, 0, -1, 0, -1), 1.0), (DN.RECT, (1, 4.4, 0, 30, 2, 3), 2.5)]
    assert_bits_equal(R["regions_subtract"].reshape(shape), DN.draw_regions(np.zeros(shape, np.float32), regions, None, True),
                      "DrawRegions, subtracting from an empty image")
    assert_bits_equal(R["regions_default"].reshape(shape), DN.draw_regions(image, regions, mask, False), "DrawRegions defaults")
    text = open(tmp_path / "progress.txt").read()
    assert text.startswith("processing coordinates 1 / 5: x,y,z(in_voxels)=4.2,5,6.9, diameter=7, th=1\n")
    assert "processing coordinates 5 / 5: x,y,z(in_voxels)=7.5,6.1,7, diameter=6, th=0\n" in text
    assert "Some coordinates in the text file lie outside the boundaries of the image." in text
    assert text.rstrip().endswith("--------------------------------------------------------------------------=---")


def test_draw_time_option_reports_three_phases(ctx):
    kw = DC.SPHERE_CASES["foreground_normalize"]()
    want, _ = DN.draw_spheres(**kw)
    assert ctx.get_option("draw_time") == 0
    with ctx.options(draw_time=1):
        assert_bits_equal(ctx.draw_spheres(**kw), want, "timed call")
        ms = ctx.draw_last_times()
    assert len(ms) == 3 and all(0.0 <= t < 1000.0 for t in ms), ms
