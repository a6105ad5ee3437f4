"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/visfd_hip.h declares; the Python binding covers exactly that set; host-side arithmetic
entry points (taps, tables) agree with the oracle bit-for-bit.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import volgen
from conftest import ROOT, assert_bits_equal, golden


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "visfd_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(visfd_hip_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    from visfd_amd import api
    if not os.path.exists(api.LIB_PATH):
        from visfd_amd import build
        build.build(verbose=False)
    return api


def test_library_exports_every_declared_symbol(lib):
    L = ctypes.CDLL(lib.LIB_PATH)
    names = _header_symbols()
    assert len(names) >= 40
    for n in names:
        assert hasattr(L, n), "libvisfd_hip.so does not export " + n
    assert sorted(lib.exported_symbols()) == names, "visfd_amd/api.py and include/visfd_hip.h disagree"
    assert L.visfd_hip_abi_version() == 10


def test_binding_types_come_from_the_header(lib):
    """The argument and return types of the binding are parsed from include/visfd_hip.h.  One prototype, typed by hand
    here, for every spelling the header uses: double, const double[3], int64_t[6], float* const*, uint32_t, uint64_t*,
    int32_t, a struct pointer, visfd_hip_ctx**, an unnamed pointer, const char* as a parameter; and for every return
    type: int, void, void*, int64_t, float, const char*."""
    c_int, i64, f32, f64, vp, u32, i32 = (ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_void_p,
                                          ctypes.c_uint32, ctypes.c_int32)
    want = {
        "visfd_hip_create": (c_int, [c_int, vp, vp]),
        "visfd_hip_get_stream": (vp, [vp]),
        "visfd_hip_last_error": (ctypes.c_char_p, []),
        "visfd_hip_set_option": (c_int, [vp, ctypes.c_char_p, i64]),
        "visfd_hip_workspace_bytes": (i64, [vp]),
        "visfd_hip_ratio_from_threshold": (f32, [f32]),
        "visfd_hip_blob_dog_abort": (None, [vp]),
        "visfd_hip_image_stats_host": (c_int, [vp, vp, i64, vp]),
        "visfd_hip_select_histogram_dev": (c_int, [vp, vp, vp, i64, c_int, u32, vp, vp]),
        "visfd_hip_slab_exchange_dev": (c_int, [vp, vp, c_int, i64, i64, c_int]),
        "visfd_hip_voxelize_quantize_host": (c_int, [vp, i64, f64, vp, vp]),
        "visfd_hip_close_surface_last": (c_int, [vp, vp, vp]),
        "visfd_hip_sort_blobs": (c_int, [vp, vp, vp, i64, c_int, c_int, vp]),
        "visfd_hip_watershed": (c_int, [vp, vp, vp, vp, i64, i64, i64, f32, c_int, c_int, c_int, i32, i32, vp, vp, vp, i64, vp]),
        "visfd_hip_isosurface_host": (c_int, [vp, i64, i64, i64, f64, c_int, vp, i64, vp, i64, vp, vp]),
    }
    for name, sig in want.items():
        assert lib._SIGS[name] == sig, name
    L = lib.load_library()
    for name, (res, args) in want.items():
        fn = getattr(L, name)
        assert fn.restype == res and list(fn.argtypes) == args, name


def test_header_parser_refuses_what_it_does_not_know(lib):
    ok = "/* a comment with visfd_hip_ghost(int); in it */\nint visfd_hip_fine(const float* src, int64_t n,\n    double w[3]);\n"
    assert lib._parse_header(ok) == {"visfd_hip_fine": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p])}
    with pytest.raises(ImportError, match="visfd_hip_odd.*long double x"):
        lib._parse_header("int visfd_hip_fine(void);\nint visfd_hip_odd(float a, long double x);\n")
    with pytest.raises(ImportError, match="visfd_hip_odd"):
        lib._parse_header("int visfd_hip_fine(void);\nsize_t visfd_hip_odd(float a);\n")
    for unnamed in ("unsigned long", "unsigned char", "unsigned int"):   # the last word is no parameter name
        with pytest.raises(ImportError, match="visfd_hip_odd.*" + unnamed):
            lib._parse_header("int visfd_hip_odd(float a, %s);\n" % unnamed)
    assert lib._parse_header("int visfd_hip_fine(unsigned, const float scale, int64_t);\n") == {
        "visfd_hip_fine": (ctypes.c_int, [ctypes.c_uint, ctypes.c_float, ctypes.c_int64])}
    with pytest.raises(ImportError, match="visfd_hip_callback"):   # a parenthesised parameter is not skipped silently
        lib._parse_header("int visfd_hip_fine(void);\nint visfd_hip_callback(int (*fn)(void* user), void* user);\n")


def test_host_arithmetic_matches_oracle(lib, oracle):
    for s, h in volgen.TAP_CASES:
        assert_bits_equal(lib.gauss_taps(s, h), oracle.gauss_taps(s, h), "taps")
    g = golden("taps")
    for s, h in volgen.TAP_CASES:
        assert_bits_equal(lib.gauss_taps(s, h), g["s%g_h%d" % (s, h)], "taps vs golden")
    assert np.float32(lib.ratio_from_threshold(0.03)) == g["ratio"]
    assert lib.gauss_halfwidths((2, 2, 0.1), 2.6482) == (5, 5, 1)
    for s, c in ((8.66, 2 ** 0.5), (3.2, 2 ** 0.5), (2.0, 2.5)):
        h, w, r = lib.tv_tables(s, c)
        ho, wo, ro = oracle.tv_tables(s, c)
        assert h == ho
        assert_bits_equal(w, wo, "tv w")
        assert_bits_equal(r, ro, "tv rhat")
    d = np.array([5, 5.8, 6.6, 100.0], np.float32)
    assert_bits_equal(lib.diameters_to_sigmas(d), oracle.diameters_to_sigmas(d), "d2s")
    assert_bits_equal(lib.sigmas_to_diameters(d), oracle.sigmas_to_diameters(d), "s2d")


def test_no_cpu_fallback(lib):
    """Without a GPU the product must fail loudly, not compute on the CPU."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(lib.VisfdHipError):
        lib.Context(0)


def test_cpp_shim_compiles_and_runs_host_entry_points(lib, tmp_path):
    """include/visfd_hip.hpp under g++ -std=c++11 -Wall -Werror, linked against the library; the program exercises
    the reference-signature wrappers of the host-side rows (LabelConnected, blob list post-processing)."""
    import subprocess
    exe = str(tmp_path / "shim_host_check")
    libdir = os.path.dirname(lib.LIB_PATH)
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "shim_host_check.cpp"), "-L" + libdir, "-lvisfd_hip", "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "clusters 2 sizes 270 108 undefined 702" in r.stdout and "blobs kept 2" in r.stdout


@pytest.mark.parametrize("src,flags", [
    ("tv_box.hip", ["-DVH_TV_STAMPS", "-DVH_TV_COUNT"]),
    ("gauss_fused.hip", ["-DVH_FUSED_H=5", "-DVH_FUSED_STAMPS"]),
])
def test_development_builds_cross_compile(src, flags, tmp_path):
    """The only build parameters left in the kernels are the instrumentation switches named in their sources (where a
    wave's time goes; what the voting kernel tests and hits).  They are not part of the product build, so nothing else
    would notice if an edit broke them: cross-compile each for gfx950 (hipcc needs no GPU)."""
    import subprocess
    from visfd_amd import build as B
    cmd = [B.HIPCC] + B.FLAGS + ["-fno-slp-vectorize"] + flags + ["-x", "hip", "-c", os.path.join(B.CSRC, src), "-o", str(tmp_path / "o.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_graft_entry_expects_the_library_abi(lib):
    """__graft_entry__.build() asserts the ABI version of the library it has just built: the number written there must be
    the library's (it was left behind once when the ABI moved on)."""
    L = ctypes.CDLL(lib.LIB_PATH)
    src = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    m = re.search(r"visfd_hip_abi_version\(\) == (\d+)", src)
    assert m and int(m.group(1)) == L.visfd_hip_abi_version()
