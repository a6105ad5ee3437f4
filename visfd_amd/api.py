"""ctypes binding of libvisfd_hip.so (include/visfd_hip.h) for Python hosts.

Two faces, like the C ABI:
  * `Context.<op>(numpy arrays)`      host face  (drop-in: synchronous, copies in and out)
  * `Context.<op>_dev(torch tensors)` device face (asynchronous on the context's stream; tensors
                                      live in HBM; multi-channel fields are channel-planar:
                                      dir (3,nz,ny,nx), tensor (6,nz,ny,nx))

There is NO CPU fallback: loading fails loudly when the HIP library is missing, and creating a
context fails when no GPU is present.  The argument types of the entry points are read from include/visfd_hip.h when this
module is imported (so that `_SIGS` is whole for every reader): without that header next to the package the import fails
with an ImportError that names the path.
"""
import ctypes as C
import os
import re
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VISFD_HIP_LIB") or os.path.join(_HERE, "libvisfd_hip.so")  # env: tuning variants (tools/build_variant.py)

INCREASING_EIVALS = 0
DECREASING_EIVALS = 1

# grayscale morphology ops (VISFD_HIP_MORPH_*, lib/visfd/morphology.hpp:134-597)
MORPH_DILATE, MORPH_ERODE, MORPH_OPEN, MORPH_CLOSE, MORPH_TOP_HAT_WHITE, MORPH_TOP_HAT_BLACK = range(6)
MORPH_PATH_GENERAL, MORPH_PATH_XRUNS, MORPH_PATH_LEVELS = 0, 1, 2   # visfd_hip_morph_last_path
MEDIAN_PATH_GENERAL, MEDIAN_PATH_TILED = 0, 1   # visfd_hip_median_last_path
FILTER3D_PATH_GENERAL, FILTER3D_PATH_TILED = 0, 1   # visfd_hip_filter3d_last_path
DISTANCE_PATH_GENERAL, DISTANCE_PATH_TRANSFORM = 0, 1   # visfd_hip_distance_last_path
DISTANCE_MAX_DIM_SUM = 46340   # VISFD_HIP_DISTANCE_MAX_DIM_SUM

_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int)
_i64 = C.c_int64
_vp = C.c_void_p


class VisfdHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("visfd_hip error %d: %s" % (code, msg))
        self.code = code


class Blob(C.Structure):
    _fields_ = [("ix", C.c_int32), ("iy", C.c_int32), ("iz", C.c_int32), ("scale", C.c_int32),
                ("sigma", C.c_float), ("score", C.c_float)]


class Region(C.Structure):   # visfd_hip_region: a SimpleRegion<float> (draw.hpp:46-81)
    _fields_ = [("type", C.c_int32), ("c", C.c_float * 6), ("value", C.c_float)]


REGION_RECT, REGION_SPHERE = 0, 1


class Stats(C.Structure):   # visfd_hip_stats
    _fields_ = [("count", C.c_int64), ("n_nonfinite", C.c_int64), ("sum", C.c_double), ("min", C.c_float),
                ("max", C.c_float), ("order_free", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k in ("count", "n_nonfinite", "sum", "min", "max", "order_free")}


class Intensity(C.Structure):   # visfd_hip_intensity: the stages of one intensity-map pass (include/visfd_hip.h)
    _fields_ = [("invert", C.c_int32), ("map", C.c_int32), ("mask_fill", C.c_int32), ("rescale01", C.c_int32),
                ("stats_mask", C.c_int32), ("reserved", C.c_int32), ("ave", C.c_double), ("t", C.c_float * 4),
                ("out_a", C.c_float), ("out_b", C.c_float), ("masked_value", C.c_float), ("dmin", C.c_float),
                ("dmax", C.c_float), ("rescale_a", C.c_float), ("rescale_b", C.c_float), ("reserved2", C.c_float)]


MAP_NONE, MAP_STEP, MAP_THRESH2, MAP_THRESH4, MAP_RANGE, MAP_GAUSS, MAP_RESCALE = range(7)   # VISFD_HIP_MAP_*


def intensity(map=MAP_NONE, t=(), out_a=0.0, out_b=1.0, invert_ave=None, masked_value=None, rescale01=None,
              stats_mask=False):
    """A visfd_hip_intensity.  map, t, out_a, out_b: the map and its numbers (MAP_RESCALE: t = (factor, offset));
    invert_ave: invert about this mean where mask != 0; masked_value: the value of voxels with mask == 0;
    rescale01 = (dmin, dmax, a, b): out = a + ((b - a) * (out - dmin)) / (dmax - dmin); stats_mask: statistics under the
    mask.  Stages run in that order (MrcSimple::Invert, HandleThresholds, the mask fill, MrcSimple::Rescale01)."""
    p = Intensity()
    p.map = int(map)
    for k, x in enumerate(t):
        p.t[k] = float(x)
    p.out_a, p.out_b = float(out_a), float(out_b)
    if invert_ave is not None:
        p.invert, p.ave = 1, float(invert_ave)
    if masked_value is not None:
        p.mask_fill, p.masked_value = 1, float(masked_value)
    if rescale01 is not None:
        p.rescale01 = 1
        p.dmin, p.dmax, p.rescale_a, p.rescale_b = [float(x) for x in rescale01]
    p.stats_mask = int(bool(stats_mask))
    return p


# ---- the signatures of the entry points, read from the header the library is compiled against
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "visfd_hip.h")
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "unsigned": C.c_uint, "uint32_t": C.c_uint32, "int64_t": C.c_int64,
            "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}
_RETURNS = dict(_SCALARS, **{"void": None, "void*": _vp, "const char*": C.c_char_p})
_PROTOTYPE = re.compile(r"^[ \t]*(\w[\w \t*]*?)[ \t]*\b(visfd_hip_\w+)[ \t]*\(([^()]*)\)\s*;", re.M)
_TYPE_WORDS = {"int", "long", "short", "char", "unsigned", "signed", "float", "double"}   # never a parameter's name


def _scalar(p):
    """The ctypes type of a scalar parameter `[const] type [name]`, or None: the whole spelling is tried as a type first, so
    that the last word of an unnamed `unsigned long` is not taken for a name"""
    words = [w for w in p.split() if w != "const"]
    if " ".join(words) in _SCALARS:
        return _SCALARS[" ".join(words)]
    if len(words) > 1 and words[-1] not in _TYPE_WORDS:
        return _SCALARS.get(" ".join(words[:-1]))
    return None


def _parse_header(text):
    """The prototypes `ret visfd_hip_name(args);` of a C header -> {name: (restype, [argtypes])} for ctypes.  Scalars by
    their spelling, `const char*` as c_char_p, every other pointer or array as c_void_p (which takes byref(), ctypes arrays
    and pointers, integers and None).  A spelling that is not in the tables raises and names the prototype, and so does a
    visfd_hip_ name followed by `(` that is no such prototype (a parenthesised parameter, say): nothing is skipped."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    sigs = {}
    for ret, name, params in _PROTOTYPE.findall(text):
        proto = "%s %s(%s)" % (ret, name, " ".join(params.split()))
        ret = re.sub(r"\s*\*", "*", " ".join(ret.split()))
        if ret not in _RETURNS:
            raise ImportError("cannot bind `%s`: return type %r is not one the binding knows" % (proto, ret))
        args = []
        for p in [" ".join(p.split()) for p in params.split(",") if params.strip() not in ("", "void")]:
            if re.fullmatch(r"const char ?\*(?: ?\w+)?", p):
                args.append(C.c_char_p)
            elif "*" in p or "[" in p:
                args.append(_vp)
            elif _scalar(p) is not None:
                args.append(_scalar(p))
            else:
                raise ImportError("cannot bind `%s`: parameter %r is not of a type the binding knows" % (proto, p))
        sigs[name] = (_RETURNS[ret], args)
    unread = set(re.findall(r"\b(visfd_hip_\w+)\s*\(", text)) - set(sigs)
    if unread:
        raise ImportError("cannot bind %s: not of the form `ret name(args);`" % ", ".join(sorted(unread)))
    return sigs


def _header_signatures():
    if not os.path.exists(HEADER_PATH):
        raise ImportError("%s is missing: the binding reads the entry points' signatures from it" % HEADER_PATH)
    with open(HEADER_PATH) as f:
        return _parse_header(f.read())


_SIGS = _header_signatures()

_SENDRECV = C.CFUNCTYPE(C.c_int, _vp, C.c_int, _vp, _vp, C.c_size_t, _vp)
_ALLREDUCE = C.CFUNCTYPE(C.c_int, _vp, _vp, C.c_size_t, _vp)
_GROUP = C.CFUNCTYPE(C.c_int, _vp)


class Transport(C.Structure):   # visfd_hip_transport
    _fields_ = [("sendrecv", _SENDRECV), ("allreduce_sum_u64", _ALLREDUCE), ("group_start", _GROUP), ("group_end", _GROUP),
                ("user", _vp)]

_lib = None


def load_library():
    """Load libvisfd_hip.so; raises if it has not been built (python -m visfd_amd.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: build it with `python -m visfd_amd.build` "
                              "(there is no CPU fallback)" % LIB_PATH)
        # PyTorch-ROCm ships its own copy of the HIP runtime; if this library pulled in the system copy first, a
        # later `import torch` in the same process would bring a second runtime that cannot see the GPU ("no
        # ROCm-capable device").  Loading torch's first makes both share one runtime.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def exported_symbols():
    return sorted(_SIGS)


WATERSHED_PATH_HOST, WATERSHED_PATH_DEVICE = 0, 1


def _watershed(call, src, mask, markers, shape, labels, halt_threshold, start_from_minima, connectivity, show_boundaries,
               label_boundary, label_undefined):
    """The capacity protocol of the watershed entry points (as for find_extrema): -> (basin index int64, score float32).
    `call(*tail)` gets everything after the context.  halt_threshold None: no threshold (+inf, or -inf from maxima)."""
    nz, ny, nx = shape
    if halt_threshold is None:
        halt_threshold = float("inf") if start_from_minima else -float("inf")
    cap = max(65536, nz * ny * nx // 32)
    while True:
        index, score, n = np.empty(cap, np.int64), np.empty(cap, np.float32), _i64()
        rc = call(src, mask, markers, nx, ny, nz, float(halt_threshold), int(bool(start_from_minima)), int(connectivity),
                  int(bool(show_boundaries)), int(label_boundary), int(label_undefined), labels, index.ctypes.data,
                  score.ctypes.data, cap, C.byref(n))
        if rc == 4 and n.value > cap:   # VISFD_HIP_ECAPACITY
            cap = int(n.value)
            continue
        if rc != 0:
            raise VisfdHipError(rc, load_library().visfd_hip_last_error().decode())
        return index[:n.value].copy(), score[:n.value].copy()


def _markers_np(markers, shape):
    if markers is None:
        return None
    assert isinstance(markers, np.ndarray) and markers.dtype == np.int32 and markers.flags["C_CONTIGUOUS"] and \
        markers.shape == tuple(shape), "markers: C int32 of src's shape"
    return markers


def watershed_host(src, mask=None, markers=None, halt_threshold=None, start_from_minima=True, connectivity=1,
                   show_boundaries=True, label_boundary=0, label_undefined=-1):
    """visfd::Watershed by the sequential flood on the host (visfd_hip_watershed_host: no context, no device), with or
    without markers (int32, entries <= 0 ignored): -> (labels int32, basin index int64, basin score float32)."""
    L = load_library()
    markers = _markers_np(markers, src.shape)
    labels = np.empty(src.shape, np.int32)
    index, score = _watershed(L.visfd_hip_watershed_host, _np(src), _np(mask), None if markers is None else markers.ctypes.data,
                              src.shape, labels.ctypes.data, halt_threshold, start_from_minima, connectivity, show_boundaries,
                              label_boundary, label_undefined)
    return labels, index, score


def _np(a):
    if a is None:
        return None
    assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags["C_CONTIGUOUS"], "need C float32"
    return a.ctypes.data


def _dev(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous() and str(t.dtype) == "torch.float32", "need contiguous cuda float32"
    return t.data_ptr()


# A face of the C ABI as Context._rc takes it: (symbol suffix, converter of float32 arrays to addresses).  _HOST_CTX: the few
# host-array entries named visfd_hip_<op>_ctx, where the plain name is the entry without a context.
_HOST, _HOST_CTX, _DEVICE = ("", _np), ("_ctx", _np), ("_dev", _dev)
_DEVICE_PLAIN = ("", _dev)   # device tensors behind a name without the suffix (visfd_hip_select_histogram_todev)


def _face_of(a):
    """The face of the methods that take numpy arrays or torch device tensors alike"""
    return _HOST if isinstance(a, np.ndarray) else _DEVICE


def _address(a):
    """Where an array of any element type starts: numpy on the host, torch on the device (checked by the caller)"""
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


def _points(points):
    """(n, 3) int32 rows x, y, z on the host (None: no points)"""
    if points is None:
        return np.zeros((0, 3), np.int32)
    return np.ascontiguousarray(points, np.int32).reshape(-1, 3)


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def _i3(v):
    return (C.c_int * 3)(*[int(x) for x in v])


def gauss_taps(sigma, h):
    out = np.empty(2 * h + 1, np.float32)
    rc = load_library().visfd_hip_gauss_taps(float(sigma), int(h), out.ctypes.data_as(_fp))
    if rc:
        raise VisfdHipError(rc, load_library().visfd_hip_last_error().decode())
    return out


def ratio_from_threshold(thr):
    return float(load_library().visfd_hip_ratio_from_threshold(float(thr)))


def blob_halo_depth(sigmas, delta, ratio):
    """visfd_hip_blob_halo_depth: the halo depth of the slab blob stage (widest LoG Z half-width + 1, float arithmetic)."""
    sig = np.ascontiguousarray(sigmas, np.float32).reshape(-1)
    out = C.c_int()
    L = load_library()
    _chk_host(L, L.visfd_hip_blob_halo_depth(sig.ctypes.data_as(_fp), len(sig), float(delta), float(ratio), C.byref(out)))
    return int(out.value)


def gauss_halfwidths(sigma, ratio):
    hw = (C.c_int * 3)()
    load_library().visfd_hip_gauss_halfwidths(_f3(sigma), float(ratio), hw)
    return tuple(hw)


def fluctuation_sigmas(radius, exponent=2.0, truncate_ratio=-1.0, truncate_threshold=0.03):
    """LocalFluctuationsByRadius' parameter arithmetic (filter3d.hpp:1908-1914, filter3d_variants.hpp:663-669):
    -> (sigma[3], ratio)."""
    sg = (C.c_float * 3)()
    r = C.c_float()
    load_library().visfd_hip_fluctuation_sigmas(_f3(radius), float(exponent), float(truncate_ratio),
                                                float(truncate_threshold), sg, C.byref(r))
    return tuple(sg), r.value


def sphere_structure(radius, radius_max=0.0, bmax=0.0):
    """The structuring element of DilateSphere / ErodeSphere (morphology.hpp:254-316): (dxyz int32 (n, 3), b float32 (n,)),
    in the reference's order (dz outermost, then dy, then dx)."""
    L = load_library()
    n = C.c_int64()
    _chk_host(L, L.visfd_hip_sphere_structure(float(radius), float(radius_max), float(bmax), None, None, 0, C.byref(n)))
    d = np.zeros((max(n.value, 1), 3), np.int32)
    b = np.zeros(max(n.value, 1), np.float32)
    _chk_host(L, L.visfd_hip_sphere_structure(float(radius), float(radius_max), float(bmax), d.ctypes.data_as(_ip),
                                              b.ctypes.data_as(_fp), len(b), C.byref(n)))
    return d[:n.value].copy(), b[:n.value].copy()


def flat_ball_dsq_max(radius):
    """The flat ball of DilateSphere / ErodeSphere (bmax == 0) as a threshold: offset (dx, dy, dz) is in sphere_structure(radius)
    exactly when dx^2 + dy^2 + dz^2 <= this integer.  Host arithmetic, any finite radius >= 0."""
    L = load_library()
    t = C.c_int64()
    _chk_host(L, L.visfd_hip_flat_ball_dsq_max(float(radius), C.byref(t)))
    return int(t.value)


def median_footprint(radius):
    """The footprint of MedianSphere (filter3d.hpp:1652-1662): dxyz int32 (n, 3) in the reference's order (dz outermost,
    then dy, then dx)."""
    L = load_library()
    n = C.c_int64()
    _chk_host(L, L.visfd_hip_median_footprint(float(radius), None, 0, C.byref(n)))
    d = np.zeros((n.value, 3), np.int32)
    _chk_host(L, L.visfd_hip_median_footprint(float(radius), d.ctypes.data_as(_ip), len(d), C.byref(n)))
    return d


def image_stats_host(src, mask=None):
    """visfd_hip_image_stats_host: the statistics of Context.image_stats from a plain host loop (no device) -> dict."""
    L = load_library()
    st = Stats()
    _chk_host(L, L.visfd_hip_image_stats_host(_np(src), _np(mask), src.size, C.byref(st)))
    return st.as_dict()


def intensity_map_host(p, out, src=None, mask=None, want_stats=False):
    """visfd_hip_intensity_map_host: Context.intensity_map by a plain host loop (no device); `out` is written in place."""
    L = load_library()
    nz, ny, nx = out.shape
    st = Stats()
    _chk_host(L, L.visfd_hip_intensity_map_host(_np(src), _np(out), _np(mask), nx, ny, nz, C.byref(p),
                                                C.byref(st) if want_stats else None))
    return st.as_dict() if want_stats else None


def gengauss3d_halfwidths(width, m_exp, truncate_ratio=-1.0, truncate_threshold=0.03):
    """Window of the generalised Gaussians (filter3d_variants.hpp:99-103, filter3d.hpp:631-633): floor(width * ratio), a
    negative ratio first replaced by pow(-log(threshold), 1 / m_exp).  -> (hx, hy, hz)"""
    L = load_library()
    hw = (C.c_int * 3)()
    _chk_host(L, L.visfd_hip_gengauss3d_halfwidths(_f3(width), float(m_exp), float(truncate_ratio),
                                                   float(truncate_threshold), hw))
    return tuple(hw)


def gengauss3d_table(width, m_exp, halfwidth):
    """GenFilterGenGauss3D(width, m_exp, halfwidth) (filter3d.hpp:546-601) -> (table float32 (2hz+1, 2hy+1, 2hx+1), A)."""
    L = load_library()
    hw = [int(h) for h in halfwidth]
    n = C.c_int64()
    _chk_host(L, L.visfd_hip_gengauss3d_table(_f3(width), float(m_exp), _i3(hw), None, 0, C.byref(n), None))
    t = np.empty((2 * hw[2] + 1, 2 * hw[1] + 1, 2 * hw[0] + 1), np.float32)
    A = C.c_float()
    _chk_host(L, L.visfd_hip_gengauss3d_table(_f3(width), float(m_exp), _i3(hw), t.ctypes.data_as(_fp), t.size,
                                              C.byref(n), C.byref(A)))
    return t, A.value


def dogg3d_table(width_a, width_b, m_exp, n_exp, truncate_ratio=-1.0, truncate_threshold=0.03):
    """GenFilterDogg3D (filter3d_variants.hpp:284-345, :441-482) -> (table float32 (2hz+1, 2hy+1, 2hx+1), A, B)."""
    L = load_library()
    args = (_f3(width_a), _f3(width_b), float(m_exp), float(n_exp), float(truncate_ratio), float(truncate_threshold))
    hw = (C.c_int * 3)()
    n = C.c_int64()
    _chk_host(L, L.visfd_hip_dogg3d_table(*(args + (hw, None, 0, C.byref(n), None, None))))
    t = np.empty((2 * hw[2] + 1, 2 * hw[1] + 1, 2 * hw[0] + 1), np.float32)
    A, B = C.c_float(), C.c_float()
    _chk_host(L, L.visfd_hip_dogg3d_table(*(args + (hw, t.ctypes.data_as(_fp), t.size, C.byref(n), C.byref(A),
                                                    C.byref(B)))))
    return t, A.value, B.value


def _filter_table(table):
    """A 3-D table (2hz+1, 2hy+1, 2hx+1) as the C ABI takes it: (float32 array, (hx, hy, hz))."""
    t = np.ascontiguousarray(table, np.float32)
    assert t.ndim == 3 and all(s % 2 == 1 for s in t.shape), "a filter table has an odd number of entries per axis"
    return t, _i3([(t.shape[2] - 1) // 2, (t.shape[1] - 1) // 2, (t.shape[0] - 1) // 2])


def _sphere_lists(centers, diameters, shell_thicknesses, foreground):
    """The four host lists of draw_spheres as ctypes arguments; None stays NULL (the reference's defaults)."""
    c = np.ascontiguousarray(centers, np.float32).reshape(-1, 3)
    n = c.shape[0]
    keep, ptrs = [c], [c.ctypes.data_as(_fp)]
    for a in (diameters, shell_thicknesses, foreground):
        if a is None:
            ptrs.append(None)
            continue
        a = np.ascontiguousarray(a, np.float32).reshape(-1)
        assert a.shape[0] == n, "one entry per sphere"
        keep.append(a)
        ptrs.append(a.ctypes.data_as(_fp))
    return n, ptrs, keep


def _regions(regions):
    """[(type, (six or four floats), value), ...] or Region objects -> (Region array, n)."""
    arr = (Region * max(len(regions), 1))()
    for k, r in enumerate(regions):
        if isinstance(r, Region):
            arr[k] = r
            continue
        t, c, v = r
        arr[k].type = int(t)
        for j, x in enumerate(c):
            arr[k].c[j] = float(x)
        arr[k].value = float(v)
    return arr, len(regions)


def _morph_table(dxyz, b):
    d = np.ascontiguousarray(dxyz, np.int32).reshape(-1, 3)
    bb = np.ascontiguousarray(b, np.float32).reshape(-1)
    assert len(d) == len(bb), "one b per (dx, dy, dz)"
    return d, bb


def tv_tables(sigma_tv, cutoff):
    L = load_library()
    h = C.c_int()
    L.visfd_hip_tv_tables(float(sigma_tv), float(cutoff), C.byref(h), None, None)
    n = 2 * h.value + 1
    w = np.empty((n, n, n), np.float32)
    r = np.empty((n, n, n, 3), np.float32)
    L.visfd_hip_tv_tables(float(sigma_tv), float(cutoff), C.byref(h), w.ctypes.data_as(_fp), r.ctypes.data_as(_fp))
    return h.value, w, r


def diameters_to_sigmas(d):
    d = np.ascontiguousarray(d, np.float32)
    s = np.empty_like(d)
    load_library().visfd_hip_blob_diameters_to_sigmas(d.ctypes.data_as(_fp), len(d), s.ctypes.data_as(_fp))
    return s


def sigmas_to_diameters(s):
    s = np.ascontiguousarray(s, np.float32)
    d = np.empty_like(s)
    load_library().visfd_hip_blob_sigmas_to_diameters(s.ctypes.data_as(_fp), len(s), d.ctypes.data_as(_fp))
    return d


# ---- voxel clustering (host-side) ---------------------------------------------------------
CONNECT_SEEDS_DEVICE, CONNECT_SEEDS_HOST = 0, 1   # visfd_hip_label_connected_device_seeds_last


def _must_link_arrays(must_link, must_link_directions):
    """must_link: list of groups, each a list of (x, y, z) locations in voxels; must_link_directions: the same shape of
    0 / 1 / 2 (same / opposite / automatic, connect.hpp DirectionPairType) or None -> (crds, group sizes, directions, n)"""
    ml_c = ml_n = ml_d = None
    ngroups = 0
    if must_link:
        ngroups = len(must_link)
        ml_c = np.ascontiguousarray(np.concatenate([np.asarray(g_, np.float32).reshape(-1, 3) for g_ in must_link], 0))
        ml_n = np.array([len(g_) for g_ in must_link], np.int64)
        if must_link_directions is not None:
            ml_d = np.ascontiguousarray(np.concatenate([np.asarray(d_, np.int32).ravel() for d_ in must_link_directions]))
    return ml_c, ml_n, ml_d, ngroups


def label_connected(saliency, threshold_saliency, mask=None, direction=None, tensor=None,
                    threshold_vector_saliency=-np.inf, threshold_vector_neighbor=-np.inf, consider_dot_product_sign=True,
                    threshold_tensor_saliency=-np.inf, threshold_tensor_neighbor=-np.inf,
                    tensor_is_positive_definite_near_target=True, connectivity=1, label_undefined=-1, sort_by_size=True,
                    standardize_directions=False, start_from_saliency_maxima=True, voxel_weights=None, must_link=None,
                    must_link_directions=None, seeds_ctx=None):
    """LabelConnected (connect.hpp:168-1427).  saliency [nz,ny,nx]; direction [nz,ny,nx,3] (rewritten in place when
    standardize_directions); tensor [nz,ny,nx,6].  Returns (labels int64 [nz,ny,nx], n_clusters, seed positions
    [n,3] in final order, sizes [n] and seed saliencies [n] in provisional order).  seeds_ctx (a Context): the seeds
    are searched on its device (Context.label_connected_device_seeds_last says whether); the flood runs on the host either
    way and the results are the same bits."""
    L = load_library()
    nz, ny, nx = saliency.shape
    labels = np.empty((nz, ny, nx), np.int64)
    n = _i64(0)
    cap = int(saliency.size)
    cm, cs, csal = np.zeros((cap, 3), np.float32), np.zeros(cap, np.float32), np.zeros(cap, np.float32)
    for a in (direction, tensor):
        assert a is None or (a.dtype == np.float32 and a.flags["C_CONTIGUOUS"])
    ml_c, ml_n, ml_d, ngroups = _must_link_arrays(must_link, must_link_directions)
    ptr = lambda a: None if a is None else a.ctypes.data
    args = (_np(saliency), labels.ctypes.data, _np(mask), nx, ny, nz, threshold_saliency,
            None if direction is None else direction.ctypes.data, threshold_vector_saliency, threshold_vector_neighbor,
            int(bool(consider_dot_product_sign)), None if tensor is None else tensor.ctypes.data, threshold_tensor_saliency,
            threshold_tensor_neighbor, int(bool(tensor_is_positive_definite_near_target)), int(connectivity),
            int(label_undefined), int(bool(sort_by_size)), int(bool(standardize_directions)),
            int(bool(start_from_saliency_maxima)), C.byref(n), cm.ctypes.data, cs.ctypes.data, csal.ctypes.data, cap,
            _np(voxel_weights), ptr(ml_c), ptr(ml_n), ngroups, ptr(ml_d))
    if seeds_ctx is None:
        _chk_host(L, L.visfd_hip_label_connected_ex(*args))
    else:
        _chk_host(L, L.visfd_hip_label_connected_device_seeds(seeds_ctx._h, *args))
    k = n.value
    return labels, k, cm[:k], cs[:k], csal[:k]


# visfd_hip_label_connected_graph_last: the path a graph call took, and why a call was handed to the flood
CONNECT_GRAPH_DEVICE, CONNECT_GRAPH_HOST_GRAPH, CONNECT_GRAPH_FLOOD = 0, 1, 2
(CONNECT_REASON_ASYMMETRIC, CONNECT_REASON_ZERO_DOT, CONNECT_REASON_UNBALANCED, CONNECT_REASON_MUST_LINK,
 CONNECT_REASON_WEIGHTS, CONNECT_REASON_OUTWARD, CONNECT_REASON_LIMITS) = (1 << k for k in range(7))


def label_connected_graph(saliency, threshold_saliency, mask=None, direction=None, tensor=None,
                          threshold_vector_saliency=-np.inf, threshold_vector_neighbor=-np.inf, consider_dot_product_sign=True,
                          threshold_tensor_saliency=-np.inf, threshold_tensor_neighbor=-np.inf,
                          tensor_is_positive_definite_near_target=True, connectivity=1, label_undefined=-1, sort_by_size=True,
                          standardize_directions=False, start_from_saliency_maxima=True, voxel_weights=None, must_link=None,
                          must_link_directions=None, ctx=None):
    """label_connected as a graph problem (include/visfd_hip.h: visfd_hip_label_connected_graph): the same labels, lists
    and directions of labelled voxels, bit for bit; the directions of unlabelled and masked voxels stay as they came in.
    numpy arrays.  ctx (a Context): the work runs on its device (Context.label_connected_graph_last says what it did);
    None: the serial host walk (label_connected_graph_last() without a context)."""
    L = load_library()
    nz, ny, nx = saliency.shape
    labels = np.empty((nz, ny, nx), np.int64)
    n = _i64(0)
    cap = int(saliency.size)
    cm, cs, csal = np.zeros((cap, 3), np.float32), np.zeros(cap, np.float32), np.zeros(cap, np.float32)
    for a in (direction, tensor):
        assert a is None or (a.dtype == np.float32 and a.flags["C_CONTIGUOUS"])
    ml_c, ml_n, ml_d, ngroups = _must_link_arrays(must_link, must_link_directions)
    ptr = lambda a: None if a is None else a.ctypes.data
    args = (_np(saliency), labels.ctypes.data, _np(mask), nx, ny, nz, threshold_saliency, ptr(direction),
            threshold_vector_saliency, threshold_vector_neighbor, int(bool(consider_dot_product_sign)), ptr(tensor),
            threshold_tensor_saliency, threshold_tensor_neighbor, int(bool(tensor_is_positive_definite_near_target)),
            int(connectivity), int(label_undefined), int(bool(sort_by_size)), int(bool(standardize_directions)),
            int(bool(start_from_saliency_maxima)), C.byref(n), cm.ctypes.data, cs.ctypes.data, csal.ctypes.data, cap,
            _np(voxel_weights), ptr(ml_c), ptr(ml_n), ngroups, ptr(ml_d))
    if ctx is None:
        _chk_host(L, L.visfd_hip_label_connected_graph_host(*args))
    else:
        ctx._call("label_connected_graph", _HOST, *args)
    k = n.value
    return labels, k, cm[:k], cs[:k], csal[:k]


def label_connected_graph_last(ctx=None):
    """(path, reasons, valid voxels, candidates of the host's vector test) of the context's last graph call, or of this
    thread's last host walk: CONNECT_GRAPH_* and CONNECT_REASON_* bits."""
    L = load_library()
    p, r, v, u = C.c_int(-1), C.c_uint(0), _i64(-1), _i64(-1)
    _chk_host(L, L.visfd_hip_label_connected_graph_last(None if ctx is None else ctx._h, C.byref(p), C.byref(r), C.byref(v),
                                                        C.byref(u)))
    return p.value, r.value, v.value, u.value


def tensor_saliency_host(tensor, order, sal_inout, mask=None):
    """lambda0 - lambda1 of every [.., 6] tensor, host arithmetic (handlers.cpp:1868-1888), into sal_inout."""
    L = load_library()
    _chk_host(L, L.visfd_hip_tensor_saliency_host(_np(tensor), _np(mask), int(tensor.size // 6), int(order),
                                                  _np(sal_inout)))
    return sal_inout


def diagonalize_sym3_f32_host(m, order):
    """DiagonalizeSym3<float> (eigen3_simple.hpp:137-266) of m [..., 3, 3] -> (eivals [..., 3], eivects [..., 3, 3] rows)."""
    L = load_library()
    m = np.ascontiguousarray(m, np.float32)
    vals = np.empty(m.shape[:-2] + (3,), np.float32)
    vecs = np.empty(m.shape, np.float32)
    mf, vf, ef = m.reshape(-1, 9), vals.reshape(-1, 3), vecs.reshape(-1, 9)
    for i in range(len(mf)):
        _chk_host(L, L.visfd_hip_diagonalize_sym3_f32_host(mf[i].ctypes.data, int(order), vf[i].ctypes.data, ef[i].ctypes.data))
    return vals, vecs


def diagonalize_flat_sym3_host(m6, order):
    """DiagonalizeFlatSym3 (eigen3_simple.hpp:271-342) of [..., 6] flat matrices on the host -> [..., 6]."""
    L = load_library()
    m6 = np.ascontiguousarray(m6, np.float32)
    out = np.empty_like(m6)
    _chk_host(L, L.visfd_hip_diagonalize_flat_sym3_host(m6.ctypes.data, out.ctypes.data, int(m6.size // 6), int(order)))
    return out


def convert_flat_sym2_evects3_host(m6, order):
    """ConvertFlatSym2Evects3<float> of [..., 6] flat matrices -> (eivals [..., 3], eivects [..., 3, 3] rows)."""
    L = load_library()
    m6 = np.ascontiguousarray(m6, np.float32)
    vals = np.empty(m6.shape[:-1] + (3,), np.float32)
    vecs = np.empty(m6.shape[:-1] + (3, 3), np.float32)
    mf, vf, ef = m6.reshape(-1, 6), vals.reshape(-1, 3), vecs.reshape(-1, 9)
    for i in range(len(mf)):
        _chk_host(L, L.visfd_hip_convert_flat_sym2_evects3_host(mf[i].ctypes.data, int(order), vf[i].ctypes.data,
                                                               ef[i].ctypes.data))
    return vals, vecs


def principal_directions_host(tensor, order, mask=None):
    """Eigenvector row 0 of every [.., 6] tensor, host arithmetic (handlers.cpp:1935-1952) -> [.., 3]."""
    L = load_library()
    out = np.zeros(tensor.shape[:-1] + (3,), np.float32)
    _chk_host(L, L.visfd_hip_principal_directions_host(_np(tensor), _np(mask), int(tensor.size // 6), int(order),
                                                       out.ctypes.data))
    return out


# ---- blob list post-processing (host-side).  Blob lists are (crds[n,3], diameters[n], scores[n]).
DO_NOT_SORT, SORT_DECREASING, SORT_INCREASING, SORT_DECREASING_MAGNITUDE, SORT_INCREASING_MAGNITUDE = range(5)


def _chk_host(L, rc):
    if rc:
        raise VisfdHipError(rc, L.visfd_hip_last_error().decode())


# visfd_hip_surface_points_last (VISFD_HIP_SURFACE_POINTS_PATH_*, _REASON_*)
SURFACE_POINTS_PATH_DEVICE, SURFACE_POINTS_PATH_HANDED_OVER = 0, 1
SURFACE_POINTS_REASON_STEPS, SURFACE_POINTS_REASON_BOUNDS = 1, 2


def _surface_points(call, L, shape, select_cluster, voxel_width, curve_ds, find_ridge, max_distance_to_feature, capacity):
    """One surface-points entry behind call(select, width, ds, ridge, maxd, crds, norms, capacity, n) -> (crds, norms) as
    numpy (n, 3).  capacity None: room for 65536 points, and once more with the reported count where that is too little; a
    given capacity is passed as it is, and VISFD_HIP_ECAPACITY raises with the needed count in the error's `needed`."""
    cap = 65536 if capacity is None else int(capacity)
    for attempt in range(2):
        crds, norms = np.zeros((cap, 3), np.float32), np.zeros((cap, 3), np.float32)
        n = _i64(0)
        rc = call(int(select_cluster), _f3(voxel_width), float(curve_ds), int(bool(find_ridge)),
                  float(max_distance_to_feature), crds.ctypes.data, norms.ctypes.data, cap, C.byref(n))
        if rc == 4 and capacity is None and attempt == 0:   # VISFD_HIP_ECAPACITY: the count came back
            cap = int(n.value)
            continue
        if rc:
            err = VisfdHipError(rc, L.visfd_hip_last_error().decode())
            err.needed = int(n.value)
            raise err
        return crds[:n.value], norms[:n.value]


def surface_points_host(saliency, direction, voxel2cluster=None, mask=None, select_cluster=1, voxel_width=(1, 1, 1),
                        curve_ds=0.2, find_ridge=True, max_distance_to_feature=1.3, capacity=None):
    """visfd_hip_surface_points (the -normals-file tail of HandleTV, handlers.cpp:2039-2309) on the host: saliency, mask and
    voxel2cluster (the labels as floats; None: every unmasked voxel as it is) float32 [nz, ny, nx], direction [nz, ny, nx, 3]
    -> (crds, norms), numpy (n, 3) each."""
    L = load_library()
    nz, ny, nx = saliency.shape
    return _surface_points(lambda *t: L.visfd_hip_surface_points(_np(saliency), _np(voxel2cluster), _np(direction), _np(mask),
                                                                 nx, ny, nz, *t),
                           L, saliency.shape, select_cluster, voxel_width, curve_ds, find_ridge, max_distance_to_feature, capacity)


# visfd_hip_discard_overlapping_blobs_last (VISFD_HIP_DISCARD_OVERLAP_PATH_*, _REASON_*)
DISCARD_OVERLAP_PATH_DEVICE, DISCARD_OVERLAP_PATH_HOST, DISCARD_OVERLAP_PATH_HANDED_OVER = 0, 1, 2
(DISCARD_OVERLAP_REASON_NONE, DISCARD_OVERLAP_REASON_NONFINITE, DISCARD_OVERLAP_REASON_NEGATIVE, DISCARD_OVERLAP_REASON_COUNT,
 DISCARD_OVERLAP_REASON_BOUNDS, DISCARD_OVERLAP_REASON_CELLS, DISCARD_OVERLAP_REASON_ROUNDS) = range(7)
DISCARD_OVERLAP_LAST_FIELDS = ("path", "reason", "rounds", "blobs_in", "blobs_kept", "pairs_crit", "pairs_share", "table_cells")


def _blob_arrays(crds, diameters, scores):
    c = np.ascontiguousarray(crds, np.float32).reshape(-1, 3).copy()
    d = np.ascontiguousarray(diameters, np.float32).copy()
    s = np.ascontiguousarray(scores, np.float32).copy()
    assert len(c) == len(d) == len(s), "blob lists differ in length"
    return c, d, s


def _fptr(a):
    return a.ctypes.data_as(_fp)


def sphere_overlap(rij, ri, rj):
    """CalcSphereOverlap (visfd_utils.hpp:95-118)."""
    return float(load_library().visfd_hip_sphere_overlap(rij, ri, rj))


def sort_blobs(crds, diameters, scores, criteria=SORT_DECREASING_MAGNITUDE, ascending=True):
    """SortBlobs (feature.hpp:573-616): returns (crds, diameters, scores, permutation)."""
    L = load_library()
    c, d, s = _blob_arrays(crds, diameters, scores)
    perm = np.arange(len(d), dtype=np.uint64)
    _chk_host(L, L.visfd_hip_sort_blobs(_fptr(c), _fptr(d), _fptr(s), len(d), int(criteria), int(bool(ascending)),
                                        perm.ctypes.data_as(C.POINTER(C.c_uint64))))
    return c, d, s, perm


def discard_masked_blobs(crds, diameters, scores, mask):
    """DiscardMaskedBlobs (feature.hpp:924-969); mask: [nz, ny, nx] float32 or None."""
    L = load_library()
    c, d, s = _blob_arrays(crds, diameters, scores)
    n = _i64(len(d))
    if mask is None:
        return c, d, s
    nz, ny, nx = mask.shape
    _chk_host(L, L.visfd_hip_discard_masked_blobs(_fptr(c), _fptr(d), _fptr(s), C.byref(n), _np(mask), nx, ny, nz))
    return c[:n.value], d[:n.value], s[:n.value]


def discard_overlapping_blobs(crds, diameters, scores, min_radial_separation_ratio, max_volume_overlap_large=np.inf,
                              max_volume_overlap_small=np.inf, criteria=SORT_DECREASING_MAGNITUDE, scale=6, ctx=None):
    """DiscardOverlappingBlobs (feature.hpp:720-913): greedy non-max suppression, best blobs first.  ctx (a Context, or
    None): with None the sequential host walk, otherwise Context.discard_overlapping_blobs on that context's device; the
    lists are the same bits either way."""
    if ctx is not None:
        return ctx.discard_overlapping_blobs(crds, diameters, scores, min_radial_separation_ratio, max_volume_overlap_large,
                                             max_volume_overlap_small, criteria, scale)
    L = load_library()
    c, d, s = _blob_arrays(crds, diameters, scores)
    n = _i64(len(d))
    _chk_host(L, L.visfd_hip_discard_overlapping_blobs(_fptr(c), _fptr(d), _fptr(s), C.byref(n),
                                                       min_radial_separation_ratio, max_volume_overlap_large,
                                                       max_volume_overlap_small, int(criteria), int(scale)))
    return c[:n.value], d[:n.value], s[:n.value]


# ---- FindSpheres and the supervised score thresholds.  `ctx` (a Context, or None): with None the spheres are searched by
# the host walk (visfd_hip_find_spheres_host), otherwise on that context's device.
FIND_SPHERES_PATH_DEVICE, FIND_SPHERES_PATH_HOST = 0, 1   # visfd_hip_find_spheres_last_path
FIND_SPHERES_MAX_R = 46340   # VISFD_HIP_FIND_SPHERES_MAX_R


def _crds(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1, 3)


def _handle(ctx):
    return None if ctx is None else ctx._h


def _mesh(vertices, triangles):
    """(n, 3) float32 vertices (x, y, z) and (m, 3) int32 triangles as C arrays."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
    return v, t


def _d3(v):
    return (C.c_double * 3)(*[float(x) for x in v])


def voxelize_quantize_host(vertices, voxel_width=1.0, origin=(0, 0, 0)):
    """The voxeliser's quantisation (visfd_hip_voxelize_quantize_host): nearbyint((v / voxel_width - origin) * 1024) in
    double, as int32 (n, 3); refused when a vertex is not finite or ends beyond 2^29, or the width is zero."""
    L = load_library()
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    q = np.empty(v.shape, np.int32)
    _chk_host(L, L.visfd_hip_voxelize_quantize_host(v.ctypes.data, len(v), float(voxel_width), _d3(origin), q.ctypes.data))
    return q


def mesh_edges_host(triangles, n_vertices):
    """visfd_hip_mesh_edges_host -> (boundary edges, non-manifold edges): undirected edges used by exactly one triangle, and
    by more than two."""
    L = load_library()
    t = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
    nb, nn = _i64(), _i64()
    _chk_host(L, L.visfd_hip_mesh_edges_host(t.ctypes.data, len(t), int(n_vertices), C.byref(nb), C.byref(nn)))
    return int(nb.value), int(nn.value)


CLOSE_OUTWARD, CLOSE_INWARD, CLOSE_AUTO = 0, 1, 2   # VISFD_HIP_CLOSE_*
CLOSE_STOP_RTOL, CLOSE_STOP_CAP, CLOSE_STOP_NONE = 0, 1, 2   # VISFD_HIP_CLOSE_STOP_*
_CLOSE_NAMES = {"outward": CLOSE_OUTWARD, "inward": CLOSE_INWARD, "auto": CLOSE_AUTO}


def _orientation(o):
    if isinstance(o, str):
        if o not in _CLOSE_NAMES:
            raise ValueError("orientation must be outward, inward or auto")
        return _CLOSE_NAMES[o]
    return int(o)


def _cloud(points, normals):
    """(n, 3) float32 points and normals (x, y, z) as C arrays; None: an empty list"""
    p = np.zeros((0, 3), np.float32) if points is None else np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    m = np.zeros((0, 3), np.float32) if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    if len(p) != len(m):
        raise ValueError("as many normals as points")
    return p, m


def close_surface_splat_host(points, normals, shape, pad=0):
    """Step 1 of close_surface (include/visfd_hip.h) by a serial walk on the host: -> (acc int64 [3, Nz, Ny, Nx] over the
    padded box, used points, skipped points).  No context, no device."""
    L = load_library()
    nz, ny, nx = [int(s) for s in shape]
    p, m = _cloud(points, normals)
    if nz < 3 or ny < 3 or nx < 3 or pad < 0:
        raise VisfdHipError(1, "close_surface: every image dimension must be at least 3 and pad at least 0")
    acc = np.empty((3, nz + 2 * pad, ny + 2 * pad, nx + 2 * pad), np.int64)
    counts = (_i64 * 2)()
    _chk_host(L, L.visfd_hip_close_surface_splat_host(p.ctypes.data if len(p) else None, m.ctypes.data if len(p) else None,
                                                      len(p), nx, ny, nz, int(pad), acc.ctypes.data, counts))
    return acc, int(counts[0]), int(counts[1])


ISO_BELOW, ISO_ABOVE = 0, 1   # VISFD_HIP_ISO_*
_ISO_NAMES = {"below": ISO_BELOW, "above": ISO_ABOVE}


def _iso_side(side):
    if isinstance(side, str):
        if side not in _ISO_NAMES:
            raise ValueError("side must be below or above")
        return _ISO_NAMES[side]
    return int(side)


def _isosurface(call, L, iso, side, alloc, vertices, triangles, count_only=False):
    """One isosurface entry behind call(iso, side, vertices pointer, cap, triangles pointer, cap, nv, nt).  Without arrays:
    the count query, then a call into arrays from alloc(rows, kind) -> (array, pointer), -> (vertices, triangles).  With
    vertices and / or triangles ((array, pointer, rows), or None): one call into them -> (n_vertices, n_triangles); an error
    carries the counts as `counts` when the call got as far as setting them.  count_only: the count query alone."""
    nv, nt = _i64(-1), _i64(-1)
    iso, side = float(iso), _iso_side(side)

    def once(v, t):
        rc = call(iso, side, v[1] if v else None, v[2] if v else 0, t[1] if t else None, t[2] if t else 0, C.byref(nv),
                  C.byref(nt))
        if rc:
            err = VisfdHipError(rc, L.visfd_hip_last_error().decode())
            err.counts = (int(nv.value), int(nt.value)) if nv.value >= 0 else None
            raise err
        return int(nv.value), int(nt.value)

    if count_only or vertices is not None or triangles is not None:
        return once(vertices, triangles)
    n, m = once(None, None)
    v, vp = alloc(n, "vertices")
    t, tp = alloc(m, "triangles")
    once((v, vp, n), (t, tp, m))
    return v, t


def _iso_host_array(a, dtype, what):
    assert isinstance(a, np.ndarray) and a.dtype == dtype and a.flags["C_CONTIGUOUS"] and a.ndim == 2 and a.shape[1] == 3, \
        what + " must be a C-contiguous (n, 3) array of " + np.dtype(dtype).name
    return a, a.ctypes.data, len(a)


def _iso_host_alloc(rows, kind):
    a = np.empty((rows, 3), np.float32 if kind == "vertices" else np.int32)
    return a, a.ctypes.data


def isosurface_host(vol, iso, side="below", vertices=None, triangles=None, count_only=False):
    """The closed triangle mesh of {vol < iso} (side "below") or {vol > iso} ("above") by marching tetrahedra, as
    include/visfd_hip.h defines it to the bit, by a serial walk on the host: no context, no device.  vol float32
    [nz, ny, nx] -> (vertices float32 (n, 3) x y z in voxel coordinates, triangles int32 (m, 3)).  With `vertices` and / or
    `triangles` (arrays to write into): one call -> (n_vertices, n_triangles); an array that is too small stays as it was
    and the call raises VisfdHipError 4, whose `counts` holds the two numbers.  count_only: -> (n_vertices, n_triangles)
    without writing anything."""
    L = load_library()
    vol = np.ascontiguousarray(vol, np.float32)
    nz, ny, nx = vol.shape if vol.ndim == 3 else (0, 0, 0)
    return _isosurface(lambda *tail: L.visfd_hip_isosurface_host(vol.ctypes.data, nx, ny, nz, *tail), L, iso, side,
                       _iso_host_alloc, None if vertices is None else _iso_host_array(vertices, np.float32, "vertices"),
                       None if triangles is None else _iso_host_array(triangles, np.int32, "triangles"), count_only)


def find_spheres_host(crds, sphere_crds, sphere_diameters):
    """FindSpheres (visfd_utils.hpp:271-359) by the host walk: for every point 1 + the index of the LAST sphere that holds
    it, 0 when none does -> int64 array."""
    L = load_library()
    q, c, d = _crds(crds), _crds(sphere_crds), np.ascontiguousarray(sphere_diameters, np.float32)
    assert len(c) == len(d), "sphere lists differ in length"
    ids = np.empty(len(q), np.int64)
    _chk_host(L, L.visfd_hip_find_spheres_host(q.ctypes.data, len(q), c.ctypes.data, d.ctypes.data, len(d), ids.ctypes.data))
    return ids


def choose_threshold_1d(scores, accepted, threshold_is_lower_bound=True):
    """ChooseThreshold1D (visfd_utils.hpp:373-516) -> float."""
    L = load_library()
    s = np.ascontiguousarray(scores, np.float32)
    a = np.ascontiguousarray(accepted, np.bool_).astype(np.uint8)
    assert len(s) == len(a), "scores and labels differ in length"
    thr = C.c_float()
    _chk_host(L, L.visfd_hip_choose_threshold_1d(s.ctypes.data, a.ctypes.data, len(s), int(bool(threshold_is_lower_bound)),
                                                 C.byref(thr)))
    return float(thr.value)


def find_blob_scores(training_crds, crds, diameters, scores, criteria=SORT_DECREASING_MAGNITUDE, ctx=None):
    """_FindBlobScores (feature_implementation.hpp:48-89) -> (scores float32, -inf where no blob holds the point; ids int64:
    1 + the position of that blob in the list sorted by increasing priority, 0 for none)."""
    L = load_library()
    c, d, s = _blob_arrays(crds, diameters, scores)
    t = _crds(training_crds)
    out, ids = np.empty(len(t), np.float32), np.empty(len(t), np.int64)
    _chk_host(L, L.visfd_hip_find_blob_scores(_handle(ctx), t.ctypes.data, len(t), c.ctypes.data, d.ctypes.data, s.ctypes.data,
                                              len(d), int(criteria), out.ctypes.data, ids.ctypes.data))
    return out, ids


def _thresholds_result(lower, upper, report):
    return float(lower.value), float(upper.value), {"false_positives": int(report[0]), "negatives": int(report[1]),
                                                    "false_negatives": int(report[2]), "positives": int(report[3])}


def choose_blob_score_thresholds(crds, diameters, scores, training_pos, training_neg, criteria=SORT_DECREASING_MAGNITUDE,
                                 ctx=None):
    """ChooseBlobScoreThresholds (feature.hpp:988-1035) -> (lower, upper, report dict).  An empty positive or negative set
    after the points outside every blob are dropped raises VisfdHipError with the reference's message."""
    L = load_library()
    c, d, s = _blob_arrays(crds, diameters, scores)
    p, n = _crds(training_pos), _crds(training_neg)
    lower, upper, report = C.c_float(), C.c_float(), np.zeros(4, np.int64)
    _chk_host(L, L.visfd_hip_choose_blob_score_thresholds(_handle(ctx), c.ctypes.data, d.ctypes.data, s.ctypes.data, len(d),
                                                          p.ctypes.data, len(p), n.ctypes.data, len(n), int(criteria),
                                                          C.byref(lower), C.byref(upper), report.ctypes.data))
    return _thresholds_result(lower, upper, report)


def choose_blob_score_thresholds_multi(blob_lists, training_pos, training_neg, criteria=SORT_DECREASING_MAGNITUDE, ctx=None):
    """ChooseBlobScoreThresholdsMulti (feature.hpp:1063-1111).  blob_lists: one (crds, diameters, scores) per set;
    training_pos / training_neg: one coordinate array per set -> (lower, upper, report dict)."""
    L = load_library()
    assert len(blob_lists) == len(training_pos) == len(training_neg), "one blob list and two training files per set"
    lists = [_blob_arrays(*b) for b in blob_lists]
    pos, neg = [_crds(p) for p in training_pos], [_crds(n) for n in training_neg]

    def cat(parts, width):
        return np.ascontiguousarray(np.concatenate([np.zeros((0, width), np.float32)] + [x.reshape(-1, width) for x in parts]))
    c, d, s = cat([b[0] for b in lists], 3), cat([b[1] for b in lists], 1), cat([b[2] for b in lists], 1)
    p, n = cat(pos, 3), cat(neg, 3)
    nb = np.array([len(b[1]) for b in lists], np.int64)
    npos, nneg = np.array([len(x) for x in pos], np.int64), np.array([len(x) for x in neg], np.int64)
    lower, upper, report = C.c_float(), C.c_float(), np.zeros(4, np.int64)
    _chk_host(L, L.visfd_hip_choose_blob_score_thresholds_multi(
        _handle(ctx), len(lists), c.ctypes.data, d.ctypes.data, s.ctypes.data, nb.ctypes.data, p.ctypes.data,
        npos.ctypes.data, n.ctypes.data, nneg.ctypes.data, int(criteria), C.byref(lower), C.byref(upper), report.ctypes.data))
    return _thresholds_result(lower, upper, report)


def discard_blobs_by_score_supervised(crds, diameters, scores, training_pos, training_neg,
                                      criteria=SORT_DECREASING_MAGNITUDE, ctx=None):
    """DiscardBlobsByScoreSupervised (feature.hpp:1124-1180) -> (crds, diameters, scores, lower, upper, report dict): the
    blobs with lower <= score <= upper, in list order."""
    L = load_library()
    c, d, s = _blob_arrays(crds, diameters, scores)
    p, n = _crds(training_pos), _crds(training_neg)
    count = _i64(len(d))
    lower, upper, report = C.c_float(), C.c_float(), np.zeros(4, np.int64)
    _chk_host(L, L.visfd_hip_discard_blobs_by_score_supervised(
        _handle(ctx), c.ctypes.data, d.ctypes.data, s.ctypes.data, C.byref(count), p.ctypes.data, len(p), n.ctypes.data,
        len(n), int(criteria), C.byref(lower), C.byref(upper), report.ctypes.data))
    k = count.value
    return (c[:k], d[:k], s[:k]) + _thresholds_result(lower, upper, report)


_BLOB_DTYPE = np.dtype([("ix", "<i4"), ("iy", "<i4"), ("iz", "<i4"), ("scale", "<i4"), ("sigma", "<f4"),
                        ("score", "<f4")])


def _blobs_to_rows(arr, n):
    """-> float32 rows x,y,z,sigma,score (the reference's list layout) plus the scale indices."""
    rec = np.frombuffer(arr, dtype=_BLOB_DTYPE, count=n)
    rows = np.empty((n, 5), np.float32)
    rows[:, 0] = rec["ix"]
    rows[:, 1] = rec["iy"]
    rows[:, 2] = rec["iz"]
    rows[:, 3] = rec["sigma"]
    rows[:, 4] = rec["score"]
    return rows, rec["scale"].copy()


class Context:
    """One GPU, one HIP stream, one workspace (visfd_hip_ctx)."""

    def __init__(self, device=0, stream=None):
        self._L = load_library()
        h = _vp()
        rc = self._L.visfd_hip_create(int(device), _vp(stream) if stream else None, C.byref(h))
        if rc:
            raise VisfdHipError(rc, self._L.visfd_hip_last_error().decode())
        self._h = h

    def _chk(self, rc):
        if rc:
            raise VisfdHipError(rc, self._L.visfd_hip_last_error().decode())

    def close(self):
        # slab handles hold a pointer to this context: they go first
        for ref in getattr(self, "_slabs", []):
            s = ref()
            if s is not None:
                s.close()
        self._slabs = []
        # blob jobs handed out and not finished: visfd_hip_destroy aborts them, so their handles are dead from here on
        for job in getattr(self, "_jobs", []):
            job[0] = None
        self._jobs = []
        if getattr(self, "_h", None):
            self._L.visfd_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        self._call("synchronize", _HOST)

    def trim(self):
        self._call("trim", _HOST)

    def workspace_bytes(self):
        return int(self._L.visfd_hip_workspace_bytes(self._h))

    def debug_poison_workspace(self):
        """Test aid (visfd_hip_debug_poison_workspace): 0xFF bytes in every workspace slot, in-slot caches forgotten."""
        self._call("debug_poison_workspace", _HOST)

    def blob_jobs_pending(self):
        return int(self._L.visfd_hip_blob_jobs_pending(self._h))

    def _forget_job(self, job):
        self._jobs = [j for j in getattr(self, "_jobs", []) if j is not job]

    def set_option(self, name, value):
        """Tuning / test switch of this context (include/visfd_hip.h: visfd_hip_set_option)."""
        self._call("set_option", _HOST, name.encode(), int(value))

    def get_option(self, name):
        v = C.c_int64()
        self._call("get_option", _HOST, name.encode(), C.byref(v))
        return int(v.value)

    def options(self, **kw):
        """Context manager: set options for the duration of a with-block, then restore the values they had before it
        (whatever their origin: the environment, an earlier set_option, an enclosing scope)."""
        ctx = self

        class _Scope:
            def __enter__(self_):
                self_.saved = {k: ctx.get_option(k) for k in kw}
                for k, v in kw.items():
                    ctx.set_option(k, v)
                return ctx

            def __exit__(self_, *a):
                for k, v in self_.saved.items():
                    ctx.set_option(k, v)
                return False
        return _Scope()

    # ---------------------------------------------------------------- the call both faces go through
    # Every operation below marshals its scalars once, in a private method that takes a face; its public methods are the
    # host face (numpy: allocates or copies the output, shapes the return value) and the device face (`_dev`: the caller's
    # torch tensors, asynchronous on the context's stream).
    def _rc(self, name, face, *args):
        """visfd_hip_<name><suffix>(ctx, *args) -> its return code.  face = (symbol suffix, pointer converter): _HOST,
        _HOST_CTX or _DEVICE.  numpy arrays and torch tensors among the arguments go through the converter (float32,
        contiguous, on the face's side); integers, floats, ctypes objects and None are passed as they are."""
        suffix, ptr = face
        fn = getattr(self._L, "visfd_hip_" + name + suffix)
        return fn(self._h, *[ptr(a) if isinstance(a, np.ndarray) or hasattr(a, "data_ptr") else a for a in args])

    def _call(self, name, face, *args):
        self._chk(self._rc(name, face, *args))

    def _vol(self, name, face, src, dst, mask, *args):
        """_call for the entries that begin (ctx, src, dst, mask, nx, ny, nz, ...)"""
        nz, ny, nx = src.shape
        self._call(name, face, src, dst, mask, nx, ny, nz, *args)

    def _last_path(self, name):
        """visfd_hip_<name>_last_path: which kernel the last call of that family ran (-1 before the first)"""
        p = C.c_int(-1)
        self._call(name + "_last_path", _HOST, C.byref(p))
        return int(p.value)

    def _last_times(self, name, n):
        """visfd_hip_<name>_last_times: the n phase times of the last call, in milliseconds"""
        ms = (C.c_float * n)()
        self._call(name + "_last_times", _HOST, ms)
        return tuple(ms)

    # ---------------------------------------------------------------- filters
    def separable3d(self, src, taps_xyz, mask=None, normalize=True):
        dst = np.empty_like(src)
        A = C.c_float()
        t = [np.ascontiguousarray(x, np.float32) for x in taps_xyz]
        h = [(len(x) - 1) // 2 for x in t]
        self._vol("separable3d", _HOST, src, dst, mask, t[0].ctypes.data_as(_fp), h[0], t[1].ctypes.data_as(_fp), h[1],
                  t[2].ctypes.data_as(_fp), h[2], int(normalize), C.byref(A))
        return dst, A.value

    def _gauss(self, face, src, dst, mask, sigma, hw, normalize):
        A = C.c_float()
        self._vol("apply_gauss", face, src, dst, mask, _f3(sigma), _i3(hw), int(normalize), C.byref(A))
        return A.value

    def gauss_hw(self, src, sigma, hw, mask=None, normalize=True):
        dst = np.empty_like(src)
        return dst, self._gauss(_HOST, src, dst, mask, sigma, hw, normalize)

    def gauss_dev(self, src, dst, sigma, hw, mask=None, normalize=True):
        return self._gauss(_DEVICE, src, dst, mask, sigma, hw, normalize)

    def gauss_ratio(self, src, sigma, ratio, mask=None, normalize=True):
        return self.gauss_hw(src, sigma, gauss_halfwidths(sigma, ratio), mask, normalize)

    def gauss_slab_dev(self, src, dst, z_lo, nz_global, sigma, hw, normalize=True):
        nz, ny, nx = src.shape
        A = C.c_float()
        self._call("apply_gauss_slab", _DEVICE, src, dst, nx, ny, nz, int(z_lo), int(nz_global), _f3(sigma), _i3(hw),
                   int(normalize), C.byref(A))
        return A.value

    def _local_fluctuations(self, name, face, src, dst, mask, sigma, ratio, normalize, exponent):
        self._vol(name, face, src, dst, mask, _f3(sigma), float(exponent), float(ratio), int(normalize))

    def local_fluctuations(self, src, sigma, ratio, mask=None, normalize=True, exponent=2.0):
        """LocalFluctuations (filter3d.hpp:1698-1853), Gaussian weights."""
        dst = np.empty_like(src)
        self._local_fluctuations("local_fluctuations", _HOST, src, dst, mask, sigma, ratio, normalize, exponent)
        return dst

    def local_fluctuations_dev(self, src, dst, sigma, ratio, mask=None, normalize=True, exponent=2.0):
        self._local_fluctuations("local_fluctuations", _DEVICE, src, dst, mask, sigma, ratio, normalize, exponent)

    def local_fluctuations_gen(self, src, sigma, ratio, mask=None, normalize=True, exponent=2.0):
        """LocalFluctuations (filter3d.hpp:1698-1853) for any exponent: the dense generalised-Gaussian window unless the
        exponent is 2, which takes the separable path of local_fluctuations."""
        dst = np.empty_like(src)
        self._local_fluctuations("local_fluctuations_gen", _HOST, src, dst, mask, sigma, ratio, normalize, exponent)
        return dst

    def local_fluctuations_gen_dev(self, src, dst, sigma, ratio, mask=None, normalize=True, exponent=2.0):
        self._local_fluctuations("local_fluctuations_gen", _DEVICE, src, dst, mask, sigma, ratio, normalize, exponent)

    def _filter3d(self, face, src, dst, mask, table, normalize, den):
        t, hw = _filter_table(table)
        self._vol("filter3d", face, src, dst, mask, t.ctypes.data_as(_fp), hw, int(normalize), den)

    def filter3d(self, src, table, mask=None, normalize=False, want_den=False):
        """Filter3D::Apply (filter3d.hpp:81-198) with a table (2hz+1, 2hy+1, 2hx+1) indexed [jz][jy][jx]: -> dst, or
        (dst, den) with want_den (the second Apply overload's denominator).  Voxels with mask == 0 get 0 in both."""
        dst = np.empty_like(src)
        den = np.empty_like(src) if want_den else None
        self._filter3d(_HOST, src, dst, mask, table, normalize, den)
        return (dst, den) if want_den else dst

    def filter3d_dev(self, src, dst, table, mask=None, normalize=False, den=None):
        """filter3d on device tensors (the table is a host array); den: optional tensor for the denominator."""
        self._filter3d(_DEVICE, src, dst, mask, table, normalize, den)

    def filter3d_last_path(self):
        """The kernel the last general-filter call ran: FILTER3D_PATH_GENERAL or FILTER3D_PATH_TILED (-1 before the first)."""
        return self._last_path("filter3d")

    def _apply_ggauss(self, face, src, dst, mask, width, m_exp, halfwidth, normalize):
        A = C.c_float()
        self._vol("apply_ggauss", face, src, dst, mask, _f3(width), float(m_exp), _i3(halfwidth), int(normalize), C.byref(A))
        return A.value

    def apply_ggauss(self, src, width, m_exp, halfwidth, mask=None, normalize=True):
        """HandleGGauss (handlers.cpp:167-187): GenFilterGenGauss3D(width, m_exp, halfwidth) applied -> (dst, A)."""
        dst = np.empty_like(src)
        return dst, self._apply_ggauss(_HOST, src, dst, mask, width, m_exp, halfwidth, normalize)

    def apply_ggauss_dev(self, src, dst, width, m_exp, halfwidth, mask=None, normalize=True):
        return self._apply_ggauss(_DEVICE, src, dst, mask, width, m_exp, halfwidth, normalize)

    def _apply_dogg(self, face, src, dst, mask, width_a, width_b, m_exp, n_exp, truncate_ratio, truncate_threshold):
        A, B = C.c_float(), C.c_float()
        self._vol("apply_dogg", face, src, dst, mask, _f3(width_a), _f3(width_b), float(m_exp), float(n_exp),
                  float(truncate_ratio), float(truncate_threshold), C.byref(A), C.byref(B))
        return A.value, B.value

    def apply_dogg(self, src, width_a, width_b, m_exp, n_exp, truncate_ratio=-1.0, truncate_threshold=0.03, mask=None):
        """HandleDogg (handlers.cpp:265-293): GenFilterDogg3D applied, never normalised -> (dst, A, B)."""
        dst = np.empty_like(src)
        return (dst,) + self._apply_dogg(_HOST, src, dst, mask, width_a, width_b, m_exp, n_exp, truncate_ratio,
                                         truncate_threshold)

    def apply_dogg_dev(self, src, dst, width_a, width_b, m_exp, n_exp, truncate_ratio=-1.0, truncate_threshold=0.03,
                       mask=None):
        return self._apply_dogg(_DEVICE, src, dst, mask, width_a, width_b, m_exp, n_exp, truncate_ratio, truncate_threshold)

    def dog(self, src, sigma_a, sigma_b, hw, mask=None):
        dst = np.empty_like(src)
        A, B = C.c_float(), C.c_float()
        self._vol("apply_dog", _HOST, src, dst, mask, _f3(sigma_a), _f3(sigma_b), _i3(hw), C.byref(A), C.byref(B))
        return dst, A.value, B.value

    def _log(self, face, src, dst, mask, sigma, delta, ratio, A, B):
        self._vol("apply_log", face, src, dst, mask, _f3(sigma), float(delta), float(ratio), A, B)

    def log(self, src, sigma, delta, ratio, mask=None):
        dst = np.empty_like(src)
        A, B = C.c_float(), C.c_float()
        self._log(_HOST, src, dst, mask, sigma, delta, ratio, C.byref(A), C.byref(B))
        return dst, A.value, B.value

    def log_dev(self, src, dst, sigma, delta, ratio, mask=None):
        """ApplyLog on device tensors; dst may be src.  Unmasked scales with one half-width 6..10 run both Gaussians in two
        shared launches (csrc/gauss_pair.hip); options log_pair (0 never, 1 by its table, 2 wherever it applies) and
        log_pair_chunk (march length, for tests).  The bits are the same on every route."""
        self._log(_DEVICE, src, dst, mask, sigma, delta, ratio, None, None)

    # ---------------------------------------------------------------- drawing, meshes, point clouds
    def _draw_spheres(self, face, dst, mask, background, centers, diameters, shell_thicknesses, foreground, background_offset,
                      background_rescale, background_normalize, foreground_normalize):
        nz, ny, nx = background.shape
        n, p, keep = _sphere_lists(centers, diameters, shell_thicknesses, foreground)
        outside = C.c_int()
        self._call("draw_spheres", face, dst, mask, background, nx, ny, nz, p[0], p[1], p[2], p[3], n, float(background_offset),
                   float(background_rescale), int(background_normalize), int(foreground_normalize), C.byref(outside))
        return bool(outside.value)

    def draw_spheres(self, background, centers, diameters=None, shell_thicknesses=None, foreground=None, mask=None,
                     background_offset=0.0, background_rescale=1.0, background_normalize=False,
                     foreground_normalize=False, want_outside=False):
        """DrawSpheres (draw.hpp:238-457): spheres or shells at centers (n, 3) in voxels (x, y, z) over the rescaled
        background; later spheres overwrite earlier ones.  None lists take the reference's defaults (diameter 0, solid,
        foreground 1).  -> dst, or (dst, any_center_outside) with want_outside."""
        dst = np.empty_like(background)
        outside = self._draw_spheres(_HOST, dst, mask, background, centers, diameters, shell_thicknesses, foreground,
                                     background_offset, background_rescale, background_normalize, foreground_normalize)
        return (dst, outside) if want_outside else dst

    def draw_spheres_dev(self, dst, background, centers, diameters=None, shell_thicknesses=None, foreground=None, mask=None,
                         background_offset=0.0, background_rescale=1.0, background_normalize=False,
                         foreground_normalize=False):
        """draw_spheres on device tensors (the lists are host arrays); dst may be background.  -> any_center_outside"""
        return self._draw_spheres(_DEVICE, dst, mask, background, centers, diameters, shell_thicknesses, foreground,
                                  background_offset, background_rescale, background_normalize, foreground_normalize)

    def _draw_regions(self, face, dst, mask, regions, negative_means_subtract):
        nz, ny, nx = dst.shape
        arr, n = _regions(regions)
        self._call("draw_regions", face, dst, mask, nx, ny, nz, arr, n, int(negative_means_subtract))

    def draw_regions(self, image, regions, mask=None, negative_means_subtract=False):
        """DrawRegions (draw.hpp:90-224) on a copy of `image`: regions is a list of (REGION_RECT, (xmin, xmax, ymin, ymax,
        zmin, zmax), value) and (REGION_SPHERE, (x0, y0, z0, r), value), acting in list order -> the new image."""
        dst = np.array(image, np.float32, copy=True, order="C")
        self._draw_regions(_HOST, dst, mask, regions, negative_means_subtract)
        return dst

    def draw_regions_dev(self, dst, regions, mask=None, negative_means_subtract=False):
        """draw_regions on a device tensor, in place (the region list is a host array)."""
        self._draw_regions(_DEVICE, dst, mask, regions, negative_means_subtract)

    def draw_last_times(self):
        """(zero fill, scatter, resolve) milliseconds of the last draw_spheres under the option draw_time."""
        return self._last_times("draw", 3)

    def _voxelize_mesh(self, face, dst, vertices, triangles, voxel_width, origin, check_closed):
        nz, ny, nx = dst.shape
        v, t = _mesh(vertices, triangles)
        self._call("voxelize_mesh", face, v.ctypes.data, len(v), t.ctypes.data, len(t), float(voxel_width), _d3(origin),
                   nx, ny, nz, int(bool(check_closed)), dst)

    def voxelize_mesh(self, vertices, triangles, shape, voxel_width=1.0, origin=(0, 0, 0), check_closed=True):
        """Which samples of an image of `shape` (nz, ny, nx) lie inside the closed triangle mesh (the job of the reference's
        voxelize_mesh.py, by the exact rule of include/visfd_hip.h): vertices (n, 3) float32 (x, y, z) in physical units,
        triangles (m, 3) int32, origin = the position of voxel 0 in voxels.  -> float32 [nz, ny, nx] of 0 and 1."""
        dst = np.empty(tuple(int(s) for s in shape), np.float32)
        self._voxelize_mesh(_HOST, dst, vertices, triangles, voxel_width, origin, check_closed)
        return dst

    def voxelize_mesh_dev(self, dst, vertices, triangles, voxel_width=1.0, origin=(0, 0, 0), check_closed=True):
        """voxelize_mesh into a device tensor [nz, ny, nx] (the mesh lists are host arrays); returns with the stream idle."""
        self._voxelize_mesh(_DEVICE, dst, vertices, triangles, voxel_width, origin, check_closed)

    def voxelize_last(self):
        """(crossings, skipped triangles, odd rows, inside voxels) of the last voxelize_mesh[_dev]."""
        s = (_i64 * 4)()
        self._call("voxelize_last", _HOST, s)
        return tuple(int(x) for x in s)

    def voxelize_last_times(self):
        """(zero fill, scatter, fill) milliseconds of the last voxelize_mesh[_dev] under the option voxelize_time."""
        return self._last_times("voxelize", 3)

    def _close_surface(self, face, points, normals, n, shape, pad, orientation, mask, chi):
        nz, ny, nx = shape
        self._call("close_surface", face, points if n else None, normals if n else None, n, nx, ny, nz, int(pad),
                   _orientation(orientation), mask, chi)

    def close_surface(self, points, normals, shape, pad=0, orientation="outward", want_chi=False):
        """An oriented point cloud closed into a mask (include/visfd_hip.h): points and normals (n, 3) float32
        (x, y, z) in voxel coordinates, shape (nz, ny, nx), orientation "outward", "inward" or "auto".
        -> float32 [nz, ny, nx] of 0 and 1, or (mask, chi) with want_chi."""
        shape = tuple(int(s) for s in shape)
        p, m = _cloud(points, normals)
        mask = np.empty(shape, np.float32)
        chi = np.empty(shape, np.float32) if want_chi else None
        self._close_surface(_HOST, p, m, len(p), shape, pad, orientation, mask, chi)
        return (mask, chi) if want_chi else mask

    def close_surface_dev(self, mask, points, normals, pad=0, orientation="outward", chi=None):
        """close_surface on device tensors: mask (and chi, optional) [nz, ny, nx], points and normals (n, 3) float32; returns
        with the stream idle."""
        n = int(points.shape[0])
        assert tuple(points.shape) == (n, 3) and tuple(normals.shape) == (n, 3), "points and normals are (n, 3)"
        self._close_surface(_DEVICE, points, normals, n, mask.shape, pad, orientation, mask, chi)

    def _close_surface_splat(self, face, points, normals, n, shape, pad, acc):
        nz, ny, nx = shape
        counts = (_i64 * 2)()
        self._call("close_surface_splat", face, points if n else None, normals if n else None, n, nx, ny, nz, int(pad), acc,
                   counts)
        return int(counts[0]), int(counts[1])

    def close_surface_splat(self, points, normals, shape, pad=0):
        """Step 1 of close_surface on the device -> (acc int64 [3, Nz, Ny, Nx], used points, skipped points)."""
        nz, ny, nx = [int(s) for s in shape]
        p, m = _cloud(points, normals)
        acc = np.empty((3, max(nz + 2 * pad, 0), max(ny + 2 * pad, 0), max(nx + 2 * pad, 0)), np.int64)
        return (acc,) + self._close_surface_splat(_HOST, p, m, len(p), (nz, ny, nx), pad, acc.ctypes.data)

    def close_surface_splat_dev(self, acc, points, normals, shape, pad=0):
        """close_surface_splat on device tensors: acc int64 [3, Nz, Ny, Nx] -> (used points, skipped points)."""
        nz, ny, nx = [int(s) for s in shape]
        n = int(points.shape[0])
        assert acc.is_cuda and acc.is_contiguous() and str(acc.dtype) == "torch.int64", "need contiguous cuda int64"
        assert tuple(acc.shape) == (3, nz + 2 * pad, ny + 2 * pad, nx + 2 * pad), "acc is [3, Nz, Ny, Nx]"
        return self._close_surface_splat(_DEVICE, points, normals, n, (nz, ny, nx), pad, acc.data_ptr())

    def close_surface_last(self):
        """The last close_surface[_dev]: dict with n_used, n_skipped, cycles, stop (CLOSE_STOP_*), orientation
        ("outward" or "inward"), touches_face, ratio (the final residual ratio) and iso."""
        s, v = (_i64 * 6)(), (C.c_double * 2)()
        self._call("close_surface_last", _HOST, s, v)
        return {"n_used": int(s[0]), "n_skipped": int(s[1]), "cycles": int(s[2]), "stop": int(s[3]),
                "orientation": "inward" if s[4] == CLOSE_INWARD else "outward", "touches_face": int(s[5]),
                "ratio": float(v[0]), "iso": float(v[1])}

    def close_surface_last_times(self):
        """(splat and right-hand side, solve, level and cut) milliseconds of the last close_surface[_dev] under the option
        close_surface_time."""
        return self._last_times("close_surface", 3)

    def _isosurface(self, face, vol, shape, *rest):
        nz, ny, nx = shape
        return _isosurface(lambda *tail: self._rc("isosurface", face, vol, nx, ny, nz, *tail), self._L, *rest)

    def isosurface(self, vol, iso, side="below", vertices=None, triangles=None, count_only=False):
        """isosurface_host's mesh, bit for bit, by the kernels of csrc/isosurface.hip: vol float32 [nz, ny, nx] on the host
        -> (vertices float32 (n, 3), triangles int32 (m, 3)); with arrays to write into -> (n_vertices, n_triangles), as
        isosurface_host."""
        vol = np.ascontiguousarray(vol, np.float32)
        return self._isosurface(_HOST, vol, vol.shape if vol.ndim == 3 else (0, 0, 0), iso, side, _iso_host_alloc,
                                None if vertices is None else _iso_host_array(vertices, np.float32, "vertices"),
                                None if triangles is None else _iso_host_array(triangles, np.int32, "triangles"), count_only)

    def isosurface_dev(self, vol, iso, side="below", vertices=None, triangles=None, count_only=False):
        """isosurface on device tensors: vol float32 [nz, ny, nx] -> (vertices float32 (n, 3), triangles int32 (m, 3)) as new
        tensors on vol's device; with tensors to write into -> (n_vertices, n_triangles), as isosurface_host.  Returns with
        the stream idle."""
        import torch

        def given(t, dtype, what):
            assert t.is_cuda and t.is_contiguous() and t.dtype == dtype and t.dim() == 2 and t.shape[1] == 3, \
                what + " must be a contiguous cuda (n, 3) tensor of " + str(dtype)
            return t, t.data_ptr(), int(t.shape[0])

        def alloc(rows, kind):
            t = torch.empty((rows, 3), dtype=torch.float32 if kind == "vertices" else torch.int32, device=vol.device)
            return t, t.data_ptr()

        return self._isosurface(_DEVICE, vol, vol.shape, iso, side, alloc,
                                None if vertices is None else given(vertices, torch.float32, "vertices"),
                                None if triangles is None else given(triangles, torch.int32, "triangles"), count_only)

    def isosurface_last(self):
        """The last isosurface[_dev]: dict with n_vertices, n_triangles, n_inside (inside nodes) and capped (1 when the
        image border cut the solid and the border layer closed it there)."""
        s = (_i64 * 4)()
        self._call("isosurface_last", _HOST, s)
        return {"n_vertices": int(s[0]), "n_triangles": int(s[1]), "n_inside": int(s[2]), "capped": int(s[3])}

    def isosurface_last_times(self):
        """(classify, scan and the host's read of the totals, vertices, triangles) milliseconds of the last isosurface[_dev]
        under the option isosurface_time; -1 for a phase that did not run."""
        return self._last_times("isosurface", 4)

    # ---------------------------------------------------------------- morphology and medians
    def _morph_sphere(self, face, op, src, dst, mask, radius, radius_max, bmax):
        self._vol("morph_sphere", face, src, dst, mask, int(op), float(radius), float(radius_max), float(bmax))

    def morph_sphere(self, op, src, radius, radius_max=0.0, bmax=0.0, mask=None, dst=None):
        """DilateSphere / ErodeSphere / OpenSphere / CloseSphere / WhiteTopHatSphere / BlackTopHatSphere (op = MORPH_*,
        morphology.hpp:241-597).  dst (default: a copy of src, as filter_mrc starts its output) keeps its values where
        mask == 0 and is what the top-hats subtract from / are subtracted from; a new array is returned."""
        dst = np.array(src if dst is None else dst, np.float32, copy=True, order="C")
        self._morph_sphere(_HOST, op, src, dst, mask, radius, radius_max, bmax)
        return dst

    def morph_sphere_dev(self, op, src, dst, radius, radius_max=0.0, bmax=0.0, mask=None):
        """morph_sphere on device tensors; dst is read (top-hats, masked voxels) and written in place."""
        self._morph_sphere(_DEVICE, op, src, dst, mask, radius, radius_max, bmax)

    def dilate_sphere(self, src, radius, radius_max=0.0, bmax=0.0, mask=None, dst=None):
        return self.morph_sphere(MORPH_DILATE, src, radius, radius_max, bmax, mask, dst)

    def erode_sphere(self, src, radius, radius_max=0.0, bmax=0.0, mask=None, dst=None):
        return self.morph_sphere(MORPH_ERODE, src, radius, radius_max, bmax, mask, dst)

    def open_sphere(self, src, radius, radius_max=0.0, bmax=0.0, mask=None, dst=None):
        return self.morph_sphere(MORPH_OPEN, src, radius, radius_max, bmax, mask, dst)

    def close_sphere(self, src, radius, radius_max=0.0, bmax=0.0, mask=None, dst=None):
        return self.morph_sphere(MORPH_CLOSE, src, radius, radius_max, bmax, mask, dst)

    def white_top_hat_sphere(self, src, radius, radius_max=0.0, bmax=0.0, mask=None, dst=None):
        return self.morph_sphere(MORPH_TOP_HAT_WHITE, src, radius, radius_max, bmax, mask, dst)

    def black_top_hat_sphere(self, src, radius, radius_max=0.0, bmax=0.0, mask=None, dst=None):
        return self.morph_sphere(MORPH_TOP_HAT_BLACK, src, radius, radius_max, bmax, mask, dst)

    def dilate_sphere_dev(self, src, dst, radius, radius_max=0.0, bmax=0.0, mask=None):
        self.morph_sphere_dev(MORPH_DILATE, src, dst, radius, radius_max, bmax, mask)

    def erode_sphere_dev(self, src, dst, radius, radius_max=0.0, bmax=0.0, mask=None):
        self.morph_sphere_dev(MORPH_ERODE, src, dst, radius, radius_max, bmax, mask)

    def open_sphere_dev(self, src, dst, radius, radius_max=0.0, bmax=0.0, mask=None):
        self.morph_sphere_dev(MORPH_OPEN, src, dst, radius, radius_max, bmax, mask)

    def close_sphere_dev(self, src, dst, radius, radius_max=0.0, bmax=0.0, mask=None):
        self.morph_sphere_dev(MORPH_CLOSE, src, dst, radius, radius_max, bmax, mask)

    def white_top_hat_sphere_dev(self, src, dst, radius, radius_max=0.0, bmax=0.0, mask=None):
        self.morph_sphere_dev(MORPH_TOP_HAT_WHITE, src, dst, radius, radius_max, bmax, mask)

    def black_top_hat_sphere_dev(self, src, dst, radius, radius_max=0.0, bmax=0.0, mask=None):
        self.morph_sphere_dev(MORPH_TOP_HAT_BLACK, src, dst, radius, radius_max, bmax, mask)

    def _morph_table_op(self, face, op, src, dst, mask, dxyz, b):
        d, bb = _morph_table(dxyz, b)
        self._vol("morph_table", face, src, dst, mask, int(op), d.ctypes.data_as(_ip), bb.ctypes.data_as(_fp), len(bb))

    def morph_table(self, op, src, dxyz, b, mask=None, dst=None):
        """Dilate / Erode (op MORPH_DILATE or MORPH_ERODE, morphology.hpp:134-229) with an arbitrary element: dxyz (n, 3)
        offsets and b (n,), walked in the given order."""
        dst = np.array(src if dst is None else dst, np.float32, copy=True, order="C")
        self._morph_table_op(_HOST, op, src, dst, mask, dxyz, b)
        return dst

    def morph_table_dev(self, op, src, dst, dxyz, b, mask=None):
        self._morph_table_op(_DEVICE, op, src, dst, mask, dxyz, b)

    def dilate(self, src, dxyz, b, mask=None, dst=None):
        return self.morph_table(MORPH_DILATE, src, dxyz, b, mask, dst)

    def erode(self, src, dxyz, b, mask=None, dst=None):
        return self.morph_table(MORPH_ERODE, src, dxyz, b, mask, dst)

    def dilate_dev(self, src, dst, dxyz, b, mask=None):
        self.morph_table_dev(MORPH_DILATE, src, dst, dxyz, b, mask)

    def erode_dev(self, src, dst, dxyz, b, mask=None):
        self.morph_table_dev(MORPH_ERODE, src, dst, dxyz, b, mask)

    def morph_last_path(self):
        """What the last morphology call ran: MORPH_PATH_GENERAL, MORPH_PATH_XRUNS or MORPH_PATH_LEVELS (the distance-map path
        of two-level images, option morph_levels); -1 before the first."""
        return self._last_path("morph")

    def _median_sphere(self, face, src, dst, mask, radius):
        self._vol("median_sphere", face, src, dst, mask, float(radius))

    def median_sphere(self, src, radius, mask=None, dst=None):
        """MedianSphere (filter3d.hpp:1639-1674, semantics in include/visfd_hip.h): the value of rank n // 2 among the n
        neighbours within `radius` voxels that lie in the image and have mask != 0.  dst (default: a copy of src, as
        filter_mrc starts its output) keeps its values where mask == 0; a new array is returned."""
        dst = np.array(src if dst is None else dst, np.float32, copy=True, order="C")
        self._median_sphere(_HOST, src, dst, mask, radius)
        return dst

    def median_sphere_dev(self, src, dst, radius, mask=None):
        """median_sphere on device tensors; dst keeps its values where mask == 0 and is written in place."""
        self._median_sphere(_DEVICE, src, dst, mask, radius)

    def _median_table(self, face, src, dst, mask, dxyz):
        d = np.ascontiguousarray(dxyz, np.int32).reshape(-1, 3)
        self._vol("median_table", face, src, dst, mask, d.ctypes.data_as(_ip), len(d))

    def median_table(self, src, dxyz, mask=None, dst=None):
        """Median (filter3d.hpp:1577-1630) with an arbitrary footprint: dxyz (n, 3) offsets; duplicates count as often as
        they appear and the centre need not be among them."""
        dst = np.array(src if dst is None else dst, np.float32, copy=True, order="C")
        self._median_table(_HOST, src, dst, mask, dxyz)
        return dst

    def median_table_dev(self, src, dst, dxyz, mask=None):
        self._median_table(_DEVICE, src, dst, mask, dxyz)

    def median_last_path(self):
        """The kernel the last median call ran: MEDIAN_PATH_GENERAL or MEDIAN_PATH_TILED (-1 before the first)."""
        return self._last_path("median")

    # ---------------------------------------------------------------- distances, statistics, intensity maps
    # (one method for both faces: numpy arrays in, numpy out; torch device tensors in, tensors out)
    def distance_sq(self, shape=None, points=None, src=None, mask=None, lo=-np.inf, hi=np.inf):
        """The exact squared distance map (include/visfd_hip.h): int32 min((nx + ny + nz)^2, |v - s|^2 over the seeds s).
        Seeds: the voxels of `src` with mask != 0 and lo <= src <= hi (src None: none) and the integer `points` ((n, 3)
        rows x, y, z; anywhere).  shape = (nz, ny, nx) when there is no src.  numpy arrays -> numpy; torch device
        tensors -> a torch int32 tensor."""
        nz, ny, nx = src.shape if src is not None else shape
        pts = _points(points)
        if src is None or isinstance(src, np.ndarray):
            face, dsq = _HOST, np.empty((nz, ny, nx), np.int32)
        else:
            import torch
            face, dsq = _DEVICE, torch.empty((nz, ny, nx), dtype=torch.int32, device=src.device)
        self._call("distance_sq", face, src, mask, nx, ny, nz, float(lo), float(hi), pts.ctypes.data, len(pts), _address(dsq))
        return dsq

    def distance_to_points(self, dst, points, voxel_width=1.0, mask=None):
        """-distance-points: sqrtf((float)dsq * (w * w)) of the distance to the nearest of `points` where mask != 0; `dst`
        (3-D float32) keeps its values where mask == 0.  numpy: a new array is returned; torch device tensors: dst is
        written in place and returned."""
        nz, ny, nx = dst.shape
        pts = _points(points)
        if isinstance(dst, np.ndarray):
            dst = np.array(dst, np.float32, copy=True, order="C")
        self._call("distance_to_points", _face_of(dst), dst, mask, nx, ny, nz, pts.ctypes.data, len(pts), float(voxel_width))
        return dst

    def distance_from_points(self, src, points, lo, hi, voxel_width=1.0, mask=None):
        """-distance-to-voxels: for every point the float distance to the nearest voxel with mask != 0 and lo <= src <= hi
        (the distance of (nx + ny + nz)^2 when there is none) -> float32 numpy array, one per point."""
        nz, ny, nx = src.shape
        pts = _points(points)
        out = np.empty(len(pts), np.float32)
        self._call("distance_from_points", _face_of(src), src, mask, nx, ny, nz, float(lo), float(hi), pts.ctypes.data,
                   len(pts), float(voxel_width), out.ctypes.data)
        return out

    def distance_last_path(self):
        """What the last distance call ran: DISTANCE_PATH_GENERAL or DISTANCE_PATH_TRANSFORM (-1 before the first)."""
        return self._last_path("distance")

    def image_stats(self, src, mask=None):
        """Statistics of the voxels with mask != 0 (all without a mask): dict of count, n_nonfinite, min, max, the exact
        sum rounded once to double (math.fsum's) and order_free (include/visfd_hip.h).  numpy arrays or torch device
        tensors of any shape; returns with the stream idle."""
        st = Stats()
        self._call("image_stats", _face_of(src), src, mask, src.size if isinstance(src, np.ndarray) else src.numel(),
                   C.byref(st))
        return st.as_dict()

    def intensity_map(self, p, out, src=None, mask=None, want_stats=False):
        """One pass of the stages of `p` (api.intensity(...)) over `out`, IN PLACE: invert, one map (the threshold family
        reads `src`, which may be `out` itself), mask fill, Rescale01.  3-D numpy arrays or torch device tensors.
        want_stats: -> the statistics of what was written (the call then waits for the stream), else None."""
        nz, ny, nx = out.shape
        st = Stats()
        self._call("intensity_map", _face_of(out), src, out, mask, nx, ny, nz, C.byref(p), C.byref(st) if want_stats else None)
        return st.as_dict() if want_stats else None

    # ---------------------------------------------------------------- blob lists
    def _find_spheres(self, face, crds, sphere_crds, sphere_diameters, ids):
        self._call("find_spheres", face, crds, int(crds.shape[0]), sphere_crds, sphere_diameters,
                   int(sphere_diameters.shape[0]), _address(ids))

    def find_spheres(self, crds, sphere_crds, sphere_diameters, ids=None):
        """FindSpheres (visfd_utils.hpp:271-359) on the device, numpy in and out: for every point 1 + the index of the LAST
        sphere that holds it, 0 when none does -> int64 array (`ids` itself when one is passed).  Option
        find_spheres_host: the host walk instead."""
        q, c, d = _crds(crds), _crds(sphere_crds), np.ascontiguousarray(sphere_diameters, np.float32)
        assert len(c) == len(d), "sphere lists differ in length"
        if ids is None:
            ids = np.empty(len(q), np.int64)
        assert isinstance(ids, np.ndarray) and ids.dtype == np.int64 and ids.flags["C_CONTIGUOUS"] and ids.size == len(q)
        self._find_spheres(_HOST, q, c, d, ids)
        return ids

    def find_spheres_dev(self, crds, sphere_crds, sphere_diameters, ids=None):
        """The same on torch device tensors: crds (n, 3), sphere_crds (m, 3), sphere_diameters (m,) float32 -> ids, an
        int64 device tensor of n entries (written in place when passed).  The search is asynchronous on the context's
        stream; the values are checked by the preparation launches, whose flag word the call waits for."""
        import torch
        n, m = int(crds.shape[0]), int(sphere_diameters.shape[0])
        assert int(sphere_crds.shape[0]) == m, "sphere lists differ in length"
        if ids is None:
            ids = torch.empty(n, dtype=torch.int64, device=crds.device)
        assert ids.is_cuda and ids.is_contiguous() and ids.dtype == torch.int64 and ids.numel() == n, "ids: n int64 on the device"
        self._find_spheres(_DEVICE, crds, sphere_crds, sphere_diameters, ids)
        return ids

    def find_spheres_last_path(self):
        """What the last FindSpheres call ran: FIND_SPHERES_PATH_DEVICE or FIND_SPHERES_PATH_HOST (-1 before the first)."""
        return self._last_path("find_spheres")

    def _discard_overlapping_blobs(self, face, crds, diameters, scores, n, min_radial_separation_ratio, max_volume_overlap_large,
                                   max_volume_overlap_small, criteria, scale):
        k = _i64(n)
        self._call("discard_overlapping_blobs", face, crds, diameters, scores, C.byref(k), min_radial_separation_ratio,
                   max_volume_overlap_large, max_volume_overlap_small, int(criteria), int(scale))
        return int(k.value)

    def discard_overlapping_blobs(self, crds, diameters, scores, min_radial_separation_ratio, max_volume_overlap_large=np.inf,
                                  max_volume_overlap_small=np.inf, criteria=SORT_DECREASING_MAGNITUDE, scale=6):
        """DiscardOverlappingBlobs (feature.hpp:720-913) on the device, numpy in and out -> (crds, diameters, scores) of
        the kept blobs, best first: the bits of the module-level function.  discard_overlapping_blobs_last() says what ran."""
        c, d, s = _blob_arrays(crds, diameters, scores)
        k = self._discard_overlapping_blobs(_HOST_CTX, c, d, s, len(d), min_radial_separation_ratio, max_volume_overlap_large,
                                            max_volume_overlap_small, criteria, scale)
        return c[:k], d[:k], s[:k]

    def discard_overlapping_blobs_dev(self, crds, diameters, scores, min_radial_separation_ratio,
                                      max_volume_overlap_large=np.inf, max_volume_overlap_small=np.inf,
                                      criteria=SORT_DECREASING_MAGNITUDE, scale=6):
        """The same on torch device tensors, IN PLACE: crds (n, 3), diameters (n,), scores (n,) float32, contiguous.
        Returns the number of kept blobs; they are the first entries of the three tensors.  Returns with the stream idle."""
        import torch
        n = int(diameters.shape[0])
        for t, m in ((crds, 3 * n), (diameters, n), (scores, n)):
            assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and t.numel() == m, "float32 device lists of one length"
        return self._discard_overlapping_blobs(_DEVICE, crds, diameters, scores, n, min_radial_separation_ratio,
                                               max_volume_overlap_large, max_volume_overlap_small, criteria, scale)

    def discard_overlapping_blobs_last(self):
        """The last discard_overlapping_blobs[_dev] of this context: dict of path (DISCARD_OVERLAP_PATH_*), reason
        (DISCARD_OVERLAP_REASON_*), rounds, blobs_in, blobs_kept, pairs_crit, pairs_share, table_cells."""
        info = (_i64 * 8)()
        self._call("discard_overlapping_blobs_last", _HOST, info)
        return dict(zip(DISCARD_OVERLAP_LAST_FIELDS, (int(x) for x in info)))

    def discard_overlapping_blobs_last_times(self):
        """Option discard_overlap_time: the last call's phases in milliseconds (reduction, ranking and records, buckets,
        rounds, compaction), -1 where a phase did not run."""
        return dict(zip(("reduce", "rank", "buckets", "rounds", "compact"),
                        (float(x) for x in self._last_times("discard_overlapping_blobs", 5))))

    def _blob_call(self, face, src, mask, shape, sigmas, aspect, delta, ratio, minima_threshold, maxima_threshold,
                   use_ratios, cap):
        nz, ny, nx = shape
        sig = np.ascontiguousarray(sigmas, np.float32)
        asp = _f3(aspect) if aspect is not None else None
        for attempt in (0, 1):
            # the record arrays are kept by the context between calls (a pipeline asks for millions of records of capacity:
            # mapping and unmapping 2 x 100 MB per call cost 1-25 ms of host time, depending on the state of the machine)
            bufs = getattr(self, "_blob_bufs", None)
            if bufs is None or len(bufs[0]) < cap:
                bufs = self._blob_bufs = (np.empty(cap, _BLOB_DTYPE), np.empty(cap, _BLOB_DTYPE))   # visfd_hip_blob records
            amin, amax = bufs   # (at least `cap` records; the call is still told `cap`)
            nmin, nmax = _i64(), _i64()
            rc = self._rc("blob_dog", face, src, mask, nx, ny, nz, sig.ctypes.data_as(_fp), len(sig), asp, float(delta),
                          float(ratio), float(minima_threshold), float(maxima_threshold), int(use_ratios),
                          amin.ctypes.data, cap, C.byref(nmin), amax.ctypes.data, cap, C.byref(nmax))
            if rc == 4 and attempt == 0:   # VISFD_HIP_ECAPACITY: the exact counts came back; once more with room for them
                cap = max(nmin.value, nmax.value, 1)
                continue
            self._chk(rc)
            break
        return _blobs_to_rows(amin, nmin.value)[0], _blobs_to_rows(amax, nmax.value)[0]

    def blob_dog(self, src, sigmas, mask=None, aspect=None, delta=0.02, ratio=2.5, minima_threshold=np.inf,
                 maxima_threshold=-np.inf, use_ratios=False, cap=1 << 16):
        return self._blob_call(_HOST, src, mask, src.shape, sigmas, aspect, delta, ratio, minima_threshold,
                               maxima_threshold, use_ratios, cap)

    def blob_dog_dev(self, src, sigmas, mask=None, aspect=None, delta=0.02, ratio=2.5, minima_threshold=np.inf,
                     maxima_threshold=-np.inf, use_ratios=False, cap=1 << 16):
        return self._blob_call(_DEVICE, src, mask, tuple(src.shape), sigmas, aspect, delta, ratio, minima_threshold,
                               maxima_threshold, use_ratios, cap)

    def blob_dog_begin_dev(self, src, sigmas, mask=None, aspect=None, delta=0.02, ratio=2.5, minima_threshold=np.inf,
                           maxima_threshold=-np.inf, use_ratios=False):
        """First half of blob_dog_dev (visfd_hip_blob_dog_begin_dev): everything queued, most lists fetched; returns a job for
        blob_dog_end().  Other calls of this context may be queued in between; src and mask must stay as they are until then."""
        nz, ny, nx = src.shape
        sig = np.ascontiguousarray(sigmas, np.float32)
        asp = _f3(aspect) if aspect is not None else None
        job = _vp()
        self._call("blob_dog_begin", _DEVICE, src, mask, nx, ny, nz, sig.ctypes.data_as(_fp), len(sig), asp, float(delta),
                   float(ratio), float(minima_threshold), float(maxima_threshold), int(use_ratios), C.byref(job))
        job = [job, src, mask, sig]   # (the tensors and the sigma array live as long as the job)
        self._jobs = getattr(self, "_jobs", []) + [job]   # close() ends what the caller has not
        return job

    def blob_dog_end(self, job, cap=1 << 16):
        """Second half: -> (minima, maxima) rows x,y,z,sigma,score, as blob_dog_dev returns them."""
        h = job[0]
        if h is None:
            raise ValueError("blob job already finished")
        for attempt in (0, 1):
            bufs = getattr(self, "_blob_bufs", None)
            if bufs is None or len(bufs[0]) < cap:
                bufs = self._blob_bufs = (np.empty(cap, _BLOB_DTYPE), np.empty(cap, _BLOB_DTYPE))
            amin, amax = bufs
            nmin, nmax = _i64(), _i64()
            rc = self._L.visfd_hip_blob_dog_end(h, amin.ctypes.data, cap, C.byref(nmin), amax.ctypes.data, cap, C.byref(nmax))
            if rc == 4 and attempt == 0:   # VISFD_HIP_ECAPACITY: the job is still alive, the counts came back
                cap = max(nmin.value, nmax.value, 1)
                continue
            job[0] = None                   # every other outcome has freed the job
            self._forget_job(job)
            if rc == 4:
                self._L.visfd_hip_blob_dog_abort(h)
            self._chk(rc)
            break
        return _blobs_to_rows(amin, nmin.value)[0], _blobs_to_rows(amax, nmax.value)[0]

    def blob_dog_abort(self, job):
        if job[0] is not None:
            self._L.visfd_hip_blob_dog_abort(job[0])
            job[0] = None
            self._forget_job(job)

    # ---------------------------------------------------------------- extrema, watershed, clusters, surface points
    def _find_extrema(self, face, src, mask, shape, find_minima, find_maxima, minima_threshold, maxima_threshold,
                      connectivity, allow_borders, labels):
        """The capacity protocol of visfd_hip_find_extrema[_dev]: a first call with room for max(65536, voxels / 32)
        entries per list, a second -- which repeats the device work -- with the returned counts if that was too little."""
        nz, ny, nx = shape
        cap = 2 * [max(65536, nz * ny * nx // 32)]
        while True:
            lists = [(np.empty(c, np.int64), np.empty(c, np.float32), np.empty(c, np.int64)) for c in cap]
            n = [_i64(), _i64()]
            tail = []
            for (i, sc, nv), c, cnt in zip(lists, cap, n):
                tail += [i.ctypes.data, sc.ctypes.data, nv.ctypes.data, c, C.byref(cnt)]
            rc = self._rc("find_extrema", face, src, mask, nx, ny, nz, int(bool(find_minima)), int(bool(find_maxima)),
                          float(minima_threshold), float(maxima_threshold), int(connectivity), int(bool(allow_borders)),
                          *(tail + [labels]))
            if rc == 4 and (n[0].value > cap[0] or n[1].value > cap[1]):   # VISFD_HIP_ECAPACITY
                cap = [max(int(n[0].value), 1), max(int(n[1].value), 1)]
                continue
            self._chk(rc)
            return [tuple(a[:cnt.value].copy() for a in l) for l, cnt in zip(lists, n)]

    def find_extrema(self, src, mask=None, find_minima=True, find_maxima=True, minima_threshold=float("inf"),
                     maxima_threshold=-float("inf"), connectivity=3, allow_borders=True, want_labels=False, labels=None):
        """Plateau-aware local minima and maxima (_FindExtrema, morphology_implementation.hpp:57-515) of a numpy
        volume (nz, ny, nx): -> (minima, maxima[, labels]), each list (root index int64, score float32, voxels int64) in
        the reference's order; a kind that was not asked for comes back empty.  want_labels / labels: also the int32
        label image (written into a copy of `labels`, default zeros: voxels with mask == 0 keep those values).
        FindMaxima's own rule -- a threshold of +inf means none -- is find_maxima_only's."""
        out = None
        if want_labels or labels is not None:
            out = np.zeros(src.shape, np.int32) if labels is None else np.array(labels, np.int32, copy=True, order="C")
            assert out.shape == src.shape
        mins, maxs = self._find_extrema(_HOST, src, mask, src.shape, find_minima, find_maxima, minima_threshold,
                                        maxima_threshold, connectivity, allow_borders,
                                        None if out is None else out.ctypes.data)
        return (mins, maxs) if out is None else (mins, maxs, out)

    def find_extrema_dev(self, src, mask=None, find_minima=True, find_maxima=True, minima_threshold=float("inf"),
                         maxima_threshold=-float("inf"), connectivity=3, allow_borders=True, labels=None):
        """find_extrema on device tensors: -> (minima, maxima) as numpy lists; labels (an int32 cuda tensor, optional) is
        written in place where mask != 0.  Returns with the stream idle."""
        if labels is not None:
            assert labels.is_cuda and labels.is_contiguous() and str(labels.dtype) == "torch.int32" and \
                tuple(labels.shape) == tuple(src.shape), "labels: contiguous cuda int32 of src's shape"
        return tuple(self._find_extrema(_DEVICE, src, mask, tuple(src.shape), find_minima, find_maxima, minima_threshold,
                                        maxima_threshold, connectivity, allow_borders,
                                        None if labels is None else labels.data_ptr()))

    def find_minima_only(self, src, mask=None, threshold=float("inf"), connectivity=3, allow_borders=True, **kw):
        """visfd::FindMinima: -> (minima[, labels])."""
        r = self.find_extrema(src, mask, True, False, threshold, -float("inf"), connectivity, allow_borders, **kw)
        return r[0] if len(r) == 2 else (r[0], r[2])

    def find_maxima_only(self, src, mask=None, threshold=float("inf"), connectivity=3, allow_borders=True, **kw):
        """visfd::FindMaxima: -> (maxima[, labels]); a threshold of +inf is taken as -inf, as the reference does."""
        if threshold == float("inf"):
            threshold = -float("inf")
        r = self.find_extrema(src, mask, False, True, float("inf"), threshold, connectivity, allow_borders, **kw)
        return r[1] if len(r) == 2 else (r[1], r[2])

    def _watershed(self, face, src, mask, markers, labels, *params):
        """_watershed (the capacity protocol) on this context; markers and labels as addresses (int32 images)"""
        return _watershed(lambda *t: self._rc("watershed", face, *t), src, mask, None if markers is None else _address(markers),
                          tuple(src.shape), _address(labels), *params)

    def watershed(self, src, mask=None, markers=None, halt_threshold=None, start_from_minima=True, connectivity=1,
                  show_boundaries=True, label_boundary=0, label_undefined=-1):
        """visfd::Watershed (segmentation.hpp:65-559) of a numpy volume (nz, ny, nx): -> (labels int32, basin index int64,
        basin score float32).  Basin k of the seed list is labelled k + 1, boundaries label_boundary, unmasked voxels
        beyond the threshold label_undefined, voxels with mask == 0 hold -1.  halt_threshold None: none.  Without markers
        the labels are computed on the device; with markers (int32, entries <= 0 ignored), or under the option
        watershed_host, by the sequential flood on the host."""
        markers = _markers_np(markers, src.shape)
        labels = np.empty(src.shape, np.int32)
        index, score = self._watershed(_HOST, src, mask, markers, labels, halt_threshold, start_from_minima, connectivity,
                                       show_boundaries, label_boundary, label_undefined)
        return labels, index, score

    def watershed_dev(self, src, labels, mask=None, markers=None, halt_threshold=None, start_from_minima=True, connectivity=1,
                      show_boundaries=True, label_boundary=0, label_undefined=-1):
        """watershed on device tensors: labels (and markers) contiguous cuda int32 of src's shape, labels written in place
        everywhere; -> (basin index, basin score) as numpy lists.  Returns with the stream idle."""
        for t in (labels, markers):
            assert t is None or (t.is_cuda and t.is_contiguous() and str(t.dtype) == "torch.int32" and
                                 tuple(t.shape) == tuple(src.shape)), "labels / markers: contiguous cuda int32 of src's shape"
        return self._watershed(_DEVICE, src, mask, markers, labels, halt_threshold, start_from_minima, connectivity,
                               show_boundaries, label_boundary, label_undefined)

    def watershed_last_stats(self):
        """(path, label rounds, boundary rounds, basins) of the last watershed call; path WATERSHED_PATH_HOST or _DEVICE."""
        out = (_i64 * 4)()
        self._call("watershed_last_stats", _HOST, out)
        return tuple(int(v) for v in out)

    def label_connected_device_seeds(self, saliency, threshold_saliency, **kw):
        """api.label_connected with the seed search on this context's device (numpy arrays; the flood on the host)."""
        return label_connected(saliency, threshold_saliency, seeds_ctx=self, **kw)

    def label_connected_device_seeds_last(self):
        """(where, seeds) of the context's last label_connected_device_seeds: CONNECT_SEEDS_DEVICE and the length of the
        device's seed list, or CONNECT_SEEDS_HOST and -1 (the image or the connectivity is beyond the device search);
        (-1, -1) before the first call."""
        p, n = C.c_int(), _i64()
        self._call("label_connected_device_seeds_last", _HOST, C.byref(p), C.byref(n))
        return p.value, n.value

    def label_connected_graph(self, saliency, threshold_saliency, **kw):
        """api.label_connected_graph on this context's device (numpy arrays)."""
        return label_connected_graph(saliency, threshold_saliency, ctx=self, **kw)

    def label_connected_graph_dev(self, saliency, labels, threshold_saliency, mask=None, direction=None, tensor=None,
                                  threshold_vector_saliency=-np.inf, threshold_vector_neighbor=-np.inf,
                                  consider_dot_product_sign=True, threshold_tensor_saliency=-np.inf,
                                  threshold_tensor_neighbor=-np.inf, tensor_is_positive_definite_near_target=True,
                                  connectivity=1, label_undefined=-1, sort_by_size=True, standardize_directions=False,
                                  start_from_saliency_maxima=True, voxel_weights=None, must_link=None,
                                  must_link_directions=None):
        """label_connected_graph on device tensors: saliency, mask, voxel_weights float32 [nz,ny,nx], direction [...,3]
        (rewritten in place at labelled voxels when standardising), tensor [...,6], labels int64 [nz,ny,nx] (written).
        Returns (n_clusters, seed positions, sizes, seed saliencies) as numpy arrays."""
        nz, ny, nx = saliency.shape
        n = _i64(0)
        cap = int(saliency.numel())
        cm, cs, csal = np.zeros((cap, 3), np.float32), np.zeros(cap, np.float32), np.zeros(cap, np.float32)
        ml_c, ml_n, ml_d, ngroups = _must_link_arrays(must_link, must_link_directions)
        ptr = lambda a: None if a is None else a.ctypes.data
        assert labels.is_cuda and labels.is_contiguous() and str(labels.dtype) == "torch.int64" and \
            tuple(labels.shape) == tuple(saliency.shape), "labels: contiguous cuda int64 of the image's shape"
        self._call(
            "label_connected_graph", _DEVICE, saliency, labels.data_ptr(), mask, nx, ny, nz, threshold_saliency, direction,
            threshold_vector_saliency, threshold_vector_neighbor, int(bool(consider_dot_product_sign)), tensor,
            threshold_tensor_saliency, threshold_tensor_neighbor, int(bool(tensor_is_positive_definite_near_target)),
            int(connectivity), int(label_undefined), int(bool(sort_by_size)), int(bool(standardize_directions)),
            int(bool(start_from_saliency_maxima)), C.byref(n), cm.ctypes.data, cs.ctypes.data, csal.ctypes.data, cap,
            voxel_weights, ptr(ml_c), ptr(ml_n), ngroups, ptr(ml_d))
        k = n.value
        return k, cm[:k], cs[:k], csal[:k]

    def label_connected_graph_last(self):
        """(path, reasons, valid voxels, candidates of the host's vector test) of the context's last graph call."""
        return label_connected_graph_last(self)

    def label_connected_graph_last_settled(self):
        """Under the option connect_settle: the CONNECT_REASON_* bits among MUST_LINK, WEIGHTS and OUTWARD that the last
        device-path graph call settled itself; 0 after a call that took the flood or ran with the option off."""
        bits = C.c_uint(0)
        self._call("label_connected_graph_last_settled", _HOST, C.byref(bits))
        return bits.value

    def label_connected_graph_last_times(self):
        """Under the option connect_time: milliseconds of the last device-path graph call by stage (seed search, classify,
        host vector test, edges, clusters, directions, copies in, copies out)."""
        return self._last_times("label_connected_graph", 8)

    def _surface_points_call(self, face, saliency, direction, voxel2cluster, mask):
        """call(*tail) -> return code of visfd_hip_surface_points_ctx / _dev with everything up to the sizes filled in"""
        nz, ny, nx = saliency.shape
        return lambda *tail: self._rc("surface_points", face, saliency, voxel2cluster, direction, mask, nx, ny, nz, *tail)

    def surface_points(self, saliency, direction, voxel2cluster=None, mask=None, select_cluster=1, voxel_width=(1, 1, 1),
                       curve_ds=0.2, find_ridge=True, max_distance_to_feature=1.3, capacity=None):
        """api.surface_points_host on this context's device (visfd_hip_surface_points_ctx; numpy arrays, direction
        [nz, ny, nx, 3]): the same points, bit for bit."""
        return _surface_points(self._surface_points_call(_HOST_CTX, saliency, direction, voxel2cluster, mask), self._L,
                               saliency.shape, select_cluster, voxel_width, curve_ds, find_ridge, max_distance_to_feature,
                               capacity)

    def surface_points_dev(self, saliency, direction, voxel2cluster=None, mask=None, select_cluster=1, voxel_width=(1, 1, 1),
                           curve_ds=0.2, find_ridge=True, max_distance_to_feature=1.3, capacity=None, crds=None, norms=None):
        """surface_points on device tensors (visfd_hip_surface_points_dev): saliency, voxel2cluster, mask float32
        [nz, ny, nx], direction channel-planar [3, nz, ny, nx].  -> (crds, norms) as numpy (n, 3); or, with crds and norms
        given as contiguous cuda float32 [capacity, 3], the points go there and the count is returned.  Returns with the
        stream idle."""
        nz, ny, nx = saliency.shape
        assert tuple(direction.shape) == (3, nz, ny, nx), "direction: channel-planar [3, nz, ny, nx]"
        call = self._surface_points_call(_DEVICE, saliency, direction, voxel2cluster, mask)
        if crds is None:
            return _surface_points(call, self._L, saliency.shape, select_cluster, voxel_width, curve_ds, find_ridge,
                                   max_distance_to_feature, capacity)
        assert tuple(crds.shape) == tuple(norms.shape) and crds.shape[1] == 3, "crds, norms: [capacity, 3]"
        n = _i64(0)
        rc = call(int(select_cluster), _f3(voxel_width), float(curve_ds), int(bool(find_ridge)), float(max_distance_to_feature),
                  crds, norms, int(crds.shape[0]), C.byref(n))
        if rc:
            err = VisfdHipError(rc, self._L.visfd_hip_last_error().decode())
            err.needed = int(n.value)
            raise err
        return int(n.value)

    def surface_points_last(self):
        """(path, reasons, selected voxels, points, longest walk in steps, steps of all walks) of the context's last
        surface_points[_dev]: path
        SURFACE_POINTS_PATH_DEVICE or _HANDED_OVER (the host entry finished the call) with the SURFACE_POINTS_REASON_* bits."""
        out = (_i64 * 6)()
        self._call("surface_points_last", _HOST, out)
        return tuple(int(v) for v in out)

    def surface_points_last_times(self):
        """Under the option surface_points_time: (select and compact, walk, ridge gather, host finish and copies out)
        milliseconds of the last device-path surface_points[_dev]."""
        return self._last_times("surface_points", 4)

    # ---------------------------------------------------------------- ridges, tensor voting, the membrane stage
    def _calc_hessian(self, face, src, grad, hess, mask, sigma, ratio):
        nz, ny, nx = src.shape
        self._call("calc_hessian", face, src, grad, hess, mask, nx, ny, nz, float(sigma), float(ratio))

    def calc_hessian(self, src, sigma, ratio, mask=None, want_grad=True):
        nz, ny, nx = src.shape
        hess = np.zeros((nz, ny, nx, 6), np.float32)
        grad = np.zeros((nz, ny, nx, 3), np.float32) if want_grad else None
        self._calc_hessian(_HOST, src, grad, hess, mask, sigma, ratio)
        return grad, hess

    def calc_hessian_dev(self, src, grad, hess, sigma, ratio, mask=None):
        self._calc_hessian(_DEVICE, src, grad, hess, mask, sigma, ratio)

    def diagonalize(self, m6, order):
        m6 = np.ascontiguousarray(m6, np.float32)
        out = np.empty_like(m6)
        self._call("diagonalize_flat_sym3", _HOST, m6, out, m6.size // 6, int(order))
        return out

    def _hessian_saliency(self, face, hess, mask, n, order, sal, dirs):
        self._call("hessian_saliency", face, hess, mask, n, int(order), sal, dirs)

    def hessian_saliency(self, hess, order, mask=None):
        shp = hess.shape[:-1]
        sal = np.empty(shp, np.float32)
        dirs = np.zeros(shp + (3,), np.float32)
        self._hessian_saliency(_HOST, hess, mask, sal.size, order, sal, dirs)
        return sal, dirs

    def hessian_saliency_dev(self, hess, sal, dirs, order, mask=None):
        self._hessian_saliency(_DEVICE, hess, mask, sal.numel(), order, sal, dirs)

    def ridge_saliency_dev(self, src, sal, dirs, sigma, ratio, order, mask=None):
        nz, ny, nx = src.shape
        self._call("ridge_saliency", _DEVICE, src, mask, nx, ny, nz, float(sigma), float(ratio), int(order), sal, dirs)

    def ridge_scores_dev(self, src, sal, smoothed, sigma, ratio, order, mask=None, background=None):
        """Smoothing + Hessian + eigenvalues + score for every voxel; `smoothed` receives the smoothed volume.
        background (a volume from peak_background_dev): every score times (src - background)."""
        nz, ny, nx = src.shape
        self._call("ridge_scores_bg", _DEVICE, src, mask, nx, ny, nz, float(sigma), float(ratio), int(order), background, sal,
                   smoothed)

    def peak_background_dev(self, src, background, sigma_background, ratio, mask=None, normalize=True):
        """The background of the peak-height factor: ApplyGauss(src, sigma_b, floor(sigma_b * ratio)) (handlers.cpp:1577-1592)."""
        nz, ny, nx = src.shape
        self._call("peak_background", _DEVICE, src, mask, nx, ny, nz, float(sigma_background), float(ratio),
                   int(bool(normalize)), background)

    def ridge_directions_dev(self, smoothed, sal, dirs, sigma, order):
        """Principal directions of the voxels with sal != 0 (the others keep what dirs held)."""
        nz, ny, nx = smoothed.shape
        self._call("ridge_directions", _DEVICE, smoothed, nx, ny, nz, float(sigma), int(order), sal, dirs)

    def debug_ridge_directions_thr_dev(self, smoothed, sal, dirs, sigma, order, thr_dev=None):
        """Test aid: ridge_directions_dev on a volume that has not been cut; thr_dev: a one-element device tensor."""
        nz, ny, nx = smoothed.shape
        self._call("debug_ridge_directions_thr", _DEVICE, smoothed, nx, ny, nz, float(sigma), int(order), sal, thr_dev, dirs)

    def _threshold_fraction(self, face, sal, mask, n, fraction):
        thr = C.c_float()
        self._call("threshold_fraction", face, sal, mask, n, float(fraction), C.byref(thr))
        return thr.value

    def threshold_fraction(self, sal, fraction, mask=None):
        return self._threshold_fraction(_HOST, sal, mask, sal.size, fraction)

    def threshold_fraction_dev(self, sal, fraction, mask=None):
        return self._threshold_fraction(_DEVICE, sal, mask, sal.numel(), fraction)

    def select_histogram_dev(self, sal, pass_, prefix, mask=None):
        hist = np.zeros(2048, np.uint64)
        n = C.c_uint64()
        self._call("select_histogram", _DEVICE, sal, mask, sal.numel(), int(pass_), int(prefix), hist.ctypes.data, C.byref(n))
        return hist, int(n.value)

    def select_histogram_todev(self, sal, pass_, prefix, hist, mask=None):
        """The round's histogram into `hist` (int64 tensor of 2048 on the device), asynchronous."""
        assert hist.is_cuda and hist.numel() == 2048 and hist.element_size() == 8 and hist.is_contiguous()
        self._call("select_histogram_todev", _DEVICE_PLAIN, sal, mask, sal.numel(), int(pass_), int(prefix), hist.data_ptr())

    def stream_handle(self):
        """The hipStream_t (as an integer) this context's device face runs on."""
        return int(self._L.visfd_hip_get_stream(self._h) or 0)

    def apply_threshold_dev(self, sal, thr):
        self._call("apply_threshold", _DEVICE, sal, sal.numel(), float(thr))

    def tv_dense_stick(self, sal, dirs, sigma_tv, exponent=4, cutoff=2.0 ** 0.5, mask_src=None, mask_dst=None,
                       curves=False):
        nz, ny, nx = sal.shape
        tensor = np.zeros((nz, ny, nx, 6), np.float32)
        self._call("tv_dense_stick", _HOST, sal, dirs, tensor, mask_src, mask_dst, nx, ny, nz, float(sigma_tv), int(exponent),
                   float(cutoff), int(curves))
        return tensor

    def tv_dense_stick_dev(self, sal, dirs, tensor, sigma_tv, exponent=4, cutoff=2.0 ** 0.5, mask_src=None,
                           mask_dst=None, curves=False, z_out=None):
        nz, ny, nx = sal.shape
        z0, z1 = (0, nz) if z_out is None else z_out
        self._call("tv_dense_stick_slab", _DEVICE, sal, dirs, tensor, mask_src, mask_dst, nx, ny, nz, int(z0), int(z1),
                   float(sigma_tv), int(exponent), float(cutoff), int(curves))

    def debug_tv_lists_dev(self, sal, dirs, h, mode=0, fold=False, thr_dev=None):
        """Test aid: the sender lists of tensor voting for the whole volume -> (rows uint32 [nz, ny + 1, ntx], entries float32
        [total, 4], positions uint32 [total], flags).  List (z, tx) is entries[rows[z, ny, tx]:rows[z, 0, tx]]; where the
        lists lie in the arrays differs from run to run."""
        nz, ny, nx = sal.shape
        ntx = (nx + 15) // 16
        nrows, total, flags = _i64(), _i64(), C.c_uint32()
        rows = np.empty((nz, ny + 1, ntx), np.uint32)
        ent, pos = np.empty((0, 4), np.float32), np.empty(0, np.uint32)
        for _ in range(2):   # the second call has arrays for the total the first one reported
            self._call("debug_tv_lists", _DEVICE, sal, dirs, thr_dev, nx, ny, nz, int(h), int(mode), int(bool(fold)),
                       rows.ctypes.data, rows.size, ent.ctypes.data, pos.ctypes.data, pos.size, C.byref(nrows), C.byref(total),
                       C.byref(flags))
            assert nrows.value == rows.size
            if total.value <= pos.size:
                break
            ent, pos = np.empty((total.value, 4), np.float32), np.empty(total.value, np.uint32)
        return rows, ent[:total.value], pos[:total.value], int(flags.value)

    def tv_weight_sum(self, sal, sigma_tv, cutoff=2.0 ** 0.5, mask_src=None, mask_dst=None):
        """The normalisation denominators of TVDenseStick(normalize=true) (feature.hpp:1761-1822); zeros where mask_dst == 0."""
        nz, ny, nx = sal.shape
        den = np.zeros_like(sal)
        self._call("tv_weight_sum", _HOST, sal, den, mask_src, mask_dst, nx, ny, nz, float(sigma_tv), float(cutoff))
        return den

    def tensor_saliency(self, tensor, order, sal_inout, mask=None):
        self._call("tensor_saliency", _HOST, tensor, mask, sal_inout.size, int(order), sal_inout)
        return sal_inout

    def tensor_saliency_dev(self, tensor, sal, order, mask=None, image=None, background=None):
        self._call("tensor_saliency_bg", _DEVICE, tensor, mask, sal.numel(), int(order), image, background, sal)

    # ---- binning (resample.hpp:53-166); numpy shapes are [nz, ny, nx] -------------------------
    @staticmethod
    def _sizes(shape):
        return (_i64 * 3)(int(shape[2]), int(shape[1]), int(shape[0]))

    def _rebin(self, name, face, src, dst, offset):
        self._call(name, face, src, self._sizes(src.shape), dst, self._sizes(dst.shape),
                   _i3(offset) if offset is not None else None)

    def bin_array3d(self, src, dst_shape, offset=None):
        dst = np.empty(tuple(dst_shape), np.float32)
        self._rebin("bin_array3d", _HOST, src, dst, offset)
        return dst

    def unbin_array3d(self, src, dst_shape, offset=None):
        dst = np.empty(tuple(dst_shape), np.float32)
        self._rebin("unbin_array3d", _HOST, src, dst, offset)
        return dst

    def bin_array3d_dev(self, src, dst, offset=None):
        self._rebin("bin_array3d", _DEVICE, src, dst, offset)

    def unbin_array3d_dev(self, src, dst, offset=None):
        self._rebin("unbin_array3d", _DEVICE, src, dst, offset)

    def _membrane_detect(self, face, src, mask, sigma, ratio, order, best_fraction, threshold_abs, sigma_tv, tv_exponent,
                         tv_cutoff, sigma_background, normalize_background, sal, tensor, dirs):
        nz, ny, nx = src.shape
        thr = C.c_float()
        self._call("membrane_detect_bg", face, src, mask, nx, ny, nz, float(sigma), float(ratio), int(order),
                   float(best_fraction), float(threshold_abs), float(sigma_tv), int(tv_exponent), float(tv_cutoff),
                   float(sigma_background), int(bool(normalize_background)), sal, tensor, dirs, C.byref(thr))
        return thr.value

    def membrane_detect(self, src, sigma, ratio, order, best_fraction=0.05, threshold_abs=0.0, sigma_tv=0.0,
                        tv_exponent=4, tv_cutoff=2.0 ** 0.5, mask=None, want_tensor=True, want_dir=False,
                        sigma_background=0.0, normalize_background=True):
        """HandleTV's compute section on host arrays -> (saliency, tensor or None, dirs or None, threshold).
        sigma_background > 0: `-membrane-background`, both scores times (image - background)."""
        nz, ny, nx = src.shape
        sal = np.empty_like(src)
        ten = np.zeros((nz, ny, nx, 6), np.float32) if want_tensor else None
        dirs = np.zeros((nz, ny, nx, 3), np.float32) if want_dir else None
        thr = self._membrane_detect(_HOST, src, mask, sigma, ratio, order, best_fraction, threshold_abs, sigma_tv, tv_exponent,
                                    tv_cutoff, sigma_background, normalize_background, sal, ten, dirs)
        return sal, ten, dirs, thr

    def membrane_detect_dev(self, src, sal, sigma, ratio, order, best_fraction=0.05, threshold_abs=0.0, sigma_tv=0.0,
                            tv_exponent=4, tv_cutoff=2.0 ** 0.5, mask=None, dirs=None, tensor=None, sigma_background=0.0,
                            normalize_background=True):
        """visfd_hip_membrane_detect_bg_dev: HandleTV's compute section on device tensors; sal receives the scores, and
        -> the threshold.  dirs (3,nz,ny,nx) and tensor (6,nz,ny,nx) are optional outputs: None keeps them in the workspace."""
        return self._membrane_detect(_DEVICE, src, mask, sigma, ratio, order, best_fraction, threshold_abs, sigma_tv,
                                     tv_exponent, tv_cutoff, sigma_background, normalize_background, sal, tensor, dirs)

    def membrane_stage_dev(self, src, sal, dirs, tensor, scratch, sigma, ratio, order, best_fraction, sigma_tv, exponent=4,
                           cutoff=2.0 ** 0.5, mask=None, sigma_background=0.0, background=None, normalize_background=True):
        """visfd_hip_membrane_stage_dev: scores, fraction cut, directions of the survivors, vote and post-vote score on the
        caller's tensors, queued in one go under the option membrane_queue (one wait, no threshold pass).  `scratch`
        receives the smoothed image, `background` the background when sigma_background > 0.  Returns the threshold."""
        nz, ny, nx = src.shape
        thr = C.c_float()
        self._call("membrane_stage", _DEVICE, src, mask, nx, ny, nz, float(sigma), float(ratio), int(order),
                   float(best_fraction), float(sigma_tv), int(exponent), float(cutoff), float(sigma_background),
                   int(bool(normalize_background)), background, scratch, sal, dirs, tensor, C.byref(thr))
        return thr.value


class Slab:
    """One rank's handle of a Z-slab run (include/visfd_hip.h, section e; csrc/slab.hip): the layout, the transport and the
    slab forms of the stages.  `transport`:
      "rccl"   -- the library's own RCCL communicator (librccl.so loaded at run time): grouped send/recv with the two
                  Z-neighbours on the slab's transfer stream, all-reduces on the context's stream.  The 128-byte id is
                  made on rank 0 and broadcast here through torch.distributed (any backend);
      "torch"  -- callbacks into torch.distributed (host-staged copies): for backends without device point-to-point (gloo:
                  CPU tests, ranks sharing one GPU in a rehearsal).  The same C code drives both."""

    def __init__(self, ctx, rank, world, nz_global, ghost, transport="rccl", group=None):
        import torch
        import torch.distributed as dist
        self.ctx, self.rank, self.world = ctx, int(rank), int(world)
        self._L = load_library()
        self._h = _vp()
        self._keep = None
        if transport == "rccl_loopback":   # a one-rank RCCL communicator (selftest on a one-GPU box)
            assert world == 1
            idbuf = (C.c_char * 128)()
            ctx._chk(self._L.visfd_hip_slab_unique_id(C.addressof(idbuf)))
            ctx._chk(self._L.visfd_hip_slab_create_rccl(ctx._h, C.addressof(idbuf), 0, 1, nz_global, ghost, C.byref(self._h)))
        elif transport == "rccl" or world == 1:
            idbuf = (C.c_char * 128)()
            if world > 1:
                # Every rank takes the SAME steps whatever fails where: the broadcast always runs (an empty id says that rank 0
                # could not make one), then the ranks agree (MIN over "I have an id and can load RCCL") before any of them
                # enters ncclCommInitRank, which blocks until all have joined.
                ok_here = bool(self._L.visfd_hip_slab_rccl_available())
                box = [b""]
                if rank == 0 and ok_here and self._L.visfd_hip_slab_unique_id(C.addressof(idbuf)) == 0:
                    box = [bytes(idbuf)]
                dist.broadcast_object_list(box, src=0, group=group)
                ok_here = ok_here and len(box[0]) == 128
                on_gpu = dist.get_backend(group) == "nccl"
                flag = torch.tensor([1 if ok_here else 0], dtype=torch.int32, device="cuda" if on_gpu else "cpu")
                dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
                if not int(flag.item()):
                    raise VisfdHipError(2, "the library's RCCL communicator cannot come up on every rank (rank %d: %s)" % (
                        rank, "ok" if ok_here else "no id from rank 0 or librccl.so not loadable"))
                idbuf = (C.c_char * 128).from_buffer_copy(box[0])
            ctx._chk(self._L.visfd_hip_slab_create_rccl(ctx._h, C.addressof(idbuf) if world > 1 else None, rank, world, nz_global,
                                                        ghost, C.byref(self._h)))
        elif transport == "torch":
            def sync(stream):
                torch.cuda.ExternalStream(int(stream)).synchronize() if stream else torch.cuda.synchronize()

            def view(ptr, nbytes, dtype):
                itemsize = torch.empty((), dtype=dtype).element_size()
                return _device_view(torch, int(ptr), nbytes // itemsize, dtype)
            pending = []

            def sendrecv(user, peer, sendbuf, recvbuf, nbytes, stream):
                try:
                    sync(stream)
                    snd = view(sendbuf, nbytes, torch.float32).cpu()
                    rcv = torch.empty_like(snd)
                    pending.append((peer, snd, rcv, recvbuf, nbytes))
                    return 0
                except Exception as e:   # an exception must not cross the C frame
                    sys.stderr.write("visfd_amd.Slab transport: %r\n" % (e,))
                    return 1

            def group_end(user):
                try:
                    ops = []
                    for peer, snd, rcv, _, _ in pending:
                        if peer == self.rank:   # the self-test's exchange with itself: gloo has no pair to its own rank
                            rcv.copy_(snd)
                            continue
                        ops.append(dist.P2POp(dist.isend, snd, peer, group))
                        ops.append(dist.P2POp(dist.irecv, rcv, peer, group))
                    for r in (dist.batch_isend_irecv(ops) if ops else []):
                        r.wait()
                    for peer, snd, rcv, recvbuf, nbytes in pending:
                        view(recvbuf, nbytes, torch.float32).copy_(rcv)
                    torch.cuda.synchronize()
                    del pending[:]
                    return 0
                except Exception as e:
                    sys.stderr.write("visfd_amd.Slab transport: %r\n" % (e,))
                    return 1

            def allreduce(user, buf, count, stream):
                try:
                    sync(stream)
                    dv = view(buf, count * 8, torch.int64)
                    h = dv.cpu()
                    dist.all_reduce(h, op=dist.ReduceOp.SUM, group=group)
                    dv.copy_(h)
                    torch.cuda.synchronize()
                    return 0
                except Exception as e:
                    sys.stderr.write("visfd_amd.Slab transport: %r\n" % (e,))
                    return 1
            tr = Transport(_SENDRECV(sendrecv), _ALLREDUCE(allreduce), _GROUP(lambda user: 0), _GROUP(group_end), None)
            self._keep = tr   # the C side copies the struct; the CFUNCTYPE objects inside must outlive the slab
            ctx._chk(self._L.visfd_hip_slab_create_custom(ctx._h, C.addressof(tr), rank, world, nz_global, ghost, C.byref(self._h)))
        else:
            raise ValueError("transport must be 'rccl' or 'torch'")
        import weakref
        if not hasattr(ctx, "_slabs"):
            ctx._slabs = []
        ctx._slabs.append(weakref.ref(self))    # Context.close() destroys its slabs first
        lay = (_i64 * 7)()
        ctx._chk(self._L.visfd_hip_slab_layout(self._h, lay))
        self.z0, self.z1, self.lo, self.hi, self.own0, self.own1, self.nz_local = [int(v) for v in lay]
        self.nz_global, self.ghost = int(nz_global), int(ghost)

    def close(self):
        if self._h:
            self._L.visfd_hip_slab_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def owned(self, t):
        return t[..., self.own0:self.own1, :, :]

    def selftest(self, count=1 << 20):
        """visfd_hip_slab_selftest: self send/receive on the transfer stream + all-reduce, verified (raises on failure)."""
        self.ctx._chk(self._L.visfd_hip_slab_selftest(self._h, int(count)))

    def set_reserve(self, workgroups):
        self.ctx._chk(self._L.visfd_hip_slab_set_reserve(self._h, int(workgroups)))

    def exchange(self, tensors, depth):
        tensors = tensors if isinstance(tensors, (list, tuple)) else [tensors]
        nz, ny, nx = tensors[0].shape
        assert nz == self.nz_local
        arr = (_vp * len(tensors))(*[_dev(t) for t in tensors])
        self.ctx._chk(self._L.visfd_hip_slab_exchange_dev(self._h, arr, len(tensors), nx, ny, int(depth)))

    def membrane_detect(self, src, sal, dirs, tensor, scratch, sigma, ratio, order, best_fraction, sigma_tv, exponent=4,
                        cutoff=2.0 ** 0.5, src_halo_ready=False, sigma_background=0.0, background=None, normalize_background=True):
        nz, ny, nx = src.shape
        assert nz == self.nz_local and dirs.shape[0] == 3 and tensor.shape[0] == 6
        thr = C.c_float()
        self.ctx._chk(self._L.visfd_hip_membrane_detect_slab_bg_dev(
            self._h, _dev(src), _dev(sal), _dev(dirs), _dev(tensor), _dev(scratch), _dev(background), nx, ny, float(sigma),
            float(ratio), int(order), float(best_fraction), float(sigma_tv), int(exponent), float(cutoff), float(sigma_background),
            int(bool(normalize_background)), int(bool(src_halo_ready)), C.byref(thr)))
        return float(thr.value)

    def membrane_detect_host(self, src_owned, sigma, ratio, order, best_fraction, sigma_tv, exponent=4, cutoff=2.0 ** 0.5,
                             want_tensor=False, sigma_background=0.0, normalize_background=True):
        """visfd_hip_membrane_detect_slab: the slab stage on HOST arrays of the rank's owned planes (numpy float32
        [z1-z0][ny][nx]).  Returns (saliency of the owned planes, tensor [..., 6] or None, threshold)."""
        src_owned = np.ascontiguousarray(src_owned, np.float32)
        nzo, ny, nx = src_owned.shape
        assert nzo == self.z1 - self.z0
        sal = np.empty_like(src_owned)
        ten = np.empty(src_owned.shape + (6,), np.float32) if want_tensor else None
        thr = C.c_float()
        self.ctx._chk(self._L.visfd_hip_membrane_detect_slab_bg(
            self._h, _np(src_owned), nx, ny, float(sigma), float(ratio), int(order), float(best_fraction), float(sigma_tv),
            int(exponent), float(cutoff), float(sigma_background), int(bool(normalize_background)), _np(sal), _np(ten),
            C.byref(thr)))
        return sal, ten, float(thr.value)

    def blob_dog(self, src, sigmas, delta=0.02, ratio=2.5, minima_threshold=np.inf, maxima_threshold=-np.inf,
                 src_halo_ready=False, cap=1 << 22):
        """-> (minima, maxima) rows x, y, z (GLOBAL plane index), sigma, score of the OWNED planes."""
        nz, ny, nx = src.shape
        sig = np.ascontiguousarray(sigmas, np.float32)
        while True:
            mn, mx = (Blob * cap)(), (Blob * cap)()
            nmin, nmax = _i64(), _i64()
            rc = self._L.visfd_hip_blob_dog_slab_dev(self._h, _dev(src), nx, ny, sig.ctypes.data_as(_fp), len(sig), float(delta),
                                                     float(ratio), float(minima_threshold), float(maxima_threshold),
                                                     int(bool(src_halo_ready)), C.addressof(mn), cap, C.byref(nmin),
                                                     C.addressof(mx), cap, C.byref(nmax))
            if rc == 4:   # VISFD_HIP_ECAPACITY: a LOCAL retry -- the ghost planes are in place, so no exchange and no other rank
                cap = max(int(nmin.value), int(nmax.value), cap) + 16
                src_halo_ready = True
                continue
            self.ctx._chk(rc)
            break
        return _slab_blob_rows(mn, int(nmin.value)), _slab_blob_rows(mx, int(nmax.value))

    def gauss_host(self, src_owned, sigma, hw, normalize=True):
        """visfd_hip_apply_gauss_slab: the Gaussian of the rank's owned planes (numpy float32 [z1-z0][ny][nx], the ghost
        planes come from the neighbours) -> (owned planes of the result, A)."""
        src_owned = np.ascontiguousarray(src_owned, np.float32)
        nzo, ny, nx = src_owned.shape
        assert nzo == self.z1 - self.z0
        dst = np.empty_like(src_owned)
        A = C.c_float()
        self.ctx._chk(self._L.visfd_hip_apply_gauss_slab(self._h, _np(src_owned), nx, ny, _f3(sigma), _i3(hw), int(bool(normalize)),
                                                         _np(dst), C.byref(A)))
        return dst, float(A.value)

    def blob_dog_host(self, src_owned, sigmas, delta=0.02, ratio=2.5, minima_threshold=np.inf, maxima_threshold=-np.inf,
                      cap=1 << 16):
        """visfd_hip_blob_dog_slab: the blobs of the rank's owned planes (numpy float32 [z1-z0][ny][nx]) -> (minima, maxima)
        rows as blob_dog returns them.  A list longer than `cap` raises (VISFD_HIP_ECAPACITY): this face exchanges the halo
        on every call, so a retry is not local to one rank."""
        src_owned = np.ascontiguousarray(src_owned, np.float32)
        nzo, ny, nx = src_owned.shape
        assert nzo == self.z1 - self.z0
        sig = np.ascontiguousarray(sigmas, np.float32)
        mn, mx = (Blob * cap)(), (Blob * cap)()
        nmin, nmax = _i64(), _i64()
        self.ctx._chk(self._L.visfd_hip_blob_dog_slab(self._h, _np(src_owned), nx, ny, sig.ctypes.data_as(_fp), len(sig), float(delta),
                                                      float(ratio), float(minima_threshold), float(maxima_threshold),
                                                      C.addressof(mn), cap, C.byref(nmin), C.addressof(mx), cap, C.byref(nmax)))
        return _slab_blob_rows(mn, int(nmin.value)), _slab_blob_rows(mx, int(nmax.value))


def _slab_blob_rows(arr, n):
    """visfd_hip_blob records -> float32 rows x, y, z, sigma, score."""
    a = np.frombuffer(arr, dtype=np.dtype([("ix", "<i4"), ("iy", "<i4"), ("iz", "<i4"), ("scale", "<i4"),
                                           ("sigma", "<f4"), ("score", "<f4")]), count=n)
    out = np.empty((n, 5), np.float32)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3], out[:, 4] = a["ix"], a["iy"], a["iz"], a["sigma"], a["score"]
    return out


def _device_view(torch, ptr, count, dtype):
    """A torch tensor over `count` elements of device memory at `ptr` (the library's buffers inside a transport callback)."""
    class _Iface:
        pass
    typestr = {torch.float32: "<f4", torch.int64: "<i8"}[dtype]
    obj = _Iface()
    obj.__cuda_array_interface__ = {"shape": (int(count),), "typestr": typestr, "data": (int(ptr), False), "version": 2}
    return torch.as_tensor(obj, device="cuda")
