"""Host-side orchestration of the hot path on device-resident volumes (torch tensors in HBM).

These functions mirror the reference's filter_mrc handlers for this path:
  gauss()            HandleGauss        bin/filter_mrc/handlers.cpp:218
  blob_detect()      HandleBlobDetector bin/filter_mrc/handlers.cpp:787  (BlobDogD part)
  membrane_detect()  HandleTV           bin/filter_mrc/handlers.cpp:1501 (up to the vote score, :1892)
  intensity_tail()   the end of main()  bin/filter_mrc/filter_mrc.cpp:746-786 (-invert, one intensity map, mask fill,
                                        -rescale-min-max); gauss() and membrane_detect() run it when given `tail`
They only sequence calls into the C ABI (visfd_amd.api.Context.*_dev); all arithmetic is in
libvisfd_hip.so.  PyTorch is used for device memory and streams only.
"""
import math

import numpy as np

from . import api

TRUNCATE_THRESHOLD = 0.03  # CLI default, bin/filter_mrc/settings.cpp:81


def cli_blob_sigmas(width_min, width_max, growth):
    """The sigma ladder of `-blob-s all <file> min max growth` (settings.cpp:1719-1750 with
    blob_width_multiplier = 2*sqrt(3), then feature.hpp:475)."""
    wmin, wmax, g = np.float32(width_min), np.float32(width_max), np.float32(growth)
    N = 1 + int(math.ceil(np.float32(np.log(np.float32(wmax / wmin), dtype=np.float32) / np.log(g, dtype=np.float32))))
    g = np.float32(math.pow(float(np.float32(wmax / wmin)), 1.0 / N))
    d = np.empty(N, np.float32)
    d[0] = np.float32(wmin * np.float32(2.0 * math.sqrt(3.0)))
    for n in range(1, N):
        d[n] = np.float32(d[n - 1] * g)
    return api.diameters_to_sigmas(d)


def intensity_tail(ctx, src, out, mask=None, invert=False, map=api.MAP_NONE, t=(), out_a=0.0, out_b=1.0,
                   masked_value=None, rescale_min_max=None):
    """The tail of a filter_mrc run on device tensors, `out` in place: -invert (about the mean of `out` inside the mask),
    one map (api.MAP_*; the threshold family maps `src`, the INPUT image, and overwrites `out` as in the reference;
    MAP_RESCALE acts on `out`), masked_value outside the mask (filter_mrc fills 0 there when there is a mask), then
    rescale_min_max = (max, min) as the flag takes them.  At most one statistics pass and two map passes.
    -invert needs a mean that is the same in every order of summation (Context.image_stats: order_free); an image without
    that proof is refused here: sum it in the order you need and call Context.intensity_map with that mean."""
    ave = None
    if invert:
        st = ctx.image_stats(out, mask)
        if st["n_nonfinite"] or not st["order_free"]:
            raise ValueError("intensity_tail: the mean of this image depends on the order of summation")
        ave = st["sum"] / st["count"] if st["count"] else float("nan")
    reads_src = map in (api.MAP_STEP, api.MAP_THRESH2, api.MAP_THRESH4, api.MAP_RANGE, api.MAP_GAUSS)
    p = api.intensity(map, t, out_a, out_b, invert_ave=ave, masked_value=masked_value if mask is not None else None,
                      stats_mask=True)
    staged = invert or map != api.MAP_NONE or p.mask_fill
    if rescale_min_max is None:
        if staged:
            ctx.intensity_map(p, out, src if reads_src else None, mask)
        return
    st = ctx.intensity_map(p, out, src if reads_src else None, mask, want_stats=True) if staged else ctx.image_stats(out, mask)
    if st["n_nonfinite"]:
        raise ValueError("intensity_tail: -rescale-min-max of an image with NaN or infinite voxels")
    hi, lo = rescale_min_max
    ctx.intensity_map(api.intensity(rescale01=(st["min"], st["max"], lo, hi)), out)


def gauss(ctx, src, dst, sigma, truncate_threshold=TRUNCATE_THRESHOLD, mask=None, normalize=True, tail=None):
    """filter_mrc -gauss sigma (voxels).  tail: keyword arguments of intensity_tail, run on dst afterwards."""
    ratio = api.ratio_from_threshold(truncate_threshold)
    sig = (sigma,) * 3 if np.isscalar(sigma) else tuple(sigma)
    hw = api.gauss_halfwidths(sig, ratio)
    A = ctx.gauss_dev(src, dst, sig, hw, mask, normalize)
    if tail is not None:
        intensity_tail(ctx, src, dst, mask, **tail)
    return A


def blob_detect(ctx, src, sigmas, truncate_threshold=TRUNCATE_THRESHOLD, delta=0.02, mask=None,
                minima_threshold=np.inf, maxima_threshold=-np.inf, use_ratios=False, cap=1 << 22):
    """filter_mrc -blob-s: returns (minima, maxima) rows x,y,z,sigma,score."""
    ratio = api.ratio_from_threshold(truncate_threshold)
    return ctx.blob_dog_dev(src, sigmas, mask, None, delta, ratio, minima_threshold, maxima_threshold,
                            use_ratios, cap)


def blob_detect_begin(ctx, src, sigmas, truncate_threshold=TRUNCATE_THRESHOLD, delta=0.02, mask=None,
                      minima_threshold=np.inf, maxima_threshold=-np.inf, use_ratios=False):
    """blob_detect in two halves: everything is queued here; blob_detect_end() hands the lists over.  Device work queued on
    the same context in between (the membrane stage) runs right behind the last scan, while the host still handles lists."""
    ratio = api.ratio_from_threshold(truncate_threshold)
    return ctx.blob_dog_begin_dev(src, sigmas, mask, None, delta, ratio, minima_threshold, maxima_threshold, use_ratios)


def blob_detect_end(ctx, job, cap=1 << 22):
    return ctx.blob_dog_end(job, cap)


def membrane_detect(ctx, src, sal, dirs, tensor, sigma, tv_sigma_ratio, tv_exponent=4, best_fraction=0.05,
                    truncate_threshold=TRUNCATE_THRESHOLD, tv_truncate_ratio=math.sqrt(2.0), minima=True,
                    mask=None, scratch=None, sigma_background=0.0, background=None, tail=None):
    """filter_mrc -membrane {minima|maxima} -tv ratio -tv-angle-exponent n: fills `sal` with the
    post-voting saliency (lambda0 - lambda1 of the vote tensor), `tensor` with the 6 vote planes.
    Returns the saliency threshold that was applied before voting.  tail: keyword arguments of intensity_tail, run on `sal`
    afterwards; only the stages that act on the output (invert, MAP_RESCALE, masked_value, rescale_min_max), as in
    filter_mrc."""
    order = api.DECREASING_EIVALS if minima else api.INCREASING_EIVALS  # handlers.cpp:1524-1535
    ratio = api.ratio_from_threshold(truncate_threshold)
    # scores for every voxel, threshold, then directions of the survivors only (`scratch`: a volume-sized tensor
    # for the smoothed image; allocated here when the caller has none to lend).  Voxels below the threshold keep
    # whatever `dirs` held: nothing downstream reads them.
    smoothed = scratch if scratch is not None else src.new_empty(src.shape)
    bg = None
    if sigma_background > 0:   # -membrane-background: both scores times (src - background), handlers.cpp:1577-1605,1698-1702
        bg = background if background is not None else src.new_empty(src.shape)
    sigma_tv = float(np.float32(tv_sigma_ratio) * np.float32(sigma))  # settings.cpp:3535-3540
    if sigma_tv > 0:
        # the whole stage in one call of the library, which queues it in one go (option membrane_queue, csrc/api.hip)
        thr = ctx.membrane_stage_dev(src, sal, dirs, tensor, smoothed, sigma, ratio, order, best_fraction, sigma_tv, tv_exponent,
                                     tv_truncate_ratio, mask, sigma_background if bg is not None else 0.0, bg)
    else:   # a vote of width 0 (the baseline kernel's self votes): stage by stage
        if bg is not None:
            ctx.peak_background_dev(src, bg, sigma_background, ratio, mask)
        ctx.ridge_scores_dev(src, sal, smoothed, sigma, ratio, order, mask, bg)
        thr = ctx.threshold_fraction_dev(sal, best_fraction, mask)
        ctx.ridge_directions_dev(smoothed, sal, dirs, sigma, order)
        ctx.tv_dense_stick_dev(sal, dirs, tensor, sigma_tv, tv_exponent, tv_truncate_ratio, mask, mask)
        ctx.tensor_saliency_dev(tensor, sal, order, mask, src if bg is not None else None, bg)
    if tail is not None:
        if tail.get("map", api.MAP_NONE) not in (api.MAP_NONE, api.MAP_RESCALE):
            raise ValueError("membrane_detect: the threshold maps read the input image; only MAP_RESCALE acts on the saliency")
        intensity_tail(ctx, src, sal, mask, **tail)
    return thr
