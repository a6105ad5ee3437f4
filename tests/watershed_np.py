"""A literal numpy / heapq restatement of the reference's watershed (Watershed, lib/visfd/segmentation.hpp:65-559): the
sequential Meyer flood from a priority queue, seeds from extrema_np (or from markers), the closing relabelling passes with
their quirks, and filter_mrc's conversion of the labels into the image it writes (HandleWatershed, handlers.cpp:1280-1391).
It deliberately knows nothing of the parallel definition the kernels compute: it is the independent
statement they are held to."""
import heapq

import numpy as np

import extrema_np

f32 = np.float32
INF = float("inf")


def watershed(src, mask=None, markers=None, halt_threshold=INF, start_from_minima=True, connectivity=1,
              show_boundaries=True, label_boundary=0, label_undefined=-1):
    """-> (labels int32 (nz, ny, nx), basin index int64, basin score float32).  halt_threshold is taken as given, except
    that +inf means -inf when starting from maxima (segmentation.hpp:125-134)."""
    src = np.asarray(src, f32)
    nz, ny, nx = src.shape
    S = src.reshape(-1)
    exist = np.ones(S.size, bool) if mask is None else (np.asarray(mask).reshape(-1) != 0)
    sign = 1.0 if start_from_minima else -1.0
    if not start_from_minima and halt_threshold == INF:
        halt_threshold = -INF
    halt = float(f32(halt_threshold)) * sign
    offsets = [(dx, dy, dz) for dz, dy, dx in extrema_np.neighbours(connectivity)]   # dz outermost, as the reference's

    if markers is not None:
        M = np.asarray(markers).reshape(-1)
        seeds, so_far = [], set()
        for i in np.nonzero(exist & (M > 0))[0]:
            if int(M[i]) not in so_far:
                so_far.add(int(M[i]))
                seeds.append(int(i))
        max_label = max(so_far) if so_far else 0
    else:
        r = extrema_np.find_extrema(src, mask, start_from_minima, not start_from_minima, halt_threshold, halt_threshold,
                                    connectivity, True)
        seeds = [int(i) for i in (r["min"] if start_from_minima else r["max"])[0]]
        max_label = len(seeds)
    scores = [S[i] for i in seeds]

    UNDEFINED, BOUNDARY, QUEUED = -1, 0, max_label + 1
    dest = [UNDEFINED] * S.size
    # the reference pops the LARGEST (-s, basin, (x, y, z)); heapq pops the smallest, so every component is negated
    q = []
    for k, i in enumerate(seeds):
        x, y, z = i % nx, (i // nx) % ny, i // (nx * ny)
        heapq.heappush(q, (float(S[i]) * sign, -k, (-x, -y, -z)))
        dest[i] = QUEUED
    while q:
        s, k, at = heapq.heappop(q)
        basin, x, y, z = -k, -at[0], -at[1], -at[2]
        i = (z * ny + y) * nx + x
        if s > halt or not exist[i]:
            dest[i] = UNDEFINED
            continue
        dest[i] = basin + 1
        for dx, dy, dz in offsets:
            xx, yy, zz = x + dx, y + dy, z + dz
            if not (0 <= xx < nx and 0 <= yy < ny and 0 <= zz < nz):
                continue
            j = (zz * ny + yy) * nx + xx
            if not exist[j] or dest[j] == BOUNDARY or dest[j] == QUEUED:
                continue
            if dest[j] == UNDEFINED:
                dest[j] = QUEUED
                heapq.heappush(q, (float(S[j]) * sign, -basin, (-xx, -yy, -zz)))
            elif dest[j] != dest[i] and show_boundaries:
                dest[i] = BOUNDARY

    dest = np.array(dest, np.int64)
    if label_boundary != BOUNDARY:
        dest[exist & (dest == BOUNDARY)] = label_boundary
    if label_undefined != UNDEFINED:
        dest[exist & (dest == UNDEFINED)] = label_undefined
    if markers is not None:
        old2new = {}
        for i in np.nonzero(M > 0)[0]:                      # masked voxels too
            if dest[i] != label_boundary and dest[i] != label_undefined:
                old2new[int(dest[i])] = int(M[i])
        for i in np.nonzero(exist & (dest != label_boundary) & (dest != label_undefined))[0]:
            dest[i] = old2new.get(int(dest[i]), label_undefined)
    return dest.astype(np.int32).reshape(src.shape), np.array(seeds, np.int64), np.array(scores, f32)


def program_output(labels, mask=None, undefined_out="max", mask_out=0.0):
    """What filter_mrc writes for these labels (it calls Watershed with label_undefined = -1): the labels as floats, -1 as
    the largest label plus one (`-undefined-out max`, the default) or as the given number, and voxels with mask == 0 as
    the `-mask-out` value."""
    out = labels.astype(f32)
    out[labels == -1] = f32(int(labels.max()) + 1) if undefined_out == "max" else f32(undefined_out)
    if mask is not None:
        out[np.asarray(mask) == 0] = f32(mask_out)
    return out
