"""Numpy restatement of the median filter's contract (the reference is lib/visfd/filter3d.hpp:
1577-1674, whose footprint loop never ends once a neighbour is skipped).

A voxel with mask == 0 keeps dst.  Any other voxel collects src at voxel + entry for every footprint entry inside the image
with mask != 0 and gets the value of rank n // 2 (0-based, ascending) among the n collected, or +0.0f when n == 0.  The
order is the total order of the keys below, so every result is defined to the bit."""
import numpy as np

F = np.float32
EXCLUDED = np.int64(1) << 32   # above every key


def footprint(radius):
    """MedianSphere's footprint (filter3d.hpp:1652-1662): Ri = ceil(radius), (float)sqrt((double)(ix^2 + iy^2 + iz^2)) <=
    radius, iz outermost, then iy, then ix.  -> int32 (n, 3) of (ix, iy, iz)"""
    radius = F(radius)
    Ri = int(np.ceil(radius))
    out = []
    for iz in range(-Ri, Ri + 1):
        for iy in range(-Ri, Ri + 1):
            for ix in range(-Ri, Ri + 1):
                if F(np.sqrt(np.float64(ix * ix + iy * iy + iz * iz))) <= radius:
                    out.append((ix, iy, iz))
    return np.array(out, np.int32).reshape(-1, 3)


def keys(a):
    """float32 -> uint32 keys whose unsigned order is the filter's order: ~u where the sign bit is set, else u | 2^31."""
    u = np.ascontiguousarray(a, F).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unkeys(k):
    k = np.ascontiguousarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7fffffff), ~k).astype(np.uint32).view(F)


def median_table(src, dxyz, mask=None, dst=None):
    """The filter with an arbitrary footprint: shifted key volumes stacked, excluded cells marked above every key, sorted
    along the stack, entry count // 2 picked."""
    src = np.ascontiguousarray(src, F)
    nz, ny, nx = src.shape
    d = np.asarray(dxyz, np.int64).reshape(-1, 3)
    K = keys(src).astype(np.int64)
    if mask is not None:
        K = np.where(np.asarray(mask) == 0, EXCLUDED, K)
    stack = np.full((len(d), nz, ny, nx), EXCLUDED, np.int64)
    for j, (dx, dy, dz) in enumerate(d):
        z0, z1 = max(0, -dz), min(nz, nz - dz)
        y0, y1 = max(0, -dy), min(ny, ny - dy)
        x0, x1 = max(0, -dx), min(nx, nx - dx)
        if z0 < z1 and y0 < y1 and x0 < x1:
            stack[j, z0:z1, y0:y1, x0:x1] = K[z0 + dz:z1 + dz, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    count = (stack != EXCLUDED).sum(axis=0)
    stack.sort(axis=0)
    pick = np.take_along_axis(stack, np.minimum(count // 2, len(d) - 1)[None], axis=0)[0]
    res = np.where(count > 0, unkeys(np.where(count > 0, pick, 0).astype(np.uint32)).view(np.uint32), np.uint32(0))
    out = np.array(src if dst is None else dst, F, copy=True)
    o = out.view(np.uint32)
    written = np.ones(src.shape, bool) if mask is None else (np.asarray(mask) != 0)
    o[written] = res.astype(np.uint32)[written]
    return out


def median_sphere(src, radius, mask=None, dst=None):
    return median_table(src, footprint(radius), mask=mask, dst=dst)


def median_brute(src, dxyz, mask=None, dst=None, voxels=None):
    """The contract voxel by voxel (python loops; for small volumes or a list of (iz, iy, ix) voxels)."""
    src = np.ascontiguousarray(src, F)
    nz, ny, nx = src.shape
    K = keys(src)
    out = np.array(src if dst is None else dst, F, copy=True)
    o = out.view(np.uint32)
    if voxels is None:
        voxels = [(z, y, x) for z in range(nz) for y in range(ny) for x in range(nx)]
    for z, y, x in voxels:
        if mask is not None and mask[z, y, x] == 0:
            continue
        got = []
        for dx, dy, dz in np.asarray(dxyz).reshape(-1, 3):
            X, Y, Z = x + int(dx), y + int(dy), z + int(dz)
            if X < 0 or X >= nx or Y < 0 or Y >= ny or Z < 0 or Z >= nz:
                continue
            if mask is not None and mask[Z, Y, X] == 0:
                continue
            got.append(int(K[Z, Y, X]))
        if not got:
            o[z, y, x] = 0
            continue
        got.sort()
        o[z, y, x] = unkeys(np.array([got[len(got) // 2]], np.uint32)).view(np.uint32)[0]
    return out
