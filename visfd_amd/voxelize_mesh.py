"""python -m visfd_amd.voxelize_mesh: a closed triangle mesh (PLY) as a 0/1 image, with the arguments of the reference's
bin/voxelize_mesh/voxelize_mesh.py.  The image is an MRC file of mode 0 (bytes 0 and 1), which filter_mrc takes as its -mask.

The samples are min + i * w per axis, ceil((max - min) / w) of them (what numpy.arange(min, max, w) gives); which of them
are inside is decided on the GPU by the exact rule of Context.voxelize_mesh (include/visfd_hip.h), not by vtk."""
import argparse
import math
import sys

import numpy as np

from . import api, ply


class InputError(Exception):
    pass


def read_mrc_header(path):
    """-> dict with n = (nx, ny, nz), m = (mx, my, mz), cella, cellb, origin (each three floats)"""
    try:
        with open(path, "rb") as f:
            raw = f.read(1024)
    except IOError:
        raise InputError('Error: Unable to open file "' + path + '" for reading.\n')
    if len(raw) < 1024:
        raise InputError('Error: "' + path + '" is too short to be an MRC file.\n')
    i, fl = np.frombuffer(raw, "<i4"), np.frombuffer(raw, "<f4")
    return {"n": tuple(int(x) for x in i[0:3]), "m": tuple(int(x) for x in i[7:10]), "cella": tuple(float(x) for x in fl[10:13]),
            "cellb": tuple(float(x) for x in fl[13:16]), "origin": tuple(float(x) for x in fl[49:52])}


def write_mrc_bytes(path, vol, cella, cellb=(90.0, 90.0, 90.0), origin=(0.0, 0.0, 0.0)):
    """vol [nz, ny, nx] of 0 and 1 as an MRC2014 file of mode 0"""
    nz, ny, nx = vol.shape
    data = np.ascontiguousarray(vol).astype("i1")
    h = np.zeros(256, "<i4")
    hf = h.view("<f4")
    h[0:3] = (nx, ny, nz)
    h[3] = 0
    h[7:10] = (nx, ny, nz)
    hf[10:13] = cella
    hf[13:16] = cellb
    h[16:19] = (1, 2, 3)
    hf[19:22] = (float(data.min()), float(data.max()), float(data.mean(dtype=np.float64)))
    h[27] = 20140
    hf[49:52] = origin
    raw = bytearray(h.tobytes())
    raw[208:212] = b"MAP "
    raw[212:216] = bytes([0x44, 0x44, 0, 0])
    with open(path, "wb") as f:
        f.write(bytes(raw))
        f.write(data.tobytes())


def plan(header=None, width=None, crop=None, bounds=None, shift=None):
    """The script's arithmetic: -> (w, bounds (xmin, xmax, ymin, ymax, zmin, zmax), (nx, ny, nz), origin in voxels,
    width_from_file).  header: read_mrc_header of the -i file, or None."""
    w = width
    if w == 0.0:
        raise InputError("Error: voxel width cannot be non-zero\n")   # the reference's wording
    from_file = False
    if header is not None:
        if w is None:
            from_file = True
            w = header["cella"][0] / header["m"][0] if header["m"][0] > 0 else 0.0
            if not (w > 0.0):
                raise InputError("Error: the input image's header gives no voxel width; use -w\n")
        if bounds is None:
            n = header["n"]
            bounds = (0.0, n[0] * w, 0.0, n[1] * w, 0.0, n[2] * w)
    elif w is None:
        w = 1.0
    if crop is not None:
        bounds = (crop[0] * w, (crop[1] + 0.99) * w, crop[2] * w, (crop[3] + 0.99) * w, crop[4] * w, (crop[5] + 0.99) * w)
    if bounds is None:
        raise InputError("Error: the image size is unknown: use -i, -c or -b\n")
    bounds = tuple(float(b) for b in bounds)
    s = (0.0, 0.0, 0.0) if shift is None else tuple(float(x) for x in shift)
    n = tuple(max(int(math.ceil((bounds[2 * d + 1] - bounds[2 * d]) / w)), 0) for d in range(3))
    if min(n) <= 0:
        raise InputError("Error: the bounds leave no voxel\n")
    origin = tuple(bounds[2 * d] / w - s[d] for d in range(3))
    return float(w), bounds, n, origin, from_file


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m visfd_amd.voxelize_mesh")
    ap.add_argument("-m", "--mesh", dest="fname_mesh", required=True, help='file containing a closed mesh (a ".ply" file)')
    ap.add_argument("-o", "--out", dest="fname_out", required=True, help="the output image (mrc/rec format, bytes 0 and 1)")
    ap.add_argument("-i", "--in", dest="fname_mrc_orig", help="an MRC (or REC) file with the size of the target")
    ap.add_argument("-w", "--width", dest="voxel_width", type=float, help="the voxel width (default 1)")
    ap.add_argument("-c", "--crop", dest="ibounds", type=float, nargs=6, help="xmin xmax ymin ymax zmin zmax in voxels")
    ap.add_argument("-b", "--bounds", dest="bounds", type=float, nargs=6, help="xmin xmax ymin ymax zmin zmax in physical units")
    ap.add_argument("-s", "--shift", dest="shift", type=float, nargs=3, help="shift of the mesh in x, y, z, in voxels")
    ap.add_argument("--device", type=int, default=0, help="GPU ordinal")
    args = ap.parse_args(argv)
    try:
        if args.fname_out == args.fname_mrc_orig:
            raise InputError("Error: Input and output image files cannot have the same name.\n")
        if args.voxel_width == 0.0:
            raise InputError("Error: voxel width cannot be non-zero\n")
        try:
            vertices, triangles = ply.read_ply(args.fname_mesh)
        except IOError:
            raise InputError('Error: Unable to open file "' + args.fname_mesh + '" for reading.\n')
        header = read_mrc_header(args.fname_mrc_orig) if args.fname_mrc_orig else None
        w, _bounds, n, origin, _from_file = plan(header, args.voxel_width, args.ibounds, args.bounds, args.shift)
        nb, nn = api.mesh_edges_host(triangles, len(vertices))
        if nb or nn:
            raise InputError("Error: The surface is not closed and manifold (%d boundary edges, %d non-manifold edges).\n"
                             % (nb, nn))
        ctx = api.Context(args.device)
        try:
            vol = ctx.voxelize_mesh(vertices, triangles, (n[2], n[1], n[0]), w, origin, check_closed=True)
        finally:
            ctx.close()
        if header is not None:
            write_mrc_bytes(args.fname_out, vol, header["cella"], header["cellb"], header["origin"])
        else:
            write_mrc_bytes(args.fname_out, vol, (w * n[0], w * n[1], w * n[2]))
    except (InputError, ValueError, api.VisfdHipError) as err:
        sys.stderr.write("\n" + str(err) + "\n")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
