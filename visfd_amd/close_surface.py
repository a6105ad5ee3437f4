"""python -m visfd_amd.close_surface: an oriented point cloud (the PLY file filter_mrc -normals-file writes) closed into a
0/1 image on the GPU, for the next run's -mask: the step the reference's Example 3 leaves to SSDRecon / PoissonRecon, meshlab
and voxelize_mesh.py.  The mask is what Context.close_surface defines (include/visfd_hip.h): the normals
spread onto the grid, a Poisson equation solved there, the solution cut at the level it takes on the points.

    python -m visfd_amd.close_surface -p CLOUD.ply -o MASK.rec [-i IMAGE.rec] [-w W] [--image-size NX NY NZ] [--pad P]
                                      [--orientation outward|inward|auto] [--chi CHI.rec] [--mesh MESH.ply [--mesh-level V]]

--mesh also writes the surface of the mask as a closed triangle mesh (Context.isosurface_dev): the field cut
at the level and on the side the mask was cut at, in physical units, so that python -m visfd_amd.voxelize_mesh gives the mask
back from it voxel for voxel.  --mesh-level cuts the mesh at another value of the field (see it with --chi).

The cloud is in physical units; it is divided by the voxel width, which comes from -w or from the header of -i, exactly as
python -m visfd_amd.voxelize_mesh takes it.  The image size comes from -i or from --image-size.  The mask is an MRC file of
mode 0 (bytes 0 and 1); --chi writes the field that was cut as floats (mode 2), for choosing --pad and the orientation by eye."""
import argparse
import sys

import numpy as np

from . import api, ply
from .voxelize_mesh import InputError, plan, read_mrc_header, write_mrc_bytes


def plan_cloud(header=None, width=None, image_size=None):
    """The tool's arithmetic -> (w, (nx, ny, nz)).  The voxel width is voxelize_mesh.plan's: -w, else cella / m of the
    header, else 1; the size is --image-size, else the header's."""
    if image_size is not None:
        n = tuple(int(s) for s in image_size)
        if header is None:
            w = 1.0 if width is None else width
            if w == 0.0:
                raise InputError("Error: voxel width cannot be zero\n")
            return float(w), n
        w = plan(header, width)[0]
        return w, n
    if header is None:
        raise InputError("Error: the image size is unknown: use -i or --image-size\n")
    w, _bounds, n, _origin, _from_file = plan(header, width)
    return w, n


def write_mrc_floats(path, vol, cella, cellb=(90.0, 90.0, 90.0), origin=(0.0, 0.0, 0.0)):
    """vol [nz, ny, nx] float32 as an MRC2014 file of mode 2"""
    nz, ny, nx = vol.shape
    data = np.ascontiguousarray(vol, "<f4")
    h = np.zeros(256, "<i4")
    hf = h.view("<f4")
    h[0:3] = (nx, ny, nz)
    h[3] = 2
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


def close_and_mesh(ctx, points, normals, shape, pad, orientation, mesh_level=None, want_chi=False, device=0):
    """close_surface and the isosurface of its field on device tensors: the field stays on the device between the two.
    -> (mask, chi or None, close_surface_last(), (vertices in voxel coordinates, triangles, level, capped)).  The mesh is cut
    at the level and on the side the mask was cut at, so that voxelising it gives the mask back; mesh_level moves the level."""
    import torch
    dev = torch.device("cuda", device)
    p = torch.from_numpy(np.ascontiguousarray(points, np.float32).reshape(-1, 3)).to(dev)
    m = torch.from_numpy(np.ascontiguousarray(normals, np.float32).reshape(-1, 3)).to(dev)
    mask = torch.empty(shape, dtype=torch.float32, device=dev)
    chi = torch.empty(shape, dtype=torch.float32, device=dev)
    ctx.close_surface_dev(mask, p, m, pad, orientation, chi=chi)
    last = ctx.close_surface_last()
    level = last["iso"] if mesh_level is None else float(mesh_level)
    v, t = ctx.isosurface_dev(chi, level, "below" if last["orientation"] == "outward" else "above")
    capped = ctx.isosurface_last()["capped"]
    return (mask.cpu().numpy(), chi.cpu().numpy() if want_chi else None, last,
            (v.cpu().numpy(), t.cpu().numpy(), level, capped))


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m visfd_amd.close_surface")
    ap.add_argument("-p", "--points", dest="fname_cloud", required=True, help='the oriented point cloud (a ".ply" file)')
    ap.add_argument("-o", "--out", dest="fname_out", required=True, help="the output mask (mrc/rec format, bytes 0 and 1)")
    ap.add_argument("-i", "--in", dest="fname_mrc_orig", help="an MRC (or REC) file with the size of the target")
    ap.add_argument("-w", "--width", dest="voxel_width", type=float, help="the voxel width (default: the -i file's, else 1)")
    ap.add_argument("--image-size", dest="image_size", type=int, nargs=3, metavar=("NX", "NY", "NZ"))
    ap.add_argument("--pad", type=int, default=0, help="nodes the solve's box extends beyond the image on every face")
    ap.add_argument("--orientation", choices=("outward", "inward", "auto"), default="auto",
                    help="where the normals point (default: auto)")
    ap.add_argument("--chi", dest="fname_chi", help="also write the field that was cut (mrc/rec format, floats)")
    ap.add_argument("--mesh", dest="fname_mesh", help='also write the surface of the mask as a closed triangle mesh (a ".ply" file)')
    ap.add_argument("--mesh-level", dest="mesh_level", type=float, metavar="V",
                    help="cut the mesh at this value of the field instead of the level the mask was cut at")
    ap.add_argument("--device", type=int, default=0, help="GPU ordinal")
    args = ap.parse_args(argv)
    try:
        if args.fname_out == args.fname_mrc_orig or (args.fname_chi and args.fname_chi in (args.fname_out, args.fname_mrc_orig)):
            raise InputError("Error: Input and output image files cannot have the same name.\n")
        if args.fname_mesh and args.fname_mesh in (args.fname_cloud, args.fname_out, args.fname_mrc_orig, args.fname_chi):
            raise InputError("Error: the mesh file cannot have the name of another file of this run.\n")
        if args.mesh_level is not None and not args.fname_mesh:
            raise InputError("Error: --mesh-level needs --mesh\n")
        if args.voxel_width == 0.0:
            raise InputError("Error: voxel width cannot be zero\n")
        try:
            xyz, normals = ply.read_ply_points(args.fname_cloud)
        except IOError:
            raise InputError('Error: Unable to open file "' + args.fname_cloud + '" for reading.\n')
        header = read_mrc_header(args.fname_mrc_orig) if args.fname_mrc_orig else None
        w, n = plan_cloud(header, args.voxel_width, args.image_size)
        points = (xyz.astype(np.float64) / w).astype(np.float32)
        ctx = api.Context(args.device)
        mesh = None
        try:
            if args.fname_mesh:
                mask, chi, last, mesh = close_and_mesh(ctx, points, normals, (n[2], n[1], n[0]), args.pad, args.orientation,
                                                       args.mesh_level, bool(args.fname_chi), args.device)
            else:
                out = ctx.close_surface(points, normals, (n[2], n[1], n[0]), args.pad, args.orientation,
                                        want_chi=bool(args.fname_chi))
                mask, chi = out if args.fname_chi else (out, None)
                last = ctx.close_surface_last()
        finally:
            ctx.close()
        same_grid = header is not None and tuple(header["n"]) == n
        cell = (header["cella"], header["cellb"], header["origin"]) if same_grid else ((w * n[0], w * n[1], w * n[2]),)
        write_mrc_bytes(args.fname_out, mask, *cell)
        if chi is not None:
            write_mrc_floats(args.fname_chi, chi, *cell)
        if mesh is not None:
            # voxel coordinates to the units python -m visfd_amd.voxelize_mesh reads: the product in double, rounded to float
            ply.write_ply(args.fname_mesh, (mesh[0].astype(np.float64) * np.float64(w)).astype(np.float32), mesh[1])
            sys.stderr.write("close_surface: mesh of %d vertices and %d triangles at level %.9g%s\n" % (
                len(mesh[0]), len(mesh[1]), mesh[2], "; the image border cut the solid, the mesh is capped there" if mesh[3] else ""))
        sys.stderr.write("close_surface: %d points used, %d skipped; %d cycles, residual %.2e (%s); normals point %s%s\n" % (
            last["n_used"], last["n_skipped"], last["cycles"], last["ratio"],
            "cycle cap reached" if last["stop"] == api.CLOSE_STOP_CAP else "converged" if last["stop"] == api.CLOSE_STOP_RTOL
            else "nothing to solve", last["orientation"],
            "; the mask touches the image border (consider --pad)" if last["touches_face"] else ""))
    except (InputError, ValueError, api.VisfdHipError) as err:
        sys.stderr.write("\n" + str(err) + "\n")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
