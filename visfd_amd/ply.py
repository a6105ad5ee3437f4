"""A small PLY reader (and a minimal writer) for triangle meshes: formats ascii, binary_little_endian and
binary_big_endian; any extra vertex properties and any other elements are read past; the face list may be named
vertex_indices or vertex_index, with any integer types; polygons with more than 3 corners become fans from corner 0."""
import numpy as np

_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
          "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
          "double": "f8", "float64": "f8"}


class PlyError(ValueError):
    pass


def _header(f):
    if f.readline().strip() != b"ply":
        raise PlyError("not a PLY file")
    fmt, elements = None, []
    while True:
        line = f.readline()
        if not line:
            raise PlyError("PLY header without end_header")
        w = line.decode("ascii", "replace").split()
        if not w or w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property":
            if not elements:
                raise PlyError("PLY property before any element")
            if w[1] == "list":
                elements[-1][2].append((w[4], _TYPES[w[2]], _TYPES[w[3]]))
            else:
                elements[-1][2].append((w[2], None, _TYPES[w[1]]))
        elif w[0] == "end_header":
            break
    if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
        raise PlyError("unknown PLY format %r" % fmt)
    return fmt, elements


def _fans(polygons):
    t = []
    for p in polygons:
        for k in range(1, len(p) - 1):
            t.append((p[0], p[k], p[k + 1]))
    return np.asarray(t, np.int64).reshape(-1, 3)


def _read_ascii(f, elements):
    tok = f.read().split()
    pos, verts, polys = 0, None, []
    for name, count, props in elements:
        rows = []
        for _ in range(count):
            row = {}
            for pname, ctype, _t in props:
                if ctype is None:
                    row[pname] = tok[pos]
                    pos += 1
                else:
                    n = int(tok[pos])
                    row[pname] = tok[pos + 1:pos + 1 + n]
                    pos += 1 + n
            rows.append(row)
        if name == "vertex":
            verts = np.array([[float(r["x"]), float(r["y"]), float(r["z"])] for r in rows], np.float64).reshape(-1, 3)
        elif name == "face":
            key = [p[0] for p in props if p[0] in ("vertex_indices", "vertex_index")]
            if not key:
                raise PlyError("PLY face element without vertex_indices")
            polys = [[int(float(x)) for x in r[key[0]]] for r in rows]
    return verts, polys


def _read_binary(f, elements, order):
    verts, polys = None, []
    for name, count, props in elements:
        scalar = all(p[1] is None for p in props)
        if scalar:
            dt = np.dtype([(p[0], order + p[2]) for p in props])
            raw = f.read(dt.itemsize * count)
            if len(raw) != dt.itemsize * count:
                raise PlyError("PLY file ends inside element " + name)
            a = np.frombuffer(raw, dt)
            if name == "vertex":
                verts = np.stack([a["x"], a["y"], a["z"]], 1).astype(np.float64) if count else np.zeros((0, 3))
            continue
        is_face = name == "face"
        # the usual case first: one list property, three corners everywhere
        if len(props) == 1 and count:
            pname, ctype, itype = props[0]
            dt = np.dtype([("n", order + ctype), ("i", order + itype, (3,))])
            start = f.tell()
            raw = f.read(dt.itemsize * count)
            a = np.frombuffer(raw, dt) if len(raw) == dt.itemsize * count else None
            if a is not None and (a["n"] == 3).all():
                if is_face and pname in ("vertex_indices", "vertex_index"):
                    polys = a["i"].astype(np.int64).tolist()
                continue
            f.seek(start)
        for _ in range(count):
            for pname, ctype, itype in props:
                if ctype is None:
                    f.read(np.dtype(itype).itemsize)
                    continue
                cd, idt = np.dtype(order + ctype), np.dtype(order + itype)
                raw = f.read(cd.itemsize)
                if len(raw) != cd.itemsize:
                    raise PlyError("PLY file ends inside element " + name)
                n = int(np.frombuffer(raw, cd)[0])
                idx = np.frombuffer(f.read(idt.itemsize * n), idt)
                if len(idx) != n:
                    raise PlyError("PLY file ends inside element " + name)
                if is_face and pname in ("vertex_indices", "vertex_index"):
                    polys.append(idx.astype(np.int64).tolist())
    return verts, polys


def read_ply(path):
    """-> (vertices float32 (n, 3), triangles int32 (m, 3))"""
    with open(path, "rb") as f:
        fmt, elements = _header(f)
        for name, _count, props in elements:
            if name == "vertex" and not {"x", "y", "z"} <= {p[0] for p in props if p[1] is None}:
                raise PlyError("PLY vertex element without x, y, z")
        if fmt == "ascii":
            verts, polys = _read_ascii(f, elements)
        else:
            verts, polys = _read_binary(f, elements, "<" if fmt == "binary_little_endian" else ">")
    if verts is None:
        raise PlyError("PLY file without a vertex element")
    return verts.astype(np.float32), _fans(polys).astype(np.int32)


_NORMALS = ("nx", "ny", "nz")


def read_ply_points(path):
    """An oriented point cloud, such as filter_mrc -normals-file writes (ascii, vertex properties x y z nx ny nz): ->
    (xyz float32 (n, 3), normals float32 (n, 3)).  All three formats; other vertex properties and other elements are read
    past; a file whose vertices lack nx, ny or nz (a plain mesh) is refused with PlyError."""
    with open(path, "rb") as f:
        fmt, elements = _header(f)
        vertex = [e for e in elements if e[0] == "vertex"]
        if not vertex:
            raise PlyError("PLY file without a vertex element")
        names = {p[0] for p in vertex[0][2] if p[1] is None}
        if not {"x", "y", "z"} <= names:
            raise PlyError("PLY vertex element without x, y, z")
        if not set(_NORMALS) <= names:
            raise PlyError("PLY vertex element without the normals nx, ny, nz: not an oriented point cloud")
        cols = ("x", "y", "z") + _NORMALS
        if fmt == "ascii":
            tok = f.read().split()
            pos, out = 0, None
            for name, count, props in elements:
                if name == "vertex":
                    if any(p[1] is not None for p in props):
                        raise PlyError("PLY vertex element with a list property")
                    w = len(props)
                    if len(tok) < pos + w * count:
                        raise PlyError("PLY file ends inside element vertex")
                    try:
                        a = np.array([float(t) for t in tok[pos:pos + w * count]], np.float64).reshape(count, w)
                    except ValueError:
                        raise PlyError("PLY vertex element with a field that is not a number")
                    idx = [[p[0] for p in props].index(c) for c in cols]
                    out = a[:, idx]
                    break
                for _ in range(count):          # an element before the vertices: read past it
                    for pname, ctype, _t in props:
                        pos += 1 if ctype is None else 1 + int(tok[pos])
        else:
            order = "<" if fmt == "binary_little_endian" else ">"
            out = None
            for name, count, props in elements:
                if any(p[1] is not None for p in props):
                    if name == "vertex":
                        raise PlyError("PLY vertex element with a list property")
                    for _ in range(count):
                        for pname, ctype, itype in props:
                            if ctype is None:
                                f.read(np.dtype(itype).itemsize)
                            else:
                                cd = np.dtype(order + ctype)
                                raw = f.read(cd.itemsize)
                                if len(raw) != cd.itemsize:
                                    raise PlyError("PLY file ends inside element " + name)
                                f.read(np.dtype(itype).itemsize * int(np.frombuffer(raw, cd)[0]))
                    continue
                dt = np.dtype([(p[0], order + p[2]) for p in props])
                raw = f.read(dt.itemsize * count)
                if len(raw) != dt.itemsize * count:
                    raise PlyError("PLY file ends inside element " + name)
                if name == "vertex":
                    a = np.frombuffer(raw, dt)
                    out = np.stack([a[c] for c in cols], 1).astype(np.float64) if count else np.zeros((0, 6))
                    break
    out = out.reshape(-1, 6).astype(np.float32)
    return np.ascontiguousarray(out[:, :3]), np.ascontiguousarray(out[:, 3:])


def write_ply(path, vertices, faces, fmt="binary_little_endian", extra=(), index_name="vertex_indices", count_type="uchar",
              index_type="int"):
    """A minimal writer.  faces: a list of polygons (index lists).  extra: [(name, type, values per vertex)] written after
    x, y, z."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    order = ">" if fmt == "binary_big_endian" else "<"
    head = ["ply", "format %s 1.0" % fmt, "comment written by visfd_amd.ply", "element vertex %d" % len(v),
            "property float x", "property float y", "property float z"]
    head += ["property %s %s" % (t, n) for n, t, _a in extra]
    head += ["element face %d" % len(faces), "property list %s %s %s" % (count_type, index_type, index_name), "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        if fmt == "ascii":
            for i in range(len(v)):
                row = [repr(float(x)) for x in v[i]] + [repr(np.asarray(a)[i].item()) for _n, _t, a in extra]
                f.write((" ".join(row) + "\n").encode("ascii"))
            for p in faces:
                f.write((" ".join([str(len(p))] + [str(int(i)) for i in p]) + "\n").encode("ascii"))
            return
        dt = np.dtype([("x", order + "f4"), ("y", order + "f4"), ("z", order + "f4")] +
                      [(n, order + _TYPES[t]) for n, t, _a in extra])
        rec = np.zeros(len(v), dt)
        rec["x"], rec["y"], rec["z"] = v[:, 0], v[:, 1], v[:, 2]
        for n, _t, a in extra:
            rec[n] = np.asarray(a)
        f.write(rec.tobytes())
        cd, idt = np.dtype(order + _TYPES[count_type]), np.dtype(order + _TYPES[index_type])
        if isinstance(faces, np.ndarray) and faces.ndim == 2:   # an (m, k) array: the same bytes in one piece
            rows = np.zeros(len(faces), np.dtype([("n", cd), ("i", idt, (faces.shape[1],))]))
            rows["n"], rows["i"] = faces.shape[1], faces
            f.write(rows.tobytes())
            return
        for p in faces:
            f.write(np.asarray([len(p)], cd).tobytes() + np.asarray(p, idt).tobytes())
