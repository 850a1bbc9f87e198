"""Surface extraction: marching cubes on the GPU, mesh clean-up (connected components, floater removal), area-weighted surface
sampling and a PLY writer and reader.

The reference meshes a trained field inside its Open3D viewer (neddf/scripts/fields_visualizer.py:528-566: voxelize ->
PyMCubes -> .dae).  Here the grid evaluation and marching cubes are HIP kernels (include/neddf_hip.h neddf_field_grid,
neddf_marching_cubes); BaseNeuralField.extract_mesh and neddf/scripts/extract_mesh.py are built on this module.  A level set of a
trained field comes with small closed blobs in empty space and open shreds at the cube's faces: connected_components,
compact_mesh and remove_small_components drop them on the device (neddf_mesh_components, neddf_mesh_compact).  Marching cubes emits
triangles at the lattice's density whether the surface is flat or not: simplify_mesh merges the vertices of every cell of a coarser
grid on the device (neddf_mesh_simplify_*), in place of the decimation the reference's users ran in Open3D.
"""
import numpy as np
import torch

from ._lib import Context, NeddfError


def marching_cubes(volume, iso, lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0)):
    """Iso-surface of a float32 [nz, ny, nx] device volume sampled on the lattice lo .. hi (np.linspace per axis, x fastest).

    Returns (vertices float32 [V, 3] in world units (x, y, z), triangles int32 [T, 3]) on the volume's device: one vertex per
    lattice edge the surface crosses, in a fixed order (include/neddf_hip.h neddf_marching_cubes).  A sample is inside when
    it is below `iso`; NaN samples are outside.  Each triangle's normal (p1 - p0) x (p2 - p0) points from the inside
    (below iso) to the outside."""
    if not isinstance(volume, torch.Tensor) or not volume.is_cuda:
        raise NeddfError("marching_cubes: the volume must be a tensor on a HIP device (got %s)"
                         % (volume.device if isinstance(volume, torch.Tensor) else type(volume).__name__))
    if volume.dtype != torch.float32:
        raise NeddfError("marching_cubes: the volume must be float32 (got %s)" % volume.dtype)
    if volume.dim() != 3:
        raise NeddfError("marching_cubes: the volume must be [nz, ny, nx] (got %d dimensions)" % volume.dim())
    if min(volume.shape) < 2:
        raise NeddfError("marching_cubes: every dimension must be at least 2 (got %s)" % (tuple(volume.shape),))
    return Context.get(volume.device).marching_cubes(volume.contiguous(), iso, lo, hi)


def select_bricks(coarse, iso, band, dilate=0):
    """Bricks that can hold the `iso` level set, from the field's values at the brick corners: coarse float32 [nbz+1, nby+1, nbx+1]
    on a HIP device (Context.field_grid_coarse, or every brick-th sample of a dense volume and its last one per axis).

    A brick is active when one of its 8 corners is NaN, two of them lie on different sides of iso, or one is within `band` of it;
    the set is then grown by `dilate` bricks (0..4) in the Chebyshev sense.  For an L-Lipschitz field, band = L * half the brick's
    diagonal leaves out no brick the surface passes through.  Returns (slot_map int32 [nbz, nby, nbx]: the rank of each brick among
    the active ones or -1, brick_ids int32 [M]: the active brick indices (bz * nby + by) * nbx + bx, ascending), independent of
    timing (include/neddf_hip.h neddf_brick_select)."""
    _device_mesh("select_bricks", coarse=coarse)
    if coarse.dtype != torch.float32 or coarse.dim() != 3 or min(coarse.shape) < 2:
        raise NeddfError("select_bricks: a float32 [nbz+1, nby+1, nbx+1] volume of at least 2 points per axis expected (got %s %s)"
                         % (coarse.dtype, tuple(coarse.shape)))
    if not float(band) >= 0.0:
        raise NeddfError("select_bricks: the band must not be negative (got %r)" % (band,))
    if int(dilate) < 0 or int(dilate) > 4:
        raise NeddfError("select_bricks: dilate must lie in [0, 4] (got %r)" % (dilate,))
    return Context.get(coarse.device).brick_select(coarse.contiguous(), iso, band, dilate)


def marching_cubes_bricks(values, brick_ids, slot_map, shape, brick, iso, lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0), dense_order=True):
    """marching_cubes restricted to the listed bricks of `brick`^3 cells of the lattice shape = (nx, ny, nz) between lo and hi.

    values float32 [M, (brick + 1)^3]: the samples on each listed brick's lattice (x fastest, NaN past the fine lattice:
    Context.field_bricks); brick_ids int32 [M] strictly ascending; slot_map int32 [nbz, nby, nbx] its inverse (select_bricks).  The
    triangles are marching_cubes' triangles of the cells inside listed bricks and the vertices those they reference, bit for bit.
    dense_order=True: reordered on the device by the library's keys into marching_cubes' order -- whenever the listed bricks cover
    every cell the surface crosses, the result IS marching_cubes' mesh.  Returns (vertices, triangles).
    dense_order=False: the library's order (bricks ascending, then local index) and the keys:
    (vertices, triangles, vertex_key int64 [V], triangle_key int64 [T]) (include/neddf_hip.h neddf_marching_cubes_bricks)."""
    _device_mesh("marching_cubes_bricks", values=values, brick_ids=brick_ids, slot_map=slot_map)
    brick = int(brick)
    if len(tuple(shape)) != 3:
        raise NeddfError("marching_cubes_bricks: shape must be (nx, ny, nz) (got %r)" % (shape,))
    if values.dtype != torch.float32 or values.dim() != 2 or values.shape != (brick_ids.shape[0], (brick + 1) ** 3):
        raise NeddfError("marching_cubes_bricks: values must be float32 [M, (brick + 1)^3] (got %s %s for %d bricks of %d)"
                         % (values.dtype, tuple(values.shape), brick_ids.shape[0], brick))
    if brick_ids.dtype != torch.int32 or slot_map.dtype != torch.int32 or brick_ids.dim() != 1:
        raise NeddfError("marching_cubes_bricks: brick_ids [M] and slot_map must be int32")
    ctx = Context.get(values.device)
    if 2 <= brick <= 16 and min(int(n) for n in shape) >= 2:        # (otherwise the library reports what is wrong)
        nb = ctx.brick_counts(shape, brick)
        if tuple(slot_map.shape) != nb[::-1]:
            raise NeddfError("marching_cubes_bricks: slot_map must be [nbz, nby, nbx] = %s (got %s)" % (nb[::-1], tuple(slot_map.shape)))
    verts, tris, vkey, tkey = ctx.marching_cubes_bricks(values.contiguous(), brick_ids.contiguous(), slot_map.contiguous(), shape, brick,
                                                        iso, lo, hi)
    if not dense_order:
        return verts, tris, vkey, tkey
    return _dense_order(verts, tris, vkey, tkey)


def _dense_order(verts, tris, vkey, tkey):
    """Vertices sorted by their key, triangle corners renumbered, triangles sorted by theirs (the keys are unique)."""
    order = torch.sort(vkey).indices
    new_id = torch.empty(order.shape[0], device=order.device, dtype=torch.int32)
    new_id[order] = torch.arange(order.shape[0], device=order.device, dtype=torch.int32)
    tris = new_id[tris.long()] if tris.numel() else tris
    return verts[order].contiguous(), tris[torch.sort(tkey).indices].contiguous()


def vertex_normals(vertices, triangles):
    """Geometric vertex normals float32 [V, 3] of an indexed device mesh: the normalised, area-weighted sum of the incident
    triangles' cross products (p1 - p0) x (p2 - p0); a vertex whose sum vanishes gets (0, 0, 0).  Independent of timing
    (include/neddf_hip.h neddf_mesh_vertex_normals)."""
    if not isinstance(vertices, torch.Tensor) or not vertices.is_cuda:
        raise NeddfError("vertex_normals: the mesh must live on a HIP device")
    return Context.get(vertices.device).mesh_vertex_normals(vertices, triangles)


def _device_mesh(what, **tensors):
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise NeddfError("%s: %s must be a tensor on a HIP device (got %s)"
                             % (what, name, t.device if isinstance(t, torch.Tensor) else type(t).__name__))


def connected_components(triangles, n_vertices):
    """Connected components of an indexed device mesh (triangles int32 [T, 3] over n_vertices vertices): two vertices belong to
    one component when a chain of triangles sharing vertices joins them.

    Returns (vertex_label int32 [V], triangle_label int32 [T], component_triangles int64 [C]).  Components are numbered in the
    order of their lowest vertex index; a vertex no valid triangle references and a triangle with an index outside [0, V) get
    -1; component_triangles[c] counts the valid triangles of component c.  Independent of timing (include/neddf_hip.h
    neddf_mesh_components)."""
    _device_mesh("connected_components", triangles=triangles)
    return Context.get(triangles.device).mesh_components(triangles, n_vertices)


def compact_mesh(vertices, triangles, keep_triangle):
    """Drops the triangles whose keep_triangle [T] entry is zero (and those with an index outside [0, V)), then the vertices
    nothing references any more, and reindexes; both keep their relative order and the coordinates are copied bit for bit.

    Returns (vertices float32 [V', 3], triangles int32 [T', 3], vertex_map int32 [V]: the new index of every old vertex or -1)
    (include/neddf_hip.h neddf_mesh_compact)."""
    _device_mesh("compact_mesh", vertices=vertices, triangles=triangles, keep_triangle=keep_triangle)
    return Context.get(vertices.device).mesh_compact(vertices, triangles, keep_triangle)


def select_components(component_triangles, min_triangles=0, keep_largest=0):
    """bool [C]: the components with at least min_triangles triangles that, if keep_largest > 0, are also among the keep_largest
    largest by triangle count (ties go to the lower label)."""
    sizes = component_triangles
    keep = sizes >= int(min_triangles)
    if int(keep_largest) > 0 and sizes.numel() > int(keep_largest):
        order = torch.sort(sizes, descending=True, stable=True).indices        # stable: equal counts stay in label order
        top = torch.zeros_like(keep)
        top[order[:int(keep_largest)]] = True
        keep = keep & top
    return keep


def _clean(vertices, triangles, min_triangles, keep_largest):
    """remove_small_components plus what it did: {"components", "components_kept", "triangles_removed"}."""
    _device_mesh("remove_small_components", vertices=vertices, triangles=triangles)
    if int(min_triangles) < 0 or int(keep_largest) < 0:
        raise ValueError("remove_small_components: min_triangles and keep_largest must not be negative")
    _, tri_label, sizes = connected_components(triangles, vertices.shape[0])
    keep = select_components(sizes, min_triangles, keep_largest)
    if sizes.numel():
        keep_tri = ((tri_label >= 0) & keep[tri_label.clamp_min(0).long()]).to(torch.uint8)
    else:
        keep_tri = torch.zeros(triangles.shape[0], device=triangles.device, dtype=torch.uint8)
    out = compact_mesh(vertices, triangles, keep_tri)
    stats = {"components": int(sizes.numel()), "components_kept": int(keep.sum().item()),
             "triangles_removed": int(triangles.shape[0] - out[1].shape[0])}
    return out, stats


def remove_small_components(vertices, triangles, min_triangles=0, keep_largest=0):
    """Floater removal: keeps the connected components with at least min_triangles triangles and, if keep_largest > 0, only the
    keep_largest largest of them by triangle count (ties go to the lower label, i.e. the lower first vertex).  Triangles with an
    index outside [0, V) go too.  Labelling and compaction run in the library; the choice over the [C] counts is torch.

    Returns (vertices, triangles, vertex_map) as compact_mesh does."""
    return _clean(vertices, triangles, min_triangles, keep_largest)[0]


def simplify_grid(bounds_lo, bounds_hi, cell=None, cells=None):
    """The cell counts (gx, gy, gz) of simplify_mesh over a box: `cells` as given, or ceil(extent / cell) per axis and at least 1 for
    an edge length `cell` in world units.  NeddfError unless exactly one of the two is given and every axis gets 1 to 1024 cells."""
    if (cell is None) == (cells is None):
        raise NeddfError("simplify_mesh: exactly one of cell and cells must be given")
    if cells is None:
        if not (float(cell) > 0.0 and float(cell) < float("inf")):
            raise NeddfError("simplify_mesh: cell must be a positive edge length (got %r)" % (cell,))
        need = [(float(h) - float(l)) / float(cell) for l, h in zip(bounds_lo, bounds_hi)]
        if max(need) > 1024.0:
            raise NeddfError("simplify_mesh: a cell of %g needs more than 1024 cells along an axis (extent / cell = %s)" % (float(cell), need))
        cells = [max(1, int(np.ceil(x))) for x in need]
    cells = tuple(int(c) for c in cells)
    if len(cells) != 3 or min(cells) < 1 or max(cells) > 1024:
        raise NeddfError("simplify_mesh: cells must be three counts in [1, 1024] (got %r)" % (cells,))
    return cells


def simplify_mesh(vertices, triangles, cell=None, cells=None, box=None, placement="mean", regularisation=2 ** -10, attributes=None, timings=None):
    """Vertex clustering: a grid of `cells` = (gx, gy, gz) cells (or of cells with edge `cell`, in world units) is laid over `box` =
    (lo, hi) -- the bounds of the finite vertices when None -- the vertices of each cell become one vertex, and the triangles that
    collapse, and duplicates of a triangle, go (include/neddf_hip.h "mesh simplification" states every rule; tests/simplify_check.py
    restates it in numpy bit for bit; the same call gives the same bits on every run).

    placement "mean": the new vertex is the fp64 mean of the cell's vertices.  "quadric": the point that minimises the area-weighted
    squared distance to the planes of the triangles around the cell's vertices, regularised towards the mean by `regularisation`
    (a knob: 0 is legal) and clamped to the bounding box of the cell's vertices -- flat regions stay flat and edges stay sharp.
    attributes: a float32 [V, k] tensor (normals, colours) or a list of them, averaged per cell and not renormalised.

    Returns (vertices float32 [V', 3], triangles int32 [T', 3], vertex_map int32 [V]: the new index of every old vertex's cell or -1,
    triangle_map int32 [T]: the new index of every surviving triangle or -1[, attributes: as given, [V', k] each]).  Every new vertex
    lies within (1 + 2^-10) cell diagonals of the old vertices mapped to it, hence every point of the new surface that close to the
    old one; components smaller than a cell vanish.  With cells so fine that no two vertices share one, the mesh comes back unchanged.
    `timings` (a dict, optional) receives the wall time in seconds of "keys", "sort", "clusters", "placement", "triangles" and
    "compaction", each ending in a device synchronise."""
    import time
    from ._lib import SIMPLIFY_PLACEMENTS
    _device_mesh("simplify_mesh", vertices=vertices, triangles=triangles)
    if placement not in SIMPLIFY_PLACEMENTS:
        raise NeddfError("simplify_mesh: placement must be 'mean' or 'quadric' (got %r)" % (placement,))
    if vertices.device != triangles.device:
        raise NeddfError("simplify_mesh: vertices and triangles must live on one device (got %s, %s)" % (vertices.device, triangles.device))
    if vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise NeddfError("simplify_mesh: vertices must be float32 [V, 3] (got %s %s)" % (vertices.dtype, tuple(vertices.shape)))
    if not (float(regularisation) >= 0.0 and float(regularisation) < float("inf")):
        raise NeddfError("simplify_mesh: the regularisation must be finite and not negative (got %r)" % (regularisation,))
    single = isinstance(attributes, torch.Tensor)
    attrs = [] if attributes is None else ([attributes] if single else list(attributes))
    for a in attrs:
        _device_mesh("simplify_mesh", attributes=a)
        if a.dtype != torch.float32 or a.dim() != 2 or a.shape[0] != vertices.shape[0] or a.shape[1] < 1 or a.device != vertices.device:
            raise NeddfError("simplify_mesh: attributes must be float32 [V, k] on the mesh's device (got %s %s)" % (a.dtype, tuple(a.shape)))
    ctx = Context.get(vertices.device)
    v = vertices.contiguous()
    t = ctx._triangles(triangles, "simplify_mesh")
    if box is None:
        finite = v[torch.isfinite(v).all(dim=1)]
        if finite.shape[0]:
            lo, hi = finite.min(dim=0).values.double().tolist(), finite.max(dim=0).values.double().tolist()
        else:
            lo, hi = [0.0] * 3, [0.0] * 3
    else:
        lo, hi = [float(x) for x in box[0]], [float(x) for x in box[1]]
        if len(lo) != 3 or len(hi) != 3:
            raise NeddfError("simplify_mesh: box must be (lo, hi) of three coordinates each (got %r)" % (box,))
    cells = simplify_grid(lo, hi, cell, cells)
    marks = [time.perf_counter()]

    def mark():
        if timings is not None:
            torch.cuda.synchronize(v.device)
            marks.append(time.perf_counter())
    keys = ctx.mesh_simplify_keys(v, lo, hi, cells)
    mark()
    keys = torch.sort(keys).values                      # distinct keys: one order (plumbing, as bvh.py sorts its keys)
    mark()
    cluster, crange = ctx.mesh_simplify_clusters(keys)
    mark()
    pairs = None
    if placement == "quadric":
        pairs = torch.sort(ctx.mesh_simplify_pairs(v, t, cluster)).values
    rep = ctx.mesh_simplify_place(v, keys, crange, SIMPLIFY_PLACEMENTS[placement], regularisation, t, pairs)
    rep_attrs = [ctx.mesh_simplify_attributes(a.contiguous(), keys, crange) for a in attrs]
    mark()
    mapped, lowest, tkeys = ctx.mesh_simplify_triangles(t, v.shape[0], cluster)
    order = torch.sort(tkeys, stable=True).indices      # by (b, c), then by a: equal triples end up next to each other in index order
    order = order[torch.sort(lowest[order], stable=True).indices]
    keep = ctx.mesh_simplify_unique(lowest, tkeys, order.contiguous())
    mark()
    out_v, out_t, cmap = ctx.mesh_compact(rep, mapped, keep)
    vmap = cmap[cluster.long()] if v.shape[0] else torch.empty(0, device=v.device, dtype=torch.int32)
    tmap = torch.where(keep != 0, torch.cumsum(keep.to(torch.int32), 0, dtype=torch.int32) - 1, torch.full_like(keep, -1, dtype=torch.int32))
    out_attrs = [a[cmap >= 0].contiguous() for a in rep_attrs]
    mark()
    if timings is not None:
        for name, a, b in zip(("keys", "sort", "clusters", "placement", "triangles", "compaction"), marks[:-1], marks[1:]):
            timings[name] = b - a
    out = (out_v, out_t, vmap.contiguous(), tmap)
    if attributes is None:
        return out
    return out + ((out_attrs[0] if single else out_attrs),)


def _host(a, dtype):
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=dtype)


def write_ply(path, vertices, triangles, normals=None, colors=None):
    """Binary little-endian PLY: vertex (float x, y, z), face (list uchar int vertex_indices).
    normals [V, 3] append `property float nx, ny, nz`; colors [V, 3] -- floats in [0, 1] in the field's channel order, which is the
    dataset's B, G, R -- append `property uchar red, green, blue`: swapped to R, G, B, times 255, rounded half to even, clamped to
    [0, 255].  With both None the file is the plain 12-bytes-per-vertex one."""
    v = _host(vertices, "<f4")
    t = _host(triangles, "<i4")
    if v.ndim != 2 or v.shape[1] != 3 or t.ndim != 2 or t.shape[1] != 3:
        raise ValueError("write_ply: vertices [V, 3] and triangles [T, 3] expected (got %s, %s)" % (v.shape, t.shape))
    fields, props = [("p", "<f4", (3,))], "property float x\nproperty float y\nproperty float z\n"
    extra = {}
    if normals is not None:
        extra["n"] = _host(normals, "<f4")
        fields.append(("n", "<f4", (3,)))
        props += "property float nx\nproperty float ny\nproperty float nz\n"
    if colors is not None:
        c = _host(colors, np.float64)
        extra["c"] = np.clip(np.rint(np.nan_to_num(c[..., ::-1]) * 255.0), 0, 255).astype(np.uint8)       # np.rint: half to even; NaN -> 0
        fields.append(("c", "u1", (3,)))
        props += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    for k, a in extra.items():
        if a.shape != v.shape:
            raise ValueError("write_ply: normals / colors must be [V, 3] like the vertices (got %s)" % (a.shape,))
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n%s"
            "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), props, len(t)))
    if extra:
        rec = np.empty(len(v), dtype=np.dtype(fields))
        rec["p"] = v
        for k, a in extra.items():
            rec[k] = a
        vbytes = rec.tobytes()
    else:
        vbytes = v.tobytes()
    faces = np.empty(len(t), dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    faces["n"] = 3
    faces["i"] = t
    with open(path, "wb") as fh:
        fh.write(head.encode("ascii"))
        fh.write(vbytes)
        fh.write(faces.tobytes())
    return path


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply(path, properties=False):
    """(vertices float32 [V, 3], triangles int32 [T, 3]) as numpy arrays from a PLY file with the elements write_ply produces: `vertex`
    with scalar properties among which x, y, z (normals, colours and others are skipped) and `face` with one list property of 3 indices
    per face -- binary little-endian, as write_ply writes its three variants, or ASCII.  ValueError on anything else.
    properties=True: (vertices, triangles, normals, colors) -- normals float32 [V, 3] from nx, ny, nz and colors float32 [V, 3] from red,
    green, blue as write_ply takes them (B, G, R order, value / 255 for an integer property), each None when the file lacks it."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError("read_ply: %s is not a PLY file (no `ply` magic or no end_header)" % path)
    lines = [ln.split() for ln in data[:end].decode("ascii", "replace").splitlines()[1:] if ln.strip() and not ln.startswith(("comment", "obj_info"))]
    body = data[end + len(b"end_header\n"):]
    if not lines or lines[0][:1] != ["format"] or len(lines[0]) != 3 or lines[0][1] not in ("binary_little_endian", "ascii"):
        raise ValueError("read_ply: %s: format binary_little_endian or ascii expected (got %r)" % (path, " ".join(lines[0]) if lines else ""))
    binary = lines[0][1] == "binary_little_endian"
    elements = []                                       # [name, count, [(property name, scalar type) or (name, count type, item type)]]
    for ln in lines[1:]:
        try:
            if ln[0] == "element" and len(ln) == 3:
                elements.append([ln[1], int(ln[2]), []])
            elif ln[0] == "property" and elements and len(ln) == 3:
                elements[-1][2].append((ln[2], _PLY_TYPES[ln[1]]))
            elif ln[0] == "property" and elements and len(ln) == 5 and ln[1] == "list":
                elements[-1][2].append((ln[4], _PLY_TYPES[ln[2]], _PLY_TYPES[ln[3]]))
            else:
                raise KeyError(ln[0])
        except (KeyError, ValueError):
            raise ValueError("read_ply: %s: header line %r not understood" % (path, " ".join(ln))) from None
    if [e[0] for e in elements] != ["vertex", "face"] or min(e[1] for e in elements) < 0:
        raise ValueError("read_ply: %s: the elements `vertex` then `face` expected (got %s)" % (path, [e[0] for e in elements]))
    (_, nv, vprops), (_, nf, fprops) = elements
    names = [p[0] for p in vprops]
    if any(len(p) != 2 for p in vprops) or any(k not in names for k in "xyz") or len(set(names)) != len(names):
        raise ValueError("read_ply: %s: the vertex element needs scalar properties x, y, z (got %s)" % (path, names))
    if len(fprops) != 1 or len(fprops[0]) != 3 or fprops[0][1][0] == "f" or fprops[0][2][0] == "f":
        raise ValueError("read_ply: %s: the face element needs exactly one list property of integer indices" % path)
    if binary:
        vdt = np.dtype([(n, "<" + t) for n, t in vprops])
        fdt = np.dtype([("n", "<" + fprops[0][1]), ("i", "<" + fprops[0][2], (3,))])
        need = nv * vdt.itemsize + nf * fdt.itemsize
        if len(body) < need:
            raise ValueError("read_ply: %s is truncated: %d bytes of data, %d needed for %d vertices and %d triangles" % (path, len(body), need, nv, nf))
        rec = np.frombuffer(body, dtype=vdt, count=nv)
        faces = np.frombuffer(body, dtype=fdt, count=nf, offset=nv * vdt.itemsize)
        if nf and (faces["n"] != 3).any():
            raise ValueError("read_ply: %s: only triangles are supported (a face with %d vertices found)" % (path, int(faces["n"][faces["n"] != 3][0])))
        verts = np.stack([rec[k].astype(np.float32) for k in "xyz"], axis=1) if nv else np.zeros((0, 3), np.float32)
        tris = faces["i"].astype(np.int32)

        def column(k):
            return rec[k].astype(np.float32)
    else:
        rows = body.decode("ascii", "replace").split("\n")
        rows = [r.split() for r in rows if r.strip()]
        if len(rows) < nv + nf:
            raise ValueError("read_ply: %s is truncated: %d data lines, %d needed" % (path, len(rows), nv + nf))
        try:
            col = [names.index(k) for k in "xyz"]
            if any(len(r) != len(names) for r in rows[:nv]):
                raise ValueError("a vertex line with the wrong number of values")
            verts = np.array([[float(r[c]) for c in col] for r in rows[:nv]], np.float32).reshape(nv, 3)

            def column(k):
                return np.array([float(r[names.index(k)]) for r in rows[:nv]], np.float32)
            if any(len(r) != 4 or int(r[0]) != 3 for r in rows[nv:nv + nf]):
                raise ValueError("only triangles `3 i j k` are supported")
            tris = np.array([[int(x) for x in r[1:]] for r in rows[nv:nv + nf]], np.int64).reshape(nf, 3).astype(np.int32)
        except ValueError as e:
            raise ValueError("read_ply: %s: %s" % (path, e)) from None
    verts, tris = np.ascontiguousarray(verts), np.ascontiguousarray(tris.reshape(nf, 3))
    if not properties:
        return verts, tris
    normals = colors = None
    if all(k in names for k in ("nx", "ny", "nz")):
        normals = np.stack([column(k) for k in ("nx", "ny", "nz")], axis=1).reshape(nv, 3)
    if all(k in names for k in ("red", "green", "blue")):
        types = dict(vprops)
        colors = np.stack([column(k) / np.float32(1.0 if types[k][0] == "f" else 255.0) for k in ("blue", "green", "red")], axis=1).reshape(nv, 3)
    return verts, tris, normals, colors


def surface_area(vertices, triangles):
    """The total area of a device mesh as a Python float: a torch fp64 sum over the triangles with every index in [0, V) (plumbing: it
    turns sample_surface's `n` into a density and is not part of the bit-checked path)."""
    t = triangles.long()
    ok = ((t >= 0) & (t < vertices.shape[0])).all(dim=1)
    p = vertices.double()[t[ok]]
    a = 0.5 * torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]).norm(dim=1)
    return float(a[torch.isfinite(a)].sum().item())


def sample_surface(vertices, triangles, density=None, n=None, seed=0):
    """Area-weighted random points on a device mesh: (points float32 [N, 3], triangle_id int32 [N]), triangle-major
    (include/neddf_hip.h neddf_mesh_sample_count / neddf_mesh_sample_write).

    Exactly one of `density` (samples per unit area) and `n` is given.  Triangle t receives floor(A_t * density + u_t) samples, u_t
    uniform in [0, 1) -- A_t * density on average -- so with `n` (turned into density = n / total area) the number of points returned
    is CLOSE to n, not equal to it.  The points are a pure function of the mesh, the density and `seed`: the same call gives the same
    bits on every run; triangles with an index outside [0, V), a non-finite vertex or no area receive none."""
    _device_mesh("sample_surface", vertices=vertices, triangles=triangles)
    if (density is None) == (n is None):
        raise NeddfError("sample_surface: exactly one of density and n must be given")
    if vertices.device != triangles.device:
        raise NeddfError("sample_surface: vertices and triangles must live on one device (got %s, %s)" % (vertices.device, triangles.device))
    if vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise NeddfError("sample_surface: vertices must be float32 [V, 3] (got %s %s)" % (vertices.dtype, tuple(vertices.shape)))
    if not 0 <= int(seed) < 2 ** 32:
        raise NeddfError("sample_surface: the seed must fit 32 bits (got %r)" % (seed,))
    if n is not None:
        if int(n) < 0:
            raise NeddfError("sample_surface: n must not be negative (got %r)" % (n,))
        area = surface_area(vertices, triangles)
        density = int(n) / area if area > 0.0 else 0.0
    density = float(density)
    if not (density >= 0.0 and density < float("inf")):
        raise NeddfError("sample_surface: the density must be finite and not negative (got %r)" % (density,))
    ctx = Context.get(vertices.device)
    v = vertices.contiguous()
    count = ctx.mesh_sample_count(v, triangles, density, seed)
    return ctx.mesh_sample_write(v, triangles, density, seed, count)


__all__ = ["marching_cubes", "select_bricks", "marching_cubes_bricks", "vertex_normals", "connected_components", "compact_mesh", "remove_small_components", "write_ply",
           "read_ply", "sample_surface", "surface_area", "simplify_grid", "simplify_mesh"]
