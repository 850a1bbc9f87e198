"""Host restatement of mesh simplification by vertex clustering (include/neddf_hip.h, "mesh simplification"), written from the
definitions there: keys, clusters, both placements, attributes, the triangle rule and the maps, in numpy with the same operation
order, so that the device results can be held to it bit for bit.  Sequential sums are np.add.at over indices in member (or
pair) order: ufunc.at is unbuffered and applies its operands one after the other.  Also the small meshes the simplification tests
share."""
import math

import numpy as np

NONFINITE = np.int64(1) << np.int64(62)
CANONICAL_NAN = np.uint32(0x7fc00000)


# ---- the grid ------------------------------------------------------------------------------------------------------------------
def default_box(vertices):
    """The bounds of the finite vertices as Python doubles; (0, 0, 0) twice when there is none."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    fin = v[np.isfinite(v).all(axis=1)]
    if not len(fin):
        return [0.0] * 3, [0.0] * 3
    return [float(x) for x in fin.min(axis=0)], [float(x) for x in fin.max(axis=0)]


def grid_cells(lo, hi, cell):
    """ceil(extent / cell) per axis, at least 1."""
    return tuple(max(1, int(math.ceil((float(h) - float(l)) / float(cell)))) for l, h in zip(lo, hi))


def axis_cell(p, lo, hi, n):
    """neddf_nn_grid_build's cell function along one axis: p float32 [N] -> int64 [N]."""
    lo32 = np.float32(lo)
    ext = float(hi) - float(lo)
    inv = np.float32(float(n) / ext) if ext > 0.0 else np.float32(0.0)
    with np.errstate(all="ignore"):
        f = ((p - lo32).astype(np.float32) * inv).astype(np.float32)
        whole = np.where(f > 0, f, np.float32(0)).astype(np.int64)          # truncation of a positive float
    return np.where(f >= np.float32(n), n - 1, whole).astype(np.int64)


def keys(vertices, lo, hi, cells):
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    idx = np.arange(len(v), dtype=np.int64)
    fin = np.isfinite(v).all(axis=1)
    safe = np.where(fin[:, None], v, np.float32(0))
    cx, cy, cz = (axis_cell(safe[:, a], lo[a], hi[a], cells[a]) for a in range(3))
    cell = (cz * cells[1] + cy) * cells[0] + cx
    return np.where(fin, (cell << np.int64(32)) | idx, NONFINITE | idx).astype(np.int64)


# ---- clusters ------------------------------------------------------------------------------------------------------------------
def clusters(sorted_keys):
    """(vertex_cluster int32 [V], cluster_range int32 [C, 2]) from the keys sorted ascending."""
    k = np.asarray(sorted_keys, np.int64)
    V = len(k)
    if V == 0:
        return np.zeros(0, np.int32), np.zeros((0, 2), np.int32)
    vertex = k & np.int64(0xffffffff)
    head = np.ones(V, bool)
    head[1:] = ((k[1:] >> np.int64(32)) != (k[:-1] >> np.int64(32))) | ((k[1:] & NONFINITE) != 0)
    run = np.cumsum(head) - 1
    start = np.flatnonzero(head)
    end = np.append(start[1:], V)
    head_vertex = vertex[start]                         # the lowest vertex index of each run
    cid_of_run = np.empty(len(start), np.int64)
    cid_of_run[np.argsort(head_vertex, kind="stable")] = np.arange(len(start))      # numbered in the order of the heads
    vertex_cluster = np.empty(V, np.int32)
    vertex_cluster[vertex] = cid_of_run[run]
    cluster_range = np.empty((len(start), 2), np.int32)
    cluster_range[cid_of_run, 0] = start
    cluster_range[cid_of_run, 1] = end
    return vertex_cluster, cluster_range


def _members(sorted_keys, cluster_range):
    """(the vertex of every sorted position, its cluster, the member count of every cluster)."""
    k = np.asarray(sorted_keys, np.int64)
    vertex = k & np.int64(0xffffffff)
    count = (cluster_range[:, 1] - cluster_range[:, 0]).astype(np.int64)
    cl = np.empty(len(k), np.int64)
    order = np.argsort(cluster_range[:, 0], kind="stable")          # clusters by their position among the sorted keys
    cl[:] = np.repeat(order, count[order])
    return vertex, cl, count


def valid_triangles(vertices, triangles):
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    ok = ((t >= 0) & (t < len(v))).all(axis=1)
    fin = np.isfinite(v).all(axis=1)
    ok[ok] = fin[t[ok]].all(axis=1)
    return ok


def pairs(vertices, triangles, vertex_cluster):
    """cluster << 32 | triangle for every distinct corner cluster of every valid triangle, triangle-major, corners in order."""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    ok = valid_triangles(vertices, triangles)
    if not ok.any():
        return np.zeros(0, np.int64)
    tid = np.flatnonzero(ok).astype(np.int64)
    c = vertex_cluster.astype(np.int64)[t[ok]]
    take = np.stack([np.ones(len(c), bool), c[:, 1] != c[:, 0], (c[:, 2] != c[:, 0]) & (c[:, 2] != c[:, 1])], axis=1)
    key = (c << np.int64(32)) | tid[:, None]
    return key[take].astype(np.int64)                   # row-major: triangle-major, corner order inside


# ---- placement ---------------------------------------------------------------------------------------------------------------
def _mean64(values, vertex, cl, count):
    """fp64 sums from +0.0 in member order, divided by the count: [C, k]."""
    s = np.zeros((len(count), values.shape[1]), np.float64)
    np.add.at(s, cl, values[vertex].astype(np.float64))
    with np.errstate(all="ignore"):
        return s / count.astype(np.float64)[:, None]


def place(vertices, sorted_keys, cluster_range, placement="mean", regularisation=2.0 ** -10, triangles=None, sorted_pairs=None):
    """float32 [C, 3]: the representative of every cluster."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    C = len(cluster_range)
    out = np.zeros((C, 3), np.float32)
    if C == 0:
        return out
    vertex, cl, count = _members(sorted_keys, cluster_range)
    single = count == 1
    first = vertex[cluster_range[:, 0]]
    m = _mean64(v, vertex, cl, count)
    x = m.copy()
    if placement == "quadric":
        v64 = v.astype(np.float64)
        lo = np.full((C, 3), np.inf)
        hi = np.full((C, 3), -np.inf)
        np.minimum.at(lo, cl, v64[vertex])
        np.maximum.at(hi, cl, v64[vertex])
        p = np.asarray(sorted_pairs, np.int64)
        pc, pt = p >> np.int64(32), p & np.int64(0xffffffff)
        t = np.asarray(triangles, np.int64).reshape(-1, 3)[pt]
        with np.errstate(all="ignore"):
            p0, p1, p2 = v64[t[:, 0]], v64[t[:, 1]], v64[t[:, 2]]
            u, w = p1 - p0, p2 - p0
            nx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
            ny = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
            nz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
            A = {k: np.zeros(C) for k in ("00", "01", "02", "11", "12", "22")}
            for k, val in (("00", nx * nx), ("01", nx * ny), ("02", nx * nz), ("11", ny * ny), ("12", ny * nz), ("22", nz * nz)):
                np.add.at(A[k], pc, val)
            mm = m[pc]
            d = (nx * (p0[:, 0] - mm[:, 0]) + ny * (p0[:, 1] - mm[:, 1])) + nz * (p0[:, 2] - mm[:, 2])
            r = [np.zeros(C) for _ in range(3)]
            for a, n in enumerate((nx, ny, nz)):
                np.add.at(r[a], pc, n * d)
            a00, a01, a02, a11, a12, a22 = (A[k] for k in ("00", "01", "02", "11", "12", "22"))
            tr = (a00 + a11) + a22
            lam = (np.float64(regularisation) * tr) / 3.0
            b00, b11, b22 = a00 + lam, a11 + lam, a22 + lam
            c00 = b11 * b22 - a12 * a12
            c01 = a02 * a12 - a01 * b22
            c02 = a01 * a12 - a02 * b11
            c11 = b00 * b22 - a02 * a02
            c12 = a01 * a02 - b00 * a12
            c22 = b00 * b11 - a01 * a01
            det = (b00 * c00 + a01 * c01) + a02 * c02
            y0 = ((c00 * r[0] + c01 * r[1]) + c02 * r[2]) / det
            y1 = ((c01 * r[0] + c11 * r[1]) + c12 * r[2]) / det
            y2 = ((c02 * r[0] + c12 * r[1]) + c22 * r[2]) / det
            ok = (tr != 0) & np.isfinite(tr) & (det != 0) & np.isfinite(det) & np.isfinite(y0) & np.isfinite(y1) & np.isfinite(y2)
            y = np.stack([y0, y1, y2], axis=1)
            x = np.where(ok[:, None], m + y, m)
            x = np.minimum(np.maximum(x, lo), hi)
    with np.errstate(all="ignore"):
        out = x.astype(np.float32)
    out.view(np.uint32)[single] = v.view(np.uint32)[first[single]]          # a singleton, non-finite ones included: its own bits
    return out


def attribute_means(attr, sorted_keys, cluster_range):
    """float32 [C, k]: a singleton's bits, otherwise the fp64 ordered mean rounded once, a NaN written as 0x7fc00000."""
    a = np.ascontiguousarray(attr, np.float32)
    C = len(cluster_range)
    if C == 0:
        return np.zeros((0, a.shape[1]), np.float32)
    vertex, cl, count = _members(sorted_keys, cluster_range)
    with np.errstate(all="ignore"):
        out = _mean64(a, vertex, cl, count).astype(np.float32)
    out.view(np.uint32)[np.isnan(out)] = CANONICAL_NAN
    single = count == 1
    out.view(np.uint32)[single] = a.view(np.uint32)[vertex[cluster_range[:, 0]][single]]
    return out


# ---- triangles ---------------------------------------------------------------------------------------------------------------
def mapped_triangles(triangles, n_vertices, vertex_cluster):
    """(mapped int32 [T, 3]: the corner clusters in corner order, rotated int32 [T, 3]: the same with the lowest first (cyclic) -- the
    triangle's identity); (-1, -1, -1) in both for a dropped triangle."""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    ok = ((t >= 0) & (t < n_vertices)).all(axis=1)
    c = np.full((len(t), 3), -1, np.int64)
    if ok.any():
        c[ok] = vertex_cluster.astype(np.int64)[t[ok]]
    ok &= (c[:, 0] != c[:, 1]) & (c[:, 1] != c[:, 2]) & (c[:, 0] != c[:, 2])
    shift = np.argmin(np.where(ok[:, None], c, 0), axis=1)
    rows = np.arange(len(t))
    rot = np.stack([c[rows, (shift + k) % 3] for k in range(3)], axis=1) if len(t) else c
    return np.where(ok[:, None], c, -1).astype(np.int32), np.where(ok[:, None], rot, -1).astype(np.int32)


def unique_triangles(canon):
    """uint8 [T]: among the triangles with one triple only the lowest index is kept; dropped ones never."""
    T = len(canon)
    keep = np.zeros(T, np.uint8)
    if T == 0:
        return keep
    order = np.lexsort((np.arange(T), canon[:, 2], canon[:, 1], canon[:, 0]))
    s = canon[order]
    first = np.ones(T, bool)
    first[1:] = (s[1:] != s[:-1]).any(axis=1)
    keep[order] = first & (s[:, 0] >= 0)
    return keep


def compact(rep, mapped, keep):
    """Clusters no kept triangle references go; the rest and the kept triangles keep their order: (vertices, triangles, cluster_map)."""
    kept = mapped[keep != 0]
    used = np.zeros(len(rep), bool)
    used[kept.reshape(-1)] = True
    cmap = np.where(used, np.cumsum(used) - 1, -1).astype(np.int32)
    return rep[used], cmap[kept].astype(np.int32).reshape(-1, 3), cmap


def simplify(vertices, triangles, cell=None, cells=None, box=None, placement="mean", regularisation=2.0 ** -10, attributes=None):
    """mesh.simplify_mesh on the host: (vertices, triangles, vertex_map, triangle_map[, attributes])."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
    assert (cell is None) != (cells is None) and placement in ("mean", "quadric")
    lo, hi = default_box(v) if box is None else ([float(x) for x in box[0]], [float(x) for x in box[1]])
    if cells is None:
        cells = grid_cells(lo, hi, cell)
    k = np.sort(keys(v, lo, hi, cells))
    cluster, crange = clusters(k)
    sp = np.sort(pairs(v, t, cluster)) if placement == "quadric" else None
    rep = place(v, k, crange, placement, regularisation, t, sp)
    mapped, rotated = mapped_triangles(t, len(v), cluster)
    keep = unique_triangles(rotated)
    ov, ot, cmap = compact(rep, mapped, keep)
    vmap = cmap[cluster].astype(np.int32) if len(v) else np.zeros(0, np.int32)
    tmap = np.where(keep != 0, np.cumsum(keep != 0) - 1, -1).astype(np.int32)
    out = (ov, ot, vmap, tmap)
    if attributes is None:
        return out
    single = isinstance(attributes, np.ndarray)
    res = [attribute_means(a, k, crange)[cmap >= 0] for a in ([attributes] if single else attributes)]
    return out + ((res[0] if single else res),)


# ---- meshes ------------------------------------------------------------------------------------------------------------------
def uv_sphere(n_lat=12, n_lon=16, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """A closed UV sphere: 2 + (n_lat - 1) n_lon vertices, 2 n_lon (n_lat - 1) triangles, normals outward."""
    v = [(0.0, 0.0, 1.0)]
    for i in range(1, n_lat):
        th = math.pi * i / n_lat
        for j in range(n_lon):
            ph = 2.0 * math.pi * j / n_lon
            v.append((math.sin(th) * math.cos(ph), math.sin(th) * math.sin(ph), math.cos(th)))
    v.append((0.0, 0.0, -1.0))
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon          # noqa: E731
    t = []
    for j in range(n_lon):
        t.append((0, ring(1, j), ring(1, j + 1)))
        t.append((len(v) - 1, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)))
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            t.append((ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)))
            t.append((ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)))
    v = (np.array(v, np.float64) * radius + np.array(centre, np.float64)).astype(np.float32)
    return v, np.array(t, np.int32)


def triangle_soup(n_vertices, n_triangles, seed=0, scale=1.0):
    rng = np.random.default_rng(seed)
    v = (rng.random((n_vertices, 3)) * scale).astype(np.float32)
    t = rng.integers(0, n_vertices, (n_triangles, 3)).astype(np.int32)
    return v, t


def box_mesh(n=12, half=1.0):
    """An axis-aligned cube [-half, half]^3, each face n x n squares of two triangles, vertices shared along edges and corners,
    normals outward: 6 n^2 + 2 vertices, 12 n^2 triangles."""
    ids, verts, tris = {}, [], []

    def vid(p):
        if p not in ids:
            ids[p] = len(verts)
            verts.append(p)
        return ids[p]
    for axis in range(3):
        for side in (0, n):
            a, b = [(1, 2), (2, 0), (0, 1)][axis]
            for i in range(n):
                for j in range(n):
                    def P(di, dj):
                        q = [0, 0, 0]
                        q[axis], q[a], q[b] = side, i + di, j + dj
                        return vid(tuple(q))
                    quad = (P(0, 0), P(1, 0), P(1, 1), P(0, 1))          # counter-clockwise seen from +axis
                    if side == 0:
                        quad = quad[::-1]
                    tris.append((quad[0], quad[1], quad[2]))
                    tris.append((quad[0], quad[2], quad[3]))
    v = ((np.array(verts, np.float64) / n * 2.0 - 1.0) * half).astype(np.float32)
    return v, np.array(tris, np.int32)
