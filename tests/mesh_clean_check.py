"""Host restatement of the mesh clean-up (include/neddf_hip.h neddf_mesh_components, neddf_mesh_compact; neddf_amd/mesh.py
remove_small_components): labelling with scipy.sparse.csgraph.connected_components renumbered by lowest vertex index, the -1
rules, component sizes, selection and compaction in numpy.  Every result is an integer (or a copied bit pattern), so the device
code is compared with this exactly."""
import functools

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components as _scipy_components
from scipy.spatial import cKDTree


def valid_triangles(triangles, n_vertices):
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    return ((t >= 0) & (t < int(n_vertices))).all(1)


def connected_components(triangles, n_vertices):
    """(vertex_label int32 [V], triangle_label int32 [T], component_triangles int64 [C]): components in the order of their lowest
    vertex index; -1 for a vertex no valid triangle references and for a triangle with an index outside [0, V)."""
    V = int(n_vertices)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    ok = valid_triangles(t, V)
    tv = t[ok]
    vlabel = np.full(V, -1, np.int32)
    tlabel = np.full(len(t), -1, np.int32)
    if V == 0 or len(tv) == 0:
        return vlabel, tlabel, np.zeros(0, np.int64)
    rows = np.concatenate([tv[:, 0], tv[:, 1]])
    cols = np.concatenate([tv[:, 1], tv[:, 2]])
    graph = coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(V, V))
    _, raw = _scipy_components(graph, directed=False)
    used = np.zeros(V, bool)
    used[tv.reshape(-1)] = True
    ids = np.nonzero(used)[0]
    # first occurrence of every raw label among the used vertices, in vertex order = the components by lowest vertex index
    _, first = np.unique(raw[ids], return_index=True)
    order = raw[ids][np.sort(first)]
    dense = np.full(int(raw.max()) + 1, -1, np.int64)
    dense[order] = np.arange(len(order))
    vlabel[ids] = dense[raw[ids]].astype(np.int32)
    tlabel[ok] = vlabel[tv[:, 0]]
    sizes = np.bincount(tlabel[ok], minlength=len(order)).astype(np.int64)
    return vlabel, tlabel, sizes


def select_components(sizes, min_triangles=0, keep_largest=0):
    """bool [C]: at least min_triangles triangles and, if keep_largest > 0, among the keep_largest largest (ties: lower label)."""
    sizes = np.asarray(sizes, np.int64)
    keep = sizes >= int(min_triangles)
    if int(keep_largest) > 0:
        order = np.argsort(-sizes, kind="stable")
        top = np.zeros(len(sizes), bool)
        top[order[:int(keep_largest)]] = True
        keep &= top
    return keep


def compact_mesh(vertices, triangles, keep_triangle):
    """(vertices [V', 3] (the same bit patterns), triangles int32 [T', 3], vertex_map int32 [V]): the flagged triangles with valid
    indices and the vertices they reference, both in their old order."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    kept = (np.asarray(keep_triangle).reshape(-1) != 0) & valid_triangles(t, len(v))
    tk = t[kept]
    used = np.zeros(len(v), bool)
    used[tk.reshape(-1)] = True
    vmap = np.full(len(v), -1, np.int32)
    vmap[used] = np.arange(int(used.sum()), dtype=np.int32)
    out_v = v.view(np.int32)[used].view(np.float32)          # through int32: NaN payloads survive
    return out_v, vmap[tk].astype(np.int32).reshape(-1, 3), vmap


def remove_small_components(vertices, triangles, min_triangles=0, keep_largest=0):
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    _, tlabel, sizes = connected_components(triangles, len(v))
    keep = select_components(sizes, min_triangles, keep_largest)
    keep_tri = np.zeros(len(tlabel), bool)
    keep_tri[tlabel >= 0] = keep[tlabel[tlabel >= 0]]
    return compact_mesh(v, triangles, keep_tri)


# ------------------------------------------------------------------------------------------------------------ test volumes
def _grid(shape, lo, hi):
    axes = [np.linspace(lo[a], hi[a], n) for a, n in enumerate(shape[::-1])]     # x, y, z
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return x, y, z


@functools.lru_cache(maxsize=None)
def volumes():
    """name -> (volume float32 [nz, ny, nx], iso, lo, hi): the cases of tests/test_mesh_clean_host.py and tests/test_gpu_mesh_clean.py."""
    out = {}
    lo, hi = (-0.9, -0.8, -1.3), (0.85, 0.9, 1.1)
    x, y, z = _grid((33, 29, 41), lo, hi)
    spheres = [(0, 0, 0, 0.5), (0.6, 0.6, 0.8, 0.12), (-0.6, -0.5, -0.9, 0.12), (-0.62, 0.55, 0.7, 0.07), (0.55, -0.6, -1.0, 0.03),
               (0.7, 0, 0, 0.03)]
    vol = np.minimum.reduce([np.sqrt((x - a) ** 2 + (y - b) ** 2 + (z - c) ** 2) - r for a, b, c, r in spheres])
    out["floaters"] = (vol.astype(np.float32), 0.0, lo, hi)
    out["random"] = (np.random.default_rng(5).standard_normal((17, 9, 13)).astype(np.float32), 0.1, (0, 0, 0), (1, 2, 3))
    lo, hi = (-1, -1, -1), (1, 1, 1)
    x, y, z = _grid((24, 24, 24), lo, hi)
    vol = np.minimum(np.sqrt((x - 0.5) ** 2 + y * y + z * z), np.sqrt((x + 0.5) ** 2 + y * y + z * z)) - 0.3
    out["twins"] = (vol.astype(np.float32), 0.0, lo, hi)
    x, y, z = _grid((56, 56, 56), lo, hi)
    s = np.linspace(0.0, 6 * np.pi, 1500)
    curve = np.stack([0.6 * np.cos(s), 0.6 * np.sin(s), -0.8 + 1.6 * s / (6 * np.pi)], 1)
    dist = cKDTree(curve).query(np.stack([x, y, z], -1).reshape(-1, 3))[0]        # the distance to 1 500 points along the curve
    out["helix"] = ((dist - 0.09).reshape(x.shape).astype(np.float32), 0.0, lo, hi)
    return out


def hand_made():
    """(vertices [7, 3], triangles [8, 3]): vertex 3 referenced by nothing valid, a triangle with index V, one with index -1, a
    degenerate (a, a, b), a duplicated triangle; vertex 0 carries a NaN with a payload."""
    v = np.arange(21, dtype=np.float32).reshape(7, 3) * 0.5
    v.view(np.int32)[0, 1] = 0x7fc01234
    t = np.array([[4, 5, 6],        # component 1 (lowest vertex 4)
                  [0, 1, 2],        # component 0
                  [0, 1, 7],        # index V: ignored
                  [2, 2, 1],        # degenerate, valid, component 0
                  [-1, 3, 4],       # index -1: ignored (vertex 3 stays unreferenced)
                  [0, 1, 2],        # a duplicate, counted again
                  [6, 5, 4],
                  [5, 5, 5]], np.int32)
    return v, t
