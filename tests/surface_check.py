"""numpy restatement of the geometric vertex normals of neddf_mesh_vertex_normals (include/neddf_hip.h): per triangle the cross
product (p1 - p0) x (p2 - p0), summed over the triangles that hold a vertex (twice the area as weight), normalised; a sum shorter than
1e-20 gives (0, 0, 0).  dtype float32 follows the kernel -- differences, products and the one subtraction per component rounded to
fp32, sums and normalisation in float64 -- and dtype float64 is the same rule without any fp32 rounding after the vertex positions."""
import numpy as np


def cross_products(verts, tris, dtype=np.float32):
    v = np.asarray(verts).astype(dtype)
    t = np.asarray(tris)
    p0, p1, p2 = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    a, b = p1 - p0, p2 - p0
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def normal_sums(verts, tris, dtype=np.float32):
    """Un-normalised float64 sums [V, 3]."""
    c = cross_products(verts, tris, dtype).astype(np.float64)
    c[~np.isfinite(c).all(1)] = 0.0
    acc = np.zeros((len(verts), 3))
    for k in range(3):
        np.add.at(acc, np.asarray(tris)[:, k], c)
    return acc


def vertex_normals(verts, tris, dtype=np.float32):
    acc = normal_sums(verts, tris, dtype)
    length = np.sqrt((acc * acc).sum(1, keepdims=True))
    out = np.where(length >= 1e-20, acc / np.where(length >= 1e-20, length, 1.0), 0.0)
    return out.astype(np.float32) if dtype == np.float32 else out
