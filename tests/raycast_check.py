"""numpy restatement of neddf_amd/csrc/raycast_kernels.hip: the watertight ray / triangle test of include/neddf_hip.h with every fp32
operation rounded once and none fused, vectorised over rays x triangles in chunks -- bit for bit what the device computes -- and the
cell lists of the grid build as sorted (list, triangle) pairs.  Plus the ray sets the host and the GPU tests share."""
import numpy as np

import geometry_check as gc

F = np.float32
D = np.float64


def _valid_triangles(vertices, triangles):
    """(corners float32 [T, 3, 3], valid bool [T]): indices in [0, V) and finite vertices."""
    v = np.asarray(vertices, F).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    ok = ((t >= 0) & (t < len(v))).all(axis=1)
    p = v[np.where(ok[:, None], t, 0)] if len(v) else np.zeros((len(t), 3, 3), F)
    ok &= np.isfinite(p).all(axis=(1, 2))
    return p, ok


def cast_rays(origins, dirs, vertices, triangles, t_min=0.0, t_max=np.inf, pad=0.0, chunk=64):
    """(t float32 [R], triangle int32 [R], b1, b2 float32 [R]) by the hit definition of include/neddf_hip.h."""
    o = np.asarray(origins, F).reshape(-1, 3)
    d = np.asarray(dirs, F).reshape(-1, 3)
    p, ok = _valid_triangles(vertices, triangles)
    index = np.flatnonzero(ok)
    p = p[index]
    t_min, t_max, pad = F(t_min), F(t_max), F(pad)
    R = len(o)
    out_t, out_j = np.full(R, np.inf, F), np.full(R, -1, np.int32)
    out_b1, out_b2 = np.zeros(R, F), np.zeros(R, F)
    ray_ok = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & (d != 0).any(axis=1)
    lo = (p.min(axis=1) - pad).astype(F)            # [T, 3]
    hi = (p.max(axis=1) + pad).astype(F)
    # the per-ray constants; rays with the same (kx, ky, kz) are handled together: the axes are then plain slices
    with np.errstate(all="ignore"):
        ad = np.abs(d)
        kz_all = np.zeros(R, np.int64)
        m = ad[:, 0].copy()
        up = ad[:, 1] > m
        kz_all[up], m[up] = 1, ad[up, 1]
        kz_all[ad[:, 2] > m] = 2
        kx_all = (kz_all + 1) % 3
        ky_all = (kx_all + 1) % 3
        swap = d[np.arange(R), kz_all] < 0
        kx_all, ky_all = np.where(swap, ky_all, kx_all), np.where(swap, kx_all, ky_all)
        groups = [(kx, ky, kz, np.flatnonzero(ray_ok & (kx_all == kx) & (kz_all == kz)))
                  for kz in range(3) for kx, ky in (((kz + 1) % 3, (kz + 2) % 3), ((kz + 2) % 3, (kz + 1) % 3))]
        for kx, ky, kz, members in groups:
            for s in range(0, len(members) if len(p) else 0, chunk):
                rows = members[s:s + chunk]
                oo, dd = o[rows], d[rows]
                Sz = (F(1.0) / dd[:, kz]).astype(F)
                Sx = (dd[:, kx] * Sz).astype(F)
                Sy = (dd[:, ky] * Sz).astype(F)
                sheared = []
                for c in range(3):
                    A = (p[None, :, c, :] - oo[:, None, :]).astype(F)                   # [r, T, 3]
                    Akz = A[:, :, kz]
                    sheared.append(((A[:, :, kx] - (Sx[:, None] * Akz).astype(F)).astype(F),
                                    (A[:, :, ky] - (Sy[:, None] * Akz).astype(F)).astype(F), (Sz[:, None] * Akz).astype(F)))
                (Ax, Ay, Az), (Bx, By, Bz), (Cx, Cy, Cz) = sheared

                def edge(a, b, c, e):
                    return ((a * b).astype(F) - (c * e).astype(F)).astype(F)

                def edge64(a, b, c, e):
                    return (a.astype(D) * b.astype(D) - c.astype(D) * e.astype(D)).astype(F)

                U, V, W = edge(Cx, By, Cy, Bx), edge(Ax, Cy, Ay, Cx), edge(Bx, Ay, By, Ax)
                again = (U == 0) | (V == 0) | (W == 0)
                if again.any():
                    U = np.where(again, edge64(Cx, By, Cy, Bx), U)
                    V = np.where(again, edge64(Ax, Cy, Ay, Cx), V)
                    W = np.where(again, edge64(Bx, Ay, By, Ax), W)
                cand = ((U >= 0) & (V >= 0) & (W >= 0)) | ((U <= 0) & (V <= 0) & (W <= 0))
                det = ((U + V).astype(F) + W).astype(F)
                cand &= det != 0
                t = ((((U * Az).astype(F) + (V * Bz).astype(F)).astype(F) + (W * Cz).astype(F)).astype(F) / det).astype(F)
                cand &= (t >= t_min) & (t <= t_max)
                pt = (oo[:, None, :] + (t[:, :, None] * dd[:, None, :]).astype(F)).astype(F)
                cand &= ((pt >= lo[None]) & (pt <= hi[None])).all(axis=2)
                tt = np.where(cand, t, np.inf).astype(F)
                k = np.argmin(tt, axis=1)                       # the first (lowest) index of the minimum; -0.0 == +0.0
                r = np.arange(len(rows))
                hit = cand[r, k]
                out_t[rows] = np.where(hit, t[r, k], np.inf)
                out_j[rows] = np.where(hit, index[k], -1)
                out_b1[rows] = np.where(hit, (V[r, k] / det[r, k]).astype(F), 0)
                out_b2[rows] = np.where(hit, (W[r, k] / det[r, k]).astype(F), 0)
    out_t[~ray_ok] = np.nan
    out_b1[~ray_ok] = np.nan
    out_b2[~ray_ok] = np.nan
    return out_t, out_j, out_b1, out_b2


def hit_points(vertices, triangles, hits):
    """p0 + b1 (p1 - p0) + b2 (p2 - p0) in fp64 for the rays that hit (NaN rows elsewhere)."""
    t, j, b1, b2 = hits
    v = np.asarray(vertices, D).reshape(-1, 3)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    out = np.full((len(t), 3), np.nan)
    h = j >= 0
    p = v[tri[j[h]]]
    out[h] = p[:, 0] + b1[h, None].astype(D) * (p[:, 1] - p[:, 0]) + b2[h, None].astype(D) * (p[:, 2] - p[:, 0])
    return out


# ---------------------------------------------------------------------------------------------------------------- the grid build
def min_pad(lo, hi):
    """The library's limit: 2^-16 of the largest of |lo|, |hi| and hi - lo over the axes."""
    lo, hi = np.asarray(lo, D), np.asarray(hi, D)
    return float(max(np.abs(lo).max(), np.abs(hi).max(), (hi - lo).max())) * 2.0 ** -16


def grid_lists(vertices, triangles, lo, hi, cells, pad):
    """(pairs, overflow): the sorted (cell, triangle) pairs of the valid triangles whose box widened by 2 pad lies inside the box widened
    by 2 pad -- the cells cell(min3 - 2 pad) .. cell(max3 + 2 pad) per axis, geometry_check.cell_index's cell function -- as an int64
    [n, 2] array, and the sorted indices of the other valid triangles."""
    p, ok = _valid_triangles(vertices, triangles)
    pad2 = F(2.0) * F(pad)
    lo_f, hi_f = np.asarray(lo, D).astype(F), np.asarray(hi, D).astype(F)
    with np.errstate(all="ignore"):
        wlo, whi = (lo_f - pad2).astype(F), (hi_f + pad2).astype(F)
        blo, bhi = (p.min(axis=1) - pad2).astype(F), (p.max(axis=1) + pad2).astype(F)
    inside = ok & (blo >= wlo[None]).all(axis=1) & (bhi <= whi[None]).all(axis=1)
    _, c0 = gc.cell_index(np.where(inside[:, None], blo, 0), lo, hi, cells)
    _, c1 = gc.cell_index(np.where(inside[:, None], bhi, 0), lo, hi, cells)
    g = np.asarray(cells, np.int64)
    pairs = []
    for j in np.flatnonzero(inside):
        z, y, x = np.meshgrid(*[np.arange(c0[j, a], c1[j, a] + 1) for a in (2, 1, 0)], indexing="ij")
        lin = ((z * g[1] + y) * g[0] + x).reshape(-1)
        pairs.append(np.stack([lin, np.full_like(lin, j)], axis=1))
    pairs = np.concatenate(pairs) if pairs else np.zeros((0, 2), np.int64)
    pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]
    return pairs, np.flatnonzero(ok & ~inside)


def cell_start(pairs, overflow, cells):
    """int32 [G + 2]: the number of pairs before each list, the overflow list last, then the total."""
    G = int(np.prod(np.asarray(cells, np.int64)))
    count = np.bincount(pairs[:, 0], minlength=G + 1)
    count[G] = len(overflow)
    return np.concatenate([[0], np.cumsum(count)]).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- shared inputs
SPHERE = (0.5, 24, 48)
EYES = np.array([[0.3, -1.9, 0.7], [1.7, 0.4, -0.6], [-0.9, 1.2, 1.3], [-1.1, -1.3, -0.8]], D)


def soup(n_tri=64, seed=11):
    """Random triangles: centres in +-0.8, corner offsets in +-0.3.  (vertices float32 [3 n, 3], triangles int32 [n, 3])."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-0.8, 0.8, (n_tri, 1, 3))
    v = (centre + rng.uniform(-0.3, 0.3, (n_tri, 3, 3))).astype(F).reshape(-1, 3)
    return v, np.arange(3 * n_tri, dtype=np.int32).reshape(n_tri, 3)


def soup_rays(vertices, triangles, n_rays=4096, seed=12):
    """Rays from radius 3 toward interior points of random triangles (barycentric weights: Dirichlet draws scaled into [0.05, 0.9])."""
    rng = np.random.default_rng(seed)
    v, t = np.asarray(vertices, D), np.asarray(triangles, np.int64)
    o = rng.standard_normal((n_rays, 3))
    o *= 3.0 / np.linalg.norm(o, axis=1, keepdims=True)
    w = 0.05 + 0.85 * rng.dirichlet(np.ones(3), n_rays)
    w /= w.sum(axis=1, keepdims=True)
    target = (v[t[rng.integers(0, len(t), n_rays)]] * w[:, :, None]).sum(axis=1)
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(F), d.astype(F)


def fan_rays(eye=EYES[0], n=160, half_width=0.45):
    """An n x n fan of rays from `eye` toward the origin, covering a sphere of radius 0.5 about it and some sky."""
    eye = np.asarray(eye, D)
    f = -eye / np.linalg.norm(eye)
    right = np.cross(f, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    upv = np.cross(right, f)
    s = np.linspace(-half_width, half_width, n)
    d = f[None, None] + s[None, :, None] * right[None, None] + s[:, None, None] * upv[None, None]
    d = d.reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.broadcast_to(eye.astype(F), d.shape).copy(), d.astype(F)


def aimed_rays(vertices, triangles, eyes=EYES):
    """Rays from every eye point at the vertices and the three edge midpoints of every triangle (duplicates kept) whose outward normal
    n (the target's direction from the origin: the mesh is a sphere about it) makes n . d < -0.3 with the ray.  (origins, dirs, the
    distance |target - eye| of each)."""
    v, t = np.asarray(vertices, D), np.asarray(triangles, np.int64)
    p = v[t]                                                                        # [T, 3, 3]
    targets = np.concatenate([p.reshape(-1, 3), (0.5 * (p + np.roll(p, -1, axis=1))).reshape(-1, 3)])
    normal = targets / np.linalg.norm(targets, axis=1, keepdims=True)
    o, d, dist = [], [], []
    for eye in np.asarray(eyes, D):
        dd = targets - eye
        ln = np.linalg.norm(dd, axis=1)
        dd = dd / ln[:, None]
        keep = (normal * dd).sum(axis=1) < -0.3
        o.append(np.broadcast_to(eye, dd.shape)[keep])
        d.append(dd[keep])
        dist.append(ln[keep])
    return np.concatenate(o).astype(F), np.concatenate(d).astype(F), np.concatenate(dist)
