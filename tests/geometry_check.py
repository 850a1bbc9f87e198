"""numpy restatement of neddf_amd/csrc/geom_kernels.hip: the counter-based hash, the per-triangle sample counts (fp64), the sample
points (fp32, the kernel's operation order), the grid cell of a point and brute-force nearest neighbours with the lowest-index tie
rule -- bit for bit what the device computes -- plus a UV sphere mesh, so that every surface a test uses exists on the CPU too."""
import numpy as np

F = np.float32
U = np.uint32


def mix(x):
    x = np.asarray(x, U).copy()
    x ^= x >> U(16)
    x *= U(0x7feb352d)
    x ^= x >> U(15)
    x *= U(0x846ca68b)
    x ^= x >> U(16)
    return x


def hash_bits(seed, t, k, w):
    """The top 24 bits of hash(seed, t, k, w) = mix(mix(mix(mix(seed + 0x9e3779b9) ^ t) ^ k) + w * 0x85ebca6b), uint32 arithmetic."""
    with np.errstate(over="ignore"):
        h = mix(U(seed) + U(0x9e3779b9))
        h = mix(h ^ np.asarray(t, U))
        h = mix(h ^ np.asarray(k, U))
        return mix(h + U(w) * U(0x85ebca6b)) >> U(8)


def _edges(vertices, triangles):
    """p0, e1 = p1 - p0, e2 = p2 - p0 in fp32 and the validity of every triangle (indices in [0, V), finite vertices)."""
    v = np.asarray(vertices, F).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    ok = ((t >= 0) & (t < len(v))).all(axis=1)
    ts = np.where(ok[:, None], t, 0) if len(v) else np.zeros_like(t)
    p = v[ts] if len(v) else np.zeros((len(t), 3, 3), F)
    ok &= np.isfinite(p).all(axis=(1, 2))
    with np.errstate(all="ignore"):
        return p[:, 0], (p[:, 1] - p[:, 0]).astype(F), (p[:, 2] - p[:, 0]).astype(F), ok


def triangle_areas(vertices, triangles):
    """A_t in fp64 from the fp32 edges: 0.5 sqrt(|e1 x e2|^2), every operation singly rounded."""
    _, e1, e2, ok = _edges(vertices, triangles)
    a, b = e1.astype(np.float64), e2.astype(np.float64)
    with np.errstate(all="ignore"):
        cx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
        cy = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
        cz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        area = 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)
    return area, ok


def sample_counts(vertices, triangles, density, seed):
    """int64 [T]: floor(A_t * density + u_t); 0 for an invalid triangle or a zero / non-finite area; 2^31 from 2^31 on."""
    area, ok = triangle_areas(vertices, triangles)
    T = len(area)
    u = hash_bits(seed, np.arange(T, dtype=np.int64).astype(U), U(0xffffffff), 2).astype(np.float64) * 2.0 ** -24
    with np.errstate(all="ignore"):
        x = area * np.float64(density) + u
        ok = ok & (area > 0.0) & np.isfinite(area)
        big = ~(x < 2147483648.0)
        c = np.floor(np.where(big | ~ok, 0.0, x)).astype(np.int64)
    return np.where(ok, np.where(big, np.int64(1) << 31, c), 0)


def sample_surface(vertices, triangles, density, seed):
    """(points float32 [N, 3], triangle_id int32 [N], counts int64 [T], offsets int64 [T]) -- triangle-major."""
    counts = sample_counts(vertices, triangles, density, seed)
    assert counts.sum() < 2 ** 31
    offsets = np.cumsum(counts) - counts
    tid = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
    k = np.arange(len(tid), dtype=np.int64) - offsets[tid]
    p0, e1, e2, _ = _edges(vertices, triangles)
    a = hash_bits(seed, tid.astype(U), k.astype(U), 0).astype(F) * F(2.0 ** -24)
    b = hash_bits(seed, tid.astype(U), k.astype(U), 1).astype(F) * F(2.0 ** -24)
    fold = (a + b).astype(F) > F(1.0)
    a = np.where(fold, (F(1.0) - a).astype(F), a)
    b = np.where(fold, (F(1.0) - b).astype(F), b)
    with np.errstate(all="ignore"):
        pts = ((p0[tid] + (a[:, None] * e1[tid]).astype(F)).astype(F) + (b[:, None] * e2[tid]).astype(F)).astype(F)
    return pts.reshape(-1, 3), tid.astype(np.int32), counts, offsets


def grid_params(lo, hi, cells):
    """(lo float32 [3], inv_cell float32 [3]) as the library derives them: the quotient in double, 0 for a zero-extent axis."""
    lo64, hi64 = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ext = hi64 - lo64
    inv = np.where(ext > 0.0, np.asarray(cells, np.float64) / np.where(ext > 0.0, ext, 1.0), 0.0).astype(F)
    return lo64.astype(F), inv


def cell_index(points, lo, hi, cells):
    """(linear cell int64 [N] with -1 for a non-finite point, per-axis cells int64 [N, 3]): f = (p - lo) * inv_cell in fp32,
    c = f >= g ? g - 1 : f > 0 ? (int)f : 0."""
    p = np.asarray(points, F).reshape(-1, 3)
    lo_f, inv = grid_params(lo, hi, cells)
    g = np.asarray(cells, np.int64)
    with np.errstate(all="ignore"):
        f = ((p - lo_f[None, :]).astype(F) * inv[None, :]).astype(F)
        c = np.where(f >= g[None, :].astype(F), g[None, :] - 1, np.where(f > 0, np.floor(np.where(np.isfinite(f), f, 0.0)).astype(np.int64), 0))
    lin = (c[:, 2] * g[1] + c[:, 1]) * g[0] + c[:, 0]
    return np.where(np.isfinite(p).all(axis=1), lin, -1), c


def nearest_brute(queries, targets, chunk=1024):
    """(d2 float32 [Q], index int32 [Q]): the float32 [Q, N] matrix d2 = (dx dx + dy dy) + dz dz, dx = qx - px, over the finite targets;
    argmin gives the lowest index of the minimum; (NaN, -1) for a non-finite query, (+inf, -1) without a finite target."""
    q = np.asarray(queries, F).reshape(-1, 3)
    p = np.asarray(targets, F).reshape(-1, 3)
    valid = np.flatnonzero(np.isfinite(p).all(axis=1))
    d2 = np.full(len(q), np.inf, F)
    idx = np.full(len(q), -1, np.int32)
    pv = p[valid]
    if len(pv):
        for s in range(0, len(q), chunk):
            qq = q[s:s + chunk]
            with np.errstate(all="ignore"):
                dx = (qq[:, None, 0] - pv[None, :, 0]).astype(F)
                dy = (qq[:, None, 1] - pv[None, :, 1]).astype(F)
                dz = (qq[:, None, 2] - pv[None, :, 2]).astype(F)
                m = (((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F) + (dz * dz).astype(F)).astype(F)
            m = np.where(np.isnan(m), np.inf, m)            # (only rows of non-finite queries hold NaN; they are overwritten below)
            k = np.argmin(m, axis=1)
            d2[s:s + chunk] = m[np.arange(len(qq)), k]
            idx[s:s + chunk] = valid[k]
    bad = ~np.isfinite(q).all(axis=1)
    d2[bad] = np.nan
    idx[bad] = -1
    return d2, idx


def uv_sphere(r, n_lat, n_lon):
    """A closed UV sphere of radius r about the origin: n_lat bands of latitude, n_lon of longitude, two pole fans, n_lon * (2 n_lat - 2)
    triangles with outward normals.  (vertices float32 [V, 3], triangles int32 [T, 3])."""
    lat = np.pi * np.arange(1, n_lat, dtype=np.float64) / n_lat            # the rings between the poles
    lon = 2.0 * np.pi * np.arange(n_lon, dtype=np.float64) / n_lon
    ring = np.stack([np.sin(lat)[:, None] * np.cos(lon)[None, :], np.sin(lat)[:, None] * np.sin(lon)[None, :],
                     np.cos(lat)[:, None] * np.ones(n_lon)[None, :]], axis=2).reshape(-1, 3)
    v = np.concatenate([[[0.0, 0.0, 1.0]], ring, [[0.0, 0.0, -1.0]]]) * r
    tris = []
    south = 1 + (n_lat - 1) * n_lon
    for j in range(n_lon):
        j1 = (j + 1) % n_lon
        tris.append((0, 1 + j, 1 + j1))
        for i in range(n_lat - 2):
            a, b = 1 + i * n_lon, 1 + (i + 1) * n_lon
            tris.append((a + j, b + j, b + j1))
            tris.append((a + j, b + j1, a + j1))
        tris.append((south, 1 + (n_lat - 2) * n_lon + j1, 1 + (n_lat - 2) * n_lon + j))
    return v.astype(F), np.array(tris, np.int32)


def sphere_sagitta(r, n_lat, n_lon):
    """An upper bound on how far inside the sphere a UV sphere's facets reach: r (1 - cos D), D = pi / n_lat + 2 pi / n_lon.  The
    corners of a facet differ by at most one step in latitude and one in longitude, so by the triangle inequality each lies within the
    angle D of corner v0; a point x of the facet is a convex combination of the corners, hence x . v0 / r >= r cos D and |x| >= r cos D."""
    return r * (1.0 - np.cos(np.pi / n_lat + 2.0 * np.pi / n_lon))
