"""numpy restatement of neddf_amd/csrc/pointmesh_kernels.hip: the closest point of a triangle mesh to every query by the arithmetic of
include/neddf_hip.h (neddf_point_mesh_brute), every fp32 operation rounded once and none fused, vectorised over queries x triangles in
chunks -- bit for bit what the device computes -- the grid query's shell walk over raycast_check.grid_lists with the library's stopping
rule, and an INDEPENDENT fp64 closest-point computation (Ericson's region tests) to measure both against."""
import numpy as np

import geometry_check as gc
import raycast_check as rc

F = np.float32
D = np.float64


def _dot(x, y):
    """(x0 y0 + x1 y1) + x2 y2 over the last axis, every operation one rounded fp32 operation."""
    return (((x[..., 0] * y[..., 0]).astype(F) + (x[..., 1] * y[..., 1]).astype(F)).astype(F) + (x[..., 2] * y[..., 2]).astype(F)).astype(F)


def triangle_constants(vertices, triangles):
    """The per-triangle constants of the header as a dict of float32 arrays over ALL triangles, and valid bool [T]."""
    p, ok = rc._valid_triangles(vertices, triangles)
    p = np.where(ok[:, None, None], p, F(0.0)).astype(F)
    with np.errstate(all="ignore"):
        a, b, c = p[:, 0], p[:, 1], p[:, 2]
        e0, e1, e2 = (b - a).astype(F), (c - a).astype(F), (c - b).astype(F)
        g00, g01, g11, g22 = _dot(e0, e0), _dot(e0, e1), _dot(e1, e1), _dot(e2, e2)
        one = F(1.0)
        r00 = (one / g00).astype(F)
        e1p = (e1 - ((g01 * r00).astype(F)[:, None] * e0).astype(F)).astype(F)         # e1 without its part along e0
        gpp = _dot(e1p, e1p)
        k = dict(a=a, b=b, c=c, e0=e0, e1=e1, e2=e2, e1p=e1p, g01=g01, gpp=gpp, r00=r00, r11=(one / g11).astype(F), r22=(one / g22).astype(F),
                 rpp=(one / gpp).astype(F))
    return k, ok


def _clamp01(u):
    return np.where(u > 0, np.where(u < 1, u, F(1.0)), F(0.0)).astype(F)          # a NaN gives 0


def _pairs(q, k):
    """(D2, b1, b2) float32 [Q, T] of every (query, triangle) pair: the interior candidate or +inf, replaced by the edge candidates ab,
    bc, ac and by the corner c when strictly smaller (a NaN never replaces)."""
    with np.errstate(all="ignore"):
        p = q[:, None, :]
        a, b, e0, e1, e2 = (k[n][None] for n in ("a", "b", "e0", "e1", "e2"))
        ap, bp = (p - a).astype(F), (p - b).astype(F)
        d1, d2, d3 = _dot(e0, ap), _dot(e1, ap), _dot(e2, bp)
        e1p, g01, gpp, r00, rpp = (k[n][None] for n in ("e1p", "g01", "gpp", "r00", "rpp"))

        def solve(x, dx0):
            w = (_dot(e1p, x) * rpp).astype(F)
            return ((dx0 - (w * g01).astype(F)).astype(F) * r00).astype(F), w

        v, w = solve(ap, d1)
        qi = ((a + (v[..., None] * e0).astype(F)).astype(F) + (w[..., None] * e1).astype(F)).astype(F)
        di = (p - qi).astype(F)
        dv, dw = solve(di, _dot(e0, di))                # one step of iterative refinement on the residual
        v, w = (v + dv).astype(F), (w + dw).astype(F)
        inside = (gpp > 0) & (v > 0) & (w > 0) & ((v + w).astype(F) < 1)
        qi = ((a + (v[..., None] * e0).astype(F)).astype(F) + (w[..., None] * e1).astype(F)).astype(F)
        di = (p - qi).astype(F)
        Di = _dot(di, di)
        take = inside & (Di < np.inf)
        best = np.where(take, Di, np.inf).astype(F)
        b1, b2 = np.where(take, v, F(0.0)).astype(F), np.where(take, w, F(0.0)).astype(F)
        zero = np.zeros_like(best)
        for s, e, h, r, which in ((a, e0, d1, k["r00"][None], 0), (b, e2, d3, k["r22"][None], 1), (a, e1, d2, k["r11"][None], 2)):
            u = _clamp01((h * r).astype(F))
            qe = (s + (u[..., None] * e).astype(F)).astype(F)
            de = (p - qe).astype(F)
            De = _dot(de, de)
            take = De < best
            best = np.where(take, De, best)
            c1, c2 = ((u, zero), ((F(1.0) - u).astype(F), u), (zero, u))[which]
            b1, b2 = np.where(take, c1, b1), np.where(take, c2, b2)
        dc = (p - k["c"][None]).astype(F)               # the corner c itself: the only corner no edge candidate reaches without a product
        Dc = _dot(dc, dc)
        take = Dc < best
        best, b1, b2 = np.where(take, Dc, best), np.where(take, F(0.0), b1).astype(F), np.where(take, F(1.0), b2).astype(F)
    return best, b1, b2


def point_mesh_brute(queries, vertices, triangles, chunk=256):
    """(d2 float32 [Q], triangle int32 [Q], b1, b2 float32 [Q]) by the definition of include/neddf_hip.h: the smallest D2 and among equal
    ones the lowest triangle index; (NaN, -1, NaN, NaN) for a non-finite query, (+inf, -1, 0, 0) without a valid triangle."""
    q = np.asarray(queries, F).reshape(-1, 3)
    k, ok = triangle_constants(vertices, triangles)
    index = np.flatnonzero(ok)
    k = {n: x[index] for n, x in k.items()}
    Q = len(q)
    out_d, out_j = np.full(Q, np.inf, F), np.full(Q, -1, np.int32)
    out_b1, out_b2 = np.zeros(Q, F), np.zeros(Q, F)
    fin = np.isfinite(q).all(axis=1)
    qq = np.where(fin[:, None], q, F(0.0)).astype(F)
    if len(index):
        for s in range(0, Q, chunk):
            d, b1, b2 = _pairs(qq[s:s + chunk], k)
            j = np.argmin(d, axis=1)                    # the first (lowest) index of the minimum; a pair's D2 is never NaN
            r = np.arange(len(j))
            out_d[s:s + chunk], out_j[s:s + chunk] = d[r, j], index[j]
            out_b1[s:s + chunk], out_b2[s:s + chunk] = b1[r, j], b2[r, j]
    out_d[~fin], out_j[~fin], out_b1[~fin], out_b2[~fin] = np.nan, -1, np.nan, np.nan
    return out_d, out_j, out_b1, out_b2


def closest_points(vertices, triangles, result):
    """p0 + b1 (p1 - p0) + b2 (p2 - p0) in fp64 (NaN rows where there is no triangle)."""
    return rc.hit_points(vertices, triangles, result)


# ---------------------------------------------------------------------------------------------------------------- the grid query
WALK_LIMIT = 2.0 ** -10         # the shells are walked when the smallest cell edge is at least this share of the largest of |wlo|, |whi|


def grid_walks(lo, hi, cells, pad):
    """(walk, safe_cell float32): whether neddf_point_mesh_grid_query walks the shells of this grid, and 0.99 * the smallest cell edge."""
    lo_f, inv = gc.grid_params(lo, hi, cells)
    hi_f = np.asarray(hi, D).astype(F)
    pad2 = F(2.0) * F(pad)
    w = max(float(np.abs((lo_f - pad2).astype(F)).max()), float(np.abs((hi_f + pad2).astype(F)).max()))
    inv_max = float(inv.max())
    safe = F(0.99 / inv_max) if inv_max > 0.0 and 0.99 / inv_max < 3.0e38 else F(3.0e38)
    return (inv_max > 0.0 and 1.0 / inv_max >= WALK_LIMIT * w) or inv_max == 0.0, safe


def point_mesh_grid(queries, vertices, triangles, lo, hi, cells, pad, return_visits=False):
    """The grid query's walk in numpy: the overflow list, then the Chebyshev shells of cells around the query's clamped cell until
    (r * safe_cell)^2 > best strictly and >= 1e-30, or every list once when the grid is not walked.  Each visited set is evaluated with
    point_mesh_brute's pair arithmetic and reduced by the same rule."""
    q = np.asarray(queries, F).reshape(-1, 3)
    pairs, overflow = rc.grid_lists(vertices, triangles, lo, hi, cells, pad)
    k, _ = triangle_constants(vertices, triangles)
    walk, safe = grid_walks(lo, hi, cells, pad)
    g = np.asarray(cells, np.int64)
    G = int(g.prod())
    start = np.searchsorted(pairs[:, 0], np.arange(G + 1))
    _, qc = gc.cell_index(q, lo, hi, cells)
    Q = len(q)
    out = (np.full(Q, np.inf, F), np.full(Q, -1, np.int32), np.zeros(Q, F), np.zeros(Q, F))
    visits = np.zeros(Q, np.int64)

    def visit(i, best, js):
        if len(js) == 0:
            return best
        js = np.asarray(js, np.int64)
        d, b1, b2 = _pairs(q[i:i + 1], {n: x[js] for n, x in k.items()})
        d, b1, b2 = d[0], b1[0], b2[0]
        visits[i] += len(js)
        m = d.min()
        j = js[d == m].min()
        at = np.flatnonzero((js == j) & (d == m))[0]
        if m < best[0] or (m == best[0] and (best[1] < 0 or j < best[1])):
            return (m, int(j), b1[at], b2[at])
        return best

    for i in range(Q):
        if not np.isfinite(q[i]).all():
            for o, x in zip(out, (np.nan, -1, np.nan, np.nan)):
                o[i] = x
            continue
        best = visit(i, (F(np.inf), -1, F(0.0), F(0.0)), overflow)
        if not walk:
            best = visit(i, best, pairs[:, 1])
        else:
            c = qc[i]
            r_max = int(max(np.maximum(c, g - 1 - c)))
            for r in range(r_max + 1):
                l0, l1 = np.maximum(c - r, 0), np.minimum(c + r, g - 1)
                z, y, x = np.meshgrid(*[np.arange(l0[a], l1[a] + 1) for a in (2, 1, 0)], indexing="ij")
                shell = np.maximum(np.maximum(np.abs(z - c[2]), np.abs(y - c[1])), np.abs(x - c[0])) == r
                lin = ((z * g[1] + y) * g[0] + x)[shell]
                js = np.concatenate([pairs[start[l]:start[l + 1], 1] for l in lin]) if len(lin) else []
                best = visit(i, best, js)
                lb = F(F(r) * safe)
                with np.errstate(over="ignore"):
                    lb2 = F(lb * lb)
                if lb2 > best[0] and lb2 >= F(1e-30):
                    break
        for o, x in zip(out, best):
            o[i] = x
    return out + (visits,) if return_visits else out


# ---------------------------------------------------------------------------------------------------------------- the fp64 yardstick
def closest_fp64(queries, vertices, triangles, chunk=512):
    """The distance (not squared) from every query to the nearest valid triangle in fp64 by Ericson's region tests (Real-Time
    Collision Detection 5.1.5): vertex regions, edge regions, else the face -- and, for a triangle whose normal vanishes, the nearest of
    its three segments.  Shares no formula with the restatement above."""
    q = np.asarray(queries, D).reshape(-1, 3)
    p, ok = rc._valid_triangles(vertices, triangles)
    p = p[ok].astype(D)
    out = np.full(len(q), np.inf)
    if not len(p):
        return out
    A, B, C = p[None, :, 0], p[None, :, 1], p[None, :, 2]

    def dot(x, y):
        return (x * y).sum(axis=-1)

    def segment(P, S, E):
        se = E - S
        l2 = dot(se, se)
        with np.errstate(all="ignore"):
            t = np.where(l2 > 0, dot(P - S, se) / np.where(l2 > 0, l2, 1.0), 0.0)
        t = np.clip(t, 0.0, 1.0)
        x = P - (S + t[..., None] * se)
        return dot(x, x)

    for s in range(0, len(q), chunk):
        P = q[s:s + chunk, None, :]
        ab, ac = B - A, C - A
        ap, bp, cp = P - A, P - B, P - C
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        n = np.cross(ab, ac)
        n2 = dot(n, n)
        with np.errstate(all="ignore"):
            plane = dot(ap, n) ** 2 / np.where(n2 > 0, n2, 1.0)
        face = (n2 > 0) & (va > 0) & (vb > 0) & (vc > 0)
        edges = np.minimum(np.minimum(segment(P, A, B), segment(P, B, C)), segment(P, A, C))
        # in the face region the foot of the perpendicular lies inside the triangle; everywhere else the boundary is nearest
        d2min = np.where(face, np.minimum(plane, edges), edges)
        out[s:s + chunk] = np.sqrt(d2min.min(axis=1))
    return out
