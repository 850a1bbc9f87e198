"""Distances between point clouds and between meshes on the GPU: exact nearest neighbours (a uniform grid, or brute force), the exact
distance from points to a mesh's triangles, Chamfer and Hausdorff distance, precision / recall / F-score at a threshold, and a check of
a distance field against the mesh of one of its level sets.

The reference's evaluation compares images (PSNR, SSIM: metrics.py); the distance between two SURFACES is what tells how far a sparse
extraction, an operand policy or a clean-up moved the level set.  Sampling (mesh.sample_surface) and the nearest-neighbour search are
HIP kernels (include/neddf_hip.h neddf_mesh_sample_*, neddf_nn_brute, neddf_nn_grid_build, neddf_nn_grid_query), and so is the
point-to-triangle search (neddf_point_mesh_brute, neddf_point_mesh_grid_query over raycast.build_grid's lists,
neddf_point_mesh_bvh_query through bvh.build_bvh's tree -- the one for queries anywhere in the volume, which distance_field_check
asks); the reductions over the per-point distances are torch fp64 on the device.
"""
import torch

from ._lib import Context, NeddfError
from .mesh import sample_surface, surface_area

# targets per grid cell of nearest()'s default grid: the fastest of the sweep 1, 2, 4, 8, 16 of tools/time_mesh_distance.py on the MI355X
# (profiles/mesh_distance_cost.json: 10^6 x 10^6 points, build + query 1.3 ms at 1 against 2.8 ms at 4 and 4.7 ms at 16; 1 is the sweep's
# best and its edge).  Results are bit-identical for any value.
POINTS_PER_CELL = 1
MAX_CELLS_PER_AXIS, MAX_CELLS = 1024, 1 << 24           # the library's limits (neddf_nn_grid_build)


def _points(what, name, t):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise NeddfError("%s: %s must be a tensor on a HIP device (got %s)" % (what, name, t.device if isinstance(t, torch.Tensor) else type(t).__name__))
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3:
        raise NeddfError("%s: %s must be float32 [N, 3] (got %s %s)" % (what, name, t.dtype, tuple(t.shape)))
    return t.contiguous()


def default_cells(n_valid, lo, hi, points_per_cell=POINTS_PER_CELL):
    """(gx, gy, gz) of a grid of cubic cells over the box lo .. hi with about points_per_cell of n_valid points per cell; an axis without
    extent gets one cell, every axis 1 .. 1024 cells, all of them at most 2^24."""
    ext = [max(float(h) - float(l), 0.0) for l, h in zip(lo, hi)]
    live = [e for e in ext if e > 0.0]
    if not live or n_valid <= 0:
        return (1, 1, 1)
    want = min(max(float(n_valid) / float(points_per_cell), 1.0), float(MAX_CELLS))
    vol = 1.0
    for e in live:
        vol *= e
    edge = (vol / want) ** (1.0 / len(live))
    cells = [min(max(int(e / edge + 0.5), 1), MAX_CELLS_PER_AXIS) if e > 0.0 else 1 for e in ext]
    while cells[0] * cells[1] * cells[2] > MAX_CELLS:       # rounding up on every axis may pass the limit
        k = cells.index(max(cells))
        cells[k] -= 1
    return tuple(cells)


def nearest(queries, targets, method="grid", box=None, cells=None):
    """The exact nearest target of every query: (distance float32 [Q], index int64 [Q]).

    The squared distance is (dx dx + dy dy) + dz dz in single-rounded fp32 and the index the LOWEST one that attains its minimum, so
    method="grid" and method="brute" return the same bits; `distance` is torch.sqrt of it.  A target with a non-finite coordinate is
    never found; a query with one gets (NaN, -1), and without a valid target every query gets (+inf, -1).
    box = (lo, hi): the grid's box, by default the finite targets' bounding box (points outside land in its border cells -- any box
    gives the same result, a fitting one the fastest); cells = (gx, gy, gz), by default cubic cells holding about POINTS_PER_CELL
    targets each (default_cells).  Both are ignored by method="brute"."""
    q, t = _points("nearest", "queries", queries), _points("nearest", "targets", targets)
    if q.device != t.device:
        raise NeddfError("nearest: queries and targets must live on one device (got %s, %s)" % (q.device, t.device))
    if method not in ("grid", "brute"):
        raise NeddfError("nearest: method must be 'grid' or 'brute' (got %r)" % (method,))
    ctx = Context.get(q.device)
    if method == "brute":
        d2, idx = ctx.nn_brute(q, t)
        return torch.sqrt(d2), idx.long()
    finite = torch.isfinite(t).all(dim=1)
    n_valid = int(finite.sum().item())
    if box is None:
        if n_valid:
            tv = t[finite]
            lo, hi = tv.min(dim=0).values.double().tolist(), tv.max(dim=0).values.double().tolist()
        else:
            lo, hi = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    else:
        try:
            lo, hi = [float(x) for x in box[0]], [float(x) for x in box[1]]
        except (TypeError, ValueError, IndexError):
            raise NeddfError("nearest: box must be (lo, hi) with 3 numbers each (got %r)" % (box,)) from None
        if len(lo) != 3 or len(hi) != 3 or not all(l <= h and abs(l) < float("inf") and abs(h) < float("inf") for l, h in zip(lo, hi)):
            raise NeddfError("nearest: box must be (lo, hi) with 3 finite numbers each and lo <= hi (got %r)" % (box,))
    if cells is None:
        cells = default_cells(n_valid, lo, hi)
    else:
        cells = tuple(int(c) for c in cells)
        if len(cells) != 3 or min(cells) < 1 or max(cells) > MAX_CELLS_PER_AXIS or cells[0] * cells[1] * cells[2] > MAX_CELLS:
            raise NeddfError("nearest: cells must be (gx, gy, gz), each in [1, %d], at most 2^24 in all (got %r)" % (MAX_CELLS_PER_AXIS, cells))
    start, order = ctx.nn_grid_build(t, lo, hi, cells)
    d2, idx = ctx.nn_grid_query(q, t, lo, hi, cells, start, order)
    return torch.sqrt(d2), idx.long()


def _one_way(dist, index, tau):
    """(mean, max, share within tau, valid count, invalid count) of one direction's distances, in fp64 on the device."""
    ok = (index >= 0) & ~torch.isnan(dist)
    d = dist[ok].double()
    n = int(d.numel())
    nan = float("nan")
    if n == 0:
        return nan, nan, nan, 0, int(dist.numel())
    within = float((d <= float(tau)).double().mean().item()) if tau is not None else nan
    return float(d.mean().item()), float(d.max().item()), within, n, int(dist.numel()) - n


def cloud_distance(a, b, tau=None, method="grid", return_samples=False):
    """Distances between two point clouds float32 [Na, 3] and [Nb, 3] on one HIP device, as a dict:

      a_to_b_mean, b_to_a_mean   the mean distance from a point of one cloud to its nearest point of the other
      chamfer                    the mean of those two
      a_to_b_max, b_to_a_max     the largest such distance per direction;  hausdorff: the larger of the two
      precision, recall, fscore  with `tau`: the share of a within tau of b, of b within tau of a, and their harmonic mean
      n_a, n_b                   the points of each cloud;  invalid_a, invalid_b: those whose query gave NaN or no neighbour (a
                                 non-finite point, or no finite point on the other side) -- excluded from every reduction

    Nearest neighbours come from nearest(method=...); the reductions are torch fp64 on the device.  return_samples=True adds
    a_to_b / b_to_a (float32 distances per point) and a_to_b_index / b_to_a_index (int64)."""
    if tau is not None and not float(tau) >= 0.0:
        raise NeddfError("cloud_distance: tau must not be negative (got %r)" % (tau,))
    dab, iab = nearest(a, b, method=method)
    dba, iba = nearest(b, a, method=method)
    mab, xab, pab, _, bad_a = _one_way(dab, iab, tau)
    mba, xba, pba, _, bad_b = _one_way(dba, iba, tau)
    out = {"a_to_b_mean": mab, "b_to_a_mean": mba, "chamfer": 0.5 * (mab + mba), "hausdorff": max(xab, xba) if xab == xab and xba == xba else float("nan"),
           "a_to_b_max": xab, "b_to_a_max": xba, "n_a": int(a.shape[0]), "n_b": int(b.shape[0]), "invalid_a": bad_a, "invalid_b": bad_b}
    if tau is not None:
        out["precision"], out["recall"] = pab, pba
        out["fscore"] = 2.0 * pab * pba / (pab + pba) if pab + pba > 0.0 else (0.0 if pab == pab and pba == pba else float("nan"))
    if return_samples:
        out.update(a_to_b=dab, b_to_a=dba, a_to_b_index=iab, b_to_a_index=iba)
    return out


def _grid_of(what, v, t, grid):
    """`grid` validated as cast_rays validates it, or build_grid's default grid of the mesh."""
    from .raycast import MeshGrid, build_grid
    if grid is None:
        return build_grid(v, t)
    if not isinstance(grid, MeshGrid) or grid.n_vertices != v.shape[0] or grid.n_triangles != t.shape[0] or grid.cell_start.device != v.device:
        raise NeddfError("%s: grid must be the MeshGrid build_grid made of this mesh" % what)
    return grid


def point_mesh_distance(queries, vertices, triangles, method="grid", grid=None, bvh=None):
    """The exact distance from every query (float32 [Q, 3]) to the SURFACE of a device mesh (vertices float32 [V, 3], triangles int32
    or int64 [T, 3]) -- to its closest triangle, not to its closest vertex or sample -- as a dict:

      distance  float32 [Q]: torch.sqrt of the library's squared distance; +inf without a valid triangle
      triangle  int64 [Q]: the closest triangle, -1 for none
      b1, b2    float32 [Q]: the closest point is p0 + b1 (p1 - p0) + b2 (p2 - p0) (closest_points evaluates it); 0 for none

    The arithmetic is specified operation by operation (include/neddf_hip.h neddf_point_mesh_brute; tests/pointmesh_check.py restates it
    in numpy bit for bit): among equal squared distances the lowest triangle index wins, so method="grid" and method="brute" return the
    same bits.  A query with a non-finite coordinate gets (NaN, -1, NaN, NaN); a triangle with an index outside [0, V) or a non-finite
    vertex is never found.  method="grid" walks the uniform grid of raycast.build_grid (`grid`: the MeshGrid of this mesh, built here
    with build_grid's defaults when None -- build it once for many calls); queries far from the surface walk many shells of cells
    and are correspondingly slower.  `grid` is ignored by method="brute".  method="bvh" descends a bounding-volume hierarchy of the
    triangles (`bvh`: the MeshBVH of this mesh, bvh.build_bvh, built here when None) and returns the same bits again: its cost barely
    depends on how far the query is from the surface, so it is the method for queries anywhere in the volume."""
    from .bvh import bvh_of
    from .raycast import _mesh
    q = _points("point_mesh_distance", "queries", queries)
    v, t = _mesh("point_mesh_distance", vertices, triangles)
    if q.device != v.device:
        raise NeddfError("point_mesh_distance: queries and mesh must live on one device (got %s, %s)" % (q.device, v.device))
    if method not in ("grid", "brute", "bvh"):
        raise NeddfError("point_mesh_distance: method must be 'grid', 'brute' or 'bvh' (got %r)" % (method,))
    ctx = Context.get(q.device)
    if grid is not None and method != "grid":
        _grid_of("point_mesh_distance", v, t, grid)
    if bvh is not None and method != "bvh":
        bvh_of("point_mesh_distance", v, t, bvh)
    if method == "brute":
        d2, j, b1, b2 = ctx.point_mesh_brute(q, v, t)
    elif method == "bvh":
        bvh = bvh_of("point_mesh_distance", v, t, bvh)
        d2, j, b1, b2 = ctx.point_mesh_bvh_query(q, v, t, bvh.leaf_triangle, bvh.children, bvh.boxes)
    else:
        grid = _grid_of("point_mesh_distance", v, t, grid)
        d2, j, b1, b2 = ctx.point_mesh_grid_query(q, v, t, grid.lo, grid.hi, grid.cells, grid.pad, grid.cell_start, grid.items)
    return {"distance": torch.sqrt(d2), "triangle": j.long(), "b1": b1, "b2": b2}


def closest_points(vertices, triangles, result):
    """p0 + b1 (p1 - p0) + b2 (p2 - p0) float32 [Q, 3] of a point_mesh_distance result, in torch; NaN rows where triangle is -1."""
    j, b1, b2 = result["triangle"], result["b1"], result["b2"]
    ok = j >= 0
    p = vertices[triangles.long()[j.clamp_min(0)]]
    out = p[:, 0] + b1[:, None] * (p[:, 1] - p[:, 0]) + b2[:, None] * (p[:, 2] - p[:, 0])
    return torch.where(ok[:, None], out, torch.full_like(out, float("nan")))


def mesh_distance(mesh_a, mesh_b, n=None, density=None, seed=0, tau=None, method="grid", return_samples=False, to="samples"):
    """Distances between two device meshes, each (vertices float32 [V, 3], triangles int32 [T, 3]), from area-weighted samples of both
    (cloud_distance's dict).

    Both meshes are sampled with the SAME density and seed (mesh.sample_surface).  Exactly one of `density` (samples per unit area) and
    `n` is given; n is turned into a density by the mean of the two areas, so each mesh gets about n points.

    to="samples" (the default): cloud_distance between the two sample sets.  Identical meshes give identical samples and every distance
    is exactly 0 -- the mode for asking WHETHER two meshes are the same -- but two meshes that differ at all are a sample spacing
    apart (about 3e-3 at 10^5 samples on a unit-sized object), whatever their true distance.
    to="surface": every sample of one mesh is measured against the other mesh's TRIANGLES (point_mesh_distance), the figure
    reconstruction papers report and the one without a sampling floor -- the mode for asking HOW FAR two different meshes are apart.
    Identical meshes then give rounding-level distances (a few 2^-24 of the coordinates), not exact zeros.  The dict has the same keys.

    return_samples=True adds points_a / points_b, triangle_a / triangle_b and the per-sample distances a_to_b / b_to_a and indices
    a_to_b_index / b_to_a_index: sample indices with to="samples"; with to="surface" triangle indices of the other mesh, and
    a_to_b_b1 / a_to_b_b2 / b_to_a_b1 / b_to_a_b2, the closest point's barycentric pair (closest_points)."""
    if to not in ("samples", "surface"):
        raise NeddfError("mesh_distance: to must be 'samples' or 'surface' (got %r)" % (to,))
    if (density is None) == (n is None):
        raise NeddfError("mesh_distance: exactly one of density and n must be given")
    (va, ta), (vb, tb) = mesh_a, mesh_b
    if density is None:
        if int(n) < 0:
            raise NeddfError("mesh_distance: n must not be negative (got %r)" % (n,))
        for what, v, t in (("mesh_a", va, ta), ("mesh_b", vb, tb)):
            if not all(isinstance(x, torch.Tensor) and x.is_cuda for x in (v, t)):
                raise NeddfError("mesh_distance: %s must be (vertices, triangles) on a HIP device" % what)
        area = 0.5 * (surface_area(va, ta) + surface_area(vb, tb))
        density = int(n) / area if area > 0.0 else 0.0
    pa, ia = sample_surface(va, ta, density=density, seed=seed)
    pb, ib = sample_surface(vb, tb, density=density, seed=seed)
    if to == "samples":
        out = cloud_distance(pa, pb, tau=tau, method=method, return_samples=return_samples)
    else:
        if tau is not None and not float(tau) >= 0.0:
            raise NeddfError("mesh_distance: tau must not be negative (got %r)" % (tau,))
        rab = point_mesh_distance(pa, vb, tb, method=method)
        rba = point_mesh_distance(pb, va, ta, method=method)
        mab, xab, pab, _, bad_a = _one_way(rab["distance"], rab["triangle"], tau)
        mba, xba, pba, _, bad_b = _one_way(rba["distance"], rba["triangle"], tau)
        out = {"a_to_b_mean": mab, "b_to_a_mean": mba, "chamfer": 0.5 * (mab + mba),
               "hausdorff": max(xab, xba) if xab == xab and xba == xba else float("nan"), "a_to_b_max": xab, "b_to_a_max": xba,
               "n_a": int(pa.shape[0]), "n_b": int(pb.shape[0]), "invalid_a": bad_a, "invalid_b": bad_b}
        if tau is not None:
            out["precision"], out["recall"] = pab, pba
            out["fscore"] = 2.0 * pab * pba / (pab + pba) if pab + pba > 0.0 else (0.0 if pab == pab and pba == pba else float("nan"))
        if return_samples:
            out.update(a_to_b=rab["distance"], b_to_a=rba["distance"], a_to_b_index=rab["triangle"], b_to_a_index=rba["triangle"],
                       a_to_b_b1=rab["b1"], a_to_b_b2=rab["b2"], b_to_a_b1=rba["b1"], b_to_a_b2=rba["b2"])
    out["density"] = float(density)
    if return_samples:
        out.update(points_a=pa, points_b=pb, triangle_a=ia, triangle_b=ib)
    return out


GOLDEN_STEP, PLASTIC_STEP = 0.6180339887498949, 0.7548776662466927      # the offsets' low-discrepancy sequence and its shift per seed


def level_set_check(distance_fn, vertices, triangles, threshold, band, n=100000, seed=0, min_distance=None, method="grid", grid=None,
                    return_samples=False, bvh=None):
    """How well a field is a DISTANCE field around one of its level sets: (vertices, triangles) is the mesh of the level set
    D = threshold (extract_mesh), distance_fn(p [M, 3]) -> D [M] the field (trace.sphere_trace's contract), and |D(p) - threshold| is
    set against the exact distance d(p) from p to the mesh (point_mesh_distance) at about n points within `band` of it.

    The points: x_k, triangle ids = sample_surface(n=n, seed=seed); n_k the unit face normal in torch fp32; the offset
    s_k = band * (2 frac((k + 1) * 0.6180339887498949 + seed * 0.7548776662466927) - 1) in fp64 (deterministic: no torch generator is
    touched); p_k = x_k + s_k n_k in fp32.  With e_k = |D_k - threshold| - d_k the dict holds

      n, band, invalid                    the points, the band, and how many D_k were not finite (left out of everything below)
      mean_error, mean_abs_error, rms_error, max_abs_error     of e_k
      slope_median, slope_p99, slope_max, n_slope              of |D_k - threshold| / d_k over the points with d_k >= min_distance
                                          (default band / 8): 1 for a distance field, above 1 where the field oversteps
      suggested_step_scale                min(1, 1 / slope_p99): the sphere tracer's step_scale that keeps 99 % of the steps short of
                                          the surface; the same number bounds extract_mesh's `lipschitz`

    Every figure carries the mesh's own error: the level set lies within marching cubes' interpolation error of its mesh, which the
    slope's min_distance keeps small against d_k.  Reductions are torch fp64 on the device.  return_samples=True adds points,
    mesh_distance and field_distance (float32, all n points)."""
    from .raycast import _mesh
    if not callable(distance_fn):
        raise NeddfError("level_set_check: distance_fn must be callable: pos [M, 3] -> distances [M]")
    v, t = _mesh("level_set_check", vertices, triangles)
    band, threshold = float(band), float(threshold)
    if not (band > 0.0 and band < float("inf")):
        raise NeddfError("level_set_check: band must be positive and finite (got %r)" % (band,))
    min_distance = band / 8.0 if min_distance is None else float(min_distance)
    if not min_distance > 0.0:
        raise NeddfError("level_set_check: min_distance must be positive (got %r)" % (min_distance,))
    x, tid = sample_surface(v, t, n=int(n), seed=seed)
    p = v[t.long()[tid.long()]]
    nrm = torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    nrm = nrm / nrm.norm(dim=1, keepdim=True).clamp_min(1e-30)
    k = torch.arange(1, x.shape[0] + 1, device=x.device, dtype=torch.float64)
    s = band * (2.0 * torch.frac(k * GOLDEN_STEP + float(int(seed)) * PLASTIC_STEP) - 1.0)
    pts = (x + s.float()[:, None] * nrm).contiguous()
    d = point_mesh_distance(pts, v, t, method=method, grid=grid, bvh=bvh)["distance"]
    with torch.no_grad():
        D = distance_fn(pts)
    if not isinstance(D, torch.Tensor) or D.device != pts.device or D.numel() != pts.shape[0]:
        raise NeddfError("level_set_check: distance_fn must return one distance per point on the points' device")
    D = D.reshape(-1).float()
    ok = torch.isfinite(D) & torch.isfinite(d)
    m = int(ok.sum().item())
    nan = float("nan")
    out = {"n": int(pts.shape[0]), "band": band, "invalid": int(pts.shape[0]) - m}
    f = (D.double() - threshold).abs()[ok]
    dd = d.double()[ok]
    e = f - dd
    if m:
        out.update(mean_error=float(e.mean().item()), mean_abs_error=float(e.abs().mean().item()),
                   rms_error=float((e * e).mean().sqrt().item()), max_abs_error=float(e.abs().max().item()))
    else:
        out.update(mean_error=nan, mean_abs_error=nan, rms_error=nan, max_abs_error=nan)
    far = dd >= min_distance
    n_slope = int(far.sum().item())
    out["n_slope"] = n_slope
    if n_slope:
        slope = f[far] / dd[far]
        if n_slope <= 1 << 24:
            p99 = float(torch.quantile(slope, 0.99).item())
        else:                                                       # (torch.quantile refuses more than 2^24 elements)
            p99 = float(slope.sort().values[int(0.99 * (n_slope - 1))].item())
        out.update(slope_median=float(slope.median().item()), slope_p99=p99, slope_max=float(slope.max().item()))
        out["suggested_step_scale"] = min(1.0, 1.0 / out["slope_p99"]) if out["slope_p99"] > 0.0 else 1.0
    else:
        out.update(slope_median=nan, slope_p99=nan, slope_max=nan, suggested_step_scale=nan)
    if return_samples:
        out.update(points=pts, mesh_distance=d, field_distance=D)
    return out


# the volume's low-discrepancy sequence: the additive recurrence with (1 / g, 1 / g^2, 1 / g^3), g the real root of x^4 = x + 1
R3_STEPS = (0.8191725133961645, 0.6710436067037893, 0.5497004779019702)


def _quantile(x, q):
    """torch.quantile, which refuses more than 2^24 elements, or the sorted element at that rank."""
    n = int(x.numel())
    return float(torch.quantile(x, q).item()) if n <= 1 << 24 else float(x.sort().values[int(q * (n - 1))].item())


def distance_field_check(distance_fn, vertices, triangles, threshold, box=None, n=100000, seed=0, bins=8, method="bvh", return_samples=False):
    """How well a field is a DISTANCE field in the whole volume -- level_set_check's question without its band: (vertices, triangles)
    is the mesh of the level set D = threshold (extract_mesh), distance_fn(p [M, 3]) -> D [M] the field, and F = |D(p) - threshold| is
    set against the exact distance d(p) from p to the mesh (point_mesh_distance; method="bvh" by default: the queries are far from
    the surface, where the grid walks many shells) at n points of `box`, and reported BY DISTANCE from the surface.

    box = (lo, hi): by default the bounds of the mesh's valid triangles widened on every side by a quarter of their diagonal.  The
    points: u_k = frac((k + 1) * (0.8191725133961645, 0.6710436067037893, 0.5497004779019702) + seed * 0.7548776662466927) per axis, k =
    0 .. n - 1, in fp64 (a low-discrepancy sequence; deterministic: no torch generator is touched), p_k = lo + u_k (hi - lo) rounded
    to fp32.  With e_k = F_k - d_k the dict holds

      n, box, invalid                     the points, the box, and how many D_k or d_k were not finite (left out of everything below)
      mean_error, mean_abs_error, rms_error, max_abs_error     of e_k
      max_distance                        the largest d_k
      bins                                a list of `bins` dicts over equal-width ranges of d up to max_distance, each with lo, hi, count,
                                          mean_error, mean_abs_error, and slope_median, slope_p99, n_slope of F_k / d_k over its points
                                          with d_k >= max_distance / (8 bins) -- an eighth of a bin, what band / 8 is to level_set_check:
                                          closer to the surface the mesh's own error dominates the quotient (NaN for an empty bin)
      suggested_step_scale                min(1, 1 / the largest slope_p99 of any bin): level_set_check's formula on the worst range

    Reductions are torch fp64 on the device.  return_samples=True adds points, mesh_distance and field_distance (float32, all n)."""
    from .bvh import valid_bounds
    from .raycast import _mesh
    if not callable(distance_fn):
        raise NeddfError("distance_field_check: distance_fn must be callable: pos [M, 3] -> distances [M]")
    v, t = _mesh("distance_field_check", vertices, triangles)
    n, bins, threshold = int(n), int(bins), float(threshold)
    if n < 1 or bins < 1:
        raise NeddfError("distance_field_check: n and bins must be positive (got %r, %r)" % (n, bins))
    if box is None:
        lo, hi = valid_bounds(v, t)
        pad = 0.25 * sum((h - l) ** 2 for l, h in zip(lo, hi)) ** 0.5
        lo, hi = [l - pad for l in lo], [h + pad for h in hi]
    else:
        try:
            lo, hi = [float(x) for x in box[0]], [float(x) for x in box[1]]
        except (TypeError, ValueError, IndexError):
            raise NeddfError("distance_field_check: box must be (lo, hi) with 3 numbers each (got %r)" % (box,)) from None
        if len(lo) != 3 or len(hi) != 3 or not all(l <= h and abs(l) < float("inf") and abs(h) < float("inf") for l, h in zip(lo, hi)):
            raise NeddfError("distance_field_check: box must be (lo, hi) with 3 finite numbers each and lo <= hi (got %r)" % (box,))
    k = torch.arange(1, n + 1, device=v.device, dtype=torch.float64)
    step = torch.tensor(R3_STEPS, device=v.device, dtype=torch.float64)
    u = torch.frac(k[:, None] * step[None, :] + float(int(seed)) * PLASTIC_STEP)
    lo_t, hi_t = (torch.tensor(x, device=v.device, dtype=torch.float64) for x in (lo, hi))
    pts = (lo_t[None, :] + u * (hi_t - lo_t)[None, :]).float().contiguous()
    d = point_mesh_distance(pts, v, t, method=method)["distance"]
    with torch.no_grad():
        D = distance_fn(pts)
    if not isinstance(D, torch.Tensor) or D.device != pts.device or D.numel() != n:
        raise NeddfError("distance_field_check: distance_fn must return one distance per point on the points' device")
    D = D.reshape(-1).float()
    ok = torch.isfinite(D) & torch.isfinite(d)
    m = int(ok.sum().item())
    nan = float("nan")
    out = {"n": n, "box": (tuple(lo), tuple(hi)), "invalid": n - m}
    f = (D.double() - threshold).abs()[ok]
    dd = d.double()[ok]
    e = f - dd

    def errors(x):
        if not x.numel():
            return dict(mean_error=nan, mean_abs_error=nan)
        return dict(mean_error=float(x.mean().item()), mean_abs_error=float(x.abs().mean().item()))

    out.update(errors(e))
    out.update(rms_error=float((e * e).mean().sqrt().item()) if m else nan, max_abs_error=float(e.abs().max().item()) if m else nan)
    d_max = float(dd.max().item()) if m else nan
    out["max_distance"] = d_max
    width = d_max / bins if m else nan
    which = (dd / width).floor().long().clamp(0, bins - 1) if m and width > 0.0 else torch.zeros_like(dd, dtype=torch.long)
    rows, worst = [], nan
    for b in range(bins):
        sel = which == b
        row = dict(lo=b * width, hi=(b + 1) * width, count=int(sel.sum().item()))
        row.update(errors(e[sel]))
        far = sel & (dd >= width / 8.0) & (dd > 0.0)
        row["n_slope"] = int(far.sum().item())
        if row["n_slope"]:
            slope = f[far] / dd[far]
            row.update(slope_median=float(slope.median().item()), slope_p99=_quantile(slope, 0.99))
            worst = row["slope_p99"] if not worst == worst else max(worst, row["slope_p99"])
        else:
            row.update(slope_median=nan, slope_p99=nan)
        rows.append(row)
    out["bins"] = rows
    out["suggested_step_scale"] = (min(1.0, 1.0 / worst) if worst > 0.0 else 1.0) if worst == worst else nan
    if return_samples:
        out.update(points=pts, mesh_distance=d, field_distance=D)
    return out


__all__ = ["nearest", "cloud_distance", "mesh_distance", "point_mesh_distance", "closest_points", "level_set_check", "distance_field_check",
           "default_cells", "POINTS_PER_CELL"]
