"""Distances between point clouds and between meshes on the GPU: exact nearest neighbours (a uniform grid, or brute force), Chamfer
and Hausdorff distance, precision / recall / F-score at a threshold.

The reference's evaluation compares images (PSNR, SSIM: metrics.py); the distance between two SURFACES is what tells how far a sparse
extraction, an operand policy or a clean-up moved the level set.  Sampling (mesh.sample_surface) and the nearest-neighbour search are
HIP kernels (include/neddf_hip.h neddf_mesh_sample_*, neddf_nn_brute, neddf_nn_grid_build, neddf_nn_grid_query); the reductions over
the per-point distances are torch fp64 on the device.
"""
import torch

from ._lib import Context, NeddfError
from .mesh import sample_surface, surface_area

# targets per grid cell of nearest()'s default grid: a placeholder until the sweep 1, 2, 4, 8, 16 at 10^6 x 10^6 points of
# tools/time_mesh_distance.py (profiles/mesh_distance_cost.json) has been run on the device -- the fastest value goes here
POINTS_PER_CELL = 4
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


def mesh_distance(mesh_a, mesh_b, n=None, density=None, seed=0, tau=None, method="grid", return_samples=False):
    """cloud_distance between area-weighted samples of two device meshes, each (vertices float32 [V, 3], triangles int32 [T, 3]).

    Both meshes are sampled with the SAME density and seed (mesh.sample_surface), so identical meshes give identical samples and every
    distance is exactly 0.  Exactly one of `density` (samples per unit area) and `n` is given; n is turned into a density by the mean
    of the two areas, so each mesh gets about n points.  return_samples=True adds points_a / points_b, triangle_a / triangle_b and the
    per-sample distances and indices of cloud_distance: where the two surfaces differ, and by how much."""
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
    out = cloud_distance(pa, pb, tau=tau, method=method, return_samples=return_samples)
    out["density"] = float(density)
    if return_samples:
        out.update(points_a=pa, points_b=pb, triangle_a=ia, triangle_b=ib)
    return out


__all__ = ["nearest", "cloud_distance", "mesh_distance", "default_cells", "POINTS_PER_CELL"]
