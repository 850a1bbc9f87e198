"""Ray casting on triangle meshes on the GPU: the first intersection of every ray with an indexed mesh, through a uniform grid or by
brute force.

What extract_mesh writes can be looked at from the dataset's cameras (NeRFRender.render_image_mesh, scripts/render_mesh.py) and put
next to the sphere-traced view of the same level set.  The hit is the watertight test of Woop, Benthin and Wald (JCGT 2013) with exactly
specified fp32 arithmetic (include/neddf_hip.h neddf_raycast_brute; tests/raycast_check.py restates it in numpy bit for bit), and the
grid returns the brute kernel's bits (neddf_raycast_grid_count / _build / _query).  Both are HIP kernels; this module is plumbing.
A third route with the same bits, through the mesh's BVH, lives in neddf_amd.bvh (cast_rays, occluded, ambient_occlusion).
"""
import math

import torch

from ._lib import Context, NeddfError
from .geometry import MAX_CELLS, MAX_CELLS_PER_AXIS, _points, default_cells

# triangles per grid cell of build_grid()'s default grid: the fastest of the sweep 1, 2, 4, 8, 16 of tools/time_raycast.py on the MI355X
# (profiles/raycast_cost.json: 800 x 800 rays against 123 k and 503 k triangles, query 1.6 and 3.6 ms at 1 against 3.8 and 7.6 ms at 16;
# the build costs 0.4 - 0.7 ms at every value)
TRIANGLES_PER_CELL = 1
PAD_FRACTION = 2.0 ** -12           # the default pad, as a share of the box diagonal
MIN_PAD_FRACTION = 2.0 ** -16       # the library's limit: pad >= this share of the largest of |lo|, |hi| and the box extent


def _mesh(what, vertices, triangles):
    v = _points(what, "vertices", vertices)
    if not isinstance(triangles, torch.Tensor) or not triangles.is_cuda:
        raise NeddfError("%s: triangles must be a tensor on a HIP device (got %s)"
                         % (what, triangles.device if isinstance(triangles, torch.Tensor) else type(triangles).__name__))
    if triangles.dtype not in (torch.int32, torch.int64) or triangles.dim() != 2 or triangles.shape[1] != 3:
        raise NeddfError("%s: triangles must be int32 or int64 [T, 3] (got %s %s)" % (what, triangles.dtype, tuple(triangles.shape)))
    if triangles.device != v.device:
        raise NeddfError("%s: vertices and triangles must live on one device (got %s, %s)" % (what, v.device, triangles.device))
    if triangles.dtype == torch.int64:
        # an index that does not fit int32 is outside [0, V) anyway (V < 2^31): it stays invalid
        triangles = triangles.clamp(-1, 2 ** 31 - 1).to(torch.int32)
    return v, triangles.contiguous()


def _pad(what, pad):
    pad = float(pad)
    if not (pad >= 0.0 and math.isfinite(pad)):
        raise NeddfError("%s: pad must be finite and not negative (got %r)" % (what, pad))
    return pad


def _bounds(v):
    """(lo, hi) of the finite vertices as lists of Python floats; a zero box without one."""
    finite = torch.isfinite(v).all(dim=1)
    if not bool(finite.any()):
        return [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    vv = v[finite]
    return vv.min(dim=0).values.double().tolist(), vv.max(dim=0).values.double().tolist()


def default_pad(lo, hi):
    """2^-12 of the diagonal of the box lo .. hi -- and, for a thin box far from the origin, twice the library's limit, which counts
    |lo| and |hi| too."""
    diag = math.sqrt(sum((float(h) - float(l)) ** 2 for l, h in zip(lo, hi)))
    return max(PAD_FRACTION * diag, 2.0 * MIN_PAD_FRACTION * max(max(abs(l), abs(h), h - l) for l, h in zip(lo, hi)))


class MeshGrid:
    """The uniform grid of a mesh for cast_rays(): the box (lo, hi), cells (gx, gy, gz), pad, and the device lists cell_start int32
    [G + 2] and items int32 [n] (neddf_raycast_grid_build).  It belongs to the vertices and triangles it was built from."""

    def __init__(self, lo, hi, cells, pad, cell_start, items, n_vertices, n_triangles):
        self.lo, self.hi, self.cells, self.pad = tuple(lo), tuple(hi), tuple(cells), float(pad)
        self.cell_start, self.items = cell_start, items
        self.n_vertices, self.n_triangles = int(n_vertices), int(n_triangles)

    @property
    def n_overflow(self):
        """How many triangles leave the box (they are tested by every ray)."""
        g = self.cells[0] * self.cells[1] * self.cells[2]
        return int((self.cell_start[g + 1] - self.cell_start[g]).item())


def build_grid(vertices, triangles, box=None, cells=None, pad=None):
    """The MeshGrid of a device mesh (vertices float32 [V, 3], triangles int32 or int64 [T, 3]).

    box = (lo, hi): by default the bounds of the finite vertices (a triangle that leaves the box is kept in an overflow list that every
    ray tests: any box gives the same hits, a fitting one the fastest).  cells = (gx, gy, gz): by default cubic cells holding about
    TRIANGLES_PER_CELL triangles each (geometry.default_cells).  pad: the slack of the hit's bounding-box clause, by default 2^-12 of
    the box diagonal; the library refuses one below 2^-16 of the largest of |lo|, |hi| and the box extent."""
    v, t = _mesh("build_grid", vertices, triangles)
    if box is None:
        lo, hi = _bounds(v)
    else:
        try:
            lo, hi = [float(x) for x in box[0]], [float(x) for x in box[1]]
        except (TypeError, ValueError, IndexError):
            raise NeddfError("build_grid: box must be (lo, hi) with 3 numbers each (got %r)" % (box,)) from None
        if len(lo) != 3 or len(hi) != 3 or not all(l <= h and math.isfinite(l) and math.isfinite(h) for l, h in zip(lo, hi)):
            raise NeddfError("build_grid: box must be (lo, hi) with 3 finite numbers each and lo <= hi (got %r)" % (box,))
    pad = default_pad(lo, hi) if pad is None else _pad("build_grid", pad)
    if cells is None:
        cells = default_cells(t.shape[0], lo, hi, TRIANGLES_PER_CELL)
    else:
        cells = tuple(int(c) for c in cells)
        if len(cells) != 3 or min(cells) < 1 or max(cells) > MAX_CELLS_PER_AXIS or cells[0] * cells[1] * cells[2] > MAX_CELLS:
            raise NeddfError("build_grid: cells must be (gx, gy, gz), each in [1, %d], at most 2^24 in all (got %r)" % (MAX_CELLS_PER_AXIS, cells))
    ctx = Context.get(v.device)
    n = ctx.raycast_grid_count(v, t, lo, hi, cells, pad)
    start, items = ctx.raycast_grid_build(v, t, lo, hi, cells, pad, n)
    if items.shape[0] != n:
        raise NeddfError("build_grid: %d pairs listed, %d counted" % (items.shape[0], n))
    return MeshGrid(lo, hi, cells, pad, start, items, v.shape[0], t.shape[0])


def cast_rays(origins, dirs, vertices, triangles, t_min=0.0, t_max=float("inf"), method="grid", grid=None, pad=None):
    """The first hit of every ray (origins, dirs float32 [R, 3], directions of any length) with a device mesh, as a dict:

      t         float32 [R]: the ray parameter of the hit (origin + t * dir), +inf on a miss
      triangle  int32 [R]: the triangle hit, -1 on a miss
      b1, b2    float32 [R]: the hit point is p0 + b1 (p1 - p0) + b2 (p2 - p0); 0 on a miss

    Hits with t outside [t_min, t_max] do not count; triangles are two-sided; among equal t the lowest triangle index wins; a ray with
    a non-finite component or a zero direction gets (NaN, -1, NaN, NaN).  method="grid" walks a uniform grid (`grid`: a MeshGrid of
    build_grid for this mesh, built here when None) and returns the bits method="brute" returns with the same pad.  pad (None: the
    grid's, or build_grid's default for the mesh's bounds) is the slack of the hit's bounding-box clause."""
    o, d = _points("cast_rays", "origins", origins), _points("cast_rays", "dirs", dirs)
    v, t = _mesh("cast_rays", vertices, triangles)
    if o.shape != d.shape:
        raise NeddfError("cast_rays: origins and dirs must have one shape (got %s, %s)" % (tuple(o.shape), tuple(d.shape)))
    if o.device != v.device or d.device != v.device:
        raise NeddfError("cast_rays: rays and mesh must live on one device (got %s, %s, %s)" % (o.device, d.device, v.device))
    if method not in ("grid", "brute"):
        raise NeddfError("cast_rays: method must be 'grid' or 'brute' (got %r); rays through a MeshBVH are cast by neddf_amd.bvh.cast_rays" % (method,))
    if grid is not None:
        if not isinstance(grid, MeshGrid) or grid.n_vertices != v.shape[0] or grid.n_triangles != t.shape[0] or grid.cell_start.device != v.device:
            raise NeddfError("cast_rays: grid must be the MeshGrid build_grid made of this mesh")
        if pad is not None and _pad("cast_rays", pad) != grid.pad:
            raise NeddfError("cast_rays: pad %r differs from the grid's %r" % (pad, grid.pad))
    ctx = Context.get(v.device)
    if method == "brute":
        if pad is None:
            pad = grid.pad if grid is not None else default_pad(*_bounds(v))
        out = ctx.raycast_brute(o, d, v, t, t_min, t_max, _pad("cast_rays", pad))
    else:
        if grid is None:
            grid = build_grid(v, t, pad=pad)
        out = ctx.raycast_grid_query(o, d, v, t, grid.lo, grid.hi, grid.cells, grid.pad, grid.cell_start, grid.items, t_min, t_max)
    return dict(zip(("t", "triangle", "b1", "b2"), out))


__all__ = ["MeshGrid", "build_grid", "cast_rays", "default_pad", "TRIANGLES_PER_CELL"]
