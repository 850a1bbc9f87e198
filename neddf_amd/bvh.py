"""A bounding-volume hierarchy over the triangles of a device mesh, built on the GPU: the accelerator of point-to-mesh queries ANYWHERE
in the volume (geometry.point_mesh_distance(method="bvh"), geometry.distance_field_check), where the uniform grid of raycast.build_grid
only pays next to the surface -- and of ray casts through the same tree: cast_rays (the first hit, raycast.cast_rays' bits), occluded
(any hit) and ambient_occlusion, so that a script that checks a field against its mesh and then looks at that mesh builds one
accelerator, whose boxes fit the triangles where they are instead of one cell size for the whole scene.

A linear BVH (Karras 2012): Morton keys of the triangles' box centres (neddf_bvh_keys), an ascending torch.sort -- plumbing, as mesh.py
sorts its keys -- then topology and boxes (neddf_bvh_build).  include/neddf_hip.h states the arrays and both traversals;
tests/bvh_check.py restates keys, tree and the point traversal in numpy, tests/bvh_raycast_check.py the ray traversal.  The kernels are
HIP; this module is plumbing.
"""
import torch

from ._lib import Context, NeddfError


class MeshBVH:
    """The tree of a mesh: leaf_triangle int32 [T] (the triangles in Morton order), children int32 [T - 1, 2] (c >= 0: internal node c,
    c < 0: leaf ~c; node 0 is the root), boxes float32 [2 T - 1, 6] (lo.xyz, hi.xyz; internal node i at row i, leaf k at row T - 1 + k),
    and the box (lo, hi) its Morton cells were laid over.  It belongs to the vertices and triangles it was built from."""

    def __init__(self, lo, hi, leaf_triangle, children, boxes, n_vertices, n_triangles):
        self.lo, self.hi = tuple(lo), tuple(hi)
        self.leaf_triangle, self.children, self.boxes = leaf_triangle, children, boxes
        self.n_vertices, self.n_triangles = int(n_vertices), int(n_triangles)


def valid_bounds(v, t):
    """(lo, hi) of the vertices of the valid triangles (indices in [0, V), finite corners) as lists of Python floats; a zero box
    without one."""
    n_v = v.shape[0]
    if n_v and t.shape[0]:
        tl = t.long()
        ok = ((tl >= 0) & (tl < n_v)).all(dim=1)
        p = v[tl.clamp(0, n_v - 1)]
        ok &= torch.isfinite(p).all(dim=2).all(dim=1)
        if bool(ok.any()):
            pv = p[ok].reshape(-1, 3)
            return pv.min(dim=0).values.double().tolist(), pv.max(dim=0).values.double().tolist()
    return [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]


def build_bvh(vertices, triangles):
    """The MeshBVH of a device mesh (vertices float32 [V, 3], triangles int32 or int64 [T, 3]).  A triangle with an index outside
    [0, V) or a non-finite vertex stays in the tree with an empty box and is never found.  Build it once for many queries."""
    from .raycast import _mesh
    v, t = _mesh("build_bvh", vertices, triangles)
    lo, hi = valid_bounds(v, t)
    ctx = Context.get(v.device)
    keys = ctx.bvh_keys(v, t, lo, hi)
    leaf, children, boxes = ctx.bvh_build(v, t, torch.sort(keys).values.contiguous())
    return MeshBVH(lo, hi, leaf, children, boxes, v.shape[0], t.shape[0])


def bvh_of(what, v, t, bvh):
    """`bvh` validated as geometry._grid_of validates a grid, or the tree of the mesh built here."""
    if bvh is None:
        return build_bvh(v, t)
    n = t.shape[0]
    if (not isinstance(bvh, MeshBVH) or bvh.n_vertices != v.shape[0] or bvh.n_triangles != n or bvh.leaf_triangle.device != v.device
            or bvh.leaf_triangle.shape[0] != n or bvh.children.shape[0] != max(n - 1, 0) or bvh.boxes.shape[0] != max(2 * n - 1, 0)):
        raise NeddfError("%s: bvh must be the MeshBVH build_bvh made of this mesh" % what)
    return bvh


def _rays(what, origins, dirs, vertices, triangles, bvh, pad):
    """The checks of raycast.cast_rays, then the tree and the pad: (o, d, v, t, bvh, pad)."""
    from .geometry import _points
    from .raycast import _bounds, _mesh, _pad, default_pad
    o, d = _points(what, "origins", origins), _points(what, "dirs", dirs)
    v, t = _mesh(what, vertices, triangles)
    if o.shape != d.shape:
        raise NeddfError("%s: origins and dirs must have one shape (got %s, %s)" % (what, tuple(o.shape), tuple(d.shape)))
    if o.device != v.device or d.device != v.device:
        raise NeddfError("%s: rays and mesh must live on one device (got %s, %s, %s)" % (what, o.device, d.device, v.device))
    pad = default_pad(*_bounds(v)) if pad is None else _pad(what, pad)
    return o, d, v, t, bvh_of(what, v, t, bvh), pad


def cast_rays(origins, dirs, vertices, triangles, t_min=0.0, t_max=float("inf"), bvh=None, pad=None, return_visits=False):
    """raycast.cast_rays through the tree: the first hit of every ray as the dict (t, triangle, b1, b2) -- the bits method="brute" returns
    with the same pad, for any rays and any pad >= 0 -- plus `visits` (int32 [R], the leaves evaluated) when asked.  bvh: the mesh's
    MeshBVH (None: built here; the tree that point_mesh_distance(method="bvh") uses).  pad (None: raycast.default_pad of the mesh's
    bounds) is the slack of the hit's bounding-box clause; it belongs to the call, not to the tree."""
    o, d, v, t, bvh, pad = _rays("bvh.cast_rays", origins, dirs, vertices, triangles, bvh, pad)
    out = Context.get(v.device).raycast_bvh_query(o, d, v, t, bvh.leaf_triangle, bvh.children, bvh.boxes, t_min, t_max, pad, return_visits)
    return dict(zip(("t", "triangle", "b1", "b2", "visits"), out))


def occluded(origins, dirs, vertices, triangles, t_min=0.0, t_max=float("inf"), bvh=None, pad=None, return_visits=False):
    """Whether every ray meets the mesh between t_min and t_max at all: bool [R], equal to cast_rays(...)["triangle"] >= 0 -- the any-hit
    mode of the same kernel, which stops a ray at its first candidate.  With return_visits: (occluded, visits int32 [R])."""
    o, d, v, t, bvh, pad = _rays("bvh.occluded", origins, dirs, vertices, triangles, bvh, pad)
    out = Context.get(v.device).raycast_bvh_occluded(o, d, v, t, bvh.leaf_triangle, bvh.children, bvh.boxes, t_min, t_max, pad, return_visits)
    return (out[0].bool(), out[1]) if return_visits else out.bool()


def fibonacci_directions(n_dirs):
    """float32 [n_dirs, 3] (numpy): the spherical Fibonacci set, z_k = 1 - (2 k + 1) / n, azimuth k * pi (3 - sqrt 5), computed in fp64."""
    import numpy as np
    k = np.arange(int(n_dirs), dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / max(int(n_dirs), 1)
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1).astype(np.float32)


def ambient_occlusion(points, normals, vertices, triangles, n_dirs=16, radius=None, bias=None, bvh=None):
    """The open share of the hemisphere above every point: float32 [P] in [0, 1], 1 = nothing within `radius`.

    n_dirs directions of the spherical Fibonacci set (fibonacci_directions: one set for every point), each flipped into the hemisphere of
    the point's normal; the ray starts at p + bias n and runs to t = radius (None: the diagonal of the mesh's bounds; bias None: 4 pad,
    pad = raycast.default_pad of those bounds).  The result is sum_k w_k (1 - occluded_k) / sum_k w_k with w_k = |d_k . n|, and 1 when
    every weight is 0.  The rays go through occluded(); the rest is torch on the device."""
    import math

    from .geometry import _points
    from .raycast import _bounds, _mesh, default_pad
    what = "bvh.ambient_occlusion"
    p, nrm = _points(what, "points", points), _points(what, "normals", normals)
    v, t = _mesh(what, vertices, triangles)
    if p.shape != nrm.shape:
        raise NeddfError("%s: points and normals must have one shape (got %s, %s)" % (what, tuple(p.shape), tuple(nrm.shape)))
    if p.device != v.device or nrm.device != v.device:
        raise NeddfError("%s: points and mesh must live on one device (got %s, %s, %s)" % (what, p.device, nrm.device, v.device))
    n_dirs = int(n_dirs)
    if n_dirs < 1:
        raise NeddfError("%s: n_dirs must be at least 1 (got %r)" % (what, n_dirs))
    lo, hi = _bounds(v)
    pad = default_pad(lo, hi)
    radius = math.sqrt(sum((h - l) ** 2 for l, h in zip(lo, hi))) if radius is None else float(radius)
    bias = 4.0 * pad if bias is None else float(bias)
    if not (radius >= 0.0 and math.isfinite(bias)):
        raise NeddfError("%s: radius must not be negative and bias must be finite (got %r, %r)" % (what, radius, bias))
    bvh = bvh_of(what, v, t, bvh)
    n_pts = p.shape[0]
    dirs = torch.from_numpy(fibonacci_directions(n_dirs)).to(v.device)                        # [K, 3]
    dot = (nrm[:, 0:1] * dirs[None, :, 0] + nrm[:, 1:2] * dirs[None, :, 1]) + nrm[:, 2:3] * dirs[None, :, 2]          # [P, K], no matrix product
    d = torch.where((dot < 0)[:, :, None], -dirs[None], dirs[None]).expand(n_pts, n_dirs, 3)
    o = (p + bias * nrm)[:, None, :].expand(n_pts, n_dirs, 3)
    occ = occluded(o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous(), v, t, 0.0, radius, bvh, pad).reshape(n_pts, n_dirs)
    w = dot.abs()
    total = w.sum(dim=1)
    open_ = (w * (~occ).to(torch.float32)).sum(dim=1)
    return torch.where(total > 0, open_ / total, torch.ones_like(total))


# (the star-import list stays the tree's: `cast_rays` would shadow raycast.cast_rays for whoever star-imports both modules; the ray
# queries are reached as bvh.cast_rays, bvh.occluded, bvh.ambient_occlusion)
__all__ = ["MeshBVH", "build_bvh"]
