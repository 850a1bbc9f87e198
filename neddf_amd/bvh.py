"""A bounding-volume hierarchy over the triangles of a device mesh, built on the GPU: the accelerator of point-to-mesh queries ANYWHERE
in the volume (geometry.point_mesh_distance(method="bvh"), geometry.distance_field_check), where the uniform grid of raycast.build_grid
only pays next to the surface.

A linear BVH (Karras 2012): Morton keys of the triangles' box centres (neddf_bvh_keys), an ascending torch.sort -- plumbing, as mesh.py
sorts its keys -- then topology and boxes (neddf_bvh_build).  include/neddf_hip.h states the arrays, so that another traversal (ray
casting, say) can use the same tree; tests/bvh_check.py restates keys, tree and traversal in numpy.  The kernels are HIP; this module
is plumbing.
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


__all__ = ["MeshBVH", "build_bvh"]
