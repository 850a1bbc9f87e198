"""Surface extraction: marching cubes on the GPU and a PLY writer.

The reference meshes a trained field inside its Open3D viewer (neddf/scripts/fields_visualizer.py:528-566: voxelize ->
PyMCubes -> .dae).  Here the grid evaluation and marching cubes are HIP kernels (include/neddf_hip.h neddf_field_grid,
neddf_marching_cubes); BaseNeuralField.extract_mesh and neddf/scripts/extract_mesh.py are built on this module.
"""
import numpy as np
import torch

from ._lib import Context, NeddfError


def marching_cubes(volume, iso, lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0)):
    """Iso-surface of a float32 [nz, ny, nx] device volume sampled on the lattice lo .. hi (np.linspace per axis, x fastest).

    Returns (vertices float32 [V, 3] in world units (x, y, z), triangles int32 [T, 3]) on the volume's device: one vertex per
    lattice edge the surface crosses, in a fixed order (include/neddf_hip.h neddf_marching_cubes).  A sample is inside when
    it is below `iso`; NaN samples are outside.  Each triangle's normal (p1 - p0) x (p2 - p0) points from the inside
    (below iso) to the outside."""
    if not isinstance(volume, torch.Tensor) or not volume.is_cuda:
        raise NeddfError("marching_cubes: the volume must be a tensor on a HIP device (got %s)"
                         % (volume.device if isinstance(volume, torch.Tensor) else type(volume).__name__))
    if volume.dtype != torch.float32:
        raise NeddfError("marching_cubes: the volume must be float32 (got %s)" % volume.dtype)
    if volume.dim() != 3:
        raise NeddfError("marching_cubes: the volume must be [nz, ny, nx] (got %d dimensions)" % volume.dim())
    if min(volume.shape) < 2:
        raise NeddfError("marching_cubes: every dimension must be at least 2 (got %s)" % (tuple(volume.shape),))
    return Context.get(volume.device).marching_cubes(volume.contiguous(), iso, lo, hi)


def vertex_normals(vertices, triangles):
    """Geometric vertex normals float32 [V, 3] of an indexed device mesh: the normalised, area-weighted sum of the incident
    triangles' cross products (p1 - p0) x (p2 - p0); a vertex whose sum vanishes gets (0, 0, 0).  Independent of timing
    (include/neddf_hip.h neddf_mesh_vertex_normals)."""
    if not isinstance(vertices, torch.Tensor) or not vertices.is_cuda:
        raise NeddfError("vertex_normals: the mesh must live on a HIP device")
    return Context.get(vertices.device).mesh_vertex_normals(vertices, triangles)


def _host(a, dtype):
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=dtype)


def write_ply(path, vertices, triangles, normals=None, colors=None):
    """Binary little-endian PLY: vertex (float x, y, z), face (list uchar int vertex_indices).
    normals [V, 3] append `property float nx, ny, nz`; colors [V, 3] -- floats in [0, 1] in the field's channel order, which is the
    dataset's B, G, R -- append `property uchar red, green, blue`: swapped to R, G, B, times 255, rounded half to even, clamped to
    [0, 255].  With both None the file is the plain 12-bytes-per-vertex one."""
    v = _host(vertices, "<f4")
    t = _host(triangles, "<i4")
    if v.ndim != 2 or v.shape[1] != 3 or t.ndim != 2 or t.shape[1] != 3:
        raise ValueError("write_ply: vertices [V, 3] and triangles [T, 3] expected (got %s, %s)" % (v.shape, t.shape))
    fields, props = [("p", "<f4", (3,))], "property float x\nproperty float y\nproperty float z\n"
    extra = {}
    if normals is not None:
        extra["n"] = _host(normals, "<f4")
        fields.append(("n", "<f4", (3,)))
        props += "property float nx\nproperty float ny\nproperty float nz\n"
    if colors is not None:
        c = _host(colors, np.float64)
        extra["c"] = np.clip(np.rint(np.nan_to_num(c[..., ::-1]) * 255.0), 0, 255).astype(np.uint8)       # np.rint: half to even; NaN -> 0
        fields.append(("c", "u1", (3,)))
        props += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    for k, a in extra.items():
        if a.shape != v.shape:
            raise ValueError("write_ply: normals / colors must be [V, 3] like the vertices (got %s)" % (a.shape,))
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n%s"
            "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), props, len(t)))
    if extra:
        rec = np.empty(len(v), dtype=np.dtype(fields))
        rec["p"] = v
        for k, a in extra.items():
            rec[k] = a
        vbytes = rec.tobytes()
    else:
        vbytes = v.tobytes()
    faces = np.empty(len(t), dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    faces["n"] = 3
    faces["i"] = t
    with open(path, "wb") as fh:
        fh.write(head.encode("ascii"))
        fh.write(vbytes)
        fh.write(faces.tobytes())
    return path


__all__ = ["marching_cubes", "vertex_normals", "write_ply"]
