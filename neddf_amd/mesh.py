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


def write_ply(path, vertices, triangles):
    """Binary little-endian PLY: vertex (float x, y, z), face (list uchar int vertex_indices)."""
    v = np.ascontiguousarray(vertices.detach().cpu().numpy() if isinstance(vertices, torch.Tensor) else vertices, dtype="<f4")
    t = np.ascontiguousarray(triangles.detach().cpu().numpy() if isinstance(triangles, torch.Tensor) else triangles, dtype="<i4")
    if v.ndim != 2 or v.shape[1] != 3 or t.ndim != 2 or t.shape[1] != 3:
        raise ValueError("write_ply: vertices [V, 3] and triangles [T, 3] expected (got %s, %s)" % (v.shape, t.shape))
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), len(t)))
    faces = np.empty(len(t), dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    faces["n"] = 3
    faces["i"] = t
    with open(path, "wb") as fh:
        fh.write(head.encode("ascii"))
        fh.write(v.tobytes())
        fh.write(faces.tobytes())
    return path


__all__ = ["marching_cubes", "write_ply"]
