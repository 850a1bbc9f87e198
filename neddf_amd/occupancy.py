"""Empty-space skipping: an occupancy bitfield over a box, built from a field's density lattice (not a reference feature:
the reference evaluates every sample of every ray).

The grid has R^3 cells; cell (x, y, z) is bit (z R + y) R + x, bit i in word i >> 5 at position i & 31.  A cell is occupied
when any of its 8 corner densities satisfies !(v <= threshold) -- a NaN corner occupies it -- and the occupied set is grown
by `dilate` cells in the Chebyshev sense.  A sample point is KEPT when it lies outside the box or is not finite (the grid
claims nothing about space it never looked at) and otherwise exactly when its cell's bit is set; the culled render passes
(NeRFRender.occupancy) evaluate the field on the kept samples only and give every other sample density 0, colour 0, normal 0.
"""
from typing import Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from ._lib import Context, NeddfError, Occupancy

MAX_RESOLUTION, MAX_DILATE = 1024, 4


def _box(lo, hi):
    lo, hi = [float(x) for x in lo], [float(x) for x in hi]
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError("lo / hi must hold three values (x, y, z)")
    if not all(a < b for a, b in zip(lo, hi)):         # NaN bounds fail too
        raise ValueError("lo < hi is required on every axis (got lo=%s, hi=%s)" % (lo, hi))
    return tuple(lo), tuple(hi)


def _check_resolution(resolution):
    R = int(resolution)
    if R != resolution or not 1 <= R <= MAX_RESOLUTION:
        raise ValueError("resolution must be an integer in [1, %d] (got %r)" % (MAX_RESOLUTION, resolution))
    return R


def _check_dilate(dilate):
    d = int(dilate)
    if d != dilate or not 0 <= d <= MAX_DILATE:
        raise ValueError("dilate must be an integer in [0, %d] (got %r)" % (MAX_DILATE, dilate))
    return d


class OccupancyGrid:
    """bits: int32 / uint32 tensor of (R^3 + 31) // 32 words on a HIP device; lo / hi: the box (three floats each)."""

    def __init__(self, bits: Tensor, resolution: int, lo: Sequence[float], hi: Sequence[float]) -> None:
        self.resolution = _check_resolution(resolution)
        self.lo, self.hi = _box(lo, hi)
        if not isinstance(bits, Tensor) or bits.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
            raise ValueError("bits must be an int32 / uint32 tensor")
        words = (self.resolution ** 3 + 31) // 32
        if bits.dim() != 1 or bits.shape[0] != words:
            raise ValueError("bits must hold %d words for resolution %d (got shape %s)" % (words, self.resolution, tuple(bits.shape)))
        self.bits = bits.contiguous().view(torch.int32)
        self._n_occupied: Optional[int] = None

    @property
    def device(self) -> torch.device:
        return self.bits.device

    def descriptor(self) -> Occupancy:
        """The library's neddf_occupancy: lo in fp32, inv_cell = (float)(R / (hi - lo)) with the quotient in double."""
        if not self.bits.is_cuda:
            raise NeddfError("the occupancy bits must live on a HIP device (got %s); there is no CPU fallback" % self.bits.device)
        o = Occupancy()
        o.d_bits = self.bits.data_ptr()
        o.res = self.resolution
        for a in range(3):
            o.lo[a] = self.lo[a]
            o.inv_cell[a] = self.resolution / (self.hi[a] - self.lo[a])
        return o

    @classmethod
    def from_field(cls, field, resolution: int = 128, cube_range: float = 1.1, threshold: float = 0.0, dilate: int = 1,
                   lo=None, hi=None) -> "OccupancyGrid":
        """The grid of `field`'s density: the [R+1]^3 lattice of cell corners over [-cube_range, cube_range]^3 (or lo .. hi)
        is evaluated as extract_mesh evaluates its lattice (neddf_field_grid: dir = (1, 0, 0), var = 0) and turned into bits
        on the device."""
        R, d = _check_resolution(resolution), _check_dilate(dilate)
        if (lo is None) != (hi is None):
            raise ValueError("give both lo and hi, or neither")
        if lo is None:
            lo, hi = (-float(cube_range),) * 3, (float(cube_range),) * 3
        lo, hi = _box(lo, hi)
        names = field._grid_fields()
        with torch.no_grad():
            ctx = Context.get(field.device)
            field.upload(ctx, field._slot)
            vol = ctx.field_grid(field._slot, names["density"], (R + 1,) * 3, lo, hi)
            bits, n = ctx.occupancy_build(vol, float(threshold), d)
        grid = cls(bits, R, lo, hi)
        grid._n_occupied = n
        return grid

    def union_(self, other: "OccupancyGrid") -> "OccupancyGrid":
        """ORs another grid of the same resolution and box into this one."""
        if (other.resolution, other.lo, other.hi) != (self.resolution, self.lo, self.hi) or other.device != self.device:
            raise ValueError("union_: the grids must share resolution, box and device")
        self.bits |= other.bits
        self._n_occupied = None
        return self

    def classify(self, points: Tensor) -> Tensor:
        """bool [...]: True for the points [..., 3] the grid keeps."""
        if points.device != self.device:
            raise ValueError("classify: points on %s, grid on %s" % (points.device, self.device))
        keep = Context.get(self.device).occupancy_classify(self.descriptor(), points)
        return keep.view(points.shape[:-1]).bool()

    def to_dense(self) -> Tensor:
        """bool [R, R, R] indexed [z, y, x] (for inspection and tests)."""
        R = self.resolution
        shifts = torch.arange(32, device=self.device, dtype=torch.int32)
        flat = ((self.bits[:, None] >> shifts[None, :]) & 1).reshape(-1)[:R ** 3]
        return flat.reshape(R, R, R).bool()

    @property
    def n_occupied(self) -> int:
        if self._n_occupied is None:
            self._n_occupied = int(self.to_dense().sum().item())
        return self._n_occupied

    @property
    def occupied_fraction(self) -> float:
        return self.n_occupied / float(self.resolution ** 3)


def pack_bits(dense) -> np.ndarray:
    """bool [R, R, R] ([z, y, x]) -> the uint32 words of the grid's layout (host-side helper for hand-made grids)."""
    flat = np.asarray(dense, bool).reshape(-1)
    padded = np.zeros((flat.size + 31) // 32 * 32, np.uint64)
    padded[:flat.size] = flat
    return (padded.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)
