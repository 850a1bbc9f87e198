"""numpy restatement of the brick-wise surface extraction (include/neddf_hip.h: neddf_field_grid_coarse, neddf_brick_select,
neddf_field_bricks, neddf_marching_cubes_bricks) for the tests.

Bricks of B^3 cells over an nx x ny x nz lattice: nb = ceil((n - 1) / B) per axis, brick (bx, by, bz) at (bz nby + by) nbx + bx; a
brick's lattice is (B+1)^3 points, local index (lz (B+1) + ly)(B+1) + lx, NaN past the fine lattice.  The restricted mesh is
mesh_check.marching_cubes on the dense volume with the triangles whose cell lies in an active brick kept in order, the vertices
nothing references dropped and the triangles reindexed."""
import numpy as np

import mesh_check as mc


def brick_counts(shape, B):
    """(nbx, nby, nbz) of the lattice shape = (nx, ny, nz)."""
    return tuple(-(-(int(n) - 1) // int(B)) for n in shape)


def coarse_indices(n, B):
    """Fine lattice indices of the brick corners along one axis: min(b B, n - 1), b = 0 .. nb."""
    nb = -(-(int(n) - 1) // int(B))
    return np.minimum(np.arange(nb + 1) * int(B), int(n) - 1)


def coarse_volume(vol, B):
    """[nbz+1, nby+1, nbx+1]: the dense [nz, ny, nx] volume at the brick corners."""
    nz, ny, nx = vol.shape
    return np.ascontiguousarray(vol[np.ix_(coarse_indices(nz, B), coarse_indices(ny, B), coarse_indices(nx, B))])


def default_band(B, spacing, lipschitz=1.0):
    """lipschitz * half the diagonal of a brick of B cells of size spacing = (hx, hy, hz)."""
    return float(lipschitz) * 0.5 * int(B) * float(np.sqrt(sum(float(h) ** 2 for h in spacing)))


def select(coarse, iso, band, dilate=0):
    """(slot_map int32 [nbz, nby, nbx], brick_ids int32 [M]) of a float32 coarse volume, as neddf_brick_select gives them."""
    c = np.asarray(coarse, np.float32)
    iso, band = np.float32(iso), np.float32(band)
    corners = np.stack([c[dz:c.shape[0] - 1 + dz, dy:c.shape[1] - 1 + dy, dx:c.shape[2] - 1 + dx]
                        for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)])
    with np.errstate(invalid="ignore"):
        inside = corners < iso
        near = np.abs(corners - iso) <= band
    active = np.isnan(corners).any(0) | near.any(0) | (inside.any(0) & ~inside.all(0))
    d = int(dilate)
    if d:
        grown = np.zeros_like(active)
        nz, ny, nx = active.shape
        for z, y, x in zip(*np.nonzero(active)):
            grown[max(z - d, 0):z + d + 1, max(y - d, 0):y + d + 1, max(x - d, 0):x + d + 1] = True
        active = grown
    return slots_of(active)


def slots_of(active):
    """(slot_map, brick_ids) of a bool [nbz, nby, nbx] array of active bricks."""
    flat = np.asarray(active, bool).reshape(-1)
    ids = np.nonzero(flat)[0].astype(np.int32)
    slot = np.full(flat.size, -1, np.int32)
    slot[ids] = np.arange(ids.size, dtype=np.int32)
    return slot.reshape(np.shape(active)), ids


def brick_values(vol, brick_ids, B):
    """float32 [M, (B+1)^3]: the dense volume gathered onto the listed bricks' lattices, quiet NaN past the fine lattice."""
    vol = np.asarray(vol, np.float32)
    nz, ny, nx = vol.shape
    nbx, nby, nbz = brick_counts((nx, ny, nz), B)
    L = B + 1
    out = np.full((len(brick_ids), L, L, L), np.nan, np.float32)
    for m, b in enumerate(np.asarray(brick_ids, np.int64)):
        bx, by, bz = b % nbx, (b // nbx) % nby, b // (nbx * nby)
        z0, y0, x0 = bz * B, by * B, bx * B
        sub = vol[z0:z0 + L, y0:y0 + L, x0:x0 + L]
        out[m, :sub.shape[0], :sub.shape[1], :sub.shape[2]] = sub
    return out.reshape(len(brick_ids), L ** 3)


def cell_cases(vol, iso):
    """Marching-cubes case int [nz-1, ny-1, nx-1] of every cell (corner b inside -> bit b, Bourke's numbering)."""
    ins = np.asarray(vol, np.float32) < np.float32(iso)
    nz, ny, nx = ins.shape
    case = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
    for b, (dx, dy, dz) in enumerate([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]):
        case |= ins[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx].astype(np.int64) << b
    return case


def cell_bricks(shape_zyx, B, nb):
    """Brick index int [nz-1, ny-1, nx-1] of every cell."""
    nz, ny, nx = shape_zyx
    nbx, nby, nbz = nb
    z, y, x = np.meshgrid(np.arange(nz - 1) // B, np.arange(ny - 1) // B, np.arange(nx - 1) // B, indexing="ij")
    return (z * nby + y) * nbx + x


def restricted_mesh(vol, iso, lo, hi, active, B):
    """(vertices, triangles) of the dense mesh restricted to the cells of the active bricks (bool [nbz, nby, nbx])."""
    vol = np.ascontiguousarray(vol, np.float32)
    verts, tris = mc.marching_cubes(vol, iso, lo, hi)
    nz, ny, nx = vol.shape
    nb = brick_counts((nx, ny, nz), B)
    case = cell_cases(vol, iso).reshape(-1)
    per_cell = (mc.TRI_TABLE[case] >= 0).sum(1) // 3
    assert per_cell.sum() == len(tris)
    tri_brick = np.repeat(cell_bricks(vol.shape, B, nb).reshape(-1), per_cell)
    keep = np.asarray(active, bool).reshape(-1)[tri_brick]
    kept = tris[keep]
    used = np.zeros(len(verts), bool)
    used[kept.reshape(-1)] = True
    new_id = np.cumsum(used) - 1
    return verts[used], new_id[kept].astype(np.int32).reshape(-1, 3)


def crossing_bricks(vol, iso, B):
    """bool [nbz, nby, nbx]: the bricks that hold a cell with a crossing; and the number of such cells."""
    vol = np.asarray(vol, np.float32)
    nz, ny, nx = vol.shape
    nb = brick_counts((nx, ny, nz), B)
    case = cell_cases(vol, iso)
    crossing = (case != 0) & (case != 255)
    hit = np.zeros(nb[0] * nb[1] * nb[2], bool)
    hit[cell_bricks(vol.shape, B, nb)[crossing]] = True
    return hit.reshape(nb[::-1]), int(crossing.sum())
