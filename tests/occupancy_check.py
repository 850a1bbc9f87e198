"""numpy restatements of neddf_amd/csrc/occupancy_kernels.hip, bit for bit (the counterpart of mesh_clean_check.py): what the GPU
tests of the occupancy grid compare against.  tests/test_occupancy_host.py pins the dilation here on scipy.ndimage."""
import numpy as np


def cell_occupancy(volume, threshold):
    """[R+1]^3 corner densities ([z, y, x]) -> bool [R, R, R]: any corner with !(v <= threshold), so a NaN corner occupies."""
    v = np.asarray(volume, np.float32)
    with np.errstate(invalid="ignore"):
        c = ~(v <= np.float32(threshold))
    R = v.shape[0] - 1
    occ = np.zeros((R, R, R), bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                occ |= c[dz:dz + R, dy:dy + R, dx:dx + R]
    return occ


def dilate(occ, d):
    """Chebyshev (26-neighbour) dilation by d cells, clipped at the box: the union of all shifts by at most d per axis."""
    occ = np.asarray(occ, bool)
    out = occ.copy()
    for axis in range(3):
        src = out.copy()
        n = src.shape[axis]
        for k in range(1, min(d, n - 1) + 1):
            a = [slice(None)] * 3
            b = [slice(None)] * 3
            a[axis], b[axis] = slice(k, None), slice(None, n - k)
            out[tuple(a)] |= src[tuple(b)]
            out[tuple(b)] |= src[tuple(a)]
    return out


def pack(dense):
    """bool [R, R, R] -> uint32 words: bit (z R + y) R + x in word i >> 5 at position i & 31, unused high bits 0."""
    flat = np.asarray(dense, bool).reshape(-1)
    padded = np.zeros((flat.size + 31) // 32 * 32, np.uint64)
    padded[:flat.size] = flat
    return (padded.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)


def unpack(words, R):
    w = np.asarray(words).view(np.uint32).astype(np.uint64)
    return ((w[:, None] >> np.arange(32, dtype=np.uint64)) & 1).reshape(-1)[:R ** 3].reshape(R, R, R).astype(bool)


def build(volume, threshold, d):
    """(dense bool [R, R, R], words uint32, number of occupied cells) of neddf_occupancy_build."""
    dense = dilate(cell_occupancy(volume, threshold), d)
    return dense, pack(dense), int(dense.sum())


def descriptor(R, lo, hi):
    """(lo fp32 [3], inv_cell fp32 [3]): inv_cell = (float)(R / (hi - lo)), the quotient in double."""
    lo64, hi64 = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    return lo64.astype(np.float32), (np.float64(R) / (hi64 - lo64)).astype(np.float32)


def classify(dense, lo, hi, points):
    """uint8 [N]: per axis c = floor((p - lo) * inv_cell) in fp32, in that order; outside [0, R) on any axis or not finite:
    kept; inside: the cell's bit."""
    dense = np.asarray(dense, bool)
    R = dense.shape[0]
    lo32, inv = descriptor(R, lo, hi)
    p = np.asarray(points, np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(((p - lo32[None, :]).astype(np.float32) * inv[None, :]).astype(np.float32))
        inside = ((f >= 0) & (f < np.float32(R))).all(1)          # NaN / Inf compare false
    keep = np.ones(p.shape[0], np.uint8)
    c = f[inside].astype(np.int64)
    keep[inside] = dense[c[:, 2], c[:, 1], c[:, 0]]
    return keep


def gather(keep, *rows):
    """(index int32 [M], the kept rows of every array) in their old order."""
    index = np.nonzero(np.asarray(keep) != 0)[0].astype(np.int32)
    return (index,) + tuple(np.asarray(r)[index] for r in rows)


def scatter(index, n, *compact):
    """zero-filled arrays of n rows with row index[k] = row k of every compact array."""
    out = []
    for c in compact:
        c = np.asarray(c)
        full = np.zeros((n,) + c.shape[1:], c.dtype)
        full[index] = c
        out.append(full)
    return tuple(out)
