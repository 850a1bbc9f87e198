"""Brick-wise surface extraction without a GPU: the numpy checker (tests/sparse_mesh_check.py) against the dense checker, and the
brick selection on the CPU oracle's bunny distance -- the end-to-end input of tests/test_gpu_sparse_mesh.py, pinned independently
of the code under test."""
import numpy as np

import mesh_check as mc
import sparse_mesh_check as sm


def _sphere(n=33, r=0.55):
    ax = np.linspace(-1, 1, n)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    return (np.sqrt(x * x + y * y + z * z) - r).astype(np.float32)


def _same(a, b):
    return (a[0].shape == b[0].shape and np.array_equal(a[0].view(np.int32), b[0].view(np.int32))
            and a[1].shape == b[1].shape and np.array_equal(a[1], b[1]))


def test_checker_all_and_no_bricks():
    rng = np.random.default_rng(3)
    lo, hi = (0, 0, 0), (1, 2, 3)
    for vol, iso in ((_sphere(), 0.0), (rng.standard_normal((11, 9, 14)).astype(np.float32), 0.1)):
        dense = mc.marching_cubes(vol, iso, lo, hi)
        assert len(dense[1])
        for B in (2, 4, 5, 16):
            nb = sm.brick_counts(vol.shape[::-1], B)
            assert _same(sm.restricted_mesh(vol, iso, lo, hi, np.ones(nb[::-1], bool), B), dense), B
            v, t = sm.restricted_mesh(vol, iso, lo, hi, np.zeros(nb[::-1], bool), B)
            assert v.shape == (0, 3) and t.shape == (0, 3)


def test_checker_conventions():
    assert sm.brick_counts((61, 64, 2), 4) == (15, 16, 1)
    assert sm.coarse_indices(64, 8).tolist() == [0, 8, 16, 24, 32, 40, 48, 56, 63]          # 63 cells: a partial last brick
    assert sm.coarse_indices(61, 4)[-1] == 60 and len(sm.coarse_indices(61, 4)) == 16
    vol = np.arange(5 * 6 * 7, dtype=np.float32).reshape(5, 6, 7)
    nb = sm.brick_counts((7, 6, 5), 4)
    assert nb == (2, 2, 1)
    vals = sm.brick_values(vol, np.arange(4), 4).reshape(4, 5, 5, 5)
    assert np.array_equal(vals[0], vol[:5, :5, :5])
    assert np.array_equal(vals[3, :, :2, :3], vol[:5, 4:6, 4:7]) and np.isnan(vals[3, :, 2:, :]).all() and np.isnan(vals[3, :, :, 3:]).all()
    coarse = sm.coarse_volume(vol, 4)
    assert coarse.shape == (2, 3, 3) and coarse[1, 2, 2] == vol[4, 5, 6] and coarse[0, 1, 1] == vol[0, 4, 4]
    # selection: a sign change, a corner inside the band, a NaN corner; dilation is Chebyshev and clipped
    c = np.full((2, 2, 6), 1.0, np.float32)
    slot, ids = sm.select(c, 0.0, 0.5)
    assert ids.size == 0 and (slot == -1).all()
    c[0, 0, 0] = -1.0
    c[1, 1, 3] = 0.5                        # exactly iso + band: inside the band
    assert sm.select(c, 0.0, 0.5)[1].tolist() == [0, 2, 3]
    assert sm.select(c, 0.0, np.nextafter(np.float32(0.5), np.float32(0)))[1].tolist() == [0]
    c[0, 1, 5] = np.nan
    slot, ids = sm.select(c, 0.0, 0.0)
    assert ids.tolist() == [0, 4] and slot.reshape(-1).tolist() == [0, -1, -1, -1, 1]
    assert sm.select(c, 0.0, 0.0, dilate=1)[1].tolist() == [0, 1, 3, 4]


def test_checker_sphere_at_the_default_band():
    """A distance to a sphere is 1-Lipschitz: the default band keeps every brick the surface crosses, and the restricted mesh is the
    dense one although most bricks are dropped."""
    vol = _sphere(41)
    lo, hi = (-1, -1, -1), (1, 1, 1)
    dense = mc.marching_cubes(vol, 0.0, lo, hi)
    for B in (4, 8):
        slot, ids = sm.select(sm.coarse_volume(vol, B), 0.0, sm.default_band(B, (2 / 40,) * 3))
        hit, cells = sm.crossing_bricks(vol, 0.0, B)
        assert cells > 0 and not (hit & (slot < 0)).any()
        assert 0 < ids.size < slot.size
        assert _same(sm.restricted_mesh(vol, 0.0, lo, hi, slot >= 0, B), dense), B


def test_selection_covers_the_oracle_bunny():
    """The shipped bunny network's distance on the 61^3 lattice over +-1.1 by the CPU oracle, bricks of 4^3 cells, iso 0.1, the
    default band at lipschitz = 1: every cell with a crossing lies in an active brick and the selection is a proper subset.
    Measured when the test was written: 16 701 crossing cells in 920 of 3 375 bricks, 1 643 active, none missed (the GPU's values
    differ from the oracle's in the last bits, so the counts themselves are not asserted)."""
    from neddf_amd.fixtures import BUNNY_SMOKE_CFG, bunny_smoke_weights
    from oracle.oracle import NeDDFOracle
    n, r, B, iso = 61, 1.1, 4, 0.1
    ax = np.linspace(-r, r, n)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    pos = np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)
    dirs = np.broadcast_to(np.array([1, 0, 0], np.float32), pos.shape).copy()
    net = NeDDFOracle(bunny_smoke_weights(), **BUNNY_SMOKE_CFG)
    vol = net.forward_fast(pos, dirs, np.zeros_like(pos))["distance"].reshape(n, n, n)
    h = 2 * r / (n - 1)
    slot, ids = sm.select(sm.coarse_volume(vol, B), iso, sm.default_band(B, (h, h, h), 1.0))
    hit, cells = sm.crossing_bricks(vol, iso, B)
    missed = int((hit & (slot < 0)).sum())
    print("crossing cells %d, bricks %d, holding a crossing %d, active %d, missed %d" % (cells, slot.size, int(hit.sum()), ids.size, missed))
    assert cells > 0 and missed == 0
    assert 0 < ids.size < slot.size
    half = sm.select(sm.coarse_volume(vol, B), iso, sm.default_band(B, (h, h, h), 0.5))      # how much slack the rule has (1 338 active, 0 missed)
    print("lipschitz 0.5: active %d, missed %d" % (half[1].size, int((hit & (half[0] < 0)).sum())))


def test_abi_is_additive_and_rejects_bad_arguments_without_a_device():
    import ctypes as C
    import os
    from conftest import ROOT
    from neddf_amd import _lib
    from neddf_amd import mesh
    names = ("neddf_field_grid_coarse", "neddf_brick_select", "neddf_field_bricks", "neddf_marching_cubes_bricks")
    hdr = open(os.path.join(ROOT, "include", "neddf_hip.h")).read()
    have = {s[0] for s in _lib.SYMBOLS}
    for n in names:
        assert "int %s(" % n in hdr and n in have, n
    assert "NEDDF_ABI_VERSION 7" in hdr and _lib.ABI_VERSION == 7
    lib = _lib.load()
    nv = C.c_int64()
    assert lib.neddf_brick_select(None, None, 1, 1, 1, 0.0, 0.0, 0, None, None, C.byref(nv), None) == -1
    assert lib.neddf_marching_cubes_bricks(None, None, None, 0, None, 4, 4, 4, 2, None, None, 0.0, None, 0, None, 0, None, None,
                                           C.byref(nv), C.byref(nv), None) == -1
    assert callable(mesh.select_bricks) and callable(mesh.marching_cubes_bricks)
    assert _lib.Context.brick_counts((61, 64, 2), 4) == (15, 16, 1)
