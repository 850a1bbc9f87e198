"""CPU-only checks of empty-space skipping: the new entry points are declared, bound and exported and reject NULL arguments
without touching memory; argument validation of OccupancyGrid / build_occupancy; the numpy restatement the GPU tests lean on
(tests/occupancy_check.py) against scipy.ndimage."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch
from conftest import BUNNY_CFG, ROOT

import occupancy_check as oc

NEW = ("neddf_occupancy_build", "neddf_occupancy_classify", "neddf_occupancy_gather", "neddf_occupancy_scatter",
       "neddf_render_rays_culled", "neddf_render_rays_single_culled", "neddf_cull_stats")


def test_symbols_declared_bound_and_exported():
    from neddf_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "neddf_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(neddf_[a-z_]+)\s*\(", hdr))
    bound = {name for name, _, _ in _lib.SYMBOLS}
    so = os.path.join(ROOT, "neddf_amd", "csrc", "libneddf_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T"}
    for name in NEW:
        assert name in declared and name in bound and name in exported, name
    assert "NEDDF_ABI_VERSION 7" in hdr and _lib.ABI_VERSION == 7         # additive: the ABI version stays
    # the stage enum and neddf_render_params keep their layout
    assert "NEDDF_STAGE_GATHER = 10, NEDDF_STAGE_COUNT = 11" in hdr
    assert len(_lib.STAGES) == 11


def test_occupancy_struct_layout_matches_header(tmp_path):
    from neddf_amd import _lib
    src = '#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%%zu %%zu %%zu %%zu %%zu", sizeof(neddf_occupancy), ' \
          'offsetof(neddf_occupancy, res), offsetof(neddf_occupancy, lo), offsetof(neddf_occupancy, inv_cell), ' \
          'sizeof(neddf_render_params)); return 0;}' % os.path.join(ROOT, "include", "neddf_hip.h")
    exe = str(tmp_path / "sizes")
    subprocess.run(["gcc", "-x", "c", "-", "-o", exe], input=src.encode(), check=True)
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    O = _lib.Occupancy
    assert got == [C.sizeof(O), O.res.offset, O.lo.offset, O.inv_cell.offset, C.sizeof(_lib.RenderParams)]


def test_null_arguments_are_rejected_without_touching_memory():
    from neddf_amd import _lib
    lib = _lib.load()
    table = {name: args for name, _, args in _lib.SYMBOLS}
    for name in NEW:
        call = [a(0) if a in (C.c_int, C.c_int64) else a(0.0) if a in (C.c_float, C.c_double) else None for a in table[name]]
        assert getattr(lib, name)(*call) == -1, name


def test_grid_argument_validation():
    from neddf_amd.occupancy import OccupancyGrid, pack_bits
    lo, hi = (-1.0,) * 3, (1.0,) * 3
    words = lambda R: torch.zeros((R ** 3 + 31) // 32, dtype=torch.int32)      # noqa: E731
    g = OccupancyGrid(words(5), 5, lo, hi)
    assert g.resolution == 5 and g.to_dense().shape == (5, 5, 5) and g.occupied_fraction == 0.0
    for R in (0, -3, 1025, 2.5):
        with pytest.raises(ValueError):
            OccupancyGrid(words(5), R, lo, hi)
    with pytest.raises(ValueError):
        OccupancyGrid(words(5), 4, lo, hi)                  # word count of another resolution
    with pytest.raises(ValueError):
        OccupancyGrid(words(5).float(), 5, lo, hi)
    for bad_lo, bad_hi in (((1.0, -1.0, -1.0), hi), (lo, (1.0, -1.0, 1.0)), ((float("nan"),) * 3, hi), (lo, (1.0, 1.0))):
        with pytest.raises(ValueError):
            OccupancyGrid(words(5), 5, bad_lo, bad_hi)
    # the layout of hand-made grids: bit (z R + y) R + x, and to_dense undoes pack_bits
    rng = np.random.default_rng(3)
    dense = rng.random((5, 5, 5)) < 0.3
    w = pack_bits(dense)
    assert np.array_equal(w, oc.pack(dense)) and w.dtype == np.uint32 and w.shape == (4,)
    assert int(w[-1]) >> (125 - 96) == 0
    i = (3 * 5 + 1) * 5 + 4
    one = np.zeros((5, 5, 5), bool)
    one[3, 1, 4] = True
    assert int(pack_bits(one)[i >> 5]) == 1 << (i & 31)
    g = OccupancyGrid(torch.from_numpy(w.view(np.int32)), 5, lo, hi)
    assert np.array_equal(g.to_dense().numpy(), dense) and g.occupied_fraction == dense.sum() / 125.0
    # a grid that is not on a HIP device cannot reach the library: no CPU fallback
    from neddf_amd import NeddfError
    with pytest.raises(NeddfError):
        g.descriptor()
    # from_field validates before it touches a device
    for kw in (dict(resolution=0), dict(resolution=1025), dict(dilate=5), dict(dilate=-1), dict(lo=(0, 0, 0), hi=(0, 1, 1)),
               dict(lo=(0, 0, 0))):
        with pytest.raises(ValueError):
            OccupancyGrid.from_field(None, **kw)


def test_render_argument_validation():
    import neddf_amd
    render = neddf_amd.NeRFRender(dict(BUNNY_CFG, _target_="neddf.network.NeDDF"), sample_coarse=4, sample_fine=4,
                                  use_coarse_network=False, ray_space="ndc")
    assert render.occupancy is None and neddf_amd.NeRFRender.occupancy is None
    with pytest.raises(NotImplementedError):
        render.build_occupancy(resolution=8)
    render.ray_space = "world"
    for kw in (dict(resolution=0), dict(resolution=2000), dict(dilate=5), dict(lo=(1, 1, 1), hi=(0, 0, 0))):
        with pytest.raises(ValueError):
            render.build_occupancy(**kw)
    from neddf_amd.occupancy import OccupancyGrid
    render.occupancy = OccupancyGrid(torch.zeros(1, dtype=torch.int32), 1, (-1,) * 3, (1,) * 3)      # a CPU grid
    with pytest.raises(ValueError):
        render._occupancy_desc(torch.device("cuda", 0))          # a grid on another device than the camera
    render.ray_space = "ndc"
    with pytest.raises(NotImplementedError):
        render._occupancy_desc(torch.device("cpu"))
    render.occupancy = None
    assert render._occupancy_desc(torch.device("cuda", 0)) is None


@pytest.mark.parametrize("R,d", [(1, 1), (5, 0), (5, 1), (7, 4), (12, 2), (9, 3)])
def test_restatement_against_scipy(R, d):
    from scipy import ndimage
    rng = np.random.default_rng(100 * R + d)
    vol = rng.standard_normal((R + 1,) * 3).astype(np.float32) - np.float32(1.2)
    vol[rng.random(vol.shape) < 0.01] = np.nan
    vol[-1, -1, 0] = np.nan
    vol[0, 0, 0] = 5.0                                      # an occupied cell at a box corner: clipping
    vol[rng.random(vol.shape) < 0.02] = 0.25                # equal to the threshold: not occupied by itself
    thr = 0.25
    with np.errstate(invalid="ignore"):
        corner = ~(vol <= np.float32(thr))
    # a window of 2 covers [i - 1, i]: output i + 1 is cell i
    raw = ndimage.maximum_filter(corner.astype(np.uint8), size=2, mode="constant", cval=0)[1:, 1:, 1:].astype(bool)
    assert np.array_equal(oc.cell_occupancy(vol, thr), raw)
    assert raw[0, 0, 0] and raw[-1, -1, 0]                  # the NaN corner occupies its cell
    want = ndimage.maximum_filter(raw.astype(np.uint8), size=2 * d + 1, mode="constant", cval=0).astype(bool)
    dense, words, n = oc.build(vol, thr, d)
    assert np.array_equal(dense, want) and n == int(want.sum())
    assert np.array_equal(oc.unpack(words, R), want) and words.shape == ((R ** 3 + 31) // 32,)


def test_restatement_classify_edges():
    R, lo, hi = 4, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    dense = np.zeros((R, R, R), bool)
    dense[1, 2, 3] = True                                    # [z, y, x]
    pts = np.array([[0.75, 0.25, -0.25],                     # inside cell (3, 2, 1): set
                    [0.5, 0.0, -0.5],                        # on that cell's lower faces: still the cell
                    [0.25, 0.25, -0.25],                     # the neighbour in x: clear
                    [-1.0, -1.0, -1.0],                      # lo exactly: cell (0, 0, 0), clear
                    [1.0, 0.0, 0.0],                         # hi exactly: outside, kept
                    [np.nextafter(np.float32(-1), np.float32(-2)), 0, 0],        # one ulp outside
                    [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], np.float32)
    assert oc.classify(dense, lo, hi, pts).tolist() == [1, 1, 0, 0, 1, 1, 1, 1, 1]
    keep = oc.classify(dense, lo, hi, pts)
    index, rows = oc.gather(keep, pts)
    assert index.tolist() == [0, 1, 4, 5, 6, 7, 8] and rows.view(np.uint32).tolist() == pts[index].view(np.uint32).tolist()
    (full,) = oc.scatter(index, len(pts), rows)
    assert np.array_equal(full.view(np.uint32)[keep == 1], pts.view(np.uint32)[keep == 1]) and not full.view(np.uint32)[keep == 0].any()
