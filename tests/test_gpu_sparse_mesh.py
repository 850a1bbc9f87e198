"""Brick-wise surface extraction on the GPU: neddf_brick_select, neddf_field_bricks and neddf_marching_cubes_bricks against the numpy
restatement (tests/sparse_mesh_check.py) bit for bit, the two-call protocol and the argument checks, BaseNeuralField.extract_mesh
with brick > 0 against the dense call, and neddf/scripts/extract_mesh.py --sparse."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from conftest import GOLDEN

import sparse_mesh_check as sm
import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bunny(dev):
    from neddf_amd import NeDDF
    from neddf_amd.fixtures import BUNNY_SMOKE_CFG, bunny_smoke_weights
    net = NeDDF(**BUNNY_SMOKE_CFG)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in bunny_smoke_weights().items()})
    net.to(dev)
    net.set_iter(-1)
    for p in net.parameters():
        p.requires_grad_(False)
    return net


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same_mesh(got, want, what):
    gv, gt = (t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in got[:2])
    wv, wt = (t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in want[:2])
    assert gv.dtype == np.float32 and gt.dtype == np.int32, what
    assert gt.shape == wt.shape and np.array_equal(gt, wt), (what, gt.shape, wt.shape)
    assert gv.shape == wv.shape and np.array_equal(_bits(gv), _bits(wv)), what     # bit for bit (NaN-safe)


# ------------------------------------------------------------------------------------------------------------- 1. selection
def _select_cases():
    rng = np.random.default_rng(17)
    out = []
    for shape in ((9, 7, 11), (2, 2, 2), (3, 10, 2)):
        c = rng.standard_normal(shape).astype(np.float32)
        c[rng.random(shape) < 0.1] = np.nan
        out.append(("random%dx%dx%d" % shape, c, 0.2))
    smooth = np.fromfunction(lambda z, y, x: 0.11 * x + 0.07 * y + 0.05 * z - 0.6, (8, 9, 10)).astype(np.float32)   # a slab of active bricks
    out.append(("plane", smooth, 0.0))
    out.append(("all_inactive", np.full((5, 4, 6), 2.0, np.float32), 0.0))
    edge = np.full((3, 3, 5), 2.0, np.float32)
    edge[0, 0, 0] = np.float32(0.3)                             # exactly iso + band (iso 0, band 0.3 in fp32): inside the band
    edge[2, 2, 4] = -np.float32(0.3)                            # exactly iso - band -- and below iso
    edge[1, 1, 2] = np.nextafter(np.float32(0.3), np.float32(9))        # one ulp outside the band
    out.append(("at_the_band", edge, 0.0))
    return out


@pytest.mark.parametrize("case", _select_cases(), ids=lambda c: c[0])
def test_selection_matches_the_checker(dev, case):
    from neddf_amd.mesh import select_bricks
    name, coarse, iso = case
    d = torch.from_numpy(coarse).to(dev)
    for band in (0.0, 0.3):
        for dilate in (0, 1, 2):
            slot, ids = select_bricks(d, iso, band, dilate)
            wslot, wids = sm.select(coarse, iso, band, dilate)
            assert slot.dtype == torch.int32 and ids.dtype == torch.int32
            assert np.array_equal(slot.cpu().numpy(), wslot), (name, band, dilate)
            assert np.array_equal(ids.cpu().numpy(), wids), (name, band, dilate)
    if name == "all_inactive":
        assert wids.size == 0
    if name == "at_the_band":
        assert sm.select(coarse, iso, 0.3)[1].tolist() == [0, 15] and sm.select(coarse, iso, 0.0)[1].tolist() == [15]


def test_selection_spans_several_workgroups(dev):
    """More bricks than one workgroup of the count / list kernels holds, an active count that is no multiple of the wave."""
    from neddf_amd.mesh import select_bricks
    rng = np.random.default_rng(2)
    coarse = rng.standard_normal((12, 13, 14)).astype(np.float32) + 1.5
    slot, ids = select_bricks(torch.from_numpy(coarse).to(dev), 0.0, 0.05)
    wslot, wids = sm.select(coarse, 0.0, 0.05)
    assert 256 < wids.size < wslot.size
    assert np.array_equal(slot.cpu().numpy(), wslot) and np.array_equal(ids.cpu().numpy(), wids)


# ------------------------------------------------------------------------------------------------------ 2. brick evaluation
@pytest.fixture(scope="module")
def bunny_box(dev, bunny):
    """The bunny's distance on a 37 x 31 x 23 lattice over an anisotropic box, by the dense grid call."""
    from neddf_amd import Context
    ctx = Context.get(dev)
    bunny.upload(ctx, bunny._slot)
    shape, lo, hi = (37, 31, 23), (-0.9, -1.0, -0.7), (1.0, 0.8, 0.9)
    return shape, lo, hi, ctx.field_grid(bunny._slot, "distance", shape, lo, hi).cpu().numpy()


@pytest.mark.parametrize("B", [4, 8])
def test_brick_evaluation_carries_the_grid_bits(dev, bunny, bunny_box, B):
    from neddf_amd import Context
    shape, lo, hi, dense = bunny_box
    ctx = Context.get(dev)
    bunny.upload(ctx, bunny._slot)
    nb = sm.brick_counts(shape, B)
    assert sum(1 for n in shape if (n - 1) % B) >= 2        # partial last bricks
    ids = np.arange(nb[0] * nb[1] * nb[2], dtype=np.int32)
    for pick in (ids, ids[::3], ids[-1:]):
        got = ctx.field_bricks(bunny._slot, "distance", shape, B, lo, hi, torch.from_numpy(pick).to(dev)).cpu().numpy()
        want = sm.brick_values(dense, pick, B)
        assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
        assert np.isnan(want).any() and np.array_equal(_bits(got), _bits(want))          # padding: the quiet NaN, everything else the grid's bits
    coarse = ctx.field_grid_coarse(bunny._slot, "distance", shape, B, lo, hi).cpu().numpy()
    assert np.array_equal(_bits(coarse), _bits(sm.coarse_volume(dense, B)))
    assert ctx.field_bricks(bunny._slot, "distance", shape, B, lo, hi, torch.empty(0, dtype=torch.int32, device=dev)).shape == (0, (B + 1) ** 3)


# ------------------------------------------------------------------------------- 3. all bricks active == dense marching cubes
def _volumes():
    rng = np.random.default_rng(5)

    def grid(shape, lo, hi):
        axes = [np.linspace(lo[a], hi[a], n) for a, n in enumerate(shape[::-1])]     # x, y, z
        z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
        return x, y, z

    out = []
    x, y, z = grid((40, 40, 40), (-1, -1, -1), (1, 1, 1))
    out.append(("sphere", np.sqrt(x * x + y * y + z * z) - 0.55, 0.0, (-1, -1, -1), (1, 1, 1)))
    lo, hi = (-0.9, -0.8, -1.3), (0.85, 0.9, 1.1)
    x, y, z = grid((23, 31, 37), lo, hi)                # nz, ny, nx all different; an anisotropic box
    out.append(("torus", np.sqrt((np.sqrt(x * x + y * y) - 0.45) ** 2 + z * z) - 0.2, 0.0, lo, hi))
    out.append(("two_spheres", np.minimum(np.sqrt((x - 0.35) ** 2 + y * y + z * z), np.sqrt((x + 0.4) ** 2 + y * y + z * z)) - 0.3,
                0.0, lo, hi))
    out.append(("random", rng.standard_normal((17, 9, 13)), 0.1, (0, 0, 0), (1, 2, 3)))
    out.append(("2x2x2", rng.standard_normal((2, 2, 2)), 0.0, (-1, -1, -1), (1, 1, 1)))
    out.append(("all_inside", -np.ones((5, 6, 7)), 0.0, (-1, -1, -1), (1, 1, 1)))
    out.append(("all_outside", np.ones((5, 6, 7)), 0.0, (-1, -1, -1), (1, 1, 1)))
    out.append(("equal_iso", rng.integers(-1, 2, (11, 12, 13)).astype(np.float64) * 0.5 + 0.25, 0.25, (-1, -1, -1), (1, 1, 1)))
    nan = rng.standard_normal((12, 10, 14))
    nan[rng.random(nan.shape) < 0.1] = np.nan
    out.append(("nan", nan, 0.0, (-2, -1, -1), (2, 1, 1)))
    return [(n, v.astype(np.float32), iso, lo, hi) for n, v, iso, lo, hi in out]


VOLUMES = {c[0]: c for c in _volumes()}


def _bricks_on_device(dev, vol, active, B):
    slot, ids = sm.slots_of(active)
    return (torch.from_numpy(sm.brick_values(vol, ids, B)).to(dev), torch.from_numpy(ids).to(dev), torch.from_numpy(slot).to(dev))


@pytest.fixture(scope="module")
def dense_meshes(dev):
    """neddf_marching_cubes' meshes of the volume families, computed once (checked against the checker in test_gpu_mesh.py)."""
    from neddf_amd.mesh import marching_cubes
    return {n: tuple(t.cpu().numpy() for t in marching_cubes(torch.from_numpy(v).to(dev), iso, lo, hi)) for n, v, iso, lo, hi in VOLUMES.values()}


@pytest.mark.parametrize("B", [2, 4, 8, 16])
@pytest.mark.parametrize("name", list(VOLUMES))
def test_all_bricks_equal_dense_marching_cubes(dev, dense_meshes, name, B):
    from neddf_amd.mesh import marching_cubes_bricks
    _, vol, iso, lo, hi = VOLUMES[name]
    shape = vol.shape[::-1]
    nb = sm.brick_counts(shape, B)
    vals, ids, slot = _bricks_on_device(dev, vol, np.ones(nb[::-1], bool), B)
    got = marching_cubes_bricks(vals, ids, slot, shape, B, iso, lo, hi)
    _same_mesh(got, dense_meshes[name], (name, B))
    if name in ("all_inside", "all_outside"):
        assert got[1].shape[0] == 0
    if name in ("sphere", "torus", "two_spheres", "random", "nan"):
        assert got[1].shape[0] > 0


# -------------------------------------------------------------------------------------------------------------- 4. subsets
def _subsets(nb):
    nbx, nby, nbz = nb
    rng = np.random.default_rng(23)

    def only(*bricks):
        a = np.zeros((nbz, nby, nbx), bool)
        for bx, by, bz in bricks:
            a[bz, by, bx] = True
        return a

    return [("half", rng.random((nbz, nby, nbx)) < 0.5),
            ("face", only((1, 0, 1), (2, 0, 1))),
            ("edge", only((0, 0, 0), (1, 1, 0))),
            ("edge_other_diagonal", only((0, 1, 0), (0, 0, 1))),           # the lower brick has the HIGHER y: ownership goes by index
            ("edge_other_diagonal_x", only((1, 0, 0), (0, 1, 0))),
            ("corner", only((0, 0, 0), (1, 1, 1))),
            ("corner_other_diagonal", only((1, 1, 0), (0, 0, 1))),
            ("last_partial", only((nbx - 1, nby - 1, nbz - 1), (nbx - 2, nby - 1, nbz - 1))),
            ("one", only((1, 1, 1)))]


@pytest.mark.parametrize("name,B", [("random", 4), ("random", 2), ("nan", 3), ("torus", 8)])
def test_subsets_of_bricks_match_the_restricted_mesh(dev, name, B):
    from neddf_amd.mesh import marching_cubes_bricks
    _, vol, iso, lo, hi = VOLUMES[name]
    shape = vol.shape[::-1]
    nb = sm.brick_counts(shape, B)
    assert min(nb) >= 2
    for what, active in _subsets(nb):
        vals, ids, slot = _bricks_on_device(dev, vol, active, B)
        want = sm.restricted_mesh(vol, iso, lo, hi, active, B)
        got = marching_cubes_bricks(vals, ids, slot, shape, B, iso, lo, hi)
        _same_mesh(got, want, (name, B, what))
        if name == "random":
            assert len(want[1]) > 0, what
        # the library's own order and its keys
        v, t, vk, tk = marching_cubes_bricks(vals, ids, slot, shape, B, iso, lo, hi, dense_order=False)
        assert vk.dtype == torch.int64 and tk.dtype == torch.int64 and vk.shape[0] == v.shape[0] and tk.shape[0] == t.shape[0]
        vk, tk = vk.cpu().numpy(), tk.cpu().numpy()
        vo, to = np.argsort(vk, kind="stable"), np.argsort(tk, kind="stable")
        assert (np.diff(vk[vo]) > 0).all() and (np.diff(tk[to]) > 0).all(), what             # unique: each vertex and triangle once
        inv = np.empty(len(vo), np.int32)
        inv[vo] = np.arange(len(vo), dtype=np.int32)
        _same_mesh((v.cpu().numpy()[vo], inv[t.cpu().numpy()][to].reshape(-1, 3)), got, (name, B, what, "keys"))
        assert ((vk % 3) >= 0).all() and (tk % 5 < 5).all() and (vk // 3 < vol.size).all() and (tk // 5 < vol.size).all()


def test_selected_bricks_at_band_zero(dev):
    """select_bricks at band 0 and dilate 0 on the torus: sign changes and nothing else -- some crossed cells are missed, and the result
    is still exactly the dense mesh restricted to the selected bricks."""
    from neddf_amd.mesh import marching_cubes_bricks, select_bricks
    _, vol, iso, lo, hi = VOLUMES["torus"]
    shape, B = vol.shape[::-1], 4
    slot, ids = select_bricks(torch.from_numpy(sm.coarse_volume(vol, B)).to(dev), iso, 0.0, 0)
    active = slot.cpu().numpy() >= 0
    assert 0 < active.sum() < active.size
    vals = torch.from_numpy(sm.brick_values(vol, ids.cpu().numpy(), B)).to(dev)
    want = sm.restricted_mesh(vol, iso, lo, hi, active, B)
    assert len(want[1])
    _same_mesh(marching_cubes_bricks(vals, ids, slot, shape, B, iso, lo, hi), want, "band 0")


def test_two_call_protocol_and_errors(dev):
    from neddf_amd import Context, NeddfError
    from neddf_amd.mesh import marching_cubes_bricks, select_bricks
    ctx = Context.get(dev)
    _, vol, iso, lo, hi = VOLUMES["random"]
    nz, ny, nx = vol.shape
    B = 4
    nb = sm.brick_counts((nx, ny, nz), B)
    active = np.random.default_rng(1).random(nb[::-1]) < 0.6
    vals, ids, slot = _bricks_on_device(dev, vol, active, B)
    wv, wt = marching_cubes_bricks(vals, ids, slot, (nx, ny, nz), B, iso, lo, hi, dense_order=False)[:2]
    wv, wt = wv.cpu().numpy(), wt.cpu().numpy()
    assert len(wv) > 10 and len(wt) > 10
    blo, bhi = (C.c_double * 3)(*lo), (C.c_double * 3)(*hi)
    nv, nt = C.c_int64(-1), C.c_int64(-1)
    s = ctx.stream()
    p = lambda t: C.c_void_p(t.data_ptr())              # noqa: E731
    fn = ctx.lib.neddf_marching_cubes_bricks

    def call(v=None, cap_v=0, t=None, cap_t=0, vk=None, tk=None, ids_=ids, slot_=slot, dims=(nx, ny, nz), brick=B, lo_=blo, m=None):
        nv.value = nt.value = -1
        return fn(ctx.h, p(vals), p(ids_), ids_.shape[0] if m is None else m, p(slot_), dims[0], dims[1], dims[2], brick, lo_, bhi, iso,
                  None if v is None else p(v), cap_v, None if t is None else p(t), cap_t, None if vk is None else p(vk),
                  None if tk is None else p(tk), C.byref(nv), C.byref(nt), s)

    assert call() == 0 and (nv.value, nt.value) == (len(wv), len(wt))
    v = torch.full((len(wv), 3), -7.0, device=dev)
    t = torch.full((len(wt), 3), -7, device=dev, dtype=torch.int32)
    vk = torch.full((len(wv),), -7, device=dev, dtype=torch.int64)
    tk = torch.full((len(wt),), -7, device=dev, dtype=torch.int64)
    for cap_v, cap_t in ((len(wv) - 1, len(wt)), (len(wv), len(wt) - 1)):         # a cap below its count: counts only
        assert call(v, cap_v, t, cap_t, vk, tk) == 0 and (nv.value, nt.value) == (len(wv), len(wt))
        torch.cuda.synchronize()
        assert (v == -7).all() and (t == -7).all() and (vk == -7).all() and (tk == -7).all()
    assert call(v, len(wv), t, len(wt), vk, tk) == 0
    _same_mesh((v, t), (wv, wt), "exact-size write")
    assert (vk >= 0).all() and (tk >= 0).all()
    # NEDDF_EINVAL: the brick size, a dimension below 2, lo >= hi, an index outside the grid, a list that is not strictly ascending
    for brick in (1, 17, 0, -4):
        assert call(brick=brick) == -1, brick
    assert call(dims=(1, ny, nz)) == -1 and call(dims=(nx, ny, 0)) == -1
    assert call(lo_=(C.c_double * 3)(lo[0], hi[1], lo[2])) == -1
    assert call(m=nb[0] * nb[1] * nb[2] + 1) == -1 and call(m=-1) == -1
    total = nb[0] * nb[1] * nb[2]
    two = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    ok_slot = torch.full((total,), -1, dtype=torch.int32, device=dev)
    ok_slot[:2] = two
    assert call(ids_=two, slot_=ok_slot) == 0                                   # (values: the first two rows of vals, whatever they hold)
    outside = torch.tensor([0, total], dtype=torch.int32, device=dev)
    assert call(ids_=outside, slot_=ok_slot) == -1
    negative = torch.tensor([-1, 1], dtype=torch.int32, device=dev)
    assert call(ids_=negative, slot_=ok_slot) == -1
    swapped = torch.tensor([1, 0], dtype=torch.int32, device=dev)
    inv_slot = ok_slot.clone()
    inv_slot[0], inv_slot[1] = 1, 0
    assert call(ids_=swapped, slot_=inv_slot) == -1                             # its own inverse, but descending
    twice = torch.tensor([1, 1], dtype=torch.int32, device=dev)
    assert call(ids_=twice, slot_=ok_slot) == -1
    stale = ok_slot.clone()
    stale[5] = 1                                                                # a slot map that names a brick the list does not hold
    assert call(ids_=two, slot_=stale) == -1
    assert b"ascending" in ctx.lib.neddf_last_error(ctx.h)
    assert call() == 0 and (nv.value, nt.value) == (len(wv), len(wt))           # and the context still works
    # no bricks at all: an empty mesh
    none = torch.empty(0, dtype=torch.int32, device=dev)
    ev, et = marching_cubes_bricks(torch.empty(0, (B + 1) ** 3, device=dev), none, torch.full(nb[::-1], -1, dtype=torch.int32, device=dev),
                                   (nx, ny, nz), B, iso, lo, hi)
    assert ev.shape == (0, 3) and et.shape == (0, 3)
    # the Python layer's own checks
    with pytest.raises(NeddfError, match="float32"):
        marching_cubes_bricks(vals.double(), ids, slot, (nx, ny, nz), B, iso, lo, hi)
    with pytest.raises(NeddfError, match="slot_map"):
        marching_cubes_bricks(vals, ids, slot[:1], (nx, ny, nz), B, iso, lo, hi)
    with pytest.raises(NeddfError, match="brick size"):
        marching_cubes_bricks(vals[:, :8], ids, slot, (nx, ny, nz), 1, iso, lo, hi)
    coarse = torch.zeros(3, 3, 3, device=dev)
    with pytest.raises(NeddfError, match="band"):
        select_bricks(coarse, 0.0, -1.0)
    with pytest.raises(NeddfError, match="dilate"):
        select_bricks(coarse, 0.0, 0.0, 5)
    with pytest.raises(NeddfError, match="float32"):
        select_bricks(coarse.double(), 0.0, 0.0)
    assert ctx.lib.neddf_brick_select(ctx.h, p(coarse), 2, 2, 2, 0.0, float("nan"), 0, p(slot), p(ids), C.byref(nv), s) == -1
    assert ctx.lib.neddf_field_bricks(ctx.h, 0, 0, nx, ny, nz, 17, blo, bhi, p(ids), ids.shape[0], p(vals), s) == -1
    assert ctx.lib.neddf_field_grid_coarse(ctx.h, 0, 0, nx, ny, nz, 1, blo, bhi, p(vals), s) == -1


# ----------------------------------------------------------------------------------------------------------- 5. end to end
@pytest.fixture(scope="module")
def bunny_dense_61(bunny):
    return tuple(t.cpu().numpy() for t in bunny.extract_mesh(resolution=61, threshold=0.1))


def test_extract_mesh_sparse_equals_dense(bunny, bunny_dense_61):
    times = {}
    got = bunny.extract_mesh(resolution=61, threshold=0.1, brick=4, timings=times)
    assert len(bunny_dense_61[1]) > 1000
    _same_mesh(got, bunny_dense_61, "bunny 61^3, brick 4")
    print("bunny 61^3, brick 4: %d of %d bricks active, %d vertices, %d triangles" % (times["bricks_active"], times["bricks"], len(got[0]), len(got[1])))
    assert times["bricks"] == 15 ** 3 and 0 < times["bricks_active"] < times["bricks"]
    assert all(times[k] >= 0 for k in ("coarse", "grid", "mcubes"))
    # brick = 0 is the dense path, the same from call to call, and reports no brick counts
    times0 = {}
    _same_mesh(bunny.extract_mesh(resolution=61, threshold=0.1, brick=0, timings=times0), bunny_dense_61, "brick 0")
    assert "bricks" not in times0 and "coarse" not in times0 and set(times0) == {"grid", "mcubes"}
    with pytest.raises(ValueError, match="brick"):
        bunny.extract_mesh(resolution=61, threshold=0.1, brick=1)
    with pytest.raises(ValueError, match="brick"):
        bunny.extract_mesh(resolution=61, threshold=0.1, brick=17)


def test_extract_mesh_sparse_with_normals_colours_and_clean_up(bunny):
    kw = dict(resolution=61, threshold=0.1, normals=True, colors=True, min_component_triangles=16, keep_largest=1)
    dense = bunny.extract_mesh(**kw)
    times = {}
    sparse = bunny.extract_mesh(brick=4, timings=times, **kw)
    assert len(dense) == len(sparse) == 4 and len(dense[1]) > 1000
    _same_mesh(sparse, dense, "positions and triangles")
    for a, b, what in zip(sparse[2:], dense[2:], ("normals", "colours")):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy())), what
    assert 0 < times["bricks_active"] < times["bricks"] and "clean" in times and "normals" in times and "colors" in times


def test_extract_mesh_sparse_partial_last_brick(bunny):
    """resolution 64: 63 cells per axis, 8 bricks of 8 with a last one of 7."""
    dense = bunny.extract_mesh(resolution=64, threshold=0.1)
    times = {}
    sparse = bunny.extract_mesh(resolution=64, threshold=0.1, brick=8, timings=times)
    assert len(dense[1]) > 1000 and times["bricks"] == 8 ** 3 and 0 < times["bricks_active"] < times["bricks"]
    _same_mesh(sparse, dense, "bunny 64^3, brick 8")


def test_extract_mesh_sparse_sdf_and_density(dev, bunny):
    from neddf_amd import Context, NeuS
    neus = NeuS().to(dev)
    neus.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.neus_state().items()})
    neus.set_iter(-1)
    for p in neus.parameters():
        p.requires_grad_(False)
    times = {}
    _same_mesh(neus.extract_mesh("sdf", 0.0, 1.1, 48, brick=4, timings=times), neus.extract_mesh("sdf", 0.0, 1.1, 48), "NeuS sdf at 0")
    assert 0 <= times["bricks_active"] <= times["bricks"] == 12 ** 3
    # a level the synthetic sdf does reach, every brick kept by a band wider than the field's range: the whole route on "sdf"
    ctx = Context.get(dev)
    neus.upload(ctx, neus._slot)
    vol = ctx.field_grid(neus._slot, "distance", (48,) * 3, (-1.1,) * 3, (1.1,) * 3)
    mid = 0.5 * (float(vol.min()) + float(vol.max()))           # (a ReLU sdf trunk: sdf >= 0, the level 0 itself holds no surface)
    dense = neus.extract_mesh("sdf", mid, 1.1, 48)
    assert len(dense[1]) > 0
    _same_mesh(neus.extract_mesh("sdf", mid, 1.1, 48, brick=5, band=1e30, timings=times), dense, "NeuS sdf, every brick")
    assert times["bricks_active"] == times["bricks"] == 10 ** 3
    # a density has no Lipschitz bound: band=None is refused, an explicit band runs (and the winding flip still applies)
    bunny.upload(ctx, bunny._slot)
    thr = 0.25 * float(ctx.field_grid(bunny._slot, "density", (40,) * 3, (-1.1,) * 3, (1.1,) * 3).max())
    assert np.isfinite(thr) and thr > 0
    with pytest.raises(ValueError, match="band"):
        bunny.extract_mesh("density", thr, resolution=40, brick=4)
    dense = bunny.extract_mesh("density", thr, resolution=40)
    assert len(dense[1]) > 0
    _same_mesh(bunny.extract_mesh("density", thr, resolution=40, brick=4, band=1e30), dense, "density, every brick")
    v, t = bunny.extract_mesh("density", thr, resolution=40, brick=4, band=0.5 * thr, brick_dilate=1, timings=times)
    assert v.shape[1] == 3 and t.shape[1] == 3 and len(t) <= len(dense[1]) and 0 < times["bricks_active"] <= times["bricks"]


# ------------------------------------------------------------------------------------------------------------ 6. the script
def test_extract_mesh_script_sparse(dev, bunny, tmp_path, capsys):
    import yaml
    from neddf_amd.fixtures import BUNNY_SMOKE_CFG, bunny_smoke_weights
    from neddf_amd.scripts.extract_mesh import main
    run = tmp_path / "run"
    (run / ".hydra").mkdir(parents=True)
    (run / "models").mkdir()
    cfg = {"dataset": {"_target_": "neddf.dataset.NeRFSyntheticDataset", "dataset_dir": os.path.join(GOLDEN, "bunny_mini"),
                       "data_split": "train", "use_depth": False, "use_mask": True},
           "render": {"_target_": "neddf.render.NeRFRender", "sample_coarse": 64, "sample_fine": 128, "dist_near": 2.0,
                      "dist_far": 6.0, "max_dist": 6.0, "use_coarse_network": False, "sampling_type": "cone"},
           "network": dict(BUNNY_SMOKE_CFG, _target_="neddf.network.NeDDF"),
           "trainer": {"_target_": "neddf.trainer.NeRFTrainer", "device": "cuda:0", "batch_size": 128, "chunk": 1024},
           "loss": {"functions": [{"_target_": "neddf.loss.ColorLoss", "weight": 1.0}]}}
    yaml.safe_dump(cfg, open(run / ".hydra" / "config.yaml", "w"))
    sd = {p + k: torch.from_numpy(v) for k, v in bunny_smoke_weights().items() for p in ("network_fine.", "network_coarse.")}
    torch.save(sd, run / "models" / "model_00007.pth")
    common = [str(run), "--epoch", "7", "--resolution", "49", "--threshold", "0.1", "--normals", "--colors", "--keep-largest"]
    path = main(common)
    plain = path.read_bytes()
    capsys.readouterr()
    for extra, B in ((["--sparse"], 8), (["--sparse", "4", "--lipschitz", "1.5", "--brick-dilate", "1"], 4)):
        path.unlink()
        assert main(common + extra) == path
        out = capsys.readouterr().out
        assert path.read_bytes() == plain, extra
        line = [ln for ln in out.splitlines() if ln.startswith("bricks: ")]
        assert len(line) == 1 and " active of %d" % ((48 // B) ** 3) in line[0], out
        active = int(line[0].split()[1])
        assert 0 < active < (48 // B) ** 3
    assert len(plain) > 10000
