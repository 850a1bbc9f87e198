"""Mesh simplification on the GPU: mesh.simplify_mesh (the neddf_mesh_simplify_* entry points and neddf_mesh_compact) against the host
restatement (tests/simplify_check.py) bit for bit, for every output array and both placements -- empty inputs, one triangle, a full
collapse, a sphere on three grids, strips whose vertex counts end at the edges of a workgroup, a soup with invalid indices,
non-finite vertices, duplicates and a folded sheet, a mesh where rounding dominates the cell function, attributes -- then the
properties: the same bits on every run, the identity, the one-way displacement bound by the exact point-to-mesh distance,
extract_mesh's simplify_cell on the shipped bunny, and neddf/scripts/extract_mesh.py end to end."""
import math
import os

import numpy as np
import pytest
import torch
from conftest import GOLDEN

import mesh_check as mc
import simplify_check as sc

pytestmark = pytest.mark.gpu

PLACEMENTS = ("mean", "quadric")


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


def N(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _device(dev, v, t, **kw):
    from neddf_amd.mesh import simplify_mesh
    if kw.get("attributes") is not None:
        a = kw["attributes"]
        kw["attributes"] = torch.from_numpy(a).to(dev) if isinstance(a, np.ndarray) else [torch.from_numpy(x).to(dev) for x in a]
    return simplify_mesh(torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev), **kw)


def _same(got, want, what):
    assert len(got) == len(want), what
    for g, w, part in zip(got, want, ("vertices", "triangles", "vertex_map", "triangle_map", "attributes")):
        gs, ws = (g, w) if isinstance(w, list) else ([g], [w])
        assert len(gs) == len(ws), (what, part)
        for g1, w1 in zip(gs, ws):
            g1 = N(g1)
            assert g1.dtype == w1.dtype and g1.shape == w1.shape, (what, part, g1.dtype, w1.dtype, g1.shape, w1.shape)
            same = np.array_equal(_bits(g1), _bits(w1)) if g1.dtype == np.float32 else np.array_equal(g1, w1)
            assert same, (what, part)


def _check(dev, v, t, what, **kw):
    """Both placements of one case against the restatement; returns the restatement's outputs of the last one."""
    want = None
    for placement in PLACEMENTS:
        want = sc.simplify(v, t, placement=placement, **kw)
        _same(_device(dev, v, t, placement=placement, **kw), want, (what, placement))
    return want


def _strip(V, seed=None):
    v = np.random.default_rng(V if seed is None else seed).random((V, 3)).astype(np.float32)
    t = (np.arange(V - 2, dtype=np.int32)[:, None] + np.arange(3, dtype=np.int32)[None, :]).astype(np.int32)
    return v, t


def _soup():
    """Random triangles over random vertices with: indices V and -1, NaN / Inf vertices (one NaN with a payload), a duplicated
    triangle in the same and in a rotated corner order, and a folded sheet -- two layers 1e-3 apart with opposite orientations,
    which fall into the same cells and collapse onto the same triples in opposite orientation."""
    v, t = sc.triangle_soup(600, 1500, seed=7)
    t[9] = (-1, 2, 3)
    t[21] = t[20]
    t[22] = t[20][[1, 2, 0]]
    t[23] = t[20][[0, 2, 1]]
    v[50, 1] = np.nan
    v[51, 0] = np.inf
    v[52, 2] = -np.inf
    _bits(v)[53, 0] = 0x7fc01234
    n = 9
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 2).astype(np.float32) / (n - 1)
    top = np.concatenate([g, np.full((n * n, 1), 0.5, np.float32)], axis=1)
    bottom = top + np.array([0, 0, 1e-3], np.float32)
    quads = [(i * n + j, (i + 1) * n + j, (i + 1) * n + j + 1, i * n + j + 1) for i in range(n - 1) for j in range(n - 1)]
    sheet = np.array([x for q in quads for x in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.int32)
    base = len(v)
    v = np.concatenate([v, top, bottom]).astype(np.float32)
    t = np.concatenate([t, sheet + base, (sheet + base + n * n)[:, [0, 2, 1]]]).astype(np.int32)
    t[5] = (0, 1, len(v))
    return v, t


def test_empty_inputs_one_triangle_and_a_full_collapse(dev):
    v, t = sc.uv_sphere(8, 10)
    for what, vv, tt, cells in (("V = 0", v[:0], t[:0], (2, 2, 2)), ("V = 0 with triangles", v[:0], t, (2, 2, 2)), ("T = 0", v, t[:0], (3, 3, 3)),
                                ("one triangle", v[:3], np.array([[0, 1, 2]], np.int32), (4, 4, 4)),
                                ("one triangle, one cell", v[:3], np.array([[0, 1, 2]], np.int32), (1, 1, 1)),
                                ("all vertices in one cell", v, t, (1, 1, 1))):
        want = _check(dev, vv, tt, what, cells=cells)
        if what in ("all vertices in one cell", "T = 0", "V = 0", "one triangle, one cell"):
            assert want[0].shape == (0, 3) and want[1].shape == (0, 3)
    attr = np.ones((len(v), 2), np.float32)
    _check(dev, v, t, "a full collapse with attributes", cells=(1, 1, 1), attributes=attr)
    _check(dev, v[:0], t[:0], "V = 0 with attributes", cells=(1, 1, 1), attributes=attr[:0])


@pytest.mark.parametrize("cells", [(1, 1, 1), (4, 4, 4), (37, 5, 1024)])
def test_sphere_matches_the_restatement(dev, cells):
    v, t = sc.uv_sphere(12, 16)                          # 178 vertices, 352 triangles
    want = _check(dev, v, t, ("sphere", cells), cells=cells)
    if cells == (4, 4, 4):
        assert 0 < len(want[1]) < len(t) and 0 < len(want[0]) < len(v)
    _check(dev, v, t, ("sphere, cell = 0.45", cells), cell=0.45)
    _check(dev, v, t, ("sphere, a box of its own", cells), cells=cells, box=([-0.5, -0.25, -2.0], [0.5, 1.5, 2.0]), regularisation=0.0)


@pytest.mark.parametrize("V", [255, 256, 257, 511, 512, 513, 4099])
def test_strips_across_the_edges_of_a_workgroup(dev, V):
    """Vertex (and key) counts of one scan block, one more and one less, two blocks likewise, and a few thousand: the kernels that
    place by rank (run heads, cluster ids, pairs) at block edges.  5^3 cells hold several members each; 64^3 mostly one."""
    v, t = _strip(V)
    for cells in ((5, 5, 5), (64, 64, 64)):
        want = _check(dev, v, t, ("strip", V, cells), cells=cells)
        assert len(want[0]) and len(want[1])


def test_soup_with_everything_wrong(dev):
    v, t = _soup()
    for cells in ((6, 6, 1), (10, 10, 10), (3, 4, 5)):
        want = _check(dev, v, t, ("soup", cells), cells=cells)
        ov, ot, vm, tm = want
        assert tm[5] == -1 and tm[9] == -1                              # out-of-range indices
        assert tm[21] == -1 and tm[22] == -1                            # duplicates of triangle 20, a rotated one included
        assert (tm[20] >= 0) == (tm[23] >= 0)                           # the opposite orientation is another triangle
        for i in (50, 51, 52, 53):                                      # non-finite vertices are clusters of their own, bit for bit
            if vm[i] >= 0:
                assert np.array_equal(_bits(ov)[vm[i]], _bits(v)[i])
    ov, ot, vm, tm = sc.simplify(v, t, cells=(6, 6, 1))
    n = 9
    top = np.arange(len(v) - 2 * n * n, len(v) - n * n)
    assert np.array_equal(vm[top], vm[top + n * n])                     # the sheet's two layers share their clusters ...
    first = len(t) - 4 * (n - 1) ** 2
    up, down = tm[first:first + 2 * (n - 1) ** 2], tm[first + 2 * (n - 1) ** 2:]
    both = (up >= 0) & (down >= 0)
    assert both.any()                                                   # ... and both orientations of a surviving triple stay
    a, b = ot[up[both]], ot[down[both]]
    assert np.array_equal(a, b[:, [0, 2, 1]])


def test_offset_mesh_where_rounding_dominates(dev):
    """A sphere of radius 2^-9 (size 2^-8) around (1000, 1000, 1000): a coordinate has 2^-14 of resolution there, 64 steps across."""
    v, t = sc.uv_sphere(16, 20, radius=2.0 ** -9, centre=(1000.0, 1000.0, 1000.0))
    for cells in ((4, 4, 4), (37, 5, 1024)):
        want = _check(dev, v, t, ("offset", cells), cells=cells)
        assert len(want[0])


@pytest.mark.parametrize("k", [1, 3, 6])
def test_attributes(dev, k):
    v, t = sc.uv_sphere(12, 16)
    rng = np.random.default_rng(k)
    attr = rng.standard_normal((len(v), k)).astype(np.float32)
    attr[7, 0], attr[8, 0], attr[30, k - 1] = np.inf, -np.inf, np.nan
    want = _check(dev, v, t, ("attributes", k), cells=(4, 4, 4), attributes=attr)
    assert want[4].shape == (len(want[0]), k)
    two = [attr, rng.random((len(v), 3)).astype(np.float32)]
    _check(dev, v, t, ("a list of attributes", k), cells=(5, 3, 4), attributes=two)


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_results_do_not_depend_on_the_run(dev, placement):
    v, t = _soup()
    attr = np.random.default_rng(0).random((len(v), 3)).astype(np.float32)
    a = _device(dev, v, t, cells=(7, 7, 7), placement=placement, attributes=attr)
    b = _device(dev, v, t, cells=(7, 7, 7), placement=placement, attributes=attr)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and torch.equal(x.view(torch.int32), y.view(torch.int32))


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_identity_when_no_two_vertices_share_a_cell(dev, placement):
    v, t = sc.uv_sphere(12, 16)
    lo, hi = sc.default_box(v)
    cells = (1024, 1024, 1024)
    assert len(np.unique(sc.keys(v, lo, hi, cells) >> 32)) == len(v)              # the premise
    attr = np.random.default_rng(0).standard_normal((len(v), 3)).astype(np.float32)
    ov, ot, vm, tm, oa = _device(dev, v, t, cells=cells, placement=placement, attributes=attr)
    assert np.array_equal(_bits(N(ov)), _bits(v)) and np.array_equal(N(ot), t) and np.array_equal(_bits(N(oa)), _bits(attr))
    assert np.array_equal(N(vm), np.arange(len(v))) and np.array_equal(N(tm), np.arange(len(t)))


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_one_way_bound_by_the_exact_distance(dev, placement):
    """Surface samples of the OUTPUT lie within (1 + 2^-10) cell diagonals of the INPUT surface, plus the point-to-mesh kernel's own
    absolute error 2^-20 W, W the largest |coordinate| (include/neddf_hip.h)."""
    from neddf_amd.geometry import point_mesh_distance
    from neddf_amd.mesh import sample_surface, simplify_mesh
    for name, (v, t) in (("sphere", sc.uv_sphere(24, 32)), ("offset", sc.uv_sphere(24, 32, radius=0.25, centre=(3.0, -2.0, 1.0)))):
        vd, td = torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev)
        lo, hi = sc.default_box(v)
        for cells in ((4, 4, 4), (9, 7, 5)):
            ov, ot, vm, tm = simplify_mesh(vd, td, cells=cells, placement=placement)
            assert 0 < len(ot) < len(t)
            pts, _ = sample_surface(ov, ot, n=4000, seed=1)
            pts = torch.cat([pts, ov])
            d = point_mesh_distance(pts, vd, td, method="bvh")["distance"]
            bound = (1.0 + 2.0 ** -10) * math.sqrt(sum(((h - l) / c) ** 2 for l, h, c in zip(lo, hi, cells)))
            W = max(float(np.abs(v).max()), float(pts.abs().max().item()))
            far = float(d.max().item())
            print("%s %s %s: %d -> %d triangles, max distance of the output to the input surface %.4e, bound %.4e"
                  % (name, placement, cells, len(t), len(ot), far, bound))
            assert far <= bound + 2.0 ** -20 * W, (name, cells, far, bound)


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_bunny_extract_mesh_simplified(bunny, placement):
    """extract_mesh(simplify_cell=...) = simplify_mesh applied to the plain call's mesh = the restatement, bit for bit; normals and
    colours belong to the simplified vertices; simplify_cell = 0 is the plain call."""
    from neddf_amd.mesh import simplify_mesh
    res, iso = 32, 0.1
    cell = 2.0 * 2.0 * 1.1 / (res - 1)
    pv, pt = bunny.extract_mesh(threshold=iso, resolution=res)
    times = {}
    v, t = bunny.extract_mesh(threshold=iso, resolution=res, simplify_cell=cell, simplify_placement=placement, timings=times)
    sv, st, vm, tm = simplify_mesh(pv, pt, cell=cell, placement=placement)
    assert torch.equal(v.view(torch.int32), sv.view(torch.int32)) and torch.equal(t, st)
    _same((sv, st, vm, tm), sc.simplify(N(pv), N(pt), cell=cell, placement=placement), ("bunny", placement))
    assert 0 < len(t) < len(pt) and 0 < len(v) < len(pv)
    assert (times["vertices_before"], times["triangles_before"]) == (len(pv), len(pt)) and times["simplify"] > 0.0
    print("bunny resolution %d, cells of 2 steps, %s: %d -> %d vertices, %d -> %d triangles, %.3f ms"
          % (res, placement, len(pv), len(v), len(pt), len(t), times["simplify"] * 1e3))
    v1, t1, n1, c1 = bunny.extract_mesh(threshold=iso, resolution=res, normals=True, colors=True, keep_largest=1, simplify_cell=cell,
                                        simplify_placement=placement)
    kv, kt = bunny.extract_mesh(threshold=iso, resolution=res, keep_largest=1)
    wv, wt = simplify_mesh(kv, kt, cell=cell, placement=placement)[:2]                # after the clean-up ...
    assert torch.equal(v1.view(torch.int32), wv.view(torch.int32)) and torch.equal(t1, wt)
    assert n1.shape == v1.shape and c1.shape == v1.shape                              # ... and before normals and colours
    assert torch.isfinite(n1).all() and torch.isfinite(c1).all()
    times = {}
    z = bunny.extract_mesh(threshold=iso, resolution=res, normals=True, colors=True, simplify_cell=0.0, timings=times)
    plain = bunny.extract_mesh(threshold=iso, resolution=res, normals=True, colors=True)
    assert "simplify" not in times and "vertices_before" not in times
    for a, b in zip(z, plain):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))
    with pytest.raises(ValueError):
        bunny.extract_mesh(threshold=iso, resolution=res, simplify_cell=cell, simplify_placement="median")


def test_errors(dev):
    from neddf_amd import NeddfError
    from neddf_amd.mesh import simplify_mesh
    v, t = (torch.from_numpy(a).to(dev) for a in sc.uv_sphere(6, 8))
    for kw in (dict(), dict(cell=0.5, cells=(2, 2, 2)), dict(cell=1e-4), dict(cells=(2, 2, 1025)), dict(cells=(0, 2, 2)),
               dict(cells=(2, 2, 2), placement="median"), dict(cells=(2, 2, 2), regularisation=-1.0),
               dict(cells=(2, 2, 2), attributes=torch.zeros(3, 2, device=dev)), dict(cells=(2, 2, 2), box=([0, 0, 0], [1, 1, float("inf")]))):
        with pytest.raises(NeddfError):
            simplify_mesh(v, t, **kw)
    with pytest.raises(NeddfError):
        simplify_mesh(v.cpu(), t, cells=(2, 2, 2))
    with pytest.raises(NeddfError):
        simplify_mesh(v, t.cpu(), cells=(2, 2, 2))


def test_extract_mesh_script_simplify(dev, bunny, tmp_path, capsys):
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
    sd = {p + k: torch.from_numpy(a) for k, a in bunny_smoke_weights().items() for p in ("network_fine.", "network_coarse.")}
    torch.save(sd, run / "models" / "model_00007.pth")
    path = main([str(run), "--epoch", "7", "--resolution", "24", "--threshold", "0.1", "--keep-largest", "--simplify"])
    out = capsys.readouterr().out
    assert path == (run / "mesh" / "mesh_24_threshold0.1.ply").resolve() and path.is_file()
    cell = 2.0 * 2.0 * 1.1 / 23
    v, t = bunny.extract_mesh(threshold=0.1, resolution=24, keep_largest=1, simplify_cell=cell)
    kv, kt = bunny.extract_mesh(threshold=0.1, resolution=24, keep_largest=1)
    line = [ln for ln in out.splitlines() if ln.startswith("simplified (mean, cells of 2 lattice steps): ")]
    assert len(line) == 1 and "%d -> %d vertices, %d -> %d triangles" % (len(kv), len(v), len(kt), len(t)) in line[0]
    assert "simplified -> unsimplified" not in out
    pv, pt = mc.read_ply(path)
    assert np.array_equal(pv, N(v)) and np.array_equal(pt, N(t)) and 0 < len(pt) < len(kt)
    path = main([str(run), "--epoch", "7", "--resolution", "24", "--threshold", "0.1", "--simplify", "3", "--simplify-placement", "quadric",
                 "--check-distance"])
    out = capsys.readouterr().out
    v, t = bunny.extract_mesh(threshold=0.1, resolution=24, simplify_cell=1.5 * cell, simplify_placement="quadric")
    pv, pt = mc.read_ply(path)
    assert np.array_equal(pv, N(v)) and np.array_equal(pt, N(t))
    assert len([ln for ln in out.splitlines() if ln.startswith("simplified (quadric, cells of 3 lattice steps): ")]) == 1
    line = [ln for ln in out.splitlines() if ln.startswith("simplified -> unsimplified surface: max ")]
    assert len(line) == 1
    far = float(line[0].split("max ")[1].split(",")[0])
    assert 0.0 < far <= (1.0 + 2.0 ** -10) * math.sqrt(3.0) * 1.5 * cell + 2.0 ** -20 * 1.1          # the header's bound, in the script's own figure
    assert out.strip().splitlines()[-1].startswith("{")                 # --check-distance's JSON line still comes last
    # without --simplify the script's output is what it was
    main([str(run), "--epoch", "7", "--resolution", "24", "--threshold", "0.1"])
    assert "simplified" not in capsys.readouterr().out
