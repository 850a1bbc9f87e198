"""Point-to-mesh distance on the GPU: the brute kernel against the numpy restatement (tests/pointmesh_check.py) bit for bit, the grid
query against the brute kernel bit for bit on boxes, cell counts, queries and meshes chosen to break it, and the Python layer end to
end: mesh_distance(to="surface") on two spheres with proven bounds, level_set_check on a field that is a distance and on one that is
not, the shipped bunny network, and the script."""
import json
import os

import numpy as np
import pytest
import torch
from conftest import GOLDEN

import geometry_check as gc
import pointmesh_check as pm
import raycast_check as rc
from test_geometry_host import SPHERE_DENSITY, SPHERE_SEED, spheres
from test_pointmesh_host import BOXES, OVERSHOOT_GATE, SPHERE_PAD

pytestmark = pytest.mark.gpu

F = np.float32
KEYS = ("d2", "triangle", "b1", "b2")


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


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def raw(ctx_result):
    """The library's own outputs (d2, triangle int32, b1, b2) as numpy."""
    return tuple(N(x) for x in ctx_result)


def same_bits(got, want, what):
    for k, g, w in zip(KEYS, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.flatnonzero(bits(g) != bits(w))
        assert bad.size == 0, (what, k, bad.size, bad[:5], g[bad[:5]], w[bad[:5]])


# ---------------------------------------------------------------------------------------------------------------- brute == restatement
def _soup_mesh(n_tri):
    """The soup with -- where it is large enough -- an exactly degenerate point triangle and segment triangle, a sliver, an index outside
    [0, V), a NaN vertex, and an exact duplicate of triangle 3 at the highest index."""
    v, t = rc.soup(n_tri, 11)
    if n_tri > 16:
        v = np.concatenate([v, [[np.nan, 0.1, 0.2]]]).astype(F)
        t = t.copy()
        t[1] = [t[1, 0], t[1, 0], t[1, 0]]                       # a point
        t[2] = [t[2, 0], t[2, 1], t[2, 1]]                       # a segment, c = b
        t[4] = [t[4, 0], t[4, 0], t[4, 1]]                       # a segment, b = a
        v[t[7, 2]] = (0.5 * (v[t[7, 0]].astype(np.float64) + v[t[7, 1]]) + [0.0, 2e-6, 0.0]).astype(F)          # a sliver
        t[5] = [t[5, 0], len(v) - 1, t[5, 1]]                    # the NaN vertex
        t[6] = [-1, t[6, 1], t[6, 2]]
        t[8] = [t[8, 0], len(v), t[8, 1]]
        t[n_tri - 1] = t[3]
    return v, t


def _query_pool(v, t):
    """Non-finite queries first, then mesh vertices, surface samples, uniform points and points at 100."""
    rng = np.random.default_rng(21)
    special = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], F)
    vv = v[np.isfinite(v).all(axis=1)]
    verts = vv[rng.integers(0, len(vv), 60)]
    area = max(gc.triangle_areas(v, t)[0][rc._valid_triangles(v, t)[1]].sum(), 1e-9)
    on = gc.sample_surface(v, t, 90.0 / area, 5)[0][:80]
    uni = rng.uniform(-1.2, 1.2, (120, 3)).astype(F)
    if len(t) > 3 and rc._valid_triangles(v, t)[1][3]:           # the centroid of triangle 3: its duplicate at the highest index ties
        uni[0] = v[t[3]].astype(np.float64).mean(axis=0).astype(F)
    far = (rng.uniform(-1.0, 1.0, (40, 3)) + 100.0).astype(F)
    pool = np.concatenate([special, verts, on, uni, far]).astype(F)
    order = np.concatenate([np.arange(3), 3 + rng.permutation(len(pool) - 3)])           # every kind among the first 63
    return pool[order]


@pytest.mark.parametrize("n_tri", [1, 255, 256, 257, 1025])
def test_brute_matches_the_restatement(dev, n_tri):
    from neddf_amd import Context
    from neddf_amd.geometry import point_mesh_distance
    v, t = _soup_mesh(n_tri)
    vd, td = T(v, dev), T(t, dev)
    pool = _query_pool(v, t)
    assert len(pool) >= 257
    ctx = Context.get(dev)
    for n_q in (1, 63, 64, 257):
        q = pool[-n_q:] if n_q == 1 else pool[:n_q]
        got = raw(ctx.point_mesh_brute(T(q, dev), vd, td))
        want = pm.point_mesh_brute(q, v, t)
        same_bits(got, want, ("brute", n_tri, n_q))
        if n_q == 257:
            assert np.isnan(got[0][:3]).all() and (got[1][:3] == -1).all() and np.isnan(got[2][:3]).all() and np.isnan(got[3][:3]).all()
            assert np.isfinite(got[0][3:]).all() and (got[1][3:] >= 0).all()
            if n_tri > 16:
                assert not np.isin(got[1], [5, 6, 8, n_tri - 1]).any()          # invalid ones, and the duplicate loses to triangle 3
            out = point_mesh_distance(T(q, dev), vd, td, method="brute")
            assert out["triangle"].dtype == torch.int64 and np.array_equal(N(out["triangle"]), got[1].astype(np.int64))
            assert np.array_equal(N(out["distance"]), np.sqrt(got[0]), equal_nan=True)
    for qq, tt in ((pool[:0], t), (pool[:5], t[:0])):                           # Q == 0 and T == 0 are legal
        same_bits(raw(ctx.point_mesh_brute(T(qq, dev), vd, T(tt, dev))), pm.point_mesh_brute(qq, v, tt), "empty")


# ---------------------------------------------------------------------------------------------------------------- grid == brute
@pytest.fixture(scope="module")
def small_sphere(dev):
    v, t = gc.uv_sphere(0.5, 12, 24)
    rng = np.random.default_rng(22)
    on = gc.sample_surface(v, t, 1000.0 / np.pi, 6)[0]
    far = np.array([[3.0, 0.1, -0.2], [-0.3, -40.0, 0.2], [100.0, 100.0, 100.0], [0.0, 0.0, 0.0], [np.nan, 0.0, 0.0]], F)
    q = np.concatenate([rng.uniform(-0.8, 0.8, (2000, 3)).astype(F), on, v, far]).astype(F)
    vd, td, qd = T(v, dev), T(t, dev), T(q, dev)
    from neddf_amd import Context
    return v, t, vd, td, qd, Context.get(dev).point_mesh_brute(qd, vd, td)


@pytest.mark.parametrize("cells", [(1, 1, 1), (2, 3, 5), (17, 17, 17), (40, 40, 40)])
@pytest.mark.parametrize("box", sorted(BOXES))
def test_grid_matches_brute_bit_for_bit(dev, small_sphere, box, cells):
    from neddf_amd.geometry import point_mesh_distance
    from neddf_amd.raycast import build_grid
    v, t, vd, td, qd, brute = small_sphere
    grid = build_grid(vd, td, box=BOXES[box], cells=cells, pad=SPHERE_PAD)
    n_items, n_over = grid.items.shape[0], grid.n_overflow
    if box == "cutting":                # both the overflow list and the cells hold triangles
        assert 0 < n_over < len(t) and n_items - n_over > 0, (n_items, n_over)
    else:
        assert n_over == 0 and n_items >= len(t)
    got = point_mesh_distance(qd, vd, td, grid=grid)
    want = point_mesh_distance(qd, vd, td, method="brute")
    assert np.array_equal(N(want["distance"]), np.sqrt(N(brute[0])), equal_nan=True)
    for k in ("distance", "triangle", "b1", "b2"):
        g, w = N(got[k]), N(want[k])
        bad = np.flatnonzero(bits(g) != bits(w))
        assert g.dtype == w.dtype and bad.size == 0, (box, cells, k, bad.size, bad[:5], g[bad[:5]], w[bad[:5]])
    assert (N(got["triangle"])[:-1] >= 0).all() and N(got["triangle"])[-1] == -1


def test_grid_on_special_meshes(dev):
    from neddf_amd import Context
    from neddf_amd.geometry import point_mesh_distance
    from neddf_amd.raycast import build_grid
    rng = np.random.default_rng(23)
    q = np.concatenate([rng.uniform(-1.0, 1.0, (300, 3)), [[np.inf, 0.0, 0.0]]]).astype(F)
    # a planar mesh: the z axis has no extent
    x, y = np.meshgrid(np.linspace(-0.5, 0.5, 9), np.linspace(-0.4, 0.4, 7))
    pv = np.stack([x.ravel(), y.ravel(), np.full(x.size, 0.25)], axis=1).astype(F)
    idx = np.arange(x.size).reshape(7, 9)
    pt = np.concatenate([np.stack([idx[:-1, :-1], idx[:-1, 1:], idx[1:, 1:]], -1).reshape(-1, 3),
                         np.stack([idx[:-1, :-1], idx[1:, 1:], idx[1:, :-1]], -1).reshape(-1, 3)]).astype(np.int32)
    sv, st = rc.soup(5, 11)
    invalid = st.copy()
    invalid[:, 1] = -3
    for name, v, t, kw in (("planar", pv, pt, {}), ("planar, 8 x 8 x 4 cells", pv, pt, dict(cells=(8, 8, 4))), ("one triangle", sv[:3], st[:1], {}),
                           ("empty", sv, st[:0], {}), ("all invalid", sv, invalid, {})):
        vd, td, qd = T(v, dev), T(t, dev), T(np.concatenate([q, v]).astype(F), dev)
        grid = build_grid(vd, td, **kw)
        got, want = point_mesh_distance(qd, vd, td, grid=grid), point_mesh_distance(qd, vd, td, method="brute")
        for k in want:
            assert np.array_equal(bits(N(got[k])), bits(N(want[k]))), (name, k)
        same_bits(raw(Context.get(dev).point_mesh_brute(qd, vd, td)), pm.point_mesh_brute(N(qd), v, t), name)
        if name in ("empty", "all invalid"):
            assert (N(want["triangle"]) == -1).all() and np.isinf(N(want["distance"])[:300]).all() and (N(want["b1"])[:300] == 0).all()
        else:
            assert (N(want["triangle"])[:300] >= 0).all()
    # a thin box far from the origin: cells below 2^-10 of the coordinates, so the query visits every list instead of walking shells
    v, t = gc.uv_sphere(0.5, 12, 24)
    far = (v * F(0.05) + F(100.0)).astype(F)
    lo, hi = far.min(axis=0).astype(np.float64), far.max(axis=0).astype(np.float64)
    vd, td = T(far, dev), T(t, dev)
    grid = build_grid(vd, td, cells=(17, 17, 17))
    assert grid.lo == tuple(lo) and grid.hi == tuple(hi) and not pm.grid_walks(grid.lo, grid.hi, grid.cells, grid.pad)[0]
    qd = T(np.concatenate([(q * F(0.1) + F(100.0)).astype(F), far, q]).astype(F), dev)
    got, want = point_mesh_distance(qd, vd, td, grid=grid), point_mesh_distance(qd, vd, td, method="brute")
    for k in want:
        assert np.array_equal(bits(N(got[k])), bits(N(want[k]))), ("far", k)


def test_refusals(dev):
    from neddf_amd._lib import NeddfError
    from neddf_amd.geometry import point_mesh_distance
    from neddf_amd.raycast import build_grid
    v, t = gc.uv_sphere(0.5, 12, 24)
    vd, td, qd = T(v, dev), T(t, dev), T(v[:7], dev)
    with pytest.raises(NeddfError, match="method"):
        point_mesh_distance(qd, vd, td, method="kd")
    with pytest.raises(NeddfError, match="grid must be the MeshGrid"):
        point_mesh_distance(qd, vd, td[:-1], grid=build_grid(vd, td))
    with pytest.raises(NeddfError, match="float32"):
        point_mesh_distance(qd.double(), vd, td)


# ---------------------------------------------------------------------------------------------------------------- mesh_distance
def test_surface_distance_between_two_spheres(dev):
    from neddf_amd.geometry import closest_points, mesh_distance, point_mesh_distance
    v, t = gc.uv_sphere(0.5, 48, 96)
    sag = gc.sphere_sagitta(0.5, 48, 96)
    inner, outer = (T(v, dev), T(t, dev)), (T((v * F(1.02)).astype(F), dev), T(t, dev))
    out = mesh_distance(inner, outer, n=2000, to="surface", return_samples=True)
    floor = mesh_distance(inner, outer, n=2000)
    msg = "to surface %.6f / %.6f, to samples %.6f / %.6f" % (out["a_to_b_mean"], out["b_to_a_mean"], floor["a_to_b_mean"], floor["b_to_a_mean"])
    print(msg)
    for k in ("a_to_b_mean", "b_to_a_mean"):
        assert 0.01 - 1.02 * sag - 1e-6 <= out[k] <= 0.01 + 1e-6, (k, msg)
    y, x = N(out["points_a"]).astype(np.float64), N(out["points_b"]).astype(np.float64)
    assert 1500 < len(y) < 2500 and 1500 < len(x) < 2500 and out["n_a"] == len(y) and out["invalid_a"] == 0 and out["invalid_b"] == 0
    assert (np.linalg.norm(y, axis=1) <= 0.5 + 1e-6).all() and (np.linalg.norm(x, axis=1) >= 1.02 * (0.5 - sag) - 1e-6).all()
    back = point_mesh_distance(T((x / 1.02).astype(F), dev), *inner)
    assert float(back["distance"].max()) <= 1e-6
    assert set(floor) <= set(out) and set(out) - set(floor) == {
        "a_to_b", "b_to_a", "a_to_b_index", "b_to_a_index", "a_to_b_b1", "a_to_b_b2", "b_to_a_b1", "b_to_a_b2", "points_a", "points_b",
        "triangle_a", "triangle_b"}
    assert out["chamfer"] == 0.5 * (out["a_to_b_mean"] + out["b_to_a_mean"]) and out["hausdorff"] == max(out["a_to_b_max"], out["b_to_a_max"])
    # the index is a triangle of the OTHER mesh and the barycentric pair names the closest point
    res = {"triangle": out["a_to_b_index"], "b1": out["a_to_b_b1"], "b2": out["a_to_b_b2"]}
    cp = closest_points(*outer, res)
    assert float(((out["points_a"] - cp).norm(dim=1) - out["a_to_b"]).abs().max()) <= 1e-6
    brute = mesh_distance(inner, outer, n=2000, to="surface", method="brute")
    for k in brute:
        assert brute[k] == out[k], k


def test_dense_and_brickwise_bunny_meshes_are_at_rounding_distance(dev, bunny):
    from neddf_amd.geometry import mesh_distance
    dense = bunny.extract_mesh(threshold=0.1, resolution=24)
    sparse = bunny.extract_mesh(threshold=0.1, resolution=24, brick=8)
    assert dense[1].shape[0] > 0 and torch.equal(dense[0], sparse[0]) and torch.equal(dense[1], sparse[1])
    out = mesh_distance(dense, sparse, n=5000, seed=4, to="surface")
    m = float(dense[0].abs().max())
    print("bunny 24: %d triangles, %d samples, hausdorff %.3e = %.2f units of 2^-24 M" % (dense[1].shape[0], out["n_a"], out["hausdorff"],
                                                                                      out["hausdorff"] / (2.0 ** -24 * m)))
    assert out["n_a"] > 4000 and out["invalid_a"] == 0 and out["hausdorff"] <= OVERSHOOT_GATE * 2.0 ** -24 * m


def test_to_samples_is_untouched_by_the_new_keyword(dev):
    from neddf_amd.geometry import mesh_distance
    (v5, t5), (v6, t6) = spheres()
    small, large = (T(v5, dev), T(t5, dev)), (T(v6, dev), T(t6, dev))
    a = mesh_distance(small, large, density=SPHERE_DENSITY, seed=SPHERE_SEED, tau=0.101, return_samples=True)
    b = mesh_distance(small, large, density=SPHERE_DENSITY, seed=SPHERE_SEED, tau=0.101, return_samples=True, to="samples")
    assert a.keys() == b.keys() and "a_to_b_b1" not in a
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert a[k].dtype == b[k].dtype and np.array_equal(bits(N(a[k])), bits(N(b[k]))), k
        else:
            assert a[k] == b[k], k
    want_a = gc.sample_surface(v5, t5, SPHERE_DENSITY, SPHERE_SEED)[0]
    want = gc.nearest_brute(want_a, gc.sample_surface(v6, t6, SPHERE_DENSITY, SPHERE_SEED)[0])
    assert np.array_equal(bits(N(a["a_to_b"])), bits(np.sqrt(want[0]))) and np.array_equal(N(a["a_to_b_index"]), want[1].astype(np.int64))


# ---------------------------------------------------------------------------------------------------------------- level_set_check
FIGURES = ("mean_error", "mean_abs_error", "rms_error", "max_abs_error", "slope_median", "slope_p99", "slope_max", "suggested_step_scale")


def test_level_set_check_of_a_distance_field(dev):
    from neddf_amd.geometry import level_set_check
    v, t = gc.uv_sphere(0.5, 24, 48)
    sag = gc.sphere_sagitta(0.5, 24, 48)

    def field(p):
        return (p.norm(dim=1) - 0.3).clamp_min(0.0)

    out = level_set_check(field, T(v, dev), T(t, dev), 0.2, 0.05, n=4000, return_samples=True)
    print({k: out[k] for k in out if not isinstance(out[k], torch.Tensor)})
    assert out["max_abs_error"] <= sag + 1e-6 and out["invalid"] == 0 and 3500 < out["n"] < 4500 and out["band"] == 0.05
    # |D - threshold| <= d + sagitta and d >= min_distance = band / 8 on the slope's points
    assert 0 < out["n_slope"] < out["n"] and 0.0 < out["slope_median"] <= out["slope_p99"] <= out["slope_max"] <= 1.0 + sag / (0.05 / 8.0) + 1e-3
    assert out["suggested_step_scale"] == min(1.0, 1.0 / out["slope_p99"])
    # the points: within the band of the mesh, on both sides of it, and the offsets are the stated sequence
    d, p = N(out["mesh_distance"]), N(out["points"]).astype(np.float64)
    assert d.max() <= 0.05 + 1e-6 and (np.linalg.norm(p, axis=1) > 0.5).sum() > 500 and (np.linalg.norm(p, axis=1) < 0.48).sum() > 500
    k = np.arange(1, out["n"] + 1, dtype=np.float64)
    s = 0.05 * (2.0 * np.modf(k * 0.6180339887498949)[0] - 1.0)
    from neddf_amd.mesh import sample_surface
    x, tid = sample_surface(T(v, dev), T(t, dev), n=4000, seed=0)
    tri = v[t[N(tid)]].astype(np.float64)
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    assert np.abs(p - (N(x).astype(np.float64) + s[:, None] * nrm)).max() <= 1e-6
    # the same seed gives the same bits, another seed other points; a non-finite field value is counted and left out
    again = level_set_check(field, T(v, dev), T(t, dev), 0.2, 0.05, n=4000, return_samples=True)
    for key in out:
        if isinstance(out[key], torch.Tensor):
            assert np.array_equal(bits(N(out[key])), bits(N(again[key]))), key
        else:
            assert out[key] == again[key], key
    other = level_set_check(field, T(v, dev), T(t, dev), 0.2, 0.05, n=4000, seed=1, return_samples=True)
    assert not np.array_equal(N(other["points"]), N(out["points"]))
    holes = level_set_check(lambda q: torch.where(torch.arange(q.shape[0], device=q.device) < 5, float("nan"), field(q)), T(v, dev), T(t, dev), 0.2,
                            0.05, n=4000)
    assert holes["invalid"] == 5 and holes["max_abs_error"] <= sag + 1e-6


def test_level_set_check_of_a_field_that_is_no_distance(dev):
    from neddf_amd.geometry import level_set_check
    v, t = gc.uv_sphere(0.5, 48, 96)
    out = level_set_check(lambda p: 2.0 * (p.norm(dim=1) - 0.3), T(v, dev), T(t, dev), 0.4, 0.2, n=4000)
    print(out)
    assert 1.7 <= out["slope_median"] <= 2.45 and out["suggested_step_scale"] < 0.6 and out["invalid"] == 0


def test_level_set_check_of_the_shipped_bunny(dev, bunny):
    v, t = bunny.extract_mesh(threshold=0.1, resolution=24)
    out = bunny.level_set_check(v, t, threshold=0.1, n=4000)
    print(out)
    assert out["invalid"] == 0 and out["n"] > 3000 and out["n_slope"] > 0 and out["band"] == 4.0 * 2.2 / 63
    assert all(np.isfinite(out[k]) for k in FIGURES), out
    from neddf_amd import NeRF
    with pytest.raises(NotImplementedError, match="no distance or sdf"):
        NeRF().to(dev).level_set_check(v, t)


def test_extract_mesh_script_check_distance(dev, tmp_path, capsys):
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
    main([str(run), "--epoch", "7", "--resolution", "24", "--threshold", "0.1"])
    plain = capsys.readouterr().out.splitlines()
    assert plain[-1].startswith("wrote ") and not any(ln.startswith("{") for ln in plain)
    main([str(run), "--epoch", "7", "--resolution", "24", "--threshold", "0.1", "--check-distance"])
    lines = capsys.readouterr().out.splitlines()
    assert [ln for ln in lines[:-1] if not ln.startswith("grid evaluation")] == [ln for ln in plain if not ln.startswith("grid evaluation")]
    out = json.loads(lines[-1])
    assert out["invalid"] == 0 and abs(out["band"] - 4.0 * 2.2 / 23) < 1e-12 and all(k in out for k in FIGURES)
    main([str(run), "--epoch", "7", "--resolution", "24", "--threshold", "0.1", "--check-distance", "0.05"])
    assert json.loads(capsys.readouterr().out.splitlines()[-1])["band"] == 0.05
