"""The triangle BVH on the GPU: the tree against the numpy restatement (tests/bvh_check.py) array for array, the query through it against
the brute kernel bit for bit on the inputs chosen to break it, its visit counts against the restatement's exactly (a tree, not a
disguised brute force: tests/test_bvh_host.py holds the restatement to 5 % of T), and the Python layer end to end: method="bvh" where
method="grid" is accepted, distance_field_check on a field that is a distance and on one that is not, the shipped bunny, the script."""
import json
import os

import numpy as np
import pytest
import torch
from conftest import GOLDEN

import bvh_check as bc
import geometry_check as gc
import pointmesh_check as pm
from test_bvh_host import cases
from test_gpu_pointmesh import N, T, _query_pool, _soup_mesh, bits, raw, same_bits

pytestmark = pytest.mark.gpu

F = np.float32


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


@pytest.fixture(scope="module")
def bunny_mesh(bunny):
    v, t = bunny.extract_mesh(threshold=0.1, resolution=24)
    assert t.shape[0] > 1000
    return v, t


def query(dev, q, vd, td, tree):
    """The library's own outputs and visit counts through `tree`, as numpy."""
    from neddf_amd import Context
    out = Context.get(dev).point_mesh_bvh_query(T(q, dev), vd, td, tree.leaf_triangle, tree.children, tree.boxes, return_visits=True)
    return raw(out[:4]), N(out[4])


# ---------------------------------------------------------------------------------------------------------------- the tree
@pytest.mark.parametrize("n_tri", [1, 2, 3, 255, 256, 257, 1025])
def test_tree_equals_the_restatement_and_bvh_equals_brute(dev, n_tri):
    from neddf_amd import Context
    from neddf_amd.bvh import build_bvh
    v, t = _soup_mesh(n_tri)
    vd, td = T(v, dev), T(t, dev)
    want = bc.build(v, t)
    trees = [build_bvh(vd, td) for _ in range(2)]                   # twice: the atomically fitted boxes do not depend on timing
    for tree in trees:
        assert tree.lo == tuple(want["lo"]) and tree.hi == tuple(want["hi"]) and tree.n_triangles == n_tri
        assert N(tree.leaf_triangle).dtype == np.int32 and np.array_equal(N(tree.leaf_triangle), want["leaf"])
        assert tree.children.shape == (n_tri - 1, 2) and np.array_equal(N(tree.children), want["children"])
        assert tree.boxes.shape == (2 * n_tri - 1, 6) and np.array_equal(bits(N(tree.boxes)), bits(want["boxes"]))
    keys = N(Context.get(dev).bvh_keys(vd, td, trees[0].lo, trees[0].hi))
    assert np.array_equal(np.sort(keys), want["keys"])
    pool = _query_pool(v, t)
    got, visits = query(dev, pool, vd, td, trees[0])
    same_bits(got, raw(Context.get(dev).point_mesh_brute(T(pool, dev), vd, td)), ("bvh == brute", n_tri))
    ref = bc.point_mesh_bvh(pool, v, t, want)
    same_bits(got, ref[:4], ("bvh == restatement", n_tri))
    assert visits.dtype == np.int32 and np.array_equal(visits, ref[4]), (n_tri, visits[:8], ref[4][:8])
    assert np.isnan(got[0][:3]).all() and (got[1][:3] == -1).all() and (visits[:3] == 0).all()
    if n_tri > 16:
        assert not np.isin(got[1], [5, 6, 8, n_tri - 1]).any()          # invalid ones, and the duplicate loses to triangle 3


@pytest.mark.parametrize("case", cases(), ids=lambda c: c[0])
def test_bvh_equals_brute_on_special_meshes(dev, case):
    from neddf_amd import Context
    from neddf_amd.bvh import build_bvh
    from neddf_amd.geometry import point_mesh_distance
    name, v, t, q = case
    vd, td = T(v, dev), T(t, dev)
    tree = build_bvh(vd, td)
    got, visits = query(dev, q, vd, td, tree)
    same_bits(got, raw(Context.get(dev).point_mesh_brute(T(q, dev), vd, td)), name)
    ref = bc.point_mesh_bvh(q, v, t)
    same_bits(got, ref[:4], name)
    assert np.array_equal(visits, ref[4]), (name, visits[:8], ref[4][:8])
    fin = np.isfinite(q).all(axis=1)
    if name in ("no triangle", "all invalid"):
        assert np.isinf(got[0][fin]).all() and (got[1] == -1).all() and (got[2][fin] == 0).all() and (visits == 0).all()
    if name == "300 duplicates":
        assert (got[1] == 0).all() and (visits == 300).all()
    if name == "offset 1000, 2^-8":                                  # rounding dominates: nearly everything must be visited
        assert visits[:60].mean() > 0.5 * len(t)
    out = point_mesh_distance(T(q, dev), vd, td, method="bvh", bvh=tree)                # the Python layer, and Q == 0
    assert np.array_equal(N(out["triangle"]), got[1].astype(np.int64)) and np.array_equal(N(out["distance"]), np.sqrt(got[0]), equal_nan=True)
    assert point_mesh_distance(T(q[:0], dev), vd, td, method="bvh")["distance"].shape == (0,)


def test_bvh_equals_grid_on_the_bunny(dev, bunny_mesh):
    from neddf_amd.bvh import build_bvh
    from neddf_amd.geometry import point_mesh_distance
    from neddf_amd.mesh import sample_surface
    v, t = bunny_mesh
    on = sample_surface(v, t, n=3000, seed=2)[0]
    lo, hi = v.min(dim=0).values, v.max(dim=0).values
    u = torch.from_numpy(np.random.default_rng(33).uniform(-0.25, 1.25, (3000, 3)).astype(F)).to(dev)
    q = torch.cat([on, lo + u * (hi - lo), v[::7]]).contiguous()
    tree = build_bvh(v, t)
    got, want = point_mesh_distance(q, v, t, method="bvh", bvh=tree), point_mesh_distance(q, v, t, method="grid")
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(bits(N(got[k])), bits(N(want[k]))), k
    from neddf_amd import Context
    visits = N(Context.get(dev).point_mesh_bvh_query(q, v, t, tree.leaf_triangle, tree.children, tree.boxes, return_visits=True)[4])
    print("bunny: %d triangles, %.1f leaf evaluations per query (max %d)" % (t.shape[0], visits.mean(), visits.max()))


def test_pass_through_returns_what_the_grid_returns(dev, bunny, bunny_mesh):
    from neddf_amd.geometry import mesh_distance
    v, t = bunny_mesh
    other = ((v * 1.01).contiguous(), t)
    a = mesh_distance((v, t), other, n=3000, seed=4, to="surface", method="bvh", return_samples=True)
    b = mesh_distance((v, t), other, n=3000, seed=4, to="surface", method="grid", return_samples=True)
    c = bunny.level_set_check(v, t, threshold=0.1, n=3000, method="bvh", return_samples=True)
    d = bunny.level_set_check(v, t, threshold=0.1, n=3000, method="grid", return_samples=True)
    for x, y in ((a, b), (c, d)):
        assert x.keys() == y.keys()
        for k in x:
            if isinstance(x[k], torch.Tensor):
                assert x[k].dtype == y[k].dtype and np.array_equal(bits(N(x[k])), bits(N(y[k]))), k
            else:
                assert x[k] == y[k] or (x[k] != x[k] and y[k] != y[k]), k
    assert a["n_a"] > 2000 and c["n"] > 2000


def test_refusals(dev):
    import ctypes as C
    from neddf_amd import Context
    from neddf_amd._lib import NeddfError, _ptr
    from neddf_amd.bvh import build_bvh
    from neddf_amd.geometry import point_mesh_distance
    v, t = gc.uv_sphere(0.5, 12, 24)
    vd, td, qd = T(v, dev), T(t, dev), T(v[:7], dev)
    tree = build_bvh(vd, td)
    with pytest.raises(NeddfError, match="'grid', 'brute' or 'bvh'"):
        point_mesh_distance(qd, vd, td, method="kd")
    with pytest.raises(NeddfError, match="bvh must be the MeshBVH"):
        point_mesh_distance(qd, vd, td[:-1], method="bvh", bvh=tree)
    with pytest.raises(NeddfError, match="bvh must be the MeshBVH"):
        point_mesh_distance(qd, vd, td, method="grid", bvh="tree")
    # the C ABI: negative counts and needed NULLs are NEDDF_EINVAL (-1), 2^31 triangles NEDDF_EUNSUPPORTED (-3), and a tree whose leaf
    # count is not the mesh's is refused, not followed
    ctx = Context.get(dev)
    lib, box = ctx.lib, (C.c_double * 3)(0.0, 0.0, 0.0)
    n_v, n_t = vd.shape[0], td.shape[0]
    keys = torch.zeros(n_t, device=dev, dtype=torch.int64)
    out = [torch.zeros(7, device=dev) for _ in range(4)]
    out[1] = out[1].int()
    assert lib.neddf_bvh_keys(ctx.h, _ptr(vd), n_v, _ptr(td), -1, box, box, _ptr(keys), None) == -1
    assert lib.neddf_bvh_keys(ctx.h, _ptr(vd), n_v, _ptr(td), n_t, box, box, None, None) == -1
    assert lib.neddf_bvh_keys(ctx.h, _ptr(vd), n_v, _ptr(td), n_t, None, box, _ptr(keys), None) == -1
    assert lib.neddf_bvh_keys(ctx.h, _ptr(vd), n_v, _ptr(td), 2 ** 31, box, box, _ptr(keys), None) == -3
    assert lib.neddf_bvh_build(ctx.h, _ptr(vd), n_v, _ptr(td), n_t, None, _ptr(tree.leaf_triangle), _ptr(tree.children), _ptr(tree.boxes), None) == -1
    assert lib.neddf_bvh_build(ctx.h, _ptr(vd), n_v, _ptr(td), -3, _ptr(keys), _ptr(tree.leaf_triangle), _ptr(tree.children), _ptr(tree.boxes), None) == -1
    tail = [_ptr(x) for x in out] + [None, None]
    args = [ctx.h, _ptr(qd), 7, _ptr(vd), n_v, _ptr(td), n_t, _ptr(tree.leaf_triangle), _ptr(tree.children), _ptr(tree.boxes)]
    assert lib.neddf_point_mesh_bvh_query(*args, n_t - 1, *tail) == -1
    assert lib.neddf_point_mesh_bvh_query(*args[:7], None, _ptr(tree.children), _ptr(tree.boxes), n_t, *tail) == -1
    assert lib.neddf_point_mesh_bvh_query(*args[:2], -1, *args[3:], n_t, *tail) == -1
    assert lib.neddf_point_mesh_bvh_query(*args[:2], 2 ** 31, *args[3:], n_t, *tail) == -3
    assert lib.neddf_point_mesh_bvh_query(*args, n_t, *tail) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- distance_field_check
SPHERE = (0.5, 96, 192)


def test_distance_field_check_of_a_distance_field_and_of_a_scaled_one(dev):
    from neddf_amd.geometry import distance_field_check
    v, t = gc.uv_sphere(*SPHERE)
    sag = gc.sphere_sagitta(*SPHERE)                # the mesh lies between the spheres of radius r - sag and r: | | |p| - r | - d | <= sag
    vd, td = T(v, dev), T(t, dev)

    def field(p):
        return (p.norm(dim=1) - 0.5).abs()

    out = distance_field_check(field, vd, td, 0.0, n=20000, return_samples=True)
    print({k: out[k] for k in out if not isinstance(out[k], torch.Tensor)})
    assert out["n"] == 20000 and out["invalid"] == 0 and len(out["bins"]) == 8 and out["max_abs_error"] <= sag + 1e-6
    assert sum(b["count"] for b in out["bins"]) == out["n"] - out["invalid"]
    half = 0.5 + 0.25 * 2.0 * 0.5 * np.sqrt(3.0)
    assert np.allclose(out["box"][0], [-half] * 3, atol=1e-6) and np.allclose(out["box"][1], [half] * 3, atol=1e-6)
    assert abs(out["max_distance"] - (half * np.sqrt(3.0) - 0.5)) < 0.05
    width = out["max_distance"] / 8
    rho = sag / (width / 8.0)                       # on the slope's points d >= width / 8, so F / d lies within 1 +- sag / d of the scale
    for i, b in enumerate(out["bins"]):
        assert b["count"] > 0 and b["mean_abs_error"] <= sag + 1e-6, (i, b)
        assert abs(b["lo"] - i * width) < 1e-12 and 0 < b["n_slope"] <= b["count"]
        assert 1.0 - rho - 1e-6 <= b["slope_median"] <= b["slope_p99"] <= 1.0 + rho + 1e-6, (i, b, rho)
    assert 1.0 / (1.0 + rho) - 1e-6 <= out["suggested_step_scale"] <= 1.0
    # the points: the stated sequence, deterministic, inside the box, on both sides of the surface; the distances: the brute kernel's
    k = np.arange(1, 20001, dtype=np.float64)[:, None]
    u = np.modf(k * np.array([0.8191725133961645, 0.6710436067037893, 0.5497004779019702])[None, :])[0]
    p = N(out["points"]).astype(np.float64)
    assert np.abs(p - (-half + u * 2.0 * half)).max() <= 1e-6
    radius = np.linalg.norm(p, axis=1)
    assert (radius < 0.45).sum() > 300 and (radius > 1.0).sum() > 3000
    from neddf_amd.geometry import point_mesh_distance
    brute = point_mesh_distance(out["points"][:2000], vd, td, method="brute")["distance"]
    assert np.array_equal(bits(N(brute)), bits(N(out["mesh_distance"][:2000])))
    again = distance_field_check(field, vd, td, 0.0, n=20000, method="grid")
    assert {k: x for k, x in out.items() if not isinstance(x, torch.Tensor)} == again
    other = distance_field_check(field, vd, td, 0.0, n=20000, seed=1, return_samples=True)
    assert not np.array_equal(N(other["points"]), N(out["points"]))
    holes = distance_field_check(lambda q: torch.where(torch.arange(q.shape[0], device=q.device) < 5, float("nan"), field(q)), vd, td, 0.0, n=20000)
    assert holes["invalid"] == 5 and sum(b["count"] for b in holes["bins"]) == 20000 - 5
    # a field that oversteps by half: slope 1.5 in every range of distances, and the tracer's step to match
    steep = distance_field_check(lambda q: 1.5 * field(q), vd, td, 0.0, n=20000, bins=4)
    rho = sag / (steep["max_distance"] / 4 / 8.0)
    assert len(steep["bins"]) == 4
    for b in steep["bins"]:
        assert 1.5 * (1.0 - rho) - 1e-6 <= b["slope_median"] <= b["slope_p99"] <= 1.5 * (1.0 + rho) + 1e-6, (b, rho)
    assert 1.0 / (1.5 * (1.0 + rho)) - 1e-6 <= steep["suggested_step_scale"] <= 1.0 / (1.5 * (1.0 - rho)) + 1e-6
    assert abs(steep["suggested_step_scale"] - 2.0 / 3.0) < 0.05


def _finite_report(out, n):
    assert out["n"] == n and sum(b["count"] for b in out["bins"]) == n - out["invalid"]
    for k in ("mean_error", "mean_abs_error", "rms_error", "max_abs_error", "max_distance", "suggested_step_scale"):
        assert np.isfinite(out[k]), (k, out[k])
    assert any(b["count"] > 0 and np.isfinite(b["mean_abs_error"]) and np.isfinite(b["slope_p99"]) for b in out["bins"])


def test_distance_field_check_of_the_shipped_bunny(dev, bunny, bunny_mesh):
    v, t = bunny_mesh
    out = bunny.distance_field_check(v, t, threshold=0.1, n=4000)
    print(out)
    _finite_report(out, 4000)
    assert out["invalid"] == 0
    from neddf_amd import NeRF
    with pytest.raises(NotImplementedError, match="no distance or sdf"):
        NeRF().to(dev).distance_field_check(v, t)


def test_extract_mesh_script_check_volume(dev, tmp_path, capsys):
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
    main([str(run), "--epoch", "7", "--resolution", "24", "--threshold", "0.1", "--check-distance", "--check-volume", "3000"])
    lines = capsys.readouterr().out.splitlines()
    near, volume = json.loads(lines[-2]), json.loads(lines[-1])
    assert "band" in near and "bins" in volume and "band" not in volume
    _finite_report(volume, 3000)
    main([str(run), "--epoch", "7", "--resolution", "24", "--threshold", "0.1", "--check-volume"])
    lines = capsys.readouterr().out.splitlines()
    assert lines[-2].startswith("wrote ") and json.loads(lines[-1])["n"] == 100000
