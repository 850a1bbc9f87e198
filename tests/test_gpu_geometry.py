"""Distances between surfaces on the GPU: surface sampling and brute-force nearest neighbours against the numpy restatement
(tests/geometry_check.py) bit for bit, the grid search against the brute kernel bit for bit on point sets chosen to break it, and the
Python layer end to end: the two spheres whose bounds tests/test_geometry_host.py proves on the CPU, the shipped bunny dense against
brick-wise, a cloud against its shifted copy."""
import numpy as np
import pytest
import torch

import geometry_check as gc
from test_geometry_host import SPHERE_DENSITY, SPHERE_SEED, check_sphere_distances, spheres

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def N(t):
    return t.cpu().numpy()


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------- sampling
def _strip(n_tri, density):
    """A triangle strip of n_tri triangles (triangle i = (i, i + 1, i + 2)) like tests/test_gpu_mesh_clean.py's, with -- where the strip is long
    enough -- a degenerate triangle, one with an index outside [0, V), one with a NaN vertex and one (triangle 0, on three appended
    vertices) large enough for 1 500 samples."""
    V = n_tri + 2
    v = np.random.default_rng(V).standard_normal((V, 3)).astype(np.float32)
    t = (np.arange(n_tri, dtype=np.int32)[:, None] + np.arange(3, dtype=np.int32)[None, :]).astype(np.int32)
    side = np.float32(np.sqrt(2.0 * 1500.0 / density))
    v = np.concatenate([v, [[3, 3, 3], [3 + side, 3, 3], [3, 3 + side, 3], [np.nan, 0, 0]]]).astype(np.float32)
    t[0] = [V, V + 1, V + 2]
    if n_tri > 8:
        t[2] = [4, 4, 5]
        t[5] = [5, V + 4, 6]
        t[7] = [7, 8, V + 3]
        t[8] = [-1, 8, 9]
    return v, t


def _check_sampling(dev, v, t, density, seed, what):
    from neddf_amd.mesh import sample_surface
    want_p, want_t, counts, offsets = gc.sample_surface(v, t, density, seed)
    got_p, got_t = sample_surface(T(v, dev), T(t, dev), density=density, seed=seed)
    gp, gt = N(got_p), N(got_t)
    assert gp.dtype == np.float32 and gt.dtype == np.int32 and gp.shape == want_p.shape and gt.shape == want_t.shape, (what, gp.shape, want_p.shape)
    assert np.array_equal(gt, want_t), what
    assert np.array_equal(np.bincount(gt, minlength=len(t)), counts), what                   # counts, hence offsets
    first = np.flatnonzero(np.r_[True, gt[1:] != gt[:-1]]) if len(gt) else np.zeros(0, np.int64)
    assert np.array_equal(first, offsets[counts > 0]), what
    assert np.array_equal(bits(gp), bits(want_p)), what
    return gp, gt, counts


@pytest.mark.parametrize("n_tri", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_sampling_matches_the_restatement(dev, n_tri):
    density = 40.0
    v, t = _strip(n_tri, density)
    gp, gt, counts = _check_sampling(dev, v, t, density, 5, ("strip", n_tri))
    assert counts[0] > 1000
    if n_tri > 8:
        assert counts[2] == 0 and counts[5] == 0 and counts[7] == 0 and counts[8] == 0 and counts[9:].sum() > 0
    gp2, _, _ = _check_sampling(dev, v, t, density, 6, ("strip", n_tri, "seed 6"))
    assert gp2.shape != gp.shape or not np.array_equal(bits(gp2), bits(gp))                  # another seed, other points
    gp3, gt3, _ = _check_sampling(dev, v, t, density, 5, ("strip", n_tri, "again"))
    assert np.array_equal(bits(gp3), bits(gp)) and np.array_equal(gt3, gt)


def test_sampling_edges_and_errors(dev):
    from neddf_amd import Context, NeddfError
    from neddf_amd.mesh import sample_surface
    v, t = _strip(300, 40.0)
    vd, td = T(v, dev), T(t, dev)
    p, i = sample_surface(vd, td, density=0.0)
    assert p.shape == (0, 3) and i.shape == (0,) and p.dtype == torch.float32 and i.dtype == torch.int32
    p, i = sample_surface(vd, td[:0], density=5.0)
    assert p.shape == (0, 3)
    _check_sampling(dev, v, t.astype(np.int64), 3.0, 0, "int64 triangles")
    # n: close to the request (each triangle's count is floor or one more: sd <= sqrt(T) / 2), not equal to it
    (sv, st), _ = spheres()
    p, i = sample_surface(T(sv, dev), T(st, dev), n=20000, seed=1)
    assert abs(p.shape[0] - 20000) <= 5 * np.sqrt(len(st)) / 2 + 1
    # a total that does not fit int32: one huge triangle, and many large ones
    tri = np.array([[0, 1, 2]], np.int32)
    big = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    for vv, tt, density in ((big, tri, 1e10), (big, np.repeat(tri, 8, axis=0), 1e9), (big * np.float32(1e18), tri, 1e30)):
        with pytest.raises(NeddfError, match="2\\^31"):
            sample_surface(T(vv, dev), T(tt, dev), density=density)
        with pytest.raises(NeddfError, match="2\\^31"):
            Context.get(dev).mesh_sample_count(T(vv, dev), T(tt, dev), density, 0)
    for bad in (dict(), dict(density=1.0, n=5), dict(density=-1.0), dict(density=float("nan")), dict(density=1.0, seed=2 ** 32), dict(n=-1)):
        with pytest.raises(NeddfError):
            sample_surface(vd, td, **bad)
    with pytest.raises(NeddfError):
        sample_surface(vd.double(), td, density=1.0)
    # a capacity below the count is refused, nothing is written
    ctx = Context.get(dev)
    n = ctx.mesh_sample_count(vd, td, 40.0, 5)
    with pytest.raises(NeddfError):
        ctx.mesh_sample_write(vd, td, 40.0, 5, n - 1)


# ------------------------------------------------------------------------------------------------------------ brute force
def _cloud(rng, n):
    return (rng.random((n, 3)) * 2.0 - 1.0).astype(np.float32)


def _check_brute(dev, q, p, what):
    from neddf_amd import Context
    want_d, want_i = gc.nearest_brute(q, p)
    got_d, got_i = Context.get(dev).nn_brute(T(q, dev), T(p, dev))
    gd, gi = N(got_d), N(got_i)
    assert gd.dtype == np.float32 and gi.dtype == np.int32 and gd.shape == want_d.shape, what
    assert np.array_equal(gi, want_i), (what, np.flatnonzero(gi != want_i)[:5])
    assert np.array_equal(bits(gd), bits(want_d)), (what, np.flatnonzero(bits(gd) != bits(want_d))[:5])
    return gd, gi


def test_brute_matches_the_restatement(dev):
    rng = np.random.default_rng(21)
    for nq in (1, 64, 65, 1025):
        for n in (1, 63, 64, 65, 257, 4099):
            _check_brute(dev, _cloud(rng, nq), _cloud(rng, n), (nq, n))
    gd, gi = _check_brute(dev, _cloud(rng, 70), np.zeros((0, 3), np.float32), "no targets")
    assert np.isposinf(gd).all() and (gi == -1).all()
    gd, gi = _check_brute(dev, np.zeros((0, 3), np.float32), _cloud(rng, 70), "no queries")
    assert gd.shape == (0,)


def test_brute_ties_and_non_finite_points(dev):
    rng = np.random.default_rng(22)
    p = _cloud(rng, 600)
    p[300:310] = p[40]                      # duplicates, in another tile than the original: the lowest index wins
    p[500] = p[299]
    q = np.concatenate([_cloud(rng, 100), p[[40, 299, 305]]]).astype(np.float32)
    gd, gi = _check_brute(dev, q, p, "duplicates")
    assert gi[100:].tolist() == [40, 299, 40] and (gd[100:] == 0).all()
    # NaN and Inf on both sides
    p2, q2 = p.copy(), q.copy()
    p2[40] = [np.nan, 0, 0]
    p2[299, 2] = np.inf
    p2[0, 1] = -np.inf
    q2[1] = [np.nan, np.nan, np.nan]
    q2[2, 0] = np.inf
    q2[3, 2] = -np.inf
    gd, gi = _check_brute(dev, q2, p2, "non-finite")
    assert np.isnan(gd[1:4]).all() and (gi[1:4] == -1).all() and gi[100:].tolist() == [300, 500, 300]
    assert not np.isin(gi, [40, 299, 0]).any()
    gd, gi = _check_brute(dev, q2, np.full((5, 3), np.nan, np.float32), "only invalid targets")
    assert np.isposinf(gd[0]) and (gi == -1).all()
    # d2 overflows to +inf: the answer is (+inf, the lowest valid index), not -1
    # (one squared difference of 2e19 is 4e38, above the largest float 3.4e38)
    far = (np.array([[1, 1, 1], [-1, 2, 1], [1, -1, -3]], np.float32) * np.float32(2e19)).astype(np.float32)
    far = np.concatenate([[[np.nan, 0, 0]], far]).astype(np.float32)
    qf = np.array([[-2e19, -2e19, -2e19], [0, 0, 0], [2e19, 2e19, 2e19], [3e38, 0, 0]], np.float32)
    gd, gi = _check_brute(dev, qf, far, "overflow")
    assert np.isposinf(gd[[0, 1, 3]]).all() and gi[[0, 1, 3]].tolist() == [1, 1, 1] and gd[2] == 0 and gi[2] == 1


# ------------------------------------------------------------------------------------------------------------------- grid
CELLS = ((1, 1, 1), (2, 3, 5), (17, 17, 17), (64, 64, 64))


def _point_sets(n):
    """name -> (targets [n, 3], queries, box or None (the targets' bounding box))."""
    rng = np.random.default_rng(100 + n)
    out = {}
    p = _cloud(rng, n)
    p[n // 2] = [np.nan, 0, 0]
    p[n // 3] = p[n // 5]                                                  # a tie
    q = np.concatenate([_cloud(rng, 300), p[[n // 5, 3]], [[np.nan, 0, 0]]]).astype(np.float32)
    out["uniform"] = (p, q, None)
    out["middle half box"] = (p, q, ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)))
    out["one cell"] = ((_cloud(rng, n) * np.float32(1e-3) + np.float32(0.31)).astype(np.float32), _cloud(rng, 300), ((-1, -1, -1), (1, 1, 1)))
    two = np.concatenate([_cloud(rng, n // 2) * np.float32(0.02) - np.float32(0.9), _cloud(rng, n - n // 2) * np.float32(0.02) + np.float32(0.9)])
    gap = (np.linspace(-0.85, 0.85, 200)[:, None] * np.ones(3)[None, :] + rng.standard_normal((200, 3)) * 0.01).astype(np.float32)
    out["two clusters"] = (two.astype(np.float32), np.concatenate([gap, _cloud(rng, 100)]).astype(np.float32), None)
    plane = _cloud(rng, n)
    plane[:, 1] = np.float32(0.25)
    out["planar"] = (plane, _cloud(rng, 300), None)
    out["single target"] = (np.array([[0.3, -0.2, 0.1]], np.float32), _cloud(rng, 300), None)
    out["single target in a box"] = (np.array([[0.3, -0.2, 0.1]], np.float32), _cloud(rng, 300), ((-1, -1, -1), (1, 1, 1)))
    out["far queries"] = (p, (_cloud(rng, 300) * np.float32(50.0) + np.float32([100.0, -30.0, 0.0])).astype(np.float32), None)
    return out


def _box(p, box):
    if box is not None:
        return box
    ok = np.isfinite(p).all(axis=1)
    return tuple(p[ok].min(axis=0).astype(np.float64)), tuple(p[ok].max(axis=0).astype(np.float64))


@pytest.mark.parametrize("n", [65, 4099])
def test_grid_matches_brute_bit_for_bit(dev, n):
    from neddf_amd import Context
    from neddf_amd.geometry import nearest
    ctx = Context.get(dev)
    for name, (p, q, box) in _point_sets(n).items():
        pd, qd = T(p, dev), T(q, dev)
        want_d, want_i = ctx.nn_brute(qd, pd)
        lo, hi = _box(p, box)
        for cells in CELLS:
            what = (name, n, cells)
            start, order = ctx.nn_grid_build(pd, lo, hi, cells)
            start2, order2 = ctx.nn_grid_build(pd, lo, hi, cells)
            lin, _ = gc.cell_index(p, lo, hi, cells)
            G = cells[0] * cells[1] * cells[2]
            hist = np.bincount(lin[lin >= 0], minlength=G)
            want_start = np.concatenate([[0], np.cumsum(hist)]).astype(np.int32)
            s, o = N(start), N(order)
            assert s.dtype == np.int32 and np.array_equal(s, want_start) and np.array_equal(N(start2), want_start), what
            assert len(o) == (lin >= 0).sum() and np.array_equal(np.sort(o), np.flatnonzero(lin >= 0)), what       # a permutation of the valid targets
            assert np.array_equal(lin[o], np.repeat(np.arange(G), hist)), what                                   # cell by cell the right set
            assert np.array_equal(np.sort(N(order2)), np.sort(o)) and np.array_equal(lin[N(order2)], lin[o]), what
            for st, od in ((start, order), (start2, order2), (start, order)):
                got_d, got_i = ctx.nn_grid_query(qd, pd, lo, hi, cells, st, od)
                assert torch.equal(got_i, want_i), (what, N(got_i != want_i).nonzero()[0][:5])
                assert torch.equal(got_d.view(torch.int32), want_d.view(torch.int32)), what
            d, i = nearest(qd, pd, method="grid", box=box, cells=cells)
            assert torch.equal(i, want_i.long()) and torch.equal(d.view(torch.int32), torch.sqrt(want_d).view(torch.int32)), what
        d, i = nearest(qd, pd)                                             # the default box and cells
        assert torch.equal(i, want_i.long()) and torch.equal(d.view(torch.int32), torch.sqrt(want_d).view(torch.int32)), (name, n, "defaults")


def test_grid_edges_and_errors(dev):
    from neddf_amd import Context, NeddfError
    from neddf_amd.geometry import nearest
    ctx = Context.get(dev)
    rng = np.random.default_rng(9)
    p, q = T(_cloud(rng, 100), dev), T(_cloud(rng, 50), dev)
    none = p[:0]
    d, i = nearest(q, none)
    assert torch.isposinf(d).all() and (i == -1).all() and i.dtype == torch.int64 and d.dtype == torch.float32
    d, i = nearest(none, p)
    assert d.shape == (0,) and i.shape == (0,)
    d, i = nearest(q, torch.full_like(p, float("nan")))
    assert torch.isposinf(d).all() and (i == -1).all()
    lo, hi = (-1, -1, -1), (1, 1, 1)
    for cells in ((0, 1, 1), (1025, 1, 1), (1024, 1024, 17)):
        with pytest.raises(NeddfError):
            ctx.nn_grid_build(p, lo, hi, cells)
        with pytest.raises(NeddfError):
            nearest(q, p, cells=cells)
    for box in (((0, 0, 0), (1, 1, -1)), ((0, 0, 0), (1, float("inf"), 1)), ((0, 0), (1, 1)), 5):
        with pytest.raises(NeddfError):
            nearest(q, p, box=box)
    with pytest.raises(NeddfError):
        ctx.nn_grid_build(p, (0, 0, 0), (1, float("nan"), 1), (2, 2, 2))
    for bad in (lambda: nearest(q.double(), p), lambda: nearest(q[:, :2], p), lambda: nearest(q, p, method="tree"), lambda: nearest(q.cpu(), p)):
        with pytest.raises(NeddfError):
            bad()


# ------------------------------------------------------------------------------------------------------------- end to end
def _same_dict(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), (k, a[k], b[k])


def test_sphere_distances_satisfy_the_proven_bounds(dev):
    from neddf_amd.geometry import cloud_distance, mesh_distance
    (v5, t5), (v6, t6) = spheres()
    small, large = (T(v5, dev), T(t5, dev)), (T(v6, dev), T(t6, dev))
    out = mesh_distance(small, large, density=SPHERE_DENSITY, seed=SPHERE_SEED, tau=0.101, return_samples=True)
    want_a = gc.sample_surface(v5, t5, SPHERE_DENSITY, SPHERE_SEED)[0]
    assert np.array_equal(bits(N(out["points_a"])), bits(want_a)) and out["n_a"] == len(want_a)
    check_sphere_distances(N(out["a_to_b"]), "device, %d -> %d samples" % (out["n_a"], out["n_b"]))
    assert out["invalid_a"] == 0 and out["invalid_b"] == 0 and out["density"] == SPHERE_DENSITY
    assert out["a_to_b_mean"] == float(out["a_to_b"].double().mean()) and out["a_to_b_max"] == float(out["a_to_b"].max())
    assert out["chamfer"] == 0.5 * (out["a_to_b_mean"] + out["b_to_a_mean"]) and out["hausdorff"] == max(out["a_to_b_max"], out["b_to_a_max"])
    assert 0.0 < out["precision"] < 1.0 and 0.0 < out["recall"] < 1.0
    assert out["fscore"] == 2 * out["precision"] * out["recall"] / (out["precision"] + out["recall"])
    assert out["precision"] == float((out["a_to_b"].double() <= 0.101).double().mean())
    grid = mesh_distance(small, large, density=SPHERE_DENSITY, seed=SPHERE_SEED, tau=0.101)
    brute = mesh_distance(small, large, density=SPHERE_DENSITY, seed=SPHERE_SEED, tau=0.101, method="brute")
    _same_dict(grid, brute)
    assert "a_to_b" not in grid and "precision" not in mesh_distance(small, large, n=2000)
    # invalid points are counted and left out of every reduction
    a = out["points_a"].clone()
    a[5] = float("nan")
    c = cloud_distance(a, out["points_b"])
    assert c["invalid_a"] == 1 and c["invalid_b"] == 0 and c["a_to_b_mean"] == c["a_to_b_mean"] and c["n_a"] == out["n_a"]


def test_a_cloud_against_its_shifted_copy(dev):
    """Sample once and shift the POINTS: the shifted copy of a sample is a candidate, so no nearest distance exceeds the shift."""
    from neddf_amd.geometry import cloud_distance
    from neddf_amd.mesh import sample_surface
    (v5, t5), _ = spheres()
    p, _ = sample_surface(T(v5, dev), T(t5, dev), n=20000, seed=3)
    out = cloud_distance(p, p + torch.tensor([0.01, 0.0, 0.0], device=dev))
    assert 0.0 < out["a_to_b_mean"] <= 0.01, out
    # no single distance exceeds the shift as fp32 carried it out: the sum's rounding (coordinates below 0.52) and d2's
    assert out["a_to_b_max"] <= 0.01 + 2.0 ** -24 * 0.52 + 0.01 * 2.0 ** -21, out
    assert 0.0 < out["b_to_a_mean"] <= 0.01
    same = cloud_distance(p, p.clone(), tau=0.0)
    assert same["chamfer"] == 0.0 and same["hausdorff"] == 0.0 and same["fscore"] == 1.0


def test_bunny_dense_and_brickwise_meshes_are_at_distance_zero(dev):
    from neddf_amd import NeDDF
    from neddf_amd.fixtures import BUNNY_SMOKE_CFG, bunny_smoke_weights
    from neddf_amd.geometry import mesh_distance
    net = NeDDF(**BUNNY_SMOKE_CFG)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in bunny_smoke_weights().items()})
    net.to(dev)
    net.set_iter(-1)
    for p in net.parameters():
        p.requires_grad_(False)
    dense = net.extract_mesh(resolution=48)
    sparse = net.extract_mesh(resolution=48, brick=8)
    assert dense[1].shape[0] > 0
    out = mesh_distance(dense, sparse, n=20000, seed=4)
    print("bunny 48: %d triangles, %d samples" % (dense[1].shape[0], out["n_a"]))
    assert out["chamfer"] == 0.0 and out["hausdorff"] == 0.0 and out["n_a"] == out["n_b"] > 15000
