"""Ray casting on meshes on the GPU: the brute kernel against the numpy restatement (tests/raycast_check.py) bit for bit, the grid
against the brute kernel bit for bit on boxes, cell counts, rays and meshes chosen to break it, the grid build against its restatement,
and the Python layer end to end: render_image_mesh against cast_rays, and the shipped bunny network's mesh seen from a dataset camera."""
import os

import numpy as np
import pytest
import torch
from conftest import GOLDEN

import geometry_check as gc
import raycast_check as rc

pytestmark = pytest.mark.gpu

KEYS = ("t", "triangle", "b1", "b2")
SPHERE_PAD = 2.0 ** -12 * np.sqrt(3.0)          # above the library's limit for every box below (the largest: 9 * 2^-16)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def N(t):
    return t.cpu().numpy()


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same_bits(got, want, what):
    """got: the dict of cast_rays (device); want: a dict of device tensors or the restatement's tuple."""
    want = dict(zip(KEYS, want)) if isinstance(want, tuple) else want
    for k in KEYS:
        g, w = N(got[k]) if isinstance(got[k], torch.Tensor) else got[k], N(want[k]) if isinstance(want[k], torch.Tensor) else want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.flatnonzero(bits(g) != bits(w))
        assert bad.size == 0, (what, k, bad.size, bad[:5], g[bad[:5]], w[bad[:5]])


# ---------------------------------------------------------------------------------------------------------------- brute == restatement
def _soup_mesh(n_tri):
    """The soup with -- where it is large enough -- a degenerate triangle, an index outside [0, V), a NaN vertex, and an exact duplicate of
    triangle 3 at the highest index."""
    v, t = rc.soup(n_tri, 11)
    if n_tri > 8:
        v = np.concatenate([v, [[np.nan, 0.1, 0.2]]]).astype(np.float32)
        t = t.copy()
        t[1] = [t[1, 0], t[1, 0], t[1, 1]]
        t[2] = [t[2, 0], len(v), t[2, 1]]
        t[5] = [t[5, 0], len(v) - 1, t[5, 1]]
        t[6] = [-1, t[6, 1], t[6, 2]]
        t[n_tri - 1] = t[3]
    return v, t


def _special_rays():
    z = np.float32(-0.0)
    o = [[np.nan, 0, 3], [0, 0, 3], [0, 0, 3], [0, np.inf, 3]]
    d = [[0, 0, -1], [0, np.inf, -1], [0, 0, 0], [0, 0, -1]]
    for a in range(3):                          # the six axis directions, zero components of both signs
        for sign in (1.0, -1.0):
            dd = np.array([z, 0.0, z], np.float32) if sign > 0 else np.array([0.0, z, 0.0], np.float32)
            dd[a] = sign
            oo = np.array([0.11, -0.07, 0.05], np.float32)
            oo[a] = -3.0 * sign
            o.append(oo)
            d.append(dd)
    o += [[0.0, 0.0, 0.0], [0.05, -0.1, 0.02], [0.2, 0.1, -0.1]]           # starting inside the soup
    d += [[0.3, -0.5, 0.8], [-1.0, 0.2, 0.1], [0.0, 0.0, 2.5]]
    return np.array(o, np.float32), np.array(d, np.float32)


def _ray_pool(n_tri):
    """(origins, dirs, the number of special rays in front): the special rays, 8 rays at triangle 3 (where there is one), rays at random
    triangles of the soup."""
    v, t = rc.soup(n_tri, 11)
    so, sd = rc.soup_rays(v, t, 257)
    if n_tri > 3:
        so[:8], sd[:8] = rc.soup_rays(v, t[3:4], 8, seed=13)
    po, pd = _special_rays()
    return np.concatenate([po, so]), np.concatenate([pd, sd]), len(po)


@pytest.mark.parametrize("n_tri", [1, 255, 256, 257, 1025])
def test_brute_matches_the_restatement(dev, n_tri):
    from neddf_amd.raycast import cast_rays
    v, t = _soup_mesh(n_tri)
    vd, td = T(v, dev), T(t, dev)
    pool_o, pool_d, n_special = _ray_pool(n_tri)
    pad = 2.0 ** -10
    for n_rays in (1, 63, 64, 65, 257):
        o, d = pool_o[:n_rays], pool_d[:n_rays]
        got = cast_rays(T(o, dev), T(d, dev), vd, td, method="brute", pad=pad)
        want = rc.cast_rays(o, d, v, t, pad=pad)
        same_bits(got, want, ("brute", n_tri, n_rays))
        if n_rays == 257:
            tri = N(got["triangle"])
            assert np.isnan(N(got["t"])[:4]).all() and (tri[:4] == -1).all() and np.isnan(N(got["b1"])[:4]).all()
            assert not np.isnan(N(got["t"])[4:]).any()
            assert (tri[n_special:] >= 0).mean() > 0.9
            if n_tri > 8:
                assert (tri[4:n_special] >= 0).any()
                assert not np.isin(tri, [1, 2, 5, 6, n_tri - 1]).any()         # degenerate, invalid, and the duplicate loses to triangle 3
                assert n_tri > 300 or (tri == 3).any()          # (in the densest soup another triangle is in front)


def test_brute_range_cuts_the_first_hit(dev):
    from neddf_amd.raycast import cast_rays
    v, t = _soup_mesh(257)
    o, d, _ = _ray_pool(257)
    pad = 2.0 ** -10
    first = rc.cast_rays(o, d, v, t, pad=pad)
    second = None
    for i in np.flatnonzero(first[1] >= 0):             # a ray with a second hit well behind its first
        nxt = rc.cast_rays(o[i:i + 1], d[i:i + 1], v, t, t_min=first[0][i] + np.float32(0.05), pad=pad)
        if nxt[1][0] >= 0:
            second = (i, nxt[0][0], nxt[1][0])
            break
    assert second is not None
    i, t2, j2 = second
    t_min, t_max = 0.5 * (first[0][i] + t2), t2 + 0.01
    got = cast_rays(T(o, dev), T(d, dev), T(v, dev), T(t, dev), t_min=t_min, t_max=t_max, method="brute", pad=pad)
    same_bits(got, rc.cast_rays(o, d, v, t, t_min=t_min, t_max=t_max, pad=pad), "range")
    assert N(got["triangle"])[i] == j2 != first[1][i] and N(got["t"])[i] == t2
    # t_min above t_max: nothing; an empty ray set and an empty mesh are legal
    none = cast_rays(T(o, dev), T(d, dev), T(v, dev), T(t, dev), t_min=2.0, t_max=1.0, method="brute", pad=pad)
    assert (N(none["triangle"]) == -1).all()
    for oo, tt in ((o[:0], t), (o, t[:0])):
        got = cast_rays(T(oo, dev), T(oo, dev) + 1.0, T(v, dev), T(tt, dev), method="brute", pad=pad)
        same_bits(got, rc.cast_rays(oo, oo + 1.0, v, tt, pad=pad), "empty")


# ---------------------------------------------------------------------------------------------------------------- grid == brute
BOXES = {"tight": None, "half": ((-0.6, -0.6, -0.013), (0.6, 0.6, 0.6)), "large": ((-4.0, -4.0, -4.0), (5.0, 5.0, 5.0))}


def _box(v, name):
    return (v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)) if BOXES[name] is None else tuple(np.array(b) for b in BOXES[name])


def _grid_rays(lo, hi, cells):
    """Rays chosen against the traversal: origins inside the sphere, rays that start on a cell plane and travel within it, rays parallel to
    each axis through cell corners, rays that miss the box."""
    rng = np.random.default_rng(17)
    lo, hi, g = np.asarray(lo, np.float64), np.asarray(hi, np.float64), np.asarray(cells)
    edge = (hi - lo) / g
    o, d = [], []
    inside = rng.uniform(-0.25, 0.25, (64, 3))
    o.append(inside)
    d.append(rng.standard_normal((64, 3)))
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for k in range(0, g[a] + 1, max(1, g[a] // 4)):
            for s in range(8):
                oo = lo - 0.3 + rng.random(3) * (hi - lo + 0.6)
                oo[a] = lo[a] + k * edge[a]                        # on the plane between cells k - 1 and k
                dd = np.zeros(3)
                dd[b], dd[c] = rng.standard_normal(2)
                o.append(oo[None])
                d.append(dd[None])
                corner = lo + np.floor(rng.random(3) * (g + 1)) * edge     # parallel to axis a through a cell corner
                dd = np.zeros(3)
                dd[a] = 1.0 if s % 2 else -1.0
                corner[a] = lo[a] - 1.0 if s % 2 else hi[a] + 1.0
                o.append(corner[None])
                d.append(dd[None])
    miss_o = np.stack([hi + 1.0 + rng.random(3) for _ in range(16)])
    o.append(miss_o)
    d.append(np.abs(rng.standard_normal((16, 3))) + 0.1)
    return np.concatenate(o).astype(np.float32), np.concatenate(d).astype(np.float32)


@pytest.fixture(scope="module")
def sphere(dev):
    v, t = gc.uv_sphere(*rc.SPHERE)
    fo, fd = rc.fan_rays()
    ao, ad, _ = rc.aimed_rays(v, t)
    return dict(v=v, t=t, vd=T(v, dev), td=T(t, dev), o=np.concatenate([fo, ao]), d=np.concatenate([fd, ad]))


@pytest.mark.parametrize("cells", [(1, 1, 1), (4, 4, 4), (17, 5, 3), (64, 64, 64)])
@pytest.mark.parametrize("box", ["tight", "half", "large"])
def test_grid_matches_brute_on_the_sphere(dev, sphere, box, cells):
    from neddf_amd.raycast import build_grid, cast_rays
    lo, hi = _box(sphere["v"], box)
    grid = build_grid(sphere["vd"], sphere["td"], box=(lo, hi), cells=cells, pad=SPHERE_PAD)
    assert (grid.n_overflow > 0) == (box == "half")
    xo, xd = _grid_rays(lo, hi, cells)
    o, d = T(np.concatenate([sphere["o"], xo]), dev), T(np.concatenate([sphere["d"], xd]), dev)
    for t_min, t_max in ((0.0, float("inf")), (1.7, 2.2), (-1.0, 0.4)):
        brute = cast_rays(o, d, sphere["vd"], sphere["td"], t_min=t_min, t_max=t_max, method="brute", pad=SPHERE_PAD)
        got = cast_rays(o, d, sphere["vd"], sphere["td"], t_min=t_min, t_max=t_max, method="grid", grid=grid)
        same_bits(got, brute, (box, cells, t_min, t_max))
    hit = N(brute["triangle"]) >= 0
    assert hit.any() and not hit.all()


def test_grid_far_origins_and_default_grid(dev, sphere):
    """Origins far beyond the box take the every-triangle route of the query; the default grid (bounds, cells, pad) returns the brute bits too."""
    from neddf_amd.raycast import build_grid, cast_rays
    rng = np.random.default_rng(3)
    target = rng.uniform(-0.25, 0.25, (256, 3))            # inside the sphere: a ray from nearby cannot miss
    o = rng.standard_normal((256, 3))
    o *= np.repeat([3.0, 300.0, 3e4, 3e6], 64)[:, None] / np.linalg.norm(o, axis=1, keepdims=True)
    d = target - o
    o, d = T(o.astype(np.float32), dev), T(d.astype(np.float32), dev)
    grid = build_grid(sphere["vd"], sphere["td"])
    assert grid.n_overflow == 0 and len(grid.cells) == 3
    got = cast_rays(o, d, sphere["vd"], sphere["td"], grid=grid)
    same_bits(got, cast_rays(o, d, sphere["vd"], sphere["td"], method="brute", pad=grid.pad), "far")
    assert (N(got["triangle"])[:64] >= 0).all()
    same_bits(cast_rays(o, d, sphere["vd"], sphere["td"]), cast_rays(o, d, sphere["vd"], sphere["td"], method="brute"), "defaults")


def _quad_mesh(n=16):
    x = np.linspace(-1.0, 1.0, n + 1)
    v = np.stack([np.tile(x, n + 1), np.repeat(x, n + 1), np.zeros((n + 1) ** 2)], axis=1).astype(np.float32)
    i = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).reshape(-1)
    t = np.concatenate([np.stack([i, i + 1, i + n + 2], 1), np.stack([i, i + n + 2, i + n + 1], 1)]).astype(np.int32)
    return v, t


def _awkward(name):
    rng = np.random.default_rng(23)
    if name == "planar":
        return _quad_mesh()
    if name == "spanning":          # one triangle across the whole box and 500 small ones
        c = rng.uniform(-0.9, 0.9, (500, 1, 3))
        v = np.concatenate([[[-1.0, -1.0, -1.0], [1.0, 1.0, -0.2], [-0.3, 1.0, 1.0]], (c + rng.uniform(-0.03, 0.03, (500, 3, 3))).reshape(-1, 3)])
        return v.astype(np.float32), np.arange(1503, dtype=np.int32).reshape(501, 3)
    if name == "empty":
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    v, t = rc.soup(40, 4)           # invalid triangles only
    v = np.concatenate([v, [[np.inf, 0, 0]]]).astype(np.float32)
    t = t.copy()
    t[::2, 1] = len(v) - 1
    t[1::2, 2] = len(v) + 3
    return v, t


@pytest.mark.parametrize("name", ["planar", "spanning", "empty", "invalid"])
def test_grid_matches_brute_on_awkward_meshes(dev, name):
    from neddf_amd.raycast import build_grid, cast_rays
    v, t = _awkward(name)
    rng = np.random.default_rng(29)
    target = np.concatenate([rng.uniform(-1.1, 1.1, (2048, 2)), np.zeros((2048, 1))], axis=1) if name == "planar" else rng.uniform(-1.0, 1.0, (2048, 3))
    if name == "spanning":          # the first 256 rays are aimed at points of the spanning triangle
        w = rng.dirichlet(np.ones(3), 256)
        target[:256] = w @ v[:3].astype(np.float64)
    o = rng.standard_normal((2048, 3))
    o *= 3.0 / np.linalg.norm(o, axis=1, keepdims=True)
    if name == "planar":
        o[:, 2] = np.where(np.abs(o[:, 2]) < 0.5, 0.5, o[:, 2])          # well off the plane: no ray is edge-on to it
    d = target - o
    aimed_at = np.linalg.norm(d, axis=1)
    d /= aimed_at[:, None]
    # rays inside the plane z = 0 (edge-on to the planar mesh) and along the axes
    o = np.concatenate([o, np.concatenate([rng.uniform(-1.5, 1.5, (64, 2)), np.zeros((64, 1))], axis=1), [[0.1, 0.2, 2.0], [-2.0, 0.3, 0.0]]])
    d = np.concatenate([d, np.concatenate([rng.standard_normal((64, 2)), np.zeros((64, 1))], axis=1), [[0.0, -0.0, -1.0], [1.0, 0.0, -0.0]]])
    od, dd, vd, td = T(o.astype(np.float32), dev), T(d.astype(np.float32), dev), T(v, dev), T(t, dev)
    for cells in (None, (16, 16, 16), (5, 3, 1)):
        grid = build_grid(vd, td, cells=cells)
        brute = cast_rays(od, dd, vd, td, method="brute", pad=grid.pad)
        same_bits(cast_rays(od, dd, vd, td, grid=grid), brute, (name, cells))
        tri, t_hit = N(brute["triangle"]), N(brute["t"])
        if name == "planar":        # a ray at a point well inside the square [-1, 1]^2 meets the plane there; one at a point outside it misses
            inside, outside = (np.abs(target[:, :2]) < 0.999).all(axis=1), (np.abs(target[:, :2]) > 1.001).any(axis=1)
            assert inside.sum() > 1000 and (tri[:2048][inside] >= 0).all() and (tri[:2048][outside] == -1).all()
            assert np.abs(t_hit[:2048][inside] - aimed_at[inside]).max() < 1e-4
            assert (tri[2048:2048 + 64] == -1).all()        # edge-on rays in the plane: every edge function is 0, det is 0
        elif name == "spanning":    # a ray at a point of the spanning triangle hits it there, or a small triangle in front of it
            assert (tri[:256] >= 0).all() and (t_hit[:256] <= aimed_at[:256] + 1e-4).all() and (tri[:256] == 0).any()
        else:
            assert (tri == -1).all() and np.isinf(t_hit).all()
        assert grid.items.shape[0] > 0 or name in ("empty", "invalid")


# ---------------------------------------------------------------------------------------------------------------- the build
@pytest.mark.parametrize("box,cells", [("tight", (4, 4, 4)), ("half", (17, 5, 3)), ("large", (17, 5, 3)), ("half", (1, 1, 1))])
def test_grid_build_matches_the_restatement(dev, sphere, box, cells):
    from neddf_amd import Context, NeddfError
    from neddf_amd.raycast import build_grid
    lo, hi = _box(sphere["v"], box)
    grid = build_grid(sphere["vd"], sphere["td"], box=(lo, hi), cells=cells, pad=SPHERE_PAD)
    pairs, overflow = rc.grid_lists(sphere["v"], sphere["t"], lo, hi, cells, SPHERE_PAD)
    want = rc.cell_start(pairs, overflow, cells)
    start, items = N(grid.cell_start), N(grid.items)
    assert start.dtype == np.int32 and np.array_equal(start, want)
    G = cells[0] * cells[1] * cells[2]
    got_pairs = np.stack([np.repeat(np.arange(G + 1), np.diff(start)), items], axis=1)
    got_pairs = got_pairs[np.lexsort((got_pairs[:, 1], got_pairs[:, 0]))]               # the order inside a list may depend on timing
    assert np.array_equal(got_pairs[got_pairs[:, 0] < G], pairs)
    assert np.array_equal(got_pairs[got_pairs[:, 0] == G][:, 1], overflow)
    ctx = Context.get(dev)
    n = ctx.raycast_grid_count(sphere["vd"], sphere["td"], lo, hi, cells, SPHERE_PAD)
    assert n == len(items) == want[-1]
    with pytest.raises(NeddfError, match="capacity"):
        ctx.raycast_grid_build(sphere["vd"], sphere["td"], lo, hi, cells, SPHERE_PAD, n - 1)
    low = 0.99 * rc.min_pad(lo, hi)
    for call in (lambda: ctx.raycast_grid_count(sphere["vd"], sphere["td"], lo, hi, cells, low),
                 lambda: ctx.raycast_grid_build(sphere["vd"], sphere["td"], lo, hi, cells, low, n),
                 lambda: ctx.raycast_grid_query(sphere["vd"][:1], sphere["vd"][:1], sphere["vd"], sphere["td"], lo, hi, cells, low, grid.cell_start,
                                                grid.items, 0.0, 1.0)):
        with pytest.raises(NeddfError, match="pad below"):
            call()
    with pytest.raises(NeddfError, match="pad"):
        ctx.raycast_brute(sphere["vd"][:1], sphere["vd"][:1], sphere["vd"], sphere["td"], 0.0, 1.0, -1.0)


# ---------------------------------------------------------------------------------------------------------------- the Python layer
W, H = 37, 29


def _look_at(eye, target):
    z = (eye - target) / np.linalg.norm(eye - target)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z], 1).astype(np.float32), eye.astype(np.float32)


@pytest.fixture(scope="module")
def view(dev):
    import neddf_amd
    from neddf_amd.fixtures import BUNNY_SMOKE_CFG
    render = neddf_amd.NeRFRender(dict(BUNNY_SMOKE_CFG, _target_="neddf.network.NeDDF"), sample_coarse=16, sample_fine=32, dist_near=2.0,
                                  dist_far=6.0, max_dist=6.0, use_coarse_network=False, sampling_type="cone").to(dev)
    R, Tr = _look_at(np.array([1.9, -2.2, 1.1]), np.zeros(3))
    cam = neddf_amd.Camera(neddf_amd.PinholeCalib(np.array([60.0, 60.0, W / 2.0, H / 2.0])), None).to(dev)
    cam.R, cam.T = torch.from_numpy(R).to(dev), torch.from_numpy(Tr).to(dev)
    return render, cam


def test_render_image_mesh(dev, sphere, view):
    from neddf_amd.raycast import cast_rays
    render, cam = view
    vd, td = sphere["vd"], sphere["td"]
    rng = np.random.default_rng(8)
    colors = T(rng.random(sphere["v"].shape).astype(np.float32), dev)
    targets = ["depth", "transmittance", "triangle", "normal", "color"]
    img = render.render_image_mesh(W, H, cam, vd, td, targets, colors=colors, background=0.25)
    assert list(img) == targets and img["depth"].shape == (H, W) and img["normal"].shape == (H, W, 3) and img["triangle"].dtype == torch.int32
    idx = torch.arange(W * H, device=dev)
    rd, ro = render._ctx(dev).raygen(torch.stack([idx % W, idx // W], 1), cam.descriptor())
    hits = cast_rays(ro, rd, vd, td, t_min=2.0, t_max=6.0)
    hit = N(hits["triangle"]) >= 0
    assert 0.1 < hit.mean() < 0.9
    depth, trans, tri = N(img["depth"]).reshape(-1), N(img["transmittance"]).reshape(-1), N(img["triangle"]).reshape(-1)
    assert np.array_equal(bits(depth[hit]), bits(N(hits["t"])[hit])) and np.array_equal(tri, N(hits["triangle"]))
    assert (depth[~hit] == 0).all() and (trans[~hit] == 1).all() and (trans[hit] == 0).all() and (tri[~hit] == -1).all()
    nrm, col = N(img["normal"]).reshape(-1, 3), N(img["color"]).reshape(-1, 3)
    assert (nrm[~hit] == 0).all() and (col[~hit] == 0.25).all()
    assert np.abs(np.linalg.norm(nrm[hit], axis=1) - 1.0).max() < 1e-5 and ((nrm[hit] * N(rd)[hit]).sum(axis=1) <= 0).all()
    # geometric normals of a sphere about the origin point along the hit point; colours are the barycentric mix of the corners'
    p = rc.hit_points(sphere["v"], sphere["t"], tuple(N(hits[k]) for k in KEYS))[hit]
    assert ((nrm[hit] * p).sum(axis=1) / np.linalg.norm(p, axis=1) > 0.99).all()
    c = N(colors)[sphere["t"][tri[hit]]].astype(np.float64)
    b1, b2 = N(hits["b1"])[hit, None].astype(np.float64), N(hits["b2"])[hit, None].astype(np.float64)
    assert np.abs(col[hit] - (c[:, 0] + b1 * (c[:, 1] - c[:, 0]) + b2 * (c[:, 2] - c[:, 0]))).max() < 1e-5
    # vertex normals: the sphere's own, interpolated and normalised
    vn = T(sphere["v"] / np.linalg.norm(sphere["v"], axis=1, keepdims=True), dev)
    smooth = N(render.render_image_mesh(W, H, cam, vd, td, ["normal"], normals=vn)["normal"]).reshape(-1, 3)
    assert np.abs(np.linalg.norm(smooth[hit], axis=1) - 1.0).max() < 1e-5 and ((smooth[hit] * p).sum(axis=1) / np.linalg.norm(p, axis=1) > 0.995).all()
    # a slab of the pixel index, brute force, int64 triangles, downsampling
    lo, hi = 301, 777
    slab = render.render_image_mesh(W, H, cam, vd, td.long(), targets, colors=colors, background=0.25, pixel_range=(lo, hi), method="brute")
    for k in targets:
        full = img[k].reshape(W * H, -1)[lo:hi]
        assert torch.equal(slab[k].reshape(hi - lo, -1), full), k
    half = render.render_image_mesh(W, H, cam, vd, td, ["depth"], downsampling=2)["depth"]
    assert half.shape == (H // 2, W // 2) and torch.equal(half, img["depth"][::2, ::2][:H // 2, :W // 2])


def test_python_layer_refusals(dev, sphere, view):
    import neddf_amd
    from neddf_amd import NeddfError
    from neddf_amd.fixtures import BUNNY_SMOKE_CFG
    from neddf_amd.raycast import build_grid, cast_rays
    render, cam = view
    vd, td = sphere["vd"], sphere["td"]
    with pytest.raises(ValueError, match="colors"):
        render.render_image_mesh(W, H, cam, vd, td, ["color"])
    with pytest.raises(ValueError, match="unknown"):
        render.render_image_mesh(W, H, cam, vd, td, ["steps"])
    ndc = neddf_amd.NeRFRender(dict(BUNNY_SMOKE_CFG, _target_="neddf.network.NeDDF"), use_coarse_network=False, ray_space="ndc").to(dev)
    with pytest.raises(NotImplementedError):
        ndc.render_image_mesh(W, H, cam, vd, td, ["depth"])
    o = vd[:4].contiguous()
    for bad in (lambda: cast_rays(o.cpu(), o, vd, td), lambda: cast_rays(o, o, vd.cpu(), td), lambda: cast_rays(o, o, vd, td.cpu()),
                lambda: cast_rays(o.double(), o, vd, td), lambda: cast_rays(o, o[:3], vd, td), lambda: cast_rays(o, o, vd, td.float()),
                lambda: cast_rays(o, o, vd, td[:, :2]), lambda: cast_rays(o, o, vd, td, method="bvh"), lambda: cast_rays(o, o, vd, td, pad=-1.0),
                lambda: cast_rays(o, o, vd, td[:5], grid=build_grid(vd, td)), lambda: build_grid(vd, td, cells=(0, 1, 1)),
                lambda: build_grid(vd, td, box=((0, 0, 0), (1, 1))), lambda: build_grid(vd, td, pad=float("nan"))):
        with pytest.raises(NeddfError):
            bad()


# ---------------------------------------------------------------------------------------------------------------- the bunny, end to end
def test_bunny_mesh_views_and_the_script(dev, tmp_path, capsys):
    import yaml
    from neddf_amd.fixtures import BUNNY_SMOKE_CFG, bunny_smoke_weights
    from neddf_amd.scripts import extract_mesh, render_mesh
    from neddf_amd.scripts.run_eval import load_config, load_trainer
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
    trainer = load_trainer(load_config(run), run, 7)
    render = trainer.neural_render
    render.set_iter(-1)
    net = render.get_network()
    dense = net.extract_mesh(threshold=0.1, resolution=24)
    sparse = net.extract_mesh(threshold=0.1, resolution=24, brick=8)
    assert dense[1].shape[0] > 4000           # (4 784 triangles on the MI355X)
    cam = trainer.cameras[0]
    cam.update_transform()
    targets = ["depth", "transmittance", "triangle", "normal"]
    grid = render.render_image_mesh(64, 64, cam, dense[0], dense[1], targets, method="grid")
    brute = render.render_image_mesh(64, 64, cam, dense[0], dense[1], targets, method="brute")
    brick = render.render_image_mesh(64, 64, cam, sparse[0], sparse[1], targets, method="grid")
    n_hit = int((grid["triangle"] >= 0).sum())
    print("bunny 24 / 0.1: %d triangles, %d of 4096 pixels hit" % (dense[1].shape[0], n_hit))
    assert n_hit >= 1
    for k in targets:
        assert torch.equal(grid[k], brute[k]) and torch.equal(grid[k], brick[k]), k
    # the script: extract with normals and colours, render every test view, compare with the traced view of the same level set
    path = extract_mesh.main([str(run), "--epoch", "7", "--resolution", "24", "--threshold", "0.1", "--normals", "--colors"])
    capsys.readouterr()
    rows = render_mesh.main([str(run), "--epoch", "7", "--compare-trace"])
    out = capsys.readouterr().out
    assert str(path) in out and len(rows) == len(trainer.dataset) == 2
    for i, row in enumerate(rows):
        for kind in ("depth", "normal", "rgb"):
            assert (run / "render" / ("%03d_%s_mesh.png" % (i, kind))).is_file()
        assert 0.0 <= row["hit_share"] <= 1.0 and abs(row["both"] + row["mesh_only"] - row["hit_share"]) < 1e-6
        assert "mesh camera %d: hit share " % i in out and "mesh against trace, camera %d: both " % i in out
    print(out)
    # a mesh without colours: no rgb image; brute force writes the same depth image
    plain = extract_mesh.main([str(run), "--epoch", "7", "--resolution", "24", "--threshold", "0.1"])
    before = open(run / "render" / "000_depth_mesh.png", "rb").read()
    os.remove(run / "render" / "000_rgb_mesh.png")
    rows2 = render_mesh.main([str(run), "--epoch", "7", "--mesh", str(plain), "--method", "brute"])
    assert not (run / "render" / "000_rgb_mesh.png").exists() and open(run / "render" / "000_depth_mesh.png", "rb").read() == before
    assert [r["hit_share"] for r in rows2] == [r["hit_share"] for r in rows] and "both" not in rows2[0]
