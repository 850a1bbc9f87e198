"""Rays through the BVH on the GPU: the kernel against the numpy restatement (tests/bvh_raycast_check.py) bit for bit with its leaf
counts, against the brute kernel bit for bit on the inputs chosen to break it, the any-hit mode against `triangle >= 0`, the C ABI's
refusals, ambient occlusion against its composition in numpy, and the Python layer end to end: render_image_mesh through the tree and
in tiles against the present call, and the script."""
import os

import numpy as np
import pytest
import torch
from conftest import GOLDEN

import bvh_check as bc
import bvh_raycast_check as brc
import geometry_check as gc
import raycast_check as rc
from test_gpu_raycast import N, T, _look_at, _quad_mesh, _soup_mesh, _special_rays, bits, same_bits

pytestmark = pytest.mark.gpu

F = np.float32
PAD = 2.0 ** -10
SPHERE_PAD = 2.0 ** -12 * np.sqrt(3.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def both(dev, o, d, vd, td, tree, **kw):
    """(cast_rays' dict with visits, occluded bool, its visits), all numpy."""
    from neddf_amd import bvh
    od, dd = T(o, dev), T(d, dev)
    hits = {k: N(a) for k, a in bvh.cast_rays(od, dd, vd, td, bvh=tree, return_visits=True, **kw).items()}
    occ, occ_visits = bvh.occluded(od, dd, vd, td, bvh=tree, return_visits=True, **kw)
    assert occ.dtype == torch.bool and hits["visits"].dtype == np.int32
    return hits, N(occ), N(occ_visits)


def brute(dev, o, d, vd, td, **kw):
    from neddf_amd.raycast import cast_rays
    return cast_rays(T(o, dev), T(d, dev), vd, td, method="brute", **kw)


# ---------------------------------------------------------------------------------------------------------------- kernel == restatement
@pytest.mark.parametrize("n_tri", [0, 1, 2, 3, 64, 65, 300, 1025])
def test_kernel_equals_the_restatement_and_brute(dev, n_tri):
    from neddf_amd.bvh import build_bvh
    v, t = _soup_mesh(n_tri) if n_tri else (rc.soup(4)[0], np.zeros((0, 3), np.int32))
    # 1 024 distinct rays, then three shuffles of them: 4 096 rays -- 64 waves -- whose restatement costs a quarter (a ray's result depends
    # on nothing but the ray; the shuffles put it into other lanes and waves)
    o, d = rc.soup_rays(*rc.soup(n_tri if n_tri else 16, 11), 1024)
    so, sd = _special_rays()
    o[8:8 + len(so)], d[8:8 + len(so)] = so, sd                     # non-finite rays, zero directions, axis rays, rays from inside
    index = np.concatenate([np.arange(1024)] + [np.random.default_rng(k).permutation(1024) for k in (71, 72, 73)])
    vd, td = T(v, dev), T(t, dev)
    tree = build_bvh(vd, td)
    want = tuple(x[index] for x in brc.cast_rays_bvh(o, d, v, t, pad=PAD)[:5])
    want_occ, want_occ_visits = (x[index] for x in brc.occluded_bvh(o, d, v, t, pad=PAD))
    o, d = o[index], d[index]
    assert n_tri == 0 or brc.walks(o[:8], bc.build(v, t), PAD).all()
    for n_rays in (0, 1, 63, 64, 65, 4096):
        runs = [both(dev, o[:n_rays], d[:n_rays], vd, td, tree, pad=PAD) for _ in range(2)]
        hits, occ, occ_visits = runs[0]
        same_bits(hits, tuple(x[:n_rays] for x in want[:4]), ("bvh == restatement", n_tri, n_rays))
        assert np.array_equal(hits["visits"], want[4][:n_rays]), (n_tri, n_rays, hits["visits"][:8], want[4][:8])
        same_bits(hits, brute(dev, o[:n_rays], d[:n_rays], vd, td, pad=PAD), ("bvh == brute", n_tri, n_rays))
        assert np.array_equal(occ, want_occ[:n_rays]) and np.array_equal(occ, hits["triangle"] >= 0)
        assert np.array_equal(occ_visits, want_occ_visits[:n_rays])
        same_bits(runs[1][0], hits, ("again", n_tri, n_rays))
        assert np.array_equal(runs[1][0]["visits"], hits["visits"]) and np.array_equal(runs[1][1], occ) and np.array_equal(runs[1][2], occ_visits)
    if n_tri >= 64:
        assert (hits["triangle"] >= 0).mean() > 0.9 and hits["visits"].mean() < 0.25 * n_tri
    if n_tri > 8:
        assert not np.isin(hits["triangle"], [1, 2, 5, 6, n_tri - 1]).any()          # degenerate, invalid, and the duplicate loses to triangle 3


# ---------------------------------------------------------------------------------------------------------------- bvh == brute
def _lattice_rays():
    """Rays at the vertices, the edge midpoints and the quad centres (on the diagonals) of the 16 x 16 lattice, from both sides: the
    neighbours of a shared edge or vertex tie, and the lowest index must win."""
    x = np.linspace(-1.0, 1.0, 33)
    target = np.stack([np.tile(x, 33), np.repeat(x, 33), np.zeros(33 * 33)], axis=1)
    eyes = np.array([[0.3, -0.2, 2.5], [-1.4, 0.9, -2.0], [0.0, 0.0, 3.0]])
    o = np.concatenate([np.broadcast_to(e, target.shape) for e in eyes])
    d = np.concatenate([target - e for e in eyes])
    # straight down at lattice points: the edge functions are exact zeros
    o = np.concatenate([o, target + [0.0, 0.0, 1.0]])
    d = np.concatenate([d, np.broadcast_to([0.0, 0.0, -1.0], target.shape)])
    return o.astype(F), d.astype(F)


def _awkward(name):
    """(vertices, triangles, origins, dirs, keywords of the casts)"""
    rng = np.random.default_rng(51)
    if name == "invalid and duplicated":
        v, t = _soup_mesh(300)
        v = np.concatenate([v, [[np.inf, 0.0, 0.0]]]).astype(F)
        t = t.copy()
        t[40:60:3, 2] = len(v) - 1
        t[100:110] = t[90:100]
        o, d = rc.soup_rays(*rc.soup(300, 11), 2048)
        return v, t, o, d, dict(pad=PAD)
    if name == "lattice":
        v, t = _quad_mesh()
        o, d = _lattice_rays()
        return v, t, o, d, {}
    if name == "300 copies":
        v = np.array([[-0.5, -0.4, 0.1], [0.6, -0.3, 0.0], [0.0, 0.7, -0.1]], F)
        t = np.tile(np.array([[0, 1, 2]], np.int32), (300, 1))
        o, d = rc.soup_rays(v, t, 512)
        return v, t, o, d, {}
    if name == "size 2^-8 at offset 1000":
        v, t = gc.uv_sphere(2.0 ** -9, 12, 24)
        v = (v.astype(np.float64) + 1000.0).astype(F)
        target = 1000.0 + rng.uniform(-2.0 ** -10, 2.0 ** -10, (1024, 3))
        o = 1000.0 + rng.standard_normal((1024, 3)) * 0.05
        return v, t, o.astype(F), (target - o).astype(F), {}
    v, t = gc.uv_sphere(*rc.SPHERE)
    if name == "bad rays":
        o, d = _special_rays()
        return v, t, o, d, dict(pad=SPHERE_PAD)
    o, d = rc.fan_rays()
    o, d = o[::8], d[::8]
    if name == "t_min above t_max":
        return v, t, o, d, dict(pad=SPHERE_PAD, t_min=2.0, t_max=1.0)
    if name == "from inside":
        o = rng.uniform(-0.25, 0.25, (2048, 3)).astype(F)
        d = rng.standard_normal((2048, 3)).astype(F)
        d[::5, 0], d[::7, 1] = 0.0, -0.0
        return v, t, o, d, dict(pad=SPHERE_PAD)
    if name == "far origins":
        target = rng.uniform(-0.25, 0.25, (256, 3))
        o = rng.standard_normal((256, 3))
        o *= np.repeat([3.0, 300.0, 3e4, 3e6], 64)[:, None] / np.linalg.norm(o, axis=1, keepdims=True)
        return v, t, o.astype(F), (target - o).astype(F), dict(pad=SPHERE_PAD)
    assert name == "pad 0"
    return v, t, o, d, dict(pad=0.0)


AWKWARD = ["invalid and duplicated", "lattice", "300 copies", "size 2^-8 at offset 1000", "bad rays", "t_min above t_max", "from inside",
           "far origins", "pad 0"]


@pytest.mark.parametrize("name", AWKWARD)
def test_bvh_equals_brute_on_awkward_cases(dev, name):
    from neddf_amd.bvh import build_bvh
    from neddf_amd.raycast import _bounds, default_pad
    v, t, o, d, kw = _awkward(name)
    vd, td = T(v, dev), T(t, dev)
    tree = build_bvh(vd, td)
    hits, occ, occ_visits = both(dev, o, d, vd, td, tree, **kw)
    pad = kw.get("pad", default_pad(*_bounds(vd)))
    want = brute(dev, o, d, vd, td, **dict(kw, pad=pad))
    same_bits(hits, want, name)
    tri, visits = hits["triangle"], hits["visits"]
    assert np.array_equal(occ, tri >= 0), name
    assert (occ_visits <= visits).all()
    valid = int(rc._valid_triangles(v, t)[1].sum())
    walk = brc.walks(o, bc.build(v, t), pad)
    ok = brc._ray_ok(o, d)
    assert (visits[ok & ~walk] == valid).all() and (visits[~ok] == 0).all() and (occ_visits[~ok] == 0).all()
    if name == "lattice":               # every lattice point is hit, and shared edges and vertices go to the lowest index
        down = slice(3 * 33 * 33, None)                                          # straight down at lattice points: exact arithmetic
        # (a slanted ray at a point of the lattice's rim may pass it by a rounding: the brute kernel decides, above)
        assert (tri[down] >= 0).all() and (tri >= 0).mean() > 0.9 and walk.all() and visits.mean() < 0.05 * len(t)
        corners = v[np.asarray(t)][:, :, :2].astype(np.float64)                  # [T, 3, 2]; coordinates are multiples of 2^-4
        q = o[down][:, None, None, :2].astype(np.float64)
        e = np.roll(corners, -1, axis=1) - corners
        side = e[None, :, :, 0] * (q[..., 1] - corners[None, :, :, 1]) - e[None, :, :, 1] * (q[..., 0] - corners[None, :, :, 0])
        holds = (side >= 0).all(axis=2) | (side <= 0).all(axis=2)                # [n, T]: the closed triangles that hold the point
        assert (holds.sum(axis=1) >= 1).all() and (holds.sum(axis=1) >= 2).mean() > 0.7
        assert np.array_equal(tri[down], np.argmax(holds, axis=1)) and (hits["t"][down] == 1.0).all()
    elif name == "300 copies":
        assert walk.all() and (tri[tri >= 0] == 0).all() and (tri >= 0).mean() > 0.9 and (visits[tri >= 0] == 300).all()
    elif name == "size 2^-8 at offset 1000":
        assert walk.all() and (tri >= 0).any()
    elif name == "bad rays":
        assert np.isnan(hits["t"][:4]).all() and (tri[:4] == -1).all() and not ok[:4].any() and (tri[4:] >= 0).any()
    elif name == "t_min above t_max":
        assert (tri == -1).all() and (visits == 0).all() and not occ.any()
    elif name == "from inside":
        assert (tri >= 0).all() and walk.all() and visits.mean() < 0.02 * len(t)
    elif name == "far origins":
        assert walk[:128].all() and not walk[192:].any() and (tri[:64] >= 0).all()
    elif name == "pad 0":
        assert not walk.any() and (tri >= 0).any()


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_c_abi_refusals(dev):
    from neddf_amd import Context
    from neddf_amd._lib import _ptr
    from neddf_amd.bvh import build_bvh
    v, t = gc.uv_sphere(0.5, 6, 12)
    vd, td, od = T(v, dev), T(t, dev), T(v[:7] * 3, dev)
    dd = -od
    tree = build_bvh(vd, td)
    ctx = Context.get(dev)
    lib = ctx.lib
    n_v, n_t = vd.shape[0], td.shape[0]
    hit = [torch.zeros(7, device=dev), torch.zeros(7, device=dev, dtype=torch.int32), torch.zeros(7, device=dev), torch.zeros(7, device=dev)]
    occ, visits = torch.zeros(7, device=dev, dtype=torch.uint8), torch.zeros(7, device=dev, dtype=torch.int32)
    for fn, name, outs in ((lib.neddf_raycast_bvh_query, "raycast_bvh_query", [_ptr(x) for x in hit]),
                           (lib.neddf_raycast_bvh_occluded, "raycast_bvh_occluded", [_ptr(occ)])):
        def call(**kw):
            a = dict(ctx=ctx.h, o=_ptr(od), d=_ptr(dd), R=7, v=_ptr(vd), V=n_v, t=_ptr(td), T=n_t, leaf=_ptr(tree.leaf_triangle),
                     children=_ptr(tree.children), boxes=_ptr(tree.boxes), L=n_t, t_min=0.0, t_max=10.0, pad=1e-3, outs=outs, visits=_ptr(visits))
            a.update(kw)
            rc_ = fn(a["ctx"], a["o"], a["d"], a["R"], a["v"], a["V"], a["t"], a["T"], a["leaf"], a["children"], a["boxes"], a["L"], a["t_min"],
                     a["t_max"], a["pad"], *a["outs"], a["visits"], None)
            return rc_, lib.neddf_last_error(ctx.h).decode()
        assert fn(None, _ptr(od), _ptr(dd), 7, _ptr(vd), n_v, _ptr(td), n_t, _ptr(tree.leaf_triangle), _ptr(tree.children), _ptr(tree.boxes), n_t,
                  0.0, 10.0, 1e-3, *outs, None, None) == -1
        for kw in (dict(R=-1), dict(V=-2), dict(T=-1, L=-1)):
            assert call(**kw) == (-1, name + ": negative count")
        for kw in (dict(o=None), dict(d=None), dict(v=None), dict(t=None)):
            assert call(**kw) == (-1, name + ": NULL rays, vertices or triangles")
        for kw in (dict(R=2 ** 31), dict(V=2 ** 31), dict(T=2 ** 31, L=2 ** 31)):
            assert call(**kw) == (-3, name + ": 2^31 rays, triangles or vertices or more (indices are int32)")
        for kw in (dict(L=n_t - 1), dict(L=n_t + 1), dict(L=0)):
            assert call(**kw) == (-1, name + ": the tree's leaves are not this mesh's triangles (n_leaves != n_triangles)")
        for kw in (dict(leaf=None), dict(children=None), dict(boxes=None)):
            assert call(**kw) == (-1, name + ": NULL leaf_triangle, children or boxes")
        for pad in (-1e-3, float("nan"), float("inf")):
            assert call(pad=pad) == (-1, name + ": pad must be finite and not negative")
        assert call(outs=[None] * len(outs)) == (-1, name + ": NULL outputs")
        if len(outs) == 4:
            assert call(outs=outs[:2] + [None] + outs[3:]) == (-1, name + ": NULL outputs")
        # legal: no visits, no rays (and then no ray or output arrays), no triangles (and then no tree), one triangle without children
        assert call(visits=None)[0] == 0 and call(R=0, o=None, d=None, outs=[None] * len(outs), visits=None)[0] == 0
        assert call(T=0, L=0, t=None, leaf=None, children=None, boxes=None)[0] == 0
        one = build_bvh(vd, td[:1].contiguous())
        assert one.children.numel() == 0
        assert call(T=1, L=1, leaf=_ptr(one.leaf_triangle), children=None, boxes=_ptr(one.boxes))[0] == 0
        assert call()[0] == 0
    torch.cuda.synchronize()
    assert (N(hit[1]) >= 0).all() and N(occ).all() and (N(visits) >= 1).all()            # rays from outside at the centre of the sphere


# ---------------------------------------------------------------------------------------------------------------- ambient occlusion
def _ao_scene():
    """A floor (z = 0), a wall (x = 1, 0 <= z <= 2) and a closed cube that floats above the floor: 16 triangles; 64 points with
    axis-aligned normals (so that d . n is a component of d, exact in any arithmetic)."""
    quad = lambda a, b, c, e: [a, b, c, e]
    vs, ts = [], []

    def add(corners):
        k = len(vs)
        vs.extend(corners)
        ts.extend([[k, k + 1, k + 2], [k, k + 2, k + 3]])
    add(quad([-4, -4, 0], [4, -4, 0], [4, 4, 0], [-4, 4, 0]))
    add(quad([1, -4, 0], [1, 4, 0], [1, 4, 2], [1, -4, 2]))
    c, h = np.array([-2.5, 0.0, 1.0]), 0.5
    for a in range(3):
        for s in (-1.0, 1.0):
            u, w = np.eye(3)[(a + 1) % 3], np.eye(3)[(a + 2) % 3]
            m = c + s * h * np.eye(3)[a]
            add([m - h * u - h * w, m + h * u - h * w, m + h * u + h * w, m - h * u + h * w])
    v, t = np.array(vs, F), np.array(ts, np.int32)
    assert len(t) == 16
    rng = np.random.default_rng(61)
    up = [0.0, 0.0, 1.0]
    near = np.stack([rng.uniform(0.05, 0.9, 24), rng.uniform(-2, 2, 24), np.zeros(24)], axis=1)          # floor next to the wall
    open_ = np.stack([rng.uniform(2.5, 3.5, 16), rng.uniform(-2, 2, 16), np.zeros(16)], axis=1)           # open floor, 1.5 from the wall
    wall = np.stack([np.ones(8), rng.uniform(-2, 2, 8), rng.uniform(0.1, 1.8, 8)], axis=1)                # on the wall, facing either way
    inside = c + rng.uniform(-0.3, 0.3, (16, 3))
    p = np.concatenate([near, open_, wall, inside]).astype(F)
    n = np.array([up] * 40 + [[1.0, 0, 0]] * 4 + [[-1.0, 0, 0]] * 4 + [up] * 8 + [[0, -1.0, 0]] * 8, F)
    return v, t, p, n, dict(near=slice(0, 24), open=slice(24, 40), wall=slice(40, 48), inside=slice(48, 64))


def _ao_composition(v, t, p, n, n_dirs, radius, bias, pad):
    """The brute composition in numpy: (occluded bool [P, K], ao float64 [P])."""
    k = np.arange(n_dirs, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / n_dirs
    r = np.sqrt(1.0 - z * z)
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    dirs = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1).astype(F)
    dot = (n[:, None, :].astype(np.float64) * dirs[None].astype(np.float64)).sum(axis=2)                # exact: n is an axis
    d = np.where((dot < 0)[:, :, None], -dirs[None], dirs[None]).astype(F)
    o = (p + (F(bias) * n).astype(F)).astype(F)
    o = np.broadcast_to(o[:, None, :], d.shape)
    hit = rc.cast_rays(o.reshape(-1, 3), d.reshape(-1, 3), v, t, t_min=0.0, t_max=radius, pad=pad)[1] >= 0
    occ = hit.reshape(len(p), n_dirs)
    w = np.abs(dot)
    return occ, (w * ~occ).sum(axis=1) / w.sum(axis=1)


def test_ambient_occlusion(dev):
    from neddf_amd import bvh
    from neddf_amd.raycast import default_pad
    v, t, p, n, part = _ao_scene()
    vd, td, pd, nd = T(v, dev), T(t, dev), T(p, dev), T(n, dev)
    tree = bvh.build_bvh(vd, td)
    lo, hi = v.min(axis=0).astype(np.float64).tolist(), v.max(axis=0).astype(np.float64).tolist()
    pad = default_pad(lo, hi)
    diag = float(np.sqrt(((np.array(hi) - np.array(lo)) ** 2).sum()))
    for radius in (None, 0.5, 2.0):
        r = diag if radius is None else radius
        want_occ, want = _ao_composition(v, t, p, n, 16, r, 4.0 * pad, pad)
        got = bvh.ambient_occlusion(pd, nd, vd, td, n_dirs=16, radius=radius, bvh=tree)
        assert got.dtype == torch.float32 and got.shape == (64,)
        got = N(got)
        # the occlusion bits: the rays of the composition through occluded()
        dirs = bvh.fibonacci_directions(16)
        d = np.where(((n[:, None, :] * dirs[None]).sum(axis=2) < 0)[:, :, None], -dirs[None], dirs[None]).astype(F)
        o = np.broadcast_to((p + (F(4.0 * pad) * n).astype(F)).astype(F)[:, None, :], d.shape)
        occ = N(bvh.occluded(T(o.reshape(-1, 3), dev), T(d.reshape(-1, 3), dev), vd, td, t_min=0.0, t_max=r, bvh=tree, pad=pad)).reshape(64, 16)
        assert np.array_equal(occ, want_occ), radius
        print("radius %s: ao near the wall %.3f, on the wall %.3f, largest difference %.2e" % (radius, got[part["near"]].mean(), got[part["wall"]].mean(), np.abs(got - want).max()))
        assert np.abs(got - want).max() <= 1e-5 and (got >= 0).all() and (got <= 1).all()
        assert (got[part["inside"]] == 0.0).all() if r >= 2.0 else True            # the cube's diagonal is sqrt 3
        if radius == 0.5:
            assert (got[part["open"]] == 1.0).all()
        if radius is None:
            assert (got[part["near"]] < 1.0).all() and (got[part["near"]] > 0.0).all() and (got[part["wall"]] < 1.0).all()
    # every weight 0 -- the single direction of K = 1 is the x axis, the normal is along y -- gives 1
    assert bvh.fibonacci_directions(1).tolist() == [[1.0, 0.0, 0.0]]
    one = bvh.ambient_occlusion(pd[:4], T(np.tile(np.array([[0.0, 1.0, 0.0]], F), (4, 1)), dev), vd, td, n_dirs=1, bvh=tree)
    assert (N(one) == 1.0).all()


# ---------------------------------------------------------------------------------------------------------------- the Python layer
@pytest.fixture(scope="module")
def render_and_camera(dev):
    import neddf_amd
    from neddf_amd.fixtures import BUNNY_SMOKE_CFG, bunny_smoke_weights
    render = neddf_amd.NeRFRender(dict(BUNNY_SMOKE_CFG, _target_="neddf.network.NeDDF"), sample_coarse=16, sample_fine=32, dist_near=2.0,
                                  dist_far=6.0, max_dist=6.0, use_coarse_network=False, sampling_type="cone").to(dev)
    net = neddf_amd.NeDDF(**BUNNY_SMOKE_CFG)
    net.load_state_dict({k: torch.from_numpy(a) for k, a in bunny_smoke_weights().items()})
    net.to(dev)
    net.set_iter(-1)

    def camera(w, h):
        R, Tr = _look_at(np.array([1.9, -2.2, 1.1]), np.zeros(3))
        cam = neddf_amd.Camera(neddf_amd.PinholeCalib(np.array([1.6 * w, 1.6 * w, w / 2.0, h / 2.0])), None).to(dev)
        cam.R, cam.T = torch.from_numpy(R).to(dev), torch.from_numpy(Tr).to(dev)
        return cam
    return render, camera, net


@pytest.mark.parametrize("mesh", ["sphere", "bunny"])
def test_mesh_views_through_the_tree_and_in_tiles(dev, render_and_camera, mesh):
    from neddf_amd.bvh import build_bvh
    render, camera, net = render_and_camera
    if mesh == "sphere":
        v, t = gc.uv_sphere(*rc.SPHERE)
        vd, td = T(v, dev), T(t, dev)
    else:
        vd, td = net.extract_mesh(threshold=0.1, resolution=24)
        assert td.shape[0] > 4000
    colors = T(np.random.default_rng(8).random(tuple(vd.shape)).astype(F), dev)
    targets = ["depth", "transmittance", "triangle", "normal", "color"]
    tree = build_bvh(vd, td)
    for w, h in ((64, 64), (50, 37)):
        cam = camera(w, h)
        kw = dict(colors=colors, background=0.25)
        present = render.render_image_mesh(w, h, cam, vd, td, targets, **kw)
        n_hit = int((present["triangle"] >= 0).sum())
        assert (0.02 * w * h if mesh == "sphere" else 1) <= n_hit < 0.9 * w * h, (mesh, n_hit)
        views = {"defaults spelled out": dict(method="grid", grid=None, bvh=None, tile=0), "bvh=True": dict(bvh=True), "a MeshBVH": dict(bvh=tree),
                 "grid in tiles": dict(tile=8), "brute": dict(method="brute"), "brute in tiles": dict(method="brute", tile=8),
                 "tree in tiles": dict(bvh=tree, tile=8)}
        for name, extra in views.items():
            got = render.render_image_mesh(w, h, cam, vd, td, targets, **kw, **extra)
            for k in targets:
                assert got[k].dtype == present[k].dtype and got[k].shape == present[k].shape, (mesh, name, k)
                assert np.array_equal(bits(N(got[k])), bits(N(present[k]))), (mesh, w, h, name, k)
        # the shaded look: 1 where nothing is hit, inside [0, 1], below 1 somewhere on a closed surface seen at a slant; the same in tiles
        ao = render.render_image_mesh(w, h, cam, vd, td, ["ambient_occlusion", "transmittance"], bvh=tree, ao_dirs=8)
        a, miss = N(ao["ambient_occlusion"]), N(ao["transmittance"]) == 1
        assert a.shape == (h, w) and a.dtype == np.float32 and (a[miss] == 1.0).all() and (a >= 0).all() and (a <= 1).all()
        tiled = render.render_image_mesh(w, h, cam, vd, td, ["ambient_occlusion"], bvh=True, tile=8, ao_dirs=8)["ambient_occlusion"]
        assert np.array_equal(bits(N(tiled)), bits(a))
        if mesh == "bunny":
            assert (a[~miss] < 1.0).any()
        print("%s %d x %d: %d pixels hit, mean ambient occlusion on them %.3f" % (mesh, w, h, n_hit, a[~miss].mean()))


def test_render_mesh_script_with_the_tree(dev, tmp_path, capsys):
    import yaml
    from neddf_amd.fixtures import BUNNY_SMOKE_CFG, bunny_smoke_weights
    from neddf_amd.scripts import extract_mesh, render_mesh
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
    extract_mesh.main([str(run), "--epoch", "7", "--resolution", "24", "--threshold", "0.1", "--normals"])
    capsys.readouterr()
    plain = render_mesh.main([str(run), "--epoch", "7"])
    depth = [open(run / "render" / ("%03d_depth_mesh.png" % i), "rb").read() for i in range(len(plain))]
    normal = [open(run / "render" / ("%03d_normal_mesh.png" % i), "rb").read() for i in range(len(plain))]
    assert not (run / "render" / "000_ao_mesh.png").exists()
    rows = render_mesh.main([str(run), "--epoch", "7", "--bvh", "--tiles", "--ao"])
    assert len(rows) == len(plain) == 2 and [r["hit_share"] for r in rows] == [r["hit_share"] for r in plain]
    for i in range(len(rows)):
        assert open(run / "render" / ("%03d_depth_mesh.png" % i), "rb").read() == depth[i]
        assert open(run / "render" / ("%03d_normal_mesh.png" % i), "rb").read() == normal[i]
        assert (run / "render" / ("%03d_ao_mesh.png" % i)).stat().st_size > 100
    with pytest.raises(SystemExit):
        render_mesh.main([str(run), "--epoch", "7", "--bvh", "--method", "brute"])
