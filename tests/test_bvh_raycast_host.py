"""Rays through the BVH, the part that needs no GPU: the declarations of the two entry points, the numpy restatement of the traversal
(tests/bvh_raycast_check.py) against the brute restatement (tests/raycast_check.py) bit for bit, how many leaves it evaluates, the rays
that do not walk, and the Python layer's exports, refusals and flags."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch
from conftest import ROOT

import bvh_check as bc
import bvh_raycast_check as brc
import geometry_check as gc
import raycast_check as rc

NEW = ("neddf_raycast_bvh_query", "neddf_raycast_bvh_occluded")
SPHERE_PAD = 2.0 ** -12 * np.sqrt(3.0)
SOUP_PAD = 2.0 ** -10


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same_bits(got, want, what):
    for k, g, w in zip(("t", "triangle", "b1", "b2"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        bad = np.flatnonzero(bits(g) != bits(w))
        assert bad.size == 0, (what, k, bad.size, bad[:5], g[bad[:5]], w[bad[:5]])


# ---------------------------------------------------------------------------------------------------------------- declarations
def test_entry_points_are_declared_bound_and_exported():
    from neddf_amd import _lib
    text = open(os.path.join(ROOT, "include", "neddf_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(neddf_[a-z_]+)\s*\(", hdr))
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    so = os.path.join(ROOT, "neddf_amd", "csrc", "libneddf_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T"}
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in bound and name in exported, name
        call = [a(0) if a in (C.c_int, C.c_int64) else a(0.0) if a in (C.c_float, C.c_double) else None for a in bound[name]]
        assert getattr(lib, name)(*call) == -1, name                    # a NULL context
    assert "#define NEDDF_ABI_VERSION 7" in hdr and _lib.ABI_VERSION == 7 and lib.neddf_abi_version() == 7
    assert "is not built" not in text and "not built" not in open(os.path.join(ROOT, "neddf_amd", "bvh.py")).read()


# ---------------------------------------------------------------------------------------------------------------- restatement == brute
@pytest.fixture(scope="module")
def sphere():
    v, t = gc.uv_sphere(*rc.SPHERE)
    assert len(t) == 2208
    return v, t, bc.build(v, t)


def _centre_rays():
    """600 rays from the centre of the sphere: 300 with one or two zero direction components (of both signs of zero), 100 of the others
    with directions scaled by 1e-3."""
    rng = np.random.default_rng(41)
    d = rng.standard_normal((600, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d.astype(np.float32)
    for i in range(300):
        axes = [(i % 3,), ((i + 1) % 3,), (i % 3, (i + 1) % 3)][(i // 3) % 3]
        for a in axes:
            d[i, a] = np.float32(-0.0) if i % 2 else np.float32(0.0)
    d[300:400] *= np.float32(1e-3)
    assert ((d[:300] == 0).sum(axis=1) >= 1).all() and ((d == 0).sum(axis=1) <= 2).all()
    return np.zeros((600, 3), np.float32), d


def _sets(sphere):
    v, t, tree = sphere
    fo, fd = rc.fan_rays()
    ao, ad, _ = rc.aimed_rays(v, t)
    pick = np.random.default_rng(40).permutation(len(ao))[:3000]
    co, cd = _centre_rays()
    sv, st = rc.soup(300)
    so, sd = rc.soup_rays(sv, st, 2000)
    stree = bc.build(sv, st)
    # name, rays, mesh, tree, pad, range, the cap on the mean of the leaves evaluated as a share of the triangles
    return [("sphere fan", fo[::8][:3000], fd[::8][:3000], v, t, tree, SPHERE_PAD, (0.0, np.inf), 0.01),
            ("sphere aimed", ao[pick], ad[pick], v, t, tree, SPHERE_PAD, (0.0, np.inf), 0.01),
            ("sphere aimed, range", ao[pick], ad[pick], v, t, tree, SPHERE_PAD, (1.0, 2.2), 0.01),
            ("sphere from the centre", co, cd, v, t, tree, SPHERE_PAD, (0.0, np.inf), 0.01),
            ("soup", so, sd, sv, st, stree, SOUP_PAD, (0.0, np.inf), 0.05)]


@pytest.mark.parametrize("index", range(5))
def test_restatement_equals_brute_and_prunes(sphere, index):
    name, o, d, v, t, tree, pad, (t_min, t_max), cap = _sets(sphere)[index]
    assert len(o) == (600 if "centre" in name else 2000 if name == "soup" else 3000)
    assert brc.walks(o, tree, pad).all()
    want = rc.cast_rays(o, d, v, t, t_min=t_min, t_max=t_max, pad=pad)
    got = brc.cast_rays_bvh(o, d, v, t, t_min=t_min, t_max=t_max, pad=pad, tree=tree)
    same_bits(got, want, name)
    visits, max_stack = got[4], got[5]
    print("%s: %d of %d rays hit; leaves evaluated mean %.2f max %d; stack %d, depth %d"
          % (name, (want[1] >= 0).sum(), len(o), visits.mean(), visits.max(), max_stack, tree["depth"]))
    assert (want[1] >= 0).any()
    assert visits.mean() < cap * len(t), (name, visits.mean())
    assert max_stack <= tree["depth"] + 1
    occluded, any_visits = brc.occluded_bvh(o, d, v, t, t_min=t_min, t_max=t_max, pad=pad, tree=tree)
    assert np.array_equal(occluded, want[1] >= 0), name
    assert (any_visits <= visits).all()                     # the two walks are one walk up to the first candidate, where any-hit stops


def test_rays_that_do_not_walk():
    v, t = gc.uv_sphere(0.5, 10, 20)                # (a coarser sphere: this route costs one restated pair per ray and triangle)
    tree = bc.build(v, t)
    o, d = rc.fan_rays()
    o, d = o[::64], d[::64]
    v2 = np.concatenate([v, [[np.nan, 0, 0]]]).astype(np.float32)               # three invalid triangles: they do not count
    t2 = t.copy()
    t2[5, 1], t2[77, 0], t2[300, 2] = len(v), -1, len(v2) - 1
    tree2 = bc.build(v2, t2)
    far = rc.soup_rays(v, t, 200, seed=5)
    far_o = (far[0].astype(np.float64) / 3.0 * 1e6).astype(np.float32)
    target = np.random.default_rng(6).uniform(-0.25, 0.25, (200, 3))
    far_d = (target - far_o).astype(np.float32)
    for name, oo, dd, pad in (("pad 0", o, d, 0.0), ("subnormal pad", o, d, 1e-40), ("far origins", far_o, far_d, SPHERE_PAD)):
        assert not brc.walks(oo, tree2, pad).any(), name
        got = brc.cast_rays_bvh(oo, dd, v2, t2, pad=pad, tree=tree2)
        want = brc.fallback(oo, dd, v2, t2, pad=pad)
        same_bits(got, want, name)
        same_bits(got, rc.cast_rays(oo, dd, v2, t2, pad=pad), name)
        assert (got[4] == len(t) - 3).all() and np.array_equal(got[4], want[4]) and got[5] == 0
        occluded, any_visits = brc.occluded_bvh(oo, dd, v2, t2, pad=pad, tree=tree2)
        assert np.array_equal(occluded, want[1] >= 0) and (any_visits[~occluded] == len(t) - 3).all()
        assert (want[1] >= 0).any()
    # the limit itself: W is the largest |coordinate| of the root box
    w = float(np.abs(tree["boxes"][0]).max())
    assert brc.walks(o, tree, 2.0 ** -16 * w).all() and not brc.walks(o, tree, np.nextafter(np.float32(2.0 ** -16 * w), np.float32(0))).any()
    edge = np.float32(2.0 ** 21 * SPHERE_PAD - 2.0 * (w + 2.0 * np.float32(SPHERE_PAD)))
    oo = np.array([[edge * 0.999, 0, 0], [0, -edge * 1.001, 0]], np.float32)
    assert brc.walks(oo, tree, SPHERE_PAD).tolist() == [True, False]
    # invalid rays: (NaN, -1, NaN, NaN) and no visit; an empty mesh and an empty ray set are legal
    bad_o = np.array([[np.nan, 0, 3], [0, 0, 3], [0, 0, 3]], np.float32)
    bad_d = np.array([[0, 0, -1], [0, 0, 0], [0, np.inf, -1]], np.float32)
    got = brc.cast_rays_bvh(bad_o, bad_d, v, t, pad=SPHERE_PAD, tree=tree)
    assert np.isnan(got[0]).all() and (got[1] == -1).all() and np.isnan(got[2]).all() and (got[4] == 0).all()
    none = brc.cast_rays_bvh(o, d, v, t[:0], pad=SPHERE_PAD)
    assert np.isinf(none[0]).all() and (none[1] == -1).all() and (none[4] == 0).all()
    assert len(brc.cast_rays_bvh(o[:0], d[:0], v, t, pad=SPHERE_PAD, tree=tree)[0]) == 0


# ---------------------------------------------------------------------------------------------------------------- the Python layer
def test_python_layer_without_a_device():
    import neddf_amd
    from neddf_amd import NeddfError, bvh
    from neddf_amd.bvh import MeshBVH, bvh_of
    for name in ("cast_rays", "occluded", "ambient_occlusion", "build_bvh", "MeshBVH"):
        assert callable(getattr(bvh, name)), name
    v = torch.zeros(6, 3)
    t = torch.zeros(4, 3, dtype=torch.int32)
    o = torch.zeros(5, 3)
    for bad in (lambda: bvh.cast_rays(o, o, v, t), lambda: bvh.occluded(o, o, v, t), lambda: bvh.ambient_occlusion(o, o, v, t),
                lambda: bvh.cast_rays(o.double(), o, v, t), lambda: bvh.cast_rays(o[:, :2], o, v, t), lambda: bvh.occluded(o, o[:3], v, t),
                lambda: bvh.cast_rays(np.zeros((5, 3), np.float32), o, v, t)):
        with pytest.raises(NeddfError):
            bad()
    # a tree of another mesh is refused, not followed
    tree = MeshBVH((0, 0, 0), (1, 1, 1), torch.zeros(4, dtype=torch.int32), torch.zeros(3, 2, dtype=torch.int32), torch.zeros(7, 6), 6, 4)
    assert bvh_of("x", v, t, tree) is tree
    for other in (MeshBVH((0, 0, 0), (1, 1, 1), tree.leaf_triangle, tree.children, tree.boxes, 6, 5),
                  MeshBVH((0, 0, 0), (1, 1, 1), tree.leaf_triangle, tree.children, tree.boxes, 7, 4),
                  MeshBVH((0, 0, 0), (1, 1, 1), tree.leaf_triangle[:3], tree.children, tree.boxes, 6, 4), "tree", True):
        with pytest.raises(NeddfError, match="MeshBVH"):
            bvh_of("x", v, t, other)
    # the refusal of raycast.cast_rays names the route
    from neddf_amd.raycast import cast_rays
    with pytest.raises(NeddfError):
        cast_rays(o, o, v, t, method="bvh")
    # render_image_mesh: refusals that come before the first device call
    render = neddf_amd.NeRFRender({"_target_": "neddf.network.NeDDF"}, use_coarse_network=False)
    assert "ambient_occlusion" in render.MESH_TARGETS
    for kw, match in ((dict(tile=4), "tile"), (dict(tile=-8), "tile"), (dict(tile=8, pixel_range=(0, 10)), "pixel_range"),
                      (dict(bvh=tree, grid=object()), "bvh"), (dict(bvh=True, method="brute"), "bvh"),
                      (dict(target_types=["ambient_occlusion"]), "ambient_occlusion"),
                      (dict(target_types=["depth", "ambient_occlusion"], method="brute"), "ambient_occlusion")):
        kw = dict(dict(target_types=["depth"]), **kw)
        with pytest.raises(ValueError, match=match):
            render.render_image_mesh(16, 16, None, v, t, **kw)


def test_tile_order_and_directions():
    import neddf_amd
    from neddf_amd.bvh import fibonacci_directions
    for w, h in ((16, 8), (50, 37), (7, 3), (8, 8)):
        order = neddf_amd.NeRFRender.tile_order(w, h, 8, "cpu").numpy()
        assert sorted(order.tolist()) == list(range(w * h))
        u, v = order % w, order // w
        tile = (v // 8) * ((w + 7) // 8) + u // 8
        assert (np.diff(tile) >= 0).all()                               # tile after tile
        if w % 8 == 0 and h % 8 == 0:                                   # 64 consecutive rays -- one wave -- are one tile, row-major inside
            assert (tile.reshape(-1, 64) == tile.reshape(-1, 64)[:, :1]).all()
            assert (u.reshape(-1, 8, 8) % 8 == np.arange(8)).all() and (v.reshape(-1, 8, 8) % 8 == np.arange(8)[:, None]).all()
    d = fibonacci_directions(16)
    assert d.dtype == np.float32 and d.shape == (16, 3) and np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    assert np.abs(d.astype(np.float64).mean(axis=0)).max() < 0.05 and np.array_equal(d[:, 2], (1.0 - (2.0 * np.arange(16) + 1.0) / 16).astype(np.float32))
    gram = d.astype(np.float64) @ d.astype(np.float64).T
    assert (gram - np.eye(16)).max() < 0.9                              # well spread: no two directions within 25 degrees


def test_render_mesh_flags():
    from neddf_amd.scripts.render_mesh import build_parser
    a = build_parser().parse_args(["run"])
    assert a.method == "grid" and a.bvh is False and a.tiles is False and a.ao is None
    a = build_parser().parse_args(["run", "--bvh", "--tiles", "--ao"])
    assert a.method == "grid" and a.bvh is True and a.tiles is True and a.ao == 16
    assert build_parser().parse_args(["run", "--ao", "32"]).ao == 32
    with pytest.raises(SystemExit):
        build_parser().parse_args(["run", "--method", "bvh"])
