"""The triangle BVH, the part that needs no GPU: the declarations of the new entry points and their refusals, the Python layer's
refusals, and the numpy restatement (tests/bvh_check.py) -- its tree against the limits the kernel's stack relies on, its traversal
against pointmesh_check.point_mesh_brute bit for bit, and the pruning cap: a tree, not a disguised brute force."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
from conftest import ROOT

import bvh_check as bc
import pointmesh_check as pm
import raycast_check as rc

F = np.float32
NEW = ("neddf_bvh_keys", "neddf_bvh_build", "neddf_point_mesh_bvh_query")


def same_bits(got, want, what):
    for k, g, w in zip(("d2", "triangle", "b1", "b2"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype)
        bad = np.flatnonzero(np.ascontiguousarray(g).view(np.int32) != np.ascontiguousarray(w).view(np.int32))
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
    assert declared == set(bound) == {n for n in exported if n.startswith("neddf_")}
    for name in NEW:
        assert name in declared and name in bound and name in exported, name
    assert "#define NEDDF_ABI_VERSION 7" in hdr and _lib.ABI_VERSION == 7
    lib = _lib.load()
    assert lib.neddf_abi_version() == 7
    for name in NEW:                # NEDDF_EINVAL for a NULL context, without a HIP call
        call = [a(0) if a in (C.c_int, C.c_int64) else a(0.0) if a in (C.c_float, C.c_double) else None for a in bound[name]]
        assert getattr(lib, name)(*call) == -1, name
    for phrase in ("THE EQUALITY ARGUMENT.  Let a box be skipped by the rule", "f = 1 - 2^-16", "s = 2^-18 * W", "d_leaf_triangle int32 [T]",
                   "d_children int32 [T - 1][2]", "d_boxes float [2 T - 1][6]", "1e-30 <= m2 < +inf"):
        assert phrase in text, phrase
    src = open(os.path.join(ROOT, "neddf_amd", "csrc", "bvh_kernels.hip")).read()
    assert "private segment size" in src and "__threadfence()" in src
    for method in ("bvh_keys", "bvh_build", "point_mesh_bvh_query"):
        assert hasattr(_lib.Context, method), method


def test_null_and_negative_count_refusals():
    """The argument checks come before any HIP call, so a context made without a device would do -- but making one needs a device.  The
    checks are exercised through their order instead: with a NULL context every entry point returns NEDDF_EINVAL whatever else it is
    given, negative counts and NULL arrays included, and never touches them."""
    from neddf_amd import _lib
    lib = _lib.load()
    box = (C.c_double * 3)(0.0, 0.0, 0.0)
    assert lib.neddf_bvh_keys(None, None, -1, None, -1, box, box, None, None) == -1
    assert lib.neddf_bvh_keys(None, None, 0, None, 5, None, None, None, None) == -1
    assert lib.neddf_bvh_build(None, None, 3, None, -2, None, None, None, None, None) == -1
    assert lib.neddf_point_mesh_bvh_query(None, None, -1, None, 0, None, 4, None, None, None, 3, None, None, None, None, None, None) == -1
    # the refusals themselves are in the source next to the point-mesh block's, by the same mesh check (tests/test_gpu_capi_refusals.py
    # holds every one of them to its code and text on the device)
    capi = open(os.path.join(ROOT, "neddf_amd", "csrc", "geom_capi.hip")).read()
    for name in ("bvh_keys", "bvh_build", "point_mesh_bvh_query"):
        assert 'mesh_counts_ok(ctx, n_vertices, d_vertices, n_triangles, d_triangles, "%s"' % name in capi, name
    assert 'if (n_leaves != n_triangles) return fail(ctx, NEDDF_EINVAL, "point_mesh_bvh_query: ' in capi


def test_python_layer_exports_and_refusals_without_a_device():
    import torch
    from neddf_amd import bvh, geometry
    from neddf_amd._lib import NeddfError
    from neddf_amd.network import BaseNeuralField
    assert "distance_field_check" in geometry.__all__ and set(bvh.__all__) == {"MeshBVH", "build_bvh"}
    assert callable(BaseNeuralField.distance_field_check)
    q, v, t = torch.zeros(4, 3), torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)
    with pytest.raises(NeddfError, match="HIP device"):
        geometry.point_mesh_distance(q, v, t, method="bvh")
    with pytest.raises(NeddfError, match="HIP device"):
        bvh.build_bvh(v, t)
    with pytest.raises(NeddfError, match="HIP device"):
        geometry.distance_field_check(lambda p: p[:, 0], v, t, 0.0)
    with pytest.raises(NeddfError, match="callable"):
        geometry.distance_field_check(None, v, t, 0.0)
    # a foreign or malformed tree is refused before anything is launched
    foreign = bvh.MeshBVH((0, 0, 0), (1, 1, 1), torch.zeros(2, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32), torch.zeros(3, 6), 3, 2)
    with pytest.raises(NeddfError, match="bvh must be the MeshBVH"):
        bvh.bvh_of("x", v, t, foreign)
    with pytest.raises(NeddfError, match="bvh must be the MeshBVH"):
        bvh.bvh_of("x", v, t, "tree")
    own = bvh.MeshBVH((0, 0, 0), (1, 1, 1), torch.zeros(1, dtype=torch.int32), torch.zeros(0, 2, dtype=torch.int32), torch.zeros(1, 6), 3, 1)
    assert bvh.bvh_of("x", v, t, own) is own
    from neddf_amd.scripts import compare_mesh, extract_mesh
    assert compare_mesh.parse_args(["a.ply", "b.ply", "--method", "bvh", "--exact"]).method == "bvh"
    with pytest.raises(SystemExit):
        compare_mesh.parse_args(["a.ply", "b.ply", "--method", "bvh"])
    args = extract_mesh.build_parser().parse_args(["run", "--check-volume"])
    assert args.check_volume == 100000 and extract_mesh.build_parser().parse_args(["run"]).check_volume is None


# ---------------------------------------------------------------------------------------------------------------- the restatement
from test_gpu_pointmesh import _query_pool, _soup_mesh          # noqa: E402  (numpy only: the soup and the query pool the GPU tests use)


@pytest.mark.parametrize("n_tri", [1, 2, 3, 255, 256, 257, 1025])
def test_restatement_equals_brute_on_the_soup_and_the_query_pool(n_tri):
    v, t = _soup_mesh(n_tri)
    q = _query_pool(v, t)
    tree = bc.build(v, t)
    got = bc.point_mesh_bvh(q, v, t, tree)
    same_bits(got[:4], pm.point_mesh_brute(q, v, t), n_tri)
    assert tree["depth"] <= 62 and got[5] <= tree["depth"] + 1, (tree["depth"], got[5])
    assert (got[4][:3] == 0).all() and (got[4][3:] >= 1).all()
    if n_tri > 16:
        assert not np.isin(got[1], [5, 6, 8, n_tri - 1]).any()          # invalid ones, and the duplicate loses to triangle 3


def lattice():
    """512 triangles in the plane z = 0.25: a 17 x 17 lattice of vertices, two triangles per square."""
    x, y = np.meshgrid(np.linspace(-0.5, 0.5, 17), np.linspace(-0.5, 0.5, 17))
    v = np.stack([x.ravel(), y.ravel(), np.full(x.size, 0.25)], axis=1).astype(F)
    idx = np.arange(x.size).reshape(17, 17)
    t = np.concatenate([np.stack([idx[:-1, :-1], idx[:-1, 1:], idx[1:, 1:]], -1).reshape(-1, 3),
                        np.stack([idx[:-1, :-1], idx[1:, 1:], idx[1:, :-1]], -1).reshape(-1, 3)]).astype(np.int32)
    mid = (0.5 * (v[t[:, 0]].astype(np.float64) + v[t[:, 1]])).astype(F)
    q = np.concatenate([v + F([0, 0, 0.1]), mid[::3] + F([0, 0, 0.05]), v[::5] - F([0, 0, 2.0])]).astype(F)           # neighbours tie
    return v, t, q


def cases():
    """(name, vertices, triangles, queries): the inputs the GPU test repeats on the device."""
    rng = np.random.default_rng(31)
    uni = rng.uniform(-1.2, 1.2, (60, 3)).astype(F)
    special = np.array([[np.nan, 0, 0], [0, np.inf, 0]], F)
    out = []
    for n in (1, 2, 3, 257):
        v, t = _soup_mesh(n)
        vv = v[np.isfinite(v).all(axis=1)]
        tie = v[t[3]].astype(np.float64).mean(axis=0).astype(F)[None] if n > 16 else uni[:1]
        out.append(("soup %d" % n, v, t, np.concatenate([special, uni, vv[::max(len(vv) // 40, 1)], tie, uni[:20] + F(100.0)]).astype(F)))
    v, t = rc.soup(500, 11)
    out.append(("no triangle", v, t[:0], uni))
    bad = t[:7].copy()
    bad[:, 1] = -3
    out.append(("all invalid", v, bad, uni))
    out.append(("300 duplicates", v, np.repeat(t[3:4], 300, axis=0), uni[:20]))
    pv, pt, pq = lattice()
    out.append(("lattice", pv, pt, pq))
    for name, scale, offset in (("offset 1000, 2^-8", 2.0 ** -8, 1000.0), ("offset 16, 2^-6", 2.0 ** -6, 16.0)):
        vs = (v.astype(np.float64) * scale + offset).astype(F)
        qs = np.concatenate([(uni.astype(np.float64) * scale + offset).astype(F), vs[::50], uni[:10]]).astype(F)
        out.append((name, vs, t, qs))
    return out


@pytest.mark.parametrize("case", cases(), ids=lambda c: c[0])
def test_restatement_equals_brute_bit_for_bit(case):
    name, v, t, q = case
    tree = bc.build(v, t)
    got = bc.point_mesh_bvh(q, v, t, tree)
    same_bits(got[:4], pm.point_mesh_brute(q, v, t), name)
    assert tree["depth"] <= 62 and got[5] <= tree["depth"] + 1, (tree["depth"], got[5])
    ok = rc._valid_triangles(v, t)[1]
    fin = np.isfinite(q).all(axis=1)
    assert (got[4][~fin] == 0).all() and (got[4] <= ok.sum()).all()                # an invalid triangle is never evaluated
    if name == "300 duplicates":
        assert (got[4] == 300).all()                                                # they all tie
    if name == "lattice":
        assert got[4].mean() < 16


def test_tree_is_a_binary_tree_over_every_leaf():
    v, t = _soup_mesh(257)
    tree = bc.build(v, t)
    leaf, children, boxes = tree["leaf"], tree["children"], tree["boxes"]
    assert sorted(leaf.tolist()) == list(range(257)) and children.shape == (256, 2) and boxes.shape == (513, 6)
    seen = np.sort(children.reshape(-1))
    assert np.array_equal(seen, np.concatenate([np.arange(-257, 0), np.arange(1, 256)]))           # every node but the root, once
    ok = rc._valid_triangles(v, t)[1]
    assert not ok[leaf[-(~ok).sum():]].any() and ok[leaf[:ok.sum()]].all()                          # the invalid ones sort last
    assert np.isinf(boxes[256:][~ok[leaf]]).all() and np.isfinite(boxes[0]).all()
    p = v[t[ok]].reshape(-1, 3)
    assert np.array_equal(boxes[0], np.concatenate([p.min(axis=0), p.max(axis=0)]))


def test_pruning_cap():
    """A condition, not a measurement: below 5 % of T leaf evaluations per query, near the mesh and 100 and 3000 mesh sizes away."""
    v, t = rc.soup(2000, 11)
    tree = bc.build(v, t)
    q = np.random.default_rng(32).uniform(-1.2, 1.2, (150, 3)).astype(F)
    for shift in (0.0, 100.0, 3000.0):
        qq = (q + F(shift)).astype(F)
        got = bc.point_mesh_bvh(qq, v, t, tree)
        same_bits(got[:4], pm.point_mesh_brute(qq, v, t), shift)
        print("shift %6.0f: %.1f leaf evaluations per query (max %d) of %d, stack %d, depth %d" % (shift, got[4].mean(), got[4].max(), len(t), got[5],
                                                                                              tree["depth"]))
        assert got[4].mean() < 0.05 * len(t), (shift, got[4].mean())
    assert tree["depth"] <= 62
