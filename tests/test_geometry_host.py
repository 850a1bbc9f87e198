"""Distances between surfaces without a GPU: the C ABI's new declarations and exports, NULL arguments, the PLY reader against the
writer, compare_mesh.py's arguments, and the numpy restatement (tests/geometry_check.py) against independent routes -- scipy's
k-d tree for the nearest neighbours, closed-form areas and a binomial bound for the sample counts, two concentric spheres for the
distances the GPU tests then have to reproduce."""
import os
import re
import subprocess

import numpy as np
import pytest
from conftest import ROOT

import geometry_check as gc

NEW_SYMBOLS = ("neddf_mesh_sample_count", "neddf_mesh_sample_write", "neddf_nn_brute", "neddf_nn_grid_build", "neddf_nn_grid_query")

# The two spheres of the end-to-end tests (tests/test_gpu_geometry.py imports these): radius 0.5 and 0.6 about the origin, 24 x 48
# facets each, sampled at one density.  Samples lie ON the facets, i.e. between r cos D and r from the centre; a sample x of the small
# sphere and a sample y of the large one are at least |y| - |x| >= (0.6 - s) - 0.5 apart, s = gc.sphere_sagitta(0.6, 24, 48) = 0.02044
# (the large sphere has the same facet counts, hence the coarser facets and the larger sagitta of the two).
SPHERE_LAT, SPHERE_LON, SPHERE_DENSITY, SPHERE_SEED = 24, 48, 1000.0, 7
SPHERE_SAGITTA = gc.sphere_sagitta(0.6, SPHERE_LAT, SPHERE_LON)
# measured with the restatement at these settings (3 118 -> 4 493 samples): mean nearest distance small -> large 0.099756, i.e. 0.000244
# BELOW the gap (the facets of both spheres lie inside them, the large sphere's further: that outweighs the sample spacing seen across
# the gap); the bound on the mean is the gap plus that deviation's size, doubled
SPHERE_MEAN_EXCESS = 2 * 0.000244


def spheres():
    return gc.uv_sphere(0.5, SPHERE_LAT, SPHERE_LON), gc.uv_sphere(0.6, SPHERE_LAT, SPHERE_LON)


def check_sphere_distances(d_small_to_large, what):
    """The bounds this file proves on the CPU, applied to any set of small -> large nearest distances."""
    d = np.asarray(d_small_to_large, np.float64)
    print("%s: %d distances, min %.6f (bound %.6f), mean %.6f (bound %.6f)"
          % (what, len(d), d.min(), 0.1 - SPHERE_SAGITTA, d.mean(), 0.1 + SPHERE_MEAN_EXCESS))
    assert d.min() >= 0.1 - SPHERE_SAGITTA, what
    assert d.mean() <= 0.1 + SPHERE_MEAN_EXCESS, what


def test_header_declares_and_library_exports_the_geometry_symbols():
    from neddf_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "neddf_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(neddf_[a-z_0-9]+)\s*\(", hdr))
    bound = {name for name, _, _ in _lib.SYMBOLS}
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW_SYMBOLS:
        assert name in declared and name in bound and re.search(r"\bT %s\b" % name, exported), name
    assert _lib.ABI_VERSION == 7 and _lib.load().neddf_abi_version() == 7
    assert re.search(r"#define\s+NEDDF_ABI_VERSION\s+7\b", hdr)


def test_entry_points_refuse_null_arguments():
    lib = __import__("neddf_amd")._lib.load()
    assert lib.neddf_mesh_sample_count(None, None, 0, None, 0, 1.0, 0, None, None) == -1
    assert lib.neddf_mesh_sample_write(None, None, 0, None, 0, 1.0, 0, None, None, 0, None, None) == -1
    assert lib.neddf_nn_brute(None, None, 0, None, 0, None, None, None) == -1
    assert lib.neddf_nn_grid_build(None, None, 0, None, None, None, None, None, None, None) == -1
    assert lib.neddf_nn_grid_query(None, None, 0, None, 0, None, None, None, None, None, None, None, None) == -1


def test_read_ply_round_trips_write_ply(tmp_path):
    from neddf_amd.mesh import read_ply, write_ply
    rng = np.random.default_rng(0)
    v = rng.standard_normal((37, 3)).astype(np.float32)
    v.view(np.int32)[3, 1] = 0x7fc01234                                    # a NaN payload survives
    t = rng.integers(0, 37, (51, 3)).astype(np.int32)
    nrm, col = rng.standard_normal((37, 3)).astype(np.float32), rng.random((37, 3))
    for name, kw in (("plain", {}), ("normals", dict(normals=nrm)), ("colors", dict(colors=col)), ("both", dict(normals=nrm, colors=col))):
        path = write_ply(str(tmp_path / (name + ".ply")), v, t, **kw)
        gv, gt = read_ply(path)
        assert gv.dtype == np.float32 and gt.dtype == np.int32 and gv.flags.c_contiguous and gt.flags.c_contiguous, name
        assert np.array_equal(gv.view(np.int32), v.view(np.int32)) and np.array_equal(gt, t), name
    gv, gt = read_ply(write_ply(str(tmp_path / "empty.ply"), v[:0], t[:0]))
    assert gv.shape == (0, 3) and gt.shape == (0, 3)
    # ASCII, with a comment, a colour column between the coordinates' columns and after them, and double coordinates
    text = ("ply\nformat ascii 1.0\ncomment made by the test\nelement vertex 4\nproperty double x\nproperty uchar red\nproperty double y\n"
            "property double z\nproperty float nx\nelement face 2\nproperty list uchar int vertex_indices\nend_header\n"
            "0 255 0 0 1\n1 0 0 0.5 1\n0 0 1 0 1\n0.25 7 0.25 -1e-3 1\n3 0 1 2\n3 2 1 3\n")
    (tmp_path / "ascii.ply").write_text(text)
    gv, gt = read_ply(str(tmp_path / "ascii.ply"))
    assert gv.tolist() == [[0, 0, 0], [1, 0, 0.5], [0, 1, 0], [0.25, 0.25, np.float32(-1e-3)]] and gt.tolist() == [[0, 1, 2], [2, 1, 3]]
    # what it refuses, and says why
    data = open(str(tmp_path / "normals.ply"), "rb").read()
    bad = {"truncated": data[:-5], "truncated in the vertices": data[:data.find(b"end_header\n") + 40], "no magic": b"plx" + data[3:],
           "big endian": data.replace(b"binary_little_endian", b"binary_big_endian"), "no header end": data[:60],
           "ascii truncated": text[:-8].encode(), "ascii quad": text.replace("3 2 1 3", "4 2 1 3 0").encode(),
           "no z": text.replace("property double z\n", "").encode(), "extra element": data.replace(b"element face", b"element edge 0\nelement face")}
    for name, blob in bad.items():
        p = tmp_path / "bad.ply"
        p.write_bytes(blob)
        with pytest.raises(ValueError, match="read_ply"):
            read_ply(str(p))
        print("refused:", name)
    faces = np.zeros(1, np.dtype([("n", "u1"), ("i", "<i4", (4,))]))
    faces["n"] = 4
    head = b"ply\nformat binary_little_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\nelement face 1\n" \
           b"property list uchar int vertex_indices\nend_header\n"
    (tmp_path / "quad.ply").write_bytes(head + faces.tobytes())
    with pytest.raises(ValueError, match="only triangles"):
        read_ply(str(tmp_path / "quad.ply"))


def test_compare_mesh_arguments():
    from neddf_amd.scripts.compare_mesh import parse_args
    a = parse_args(["a.ply", "b.ply"])
    assert (str(a.mesh_a), str(a.mesh_b), a.samples, a.density, a.seed, a.tau, a.method) == ("a.ply", "b.ply", 100000, None, 0, None, "grid")
    a = parse_args(["a.ply", "b.ply", "--density", "2.5", "--seed", "9", "--tau", "0.01", "--method", "brute"])
    assert (a.samples, a.density, a.seed, a.tau, a.method) == (None, 2.5, 9, 0.01, "brute")
    assert parse_args(["a.ply", "b.ply", "--samples", "500"]).samples == 500
    for bad in (["a.ply"], ["a.ply", "b.ply", "--samples", "5", "--density", "1"], ["a.ply", "b.ply", "--method", "tree"],
                ["a.ply", "b.ply", "--samples", "0"], ["a.ply", "b.ply", "--density", "-1"], ["a.ply", "b.ply", "--tau", "-1"],
                ["a.ply", "b.ply", "--seed", "-1"], ["a.ply", "b.ply", "--seed", str(2 ** 32)]):
        with pytest.raises(SystemExit):
            parse_args(bad)
    alias = open(os.path.join(ROOT, "neddf", "scripts", "compare_mesh.py")).read()
    assert "from neddf_amd.scripts.compare_mesh import main" in alias


def test_python_entry_points_validate_their_arguments():
    import torch
    from neddf_amd import NeddfError
    from neddf_amd.geometry import cloud_distance, default_cells, mesh_distance, nearest
    from neddf_amd.mesh import sample_surface
    p = torch.zeros(4, 3)
    for call in (lambda: nearest(p, p), lambda: nearest(p.numpy(), p), lambda: cloud_distance(p, p), lambda: sample_surface(p, p.int(), density=1.0),
                 lambda: mesh_distance((p, p.int()), (p, p.int()), n=10), lambda: mesh_distance((p, p.int()), (p, p.int()))):
        with pytest.raises(NeddfError):                                    # CPU tensors: no fallback
            call()
    assert default_cells(0, (0, 0, 0), (1, 1, 1)) == (1, 1, 1) and default_cells(1000, (0, 0, 0), (0, 0, 0)) == (1, 1, 1)
    assert default_cells(4000, (0, 0, 0), (1, 1, 1), 4) == (10, 10, 10) and default_cells(4000, (0, 0, 5), (2, 1, 5), 4) == (45, 22, 1)
    big = default_cells(10 ** 9, (0, 0, 0), (1, 1, 1), 1)
    assert max(big) <= 1024 and big[0] * big[1] * big[2] <= 1 << 24
    assert default_cells(10 ** 9, (0, 0, 0), (1, 1, 0), 1) == (1024, 1024, 1)


def test_restated_neighbours_against_a_kd_tree():
    """Distances within fp32 rounding of the tree's on float64 copies -- d2 is five rounded fp32 operations on exactly known inputs, a
    relative error below 5 * 2^-24 in d2, 2.5 * 2^-24 in d: 2^-22 bounds it -- and the same index wherever the tree's minimum is unique
    beyond that rounding."""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(11)
    p = rng.random((3000, 3)).astype(np.float32)
    p[100:110] = p[50]                                                     # duplicates: the lowest index wins
    p[7] = [np.nan, 0, 0]
    p[8] = [0, np.inf, 0]
    q = np.concatenate([rng.random((1500, 3)) * 1.4 - 0.2, p[40:60]]).astype(np.float32)
    q[3] = [0, np.nan, 0]
    d2, idx = gc.nearest_brute(q, p)
    assert np.isnan(d2[3]) and idx[3] == -1 and d2.dtype == np.float32 and idx.dtype == np.int32
    assert idx[1500 + 10] == 50 and d2[1500 + 10] == 0                     # q = p[50] = p[100..109]
    ok = np.isfinite(q).all(axis=1)
    valid = np.flatnonzero(np.isfinite(p).all(axis=1))
    dist, near = cKDTree(p[valid].astype(np.float64)).query(q[ok].astype(np.float64), k=2)
    got = np.sqrt(d2[ok].astype(np.float64))
    assert (np.abs(got - dist[:, 0]) <= 2.0 ** -22 * dist[:, 0]).all()
    unique = dist[:, 1] - dist[:, 0] > 2.0 ** -21 * dist[:, 1]
    assert unique.sum() > 1400 and np.array_equal(idx[ok][unique], valid[near[unique, 0]])
    assert 7 not in idx and 8 not in idx
    e = gc.nearest_brute(q[:5], p[:0])
    assert np.isposinf(e[0][[0, 1, 2, 4]]).all() and np.isnan(e[0][3]) and (e[1] == -1).all()


def test_restated_sample_counts():
    rng = np.random.default_rng(2)
    v = rng.standard_normal((300, 3)).astype(np.float32)
    t = rng.integers(0, 300, (1000, 3)).astype(np.int32)
    t[5] = [1, 1, 2]                                                       # no area
    t[6] = [0, 300, 2]                                                     # an index outside [0, V)
    t[7, 0] = -1
    v[9] = np.nan
    area, ok = gc.triangle_areas(v, t)
    exact = 0.5 * np.linalg.norm(np.cross(v[t[ok, 1]].astype(np.float64) - v[t[ok, 0]], v[t[ok, 2]].astype(np.float64) - v[t[ok, 0]]), axis=1)
    assert np.allclose(area[ok], exact, rtol=1e-6, atol=1e-9)              # fp32 edges against fp64 edges
    for density in (0.0, 0.3, 7.7, 1234.5):
        c = gc.sample_counts(v, t, density, 3)
        lo = np.floor(area * density)
        good = ok & (area > 0)
        assert ((c[good] == lo[good]) | (c[good] == lo[good] + 1)).all()
        assert (c[~good] == 0).all() and c[5] == 0 and c[6] == 0 and c[7] == 0 and (c[(t == 9).any(axis=1)] == 0).all()
    assert not np.array_equal(gc.sample_counts(v, t, 7.7, 3), gc.sample_counts(v, t, 7.7, 4))
    # 4 096 equal triangles of area 0.5 at density 2.5: A density = 1.25, so a triangle gets 2 samples with probability 0.25
    tri = (np.arange(4096, dtype=np.int32)[:, None] * 3 + np.arange(3, dtype=np.int32)[None, :]).astype(np.int32)
    base = rng.standard_normal((4096, 1, 3)).astype(np.float32).round(2)
    vv = (base + np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)[None]).astype(np.float32).reshape(-1, 3)
    c = gc.sample_counts(vv, tri, 2.5, 0)
    share = float((c == 2).mean())
    sigma = np.sqrt(0.25 * 0.75 / 4096)
    print("share rounded up: %.4f (0.25 +- %.4f)" % (share, 5 * sigma))
    assert set(np.unique(c)) == {1, 2} and abs(share - 0.25) <= 5 * sigma
    pts, tid, counts, offsets = gc.sample_surface(vv, tri, 2.5, 0)
    assert len(pts) == c.sum() and np.array_equal(np.bincount(tid, minlength=4096), c) and (np.diff(tid) >= 0).all()
    local = pts - vv[tri[tid, 0]]                                          # inside the triangle: a, b >= 0 and a + b <= 1 (to rounding)
    assert (local[:, :2] >= -1e-6).all() and (local[:, 0] + local[:, 1] <= 1 + 1e-6).all() and (np.abs(local[:, 2]) <= 1e-6).all()
    # uniform over the triangle: the mean of the barycentric coordinates is 1/3 each (sd 0.2357 / sqrt(N))
    assert np.abs(local[:, :2].mean(axis=0) - 1.0 / 3.0).max() <= 5 * 0.2357 / np.sqrt(len(pts))


def test_cell_index_restatement():
    lo, hi, cells = (0.0, -1.0, 2.0), (1.0, 1.0, 2.0), (4, 8, 3)
    p = np.array([[0.0, -1.0, 2.0], [0.999, 0.999, 2.0], [1.0, 1.0, 2.0], [-5.0, 9.0, 7.0], [0.25, 0.0, 1.0], [np.nan, 0, 2], [0.5, -0.75, 2.0]], np.float32)
    lin, c = gc.cell_index(p, lo, hi, cells)
    assert c[:5].tolist() == [[0, 0, 0], [3, 7, 0], [3, 7, 0], [0, 7, 0], [1, 4, 0]] and c[6].tolist() == [2, 1, 0]
    assert lin.tolist() == [0, 31, 31, 28, 17, -1, 6]
    lo_f, inv = gc.grid_params(lo, hi, cells)
    assert inv.tolist() == [4.0, 4.0, 0.0] and lo_f.dtype == np.float32


@pytest.fixture(scope="module")
def sphere_samples():
    (v5, t5), (v6, t6) = spheres()
    return gc.sample_surface(v5, t5, SPHERE_DENSITY, SPHERE_SEED)[0], gc.sample_surface(v6, t6, SPHERE_DENSITY, SPHERE_SEED)[0]


def test_sphere_mesh_and_its_bounds(sphere_samples):
    (v5, t5), (v6, t6) = spheres()
    assert len(t5) == SPHERE_LON * (2 * SPHERE_LAT - 2) and len(v5) == 2 + (SPHERE_LAT - 1) * SPHERE_LON
    assert np.allclose(np.linalg.norm(v5.astype(np.float64), axis=1), 0.5, atol=1e-7)
    p = v5[t5].astype(np.float64)
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert (np.einsum("ij,ij->i", n, p.mean(axis=1)) > 0).all()            # outward
    area = gc.triangle_areas(v5, t5)[0].sum()
    assert 0.99 * np.pi < area < np.pi                                     # inscribed: a little below 4 pi r^2
    edges = np.sort(np.concatenate([t5[:, [0, 1]], t5[:, [1, 2]], t5[:, [2, 0]]]), axis=1)
    assert (np.unique(edges, axis=0, return_counts=True)[1] == 2).all()    # closed: every edge twice
    a, b = sphere_samples
    assert abs(len(a) - SPHERE_DENSITY * area) < 5 * np.sqrt(len(t5) / 4.0) + 1     # each count: floor or one more, variance <= 1/4
    ra, rb = np.linalg.norm(a.astype(np.float64), axis=1), np.linalg.norm(b.astype(np.float64), axis=1)
    assert ra.max() <= 0.5 + 1e-6 and ra.min() >= 0.5 - gc.sphere_sagitta(0.5, SPHERE_LAT, SPHERE_LON) - 1e-6
    assert rb.max() <= 0.6 + 1e-6 and rb.min() >= 0.6 - SPHERE_SAGITTA - 1e-6
    d2, _ = gc.nearest_brute(a, b)
    check_sphere_distances(np.sqrt(d2.astype(np.float64)), "restatement, %d -> %d samples" % (len(a), len(b)))
    assert 0.02 < SPHERE_SAGITTA < 0.021
