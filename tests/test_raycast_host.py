"""Ray casting on meshes, the part that needs no GPU: the declarations of the new entry points, the numpy restatement of the hit
definition (tests/raycast_check.py) against an independent fp64 Moeller-Trumbore on a triangle soup and against the geometry of a UV
sphere -- watertight along its edges and at its vertices --, the restatement of the grid build, and the script's plumbing."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
from conftest import ROOT

import geometry_check as gc
import raycast_check as rc

NEW = ("neddf_raycast_brute", "neddf_raycast_grid_count", "neddf_raycast_grid_build", "neddf_raycast_grid_query")


# ---------------------------------------------------------------------------------------------------------------- declarations
def test_entry_points_are_declared_bound_and_exported():
    from neddf_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "neddf_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(neddf_[a-z_]+)\s*\(", hdr))
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    so = os.path.join(ROOT, "neddf_amd", "csrc", "libneddf_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T"}
    for name in NEW:
        assert name in declared and name in bound and name in exported, name
        # only the argument kinds the generic NULL-context test knows
        assert all(a in (C.c_int, C.c_int64, C.c_float, C.c_double) or issubclass(a, (C._Pointer, C.c_void_p)) for a in bound[name]), name
    assert "#define NEDDF_ABI_VERSION 7" in hdr and _lib.ABI_VERSION == 7
    lib = _lib.load()
    assert lib.neddf_abi_version() == 7
    for name in NEW:
        call = [a(0) if a in (C.c_int, C.c_int64) else a(0.0) if a in (C.c_float, C.c_double) else None for a in bound[name]]
        assert getattr(lib, name)(*call) == -1, name


# ---------------------------------------------------------------------------------------------------------------- soup vs fp64
def _moller_trumbore64(o, d, v, t):
    """Independent fp64 reference: (t, u, v, w = 1 - u - v) [R, T] of every ray on every triangle's plane (NaN for a parallel ray)."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    p = np.asarray(v, np.float64)[np.asarray(t, np.int64)]
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    with np.errstate(all="ignore"):
        pv = np.cross(d[:, None, :], e2[None])
        det = (pv * e1[None]).sum(axis=2)
        inv = np.where(det != 0, 1.0 / det, np.nan)
        tv = o[:, None, :] - p[None, :, 0]
        u = (tv * pv).sum(axis=2) * inv
        qv = np.cross(tv, e1[None])
        w = (d[:, None, :] * qv).sum(axis=2) * inv
        tt = (e2[None] * qv).sum(axis=2) * inv
    return tt, u, w, 1.0 - u - w


def test_restatement_against_fp64_on_a_triangle_soup():
    v, t = rc.soup(64, 11)
    o, d = rc.soup_rays(v, t, 4096)
    got_t, got_j, got_b1, got_b2 = rc.cast_rays(o, d, v, t, pad=2.0 ** -12 * 4.0)
    tt, u, w, s = _moller_trumbore64(o, d, v, t)
    inside = (u >= 0) & (w >= 0) & (s >= 0) & (tt >= 0)
    hits = np.where(inside, tt, np.inf)
    order = np.sort(hits, axis=1)
    first, ref_j = order[:, 0], np.argmin(hits, axis=1)
    assert np.isfinite(first).all()                                         # every ray is aimed at the inside of a triangle
    close_pair = order[:, 1] - order[:, 0] < 1e-4
    lo = np.minimum(np.minimum(u, w), s)
    near_edge = ((lo > -1e-3) & (lo < 1e-3) & (tt >= 0) & (tt <= first[:, None] + 1e-4)).any(axis=1)
    left_out = close_pair | near_edge
    print("left out: %.2f %% of %d rays" % (100.0 * left_out.mean(), len(o)))
    assert left_out.mean() <= 0.02
    keep = ~left_out
    assert (got_j[keep] == ref_j[keep]).all(), int((got_j[keep] != ref_j[keep]).sum())
    # the fp32 hit point o + t d against the fp64 plane of the triangle it names, over ALL rays (t itself differs by up to 9e-5 on grazing
    # triangles -- conditioning, not error)
    assert (got_j >= 0).all()
    p = np.asarray(v, np.float64)[t[got_j]]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    hit = o.astype(np.float64) + got_t.astype(np.float64)[:, None] * d.astype(np.float64)
    dist = np.abs(((hit - p[:, 0]) * n).sum(axis=1))
    print("plane distance of the fp32 hit point: max %.3e" % dist.max())
    assert dist.max() <= 2.5e-6
    # the barycentric pair names the same point
    assert np.abs(rc.hit_points(v, t, (got_t, got_j, got_b1, got_b2)) - hit).max() <= 1e-5


# ---------------------------------------------------------------------------------------------------------------- the UV sphere
@pytest.fixture(scope="module")
def sphere():
    return gc.uv_sphere(*rc.SPHERE)


def test_restatement_on_the_sphere_fan(sphere):
    v, t = sphere
    r, sag = rc.SPHERE[0], gc.sphere_sagitta(*rc.SPHERE)
    o, d = rc.fan_rays()
    got = rc.cast_rays(o, d, v, t, pad=2.0 ** -12 * np.sqrt(3.0))
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    d64 /= np.linalg.norm(d64, axis=1, keepdims=True)
    closest = np.linalg.norm(o64 - (o64 * d64).sum(axis=1, keepdims=True) * d64, axis=1)          # the ray's distance from the centre
    hit = got[1] >= 0
    must_hit, must_miss = closest < r - sag - 1e-6, closest > r + 1e-6
    assert must_hit.sum() > 5000 and must_miss.sum() > 5000
    assert hit[must_hit].all(), int((~hit[must_hit]).sum())
    assert not hit[must_miss].any()
    radius = np.linalg.norm(rc.hit_points(v, t, got)[hit], axis=1)
    print("%d of %d rays hit, hit radius %.5f .. %.5f" % (hit.sum(), len(o), radius.min(), radius.max()))
    assert radius.min() >= r - sag - 1e-6 and radius.max() <= r + 1e-6
    # the near side (away from the limb, where a facet's chord may end behind the centre's foot on the ray)
    central = hit & (closest < 0.4)
    assert (got[0][central] < (-(o64 * d64).sum(axis=1))[central]).all()


def test_restatement_is_watertight_on_vertex_and_edge_aimed_rays(sphere):
    v, t = sphere
    o, d, dist = rc.aimed_rays(v, t)
    assert len(o) > 6000
    got = rc.cast_rays(o, d, v, t, pad=2.0 ** -12 * np.sqrt(3.0))
    assert (got[1] >= 0).all(), int((got[1] < 0).sum())
    err = np.abs(got[0].astype(np.float64) - dist)
    print("%d aimed rays, max |t - |target - eye|| = %.3e" % (len(o), err.max()))
    assert err.max() <= 1e-3                # a ray that slips between two triangles hits the far side, about one unit later


# ---------------------------------------------------------------------------------------------------------------- the grid build
@pytest.mark.parametrize("box", ["tight", "half", "large"])
def test_build_restatement_covers_every_widened_box(sphere, box):
    v, t = sphere
    lo, hi = {"tight": (v.min(axis=0), v.max(axis=0)), "half": (np.array([-0.6, -0.6, -0.013]), np.array([0.6, 0.6, 0.6])),
              "large": (np.full(3, -4.0), np.full(3, 5.0))}[box]
    cells, pad = (17, 5, 3), 2.0 ** -12 * np.sqrt(3.0)
    assert pad >= rc.min_pad(lo, hi)
    pairs, overflow = rc.grid_lists(v, t, lo, hi, cells, pad)
    p = v[t].astype(np.float64)
    blo, bhi = p.min(axis=1) - 2.0 * pad, p.max(axis=1) + 2.0 * pad
    leaves = ((blo < np.asarray(lo, np.float64) - 2.0 * pad) | (bhi > np.asarray(hi, np.float64) + 2.0 * pad)).any(axis=1)
    # (no triangle of these boxes is a borderline case of that comparison: the fp32 rounding of the bounds cannot flip it)
    margin = np.minimum(blo - (np.asarray(lo, np.float64) - 2.0 * pad), (np.asarray(hi, np.float64) + 2.0 * pad) - bhi)
    assert (np.abs(margin) > 1e-6).all() or box == "tight"
    if box == "tight":
        assert len(overflow) == 0
    else:
        assert np.array_equal(overflow, np.flatnonzero(leaves)) and (len(overflow) > 0) == (box == "half")
    listed = set(map(tuple, pairs.tolist()))
    assert len(listed) == len(pairs)
    rng = np.random.default_rng(5)
    inside = np.setdiff1d(np.arange(len(t)), overflow)
    for k in range(8):                       # the corners and random points of every widened box, shrunk by the cell function's rounding
        w = rng.random((len(inside), 3)) if k else np.zeros((len(inside), 3))
        if k == 1:
            w[:] = 1.0
        q = (blo[inside] + 1e-6) + w * ((bhi[inside] - 1e-6) - (blo[inside] + 1e-6))
        cell, _ = gc.cell_index(q.astype(np.float32), lo, hi, cells)
        assert all((int(c), int(j)) in listed for c, j in zip(cell, inside)), (box, k)
    start = rc.cell_start(pairs, overflow, cells)
    G = cells[0] * cells[1] * cells[2]
    assert len(start) == G + 2 and start[0] == 0 and start[G + 1] == len(pairs) + len(overflow) and start[G + 1] - start[G] == len(overflow)


def test_build_restatement_skips_invalid_triangles():
    v, t = rc.soup(8, 3)
    v = np.concatenate([v, [[np.nan, 0, 0]]]).astype(np.float32)
    t = np.concatenate([t, [[0, 1, 24]], [[0, 1, 25]], [[-1, 1, 2]]]).astype(np.int32)
    pairs, overflow = rc.grid_lists(v, t, np.full(3, -2.0), np.full(3, 2.0), (3, 3, 3), 1e-3)
    assert set(pairs[:, 1].tolist()) == set(range(8)) and len(overflow) == 0


# ---------------------------------------------------------------------------------------------------------------- script and reader
def test_render_mesh_argument_parser():
    from neddf_amd.scripts.render_mesh import build_parser, threshold_of
    a = build_parser().parse_args(["run"])
    assert str(a.output_dir) == "run" and a.epoch == 2000 and a.mesh is None and a.compare_trace is None and a.method == "grid"
    a = build_parser().parse_args(["run", "--epoch", "7", "--mesh", "m.ply", "--compare-trace", "--method", "brute"])
    assert a.epoch == 7 and str(a.mesh) == "m.ply" and a.compare_trace != a.compare_trace and a.method == "brute"
    assert build_parser().parse_args(["run", "--compare-trace", "0.1"]).compare_trace == 0.1
    with pytest.raises(SystemExit):
        build_parser().parse_args(["run", "--method", "bvh"])
    assert threshold_of("run/mesh/mesh_48_threshold0.0275.ply") == 0.0275 and threshold_of("mesh_24_threshold0.1.ply") == 0.1
    with pytest.raises(ValueError):
        threshold_of("bunny.ply")


def test_read_ply_properties_round_trip(tmp_path):
    from neddf_amd.mesh import read_ply, write_ply
    rng = np.random.default_rng(2)
    v = rng.standard_normal((7, 3)).astype(np.float32)
    t = rng.integers(0, 7, (5, 3)).astype(np.int32)
    n = rng.standard_normal((7, 3)).astype(np.float32)
    c = rng.random((7, 3))
    for name, kw in (("plain", {}), ("n", dict(normals=n)), ("c", dict(colors=c)), ("nc", dict(normals=n, colors=c))):
        path = write_ply(tmp_path / (name + ".ply"), v, t, **kw)
        two = read_ply(path)
        assert len(two) == 2 and np.array_equal(two[0], v) and np.array_equal(two[1], t)           # the present return value stays
        gv, gt, gn, gc_ = read_ply(path, properties=True)
        assert np.array_equal(gv, v) and np.array_equal(gt, t)
        assert (gn is None) == ("normals" not in kw) and (gc_ is None) == ("colors" not in kw)
        if gn is not None:
            assert gn.dtype == np.float32 and np.array_equal(gn, n)
        if gc_ is not None:                 # B, G, R floats again, quantised to 1 / 255
            assert gc_.dtype == np.float32 and gc_.shape == (7, 3) and np.abs(gc_ - c).max() <= 0.5 / 255 + 1e-6
            again = write_ply(tmp_path / "again.ply", v, t, colors=gc_)
            assert np.array_equal(read_ply(again, properties=True)[3], gc_)
    ascii_ply = ("ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\n"
                 "property float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nelement face 1\n"
                 "property list uchar int vertex_indices\nend_header\n0 0 0 0 0 1 255 0 0\n1 0 0 0 1 0 0 255 0\n0 1 0 1 0 0 0 0 51\n3 0 1 2\n")
    path = tmp_path / "a.ply"
    path.write_text(ascii_ply)
    gv, gt, gn, gc_ = read_ply(path, properties=True)
    assert np.array_equal(gn, [[0, 0, 1], [0, 1, 0], [1, 0, 0]]) and np.allclose(gc_, [[0, 0, 1], [0, 1, 0], [0.2, 0, 0]])


def test_render_mesh_alias_imports():
    import importlib.util
    spec = importlib.util.spec_from_file_location("neddf_scripts_render_mesh", os.path.join(ROOT, "neddf", "scripts", "render_mesh.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from neddf_amd.scripts import render_mesh
    assert mod.main is render_mesh.main
    assert open(os.path.join(ROOT, "neddf", "scripts", "render_mesh.py")).read() == \
        open(os.path.join(ROOT, "neddf", "scripts", "compare_mesh.py")).read().replace("compare_mesh", "render_mesh")
