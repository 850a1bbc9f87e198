"""Point-to-mesh distance, the part that needs no GPU: the declarations of the new entry points, the numpy restatement of the
arithmetic (tests/pointmesh_check.py) against an independent fp64 closest-point computation and against the geometry of a UV sphere,
the grid query's shell walk against the restatement bit for bit, and the Python layer's refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
from conftest import ROOT

import geometry_check as gc
import pointmesh_check as pm
import raycast_check as rc

F = np.float32
NEW = ("neddf_point_mesh_brute", "neddf_point_mesh_grid_query")

# The restatement against closest_fp64, in units of 2^-24 M (M: the largest |coordinate| among vertices and queries), measured on the
# CPU over the six cases of _cases() below -- never against the kernel:
#     case                         worst overshoot   worst undershoot
#     uniform around the sphere         1.31              1.15
#     samples ON the sphere             1.40              1.13
#     200-triangle soup                 0.87              1.03
#     100 slivers of aspect 1e-5        1.17              1.08
#     exactly degenerate triangles      1.21              1.09
#     the sphere moved to +100          1.60              1.36
# The gates are four times the worst of each column.  (With the interior candidate solved through the Gram determinant and not refined
# the samples ON the sphere overshoot by 15.9 -- the polar fans' 7.5-degree triangles -- and samples of a marching-cubes mesh on
# their own triangles by 79 and more: the header says why the interior candidate is orthogonalised and refined once.)
OVERSHOOT_GATE = 6.5             # 4 * 1.60, rounded up to the next half
UNDERSHOOT_GATE = 5.5            # 4 * 1.36, rounded up to the next half


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
    for name in NEW:
        assert name in declared and name in bound and name in exported, name
        # only the argument kinds the generic NULL-context test knows
        assert all(a in (C.c_int, C.c_int64, C.c_float, C.c_double) or issubclass(a, (C._Pointer, C.c_void_p)) for a in bound[name]), name
    assert "#define NEDDF_ABI_VERSION 7" in hdr and _lib.ABI_VERSION == 7
    lib = _lib.load()
    assert lib.neddf_abi_version() == 7
    for name in NEW:                # NEDDF_EINVAL for a NULL context, without a HIP call (this machine may have no device)
        call = [a(0) if a in (C.c_int, C.c_int64) else a(0.0) if a in (C.c_float, C.c_double) else None for a in bound[name]]
        assert getattr(lib, name)(*call) == -1, name
    # the header states the arithmetic and the equality argument
    for phrase in ("THE EQUALITY ARGUMENT.  Let the walk stop after shell", "rpp = 1 / gpp", "clamp01(u) = u > 0 ? (u < 1 ? u : 1) : 0",
                   "e >= 2^-10 W", "(r * safe_cell)^2 > best D2 strictly"):
        assert phrase in text, phrase
    assert hasattr(_lib.Context, "point_mesh_brute") and hasattr(_lib.Context, "point_mesh_grid_query")


def test_python_layer_exports_and_refusals_without_a_device():
    import torch
    from neddf_amd import geometry
    from neddf_amd._lib import NeddfError
    from neddf_amd.network import BaseNeuralField
    for name in ("point_mesh_distance", "closest_points", "level_set_check", "mesh_distance"):
        assert name in geometry.__all__ and callable(getattr(geometry, name)), name
    assert callable(BaseNeuralField.level_set_check)
    q, v, t = torch.zeros(4, 3), torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)
    with pytest.raises(NeddfError, match="HIP device"):
        geometry.point_mesh_distance(q, v, t)
    with pytest.raises(NeddfError, match="HIP device"):
        geometry.level_set_check(lambda p: p[:, 0], v, t, 0.0, 0.1)
    with pytest.raises(NeddfError, match="callable"):
        geometry.level_set_check(None, v, t, 0.0, 0.1)
    with pytest.raises(NeddfError, match="'samples' or 'surface'"):
        geometry.mesh_distance((v, t), (v, t), n=10, to="triangles")


# ---------------------------------------------------------------------------------------------------------------- against fp64
@pytest.fixture(scope="module")
def sphere():
    return gc.uv_sphere(*rc.SPHERE)


def _cases(sphere):
    v, t = sphere
    rng = np.random.default_rng(5)
    q = rng.uniform(-1.0, 1.0, (3000, 3)).astype(F)
    on, _, _, _ = gc.sample_surface(v, t, 3000.0 / np.pi, 3)           # 2 969 samples of the sphere's own triangles
    sv, st = rc.soup(200, 11)
    a, e, n = rng.uniform(-0.5, 0.5, (100, 3)), rng.uniform(-0.3, 0.3, (100, 3)), rng.standard_normal((100, 3))
    height = 1e-5 * np.linalg.norm(e, axis=1, keepdims=True) * n / np.linalg.norm(n, axis=1, keepdims=True)
    ids = np.arange(300, dtype=np.int32).reshape(100, 3)
    slivers = np.stack([a, a + e, a + 0.5 * e + height], axis=1).astype(F)
    flat = np.stack([a, a, a], axis=1).astype(F)                        # 50 points, then 50 segments a .. a + e with c = b
    flat[50:, 1] = (a + e)[50:]
    flat[50:, 2] = flat[50:, 1]
    return [("uniform", q, v, t), ("on the surface", on, v, t), ("soup", q, sv, st), ("slivers", q, slivers.reshape(-1, 3), ids),
            ("degenerate", q, flat.reshape(-1, 3), ids), ("moved to +100", (q + F(100.0)).astype(F), (v + F(100.0)).astype(F), t)]


def test_restatement_against_an_independent_fp64_closest_point(sphere):
    worst_over = worst_under = 0.0
    for name, q, v, t in _cases(sphere):
        d2, j, b1, b2 = pm.point_mesh_brute(q, v, t)
        assert (j >= 0).all() and np.isfinite(d2).all(), name
        ref = pm.closest_fp64(q, v, t)
        unit = 2.0 ** -24 * max(float(np.abs(v).max()), float(np.abs(q).max()))
        u = (np.sqrt(d2.astype(np.float64)) - ref) / unit
        print("%-16s overshoot %6.2f  undershoot %6.2f  (units of 2^-24 M)" % (name, u.max(), -u.min()))
        worst_over, worst_under = max(worst_over, u.max()), max(worst_under, -u.min())
        # the barycentric pair names the point the distance was measured to
        cp = pm.closest_points(v, t, (d2, j, b1, b2))
        back = np.linalg.norm(q.astype(np.float64) - cp, axis=1)
        assert np.abs(back - ref).max() <= OVERSHOOT_GATE * unit, name
        assert (b1 >= 0).all() and (b2 >= 0).all() and (b1.astype(np.float64) + b2 <= 1.0 + 2.0 ** -22).all(), name
    assert worst_over <= OVERSHOOT_GATE and worst_under <= UNDERSHOOT_GATE, (worst_over, worst_under)


def test_restatement_on_the_sphere(sphere):
    v, t = sphere
    r, sag = rc.SPHERE[0], gc.sphere_sagitta(*rc.SPHERE)
    q = np.random.default_rng(6).uniform(-1.0, 1.0, (2000, 3)).astype(F)
    d = np.sqrt(pm.point_mesh_brute(q, v, t)[0].astype(np.float64))
    radius = np.linalg.norm(q.astype(np.float64), axis=1)
    out = radius >= r
    assert out.sum() > 800
    assert (d[out] >= radius[out] - r - 1e-6).all() and (d[out] <= radius[out] - r + sag + 1e-6).all()


def test_a_vertex_is_at_distance_zero_of_its_lowest_triangle(sphere):
    v, t = sphere
    d2, j, b1, b2 = pm.point_mesh_brute(v, v, t)
    assert (d2 == 0).all()
    lowest = np.full(len(v), len(t), np.int64)
    np.minimum.at(lowest, t.reshape(-1), np.repeat(np.arange(len(t)), 3))
    assert (j == lowest).all()
    # (the barycentric pair may be that of an edge candidate whose u is one rounding short of 1 and whose rounded point is the vertex)
    assert np.abs(pm.closest_points(v, t, (d2, j, b1, b2)) - v).max() <= 2.0 ** -24


def test_special_inputs():
    v, t = rc.soup(8, 11)
    q = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0.1, 0.2, 0.3]], F)
    d2, j, b1, b2 = pm.point_mesh_brute(q, v, t)
    assert np.isnan(d2[:2]).all() and (j[:2] == -1).all() and np.isnan(b1[:2]).all() and np.isnan(b2[:2]).all() and j[2] >= 0
    bad = t.copy()
    bad[:, 0] = len(v)                                                  # no valid triangle
    d2, j, b1, b2 = pm.point_mesh_brute(q[2:], v, bad)
    assert d2[0] == np.inf and j[0] == -1 and b1[0] == 0 and b2[0] == 0
    d2, j, _, _ = pm.point_mesh_brute(q[2:], v, t[:0])
    assert d2[0] == np.inf and j[0] == -1
    dup = np.concatenate([t, t[3:4]])                                   # an exact duplicate at a higher index never wins
    assert (pm.point_mesh_brute(v, v, dup)[1] < len(t)).all()


# ---------------------------------------------------------------------------------------------------------------- the shell walk
SPHERE_PAD = 2.0 ** -12 * np.sqrt(3.0)          # above the library's limit for every box below (the largest: 3 * 2^-16)
BOXES = {"own": ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)), "cutting": ((-0.2, -0.6, -0.6), (0.6, 0.6, 0.3)), "three times": ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))}


def walk_queries(v, t):
    rng = np.random.default_rng(7)
    on, _, _, _ = gc.sample_surface(v, t, 12.0 / np.pi, 4)
    far = np.array([[3.0, 0.1, -0.2], [-0.3, -40.0, 0.2], [100.0, 100.0, 100.0], [0.0, 0.0, 0.0]], F)
    return np.concatenate([rng.uniform(-0.7, 0.7, (12, 3)).astype(F), on[:12], v[::181], far]).astype(F)


@pytest.fixture(scope="module")
def walk_reference(sphere):
    q = walk_queries(*sphere)
    return q, pm.point_mesh_brute(q, *sphere)


@pytest.mark.parametrize("cells", [(1, 1, 1), (2, 3, 5), (17, 17, 17), (40, 40, 40)])
@pytest.mark.parametrize("box", sorted(BOXES))
def test_shell_walk_equals_the_restatement(sphere, walk_reference, box, cells):
    v, t = sphere
    q, want = walk_reference
    lo, hi = BOXES[box]
    assert pm.grid_walks(lo, hi, cells, SPHERE_PAD)[0]
    got = pm.point_mesh_grid(q, v, t, lo, hi, cells, SPHERE_PAD, return_visits=True)
    for g, w, k in zip(got, want, ("d2", "triangle", "b1", "b2")):
        assert g.dtype == w.dtype and (g.view(np.int32) == w.view(np.int32)).all(), (box, cells, k)
    if cells == (40, 40, 40) and box == "own":           # the walk does stop early: a query on the surface meets a fraction of the mesh
        assert got[4][12:24].max() < len(t) // 4 and got[4][-2] >= len(t)


def test_small_cells_far_from_the_origin_are_not_walked(sphere):
    v, t = sphere
    far = (v * F(0.05) + F(100.0)).astype(F)
    lo, hi = far.min(axis=0).astype(np.float64), far.max(axis=0).astype(np.float64)
    pad = 4.0 * rc.min_pad(lo, hi)
    assert not pm.grid_walks(lo, hi, (17, 17, 17), pad)[0]            # cells of 0.003 at coordinates of 100: below 2^-10
    q = np.concatenate([far[::97], [[100.0, 100.0, 100.0], [0.0, 0.0, 0.0]]]).astype(F)
    want = pm.point_mesh_brute(q, far, t)
    got = pm.point_mesh_grid(q, far, t, lo, hi, (17, 17, 17), pad)
    for g, w in zip(got, want):
        assert (g.view(np.int32) == w.view(np.int32)).all()
