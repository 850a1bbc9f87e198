"""CPU checks of mesh simplification by vertex clustering: the numpy restatement (tests/simplify_check.py) against a brute-force
Python version on tiny meshes, the identity property, the displacement bound of include/neddf_hip.h, the quadric placement against
the mean on a subdivided box, and the new entry points in the binding."""
import math

import numpy as np
import pytest

import pointmesh_check as pm
import simplify_check as sc

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    assert len(got) == len(want), what
    for g, w, part in zip(got, want, ("vertices", "triangles", "vertex_map", "triangle_map", "attributes")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, part, g.dtype, w.dtype, g.shape, w.shape)
        same = np.array_equal(_bits(g), _bits(w)) if g.dtype == np.float32 else np.array_equal(g, w)
        assert same, (what, part)


# ---- the definition, one vertex and one triangle at a time, in Python floats (IEEE doubles, one rounding per operation) -------------
def _cell(p, lo, hi, n):
    lo32 = F(lo)
    ext = float(hi) - float(lo)
    inv = F(float(n) / ext) if ext > 0.0 else F(0.0)
    f = F(F(p - lo32) * inv)
    return n - 1 if f >= F(n) else (int(f) if f > 0 else 0)


def brute_simplify(v, t, cells, box=None, placement="mean", reg=2.0 ** -10, attr=None):
    v = np.asarray(v, F).reshape(-1, 3)
    t = np.asarray(t, np.int32).reshape(-1, 3)
    V = len(v)
    lo, hi = sc.default_box(v) if box is None else box
    groups = {}
    for i in range(V):
        if all(math.isfinite(float(x)) for x in v[i]):
            key = tuple(_cell(v[i, a], lo[a], hi[a], cells[a]) for a in range(3))
        else:
            key = ("non-finite", i)
        groups.setdefault(key, []).append(i)
    members = sorted(groups.values(), key=lambda m: m[0])          # numbered in the order of their lowest vertex
    cluster = np.zeros(V, np.int64)
    for c, m in enumerate(members):
        cluster[m] = c
    finite = [all(math.isfinite(float(x)) for x in p) for p in v]
    valid = [all(0 <= int(i) < V for i in tri) and all(finite[int(i)] for i in tri) for tri in t]
    rep = np.zeros((len(members), 3), F)
    rep_attr = None if attr is None else np.zeros((len(members), attr.shape[1]), F)
    for c, m in enumerate(members):
        if attr is not None:
            for k in range(attr.shape[1]):
                s = 0.0
                for i in m:
                    s += float(attr[i, k])
                val = F(s / float(len(m)))
                rep_attr[c, k] = val
                if math.isnan(float(val)):
                    _bits(rep_attr)[c, k] = 0x7fc00000
            if len(m) == 1:
                _bits(rep_attr)[c] = _bits(attr)[m[0]]
        if len(m) == 1:
            _bits(rep)[c] = _bits(v)[m[0]]
            continue
        mean = []
        for a in range(3):
            s = 0.0
            for i in m:
                s += float(v[i, a])
            mean.append(s / float(len(m)))
        x = list(mean)
        if placement == "quadric":
            A = [[0.0] * 3 for _ in range(3)]
            r = [0.0] * 3
            for j in range(len(t)):
                if not valid[j] or not any(cluster[int(i)] == c for i in t[j]):
                    continue
                p0, p1, p2 = ([float(x_) for x_ in v[int(i)]] for i in t[j])
                u = [p1[a] - p0[a] for a in range(3)]
                w = [p2[a] - p0[a] for a in range(3)]
                n = [u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]]
                for a in range(3):
                    for b in range(a, 3):
                        A[a][b] += n[a] * n[b]
                d = (n[0] * (p0[0] - mean[0]) + n[1] * (p0[1] - mean[1])) + n[2] * (p0[2] - mean[2])
                for a in range(3):
                    r[a] += n[a] * d
            tr = (A[0][0] + A[1][1]) + A[2][2]
            if tr != 0.0 and math.isfinite(tr):
                lam = (reg * tr) / 3.0
                b00, b11, b22 = A[0][0] + lam, A[1][1] + lam, A[2][2] + lam
                a01, a02, a12 = A[0][1], A[0][2], A[1][2]
                c00, c01, c02 = b11 * b22 - a12 * a12, a02 * a12 - a01 * b22, a01 * a12 - a02 * b11
                c11, c12, c22 = b00 * b22 - a02 * a02, a01 * a02 - b00 * a12, b00 * b11 - a01 * a01
                det = (b00 * c00 + a01 * c01) + a02 * c02
                if det != 0.0 and math.isfinite(det):
                    y = [((c00 * r[0] + c01 * r[1]) + c02 * r[2]) / det, ((c01 * r[0] + c11 * r[1]) + c12 * r[2]) / det,
                         ((c02 * r[0] + c12 * r[1]) + c22 * r[2]) / det]
                    if all(math.isfinite(q) for q in y):
                        x = [mean[a] + y[a] for a in range(3)]
            for a in range(3):
                mn, mx = min(float(v[i, a]) for i in m), max(float(v[i, a]) for i in m)
                x[a] = min(max(x[a], mn), mx)
        rep[c] = [F(q) for q in x]
    seen, keep, canon = set(), [], []
    for tri in t:
        if not all(0 <= int(i) < V for i in tri):
            keep.append(False)
            canon.append(None)
            continue
        c = [int(cluster[int(i)]) for i in tri]
        k = c.index(min(c))
        identity = tuple(c[k:] + c[:k])                  # rotated, the lowest first: which triangles are the same
        ok = len(set(c)) == 3 and identity not in seen
        if len(set(c)) == 3:
            seen.add(identity)
        keep.append(ok)
        canon.append(tuple(c))                          # the output keeps the corner order
    used = sorted({c for k, tri in zip(keep, canon) if k for c in tri})
    new = {c: i for i, c in enumerate(used)}
    out_v = rep[used] if used else np.zeros((0, 3), F)
    out_t = np.array([[new[c] for c in tri] for k, tri in zip(keep, canon) if k], np.int32).reshape(-1, 3)
    vmap = np.array([new.get(int(c), -1) for c in cluster], np.int32)
    tmap, n = [], 0
    for k in keep:
        tmap.append(n if k else -1)
        n += bool(k)
    out = (out_v, out_t, vmap, np.array(tmap, np.int32))
    if attr is None:
        return out
    return out + ((rep_attr[used] if used else np.zeros((0, attr.shape[1]), F)),)


def tiny_meshes():
    out = {}
    out["sphere"] = sc.uv_sphere(5, 6)
    v, t = sc.triangle_soup(40, 60, seed=2)
    t[3] = (0, 1, 40)                                    # out of range
    t[7] = (-1, 2, 3)
    t[11] = t[10]                                        # a duplicate
    t[12] = t[10][[1, 2, 0]]                             # ... and a rotation of it
    t[13] = t[10][[0, 2, 1]]                             # the opposite orientation
    v[5, 1] = np.nan
    v[9, 0] = np.inf
    _bits(v)[17, 2] = 0x7fc01234                          # a NaN with a payload
    out["soup"] = (v, t)
    out["single"] = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F), np.array([[0, 1, 2]], np.int32))
    out["flat"] = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [2, 0, 0], [2, 1, 0]], F),
                   np.array([[0, 1, 2], [1, 3, 2], [1, 4, 3], [4, 5, 3]], np.int32))          # a zero-extent axis
    return out


@pytest.mark.parametrize("name", ["sphere", "soup", "single", "flat"])
@pytest.mark.parametrize("placement", ["mean", "quadric"])
def test_restatement_against_brute_force(name, placement):
    v, t = tiny_meshes()[name]
    attr = np.random.default_rng(1).standard_normal((len(v), 4)).astype(F)
    attr[len(v) // 2, 0], attr[len(v) // 2 + 1, 0], attr[0, 1] = np.inf, -np.inf, np.nan          # inf - inf in a cell of both: NaN
    for cells in ((1, 1, 1), (2, 2, 2), (3, 2, 5), (1024, 7, 1)):
        got = sc.simplify(v, t, cells=cells, placement=placement, attributes=attr)
        want = brute_simplify(v, t, cells, placement=placement, attr=attr)
        _same(got, want, (name, placement, cells))
    box = ([0.25, 0.25, 0.25], [0.75, 0.5, 1.0])           # a box smaller than the mesh: outside points are clamped
    _same(sc.simplify(v, t, cells=(2, 3, 2), box=box, placement=placement, regularisation=0.0),
          brute_simplify(v, t, (2, 3, 2), box=box, placement=placement, reg=0.0), (name, placement, "box"))


def test_empty_inputs_and_full_collapse():
    v, t = sc.uv_sphere(5, 6)
    for placement in ("mean", "quadric"):
        ov, ot, vm, tm = sc.simplify(v[:0], t[:0], cells=(2, 2, 2), placement=placement)
        assert ov.shape == (0, 3) and ot.shape == (0, 3) and vm.shape == (0,) and tm.shape == (0,)
        ov, ot, vm, tm = sc.simplify(v, t[:0], cells=(2, 2, 2), placement=placement)
        assert ov.shape == (0, 3) and ot.shape == (0, 3) and (vm == -1).all() and len(vm) == len(v)
        ov, ot, vm, tm = sc.simplify(v[:0], t, cells=(2, 2, 2), placement=placement)
        assert ov.shape == (0, 3) and ot.shape == (0, 3) and (tm == -1).all() and len(tm) == len(t)
        ov, ot, vm, tm = sc.simplify(v, t, cells=(1, 1, 1), placement=placement)          # everything in one cell
        assert ov.shape == (0, 3) and ot.shape == (0, 3) and (vm == -1).all() and (tm == -1).all()


def test_grid_cells_from_an_edge_length():
    assert sc.grid_cells([0, 0, 0], [1, 2, 0], 0.5) == (2, 4, 1)
    assert sc.grid_cells([0, 0, 0], [1, 1, 1], 0.3) == (4, 4, 4)
    v, t = sc.uv_sphere(6, 8)
    _same(sc.simplify(v, t, cell=0.7), sc.simplify(v, t, cells=(3, 3, 3)), "cell = 0.7 over an extent of 2")


@pytest.mark.parametrize("placement", ["mean", "quadric"])
def test_identity_when_no_two_vertices_share_a_cell(placement):
    v, t = sc.uv_sphere(12, 16)
    lo, hi = sc.default_box(v)
    cells = (1024, 1024, 1024)
    k = sc.keys(v, lo, hi, cells)
    assert len(np.unique(k >> 32)) == len(v)                # the premise: one vertex per cell
    attr = np.random.default_rng(0).standard_normal((len(v), 3)).astype(F)
    ov, ot, vm, tm, oa = sc.simplify(v, t, cells=cells, placement=placement, attributes=attr)
    assert np.array_equal(_bits(ov), _bits(v)) and np.array_equal(ot, t) and np.array_equal(_bits(oa), _bits(attr))
    assert np.array_equal(vm, np.arange(len(v))) and np.array_equal(tm, np.arange(len(t)))


def _bound(lo, hi, cells):
    return (1.0 + 2.0 ** -10) * math.sqrt(sum(((h - l) / c) ** 2 for l, h, c in zip(lo, hi, cells)))


@pytest.mark.parametrize("placement", ["mean", "quadric"])
@pytest.mark.parametrize("mesh", ["sphere", "soup", "offset"])
def test_displacement_bound(mesh, placement):
    """Every input vertex whose cluster survives lies within (1 + 2^-10) cell diagonals of its output vertex."""
    if mesh == "sphere":
        v, t = sc.uv_sphere(24, 32)
    elif mesh == "soup":
        v, t = sc.triangle_soup(3000, 6000, seed=4)
    else:                                                   # rounding dominates the cell function
        v, t = sc.uv_sphere(24, 32, radius=2.0 ** -9, centre=(1000.0, 1000.0, 1000.0))
    lo, hi = sc.default_box(v)
    for cells in ((4, 4, 4), (37, 5, 1024), (9, 9, 9)):
        ov, ot, vm, tm = sc.simplify(v, t, cells=cells, placement=placement)
        moved = np.linalg.norm(v[vm >= 0].astype(np.float64) - ov[vm[vm >= 0]].astype(np.float64), axis=1)
        assert len(moved) and moved.max() <= _bound(lo, hi, cells), (mesh, cells, moved.max(), _bound(lo, hi, cells))
        assert len(ot) == (tm >= 0).sum() and (ot >= 0).all() and (ot < len(ov)).all()
        assert len(ov) < len(v)


def test_quadric_stays_on_a_box_where_the_mean_cuts_its_corners():
    """An axis-aligned cube of half-width 1, each face 12 x 12 squares, cells of 3 face steps (4 x 4 x 4 cells): the distance of the
    output vertices to the INPUT surface (tests/pointmesh_check.py's restatement of the exact point-to-mesh distance).

    Measured on the CPU: mean max 1.892e-01 (the corner clusters' means lie inside the cube), quadric max 1.846e-04 (the
    regularisation's pull towards the mean, 2^-10 of it): a ratio of 1025.  The gate is quadric <= mean / 4, which the measurement
    passes with a factor of 256 to spare -- far more than the factor two the gate wants."""
    v, t = sc.box_mesh(12)
    assert len(v) == 6 * 144 + 2 and len(t) == 12 * 144
    cell = 3 * 2.0 / 12
    far = {}
    for placement in ("mean", "quadric"):
        ov, ot, vm, tm = sc.simplify(v, t, cell=cell, placement=placement)
        assert len(ov) and len(ot)
        d2 = pm.point_mesh_brute(ov, v, t)[0]
        far[placement] = float(np.sqrt(d2.astype(np.float64)).max())
    print("box 12 x 12, cell of 3 steps: max distance to the input surface: mean %.3e, quadric %.3e, ratio %.1f"
          % (far["mean"], far["quadric"], far["mean"] / max(far["quadric"], 1e-300)))
    assert far["mean"] > 0.0
    assert far["quadric"] <= far["mean"] / 4.0, far


def test_binding_declares_the_new_entry_points():
    """(tests/test_host.py::test_capi_exports_every_declared_symbol holds header, binding and library to one list.)"""
    from neddf_amd import _lib
    names = {n for n, _, _ in _lib.SYMBOLS}
    new = {"neddf_mesh_simplify_keys", "neddf_mesh_simplify_clusters", "neddf_mesh_simplify_pairs", "neddf_mesh_simplify_place",
           "neddf_mesh_simplify_attributes", "neddf_mesh_simplify_triangles", "neddf_mesh_simplify_unique"}
    assert new <= names
    lib = _lib.load()
    for n in new:
        assert hasattr(lib, n), n
    from neddf_amd.mesh import simplify_grid, simplify_mesh
    from neddf_amd import NeddfError
    assert simplify_grid([0, 0, 0], [1, 2, 0], cell=0.5) == (2, 4, 1) == sc.grid_cells([0, 0, 0], [1, 2, 0], 0.5)
    for bad in (dict(), dict(cell=0.5, cells=(1, 1, 1)), dict(cell=1e-4), dict(cells=(0, 1, 1)), dict(cells=(1, 1, 1025)), dict(cell=-1.0)):
        with pytest.raises(NeddfError):
            simplify_grid([0, 0, 0], [1, 1, 1], **bad)
    import torch
    with pytest.raises(NeddfError):                      # no CPU fallback
        simplify_mesh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), cells=(1, 1, 1))
