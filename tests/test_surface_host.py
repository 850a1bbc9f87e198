"""Surface normals on the CPU: the additive C ABI (still version 7), the PLY writer's normal / colour properties, the numpy restatement of
the geometric vertex normals on analytic surfaces, and the new command-line flags."""
import os
import re
import subprocess

import numpy as np
import pytest

import mesh_check as mc
import surface_check as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("neddf_field_forward_surface", "neddf_composite_normal", "neddf_render_rays_surface", "neddf_render_rays_single_surface",
               "neddf_mesh_vertex_normals")


def test_abi_is_additive():
    from neddf_amd import _lib
    header = open(os.path.join(ROOT, "include", "neddf_hip.h")).read()
    assert "#define NEDDF_ABI_VERSION 7" in header and _lib.ABI_VERSION == 7
    names = [s[0] for s in _lib.SYMBOLS]
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert names.count(name) == 1, name
        assert re.search(r" T %s$" % name, exported, re.M), name
    # (tests/test_host.py calls every entry of SYMBOLS with a NULL context and expects NEDDF_EINVAL: the new ones are in that loop)


def _read_ply(path):
    """A reader of the writer's format, written here: header properties -> structured vertex array, faces."""
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = int([l for l in lines if l.startswith("element vertex")][0].split()[-1])
    nf = int([l for l in lines if l.startswith("element face")][0].split()[-1])
    i0 = [i for i, l in enumerate(lines) if l.startswith("element vertex")][0]
    i1 = [i for i, l in enumerate(lines) if l.startswith("element face")][0]
    props = [l.split()[1:] for l in lines[i0 + 1:i1]]
    dt = np.dtype([(name, {"float": "<f4", "uchar": "u1"}[ty]) for ty, name in props])
    verts = np.frombuffer(body[:nv * dt.itemsize], dtype=dt)
    faces = np.frombuffer(body[nv * dt.itemsize:], dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    assert len(faces) == nf and (faces["n"] == 3).all()
    return [p[1] for p in props], verts, faces["i"]


def test_write_ply_options(tmp_path):
    from neddf_amd.mesh import write_ply
    rng = np.random.default_rng(3)
    v = rng.standard_normal((7, 3)).astype(np.float32)
    t = rng.integers(0, 7, (5, 3)).astype(np.int32)
    n = rng.standard_normal((7, 3)).astype(np.float32)
    # B, G, R floats whose 255-fold is EXACTLY a half (checked below), below 0, above 1, and plain values
    c = np.array([[0.5, 1.5, 2.5], [3.5, 254.5, 253.5], [-20.0, 300.0, 127.0], [0.0, 255.0, 128.0], [10.2, 10.7, 10.5],
                  [1.0, 2.0, 3.0], [100.49, 100.51, 100.5]]) / 255.0
    half = np.array([[0, 2, 2], [4, 254, 254], [0, 255, 127], [0, 255, 128], [10, 11, 10], [1, 2, 3], [100, 101, 100]])
    exact = (c * 255.0 * 2 == np.round(c * 255.0 * 2))
    want_rgb = np.clip(np.rint(c * 255.0), 0, 255).astype(np.uint8)[:, ::-1]
    assert np.array_equal(np.where(exact, half, want_rgb[:, ::-1]), want_rgb[:, ::-1])       # half to even wherever the half is exact
    assert exact[0].all(), "the hand-made halves must be exact in float64"
    # without options: the bytes of the documented layout, assembled here
    plain = write_ply(tmp_path / "plain.ply", v, t)
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty float x\nproperty float y\nproperty float z\n"
            "element face 5\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")
    faces = b"".join(b"\x03" + row.astype("<i4").tobytes() for row in t)
    assert open(plain, "rb").read() == head + v.astype("<f4").tobytes() + faces
    assert open(write_ply(tmp_path / "none.ply", v, t, normals=None, colors=None), "rb").read() == head + v.tobytes() + faces
    rv, rt = mc.read_ply(plain)
    assert np.array_equal(rv, v) and np.array_equal(rt, t)
    for kw, names in ((dict(normals=n), ["x", "y", "z", "nx", "ny", "nz"]),
                      (dict(colors=c), ["x", "y", "z", "red", "green", "blue"]),
                      (dict(normals=n, colors=c), ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"])):
        got_names, verts, tris = _read_ply(write_ply(tmp_path / "o.ply", v, t, **kw))
        assert got_names == names
        assert np.array_equal(np.stack([verts[k] for k in "xyz"], 1), v) and np.array_equal(tris, t)
        if "normals" in kw:
            assert np.array_equal(np.stack([verts[k] for k in ("nx", "ny", "nz")], 1), n)
        if "colors" in kw:
            assert np.array_equal(np.stack([verts[k] for k in ("red", "green", "blue")], 1), want_rgb)     # B, G, R in -> R, G, B out
    with pytest.raises(ValueError):
        write_ply(tmp_path / "bad.ply", v, t, normals=n[:3])


def _grid(n, lo=-1.0, hi=1.0):
    x = np.linspace(lo, hi, n)
    z, y, x = np.meshgrid(x, x, x, indexing="ij")
    return x, y, z


def _analytic_cases():
    n, r = 64, 0.6
    x, y, z = _grid(n)
    v, t = mc.marching_cubes((np.sqrt(x * x + y * y + z * z) - r).astype(np.float32), 0.0)
    p = v.astype(np.float64)
    yield "sphere", v, t, p / np.linalg.norm(p, axis=1, keepdims=True), 2.0 / (n - 1), r
    n, R, r = 48, 0.5, 0.2
    x, y, z = _grid(n)
    v, t = mc.marching_cubes((np.sqrt((np.sqrt(x * x + y * y) - R) ** 2 + z * z) - r).astype(np.float32), 0.0)
    p = v.astype(np.float64)
    q = np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2)
    g = np.stack([(q - R) * p[:, 0] / q, (q - R) * p[:, 1] / q, p[:, 2]], 1)
    # smallest radius of curvature of the torus: the tube radius r (the inner equator's other principal radius is R - r = 0.3 > r)
    yield "torus", v, t, g / np.linalg.norm(g, axis=1, keepdims=True), 2.0 / (n - 1), r


@pytest.mark.parametrize("case", list(_analytic_cases()), ids=lambda c: c[0])
def test_geometric_normals_on_analytic_surfaces(case):
    name, v, t, want, h, r = case
    n64 = sc.vertex_normals(v, t, np.float64)
    n32 = sc.vertex_normals(v, t, np.float32).astype(np.float64)
    assert np.abs(np.linalg.norm(n64, axis=1) - 1).max() < 1e-12 and np.abs(np.linalg.norm(n32, axis=1) - 1).max() < 1e-6
    cos64, cos32 = (n64 * want).sum(1), (n32 * want).sum(1)
    worst = float(np.arccos(np.clip(cos64, -1, 1)).max())
    bound = float(np.arcsin(h / r))          # first-order facet bound: a facet of size h on a surface of curvature radius r turns by h / r
    print("%s: %d vertices, fp64 restatement max angle %.4f rad (bound arcsin(h / r) = %.4f), fp32 - fp64 cosine min %.2e"
          % (name, len(v), worst, bound, float((cos32 - cos64).min())))
    assert worst <= bound, (name, worst, bound)
    # fp32 against the bound the fp64 restatement sets on the same mesh, per vertex.  Margin 1e-4 in cosine: the fp32 cross product of
    # two edges of length ~h carries a relative error of a few 2^-24 of |a||b|, i.e. an angle error of order 1e-6 rad on a triangle that
    # is not a sliver, and slivers carry little weight in an area-weighted sum; a cosine moves by sin(angle) * 1e-6 + 1e-12, below
    # 1e-6 for the angles allowed here.  1e-4 leaves two orders of magnitude for the slivers' share.
    assert (cos32 >= cos64 - 1e-4).all(), (name, float((cos32 - cos64).min()))


def test_geometric_normal_rule_details():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [5, 5, 5]], np.float32)
    t = np.array([[0, 1, 2], [0, 2, 1], [1, 2, 3]], np.int32)        # the first two cancel at vertex 0; vertex 4 is in no triangle
    n = sc.vertex_normals(v, t)
    assert np.array_equal(n[0], [0, 0, 0]) and np.array_equal(n[4], [0, 0, 0])
    assert np.allclose(n[3], np.ones(3) / np.sqrt(3), atol=1e-7)
    big = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, 1], [0, 1, 0]], np.float32)
    tb = np.array([[0, 1, 2], [0, 4, 3]], np.int32)                  # areas 2 and 1/2 at vertex 0: weights 4 : 1
    assert np.allclose(sc.vertex_normals(big, tb)[0], np.array([1, 0, 4]) / np.sqrt(17), atol=1e-7)


def test_script_flags_default_off():
    from neddf_amd.scripts import extract_mesh, run_eval
    a = extract_mesh.build_parser().parse_args(["run"])
    assert a.normals is None and a.colors is False
    assert extract_mesh.build_parser().parse_args(["run", "--normals"]).normals == "auto"
    assert extract_mesh.build_parser().parse_args(["run", "--normals", "geometric", "--colors"]).normals == "geometric"
    with pytest.raises(SystemExit):
        extract_mesh.build_parser().parse_args(["run", "--normals", "smooth"])
    assert run_eval.build_parser().parse_args(["run"]).normals is False
    assert run_eval.build_parser().parse_args(["run", "--normals"]).normals is True


def test_python_surface_defaults():
    import inspect
    from neddf_amd import NeDDF, NeRF, NeRFRender
    from neddf_amd.mesh import write_ply
    sig = inspect.signature(NeDDF.extract_mesh).parameters
    assert sig["normals"].default is False and sig["colors"].default is False
    assert inspect.signature(write_ply).parameters["normals"].default is None
    assert inspect.signature(NeRFRender.render_image_single_pass).parameters["normals"].default is False
    assert NeRFRender.normal_output is False
    assert hasattr(NeDDF, "forward_surface") and not NeRF()._has_surface()
