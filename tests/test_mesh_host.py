"""Surface extraction on the CPU: the marching-cubes case tables through the numpy restatement (tests/mesh_check.py) on
analytic fields, the committed table header against its generator, and the PLY writer."""
import importlib.util
import os

import numpy as np
import pytest

import mesh_check as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grid(n, lo=-1.0, hi=1.0):
    x = np.linspace(lo, hi, n)
    z, y, x = np.meshgrid(x, x, x, indexing="ij")      # [nz, ny, nx]
    return x, y, z


def test_table_header_is_the_generator_output():
    spec = importlib.util.spec_from_file_location("gen_mc_tables", os.path.join(ROOT, "tools", "gen_mc_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert open(mc.TABLES_H).read() == gen.header()
    edge, tri = gen.tables()
    assert edge[1] == 0x109 and edge[255] == 0 and edge[0] == 0        # Bourke's edge table
    assert np.array_equal(mc.EDGE_TABLE, edge)
    for c in range(256):                                                # the triangles use exactly the crossed edges
        used = {int(e) for e in mc.TRI_TABLE[c] if e >= 0}
        assert used == {e for e in range(12) if edge[c] >> e & 1}, c


def test_sphere_is_a_closed_outward_sphere():
    n, r = 64, 0.6
    x, y, z = _grid(n)
    v, t = mc.marching_cubes((np.sqrt(x * x + y * y + z * z) - r).astype(np.float32), 0.0)
    assert v.dtype == np.float32 and t.dtype == np.int32 and v.shape[1] == 3 and t.shape[1] == 3
    und, dire = mc.edge_counts(t)
    assert (und == 2).all() and (dire == 1).all()
    assert mc.euler_characteristic(v, t) == 2
    vol = mc.signed_volume(v, t)
    assert 0 < vol and abs(vol - 4 / 3 * np.pi * r ** 3) < 0.01 * vol
    h = 2.0 / (n - 1)
    assert np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - r).max() < 0.02 * h


def test_torus_has_euler_characteristic_zero():
    x, y, z = _grid(48)
    f = np.sqrt((np.sqrt(x * x + y * y) - 0.5) ** 2 + z * z) - 0.2
    v, t = mc.marching_cubes(f.astype(np.float32), 0.0)
    assert mc.closed_and_oriented(t) and mc.euler_characteristic(v, t) == 0 and mc.signed_volume(v, t) > 0


@pytest.mark.parametrize("kind", ["normal", "ternary"])
def test_random_volumes_are_closed_and_oriented(kind):
    """Volumes whose boundary layer is outside: every case of the table and every ambiguous face occurs; a crack or a
    flipped case breaks closure or orientation."""
    rng = np.random.default_rng(7 if kind == "normal" else 8)
    seen = set()
    for _ in range(60):
        shape = tuple(int(s) for s in rng.integers(3, 12, 3))
        vol = rng.standard_normal(shape) if kind == "normal" else rng.integers(-1, 2, shape).astype(np.float64)
        vol[[0, -1]] = 1
        vol[:, [0, -1]] = 1
        vol[:, :, [0, -1]] = 1
        v, t = mc.marching_cubes(vol.astype(np.float32), 0.0)
        if not len(t):
            continue
        assert mc.closed_and_oriented(t)
        assert mc.signed_volume(v, t) > 0
        ins = vol < 0
        c = sum(ins[(slice(dz, ins.shape[0] - 1 + dz),) + (slice(dy, ins.shape[1] - 1 + dy),) + (slice(dx, ins.shape[2] - 1 + dx),)]
                .astype(int) << b for b, (dx, dy, dz) in enumerate([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0),
                                                                    (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]))
        seen |= set(np.unique(c).tolist())
    assert len(seen) > 200, len(seen)


def test_write_ply_round_trip(tmp_path):
    from neddf_amd.mesh import write_ply
    rng = np.random.default_rng(3)
    v = rng.standard_normal((17, 3)).astype(np.float32)
    t = rng.integers(0, 17, (29, 3)).astype(np.int32)
    path = write_ply(tmp_path / "m.ply", v, t)
    head = open(path, "rb").read(300).split(b"end_header\n")[0].decode()
    assert "format binary_little_endian 1.0" in head and "element vertex 17" in head and "element face 29" in head
    rv, rt = mc.read_ply(path)
    assert np.array_equal(rv.view(np.int32), v.view(np.int32)) and np.array_equal(rt, t)
    write_ply(tmp_path / "e.ply", np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    ev, et = mc.read_ply(tmp_path / "e.ply")
    assert ev.shape == (0, 3) and et.shape == (0, 3)
    with pytest.raises(ValueError):
        write_ply(tmp_path / "bad.ply", v[:, :2], t)


def test_marching_cubes_refuses_host_tensors():
    import torch
    from neddf_amd import NeddfError
    from neddf_amd.mesh import marching_cubes
    with pytest.raises(NeddfError, match="HIP device"):
        marching_cubes(torch.zeros(4, 4, 4), 0.0)
    with pytest.raises(NeddfError, match="HIP device"):
        marching_cubes(np.zeros((4, 4, 4), np.float32), 0.0)
