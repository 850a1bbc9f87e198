"""Mesh clean-up without a GPU: the host restatement (tests/mesh_clean_check.py) on marching-cubes meshes whose component counts
are known, a hand-made mesh with every irregular entry checked one by one, and the host side of the public interface."""
import numpy as np
import pytest
import torch

import mesh_check as mc
import mesh_clean_check as cc


@pytest.fixture(scope="module")
def meshes():
    return {name: mc.marching_cubes(vol, iso, lo, hi) for name, (vol, iso, lo, hi) in cc.volumes().items()}


def _components(mesh):
    v, t = mesh
    vl, tl, sizes = cc.connected_components(t, len(v))
    assert vl.dtype == np.int32 and tl.dtype == np.int32 and sizes.dtype == np.int64
    assert sizes.sum() == len(t) and (np.bincount(tl, minlength=len(sizes)) == sizes).all()
    # numbered by lowest vertex index: the first vertex of every component, in label order, ascends
    first = [int(np.nonzero(vl == c)[0][0]) for c in range(len(sizes))]
    assert first == sorted(first)
    return vl, tl, sizes


def test_floaters(meshes):
    v, t = meshes["floaters"]
    assert (len(v), len(t)) == (1594, 3168)
    _, _, sizes = _components(meshes["floaters"])
    assert sorted(sizes.tolist()) == [8, 48, 144, 160, 2808]          # one of the two smallest spheres falls between lattice points
    ov, ot, vmap = cc.remove_small_components(v, t, min_triangles=64)
    assert sorted(_components((ov, ot))[2].tolist()) == [144, 160, 2808]
    ov, ot, vmap = cc.remove_small_components(v, t, keep_largest=1)
    assert _components((ov, ot))[2].tolist() == [2808]
    assert mc.closed_and_oriented(ot) and mc.euler_characteristic(ov, ot) == 2
    assert (vmap >= 0).sum() == len(ov) and np.array_equal(ov.view(np.int32), v.view(np.int32)[vmap >= 0])


def test_random(meshes):
    v, t = meshes["random"]
    assert (len(v), len(t)) == (2697, 4937)
    _, _, sizes = _components(meshes["random"])
    assert len(sizes) == 18 and sizes.max() == 4849
    rest = np.sort(sizes)[:-1]
    assert rest.min() == 2 and rest.max() == 10                       # open shreds at the cube's faces
    ov, ot, _ = cc.remove_small_components(v, t, min_triangles=9, keep_largest=3)
    assert sorted(_components((ov, ot))[2].tolist()) == [10, 4849]    # the three largest are 4849, 10 and an 8: the 8 misses the minimum


def test_twins_tie_goes_to_the_lower_label(meshes):
    v, t = meshes["twins"]
    assert (len(v), len(t)) == (416, 824)
    vl, _, sizes = _components(meshes["twins"])
    assert sizes.tolist() == [412, 412]
    assert cc.select_components(sizes, keep_largest=1).tolist() == [True, False]
    ov, ot, _ = cc.remove_small_components(v, t, keep_largest=1)
    assert len(ot) == 412 and (ov[:, 0] < 0).all()                    # label 0 is the sphere at x < 0
    assert (v[vl == 0, 0] < 0).all() and (v[vl == 1, 0] > 0).all()


def test_helix_is_one_closed_component(meshes):
    v, t = meshes["helix"]
    assert (len(v), len(t)) == (7192, 14380)
    vl, tl, sizes = _components(meshes["helix"])
    assert sizes.tolist() == [14380] and (vl == 0).all() and (tl == 0).all()
    assert mc.closed_and_oriented(t) and mc.euler_characteristic(v, t) == 2


def test_hand_made_mesh_entry_by_entry():
    v, t = cc.hand_made()
    vl, tl, sizes = cc.connected_components(t, len(v))
    assert vl.tolist() == [0, 0, 0, -1, 1, 1, 1]                      # vertex 3: only an invalid triangle names it
    assert tl.tolist() == [1, 0, -1, 0, -1, 0, 1, 1]                  # index V and index -1 are ignored; (2, 2, 1) and (5, 5, 5) count
    assert sizes.tolist() == [3, 3]                                   # the duplicate counts twice
    ov, ot, vmap = cc.compact_mesh(v, t, [1, 1, 1, 1, 1, 0, 1, 1])
    assert vmap.tolist() == [0, 1, 2, -1, 3, 4, 5]
    assert ot.tolist() == [[3, 4, 5], [0, 1, 2], [2, 2, 1], [5, 4, 3], [4, 4, 4]]
    assert np.array_equal(ov.view(np.int32), v.view(np.int32)[[0, 1, 2, 4, 5, 6]]) and ov.view(np.int32)[0, 1] == 0x7fc01234
    ov, ot, vmap = cc.compact_mesh(v, t, [1, 0, 0, 0, 0, 0, 0, 1])
    assert vmap.tolist() == [-1, -1, -1, -1, 0, 1, 2] and ot.tolist() == [[0, 1, 2], [1, 1, 1]] and len(ov) == 3
    ov, ot, vmap = cc.compact_mesh(v, t, np.zeros(8))
    assert ov.shape == (0, 3) and ot.shape == (0, 3) and (vmap == -1).all()
    ov, ot, vmap = cc.remove_small_components(v, t, keep_largest=1)   # 3 against 3: the lower label stays
    assert vmap.tolist() == [0, 1, 2, -1, -1, -1, -1] and ot.tolist() == [[0, 1, 2], [2, 2, 1], [0, 1, 2]]
    e = cc.connected_components(np.zeros((0, 3), np.int32), 5)
    assert e[0].tolist() == [-1] * 5 and len(e[1]) == 0 and len(e[2]) == 0
    e = cc.connected_components(np.zeros((2, 3), np.int32), 0)
    assert len(e[0]) == 0 and e[1].tolist() == [-1, -1] and len(e[2]) == 0


def test_selection_in_torch_equals_the_checker():
    """mesh.select_components (the [C]-sized choice, torch) against the numpy one, ties included."""
    from neddf_amd.mesh import select_components
    rng = np.random.default_rng(0)
    for n in (0, 1, 2, 7, 40):
        sizes = rng.integers(1, 6, n).astype(np.int64)
        for m, k in ((0, 0), (3, 0), (0, 1), (0, 2), (2, 3), (0, 100), (6, 1)):
            got = select_components(torch.from_numpy(sizes), m, k).numpy()
            assert np.array_equal(got, cc.select_components(sizes, m, k)), (sizes, m, k)


def test_clean_up_refuses_host_tensors():
    from neddf_amd import NeddfError
    from neddf_amd.mesh import compact_mesh, connected_components, remove_small_components
    v, t = cc.hand_made()
    with pytest.raises(NeddfError, match="HIP device"):
        connected_components(torch.from_numpy(t), len(v))
    with pytest.raises(NeddfError, match="HIP device"):
        connected_components(t, len(v))
    with pytest.raises(NeddfError, match="HIP device"):
        remove_small_components(torch.from_numpy(v), torch.from_numpy(t), min_triangles=2)
    with pytest.raises(NeddfError, match="HIP device"):
        compact_mesh(torch.from_numpy(v), torch.from_numpy(t), torch.ones(len(t), dtype=torch.uint8))


def test_parser_accepts_the_clean_up_flags():
    from neddf_amd.scripts.extract_mesh import build_parser
    p = build_parser()
    a = p.parse_args(["run"])
    assert (a.min_component, a.keep_largest) == (0, 0)
    a = p.parse_args(["run", "--keep-largest", "--normals"])
    assert a.keep_largest == 1 and a.normals == "auto" and a.min_component == 0
    a = p.parse_args(["run", "--keep-largest", "3", "--min-component", "64"])
    assert (a.min_component, a.keep_largest) == (64, 3)


def test_abi_stays_and_the_symbols_are_bound():
    import inspect
    import neddf_amd.mesh as mesh
    from neddf_amd import _lib
    from neddf_amd.network import BaseNeuralField
    assert _lib.ABI_VERSION == 7
    names = [s[0] for s in _lib.SYMBOLS]
    assert "neddf_mesh_components" in names and "neddf_mesh_compact" in names
    lib = _lib.load()
    assert lib.neddf_abi_version() == 7
    assert lib.neddf_mesh_components(None, None, 0, 0, None, None, None, None, None) == -1
    assert lib.neddf_mesh_compact(None, None, 0, None, 0, None, None, 0, None, 0, None, None, None, None) == -1
    assert {"connected_components", "compact_mesh", "remove_small_components"} <= set(mesh.__all__)
    sig = inspect.signature(BaseNeuralField.extract_mesh).parameters
    assert sig["min_component_triangles"].default == 0 and sig["keep_largest"].default == 0
