"""Mesh clean-up on the GPU: neddf_mesh_components and neddf_mesh_compact against the host restatement
(tests/mesh_clean_check.py) exactly -- every result is an integer or a copied bit pattern -- on marching-cubes meshes with
floaters, shreds, a tie, a long tube and no triangles at all, a hand-made irregular mesh, triangle strips that end at the edges of a
wave and of a workgroup, the two-call protocol, the guard bands, extract_mesh's clean-up options on the shipped bunny and neddf/scripts/extract_mesh.py end to end."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from conftest import GOLDEN

import mesh_check as mc
import mesh_clean_check as cc

pytestmark = pytest.mark.gpu

SELECTIONS = ((64, 0), (0, 1), (0, 2), (9, 3))           # (min_triangles, keep_largest)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bunny(dev):
    from neddf_amd import NeDDF
    from neddf_amd.fixtures import BUNNY_SMOKE_CFG, bunny_smoke_weights
    net = NeDDF(**BUNNY_SMOKE_CFG)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in bunny_smoke_weights().items()})
    net.to(dev)
    net.set_iter(-1)
    for p in net.parameters():
        p.requires_grad_(False)
    return net


def _cases():
    out = dict(cc.volumes())
    rng = np.random.default_rng(5)
    rng.standard_normal((17, 9, 13))                    # the draws of tests/test_gpu_mesh.py before its 2x2x2 volume
    out["2x2x2"] = (rng.standard_normal((2, 2, 2)).astype(np.float32), 0.0, (-1, -1, -1), (1, 1, 1))
    out["all_outside"] = (np.ones((5, 6, 7), np.float32), 0.0, (-1, -1, -1), (1, 1, 1))
    return out


@pytest.fixture(scope="module")
def meshes(dev):
    """name -> (vertices, triangles) on the device, from the GPU's marching cubes (pinned bit for bit by tests/test_gpu_mesh.py)."""
    from neddf_amd.mesh import marching_cubes
    return {name: marching_cubes(torch.from_numpy(vol).to(dev), iso, lo, hi) for name, (vol, iso, lo, hi) in _cases().items()}


def N(t):
    return t.cpu().numpy()


def _same_components(got, want, what):
    for g, w, part in zip(got, want, ("vertex labels", "triangle labels", "component sizes")):
        g = N(g)
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, part)


def _same_compaction(got, want, what):
    gv, gt, gm = (N(a) for a in got)
    wv, wt, wm = want
    assert gv.dtype == np.float32 and gt.dtype == np.int32 and gm.dtype == np.int32, what
    assert gt.shape == wt.shape and np.array_equal(gt, wt), (what, gt.shape, wt.shape)
    assert gv.shape == wv.shape and np.array_equal(gv.view(np.int32), wv.view(np.int32)), what      # bit for bit (NaN-safe)
    assert gm.shape == wm.shape and np.array_equal(gm, wm), what


@pytest.mark.parametrize("name", ["floaters", "random", "twins", "helix", "2x2x2", "all_outside"])
def test_components_and_removal_match_the_checker(dev, meshes, name):
    from neddf_amd import Context
    from neddf_amd.mesh import connected_components, remove_small_components
    v, t = meshes[name]
    vn, tn = N(v), N(t)
    want = cc.connected_components(tn, len(vn))
    got = connected_components(t, len(v))
    print("%s: %d vertices, %d triangles, %d components, %d union-find rounds"
          % (name, len(vn), len(tn), len(want[2]), Context.get(dev).mesh_components_rounds()))
    _same_components(got, want, name)
    if name == "all_outside":
        assert len(tn) == 0 and len(want[2]) == 0
    if name == "helix":
        assert want[2].tolist() == [14380]
    for m, k in SELECTIONS:
        _same_compaction(remove_small_components(v, t, m, k), cc.remove_small_components(vn, tn, m, k), (name, m, k))
    if name == "twins":
        ov = N(remove_small_components(v, t, keep_largest=1)[0])
        assert len(ov) and (ov[:, 0] < 0).all()          # the tie goes to label 0, the sphere at x < 0


@pytest.mark.parametrize("name", ["helix", "random"])
def test_results_do_not_depend_on_the_run(meshes, name):
    from neddf_amd.mesh import connected_components, remove_small_components
    v, t = meshes[name]
    a, b = connected_components(t, len(v)), connected_components(t, len(v))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    a, b = remove_small_components(v, t, 9, 3), remove_small_components(v, t, 9, 3)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_hand_made_mesh(dev):
    """Unreferenced vertex, indices V and -1, a degenerate and a duplicated triangle, a NaN with a payload; int64 triangles and a
    bool mask are converted; more than one workgroup of isolated triangles (every third vertex unused)."""
    from neddf_amd.mesh import compact_mesh, connected_components, remove_small_components
    vn, tn = cc.hand_made()
    v, t = torch.from_numpy(vn).to(dev), torch.from_numpy(tn).to(dev)
    got = connected_components(t, len(v))
    assert N(got[0]).tolist() == [0, 0, 0, -1, 1, 1, 1] and N(got[1]).tolist() == [1, 0, -1, 0, -1, 0, 1, 1] and N(got[2]).tolist() == [3, 3]
    _same_components(connected_components(t.long(), len(v)), cc.connected_components(tn, len(vn)), "int64 triangles")
    keep = np.array([1, 1, 1, 1, 1, 0, 1, 1], np.uint8)
    got = compact_mesh(v, t, torch.from_numpy(keep).to(dev))
    _same_compaction(got, cc.compact_mesh(vn, tn, keep), "hand-made")
    assert N(got[2]).tolist() == [0, 1, 2, -1, 3, 4, 5] and N(got[0]).view(np.int32)[0, 1] == 0x7fc01234
    _same_compaction(compact_mesh(v, t, torch.from_numpy(keep.astype(bool)).to(dev)), cc.compact_mesh(vn, tn, keep), "bool mask")
    _same_compaction(remove_small_components(v, t, keep_largest=1), cc.remove_small_components(vn, tn, keep_largest=1), "tie")
    _same_components(connected_components(t[:0], 5), cc.connected_components(tn[:0], 5), "no triangles")
    _same_components(connected_components(t, 0), cc.connected_components(tn, 0), "no vertices")
    _same_compaction(compact_mesh(v[:0], t, torch.ones(len(t), device=dev, dtype=torch.uint8)),
                     cc.compact_mesh(vn[:0], tn, np.ones(len(tn))), "no vertices")
    # 700 separate triangles over 2800 vertices, every fourth vertex unused, in a shuffled order: many components, several workgroups
    rng = np.random.default_rng(3)
    base = np.arange(700, dtype=np.int32)[:, None] * 4 + np.array([[0, 1, 2]], np.int32)
    tn = base[rng.permutation(700)]
    tn[::7, 2] = tn[::7, 0] + 4 * (np.arange(len(tn[::7])) % 3 == 0)             # some join their neighbour, some degenerate
    tn = np.minimum(tn, 2799).astype(np.int32)
    vn = rng.standard_normal((2800, 3)).astype(np.float32)
    v, t = torch.from_numpy(vn).to(dev), torch.from_numpy(tn).to(dev)
    _same_components(connected_components(t, len(v)), cc.connected_components(tn, len(vn)), "isolated triangles")
    keep = rng.random(700) < 0.5
    _same_compaction(compact_mesh(v, t, torch.from_numpy(keep).to(dev)), cc.compact_mesh(vn, tn, keep), "isolated triangles")
    _same_compaction(remove_small_components(v, t, 2, 0), cc.remove_small_components(vn, tn, 2, 0), "isolated triangles")


def _strip(V):
    """A triangle strip over V vertices built on the host: triangle i = (i, i + 1, i + 2), T = V - 2; vertex 0 carries a NaN payload."""
    v = np.random.default_rng(V).standard_normal((V, 3)).astype(np.float32)
    v.view(np.int32)[0, 1] = 0x7fc01234
    t = (np.arange(V - 2, dtype=np.int32)[:, None] + np.arange(3, dtype=np.int32)[None, :]).astype(np.int32)
    return v, t


def _strip_masks(T):
    every_other = np.zeros(T, np.uint8)
    every_other[::2] = 1
    last = np.zeros(T, np.uint8)
    last[-1] = 1
    every_fourth = np.zeros(T, np.uint8)            # leaves every fourth vertex unused: a vertex's rank differs from its index
    every_fourth[::4] = 1
    return {"all": np.ones(T, np.uint8), "none": np.zeros(T, np.uint8), "every other": every_other, "only the last": last,
            "every fourth": every_fourth}


@pytest.mark.parametrize("V", [63, 64, 65, 255, 256, 257, 1025])
def test_strip_ranks_across_waves_and_workgroups(dev, V):
    """The kernels that place by rank inside the workgroup (cc_root_label, compact_vertex, compact_triangle) at the edges of a wave
    (64 lanes) and of a workgroup (256 threads): kept elements that end or begin exactly there, none, all, and a single one in the
    last workgroup.  Every result against tests/mesh_clean_check.py bit for bit.  A strip is one component (one root); every
    fourth and every third triangle alone give separate components with roots in every wave."""
    from neddf_amd.mesh import compact_mesh, connected_components
    vn, tn = _strip(V)
    v, t = torch.from_numpy(vn).to(dev), torch.from_numpy(tn).to(dev)
    for name, keep in _strip_masks(len(tn)).items():
        what = ("strip", V, name)
        _same_compaction(compact_mesh(v, t, torch.from_numpy(keep).to(dev)), cc.compact_mesh(vn, tn, keep), what)
        sub = np.ascontiguousarray(tn[keep != 0])
        _same_components(connected_components(torch.from_numpy(sub).to(dev), V), cc.connected_components(sub, V), what)
    sub = np.ascontiguousarray(tn[::3])
    want = cc.connected_components(sub, V)
    assert len(want[2]) == len(sub) == (V - 2 + 2) // 3
    _same_components(connected_components(torch.from_numpy(sub).to(dev), V), want, ("strip", V, "every third"))


def test_compact_two_call_protocol_and_errors(dev, meshes):
    from neddf_amd import Context
    ctx = Context.get(dev)
    v, t = meshes["floaters"]
    vn, tn = N(v), N(t)
    V, T = len(vn), len(tn)
    rng = np.random.default_rng(1)
    keep_n = (rng.random(T) < 0.4).astype(np.uint8)
    keep = torch.from_numpy(keep_n).to(dev)
    wv, wt, wm = cc.compact_mesh(vn, tn, keep_n)
    assert 0 < len(wt) < T and 0 < len(wv) < V
    s = ctx.stream()
    nv, nt = C.c_int64(-1), C.c_int64(-1)
    P = lambda x, off=0: C.c_void_p(x.data_ptr() + off)          # noqa: E731
    fn = ctx.lib.neddf_mesh_compact
    pad = 64                                                    # sentinel words around every output
    ov = torch.full((len(wv) * 3 + 2 * pad,), -7.0, device=dev)
    ot = torch.full((len(wt) * 3 + 2 * pad,), -7, device=dev, dtype=torch.int32)
    om = torch.full((V + 2 * pad,), -7, device=dev, dtype=torch.int32)
    args = (ctx.h, P(v), V, P(t), T, P(keep))
    assert fn(*args, None, 0, None, 0, None, C.byref(nv), C.byref(nt), s) == 0               # NULL outputs: the counts only
    assert (nv.value, nt.value) == (len(wv), len(wt))
    for ptr_v, cap_v, ptr_t, cap_t in ((P(ov, 4 * pad), len(wv) - 1, P(ot, 4 * pad), len(wt)), (P(ov, 4 * pad), len(wv), P(ot, 4 * pad), len(wt) - 1),
                                       (None, len(wv), P(ot, 4 * pad), len(wt)), (P(ov, 4 * pad), len(wv), None, len(wt))):
        nv.value = nt.value = -1
        assert fn(*args, ptr_v, cap_v, ptr_t, cap_t, P(om, 4 * pad), C.byref(nv), C.byref(nt), s) == 0
        assert (nv.value, nt.value) == (len(wv), len(wt))
        torch.cuda.synchronize()
        assert (ov == -7).all() and (ot == -7).all() and (om == -7).all()                    # untouched
    assert fn(*args, P(ov, 4 * pad), len(wv), P(ot, 4 * pad), len(wt), P(om, 4 * pad), C.byref(nv), C.byref(nt), s) == 0
    torch.cuda.synchronize()
    _same_compaction((ov[pad:-pad].view(-1, 3), ot[pad:-pad].view(-1, 3), om[pad:-pad]), (wv, wt, wm), "exact caps")
    for buf in (ov, ot, om):
        assert (buf[:pad] == -7).all() and (buf[-pad:] == -7).all()                          # no word outside any output
    ot.fill_(-7)
    ov.fill_(-7.0)
    assert fn(*args, P(ov, 4 * pad), len(wv), P(ot, 4 * pad), len(wt), None, C.byref(nv), C.byref(nt), s) == 0          # no vertex map
    torch.cuda.synchronize()
    assert np.array_equal(N(ot[pad:-pad].view(-1, 3)), wt) and np.array_equal(N(ov[pad:-pad]).view(np.int32), wv.view(np.int32).reshape(-1))
    # all-one and all-zero masks
    ones, zeros = torch.ones(T, device=dev, dtype=torch.uint8), torch.zeros(T, device=dev, dtype=torch.uint8)
    assert fn(ctx.h, P(v), V, P(t), T, P(ones), None, 0, None, 0, None, C.byref(nv), C.byref(nt), s) == 0
    assert (nv.value, nt.value) == (V, T)
    fv, ft, fm = torch.empty_like(v), torch.empty_like(t), torch.empty(V, device=dev, dtype=torch.int32)
    assert fn(ctx.h, P(v), V, P(t), T, P(ones), P(fv), V, P(ft), T, P(fm), C.byref(nv), C.byref(nt), s) == 0
    torch.cuda.synchronize()
    assert torch.equal(fv.view(torch.int32), v.view(torch.int32)) and torch.equal(ft, t) and torch.equal(fm, torch.arange(V, device=dev, dtype=torch.int32))
    fm.fill_(-7)
    assert fn(ctx.h, P(v), V, P(t), T, P(zeros), P(fv), V, P(ft), T, P(fm), C.byref(nv), C.byref(nt), s) == 0
    torch.cuda.synchronize()
    assert (nv.value, nt.value) == (0, 0) and (fm == -1).all()
    # errors
    assert fn(ctx.h, P(v), -1, P(t), T, P(keep), None, 0, None, 0, None, C.byref(nv), C.byref(nt), s) == -1
    assert fn(ctx.h, P(v), V, P(t), -1, P(keep), None, 0, None, 0, None, C.byref(nv), C.byref(nt), s) == -1
    assert fn(ctx.h, P(v), V, P(t), T, None, None, 0, None, 0, None, C.byref(nv), C.byref(nt), s) == -1
    nc = C.c_int64(-1)
    lab = torch.empty(V, device=dev, dtype=torch.int32)
    siz = torch.empty(V, device=dev, dtype=torch.int64)
    assert ctx.lib.neddf_mesh_components(ctx.h, P(t), -1, V, P(lab), None, P(siz), C.byref(nc), s) == -1
    assert ctx.lib.neddf_mesh_components(ctx.h, P(t), T, -1, P(lab), None, P(siz), C.byref(nc), s) == -1
    assert ctx.lib.neddf_mesh_components(ctx.h, P(t), T, V, None, None, P(siz), C.byref(nc), s) == -1
    # sentinels around the labelling outputs; the triangle labels may be NULL; only the first C sizes are written
    lab = torch.full((V + 2 * pad,), -7, device=dev, dtype=torch.int32)
    tl = torch.full((T + 2 * pad,), -7, device=dev, dtype=torch.int32)
    siz = torch.full((V + 2 * pad,), -7, device=dev, dtype=torch.int64)
    assert ctx.lib.neddf_mesh_components(ctx.h, P(t), T, V, P(lab, 4 * pad), P(tl, 4 * pad), P(siz, 8 * pad), C.byref(nc), s) == 0
    torch.cuda.synchronize()
    want = cc.connected_components(tn, V)
    assert nc.value == len(want[2]) == 5
    _same_components((lab[pad:-pad], tl[pad:-pad], siz[pad:pad + 5]), want, "sentinels")
    assert (lab[:pad] == -7).all() and (lab[-pad:] == -7).all() and (tl[:pad] == -7).all() and (tl[-pad:] == -7).all()
    assert (siz[:pad] == -7).all() and (siz[pad + 5:] == -7).all()
    lab.fill_(-7)
    assert ctx.lib.neddf_mesh_components(ctx.h, P(t), T, V, P(lab, 4 * pad), None, P(siz, 8 * pad), C.byref(nc), s) == 0
    torch.cuda.synchronize()
    assert np.array_equal(N(lab[pad:-pad]), want[0]) and np.array_equal(N(siz[pad:pad + 5]), want[2])


def _gather_close(clean, plain, vmap, rtol, atol, what):
    """clean [V', 3] against plain [V, 3] gathered through vertex_map."""
    want = plain[vmap >= 0]
    assert clean.shape == want.shape, what
    over = float((np.abs(clean - want) - (atol + rtol * np.abs(want))).max()) if len(want) else 0.0
    assert over <= 0, (what, over)


@pytest.mark.parametrize("res,iso", [(48, 0.0275), (24, 0.1)])
def test_bunny_extract_mesh_keeps_the_largest_component(bunny, res, iso):
    """extract_mesh(keep_largest=1) = the checker applied to the plain call's mesh, bit for bit; normals and colours are computed on
    the cleaned mesh and agree with the plain call's gathered through vertex_map within tests/test_gpu_surface.py's tolerances for the
    same quantities (normals 1e-5 absolute, colours 1e-4 relative + 1e-5 absolute)."""
    v0, t0, n0, c0 = bunny.extract_mesh(threshold=iso, resolution=res, normals=True, colors=True)
    pv, pt = bunny.extract_mesh(threshold=iso, resolution=res)
    assert torch.equal(pv.view(torch.int32), v0.view(torch.int32)) and torch.equal(pt, t0)
    found = cc.connected_components(N(pt), len(pv))[2]
    wv, wt, wm = cc.remove_small_components(N(pv), N(pt), 0, 1)
    times = {}
    v, t = bunny.extract_mesh(threshold=iso, resolution=res, keep_largest=1, timings=times)
    print("bunny resolution %d threshold %g: %d vertices, %d triangles, %d components %s; kept %d triangles; clean-up %.3f ms"
          % (res, iso, len(pv), len(pt), len(found), sorted(found.tolist()), len(wt), times["clean"] * 1e3))
    assert np.array_equal(N(t), wt) and np.array_equal(N(v).view(np.int32), wv.view(np.int32))
    assert len(wt) and len(cc.connected_components(N(t), len(v))[2]) == 1
    assert (times["components"], times["components_kept"], times["triangles_removed"]) == (len(found), 1, len(pt) - len(wt))
    v1, t1, n1, c1 = bunny.extract_mesh(threshold=iso, resolution=res, normals=True, colors=True, keep_largest=1)
    assert torch.equal(v1.view(torch.int32), v.view(torch.int32)) and torch.equal(t1, t)
    assert n1.shape == v.shape and c1.shape == v.shape
    _gather_close(N(n1), N(n0), wm, 0.0, 1e-5, "normals")
    _gather_close(N(c1), N(c0), wm, 1e-4, 1e-5, "colours")
    # both options 0: nothing new runs, the outputs are the plain call's
    times = {}
    z = bunny.extract_mesh(threshold=iso, resolution=res, normals=True, colors=True, min_component_triangles=0, keep_largest=0, timings=times)
    assert "clean" not in times
    for a, b in zip(z, (v0, t0, n0, c0)):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))
    wv, wt, _ = cc.remove_small_components(N(pv), N(pt), 64, 0)
    v, t = bunny.extract_mesh(threshold=iso, resolution=res, min_component_triangles=64)
    assert np.array_equal(N(t), wt) and np.array_equal(N(v).view(np.int32), wv.view(np.int32))


def test_extract_mesh_script_keep_largest(dev, bunny, tmp_path, capsys):
    import yaml
    from neddf_amd.fixtures import BUNNY_SMOKE_CFG, bunny_smoke_weights
    from neddf_amd.scripts.extract_mesh import main
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
    path = main([str(run), "--epoch", "7", "--resolution", "24", "--threshold", "0.1", "--keep-largest", "--normals"])
    out = capsys.readouterr().out
    assert path == (run / "mesh" / "mesh_24_threshold0.1.ply").resolve() and path.is_file()
    assert "vertices: " in out and "grid evaluation: " in out and "marching cubes: " in out
    line = [ln for ln in out.splitlines() if ln.startswith("components: ")]
    assert len(line) == 1 and " found, 1 kept, triangles removed: " in line[0] and "clean-up: " in line[0]
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    assert b"property float nx" in head
    nv = int([ln for ln in head.decode().splitlines() if ln.startswith("element vertex")][0].split()[2])
    nf = int([ln for ln in head.decode().splitlines() if ln.startswith("element face")][0].split()[2])
    rec = np.frombuffer(body[:nv * 24], dtype=np.dtype([("p", "<f4", (3,)), ("n", "<f4", (3,))]))
    faces = np.frombuffer(body[nv * 24:], dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    assert len(faces) == nf and nf > 0
    assert len(cc.connected_components(faces["i"], nv)[2]) == 1
    v, t, n = bunny.extract_mesh(threshold=0.1, resolution=24, normals=True, keep_largest=1)
    assert np.array_equal(rec["p"], N(v)) and np.array_equal(faces["i"], N(t)) and np.array_equal(rec["n"], N(n))
    # without --normals the file is the plain one mesh_check.read_ply reads
    path = main([str(run), "--epoch", "7", "--resolution", "24", "--threshold", "0.1", "--keep-largest"])
    pv, pt = mc.read_ply(path)
    assert np.array_equal(pv, N(v)) and np.array_equal(pt, N(t)) and len(cc.connected_components(pt, len(pv))[2]) == 1


def test_no_guard_band_written(dev, bunny, meshes):
    """Under NEDDF_GUARD=1 the clean-up workspaces sit between poisoned bands: none of their bytes changed."""
    from neddf_amd import Context
    from neddf_amd._lib import guard_mode
    from neddf_amd.mesh import connected_components, remove_small_components
    ctx = Context.get(dev)
    v, t = meshes["random"]
    connected_components(t, len(v))
    remove_small_components(v, t, 9, 3)
    v, t = bunny.extract_mesh(resolution=33, keep_largest=1)
    assert len(t)
    bands, bad = ctx.check_guards()
    assert bad == 0, (bands, bad)
    assert bands > 0 if guard_mode() else bands == 0
