"""Surface extraction on the GPU: neddf_marching_cubes against the numpy restatement (tests/mesh_check.py) bit for bit,
its two-call protocol, neddf_field_grid against voxelize, meshes of the shipped bunny NeDDF and of synthetic NeRF / NeuS
fields, and neddf/scripts/extract_mesh.py end to end."""
import os

import numpy as np
import pytest
import torch
from conftest import GOLDEN

import mesh_check as mc
import synth

pytestmark = pytest.mark.gpu


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


def _same_mesh(got, want, what):
    gv, gt = (t.cpu().numpy() for t in got)
    wv, wt = want
    assert gv.dtype == np.float32 and gt.dtype == np.int32, what
    assert gt.shape == wt.shape and np.array_equal(gt, wt), (what, gt.shape, wt.shape)
    assert gv.shape == wv.shape and np.array_equal(gv.view(np.int32), wv.view(np.int32)), what     # bit for bit (NaN-safe)


def _volumes():
    rng = np.random.default_rng(5)

    def grid(shape, lo, hi):
        axes = [np.linspace(lo[a], hi[a], n) for a, n in enumerate(shape[::-1])]     # x, y, z
        z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
        return x, y, z

    out = []
    x, y, z = grid((40, 40, 40), (-1, -1, -1), (1, 1, 1))
    out.append(("sphere", np.sqrt(x * x + y * y + z * z) - 0.55, 0.0, (-1, -1, -1), (1, 1, 1)))
    lo, hi = (-0.9, -0.8, -1.3), (0.85, 0.9, 1.1)
    x, y, z = grid((23, 31, 37), lo, hi)                # nz, ny, nx all different; an anisotropic box
    out.append(("torus", np.sqrt((np.sqrt(x * x + y * y) - 0.45) ** 2 + z * z) - 0.2, 0.0, lo, hi))
    out.append(("two_spheres", np.minimum(np.sqrt((x - 0.35) ** 2 + y * y + z * z), np.sqrt((x + 0.4) ** 2 + y * y + z * z)) - 0.3,
                0.0, lo, hi))
    out.append(("random", rng.standard_normal((17, 9, 13)), 0.1, (0, 0, 0), (1, 2, 3)))
    out.append(("2x2x2", rng.standard_normal((2, 2, 2)), 0.0, (-1, -1, -1), (1, 1, 1)))
    out.append(("all_inside", -np.ones((5, 6, 7)), 0.0, (-1, -1, -1), (1, 1, 1)))
    out.append(("all_outside", np.ones((5, 6, 7)), 0.0, (-1, -1, -1), (1, 1, 1)))
    out.append(("equal_iso", rng.integers(-1, 2, (11, 12, 13)).astype(np.float64) * 0.5 + 0.25, 0.25, (-1, -1, -1), (1, 1, 1)))
    nan = rng.standard_normal((12, 10, 14))
    nan[rng.random(nan.shape) < 0.1] = np.nan
    out.append(("nan", nan, 0.0, (-2, -1, -1), (2, 1, 1)))
    return out


@pytest.mark.parametrize("case", _volumes(), ids=lambda c: c[0])
def test_marching_cubes_matches_the_checker(dev, case):
    from neddf_amd.mesh import marching_cubes
    name, vol, iso, lo, hi = case
    vol = vol.astype(np.float32)
    got = marching_cubes(torch.from_numpy(vol).to(dev), iso, lo, hi)
    want = mc.marching_cubes(vol, iso, lo, hi)
    _same_mesh(got, want, name)
    if name == "all_outside" or name == "all_inside":
        assert len(want[1]) == 0
    if name in ("sphere", "two_spheres", "torus"):
        assert mc.closed_and_oriented(want[1]) and mc.signed_volume(*want) > 0
        assert mc.euler_characteristic(*want) == {"sphere": 2, "two_spheres": 4, "torus": 0}[name]
    if name == "nan":
        assert np.isfinite(want[0]).all() and len(want[1])


def test_two_call_protocol_and_errors(dev):
    import ctypes as C
    from neddf_amd import Context, NeddfError
    from neddf_amd.mesh import marching_cubes
    ctx = Context.get(dev)
    x = np.linspace(-1, 1, 21)
    z, y, x = np.meshgrid(x, x, x, indexing="ij")
    vol = torch.from_numpy((np.sqrt(x * x + y * y + z * z) - 0.5).astype(np.float32)).to(dev)
    wv, wt = mc.marching_cubes(vol.cpu().numpy(), 0.0)
    lo, hi = (C.c_double * 3)(-1, -1, -1), (C.c_double * 3)(1, 1, 1)
    nv, nt = C.c_int64(-1), C.c_int64(-1)
    s = ctx.stream()
    ptr = C.c_void_p(vol.data_ptr())
    assert ctx.lib.neddf_marching_cubes(ctx.h, ptr, 21, 21, 21, lo, hi, 0.0, None, 0, None, 0, C.byref(nv), C.byref(nt), s) == 0
    assert (nv.value, nt.value) == (len(wv), len(wt))
    v = torch.full((len(wv), 3), -7.0, device=dev)
    t = torch.full((len(wt), 3), -7, device=dev, dtype=torch.int32)
    for cap_v, cap_t in ((len(wv) - 1, len(wt)), (len(wv), len(wt) - 1)):         # a cap below its count: counts only
        nv.value = nt.value = -1
        assert ctx.lib.neddf_marching_cubes(ctx.h, ptr, 21, 21, 21, lo, hi, 0.0, C.c_void_p(v.data_ptr()), cap_v, C.c_void_p(t.data_ptr()),
                                            cap_t, C.byref(nv), C.byref(nt), s) == 0
        assert (nv.value, nt.value) == (len(wv), len(wt))
        torch.cuda.synchronize()
        assert (v == -7).all() and (t == -7).all()
    assert ctx.lib.neddf_marching_cubes(ctx.h, ptr, 21, 21, 21, lo, hi, 0.0, C.c_void_p(v.data_ptr()), len(wv), C.c_void_p(t.data_ptr()),
                                        len(wt), C.byref(nv), C.byref(nt), s) == 0
    _same_mesh((v, t), (wv, wt), "exact-size write")
    assert ctx.lib.neddf_marching_cubes(ctx.h, ptr, 1, 21, 21, lo, hi, 0.0, None, 0, None, 0, C.byref(nv), C.byref(nt), s) == -1
    bad = (C.c_double * 3)(1, -1, -1)
    assert ctx.lib.neddf_marching_cubes(ctx.h, ptr, 21, 21, 21, bad, hi, 0.0, None, 0, None, 0, C.byref(nv), C.byref(nt), s) == -1
    with pytest.raises(NeddfError, match="float32"):
        marching_cubes(vol.double(), 0.0)
    with pytest.raises(NeddfError, match="dimensions"):
        marching_cubes(vol[0], 0.0)
    with pytest.raises(NeddfError, match="at least 2"):
        marching_cubes(vol[:1], 0.0)


@pytest.mark.parametrize("res", [64, 37])
@pytest.mark.parametrize("field", ["distance", "density"])
def test_field_grid_equals_voxelize(dev, bunny, field, res):
    """The same points (np.linspace rounded to float32), the same kernels (the eval-minimal route: voxelize is run with
    output_mode "minimal", whose distance kernel is the grid's), and a point's result does not depend on its tile."""
    from neddf_amd import Context, NeddfError
    ctx = Context.get(dev)
    bunny.upload(ctx, bunny._slot)
    grid = ctx.field_grid(bunny._slot, field, (res, res, res), (-1.1,) * 3, (1.1,) * 3).cpu().numpy()
    mode = bunny.output_mode
    bunny.output_mode = "minimal"
    try:
        vox = bunny.voxelize(field, 1.1, res)
    finally:
        bunny.output_mode = mode
    assert grid.shape == (res, res, res)
    assert np.array_equal(grid.view(np.int32), vox.transpose(1, 0, 2).view(np.int32))
    for shape, lo, hi in (((1, 4, 4), (-1,) * 3, (1,) * 3), ((4, 4, 4), (1, -1, -1), (1, 1, 1))):
        with pytest.raises(NeddfError):
            ctx.field_grid(bunny._slot, field, shape, lo, hi)


def test_bunny_mesh(bunny):
    """extract_mesh at resolution 96: closed, outward, inside the cube, and on the level set within what linear
    interpolation over one grid step allows.  Measured on the MI355X: max |distance(vertex) - 0.0275| = 7.9e-4 (grid step 2.3e-2,
    520 vertices); the gate leaves a factor of about four."""
    from neddf_amd import Context
    from neddf_amd.ray import Sampling
    res, r, iso = 96, 1.1, 0.0275
    ctx = Context.get(bunny.device)
    bunny.upload(ctx, bunny._slot)
    vol = ctx.field_grid(bunny._slot, "distance", (res,) * 3, (-r,) * 3, (r,) * 3)
    b = torch.cat([vol[[0, -1]].flatten(), vol[:, [0, -1]].flatten(), vol[:, :, [0, -1]].flatten()])
    assert (b >= iso).all(), float(b.min())              # precondition: the surface does not reach the cube's faces
    v, t = bunny.extract_mesh(resolution=res)
    assert v.device == bunny.device and t.dtype == torch.int32 and len(t) > 500
    vn, tn = v.cpu().numpy(), t.cpu().numpy()
    assert mc.closed_and_oriented(tn) and mc.signed_volume(vn, tn) > 0
    assert (np.abs(vn) <= r).all()
    with torch.no_grad():
        out = bunny(Sampling(v[None], torch.tensor([1.0, 0.0, 0.0], device=v.device).expand(1, len(v), 3).contiguous(),
                             torch.zeros(1, len(v), 3, device=v.device)))
    err = (out["distance"][0] - iso).abs().max().item()
    print("bunny mesh: %d vertices, %d triangles, max |distance - iso| = %.3e (grid step %.3e)" % (len(v), len(t), err, 2 * r / (res - 1)))
    assert err < 3e-3, err


def _closed_level_set_mesh(net, field):
    """A threshold whose level set stays inside the cube (every boundary sample on one side of it) -> extract_mesh's mesh,
    closed, with its normals pointing up the field for an sdf and down it for a density (out of the object either way)."""
    from neddf_amd import Context
    ctx = Context.get(net.device)
    net.upload(ctx, net._slot)
    for r in (1.1, 0.8, 0.5, 0.3, 1.6, 4.0):
        vol = ctx.field_grid(net._slot, "distance" if field == "sdf" else field, (48,) * 3, (-r,) * 3, (r,) * 3)
        b = torch.cat([vol[[0, -1]].flatten(), vol[:, [0, -1]].flatten(), vol[:, :, [0, -1]].flatten()])
        iso = float(b.min())                    # boundary at or above iso: the enclosed part is below it
        if float(vol.min()) < iso:
            enclosed_low = True
            break
        iso = float(np.nextafter(np.float32(b.max().item()), np.float32(np.inf)))       # boundary below iso: the enclosed part is above
        if float(vol.max()) >= iso:
            enclosed_low = False
            break
    else:
        pytest.fail("no cube holds a closed level set of this field")
    v, t = net.extract_mesh(field, iso, r, 48)
    vn, tn = v.cpu().numpy(), t.cpu().numpy()
    assert len(tn) and mc.closed_and_oriented(tn), field
    # normals out of the low side for an sdf, out of the high side for a density (extract_mesh's flip): the enclosed part's
    # signed volume is positive when the normals leave it
    outward = enclosed_low if field == "sdf" else not enclosed_low
    assert (mc.signed_volume(vn, tn) > 0) == outward, (field, enclosed_low, r, iso)


def test_nerf_density_and_neus_sdf_meshes(dev):
    from neddf_amd import NeRF, NeuS
    nerf = NeRF().to(dev)
    nerf.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.nerf_state(seed=11).items()})
    neus = NeuS().to(dev)
    neus.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.neus_state().items()})
    for net in (nerf, neus):
        net.set_iter(-1)
        for p in net.parameters():
            p.requires_grad_(False)
    _closed_level_set_mesh(nerf, "density")
    _closed_level_set_mesh(neus, "sdf")             # (a ReLU sdf trunk: sdf >= 0, so its closed level sets enclose maxima)
    with pytest.raises(ValueError):
        nerf.extract_mesh("distance")
    with pytest.raises(ValueError):
        neus.extract_mesh("distance")


def test_extract_mesh_script(dev, bunny, tmp_path, capsys):
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
    sd = {p + k: torch.from_numpy(v) for k, v in bunny_smoke_weights().items() for p in ("network_fine.", "network_coarse.")}
    torch.save(sd, run / "models" / "model_00007.pth")
    path = main([str(run), "--epoch", "7", "--resolution", "40"])
    out = capsys.readouterr().out
    assert path == (run / "mesh" / "mesh_40_threshold0.0275.ply").resolve() and path.is_file()
    assert "vertices: " in out and "triangles: " in out and "grid evaluation: " in out and "marching cubes: " in out
    v, t = mc.read_ply(path)
    _same_mesh(bunny.extract_mesh(resolution=40), (v, t), "script")


def test_no_guard_band_written(dev, bunny):
    """Under NEDDF_GUARD=1 the grid and marching-cubes workspaces sit between poisoned bands: none of their bytes changed."""
    from neddf_amd import Context
    from neddf_amd._lib import guard_mode
    ctx = Context.get(dev)
    v, t = bunny.extract_mesh(resolution=33)
    assert len(t)
    bands, bad = ctx.check_guards()
    assert bad == 0, (bands, bad)
    assert bands > 0 if guard_mode() else bands == 0
