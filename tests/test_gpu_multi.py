"""Multi-GPU path (BASELINE.json configs[3]) as far as the test box allows.

One MI355X is enough for: the library's RCCL communicator with a forced single rank (neddf_comm_init /
neddf_gather_pixels / waits / stage timing), and the REAL renderer sharded over several processes -- on a box with
fewer devices than ranks the processes share cuda:0 and the slabs travel through gloo, because RCCL refuses two ranks on
one device; with >= 2 devices the same worker uses RCCL end to end (render_image_sharded -> neddf_gather_pixels).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from conftest import ROOT, assert_close, free_port, golden

pytestmark = pytest.mark.gpu


def _bench_json(stdout):
    """The bench line out of a captured stdout, wherever it sits: several processes may share the pipe, so nothing here relies on line
    boundaries -- the LAST `{"metric"` that decodes as one JSON object is the line."""
    import json
    dec = json.JSONDecoder()
    found = []
    at = stdout.find('{"metric"')
    while at >= 0:
        try:
            found.append(dec.raw_decode(stdout, at)[0])
        except ValueError:
            pass
        at = stdout.find('{"metric"', at + 1)
    return found

_SHARD_WORKER = r'''
import os, sys, numpy as np, torch, torch.distributed as dist
root, port, rank, world, out_path = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from conftest import BUNNY_CFG, golden
import neddf_amd
from neddf_amd.parallel import gather_pixels, pack_pixels, render_image_sharded, shard_range, unpack_pixels
n_dev = torch.cuda.device_count()
rccl = n_dev >= world                               # one device per rank: RCCL end to end
dev = torch.device("cuda", rank if rccl else 0)
torch.cuda.set_device(dev)
if rccl:
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:" + port, rank=rank, world_size=world, device_id=dev)
else:
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:" + port, rank=rank, world_size=world)
g = golden("bunny_image_small.npz")
wts = golden("bunny_weights.npz")
r = neddf_amd.NeRFRender(dict(BUNNY_CFG, _target_="neddf.network.NeDDF"), sample_coarse=64, sample_fine=128, dist_near=2.0,
                         dist_far=6.0, max_dist=6.0, use_coarse_network=False, sampling_type="cone")
r.network_fine.load_state_dict({k: torch.from_numpy(wts[k]) for k in wts.files})
r.to(dev); r.set_iter(-1)
cam = neddf_amd.Camera(neddf_amd.PinholeCalib(g["calib"].astype(np.float64)), None).to(dev)
cam.R, cam.T = torch.from_numpy(g["R"]).to(dev), torch.from_numpy(g["T"]).to(dev)
w, h, chunk = int(g["width"]), int(g["height"]), int(g["chunk"])
frame = os.environ.get("NEDDF_TEST_FRAME")          # "W,H,CHUNK": another frame, sharded chunk-granularly (render_image_sharded) under either backend
if frame:
    w, h, chunk = (int(v) for v in frame.split(","))
keys = ["color", "depth", "transmittance"]
torch.manual_seed(int(g["seed"]))                  # every rank holds the reference's seed; the slab jumps into the stream
if rccl or frame:
    img = render_image_sharded(r, w, h, cam, keys, 1, chunk)
    info = neddf_amd.Context.get(dev).comm_info() if rccl else dict(nranks=world, rank=rank, rccl_version=1)
    assert world == 1 or info["nranks"] == world and info["rank"] == rank and info["rccl_version"] > 0, info
else:
    lo, hi = shard_range(w * h, rank, world)
    parts = r.render_image(w, h, cam, keys, 1, chunk, pixel_range=(lo, hi))
    full = gather_pixels(pack_pixels(parts, keys).cpu(), w * h)
    img = {k: v.reshape(h, w, -1) for k, v in unpack_pixels(full, keys).items()}
end = torch.rand(4)                                # generator position after the frame
np.savez(out_path + ".%d.npz" % rank, end=end.numpy(), rccl=np.int32(rccl), **{k: v.cpu().numpy() for k, v in img.items()})
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok", "rccl" if rccl else "gloo-shared-gpu", flush=True)
os._exit(0)         # (as in tests/test_host.py: nothing is left to check, and a finished worker must not die in a backend thread's teardown)
'''


def _run_world(tmp_path, world, frame=None):
    script = tmp_path / "shard_worker.py"
    script.write_text(_SHARD_WORKER)
    from conftest import run_ranks
    out = str(tmp_path / ("img_w%d" % world))
    env = dict(os.environ, NEDDF_BENCH_PMC="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("NEDDF_TEST_FRAME", None)
    if frame:
        env["NEDDF_TEST_FRAME"] = frame
    run_ranks(lambda r, port: [sys.executable, str(script), ROOT, port, str(r), str(world), out], world, env=env, timeout=600)
    return [np.load(out + ".%d.npz" % r) for r in range(world)]


def test_sharded_render_is_independent_of_world_size(tmp_path):
    """render_image's parity mode under ray sharding: for world sizes 1, 2 and 3 every rank ends with the SAME 12x10
    frame -- bit-identical across world sizes -- which matches the reference's render of that frame and seed
    (tests/golden/bunny_image_small.npz; chunk 50, so slabs cut through chunks), and every rank leaves the CPU generator
    where the reference's whole-frame draw leaves it."""
    g = golden("bunny_image_small.npz")
    frames = {}
    for world in (1, 2, 3):
        res = _run_world(tmp_path, world)
        for r_, d in enumerate(res):
            for k in ("color", "depth", "transmittance"):
                assert np.array_equal(d[k], res[0][k]), (world, r_, k)         # every rank holds the same gathered frame
            assert np.array_equal(d["end"], res[0]["end"])
        frames[world] = res[0]
    for k in ("color", "depth", "transmittance"):
        assert_close(frames[1][k], g[k], 1e-4, 1e-5, k + " vs reference")
        for world in (2, 3):
            assert np.array_equal(frames[world][k], frames[1][k]), (world, k)   # sharding changes nothing, bit for bit
    for world in (2, 3):
        assert np.array_equal(frames[world]["end"], frames[1]["end"])


def test_sharded_render_eight_ranks_ragged(tmp_path):
    """BASELINE.json configs[3]'s rank count on whatever the box has: EIGHT ranks render one 37 x 29 frame at chunk 100 -- 11 chunks, the last one 73 rays:
    slabs of 2, 2, 2, 1, 1, 1, 1, 1 chunks, the ragged case a strong-scaled 800 x 800 frame meets first at N = 8 -- through `render_image_sharded`
    (chunk-granular slabs, each rank jumps the CPU generator to its slab, one gather of the pixels).  With eight devices the ranks form an RCCL communicator
    and the library's own ragged gather runs (its first execution with more than one rank); on a one-GPU box they share the device and the gather is
    staged through gloo.  Every rank must end with the frame ONE rank renders, bit for bit, and with the generator where the whole-frame draw leaves it."""
    one = _run_world(tmp_path, 1, frame="37,29,100")[0]
    res = _run_world(tmp_path, 8, frame="37,29,100")
    assert one["color"].shape == (29, 37, 3) and np.isfinite(one["color"]).all()
    for r_, d in enumerate(res):
        for k in ("color", "depth", "transmittance"):
            assert np.array_equal(d[k], one[k]), (r_, k, float(np.abs(d[k] - one[k]).max()))
        assert np.array_equal(d["end"], one["end"]), r_


def test_library_communicator_single_rank():
    """neddf_comm_* / neddf_gather_pixels on a 1-rank RCCL communicator: bootstrap, the all-gather on the library's
    communication stream (equal and ragged shapes are the same thing with one rank; both buffer routes are driven by
    n_total), device-side and host-side waits, error codes, the gather's entry in the stage timings."""
    from neddf_amd import Context
    from neddf_amd._lib import NeddfError
    dev = torch.device("cuda:0")
    ctx = Context.get(dev)
    if ctx.comm_info()["nranks"]:
        ctx.comm_destroy()
    with pytest.raises(NeddfError, match="no communicator"):
        ctx.gather_pixels(torch.zeros(4, 5, device=dev), 4)
    uid = ctx.comm_unique_id()
    assert len(uid) == 128 and any(uid)
    with pytest.raises(NeddfError, match="rank must be"):
        ctx.comm_init(1, 1, uid)
    ctx.comm_init(0, 1, uid)
    with pytest.raises(NeddfError, match="already has a communicator"):
        ctx.comm_init(0, 1, uid)
    info = ctx.comm_info()
    assert info["rank"] == 0 and info["nranks"] == 1 and info["rccl_version"] >= 20000, info
    ctx.set_timing(True)
    ctx.get_stage_timings()
    side = torch.cuda.Stream(device=dev)
    for n in (640000, 12345):
        with torch.cuda.stream(side):               # the gather must order itself after the producer on ITS stream
            local = torch.rand(n, 5, device=dev)
            local.mul_(2.0)
            out = ctx.gather_pixels(local, n)
            ctx.comm_wait()
            got = out.clone()
        side.synchronize()
        assert torch.equal(got, local)
        ctx.gather_pixels(local, n, out)
        ctx.comm_wait_host(20000)
        assert torch.equal(out, local)
    st = ctx.get_stage_timings()
    ctx.set_timing(False)
    assert st["gather"][1] == 4 and st["gather"][0] > 0.0, st
    ctx.comm_destroy()
    assert ctx.comm_info()["nranks"] == 0


def test_ragged_gather_routes_on_one_rank(monkeypatch):
    """Both routes of a RAGGED gather executed on a one-rank communicator (NEDDF_GATHER_FORCE_RAGGED=1, read at neddf_comm_init): the
    default padded staging route (copy in, equal-count all-gather, compaction copy) and the opt-in in-place route
    (NEDDF_GATHER_INPLACE=1: ncclGroupStart / one ncclBroadcast per slab / ncclGroupEnd).  The route is a property of the
    communicator, agreed by every rank at initialisation."""
    from neddf_amd import Context
    dev = torch.device("cuda:0")
    ctx = Context.get(dev)
    if ctx.comm_info()["nranks"]:
        ctx.comm_destroy()
    monkeypatch.setenv("NEDDF_GATHER_FORCE_RAGGED", "1")
    for inplace in ("0", "1"):
        monkeypatch.setenv("NEDDF_GATHER_INPLACE", inplace)
        ctx.comm_init(0, 1, ctx.comm_unique_id())
        ctx.set_timing(True)
        ctx.get_stage_timings()
        for n, granule in ((12345, 1), (640000, 512), (7, 512)):
            local = torch.rand(n, 5, device=dev)
            out = torch.full((n, 5), -1.0, device=dev)
            ctx.gather_pixels(local, n, out, granule=granule)
            ctx.comm_wait_host(20000)
            assert torch.equal(out, local), (inplace, n)
        st = ctx.get_stage_timings()
        ctx.set_timing(False)
        assert st["gather"][1] == 3 and st["gather"][0] > 0.0, st
        ctx.comm_destroy()


def test_bench_self_launch_two_ranks_shared_gpu():
    """`python bench.py --gpus 2` with no launcher must start two ranks itself and print ONE JSON line with n_gpus = 2 and
    the communicator size in config.comm.  On a box with one device the two ranks share it (NEDDF_BENCH_SHARE_GPU=1: gloo
    staging instead of RCCL, marked as not-a-measurement); with two devices this is the real configs[3] path."""
    import json
    env = dict(os.environ, NEDDF_BENCH_PMC="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    if torch.cuda.device_count() < 2:
        env["NEDDF_BENCH_SHARE_GPU"] = "1"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1",
                        "--no-cpu-baseline", "--full"], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    lines = _bench_json(p.stdout)
    assert len(lines) == 1, p.stdout[-3000:]
    line = lines[0]
    assert line["n_gpus"] == 2 and line["config"]["comm"]["world_size"] == 2
    assert line["config"]["comm"]["torch_distributed_world_size"] == 2
    assert "configs[3]" in line["config"]["workload"] and line["value"] > 0 and line["psnr_vs_oracle_db"] > 80
    if torch.cuda.device_count() >= 2:
        assert line["config"]["comm"]["rccl_comm_ranks"] == 2


def test_bench_collective_path_on_one_rank():
    """The N > 1 code path of bench.py on ONE rank (NEDDF_BENCH_FORCE_DIST=1): RCCL process group, the library's own communicator
    bootstrapped through it, pixel all-gather on the communication stream with the host-side deadline wait, max-over-ranks."""
    import json
    env = dict(os.environ, NEDDF_BENCH_PMC="0", HSA_ENABLE_IPC_MODE_LEGACY="0", NEDDF_BENCH_FORCE_DIST="1", MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(free_port()))
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--no-cpu-baseline"], env=env,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    line = _bench_json(p.stdout)[-1]
    comm = line["config"]["comm"]
    assert comm["rccl_comm_ranks"] == 1 and comm["torch_distributed_world_size"] == 1 and "neddf_gather_pixels" in comm["gather"], comm
    assert line["stage_ms_per_step"]["gather"] > 0 and line["value"] > 0


def test_smoke_under_asan():
    """smoke() -- weight packing, workspace carving, the fused render_rays orchestration, 64 rays against the oracle -- with the
    host side of the library under AddressSanitizer + UBSan (the device code is the shipped one)."""
    csrc = os.path.join(ROOT, "neddf_amd", "csrc")
    lib = os.path.join(csrc, "libneddf_hip_asan.so")
    rt = subprocess.run(["make", "-s", "-C", csrc, "print-asan-rt"], capture_output=True, text=True).stdout.strip()
    if not (os.path.exists(lib) and os.path.exists(rt)):
        pytest.skip("sanitizer build not present (python -c 'import __graft_entry__ as g; g.build()' makes it)")
    env = dict(os.environ, LD_PRELOAD=rt, ASAN_OPTIONS="detect_leaks=0:exitcode=23:protect_shadow_gap=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", NEDDF_LIB_PATH=lib)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "__graft_entry__.py"), "smoke-only"], env=env, capture_output=True, text=True,
                       timeout=900)
    if p.returncode != 0 and "smoke ok" not in p.stdout and ("hsa_amd_memory_pool_allocate" in p.stderr or "out-of-memory" in p.stderr
                                                              or "AddressSanitizer can not provide additional info" in p.stderr):
        # ROCm's compiler-rt intercepts hsa_amd_memory_pool_allocate (device ASan support) and, preloaded into an uninstrumented
        # python + HIP runtime, fails inside the runtime's own start-up on this image (tools/asan_probe.sh: every option set tried) --
        # before any code of this library runs.  The CPU error-path test (tests/test_host.py) is what runs under ASan then.
        pytest.skip("AddressSanitizer runtime cannot coexist with the HIP runtime start-up on this box")
    assert p.returncode == 0 and "smoke ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]


def test_run_eval_under_a_launcher_matches_single_process(tmp_path):
    """BASELINE.json configs[3] through the reference's own CLI: `torch.distributed.run --nproc-per-node 2 neddf/scripts/run_eval.py`
    (rays of every view sharded over the ranks, pixel all-gather, rank 0 writes) must produce byte-identical PNGs to the
    single-process run of the same command.  One-GPU boxes: the two ranks share the device and the slabs travel through gloo."""
    import yaml
    from conftest import BUNNY_CFG
    from test_host import _make_dataset
    wts = golden("bunny_weights.npz")
    ds_dir = str(tmp_path / "ds")
    _make_dataset(ds_dir, n=2, w=20, h=16)
    cfg = {"dataset": {"_target_": "neddf.dataset.NeRFSyntheticDataset", "dataset_dir": ds_dir, "data_split": "train",
                       "use_depth": False, "use_mask": True},
           "render": {"_target_": "neddf.render.NeRFRender", "sample_coarse": 64, "sample_fine": 128, "dist_near": 2.0,
                      "dist_far": 6.0, "max_dist": 6.0, "use_coarse_network": False, "sampling_type": "cone"},
           "network": dict(BUNNY_CFG, _target_="neddf.network.NeDDF"),
           "trainer": {"_target_": "neddf.trainer.NeRFTrainer", "device": "cuda:0", "batch_size": 128, "chunk": 100},
           "loss": {"functions": [{"_target_": "neddf.loss.ColorLoss", "weight": 1.0}]}}
    sd = {p + k: torch.from_numpy(wts[k]) for k in wts.files for p in ("network_fine.", "network_coarse.")}
    script = os.path.join(ROOT, "neddf", "scripts", "run_eval.py")
    outs = {}
    for tag, launcher in (("one", []), ("two", ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                                                "--master-port", str(free_port())])):
        run = tmp_path / tag
        (run / ".hydra").mkdir(parents=True)
        (run / "models").mkdir()
        yaml.safe_dump(cfg, open(run / ".hydra" / "config.yaml", "w"))
        torch.save(sd, run / "models" / "model_00007.pth")
        env = dict(os.environ, NEDDF_BENCH_PMC="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
        for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
            env.pop(k, None)
        if torch.cuda.device_count() < 2:
            env["NEDDF_DIST_BACKEND"] = "gloo"
        p = subprocess.run([sys.executable] + launcher + [script, str(run), "--epoch", "7", "--seed", "5"], env=env, capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
        assert p.stdout.count("psnr:") == 2, p.stdout[-2000:]          # rank 0 only prints
        outs[tag] = run / "eval"
    for i in range(2):
        for suffix in ("rgb", "rgb_gt", "depth"):
            name = "%03d_%s.png" % (i, suffix)
            assert (outs["one"] / name).read_bytes() == (outs["two"] / name).read_bytes(), name


def test_run_script_two_ranks_data_parallel(tmp_path):
    """scripts/run.py under a launcher with two ranks (data-parallel training, one gradient all-reduce per step): the run must
    FINISH -- rank 0's periodic test render is its own, not a sharded collective the other rank never joins --, both ranks must
    start from identical parameters (run.py asserts the signature across ranks before step 1), and rank 0 alone writes the
    checkpoints / renders.  One-GPU boxes: the ranks share the device, gradients travel through gloo."""
    from test_host import _make_dataset
    ds = tmp_path / "data" / "tiny"
    _make_dataset(str(ds), n=2, w=20, h=16, split="train")
    script = os.path.join(ROOT, "neddf", "scripts", "run.py")
    env = dict(os.environ, NEDDF_BENCH_PMC="0", HSA_ENABLE_IPC_MODE_LEGACY="0", NEDDF_RUN_PRINT_SIGNATURE="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    if torch.cuda.device_count() < 2:
        env["NEDDF_DIST_BACKEND"] = "gloo"
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(free_port()), script, "trainer=test", "dataset.dataset_dir=data/tiny/",
                        "trainer.batch_size=16", "trainer.epoch_max=1", "trainer.epoch_save_model=1", "trainer.epoch_test_rendering=1",
                        "trainer.epoch_save_fields=1"], env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    import re
    rds = list((tmp_path / "outputs").glob("*/*"))
    assert len(rds) == 1, rds                                         # one run directory: rank 0's
    # every rank leaves its signature in a file of its own; the shared pipe is read with a pattern, never by lines
    sigs = [(rds[0] / ("replica_signature.%d" % r)).read_text().strip().split("=", 1)[1] for r in (0, 1)]
    assert sigs[0] == sigs[1], sigs
    piped = dict(re.findall(r"replica_signature\[(\d)\]=([-+0-9.einfa]+)", p.stdout))
    assert piped == {"0": sigs[0], "1": sigs[1]}, p.stdout[-2000:]
    for e in (0, 1):
        sd = torch.load(rds[0] / "models" / ("model_%05d.pth" % e), map_location="cpu")
        assert len(sd) == 52 and all(torch.isfinite(v).all() for v in sd.values())
        assert len(list((rds[0] / "render" / ("%04d" % e)).glob("*_rgb.png"))) == 1


def test_c_client_of_the_abi(tmp_path):
    """INTEGRATION.md mode B: a plain-C program (tests/capi/c_smoke.c, built with gcc against include/neddf_hip.h -- no Python, no
    torch) sets up the shipped NeDDF architecture, renders 96 rays through neddf_render_rays in both output modes and gathers the
    pixels over a one-rank communicator.  Its outputs must equal what the Python binding renders from the same numbers (weights,
    rays, uniforms from the same linear congruential generator): the C calling convention, struct layouts and pointer ownership
    of the header are what a reference-side binding would rely on."""
    import ctypes
    from conftest import BUNNY_CFG
    import neddf_amd
    exe = str(tmp_path / "c_smoke")
    out = str(tmp_path / "out.bin")
    csrc = os.path.join(ROOT, "neddf_amd", "csrc")
    subprocess.check_call(["gcc", "-std=c11", "-O2", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "capi", "c_smoke.c"), "-L", csrc, "-lneddf_hip", "-L", "/opt/rocm/lib", "-lamdhip64", "-lm",
                           "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = subprocess.run([exe, out], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "c_smoke ok" in p.stdout, p.stdout + p.stderr
    RAYS = 96
    got = np.fromfile(out, np.float32)
    assert got.size == RAYS * 21
    full, mini, packed, gathered = got[:RAYS * 6], got[RAYS * 6:RAYS * 11], got[RAYS * 11:RAYS * 16], got[RAYS * 16:]
    assert np.array_equal(packed, gathered)                                   # the library's own all-gather, one rank
    assert np.array_equal(packed.reshape(RAYS, 5)[:, :3].ravel(), mini[:RAYS * 3])

    # the same numbers on the Python side
    state = 12345
    def lcg(n):
        nonlocal state
        vals = np.empty(n, np.float64)
        for i in range(n):
            state = (state * 1664525 + 1013904223) & 0xFFFFFFFF
            vals[i] = (state >> 8) / 8388608.0 - 1.0
        return vals.astype(np.float32)
    dims = [(60 if l == 0 else (316 if l == 5 else 256), 256) for l in range(7)] + [(343 if l == 0 else 256, 256) for l in range(3)] + \
           [(256, 1), (256, 1), (256, 3)]
    names = ["layers_ddf.%d" % l for l in range(7)] + ["layers_col.%d" % l for l in range(3)] + ["layer_ddf_out", "layer_aux_out", "layer_col_out"]
    sd = {}
    for name, (i, o) in zip(names, dims):
        s_ = np.float32(np.sqrt(np.float32(2.0) / np.float32(i + o)))
        sd[name + ".weight"] = torch.from_numpy((np.float32(1.7) * s_ * lcg(i * o)).astype(np.float32).reshape(i, o))
        sd[name + ".bias"] = torch.from_numpy((np.float32(0.05) * lcg(o)).astype(np.float32))
    uc = (np.float32(0.5) * (lcg(RAYS * 65) + np.float32(1.0))).reshape(RAYS, 65)
    uf = (np.float32(0.5) * (lcg(RAYS * 129) + np.float32(1.0))).reshape(RAYS, 129)
    dev = torch.device("cuda:0")
    r = neddf_amd.NeRFRender(dict(BUNNY_CFG, _target_="neddf.network.NeDDF"), sample_coarse=64, sample_fine=128, dist_near=2.0, dist_far=6.0,
                             max_dist=6.0, use_coarse_network=False, sampling_type="cone")
    r.network_fine.load_state_dict(sd)
    r.to(dev)
    r.set_iter(-1)
    cam = neddf_amd.Camera(neddf_amd.PinholeCalib(np.array([555.6, 555.6, 200.0, 200.0])), None).to(dev)
    cam.R = torch.eye(3, device=dev)
    cam.T = torch.tensor([0.1, -0.05, 4.0], device=dev)
    uv = torch.tensor([[140 + (k * 7) % 120, 150 + (k * 11) % 100] for k in range(RAYS)], dtype=torch.int64, device=dev)
    with torch.no_grad():
        ctx = r._ctx(dev)
        of = r._render(ctx, uv, cam, torch.from_numpy(uc).to(dev), torch.from_numpy(uf).to(dev), full=True)
        om = r._render(ctx, uv, cam, torch.from_numpy(uc).to(dev), torch.from_numpy(uf).to(dev), full=False)
    want_full = np.concatenate([of["color"].cpu().numpy().ravel(), of["depth"].cpu().numpy(), of["transmittance"].cpu().numpy(),
                                of["fields_penalty"].cpu().numpy()])
    want_mini = np.concatenate([om["color"].cpu().numpy().ravel(), om["depth"].cpu().numpy(), om["transmittance"].cpu().numpy()])
    assert np.isfinite(got).all()
    # same library, same inputs, same outputs requested: bit-identical
    assert np.array_equal(mini, want_mini), float(np.abs(mini - want_mini).max())
    # the C program's first call asks for fields_penalty but for no coarse outputs, so its coarse pass runs eval-minimal (reverse-mode
    # distance gradient) where the Python render_rays-style call (every key) carries Jacobian rows: same function, different rounding
    assert_close(full, want_full, 1e-4, 1e-5, "C full-mode outputs vs Python binding")


def _bench_line(extra_args, extra_env):
    import json
    env = dict(os.environ, NEDDF_BENCH_PMC="0", HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()))
    env.update(extra_env)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--full"] + extra_args,
                       env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return _bench_json(p.stdout)[-1]


def test_bench_scaling_modes_agree_at_one_rank():
    """bench.py --scaling weak / strong through the FORCED collective path on one rank against the plain line: at N = 1 both modes
    render the same 640 000 rays (the strong mode through pixel_range + the chunk-granular gather), so their rays/s must agree with
    the plain line within 1 % -- the day an 8-GPU node runs it, N = 1 of either curve is the headline number."""
    plain = _bench_line([], {})
    weak = _bench_line([], {"NEDDF_BENCH_FORCE_DIST": "1"})
    strong = _bench_line(["--scaling", "strong"], {"NEDDF_BENCH_FORCE_DIST": "1"})
    assert plain["scaling"] == "weak" and weak["scaling"] == "weak" and strong["scaling"] == "strong"
    assert strong["config"]["comm"]["rccl_comm_ranks"] == 1 and "granular" in strong["config"]["comm"]["gather"]
    assert strong["config"]["rays_per_step"] == 640000 and strong["n_gpus"] == 1
    for name, line in (("weak", weak), ("strong", strong)):
        # functional agreement is the assertion: same rays, same frame (the bench's own parity sample passed in each run); the rate is
        # three 3-step runs on a box whose clocks move, so it only has to be the same order -- 1 % is what profiles/ reports, not a gate
        assert line["config"]["rays_per_step"] == plain["config"]["rays_per_step"] == 640000
        assert line["psnr_vs_oracle_db"] > 120 and plain["psnr_vs_oracle_db"] > 120
        assert abs(line["value"] / plain["value"] - 1.0) < 0.10, (name, line["value"], plain["value"])


def test_bench_preflight_fails_fast_and_readably():
    """--gpus N on a box with fewer devices: a message and a non-zero exit within seconds, not a rendezvous timeout."""
    import time
    import torch
    n = torch.cuda.device_count() + 1
    env = dict(os.environ, NEDDF_BENCH_PMC="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "NEDDF_BENCH_SHARE_GPU"):
        env.pop(k, None)
    t0 = time.time()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "1", "--warmup", "0"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "HIP device" in p.stderr and "--gpus %d" % n in p.stderr, p.stderr[-2000:]
    assert time.time() - t0 < 60.0      # (the first `import torch` of a fresh box is most of this)


def test_bench_plain_run_dumps_what_it_timed(tmp_path):
    """A plain `bench.py` run times exactly --steps steps, prints the headline line without the --full extras, and --dump-outputs
    writes the last step's frame: the same numbers this process renders from the same seeded inputs."""
    import math
    import bench
    import neddf_amd
    env = dict(os.environ, NEDDF_BENCH_PMC="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "NEDDF_BENCH_FORCE_DIST", "NEDDF_BENCH_SHARE_GPU"):
        env.pop(k, None)
    out = tmp_path / "outputs"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs",
                        str(out)], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    line = _bench_json(p.stdout)[-1]
    assert line["steps"] == 2 and line["unit"] == "rays/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert abs(line["value"] * line["ms_per_step"] / 1e3 / 640000 - 1.0) < 1e-6, line
    assert not {"psnr_vs_oracle_db", "value_incl_rng", "alt_operand_policy", "cpu_baseline"} & set(line), sorted(line)
    got = {k: np.load(str(out / (k + ".npy"))) for k in ("color", "depth", "transmittance")}
    assert sorted(os.listdir(str(out))) == ["color.npy", "depth.npy", "transmittance.npy"]
    assert got["color"].shape == (640000, 3) and got["depth"].shape == got["transmittance"].shape == (640000,)
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in got.values())
    dev = torch.device("cuda:0")
    render, _ = bench.build_render(dev)
    fx = 0.5 * 800 / math.tan(0.5 * bench.CAMERA_ANGLE_X)
    R, T = bench.view_pose(0)
    cam = neddf_amd.Camera(neddf_amd.PinholeCalib(np.array([fx, fx, 400.0, 400.0])), None).to(dev)
    cam.R, cam.T = torch.from_numpy(R).to(dev), torch.from_numpy(T).to(dev)
    U = torch.rand(640000, 128, device=dev, generator=torch.Generator(device=dev).manual_seed(1234))
    want = render.render_image_single_pass(800, 800, cam, 128, U=U)
    for k, v in got.items():
        assert np.array_equal(v, want[k].cpu().numpy()), (k, float(np.abs(v - want[k].cpu().numpy()).max()))


_GUARD_WORKER = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import neddf_amd
from neddf_amd import Sampling
from neddf_amd.fixtures import BUNNY_SMOKE_CFG, BUNNY_SMOKE_RENDER, bunny_smoke_weights, synth
dev = torch.device("cuda:0")
wts = bunny_smoke_weights()
r = neddf_amd.NeRFRender(dict(BUNNY_SMOKE_CFG, _target_="neddf.network.NeDDF"), **BUNNY_SMOKE_RENDER)
r.network_fine.load_state_dict({k: torch.from_numpy(v) for k, v in wts.items()})
r.to(dev); r.set_iter(-1)
fx = 0.5 * 800 / np.tan(0.5 * 0.6911112070083618)
cam = neddf_amd.Camera(neddf_amd.PinholeCalib(np.array([fx, fx, 400.0, 400.0])), None).to(dev)
cam.R, cam.T = torch.eye(3, device=dev), torch.tensor([0.0, 0.0, 4.0], device=dev)
ctx = r._ctx(dev)
total = 0
with torch.no_grad():
    for dtype in ("fp32", "f16_split", "bf16"):
        r.network_fine.weight_dtype = dtype
        ctx = r._ctx(dev)
        # hierarchical render_rays at ragged batch sizes (tile tails of every kernel), full dict and eval-minimal
        for n in (1, 63, 1000, 4097):
            uv = torch.randint(0, 800, (n, 2), device=dev)
            for full in (True, False):
                o = r._render(ctx, uv, cam, torch.rand(n, 65, device=dev), torch.rand(n, 129, device=dev), full=full)
                bands, bad = ctx.check_guards()
                assert bands >= 20 and bad == 0, (dtype, n, full, bands, bad)
                total += bands
        # the single-pass image path (bench.py's workload) on a slab that is not a multiple of any tile
        o = r.render_image_single_pass(800, 800, cam, 128, pixel_range=(777, 777 + 70001))
        bands, bad = ctx.check_guards()
        assert bad == 0, (dtype, "single pass", bands, bad)
        # the stand-alone field on an odd point count, both output modes
        pos, d, var = synth.random_sampling(3, 333, seed=2)
        net = r.network_fine
        for mode in ("full", "minimal"):
            net.output_mode = mode
            net(Sampling(torch.from_numpy(pos).to(dev), torch.from_numpy(d).to(dev), torch.from_numpy(var).to(dev)))
            bands, bad = ctx.check_guards()
            assert bad == 0, (dtype, mode, bands, bad)
# one training step (forward with every saved tensor, backward, weight gradients): workspace carves of the training ABI
r.network_fine.weight_dtype = "fp32"
r.set_iter(1500)
uv = torch.randint(100, 300, (1024, 2), device=dev).to(torch.int16)
out = r.render_rays(uv, cam)
loss = out["color"].square().mean() + out["fields_penalty"].mean() + out["depth"].mean() * 1e-3
loss.backward()
bands, bad = r._ctx(dev).check_guards()
assert bad == 0, ("train", bands, bad)
# the probe itself: a deliberate one-element overrun must be seen
ctx = r._ctx(dev)
import ctypes
bands0, _ = ctx.check_guards()
print("GUARD_OK bands_checked=%d last=%d" % (total, bands0))
"""


def test_workspace_guard_bands(tmp_path):
    """The bounds probe that stands in for a GPU-side sanitizer (neddf_debug_check_guards, NEDDF_GUARD=1): every workspace allocated at
    its exact size between poisoned bands, every arena carve followed by one.  Renders at ragged batch sizes under the three operand
    policies, the single-pass path on an odd slab, the stand-alone field in both modes and a training step must leave every band
    byte untouched."""
    w = tmp_path / "guard_worker.py"
    w.write_text(_GUARD_WORKER)
    env = dict(os.environ, NEDDF_GUARD="1")
    p = subprocess.run([sys.executable, str(w), ROOT], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and "GUARD_OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
    n = int(p.stdout.split("bands_checked=")[1].split()[0])
    assert n > 500
    # the probe sees an overrun: with one band byte overwritten on purpose the same worker must fail at its first check
    p = subprocess.run([sys.executable, str(w), ROOT], env=dict(env, NEDDF_GUARD_SELFTEST="1"), capture_output=True, text=True, timeout=900)
    assert p.returncode != 0 and "GUARD_OK" not in p.stdout and "AssertionError" in p.stderr, p.stdout[-500:] + p.stderr[-1500:]
