#!/usr/bin/env python3
"""Headline benchmark: rendered rays/s on BASELINE.json configs[1]
(800x800 view, 128 stratified cone samples per ray, NeDDF fp32, one MI355X per
rank).  A "step" renders one full view per GPU: raygen -> stratified sampling
-> cone moments -> NeDDF field (distance trunk with the distance gradient in
reverse mode + colour trunk) -> wave-scan compositing, plus -- for N > 1 -- the RCCL gather of
the rendered pixels (20 B/ray) so that every rank ends the step with all N
views.  Weak scaling: N GPUs render N views.

    python bench.py --gpus 1 --steps 3 --warmup 1
    python bench.py --gpus 1 --steps 3 --warmup 1 --full --dump-outputs DIR
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Prints ONE JSON line on rank 0 (metric, value, unit, higher_is_better, dtype,
ms_per_step = milliseconds per timed step, ...), extended with
  roofline      the distance-trunk kernel (78 % of the step) against the fp32 MFMA
                peak, timed live with HIP events on its stream
A plain run sets up, warms up, times --steps steps and prints that line.  With
--full it then also measures and checks, outside the timed region:
  psnr_vs_oracle_db, parity_sample   the HIP pixels against the CPU oracle (asserted)
  value_incl_rng                     rays/s with the uniforms drawn inside the step
  alt_operand_policy                 the same workload under split-fp16 operands
  cpu_baseline  the CPU oracle (oracle/, a C port of the reference) on the host
                cores, on a bounded sample of the same workload (rank 0, N=1)
--dump-outputs DIR writes what the last timed step returned (rendered colour,
depth, transmittance per ray; for --workload train the loss and the updated
parameters) as DIR/<name>.npy.  The inputs are seeded: equal arguments, equal inputs.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WIDTH = HEIGHT = 800
SAMPLES = 128
CAMERA_ANGLE_X = 0.6911112070083618
# algorithmic work per field evaluation, shipped NeDDF architecture, eval-minimal:
#   distance trunk with the Jacobian carried FORWARD (the reference's formulation; NEDDF_DDF_REVERSE=0 and the training-mode
#   outputs): 4 rows x (60*256 + 4*256*256 + 316*256 + 256*256 + 256 [ddf head]) + 256 [aux head] MACs
DDF_FLOP_PER_POINT_FORWARD = 2 * (4 * (423936 + 256) + 256)
#   distance trunk with the distance gradient in REVERSE mode (eval-minimal under every operand policy, ddf_rev_kernel): value rows
#   forward (423 936 + both heads 512) + one gradient row backward (6 hidden transposes 393 216 + the encoding rows of W_0 and
#   of the skip layer 2 x 15 360) MACs -- the same function with half the matrix work
DDF_FLOP_PER_POINT_REVERSE = 2 * (423936 + 512 + 393216 + 2 * 15360)
DDF_FLOP_PER_POINT = DDF_FLOP_PER_POINT_FORWARD
#   colour trunk (value row only): 343*256 + 2*256*256 + 256*3 = 219 648 MACs
COL_FLOP_PER_POINT = 2 * 219648


def field_flops(cfg):
    """Algorithmic flop per field evaluation of a NeDDF configuration (the constants above are this at the shipped one):
    (distance trunk forward-mode, distance trunk reverse-mode, colour trunk value row)."""
    W, cpe, cdir = cfg["ddf_layer_width"], 6 * cfg["embed_pos_rank"], 6 * cfg["embed_dir_rank"]
    n_trunk, n_col, skips = cfg["ddf_layer_count"] - 1, cfg["col_layer_count"] - 1, list(cfg["skips"])
    wide = [l for l in range(1, n_trunk) if (l - 1) in skips]
    trunk = cpe * W + sum((W + (cpe if l in wide else 0)) * W for l in range(1, n_trunk))
    fwd = 4 * (trunk + W) + W
    rev = trunk + 2 * W + (n_trunk - 1) * W * W + (1 + len(wide)) * cpe * W
    col = (cpe + cdir + 3 + W) * W + (n_col - 1) * W * W + 3 * W
    return 2 * fwd, 2 * rev, 2 * col


assert field_flops(dict(ddf_layer_width=256, embed_pos_rank=10, embed_dir_rank=4, ddf_layer_count=8, col_layer_count=4, skips=[4])) == \
    (DDF_FLOP_PER_POINT_FORWARD, DDF_FLOP_PER_POINT_REVERSE, COL_FLOP_PER_POINT)
PEAK_FP32_MFMA_TFLOPS = 157.3          # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, 256 CU x 2.4 GHz
PEAK_BF16_MFMA_TFLOPS = 2500.0         # MI355X_MICROARCH.md: dense bf16, v_mfma_f32_32x32x16_bf16
# BASELINE.json configs[4] ("LLFF fern forward-facing, NDC rays, bf16 MLP weights"): fern at the customary 1/4 scale
C5_WIDTH, C5_HEIGHT, C5_FOCAL, C5_NEAR = 1008, 756, 815.13, 1.0


def view_pose(i):
    """Blender-convention camera on a radius-4.03 sphere looking at the origin (azimuth by view index)."""
    az, el, rad = 2 * math.pi * (i % 8) / 8 + 0.3, math.radians(30), 4.03
    pos = np.array([rad * math.cos(el) * math.cos(az), rad * math.cos(el) * math.sin(az), rad * math.sin(el)])
    back = pos / np.linalg.norm(pos)                     # camera looks down -z
    right = np.cross([0, 0, 1.0], back); right /= np.linalg.norm(right)
    up = np.cross(back, right)
    return np.stack([right, up, back], 1).astype(np.float32), pos.astype(np.float32)


def network_config(width=256):
    """The shipped bunny_smoke network (neddf_amd/fixtures: pretrained weights as arrays + the frozen run configuration); with
    another hidden width the same architecture on the deterministic synthetic weights of neddf_amd/fixtures/synth.py."""
    from neddf_amd.fixtures import BUNNY_SMOKE_CFG, bunny_smoke_weights, synth
    if width == 256:
        return dict(BUNNY_SMOKE_CFG), bunny_smoke_weights()
    cfg = dict(BUNNY_SMOKE_CFG, ddf_layer_width=width, col_layer_width=width)
    return cfg, dict(synth.neddf_state(cfg["embed_pos_rank"], cfg["embed_dir_rank"], cfg["ddf_layer_count"], width,
                                       cfg["col_layer_count"], width, tuple(cfg["skips"]), seed=7))


def build_render(dev, width=256, activation=None):
    """activation (probes only): another hidden activation on the same weights, e.g. "ReLU" to measure the mask-bit y' path."""
    import neddf_amd
    from neddf_amd.fixtures import BUNNY_SMOKE_RENDER
    net_cfg, wts = network_config(width)
    if activation:
        net_cfg = dict(net_cfg, activation_type=activation)
    render = neddf_amd.NeRFRender(dict(net_cfg, _target_="neddf.network.NeDDF"), **BUNNY_SMOKE_RENDER)
    render.network_fine.load_state_dict({k: torch.from_numpy(v) for k, v in wts.items()})
    render.to(dev)
    render.set_iter(-1)
    render.rng = "device"
    render.bench_network_config = net_cfg
    return render, wts


def host_cpu_limits():
    """What the process may actually use of the host: scheduler affinity and the cgroup CPU quota (a container often sees every
    logical CPU of the box in os.cpu_count() while its quota is a fraction of them -- which is where an OpenMP sweep stops scaling)."""
    info = {"logical_cpus": os.cpu_count()}
    try:
        info["sched_affinity"] = len(os.sched_getaffinity(0))
    except Exception:
        pass
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                info["cgroup_cpu_quota"] = "unlimited" if txt[0] == "max" else round(int(txt[0]) / int(txt[1]), 2)
            else:
                q = int(txt[0])
                info["cgroup_cpu_quota"] = "unlimited" if q < 0 else round(q / int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read()), 2)
            break
        except Exception:
            continue
    return info


def cpu_baseline(weights, net_cfg, R, T, calib, budget_s=20.0):
    """The path on the host cores, on a bounded sample of the same workload (rank 0, N = 1).  Two CPU implementations are timed:
    `value` = oracle/neddf_cpu_fast.c, the SAME algorithm as the HIP path (eval-minimal: value rows forward, reverse-mode
    distance gradient, colour trunk on value rows = 2.14 MFLOP/point at the shipped architecture) on blocked AVX-512 / AVX2 GEMM
    micro-kernels with OpenMP over 64-point blocks -- what a CPU implementation would do; `as_written` = oracle/neddf_oracle.c,
    the operation-by-operation port of the reference (Jacobian rows through both trunks + penalties = 5.15 MFLOP/point), the
    parity checker.  The OpenMP thread count is swept first (a container's affinity mask can exceed its CPU quota)."""
    from oracle import oracle as orc
    net = orc.NeDDFOracle(weights, **net_cfg)
    lib = orc.lib()
    rng = np.random.default_rng(0)

    def one_pass(n_rays, fast):
        idx = rng.integers(0, WIDTH * HEIGHT, n_rays)
        uv = np.stack([idx % WIDTH, idx // WIDTH], 1).astype(np.float32)
        U = rng.uniform(0, 1, (n_rays, SAMPLES)).astype(np.float32)
        t0 = time.perf_counter()
        rd, ro = orc.create_rays(uv, R, T, calib)
        d = orc.sample_coarse(U, 2.0, 6.0)
        smp = orc.sampling(rd, ro, d, 1.0 / 1111 / math.sqrt(12))
        v = net.forward_fast(*smp) if fast else net.forward(*smp)
        orc.integrate(d, v["density"], v["color"], 6.0)
        return n_rays / (time.perf_counter() - t0)

    avail = int(lib.orc_num_threads())
    t_start = time.perf_counter()
    sweep = {}
    for th in sorted({avail, max(avail // 2, 1), max(avail // 4, 1), min(avail, 64), min(avail, 32), min(avail, 16), min(avail, 8)}, reverse=True):
        lib.orc_set_num_threads(th)
        one_pass(2 * th, True)                        # warm the thread pool
        sweep[th] = one_pass(max(2048, 48 * th), True)      # large enough that the per-call weight packing and page faults do not decide the sweep
    best = max(sweep, key=sweep.get)
    lib.orc_set_num_threads(best)
    remaining = max(3.0, 0.6 * budget_s - (time.perf_counter() - t_start))
    n_rays = int(min(1 << 18, max(1024, sweep[best] * remaining * 0.8)))
    rate = one_pass(n_rays, True)
    # the as-written port on a smaller sample, same thread count as its own best (it stops scaling earlier: 16-32 threads)
    aw = {}
    for th in sorted({min(avail, 32), min(avail, 16)}):
        lib.orc_set_num_threads(th)
        one_pass(64, False)
        aw[th] = one_pass(max(256, 8 * th), False)
    aw_best = max(aw, key=aw.get)
    lib.orc_set_num_threads(aw_best)
    aw_rays = int(min(1 << 14, max(512, aw[aw_best] * 0.3 * budget_s)))
    aw_rate = one_pass(aw_rays, False)
    lib.orc_set_num_threads(avail)
    _, flop_rev, flop_col = field_flops(net_cfg)
    return {"value": rate, "unit": "rays/s", "cores": best, "host_logical_cpus": os.cpu_count(), "host": host_cpu_limits(), "openmp_max_threads": avail,
            "kind": "port",
            "simd": "avx512" if int(lib.fast_uses_avx512()) else "avx2",
            "flop_per_point": flop_rev + flop_col,
            "achieved_gflops": rate * SAMPLES * (flop_rev + flop_col) / 1e9,
            "sample": "%d random rays of the same 800x800 view, 128 samples/ray, through oracle/neddf_cpu_fast.c: the algorithm of the HIP "
                      "path (eval-minimal, reverse-mode distance gradient, %.2f MFLOP/point) on blocked GEMM micro-kernels, OpenMP thread "
                      "sweep %s rays/s -> %d threads of the box's %d logical CPUs"
                      % (n_rays, (flop_rev + flop_col) / 1e6, {k: round(v, 1) for k, v in sorted(sweep.items())}, best, os.cpu_count() or -1),
            "as_written": {"value": aw_rate, "unit": "rays/s", "cores": aw_best,
                           "sample": "%d rays through oracle/neddf_oracle.c, the operation-order-exact port of the reference (Jacobian rows "
                                     "through both trunks + penalties, 5.15 MFLOP/point, point-at-a-time loops): the parity checker, and "
                                     "what rounds 1-2 reported as the baseline" % aw_rays}}


def train_workload(args, dev, world=1, rank=0, use_dist=False):
    """One training step of the reference's configuration (config/trainer/neddf_trainer.yaml: 1024 rays, 64 + 128 samples, the
    three losses of config/loss/neddf_loss.yaml, Adam) on synthetic targets; uniforms drawn on the device.  With N ranks the
    step is data-parallel: 1024 rays per rank (weak scaling), one all-reduce of the flattened gradients per step."""
    import neddf_amd
    from neddf_amd.loss import ColorLoss, FieldsConstraintLoss, MaskBCELoss
    from neddf_amd.parallel import average_gradients
    from neddf_amd.fixtures import BUNNY_SMOKE_CFG, BUNNY_SMOKE_RENDER, bunny_smoke_weights
    rays = 1024
    wts = bunny_smoke_weights()
    cfg = dict(BUNNY_SMOKE_CFG, density_activation_type="ReLU", _target_="neddf.network.NeDDF")      # config/network/neddf.yaml default
    render = neddf_amd.NeRFRender(cfg, **BUNNY_SMOKE_RENDER)
    render.network_fine.load_state_dict({k: torch.from_numpy(v) for k, v in wts.items()})
    render.to(dev)
    render.set_iter(1500)
    render.rng = "device"
    render.network_fine.weight_dtype = {"f32": "fp32", "f16_split": "f16_split"}[args.dtype]
    fx = 0.5 * 400 / math.tan(0.5 * CAMERA_ANGLE_X)
    R, T = view_pose(0)
    cam = neddf_amd.Camera(neddf_amd.PinholeCalib(np.array([fx, fx, 200.0, 200.0])), None).to(dev)
    cam.R, cam.T = torch.from_numpy(R).to(dev), torch.from_numpy(T).to(dev)
    losses = [ColorLoss(1.0, 0.1), MaskBCELoss(0.05, 0.005), FieldsConstraintLoss(0.01, 0.01)]
    opt = torch.optim.Adam(render.get_parameters_list(), lr=5e-4)
    gen = torch.Generator(device="cpu").manual_seed(1 + rank)
    uv = (torch.rand(rays, 2, generator=gen) * 120 + 140).to(torch.int16).to(dev)
    target = {"color": torch.rand(rays, 3, generator=gen).to(dev), "mask": (torch.rand(rays, generator=gen) > 0.5).float().to(dev),
              "fields_penalty": torch.zeros(rays, device=dev)}

    def step():
        opt.zero_grad()
        out = render.render_rays(uv, cam)
        ld = {}
        for f in losses:
            ld.update(f(out, target))
        loss = torch.sum(torch.stack(list(ld.values())))
        loss.backward()
        if use_dist:
            average_gradients(render.get_parameters_list(), force_collective=True)
        opt.step()
        return loss

    def sync():
        if use_dist:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    for _ in range(max(args.warmup, 1)):
        step()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    sync()
    elapsed = time.perf_counter() - t0
    if use_dist:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs and rank == 0:     # what the step leaves its caller: the loss and the parameters after the optimiser step
        dump_outputs(args.dump_outputs, dict({"loss": loss.reshape(1)},
                                             **{"param." + k: v for k, v in render.network_fine.named_parameters()}))
    pts = rays * (65 + 194) * world
    # forward GEMMs (Jacobian rows everywhere, as the reference trains) + dX + dW: 3 x 2 x 4 x 644 096 MACs per point, minus the
    # input gradients of the first layers of both trunks, which are never needed
    flop = pts * (3 * 2 * 4 * 644096 - 2 * 4 * (60 * 256 + 87 * 256))
    achieved = flop * args.steps / elapsed / 1e12
    return {"metric": "training rays/sec (1024-ray steps, 65 coarse + 194 fine samples, NeDDF %s)" % ("fp32" if args.dtype == "f32" else args.dtype),
            "value": rays * world * args.steps / elapsed,
            "unit": "rays/s", "n_gpus": world, "steps": args.steps, "warmup": max(args.warmup, 1), "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": "training step: render_rays with autograd -> ColorLoss + MaskBCELoss + FieldsConstraintLoss -> backward -> "
                                   "Adam, shipped bunny_smoke weights, synthetic targets", "rays_per_step_per_gpu": rays,
                       "samples_per_ray": 65 + 194, "workload_id": "train",
                       "parallelism": "data-parallel x%d, one gradient all-reduce per step" % world},
            "roofline": {"bound": "mfma", "achieved": achieved / world, "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s",
                         "frac": achieved / world / PEAK_FP32_MFMA_TFLOPS, "traffic": None,
                         "kernel": "per GPU, whole step (forward + dX + dW GEMMs of both passes over wall time)"},
            "final_loss": float(loss.item())}


def preflight(world, share=False):
    """Fail in seconds, with a readable message, when this box cannot run `world` ranks (instead of a rendezvous timeout or an
    RCCL "Duplicate GPU" abort minutes later)."""
    if not torch.cuda.is_available():
        raise SystemExit("bench.py: no HIP device visible (torch.cuda.is_available() is False); the benchmark has no CPU path")
    n_dev = torch.cuda.device_count()
    if world > n_dev and not share:
        raise SystemExit("bench.py: --gpus %d but this process sees %d HIP device(s) (HIP_VISIBLE_DEVICES=%s, ROCR_VISIBLE_DEVICES=%s); "
                         "RCCL needs one device per rank.  NEDDF_BENCH_SHARE_GPU=1 runs the ranks on shared devices through gloo -- a "
                         "functional test mode, never a measurement" % (world, n_dev, os.environ.get("HIP_VISIBLE_DEVICES"),
                                                                        os.environ.get("ROCR_VISIBLE_DEVICES")))
    return n_dev


def self_launch(args):
    """`python bench.py --gpus N` without a launcher: re-execute under torch.distributed.run, one rank per GPU, and pass
    the ranks' stdout through (rank 0 prints the JSON line).  Every rank's stderr goes to its own file; when the run fails, the
    tail of each is printed, so that the rank that died first can be told from the ranks that died of it."""
    import glob
    import socket
    import subprocess
    import tempfile
    preflight(args.gpus, os.environ.get("NEDDF_BENCH_SHARE_GPU") == "1")
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    logs = tempfile.mkdtemp(prefix="neddf_bench_ranks_")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), "--log-dir", logs, "--redirects", "2", os.path.abspath(__file__)] + sys.argv[1:]
    sys.stdout.flush()
    rc = subprocess.run(cmd, env=env).returncode
    if rc != 0:
        for path in sorted(glob.glob(os.path.join(logs, "**", "stderr.log"), recursive=True)):
            try:
                tail = open(path, errors="replace").read()[-1500:]
            except OSError:
                continue
            sys.stderr.write("---- %s (tail) ----\n%s\n" % (os.path.relpath(path, logs), tail))
        sys.stderr.write("bench.py: the %d-rank run failed with exit code %d (per-rank stderr under %s)\n" % (args.gpus, rc, logs))
    raise SystemExit(rc)


def _kernel_matches(name, kernel_substr, dtype, masked):
    """Is `name` (a demangled kernel name from rocprofv3) the dominant kernel of this run?  ddf_rev_kernel<MT, NW, WPS, Ops, MASKY, FUSED>:
    the operand policy and the MASKY flag (ReLU / LeakyReLU: y' as mask bits) select the instantiation; FUSED defaults to false."""
    if kernel_substr not in name:
        return False
    if ("OpsBF16" in name) != (dtype == "bf16") or ("OpsF16Split" in name) != (dtype == "f16_split"):
        return False
    if kernel_substr != "ddf_rev_kernel":
        return True
    head = name.split("(")[0]
    flags = [a.strip() for a in head[head.index("<") + 1:head.rindex(">")].split(",") if a.strip() in ("true", "false")]
    return bool(flags) and (flags[0] == "true") == masked


def measured_traffic(kernel_substr, dtype, masked):
    """HBM bytes per launch of the dominant kernel measured NOW (opt-in: NEDDF_BENCH_PMC=1; the default line reads the committed, calibrated table) --
    two rocprofv3 --pmc passes (FETCH_SIZE, then WRITE_SIZE: the TCC has four counter slots, FETCH_SIZE takes three) over
    tools/pmc_probe.py, which renders one 65 536-ray x 128-sample slab of the same workload (ONE launch of 2^23 points at the default
    launch size).  bytes = (2.000 x FETCH_SIZE + 1.000 x WRITE_SIZE) x 1024: both counters are in KB, and on gfx950 FETCH_SIZE reports half of
    the bytes read (128-byte requests tallied at 64) -- factors calibrated ON THE BOX for this kernel's access patterns (tools/traffic_calib.hip,
    profiles/r06_traffic_calib.txt: 2.000 / 1.000 for 16 B per lane cold, Infinity-Cache-warm, written-then-read-back, and 4 B per lane).  Counter passes run with --kernel-trace only (no hip /
    hsa / memory-copy tracing).  A dispatch may come as several rows (per XCD / dimension): values are SUMMED per Dispatch_Id and the
    mean is over distinct dispatches."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    if shutil.which("rocprofv3") is None:
        raise RuntimeError("rocprofv3 not on PATH")
    vals = {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        out = tempfile.mkdtemp(prefix="neddf_pmc_", dir="/tmp")
        env = dict(os.environ, TMPDIR="/tmp", NEDDF_PROBE_DTYPE={"f32": "fp32"}.get(dtype, dtype), NEDDF_BENCH_PMC="0")
        subprocess.run(["rocprofv3", "--pmc", counter, "--kernel-trace", "-d", out, "--output-format", "csv", "--", sys.executable,
                        os.path.join(ROOT, "tools", "pmc_probe.py"), "1"], cwd="/tmp", env=env, check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL, timeout=300)
        per = {}
        for path in glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True):
            for r in csv.DictReader(open(path)):
                if r["Counter_Name"] == counter and _kernel_matches(r["Kernel_Name"], kernel_substr, dtype, masked):
                    key = (path, r.get("Dispatch_Id", len(per)))
                    per[key] = per.get(key, 0.0) + float(r["Counter_Value"])
        shutil.rmtree(out, ignore_errors=True)
        if not per:
            raise RuntimeError("no %s rows for %s" % (counter, kernel_substr))
        vals[counter] = sum(per.values()) / len(per)
        vals[counter + "_dispatches"] = len(per)
    if vals["FETCH_SIZE_dispatches"] != vals["WRITE_SIZE_dispatches"]:
        raise RuntimeError("the two counter passes saw different dispatch counts: %r" % (vals,))
    # factors calibrated on the box (tools/traffic_calib.hip, profiles/r06_traffic_calib.txt): reads 2.000, writes 1.000
    vals["read_bytes"] = 2.0 * vals["FETCH_SIZE"] * 1024.0
    vals["write_bytes"] = 1.0 * vals["WRITE_SIZE"] * 1024.0
    vals["hbm_bytes_per_launch"] = vals["read_bytes"] + vals["write_bytes"]
    vals["points_per_dispatch"] = 65536.0 * 128 / vals["FETCH_SIZE_dispatches"]     # tools/pmc_probe.py renders ONE 65 536-ray x 128-sample slab
    return vals


def psnr_vs_oracle(render, ctx, cam, weights, R, T, calib, U, n_sample=256, lo=0):
    """PSNR (data range 1.0) of the HIP path's pixel colours against the CPU oracle on a sample of the benchmarked view's
    rays with the same uniforms (outside the timed region; BASELINE.json's metric reads "...; PSNR vs ref")."""
    from neddf_amd._lib import SLOT_FINE
    from oracle import oracle as orc
    dev = U.device
    gen = torch.Generator(device="cpu").manual_seed(99)
    idx = torch.randint(0, U.shape[0], (n_sample,), generator=gen)       # U holds this rank's slab [lo, lo + len(U)) of the pixel index
    pix = idx + lo
    uv = torch.stack([pix % WIDTH, pix // WIDTH], 1).to(dev)
    Us = U[idx.to(dev)].contiguous()
    out = dict(color=torch.empty(n_sample, 3, device=dev), depth=torch.empty(n_sample, device=dev),
               transmittance=torch.empty(n_sample, device=dev))
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    ctx.render_rays(uv, cam.descriptor(), render._params(), Us, None, dict(out, nan_flag=flag), single_slot=SLOT_FINE)
    torch.cuda.synchronize()
    net = orc.NeDDFOracle(weights, **render.bench_network_config)
    rd, ro = orc.create_rays(uv.cpu().numpy().astype(np.float32), R, T, calib.astype(np.float32))
    d = orc.sample_coarse(Us.cpu().numpy(), float(render.dist_near), float(render.dist_far))
    v = net.forward(*orc.sampling(rd, ro, d, 1.0 / 1111 / math.sqrt(12)))
    ref = orc.integrate(d, v["density"], v["color"], float(render.max_dist))
    mse = float(np.mean((out["color"].cpu().numpy().astype(np.float64) - ref["color"].astype(np.float64)) ** 2))
    worst = {k: float(np.max(np.abs(out[k].cpu().numpy() - ref[k]))) for k in ("color", "depth", "transmittance")}
    # how far inside the north-star gate (|a - b| <= 1e-4 |b| + 1e-5) the worst element of each output sits (<= 1 passes)
    margin = {k: float(np.max(np.abs(out[k].cpu().numpy().astype(np.float64) - ref[k]) / (1e-4 * np.abs(ref[k].astype(np.float64)) + 1e-5)))
              for k in ("color", "depth", "transmittance")}
    return (10 * math.log10(1.0 / mse) if mse > 0 else float("inf")), worst, n_sample, margin


DUMP_BUDGET_BYTES = 64 * 1000 * 1000        # 64 MB in all, read strictly


def dump_outputs(path, arrays):
    """--dump-outputs: `arrays` ({name: tensor}) as path/<name>.npy in float32 (float64 stays float64).  Past 64 MB in all, every
    array with the shared leading dimension keeps the same fixed, seeded sample of rows, and sample_rows.npy records which."""
    os.makedirs(path, exist_ok=True)
    arrays = {k: v.detach().cpu().numpy() for k, v in arrays.items()}
    arrays = {k: v if v.dtype == np.float64 else v.astype(np.float32) for k, v in arrays.items()}
    total = sum(v.nbytes for v in arrays.values())
    if total > DUMP_BUDGET_BYTES:
        n = max(v.shape[0] for v in arrays.values() if v.ndim)
        per_row = 8 + sum(v.nbytes // n for v in arrays.values() if v.ndim and v.shape[0] == n)     # 8: the row's entry in sample_rows
        fixed = sum(v.nbytes for v in arrays.values() if not (v.ndim and v.shape[0] == n))
        keep = (DUMP_BUDGET_BYTES - fixed - 4096) // per_row
        rows = np.sort(np.random.default_rng(0).choice(n, keep, replace=False))
        arrays = {k: v[rows] if v.ndim and v.shape[0] == n else v for k, v in arrays.items()}
        arrays["sample_rows"] = rows.astype(np.float64)
    for k, v in arrays.items():
        np.save(os.path.join(path, k + ".npy"), v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure and check what the headline figure does not need: the parity sample "
                         "against the CPU oracle (psnr_vs_oracle_db, asserted), the RNG-inclusive rates, the split-fp16 operand "
                         "policy, the CPU baseline and (NEDDF_BENCH_PMC=1) the in-run PMC passes.  Off by default")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path returned in its last step as DIR/<name>.npy (float32; "
                         "a fixed row sample when the arrays exceed 64 MB in all)")
    ap.add_argument("--workload", choices=["c2", "c3", "c5", "train"], default="c2",
                    help="c2 = BASELINE configs[1] (headline, default; with --gpus N > 1 it is configs[3]: N views, rays sharded one "
                         "view per GPU, RCCL pixel gather); c3 = configs[2], 65 coarse + 129 importance samples; "
                         "c5 = configs[4], 1008x756 forward-facing view, NDC rays, hierarchical sampling, bf16 operands; "
                         "train = one training step (SURVEY 8f item 2): 1024 rays x (65 + 194) samples, losses, backward, Adam")
    ap.add_argument("--width", type=int, default=256,
                    help="hidden width of the NeDDF (default 256 = the shipped network and its pretrained weights; any other width "
                         "in [1, 512] runs the same architecture on synthetic weights -- a supplementary line, never the headline)")
    ap.add_argument("--dtype", choices=["f32", "bf16", "f16_split"], default=None,
                    help="operand type of the 256-wide layers (default f32 = fp32 MFMA; c5 defaults to bf16; f16_split = fp32 data, "
                         "operands split into two fp16 terms, three fp16 MFMAs per multiply-add)")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                    help="weak (default): every GPU renders its own 800x800 view, N views per step (BASELINE configs[3]); strong: ONE "
                         "800x800 view per step, its rays cut into N contiguous chunk-granular slabs (render_image's pixel_range, "
                         "neddf_shard_range_granular), pixels all-gathered by neddf_gather_pixels_granular -- north_star's 'rays shard "
                         "across the GPUs' read literally.  c2 only")
    args = ap.parse_args()
    if args.scaling == "strong" and args.workload != "c2":
        raise SystemExit("bench.py: --scaling strong exists for the c2 workload")
    # dmabuf IPC for RCCL / cross-process device memory (the host driver supports nothing else): must be in the environment before
    # the HIP runtime initialises, i.e. before the first torch.cuda call below
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if args.dtype is None:
        args.dtype = "bf16" if args.workload == "c5" else "f32"
    global WIDTH, HEIGHT
    if args.workload == "c5":
        WIDTH, HEIGHT = C5_WIDTH, C5_HEIGHT

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus, "WORLD_SIZE=%d but --gpus %d" % (world, args.gpus)
    n_dev = preflight(world, os.environ.get("NEDDF_BENCH_SHARE_GPU") == "1")
    # NEDDF_BENCH_SHARE_GPU=1 (test mode for boxes with fewer GPUs than ranks): ranks share devices and the pixel gather is
    # staged through gloo, because RCCL refuses two ranks on one device.  Never a measurement; the line says so.
    share = os.environ.get("NEDDF_BENCH_SHARE_GPU") == "1" and world > n_dev
    local = local % n_dev
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    # NEDDF_BENCH_FORCE_DIST=1 runs the N > 1 code path (communicator, pixel all-gather, max-over-ranks) with one rank
    use_dist = world > 1 or os.environ.get("NEDDF_BENCH_FORCE_DIST") == "1"
    if use_dist:
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        if share:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    import neddf_amd
    from neddf_amd.parallel import gather_pixels, native_comm, pack_pixels
    if args.workload == "train":
        line = train_workload(args, dev, world, rank, use_dist)
        if use_dist:
            torch.distributed.destroy_process_group()
        if rank == 0:
            import ctypes
            ctypes.CDLL(None).fflush(None)
            print(json.dumps(line), flush=True)
        return
    render, weights = build_render(dev, args.width)
    render.network_fine.weight_dtype = {"f32": "fp32", "bf16": "bf16", "f16_split": "f16_split"}[args.dtype]
    fx = 0.5 * WIDTH / math.tan(0.5 * CAMERA_ANGLE_X)
    calib = np.array([fx, fx, WIDTH / 2.0, HEIGHT / 2.0])
    strong = args.scaling == "strong"
    R, T = view_pose(0 if strong else rank)      # strong scaling: every rank renders its slab of the SAME view
    if args.workload == "c5":       # forward-facing: camera near the origin looking down -z, NDC depths 0..1, point samples
        calib = np.array([C5_FOCAL, C5_FOCAL, WIDTH / 2.0, HEIGHT / 2.0])
        R, T = np.eye(3, dtype=np.float32), np.array([0.05 * rank, -0.02, 0.1], np.float32)
        render.sampling_type, render.dist_near, render.dist_far, render.max_dist = "point", 0.0, 1.0, 1.0
        render.ray_space, render.ndc_width, render.ndc_height, render.ndc_near = "ndc", WIDTH, HEIGHT, C5_NEAR
    cam = neddf_amd.Camera(neddf_amd.PinholeCalib(calib), None).to(dev)
    cam.R, cam.T = torch.from_numpy(R).to(dev), torch.from_numpy(T).to(dev)
    n_rays = WIDTH * HEIGHT
    # strong scaling: this rank's contiguous slab of the flat pixel index, cut on render_image's chunk (512 rays) like
    # parallel.render_image_sharded / neddf_shard_range_granular do -- no chunk is split between two ranks
    from neddf_amd.parallel import shard_range
    GRANULE = 512
    slab_lo, slab_hi = shard_range(n_rays, rank, world, GRANULE) if strong else (0, n_rays)
    n_local = slab_hi - slab_lo
    n_total = n_rays if strong else n_rays * world            # pixels every rank ends a step with
    # synthetic inputs resident in HBM before the timed region
    U = torch.rand(n_local, SAMPLES, device=dev, generator=torch.Generator(device=dev).manual_seed(1234 + rank))
    ctx = render._ctx(dev)
    keys = ("color", "depth", "transmittance")
    idx = torch.arange(n_rays, device=dev)
    uv_all = torch.stack([idx % WIDTH, idx // WIDTH], 1)
    samples_per_ray = SAMPLES if args.workload == "c2" else 65 + 194
    cam_desc = cam.descriptor()

    if args.workload in ("c3", "c5"):
        U_c = torch.rand(n_rays, 65, device=dev)
        U_f = torch.rand(n_rays, 129, device=dev)

    # multi-GPU exchange: the HIP library's own RCCL communicator (neddf_comm_init / neddf_gather_pixels); torch.distributed
    # only bootstraps it and provides the barrier / max-over-ranks of the timing contract
    comm = {"world_size": world, "gather": "none (single rank)"}
    if use_dist:
        comm["torch_distributed_world_size"] = torch.distributed.get_world_size()
        comm["backend"] = str(torch.distributed.get_backend())
        if share:
            comm["gather"] = "gloo, staged through the host (NEDDF_BENCH_SHARE_GPU test mode: NOT a measurement)"
        else:
            try:
                info = native_comm(ctx)
                comm.update(gather="neddf_gather_pixels%s: library-owned RCCL communicator, all-gather on its own stream, "
                                   "overlapped with the next view's render" % ("_granular" if strong else ""), rccl_comm_ranks=info["nranks"],
                            rccl_version=info["rccl_version"])
                if info["nranks"] != world:
                    raise SystemExit("bench.py: the library's RCCL communicator came up with %d ranks, %d were launched" % (info["nranks"], world))
            except Exception as e:      # a second RCCL route, never a CPU path: torch.distributed's all_gather_into_tensor
                comm.update(gather="torch.distributed all_gather_into_tensor (RCCL); library communicator failed: %s" % e)
    native = use_dist and "rccl_comm_ranks" in comm
    gathered = [torch.empty(n_total, 5, device=dev) for _ in range(2)] if use_dist else None
    nan_flags = []
    state = {"i": 0, "pending": None, "last_packed": None}

    def render_view():
        if args.workload in ("c3", "c5"):
            parts = {k: [] for k in keys}
            for lo in range(0, n_rays, render.rays_per_call):
                hi = min(n_rays, lo + render.rays_per_call)
                o = render._render(ctx, uv_all[lo:hi], cam, U_c[lo:hi], U_f[lo:hi], full=False, cam_desc=cam_desc)
                nan_flags.append(o["_nan"])
                for k in keys:
                    parts[k].append(o[k])
            return {k: torch.cat(v) for k, v in parts.items()}
        out = render.render_image_single_pass(WIDTH, HEIGHT, cam, SAMPLES, U=U, pixel_range=(slab_lo, slab_hi) if strong else None)
        nan_flags.append(out["_nan"])
        return out

    def step():
        out = render_view()
        if not use_dist:
            return out
        packed = pack_pixels(out, keys)
        state["last_packed"] = packed
        if native:          # every rank ends with all N views [N * n_rays, 5]; view i's pixels travel while view i+1 renders
            if state["pending"] is not None:
                state["pending"].wait()
            state["pending"] = gather_pixels(packed, n_total, force_collective=True, wait=False, out=gathered[state["i"] & 1],
                                             granule=GRANULE if strong else 1)
            state["i"] += 1
            return state["pending"]
        if share:
            full = gather_pixels(packed.cpu(), n_total, force_collective=True, granule=GRANULE if strong else 1)
            gathered[0].copy_(full)
            return gathered[0]
        if strong:          # ragged slabs: only the library's granular gather (or the gloo test route) assembles them
            raise SystemExit("bench.py: --scaling strong needs the library's RCCL communicator (neddf_gather_pixels_granular): %s" % comm["gather"])
        full = packed.new_empty(world * n_rays, 5)
        torch.distributed.all_gather_into_tensor(full, packed)
        return full

    def sync():
        if state["pending"] is not None:
            if native:      # host-side wait with a deadline: a peer that died or a stuck collective ends the bench with
                ctx.comm_wait_host(300000)      # NEDDF_ETIMEOUT / the asynchronous RCCL error instead of hanging it
            state["pending"].wait()
            state["pending"] = None
        if use_dist:
            torch.cuda.synchronize()
            torch.distributed.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    sync()
    ctx.set_timing(True)
    ctx.get_timings()
    nan_flags.clear()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        res = step()
    sync()
    elapsed = time.perf_counter() - t0
    stage = ctx.get_stage_timings()
    ctx.set_timing(False)
    tm = dict(ddf_ms=stage["ddf"][0], col_ms=stage["col"][0], ddf_launches=stage["ddf"][1], col_launches=stage["col"][1])
    if use_dist:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if share else dev)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())
    nan = int(torch.stack(nan_flags).sum().item()) if nan_flags else 0          # every batch of every step
    assert nan == 0, "NaN weight in integrate_volume_render"
    if use_dist and native:       # the gathered frame must hold this rank's own view at its slab
        full = res.out if hasattr(res, "out") else res
        assert full.shape[0] == n_total and torch.isfinite(full).all(), "gathered frame incomplete"
        off = slab_lo if strong else rank * n_rays
        assert torch.equal(full[off:off + n_local], state["last_packed"]), "the gathered frame does not hold this rank's pixels at its slab"
    if args.dump_outputs and rank == 0:
        if use_dist:        # what every rank ends the step with: the whole gathered frame, [n_total] rays
            from neddf_amd.parallel import unpack_pixels
            full = unpack_pixels(res.out if hasattr(res, "out") else res, keys)
            dump_outputs(args.dump_outputs, {k: v.reshape(v.shape[0]) if v.shape[1] == 1 else v for k, v in full.items()})
        else:
            dump_outputs(args.dump_outputs, {k: res[k] for k in keys})

    if rank == 0:
        pts = n_local * samples_per_ray * args.steps              # field evaluations on this rank
        ddf_s = tm["ddf_ms"] / 1e3
        # the library's rule (neddf_capi.hip field_forward): fp32 eval-minimal takes the reverse-mode kernel unless switched off
        reverse = os.environ.get("NEDDF_DDF_REVERSE", "1") != "0"
        flop_fwd, flop_rev, flop_col = field_flops(render.bench_network_config)
        DDF_FLOP_PER_POINT = flop_rev if reverse else flop_fwd
        achieved = pts * DDF_FLOP_PER_POINT / ddf_s / 1e12 if ddf_s > 0 else 0.0
        peak = PEAK_FP32_MFMA_TFLOPS
        if args.dtype == "bf16":
            peak = PEAK_BF16_MFMA_TFLOPS
        elif args.dtype == "f16_split":   # three fp16 products per multiply-add (fp16 and bf16 MFMA run at the same rate)
            peak = PEAK_BF16_MFMA_TFLOPS / 3
        net_name = ("shipped bunny_smoke weights" if args.width == 256 else
                    "SUPPLEMENTARY hidden width %d (same architecture, synthetic weights; engine width %d)" % (args.width, -(-args.width // 128) * 128))
        c2_name = ("BASELINE.json configs[1]: 800x800 view, 128 stratified cone samples/ray, NeDDF (8x%d distance trunk, distance gradient %s"
                   " + 4x%d colour trunk on value rows) %s, 1 view per GPU per step, synthetic poses, %s"
                   % (args.width, "in reverse mode (value rows forward, one gradient row backward)" if reverse else
                      "as forward-mode Jacobian rows (the reference's formulation)", args.width, args.dtype, net_name))
        if strong:
            c2_name = ("STRONG scaling of BASELINE.json configs[1]: ONE 800x800 view per step, its 640 000 rays cut into %d contiguous "
                       "chunk-granular slabs (512-ray chunks, neddf_shard_range_granular), one slab per MI355X, RCCL all-gather of the "
                       "rendered pixels (20 B/ray) so that every rank ends with the whole view; 128 stratified cone samples/ray, NeDDF %s, "
                       "distance gradient %s" % (world, args.dtype, "in reverse mode" if reverse else "as forward-mode Jacobian rows"))
        elif world > 1:
            c2_name = ("BASELINE.json configs[3]: %d-view batch 800x800 (8 azimuths), rays sharded one view per GPU over %d x MI355X "
                       "(contiguous slabs of the flat pixel index), RCCL all-gather of the rendered pixels (20 B/ray) so that every "
                       "rank ends with all %d views; per-GPU work = configs[1] (128 stratified cone samples/ray, NeDDF %s)"
                       % (world, world, world, args.dtype))
        line = {
            "metric": {"c2": "rendered rays/sec (800x800, 128 samples/ray)",
                       "c3": "rendered rays/sec (800x800, 65 coarse + 194 fine hierarchical samples/ray)",
                       "c5": "rendered rays/sec (1008x756 forward-facing NDC view, 65 coarse + 194 fine samples/ray)"}[args.workload],
            "value": n_total * args.steps / elapsed,
            "unit": "rays/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
            "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": {"c2": c2_name,
                                    "c3": "BASELINE.json configs[2]: as configs[1] with render_rays' hierarchical sampling "
                                          "(65 coarse + 129 importance samples merged to 194), %s" % args.dtype,
                                    "c5": "BASELINE.json configs[4]: 1008x756 forward-facing view (fern at 1/4 scale), NDC rays, "
                                          "point samples, hierarchical 65 + 194, NeDDF with %s operands" % args.dtype}[args.workload],
                       "rays_per_step_per_gpu": n_local, "rays_per_step": n_total, "samples_per_ray": samples_per_ray, "workload_id": args.workload,
                       "parallelism": "ray-parallel x%d%s" % (world, " (one view, chunk-granular pixel slabs)" if strong else ""), "comm": comm},
            "roofline": {"bound": "mfma", "achieved": achieved, "peak": peak, "unit": "TFLOP/s",
                         "frac": achieved / peak, "traffic": None,
                         "kernel": "neddf::ddf_rev_kernel" if reverse else "neddf::ddf_trunk_kernel", "launches": tm["ddf_launches"],
                         "avg_launch_ms": tm["ddf_ms"] / max(tm["ddf_launches"], 1),
                         "flop_per_point": DDF_FLOP_PER_POINT,
                         "algorithm": ("distance gradient in reverse mode: value rows forward + one gradient row backward = 2 rows of matrix "
                                       "work per point and layer; `achieved` / `frac` count THESE flops" if reverse else
                                       "Jacobian rows carried forward (value + 3 rows per point), the reference's formulation"),
                         "forward_mode_flop_per_point": flop_fwd,
                         "forward_mode_equivalent_tflops": (pts * flop_fwd / ddf_s / 1e12) if ddf_s > 0 else 0.0,
                         "colour_kernel": {"avg_launch_ms": tm["col_ms"] / max(tm["col_launches"], 1),
                                           "flop_per_point": flop_col,
                                           # the hierarchical workloads skip the colour trunk on the coarse pass (its colours are not an output)
                                           "points_per_ray": SAMPLES if args.workload == "c2" else 194,
                                           "achieved": ((pts if args.workload == "c2" else n_local * 194 * args.steps) * flop_col / (tm["col_ms"] / 1e3) / 1e12)
                                                       if tm["col_ms"] > 0 else 0.0}},
            # every stage kernel of the timed region (HIP events on its stream): summed ms per step and launches per step
            "stage_ms_per_step": {k: round(v[0] / args.steps, 4) for k, v in stage.items() if v[1]},
        }
        try:        # HBM bytes per launch (PMC passes exist for the headline workload under the fp32 and bf16 policies)
            if args.dtype not in ("f32", "bf16") or args.workload != "c2" or args.width != 256:
                raise KeyError("no PMC pass for this workload")
            # HBM bytes per launch of the dominant kernel, from the committed PMC passes (bench.py cannot run rocprofv3 on itself)
            pmc = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
            want = "ddf_rev_kernel" if reverse else "ddf_trunk_kernel"
            masked = render.bench_network_config["activation_type"] != "tanhExp"      # ReLU / LeakyReLU: the mask-bit kernel
            ent = next(v for k, v in pmc.items() if _kernel_matches(k, want, args.dtype, masked))
            # the committed pass measured launches of ent["points_per_launch"] points; this run's launches may be larger (the per-point
            # traffic of these kernels does not depend on the launch size: per-workgroup scratch, per-point hand-off)
            per_launch = pts / max(tm["ddf_launches"], 1)
            scale = per_launch / float(ent.get("points_per_launch", per_launch))
            ent = dict(ent, hbm_bytes_per_launch=ent["hbm_bytes_per_launch"] * scale,
                       algorithmic_bytes_per_launch=ent["algorithmic_bytes_per_launch"] * scale)
            line["roofline"]["points_per_launch"] = per_launch
            line["roofline"]["traffic"] = ent["hbm_bytes_per_launch"]
            line["roofline"]["traffic_source"] = ("%s: a committed rocprofv3 --pmc pass of this kernel at this launch size (FETCH_SIZE, WRITE_SIZE in separate passes, "
                                                  "--kernel-trace only), scaled per point; NEDDF_BENCH_PMC=1 measures it in the run instead" % ent["source"])
            if "calibration" in ent:
                line["roofline"]["traffic_calibration"] = ent["calibration"]
            bd = ent.get("breakdown")
            if bd:      # what the bytes are: the design's stores and scratch reads, and the weight fragments that missed L2 (named counters: TCC_HIT / TCC_MISS)
                line["roofline"]["traffic_breakdown"] = {k: (v * scale if k not in ("l2_hit_rate",) else v) for k, v in bd.items()}
            # NEDDF_BENCH_PMC=1: measured in this run (two extra passes over a one-slab probe, outside the timed region, ~1 min, while this
            # process keeps its context); default: the committed, calibrated table above
            if args.full and os.environ.get("NEDDF_BENCH_PMC", "") == "1" and world == 1:
                try:
                    m = measured_traffic(want, args.dtype, masked)
                    # the probe's launches must be of this run's size (one 65 536-ray slab = one launch at the default cap): per-point traffic
                    # of these kernels moved by +55 % between 2^21- and 2^23-point launches, so a mismatch is an error, not a scale factor
                    if not 0.5 < m["points_per_dispatch"] / per_launch < 2.0:
                        raise RuntimeError("probe dispatches hold %.0f points, this run's launches %.0f" % (m["points_per_dispatch"], per_launch))
                    k = per_launch / m["points_per_dispatch"]
                    m["hbm_bytes_per_launch"] *= k
                    line["roofline"]["traffic"] = m["hbm_bytes_per_launch"]
                    line["roofline"]["traffic_source"] = ("measured in this run: rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate passes, "
                                                          "--kernel-trace only) over tools/pmc_probe.py, %d dispatch(es) of one 65 536-ray slab, scaled to this run's launch size; bytes = "
                                                          "2.000 x FETCH_SIZE x 1024 + 1.000 x WRITE_SIZE x 1024 (factors calibrated on the box)" % m["FETCH_SIZE_dispatches"])
                    line["roofline"]["traffic_counters_kb"] = {"FETCH_SIZE": m["FETCH_SIZE"], "WRITE_SIZE": m["WRITE_SIZE"]}
                    line["roofline"]["traffic_static"] = ent["hbm_bytes_per_launch"]
                    if bd:
                        tb = line["roofline"]["traffic_breakdown"]
                        tb.update(write=m["write_bytes"] * k, read=m["read_bytes"] * k, weight_refetch=m["read_bytes"] * k - tb["designed_read"])
                        tb["note"] = "write / read / weight_refetch from this run's counters; the TCC hit / miss counts from the committed pass"
                    ent = dict(ent, hbm_bytes_per_launch=m["hbm_bytes_per_launch"])
                except Exception as e:
                    line["roofline"]["traffic_source"] += "; the in-run PMC pass failed: %r" % (e,)
            if bd:
                tb = line["roofline"]["traffic_breakdown"]
                line["roofline"]["traffic_explained"] = (
                    "traffic = fabric-side bytes (L2 misses; Infinity-Cache hits included).  %.1f GB written (design: %.1f) + %.1f GB read = %.1f GB of "
                    "per-workgroup scratch read back once (y' of every layer, parked gradients) + %.1f GB of WEIGHT fragments that missed the 4 MB L2 slices "
                    "(%.0f %% of the %.0f GB the tiles pull through L2; TCC hit rate %.1f %%, TCC_MISS x 128 B = %.1f GB in the committed pass)"
                    % (tb["write"] / 1e9, tb["designed_write"] / 1e9, tb["read"] / 1e9, tb["designed_read"] / 1e9, tb["weight_refetch"] / 1e9,
                       100 * tb["weight_refetch"] / tb["weight_stream_from_l2"], tb["weight_stream_from_l2"] / 1e9, 100 * tb["l2_hit_rate"], tb["tcc_miss_x_128B"] / 1e9))
            line["roofline"]["algorithmic_hbm_bytes_per_launch"] = ent["algorithmic_bytes_per_launch"]
            # the same launch against the HBM roofline (the 16-bit policies are partly bound by the y' round trip)
            ms = line["roofline"]["avg_launch_ms"]
            if ms > 0:
                line["roofline"]["hbm"] = {"achieved": ent["hbm_bytes_per_launch"] / (ms * 1e-3) / 1e9, "peak": 8000.0, "unit": "GB/s",
                                           "frac": ent["hbm_bytes_per_launch"] / (ms * 1e-3) / 8e12}
        except Exception:
            pass
        # --full: the parity sample against the oracle, the RNG-inclusive rates, the other operand policy, the CPU baseline
        if args.full and args.workload == "c2":
            psnr, worst, ns, margin = psnr_vs_oracle(render, ctx, cam, weights, R, T, calib, U, lo=slab_lo)
            line["psnr_vs_oracle_db"] = psnr
            line["parity_sample"] = {"rays": ns, "max_abs_err": worst, "gate_margin": margin,
                                     "oracle": "oracle/neddf_oracle.c (pinned on the reference's goldens)",
                                     "note": "same rays, same uniforms, outside the timed region; gate_margin = max |a-b| / (1e-4 |b| + 1e-5), "
                                             "asserted <= 1 for the fp32 and split-fp16 policies (bf16 is held to PSNR only)"}
            # a benchmark line of a renderer that disagrees with the reference is not a measurement: fail instead of printing it
            if os.environ.get("NEDDF_BENCH_PROBE") == "1":       # timing-probe libraries (make variant ... -DNEDDF_PROBE_*): results are invalid BY DESIGN
                line["metric"] = "INVALID (timing probe build): " + line["metric"]
            elif args.dtype != "bf16":
                assert max(margin.values()) <= 1.0 and psnr > 120.0, "parity sample outside the 1e-4 + 1e-5 gate: %s, PSNR %.1f dB" % (margin, psnr)
            else:
                assert psnr > 60.0, "bf16 parity sample: PSNR %.1f dB" % psnr
        if args.full and world == 1 and args.workload == "c2":
            # SURVEY 8d counts RNG generation/upload into rays/s; `value` keeps its inputs resident, these two add the draw
            line["value_incl_rng"] = rng_inclusive(render, cam, n_rays, dev)
        if args.full and world == 1 and args.workload == "c2" and args.dtype == "f32":
            # supplementary: the same workload under the split-fp16 operand policy (fp32 data, fp32-level errors);
            # `value` above stays the exact fp32 MFMA path
            render.network_fine.weight_dtype = "f16_split"
            step()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(2):
                step()
            torch.cuda.synchronize()
            line["alt_operand_policy"] = {"dtype": "f16_split (fp32 operands as two fp16 terms, three fp16 MFMAs per multiply-add, fp32 accumulation)",
                                          "value": n_rays * 2 / (time.perf_counter() - t1), "unit": "rays/s", "steps": 2,
                                          "parity": "same 1e-4 gates as the fp32 path (tests/test_gpu_c5.py)"}
            render.network_fine.weight_dtype = "fp32"
        if args.full and world == 1 and not args.no_cpu_baseline and args.workload != "c5":
            line["cpu_baseline"] = cpu_baseline(weights, render.bench_network_config, R, T, calib.astype(np.float32))
    if use_dist:
        torch.distributed.barrier()
        if native:
            ctx.comm_destroy()
        torch.distributed.destroy_process_group()
    if rank == 0:
        # RCCL prints a version banner through C stdio; flush it first so that the JSON line is the last line of stdout
        import ctypes
        ctypes.CDLL(None).fflush(None)
        sys.stdout.flush()
        # ONE write of the whole line through Python's own stdout (so that a redirected sys.stdout is honoured), flushed at once: the line
        # cannot interleave with another process's on a shared pipe
        sys.stdout.write(json.dumps(line) + "\n")
        sys.stdout.flush()


def rng_inclusive(render, cam, n_rays, dev):
    """One extra step per RNG mode with the uniforms drawn INSIDE the timed region: "device" (torch.rand on the GPU) and
    "torch_cpu" (the reference's CPU generator, drawn per 65 536-ray batch on the host and uploaded while the previous batch
    renders -- what the drop-in render_image does)."""
    res = {}
    for mode in ("device", "torch_cpu"):
        render.rng = mode
        render.render_image_single_pass(WIDTH, HEIGHT, cam, SAMPLES)        # warm the pinned path
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        render.render_image_single_pass(WIDTH, HEIGHT, cam, SAMPLES)
        torch.cuda.synchronize()
        res[mode] = n_rays / (time.perf_counter() - t0)
    render.rng = "device"
    res["unit"] = "rays/s"
    res["note"] = "uniforms (128 per ray, 328 MB per view) generated inside the timed region; torch_cpu = host MT19937 + PCIe upload"
    return res


if __name__ == "__main__":
    main()
