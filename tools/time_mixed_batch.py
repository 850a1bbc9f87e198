#!/usr/bin/env python3
"""Time the training step on batches that mix views, and an image rendered from a ray bundle: NeRFTrainer on a synthetic dataset (random
64 x 64 RGBA views on a ring around the origin), the shipped bunny_smoke network (65 coarse + 194 fine cone samples, fp32 operands),
1024 rays, ColorLoss + MaskBCELoss + FieldsConstraintLoss.  A step is the whole run_train_step / run_train_step_mixed -- host draws, ground
truth, forward, backward, Adam -- timed with the host clock between two device synchronises; per configuration `--warmup` steps, then
the median of `--reps`.  Records, to profiles/view_table_cost.json (profiles/mixed_batch_cost.json is the record of the tree before the
camera table and stays as it is):

    single_ms                   batch_views="single" on this tree, and with --parent PATH on that checkout of the parent commit (a child
                                process that imports the package from PATH and runs this file's step timings)
    mixed_ms[views][poses]      batch_views="mixed" over 1, 10 and 100 views, optimize_cameras off and on; under "parent" the same six
                                from the parent checkout, in the same session
    views_do_not_matter         the soft criterion: the 100-view fields-only median lies inside the min..max of the 1-view one
    table_kernels_ms            the camera-table ray generation and its backward alone (device events around 20 launches) at
                                (rays, cameras) = (1024, 100) and (65536, 1000)
    image_ms                    with --images: render_image, 800 x 800, colour, rng="device": a pinhole camera through the uv path, and the
                                same camera as a calib class that makes the same rays in torch (the bundle path)

    python tools/time_mixed_batch.py [--parent PATH] [--rays 1024] [--reps 5] [--warmup 3] [--images]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 64


def make_dataset(root, n):
    from PIL import Image
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(0)
    os.makedirs(os.path.join(root, "train"), exist_ok=True)
    frames = []
    for i in range(n):
        Image.fromarray(rng.integers(0, 256, (SIZE, SIZE, 4), dtype=np.uint8), "RGBA").save(os.path.join(root, "train", "r_%d.png" % i))
        m = np.eye(4)
        m[:3, :3] = Rotation.from_euler("zx", [2 * np.pi * i / n, 1.1]).as_matrix()
        m[:3, 3] = m[:3, :3] @ np.array([0.0, 0.0, 4.0])           # on a ring, looking at the origin along the camera's -z
        frames.append({"file_path": "./train/r_%d" % i, "transform_matrix": m.tolist()})
    json.dump({"camera_angle_x": 0.6911112070083618, "frames": frames}, open(os.path.join(root, "transforms_train.json"), "w"))


def make_trainer(n_views, rays, **kw):
    import torch
    from neddf_amd.config import instantiate
    from neddf_amd.fixtures import BUNNY_SMOKE_CFG, bunny_smoke_weights
    root = tempfile.mkdtemp()
    make_dataset(root, n_views)
    cfg = {"dataset": {"_target_": "neddf.dataset.NeRFSyntheticDataset", "dataset_dir": root, "data_split": "train", "use_depth": False,
                       "use_mask": True},
           "render": {"_target_": "neddf.render.NeRFRender", "sample_coarse": 64, "sample_fine": 128, "dist_near": 2.0, "dist_far": 6.0,
                      "max_dist": 6.0, "use_coarse_network": False, "sampling_type": "cone"},
           "network": dict(BUNNY_SMOKE_CFG, density_activation_type="ReLU", _target_="neddf.network.NeDDF"),
           "trainer": dict({"_target_": "neddf.trainer.NeRFTrainer", "device": "cuda:0", "batch_size": rays, "chunk": 1024}, **kw),
           "loss": {"functions": [{"_target_": "neddf.loss.ColorLoss", "weight": 1.0, "weight_coarse": 0.1},
                                  {"_target_": "neddf.loss.MaskBCELoss", "weight": 0.05, "weight_coarse": 0.005},
                                  {"_target_": "neddf.loss.FieldsConstraintLoss", "weight": 0.01, "weight_coarse": 0.01}]}}
    torch.manual_seed(11)
    tr = instantiate(cfg["trainer"], global_config=cfg, _recursive_=False)
    tr.writes_outputs = False
    tr.neural_render.network_fine.load_state_dict({k: torch.from_numpy(v) for k, v in bunny_smoke_weights().items()})
    tr.neural_render.set_iter(1500)
    return tr


def median_ms(fn, warmup, reps):
    import torch
    times = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(1e3 * (time.perf_counter() - t0))
    return {"median": statistics.median(times), "min": min(times), "max": max(times)}


def time_single(args):
    tr = make_trainer(10, args.rays)
    views = iter(range(10 ** 9))
    return median_ms(lambda: tr.run_train_step(next(views) % 10), args.warmup, args.reps)


def time_mixed(args):
    out = {}
    for n_views in (1, 10, 100):
        row = out["%d_views" % n_views] = {}
        for poses in (False, True):
            tr = make_trainer(n_views, args.rays, batch_views="mixed", optimize_cameras=poses)
            row["optimize_cameras" if poses else "fields_only"] = median_ms(tr.run_train_step_mixed, args.warmup, args.reps)
            del tr
    return out


def time_table_kernels():
    """The two camera-table launches alone: device events around 20 launches after a warm-up, ms per launch."""
    import torch
    from neddf_amd._lib import Context, ViewRays
    dev = torch.device("cuda:0")
    ctx = Context.get(dev)
    gen = torch.Generator().manual_seed(5)
    out = {}
    for rays, cams in ((1024, 100), (65536, 1000)):
        table = torch.rand(cams, 16, generator=gen).to(dev) + 0.5
        uv = (torch.rand(rays, 2, generator=gen) * 63).to(torch.int16).to(dev)
        view = (torch.rand(rays, generator=gen) * cams).to(torch.int32).to(dev)
        g_rd, g_ro = torch.randn(rays, 3, generator=gen).to(dev), torch.randn(rays, 3, generator=gen).to(dev)
        arg = ViewRays(uv, view, table)
        row = out["%d_rays_%d_cameras" % (rays, cams)] = {}
        for name, fn in (("raygen", lambda: ctx.raygen(arg)), ("raygen_backward", lambda: ctx.raygen_backward(arg, None, g_rd, g_ro))):
            for _ in range(3):
                fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(20):
                fn()
            b.record()
            b.synchronize()
            row[name] = a.elapsed_time(b) / 20
    return out


def time_images(args):
    import torch
    from torch import nn

    import neddf_amd
    from neddf_amd.camera import BaseCameraCalib
    from neddf_amd.fixtures import BUNNY_SMOKE_CFG, bunny_smoke_weights

    class PinholeInTorch(BaseCameraCalib):
        """PinholeCalib's rays made in torch: not a PinholeCalib, so render_image takes them as a bundle."""

        def unproject_local(self, uv):
            x = (1.0 / self.params[0]) * (uv[:, 0] - self.params[2])
            y = (1.0 / self.params[1]) * (uv[:, 1] - self.params[3])
            return nn.functional.normalize(torch.stack([x, -y, -torch.ones_like(x)], 1), p=2, dim=1)

    dev = torch.device("cuda:0")
    render = neddf_amd.NeRFRender(dict(BUNNY_SMOKE_CFG, _target_="neddf.network.NeDDF"), sample_coarse=64, sample_fine=128, dist_near=2.0,
                                  dist_far=6.0, max_dist=6.0, use_coarse_network=False, sampling_type="cone")
    render.network_fine.load_state_dict({k: torch.from_numpy(v) for k, v in bunny_smoke_weights().items()})
    render.to(dev)
    render.rng = "device"
    render.set_iter(-1)
    focal = 0.5 * 800 / np.tan(0.5 * 0.6911112070083618)
    calib, pose = np.array([focal, focal, 400.0, 400.0]), np.array([2.1, 0.3, -0.2, 0.0, 2.74, 2.96], np.float32)
    out = {}
    for key, cls in (("uv", neddf_amd.PinholeCalib), ("bundle", PinholeInTorch)):
        cam = neddf_amd.Camera(cls(calib), pose).to(dev)
        cam.update_transform()
        out[key] = median_ms(lambda: render.render_image(800, 800, cam, ["color"]), args.warmup, args.reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, built: its steps are timed in a child process")
    ap.add_argument("--tree", default=HERE, help="the checkout whose package is imported (default: this one)")
    ap.add_argument("--steps-only", action="store_true", help="time the single-view and the mixed steps, print them as JSON and stop (the --parent child)")
    ap.add_argument("--images", action="store_true", help="also time render_image through the uv path and as a bundle")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "view_table_cost.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch

    import neddf_amd
    assert os.path.abspath(os.path.dirname(os.path.dirname(neddf_amd.__file__))) == os.path.abspath(args.tree), neddf_amd.__file__
    if args.steps_only:
        print("STEPS " + json.dumps({"single_ms": time_single(args), "mixed_ms": time_mixed(args)}))
        return
    rec = {"workload": "training step (host draws, ground truth, forward, backward, Adam), %d rays x 259 samples, NeDDF fp32, shipped "
                       "bunny_smoke weights, %d x %d views; host clock between device synchronises" % (args.rays, SIZE, SIZE),
           "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    rec["single_ms"] = {"this_tree": time_single(args)}
    rec["mixed_ms"] = time_mixed(args)
    if args.parent:
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps-only", "--tree", os.path.abspath(args.parent), "--rays",
                                str(args.rays), "--reps", str(args.reps), "--warmup", str(args.warmup)], cwd=os.path.abspath(args.parent),
                               capture_output=True, text=True, timeout=900)
        lines = [l for l in child.stdout.splitlines() if l.startswith("STEPS ")]
        if child.returncode or not lines:
            raise SystemExit("the parent's timing failed:\n" + child.stdout[-2000:] + child.stderr[-2000:])
        parent = json.loads(lines[-1][len("STEPS "):])
        rec["single_ms"]["parent"] = parent["single_ms"]
        rec["mixed_ms"]["parent"] = parent["mixed_ms"]
    one, hundred = rec["mixed_ms"]["1_views"]["fields_only"], rec["mixed_ms"]["100_views"]["fields_only"]
    rec["views_do_not_matter"] = {"criterion": "fields only: the 100-view median inside the min..max of the 1-view step, same process",
                                  "holds": one["min"] <= hundred["median"] <= one["max"]}
    rec["table_kernels_ms"] = dict(time_table_kernels(), what="ray generation with a camera per row and its pose backward alone, ms per launch")
    if args.images:
        rec["image_ms"] = dict(time_images(args), what="render_image 800 x 800, colour, rng='device': the uv path against the same rays made "
                                                       "in torch and rendered as a bundle")
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
