#!/usr/bin/env python3
"""Time one training step (render_rays under autograd -> ColorLoss -> backward) with pose gradients off and on: shipped bunny_smoke
weights, 1024 rays, 65 coarse + 194 fine cone samples, fp32 operands.  Per configuration: warm-up steps, then `--reps` steps each
timed with a pair of device events around the whole step (one synchronisation per step, after the second event); configurations
interleaved so that clock drift hits both.  Writes median / min / max per configuration and their ratio to profiles/pose_grad_step.json.

    python tools/time_pose_step.py [--rays 1024] [--reps 20] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_grad_step.json"))
    args = ap.parse_args()
    import neddf_amd
    from neddf_amd.fixtures import BUNNY_SMOKE_CFG, bunny_smoke_weights
    from neddf_amd.loss import ColorLoss
    dev = torch.device("cuda:0")
    cfg = dict(BUNNY_SMOKE_CFG, density_activation_type="ReLU", _target_="neddf.network.NeDDF")
    render = neddf_amd.NeRFRender(cfg, sample_coarse=64, sample_fine=128, dist_near=2.0, dist_far=6.0, max_dist=6.0,
                                  use_coarse_network=False, sampling_type="cone")
    render.network_fine.load_state_dict({k: torch.from_numpy(v) for k, v in bunny_smoke_weights().items()})
    render.to(dev)
    render.rng = "device"
    render.set_iter(1500)
    focal = 0.5 * 400 / np.tan(0.5 * 0.6911112070083618)
    cam = neddf_amd.Camera(neddf_amd.PinholeCalib(np.array([focal, focal, 200.0, 200.0])),
                           np.array([2.1, 0.3, -0.2, 0.0, 2.74, 2.96], np.float32)).to(dev)
    loss_fn = ColorLoss(weight=1.0, weight_coarse=0.1)
    rng = np.random.default_rng(3)
    uv = torch.from_numpy(rng.integers(120, 280, (args.rays, 2)).astype(np.int16)).to(dev)
    target = {"color": torch.from_numpy(rng.uniform(0, 1, (args.rays, 3)).astype(np.float32)).to(dev)}

    def step(on):
        render.pose_gradients = on
        cam.update_transform()
        render.zero_grad()
        cam.params.grad = None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = torch.stack(list(loss_fn(render.render_rays(uv, cam), target).values())).sum()
        loss.backward()
        e1.record()
        e1.synchronize()
        assert (cam.params.grad is not None) == on
        return e0.elapsed_time(e1)

    times = {False: [], True: []}
    for i in range(args.warmup + args.reps):
        for on in (False, True):
            t = step(on)
            if i >= args.warmup:
                times[on].append(t)
    rec = {"workload": "training step forward + backward, %d rays x 259 samples, NeDDF fp32, shipped bunny_smoke weights" % args.rays,
           "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    for on, key in ((False, "pose_gradients_off_ms"), (True, "pose_gradients_on_ms")):
        rec[key] = {"median": statistics.median(times[on]), "min": min(times[on]), "max": max(times[on])}
    rec["on_over_off"] = rec["pose_gradients_on_ms"]["median"] / rec["pose_gradients_off_ms"]["median"]
    rec["added_ms"] = rec["pose_gradients_on_ms"]["median"] - rec["pose_gradients_off_ms"]["median"]
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
