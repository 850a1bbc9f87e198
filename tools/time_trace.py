#!/usr/bin/env python3
"""What the sphere-traced surface view costs on the shipped bunny network (writes profiles/trace_cost.json):

    python tools/time_trace.py [--out profiles/trace_cost.json] [--reps 5] [--size 800] [--threshold 0.0275] [--max-steps 32 64 128]

fp32 operands, the fixture's view at 800 x 800, step_scale 1, refine 4, min_step = (far - near) 2^-10.  Per max_steps:
  frame_ms            render_image_traced (color, depth, normal) between device synchronises, median of --reps after one warm-up
  evaluations_per_ray distance evaluations of neddf_trace_field over the rays; hit / miss / exhausted shares; mean advances per ray
  iterations          the same march driven from the stage entry points (trace.sphere_trace's loop), one row per iteration:
                      active rays and the milliseconds of compact + field + advance between device synchronises (one run)
  psnr_db_vs_volume   the traced colour against the hierarchical volume render of the same view (background 0 in both)
and, from the same process, the volume renders of that view: render_image_single_pass with 128 samples and the hierarchical
65 + 194 render_image (uniforms drawn on the device, so that the host generator is not what is measured)."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_cost.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--threshold", type=float, default=0.0275)
    ap.add_argument("--max-steps", type=int, nargs="*", default=[32, 64, 128])
    args = ap.parse_args(argv)
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import neddf_amd
    from neddf_amd._lib import OUT_MINIMAL, SLOT_FINE
    from neddf_amd.fixtures import BUNNY_SMOKE_CFG, bunny_smoke_weights
    from neddf_amd.trace import EXHAUSTED, HIT, MISS, trace_params
    assert torch.cuda.is_available(), "time_trace.py measures on a HIP device; there is nothing to measure without one"
    dev = torch.device("cuda:0")
    g = np.load(os.path.join(ROOT, "tests", "golden", "bunny_stages.npz"))
    render = neddf_amd.NeRFRender(dict(BUNNY_SMOKE_CFG, _target_="neddf.network.NeDDF"), sample_coarse=64, sample_fine=128, dist_near=2.0,
                                  dist_far=6.0, max_dist=6.0, use_coarse_network=False, sampling_type="cone")
    render.network_fine.load_state_dict({k: torch.from_numpy(v) for k, v in bunny_smoke_weights().items()})
    render.to(dev)
    render.set_iter(-1)
    render.rng = "device"
    for p in render.parameters():
        p.requires_grad_(False)
    n = args.size
    calib = g["calib"].astype(np.float64) * (n / 400.0)                 # the fixture's 400 x 400 view at the asked size
    cam = neddf_amd.Camera(neddf_amd.PinholeCalib(calib), None).to(dev)
    cam.R, cam.T = torch.from_numpy(g["R"]).to(dev), torch.from_numpy(g["T"]).to(dev)
    ctx = render._ctx(dev)

    def timed(fn):
        out, ts = None, []
        for k in range(args.reps + 1):
            torch.manual_seed(1234)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if k:
                ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), ts, out

    res = {"device": torch.cuda.get_device_name(0), "operands": "fp32", "size": [n, n], "threshold": args.threshold, "step_scale": 1.0, "refine": 4,
           "unit": "ms between device synchronises; frame times are the median of %d runs after one warm-up" % args.reps}
    ms, runs, single = timed(lambda: render.render_image_single_pass(n, n, cam, 128)["color"].reshape(-1, 3))
    res["volume_single_pass_128"] = {"frame_ms": ms, "runs_ms": runs}
    print("volume, single pass 128      %9.2f ms  (runs %s)" % (ms, " ".join("%.1f" % t for t in runs)), flush=True)
    ms, runs, volume = timed(lambda: render.render_image(n, n, cam, ["color", "depth"], 1, 1024)["color"].reshape(-1, 3))
    res["volume_hierarchical_65_194"] = {"frame_ms": ms, "runs_ms": runs}
    print("volume, hierarchical 65+194  %9.2f ms  (runs %s)" % (ms, " ".join("%.1f" % t for t in runs)), flush=True)

    idx = torch.arange(n * n, device=dev)
    rd, ro = ctx.raygen(torch.stack([idx % n, idx // n], 1), cam.descriptor())
    unit = torch.tensor([1.0, 0.0, 0.0], device=dev)
    for max_steps in args.max_steps:
        p = trace_params(args.threshold, render.dist_near, render.dist_far, max_steps=max_steps)
        ms, runs, color = timed(lambda: render.render_image_traced(n, n, cam, ["color", "depth", "normal"], args.threshold,
                                                                   max_steps=max_steps)["color"].reshape(-1, 3))
        st, ev = ctx.trace_field(SLOT_FINE, ro, rd, p)
        status = st["status"]
        # the same march from the stage entry points, timed per iteration
        rows = []
        st2 = ctx.trace_begin(ro, rd, p.t_near)
        for it in range(max_steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            index, pos = ctx.trace_compact(ro, rd, st2)
            if index.shape[0] == 0:
                break
            D = ctx.field_forward(SLOT_FINE, pos, unit.expand_as(pos).contiguous(), torch.zeros_like(pos), OUT_MINIMAL, ["distance"])["distance"]
            ctx.trace_advance(index, D, st2, p.threshold, p.step_scale, p.min_step, p.t_far)
            torch.cuda.synchronize()
            rows.append({"iteration": it, "active_rays": int(index.shape[0]), "ms": (time.perf_counter() - t0) * 1e3})
        mse = float(((color.double() - volume.double()) ** 2).mean().item())
        row = {"frame_ms": ms, "runs_ms": runs, "speedup_vs_single_pass_128": res["volume_single_pass_128"]["frame_ms"] / ms,
               "speedup_vs_hierarchical": res["volume_hierarchical_65_194"]["frame_ms"] / ms, "evaluations_per_ray": ev / float(n * n),
               "hit_share": float((status == HIT).float().mean()), "miss_share": float((status == MISS).float().mean()),
               "exhausted_share": float((status == EXHAUSTED).float().mean()), "mean_advances_per_ray": float(st["steps"].float().mean()),
               "psnr_db_vs_volume": None if mse == 0.0 else 10.0 * math.log10(1.0 / mse), "iterations": rows}
        res["max_steps_%d" % max_steps] = row
        print("traced, max_steps %-4d       %9.2f ms  x%.1f vs single pass, x%.1f vs hierarchical  %.2f evaluations/ray  hit %.4f  exhausted %.4f  "
              "PSNR vs volume %.2f dB" % (max_steps, ms, row["speedup_vs_single_pass_128"], row["speedup_vs_hierarchical"], row["evaluations_per_ray"],
                                         row["hit_share"], row["exhausted_share"], row["psnr_db_vs_volume"] or float("inf")), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
