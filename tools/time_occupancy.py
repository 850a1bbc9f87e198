#!/usr/bin/env python3
"""What empty-space skipping costs and saves on the shipped bunny network (writes profiles/occupancy_cost.json):

    python tools/time_occupancy.py [--out profiles/occupancy_cost.json] [--reps 5] [--resolutions 64 128 256]

  single_pass   800 x 800 rays, 128 stratified cone samples per ray (render_image_single_pass)
  hierarchical  800 x 800 rays, 65 + 194 samples (render_image, targets color + depth)
Both with fp32 operands, first with occupancy = None, then with the grid of build_occupancy(resolution=R, threshold=0, dilate=1)
for every R: the grid's build time and occupied fraction, kept / total samples, the frame time, and the PSNR of the culled frame's
colour against the unculled one drawn with the same uniforms.  Each time is the median of --reps runs between device
synchronises after one warm-up; uniforms are drawn on the device (rng = "device") so that the host generator is not what is
measured.

The plain path of another checkout (the parent commit, to show that it did not slow down) is measured by the same tool:
    python tools/time_occupancy.py --plain-only --package-root <checkout> --out parent.json
and merged into the record with --parent parent.json."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occupancy_cost.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--resolutions", type=int, nargs="*", default=[64, 128, 256])
    ap.add_argument("--plain-only", action="store_true", help="time the plain path only (works on a checkout without occupancy grids)")
    ap.add_argument("--package-root", default=ROOT, help="the checkout whose neddf_amd is measured")
    ap.add_argument("--parent", default=None, help="a --plain-only record of the parent commit to embed")
    args = ap.parse_args(argv)
    root = os.path.abspath(args.package_root)
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import neddf_amd
    from neddf_amd.fixtures import BUNNY_SMOKE_CFG, bunny_smoke_weights
    assert os.path.abspath(neddf_amd.__file__).startswith(root), neddf_amd.__file__
    dev = torch.device("cuda:0")
    g = np.load(os.path.join(root, "tests", "golden", "bunny_stages.npz"))
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

    modes = {"single_pass_%dx%d_128" % (n, n): lambda: render.render_image_single_pass(n, n, cam, 128)["color"].reshape(-1, 3),
             "hierarchical_%dx%d_65_194" % (n, n): lambda: render.render_image(n, n, cam, ["color", "depth"], 1, 1024)["color"].reshape(-1, 3)}

    def timed(fn):
        """(median ms, every run's ms, the colour of the last run); every run draws the same uniforms"""
        out = None
        ts = []
        for k in range(args.reps + 1):
            torch.manual_seed(1234)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if k:
                ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), ts, out

    res = {"device": torch.cuda.get_device_name(0), "unit": "ms per frame, median of %d runs between device synchronises" % args.reps,
           "operands": "fp32"}
    plain = {}
    for name, fn in modes.items():
        ms, runs, color = timed(fn)
        plain[name] = color
        res[name] = {"plain_ms": ms, "plain_runs_ms": runs, "plain_spread_pct": 100.0 * (max(runs) - min(runs)) / ms}
        print("%-30s plain %9.2f ms  (runs %s)" % (name, ms, " ".join("%.1f" % t for t in runs)), flush=True)
    if not args.plain_only:
        ctx = neddf_amd.Context.get(dev)
        for R in args.resolutions:
            builds = []
            for k in range(args.reps + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                grid = render.build_occupancy(resolution=R, threshold=0.0, dilate=1)
                torch.cuda.synchronize()
                if k:
                    builds.append((time.perf_counter() - t0) * 1e3)
            for name, fn in modes.items():
                ctx.cull_stats(reset=True)
                ms, runs, color = timed(fn)
                samples, kept = ctx.cull_stats(reset=True)
                mse = float(((color.double() - plain[name].double()) ** 2).mean().item())
                row = {"ms": ms, "runs_ms": runs, "speedup_vs_plain": res[name]["plain_ms"] / ms, "kept_samples": kept // (args.reps + 1),
                       "total_samples": samples // (args.reps + 1), "kept_fraction": kept / float(samples),
                       "psnr_db_vs_plain": None if mse == 0.0 else 10.0 * math.log10(1.0 / mse), "mse_vs_plain": mse,
                       "grid_build_ms": statistics.median(builds), "grid_occupied_fraction": grid.occupied_fraction}
                res[name]["R%d" % R] = row
                print("%-30s R=%-4d %9.2f ms  x%.2f  kept %.2f %%  grid %.2f %% occupied, built in %.1f ms  PSNR %s dB"
                      % (name, R, ms, row["speedup_vs_plain"], 100 * row["kept_fraction"], 100 * row["grid_occupied_fraction"],
                         row["grid_build_ms"], "inf" if mse == 0.0 else "%.2f" % row["psnr_db_vs_plain"]), flush=True)
            render.occupancy = None
    if args.parent:
        with open(args.parent) as fh:
            parent = json.load(fh)
        for name in modes:
            if name in parent:
                res[name]["parent_commit_plain_ms"] = parent[name]["plain_ms"]
                res[name]["parent_commit_plain_runs_ms"] = parent[name]["plain_runs_ms"]
                res[name]["plain_vs_parent_pct"] = 100.0 * (res[name]["plain_ms"] / parent[name]["plain_ms"] - 1.0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
