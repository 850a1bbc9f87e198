#!/usr/bin/env python3
"""What the surface-normal outputs cost on the shipped bunny network (writes profiles/surface_normals_cost.json):

    python tools/time_normal_target.py [--out profiles/surface_normals_cost.json] [--reps 3]

  single_pass   800 x 800 rays, 128 stratified cone samples per ray (render_image_single_pass), without / with normals=True
  hierarchical  800 x 800 rays, 65 + 194 samples (render_image, targets color + depth), without / with the "normal" target
  mesh          extract_mesh at 128^3, plain / with field normals and colours / with geometric normals
Each figure is the median of --reps timed runs after one warm-up, uniforms drawn on the device (rng = "device") so that the host
generator is not what is measured; every run ends in a device synchronise."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3, [t * 1e3 for t in ts]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_normals_cost.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--mesh-resolution", type=int, default=128)
    args = ap.parse_args(argv)
    import neddf_amd
    from neddf_amd.fixtures import BUNNY_SMOKE_CFG, bunny_smoke_weights
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
    calib = g["calib"].astype(np.float64) * (args.size / 400.0)             # the fixture's 400 x 400 view at the asked size
    cam = neddf_amd.Camera(neddf_amd.PinholeCalib(calib), None).to(dev)
    cam.R, cam.T = torch.from_numpy(g["R"]).to(dev), torch.from_numpy(g["T"]).to(dev)
    n, res = args.size, {}

    def case(name, off, on, extra=None):
        a, ra = timed(off, args.reps)
        b, rb = timed(on, args.reps)
        res[name] = {"off_ms": a, "on_ms": b, "ratio": b / a, "off_runs_ms": ra, "on_runs_ms": rb}
        if extra:
            res[name].update(extra)
        print("%-28s off %9.2f ms   on %9.2f ms   (+%.2f %%)" % (name, a, b, 100 * (b / a - 1)), flush=True)

    case("single_pass_%dx%d_128" % (n, n), lambda: render.render_image_single_pass(n, n, cam, 128),
         lambda: render.render_image_single_pass(n, n, cam, 128, normals=True))
    case("hierarchical_%dx%d_65_194" % (n, n), lambda: render.render_image(n, n, cam, ["color", "depth"], 1, 1024),
         lambda: render.render_image(n, n, cam, ["color", "depth", "normal"], 1, 1024))
    net, r = render.network_fine, args.mesh_resolution
    v, t = net.extract_mesh(resolution=r)
    case("mesh_%d_field_normals_colors" % r, lambda: net.extract_mesh(resolution=r), lambda: net.extract_mesh(resolution=r, normals="field", colors=True),
         {"vertices": int(v.shape[0]), "triangles": int(t.shape[0])})
    case("mesh_%d_geometric_normals" % r, lambda: net.extract_mesh(resolution=r), lambda: net.extract_mesh(resolution=r, normals="geometric"))
    res["device"] = torch.cuda.get_device_name(0)
    res["unit"] = "ms per call, median of %d" % args.reps
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
