"""`python tools/time_raycast.py [--out profiles/raycast_cost.json] [--repeats 5]` -- what looking at a mesh costs on the device.

  grid / brute   800 x 800 rays of one pinhole view against the level set 0 of tools/time_mesh_clean.py's seeded synthetic volume -- one
                 large sphere and 300 small ones -- meshed at 128^3 and 256^3: the brute kernel, and the grid at 1, 2, 4, 8 and 16
                 triangles per cell with the build (count + build) listed apart from the query.  The grid's query is timed twice: rays in
                 row-major pixel order, and the same rays ordered by 8 x 8 pixel tiles (one wave64 = one tile), since the rays of a wave
                 diverge in the DDA.  Grid and brute must agree bit for bit (a checksum across processes).
  views          the shipped bunny meshed at resolution 256 seen through render_image_mesh, against the sphere-traced frame and the
                 128-sample single pass of the same camera (the fixture's view at 800 x 800).
  compare        what scripts/render_mesh.py --compare-trace prints, for the shipped bunny at resolution 48 / threshold 0.0275 and at
                 resolution 24 / threshold 0.1 (the settings the tests use), same camera at 400 x 400.

Every time is the median of --repeats runs between device synchronises after one untimed warm-up; every method runs in a process of its own."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PER_CELL = (1, 2, 4, 8, 16)
RESOLUTIONS = (128, 256)
SIZE = 800
METHODS = ("grid", "brute", "views", "compare")


def timed(fn, repeats, dev):
    """(median milliseconds, the last result) after one untimed warm-up: synchronise, run, synchronise."""
    fn()
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), out


def mesh(res, dev):
    from neddf_amd.mesh import marching_cubes
    from time_mesh_clean import volume
    return marching_cubes(torch.from_numpy(volume(res)).to(dev), 0.0, (-1.0,) * 3, (1.0,) * 3)


def view_rays(dev, n=SIZE, tiles=False):
    """n x n pinhole rays from (2.2, -2.6, 1.6) at the origin, the cube [-1, 1]^3 filling the frame; row-major, or in 8 x 8 pixel tiles."""
    eye = np.array([2.2, -2.6, 1.6])
    f = -eye / np.linalg.norm(eye)
    right = np.cross(f, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, f)
    s = (np.arange(n) + 0.5) / n - 0.5
    d = f[None, None] + 0.9 * (s[None, :, None] * right[None, None] - s[:, None, None] * up[None, None])
    if tiles:
        d = d.reshape(n // 8, 8, n // 8, 8, 3).transpose(0, 2, 1, 3, 4)
    d = d.reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.broadcast_to(eye, d.shape)
    return torch.from_numpy(o.astype(np.float32).copy()).to(dev), torch.from_numpy(d.astype(np.float32)).to(dev)


def checksum(hits):
    return {"hits": int((hits["triangle"] >= 0).sum().item()), "triangle_sum": int(hits["triangle"].long().sum().item()),
            "t_sum": float(torch.where(hits["triangle"] >= 0, hits["t"], torch.zeros_like(hits["t"])).double().sum().item())}


def run_grid(repeats, dev):
    from neddf_amd.geometry import default_cells
    from neddf_amd.raycast import build_grid, cast_rays
    rows = []
    o, d = view_rays(dev)
    ot, dt = view_rays(dev, tiles=True)
    for res in RESOLUTIONS:
        v, t = mesh(res, dev)
        lo, hi = v.min(dim=0).values.tolist(), v.max(dim=0).values.tolist()
        for per_cell in PER_CELL:
            cells = default_cells(t.shape[0], lo, hi, per_cell)
            build_ms, grid = timed(lambda: build_grid(v, t, cells=cells), repeats, dev)
            query_ms, hits = timed(lambda: cast_rays(o, d, v, t, grid=grid), repeats, dev)
            tiles_ms, tiled = timed(lambda: cast_rays(ot, dt, v, t, grid=grid), repeats, dev)
            rows.append(dict(resolution=res, triangles=int(t.shape[0]), rays=int(o.shape[0]), triangles_per_cell=per_cell, cells=list(cells),
                             pairs=int(grid.items.shape[0]), build_ms=build_ms, query_ms=query_ms, query_8x8_tiles_ms=tiles_ms,
                             total_ms=build_ms + query_ms, pad=grid.pad, **checksum(hits)))
            assert checksum(tiled)["hits"] == rows[-1]["hits"]
            print(rows[-1], flush=True)
    return rows


def run_brute(repeats, dev):
    from neddf_amd.raycast import cast_rays, default_pad
    rows = []
    o, d = view_rays(dev)
    for res in RESOLUTIONS:
        v, t = mesh(res, dev)
        pad = default_pad(v.min(dim=0).values.double().tolist(), v.max(dim=0).values.double().tolist())
        ms, hits = timed(lambda: cast_rays(o, d, v, t, method="brute", pad=pad), repeats, dev)
        rows.append(dict(resolution=res, triangles=int(t.shape[0]), rays=int(o.shape[0]), brute_ms=ms, pad=pad, **checksum(hits)))
        print(rows[-1], flush=True)
    return rows


def bunny_view(dev, n):
    import neddf_amd
    from neddf_amd.fixtures import BUNNY_SMOKE_CFG, bunny_smoke_weights
    g = np.load(os.path.join(ROOT, "tests", "golden", "bunny_stages.npz"))
    render = neddf_amd.NeRFRender(dict(BUNNY_SMOKE_CFG, _target_="neddf.network.NeDDF"), sample_coarse=64, sample_fine=128, dist_near=2.0,
                                  dist_far=6.0, max_dist=6.0, use_coarse_network=False, sampling_type="cone")
    render.network_fine.load_state_dict({k: torch.from_numpy(v) for k, v in bunny_smoke_weights().items()})
    render.to(dev)
    render.set_iter(-1)
    render.rng = "device"
    for p in render.parameters():
        p.requires_grad_(False)
    cam = neddf_amd.Camera(neddf_amd.PinholeCalib(g["calib"].astype(np.float64) * (n / 400.0)), None).to(dev)      # the fixture's 400 x 400 view at n x n
    cam.R, cam.T = torch.from_numpy(g["R"]).to(dev), torch.from_numpy(g["T"]).to(dev)
    return render, cam


def run_views(repeats, dev):
    from neddf_amd.raycast import build_grid
    render, cam = bunny_view(dev, SIZE)
    net = render.get_network()
    extract_ms, (v, t, nrm) = timed(lambda: net.extract_mesh(resolution=256, normals=True), repeats, dev)
    targets = ["depth", "transmittance", "normal"]
    build_ms, grid = timed(lambda: build_grid(v, t), repeats, dev)
    mesh_ms, img = timed(lambda: render.render_image_mesh(SIZE, SIZE, cam, v, t, targets, normals=nrm, grid=grid), repeats, dev)
    cold_ms, _ = timed(lambda: render.render_image_mesh(SIZE, SIZE, cam, v, t, targets, normals=nrm), repeats, dev)
    traced_ms, traced = timed(lambda: render.render_image_traced(SIZE, SIZE, cam, ["color", "depth", "normal", "transmittance"], 0.0275), repeats, dev)
    single_ms, _ = timed(lambda: render.render_image_single_pass(SIZE, SIZE, cam, 128)["color"], repeats, dev)
    return dict(size=[SIZE, SIZE], resolution=256, threshold=0.0275, triangles=int(t.shape[0]), cells=list(grid.cells), extract_mesh_ms=extract_ms,
                grid_build_ms=build_ms, mesh_view_ms=mesh_ms, mesh_view_with_grid_build_ms=cold_ms, traced_view_ms=traced_ms,
                single_pass_128_ms=single_ms, mesh_hit_share=1.0 - float(img["transmittance"].mean()),
                traced_hit_share=1.0 - float(traced["transmittance"].mean()))


def run_compare(repeats, dev):
    from neddf_amd.scripts.render_mesh import compare_hits
    n = 400
    render, cam = bunny_view(dev, n)
    net = render.get_network()
    rows = []
    for res, threshold in ((48, 0.0275), (24, 0.1)):
        v, t = net.extract_mesh(threshold=threshold, resolution=res)
        img = render.render_image_mesh(n, n, cam, v, t, ["depth", "transmittance"])
        traced = render.render_image_traced(n, n, cam, ["depth", "transmittance"], threshold)
        rows.append(dict(resolution=res, threshold=threshold, triangles=int(t.shape[0]), size=[n, n], lattice_step=2.2 / (res - 1),
                         **compare_hits(img["depth"], img["transmittance"] == 0, traced["depth"], traced["transmittance"] == 0)))
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raycast_cost.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--methods", nargs="+", default=list(METHODS), choices=METHODS)
    ap.add_argument("--method", default=None, choices=METHODS, help="(internal) run this one method and print its JSON")
    args = ap.parse_args(argv)
    if args.method:
        dev = torch.device("cuda:0")
        rows = {"grid": run_grid, "brute": run_brute, "views": run_views, "compare": run_compare}[args.method](args.repeats, dev)
        print("CASE " + json.dumps(rows), flush=True)
        return None
    result = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats,
              "inputs": "level set 0 of the synthetic sphere volume of tools/time_mesh_clean.py at 128^3 and 256^3; %d x %d pinhole rays" % (SIZE, SIZE)}
    for method in args.methods:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--method", method, "--repeats", str(args.repeats)],
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        if out.returncode != 0:
            raise SystemExit("%s failed (exit %d):\n%s" % (method, out.returncode, out.stdout[-4000:]))
        result[method] = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("CASE ")][-1][5:])
        print(method, json.dumps(result[method]), flush=True)
    if "grid" in result:
        at = [r for r in result["grid"] if r["resolution"] == max(RESOLUTIONS)]
        result["fastest_triangles_per_cell_at_the_largest_mesh"] = min(at, key=lambda r: r["query_ms"])["triangles_per_cell"]
        if "brute" in result:
            for b in result["brute"]:
                g = [r for r in result["grid"] if r["resolution"] == b["resolution"]]
                b["agrees_with_grid"] = all(r["hits"] == b["hits"] and r["triangle_sum"] == b["triangle_sum"] and r["t_sum"] == b["t_sum"] for r in g)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    return result


if __name__ == "__main__":
    main()
