"""`python tools/time_point_mesh.py [--out profiles/point_mesh_cost.json] [--repeats 5]` -- what the exact distance from points to a mesh
costs on the device, and what it measures that the sample-to-sample distance cannot.

  brute / grid   queries: about 10^4, 10^5 and 10^6 surface samples of the level set 0.01 of tools/time_mesh_clean.py's seeded synthetic
                 volume -- one large sphere and 300 small ones; mesh: its level set 0, at 128^3 and 256^3 (tools/time_raycast.py's
                 meshes).  The brute kernel, and the grid query at 1, 2, 4, 8 and 16 triangles per cell with the build listed apart and
                 the triangle evaluations per query (a triangle listed in several visited cells counts every time: the cost of the
                 duplicates).  Grid and brute must agree bit for bit (a checksum across processes).
  uniform        10^4 queries uniform in the mesh's box against the 256^3 mesh: far from the surface a query walks many shells.
  samples        mesh_distance between the two level sets with to="samples" and to="surface" at the same sample counts.
  bunny          mesh_distance, both modes, between the shipped bunny's fp32 and bf16 meshes and between its sparse meshes with
                 lipschitz 1 and 0.25 at resolution 256.
  level_set      level_set_check of the shipped bunny at threshold 0.0275 / resolution 48 and at 0.1 / 24.

Every time is the median of --repeats runs between device synchronises after one untimed warm-up; every method runs in a process of its
own.  Evaluations per query are computed from the result, not counted in the kernel: the walk stops after the first shell r with
(r * safe_cell)^2 > the final squared distance (the closest triangle is listed inside that shell: the header's equality argument), so the
count is the overflow list plus the list lengths of the cells within r of the query's cell -- a box sum over a 3D prefix sum."""
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

SIZES = (10 ** 4, 10 ** 5, 10 ** 6)
PER_CELL = (1, 2, 4, 8, 16)
RESOLUTIONS = (128, 256)
METHODS = ("grid", "brute", "uniform", "samples", "bunny", "level_set")


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


def surfaces(res, dev):
    from neddf_amd.mesh import marching_cubes
    from time_mesh_clean import volume
    vol = torch.from_numpy(volume(res)).to(dev)
    lo, hi = (-1.0,) * 3, (1.0,) * 3
    return marching_cubes(vol, 0.0, lo, hi), marching_cubes(vol, 0.01, lo, hi)


def queries(other, n):
    from neddf_amd.mesh import sample_surface
    return sample_surface(*other, n=n, seed=0)[0]


def checksum(out):
    d2, j = out[0], out[1]
    return {"triangle_sum": int(j.long().sum().item()), "d2_sum": float(d2.double().sum().item())}


def evaluations(grid, q, d2):
    """Mean triangle evaluations per query of the grid walk (see the module's docstring); every list for a grid that is not walked."""
    g = grid.cells
    G = g[0] * g[1] * g[2]
    start = grid.cell_start.long()
    n_items, overflow = int(start[G + 1].item()), int((start[G + 1] - start[G]).item())
    lo = torch.tensor(grid.lo, dtype=torch.float64)
    ext = torch.tensor(grid.hi, dtype=torch.float64) - lo
    inv = torch.where(ext > 0, torch.tensor(g, dtype=torch.float64) / ext.clamp_min(1e-300), torch.zeros(3, dtype=torch.float64)).float()
    inv_max = float(inv.max())
    w = max(abs(float(np.float32(l)) - 2.0 * grid.pad) for l in grid.lo + grid.hi)
    if inv_max > 0.0 and 1.0 / inv_max < 2.0 ** -10 * w:
        return float(n_items)
    safe = np.float32(0.99 / inv_max) if inv_max > 0.0 else np.float32(3.0e38)
    dev = q.device
    gt = torch.tensor(g, device=dev)
    f = (q - lo.float().to(dev)) * inv.to(dev)
    c = torch.where(f >= gt.float(), gt - 1, torch.where(f > 0, f.long(), torch.zeros_like(f, dtype=torch.long)))
    r0 = torch.floor(torch.sqrt(d2) / float(safe)).long()
    r = torch.full_like(r0, 1 << 20)
    for k in (2, 1, 0, -1):
        cand = (r0 + k).clamp_min(0)
        lb = cand.float() * float(safe)
        ok = (lb * lb > d2) & (lb * lb >= 1e-30)
        r = torch.where(ok, cand, r)
    count = (start[1:G + 1] - start[:G]).reshape(g[2], g[1], g[0])
    pre = torch.zeros(g[2] + 1, g[1] + 1, g[0] + 1, dtype=torch.long, device=dev)
    pre[1:, 1:, 1:] = count.cumsum(0).cumsum(1).cumsum(2)
    a0 = (c - r[:, None]).clamp_min(0)
    a1 = torch.minimum(c + r[:, None], gt - 1) + 1
    x0, y0, z0, x1, y1, z1 = a0[:, 0], a0[:, 1], a0[:, 2], a1[:, 0], a1[:, 1], a1[:, 2]
    box = (pre[z1, y1, x1] - pre[z0, y1, x1] - pre[z1, y0, x1] - pre[z1, y1, x0] + pre[z0, y0, x1] + pre[z0, y1, x0] + pre[z1, y0, x0] - pre[z0, y0, x0])
    ok = torch.isfinite(d2)
    return float((box[ok] + overflow).double().mean().item()) if bool(ok.any()) else 0.0


def run_grid(repeats, dev):
    from neddf_amd import Context
    from neddf_amd.geometry import default_cells
    from neddf_amd.raycast import build_grid
    ctx = Context.get(dev)
    rows = []
    for res in RESOLUTIONS:
        (v, t), other = surfaces(res, dev)
        lo, hi = v.min(dim=0).values.tolist(), v.max(dim=0).values.tolist()
        qs = [queries(other, n) for n in SIZES]
        for per_cell in PER_CELL:
            cells = default_cells(t.shape[0], lo, hi, per_cell)
            build_ms, grid = timed(lambda: build_grid(v, t, cells=cells), repeats, dev)
            for q in qs:
                ms, out = timed(lambda: ctx.point_mesh_grid_query(q, v, t, grid.lo, grid.hi, grid.cells, grid.pad, grid.cell_start, grid.items),
                                repeats, dev)
                rows.append(dict(resolution=res, triangles=int(t.shape[0]), queries=int(q.shape[0]), triangles_per_cell=per_cell, cells=list(cells),
                                 pairs=int(grid.items.shape[0]), build_ms=build_ms, query_ms=ms,
                                 evaluations_per_query=evaluations(grid, q, out[0]), **checksum(out)))
                print(rows[-1], flush=True)
    return rows


def run_brute(repeats, dev):
    from neddf_amd import Context
    ctx = Context.get(dev)
    rows = []
    for res in RESOLUTIONS:
        (v, t), other = surfaces(res, dev)
        for n in SIZES:
            q = queries(other, n)
            runs = repeats if n < 10 ** 6 else min(repeats, 3)
            ms, out = timed(lambda: ctx.point_mesh_brute(q, v, t), runs, dev)
            rows.append(dict(resolution=res, triangles=int(t.shape[0]), queries=int(q.shape[0]), brute_ms=ms, runs=runs, **checksum(out)))
            print(rows[-1], flush=True)
    return rows


def run_uniform(repeats, dev):
    from neddf_amd import Context
    from neddf_amd.raycast import build_grid
    ctx = Context.get(dev)
    (v, t), _ = surfaces(256, dev)
    grid = build_grid(v, t)
    lo, hi = torch.tensor(grid.lo, device=dev).float(), torch.tensor(grid.hi, device=dev).float()
    u = torch.from_numpy(np.random.default_rng(0).random((10 ** 4, 3)).astype(np.float32)).to(dev)
    q = (lo + u * (hi - lo)).contiguous()
    ms, out = timed(lambda: ctx.point_mesh_grid_query(q, v, t, grid.lo, grid.hi, grid.cells, grid.pad, grid.cell_start, grid.items), repeats, dev)
    bms, ref = timed(lambda: ctx.point_mesh_brute(q, v, t), repeats, dev)
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out, ref))
    return dict(resolution=256, triangles=int(t.shape[0]), queries=int(q.shape[0]), cells=list(grid.cells), query_ms=ms, brute_ms=bms,
                identical_to_brute=bool(same), evaluations_per_query=evaluations(grid, q, out[0]),
                mean_distance=float(torch.sqrt(out[0]).double().mean().item()), max_distance=float(torch.sqrt(out[0]).max().item()))


KEYS = ("a_to_b_mean", "b_to_a_mean", "chamfer", "hausdorff", "n_a", "n_b", "invalid_a", "invalid_b")


def both_modes(a, b, n, repeats, dev):
    from neddf_amd.geometry import mesh_distance
    row = {"requested": n, "triangles_a": int(a[1].shape[0]), "triangles_b": int(b[1].shape[0])}
    for to in ("samples", "surface"):
        ms, d = timed(lambda: mesh_distance(a, b, n=n, seed=0, to=to), repeats, dev)
        row[to] = dict({k: d[k] for k in KEYS}, ms=ms)
    return row


def run_samples(repeats, dev):
    rows = []
    for res in RESOLUTIONS:
        a, b = surfaces(res, dev)
        for n in SIZES:
            rows.append(dict(both_modes(a, b, n, repeats, dev), resolution=res))
            print(rows[-1], flush=True)
    return rows


def run_bunny(repeats, dev):
    from time_sparse_mesh import bunny
    net = bunny(dev)
    fp32 = net.extract_mesh(resolution=256)
    net.weight_dtype = "bf16"
    bf16 = net.extract_mesh(resolution=256)
    net.weight_dtype = "fp32"
    l1 = net.extract_mesh(resolution=256, brick=8, lipschitz=1.0)
    l025 = net.extract_mesh(resolution=256, brick=8, lipschitz=0.25)
    out = {"note": "resolution 256, threshold 0.0275, cube_range 1.1, brick 8; seed 0"}
    for name, a, b in (("fp32_vs_bf16", fp32, bf16), ("sparse_lipschitz_1_vs_0.25", l1, l025)):
        out[name] = [both_modes(a, b, n, repeats, dev) for n in (10 ** 5, 10 ** 6)]
    return out


def run_level_set(repeats, dev):
    from time_sparse_mesh import bunny
    net = bunny(dev)
    rows = []
    for res, threshold in ((48, 0.0275), (24, 0.1)):
        v, t = net.extract_mesh(threshold=threshold, resolution=res)
        ms, out = timed(lambda: net.level_set_check(v, t, threshold=threshold), repeats, dev)
        rows.append(dict(out, resolution=res, threshold=threshold, triangles=int(t.shape[0]), ms=ms))
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_mesh_cost.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--methods", nargs="+", default=list(METHODS), choices=METHODS)
    ap.add_argument("--method", default=None, choices=METHODS, help="(internal) run this one method and print its JSON")
    args = ap.parse_args(argv)
    if args.method:
        dev = torch.device("cuda:0")
        rows = {"grid": run_grid, "brute": run_brute, "uniform": run_uniform, "samples": run_samples, "bunny": run_bunny,
                "level_set": run_level_set}[args.method](args.repeats, dev)
        print("CASE " + json.dumps(rows), flush=True)
        return None
    result = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats,
              "inputs": "mesh: level set 0 of the synthetic sphere volume of tools/time_mesh_clean.py at 128^3 and 256^3; queries: surface samples of "
                        "its level set 0.01 in sampling order"}
    for method in args.methods:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--method", method, "--repeats", str(args.repeats)],
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        if out.returncode != 0:
            raise SystemExit("%s failed (exit %d):\n%s" % (method, out.returncode, out.stdout[-4000:]))
        result[method] = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("CASE ")][-1][5:])
        print(method, json.dumps(result[method]), flush=True)
    if "grid" in result:
        at = [r for r in result["grid"] if r["resolution"] == max(RESOLUTIONS)]
        at = [r for r in at if r["queries"] == max(x["queries"] for x in at)]
        result["fastest_triangles_per_cell_at_the_largest_case"] = min(at, key=lambda r: r["query_ms"])["triangles_per_cell"]
        if "brute" in result:
            for b in result["brute"]:
                g = [r for r in result["grid"] if r["resolution"] == b["resolution"] and r["queries"] == b["queries"]]
                b["agrees_with_grid"] = all(r["triangle_sum"] == b["triangle_sum"] and r["d2_sum"] == b["d2_sum"] for r in g)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    return result


if __name__ == "__main__":
    main()
