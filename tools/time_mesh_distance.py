"""`python tools/time_mesh_distance.py [--out profiles/mesh_distance_cost.json] [--repeats 5]` -- what a distance between two surfaces
costs on the device: surface sampling, the uniform grid (build and query at 1, 2, 4, 8 and 16 targets per cell), the brute-force kernel
and, on the host, scipy's k-d tree (download, build, query with every core the process may use).

Inputs: two level sets (0 and 0.01) of tools/time_mesh_clean.py's seeded synthetic volume at 256^3 -- one large sphere and 300 small ones
-- each sampled at about 10^4, 10^5 and 10^6 points; queries are the first surface's samples in the order sampling produces them
(triangle-major, i.e. lattice order), targets the second's.  Every time is the median of --repeats runs between device synchronises
after one untimed warm-up; every method runs in a process of its own.  The brute kernel and the k-d tree must reproduce the grid's
result (bit for bit, and within fp32 rounding).  Also recorded, as numbers without a pass mark: mesh_distance between the shipped
bunny's fp32 and bf16 meshes at resolution 256, and between its sparse meshes with lipschitz=1 and lipschitz=0.25."""
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
BRUTE_MAX = 10 ** 6             # the largest size the brute kernel is timed at (about a second per run on an MI355X)
METHODS = ("sample", "grid", "brute", "host", "bunny")


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


def surfaces(dev):
    from neddf_amd.mesh import marching_cubes
    from time_mesh_clean import volume
    vol = torch.from_numpy(volume(256)).to(dev)
    lo, hi = (-1.0,) * 3, (1.0,) * 3
    return marching_cubes(vol, 0.0, lo, hi), marching_cubes(vol, 0.01, lo, hi)


def clouds(dev, n):
    from neddf_amd.mesh import sample_surface
    a, b = surfaces(dev)
    return sample_surface(*a, n=n, seed=0)[0], sample_surface(*b, n=n, seed=0)[0]


def checksum(d2, idx):
    """What two methods must agree on: the sum of the index and the fp64 sum of d2 (exact comparisons happen inside one process)."""
    return {"index_sum": int(idx.long().sum().item()), "d2_sum": float(d2.double().sum().item())}


def run_sample(repeats, dev):
    from neddf_amd.mesh import sample_surface
    a, _ = surfaces(dev)
    rows = []
    for n in SIZES:
        ms, (p, _) = timed(lambda: sample_surface(*a, n=n, seed=0), repeats, dev)
        rows.append({"requested": n, "samples": int(p.shape[0]), "triangles": int(a[1].shape[0]), "ms": ms})
    return rows


def run_grid(repeats, dev):
    from neddf_amd import Context
    from neddf_amd.geometry import default_cells
    ctx = Context.get(dev)
    rows = []
    for n in SIZES:
        q, t = clouds(dev, n)
        lo, hi = t.min(dim=0).values.double().tolist(), t.max(dim=0).values.double().tolist()
        for ppc in PER_CELL:
            cells = default_cells(t.shape[0], lo, hi, ppc)
            t_build, (start, order) = timed(lambda: ctx.nn_grid_build(t, lo, hi, cells), repeats, dev)
            t_query, (d2, idx) = timed(lambda: ctx.nn_grid_query(q, t, lo, hi, cells, start, order), repeats, dev)
            rows.append(dict(checksum(d2, idx), queries=int(q.shape[0]), targets=int(t.shape[0]), targets_per_cell=ppc, cells=list(cells),
                             build_ms=t_build, query_ms=t_query, total_ms=t_build + t_query))
    return rows


def run_brute(repeats, dev):
    from neddf_amd import Context
    from neddf_amd.geometry import nearest
    ctx = Context.get(dev)
    rows = []
    for n in SIZES:
        if n > BRUTE_MAX:
            continue
        q, t = clouds(dev, n)
        ms, (d2, idx) = timed(lambda: ctx.nn_brute(q, t), repeats if n < 10 ** 6 else min(repeats, 3), dev)
        gd, gi = nearest(q, t)                               # the grid with its defaults: the same bits
        same = bool(torch.equal(gi, idx.long()) and torch.equal(gd.view(torch.int32), torch.sqrt(d2).view(torch.int32)))
        rows.append(dict(checksum(d2, idx), queries=int(q.shape[0]), targets=int(t.shape[0]), ms=ms, runs=repeats if n < 10 ** 6 else min(repeats, 3),
                         identical_to_grid=same))
    return rows


def run_host(repeats, dev):
    from scipy.spatial import cKDTree
    from neddf_amd.geometry import nearest
    rows = []
    for n in SIZES:
        q, t = clouds(dev, n)
        parts = {}

        def host():
            t0 = time.perf_counter()
            qn, tn = q.cpu().numpy().astype(np.float64), t.cpu().numpy().astype(np.float64)
            t1 = time.perf_counter()
            tree = cKDTree(tn)
            t2 = time.perf_counter()
            d, i = tree.query(qn, workers=-1)
            parts.update(download_ms=(t1 - t0) * 1e3, build_ms=(t2 - t1) * 1e3, query_ms=(time.perf_counter() - t2) * 1e3)
            return d, i
        runs = repeats if n < 10 ** 6 else min(repeats, 3)
        ms, (d, i) = timed(host, runs, dev)
        gd, gi = nearest(q, t)
        err = float(np.abs(gd.cpu().numpy().astype(np.float64) - d).max())
        rows.append(dict(queries=int(q.shape[0]), targets=int(t.shape[0]), ms=ms, runs=runs, last_run=parts, cpus=len(os.sched_getaffinity(0)),
                         max_distance_difference_to_grid=err, indices_differing_from_grid=int((gi.cpu().numpy() != i).sum())))
    return rows


def run_bunny(repeats, dev):
    """The two questions the feature exists to answer, as numbers: how far bf16 operands move the level set, and how far a sparse
    extraction with too low a Lipschitz bound is from the one with the default."""
    from time_sparse_mesh import bunny
    from neddf_amd.geometry import mesh_distance
    net = bunny(dev)
    keys = ("a_to_b_mean", "b_to_a_mean", "chamfer", "hausdorff", "a_to_b_max", "b_to_a_max", "n_a", "n_b", "invalid_a", "invalid_b", "density")
    out = {}
    fp32 = net.extract_mesh(resolution=256)
    net.weight_dtype = "bf16"
    bf16 = net.extract_mesh(resolution=256)
    net.weight_dtype = "fp32"
    l1 = net.extract_mesh(resolution=256, brick=8, lipschitz=1.0)
    l025 = net.extract_mesh(resolution=256, brick=8, lipschitz=0.25)
    for name, a, b in (("fp32_vs_bf16", fp32, bf16), ("sparse_lipschitz_1_vs_0.25", l1, l025), ("dense_vs_sparse_lipschitz_1", fp32, l1)):
        ms, d = timed(lambda: mesh_distance(a, b, n=10 ** 6, seed=0, tau=2.0 * 2.2 / 255), repeats, dev)
        out[name] = dict({k: d[k] for k in keys}, tau=2.0 * 2.2 / 255, precision=d["precision"], recall=d["recall"], fscore=d["fscore"],
                         triangles_a=int(a[1].shape[0]), triangles_b=int(b[1].shape[0]), mesh_distance_ms=ms)
    out["note"] = "resolution 256, threshold 0.0275, cube_range 1.1, brick 8; about 10^6 samples per mesh, seed 0; tau = two lattice steps"
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_distance_cost.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--methods", nargs="+", default=list(METHODS), choices=METHODS)
    ap.add_argument("--method", default=None, choices=METHODS, help="(internal) run this one method and print its JSON")
    args = ap.parse_args(argv)
    if args.method:
        dev = torch.device("cuda:0")
        rows = {"sample": run_sample, "grid": run_grid, "brute": run_brute, "host": run_host, "bunny": run_bunny}[args.method](args.repeats, dev)
        print("CASE " + json.dumps(rows), flush=True)
        return None
    result = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats,
              "inputs": "level sets 0 and 0.01 of the synthetic sphere volume of tools/time_mesh_clean.py at 256^3; queries in sampling order"}
    for method in args.methods:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--method", method, "--repeats", str(args.repeats)],
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        if out.returncode != 0:
            raise SystemExit("%s failed (exit %d):\n%s" % (method, out.returncode, out.stdout[-4000:]))
        result[method] = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("CASE ")][-1][5:])
        print(method, json.dumps(result[method]), flush=True)
    if "grid" in result:
        at = [r for r in result["grid"] if r["queries"] == max(x["queries"] for x in result["grid"])]
        result["fastest_targets_per_cell_at_the_largest_size"] = min(at, key=lambda r: r["total_ms"])["targets_per_cell"]
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    return result


if __name__ == "__main__":
    main()
