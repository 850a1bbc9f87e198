"""`python tools/time_bvh.py [--out profiles/bvh_cost.json] [--repeats 5]` -- what the point-to-mesh distance costs through the triangle
BVH (neddf_amd/bvh.py), next to the grid query and the brute kernel of the same tree, on the workloads of tools/time_point_mesh.py:

  uniform   10^4 queries uniform in the mesh's box against the 256^3 mesh -- far from the surface, the case the BVH exists for; first
  near      about 10^4, 10^5 and 10^6 surface samples of the level set 0.01 against the level set 0 at 128^3 and 256^3

Per row: the build (keys, torch.sort, topology and boxes; the grid's build for the grid), the query, the mean and the largest number of
leaf evaluations per query (the kernel's own count) and a checksum that must agree across the methods (they return the same bits).
Every time is the median of --repeats runs between device synchronises after one untimed warm-up; every method runs in a process of its
own.  The private segment size of pm_bvh_kernel is read from the gfx950 assembly's metadata (0: the traversal stack is in LDS)."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from time_point_mesh import RESOLUTIONS, SIZES, checksum, queries, surfaces, timed          # noqa: E402

METHODS = ("bvh", "grid", "brute")


def uniform_queries(v, dev):
    lo, hi = v.min(dim=0).values, v.max(dim=0).values
    u = torch.from_numpy(np.random.default_rng(0).random((10 ** 4, 3)).astype(np.float32)).to(dev)
    return (lo + u * (hi - lo)).contiguous()


def workloads(dev):
    """(name, resolution, (v, t), queries), the uniform case first."""
    meshes = {res: surfaces(res, dev) for res in RESOLUTIONS}
    v, t = meshes[256][0]
    yield "uniform", 256, (v, t), uniform_queries(v, dev)
    for res in RESOLUTIONS:
        mesh, other = meshes[res]
        for n in SIZES:
            yield "near", res, mesh, queries(other, n)


def run(method, repeats, dev):
    from neddf_amd import Context
    from neddf_amd.bvh import build_bvh
    from neddf_amd.raycast import build_grid
    ctx = Context.get(dev)
    rows, built = [], {}
    for name, res, (v, t), q in workloads(dev):
        row = dict(workload=name, resolution=res, triangles=int(t.shape[0]), queries=int(q.shape[0]), method=method)
        runs = repeats if method != "brute" or q.shape[0] < 10 ** 6 else min(repeats, 2)
        if method == "bvh":
            if res not in built:
                built[res] = timed(lambda: build_bvh(v, t), repeats, dev)
            row["build_ms"], tree = built[res]
            ms, out = timed(lambda: ctx.point_mesh_bvh_query(q, v, t, tree.leaf_triangle, tree.children, tree.boxes, return_visits=True), runs, dev)
            visits = out[4][torch.isfinite(out[0])].double()
            row.update(visits_mean=float(visits.mean().item()), visits_max=int(visits.max().item()))
        elif method == "grid":
            if res not in built:
                built[res] = timed(lambda: build_grid(v, t), repeats, dev)
            row["build_ms"], grid = built[res]
            ms, out = timed(lambda: ctx.point_mesh_grid_query(q, v, t, grid.lo, grid.hi, grid.cells, grid.pad, grid.cell_start, grid.items), runs, dev)
        else:
            ms, out = timed(lambda: ctx.point_mesh_brute(q, v, t), runs, dev)
        row.update(query_ms=ms, runs=runs, mean_distance=float(torch.sqrt(out[0]).double().mean().item()), **checksum(out))
        rows.append(row)
        print(row, flush=True)
    return rows


def private_segment_size():
    """.private_segment_fixed_size of pm_bvh_kernel in the gfx950 assembly of bvh_kernels.hip; None when it cannot be compiled here."""
    src = os.path.join(ROOT, "neddf_amd", "csrc", "bvh_kernels.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "bvh.s")
        try:
            subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--cuda-device-only", "-S", "-o", asm, src],
                           check=True, capture_output=True, timeout=300)
        except (OSError, subprocess.SubprocessError):
            return None
        text = open(asm).read()
    for block in text.split("- .agpr_count:")[1:]:
        if re.search(r"\.name:\s+\S*pm_bvh_kernel", block):
            m = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
            return int(m.group(1)) if m else None
    return None


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bvh_cost.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--methods", nargs="+", default=list(METHODS), choices=METHODS)
    ap.add_argument("--method", default=None, choices=METHODS, help="(internal) run this one method and print its JSON")
    args = ap.parse_args(argv)
    if args.method:
        print("CASE " + json.dumps(run(args.method, args.repeats, torch.device("cuda:0"))), flush=True)
        return None
    result = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats,
              "inputs": "tools/time_point_mesh.py's: the level set 0 of the synthetic sphere volume at 128^3 and 256^3; queries uniform in the 256^3 "
                        "mesh's box, and surface samples of the level set 0.01",
              "pm_bvh_kernel_private_segment_bytes": private_segment_size(), "rows": []}
    for method in args.methods:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--method", method, "--repeats", str(args.repeats)],
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        if out.returncode != 0:
            raise SystemExit("%s failed (exit %d):\n%s" % (method, out.returncode, out.stdout[-4000:]))
        result[method] = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("CASE ")][-1][5:])
        print(method, "done", flush=True)
    by_case = {}
    for method in args.methods:
        for r in result.pop(method):
            by_case.setdefault((r["workload"], r["resolution"], r["queries"]), {})[method] = r
    for (name, res, n), ms in by_case.items():            # the uniform case first (insertion order)
        first = next(iter(ms.values()))
        row = dict(workload=name, resolution=res, triangles=first["triangles"], queries=n, mean_distance=first["mean_distance"],
                   identical=len({(r["triangle_sum"], r["d2_sum"]) for r in ms.values()}) == 1)
        for method, r in ms.items():
            row[method + "_query_ms"] = r["query_ms"]
            if "build_ms" in r:
                row[method + "_build_ms"] = r["build_ms"]
            if "visits_mean" in r:
                row.update(bvh_visits_mean=r["visits_mean"], bvh_visits_max=r["visits_max"])
        result["rows"].append(row)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result["rows"], indent=1))
    return result


if __name__ == "__main__":
    main()
