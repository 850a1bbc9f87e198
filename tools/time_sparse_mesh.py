"""`python tools/time_sparse_mesh.py [--out profiles/sparse_mesh_cost.json] [--repeats 5]` -- what brick-wise (sparse) surface
extraction costs against the dense route, on the shipped bunny network with fp32 operands.

Per resolution (256 and 512: dense against brick=8, the median of --repeats runs after a warm-up; 1024: brick=8 the same way plus ONE
dense run) it records extract_mesh's own stage times (each ends in a device synchronise), the wall time of the whole call, the active
and total bricks, the number of lattice points the field was evaluated at, V, T, the extra device memory at the peak, and whether the
two meshes are identical bit for bit (their SHA-256).  Every route of every resolution runs in a fresh child process (the library's
workspaces only ever grow); memory = the growth of the device's used memory outside torch's allocator (the library's workspaces, which stay
allocated) plus the peak of torch's allocator above its level before the call."""
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

THRESHOLD, CUBE_RANGE, BRICK = 0.0275, 1.1, 8


def bunny(dev):
    from neddf_amd import NeDDF
    from neddf_amd.fixtures import BUNNY_SMOKE_CFG, bunny_smoke_weights
    net = NeDDF(**BUNNY_SMOKE_CFG)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in bunny_smoke_weights().items()})
    net.to(dev)
    net.set_iter(-1)
    for p in net.parameters():
        p.requires_grad_(False)
    assert net.weight_dtype == "fp32"
    return net


def used_outside_torch(dev):
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info(dev)
    return total - free - torch.cuda.memory_reserved(dev)


def run(net, res, brick, repeats, warm):
    """Stage medians (ms) of `repeats` calls after `warm` warm-up calls, the last mesh, and the memory the first call added."""
    dev = net.device
    kw = dict(threshold=THRESHOLD, cube_range=CUBE_RANGE, resolution=res, brick=brick)
    before_lib, before_torch = used_outside_torch(dev), torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    rows, mesh = [], None
    for i in range(warm + repeats):
        mesh = None                                  # the previous mesh is not part of this call's footprint
        times = {}
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        mesh = net.extract_mesh(timings=times, **kw)
        torch.cuda.synchronize(dev)
        times["total"] = time.perf_counter() - t0
        if i == 0:
            peak_torch = torch.cuda.max_memory_allocated(dev) - before_torch
        if i >= warm:
            rows.append(times)
    lib = used_outside_torch(dev) - before_lib
    out = {"runs": repeats, "warm_up_runs": warm,
           "ms": {k: float(np.median([r[k] for r in rows])) * 1e3 for k in ("coarse", "grid", "mcubes", "total") if k in rows[0]},
           "vertices": int(mesh[0].shape[0]), "triangles": int(mesh[1].shape[0]),
           "peak_extra_device_bytes": int(peak_torch + lib), "of_which_library_workspaces": int(lib)}
    if brick:
        nb = -(-(res - 1) // brick)
        out.update(bricks_active=int(rows[0]["bricks_active"]), bricks_total=int(rows[0]["bricks"]),
                   evaluated_points=int((nb + 1) ** 3 + rows[0]["bricks_active"] * (brick + 1) ** 3))
    else:
        out["evaluated_points"] = res ** 3
    return out, mesh


def case(res, mode, repeats):
    import hashlib
    dev = torch.device("cuda:0")
    net = bunny(dev)
    net.extract_mesh(resolution=16, brick=4)         # the context, the packed weights and the kernels' code objects exist
    net.extract_mesh(resolution=16)
    if mode == "sparse":
        out, mesh = run(net, res, BRICK, repeats, 1)
    else:
        out, mesh = run(net, res, 0, *((repeats, 1) if res < 1024 else (1, 0)))
    out["mesh_sha256"] = hashlib.sha256(b"".join(t.cpu().numpy().tobytes() for t in mesh)).hexdigest()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_mesh_cost.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--case", type=int, default=0, help="(internal) measure this one resolution and print its JSON")
    ap.add_argument("--mode", default="sparse", choices=["sparse", "dense"], help="(internal) the route --case measures")
    args = ap.parse_args(argv)
    if args.case:
        print("CASE " + json.dumps(case(args.case, args.mode, args.repeats)), flush=True)
        return None
    cases = []
    for res in args.resolutions:
        row = {"resolution": res, "brick": BRICK}
        for mode in ("sparse", "dense"):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(res), "--mode", mode, "--repeats", str(args.repeats)],
                                 stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
            if out.returncode != 0:
                raise SystemExit("resolution %d (%s) failed (exit %d):\n%s" % (res, mode, out.returncode, out.stdout[-4000:]))
            row[mode] = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("CASE ")][-1][5:])
        row["meshes_identical"] = row["sparse"]["mesh_sha256"] == row["dense"]["mesh_sha256"]
        cases.append(row)
        print(json.dumps(row), flush=True)
    result = {"device": torch.cuda.get_device_name(0), "network": "bunny_smoke_weights (NeDDF), fp32 operands", "field": "distance",
              "threshold": THRESHOLD, "cube_range": CUBE_RANGE, "band": "default (lipschitz 1)", "repeats": args.repeats, "cases": cases}
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    return result


if __name__ == "__main__":
    main()
