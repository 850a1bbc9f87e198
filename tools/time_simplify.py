"""`python tools/time_simplify.py [--out profiles/simplify_cost.json] [--repeats 5]` -- what mesh simplification by vertex clustering
(mesh.simplify_mesh) costs on the device, what it removes and how far the result is from the mesh it came from.

Meshes: the seeded synthetic volume of tools/time_mesh_clean.py (one large sphere, 300 small ones) at 128^3 and 256^3 through
marching cubes, and the shipped bunny network at resolution 256 and 512 through the sparse extraction (brick = 8).  For cells of
K = 2, 4 and 8 lattice steps and both placements: the stage times (keys, sort, clusters, placement, triangles, compaction; each the
median of --repeats runs between device synchronises, after a warm-up), the time of the whole call without the stage synchronises,
the counts before and after, and the one-way maximum and mean distance from the simplified surface to the original one
(geometry.mesh_distance, to="surface", 100 000 samples, through the BVH).  For comparison the numpy restatement of
tests/simplify_check.py on the host, download and upload included (--host-repeats runs), and whether its mesh is the device's bit
for bit.  Times in milliseconds; writes JSON."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

STAGES = ("keys", "sort", "clusters", "placement", "triangles", "compaction")


def timed(fn, repeats, dev):
    """(median milliseconds, the last result): synchronise, run, synchronise."""
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), out


def sphere_mesh(res, dev):
    from time_mesh_clean import volume
    from neddf_amd.mesh import marching_cubes
    v, t = marching_cubes(torch.from_numpy(volume(res)).to(dev), 0.0, (-1.0,) * 3, (1.0,) * 3)
    return v, t, 2.0 / (res - 1)


def bunny_mesh(res, dev):
    from neddf_amd import NeDDF
    from neddf_amd.fixtures import BUNNY_SMOKE_CFG, bunny_smoke_weights
    net = NeDDF(**BUNNY_SMOKE_CFG)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in bunny_smoke_weights().items()})
    net.to(dev)
    net.set_iter(-1)
    for p in net.parameters():
        p.requires_grad_(False)
    v, t = net.extract_mesh(resolution=res, brick=8)
    return v, t, 2.0 * 1.1 / (res - 1)


def measure(name, res, v, t, step, steps, repeats, host_repeats, dev):
    import simplify_check as sc
    from neddf_amd.geometry import mesh_distance
    from neddf_amd.mesh import simplify_mesh
    case = {"mesh": name, "resolution": res, "lattice_step": step, "vertices": int(len(v)), "triangles": int(len(t)), "runs": []}
    for K in steps:
        cell = K * step
        for placement in ("mean", "quadric"):
            simplify_mesh(v, t, cell=cell, placement=placement)              # warm-up: workspaces allocated, kernels loaded, sorts tuned
            stage_ms = {s: [] for s in STAGES}
            for _ in range(repeats):
                times = {}
                simplify_mesh(v, t, cell=cell, placement=placement, timings=times)
                for s in STAGES:
                    stage_ms[s].append(times[s] * 1e3)
            total, gpu = timed(lambda: simplify_mesh(v, t, cell=cell, placement=placement), repeats, dev)
            dist = mesh_distance((gpu[0], gpu[1]), (v, t), n=100000, to="surface", method="bvh") if len(gpu[1]) else None

            def host():
                vn, tn = v.cpu().numpy(), t.cpu().numpy()
                t0 = time.perf_counter()
                out = sc.simplify(vn, tn, cell=cell, placement=placement)
                host.compute = (time.perf_counter() - t0) * 1e3
                return [torch.from_numpy(a).to(dev) for a in out]
            t_host, ref = timed(host, host_repeats, dev)
            same = all(a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(gpu, ref))
            case["runs"].append({"cell_steps": K, "cell": cell, "placement": placement, "vertices_after": int(len(gpu[0])),
                                 "triangles_after": int(len(gpu[1])),
                                 "gpu_ms": dict({s: float(np.median(stage_ms[s])) for s in STAGES}, whole_call=total),
                                 "to_original_max": None if dist is None else dist["a_to_b_max"],
                                 "to_original_mean": None if dist is None else dist["a_to_b_mean"],
                                 "host_ms": {"whole_call": t_host, "of_which_numpy": host.compute}, "host_matches_bit_for_bit": bool(same)})
            print(json.dumps(dict(case["runs"][-1], mesh=name, resolution=res)), flush=True)
    return case


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_cost.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--sphere", type=int, nargs="*", default=[128, 256], help="resolutions of the synthetic volume")
    ap.add_argument("--bunny", type=int, nargs="*", default=[256, 512], help="resolutions of the shipped bunny (brick = 8)")
    ap.add_argument("--steps", type=int, nargs="+", default=[2, 4, 8], help="cell edges in lattice steps")
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    cases = []
    for name, make, resolutions in (("synthetic spheres", sphere_mesh, args.sphere), ("bunny", bunny_mesh, args.bunny)):
        for res in resolutions:
            v, t, step = make(res, dev)
            cases.append(measure(name, res, v, t, step, args.steps, args.repeats, args.host_repeats, dev))
    result = {"device": torch.cuda.get_device_name(dev), "repeats": args.repeats, "host_repeats": args.host_repeats,
              "regularisation": 2.0 ** -10, "distance_samples": 100000, "cases": cases}
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("wrote %s" % args.out)
    return result


if __name__ == "__main__":
    main()
