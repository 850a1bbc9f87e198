"""`python tools/time_mesh_clean.py [--out profiles/mesh_clean_cost.json] [--repeats 5]` -- what floater removal costs on the
device against the host route it replaces.

Volume: a seeded synthetic one at 128^3 and 256^3 on [-1, 1]^3, one large sphere plus 300 small ones around it (the smoke
network's bunny has too few components to time anything).  GPU route: marching cubes, then remove_small_components with
min_triangles=64 split into its stages (labelling, selection, compaction), each timed after a warm-up with a device synchronise
at both ends.  Host route, in the same process: download the mesh, scipy.sparse.csgraph.connected_components, numpy selection
and compaction, upload.  Both routes must produce the same mesh.  Writes the vertex, triangle and component counts, the
union-find rounds and the times (milliseconds, the median of --repeats runs) as JSON."""
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


def volume(res, seed=7, n_small=300):
    """float32 [res, res, res]: min over the spheres of (distance to the centre - radius); the small spheres are written into the
    boxes around them only (outside its box a small sphere is farther than the grid step, so the sign is unchanged)."""
    rng = np.random.default_rng(seed)
    ax = np.linspace(-1.0, 1.0, res)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    vol = np.sqrt(x * x + y * y + z * z) - 0.45
    step = 2.0 / (res - 1)
    for _ in range(n_small):
        c = rng.uniform(-0.9, 0.9, 3)
        if np.linalg.norm(c) < 0.6:
            c *= 0.6 / max(np.linalg.norm(c), 1e-6)         # keep it off the large sphere
            c = np.clip(c, -0.9, 0.9)
        r = rng.uniform(0.02, 0.07)
        lo = np.clip(np.floor((c - r + 1.0) / step).astype(int) - 2, 0, res - 1)
        hi = np.clip(np.ceil((c + r + 1.0) / step).astype(int) + 3, 1, res)
        sl = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
        d = np.sqrt((x[sl] - c[0]) ** 2 + (y[sl] - c[1]) ** 2 + (z[sl] - c[2]) ** 2) - r
        vol[sl] = np.minimum(vol[sl], d)
    return vol.astype(np.float32)


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


def measure(res, repeats, dev):
    import mesh_clean_check as cc
    from neddf_amd import Context
    from neddf_amd.mesh import compact_mesh, connected_components, marching_cubes, remove_small_components, select_components
    ctx = Context.get(dev)
    vol = torch.from_numpy(volume(res)).to(dev)
    lo, hi = (-1.0,) * 3, (1.0,) * 3
    v, t = marching_cubes(vol, 0.0, lo, hi)                 # warm-up of every stage: workspaces allocated, kernels loaded
    remove_small_components(v, t, 64, 0)
    t_mc, (v, t) = timed(lambda: marching_cubes(vol, 0.0, lo, hi), repeats, dev)
    t_label, (_, tri_label, sizes) = timed(lambda: connected_components(t, len(v)), repeats, dev)
    rounds = ctx.mesh_components_rounds()

    def select():
        return (tri_label >= 0) & select_components(sizes, 64, 0)[tri_label.clamp_min(0).long()]
    t_select, keep = timed(select, repeats, dev)
    t_compact, _ = timed(lambda: compact_mesh(v, t, keep), repeats, dev)
    t_clean, gpu = timed(lambda: remove_small_components(v, t, 64, 0), repeats, dev)

    def host():
        vn, tn = v.cpu().numpy(), t.cpu().numpy()
        t0 = time.perf_counter()
        ov, ot, _ = cc.remove_small_components(vn, tn, 64, 0)
        t1 = time.perf_counter()
        host.compute = (t1 - t0) * 1e3
        return torch.from_numpy(ov).to(dev), torch.from_numpy(ot).to(dev)
    host()
    t_host, ref = timed(host, repeats, dev)
    assert torch.equal(gpu[0].view(torch.int32), ref[0].view(torch.int32)) and torch.equal(gpu[1], ref[1]), "the two routes disagree"
    return {"resolution": res, "vertices": int(len(v)), "triangles": int(len(t)), "components": int(sizes.numel()),
            "components_kept": int((sizes >= 64).sum().item()), "vertices_kept": int(len(gpu[0])), "triangles_kept": int(len(gpu[1])),
            "union_find_rounds": rounds,
            "gpu_ms": {"marching_cubes": t_mc, "labelling": t_label, "selection": t_select, "compaction": t_compact, "clean_up": t_clean},
            "host_ms": {"clean_up": t_host, "of_which_scipy_and_numpy": host.compute}}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_clean_cost.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[128, 256])
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(dev), "min_triangles": 64, "repeats": args.repeats,
              "cases": [measure(r, args.repeats, dev) for r in args.resolutions]}
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
