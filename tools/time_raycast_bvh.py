"""`python tools/time_raycast_bvh.py [--out profiles/raycast_bvh_cost.json] [--repeats 5]` -- what rays through the BVH cost on the
device, next to the uniform grid and the brute kernel.

  scenes   the workloads of tools/time_raycast.py -- 800 x 800 pinhole rays against the level set 0 of tools/time_mesh_clean.py's seeded
           synthetic volume meshed at 128^3 and 256^3 -- and one scene the grid's default does not suit: the 256^3 mesh scaled by 1 / 64
           into a corner of the unit box, standing on a floor of two triangles that spans the box, seen by the same camera moved along
           (the object fills the frame as before; the rays that miss it meet the floor or nothing).  The default pad, 2^-12 of the box
           diagonal, is five triangle edges of the shrunk mesh there, so that scene is cast a second time with a pad of 2^-15.
  bvh      build (keys + sort + tree), query in row-major pixel order and in 8 x 8 pixel tiles (one wave64 = one tile), the mean and the
           largest number of leaves evaluated per ray, and bvh.occluded over the same rays in both orders.
  grid     raycast.build_grid at its default (TRIANGLES_PER_CELL) and the query in both orders.
  brute    the brute kernel.
  ao       the ambient-occlusion frame of the bunny view of tools/time_raycast.py (the shipped bunny meshed at resolution 256, 800 x 800,
           16 directions) through render_image_mesh, next to the plain depth / normal frame through the tree and through the grid.

Every time is the median of --repeats runs between device synchronises after one untimed warm-up; every method runs in a process of its
own; the three ray casts must agree on every scene (one checksum across the processes)."""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from time_raycast import SIZE, bunny_view, checksum, mesh, timed, view_rays          # noqa: E402

METHODS = ("bvh", "grid", "brute", "ao")
SCENES = ("128", "256", "corner", "corner, pad 2^-15")
SHRINK = 1.0 / 64.0
SMALL_PAD = 2.0 ** -15          # twice the least the grid accepts in the unit box: half a triangle of the shrunk mesh


def scene(name, dev):
    """(vertices, triangles, (origins, dirs) row-major, (origins, dirs) in 8 x 8 tiles, pad or None for the default)"""
    rays, tiled = view_rays(dev), view_rays(dev, tiles=True)
    if not name.startswith("corner"):
        v, t = mesh(int(name), dev)
        return v, t, rays, tiled, None
    v, t = mesh(256, dev)
    v = ((v + 1.0) * (0.5 * SHRINK)).contiguous()                   # [-1, 1]^3 -> [0, 1 / 64]^3
    floor = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0]], device=dev)
    n = v.shape[0]
    t = torch.cat([t, torch.tensor([[n, n + 1, n + 2], [n, n + 2, n + 3]], device=dev, dtype=t.dtype)]).contiguous()
    v = torch.cat([v, floor]).contiguous()
    move = lambda od: ((od[0] + 1.0) * (0.5 * SHRINK), od[1])       # the camera moves with the object; directions stay
    return v, t, move(rays), move(tiled), SMALL_PAD if name != "corner" else None


def row_of(name, v, t, rays, pad):
    return dict(scene=name, pad=pad, triangles=int(t.shape[0]), rays=int(rays[0].shape[0]))


def run_bvh(repeats, dev):
    from neddf_amd import bvh
    rows = []
    for name in SCENES:
        v, t, rays, tiled, pad = scene(name, dev)
        build_ms, tree = timed(lambda: bvh.build_bvh(v, t), repeats, dev)
        query_ms, hits = timed(lambda: bvh.cast_rays(*rays, v, t, bvh=tree, pad=pad), repeats, dev)
        tiles_ms, hits_tiled = timed(lambda: bvh.cast_rays(*tiled, v, t, bvh=tree, pad=pad), repeats, dev)
        occluded_ms, occ = timed(lambda: bvh.occluded(*rays, v, t, bvh=tree, pad=pad), repeats, dev)
        occluded_tiles_ms, _ = timed(lambda: bvh.occluded(*tiled, v, t, bvh=tree, pad=pad), repeats, dev)
        visits = bvh.cast_rays(*rays, v, t, bvh=tree, pad=pad, return_visits=True)["visits"]
        any_visits = bvh.occluded(*rays, v, t, bvh=tree, pad=pad, return_visits=True)[1]
        assert checksum(hits_tiled)["hits"] == checksum(hits)["hits"] == int(occ.sum().item())
        rows.append(dict(row_of(name, v, t, rays, pad), build_ms=build_ms, query_ms=query_ms, query_8x8_tiles_ms=tiles_ms, total_ms=build_ms + query_ms,
                         leaves_per_ray_mean=float(visits.double().mean().item()), leaves_per_ray_max=int(visits.max().item()),
                         occluded_ms=occluded_ms, occluded_8x8_tiles_ms=occluded_tiles_ms,
                         occluded_leaves_per_ray_mean=float(any_visits.double().mean().item()), **checksum(hits)))
        print(rows[-1], flush=True)
    return rows


def run_grid(repeats, dev):
    from neddf_amd.raycast import TRIANGLES_PER_CELL, build_grid, cast_rays
    rows = []
    for name in SCENES:
        v, t, rays, tiled, pad = scene(name, dev)
        build_ms, grid = timed(lambda: build_grid(v, t, pad=pad), repeats, dev)
        query_ms, hits = timed(lambda: cast_rays(*rays, v, t, grid=grid), repeats, dev)
        tiles_ms, hits_tiled = timed(lambda: cast_rays(*tiled, v, t, grid=grid), repeats, dev)
        assert checksum(hits_tiled)["hits"] == checksum(hits)["hits"]
        rows.append(dict(row_of(name, v, t, rays, pad), triangles_per_cell=TRIANGLES_PER_CELL, cells=list(grid.cells), pairs=int(grid.items.shape[0]),
                         build_ms=build_ms, query_ms=query_ms, query_8x8_tiles_ms=tiles_ms, total_ms=build_ms + query_ms, **checksum(hits)))
        print(rows[-1], flush=True)
    return rows


def run_brute(repeats, dev):
    from neddf_amd.raycast import cast_rays
    rows = []
    for name in SCENES:
        v, t, rays, _, pad = scene(name, dev)
        ms, hits = timed(lambda: cast_rays(*rays, v, t, method="brute", pad=pad), repeats, dev)
        rows.append(dict(row_of(name, v, t, rays, pad), brute_ms=ms, **checksum(hits)))
        print(rows[-1], flush=True)
    return rows


def run_ao(repeats, dev):
    from neddf_amd.bvh import build_bvh
    from neddf_amd.raycast import build_grid
    render, cam = bunny_view(dev, SIZE)
    v, t, nrm = render.get_network().extract_mesh(resolution=256, normals=True)
    plain = ["depth", "transmittance", "normal"]
    build_ms, tree = timed(lambda: build_bvh(v, t), repeats, dev)
    grid = build_grid(v, t)
    grid_ms, a = timed(lambda: render.render_image_mesh(SIZE, SIZE, cam, v, t, plain, normals=nrm, grid=grid), repeats, dev)
    tree_ms, b = timed(lambda: render.render_image_mesh(SIZE, SIZE, cam, v, t, plain, normals=nrm, bvh=tree), repeats, dev)
    tree_tiles_ms, c = timed(lambda: render.render_image_mesh(SIZE, SIZE, cam, v, t, plain, normals=nrm, bvh=tree, tile=8), repeats, dev)
    grid_tiles_ms, e = timed(lambda: render.render_image_mesh(SIZE, SIZE, cam, v, t, plain, normals=nrm, grid=grid, tile=8), repeats, dev)
    assert all(torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]) and torch.equal(a[k], e[k]) for k in plain)
    ao_ms, img = timed(lambda: render.render_image_mesh(SIZE, SIZE, cam, v, t, plain + ["ambient_occlusion"], normals=nrm, bvh=tree), repeats, dev)
    hit = img["transmittance"] == 0
    return dict(size=[SIZE, SIZE], resolution=256, triangles=int(t.shape[0]), ao_dirs=16, bvh_build_ms=build_ms, mesh_view_grid_ms=grid_ms,
                mesh_view_grid_8x8_tiles_ms=grid_tiles_ms, mesh_view_bvh_ms=tree_ms, mesh_view_bvh_8x8_tiles_ms=tree_tiles_ms,
                mesh_view_bvh_with_ambient_occlusion_ms=ao_ms, occlusion_rays=16 * int(hit.sum().item()), hit_share=float(hit.float().mean().item()),
                mean_ambient_occlusion_on_hits=float(img["ambient_occlusion"][hit].mean().item()))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raycast_bvh_cost.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--methods", nargs="+", default=list(METHODS), choices=METHODS)
    ap.add_argument("--method", default=None, choices=METHODS, help="(internal) run this one method and print its JSON")
    args = ap.parse_args(argv)
    if args.method:
        dev = torch.device("cuda:0")
        rows = {"bvh": run_bvh, "grid": run_grid, "brute": run_brute, "ao": run_ao}[args.method](args.repeats, dev)
        print("CASE " + json.dumps(rows), flush=True)
        return None
    result = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats,
              "inputs": "level set 0 of the synthetic sphere volume of tools/time_mesh_clean.py at 128^3 and 256^3, and the latter scaled by 1/64 "
                        "into a corner of the unit box over a two-triangle floor; %d x %d pinhole rays" % (SIZE, SIZE)}
    for method in args.methods:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--method", method, "--repeats", str(args.repeats)],
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        if out.returncode != 0:
            raise SystemExit("%s failed (exit %d):\n%s" % (method, out.returncode, out.stdout[-4000:]))
        result[method] = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("CASE ")][-1][5:])
        print(method, json.dumps(result[method]), flush=True)
    casts = [m for m in ("bvh", "grid", "brute") if m in result]
    if len(casts) > 1:                          # one checksum over all methods, scene by scene
        agree = {}
        for i, name in enumerate(SCENES):
            sums = [tuple(result[m][i][k] for k in ("hits", "triangle_sum", "t_sum")) for m in casts]
            agree[name] = all(s == sums[0] for s in sums)
        result["methods_agree"] = agree
        if not all(agree.values()):
            raise SystemExit("the ray casts disagree: %s" % json.dumps({m: result[m] for m in casts}))
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    return result


if __name__ == "__main__":
    main()
