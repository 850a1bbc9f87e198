"""`python neddf/scripts/render_mesh.py <run_dir> [--epoch 2000] [--mesh PATH.ply] [--compare-trace [THRESHOLD]] [--method grid|brute]
[--bvh] [--tiles] [--ao [K]] [--ortho SCALE]` --
views of an extracted mesh from the run's test cameras (no reference counterpart: the reference looks at its meshes in an Open3D
viewer).  The run is loaded as extract_mesh.py loads it; the mesh is read with neddf_amd.mesh.read_ply, by default the newest file
under `<run_dir>/mesh/`.  For every test camera NeRFRender.render_image_mesh casts the camera's rays -- the pixels of
render_image_traced and of the volume-rendered image -- at the mesh and `{id:03}_depth_mesh.png`, `{id:03}_normal_mesh.png` and, when
the file has vertex colours, `{id:03}_rgb_mesh.png` go to `<run_dir>/render/`, scaled as the traced view's; one line per view gives
the hit share and the time.  --compare-trace also sphere-traces the field at THRESHOLD (default: the one in the mesh's file name,
`mesh_{resolution}_threshold{threshold}.ply`) and prints per view the share of pixels hit by both, by the mesh only and by the
trace only, and the mean and maximum |t_mesh - t_traced| over the pixels hit by both.  --bvh casts the rays through the mesh's BVH
(neddf_amd.bvh: the same images, bit for bit) instead of --method's route, --tiles casts them ordered by 8 x 8 pixel tiles (the same
images again), and --ao [K] (K directions, default 16; implies --bvh) also writes `{id:03}_ao_mesh.png`, the ambient occlusion at the
hit points: a shaded look at the mesh.  --ortho SCALE looks from the test cameras' poses through an orthographic camera of SCALE pixels per
world unit (camera.OrthographicCalib, the principal point at the image centre) instead of the dataset's pinhole."""
import re
from argparse import ArgumentParser
from pathlib import Path


def build_parser() -> ArgumentParser:
    parser = ArgumentParser()
    parser.add_argument("output_dir", type=Path, help="directory path where models are located")
    parser.add_argument("--epoch", type=int, default=2000, help="epoch number of model")
    parser.add_argument("--mesh", type=Path, default=None, help="PLY file (default: the newest under <run_dir>/mesh/)")
    parser.add_argument("--compare-trace", type=float, nargs="?", const=float("nan"), default=None, metavar="THRESHOLD",
                        help="also sphere-trace the field at THRESHOLD (default: the one in the mesh's file name) and compare per pixel")
    parser.add_argument("--method", default="grid", choices=["grid", "brute"], help="ray casting through the grid or by brute force")
    parser.add_argument("--bvh", action="store_true", help="cast the rays through the mesh's BVH instead of --method's route (the same images)")
    parser.add_argument("--tiles", action="store_true", help="cast the rays ordered by 8 x 8 pixel tiles (the same images)")
    parser.add_argument("--ao", type=int, nargs="?", const=16, default=None, metavar="K",
                        help="also write {id:03}_ao_mesh.png: ambient occlusion from K directions (default 16); implies --bvh")
    parser.add_argument("--ortho", type=float, default=None, metavar="SCALE",
                        help="orthographic views from the test cameras' poses, SCALE pixels per world unit")
    return parser


def threshold_of(path) -> float:
    """The threshold in a file name extract_mesh.py writes, mesh_{resolution}_threshold{threshold}.ply; ValueError without one."""
    m = re.search(r"threshold([-+0-9.eE]+?)\.ply$", Path(path).name)
    try:
        return float(m.group(1))
    except (AttributeError, ValueError):
        raise ValueError("%s: no threshold in the file name; give --compare-trace THRESHOLD" % path) from None


def newest_mesh(output_dir: Path) -> Path:
    files = sorted((output_dir / "mesh").glob("*.ply"), key=lambda p: (p.stat().st_mtime, p.name))
    if not files:
        raise FileNotFoundError("no .ply under %s: run extract_mesh.py first, or give --mesh" % (output_dir / "mesh"))
    return files[-1]


def compare_hits(t_mesh, hit_mesh, t_traced, hit_traced) -> dict:
    """Shares of the pixels hit by both, by the mesh only and by the trace only, and mean / max |t_mesh - t_traced| over `both`."""
    both = hit_mesh & hit_traced
    n = float(hit_mesh.numel())
    diff = (t_mesh - t_traced).abs()[both].double()
    return {"both": float(both.sum()) / n, "mesh_only": float((hit_mesh & ~hit_traced).sum()) / n,
            "trace_only": float((hit_traced & ~hit_mesh).sum()) / n,
            "mean_abs_dt": float(diff.mean()) if diff.numel() else float("nan"), "max_abs_dt": float(diff.max()) if diff.numel() else float("nan")}


def main(argv=None) -> list:
    args = build_parser().parse_args(argv)
    import time

    import numpy as np
    import torch

    from neddf_amd.bvh import build_bvh
    from neddf_amd.mesh import read_ply
    from neddf_amd.raycast import build_grid
    from neddf_amd.scripts.run_eval import load_config, load_trainer
    from neddf_amd.trainer import imwrite_bgr
    output_dir = args.output_dir.resolve()
    path = args.mesh if args.mesh is not None else newest_mesh(output_dir)
    threshold = None
    if args.compare_trace is not None:
        threshold = threshold_of(path) if args.compare_trace != args.compare_trace else args.compare_trace
    trainer = load_trainer(load_config(output_dir), output_dir, args.epoch)
    if args.ortho is not None:
        trainer.use_orthographic_cameras(args.ortho)
    render = trainer.neural_render
    render.set_iter(-1)
    dev = trainer.device
    verts, tris, normals, colors = (None if a is None else torch.from_numpy(a).to(dev) for a in read_ply(path, properties=True))
    use_bvh = args.bvh or args.ao is not None
    if use_bvh and args.method != "grid":
        raise SystemExit("render_mesh.py: --bvh and --ao cast the rays through the tree; leave --method at its default")
    grid = build_grid(verts, tris) if args.method == "grid" and not use_bvh else None
    bvh = build_bvh(verts, tris) if use_bvh else None
    targets = ["depth", "transmittance", "normal"] + (["color"] if colors is not None else []) + (["ambient_occlusion"] if args.ao is not None else [])
    save_dir = output_dir / "render"
    save_dir.mkdir(exist_ok=True)
    print("mesh %s: %d vertices, %d triangles" % (path, verts.shape[0], tris.shape[0]))
    rows = []
    for camera_id in range(len(trainer.dataset)):
        camera = trainer.cameras[camera_id]
        camera.update_transform()
        h, w = trainer.dataset[camera_id]["rgb_images"].shape[:2]
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        images = render.render_image_mesh(w, h, camera, verts, tris, targets, normals=normals, colors=colors, method=args.method, grid=grid, bvh=bvh,
                                          tile=8 if args.tiles else 0, ao_dirs=args.ao if args.ao is not None else 16)
        torch.cuda.synchronize(dev)
        ms = 1e3 * (time.perf_counter() - t0)
        depth = torch.clamp((images["depth"] - 2.0) / 4.0 * 50000 / 256, 0, 255).cpu().numpy().astype(np.uint8)
        imwrite_bgr(save_dir / "{:03}_depth_mesh.png".format(camera_id), depth)
        nrm = torch.clamp((images["normal"] * 0.5 + 0.5) * 255, 0, 255).cpu().numpy().astype(np.uint8)
        imwrite_bgr(save_dir / "{:03}_normal_mesh.png".format(camera_id), np.ascontiguousarray(nrm[:, :, ::-1]))
        if colors is not None:
            imwrite_bgr(save_dir / "{:03}_rgb_mesh.png".format(camera_id), torch.clamp(images["color"] * 255, 0, 255).cpu().numpy().astype(np.uint8))
        if args.ao is not None:
            imwrite_bgr(save_dir / "{:03}_ao_mesh.png".format(camera_id), torch.clamp(images["ambient_occlusion"] * 255, 0, 255).cpu().numpy().astype(np.uint8))
        row = {"camera": camera_id, "hit_share": 1.0 - float(images["transmittance"].mean()), "ms": ms}
        print("mesh camera {}: hit share {:.4f}, {:.1f} ms".format(camera_id, row["hit_share"], ms))
        if threshold is not None:
            traced = render.render_image_traced(w, h, camera, ["depth", "transmittance"], threshold)
            row.update(compare_hits(images["depth"], images["transmittance"] == 0, traced["depth"], traced["transmittance"] == 0))
            print("mesh against trace, camera {}: both {:.4f}, mesh only {:.4f}, trace only {:.4f}, |t_mesh - t_traced| mean {:.3e} max {:.3e}".format(
                camera_id, row["both"], row["mesh_only"], row["trace_only"], row["mean_abs_dt"], row["max_abs_dt"]))
        rows.append(row)
    return rows


if __name__ == "__main__":
    main()
