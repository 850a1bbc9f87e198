"""`python neddf/scripts/run_eval.py <run_dir> [--epoch N]` -- same command line,
inputs (`<run_dir>/.hydra/config.yaml`, `<run_dir>/models/model_{epoch:05}.pth`)
and outputs (`<run_dir>/eval/*.png`, psnr/ssim printout) as the reference's
neddf/scripts/run_eval.py:10-44.  The frozen config is read with PyYAML and the
`dataset.data_split=test` override applied by hand (hydra is not required).

Under a launcher (`python -m torch.distributed.run --nproc-per-node N neddf/scripts/run_eval.py <run_dir>`; not in the
reference) the rays of every view are sharded over the N GPUs (contiguous slabs of the pixel index, one RCCL all-gather of
20 B/ray per view, BASELINE.json configs[3]); rank 0 writes the PNGs and prints the metrics.  Every rank seeds identically
and jumps torch's CPU generator to its slab, so the images are the single-GPU ones bit for bit."""
import os
from argparse import ArgumentParser
from pathlib import Path

import torch
import yaml

from neddf_amd.config import instantiate


def load_config(output_dir: Path) -> dict:
    """The run's frozen `.hydra/config.yaml` with the test split selected (the reference's override)."""
    conf = output_dir / ".hydra" / "config.yaml"
    assert conf.is_file(), conf
    cfg = yaml.safe_load(open(conf))
    cfg["dataset"]["data_split"] = "test"
    return cfg


def load_trainer(cfg: dict, output_dir: Path, epoch: int):
    """The trainer of `cfg` with the checkpoint `models/model_{epoch:05}.pth` of the run loaded."""
    trainer = instantiate(cfg["trainer"], global_config=cfg, _recursive_=False)
    trainer.load_pretrained_model(output_dir / "models/model_{:05}.pth".format(epoch))
    return trainer


def build_parser() -> ArgumentParser:
    parser = ArgumentParser()
    parser.add_argument("output_dir", type=Path, help="directory path where models and render are located")
    parser.add_argument("--epoch", type=int, default=2000, help="epoch number of model")
    parser.add_argument("--seed", type=int, default=None,
                        help="torch seed for the sample uniforms (not a reference option: the reference's run_eval never seeds, and "
                             "torch seeds its default generator randomly per process)")
    parser.add_argument("--normals", action="store_true",
                        help="also write {id:03}_normal.png, the normal render target as clamp((n * 0.5 + 0.5) * 255) with world "
                             "x, y, z as R, G, B (not a reference option; NeDDF and NeuS fields, one device)")
    parser.add_argument("--skip-empty", type=int, nargs="?", const=128, default=None, metavar="R",
                        help="skip empty space: build an R^3 occupancy grid (default 128) from the loaded networks and render through "
                             "the culled entry points (not a reference option; world-space rays; prints the occupied fraction and "
                             "kept / total samples)")
    parser.add_argument("--trace", type=float, default=None, metavar="THRESHOLD",
                        help="also render every view by sphere tracing the distance field to this level set (extract_mesh's threshold; "
                             "0.0275 for the shipped bunny) and write {id:03}_rgb_traced.png / _depth_traced.png (and _normal_traced.png "
                             "with --normals) next to the usual images; prints hit share, mean advances per ray and milliseconds per "
                             "view (not a reference option; NeDDF and NeuS fields, world-space rays, rank 0's device)")
    parser.add_argument("--ortho", type=float, default=None, metavar="SCALE",
                        help="render the test cameras' poses through an orthographic camera of SCALE pixels per world unit, the "
                             "principal point at the image centre (not a reference option; an inspection view: the PSNR / SSIM "
                             "against the dataset's perspective images then mean nothing; one device)")
    parser.add_argument("--trace-steps", type=int, default=64, metavar="N", help="marching iterations of --trace (default 64)")
    return parser


def render_traced(trainer, save_dir: Path, threshold: float, max_steps: int, normals: bool) -> None:
    """Every test view through NeRFRender.render_image_traced: the images with a _traced suffix and one line per view."""
    import time

    import numpy as np

    from neddf_amd.trainer import imwrite_bgr
    trainer.neural_render.set_iter(-1)
    targets = ["color", "depth", "transmittance", "steps"] + (["normal"] if normals else [])
    for camera_id in range(len(trainer.dataset)):
        camera = trainer.cameras[camera_id]
        camera.update_transform()
        h, w = trainer.dataset[camera_id]["rgb_images"].shape[:2]
        torch.cuda.synchronize(trainer.device)
        t0 = time.perf_counter()
        images = trainer.neural_render.render_image_traced(w, h, camera, targets, threshold, max_steps=max_steps)
        torch.cuda.synchronize(trainer.device)
        ms = 1e3 * (time.perf_counter() - t0)
        rgb = torch.clamp(images["color"] * 255, 0, 255).cpu().numpy().astype(np.uint8)
        depth = torch.clamp((images["depth"] - 2.0) / 4.0 * 50000 / 256, 0, 255).cpu().numpy().astype(np.uint8)
        imwrite_bgr(save_dir / "{:03}_rgb_traced.png".format(camera_id), rgb)
        imwrite_bgr(save_dir / "{:03}_depth_traced.png".format(camera_id), depth)
        if normals:
            nrm = torch.clamp((images["normal"] * 0.5 + 0.5) * 255, 0, 255).cpu().numpy().astype(np.uint8)
            imwrite_bgr(save_dir / "{:03}_normal_traced.png".format(camera_id), np.ascontiguousarray(nrm[:, :, ::-1]))
        print("traced camera {}: hit share {:.4f}, mean advances per ray {:.2f}, {:.1f} ms".format(
            camera_id, 1.0 - float(images["transmittance"].mean()), float(images["steps"].float().mean()), ms))


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    output_dir = args.output_dir.resolve()
    cfg = load_config(output_dir)
    world, rank, local = (int(os.environ.get(k, d)) for k, d in (("WORLD_SIZE", "1"), ("RANK", "0"), ("LOCAL_RANK", "0")))
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        n_dev = torch.cuda.device_count()
        # NEDDF_DIST_BACKEND=gloo: ranks may share devices (tests on a one-GPU box); the pixel slabs are then staged through the host
        backend = os.environ.get("NEDDF_DIST_BACKEND", "nccl")
        local = local % max(n_dev, 1)
        torch.cuda.set_device(local)
        if backend == "nccl":
            torch.distributed.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            torch.distributed.init_process_group(backend)
        cfg["trainer"]["device"] = "cuda:%d" % local
    trainer = load_trainer(cfg, output_dir, args.epoch)
    trainer.writes_outputs = rank == 0
    if args.ortho is not None:
        if world > 1:
            raise SystemExit("run_eval.py: --ortho renders ray bundles, which are not ray-sharded; run it on one device")
        trainer.use_orthographic_cameras(args.ortho)
    save_dir = args.output_dir / "eval"
    if rank == 0:
        save_dir.mkdir(exist_ok=True)
    # ray sharding replays ONE stream of uniforms (each rank jumps the CPU generator to its slab): every rank needs rank 0's seed
    seed = args.seed
    if world > 1:
        box = [torch.initial_seed() if seed is None else seed]
        torch.distributed.broadcast_object_list(box, src=0)
        seed = int(box[0]) % (1 << 63)
    if seed is not None:
        torch.manual_seed(seed)
    if args.skip_empty is not None:
        # after the checkpoint is loaded, in the state render_all evaluates in; the grid is integer-valued: every rank builds the same one
        trainer.neural_render.set_iter(-1)
        grid = trainer.neural_render.build_occupancy(resolution=args.skip_empty)
        if rank == 0:
            print("skip-empty: %d^3 grid, %.2f %% of the cells occupied" % (grid.resolution, 100.0 * grid.occupied_fraction))
        from neddf_amd import Context
        Context.get(grid.device).cull_stats(reset=True)
    if args.normals:
        trainer.render_all(save_dir, normals=True)
    else:
        trainer.render_all(save_dir)
    if args.trace is not None and rank == 0:
        render_traced(trainer, save_dir, args.trace, args.trace_steps, args.normals)
    if args.skip_empty is not None:
        samples, kept = Context.get(grid.device).cull_stats()
        print("skip-empty: rank %d evaluated %d of %d samples (%.2f %%)" % (rank, kept, samples, 100.0 * kept / max(samples, 1)))
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
