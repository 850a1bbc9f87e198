"""`python neddf/scripts/refine_pose.py <run_dir> --epoch N --view K [--perturb rx ry rz tx ty tz] [--steps S] [--batch B] [--lr LR]
[--seed SEED]` -- register one view against a trained field: the field stays as trained, only the view's `camera.params` (the SE(3)
perturbation of its dataset pose, camera.py:66-118) is optimised with Adam against the view's image, through the pose gradient of
render_rays (`render.pose_gradients`).  `--perturb` starts from a displaced pose.  The run is loaded as run_eval loads it.  Prints
loss and pose error against the dataset pose (rotation angle in radians, translation norm) per step and writes the refined 4x4
camera-to-world matrix to `<run_dir>/poses/view_{K:03}.json`.  The reference has no such script; the learning rate default is the
trainer's camera_lr."""
import json
import math
from argparse import ArgumentParser
from pathlib import Path

import numpy as np
import torch

from neddf_amd.scripts.run_eval import load_config, load_trainer


def build_parser() -> ArgumentParser:
    parser = ArgumentParser()
    parser.add_argument("output_dir", type=Path, help="directory path where models are located")
    parser.add_argument("--epoch", type=int, default=2000, help="epoch number of model")
    parser.add_argument("--view", type=int, default=0, help="index of the view in the test split")
    parser.add_argument("--perturb", type=float, nargs=6, default=[0.0] * 6, metavar=("rx", "ry", "rz", "tx", "ty", "tz"),
                        help="initial camera.params: rotation vector and translation applied on top of the dataset pose")
    parser.add_argument("--steps", type=int, default=200)
    parser.add_argument("--batch", type=int, default=1024, help="random pixels per step")
    parser.add_argument("--lr", type=float, default=1e-3)
    parser.add_argument("--seed", type=int, default=None, help="torch seed for the pixel and sample draws")
    return parser


def pose_error(camera, R_ref: torch.Tensor, T_ref: torch.Tensor):
    """(rotation angle between R and R_ref in radians, |T - T_ref|)"""
    rel = torch.matmul(camera.R.detach(), R_ref.T)
    cos = float(((torch.trace(rel) - 1.0) * 0.5).clamp(-1.0, 1.0))
    return math.acos(cos), float(torch.norm(camera.T.detach() - T_ref))


def main(argv=None) -> Path:
    args = build_parser().parse_args(argv)
    output_dir = args.output_dir.resolve()
    if args.seed is not None:
        torch.manual_seed(args.seed)
    trainer = load_trainer(load_config(output_dir), output_dir, args.epoch)
    render = trainer.neural_render
    render.set_iter(-1)                     # the evaluation state of the field
    render.pose_gradients = True
    camera = trainer.cameras[args.view]
    camera.update_transform()
    R_ref, T_ref = camera.R.detach().clone(), camera.T.detach().clone()
    with torch.no_grad():
        camera.params.copy_(torch.tensor(args.perturb, dtype=torch.float32, device=camera.device))
    optimizer = torch.optim.Adam([camera.params], lr=args.lr)      # the field's parameters are in no optimiser: it stays as trained
    h, w = trainer.dataset[args.view]["rgb_images"].shape[:2]
    names = [type(f).__name__ for f in trainer.loss_functions]
    history = []
    for step in range(args.steps):
        camera.update_transform()
        optimizer.zero_grad()
        render.zero_grad()
        us = (torch.rand(args.batch) * (w - 1)).to(torch.int16).to(trainer.device)
        vs = (torch.rand(args.batch) * (h - 1)).to(torch.int16).to(trainer.device)
        targets = trainer.construct_ground_truth(args.view, us, vs, names)
        with torch.enable_grad():
            rendered = render.render_rays(torch.stack([us, vs], 1), camera)
            terms = {}
            for f in trainer.loss_functions:
                terms.update(f(rendered, targets))
            loss = torch.stack(list(terms.values())).sum()
            loss.backward()
        optimizer.step()
        camera.update_transform()
        rot, trans = pose_error(camera, R_ref, T_ref)
        history.append((float(loss.item()), rot, trans))
        print("step %d: loss %.6f, rotation error %.6f rad, translation error %.6f" % (step, history[-1][0], rot, trans))
    camera.update_transform()
    pose = np.eye(4)
    pose[:3, :3] = camera.R.detach().cpu().numpy()
    pose[:3, 3] = camera.T.detach().cpu().numpy()
    save_dir = output_dir / "poses"
    save_dir.mkdir(exist_ok=True)
    path = save_dir / "view_{:03}.json".format(args.view)
    rot, trans = pose_error(camera, R_ref, T_ref)
    json.dump({"view": args.view, "transform_matrix": pose.tolist(), "params": camera.params.detach().cpu().tolist(),
               "rotation_error": rot, "translation_error": trans, "steps": args.steps, "batch": args.batch, "lr": args.lr},
              open(path, "w"), indent=1)
    print("wrote %s" % path)
    return path


if __name__ == "__main__":
    main()
