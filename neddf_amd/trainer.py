"""Trainer -- host-side mirror of neddf/trainer/{base_trainer,nerf_trainer}.py: construct from the run config,
train (random pixel batches -> render_rays -> losses -> backward -> Adam, exponential LR decay per epoch, periodic
field slices / test renders / checkpoints) and evaluate (render every view, PNGs, PSNR/SSIM).  The per-step device
work -- both field evaluations, both volume integrals and their backward passes -- is HIP kernels (autograd.py);
the optimiser is torch.optim.Adam on the parameter tensors the kernels read in place.
"""
import math
from pathlib import Path
from typing import Any, Dict, List

import numpy as np
import torch

from .camera import Camera, CameraSet, OrthographicCalib, PinholeCalib
from .config import instantiate, to_plain
from .dataset import imwrite_bgr
from .logger import ScalarLog
from .metrics import peak_signal_noise_ratio, structural_similarity
from .parallel import average_gradients, render_image_sharded
from .render import render_from_config


def _get(cfg: Any, key: str) -> Any:
    return cfg[key] if isinstance(cfg, dict) else getattr(cfg, key)


def _has(cfg: Any, key: str) -> bool:
    return key in cfg if isinstance(cfg, dict) else hasattr(cfg, key)


class BaseTrainer:
    """base_trainer.py:50-113 constructor keywords."""

    def __init__(self, global_config: Any, device: str = "cuda:0", batch_size: int = 1024, chunk: int = 1024,
                 epoch_max: int = 2000, epoch_save_fields: int = 2, epoch_test_rendering: int = 10,
                 epoch_save_model: int = 100, scheduler_lr: float = 0.99815, optimizer_lr: float = 0.0005,
                 optimizer_weight_decay: float = 0.0) -> None:
        self.config = global_config
        self.device = torch.device(device)
        self.batch_size, self.chunk = batch_size, chunk
        self.epoch_max, self.epoch_save_fields = epoch_max, epoch_save_fields
        self.epoch_test_rendering, self.epoch_save_model = epoch_test_rendering, epoch_save_model
        self.scheduler_lr, self.optimizer_lr, self.optimizer_weight_decay = scheduler_lr, optimizer_lr, optimizer_weight_decay
        self.writes_outputs = True      # multi-rank runs: rank 0 only (scripts/run.py, scripts/run_eval.py set it)
        self.dataset = instantiate(_get(self.config, "dataset"))
        self.camera_calib = PinholeCalib(self.dataset[0]["camera_calib_params"]).to(self.device)
        self.cameras: List[Camera] = [Camera(self.camera_calib, self.dataset[i]["camera_params"]).to(self.device)
                                      for i in range(len(self.dataset))]
        loss_cfg = _get(self.config, "loss") if _has(self.config, "loss") else {"functions": []}
        self.loss_functions = [instantiate(f).to(self.device) for f in _get(loss_cfg, "functions")]     # base_trainer.py:110-113
        self._gt_stacks: Dict[str, Any] = {}    # construct_ground_truth_mixed's device images, built on first use
        self._view_sizes = None                 # draw_mixed_batch's per-view (w - 1, h - 1)
        self._camera_set = None                 # run_train_step_mixed's camera table (CameraSet), built on first use

    def use_orthographic_cameras(self, scale: float) -> None:
        """Replaces every view's camera by an orthographic one at the same pose (not in the reference): `scale` pixels per world
        unit, the principal point at the image centre -- the inspection views of render_mesh.py --ortho and run_eval.py --ortho."""
        h, w = self.dataset[0]["rgb_images"].shape[:2]
        self.camera_calib = OrthographicCalib(np.array([scale, scale, 0.5 * w, 0.5 * h], dtype=np.float32)).to(self.device)
        self.cameras = [Camera(self.camera_calib, self.dataset[i]["camera_params"]).to(self.device) for i in range(len(self.dataset))]

    def load_pretrained_model(self, model_path: Path) -> None:
        """base_trainer.py:115-121"""
        self.neural_render.load_state_dict(torch.load(str(model_path), map_location="cpu"))

    def render_test(self, output_dir: Path, camera_id: int, downsampling: int = 1, sharded: Any = None, normals: bool = False) -> None:
        """base_trainer.py:123-174: colour -> clamp(c*255) uint8, depth -> clamp((d-2)/4*50000/256) uint8,
        PNGs {id:03}_rgb / _rgb_gt / _depth, PSNR + SSIM vs the ground truth at full resolution.
        sharded (not a reference keyword): None = ray-shard the frame over the ranks whenever a process group is up (a
        COLLECTIVE: every rank must call, with the same torch seed -- run_eval.py / render_all); False = render on this rank
        alone (the periodic test render of a data-parallel training run, which only rank 0 makes).
        normals (not a reference keyword): also render the "normal" target and write {id:03}_normal.png =
        clamp((n * 0.5 + 0.5) * 255), world x, y, z as R, G, B; single-device renders only."""
        rgb_gt = self.dataset[camera_id]["rgb_images"].astype(np.uint8)
        targets = ["color", "depth"] + (["normal"] if normals else [])
        camera = self.cameras[camera_id]
        camera.update_transform()
        h, w = rgb_gt.shape[0], rgb_gt.shape[1]
        if sharded is None:
            sharded = torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1
        if sharded:
            # under a launcher (scripts/run_eval.py, BASELINE.json configs[3]): every rank renders a slab of the frame's pixel
            # index, one all-gather of the pixels, rank 0 writes the files.  Same seed on every rank => the single-GPU image
            images = render_image_sharded(self.neural_render, w, h, camera, targets, downsampling, self.chunk)
            if not self.writes_outputs:
                return
        else:
            images = self.neural_render.render_image(w, h, camera, targets, downsampling, self.chunk)
        rgb_np = torch.clamp(images["color"] * 255, 0, 255).detach().cpu().numpy().astype(np.uint8)
        depth_np = torch.clamp((images["depth"] - 2.0) / 4.0 * 50000 / 256, 0, 255).detach().cpu().numpy().astype(np.uint8)
        output_dir = Path(output_dir)
        imwrite_bgr(output_dir / "{:03}_rgb.png".format(camera_id), rgb_np)
        imwrite_bgr(output_dir / "{:03}_rgb_gt.png".format(camera_id), rgb_gt)
        imwrite_bgr(output_dir / "{:03}_depth.png".format(camera_id), depth_np)
        if normals:         # imwrite_bgr takes B, G, R: x, y, z -> R, G, B
            normal_np = torch.clamp((images["normal"] * 0.5 + 0.5) * 255, 0, 255).detach().cpu().numpy().astype(np.uint8)
            imwrite_bgr(output_dir / "{:03}_normal.png".format(camera_id), np.ascontiguousarray(normal_np[:, :, ::-1]))
        if downsampling == 1:
            psnr = peak_signal_noise_ratio(rgb_np, rgb_gt)
            ssim = structural_similarity(rgb_np, rgb_gt, channel_axis=2)
            print("psnr: {}, ssim: {}".format(psnr, ssim))
            self.last_metrics = (psnr, ssim)

    def render_all(self, output_dir: Path, normals: bool = False) -> None:
        """base_trainer.py:176-188; normals: as render_test"""
        self.neural_render.set_iter(-1)
        for camera_id in range(len(self.dataset)):
            if self.writes_outputs:
                print("rendering from camera {}".format(camera_id))
            self.render_test(output_dir, camera_id, 1, normals=normals)
        if self.writes_outputs and len(self.dataset):
            # (one line after the reference's own printout, not inside it: the "psnr: .., ssim: .." lines keep the reference's format)
            print("note: PSNR is pinned on the reference's eval harness (tests/golden/eval_harness.npz); SSIM is restated from the published "
                  "algorithm with skimage's defaults and UNPINNED (skimage is not installed here)")

    def render_field_slices(self, output_field_dir: Path, epoch: int = 0) -> None:
        """base_trainer.py:190-204"""
        images = self.neural_render.render_field_slice()
        for key in images:
            imwrite_bgr(Path(output_field_dir) / "field_{}_{:04}.png".format(key, epoch), images[key])

    def construct_ground_truth(self, camera_id: int, us_int: torch.Tensor, vs_int: torch.Tensor,
                               loss_types: List[str]) -> Dict[str, torch.Tensor]:
        """base_trainer.py:206-246: targets of the selected pixels (rgb / 256, mask / 256, zero penalty)."""
        targets: Dict[str, torch.Tensor] = {}
        us, vs = us_int.cpu().numpy().astype(np.int64), vs_int.cpu().numpy().astype(np.int64)
        if "ColorLoss" in loss_types:
            rgb = self.dataset[camera_id]["rgb_images"]
            targets["color"] = torch.from_numpy(((1.0 / 256) * rgb[vs, us, :]).astype(np.float32)).to(self.device)
        if "MaskBCELoss" in loss_types or "MaskMSELoss" in loss_types:
            mask = self.dataset[camera_id]["mask_images"]
            targets["mask"] = torch.from_numpy(((1.0 / 256) * mask[vs, us]).astype(np.float32)).to(self.device)
        if "FieldsConstraintLoss" in loss_types:
            targets["fields_penalty"] = torch.zeros(us_int.shape, dtype=torch.float32)
        return targets

    def construct_ground_truth_mixed(self, view: torch.Tensor, us_int: torch.Tensor, vs_int: torch.Tensor,
                                     loss_types: List[str]) -> Dict[str, torch.Tensor]:
        """construct_ground_truth for a batch that mixes views: row b is pixel (us_int[b], vs_int[b]) of view[b], and holds the
        bits construct_ground_truth(view[b], ...) gives for that pixel.  When every view has one image size the images are stacked
        on the device once ([V,h,w,3]; masks [V,h,w]) and a step is one gather there -- x * 2^-8 is exact in fp32, so the device's
        product is the host's; otherwise the rows are gathered per view on the host with the method above."""
        view = torch.as_tensor(view).to(torch.int64)
        want_color = "ColorLoss" in loss_types
        want_mask = "MaskBCELoss" in loss_types or "MaskMSELoss" in loss_types
        targets: Dict[str, torch.Tensor] = {}
        stacks = self._ground_truth_stacks(want_color, want_mask)
        if stacks is not None:
            v, us, vs = view.to(self.device), us_int.to(self.device).to(torch.int64), vs_int.to(self.device).to(torch.int64)
            if want_color:
                targets["color"] = stacks["color"][v, vs, us].to(torch.float32) * (1.0 / 256)
            if want_mask:
                targets["mask"] = stacks["mask"][v, vs, us].to(torch.float32) * (1.0 / 256)
        else:
            view_host = view.cpu()
            if want_color:
                targets["color"] = torch.empty(view.shape[0], 3, dtype=torch.float32, device=self.device)
            if want_mask:
                targets["mask"] = torch.empty(view.shape[0], dtype=torch.float32, device=self.device)
            for camera_id in torch.unique(view_host).tolist():
                rows = (view_host == camera_id).nonzero().squeeze(1)
                part = self.construct_ground_truth(int(camera_id), us_int.cpu()[rows], vs_int.cpu()[rows],
                                                   [t for t in loss_types if t != "FieldsConstraintLoss"])
                for key in part:
                    targets[key][rows.to(self.device)] = part[key]
        if "FieldsConstraintLoss" in loss_types:
            targets["fields_penalty"] = torch.zeros(us_int.shape, dtype=torch.float32)
        return targets

    def _ground_truth_stacks(self, want_color: bool, want_mask: bool):
        """The device-resident image stacks of construct_ground_truth_mixed, built on first use and kept in the images' own type
        (uint8, or the float32 of alpha-premultiplied colours: either way the fp32 product with 2^-8 is the host's value); None
        when the views differ in size or hold another type (the host route then reads the images as they are)."""
        cache = self._gt_stacks
        for key, field, want in (("color", "rgb_images", want_color), ("mask", "mask_images", want_mask)):
            if not want or key in cache:
                continue
            images = [np.asarray(self.dataset[i][field]) for i in range(len(self.dataset))]
            fits = all(im.shape == images[0].shape and im.dtype == images[0].dtype for im in images) and images[0].dtype in (np.uint8, np.float32)
            cache[key] = torch.from_numpy(np.stack(images)).to(self.device) if fits else None
        if (want_color and cache["color"] is None) or (want_mask and cache["mask"] is None):
            return None
        return cache

    def run_train(self) -> None:
        raise NotImplementedError()

    def run_train_step(self, camera_id: int) -> float:
        raise NotImplementedError()


class NeRFTrainer(BaseTrainer):
    """nerf_trainer.py:23-140.  Two keywords the reference does not have: optimize_cameras (default False) puts every view's
    Camera.params -- the SE(3) perturbation of its dataset pose -- into Adam as a second parameter group and switches the
    render's pose_gradients on; camera_lr is that group's learning rate.  The reference leaves the pose parameters out of its
    optimiser, so it has no value to follow: 1e-3 is the step of published joint pose / field optimisation (BARF, Lin et al.
    2021, train their poses at 1e-3), twice the field's 5e-4 here, and decays with the same scheduler.
    A third: batch_views.  "single" (default, the reference): a step draws all its rays from one view, an epoch visits the views in
    a random permutation.  "mixed": every ray of a step draws its own view (run_train_step_mixed), an epoch is still len(dataset)
    steps; with optimize_cameras every view a step visits receives a pose gradient."""

    def __init__(self, optimize_cameras: bool = False, camera_lr: float = 1e-3, batch_views: str = "single", **kwargs: Any) -> None:
        if batch_views not in ("single", "mixed"):
            raise ValueError("batch_views must be 'single' or 'mixed' (got %r)" % (batch_views,))
        super().__init__(**kwargs)
        self.batch_views = batch_views
        self.optimize_cameras, self.camera_lr = bool(optimize_cameras), float(camera_lr)
        self.neural_render = render_from_config(to_plain(_get(self.config, "render")), network_config=to_plain(_get(self.config, "network")),
                                                _recursive_=False).to(self.device)
        if getattr(self.neural_render, "ray_space", "world") == "ndc":      # forward-facing data: NDC of the full image
            self.neural_render.ndc_width, self.neural_render.ndc_height = self.dataset.image_width, self.dataset.image_height
        self.optimizer = torch.optim.Adam(self.neural_render.get_parameters_list(), lr=self.optimizer_lr,
                                          weight_decay=self.optimizer_weight_decay)
        if self.optimize_cameras:
            self.neural_render.pose_gradients = True
            self.optimizer.add_param_group({"params": self.camera_parameters(), "lr": self.camera_lr, "weight_decay": 0.0})
        self.scheduler = torch.optim.lr_scheduler.ExponentialLR(self.optimizer, gamma=self.scheduler_lr)
        self.logger = None      # created by the first training step: evaluation runs leave no ./log behind

    def camera_parameters(self) -> List[torch.nn.Parameter]:
        return [c.params for c in self.cameras]

    def run_train(self) -> None:
        """nerf_trainer.py:47-79: epochs over a random permutation of the frames, outputs under the working directory
        (models/, render/)."""
        if self.writes_outputs:
            Path("models").mkdir(parents=True)
        render_dir = Path("render")
        frame_length = len(self.dataset)
        self.neural_render.set_iter(0)
        for epoch in range(0, self.epoch_max + 1):
            print("epoch: ", epoch)
            camera_ids = np.random.permutation(frame_length)
            for camera_id in camera_ids:
                if self.batch_views == "mixed":     # (the permutation is drawn either way; its first view is the test render's)
                    self.run_train_step_mixed()
                else:
                    self.run_train_step(int(camera_id))
                self.neural_render.next_iter()
            self.scheduler.step()
            if not self.writes_outputs:
                continue
            if epoch % self.epoch_save_fields == 0:
                output_field_dir = render_dir / "fields"
                output_field_dir.mkdir(parents=True, exist_ok=True)
                self.render_field_slices(output_field_dir, epoch)
            if epoch % self.epoch_test_rendering == 0:
                print("test rendering...")
                output_dir = render_dir / "{:04}".format(epoch)
                output_dir.mkdir(parents=True)
                # rank 0 alone: the other ranks are already in the next epoch's gradient all-reduce, and their generators
                # hold other seeds -- a sharded (collective) render here would mismatch collectives and deadlock
                self.render_test(output_dir, int(camera_ids[0]), downsampling=3, sharded=False)
            if epoch % self.epoch_save_model == 0:
                torch.save(self.neural_render.state_dict(), "models/model_{:0=5}.pth".format(epoch))

    def run_train_step(self, camera_id: int) -> float:
        """nerf_trainer.py:81-140; RNG draw order: u pixels, v pixels, then render_rays' own draws."""
        if self.logger is None:
            self.logger = ScalarLog() if self.writes_outputs else ScalarLog(sink="null")
        camera = self.cameras[camera_id]
        camera.update_transform()
        h, w = self.dataset[camera_id]["rgb_images"].shape[:2]
        with self.logger.step() as rec:
            self.optimizer.zero_grad()
            us_int = (torch.rand(self.batch_size) * (w - 1)).to(torch.int16).to(self.device)
            vs_int = (torch.rand(self.batch_size) * (h - 1)).to(torch.int16).to(self.device)
            names = [type(f).__name__ for f in self.loss_functions]
            targets = self.construct_ground_truth(camera_id, us_int, vs_int, names)
            with torch.enable_grad():
                rendered = self.neural_render.render_rays(torch.stack([us_int, vs_int], 1), camera)
                loss_value = self._finish_step(rec, rendered, targets)
        return loss_value

    def draw_mixed_batch(self):
        """The pixel draws of a mixed-view step, on the CPU generator and in this order -- the contract of batch_views="mixed":

            view = (torch.rand(B) * n_views).to(torch.int64)            each ray's view
            us   = (torch.rand(B) * (w[view] - 1)).to(torch.int16)      then its column, scaled by ITS view's width
            vs   = (torch.rand(B) * (h[view] - 1)).to(torch.int16)      then its row, by its view's height

        (host tensors; render_rays_mixed's own draws follow).  The scale factors are fp32, as the single-view step's are."""
        sizes = self._view_sizes
        if sizes is None:
            hw = [self.dataset[i]["rgb_images"].shape[:2] for i in range(len(self.dataset))]
            sizes = self._view_sizes = (torch.tensor([s[1] - 1 for s in hw], dtype=torch.float32),
                                        torch.tensor([s[0] - 1 for s in hw], dtype=torch.float32))
        view = (torch.rand(self.batch_size) * len(self.dataset)).to(torch.int64)
        us_int = (torch.rand(self.batch_size) * sizes[0][view]).to(torch.int16)
        vs_int = (torch.rand(self.batch_size) * sizes[1][view]).to(torch.int16)
        return view, us_int, vs_int

    def camera_set(self):
        """The CameraSet of `cameras` (built once per camera list), or None where a camera is not a pinhole."""
        held = self._camera_set
        if held is None or held[0] is not self.cameras:
            pinholes = all(isinstance(c.camera_calib, PinholeCalib) for c in self.cameras)
            held = self._camera_set = (self.cameras, CameraSet(self.cameras) if pinholes else None)
        return held[1]

    def run_train_step_mixed(self) -> float:
        """run_train_step on rays drawn across all views (not a reference method).  RNG draw order: draw_mixed_batch's three
        draws (view, u, v), then the renderer's own (render_rays' [B,Sc+1] and [B,Sf+1]).  The cameras reach ray generation as a
        device-resident table (CameraSet, NeRFRender.render_rays_views): no work per view on the host, one ray-generation launch.
        Without optimize_cameras that is the cached table of all views.  With it the table is composed, with its graph, from the
        parameters of the views the HOST draw visits: every view the step visits receives a pose gradient from one backward
        launch; a view it does not visit has none (single rank) or is reset by the all-zero rule of _finish_step (several ranks).
        Cameras that are not pinholes keep the per-camera route (render_rays_mixed)."""
        if self.logger is None:
            self.logger = ScalarLog() if self.writes_outputs else ScalarLog(sink="null")
        cams = self.camera_set()
        if cams is None:
            for camera in self.cameras:
                camera.update_transform()
        with self.logger.step() as rec:
            self.optimizer.zero_grad()
            view, us_int, vs_int = self.draw_mixed_batch()
            names = [type(f).__name__ for f in self.loss_functions]
            targets = self.construct_ground_truth_mixed(view, us_int, vs_int, names)
            with torch.enable_grad():
                uv = torch.stack([us_int, vs_int], 1).to(self.device)
                if cams is None:
                    rendered = self.neural_render.render_rays_mixed(uv, view.to(self.device), self.cameras)
                elif self.optimize_cameras:
                    visited, local = cams.select(view)      # (validated and renumbered on the host: the draw never left it)
                    rendered = self.neural_render.render_rays_views(uv, local.to(self.device), cams.table(visited, grad=True))
                else:
                    cams.check_view(view)
                    rendered = self.neural_render.render_rays_views(uv, view.to(self.device), cams.table())
                loss_value = self._finish_step(rec, rendered, targets)
        return loss_value

    def _finish_step(self, rec, rendered: Dict[str, torch.Tensor], targets: Dict[str, torch.Tensor]) -> float:
        """Losses, backward, the gradient all-reduce, the optimiser step and the log record of one training step (under
        enable_grad, inside the logger's step)."""
        terms: Dict[str, torch.Tensor] = {}
        for f in self.loss_functions:
            terms.update(f(rendered, targets))
        total = torch.stack(list(terms.values())).sum()
        total.backward()
        with torch.no_grad():
            # data-parallel runs (scripts/run.py under torchrun: per-rank seed and device): one all-reduce of the gradients
            average_gradients(self.neural_render.get_parameters_list())
            if self.optimize_cameras:       # (every rank passes the same list; the ranks visit different views per step)
                average_gradients(self.camera_parameters())
                # the all-reduce hands every camera a gradient tensor, zeros for the views no rank visited; Adam would then step
                # those too (a view visited once would keep drifting on its decaying first moment).  As in a single-rank run a
                # view nobody visited has no gradient: same decision on every rank, since the averaged values are the same
                held = [p for p in self.camera_parameters() if p.grad is not None]
                if held:        # one device -> host read for all cameras
                    for p, moved in zip(held, torch.stack([p.grad for p in held]).ne(0).any(dim=1).tolist()):
                        if not moved:
                            p.grad = None
            self.optimizer.step()
            mse = float(torch.mean(torch.square(rendered["color"].detach() - targets["color"])).item())
            loss_value = float(total.item())
            rec.report(loss_value, 10 * math.log10(1.0 / mse), terms)
        return loss_value
