"""Volume renderer -- host-side mirror of neddf/render/{base_neural_render,nerf_render}.py.

Same constructor keywords, methods, dict keys and RNG draw order as the
reference; the work is the fused HIP pipeline behind neddf_render_rays
(raygen -> stratified/cone sampling -> field -> wave-scan compositing ->
inverse-CDF resampling -> field -> compositing) on the current HIP stream.
"""
import math
from typing import Any, Dict, Iterable, List, Optional

import os

import torch
from torch import Tensor, nn

from ._lib import SLOT_COARSE, SLOT_FINE, Context, NeddfError, RenderParams, ViewRays
from .camera import Camera, PinholeCalib
from .config import instantiate
from .network import BaseNeuralField, NeDDF
from .ray import Ray
from .rng import skip_uniforms

RenderTarget = str          # Literal["color", "depth", "transmittance", "normal"]
SamplingType = str          # Literal["point", "cone"]


class BaseNeuralRender(nn.Module):
    def __init__(self) -> None:
        super().__init__()
        self.iteration: int = -1

    def next_iter(self) -> None:
        self.set_iter(self.iteration + 1)

    def set_iter(self, iter: int) -> None:
        self.iteration = iter


def render_from_config(render_config: Any, **kwargs: Any) -> "NeRFRender":
    """instantiate() a render configuration; the key `pose_gradients` (not a reference keyword) becomes the attribute."""
    cfg = dict(render_config)
    pose = bool(cfg.pop("pose_gradients", False))
    render = instantiate(cfg, **kwargs)
    render.pose_gradients = pose
    return render


def _is_pinhole(camera: Any) -> bool:
    """Whether `camera` goes through the raygen kernel by its descriptor(): a Camera with a PinholeCalib, or any object that only
    offers a descriptor.  A Camera with another calib makes its rays in create_rays."""
    calib = getattr(camera, "camera_calib", None)
    return calib is None or isinstance(calib, PinholeCalib)


class NeRFRender(BaseNeuralRender):
    """nerf_render.py:40-81.  Extra (non-reference) attributes:

    rng            "torch_cpu" (default; the reference draws its uniforms with
                   torch.rand on the CPU generator, nerf_render.py:137 and
                   base_neural_render.py:75 -- same seed => same samples) or
                   "device" (draw on the HIP device; faster, not seed-compatible)
    rays_per_call  rays handed to one neddf_render_rays call by render_image
    ray_space      "world" (the reference) or "ndc": forward-facing captures sampled along normalised-device-coordinate
                   rays of an ndc_width x ndc_height view with near plane ndc_near (original NeRF paper, appendix C;
                   the reference has no such mode).  dist_near / dist_far are then NDC depths (0 and 1) and the fields
                   still receive the world-space viewing direction.  Use sampling_type="point" with it.
    pose_gradients (attribute, set after construction or through `render.pose_gradients` of a run configuration -- see
                   render_from_config; the constructor keeps the reference's keywords)
                   False (default): render_rays under autograd differentiates the network parameters only; True: ray
                   generation and the samplers join the graph as in the reference (camera.py:155-171, ray.py:88-194 are
                   differentiable torch there), so loss.backward() fills camera.params.grad.  NeDDF and NeRF fields with fp32
                   operands and world-space rays; NeuS, NDC rays and split-fp16 operands raise.  The intrinsics get no gradient.
    normal_output  (attribute) False (default): render_rays returns the reference's keys.  True: its inference path appends `normal`
                   and `normal_coarse` [B,3] = sum_j weight[b,j] * normal[b,j], the field's per-sample normal (the value its colour trunk
                   receives: BaseNeuralField.forward_surface) integrated over the intervals and with the weights of `color`
                   (base_neural_render.py:154-160).  Not normalised: the length is at most 1 - transmittance for NeDDF's unit
                   normals, the background is the zero vector.  NeDDF and NeuS fields; NeRF fields raise.  The autograd path
                   (training) ignores it.  render_image takes the same quantity as the target type "normal",
                   render_image_single_pass as normals=True.
    occupancy      (attribute) None (default): every sample of every ray goes through the field.  An OccupancyGrid
                   (occupancy.py; build_occupancy makes one from the networks): render_image and render_image_single_pass skip
                   empty space -- every pass classifies its sample positions against the grid, evaluates the field on the kept ones
                   only and gives the others density 0, colour 0 and normal 0; samples outside the grid's box are evaluated as
                   before.  One stream synchronise per pass.  render_rays, the autograd paths and render_field_slice never use it.
                   World-space rays only (ray_space="ndc" raises); the grid must live on the camera's device.
    """

    pose_gradients = False
    normal_output = False
    occupancy = None

    def __init__(self, network_config: Any, sample_coarse: int = 128, sample_fine: int = 128, dist_near: float = 2.0,
                 dist_far: float = 6.0, max_dist: float = 6.0, use_coarse_network: bool = True,
                 sampling_type: SamplingType = "point", ray_space: str = "world", ndc_near: float = 1.0) -> None:
        super().__init__()
        self.use_coarse_network = use_coarse_network
        self.network_fine: BaseNeuralField = instantiate(network_config)
        self.network_coarse: BaseNeuralField = instantiate(network_config) if use_coarse_network else self.network_fine
        # library slots the modules work in when called directly (training step, stage API); render_rays' fused path
        # loads SLOT_COARSE / SLOT_FINE itself
        self.network_fine._slot = SLOT_FINE
        if use_coarse_network:
            self.network_coarse._slot = SLOT_COARSE
        self.sample_coarse, self.sample_fine = sample_coarse, sample_fine
        self.dist_near, self.dist_far, self.max_dist = dist_near, dist_far, max_dist
        self.sampling_type = sampling_type
        self.rng = "torch_cpu"
        self.rays_per_call = int(os.environ.get("NEDDF_RAYS_PER_CALL", 1 << 16))
        self.ray_space = ray_space          # the two keywords after sampling_type are not reference keywords
        self.ndc_width, self.ndc_height, self.ndc_near = 0, 0, ndc_near

    # ------------------------------------------------------------------ helpers
    def get_network(self) -> BaseNeuralField:
        return self.network_fine

    def get_parameters_list(self) -> List[Any]:
        if self.use_coarse_network:
            return list(self.network_coarse.parameters()) + list(self.network_fine.parameters())
        return list(self.network_coarse.parameters())

    def set_iter(self, iter: int) -> None:
        super().set_iter(iter)
        self.network_coarse.set_iter(iter)
        self.network_fine.set_iter(iter)

    def _params(self, nan_group: int = 0, nan_group_offset: int = 0) -> RenderParams:
        if self.sampling_type not in ("point", "cone"):
            raise ValueError("sampling_type must be 'point' or 'cone'")
        p = RenderParams()
        p.sample_coarse, p.sample_fine = self.sample_coarse, self.sample_fine
        p.dist_near, p.dist_far, p.max_dist = self.dist_near, self.dist_far, self.max_dist
        p.cone_sampling = int(self.sampling_type == "cone")
        # rays per sample_pdf NaN-fallback decision (render_image: its chunk) and where in a group this batch starts
        p.nan_group, p.nan_group_offset = int(nan_group), int(nan_group_offset)
        p.ray_radius = 1.0 / 1111 / math.sqrt(12)      # nerf_render.py:144-145
        if self.ray_space not in ("world", "ndc"):
            raise ValueError("ray_space must be 'world' or 'ndc'")
        p.ndc_rays = int(self.ray_space == "ndc")
        if p.ndc_rays:
            if self.ndc_width < 1 or self.ndc_height < 1:
                raise ValueError("ray_space='ndc' needs ndc_width / ndc_height (the full image size)")
            p.ndc_width, p.ndc_height, p.ndc_near = int(self.ndc_width), int(self.ndc_height), float(self.ndc_near)
        return p

    def _ctx(self, device) -> Context:
        ctx = Context.get(device)
        self.network_coarse.upload(ctx, SLOT_COARSE)
        self.network_fine.upload(ctx, SLOT_FINE)
        return ctx

    def _rand(self, rows: int, cols: int, device) -> Tensor:
        if self.rng == "torch_cpu":     # page-locked, so the upload overlaps the draw of the next batch
            return torch.rand(rows, cols, pin_memory=torch.device(device).type == "cuda").to(device, non_blocking=True)
        if self.rng == "device":
            return torch.rand(rows, cols, device=device)
        raise ValueError("rng must be 'torch_cpu' or 'device'")

    def _draw_pair(self, B: int, device):
        """The uniforms of one hierarchical batch, U_c [B,Sc+1] then U_f [B,Sf+1]: draw order is part of the contract."""
        return self._rand(B, self.sample_coarse + 1, device), self._rand(B, self.sample_fine + 1, device)

    @staticmethod
    def _pixel_grid(width: int, height: int, downsampling: int, device, pixel_range=None):
        """(uv, w, h): every `downsampling`-th pixel as int64 rows (u, v), row-major (idx = v*w + u); pixel_range=(lo, hi): that slab."""
        w, h = width // downsampling, height // downsampling
        us = torch.arange(w, device=device).reshape(1, w).expand(h, w).reshape(-1) * downsampling
        vs = torch.arange(h, device=device).reshape(h, 1).expand(h, w).reshape(-1) * downsampling
        lo, hi = (0, w * h) if pixel_range is None else pixel_range
        return torch.stack([us, vs], 1)[lo:hi], w, h

    @staticmethod
    def _hit_targets(hit: Tensor, t: Tensor, target_types: List[RenderTarget]) -> Dict[str, Tensor]:
        """The targets a hit mask decides (traced and mesh views): depth = t on HIT pixels, 0 elsewhere; transmittance 0 / 1."""
        make = dict(depth=lambda: torch.where(hit, t, torch.zeros_like(t)),
                    transmittance=lambda: torch.where(hit, torch.zeros_like(t), torch.ones_like(t)))
        return {k: f() for k, f in make.items() if k in target_types}

    @staticmethod
    def _as_images(out: Dict[str, Tensor], target_types: List[RenderTarget], w: int, h: int, pixel_range) -> Dict[str, Tensor]:
        """Flat per-pixel tensors -> [h, w, 3] / [h, w] images (a slab stays flat), in the order of target_types."""
        if pixel_range is None:
            out = {k: v.reshape(h, w, 3) if v.dim() == 2 else v.reshape(h, w) for k, v in out.items()}
        return {k: out[k] for k in target_types}

    def _has_penalty(self) -> bool:
        return isinstance(self.network_fine, NeDDF)

    # --------------------------------------------------------------- stage API
    def integrate_volume_render(self, dists: Tensor, densities: Tensor, colors: Tensor) -> Dict[str, Tensor]:
        """base_neural_render.py:117-172: weight [B,S-1], depth [B], color [B,3], transmittance [B]."""
        ctx = Context.get(dists.device)
        if torch.is_grad_enabled() and (densities.requires_grad or colors.requires_grad):
            from .autograd import CompositeFunction
            w, depth, color, trans, flag = CompositeFunction.apply(ctx, self.max_dist, dists.detach(), densities, colors)
            out = dict(weight=w, depth=depth, color=color, transmittance=trans)
        else:
            out, flag = ctx.composite(dists, densities, colors, self.max_dist)
        assert int(flag.item()) == 0, "NaN weight in integrate_volume_render"      # reference asserts (:155)
        return out

    def sample_pdf(self, dists: Tensor, weights: Tensor, samples_fine: int, cat_coarse: bool = True) -> Tensor:
        """base_neural_render.py:27-115.  `weights` is sanitised in place like the reference."""
        ctx = Context.get(dists.device)
        U = self._rand(dists.shape[0], samples_fine, dists.device).contiguous()
        if weights.dtype == torch.float32 and weights.is_contiguous():
            return ctx.importance_resample(dists, weights, U, cat_coarse)
        w = weights.to(torch.float32).contiguous()
        out = ctx.importance_resample(dists, w, U, cat_coarse)
        weights.copy_(w)
        return out

    # -------------------------------------------------------------- render_rays
    def _check_normal_fields(self, coarse: bool) -> None:
        for net in ([self.network_coarse] if coarse else []) + [self.network_fine]:
            if not net._has_surface():
                raise NotImplementedError("the normal target needs a field with a distance or sdf trunk (NeDDF, NeuS); %s has none"
                                          % type(net).__name__)

    def build_occupancy(self, **kw: Any):
        """Builds the occupancy grid of network_fine (OccupancyGrid.from_field's keywords: resolution, cube_range, threshold,
        dilate, lo, hi), ORs in the grid of network_coarse when use_coarse_network is set -- a coarse pass never loses what only
        the coarse network sees -- stores it in `occupancy` and returns it."""
        from .occupancy import OccupancyGrid
        if self.ray_space == "ndc":
            raise NotImplementedError("occupancy grids live in world space: ray_space='ndc' is not supported")
        grid = OccupancyGrid.from_field(self.network_fine, **kw)
        if self.use_coarse_network:
            grid.union_(OccupancyGrid.from_field(self.network_coarse, **kw))
        self.occupancy = grid
        return grid

    def _occupancy_desc(self, device):
        """The library descriptor of `occupancy` for a culled image render on `device`, or None without a grid."""
        grid = self.occupancy
        if grid is None:
            return None
        if self.ray_space == "ndc":
            raise NotImplementedError("occupancy grids live in world space: ray_space='ndc' is not supported")
        dev = torch.device(device)
        if grid.device.type != dev.type or (dev.index is not None and grid.device.index != dev.index):
            raise ValueError("the occupancy grid lives on %s, the camera on %s" % (grid.device, dev))
        return grid.descriptor()

    def _render(self, ctx: Context, uv, camera: Optional[Camera], U_c: Tensor, U_f: Tensor, full: bool, cam_desc=None,
                nan_group: int = 0, nan_group_offset: int = 0, normal: bool = False, occupancy=None, bundle: bool = False) -> Dict[str, Tensor]:
        """uv: pixels [B,2] of `camera` (or of the descriptor cam_desc), or a ray bundle -- a Ray, or with bundle=True float32
        [B,6] (direction, origin) rows -- which needs neither."""
        views = isinstance(uv, ViewRays)        # a camera per row: the table travels inside `uv`
        B = len(uv) if isinstance(uv, Ray) else uv.uv.shape[0] if views else uv.shape[0]
        dev = uv.uv.device if views else uv.device
        if cam_desc is None and not bundle and not views and not isinstance(uv, Ray):
            cam_desc = camera.descriptor()
        S2 = self.sample_coarse + self.sample_fine + 2

        def buf(*shape):
            return torch.empty(*shape, device=dev, dtype=torch.float32)

        o = dict(color=buf(B, 3), depth=buf(B), transmittance=buf(B))
        if full:
            o.update(weight=buf(B, S2 - 1), color_coarse=buf(B, 3), depth_coarse=buf(B), transmittance_coarse=buf(B),
                     weight_coarse=buf(B, self.sample_coarse))
            if self._has_penalty():
                o.update(fields_penalty=buf(B), fields_penalty_coarse=buf(B))
        if normal:
            self._check_normal_fields(coarse=full)
            o.update(normal=buf(B, 3))
            if full:
                o.update(normal_coarse=buf(B, 3))
        flag = torch.zeros(1, device=dev, dtype=torch.int32)
        ctx.render_rays(uv, cam_desc, self._params(nan_group, nan_group_offset), U_c, U_f, dict(o, nan_flag=flag),
                        occupancy=occupancy, bundle=bundle)
        o["_nan"] = flag
        return o

    RAY_KEYS = ("weight", "depth", "color", "transmittance", "fields_penalty", "weight_coarse", "depth_coarse",
                "color_coarse", "transmittance_coarse", "fields_penalty_coarse", "normal", "normal_coarse")

    def render_rays(self, uv: Tensor, camera: Camera) -> Dict[str, Tensor]:
        """nerf_render.py:109-188.  Keys: weight, depth, color, transmittance[, fields_penalty] + *_coarse.
        With the attribute normal_output set, the inference path appends normal and normal_coarse [B,3] (see the class
        docstring); the autograd path below ignores the attribute."""
        uv = uv.to(camera.device)
        B = uv.shape[0]
        if not _is_pinhole(camera):       # any other calib makes its rays in torch
            with torch.set_grad_enabled(torch.is_grad_enabled() and bool(self.pose_gradients)):
                rays = camera.create_rays(uv)
            return self.render_bundle(rays)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return self._render_rays_with_grad(uv, camera)
        return self._render_rays_fused(uv, camera, B, uv.device)

    def _render_rays_fused(self, uv, camera: Optional[Camera], B: int, device) -> Dict[str, Tensor]:
        """The inference path of render_rays (uv: pixels of `camera`) and render_bundle (uv: a Ray, no camera): one fused call."""
        ctx = self._ctx(device)
        U_c, U_f = self._draw_pair(B, device)
        o = self._render(ctx, uv, camera, U_c, U_f, full=True, normal=bool(self.normal_output))
        assert int(o.pop("_nan").item()) == 0, "NaN weight in integrate_volume_render"
        return {k: o[k] for k in self.RAY_KEYS if k in o}

    def _render_rays_with_grad(self, uv: Tensor, camera: Camera) -> Dict[str, Tensor]:
        """render_rays as the training step needs it (nerf_render.py:109-188 under autograd): the samplers run as in
        inference, the two field evaluations and the two volume integrals are autograd nodes (autograd.py)."""
        ctx = Context.get(uv.device)
        B = uv.shape[0]
        p = self._params()
        U_c, U_f = self._draw_pair(B, uv.device)
        radius = p.ray_radius if p.cone_sampling else None
        if self.pose_gradients:
            return self._render_rays_with_pose_grad(ctx, uv, camera, p, radius, U_c, U_f)
        with torch.no_grad():
            cam = camera.descriptor()
            rd, ro = ctx.raygen(uv, cam)
            view = None
            if p.ndc_rays:
                view = rd
                rd, ro = ctx.rays_to_ndc(rd, ro, p.ndc_width, p.ndc_height, cam.calib[0], cam.calib[1], p.ndc_near)
        return self._render_generated_rays(ctx, rd, ro, radius, U_c, U_f, view=view)

    def _render_rays_with_pose_grad(self, ctx: Context, uv: Tensor, camera: Camera, p: RenderParams, radius, U_c: Tensor,
                                    U_f: Tensor) -> Dict[str, Tensor]:
        """_render_rays_with_grad with ray generation and both samplers as autograd nodes (autograd.py RayFunction,
        SamplingFunction): the same kernels, draws and outputs, and camera.R / camera.T (differentiable results of
        Camera.update_transform) receive their gradients."""
        from .autograd import RayFunction
        if p.ndc_rays:
            raise NotImplementedError("pose_gradients: NDC rays (ray_space='ndc') are not differentiated")
        self._check_pose_fields()
        # (the intrinsics are not differentiated: PinholeCalib.params reaches the kernels as plain numbers and receives no gradient;
        # NeRFTrainer refuses to put it into the optimiser together with the poses)
        rd, ro = RayFunction.apply(ctx, uv, camera.descriptor(), camera.R, camera.T)
        return self._render_generated_rays(ctx, rd, ro, radius, U_c, U_f, ray_graph=True)

    def _check_pose_fields(self) -> None:
        from .network import NeuS
        if isinstance(self.network_coarse, NeuS) or isinstance(self.network_fine, NeuS):
            raise NotImplementedError("pose_gradients through a NeuS field need a third derivative of the sdf trunk: not implemented")

    def _render_generated_rays(self, ctx: Context, rd: Tensor, ro: Tensor, radius, U_c: Tensor, U_f: Tensor, view: Optional[Tensor] = None,
                               ray_graph: bool = False) -> Dict[str, Tensor]:
        """The training forward from the rays on, shared by the uv routes above and render_bundle: coarse distances, sampling,
        field, volume integral, resampling, and the same again through the fine network.  ray_graph=False: the samplers run as in
        inference (`view`: the world-space viewing direction of NDC rays); True: they are autograd nodes (SamplingFunction), so
        gradients reach whatever rd / ro were computed from."""
        from .autograd import SamplingFunction
        from .ray import Sampling
        B = rd.shape[0]

        def sample(dists: Tensor) -> Sampling:
            if ray_graph:
                return Sampling(*SamplingFunction.apply(ctx, rd, ro, dists, radius))
            with torch.no_grad():
                return Sampling(*ctx.sampling(rd, ro, dists, radius, view))

        def integrate(network: BaseNeuralField, smp: Sampling, dists: Tensor) -> Dict[str, Tensor]:
            val = network(smp)
            integ = self.integrate_volume_render(dists, val["density"], val["color"])
            for key in val:
                if "penalty" in key:
                    delta = dists[:, 1:] - dists[:, :-1]
                    integ[key] = torch.sum(delta * val[key].reshape(B, -1)[:, :-1], dim=1)
            return integ

        with torch.no_grad():
            dists_c = ctx.sample_coarse(U_c, self.dist_near, self.dist_far)
        integ_c = integrate(self.network_coarse, sample(dists_c), dists_c)
        with torch.no_grad():
            # sanitises the coarse weights in place, as the reference does under set_grad_enabled(False)
            dists_f = ctx.importance_resample(dists_c, integ_c["weight"].detach(), U_f, True)
        integ = integrate(self.network_fine, sample(dists_f), dists_f)
        for key in list(integ_c):
            integ["{}_coarse".format(key)] = integ_c[key]
        return integ

    # ------------------------------------------------------------------ bundles
    def render_bundle(self, rays: Ray) -> Dict[str, Tensor]:
        """render_rays on explicit rays (not a reference method): rays.ray_dir / rays.ray_orig [B,3] in world space, unit directions
        by the caller's contract (nothing is normalised), rays.uv unused.  The same keys, the same uniform draw order ([B,Sc+1] then
        [B,Sf+1]) and the same NaN assertion as render_rays; every stage after ray generation is the one render_rays runs, so a
        bundle made from ctx.raygen(uv, camera) gives render_rays(uv, camera)'s bits.  Inference goes to the fused path
        (NEDDF_UV_RAYS; normal_output is honoured).  Under autograd the network parameters receive gradients as in render_rays;
        with pose_gradients set and rays.ray_dir / ray_orig requiring grad the samplers join the graph, and the gradients arrive
        at the tensors the caller built the rays from.  ray_space='ndc' raises: the NDC map needs a camera's focal lengths."""
        if self.ray_space == "ndc":
            raise NotImplementedError("render_bundle: NDC rays (ray_space='ndc') need a camera's focal lengths; a bundle has none")
        rd, ro = rays.ray_dir, rays.ray_orig
        if rd.dim() != 2 or rd.shape[1] != 3 or ro.shape != rd.shape:
            raise ValueError("render_bundle: ray_dir and ray_orig must be [B, 3] (got %s and %s)" % (tuple(rd.shape), tuple(ro.shape)))
        B, dev = rd.shape[0], rd.device
        if torch.is_grad_enabled():
            ray_graph = bool(self.pose_gradients) and (rd.requires_grad or ro.requires_grad)
            if ray_graph or any(p.requires_grad for p in self.parameters()):
                ctx = Context.get(dev)
                p = self._params()
                U_c, U_f = self._draw_pair(B, dev)
                radius = p.ray_radius if p.cone_sampling else None
                if ray_graph:
                    self._check_pose_fields()
                    rd, ro = rd.to(torch.float32), ro.to(torch.float32)
                else:
                    rd, ro = rd.detach().to(torch.float32).contiguous(), ro.detach().to(torch.float32).contiguous()
                return self._render_generated_rays(ctx, rd, ro, radius, U_c, U_f, ray_graph=ray_graph)
        return self._render_rays_fused(rays, None, B, dev)

    def render_rays_views(self, uv: Tensor, view_index: Tensor, table: Tensor) -> Dict[str, Tensor]:
        """render_rays on a batch in which every row has its own camera (not a reference method): row b is pixel uv[b] of the
        camera in row view_index[b] of `table` (uv [B,2]; view_index int32 or int64 [B]; table float32 [K,16] rows of R row-major,
        T, calib -- CameraSet.table builds them).  ONE ray-generation launch whatever K is, then render_bundle's stages, draws
        and keys.  Inference is the fused call with the library's camera-table flag: no ray tensor is made.  Under autograd the
        network parameters receive gradients as in render_rays, and with pose_gradients set and `table` requiring grad ray
        generation is RayTableFunction: one backward launch fills the [K,16] gradient (intrinsics columns zero).  Nothing here
        reads the device, so view_index is the caller's to validate (CameraSet.select / check_view on the host draw): a row
        whose index lies outside [0, K) reads no camera and renders NaN, which the inference path's assertion reports."""
        from .autograd import RayTableFunction
        if self.ray_space == "ndc":
            raise NotImplementedError("render_rays_views: NDC rays (ray_space='ndc') take one camera's focal lengths")
        dev = table.device
        uv = uv.to(dev)
        view_index = torch.as_tensor(view_index).to(dev)
        if view_index.dtype not in (torch.int32, torch.int64):
            view_index = view_index.to(torch.int64)
        if uv.dim() != 2 or uv.shape[1] != 2 or view_index.shape != (uv.shape[0],):
            raise ValueError("render_rays_views: uv must be [B, 2] and view_index [B]")
        if table.dim() != 2 or table.shape[1] != 16 or table.shape[0] < 1:
            raise ValueError("render_rays_views: table must be [K, 16] with K >= 1")
        B = uv.shape[0]
        if torch.is_grad_enabled():
            graph = bool(self.pose_gradients) and table.requires_grad
            if graph or any(p.requires_grad for p in self.parameters()):
                ctx = Context.get(dev)
                p = self._params()
                U_c, U_f = self._draw_pair(B, dev)
                radius = p.ray_radius if p.cone_sampling else None
                if graph:
                    self._check_pose_fields()
                    rd, ro = RayTableFunction.apply(ctx, uv, view_index, table.to(torch.float32))
                else:
                    with torch.no_grad():
                        rd, ro = ctx.raygen(ViewRays(uv, view_index, table.detach().to(torch.float32)))
                return self._render_generated_rays(ctx, rd, ro, radius, U_c, U_f, ray_graph=graph)
        return self._render_rays_fused(ViewRays(uv, view_index, table.detach().to(torch.float32)), None, B, dev)

    def render_rays_mixed(self, uv: Tensor, view_index: Tensor, cameras: List[Camera]) -> Dict[str, Tensor]:
        """render_rays on a batch that mixes views (not a reference method): row b is pixel uv[b] of cameras[view_index[b]]
        (uv [B,2], view_index int64 [B]).  The visited cameras' R / T / intrinsics AS THEY STAND are stacked into a camera table
        (under pose_gradients with their graph, so that each visited camera's R / T receive gradients) and the batch goes through
        render_rays_views: one ray-generation launch and one backward launch whatever the number of views, no descriptor read.
        Its keys, draws and assertion are render_bundle's, and every output carries the bits of generating each camera's rows
        with render_rays' own ray generation.  A camera that owns no row costs nothing and gets no gradient; an index outside
        the list raises ValueError (the one device -> host read).  If a VISITED camera is not a pinhole the batch takes the
        per-camera route instead (_render_rays_mixed_per_camera): its rays are made in torch."""
        if self.ray_space == "ndc":
            raise NotImplementedError("render_rays_mixed: NDC rays (ray_space='ndc') are not supported")
        cameras = list(cameras)
        if not cameras:
            raise ValueError("render_rays_mixed: no cameras")
        dev = cameras[0].device
        uv = uv.to(dev)
        view_index = torch.as_tensor(view_index).to(device=dev, dtype=torch.int64)
        if uv.dim() != 2 or uv.shape[1] != 2 or view_index.shape != (uv.shape[0],):
            raise ValueError("render_rays_mixed: uv must be [B, 2] and view_index [B]")
        B = uv.shape[0]
        counts = [0] * len(cameras)
        if B:       # one device -> host read: the smallest index, then the rows per camera
            lowest, *counts = torch.cat([view_index.min().view(1), torch.bincount(view_index.clamp(min=0), minlength=len(cameras))]).tolist()
            if lowest < 0 or len(counts) > len(cameras):
                raise ValueError("render_rays_mixed: view_index must lie in [0, %d)" % len(cameras))
        visited = [i for i, count in enumerate(counts) if count]
        if not visited:
            return self.render_bundle(Ray(torch.empty(0, 3, device=dev), torch.empty(0, 3, device=dev)))
        if not all(_is_pinhole(cameras[i]) for i in visited):
            return self._render_rays_mixed_per_camera(uv, view_index, cameras, counts)
        graph = torch.is_grad_enabled() and bool(self.pose_gradients)
        with torch.set_grad_enabled(graph):
            table = torch.cat([torch.stack([cameras[i].R.to(torch.float32).reshape(9) for i in visited]),
                               torch.stack([cameras[i].T.to(torch.float32) for i in visited]),
                               torch.stack([cameras[i].camera_calib.params.detach().to(torch.float32) for i in visited])], 1)
        local = view_index
        if len(visited) != len(cameras):        # positions in the visited list
            lut = torch.full((len(cameras),), -1, dtype=torch.int64)
            lut[visited] = torch.arange(len(visited))
            local = lut.to(dev)[view_index]
        return self.render_rays_views(uv, local, table)

    def _render_rays_mixed_per_camera(self, uv: Tensor, view_index: Tensor, cameras: List[Camera], counts: List[int]) -> Dict[str, Tensor]:
        """render_rays_mixed where a visited camera is not a pinhole: every camera that owns rows generates them, in batch order,
        with render_rays' own ray generation (a launch, or Camera.create_rays in torch, per visited camera), the rays go back to
        their batch positions and the batch runs as one bundle."""
        from .autograd import RayFunction
        dev, B = uv.device, uv.shape[0]
        order = torch.argsort(view_index, stable=True)          # rows grouped by camera, batch order inside a group
        graph = torch.is_grad_enabled() and bool(self.pose_gradients)
        ctx = Context.get(dev)
        dirs, origs, start = [], [], 0
        for camera, count in zip(cameras, counts):
            if not count:
                continue
            rows = uv[order[start:start + count]]
            start += count
            if not _is_pinhole(camera):
                with torch.set_grad_enabled(graph):
                    part = camera.create_rays(rows)
                rd, ro = part.ray_dir, part.ray_orig
            elif graph:
                rd, ro = RayFunction.apply(ctx, rows, camera.descriptor(), camera.R, camera.T)
            else:
                with torch.no_grad():
                    rd, ro = ctx.raygen(rows, camera.descriptor())
            dirs.append(rd)
            origs.append(ro)
        back = torch.empty_like(order)
        back[order] = torch.arange(B, device=dev)               # where batch row b stands in the grouped order
        return self.render_bundle(Ray(torch.cat(dirs)[back], torch.cat(origs)[back]))

    def _view_rays(self, uv: Tensor, camera: Camera):
        """What the fused entry points take for pixels `uv` of `camera`, (uv argument, camera descriptor, bundle): the pixels and
        the pinhole descriptor for a PinholeCalib -- the path every release took -- and otherwise the rays Camera.create_rays makes
        in torch, as float32 [n, 6] (direction, origin) rows with no descriptor."""
        if _is_pinhole(camera):
            return uv, camera.descriptor(), False
        if self.ray_space == "ndc":
            raise NotImplementedError("NDC rays (ray_space='ndc') need a pinhole camera's focal lengths")
        with torch.no_grad():
            rays = camera.create_rays(uv)
            return torch.cat([rays.ray_dir, rays.ray_orig], 1).contiguous(), None, True

    # ------------------------------------------------------------- render_image
    def render_image(self, width: int, height: int, camera: Camera, target_types: Iterable[RenderTarget],
                     downsampling: int = 1, chunk: int = 512, pixel_range=None) -> Dict[str, Tensor]:
        """nerf_render.py:190-249.  Pixels are row-major (idx = v*w + u).  In
        "torch_cpu" RNG mode the uniforms are drawn chunk by chunk in the
        reference's order ([B,Sc+1] then [B,Sf+1] per chunk of `chunk` rays), so a
        given torch seed renders the same samples; rays are then processed in
        batches of `rays_per_call` regardless of `chunk` (rays are independent).
        pixel_range=(lo, hi) (not in the reference) renders only that slab of the
        row-major pixel index and returns flat [hi-lo, C] tensors -- the unit of
        multi-GPU ray sharding (neddf_amd/parallel.py); the slab's uniforms are the
        ones the whole-frame draw would have given it (generator jump-ahead, rng.py),
        so the image does not depend on the sharding.
        target_types may hold "normal" (not a reference target): [h, w, 3], the normal_output quantity of the class docstring;
        the other targets are the same bits with or without it."""
        target_types = list(target_types)
        want_normal = "normal" in target_types
        if want_normal:
            self._check_normal_fields(coarse=False)
        with torch.no_grad():
            dev = camera.device
            uv, w, h = self._pixel_grid(width, height, downsampling, dev)
            n = uv.shape[0]
            self.network_coarse.eval()
            self.network_fine.eval()
            ctx = self._ctx(dev)
            parts: Dict[str, List[Tensor]] = {k: [] for k in target_types}
            flags = []
            lo, hi = (0, n) if pixel_range is None else pixel_range

            uv, cam_desc, bundle = self._view_rays(uv, camera)    # three device -> host reads: once per image, not per batch
            occ = self._occupancy_desc(dev)

            def launch(below, above, U_c, U_f):
                # sample_pdf's NaN fallback keeps the reference's per-chunk granularity: batches start on chunk boundaries,
                # except a slab's first batch, which may start inside a chunk another rank shares
                o = self._render(ctx, uv[below:above], camera, U_c, U_f, full=False, cam_desc=cam_desc, nan_group=chunk,
                                 nan_group_offset=below % chunk, normal=want_normal, occupancy=occ, bundle=bundle)
                flags.append(o["_nan"])
                for k in target_types:
                    parts[k].append(o[k])

            if self.rng == "torch_cpu":
                # Draw chunk by chunk in the reference's order, but hand rays_per_call rays at a time to the GPU:
                # launches are asynchronous, so the host draws the next batch while the device renders this one.
                # A slab (pixel_range) starts its draws where the reference's stream would be at its first chunk:
                # the generator JUMPS there (rng.py, milliseconds) instead of drawing and discarding, so the host
                # cost of a rank shrinks with the slab; after the slab it jumps to where the whole frame would have
                # left it, i.e. every rank ends in the reference's generator state.
                per_ray = self.sample_coarse + 1 + self.sample_fine + 1
                first = (lo // chunk) * chunk if hi > lo else n      # chunks before the slab are all full
                skip_uniforms(first * per_ray)
                uc, uf, start, count, below = [], [], first, 0, first
                while below < min(n, hi):
                    b = min(n, below + chunk) - below
                    uc.append(torch.rand(b, self.sample_coarse + 1)); uf.append(torch.rand(b, self.sample_fine + 1))
                    count += b
                    below += b
                    if count >= self.rays_per_call or below >= min(n, hi):
                        a0, a1 = max(start, lo), min(start + count, hi)
                        U_c = torch.cat(uc)[a0 - start:a1 - start].to(dev, non_blocking=True)
                        U_f = torch.cat(uf)[a0 - start:a1 - start].to(dev, non_blocking=True)
                        launch(a0, a1, U_c, U_f)
                        uc, uf, start, count = [], [], start + count, 0
                skip_uniforms((n - below) * per_ray)
            else:
                # batches of whole chunks (sample_pdf's NaN fallback is decided per chunk, never on part of one)
                step = max(chunk, self.rays_per_call // chunk * chunk)
                for below in range(lo, hi, step):
                    above = min(hi, below + step)
                    launch(below, above, *self._draw_pair(above - below, dev))
            assert not flags or int(torch.stack(flags).sum().item()) == 0, "NaN weight in integrate_volume_render"
            if pixel_range is None:
                images = {k: torch.cat(parts[k], 0).reshape(h, w, -1) for k in target_types}
            elif hi <= lo:          # an empty slab (more ranks than chunks)
                images = {k: torch.empty(0, 3 if k in ("color", "normal") else 1, device=dev) for k in target_types}
            else:
                images = {k: torch.cat(parts[k], 0).reshape(hi - lo, -1) for k in target_types}
            self.network_coarse.train(True)
            self.network_fine.train(True)
        return images

    def render_image_single_pass(self, width: int, height: int, camera: Camera, samples: int,
                                 U: Optional[Tensor] = None, pixel_range=None, normals: bool = False) -> Dict[str, Tensor]:
        """One stratified pass of `samples` points per ray through network_fine
        (BASELINE.json configs[1]).  Not a reference method: it is render_rays'
        coarse half (nerf_render.py:128-152) at image scale.  pixel_range=(lo,hi)
        restricts to a slab of the row-major pixel index (multi-GPU sharding).
        Returns flat per-ray tensors color [n,3], depth [n], transmittance [n]; with normals=True also normal [n,3]
        (the normal_output quantity of the class docstring), the others unchanged."""
        if normals:
            self._check_normal_fields(coarse=False)
        with torch.no_grad():
            dev = camera.device
            lo, hi = (0, width * height) if pixel_range is None else pixel_range
            idx = torch.arange(lo, hi, device=dev)
            uv = torch.stack([idx % width, idx // width], 1)
            n = hi - lo
            ctx = self._ctx(dev)
            out = dict(color=torch.empty(n, 3, device=dev), depth=torch.empty(n, device=dev),
                       transmittance=torch.empty(n, device=dev))
            if normals:
                out["normal"] = torch.empty(n, 3, device=dev)
            flag = torch.zeros(1, device=dev, dtype=torch.int32)
            uv, cam_desc, bundle = self._view_rays(uv, camera)
            occ = self._occupancy_desc(dev)
            for below in range(0, n, self.rays_per_call):
                above = min(n, below + self.rays_per_call)
                o = {k: v[below:above] for k, v in out.items()}
                # without U the uniforms are drawn per batch: in "torch_cpu" mode the host draws batch k+1 while batch k renders
                Ub = U[below:above] if U is not None else self._rand(above - below, samples, dev)
                ctx.render_rays(uv[below:above], cam_desc, self._params(), Ub, None,
                                dict(o, nan_flag=flag), single_slot=SLOT_FINE, occupancy=occ, bundle=bundle)
            out["_nan"] = flag
        return out

    TRACED_TARGETS = ("color", "depth", "transmittance", "normal", "steps")

    def render_image_traced(self, width: int, height: int, camera: Camera, target_types: Iterable[RenderTarget], threshold: float,
                            downsampling: int = 1, pixel_range=None, max_steps: int = 64, step_scale: float = 1.0,
                            min_step: Optional[float] = None, refine: int = 4, background: float = 0.0) -> Dict[str, Tensor]:
        """A surface view by sphere tracing (trace.py; not a reference method): render_image's world-space rays march through
        network_fine's distance (NeuS: sdf) from dist_near to dist_far until it falls to `threshold` -- the level set
        extract_mesh meshes -- inside the library (neddf_trace_field: distance-only evaluations on the rays still marching),
        then ONE full evaluation (field_forward_surface, dir = the ray direction, var = 0) at the points of the rays that hit,
        compacted in ray order, gives colour and normal.  Targets, [h, w, 3] or [h, w]:

            color          the field's colour on HIT pixels, `background` elsewhere
            depth          t on HIT pixels, 0 elsewhere
            transmittance  0 on HIT pixels, 1 elsewhere (the hit mask)
            normal         the field's `normal` output (forward_surface) on HIT pixels, 0 elsewhere
            steps          int32: advances the ray took, whatever its end

        pixel_range=(lo, hi) renders that slab of the row-major pixel index and returns flat [hi - lo, 3] / [hi - lo] tensors.
        max_steps, step_scale, min_step (None: (dist_far - dist_near) * 2**-10) and refine are trace.sphere_trace's; a trained
        distance is only roughly 1-Lipschitz, step_scale < 1 is the knob for a field that oversteps, and no default is tuned.
        NeDDF and NeuS fields with world-space rays; NeRF fields and ray_space='ndc' raise.  No random numbers are drawn."""
        from ._lib import OUT_MINIMAL
        from .trace import HIT, trace_params
        target_types = list(target_types)
        unknown = [k for k in target_types if k not in self.TRACED_TARGETS]
        if unknown:
            raise ValueError("render_image_traced: unknown target(s) %s; it offers %s" % (unknown, list(self.TRACED_TARGETS)))
        if self.ray_space != "world":
            raise NotImplementedError("render_image_traced marches world-space rays: ray_space=%r is not supported" % (self.ray_space,))
        if not self.network_fine._has_surface():
            raise NotImplementedError("render_image_traced needs a field with a distance or sdf (NeDDF, NeuS); %s has none"
                                      % type(self.network_fine).__name__)
        params = trace_params(threshold, self.dist_near, self.dist_far, max_steps, step_scale, min_step, refine)
        with torch.no_grad():
            dev = camera.device
            uv, w, h = self._pixel_grid(width, height, downsampling, dev, pixel_range)
            n = uv.shape[0]
            ctx = self._ctx(dev)
            uv, cam_desc, bundle = self._view_rays(uv, camera)
            rd, ro = ctx.raygen(uv, cam_desc, bundle=bundle)
            st, _ = ctx.trace_field(SLOT_FINE, ro, rd, params)
            hit = st["status"] == HIT
            out = self._hit_targets(hit, st["t"], target_types)
            if "steps" in target_types:
                out["steps"] = st["steps"]
            wide = [k for k in ("color", "normal") if k in target_types]
            if wide:
                idx = hit.nonzero().squeeze(1)
                if "color" in wide:
                    out["color"] = torch.as_tensor(background, dtype=torch.float32, device=dev).expand(n, 3).contiguous()
                if "normal" in wide:
                    out["normal"] = torch.zeros(n, 3, device=dev)
                if idx.shape[0]:
                    pos = ro[idx] + st["t"][idx, None] * rd[idx]        # a rounded product, then a rounded sum: the tracer's own points
                    o = ctx.field_forward_surface(SLOT_FINE, pos, rd[idx], torch.zeros_like(pos), OUT_MINIMAL, wide)
                    for k in wide:
                        out[k][idx] = o[k].view(-1, 3)
        return self._as_images(out, target_types, w, h, pixel_range)

    MESH_TARGETS = ("depth", "transmittance", "triangle", "normal", "color", "ambient_occlusion")
    MESH_TILE = 8

    @staticmethod
    def tile_order(w: int, h: int, tile: int, device) -> Tensor:
        """int64 [w * h]: the row-major pixel indices ordered by tile x tile pixel tiles (tiles row-major, pixels row-major inside a
        tile; partial tiles at the right and bottom edges) -- 64 consecutive entries are one 8 x 8 tile where the tile is whole."""
        v, u = torch.meshgrid(torch.arange(h, device=device), torch.arange(w, device=device), indexing="ij")
        key = (((v // tile) * ((w + tile - 1) // tile) + u // tile) * tile + v % tile) * tile + u % tile
        return torch.argsort(key.reshape(-1))

    def render_image_mesh(self, width: int, height: int, camera: Camera, vertices: Tensor, triangles: Tensor,
                          target_types: Iterable[RenderTarget], normals: Optional[Tensor] = None, colors: Optional[Tensor] = None,
                          downsampling: int = 1, pixel_range=None, method: str = "grid", background: float = 0.0, grid=None, bvh=None,
                          tile: int = 0, ao_dirs: int = 16, ao_radius: Optional[float] = None) -> Dict[str, Tensor]:
        """A view of a triangle mesh (vertices float32 [V, 3], triangles int32 or int64 [T, 3] on the camera's device; not a
        reference method): render_image_traced's world-space rays -- the same pixels -- meet the mesh between dist_near and
        dist_far inside the library (raycast.cast_rays: the first watertight hit, method "grid" or "brute", the same bits).
        Targets, [h, w, 3] or [h, w]:

            depth          t on HIT pixels, 0 elsewhere
            transmittance  0 on HIT pixels, 1 elsewhere (the hit mask)
            triangle       int32: the triangle hit, -1 elsewhere
            normal         the vertex `normals` [V, 3] interpolated at the hit when given, otherwise the face's geometric normal;
                           normalised, turned to face the ray, 0 elsewhere
            color          the vertex `colors` [V, 3] interpolated at the hit, `background` elsewhere (raises without colors)
            ambient_occlusion  [h, w]: bvh.ambient_occlusion (ao_dirs directions, radius ao_radius) at the hit points p0 + b1 (p1 - p0)
                           + b2 (p2 - p0) with the `normal` target's normals, 1 elsewhere; needs `bvh`

        pixel_range=(lo, hi) renders that slab of the row-major pixel index and returns flat tensors.  grid: the mesh's
        raycast.build_grid, to be built once for many views (None: built here).  bvh: the mesh's bvh.build_bvh, or True to build it
        here -- the rays then go through bvh.cast_rays (the same bits; not together with `grid` or method="brute").  tile=8 casts the
        rays ordered by 8 x 8 pixel tiles (tile_order: one wave of the kernels is one tile) and scatters the results back: every pixel
        keeps its bits, with every method; not together with pixel_range.  Interpolation and normals are torch gathers over the hit
        pixels.  ray_space='ndc' raises.  No network is evaluated, no random number drawn."""
        from . import bvh as bvh_module
        from .raycast import cast_rays
        target_types = list(target_types)
        if tile not in (0, self.MESH_TILE):
            raise ValueError("render_image_mesh: tile must be 0 or %d (got %r)" % (self.MESH_TILE, tile))
        if tile and pixel_range is not None:
            raise ValueError("render_image_mesh: tile orders the whole image; it cannot be combined with pixel_range")
        if bvh is not None and bvh is not False and (grid is not None or method == "brute"):
            raise ValueError("render_image_mesh: bvh casts the rays through the tree; it cannot be combined with grid or method='brute'")
        if bvh is False:
            bvh = None
        if "ambient_occlusion" in target_types and bvh is None:
            raise ValueError("render_image_mesh: the ambient_occlusion target needs bvh (a MeshBVH, or True)")
        unknown = [k for k in target_types if k not in self.MESH_TARGETS]
        if unknown:
            raise ValueError("render_image_mesh: unknown target(s) %s; it offers %s" % (unknown, list(self.MESH_TARGETS)))
        if self.ray_space != "world":
            raise NotImplementedError("render_image_mesh casts world-space rays: ray_space=%r is not supported" % (self.ray_space,))
        if "color" in target_types and colors is None:
            raise ValueError("render_image_mesh: the color target needs vertex colors")
        for name, a in (("normals", normals), ("colors", colors)):
            if a is not None and (a.dim() != 2 or tuple(a.shape) != tuple(vertices.shape)):
                raise ValueError("render_image_mesh: %s must be [V, 3] like the vertices (got %s)" % (name, tuple(a.shape)))
        with torch.no_grad():
            dev = camera.device
            uv, w, h = self._pixel_grid(width, height, downsampling, dev, pixel_range)
            n = uv.shape[0]
            uv, cam_desc, bundle = self._view_rays(uv, camera)
            rd, ro = self._ctx(dev).raygen(uv, cam_desc, bundle=bundle)
            order = self.tile_order(w, h, tile, dev) if tile else None
            co, cd = (ro, rd) if order is None else (ro[order].contiguous(), rd[order].contiguous())
            if bvh is not None:
                if bvh is True:
                    bvh = bvh_module.build_bvh(vertices, triangles)
                hits = bvh_module.cast_rays(co, cd, vertices, triangles, t_min=self.dist_near, t_max=self.dist_far, bvh=bvh)
            else:
                hits = cast_rays(co, cd, vertices, triangles, t_min=self.dist_near, t_max=self.dist_far, method=method, grid=grid)
            if order is not None:
                hits = {k: torch.empty_like(a).index_copy_(0, order, a) for k, a in hits.items()}
            hit = hits["triangle"] >= 0
            out = self._hit_targets(hit, hits["t"], target_types)
            if "triangle" in target_types:
                out["triangle"] = hits["triangle"]
            wide = [k for k in ("color", "normal", "ambient_occlusion") if k in target_types]
            if wide:
                idx = hit.nonzero().squeeze(1)
                corners = triangles[hits["triangle"][idx].long()].long()                 # [n_hit, 3] vertex indices
                b1, b2 = hits["b1"][idx, None], hits["b2"][idx, None]

                def interpolate(a):
                    a = a.to(torch.float32)
                    a0 = a[corners[:, 0]]
                    return a0 + b1 * (a[corners[:, 1]] - a0) + b2 * (a[corners[:, 2]] - a0)
                if "color" in wide:
                    out["color"] = torch.as_tensor(background, dtype=torch.float32, device=dev).expand(n, 3).contiguous()
                    out["color"][idx] = interpolate(colors)
                if "normal" in wide or "ambient_occlusion" in wide:
                    if normals is not None:
                        nrm = interpolate(normals)
                    else:
                        p0 = vertices[corners[:, 0]]
                        nrm = torch.cross(vertices[corners[:, 1]] - p0, vertices[corners[:, 2]] - p0, dim=1)
                    nrm = torch.nn.functional.normalize(nrm, dim=1)
                    away = (nrm * rd[idx]).sum(dim=1, keepdim=True) > 0
                    nrm = torch.where(away, -nrm, nrm)
                if "normal" in wide:
                    out["normal"] = torch.zeros(n, 3, device=dev)
                    out["normal"][idx] = nrm
                if "ambient_occlusion" in wide:
                    out["ambient_occlusion"] = torch.ones(n, device=dev)
                    if idx.shape[0]:
                        ao = bvh_module.ambient_occlusion(interpolate(vertices), nrm, vertices, triangles, n_dirs=ao_dirs, radius=ao_radius, bvh=bvh)
                        out["ambient_occlusion"][idx] = ao
        return self._as_images(out, target_types, w, h, pixel_range)

    def render_field_slice(self, slice_t: float = 0.0, render_size: float = 1.1, render_resolution: int = 128,
                           colormap: bool = True):
        """nerf_render.py:263-336: z = slice_t plane of the fine network's fields as uint8 images (debug view).
        Scalar fields are JET colour-mapped (BGR, same control points as cv2.COLORMAP_JET; cv2 itself is not a
        dependency here), colour is scaled by 256.  colormap=False (not a reference keyword) returns the scalar
        fields as the [n,n,1] uint8 images the reference hands to cv2.applyColorMap."""
        import numpy as np
        from .ray import Sampling
        with torch.no_grad():
            device = self.network_fine.device
            n = render_resolution
            lin = torch.linspace(-render_size, render_size, n, device=device)
            xs = lin.reshape(1, n).expand(n, n)
            ys = -lin.reshape(n, 1).expand(n, n)
            zs = torch.zeros(n, n, device=device) + slice_t
            pos = torch.stack([xs, ys, zs], 2).contiguous()
            d = torch.zeros(n, n, 3, device=device)
            d[:, :, 2] = 1.0
            self.network_fine.train(False)
            values = self.network_fine(Sampling(pos, d, torch.zeros_like(pos)))
            self.network_fine.train(True)
            scales = {"distance": 256.0, "density": 12.8, "color": 256.0, "aux_grad": 256.0}
            fields = {}
            for key, val in values.items():
                if key not in scales:
                    continue
                f = (scales[key] * val.reshape(n, n, -1)).cpu().numpy().clip(0, 255).astype(np.uint8)
                fields[key] = jet_bgr(f[:, :, 0]) if (f.shape[2] == 1 and colormap) else f
            return fields


def jet_bgr(gray):
    """uint8 [h,w] -> uint8 [h,w,3] (B,G,R): cv2.applyColorMap(gray, cv2.COLORMAP_JET) restated (nerf_render.py:330; cv2 is in neither
    container, so this is pinned on the published algorithm, not on cv2's output).  OpenCV builds the table from three float arrays
    r, g, b of 256 entries -- the piecewise-linear ramps clamp(1.5 - |4 i/255 - c|, 0, 1) with c = 3, 2, 1, written out as literals --
    and converts them with `convertTo(CV_8U, 255.)`: a float product and cvRound (round half to EVEN).  Every ramp entry times 255 is
    an exact half-integer (382.5 - |4 i - 255 c|), so the rounding mode decides each of them: the ramps step by 4 (blue: 128, 132,
    136, ... at i = 0, 1, 2, ...; entries 0 / 255 are (128, 0, 0) / (0, 0, 128) in B, G, R).  Round 3's `+ 0.5` truncation in double
    differed from this on 149 of the 768 entries by one count."""
    import numpy as np
    x = np.arange(256, dtype=np.float64) / 255.0
    lut = np.stack([np.rint(np.clip(1.5 - np.abs(4 * x - c), 0, 1).astype(np.float32) * np.float32(255.0)) for c in (1, 2, 3)], 1)
    return lut.astype(np.uint8)[gray]
