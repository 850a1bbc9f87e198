"""torch.autograd glue of the training step.

The reference trains through torch autograd over its with_grad modules
(neddf/nn_module/with_grad/*.py carry hand-written backward passes for the
(value, Jacobian) pairs) and plain torch ops for the volume integral
(base_neural_render.py:148-171).  Here both are single autograd nodes whose
forward and backward are HIP kernels behind the C ABI
(neddf_train_field_forward / _backward, neddf_composite / _composite_backward);
torch only carries the small per-ray tensors between them and into the losses.

Pose gradients (opt-in, `render.pose_gradients = True`): the reference builds its rays from camera.R / camera.T with
differentiable torch ops, so its loss reaches Camera.params.  Here that chain is three more nodes over HIP kernels --
FieldFunction's input gradients, SamplingFunction, RayFunction -- and torch carries g_R / g_T through Rodrigues
(Camera.update_transform) to the six pose parameters.
"""
from typing import Tuple

import torch
from torch import Tensor

from ._lib import Context, ViewRays


class FieldFunction(torch.autograd.Function):
    """NeDDF.forward (neddf.py:162-309) on [N,3] samples -> distance, density, color, fields_penalty, aux_grad.

    Gradients flow to the parameters and, when pos / dir / var require them, to the sample inputs
    (neddf_train_field_backward_inputs): in the reference the samplers are differentiable torch ops, so the loss reaches the
    rays and the camera pose through them.  The gradient of var is zero, as in the reference (get_pe_weights runs with
    gradients disabled, sampling.py:55).  Inputs that do not require a gradient cost nothing: the parameter-only kernel
    path runs, bit for bit as before."""

    @staticmethod
    def forward(ctx, hip: Context, slot: int, iter_state, n_tensors: int, pos: Tensor, dir: Tensor, var: Tensor,
                *params: Tensor) -> Tuple[Tensor, ...]:
        weights = [p.detach() for p in params[:n_tensors]]
        biases = [p.detach() for p in params[n_tensors:]]
        hip.set_iter(slot, *iter_state)
        ws, distance, density, color, penalty, aux = hip.train_field_forward(slot, weights, biases, pos, dir, var)
        ctx.hip, ctx.slot, ctx.iter_state, ctx.n_tensors, ctx.n_points = hip, slot, iter_state, n_tensors, distance.shape[0]
        ctx.input_grads = any(ctx.needs_input_grad[4:7])
        ctx.save_for_backward(ws, *((pos, dir, var) if ctx.input_grads else ()), *params)
        return distance, density, color, penalty, aux

    @staticmethod
    def backward(ctx, g_distance, g_density, g_color, g_penalty, g_aux):
        ws, *params = ctx.saved_tensors
        inputs = None
        if ctx.input_grads:
            inputs, params = tuple(t.detach() for t in params[:3]), params[3:]
        n = ctx.n_tensors
        weights = [p.detach() for p in params[:n]]
        biases = [p.detach() for p in params[n:]]
        ctx.hip.set_iter(ctx.slot, *ctx.iter_state)
        with torch.cuda.device(ws.device):
            if ctx.input_grads:
                gw, gb, g_in = ctx.hip.train_field_backward(ctx.slot, weights, biases, ctx.n_points, ws, g_distance, g_density,
                                                            g_color, g_penalty, g_aux, inputs=inputs)
                g_in = tuple(g.view(t.shape) if need else None for g, t, need in zip(g_in, inputs, ctx.needs_input_grad[4:7]))
                return (None,) * 4 + g_in + tuple(gw) + tuple(gb)
            gw, gb = ctx.hip.train_field_backward(ctx.slot, weights, biases, ctx.n_points, ws, g_distance, g_density, g_color,
                                                  g_penalty, g_aux)
        return (None,) * 7 + tuple(gw) + tuple(gb)


class RadianceFieldFunction(torch.autograd.Function):
    """NeRF.forward (nerf.py:107-165) on [N,3] samples -> density, color.  The reference differentiates this network
    with plain torch autograd over nn.Linear; here forward and backward are the same HIP building blocks as NeDDF's
    (value rows only), one autograd node for the whole field."""

    @staticmethod
    def forward(ctx, hip: Context, slot: int, iter_state, n_tensors: int, pos: Tensor, dir: Tensor, var: Tensor,
                *params: Tensor) -> Tuple[Tensor, Tensor]:
        weights = [p.detach() for p in params[:n_tensors]]
        biases = [p.detach() for p in params[n_tensors:]]
        hip.set_iter(slot, *iter_state)
        ws, _, density, color, _, _ = hip.train_field_forward(slot, weights, biases, pos, dir, var, radiance_only=True)
        ctx.hip, ctx.slot, ctx.iter_state, ctx.n_tensors, ctx.n_points = hip, slot, iter_state, n_tensors, density.shape[0]
        ctx.input_grads = any(ctx.needs_input_grad[4:7])        # as FieldFunction: gradients of pos / dir (var: zero)
        ctx.save_for_backward(ws, *((pos, dir, var) if ctx.input_grads else ()), *params)
        return density, color

    @staticmethod
    def backward(ctx, g_density, g_color):
        ws, *params = ctx.saved_tensors
        inputs = None
        if ctx.input_grads:
            inputs, params = tuple(t.detach() for t in params[:3]), params[3:]
        n = ctx.n_tensors
        weights = [p.detach() for p in params[:n]]
        biases = [p.detach() for p in params[n:]]
        ctx.hip.set_iter(ctx.slot, *ctx.iter_state)
        with torch.cuda.device(ws.device):
            if ctx.input_grads:
                gw, gb, g_in = ctx.hip.train_field_backward(ctx.slot, weights, biases, ctx.n_points, ws, None, g_density, g_color, None,
                                                            None, inputs=inputs)
                g_in = tuple(g.view(t.shape) if need else None for g, t, need in zip(g_in, inputs, ctx.needs_input_grad[4:7]))
                return (None,) * 4 + g_in + tuple(gw) + tuple(gb)
            gw, gb = ctx.hip.train_field_backward(ctx.slot, weights, biases, ctx.n_points, ws, None, g_density, g_color, None, None)
        return (None,) * 7 + tuple(gw) + tuple(gb)


class SdfFieldFunction(torch.autograd.Function):
    """NeuS.forward (neus.py:101-162) on [N,3] samples -> sdf, density, color.  The reference takes the normal with
    torch.autograd.grad(create_graph=True), so its parameter gradients are a double backward; here the normal is the
    Jacobian rows of the sdf trunk and the backward is the ordinary reverse pass over (value, Jacobian) rows.  `params` =
    weights (..., variance as a 1-element tensor) followed by biases (..., an unused 1-element tensor)."""

    @staticmethod
    def forward(ctx, hip: Context, slot: int, n_tensors: int, pos: Tensor, dir: Tensor, *params: Tensor) -> Tuple[Tensor, ...]:
        if any(ctx.needs_input_grad[3:5]):
            raise NotImplementedError("pose gradients through a NeuS field need a third derivative of the sdf trunk: not implemented")
        weights = [p.detach() for p in params[:n_tensors]]
        biases = [p.detach() for p in params[n_tensors:]]
        ws, sdf, density, color, _, _ = hip.train_field_forward(slot, weights, biases, pos, dir, torch.zeros_like(pos),
                                                                radiance_only=False, sdf=True)
        ctx.hip, ctx.slot, ctx.n_tensors, ctx.n_points = hip, slot, n_tensors, sdf.shape[0]
        ctx.save_for_backward(ws, *params)
        return sdf, density, color

    @staticmethod
    def backward(ctx, g_sdf, g_density, g_color):
        ws, *params = ctx.saved_tensors
        n = ctx.n_tensors
        weights = [p.detach() for p in params[:n]]
        biases = [p.detach() for p in params[n:]]
        with torch.cuda.device(ws.device):
            gw, gb = ctx.hip.train_field_backward(ctx.slot, weights, biases, ctx.n_points, ws, g_sdf, g_density, g_color, None, None)
        return (None,) * 5 + tuple(gw) + tuple(gb[:-1]) + (None,)


class CompositeFunction(torch.autograd.Function):
    """integrate_volume_render (base_neural_render.py:117-172) -> weight, depth, color, transmittance."""

    @staticmethod
    def forward(ctx, hip: Context, max_dist: float, dists: Tensor, densities: Tensor, colors: Tensor):
        out, flag = hip.composite(dists, densities, colors, max_dist)
        ctx.hip, ctx.max_dist = hip, max_dist
        ctx.save_for_backward(dists, densities, colors)
        ctx.mark_non_differentiable(flag)
        return out["weight"], out["depth"], out["color"], out["transmittance"], flag

    @staticmethod
    def backward(ctx, g_weight, g_depth, g_color, g_trans, _g_flag):
        dists, densities, colors = ctx.saved_tensors
        with torch.cuda.device(dists.device):
            g_density, g_point_color = ctx.hip.composite_backward(dists, densities, colors, ctx.max_dist, g_weight, g_depth,
                                                                  g_color, g_trans)
        return None, None, None, g_density, g_point_color


class SamplingFunction(torch.autograd.Function):
    """Ray.get_sampling_cones (ray.py:128-194) / get_sampling_points (ray.py:88-126) with the ray differentiable:
    (ray_dir, ray_orig) [B,3] -> (pos, dir, var) [B,S,3].  The distances are not differentiated, as in the reference (stratified
    uniforms and sample_pdf output under no_grad)."""

    @staticmethod
    def forward(ctx, hip: Context, ray_dir: Tensor, ray_orig: Tensor, dists: Tensor, radius):
        pos, d, var = hip.sampling(ray_dir, ray_orig, dists, radius)
        ctx.hip, ctx.radius = hip, radius
        ctx.save_for_backward(ray_dir, dists)
        return pos, d, var

    @staticmethod
    def backward(ctx, g_pos, g_dir, g_var):
        ray_dir, dists = ctx.saved_tensors
        with torch.cuda.device(dists.device):
            g_rd, g_ro = ctx.hip.sampling_backward(g_pos, g_dir, g_var, ray_dir, dists, ctx.radius)
        return None, g_rd, g_ro, None, None


class RayFunction(torch.autograd.Function):
    """Camera.create_rays (camera.py:155-171) with the pose differentiable: (R [3,3], T [3]) -> (ray_dir, ray_orig) [B,3].
    `cam` is the POD descriptor built from the same R and T; the intrinsics are not differentiated."""

    @staticmethod
    def forward(ctx, hip: Context, uv: Tensor, cam, R: Tensor, T: Tensor):
        rd, ro = hip.raygen(uv, cam)
        ctx.hip, ctx.cam = hip, cam
        ctx.save_for_backward(uv)
        return rd, ro

    @staticmethod
    def backward(ctx, g_rd, g_ro):
        with torch.cuda.device(g_rd.device):
            g_R, g_T = ctx.hip.raygen_backward(ctx.saved_tensors[0], ctx.cam, g_rd, g_ro)
        return None, None, None, g_R, g_T


class RayTableFunction(torch.autograd.Function):
    """Ray generation with a camera per row (ViewRays) and every pose differentiable: (uv [B,2], view [B], table [K,16]) ->
    (ray_dir, ray_orig) [B,3].  The gradient of `table` is [K,16]: columns 0..11 are (g_R row-major, g_T) of each camera over its
    own rows, one launch for all cameras; columns 12..15 are zero, the intrinsics are not differentiated."""

    @staticmethod
    def forward(ctx, hip: Context, uv: Tensor, view: Tensor, table: Tensor):
        rd, ro = hip.raygen(ViewRays(uv, view, table))
        ctx.hip = hip
        ctx.save_for_backward(uv, view, table)
        return rd, ro

    @staticmethod
    def backward(ctx, g_rd, g_ro):
        uv, view, table = ctx.saved_tensors
        with torch.cuda.device(g_rd.device):
            g = ctx.hip.raygen_backward(ViewRays(uv, view, table), None, g_rd, g_ro)
        return None, None, None, torch.nn.functional.pad(g, (0, 4))

