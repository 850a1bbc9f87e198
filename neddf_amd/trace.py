"""Sphere tracing of a distance field (not a reference feature: the reference renders by volume integration only).

A ray o + t d marches from t_near towards the level set D = threshold: where the distance is d it advances by
max(step_scale * (d - threshold), min_step).  For a 1-Lipschitz D and step_scale <= 1 such a step never crosses the level
set; a trained NeDDF distance is only roughly 1-Lipschitz, and step_scale < 1 is the knob for that -- no
default has been tuned.  Per ray (include/neddf_hip.h, "sphere tracing"):

    t         current depth                      status  ACTIVE 0, HIT 1 (D(t) <= threshold), MISS 2 (t passed t_far),
    t_lo      last depth with D > threshold              EXHAUSTED 3 (still active after max_steps), INVALID 4 (non-finite
    steps     advances taken                             ray or a NaN distance)
    distance  last distance read

After the march the HIT rays are refined by `refine` bisection rounds of [t_lo, t], which keep D(t) <= threshold < D(t_lo).
Every kernel step is restated in numpy by tests/trace_check.py, bit for bit.
"""
from typing import Callable, NamedTuple, Optional

import torch
from torch import Tensor

from ._lib import Context, NeddfError, TraceParams

ACTIVE, HIT, MISS, EXHAUSTED, INVALID = 0, 1, 2, 3, 4
MAX_STEPS, MAX_REFINE = 4096, 32


class TraceResult(NamedTuple):
    t: Tensor               # float32 [n]
    t_lo: Tensor            # float32 [n]
    status: Tensor          # uint8 [n]
    steps: Tensor           # int32 [n]
    distance: Tensor        # float32 [n]
    evaluations: int        # points the distance was evaluated at, the refinement included


def default_min_step(t_near: float, t_far: float) -> float:
    """(t_far - t_near) * 2**-10: a march of least steps crosses the range in 1024 advances.  A documented choice, not a tuned value."""
    return (float(t_far) - float(t_near)) * 2.0 ** -10


def trace_params(threshold: float, t_near: float, t_far: float, max_steps: int = 64, step_scale: float = 1.0,
                 min_step: Optional[float] = None, refine: int = 4) -> TraceParams:
    """The validated neddf_trace_params of a run (the library checks the same ranges)."""
    threshold, t_near, t_far, step_scale = float(threshold), float(t_near), float(t_far), float(step_scale)
    if threshold != threshold:
        raise ValueError("threshold must be a number (got NaN)")
    if not t_near < t_far:
        raise ValueError("t_near < t_far is required (got %r, %r)" % (t_near, t_far))
    if not 0.0 < step_scale <= 1.0:
        raise ValueError("step_scale must lie in (0, 1] (got %r)" % step_scale)
    min_step = default_min_step(t_near, t_far) if min_step is None else float(min_step)
    if not min_step > 0.0:
        raise ValueError("min_step must be positive (got %r)" % min_step)
    if int(max_steps) != max_steps or not 1 <= int(max_steps) <= MAX_STEPS:
        raise ValueError("max_steps must be an integer in [1, %d] (got %r)" % (MAX_STEPS, max_steps))
    if int(refine) != refine or not 0 <= int(refine) <= MAX_REFINE:
        raise ValueError("refine must be an integer in [0, %d] (got %r)" % (MAX_REFINE, refine))
    p = TraceParams()
    p.threshold, p.t_near, p.t_far, p.step_scale, p.min_step = threshold, t_near, t_far, step_scale, min_step
    p.max_steps, p.refine = int(max_steps), int(refine)
    return p


def _check_rays(origins: Tensor, dirs: Tensor) -> None:
    if not isinstance(origins, Tensor) or not isinstance(dirs, Tensor):
        raise ValueError("origins and dirs must be tensors")
    if origins.dim() != 2 or origins.shape[1] != 3 or dirs.shape != origins.shape:
        raise ValueError("origins and dirs must both be [n, 3] (got %s, %s)" % (tuple(origins.shape), tuple(dirs.shape)))
    if not origins.is_cuda or dirs.device != origins.device:
        raise NeddfError("origins and dirs must live on one HIP device (got %s, %s); there is no CPU fallback" % (origins.device, dirs.device))


def sphere_trace(origins: Tensor, dirs: Tensor, distance_fn: Callable[[Tensor], Tensor], *, threshold: float, t_near: float,
                 t_far: float, max_steps: int = 64, step_scale: float = 1.0, min_step: Optional[float] = None,
                 refine: int = 4) -> TraceResult:
    """Traces the rays origins + t * dirs ([n, 3] each, on a HIP device) against any distance_fn(pos [M, 3]) -> D [M] on that
    device, built from the library's stage entry points: per iteration the ACTIVE rays are compacted (one stream
    synchronise tells the host how many), distance_fn sees their points only, and the loop ends when none is left.
    min_step=None means default_min_step(t_near, t_far)."""
    p = trace_params(threshold, t_near, t_far, max_steps, step_scale, min_step, refine)
    _check_rays(origins, dirs)
    if not callable(distance_fn):
        raise ValueError("distance_fn must be callable: pos [M, 3] -> distances [M]")
    ctx = Context.get(origins.device)
    evaluations = 0

    def distances(pos: Tensor) -> Tensor:
        nonlocal evaluations
        D = distance_fn(pos)
        if not isinstance(D, Tensor) or D.numel() != pos.shape[0] or D.device != pos.device:
            raise ValueError("distance_fn must return one distance per point on the points' device")
        evaluations += pos.shape[0]
        return D

    with torch.no_grad():
        st = ctx.trace_begin(origins, dirs, p.t_near)
        for _ in range(p.max_steps):
            index, pos = ctx.trace_compact(origins, dirs, st)
            if index.shape[0] == 0:
                break
            ctx.trace_advance(index, distances(pos), st, p.threshold, p.step_scale, p.min_step, p.t_far)
        ctx.trace_finish(st)
        for _ in range(p.refine):
            index, pos = ctx.trace_bisect_points(origins, dirs, st)
            if index.shape[0] == 0:
                break
            ctx.trace_bisect_update(index, distances(pos), st, p.threshold)
    return TraceResult(st["t"], st["t_lo"], st["status"], st["steps"], st["distance"], evaluations)
