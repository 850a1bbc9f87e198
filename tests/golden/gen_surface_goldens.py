#!/usr/bin/env python3
"""Golden vectors of the surface-normal outputs (tests/golden/surface_normals.npz).  Like gen_pose_goldens.py this runs only where
the reference checkout exists; it drives the reference's own modules and stores inputs and results, data only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_surface_goldens.py

Records
  field level  f_<case>_*   NeDDF.forward (neddf.py:162-309) on the shipped bunny network and two synthetic ones (two skips / LeakyReLU):
                            pos, dir, var (half of the points with cone variances, half with zero variance, a share of them close
                            to the origin, i.e. inside the object), distance, density, color and the two values the forward computes
                            on the way and does not return -- distance_grad (neddf.py:223) and norm_dir (:241).  distance_grad is
                            captured by wrapping SoftplusGradFunction.apply in the reference module's namespace, norm_dir is :235 and
                            :241 restated on it with the reference's own torch ops.  The same from the reference run in float64
                            (suffix 64).
  NeuS         f_neus_*     NeuS.forward (neus.py:101-162): sdf, density, color and `gradients` (:135-143), captured by wrapping
                            torch.autograd.grad; float64 likewise
  render       r_*          NeRFRender.render_rays on 16 rays of bunny_stages.npz (its uniforms): per-sample norm_dir of both passes,
                            the weights `color` is integrated with (the coarse ones before sample_pdf sanitises them in place),
                            and sum_j w n accumulated in float64
The normal is ill-conditioned where |distance_grad| is small; the generator asserts that the propagated gate of the tests,
2 (1e-4 |g| + 1e-5) / (|g| + 1e-7) + 1e-6, exceeds 0.1 on at most 5 % of the points of every case.
"""
import os

import numpy as np
import torch
import yaml

from gen_goldens import HERE, REF, npy, save, synth

import neddf.network.neddf as ref_neddf  # noqa: E402
from neddf.network import NeDDF, NeuS  # noqa: E402
from neddf.ray import Sampling  # noqa: E402
from neddf.render import NeRFRender  # noqa: E402


class _SoftplusTap:
    """Stands in for SoftplusGradFunction inside neddf.network.neddf: same apply, and keeps distance_grad of every call."""

    def __init__(self, inner):
        self.inner, self.grads = inner, []

    def apply(self, x, J):
        out = self.inner.apply(x, J)
        self.grads.append(out[1][:, :, 0].detach().clone())
        return out


def _norm_dir(g):
    return torch.reciprocal(torch.norm(g, dim=1)[:, None] + 1e-7) * g       # neddf.py:235,241


def tapped(fn):
    """fn() with the tap installed -> (result, [distance_grad per NeDDF.forward call])."""
    tap = _SoftplusTap(ref_neddf.SoftplusGradFunction)
    ref_neddf.SoftplusGradFunction = tap
    try:
        out = fn()
    finally:
        ref_neddf.SoftplusGradFunction = tap.inner
    return out, tap.grads


def inputs(rays, samples, seed):
    pos, dd, var = synth.random_sampling(rays, samples, seed=seed, cone=True)
    rng = np.random.default_rng(seed + 7)
    var[rays // 2:] = 0.0                                   # half cone samples, half point samples
    inside = rng.random((rays, samples)) < 0.25             # a quarter close to the origin: inside the bunny / small distances
    pos[inside] *= np.float32(0.15)
    return pos, dd, var


def check_conditioning(tag, g):
    n = np.linalg.norm(g.astype(np.float64), axis=-1)
    gate = 2 * (1e-4 * n + 1e-5) / (n + 1e-7) + 1e-6
    frac = float((gate > 0.1).mean())
    print("  %s: |g| min %.3e median %.3e, normal gate > 0.1 on %.2f %% of the points" % (tag, n.min(), np.median(n), 100 * frac))
    assert frac <= 0.05, (tag, frac)


def field_case(arrs, tag, make, iteration, rays, samples, seed):
    pos, dd, var = inputs(rays, samples, seed)
    pre = "f_%s_" % tag
    arrs.update({pre + "pos": pos, pre + "dir": dd, pre + "var": var, pre + "iteration": np.int32(iteration)})
    for dt, sfx in ((torch.float32, ""), (torch.float64, "64")):
        torch.set_default_dtype(dt)
        try:
            m = make(dt)
            m.set_iter(iteration)
            smp = Sampling(*[torch.from_numpy(a).to(dt) for a in (pos, dd, var)])
            o, grads = tapped(lambda: m(smp))
        finally:
            torch.set_default_dtype(torch.float32)
        assert len(grads) == 1
        g = grads[0]
        for k in ("distance", "density", "color"):
            arrs[pre + k + sfx] = npy(o[k])
        arrs[pre + "distance_grad" + sfx] = npy(g).reshape(rays, samples, 3)
        arrs[pre + "norm_dir" + sfx] = npy(_norm_dir(g)).reshape(rays, samples, 3)
    check_conditioning(tag, arrs[pre + "distance_grad"])


def bunny_parts():
    cfg = yaml.safe_load(open(os.path.join(REF, "pretrained/bunny_smoke/.hydra/config.yaml")))
    sd = torch.load(os.path.join(REF, "pretrained/bunny_smoke/models/model_02000.pth"), map_location="cpu")
    return cfg, sd


def gen_fields(arrs):
    cfg, sd = bunny_parts()
    ncfg = dict(cfg["network"])              # the shipped configuration as it is (neddf_amd.fixtures.BUNNY_SMOKE_CFG)
    ncfg.pop("_target_")

    def bunny(dt):
        net = NeDDF(**ncfg)
        net.load_state_dict({k[len("network_fine."):]: v.to(dt) for k, v in sd.items() if k.startswith("network_fine.")})
        return net

    field_case(arrs, "bunny", bunny, -1, 32, 48, 401)
    for tag, iteration, kw in (("skips2", -1, dict(embed_pos_rank=6, embed_dir_rank=3, ddf_layer_count=6, col_layer_count=3, skips=[1, 3],
                                                    activation_type="ReLU", density_activation_type="LeakyReLU")),
                               ("leaky", 2500, dict(embed_pos_rank=10, embed_dir_rank=4, ddf_layer_count=8, col_layer_count=4, skips=[4],
                                                    activation_type="LeakyReLU", density_activation_type="tanhExp"))):
        def synthetic(dt, kw=kw):
            net = NeDDF(ddf_layer_width=256, col_layer_width=256, d_near=0.01, lowpass_alpha_offset=10, **kw)
            net.load_state_dict({k: torch.from_numpy(v).to(dt) for k, v in synth.neddf_state(
                embed_pos_rank=kw["embed_pos_rank"], embed_dir_rank=kw["embed_dir_rank"], ddf_layer_count=kw["ddf_layer_count"],
                col_layer_count=kw["col_layer_count"], skips=tuple(kw["skips"]), seed=29).items()})
            return net

        arrs["f_%s_config" % tag] = np.array(__import__("json").dumps(kw))
        field_case(arrs, tag, synthetic, iteration, 12, 32, 411)


NEUS_KW = dict(embed_pos_rank=6, embed_dir_rank=4, sdf_layer_count=8, sdf_layer_width=256, col_layer_count=4, col_layer_width=256,
               init_variance=0.3, activation_type="tanhExp", skips=[4])


def gen_neus(arrs):
    """tanhExp: with ReLU the sdf gradient is piecewise constant and a kink within rounding of a sample flips a whole term."""
    kw = NEUS_KW
    rays, samples = 12, 32
    pos, dd, var = inputs(rays, samples, 421)
    pre = "f_neus_"
    arrs.update({pre + "pos": pos, pre + "dir": dd, pre + "var": var, pre + "config": np.array(__import__("json").dumps(kw))})
    for dt, sfx in ((torch.float32, ""), (torch.float64, "64")):
        torch.set_default_dtype(dt)
        taken = []
        real = torch.autograd.grad

        def tap(*a, **k):
            out = real(*a, **k)
            taken.append(out[0].detach().clone())
            return out

        try:
            net = NeuS(**kw)
            sd = synth.neus_state(kw["embed_pos_rank"], kw["embed_dir_rank"], kw["sdf_layer_count"], kw["sdf_layer_width"],
                                  kw["col_layer_count"], kw["col_layer_width"], tuple(kw["skips"]), kw["init_variance"], seed=19)
            net.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(dt) for k, v in sd.items()})
            torch.autograd.grad = tap
            with torch.enable_grad():
                o = net(Sampling(*[torch.from_numpy(a.copy()).to(dt) for a in (pos, dd, var)]))
        finally:
            torch.autograd.grad = real
            torch.set_default_dtype(torch.float32)
        assert len(taken) == 1
        for k in ("sdf", "density", "color"):
            arrs[pre + k + sfx] = npy(o[k])
        arrs[pre + "gradients" + sfx] = npy(taken[0]).reshape(rays, samples, 3)


def gen_render(arrs):
    cfg, sd = bunny_parts()
    rcfg = dict(cfg["render"])
    rcfg.pop("_target_")
    render = NeRFRender(network_config=cfg["network"], **rcfg)
    render.load_state_dict(sd)
    render.set_iter(-1)
    g = np.load(os.path.join(HERE, "bunny_stages.npz"))
    n = 16
    uv = torch.from_numpy(g["uv"][:n])
    from neddf.camera import Camera, PinholeCalib
    cam = Camera(PinholeCalib(g["calib"].astype(np.float64)), np.zeros(6, np.float32))
    cam.R, cam.T = torch.from_numpy(g["R"]), torch.from_numpy(g["T"])
    u_c, u_f = torch.from_numpy(g["u_coarse"][:n]), torch.from_numpy(g["u_fine"][:n])
    draws = [u_c, u_f]
    real = torch.rand
    torch.rand = lambda *a, **k: draws.pop(0)              # the two draws of render_rays (nerf_render.py:137, base_neural_render.py:75)
    # the weights as integrate_volume_render computes them -- the ones `color` is integrated with.  The coarse ones come back from
    # render_rays SANITISED: sample_pdf zeroes negative weights in place (base_neural_render.py:52-55), and the shipped network's
    # LeakyReLU density does go negative
    raw = []
    integrate = render.integrate_volume_render

    def integrate_tap(*a, **k):
        o = integrate(*a, **k)
        raw.append(o["weight"].detach().clone())
        return o

    render.integrate_volume_render = integrate_tap
    try:
        out, grads = tapped(lambda: render.render_rays(uv, cam))
    finally:
        torch.rand = real
        del render.integrate_volume_render
    assert not draws and len(grads) == 2 and len(raw) == 2
    Sc1, S2 = render.sample_coarse + 1, render.sample_coarse + render.sample_fine + 2
    n_c = npy(_norm_dir(grads[0])).reshape(n, Sc1, 3)
    n_f = npy(_norm_dir(grads[1])).reshape(n, S2, 3)
    arrs.update(r_uv=g["uv"][:n], r_R=g["R"], r_T=g["T"], r_calib=g["calib"], r_u_coarse=g["u_coarse"][:n], r_u_fine=g["u_fine"][:n],
                r_sample_coarse=np.int32(render.sample_coarse), r_sample_fine=np.int32(render.sample_fine),
                r_norm_dir_coarse=n_c, r_norm_dir=n_f)
    for k in ("weight", "weight_coarse", "color", "depth", "transmittance"):
        arrs["r_" + k] = npy(out[k])
    assert torch.equal(raw[1], out["weight"])
    arrs["r_weight_coarse_raw"] = npy(raw[0])
    print("  render: coarse weights, raw min %.3e, returned (sanitised) min %.3e" % (float(raw[0].min()), float(out["weight_coarse"].min())))
    w_f, w_c = npy(raw[1]).astype(np.float64), npy(raw[0]).astype(np.float64)
    arrs["r_normal64"] = np.einsum("bj,bjk->bk", w_f, n_f[:, :-1].astype(np.float64))
    arrs["r_normal_coarse64"] = np.einsum("bj,bjk->bk", w_c, n_c[:, :-1].astype(np.float64))
    print("  render: |normal| max %.4f, 1 - T min %.4f" % (np.linalg.norm(arrs["r_normal64"], axis=1).max(),
                                                          (1 - arrs["r_transmittance"]).min()))


def main():
    arrs = {}
    gen_fields(arrs)
    gen_neus(arrs)
    gen_render(arrs)
    save("surface_normals.npz", **arrs)
    size = os.path.getsize(os.path.join(HERE, "surface_normals.npz"))
    assert size < (1 << 20), "fixture over the 1 MiB limit of a committed file: %d B" % size


if __name__ == "__main__":
    main()
