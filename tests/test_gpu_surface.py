"""Surface normals on the GPU: the field's position gradient and normal against the reference (tests/golden/surface_normals.npz,
written by gen_surface_goldens.py), the normal render target, and normals / colours on extracted meshes.

The measured figures are printed; with NEDDF_SURFACE_PROFILE=<path> in the environment they are also written there as JSON (that is how
profiles/surface_normals_parity.json is produced)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
from conftest import BUNNY_CFG, GOLDEN, assert_close, golden

import mesh_check as mc
import surface_check as sc
import synth

pytestmark = pytest.mark.gpu

FIGURES = {}


def _record(key, value):
    FIGURES[key] = value
    path = os.environ.get("NEDDF_SURFACE_PROFILE")
    if path:
        with open(path, "w") as fh:
            json.dump(FIGURES, fh, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g():
    d = golden("surface_normals.npz")
    return {k: d[k] for k in d.files}


def _freeze(net, dev, iteration=-1):
    net.to(dev)
    net.set_iter(int(iteration))
    for p in net.parameters():
        p.requires_grad_(False)
    return net


def _neddf(case, g, dev, dtype="fp32"):
    from neddf_amd import NeDDF
    from neddf_amd.fixtures import bunny_smoke_weights
    if case == "bunny":
        net = NeDDF(**BUNNY_CFG)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in bunny_smoke_weights().items()})
    else:
        kw = json.loads(str(g["f_%s_config" % case]))
        net = NeDDF(ddf_layer_width=256, col_layer_width=256, d_near=0.01, lowpass_alpha_offset=10, **kw)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.neddf_state(
            embed_pos_rank=kw["embed_pos_rank"], embed_dir_rank=kw["embed_dir_rank"], ddf_layer_count=kw["ddf_layer_count"],
            col_layer_count=kw["col_layer_count"], skips=tuple(kw["skips"]), seed=29).items()})
    net.weight_dtype = dtype
    return _freeze(net, dev, g["f_%s_iteration" % case])


@pytest.fixture(scope="module")
def bunny(g, dev):
    return _neddf("bunny", g, dev)


def _smp(g, pre, dev):
    from neddf_amd.ray import Sampling
    return Sampling(*[torch.from_numpy(g[pre + k]).to(dev) for k in ("pos", "dir", "var")])


def N(t):
    return t.detach().cpu().numpy()


def _field_gate(a, b):
    return np.abs(a.astype(np.float64) - b) - (1e-4 * np.abs(b) + 1e-5)


@pytest.mark.parametrize("mode", ["minimal", "full"])
@pytest.mark.parametrize("dtype", ["fp32", "f16_split"])
@pytest.mark.parametrize("case", ["bunny", "skips2", "leaky"])
def test_field_gradient_and_normal_vs_reference(g, dev, case, dtype, mode):
    """distance_grad at the project's field gate 1e-4 |ref| + 1e-5 against the reference's fp32 values (the product route of fp32 fields
    is fixed per process: the default one runs here).  Where the shipped bunny network misses that gate, the rule of the density gate
    (test_gpu_parity.py: error against the float64 fixture <= 1.5 x the reference's own fp32-vs-float64 error on the same points) applies
    instead, and the measured ratio is recorded.  The normal is gated by propagation: per component
    |n - n_ref| <= 2 (1e-4 |g_ref| + 1e-5) / (|g_ref| + 1e-7) + 1e-6."""
    pre = "f_%s_" % case
    net = _neddf(case, g, dev, dtype)
    net.output_mode = mode
    with torch.no_grad():
        o = net.forward_surface(_smp(g, pre, dev))
    assert set(o) == {"distance", "density", "color", "aux_grad", "distance_grad", "normal"} | ({"fields_penalty"} if mode == "full" else set())
    got, ref, ref64 = N(o["distance_grad"]), g[pre + "distance_grad"].astype(np.float64), g[pre + "distance_grad64"]
    assert got.shape == ref.shape
    over = float(_field_gate(got, ref).max())
    e_hip = float(np.abs(got.astype(np.float64) - ref64).max())
    e_ref = float(np.abs(ref - ref64).max())
    ratio = e_hip / e_ref
    print("%s %s %s: distance_grad max |err| vs fp32 reference %.3e (gate excess %.3e); vs float64 %.3e, reference's own %.3e, ratio %.3f"
          % (case, dtype, mode, float(np.abs(got - ref).max()), over, e_hip, e_ref, ratio))
    _record("gradient_%s_%s_%s" % (case, dtype, mode), dict(max_abs_err_vs_ref32=float(np.abs(got - ref).max()), field_gate_excess=over,
                                                           err_vs_float64=e_hip, reference_fp32_vs_float64=e_ref, ratio=ratio))
    if over > 0 and case == "bunny":
        assert e_hip <= 1.5 * e_ref, (case, dtype, mode, e_hip, e_ref)
    else:
        assert over <= 0, (case, dtype, mode, over)
    gn = np.linalg.norm(ref, axis=-1, keepdims=True)
    bound = 2 * (1e-4 * gn + 1e-5) / (gn + 1e-7) + 1e-6
    assert float((bound > 0.1).mean()) <= 0.05           # the gate stays meaningful on the fixture's points
    nerr = np.abs(N(o["normal"]).astype(np.float64) - g[pre + "norm_dir"])
    print("   normal: max |err| %.3e, max err / bound %.3f" % (float(nerr.max()), float((nerr / bound).max())))
    assert (nerr <= bound).all(), (case, dtype, mode, float((nerr / bound).max()))
    for k in ("distance", "density", "color"):
        assert_close(N(o[k]), g[pre + k], 1e-4, 3e-4 if k == "density" else 1e-5, "%s %s" % (case, k))


@pytest.mark.parametrize("mode", ["minimal", "full"])
@pytest.mark.parametrize("dtype", ["fp32", "f16_split", "bf16"])
def test_normal_is_the_gradient_normalised_and_other_outputs_do_not_move(g, dev, dtype, mode):
    net = _neddf("bunny", g, dev, dtype)
    net.output_mode = mode
    with torch.no_grad():
        s = net.forward_surface(_smp(g, "f_bunny_", dev))
        f = net(_smp(g, "f_bunny_", dev))
    for k in f:
        assert torch.equal(s[k].view(torch.int32), f[k].view(torch.int32)), (dtype, mode, k)       # bit for bit
    gr = N(s["distance_grad"]).astype(np.float64)
    want = gr / (np.linalg.norm(gr, axis=-1, keepdims=True) + 1e-7)
    err = float(np.abs(N(s["normal"]) - want).max())
    print("%s %s: max |normal - g / (|g| + 1e-7)| = %.3e" % (dtype, mode, err))
    assert err <= 1e-6, (dtype, mode, err)


def test_bf16_normals_are_finite_and_unit(g, dev):
    """Not gated against the reference, like the rest of that policy: finite, unit length where the gradient is not tiny, and the
    median cosine to the fp32 normal is recorded."""
    with torch.no_grad():
        b = _neddf("bunny", g, dev, "bf16").forward_surface(_smp(g, "f_bunny_", dev))
        f = _neddf("bunny", g, dev, "fp32").forward_surface(_smp(g, "f_bunny_", dev))
    for k, v in b.items():
        assert torch.isfinite(v).all(), k
    n, gr = N(b["normal"]).astype(np.float64), N(b["distance_grad"]).astype(np.float64)
    big = np.linalg.norm(gr, axis=-1) > 1e-3
    assert big.any() and float(np.abs(np.linalg.norm(n, axis=-1) - 1)[big].max()) <= 1e-3
    cos = (n * N(f["normal"])).sum(-1)
    _record("bf16_median_cosine_to_fp32_normal", float(np.median(cos)))
    print("bf16: median cosine to the fp32 normal %.6f, min %.4f" % (float(np.median(cos)), float(cos.min())))


def _neus(g, dev):
    from neddf_amd import NeuS
    kw = json.loads(str(g["f_neus_config"]))
    net = NeuS(**kw)
    sd = synth.neus_state(kw["embed_pos_rank"], kw["embed_dir_rank"], kw["sdf_layer_count"], kw["sdf_layer_width"],
                          kw["col_layer_count"], kw["col_layer_width"], tuple(kw["skips"]), kw["init_variance"], seed=19)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return _freeze(net, dev)


def test_neus_gradient_vs_reference(g, dev):
    """The sdf gradient the reference takes by autograd (neus.py:135-143) at the field gate; NeuS hands that gradient, un-normalised,
    to its colour trunk (neus.py:144-145), so `normal` is the same array."""
    net = _neus(g, dev)
    with torch.no_grad():
        o = net.forward_surface(_smp(g, "f_neus_", dev))
        f = net(_smp(g, "f_neus_", dev))
    assert set(o) == {"sdf", "density", "color", "distance_grad", "normal"}
    got, ref = N(o["distance_grad"]), g["f_neus_gradients"].astype(np.float64)
    over = float(_field_gate(got, ref).max())
    print("neus: gradient max |err| %.3e, |g| max %.3e, gate excess %.3e" % (float(np.abs(got - ref).max()), float(np.abs(ref).max()), over))
    _record("gradient_neus", dict(max_abs_err_vs_ref32=float(np.abs(got - ref).max()), field_gate_excess=over,
                                  err_vs_float64=float(np.abs(got - g["f_neus_gradients64"]).max()),
                                  reference_fp32_vs_float64=float(np.abs(ref - g["f_neus_gradients64"]).max())))
    assert over <= 0, over
    assert torch.equal(o["normal"], o["distance_grad"])
    for k in f:
        assert torch.equal(o[k], f[k]), k


def _nerf(dev):
    from neddf_amd import NeRF
    net = NeRF()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.nerf_state(seed=11).items()})
    return _freeze(net, dev)


def test_nerf_fields_refuse(dev):
    from neddf_amd import Context
    from neddf_amd.ray import Sampling
    net = _nerf(dev)
    ctx = Context.get(dev)
    net.upload(ctx, net._slot)
    p = torch.zeros(4, 3, device=dev)
    out = torch.zeros(4, 3, device=dev)
    vp = lambda t: C.c_void_p(t.data_ptr())
    rc = ctx.lib.neddf_field_forward_surface(ctx.h, net._slot, vp(p), vp(p), vp(p), 4, 0, None, None, None, None, None, vp(out), None, ctx.stream())
    assert rc == -3 and b"NeRF" in ctx.lib.neddf_last_error(ctx.h)
    with torch.no_grad(), pytest.raises(NotImplementedError):
        net.forward_surface(Sampling(p[None], p[None], p[None]))


def test_forward_surface_is_inference_only(bunny, g, dev):
    with torch.enable_grad(), pytest.raises(RuntimeError, match="no_grad"):
        bunny.forward_surface(_smp(g, "f_bunny_", dev))


# ------------------------------------------------------------------------------------------------------------ render level
def _bunny_render(dev, g, density=None):
    """The shipped network in the reference's render configuration.  density="ReLU" replaces its LeakyReLU density activation: the
    weights of the volume integral are then non-negative, which is what the bound |normal| <= 1 - transmittance presupposes."""
    import neddf_amd
    from neddf_amd.fixtures import bunny_smoke_weights
    cfg = dict(BUNNY_CFG, _target_="neddf.network.NeDDF")
    if density:
        cfg["density_activation_type"] = density
    r = neddf_amd.NeRFRender(cfg, sample_coarse=int(g["r_sample_coarse"]), sample_fine=int(g["r_sample_fine"]), dist_near=2.0, dist_far=6.0,
                             max_dist=6.0, use_coarse_network=False, sampling_type="cone")
    r.network_fine.load_state_dict({k: torch.from_numpy(v) for k, v in bunny_smoke_weights().items()})
    r.to(dev)
    r.set_iter(-1)
    for p in r.parameters():
        p.requires_grad_(False)
    cam = neddf_amd.Camera(neddf_amd.PinholeCalib(g["r_calib"].astype(np.float64)), None).to(dev)
    cam.R, cam.T = torch.from_numpy(g["r_R"]).to(dev), torch.from_numpy(g["r_T"]).to(dev)
    return r, cam


def _bits_equal(a, b, keys, what):
    for k in keys:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (what, k)


def test_render_rays_normal_vs_fixture(g, dev):
    """The fused renderer on the fixture's rays and uniforms: normal / normal_coarse against sum_j w n accumulated in float64 from the
    reference's weights and per-sample norm_dir, at the colour gate; everything else bit-identical with the target on and off.

    |normal| <= 1 - transmittance + 1e-5 presupposes non-negative weights (sum_j w_j = 1 - T, then the triangle inequality).  The
    shipped network's density activation is LeakyReLU: its densities and weights do go negative, and on nearly empty rays the bound
    is missed with it (measured on the MI355X: |normal| = 8e-4 .. 2.8e-3 against 1 - T = 5e-4 .. 5.4e-3 on background pixels).  So the
    bound is asserted with the same weights under a ReLU density, where its premise holds, and with the shipped activation the
    inequality that holds for any sign, |normal| <= sum_j |w_j| + 1e-5, is asserted instead."""
    r, cam = _bunny_render(dev, g)
    ctx = r._ctx(dev)
    uv = torch.from_numpy(g["r_uv"]).to(dev)
    U_c, U_f = torch.from_numpy(g["r_u_coarse"]).to(dev), torch.from_numpy(g["r_u_fine"]).to(dev)
    off = r._render(ctx, uv, cam, U_c, U_f, full=True)
    on = r._render(ctx, uv, cam, U_c, U_f, full=True, normal=True)
    on2 = r._render(ctx, uv, cam, U_c, U_f, full=True, normal=True)
    torch.cuda.synchronize()
    assert set(on) - set(off) == {"normal", "normal_coarse"}
    _bits_equal(on, off, [k for k in off if k != "_nan"], "render_rays on / off")
    _bits_equal(on, on2, ["normal", "normal_coarse"], "two runs")
    for k in ("weight", "weight_coarse"):
        print("%s: max |GPU - reference| %.3e" % (k, float(np.abs(N(on[k]) - g["r_" + k]).max())))
    # the coarse pass stage by stage: per-sample normals of the stand-alone field entry at the same sample points
    from neddf_amd.ray import Sampling
    rd, ro = ctx.raygen(uv, cam.descriptor())
    dists_c = ctx.sample_coarse(U_c, 2.0, 6.0)
    smp = Sampling(*ctx.sampling(rd, ro, dists_c, r._params().ray_radius))
    with torch.no_grad():
        st = r.network_fine.forward_surface(smp)
    per = np.abs(N(st["normal"]) - g["r_norm_dir_coarse"])
    wref = np.concatenate([g["r_weight_coarse"], np.zeros((len(per), 1), np.float32)], 1)
    print("coarse per-sample normals, stand-alone entry vs reference: max |err| %.3e, weighted by the reference's weights %.3e"
          % (float(per.max()), float((per * wref[..., None]).sum(1).max())))
    staged = ctx.composite_normal(dists_c, st["density"], st["normal"])
    print("staged normal_coarse vs fused %.3e, vs fixture %.3e" % (float((staged - on["normal_coarse"]).abs().max()),
                                                                  float(np.abs(N(staged) - g["r_normal_coarse64"]).max())))
    for k in ("normal", "normal_coarse"):
        ref = g["r_%s64" % k]
        print("%s: max |err| %.3e" % (k, float(np.abs(N(on[k]) - ref).max())))
        assert_close(N(on[k]), ref, 1e-4, 1e-5, k)
    assert (on["normal"].double().norm(dim=1) <= on["weight"].double().abs().sum(1) + 1e-5).all()
    rr, _ = _bunny_render(dev, g, density="ReLU")
    pos = rr._render(rr._ctx(dev), uv, cam, U_c, U_f, full=True, normal=True)
    assert float(pos["weight"].min()) >= 0
    for k, t in (("normal", "transmittance"), ("normal_coarse", "transmittance_coarse")):
        assert (pos[k].double().norm(dim=1) <= 1 - pos[t].double() + 1e-5).all(), k
    assert_close(N(on["color"]), g["r_color"], 1e-4, 1e-5, "color")


def test_render_rays_attribute_and_keys(g, dev):
    r, cam = _bunny_render(dev, g)
    uv = torch.from_numpy(g["r_uv"]).to(dev)
    torch.manual_seed(5)
    off = r.render_rays(uv, cam)
    r.normal_output = True
    torch.manual_seed(5)
    on = r.render_rays(uv, cam)
    assert list(on)[:len(off)] == list(off) and list(on)[len(off):] == ["normal", "normal_coarse"]
    _bits_equal(on, off, list(off), "render_rays attribute")


def test_composite_normal_on_random_stages(dev):
    """The stand-alone compositor on the random integrate_volume_render inputs of stages_random.npz with random unit normals, against
    numpy float64 with the GPU's own weights -- and the weights / colour of the plain compositor are not touched."""
    from neddf_amd import Context
    ctx = Context.get(dev)
    d = golden("stages_random.npz")
    rng = np.random.default_rng(11)
    i, seen = 0, 0
    while "iv%d_dists" % i in d.files:
        dists, dens, col = (torch.from_numpy(d["iv%d_%s" % (i, k)]).to(dev) for k in ("dists", "dens", "col"))
        i += 1
        if not (np.isfinite(d["iv%d_weight" % (i - 1)]).all() and np.isfinite(d["iv%d_col" % (i - 1)]).all()):
            continue
        B, S = dists.shape
        n = rng.standard_normal((B, S, 3))
        n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
        nt = torch.from_numpy(n).to(dev)
        a = ctx.composite_normal(dists, dens, nt)
        b = ctx.composite_normal(dists, dens, nt)
        out, _ = ctx.composite(dists, dens, col, 6.0)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        w = N(out["weight"]).astype(np.float64)
        want = np.einsum("bj,bjk->bk", w, n[:, :-1].astype(np.float64))
        # fp32 accumulation: at most 3 terms per lane (S <= 130 here) and six butterfly additions, each product and sum rounded once:
        # below 10 roundings of 2^-24 relative to sum_j |w_j| -> 1e-6 of it, next to the colour gate on the value itself
        scale = np.abs(w).sum(1, keepdims=True)
        assert (np.abs(N(a) - want) <= 1e-4 * np.abs(want) + 1e-5 + 1e-6 * scale).all(), i - 1
        # the same kernel as a colour compositor: its weights are the plain compositor's
        c = ctx.composite_normal(dists, dens, col)
        assert_close(N(c), N(out["color"]), 1e-6, 1e-6, "composite_normal(colour) vs composite")
        seen += 1
    assert seen >= 3


def test_render_image_normal_target(g, dev):
    """A 20 x 13 frame in chunks of 64 (last chunk: 4 rays): targets with and without "normal" agree bit for bit, the normal equals the
    per-chunk render_rays loop with the same seed at the colour gate, and single-pass renders agree bit for bit on / off."""
    r, cam = _bunny_render(dev, g)
    w, h, chunk = 20, 13, 64
    torch.manual_seed(9)
    off = r.render_image(w, h, cam, ["color", "depth", "transmittance"], 1, chunk)
    torch.manual_seed(9)
    on = r.render_image(w, h, cam, ["color", "depth", "transmittance", "normal"], 1, chunk)
    assert on["normal"].shape == (h, w, 3)
    _bits_equal(on, off, list(off), "render_image on / off")
    us = torch.arange(w, device=dev).reshape(1, w).expand(h, w).reshape(-1)
    vs = torch.arange(h, device=dev).reshape(h, 1).expand(h, w).reshape(-1)
    uv = torch.stack([us, vs], 1)
    r.normal_output = True
    torch.manual_seed(9)
    parts = [r.render_rays(uv[b:b + chunk], cam) for b in range(0, w * h, chunk)]
    for k in ("normal", "color"):
        loop = torch.cat([p[k] for p in parts]).reshape(h, w, 3)
        # (at the colour gate, not bit for bit, as in test_gpu_parity.py::test_render_image_is_the_chunk_loop_over_render_rays: render_rays
        # also returns penalties, which takes the forward-mode field kernel, render_image the reverse-mode one -- the same function in
        # another summation order; a wrong pixel, chunk boundary or draw order would be off by O(1))
        assert_close(N(on[k]), N(loop), 1e-4, 1e-5, "render_image vs the chunk loop: " + k)
    U = torch.rand(w * h, 48).to(dev)
    a = r.render_image_single_pass(w, h, cam, 48, U=U)
    b = r.render_image_single_pass(w, h, cam, 48, U=U, normals=True)
    assert set(b) - set(a) == {"normal"} and b["normal"].shape == (w * h, 3)
    _bits_equal(a, b, ["color", "depth", "transmittance"], "single pass on / off")
    # the length bound where its premise (non-negative weights) holds: the same network under a ReLU density
    rr, _ = _bunny_render(dev, g, density="ReLU")
    torch.manual_seed(9)
    img = rr.render_image(w, h, cam, ["transmittance", "normal"], 1, chunk)
    assert (img["normal"].double().norm(dim=2) <= 1 - img["transmittance"][..., 0].double() + 1e-5).all()
    sp = rr.render_image_single_pass(w, h, cam, 48, U=U, normals=True)
    assert (sp["normal"].double().norm(dim=1) <= 1 - sp["transmittance"].double() + 1e-5).all()


def test_normal_target_refusals(g, dev):
    import neddf_amd
    from neddf_amd.parallel import render_image_sharded
    r, cam = _bunny_render(dev, g)
    with pytest.raises(NotImplementedError, match="normal"):
        render_image_sharded(r, 8, 8, cam, ["color", "normal"])
    nr = neddf_amd.NeRFRender(dict(_target_="neddf.network.NeRF"), sample_coarse=8, sample_fine=8, use_coarse_network=False)
    nr.network_fine.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.nerf_state(seed=11).items()})
    nr.to(dev)
    nr.set_iter(-1)
    with pytest.raises(NotImplementedError):
        nr.render_image(8, 8, cam, ["normal"])
    with pytest.raises(NotImplementedError):
        nr.render_image_single_pass(8, 8, cam, 8, normals=True)
    # the C entry itself
    ctx = nr._ctx(dev)
    uv = torch.zeros(4, 2, device=dev, dtype=torch.int64)
    with pytest.raises(neddf_amd.NeddfError, match="NeRF"):
        ctx.render_rays(uv, cam.descriptor(), nr._params(), torch.rand(4, 9, device=dev), torch.rand(4, 9, device=dev),
                        dict(normal=torch.empty(4, 3, device=dev)))


# -------------------------------------------------------------------------------------------------------------- mesh level
def test_bunny_mesh_normals_and_colors(bunny, dev):
    from neddf_amd.mesh import vertex_normals
    from oracle import oracle as orc
    from neddf_amd.fixtures import bunny_smoke_weights
    v, t, nf, col = bunny.extract_mesh(resolution=48, normals=True, colors=True)
    v0, t0 = bunny.extract_mesh(resolution=48)
    assert torch.equal(v, v0) and torch.equal(t, t0)
    assert nf.shape == v.shape and col.shape == v.shape
    assert float((nf.double().norm(dim=1) - 1).abs().max()) <= 1e-6
    v_, t_, ng = bunny.extract_mesh(resolution=48, normals="geometric")
    ng2 = vertex_normals(v, t)
    assert torch.equal(ng.view(torch.int32), ng2.view(torch.int32))          # bitwise repeatable
    vn, tn = N(v), N(t)
    sums = sc.normal_sums(vn, tn)
    length = np.linalg.norm(sums, axis=1)
    want = sc.vertex_normals(vn, tn)
    keep = length > 1e-6 * length.max()
    err = float(np.abs(N(ng) - want)[keep].max())
    print("bunny mesh: %d vertices; geometric normals kernel vs numpy max |err| %.3e" % (len(vn), err))
    assert keep.all() and err <= 1e-5
    # orientation: the field normal and the geometric normal point the same way on (nearly) every vertex; the yardstick is the float32
    # oracle's central-difference gradient of the distance (step 1e-3) against the numpy geometric normals
    net = orc.NeDDFOracle(bunny_smoke_weights(), **BUNNY_CFG)
    dirs = np.tile(np.array([1, 0, 0], np.float32), (len(vn), 1))
    zero = np.zeros_like(vn)
    grad = np.stack([(net.forward(vn + e, dirs, zero)["distance"].astype(np.float64) - net.forward(vn - e, dirs, zero)["distance"]) / 2e-3
                     for e in (np.eye(3, dtype=np.float32) * np.float32(1e-3))], 1)
    frac_oracle = float(((grad * want).sum(1) > 0).mean())
    frac_gpu = float(((N(nf).astype(np.float64) * N(ng)).sum(1) > 0).mean())
    print("field normal . geometric normal > 0: GPU %.4f of the vertices, float32 oracle (central differences) %.4f" % (frac_gpu, frac_oracle))
    _record("mesh_normal_agreement", dict(gpu=frac_gpu, oracle=frac_oracle, vertices=int(len(vn))))
    assert frac_gpu >= frac_oracle - 0.01
    # colours: the oracle's colour trunk fed the GPU's own normals
    ref = net.forward(vn, -N(nf), zero)["color"]
    assert_close(N(col), ref, 1e-4, 1e-5, "vertex colours vs oracle")


def test_nerf_density_mesh_gets_geometric_normals(dev):
    from oracle import oracle as orc
    net = _nerf(dev)
    from neddf_amd import Context
    ctx = Context.get(dev)
    net.upload(ctx, net._slot)
    vol = ctx.field_grid(net._slot, "density", (32,) * 3, (-1.1,) * 3, (1.1,) * 3)
    iso = float(vol.median())
    v, t, n, c = net.extract_mesh("density", iso, 1.1, 32, normals=True, colors=True)
    assert len(t) and n.shape == v.shape and c.shape == v.shape
    assert torch.equal(n.view(torch.int32), net.extract_mesh("density", iso, 1.1, 32, normals="geometric")[2].view(torch.int32))
    with pytest.raises(ValueError, match="geometric"):
        net.extract_mesh("density", iso, 1.1, 32, normals="field")
    want = sc.vertex_normals(N(v), N(t))
    length = np.linalg.norm(sc.normal_sums(N(v), N(t)), axis=1)
    keep = length > 1e-6 * length.max()
    assert float(np.abs(N(n) - want)[keep].max()) <= 1e-5
    ref = orc.NeRFOracle({k: np.asarray(a) for k, a in synth.nerf_state(seed=11).items()}).forward(N(v), -N(n), np.zeros_like(N(v)))["color"]
    assert_close(N(c), ref, 1e-4, 1e-5, "NeRF vertex colours vs oracle")


def test_mesh_normals_of_degenerate_input(dev):
    from neddf_amd.mesh import vertex_normals
    v = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [5, 5, 5]], device=dev, dtype=torch.float32)
    t = torch.tensor([[0, 1, 2], [0, 2, 1], [1, 2, 3], [0, 1, 99], [-1, 1, 2]], device=dev, dtype=torch.int32)     # two out-of-range rows: ignored
    n = N(vertex_normals(v, t))
    assert np.array_equal(n, sc.vertex_normals(N(v), N(t)[:3]))
    assert np.array_equal(n[0], [0, 0, 0]) and np.array_equal(n[4], [0, 0, 0])
    assert np.array_equal(N(vertex_normals(v, t[:0])), np.zeros((5, 3), np.float32))


def test_extract_mesh_script_flags(dev, bunny, tmp_path, capsys):
    import yaml
    from neddf_amd.fixtures import BUNNY_SMOKE_CFG, bunny_smoke_weights
    from neddf_amd.scripts.extract_mesh import main
    run = tmp_path / "run"
    (run / ".hydra").mkdir(parents=True)
    (run / "models").mkdir()
    cfg = {"dataset": {"_target_": "neddf.dataset.NeRFSyntheticDataset", "dataset_dir": os.path.join(GOLDEN, "bunny_mini"),
                       "data_split": "train", "use_depth": False, "use_mask": True},
           "render": {"_target_": "neddf.render.NeRFRender", "sample_coarse": 64, "sample_fine": 128, "dist_near": 2.0,
                      "dist_far": 6.0, "max_dist": 6.0, "use_coarse_network": False, "sampling_type": "cone"},
           "network": dict(BUNNY_SMOKE_CFG, _target_="neddf.network.NeDDF"),
           "trainer": {"_target_": "neddf.trainer.NeRFTrainer", "device": "cuda:0", "batch_size": 128, "chunk": 1024},
           "loss": {"functions": [{"_target_": "neddf.loss.ColorLoss", "weight": 1.0}]}}
    yaml.safe_dump(cfg, open(run / ".hydra" / "config.yaml", "w"))
    sd = {p + k: torch.from_numpy(a) for k, a in bunny_smoke_weights().items() for p in ("network_fine.", "network_coarse.")}
    torch.save(sd, run / "models" / "model_00007.pth")
    path = main([str(run), "--epoch", "7", "--resolution", "40"])
    v, t = mc.read_ply(path)                                # the plain file: 12 bytes per vertex
    v0, t0 = bunny.extract_mesh(resolution=40)
    assert np.array_equal(v, N(v0)) and np.array_equal(t, N(t0))
    path = main([str(run), "--epoch", "7", "--resolution", "40", "--normals", "--colors"])
    capsys.readouterr()
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    for prop in (b"property float nx", b"property uchar blue"):
        assert prop in head
    dt = np.dtype([("p", "<f4", (3,)), ("n", "<f4", (3,)), ("c", "u1", (3,))])
    rec = np.frombuffer(body[:len(v) * dt.itemsize], dtype=dt)
    v1, t1, n1, c1 = bunny.extract_mesh(resolution=40, normals=True, colors=True)
    assert np.array_equal(rec["p"], N(v1)) and np.array_equal(rec["n"], N(n1))
    assert np.array_equal(rec["c"], np.clip(np.rint(N(c1).astype(np.float64)[:, ::-1] * 255.0), 0, 255).astype(np.uint8))


def test_no_guard_band_written(dev, bunny, g):
    """One run of the field, render and mesh paths; under NEDDF_GUARD=1 every workspace sits between poisoned bands: none changed."""
    from neddf_amd import Context
    from neddf_amd._lib import guard_mode
    ctx = Context.get(dev)
    with torch.no_grad():
        bunny.forward_surface(_smp(g, "f_bunny_", dev))
    r, cam = _bunny_render(dev, g)
    r.render_image(12, 7, cam, ["color", "normal"], 1, 32)
    r.render_image_single_pass(12, 7, cam, 16, normals=True)
    out = bunny.extract_mesh(resolution=33, normals="geometric", colors=True)
    assert len(out[1])
    bands, bad = ctx.check_guards()
    assert bad == 0, (bands, bad)
    assert bands > 0 if guard_mode() else bands == 0
