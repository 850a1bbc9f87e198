"""What the field kernels return for NaN and Inf, against the reference (tests/golden/nonfinite.npz, gen_nonfinite_goldens.py).

Eight 128-wide networks (NeDDF x 4, NeRF x 2, NeuS x 2; neddf_amd/fixtures/synth.py NONFINITE_*), 229 points = three 64-row tiles and
a ragged 37 with nine poisoned rows on both sides of every tile edge (NaN / +Inf / -Inf in a position, a direction or a variance
coordinate, var = +Inf), and four poisoned weights on the clean points.  Every operand policy -- fp32 under both
NEDDF_F32_PRODUCTS routes, f16_split, bf16 -- and, for NeDDF, both output modes:
  class      every element the fixture keeps has the reference's class (finite / NaN / +Inf / -Inf); bf16 has the fp32 exponent range
             and is held to the same classes
  value      the kept finite elements meet the 1e-4 rel + 1e-5 abs gate of test_neddf_synth / test_nerf_synth / test_neus_synth
             (fp32, f16_split) or the bf16 gates of test_gpu_c5.py against this library's fp32 result
  isolation  the clean rows are bit-identical to a run in which the poisoned rows carry clean values
  render     render_rays raises its NaN flag, falls back to the linspace in the chunk that the reference falls back in and nowhere
             else, and its pixels have the reference's classes
  training   forward classes, a NaN loss and NaN parameter gradients where the reference has them
The switch NEDDF_F32_PRODUCTS is read once per process, so both routes run in subprocesses of this file, once per module.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE, os.path.join(HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import synth  # noqa: E402

CASES = ["input"] + list(synth.NONFINITE_WEIGHT_POISONS)
# (route of the fp32 products = worker process, weight_dtype)
POLICIES = [("mfma", "fp32"), ("split3", "fp32"), ("mfma", "f16_split"), ("mfma", "bf16")]
NET_MODES = [(n, m) for n, (kind, _) in synth.NONFINITE_NETS.items() for m in (("full", "minimal") if kind == "neddf" else ("full",))]
TRAIN_NETS = ("neddf_relu", "nerf_relu")
RENDER_CASES = ("nanweights", "nanray", "clean")


def _keys(kind, mode):
    return tuple(k for k in synth.FIELD_KEYS[kind] if not (mode == "minimal" and k == "fields_penalty"))


def _worker(out):
    import torch

    import neddf_amd
    from conftest import golden
    from neddf_amd import Sampling
    dev = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    g = golden("nonfinite.npz")
    dtypes = [d for r, d in POLICIES if r == os.environ["NEDDF_F32_PRODUCTS"]]
    res = {}
    clean, bad = synth.nonfinite_inputs()
    cls = {"neddf": neddf_amd.NeDDF, "nerf": neddf_amd.NeRF, "neus": neddf_amd.NeuS}

    def module(name, poison):
        kind, kw = synth.NONFINITE_NETS[name]
        net = cls[kind](**kw)
        net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.nonfinite_state(name, poison).items()})
        return net.to(dev)

    with torch.no_grad():
        for name, (kind, kw) in synth.NONFINITE_NETS.items():
            for case in CASES + ["clean"]:
                net = module(name, case if case in synth.NONFINITE_WEIGHT_POISONS else None)
                net.set_iter(-1)
                smp = Sampling(*[T(a) for a in (bad if case == "input" else clean)])
                for dtype in dtypes:
                    net.weight_dtype = dtype
                    for mode in ("full", "minimal") if kind == "neddf" else ("full",):
                        if kind == "neddf":
                            net.output_mode = mode
                        o = net(smp)
                        torch.cuda.synchronize()
                        for k in _keys(kind, mode):
                            res["%s/%s/%s/%s/%s" % (dtype, name, mode, case, k)] = o[k].cpu().numpy()

        # ---- render_rays over neddf_relu: 8 rays, nan_group = the fixture's chunk
        kind, kw = synth.NONFINITE_NETS["neddf_relu"]
        B, chunk, Sc, Sf = g["r_uv"].shape[0], int(g["r_chunk"]), int(g["r_sample_coarse"]), int(g["r_sample_fine"])
        for case in RENDER_CASES:
            r = neddf_amd.NeRFRender(dict(kw, _target_="neddf.network.NeDDF"), sample_coarse=Sc, sample_fine=Sf, dist_near=2.0, dist_far=6.0,
                                     max_dist=6.0, use_coarse_network=False, sampling_type="cone")
            r.network_fine.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in
                                            synth.nonfinite_state("neddf_relu", "trunk_nan" if case == "nanweights" else None).items()})
            r.to(dev)
            r.set_iter(-1)
            cam = neddf_amd.Camera(neddf_amd.PinholeCalib(g["r_calib"].astype(np.float64)), None).to(dev)
            cam.R, cam.T = T(g["r_R"]), T(g["r_T"])
            U_c, U_f = T(g["r_nanray_u_coarse"] if case == "nanray" else g["r_u_coarse"]), T(g["r_u_fine"])
            for dtype in [d for d in dtypes if d != "f16_split"]:
                r.network_fine.weight_dtype = r.network_coarse.weight_dtype = dtype
                ctx = r._ctx(dev)
                S2 = Sc + Sf + 2
                buf = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
                o = dict(color=buf(B, 3), depth=buf(B), transmittance=buf(B), weight=buf(B, S2 - 1), color_coarse=buf(B, 3), depth_coarse=buf(B),
                         transmittance_coarse=buf(B), weight_coarse=buf(B, Sc), fields_penalty=buf(B), fields_penalty_coarse=buf(B),
                         dists_coarse=buf(B, Sc + 1), dists_fine=buf(B, S2))
                flag = torch.zeros(1, dtype=torch.int32, device=dev)
                ctx.render_rays(T(g["r_uv"]), cam.descriptor(), r._params(chunk, 0), U_c, U_f, dict(o, nan_flag=flag))
                torch.cuda.synchronize()
                for k, v in o.items():
                    res["render/%s/%s/%s" % (dtype, case, k)] = v.cpu().numpy()
                res["render/%s/%s/_nan" % (dtype, case)] = flag.cpu().numpy()

    # ---- training: the autograd route over the layer-by-layer kernels, poisoned points, set_iter(2500)
    for name in TRAIN_NETS:
        kind, _ = synth.NONFINITE_NETS[name]
        ups = synth.nonfinite_upstream(kind)
        for dtype in [d for d in dtypes if d != "bf16"]:
            net = module(name, None)
            net.weight_dtype = dtype
            net.set_iter(2500)
            with torch.enable_grad():
                o = net(Sampling(*[T(a) for a in bad]))
                loss = sum((o[k] * T(ups[k])).sum() for k in ups)
                loss.backward()
            torch.cuda.synchronize()
            pre = "train/%s/%s/" % (dtype, name)
            for k in ups:
                assert o[k].requires_grad
                res[pre + "out_" + k] = o[k].detach().cpu().numpy()
            res[pre + "loss"] = loss.detach().cpu().numpy()
            for k, p in net.named_parameters():
                res[pre + "grad_" + k] = p.grad.cpu().numpy()
    np.savez(out, **res)


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    d = tmp_path_factory.mktemp("nonfinite")
    out = {}
    for route in ("mfma", "split3"):
        path = str(d / (route + ".npz"))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "worker", path], env=dict(os.environ, NEDDF_F32_PRODUCTS=route), cwd=ROOT,
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, route + p.stdout[-3000:] + p.stderr[-3000:]
        z = np.load(path)
        out[route] = {k: z[k] for k in z.files}
    return out


@pytest.fixture(scope="module")
def g():
    from conftest import golden
    z = golden("nonfinite.npz")
    return {k: z[k] for k in z.files}


def _same_class(have, want, keep, what):
    cg, cw = synth.float_class(have), synth.float_class(want)
    bad = keep & (cg != cw)
    print("%-60s %5d kept, reference %4d NaN %3d Inf, %d differ" % (what, int(keep.sum()), int((keep & (cw == 1)).sum()), int((keep & (cw >= 2)).sum()),
                                                                     int(bad.sum())))
    if bad.any():
        return "%s: class differs on %d elements, first at %s: got %s, reference %s" % (
            what, int(bad.sum()), tuple(int(i) for i in np.argwhere(bad)[0]), have[bad][:4], want[bad][:4])
    return None


def _none_failed(msgs):
    msgs = [m for m in msgs if m]
    assert not msgs, "%d checks failed:\n  " % len(msgs) + "\n  ".join(msgs)


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", NET_MODES)
@pytest.mark.parametrize("route,dtype", POLICIES)
def test_nonfinite_classes(routes, g, route, dtype, name, mode):
    kind, _ = synth.NONFINITE_NETS[name]
    msgs = []
    for case in CASES:
        for k in _keys(kind, mode):
            pre = "%s/%s/eval/" % (name, case)
            have = routes[route]["%s/%s/%s/%s/%s" % (dtype, name, mode, case, k)].reshape(g[pre + k].shape)
            msgs.append(_same_class(have, g[pre + k], g[pre + "keep_" + k], "%s %s %s %s %s %s" % (route, dtype, name, mode, case, k)))
    _none_failed(msgs)


def _bf16_gate(have, f32, kind, k, what):
    """test_gpu_c5.py's gates of the bf16 policy against this library's fp32 result: test_operand_policies_on_other_widths_and_activations
    (NeDDF), test_nerf_operand_policies_on_other_widths (NeRF), test_bf16_neus_close_to_fp32 (NeuS)."""
    e = np.abs(have - f32) / max(float(np.abs(f32).max()), 1e-3)
    print("%-60s bf16 vs fp32 / range: max %.3g, 99th percentile %.3g, median %.3g" % (what, e.max(), np.percentile(e, 99), np.median(e)))
    if kind == "neddf" and k in ("distance", "aux_grad"):
        assert float(e.max()) < 1e-2, what
    elif kind == "neddf" and k in ("density", "color"):
        assert float(np.percentile(e, 99)) < 5e-2 and float(np.median(e)) < 5e-3 and float(e.max()) < 0.25, what
    elif kind == "nerf":
        assert float(e.max()) < 3e-2, what
    elif kind == "neus":
        assert float(e.max()) < (0.25 if k == "color" else 5e-2), what


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", NET_MODES)
@pytest.mark.parametrize("route,dtype", POLICIES)
def test_nonfinite_values(routes, g, route, dtype, name, mode):
    from conftest import close
    kind, _ = synth.NONFINITE_NETS[name]
    checked = 0
    for case in CASES:
        for k in _keys(kind, mode):
            pre = "%s/%s/eval/" % (name, case)
            want = g[pre + k]
            have = routes[route]["%s/%s/%s/%s/%s" % (dtype, name, mode, case, k)].reshape(want.shape)
            fin = g[pre + "keep_" + k] & np.isfinite(want)
            what = "%s %s %s %s %s %s" % (route, dtype, name, mode, case, k)
            assert np.isfinite(have[fin]).all(), what
            if not fin.any():
                continue
            checked += 1
            if dtype == "bf16":
                if kind == "neddf" and k == "fields_penalty":      # not gated under bf16 by test_gpu_c5.py either; its class is
                    continue
                f32 = routes["mfma"]["fp32/%s/%s/%s/%s" % (name, mode, case, k)].reshape(want.shape)
                both = fin & np.isfinite(f32)
                _bf16_gate(have[both], f32[both], kind, k, what)
            else:
                ok, mabs, mrel = close(have[fin], want[fin], 1e-4, 1e-5)
                print("%-60s %5d finite, max abs %.3e, max rel %.3e" % (what, int(fin.sum()), mabs, mrel))
                assert ok, "%s: max abs %.3e, max rel %.3e (rtol 1e-4 atol 1e-5)" % (what, mabs, mrel)
    assert checked >= len(_keys(kind, mode))          # the input case and the colour-only poison leave finite values on every key


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", NET_MODES)
@pytest.mark.parametrize("route,dtype", POLICIES)
def test_nonfinite_rows_stay_with_their_own_point(routes, route, dtype, name, mode):
    """The clean rows of the poisoned batch, bit for bit what they are when the nine poisoned rows carry clean values."""
    kind, _ = synth.NONFINITE_NETS[name]
    rest = np.setdiff1d(np.arange(synth.NONFINITE_POINTS), synth.NONFINITE_ROWS)
    for k in _keys(kind, mode):
        a = routes[route]["%s/%s/%s/input/%s" % (dtype, name, mode, k)]
        b = routes[route]["%s/%s/%s/clean/%s" % (dtype, name, mode, k)]
        assert np.isfinite(b).all(), (k, "the clean run is not finite")
        assert np.array_equal(a[rest], b[rest]), "%s %s %s %s %s: a poisoned row changed %d other rows" % (
            route, dtype, name, mode, k, int((a[rest] != b[rest]).reshape(len(rest), -1).any(1).sum()))


PIXEL_KEYS = ("color", "depth", "transmittance", "weight", "color_coarse", "depth_coarse", "transmittance_coarse", "weight_coarse",
              "fields_penalty", "fields_penalty_coarse")


@pytest.mark.gpu
@pytest.mark.parametrize("route,dtype", [p for p in POLICIES if p[1] != "f16_split"])
def test_nonfinite_render_rays(routes, g, route, dtype):
    """render_rays in chunks of 4 rays (nan_group) over (a) the network with a NaN weight and (b) the clean network with a NaN in the
    coarse uniforms of ray 5.  integrate_volume_render asserts on a NaN weight (base_neural_render.py:155), which the library reports
    as its NaN flag: the reference raises in both chunks of (a) and in the second chunk of (b).  The expected outputs are those of the
    reference with the assert statements compiled out: in (a) sample_pdf zeroes the NaN weights (:52-55) and draws from the flat pdf --
    NO fallback, the samples are finite -- and every pixel is NaN; in (b) the NaN distance reaches the sorted samples and the second
    chunk falls back to the linspace of its first ray (:105-114), after which its fine pass is finite."""
    z = routes[route]
    chunk = int(g["r_chunk"])
    assert g["r_nanweights_asserts"].tolist() == [True, True] and g["r_nanray_asserts"].tolist() == [False, True]
    assert g["r_nanweights_fallback"].tolist() == [False, False] and g["r_nanray_fallback"].tolist() == [False, True]
    get = lambda case, k: z["render/%s/%s/%s" % (dtype, case, k)]
    assert int(get("clean", "_nan")[0]) == 0
    msgs = []
    for case in ("nanweights", "nanray"):
        if int(get(case, "_nan")[0]) == 0:
            msgs.append("%s: the NaN flag is not raised" % case)
        for k in PIXEL_KEYS:
            want = g["r_%s_out_%s" % (case, k)]
            msgs.append(_same_class(get(case, k).reshape(want.shape), want, np.ones(want.shape, bool), "render %s %s %s %s" % (route, dtype, case, k)))
    _none_failed(msgs)
    if dtype == "bf16":
        return
    for case in ("nanweights", "nanray"):
        dc, df = get(case, "dists_coarse"), get(case, "dists_fine")
        assert np.array_equal(dc, g["r_%s_dists_coarse" % case], equal_nan=True)
        for c, fell in enumerate(g["r_%s_fallback" % case]):
            rows = slice(c * chunk, (c + 1) * chunk)
            if fell:    # the 1e-6 allowance of test_nan_fallback_has_chunk_granularity: torch's CPU linspace differs in its last bit between hosts
                lin = np.linspace(np.float32(dc[c * chunk, 0]), np.float32(dc[c * chunk, -1]), df.shape[1], dtype=np.float64)
                assert np.abs(df[rows] - lin[None]).max() <= 1e-6, (case, c, float(np.abs(df[rows] - lin[None]).max()))
                assert np.abs(df[rows] - g["r_%s_dists_fine" % case][rows]).max() <= 1e-6
                assert np.array_equal(df[rows], np.broadcast_to(df[c * chunk], df[rows].shape))
            elif case == "nanray":
                assert np.array_equal(df[rows], get("clean", "dists_fine")[rows]), "a chunk without a NaN differs from the clean run"
                for k in PIXEL_KEYS:
                    assert np.array_equal(get(case, k)[rows], get("clean", k)[rows]), k
            else:       # zero weights, the same uniforms and knots: the flat-pdf samples of the reference, within the same 2 ulp
                assert np.isfinite(df[rows]).all()
                assert np.abs(df[rows] - g["r_%s_dists_fine" % case][rows]).max() <= 1e-6, float(np.abs(df[rows] - g["r_%s_dists_fine" % case][rows]).max())


@pytest.mark.gpu
@pytest.mark.parametrize("name", TRAIN_NETS)
@pytest.mark.parametrize("route,dtype", [p for p in POLICIES if p[1] != "bf16"])
def test_nonfinite_training_step(routes, g, route, dtype, name):
    """Training-mode forward and backward on the poisoned points: the forward's classes, a NaN loss, and NaN in every element of a
    parameter gradient in which the reference has NaN."""
    kind, _ = synth.NONFINITE_NETS[name]
    z, pre, gpre = routes[route], "train/%s/%s/" % (dtype, name), "t_%s_" % name
    msgs = []
    for k in synth.FIELD_KEYS[kind]:
        want = g[gpre + "out_" + k]
        msgs.append(_same_class(z[pre + "out_" + k].reshape(want.shape), want, np.ones(want.shape, bool), "train %s %s %s %s" % (route, dtype, name, k)))
    assert np.isnan(g[gpre + "loss"])
    if not np.isnan(z[pre + "loss"]):
        msgs.append("the loss is %s, the reference's is NaN" % z[pre + "loss"])
    names = json.loads(str(g[gpre + "param_names"]))
    assert any((g[gpre + "gclass_" + k] == 1).any() for k in names)
    for k in names:
        want_nan = g[gpre + "gclass_" + k] == 1
        have = z[pre + "grad_" + k].reshape(want_nan.shape)
        miss = want_nan & ~np.isnan(have)
        if miss.any():
            msgs.append("%s %s %s gradient of %s: %d of the %d elements the reference has NaN in are not, %s ..." % (
                route, dtype, name, k, int(miss.sum()), int(want_nan.sum()), have[miss][:4]))
    _none_failed(msgs)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "worker":
        _worker(sys.argv[2])
