#!/usr/bin/env python3
"""Golden vectors of the fields' NaN / Inf propagation (tests/golden/nonfinite.npz).  Like gen_surface_goldens.py this runs only
where the reference checkout exists; it drives the reference's own modules and stores inputs and results, data only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_nonfinite_goldens.py

Everything that defines a case lives in neddf_amd/fixtures/synth.py (NONFINITE_*): eight 128-wide networks (NeDDF x 4, NeRF x 2,
NeuS x 2), 229 points with nine poisoned rows (NaN / +Inf / -Inf in a position, a direction or a variance coordinate, var = +Inf in
all three coordinates, the latter with a NaN position), and four poisoned weights on the clean points.

Records, per network <net> and case <case> (`input` or the name of a weight poison):
  <net>/<case>/<mode>/<key>        the reference's fp32 output; mode `eval` (set_iter(-1)) and, for NeDDF, `train` (set_iter(2500))
  <net>/<case>/<mode>/keep_<key>   True where the class of the element (finite / NaN / +Inf / -Inf) is the same in the reference run
                                   in fp32 and in fp64 (torch default dtype float64: same code, same weights)
  pos, dir, var                    the poisoned points (the clean ones are synth.nonfinite_inputs()[0])
  t_<net>_*                        training: loss = sum_k (o[k] * upstream[k]).sum() on the poisoned points at set_iter(2500),
                                   loss.backward(); the forward's outputs, the loss and the class of every element of every parameter gradient
  r_<case>_*                       NeRFRender.render_rays over `neddf_relu`, 8 rays in chunks of 4 (one call per chunk, as render_image
                                   makes them), 16 coarse + 16 fine cone samples: (a) `nanweights`, the trunk_nan network, (b)
                                   `nanray`, the clean network with one NaN in the coarse uniforms of ray 5.  integrate_volume_render
                                   asserts that no weight is NaN (base_neural_render.py:155), so the reference as it stands raises on
                                   both; `r_<case>_asserts` records that per chunk, and the outputs are those of the same code with the
                                   assert statements compiled out (this script re-run under `python -O`).  dists_coarse / dists_fine are
                                   sample_pdf's input and output, `fallback` says per chunk whether it took the linspace branch (:105-114).
The caps below are conditions on the fixture, not measurements of any kernel: `keep` may drop at most 1 % of the elements of a case,
and every poisoned row keeps at least one element of every output key.
"""
import json
import os
import subprocess
import sys

import numpy as np
import torch

from gen_goldens import HERE, npy, synth

from neddf.camera import Camera, PinholeCalib  # noqa: E402
from neddf.network import NeDDF, NeRF, NeuS  # noqa: E402
from neddf.ray import Sampling  # noqa: E402
from neddf.render import NeRFRender  # noqa: E402

CLS = {"neddf": NeDDF, "nerf": NeRF, "neus": NeuS}
OUT = "nonfinite.npz"
RENDER_RAYS, RENDER_CHUNK, RENDER_COARSE, RENDER_FINE = 8, 4, 16, 16


def make(kind, kw, sd, dtype):
    net = CLS[kind](**kw)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in sd.items()})
    return net


def forward(kind, net, pts, dtype, grad=False):
    smp = Sampling(*[torch.from_numpy(a.copy()).to(dtype) for a in pts])
    with torch.set_grad_enabled(grad or kind == "neus"):          # NeuS takes its normal from torch.autograd.grad
        return net(smp)


def field_case(arrs, name, case, sd, pts, rows):
    kind, kw = synth.NONFINITE_NETS[name]
    modes = (("eval", -1), ("train", 2500)) if kind == "neddf" else (("eval", -1),)
    dropped = total = 0
    for mode, it in modes:
        out = {}
        for dtype in (torch.float32, torch.float64):
            torch.set_default_dtype(dtype)
            try:
                net = make(kind, kw, sd, dtype)
                net.set_iter(it)
                out[dtype] = {k: npy(v) for k, v in forward(kind, net, pts, dtype).items()}
            finally:
                torch.set_default_dtype(torch.float32)
        assert tuple(out[torch.float32]) == synth.FIELD_KEYS[kind], tuple(out[torch.float32])
        for k, v in out[torch.float32].items():
            assert v.dtype == np.float32 and out[torch.float64][k].dtype == np.float64
            keep = synth.float_class(v) == synth.float_class(out[torch.float64][k])
            pre = "%s/%s/%s/" % (name, case, mode)
            arrs[pre + k], arrs[pre + "keep_" + k] = v, keep
            dropped += int((~keep).sum())
            total += keep.size
            for r in rows:
                assert keep[r].any(), "%s: row %d keeps no element of %s" % (pre, r, k)
    assert dropped <= 0.01 * total, "%s/%s: keep drops %d of %d elements" % (name, case, dropped, total)
    cls = synth.float_class(arrs["%s/%s/eval/%s" % (name, case, synth.FIELD_KEYS[kind][0])])
    print("  %-14s %-14s dropped %d of %d; %s: %d NaN, %d Inf of %d" % (name, case, dropped, total, synth.FIELD_KEYS[kind][0],
                                                                        int((cls == 1).sum()), int((cls >= 2).sum()), cls.size))


def gen_fields(arrs):
    clean, bad = synth.nonfinite_inputs()
    arrs.update(pos=bad[0], dir=bad[1], var=bad[2], rows=np.array(synth.NONFINITE_ROWS, np.int32))
    for name in synth.NONFINITE_NETS:
        field_case(arrs, name, "input", synth.nonfinite_state(name), bad, synth.NONFINITE_ROWS)
        for poison in synth.NONFINITE_WEIGHT_POISONS:
            field_case(arrs, name, poison, synth.nonfinite_state(name, poison), clean, ())


def gen_train(arrs):
    _, bad = synth.nonfinite_inputs()
    for name in ("neddf_relu", "nerf_relu"):
        kind, kw = synth.NONFINITE_NETS[name]
        net = make(kind, kw, synth.nonfinite_state(name), torch.float32)
        net.set_iter(2500)
        ups = synth.nonfinite_upstream(kind)
        with torch.enable_grad():
            net.zero_grad()
            o = forward(kind, net, bad, torch.float32, grad=True)
            loss = sum((o[k] * torch.from_numpy(ups[k])).sum() for k in ups)
            loss.backward()
        pre = "t_%s_" % name
        arrs[pre + "loss"] = npy(loss)
        for k in ups:
            arrs[pre + "out_" + k] = npy(o[k])
        names = []
        for k, p in net.named_parameters():
            names.append(k)
            arrs[pre + "gclass_" + k] = synth.float_class(npy(p.grad))
        arrs[pre + "param_names"] = np.array(json.dumps(names))
        nan = sum(int((arrs[pre + "gclass_" + k] == 1).all()) for k in names)
        print("  train %-12s loss %s; %d of %d parameter gradients are NaN in every element" % (name, arrs[pre + "loss"], nan, len(names)))


# ---------------------------------------------------------------------------------------------------------------- render cases
def render_inputs():
    rng = np.random.default_rng(61)
    uv = np.stack([np.arange(RENDER_RAYS) * 9 + 280, np.arange(RENDER_RAYS) * 7 + 210], 1).astype(np.int64)
    u_c = rng.uniform(0, 1, (RENDER_RAYS, RENDER_COARSE + 1)).astype(np.float32)
    u_f = rng.uniform(0, 1, (RENDER_RAYS, RENDER_FINE + 1)).astype(np.float32)
    calib = np.array([400.0, 400.0, 320.0, 240.0])
    pose = np.array([0.02, 0.04, 0.06, 0.1, 0.2, -4.0], np.float32)
    return uv, u_c, u_f, calib, pose


def render_cases():
    """case -> (weight poison or None, coarse uniforms)"""
    uv, u_c, u_f, calib, pose = render_inputs()
    bad = u_c.copy()
    bad[5, 3] = np.nan
    return {"nanweights": ("trunk_nan", u_c), "nanray": (None, bad), "clean": (None, u_c)}


def render_run(arrs):
    """Runs the three render configurations with whatever this interpreter does about assert statements."""
    uv, _, u_f, calib, pose = render_inputs()
    kind, kw = synth.NONFINITE_NETS["neddf_relu"]
    for case, (poison, u_c) in render_cases().items():
        render = NeRFRender(network_config=dict(kw, _target_="neddf.network.NeDDF"), sample_coarse=RENDER_COARSE, sample_fine=RENDER_FINE,
                            dist_near=2.0, dist_far=6.0, max_dist=6.0, use_coarse_network=False, sampling_type="cone")
        render.network_fine.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.nonfinite_state("neddf_relu", poison).items()})
        render.set_iter(-1)
        cam = Camera(PinholeCalib(calib), pose)
        taps = []
        inner = render.sample_pdf

        def tap(dists, weights, n, cat_coarse=True):
            out = inner(dists, weights, n, cat_coarse)
            taps.append((dists.detach().clone(), out.detach().clone()))
            return out

        render.sample_pdf = tap
        real = torch.rand
        outs, raised = [], []
        try:
            for lo in range(0, RENDER_RAYS, RENDER_CHUNK):
                draws = [torch.from_numpy(u_c[lo:lo + RENDER_CHUNK].copy()), torch.from_numpy(u_f[lo:lo + RENDER_CHUNK].copy())]
                torch.rand = lambda *a, **k: draws.pop(0)          # nerf_render.py:137, base_neural_render.py:75
                try:
                    outs.append(render.render_rays(torch.from_numpy(uv[lo:lo + RENDER_CHUNK]), cam))
                    raised.append(False)
                except AssertionError:
                    raised.append(True)
        finally:
            torch.rand = real
        pre = "r_%s_" % case
        arrs[pre + "asserts"] = np.array(raised)
        if not any(raised):
            for k in outs[0]:
                arrs[pre + "out_" + k] = np.concatenate([npy(o[k]) for o in outs])
            arrs[pre + "dists_coarse"] = np.concatenate([npy(t[0]) for t in taps])
            arrs[pre + "dists_fine"] = np.concatenate([npy(t[1]) for t in taps])
            arrs[pre + "fallback"] = np.array([bool((t[1] == t[1][:1]).all()) and t[1].shape[0] > 1 for t in taps])
        arrs.update(r_R=npy(cam.R), r_T=npy(cam.T))


def gen_render(arrs):
    uv, u_c, u_f, calib, pose = render_inputs()
    arrs.update(r_uv=uv, r_u_coarse=u_c, r_u_fine=u_f, r_calib=calib.astype(np.float32), r_nanray_u_coarse=render_cases()["nanray"][1],
                r_chunk=np.int32(RENDER_CHUNK), r_sample_coarse=np.int32(RENDER_COARSE), r_sample_fine=np.int32(RENDER_FINE))
    here = {}
    render_run(here)
    for case in render_cases():
        arrs["r_%s_asserts" % case] = here["r_%s_asserts" % case]
    assert not here["r_clean_asserts"].any()
    tmp = os.path.join(HERE, "_nonfinite_render_tmp.npz")
    try:            # the same code with the assert statements compiled out
        subprocess.check_call([sys.executable, "-O", os.path.abspath(__file__), "render", tmp], env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
        z = np.load(tmp)
        for k in z.files:
            if k.endswith("_asserts"):
                assert not z[k].any(), k
            else:
                arrs[k] = z[k]
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    for k in [k for k in here if k.startswith("r_clean_")]:       # the clean run is the same with and without assert statements
        assert np.array_equal(here[k], arrs[k]), k
    for case in render_cases():
        print("  render %-10s asserts per chunk %s, sample_pdf fell back per chunk %s, colour classes %s" % (
            case, arrs["r_%s_asserts" % case].tolist(), arrs["r_%s_fallback" % case].tolist(),
            synth.float_class(arrs["r_%s_out_color" % case]).max(1).tolist()))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "render":
        arrs = {}
        render_run(arrs)
        np.savez(sys.argv[2], **arrs)
        return
    arrs = {}
    gen_fields(arrs)
    gen_train(arrs)
    gen_render(arrs)
    path = os.path.join(HERE, OUT)
    np.savez_compressed(path, **arrs)          # mostly NaN patterns and masks: compresses to a fraction
    size = os.path.getsize(path)
    print("wrote %s (%.1f KB)" % (OUT, size / 1024))
    assert size < 400 * 1024, "fixture larger than intended: %d B" % size


if __name__ == "__main__":
    main()
