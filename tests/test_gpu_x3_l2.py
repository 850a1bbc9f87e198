"""NEDDF_X3_L2 (neddf_capi.hip field_forward, tile_engine.h OpsF32x3L2T) switches the three-term fp32 distance kernel's L2 residency
mechanisms: `stream` (y' and the parked encoding gradient are read back non-temporal; the default), `wb` (a write-back of an XCD's
L2 every NEDDF_X3_L2_PERIOD of its tiles) and `both`.  A cache policy and a write-back touch no value: every setting must
reproduce setting `0`, the plain kernel, bit for bit.

Each setting runs in a fresh subprocess of this file (all started together), on the shipped network and a 128-wide synthetic one:
neddf_field_forward outputs at N = 1, 63, 64, 65 and 64 x 1024 + 17 points (more than two tiles for each of the 512 workgroups, so
a period-1 write-back fires in every workgroup between tiles and on the ragged last tile), render_rays at (B, S) = (3, 128) and
(65, 3), and `0` against `both` once more at NEDDF_FIELD_CHUNK_LOG2=16, where three launches follow each other on the stream.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

KEYS = ("distance", "density", "color")
SIZES = (1, 63, 64, 65, 64 * 1024 + 17)
RAYS = ((3, 128), (65, 3))
# name -> environment on top of the caller's
SETTINGS = {
    "0": dict(NEDDF_X3_L2="0"),
    "stream": dict(NEDDF_X3_L2="stream"),
    "wb": dict(NEDDF_X3_L2="wb", NEDDF_X3_L2_PERIOD="1"),
    "both": dict(NEDDF_X3_L2="both", NEDDF_X3_L2_PERIOD="1"),
    "chunk16/0": dict(NEDDF_X3_L2="0", NEDDF_FIELD_CHUNK_LOG2="16"),
    "chunk16/both": dict(NEDDF_X3_L2="both", NEDDF_X3_L2_PERIOD="1", NEDDF_FIELD_CHUNK_LOG2="16"),
}


def _worker(out, chunked):
    import torch

    import neddf_amd
    from neddf_amd import Sampling
    from neddf_amd._lib import SLOT_FINE
    from neddf_amd.fixtures import BUNNY_SMOKE_CFG, BUNNY_SMOKE_RENDER, bunny_smoke_weights, synth
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    res = {}
    c = BUNNY_SMOKE_CFG
    nets = {"shipped": (dict(c), bunny_smoke_weights()),
            "w128": (dict(c, ddf_layer_width=128, col_layer_width=128),
                     dict(synth.neddf_state(c["embed_pos_rank"], c["embed_dir_rank"], c["ddf_layer_count"], 128, c["col_layer_count"], 128,
                                            tuple(c["skips"]), seed=7)))}
    # the chunked pair: one batch of 2 x 2^16 + 17 points = three launches of each kernel
    sizes = (2 * 65536 + 17,) if chunked else SIZES
    for name, (cfg, wts) in nets.items():
        render = neddf_amd.NeRFRender(dict(cfg, _target_="neddf.network.NeDDF"), **BUNNY_SMOKE_RENDER)
        render.network_fine.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in wts.items()})
        render.to(dev)
        render.set_iter(-1)
        net = render.network_fine
        net.output_mode = "minimal"
        for n in sizes:
            pos, d, var = synth.random_sampling(1, n, seed=100 + n % 97)
            o = net(Sampling(T(pos), T(d), T(var)))
            torch.cuda.synchronize()
            for k in KEYS:
                res["%s/field/%d/%s" % (name, n, k)] = o[k].cpu().numpy()
        if name != "shipped" or chunked:
            continue
        g = np.load(os.path.join(HERE, "golden", "bunny_stages.npz"))      # pose and calibration of the reference's own 64 rays
        cam = neddf_amd.Camera(neddf_amd.PinholeCalib(g["calib"].astype(np.float64)), None).to(dev)
        cam.R, cam.T = torch.from_numpy(g["R"]).to(dev), torch.from_numpy(g["T"]).to(dev)
        ctx = render._ctx(dev)
        for B, S in RAYS:
            gen = torch.Generator(device="cpu").manual_seed(B * 1000 + S)
            uv = torch.stack([torch.randint(150, 350, (B,), generator=gen), torch.randint(150, 350, (B,), generator=gen)], 1).to(dev)
            U = torch.rand(B, S, generator=gen).to(dev)
            o = dict(color=torch.empty(B, 3, device=dev), depth=torch.empty(B, device=dev), transmittance=torch.empty(B, device=dev))
            flag = torch.zeros(1, device=dev, dtype=torch.int32)
            ctx.render_rays(uv, cam.descriptor(), render._params(), U, None, dict(o, nan_flag=flag), single_slot=SLOT_FINE)
            torch.cuda.synchronize()
            for k, v in o.items():
                res["shipped/rays/%dx%d/%s" % (B, S, k)] = v.cpu().numpy()
    np.savez(out, **res)


@pytest.fixture(scope="module")
def settings(tmp_path_factory):
    d = tmp_path_factory.mktemp("x3_l2")
    procs = {}
    for name, extra in SETTINGS.items():
        path = str(d / (name.replace("/", "_") + ".npz"))
        env = dict(os.environ, **extra)
        env.pop("NEDDF_F32_PRODUCTS", None)        # the default route: three-term products
        if "NEDDF_FIELD_CHUNK_LOG2" not in extra:
            env.pop("NEDDF_FIELD_CHUNK_LOG2", None)
        procs[name] = (path, subprocess.Popen([sys.executable, os.path.abspath(__file__), "worker", path, "chunked" if "chunk16" in name else "whole"],
                                              env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    out, failed = {}, []
    for name, (path, p) in procs.items():
        try:
            log, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            p.kill()
            log, _ = p.communicate()
            log += "\n(timed out)"
        if p.returncode != 0:
            failed.append("%s: exit %s\n%s" % (name, p.returncode, log[-3000:]))
            continue
        z = np.load(path)
        out[name] = {k: z[k] for k in z.files}
    assert not failed, "\n".join(failed)
    return out


def _same(a, b):
    assert sorted(a) == sorted(b) and a, (sorted(a), sorted(b))
    bad = [k for k in sorted(a) if a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]
    assert not bad, "outputs differ from setting 0 in %s" % bad


@pytest.mark.gpu
@pytest.mark.parametrize("setting", ["stream", "wb", "both"])
def test_l2_setting_is_bit_identical_to_the_plain_kernel(settings, setting):
    ref = settings["0"]
    assert all(np.isfinite(v).all() for v in ref.values())
    assert len(ref) == 2 * len(SIZES) * len(KEYS) + 3 * len(RAYS)
    _same(ref, settings[setting])


@pytest.mark.gpu
def test_l2_setting_is_bit_identical_over_consecutive_launches(settings):
    _same(settings["chunk16/0"], settings["chunk16/both"])


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "worker":
        _worker(sys.argv[2], sys.argv[3] == "chunked")
