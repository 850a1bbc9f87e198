"""The cases of the plain fp16 operand policy's accuracy check, shared by tests/test_gpu_f16_policy.py (which gates them) and
tools/time_f16_policy.py (which records them): eight networks of tests/golden/ at 257 points each, the modules that evaluate them and
the error figure.  257 = the fixture's 240 points and its first 17 again: four 64-row tiles and one point, two 128-row tiles and one."""
import json
import os

import numpy as np
import torch

import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

SIZES = (1, 63, 64, 65, 257)
N_MAX = SIZES[-1]
FACTOR = 0.5
CASES = {"bunny": "neddf", "neddf_w128": "neddf", "neddf_w384": "neddf", "neddf_skips2": "neddf", "nerf_w128": "nerf", "nerf_w384": "nerf",
         "neus_w128_384": "neus", "neus_tanhexp": "neus"}
MODES = {"neddf": ("full", "minimal"), "nerf": ("full",), "neus": ("full",)}
CASE_MODES = [(c, m) for c, k in CASES.items() for m in MODES[k]]


def golden(name):
    return np.load(os.path.join(GOLDEN, name))


def bunny():
    """(weights, stages) of the shipped network and the reference's own sample points for it"""
    from neddf_amd.fixtures import bunny_smoke_weights
    g = golden("bunny_stages.npz")
    return bunny_smoke_weights(), {k: g[k] for k in ("c_pos", "c_dir", "c_var")}


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def load(net, sd, dev):
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    net.to(dev)
    net.set_iter(-1)
    return net


def network_case(name, dev, bunny_weights, bunny_stages):
    """(kind, module, [257, 3] inputs, {output: fp64 values} where the fixtures hold them)"""
    import neddf_amd
    from neddf_amd.fixtures import BUNNY_SMOKE_CFG
    kind = CASES[name]
    if name == "bunny":
        g, g64 = bunny_stages, golden("bunny_field_fp64.npz")
        pts = [g["c_" + k].reshape(-1, 3)[:N_MAX] for k in ("pos", "dir", "var")]
        exact = {k: g64["c_" + k].reshape(-1)[:N_MAX] for k in ("distance", "density")}
        return kind, load(neddf_amd.NeDDF(**BUNNY_SMOKE_CFG), bunny_weights, dev), pts, exact
    g = golden(name + ".npz")
    kw = json.loads(str(g["config"]))
    rows = np.concatenate([np.arange(240), np.arange(N_MAX - 240)])
    pts = [g[k].reshape(-1, 3)[rows] for k in ("pos", "dir", "var")]
    exact = {}
    if kind == "neddf":
        sd = synth.neddf_state(kw["embed_pos_rank"], kw["embed_dir_rank"], kw["ddf_layer_count"], kw["ddf_layer_width"], kw["col_layer_count"],
                               kw["col_layer_width"], tuple(kw["skips"]), seed=7)
        net = neddf_amd.NeDDF(**kw)
        for k in synth.FIELD_KEYS["neddf"]:
            e = g["eval_%s_fp64" % k]
            exact[k] = e.reshape(240, -1)[rows].reshape((N_MAX,) + e.shape[2:])
    elif kind == "nerf":
        sd = synth.nerf_state(kw["embed_pos_rank"], kw["embed_dir_rank"], kw["layer_count"], kw["layer_width"], tuple(kw["skips"]), seed=11)
        net = neddf_amd.NeRF(**kw)
    else:
        sd = synth.neus_state(kw["embed_pos_rank"], kw["embed_dir_rank"], kw["sdf_layer_count"], kw["sdf_layer_width"], kw["col_layer_count"],
                              kw["col_layer_width"], tuple(kw["skips"]), kw["init_variance"], seed=13)
        net = neddf_amd.NeuS(**kw)
    return kind, load(net, sd, dev), pts, exact


def evaluate(net, kind, pts, n, dev, surface=True):
    from neddf_amd import Sampling
    s = Sampling(*[T(a[:n][None], dev) for a in pts])
    o = net.forward_surface(s) if (surface and kind != "nerf") else net(s)
    torch.cuda.synchronize()
    return {k: N(v)[0] for k, v in o.items()}


def rms(a, ref):
    return float(np.sqrt(np.mean((a.astype(np.float64) - ref.astype(np.float64)) ** 2)))
