"""The three-term split route (NEDDF_F32_PRODUCTS=split3, tile_engine.h OpsF32x3T) splits the next super-step's A fragments
while the current super-step's MFMAs issue (dense_mfma_split).  These cases stress that pipeline where it has edges: every
engine width (128 / 256 / 384 / 512), odd and single-super-step k extents (position encodings of 48 and 12 columns), skip
layers, tanhExp / ReLU / LeakyReLU fields, NaN inputs and a short final launch.

Both routes run in subprocesses of this file (the switch is read once per process), in 2^16-point launches.  On the golden
fixtures, evaluated in the short last launch of a two-launch batch, the split route's errors against fp64 stay within the
bounds of test_gpu_f32_products.py (1.1x the fp32 MFMA route's, geometric mean; 1.5x for any single output).  On networks
without an fp64 golden, under both routes, results are batch-invariant and a NaN input stays with its own point.
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

FIXTURES = ["neddf_relu", "neddf_tanhexp", "neddf_leaky", "neddf_w128", "neddf_w384", "neddf_skips2", "neddf_negbias"]
# networks without an fp64 golden: (embed_pos_rank, embed_dir_rank, ddf layers, width, col layers, activation, density activation, skips)
NETS = {
    "w512_odd": (8, 4, 8, 512, 4, "tanhExp", "ReLU", (2,)),          # 48 encoding columns: 3 super-steps; a 512 + 48 skip layer
    "w128_one": (2, 1, 6, 128, 3, "ReLU", "ReLU", (1, 3)),            # 12 encoding columns: a single super-step
    "w384_leaky": (10, 4, 8, 384, 4, "LeakyReLU", "ReLU", (4,)),
    "w256_odd": (8, 2, 8, 256, 4, "tanhExp", "ReLU", (4,)),
}
KEYS = ("distance", "density", "color", "aux_grad")
FILL = 65536               # at NEDDF_FIELD_CHUNK_LOG2=16 the points after the first 2^16 run in a second, short launch


def _worker(out):
    import torch

    import synth
    import neddf_amd
    from conftest import golden
    from neddf_amd import Sampling
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    res = {}

    def module(kw, sd):
        net = neddf_amd.NeDDF(**kw)
        net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
        net = net.to(dev)
        net.output_mode = "minimal"
        net.set_iter(-1)
        return net

    def run(net, pos, d, var):
        o = net(Sampling(T(pos), T(d), T(var)))
        torch.cuda.synchronize()
        return {k: o[k].cpu().numpy() for k in KEYS}

    fill = [a.reshape(-1, 3) for a in synth.random_sampling(1, FILL, seed=21)]
    for name in FIXTURES:
        g = golden(name + ".npz")
        kw = json.loads(str(g["config"]))
        make = synth.neddf_state_negbias if name == "neddf_negbias" else synth.neddf_state
        sd = make(kw["embed_pos_rank"], kw["embed_dir_rank"], kw["ddf_layer_count"], kw["ddf_layer_width"],
                  kw["col_layer_count"], kw["col_layer_width"], tuple(kw["skips"]), seed=7)
        net = module(kw, sd)
        x = [np.concatenate([f, np.asarray(g[k], np.float32).reshape(-1, 3)])[None] for f, k in zip(fill, ("pos", "dir", "var"))]
        o = run(net, *x)
        for k in KEYS:
            v = o[k].reshape((-1,) + o[k].shape[2:])[FILL:]
            res["%s/%s" % (name, k)] = v.reshape(np.shape(g["eval_%s_fp64" % k]))
    for name, (E, Ed, L, W, LC, act, dact, skips) in NETS.items():
        kw = dict(embed_pos_rank=E, embed_dir_rank=Ed, ddf_layer_count=L, ddf_layer_width=W, col_layer_count=LC, col_layer_width=W,
                  activation_type=act, density_activation_type=dact, skips=list(skips))
        net = module(kw, synth.neddf_state(E, Ed, L, W, LC, W, skips, seed=31))
        pos, d, var = synth.random_sampling(1, FILL + 777, seed=17)
        full = run(net, pos, d, var)
        for k in KEYS:
            res["%s/%s" % (name, k)] = full[k]
        # batch invariance: a 1000-point batch (one short launch, a ragged last tile) against the same points of the long one
        part = run(net, pos[:, :1000], d[:, :1000], var[:, :1000])
        res["%s/prefix_equal" % name] = np.array(all(np.array_equal(part[k], full[k][:, :1000]) for k in KEYS))
        # NaN positions: every other point of their tiles keeps its outputs bit for bit
        bad = [3, 64, 65, 999]
        pn = pos[:, :1000].copy()
        pn[0, bad, 0] = np.nan
        o = run(net, pn, d[:, :1000], var[:, :1000])
        keep = np.setdiff1d(np.arange(1000), bad)
        res["%s/nan_isolated" % name] = np.array(all(np.array_equal(o[k][:, keep], full[k][:, keep]) for k in KEYS))
    np.savez(out, **res)


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    d = tmp_path_factory.mktemp("f32_split_pipeline")
    out = {}
    for route in ("mfma", "split3"):
        path = str(d / (route + ".npz"))
        env = dict(os.environ, NEDDF_F32_PRODUCTS=route, NEDDF_FIELD_CHUNK_LOG2="16")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "worker", path], env=env, cwd=ROOT, capture_output=True,
                           text=True, timeout=900)
        assert p.returncode == 0, route + p.stdout[-3000:] + p.stderr[-3000:]
        z = np.load(path)
        out[route] = {k: z[k] for k in z.files}
    return out


def _errs(got, exact):
    e = np.abs(got.astype(np.float64) - exact.astype(np.float64)).ravel()
    return float(e.max()), float(np.percentile(e, 99))


@pytest.mark.gpu
def test_split_pipeline_against_fp64_in_a_short_final_launch(routes):
    from conftest import golden
    report, ratios = [], []
    for name in FIXTURES:
        g = golden(name + ".npz")
        for k in KEYS:
            key = "%s/%s" % (name, k)
            exact = g["eval_%s_fp64" % k]
            em, e99m = _errs(routes["mfma"][key], exact)
            es, e99s = _errs(routes["split3"][key], exact)
            report.append("%-28s max %.3g / %.3g   p99 %.3g / %.3g" % (key, es, em, e99s, e99m))
            ratios.append(((es + 1e-12) / (em + 1e-12), (e99s + 1e-12) / (e99m + 1e-12)))
    r = np.array(ratios)
    gmean = np.exp(np.log(r).mean(0))
    print("\nerror vs fp64, split3 / mfma\n" + "\n".join(report) +
          "\ngeometric mean of the ratios: max %.3f, p99 %.3f; largest single ratio %.3f" % (gmean[0], gmean[1], r.max()))
    assert gmean[0] <= 1.1 and gmean[1] <= 1.1, (gmean, "\n".join(report))
    assert r.max() <= 1.5, (r.max(), "\n".join(report))


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["split3", "mfma"])
@pytest.mark.parametrize("name", sorted(NETS))
def test_split_pipeline_batch_invariance_and_nan_isolation(routes, route, name):
    z = routes[route]
    assert bool(z["%s/prefix_equal" % name]), "a 1000-point batch differs from the first 1000 points of a two-launch batch"
    assert bool(z["%s/nan_isolated" % name]), "a NaN position changed another point's outputs"


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "worker":
        _worker(sys.argv[2])
