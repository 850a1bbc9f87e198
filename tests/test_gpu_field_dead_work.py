"""The three-term fp32 field kernels skip work no result reads; every output stays bit for bit what it was.

1. A render pass whose per-sample arrays never leave the library evaluates S - 1 samples per ray (kernels.h RaySrc::Se): the volume
   integral reads density / colour / normal of samples 0 .. S - 2 and of the last sample its distance alone.  The image of
   render_image_single_pass is compared BITWISE with the stand-alone compositors applied to a full [B, S] evaluation of the same rays and
   uniforms -- S = 2 (one sample per ray), 3, 64 / 65 (the compositor's 64-lane chunk edge), 128 (127 evaluated samples against the
   64-point tile); B = 1, 3, 65 (B (S - 1) mostly no multiple of 64: rays straddle tiles); cone and point samples; with and without the
   normal target.  A caller that receives per-sample arrays still gets S entries per ray, the last one as recorded from the parent
   commit.
2. The split pipeline of the distance kernel (tile_engine.h dense_pipeline) neither requests, reads nor splits a super-step past a
   product's last one.  Fields whose products have 1, 2, 3, 4, 5, 6, 8 and 16 super-steps (both parities, the one-super-step product and
   the four-super-step encoding product included), at 1 / 63 / 64 / 65 / 129 / 193 points: every output bitwise equal to the recording.
3. The colour kernel's outputs against the same recording, plus a batch of 512 x 64 + 65 points whose last tiles run on workgroups that
   have processed a tile before (LDS full of the previous tile's last-layer activations) and whose very last tile is ragged: what a
   change to how that kernel clears its small-input columns has to keep (zeroing only the padding columns, without the barrier, kept it
   and measured slower: docs/lab_notebook.md R10.1).

The recording (tests/golden/field_dead_work_parent.npz) was made once on an MI355X from the library of the commit before this change:
    NEDDF_LIB_PATH=<that commit's libneddf_hip.so> python tests/test_gpu_field_dead_work.py record tests/golden/field_dead_work_parent.npz
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE, os.path.join(HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

RECORDING = "field_dead_work_parent.npz"

# (embed_pos_rank, embed_dir_rank, ddf layers, width, col layers, activation, density activation, skips) -> super-steps of 16 k-values:
NETS = {
    "w256": (10, 4, 8, 256, 4, "tanhExp", "ReLU", (4,)),         # encoding 4, hidden 16, colour inputs 6: the shipped shape
    "w256_odd": (8, 2, 8, 256, 4, "tanhExp", "ReLU", (4,)),      # encoding 3, hidden 16, colour inputs 5
    "w128_one": (2, 1, 6, 128, 3, "ReLU", "ReLU", (1, 3)),        # encoding 1, hidden 8, colour inputs 2; two skip layers
}
KEYS = ("distance", "density", "color", "aux_grad")
POINTS = (1, 63, 64, 65, 129, 193)
WGS = 512                         # workgroup slots of the colour / distance grids on the 256-CU part: tiles past 512 reuse a workgroup
LONG = WGS * 64 + 65              # ... so the last tiles of this batch follow another tile in their workgroup, and the last one is ragged
TAIL = 193                        # points of the long batch that are recorded (its end)

BS = (1, 3, 65)
SS = (2, 3, 64, 65, 128)
SAMPLINGS = ("cone", "point")


def _dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _field(name, dev):
    import torch

    import neddf_amd
    import synth
    E, Ed, L, W, LC, act, dact, skips = NETS[name]
    net = neddf_amd.NeDDF(embed_pos_rank=E, embed_dir_rank=Ed, ddf_layer_count=L, ddf_layer_width=W, col_layer_count=LC, col_layer_width=W,
                          activation_type=act, density_activation_type=dact, skips=list(skips))
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.neddf_state(E, Ed, L, W, LC, W, skips, seed=31).items()})
    net = net.to(dev)
    net.output_mode = "minimal"
    net.set_iter(-1)
    for p in net.parameters():
        p.requires_grad_(False)
    return net


def field_outputs(dev):
    """{"<net>/<points>/<key>": array}: the eval-minimal outputs of every NETS field on the first n points of one random batch."""
    import torch

    import synth
    from neddf_amd import Sampling
    res = {}
    pos, d, var = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in synth.random_sampling(1, LONG, seed=17))
    with torch.no_grad():
        for name in NETS:
            net = _field(name, dev)
            for n in POINTS + (LONG,):
                o = net(Sampling(pos[:, :n], d[:, :n], var[:, :n]))
                torch.cuda.synchronize()
                for k in KEYS:
                    v = o[k].cpu().numpy()
                    res["%s/%d/%s" % (name, n, k)] = v[:, -TAIL:] if n == LONG else v
    return res


def _renderer(dev, sampling):
    import torch

    import neddf_amd
    from conftest import BUNNY_CFG, golden
    from neddf_amd.fixtures import bunny_smoke_weights
    g = golden("surface_normals.npz")
    r = neddf_amd.NeRFRender(dict(BUNNY_CFG, _target_="neddf.network.NeDDF"), sample_coarse=64, sample_fine=128, dist_near=2.0, dist_far=6.0,
                             max_dist=6.0, use_coarse_network=False, sampling_type=sampling)
    r.network_fine.load_state_dict({k: torch.from_numpy(v) for k, v in bunny_smoke_weights().items()})
    r.to(dev)
    r.set_iter(-1)
    r.network_fine.output_mode = "minimal"
    for p in r.parameters():
        p.requires_grad_(False)
    cam = neddf_amd.Camera(neddf_amd.PinholeCalib(g["r_calib"].astype(np.float64)), None).to(dev)
    cam.R, cam.T = torch.from_numpy(g["r_R"]).to(dev), torch.from_numpy(g["r_T"]).to(dev)
    return r, cam


WIDTH = HEIGHT = 400              # the fixture camera's image (principal point 200, 200)


def _rays(B, S):
    """B pixels in a row through the middle of the object, and their uniforms."""
    import torch
    lo = (HEIGHT // 2) * WIDTH + WIDTH // 2 - B // 2
    U = torch.rand(B, S, generator=torch.Generator().manual_seed(1000 * B + S))
    return lo, U


def full_evaluation(r, cam, dev, B, S):
    """The stages of one pass, every one of the [B, S] samples evaluated: (dists, {density, color, normal})."""
    import torch
    from neddf_amd import Sampling
    lo, U = _rays(B, S)
    ctx = r._ctx(dev)
    idx = torch.arange(lo, lo + B, device=dev)
    uv = torch.stack([idx % WIDTH, idx // WIDTH], 1)
    rd, ro = ctx.raygen(uv, cam.descriptor())
    dists = ctx.sample_coarse(U.to(dev), r.dist_near, r.dist_far)
    p = r._params()
    smp = Sampling(*ctx.sampling(rd, ro, dists, p.ray_radius if p.cone_sampling else None))
    with torch.no_grad():
        st = r.network_fine.forward_surface(smp, want=("density", "color", "normal"))
    torch.cuda.synchronize()
    return dists, st


def last_samples(dev):
    """{"last/<sampling>/<B>x<S>/<key>": array}: what a caller of the field gets for each ray's LAST sample."""
    res = {}
    for sampling in SAMPLINGS:
        r, cam = _renderer(dev, sampling)
        for B in BS:
            for S in SS:
                _, st = full_evaluation(r, cam, dev, B, S)
                for k in ("density", "color", "normal"):
                    assert st[k].shape[:2] == (B, S)
                    res["last/%s/%dx%d/%s" % (sampling, B, S, k)] = st[k][:, -1].cpu().numpy()
    return res


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def dev():
    return _dev()


@pytest.fixture(scope="module")
def recording():
    from conftest import golden
    z = golden(RECORDING)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def fields(dev):
    return field_outputs(dev)


@pytest.fixture(scope="module")
def renderers(dev):
    return {s: _renderer(dev, s) for s in SAMPLINGS}


@pytest.mark.gpu
@pytest.mark.parametrize("S", SS)
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_image_equals_the_compositors_on_a_full_evaluation(dev, renderers, recording, sampling, B, S):
    import torch
    r, cam = renderers[sampling]
    lo, U = _rays(B, S)
    dists, st = full_evaluation(r, cam, dev, B, S)
    ctx = r._ctx(dev)
    want, _ = ctx.composite(dists, st["density"], st["color"], r.max_dist)
    want["normal"] = ctx.composite_normal(dists, st["density"], st["normal"])
    # the caller of the field still has S entries per ray, and the last one is the parent commit's
    for k in ("density", "color", "normal"):
        assert st[k].shape[:2] == (B, S)
        assert np.array_equal(_bits(st[k][:, -1].cpu().numpy()), _bits(recording["last/%s/%dx%d/%s" % (sampling, B, S, k)])), ("last sample", k)
    for normals in (False, True):
        got = r.render_image_single_pass(WIDTH, HEIGHT, cam, S, U=U.to(dev), pixel_range=(lo, lo + B), normals=normals)
        torch.cuda.synchronize()
        assert int(got["_nan"].item()) == 0
        for k in ("color", "depth", "transmittance") + (("normal",) if normals else ()):
            a, b = got[k].reshape(B, -1), want[k].reshape(B, -1)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (k, "normals" if normals else "plain", float((a - b).abs().max()))
    # not a vacuous comparison: the samples carry density and the pixels colour
    print("%s B=%d S=%d: transmittance %.3f .. %.3f" % (sampling, B, S, float(want["transmittance"].min()), float(want["transmittance"].max())))
    assert float(st["density"].abs().max()) > 0 and float(want["color"].abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", POINTS)
@pytest.mark.parametrize("name", sorted(NETS))
def test_field_outputs_equal_the_parent_recording(fields, recording, name, n):
    for k in KEYS:
        key = "%s/%d/%s" % (name, n, k)
        assert fields[key].shape == recording[key].shape
        assert np.array_equal(_bits(fields[key]), _bits(recording[key])), key


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(NETS))
def test_tiles_behind_another_tile_of_their_workgroup_equal_the_parent_recording(fields, recording, name):
    for k in KEYS:
        key = "%s/%d/%s" % (name, LONG, k)
        assert fields[key].shape == recording[key].shape
        assert np.array_equal(_bits(fields[key]), _bits(recording[key])), key


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "record":
        d = _dev()
        out = field_outputs(d)
        out.update(last_samples(d))
        np.savez_compressed(sys.argv[2], **out)
        print("recorded %d arrays, %d bytes" % (len(out), os.path.getsize(sys.argv[2])))
