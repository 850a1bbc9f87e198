"""The plain fp16 operand policy (weight_dtype "f16": fp16 weights and activations on v_mfma_f32_32x32x16_f16, fp32 accumulation) on
the device.  It exists to be more accurate than bf16 at bf16's cost, so accuracy is what is gated:

  ratio      rms(f16 - ref) <= 0.5 * rms(bf16 - ref) for EVERY output of every case, ref = the network evaluated in double
             (tests/golden/*_fp64, bunny_field_fp64.npz) where the fixtures hold it and this library's fp32 policy (1e-6 .. 1e-5 of
             the values: two orders below either policy's error) where they do not.  The factor is the requirement, not a tolerance:
             operand roundoff is 8x smaller, and a policy that is not twice as accurate as bf16 has no reason to exist.
             Cases: the shipped bunny, NeDDF at widths 128 / 384 and with two skips (both output modes: "full" = forward-mode
             distance gradient, "minimal" = reverse-mode), NeRF at 128 / 384, NeuS at 128 / 384 and with tanhExp; 257 points each
             (the fixture's 240 and its first 17 again -- four 64-row tiles and one point, two 128-row tiles and one point).
  N          the f16 results at N = 1, 63, 64, 65 are the first rows of the 257-point call BIT FOR BIT, for every output: a row does not
             depend on the batch it is in, so the 257-point figures above are those of every smaller N, and a single point's error
             against bf16's (a ratio of two samples, not of two rms) needs no gate of its own
  bits       two runs agree, neddf_field_forward and neddf_field_forward_surface agree on the outputs they share
  classes    NaN / Inf propagate in the reference's classes (tests/golden/nonfinite.npz, the method of tests/test_gpu_nonfinite.py)
  guards     NEDDF_GUARD=1 in a child process: every entry point that evaluates a field, 257 points or rays, no band byte written
  render     render_rays (257 rays, 8 + 8 samples), render_image (37 x 29): finite, PSNR against the fp32 render with the same
             uniforms higher than bf16's; render_image_traced and extract_mesh run, and the f16 mesh is no further from the fp32 mesh
             than the bf16 mesh is (mesh_distance, to="surface")
  slot       fp32 -> f16 -> fp32 restores the fp32 bits, a bf16 result is the same before and after an f16 upload, and a field with
             a finite weight beyond +-65504 is refused while the slot's previous field keeps answering with the same bits

Measured ratios rms(f16) / rms(bf16) (MI355X; worst output of each case; docs/lab_notebook.md R13.1 has the whole table):
    bunny full 0.192 (normal), minimal 0.177 (normal)            neddf_w128 full 0.141 (distance_grad), minimal 0.155 (normal)
    neddf_w384 full 0.445 (density), minimal 0.441 (density)     neddf_skips2 full 0.140 (distance), minimal 0.160 (normal)
    nerf_w128 0.131 (color)   nerf_w384 0.139 (color)            neus_w128_384 0.147 (distance_grad)   neus_tanhexp 0.144 (density)
  median over the 66 outputs 0.136 -- the 0.13 of operand rounding alone.  neddf_w384 is the one case above 0.2: its distance_grad has
  ONE point whose error is 2.4e-2 under both policies (max f16 = max bf16; rms ratio 0.33), which (1 - |grad D|) / D carries into
  density and fields_penalty; every other output of that case sits at 0.10 .. 0.17.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from conftest import BUNNY_CFG, ROOT, golden

import synth
from f16_policy_cases import CASE_MODES, FACTOR, MODES, N_MAX, SIZES, N, T, network_case, evaluate, load, rms

pytestmark = pytest.mark.gpu

WIDE = ("color", "distance_grad", "normal")


@pytest.fixture(autouse=True)
def _inference():
    with torch.no_grad():
        yield


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def evals(dev, bunny_weights, bunny_stages):
    """{(case, mode): dict(exact=..., fp32=..., bf16=..., f16=..., again=..., plain=..., n1 / n63 / n64 / n65=...)}, computed once"""
    out = {}
    with torch.no_grad():
        for name in dict(CASE_MODES):
            kind, net, pts, exact = network_case(name, dev, bunny_weights, bunny_stages)
            for mode in MODES[kind]:
                if kind == "neddf":
                    net.output_mode = mode
                r = dict(exact=exact)
                for dtype in ("fp32", "bf16", "f16"):
                    net.weight_dtype = dtype
                    r[dtype] = evaluate(net, kind, pts, N_MAX, dev)
                r["again"] = evaluate(net, kind, pts, N_MAX, dev)
                r["plain"] = evaluate(net, kind, pts, N_MAX, dev, surface=False)
                for n in SIZES[:-1]:
                    r["n%d" % n] = evaluate(net, kind, pts, n, dev)
                out[name, mode] = r
    return out


def test_f16_is_a_weight_dtype(dev, bunny_weights, bunny_stages):
    """Fails without the feature: "f16" is no key of _lib.DTYPE and 3 is a bad weight_dtype of neddf_set_field."""
    kind, net, pts, _ = network_case("bunny", dev, bunny_weights, bunny_stages)
    net.weight_dtype = "f16"
    o = evaluate(net, kind, pts, 65, dev)
    assert set(o) >= {"distance", "density", "color", "distance_grad", "normal"} and all(np.isfinite(v).all() for v in o.values())
    net.weight_dtype = "fp32"
    o32 = evaluate(net, kind, pts, 65, dev)
    assert not all(np.array_equal(o[k], o32[k]) for k in o), "fp16 operands must show in the result"


@pytest.mark.parametrize("name,mode", CASE_MODES)
def test_f16_is_at_least_twice_as_accurate_as_bf16(evals, name, mode):
    r = evals[name, mode]
    bad = []
    for k in r["f16"]:
        ref, src = (r["exact"][k], "fp64") if k in r["exact"] else (r["fp32"][k], "fp32")
        ref = ref.reshape(r["f16"][k].shape)
        e16, eb = rms(r["f16"][k], ref), rms(r["bf16"][k], ref)
        m16, mb = float(np.abs(r["f16"][k] - ref).max()), float(np.abs(r["bf16"][k] - ref).max())
        print("%-14s %-8s %-14s vs %s: rms f16 %.3e bf16 %.3e ratio %.3f | max f16 %.3e bf16 %.3e" % (
            name, mode, k, src, e16, eb, e16 / eb if eb > 0 else float("nan"), m16, mb))
        assert np.isfinite(r["f16"][k]).all(), (name, mode, k)
        if not e16 <= FACTOR * eb:
            bad.append("%s: rms f16 %.3e > %.1f x rms bf16 %.3e (ratio %.3f)" % (k, e16, FACTOR, eb, e16 / eb if eb > 0 else float("inf")))
    assert not bad, "%s %s:\n  " % (name, mode) + "\n  ".join(bad)


@pytest.mark.parametrize("name,mode", CASE_MODES)
def test_f16_rows_do_not_depend_on_the_batch(evals, name, mode):
    r = evals[name, mode]
    for n in SIZES[:-1]:
        for k, v in r["n%d" % n].items():
            assert v.shape[0] == n and np.array_equal(v, r["f16"][k][:n]), "%s %s %s: the %d-point call differs from rows 0..%d of the %d-point call" % (
                name, mode, k, n, n - 1, N_MAX)


@pytest.mark.parametrize("name,mode", CASE_MODES)
def test_f16_runs_agree_bit_for_bit(evals, name, mode):
    r = evals[name, mode]
    for k, v in r["again"].items():
        assert np.array_equal(v, r["f16"][k]), "%s %s %s: two runs differ" % (name, mode, k)
    assert set(r["plain"]) <= set(r["f16"])
    for k, v in r["plain"].items():
        assert np.array_equal(v, r["f16"][k]), "%s %s %s: field_forward and field_forward_surface differ" % (name, mode, k)


# ------------------------------------------------------------------------------------------------ NaN and Inf
def _nonfinite_keys(kind, mode):
    return tuple(k for k in synth.FIELD_KEYS[kind] if not (mode == "minimal" and k == "fields_penalty"))


NONFINITE_CASES = ["input"] + list(synth.NONFINITE_WEIGHT_POISONS)


@pytest.fixture(scope="module")
def nonfinite(dev):
    import neddf_amd
    from neddf_amd import Sampling
    res = {}
    clean, bad = synth.nonfinite_inputs()
    cls = {"neddf": neddf_amd.NeDDF, "nerf": neddf_amd.NeRF, "neus": neddf_amd.NeuS}
    with torch.no_grad():
        for name, (kind, kw) in synth.NONFINITE_NETS.items():
            for case in NONFINITE_CASES + ["clean"]:
                net = load(cls[kind](**kw), synth.nonfinite_state(name, case if case in synth.NONFINITE_WEIGHT_POISONS else None), dev)
                net.weight_dtype = "f16"
                smp = Sampling(*[T(a, dev) for a in (bad if case == "input" else clean)])
                for mode in MODES[kind] if kind == "neddf" else ("full",):
                    if kind == "neddf":
                        net.output_mode = mode
                    o = net(smp)
                    torch.cuda.synchronize()
                    for k in _nonfinite_keys(kind, mode):
                        res[name, mode, case, k] = N(o[k])
    return res


@pytest.mark.parametrize("name,mode", [(n, m) for n, (kind, _) in synth.NONFINITE_NETS.items() for m in (("full", "minimal") if kind == "neddf" else ("full",))])
def test_f16_nonfinite_classes(nonfinite, name, mode):
    g = golden("nonfinite.npz")
    kind, _ = synth.NONFINITE_NETS[name]
    msgs = []
    for case in NONFINITE_CASES:
        for k in _nonfinite_keys(kind, mode):
            pre = "%s/%s/eval/" % (name, case)
            want, keep = g[pre + k], g[pre + "keep_" + k]
            have = nonfinite[name, mode, case, k].reshape(want.shape)
            diff = keep & (synth.float_class(have) != synth.float_class(want))
            if diff.any():
                msgs.append("%s %s %s %s: class differs on %d elements, first at %s: got %s, reference %s" % (
                    name, mode, case, k, int(diff.sum()), tuple(int(i) for i in np.argwhere(diff)[0]), have[diff][:4], want[diff][:4]))
    assert not msgs, "\n  ".join(msgs)
    # the clean rows of the poisoned batch are the clean batch's, bit for bit
    rest = np.setdiff1d(np.arange(synth.NONFINITE_POINTS), synth.NONFINITE_ROWS)
    for k in _nonfinite_keys(kind, mode):
        a, b = nonfinite[name, mode, "input", k], nonfinite[name, mode, "clean", k]
        assert np.isfinite(b).all() and np.array_equal(a[rest], b[rest]), (name, mode, k)


# ------------------------------------------------------------------------------------------------ guard bands
_GUARD_WORKER = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import neddf_amd
from neddf_amd import Context
from neddf_amd._lib import OUT_FULL, OUT_MINIMAL
from neddf_amd.fixtures import BUNNY_SMOKE_CFG, bunny_smoke_weights, synth
from neddf_amd.occupancy import OccupancyGrid
from neddf_amd.render import SLOT_FINE
from neddf_amd.trace import trace_params
dev, N = torch.device("cuda:0"), 257
r = neddf_amd.NeRFRender(dict(BUNNY_SMOKE_CFG, _target_="neddf.network.NeDDF"), sample_coarse=8, sample_fine=8, dist_near=2.0, dist_far=6.0,
                         max_dist=6.0, use_coarse_network=False, sampling_type="cone")
r.network_fine.load_state_dict({k: torch.from_numpy(v) for k, v in bunny_smoke_weights().items()})
r.to(dev); r.set_iter(-1)
r.network_fine.weight_dtype = r.network_coarse.weight_dtype = "f16"
fx = 0.5 * 800 / np.tan(0.5 * 0.6911112070083618)
cam = neddf_amd.Camera(neddf_amd.PinholeCalib(np.array([fx, fx, 400.0, 400.0])), None).to(dev)
cam.R, cam.T = torch.eye(3, device=dev), torch.tensor([0.0, 0.0, 4.0], device=dev)
done = []
def check(what):
    bands, bad = ctx.check_guards()
    assert bands > 0 and bad == 0, (what, bands, bad)
    done.append(what)
with torch.no_grad():
    ctx = r._ctx(dev)
    pos, d, var = [torch.from_numpy(a.reshape(-1, 3)[:N].copy()).to(dev) for a in synth.random_sampling(3, 100, seed=2)]
    for mode, want in ((OUT_FULL, ("distance", "density", "color", "fields_penalty", "aux_grad")), (OUT_MINIMAL, ("distance", "density", "color", "aux_grad"))):
        ctx.field_forward(SLOT_FINE, pos, d, var, mode, want); check("field_forward")
        ctx.field_forward_surface(SLOT_FINE, pos, d, var, mode, want + ("distance_grad", "normal")); check("field_forward_surface")
    LO, HI, shape = (-1.1,) * 3, (1.1,) * 3, (24, 24, 24)
    ctx.field_grid(SLOT_FINE, "distance", (N, 2, 2), LO, HI); check("field_grid")
    ctx.field_grid(SLOT_FINE, "density", (17, 9, 13), LO, HI); check("field_grid")
    ctx.field_grid_coarse(SLOT_FINE, "distance", shape, 8, LO, HI); check("field_grid_coarse")
    ctx.field_bricks(SLOT_FINE, "distance", shape, 8, LO, HI, torch.tensor([0, 5, 13, 26], dtype=torch.int32, device=dev)); check("field_bricks")
    grid = OccupancyGrid.from_field(r.network_fine, resolution=16, cube_range=1.1, threshold=0.0, dilate=1)
    torch.cuda.synchronize()
    uv = torch.randint(300, 500, (N, 2), device=dev)
    Sc, S2 = 8, 8 + 8 + 2
    buf = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
    for occ in (None, grid.descriptor()):
        for single in (False, True):
            for normal in ((False, True) if occ is None else (False,)):
                o = dict(color=buf(N, 3), depth=buf(N), transmittance=buf(N))
                if not single:
                    o.update(weight=buf(N, S2 - 1), color_coarse=buf(N, 3), depth_coarse=buf(N), transmittance_coarse=buf(N), weight_coarse=buf(N, Sc),
                             dists_coarse=buf(N, Sc + 1), dists_fine=buf(N, S2))
                if normal:
                    o["normal"] = buf(N, 3)
                    if not single:
                        o["normal_coarse"] = buf(N, 3)
                flag = torch.zeros(1, device=dev, dtype=torch.int32)
                ctx.render_rays(uv, cam.descriptor(), r._params(), torch.rand(N, Sc + 1, device=dev), None if single else torch.rand(N, 9, device=dev),
                                dict(o, nan_flag=flag), single_slot=SLOT_FINE if single else None, occupancy=occ)
                check("render_rays%s%s%s" % ("_single" if single else "", "_surface" if normal else "", "_culled" if occ is not None else ""))
                assert all(torch.isfinite(v).all() for v in o.values())
    rd, ro = ctx.raygen(uv, cam.descriptor())
    ctx.trace_field(SLOT_FINE, ro, rd, trace_params(threshold=0.05, t_near=2.0, t_far=6.0, max_steps=8, refine=2)); check("trace_field")
assert len(set(done)) == 12, sorted(set(done))
print("GUARD_OK %d checks" % len(done))
"""


def test_f16_entry_points_leave_the_guard_bands_alone(tmp_path):
    w = tmp_path / "guard_worker_f16.py"
    w.write_text(_GUARD_WORKER)
    p = subprocess.run([sys.executable, str(w), ROOT], env=dict(os.environ, NEDDF_GUARD="1"), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "GUARD_OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


# ------------------------------------------------------------------------------------------------ render level
def _renderer(dev, bunny_weights):
    import neddf_amd
    r = neddf_amd.NeRFRender(dict(BUNNY_CFG, _target_="neddf.network.NeDDF"), sample_coarse=8, sample_fine=8, dist_near=2.0, dist_far=6.0, max_dist=6.0,
                             use_coarse_network=False, sampling_type="cone")
    load(r.network_fine, bunny_weights, dev)
    r.to(dev)
    r.set_iter(-1)
    W, H = 37, 29
    fx = 0.5 * W / np.tan(0.5 * 0.6911112070083618)
    cam = neddf_amd.Camera(neddf_amd.PinholeCalib(np.array([fx, fx, 0.5 * W, 0.5 * H])), None).to(dev)
    cam.R, cam.T = torch.eye(3, device=dev), torch.tensor([0.0, 0.0, 4.0], device=dev)
    return r, cam, W, H


def _psnr(a, b):
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return 10.0 * np.log10(1.0 / mse) if mse > 0 else float("inf")


def _set(r, dtype):
    r.network_fine.weight_dtype = r.network_coarse.weight_dtype = dtype


def test_f16_renders_closer_to_fp32_than_bf16(dev, bunny_weights):
    r, cam, W, H = _renderer(dev, bunny_weights)
    rng = np.random.default_rng(5)
    uv = T(np.stack([rng.integers(0, W, 257), rng.integers(0, H, 257)], 1).astype(np.int64), dev)
    U_c, U_f = T(rng.random((257, 9), dtype=np.float32), dev), T(rng.random((257, 9), dtype=np.float32), dev)
    rays, images = {}, {}
    for dtype in ("fp32", "bf16", "f16"):
        _set(r, dtype)
        o = r._render(r._ctx(dev), uv, cam, U_c, U_f, full=False)
        assert int(o["_nan"].item()) == 0
        rays[dtype] = {k: N(v) for k, v in o.items() if k != "_nan"}
        torch.manual_seed(11)
        images[dtype] = {k: N(v) for k, v in r.render_image(W, H, cam, ["color", "depth", "transmittance"]).items()}
    for what, res in (("render_rays", rays), ("render_image", images)):
        assert all(np.isfinite(v).all() for v in res["f16"].values()), what
        p16, pb = _psnr(res["f16"]["color"], res["fp32"]["color"]), _psnr(res["bf16"]["color"], res["fp32"]["color"])
        print("%s: PSNR against the fp32 render, f16 %.2f dB, bf16 %.2f dB" % (what, p16, pb))
        assert res["f16"]["color"].std() > 1e-3, what + ": the view must show the object"
        assert p16 > pb, "%s: f16 %.2f dB is not above bf16's %.2f dB" % (what, p16, pb)


def test_f16_traced_view_and_mesh(dev, bunny_weights):
    from neddf_amd.geometry import mesh_distance
    r, cam, W, H = _renderer(dev, bunny_weights)
    meshes = {}
    for dtype in ("fp32", "bf16", "f16"):
        _set(r, dtype)
        meshes[dtype] = r.network_fine.extract_mesh(resolution=24, threshold=0.1)
    o = r.render_image_traced(W, H, cam, ["color", "depth", "transmittance", "normal"], threshold=0.1)
    assert all(torch.isfinite(v).all() for v in o.values()) and float(o["transmittance"].min()) == 0.0, "the traced view must hit the object"
    assert all(m[1].shape[0] > 100 for m in meshes.values())
    d16 = mesh_distance(meshes["f16"], meshes["fp32"], n=4000, to="surface")
    db = mesh_distance(meshes["bf16"], meshes["fp32"], n=4000, to="surface")
    print("mesh_distance to the fp32 mesh (chamfer / hausdorff): f16 %.3e / %.3e, bf16 %.3e / %.3e" % (
        d16["chamfer"], d16["hausdorff"], db["chamfer"], db["hausdorff"]))
    assert d16["chamfer"] <= db["chamfer"]


# ------------------------------------------------------------------------------------------------ the slot
def test_f16_round_trips_and_leaves_the_other_policies_alone(dev, bunny_weights, bunny_stages):
    kind, net, pts, _ = network_case("bunny", dev, bunny_weights, bunny_stages)
    got = {}
    for step, dtype in enumerate(("fp32", "bf16", "f16", "bf16", "fp32")):
        net.weight_dtype = dtype
        got[step] = evaluate(net, kind, pts, 65, dev)
    for k in got[0]:
        assert np.array_equal(got[4][k], got[0][k]), "fp32 -> f16 -> fp32: %s changed" % k
        assert np.array_equal(got[3][k], got[1][k]), "bf16 before and after an f16 upload: %s changed" % k


def test_out_of_range_weight_is_refused_and_the_slot_keeps_its_field(dev, bunny_weights, bunny_stages):
    import neddf_amd
    from neddf_amd import Context
    from neddf_amd._lib import OUT_MINIMAL, NeddfError
    kind, net, pts, _ = network_case("bunny", dev, bunny_weights, bunny_stages)
    net.weight_dtype = "f16"
    net.output_mode = "minimal"
    ctx, want = Context.get(dev), ("distance", "density", "color", "aux_grad")
    p, d, v = [T(a[:65], dev) for a in pts]
    net.upload(ctx, net._slot)
    before = {k: N(x) for k, x in ctx.field_forward(net._slot, p, d, v, OUT_MINIMAL, want).items()}
    for value, ok in ((70000.0, False), (-65519.0, False), (float("inf"), True), (float("nan"), True)):
        other = load(neddf_amd.NeDDF(**BUNNY_CFG), bunny_weights, dev)
        other.weight_dtype = "f16"
        other.output_mode = "minimal"
        with torch.no_grad():
            other.layers_ddf[2].weight[3, 5] = value
        if ok:
            other.upload(ctx, net._slot)         # NaN and Inf weights pass, as under every policy
            continue
        with pytest.raises(NeddfError, match="65504"):
            other.upload(ctx, net._slot)
        after = {k: N(x) for k, x in ctx.field_forward(net._slot, p, d, v, OUT_MINIMAL, want).items()}      # no upload in between
        for k in want:
            assert np.array_equal(after[k], before[k]), "%s changed after the refused upload of %r" % (k, value)
        other.weight_dtype = "bf16"              # the policies with fp32's range keep taking the weight
        other.upload(ctx, net._slot)
        net.invalidate()
        net.upload(ctx, net._slot)
