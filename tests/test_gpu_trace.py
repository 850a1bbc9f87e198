"""Sphere tracing on the GPU: the stage kernels in lockstep with the numpy restatement (tests/trace_check.py) bit for bit, the closed
form of a sphere, neddf_trace_field on the shipped bunny network and a NeuS field against a lockstep loop without compaction, the
bracket on the real field, and NeRFRender.render_image_traced against field_forward_surface at the traced points."""
import json

import numpy as np
import pytest
import torch
from conftest import BUNNY_CFG, golden

import trace_check as tc

pytestmark = pytest.mark.gpu

W, H = 37, 29                   # the view of the field tests: 1073 rays, as tests/test_gpu_occupancy.py renders
THRESHOLD = 0.0275              # extract_mesh's level set of the shipped bunny network
STATE = ("t", "t_lo", "status", "steps", "distance")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def N(t):
    return t.detach().cpu().numpy()


def _ctx(dev):
    from neddf_amd import Context
    return Context.get(dev)


def _assert_state(got, want, what):
    for k in STATE:
        assert tc.same_bits(N(got[k]), want[k]), "%s: %s differs in %d rows" % (what, k, int((N(got[k]).view(np.uint8).reshape(len(want[k]), -1)
                                                                                              != want[k].view(np.uint8).reshape(len(want[k]), -1)).any(1).sum()))


# ------------------------------------------------------------------------------------------------------- 1. kernels in lockstep
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025, 70001])
def test_stage_kernels_in_lockstep_with_the_restatement(dev, n):
    """Sphere + torus, distances by torch on the device from the kernel's own points (NaN planted in a few rows of two iterations); after
    every stage the GPU state equals the restatement's, given that same distance array, bit for bit.  max_steps = 12 leaves EXHAUSTED rays."""
    ctx = _ctx(dev)
    t_near, t_far, tau, max_steps, refine = 2.0, 6.0, 0.02, 12, 3
    step_scale, min_step = 1.0, float(np.float32((t_far - t_near) * 2.0 ** -10))
    o_h, d_h = tc.scene_rays(n, t_near, tau)
    o, d = torch.from_numpy(o_h).to(dev), torch.from_numpy(d_h).to(dev)
    st = ctx.trace_begin(o, d, t_near)
    ref = tc.begin(o_h, d_h, t_near)
    _assert_state(st, ref, "begin")

    def step(points_gpu, points_ref, it, plant):
        index, pos = points_gpu(o, d, st)
        r_index, r_pos = points_ref(o_h, d_h, ref)
        assert tc.same_bits(N(index), r_index) and tc.same_bits(N(pos), r_pos), "iteration %d: index / pos" % it
        if index.shape[0] == 0:
            return None, None
        D = tc.scene_distance(pos, torch)
        if plant:
            D[torch.arange(D.shape[0], device=dev) % 41 == 7] = float("nan")
        return index, D

    for it in range(max_steps):
        index, D = step(ctx.trace_compact, tc.compact, it, plant=it in (1, 3))
        if index is None:
            break
        ctx.trace_advance(index, D, st, tau, step_scale, min_step, t_far)
        tc.advance(ref, N(index), N(D), tau, step_scale, min_step, t_far)
        _assert_state(st, ref, "advance %d" % it)
    ctx.trace_finish(st)
    tc.finish(ref)
    _assert_state(st, ref, "finish")
    for rnd in range(refine):
        index, D = step(ctx.trace_bisect_points, tc.bisect_points, rnd, plant=rnd == 1)
        if index is None:
            break
        ctx.trace_bisect_update(index, D, st, tau)
        tc.bisect_update(ref, N(index), N(D), tau)
        _assert_state(st, ref, "bisect %d" % rnd)
    status, k = ref["status"], np.arange(n) % 16
    assert not (status == tc.ACTIVE).any()
    if n >= 1025:           # the ray set holds every kind of ray
        for code in (tc.HIT, tc.MISS, tc.EXHAUSTED, tc.INVALID):
            assert (status == code).any(), code
        assert (status[(k >= 6) & (k <= 9)] == tc.INVALID).all()
        assert (status[k == 5] == tc.HIT).all() and (ref["steps"][k == 5] == 0).all()           # rays that start inside
        assert ((status == tc.INVALID) & (k < 6)).any()                                          # a planted NaN distance ended a sound ray


def test_sphere_trace_is_the_stage_loop(dev):
    """trace.sphere_trace drives the same stages: equal to the restatement's whole loop on the same torch distance function."""
    from neddf_amd.trace import sphere_trace
    o_h, d_h = tc.scene_rays(1025, 2.0, 0.02)
    fn = lambda p: tc.scene_distance(p, torch)                       # noqa: E731
    res = sphere_trace(torch.from_numpy(o_h).to(dev), torch.from_numpy(d_h).to(dev), fn, threshold=0.02, t_near=2.0, t_far=6.0, max_steps=24,
                       refine=2)
    ref, ev = tc.trace(o_h, d_h, lambda p: N(fn(torch.from_numpy(p).to(dev))), 0.02, 2.0, 6.0, 24, 1.0, np.float32(4.0 * 2.0 ** -10), 2)
    _assert_state(dict(zip(STATE, res[:5])), ref, "sphere_trace")
    assert res.evaluations == ev


# ------------------------------------------------------------------------------------------------------- 2. closed form
def test_sphere_closed_form(dev):
    """Sphere only, step_scale 1, tau 0.02, refine 4: HIT within [t_tau, t_tau + min_step 2^-4 + 1e-5] for impact parameters up to
    0.9 (R + tau), MISS beyond R + tau + 1e-5 (tests/trace_check.py check_sphere_closed_form states the gate and its reasons)."""
    from neddf_amd.trace import sphere_trace
    t_near, t_far, tau = 1.0, 5.0, 0.02
    o_h, d_h = tc.sphere_rays(4096)
    res = sphere_trace(torch.from_numpy(o_h).to(dev), torch.from_numpy(d_h).to(dev), lambda p: p.norm(dim=1) - tc.SPHERE_R, threshold=tau,
                       t_near=t_near, t_far=t_far, max_steps=256, step_scale=1.0, refine=4)        # 256: tests/test_trace_host.py MAX_STEPS
    st = dict(zip(STATE, (N(x) for x in res[:5])))
    tc.check_sphere_closed_form(o_h, d_h, st, tau, (t_far - t_near) * 2.0 ** -10, 4)


# ------------------------------------------------------------------------------------------------------- 3. / 4. the field path
def _look_at(eye, target):
    """R (columns: camera x, y, z in world space; the camera looks along its -z) and T of a camera at `eye` looking at `target`."""
    z = (eye - target) / np.linalg.norm(eye - target)
    x = np.cross([0.0, 1.0, 0.0], z); x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z], 1).astype(np.float32), eye.astype(np.float32)


@pytest.fixture(scope="module")
def bunny(dev):
    """The shipped bunny network behind a 37 x 29 view.  Its distance falls below 0.0275 only in small pockets (minimum 0.0234 on a 48^3
    lattice over [-1.1, 1.1]^3), and the pose of the bunny_stages fixture sees 0.8 % of its rays hit.  The camera is therefore moved to
    look at the largest pocket from 2.6 away with a focal length of 140 pixels: the CPU oracle gives 14.6 % HIT and 85.3 % MISS there."""
    import neddf_amd
    from neddf_amd.fixtures import bunny_smoke_weights
    render = neddf_amd.NeRFRender(dict(BUNNY_CFG, _target_="neddf.network.NeDDF"), sample_coarse=16, sample_fine=32, dist_near=2.0, dist_far=6.0,
                                  max_dist=6.0, use_coarse_network=False, sampling_type="cone")
    render.network_fine.load_state_dict({k: torch.from_numpy(v) for k, v in bunny_smoke_weights().items()})
    render.to(dev)
    render.set_iter(-1)
    for p in render.parameters():
        p.requires_grad_(False)
    target = np.array([-0.12, 0.33, -0.10])
    R, T = _look_at(target + 2.6 * np.array([-1.0, 1.0, 0.0]) / np.sqrt(2.0), target)
    cam = neddf_amd.Camera(neddf_amd.PinholeCalib(np.array([140.0, 140.0, W / 2.0, H / 2.0])), None).to(dev)
    cam.R, cam.T = torch.from_numpy(R).to(dev), torch.from_numpy(T).to(dev)
    idx = torch.arange(W * H, device=dev)
    ctx = render._ctx(dev)
    rd, ro = ctx.raygen(torch.stack([idx % W, idx // W], 1), cam.descriptor())
    return dict(render=render, cam=cam, ctx=ctx, rd=rd, ro=ro)


def _field_lockstep(ctx, slot, ro, rd, p):
    """The restatement's loop with the field evaluated on ALL rays' points, no compaction: (state, evaluations)."""
    from neddf_amd._lib import OUT_MINIMAL
    o_h, d_h = N(ro), N(rd)
    n = o_h.shape[0]
    unit = torch.tensor([1.0, 0.0, 0.0], device=ro.device).expand(n, 3).contiguous()
    zero = torch.zeros(n, 3, device=ro.device)

    def all_distances(depth):
        pos = tc._points(o_h, d_h, np.arange(n), depth)
        return N(ctx.field_forward(slot, torch.from_numpy(pos).to(ro.device), unit, zero, OUT_MINIMAL, ["distance"])["distance"])

    st, ev = tc.begin(o_h, d_h, p.t_near), 0
    for _ in range(p.max_steps):
        index, _pos = tc.compact(o_h, d_h, st)
        if index.size == 0:
            break
        ev += index.size
        tc.advance(st, index, all_distances(st["t"])[index], p.threshold, p.step_scale, p.min_step, p.t_far)
    tc.finish(st)
    for _ in range(p.refine):
        index, _pos = tc.bisect_points(o_h, d_h, st)
        if index.size == 0:
            break
        ev += index.size
        tc.bisect_update(st, index, all_distances(tc._mid(st, np.arange(n)))[index], p.threshold)
    return st, ev


@pytest.fixture(scope="module")
def bunny_traced(bunny):
    from neddf_amd._lib import SLOT_FINE
    from neddf_amd.trace import trace_params
    p = trace_params(THRESHOLD, 2.0, 6.0, max_steps=64, refine=4)
    st, ev = bunny["ctx"].trace_field(SLOT_FINE, bunny["ro"], bunny["rd"], p)
    torch.cuda.synchronize()
    return dict(p=p, st=st, ev=ev)


def test_trace_field_equals_the_uncompacted_lockstep_loop(bunny, bunny_traced):
    from neddf_amd._lib import SLOT_FINE
    p, st = bunny_traced["p"], bunny_traced["st"]
    ref, ev = _field_lockstep(bunny["ctx"], SLOT_FINE, bunny["ro"], bunny["rd"], p)
    status = N(st["status"])
    shares = {name: float((status == code).mean()) for name, code in (("hit", tc.HIT), ("miss", tc.MISS), ("exhausted", tc.EXHAUSTED))}
    print("bunny view:", shares, "evaluations per ray %.2f" % (bunny_traced["ev"] / float(W * H)))
    assert shares["hit"] >= 0.05 and shares["miss"] >= 0.05, shares
    _assert_state(st, ref, "trace_field")
    assert bunny_traced["ev"] == ev


def test_trace_field_on_a_neus_field(dev, bunny):
    """The same equality on a NeuS field (synthetic weights, widths 128 / 384) at the sdf's zero level set."""
    import neddf_amd
    from neddf_amd.fixtures import synth
    from neddf_amd.trace import trace_params
    kw = json.loads(str(golden("neus_w128_384.npz")["config"]))
    sd = synth.neus_state(kw["embed_pos_rank"], kw["embed_dir_rank"], kw["sdf_layer_count"], kw["sdf_layer_width"], kw["col_layer_count"],
                          kw["col_layer_width"], tuple(kw["skips"]), kw["init_variance"], seed=13)
    net = neddf_amd.NeuS(**kw)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    net.to(dev)
    ctx = _ctx(dev)
    net.upload(ctx, net._slot)
    p = trace_params(0.0, 2.0, 6.0, max_steps=24, refine=3)
    st, ev = ctx.trace_field(net._slot, bunny["ro"], bunny["rd"], p)
    ref, r_ev = _field_lockstep(ctx, net._slot, bunny["ro"], bunny["rd"], p)
    print("neus view:", {int(c): int(k) for c, k in zip(*np.unique(ref["status"], return_counts=True))})
    _assert_state(st, ref, "trace_field (NeuS)")
    assert ev == r_ev
    with pytest.raises(neddf_amd.NeddfError):
        bad = trace_params(0.0, 2.0, 6.0)
        bad.step_scale = 2.0
        ctx.trace_field(net._slot, bunny["ro"], bunny["rd"], bad)


def test_bracket_on_the_real_field(bunny, bunny_traced):
    """For every HIT ray D(t) <= threshold; where t_lo < t also D(t_lo) > threshold, and t - t_lo <= min_step 2^-refine up to one ulp of t."""
    from neddf_amd._lib import OUT_MINIMAL, SLOT_FINE
    p, st, ctx, ro, rd = bunny_traced["p"], bunny_traced["st"], bunny["ctx"], bunny["ro"], bunny["rd"]
    hit = st["status"] == tc.HIT
    o, d, t, t_lo = ro[hit], rd[hit], st["t"][hit], st["t_lo"][hit]
    unit = torch.tensor([1.0, 0.0, 0.0], device=o.device).expand_as(o).contiguous()

    def D(depth):
        return ctx.field_forward(SLOT_FINE, o + depth[:, None] * d, unit, torch.zeros_like(o), OUT_MINIMAL, ["distance"])["distance"]

    thr = torch.tensor(p.threshold, device=o.device)        # the float32 the library compares against
    assert bool((D(t) <= thr).all())
    assert tc.same_bits(N(D(t)), N(st["distance"][hit]))    # ... and it is the last distance the tracer read
    adv = t_lo < t
    assert bool(adv.any()) and bool((D(t_lo)[adv] > thr).all())
    width, ulp = N(t - t_lo).astype(np.float64), np.spacing(N(t)).astype(np.float64)
    assert (width <= float(p.min_step) * 2.0 ** -p.refine + ulp).all(), float((width - ulp).max())


# ------------------------------------------------------------------------------------------------------- 5. render_image_traced
def test_render_image_traced(bunny, bunny_traced):
    from neddf_amd._lib import OUT_MINIMAL, SLOT_FINE
    render, cam, ctx, ro, rd, st = bunny["render"], bunny["cam"], bunny["ctx"], bunny["ro"], bunny["rd"], bunny_traced["st"]
    targets = ["color", "depth", "transmittance", "normal", "steps"]
    rng_before = torch.get_rng_state()
    img = render.render_image_traced(W, H, cam, targets, THRESHOLD, background=0.25)
    torch.cuda.synchronize()
    assert torch.equal(torch.get_rng_state(), rng_before)
    assert [tuple(img[k].shape) for k in targets] == [(H, W, 3), (H, W), (H, W), (H, W, 3), (H, W)] and img["steps"].dtype == torch.int32
    hit = (st["status"] == tc.HIT).reshape(H, W)
    t = st["t"].reshape(H, W)
    assert tc.same_bits(N(img["depth"]), N(torch.where(hit, t, torch.zeros_like(t))))
    assert tc.same_bits(N(img["transmittance"]), N(torch.where(hit, torch.zeros_like(t), torch.ones_like(t))))
    assert tc.same_bits(N(img["steps"]), N(st["steps"].reshape(H, W)))
    idx = hit.reshape(-1).nonzero().squeeze(1)
    pos = ro[idx] + st["t"][idx, None] * rd[idx]
    want = ctx.field_forward_surface(SLOT_FINE, pos, rd[idx], torch.zeros_like(pos), OUT_MINIMAL, ("color", "normal"))
    for k, fill in (("color", 0.25), ("normal", 0.0)):
        flat = img[k].reshape(-1, 3)
        assert tc.same_bits(N(flat[idx]), N(want[k].view(-1, 3))), k
        assert bool((flat[~hit.reshape(-1)] == fill).all()), k
    lo, hi = 5 * W + 3, 23 * W + 11
    slab = render.render_image_traced(W, H, cam, targets, THRESHOLD, background=0.25, pixel_range=(lo, hi))
    for k in targets:
        full = img[k].reshape(W * H, 3) if img[k].dim() == 3 else img[k].reshape(W * H)
        assert tc.same_bits(N(slab[k]), N(full[lo:hi])), k


def test_render_image_traced_refuses_nerf_fields_and_ndc_rays(dev, bunny):
    import neddf_amd
    render, cam = bunny["render"], bunny["cam"]
    render.ray_space = "ndc"
    try:
        with pytest.raises(NotImplementedError):
            render.render_image_traced(W, H, cam, ["color"], THRESHOLD)
    finally:
        render.ray_space = "world"
    nerf = neddf_amd.NeRFRender(dict(_target_="neddf.network.NeRF", embed_pos_rank=4, embed_dir_rank=2, layer_count=2, layer_width=64,
                                     activation_type="ReLU", density_activation_type="ReLU", skips=[]), use_coarse_network=False).to(dev)
    with pytest.raises(NotImplementedError):
        nerf.render_image_traced(W, H, cam, ["color"], THRESHOLD)
    from neddf_amd._lib import SLOT_FINE
    from neddf_amd.trace import trace_params
    ctx = nerf._ctx(dev)                                     # the library refuses as well: a NeRF field has no distance
    with pytest.raises(neddf_amd.NeddfError):
        ctx.trace_field(SLOT_FINE, bunny["ro"], bunny["rd"], trace_params(THRESHOLD, 2.0, 6.0))
    bunny["render"]._ctx(dev)                                # the bunny network back into its slot for whoever runs next


# ------------------------------------------------------------------------------------------------------- the command line
def test_run_eval_trace_flag(tmp_path, capsys):
    """run_eval.py --trace: the usual files and lines as without the flag, plus {id}_rgb_traced / _depth_traced PNGs and one line per view."""
    import os
    import re

    import yaml
    from PIL import Image
    from conftest import GOLDEN
    from neddf_amd.fixtures import bunny_smoke_weights
    from neddf_amd.scripts.run_eval import main
    run = tmp_path / "run"
    (run / ".hydra").mkdir(parents=True)
    (run / "models").mkdir()
    cfg = {"dataset": {"_target_": "neddf.dataset.NeRFSyntheticDataset", "dataset_dir": os.path.join(GOLDEN, "bunny_mini"),
                       "data_split": "train", "use_depth": False, "use_mask": True},
           "render": {"_target_": "neddf.render.NeRFRender", "sample_coarse": 16, "sample_fine": 32, "dist_near": 2.0, "dist_far": 6.0,
                      "max_dist": 6.0, "use_coarse_network": False, "sampling_type": "cone"},
           "network": dict(BUNNY_CFG, _target_="neddf.network.NeDDF"),
           "trainer": {"_target_": "neddf.trainer.NeRFTrainer", "device": "cuda:0", "batch_size": 128, "chunk": 1024},
           "loss": {"functions": [{"_target_": "neddf.loss.ColorLoss", "weight": 1.0}]}}
    yaml.safe_dump(cfg, open(run / ".hydra" / "config.yaml", "w"))
    sd = {p + k: torch.from_numpy(v) for k, v in bunny_smoke_weights().items() for p in ("network_fine.", "network_coarse.")}
    torch.save(sd, run / "models" / "model_00007.pth")
    main([str(run), "--epoch", "7", "--seed", "5"])
    plain = capsys.readouterr().out.splitlines()
    usual = {f: (run / "eval" / f).read_bytes() for f in sorted(os.listdir(run / "eval"))}
    main([str(run), "--epoch", "7", "--seed", "5", "--trace", str(THRESHOLD), "--trace-steps", "32"])
    lines = capsys.readouterr().out.splitlines()
    traced = [ln for ln in lines if ln.startswith("traced camera")]
    assert [ln for ln in lines if not ln.startswith("traced camera")] == plain
    views = len([f for f in usual if f.endswith("_rgb.png")])
    assert views >= 1 and len(traced) == views
    for k, ln in enumerate(traced):
        assert re.fullmatch(r"traced camera %d: hit share \d\.\d{4}, mean advances per ray \d+\.\d\d, \d+\.\d ms" % k, ln), ln
        rgb, dep = (np.asarray(Image.open(run / "eval" / ("%03d_%s_traced.png" % (k, s)))) for s in ("rgb", "depth"))
        want = np.asarray(Image.open(run / "eval" / ("%03d_rgb.png" % k))).shape
        assert rgb.shape == want and dep.shape == want[:2] and rgb.dtype == np.uint8
    for f, data in usual.items():
        assert (run / "eval" / f).read_bytes() == data, f
