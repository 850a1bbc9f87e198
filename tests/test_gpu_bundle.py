"""Ray bundles on the GPU: NEDDF_UV_RAYS through neddf_raygen and the fused render entry points, NeRFRender.render_bundle and
render_rays_mixed against the per-camera uv path, gradients to hand-built rays, the orthographic camera, the trainer's mixed-view step.

Where two routes must see the same uniforms the test replaces `_rand` on the render instance by a function that hands out rows of
two fixed tensors (first call: the coarse rows, second call: the fine rows), so ray i gets the same uniforms in both routes.

Gates.  Inference outputs and the training forward's per-ray outputs: bit equality (every row's arithmetic is independent of its
neighbours).  Parameter gradients: those of test_gpu_train._check_named (norm within 1e-4 relative, entries within 1e-4 of the largest
entry) against the gradients the per-camera path accumulates; two runs of one weight-gradient pass already differ by 1e-7 .. 2e-7
(tests/test_gpu_pose.py), so bit equality is not asked.  Pose gradients: the 1e-4 base gates of tests/test_gpu_pose.py (`check`).
Orthographic sphere depth: tests/test_gpu_raycast.py holds no closed-form depth of its sphere, so the bound is the one its mesh has by
construction (geometry_check.sphere_sagitta): the facets of the UV sphere lie between the radii r - sagitta and r, hence a ray at the
lateral offset q from the centre meets the mesh at L - sqrt(s^2 - q^2) for some s in [r - sagitta, r], plus 1e-5 for the fp32 casts."""
import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

import geometry_check as gc
import raycast_check as rc
from test_gpu_pose import check
from test_gpu_train import N, T, TRAIN_CFG, _train_cfg

pytestmark = pytest.mark.gpu

SC = SF = 16
W, H = 20, 16
B1 = 257                        # one lane past a 256-lane block of the copy kernel, a ragged 64-row field tile
COUNTS = (37, 0, 1, 58)         # rows per camera of the mixed batch: one camera owns none, one a single row
LOSS_TERMS = {"color", "color_coarse", "mask", "mask_coarse", "fields_penalty", "fields_penalty_coarse"}
# batch_views="single", seed 11, first step on view 0 of test_trainer_run_train_step's dataset: the loss the parent commit returns
PARENT_SINGLE_LOSS = 0.22333687543869019


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def make(dev, bunny_weights, coarse=False, dtype="fp32", kind="neddf"):
    import neddf_amd
    import synth
    if kind == "nerf":
        cfg = dict(synth.NERF_RELU250["kw"], _target_="neddf.network.NeRF")
        state = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.nerf_state(**synth.NERF_RELU250["state"]).items()}
        iteration = synth.NERF_RELU250["iteration"]
    else:
        cfg = dict(TRAIN_CFG, _target_="neddf.network.NeDDF")
        state = {k: torch.from_numpy(v) for k, v in bunny_weights.items()}
        iteration = 1500
    r = neddf_amd.NeRFRender(cfg, sample_coarse=SC, sample_fine=SF, dist_near=2.0, dist_far=6.0, max_dist=6.0, use_coarse_network=coarse,
                             sampling_type="cone")
    r.network_fine.load_state_dict(state)
    if coarse:
        r.network_coarse.load_state_dict(state)
    r.to(dev)
    r.set_iter(iteration)
    r.network_fine.weight_dtype = dtype
    if coarse:
        r.network_coarse.weight_dtype = dtype
    return r


def look_at(eye):
    eye = np.asarray(eye, np.float64)
    z = eye / np.linalg.norm(eye)
    x = np.cross([0.0, 0.0, 1.0], z)
    x /= np.linalg.norm(x)
    return np.concatenate([Rotation.from_matrix(np.stack([x, np.cross(z, x), z], 1)).as_rotvec(), eye]).astype(np.float32)


EYES = ([3.2, -1.9, 1.1], [-2.6, 2.4, 1.4], [0.8, 3.6, -0.9], [-1.7, -3.1, 1.9])


def cameras(dev, perturbed=False):
    """Four pinhole views of the origin from four sides (20 x 16 pixels); `perturbed`: non-zero pose parameters."""
    import neddf_amd
    calib = neddf_amd.PinholeCalib(np.array([28.0, 28.0, W / 2.0, H / 2.0])).to(dev)
    cams = [neddf_amd.Camera(calib, look_at(e)).to(dev) for e in EYES]
    for i, c in enumerate(cams):
        if perturbed:
            c.params.data.copy_(torch.tensor([0.01, -0.02, 0.015, 0.03, -0.01, 0.02]) * (i + 1) / 4)
        c.update_transform()
    return cams


def mixed_batch(dev, seed=5):
    """uv [96, 2] int64 and view_index [96]: COUNTS rows per camera, interleaved in batch order."""
    rng = np.random.default_rng(seed)
    view = rng.permutation(np.repeat(np.arange(len(COUNTS)), COUNTS))
    assert not (np.diff(view) >= 0).all()
    uv = np.stack([rng.integers(0, W, view.size), rng.integers(0, H, view.size)], 1)
    return T(uv, dev), T(view, dev)


def uniforms(dev, B, seed=3):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(B, SC + 1, generator=gen).to(dev), torch.rand(B, SF + 1, generator=gen).to(dev)


def hand_out(render, U, rows=None):
    """The next two `_rand` calls of `render` return the rows `rows` of U[0] (coarse) and U[1] (fine)."""
    queue = [u if rows is None else u[rows] for u in U]

    def _rand(n, cols, device):
        u = queue.pop(0)
        assert tuple(u.shape) == (n, cols), (tuple(u.shape), n, cols)
        return u.clone()
    render._rand = _rand


def same(a, b, what):
    assert list(a) == list(b), (what, list(a), list(b))
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, k)
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (what, k, float((a[k] - b[k]).abs().max()))


def bundle_of(ctx, uv, cam):
    from neddf_amd import Ray
    rd, ro = ctx.raygen(uv, cam.descriptor())
    return Ray(rd, ro)


# ---------------------------------------------------------------------------------------------------------------- 1. bundle == uv
def test_raygen_returns_the_bundle_bits(dev):
    from neddf_amd import Context, Ray
    ctx = Context.get(dev)
    rng = np.random.default_rng(1)
    rows = rng.standard_normal((B1, 6)).astype(np.float32)
    rows[:, :3] /= np.linalg.norm(rows[:, :3], axis=1, keepdims=True)
    rows[7, :3] *= 3.5                                                  # not unit length: nothing normalises it
    bits = rows.view(np.uint32)
    bits[11] = [0x7FC12345, 0xFFC00001, 0x7F800001, 0x7FFFFFFF, 0x80000000, 0x00000001]     # NaN payloads, -0, a denormal
    packed = T(rows, dev)
    for rd, ro in (ctx.raygen(packed, None, bundle=True), ctx.raygen(Ray(packed[:, :3], packed[:, 3:])),
                   ctx.raygen(packed, cameras(dev)[0].descriptor(), bundle=True)):
        assert np.array_equal(N(rd).view(np.uint32), bits[:, :3]) and np.array_equal(N(ro).view(np.uint32), bits[:, 3:])
    rd, ro = ctx.raygen(packed[:0], None, bundle=True)
    assert rd.shape == (0, 3) and ro.shape == (0, 3)


@pytest.mark.parametrize("coarse", [False, True])
def test_bundle_renders_the_uv_bits(dev, bunny_weights, coarse):
    """render_rays inference (every key), with normal_output, render_image_single_pass's entry and the culled variants."""
    from neddf_amd import Ray
    from neddf_amd._lib import SLOT_FINE
    from neddf_amd.occupancy import OccupancyGrid, pack_bits
    r = make(dev, bunny_weights, coarse)
    cam = cameras(dev)[0]
    rng = np.random.default_rng(2)
    uv = T(np.stack([rng.integers(0, W, B1), rng.integers(0, H, B1)], 1), dev)
    U = uniforms(dev, B1)
    with torch.no_grad():
        ctx = r._ctx(dev)
        rays = bundle_of(ctx, uv, cam)
        for normal in (False, True):
            r.normal_output = normal
            hand_out(r, U)
            want = r.render_rays(uv, cam)
            hand_out(r, U)
            got = r.render_bundle(rays)
            assert ("normal" in want) == normal and "weight" in want and "fields_penalty_coarse" in want
            same(got, want, "render_rays normal_output=%s" % normal)
        r.normal_output = False
        # the single-pass entry (render_image_single_pass calls it per batch), plain and with normals
        packed = torch.cat([rays.ray_dir, rays.ray_orig], 1)
        for normal in (False, True):
            outs = []
            for arg, desc, bundle in ((uv, cam.descriptor(), False), (packed, None, True)):
                o = dict(color=torch.empty(B1, 3, device=dev), depth=torch.empty(B1, device=dev), transmittance=torch.empty(B1, device=dev))
                if normal:
                    o["normal"] = torch.empty(B1, 3, device=dev)
                flag = torch.zeros(1, device=dev, dtype=torch.int32)
                ctx.render_rays(arg, desc, r._params(), U[0], None, dict(o, nan_flag=flag), single_slot=SLOT_FINE, bundle=bundle)
                assert int(flag.item()) == 0
                outs.append(o)
            same(outs[1], outs[0], "single pass normals=%s" % normal)
        # the culled variants: a hand-made grid that keeps a ball of cells around the origin and drops the rest of the box
        R = 16
        z, y, x = np.meshgrid(*(np.arange(R) + 0.5 - R / 2,) * 3, indexing="ij")
        dense = x * x + y * y + z * z < (0.3 * R) ** 2
        grid = OccupancyGrid(T(pack_bits(dense).view(np.int32), dev), R, (-1.1,) * 3, (1.1,) * 3)
        assert 0 < dense.sum() < dense.size
        occ = grid.descriptor()
        want = r._render(ctx, uv, cam, U[0], U[1], full=False, normal=True, occupancy=occ)
        got = r._render(ctx, rays, None, U[0], U[1], full=False, normal=True, occupancy=occ)
        plain = r._render(ctx, uv, cam, U[0], U[1], full=False, normal=True)
        same(got, want, "culled")
        assert not torch.equal(plain["color"], want["color"])           # the grid did cull something
        outs = []
        for arg, desc, bundle in ((uv, cam.descriptor(), False), (packed, None, True)):
            o = dict(color=torch.empty(B1, 3, device=dev), depth=torch.empty(B1, device=dev), transmittance=torch.empty(B1, device=dev),
                     normal=torch.empty(B1, 3, device=dev))
            ctx.render_rays(arg, desc, r._params(), U[0], None, dict(o, nan_flag=torch.zeros(1, device=dev, dtype=torch.int32)),
                            single_slot=SLOT_FINE, occupancy=occ, bundle=bundle)
            outs.append(o)
        same(outs[1], outs[0], "single culled")
        # no rays
        del r._rand
        empty = r.render_bundle(Ray(torch.empty(0, 3, device=dev), torch.empty(0, 3, device=dev)))
        assert list(empty) == list(r.render_rays(uv[:0], cam)) and all(v.shape[0] == 0 for v in empty.values())


# ---------------------------------------------------------------------------------------------------------------- 2. mixed, inference
@pytest.mark.parametrize("coarse", [False, True])
def test_mixed_inference_equals_per_camera(dev, bunny_weights, coarse):
    r = make(dev, bunny_weights, coarse)
    cams = cameras(dev)
    uv, view = mixed_batch(dev)
    U = uniforms(dev, uv.shape[0])
    with torch.no_grad():
        hand_out(r, U)
        got = r.render_rays_mixed(uv, view, cams)
        assert all(v.shape[0] == uv.shape[0] for v in got.values())
        for k, cam in enumerate(cams):
            rows = (view == k).nonzero().squeeze(1)
            assert rows.shape[0] == COUNTS[k]
            if not COUNTS[k]:
                continue
            hand_out(r, U, rows)
            want = r.render_rays(uv[rows], cam)
            same({key: v[rows] for key, v in got.items()}, want, "camera %d" % k)
        with pytest.raises(ValueError):
            r.render_rays_mixed(uv, view + 1, cams)
        with pytest.raises(ValueError):
            r.render_rays_mixed(uv, view - 1, cams)


# ---------------------------------------------------------------------------------------------------------------- 3. mixed, training
def _losses():
    from neddf_amd.loss import ColorLoss, FieldsConstraintLoss, MaskBCELoss
    return [ColorLoss(weight=1.0, weight_coarse=0.1), MaskBCELoss(weight=0.05, weight_coarse=0.005),
            FieldsConstraintLoss(weight=0.01, weight_coarse=0.01)]


def _targets(dev, B, rows=None, seed=7):
    rng = np.random.default_rng(seed)
    t = {"color": T(rng.random((B, 3)).astype(np.float32), dev), "mask": T((rng.random(B) < 0.5).astype(np.float32), dev),
         "fields_penalty": torch.zeros(B, device=dev)}
    return t if rows is None else {k: v[rows] for k, v in t.items()}


def _loss(out, target, losses, share=1.0):
    """The training loss; `share` = rows of this call / rows of the batch turns the per-call means into the batch's means."""
    terms = {}
    for f in losses:
        if f.key_output in out:
            terms.update(f(out, target))
    return share * torch.sum(torch.stack(list(terms.values())))


def _grad_close(got, want, what):
    """test_gpu_train._check_named's gates against another pass on the device: norm within 1e-4 relative, entries within 1e-4 of the
    largest entry."""
    got, want = N(got).astype(np.float64), N(want).astype(np.float64)
    nw, scale = np.linalg.norm(want), np.abs(want).max()
    dn, de = abs(np.linalg.norm(got) - nw), np.abs(got - want).max()
    print("%s: norm deviation %.2e of the norm, entry deviation %.2e of the largest entry" % (what, dn / nw, de / scale))
    assert nw > 0 and dn <= 1e-4 * nw and de <= 1e-4 * scale, (what, dn / nw, de / scale)


@pytest.mark.parametrize("dtype", ["fp32", "f16_split"])
def test_mixed_training_equals_per_camera(dev, bunny_weights, dtype):
    r = make(dev, bunny_weights, dtype=dtype)
    cams = cameras(dev)
    uv, view = mixed_batch(dev)
    B = uv.shape[0]
    U = uniforms(dev, B)
    losses = _losses()
    # the existing per-camera path: every camera's rows through render_rays, gradients accumulated
    r.zero_grad()
    per_camera, total = {}, 0.0
    for k, cam in enumerate(cams):
        rows = (view == k).nonzero().squeeze(1)
        if not COUNTS[k]:
            continue
        hand_out(r, U, rows)
        out = r.render_rays(uv[rows], cam)
        assert out["color"].requires_grad
        loss = _loss(out, _targets(dev, B, rows), losses, COUNTS[k] / B)
        loss.backward()
        total += float(loss.item())
        per_camera[k] = (rows, {key: v.detach() for key, v in out.items()})
    want = {n: p.grad.clone() for n, p in r.named_parameters()}
    # the mixed batch as one bundle
    r.zero_grad()
    hand_out(r, U)
    out = r.render_rays_mixed(uv, view, cams)
    assert list(out) == ["weight", "depth", "color", "transmittance", "fields_penalty", "weight_coarse", "depth_coarse", "color_coarse",
                         "transmittance_coarse", "fields_penalty_coarse"]
    for k, (rows, ref) in per_camera.items():
        same({key: v.detach()[rows] for key, v in out.items()}, ref, "camera %d" % k)
    loss = _loss(out, _targets(dev, B), losses)
    loss.backward()
    np.testing.assert_allclose(float(loss.item()), total, rtol=1e-5)
    for n, p in r.named_parameters():
        _grad_close(p.grad, want[n], "%s %s" % (dtype, n))
    assert all(c.params.grad is None for c in cams)                     # pose_gradients is off


# ---------------------------------------------------------------------------------------------------------------- 4. mixed pose gradients
@pytest.mark.parametrize("kind", ["neddf", "nerf"])
def test_mixed_pose_gradients(dev, bunny_weights, kind):
    r = make(dev, bunny_weights, kind=kind)
    r.pose_gradients = True
    uv, view = mixed_batch(dev)
    B = uv.shape[0]
    U = uniforms(dev, B)
    losses = _losses()
    want = {}
    for k in range(len(COUNTS)):
        if not COUNTS[k]:
            continue
        cams = cameras(dev, perturbed=True)
        rows = (view == k).nonzero().squeeze(1)
        hand_out(r, U, rows)
        _loss(r.render_rays(uv[rows], cams[k]), _targets(dev, B, rows), losses, COUNTS[k] / B).backward()
        want[k] = cams[k].params.grad.clone()
    cams = cameras(dev, perturbed=True)
    hand_out(r, U)
    _loss(r.render_rays_mixed(uv, view, cams), _targets(dev, B), losses).backward()
    for k, cam in enumerate(cams):
        if COUNTS[k]:
            assert cam.params.grad is not None and bool(cam.params.grad.any())
            check("%s camera %d d/dparams" % (kind, k), N(cam.params.grad), N(want[k]))
        else:
            assert cam.params.grad is None


# ---------------------------------------------------------------------------------------------------------------- 5. hand-built rays
def test_gradients_reach_hand_built_rays(dev, bunny_weights):
    """render_bundle with leaf rays: their .grad equals what RayFunction's outputs receive on the uv path for the same rays."""
    from neddf_amd import Ray
    r = make(dev, bunny_weights)
    r.pose_gradients = True
    cam = cameras(dev, perturbed=True)[0]
    rng = np.random.default_rng(9)
    B = 70
    uv = T(np.stack([rng.integers(0, W, B), rng.integers(0, H, B)], 1), dev)
    U = uniforms(dev, B)
    losses, target = _losses(), _targets(dev, B)
    seen = {}
    orig = r._render_generated_rays

    def spy(ctx, rd, ro, *a, **kw):
        rd.retain_grad(); ro.retain_grad()
        seen["rd"], seen["ro"] = rd, ro
        return orig(ctx, rd, ro, *a, **kw)
    r._render_generated_rays = spy
    hand_out(r, U)
    out_uv = r.render_rays(uv, cam)
    _loss(out_uv, target, losses).backward()
    del r._render_generated_rays
    rd = seen["rd"].detach().clone().requires_grad_(True)
    ro = seen["ro"].detach().clone().requires_grad_(True)
    hand_out(r, U)
    out = r.render_bundle(Ray(rd, ro))
    same({k: v.detach() for k, v in out.items()}, {k: v.detach() for k, v in out_uv.items()}, "forward")
    _loss(out, target, losses).backward()
    assert rd.grad is not None and ro.grad is not None and bool(rd.grad.any()) and bool(ro.grad.any())
    check("d/dray_dir", N(rd.grad), N(seen["rd"].grad))
    check("d/dray_orig", N(ro.grad), N(seen["ro"].grad))
    # without pose_gradients the rays stay outside the graph
    r.pose_gradients = False
    rd2 = rd.detach().clone().requires_grad_(True)
    hand_out(r, U)
    _loss(r.render_bundle(Ray(rd2, ro.detach())), target, losses).backward()
    assert rd2.grad is None


# ---------------------------------------------------------------------------------------------------------------- 6. orthographic view
def test_orthographic_views(dev, bunny_weights):
    import neddf_amd
    r = make(dev, bunny_weights)
    w, h, scale, L = 64, 48, 40.0, 4.0
    pose = look_at(np.array([1.9, -2.2, 1.1]) * L / np.linalg.norm([1.9, -2.2, 1.1]))
    cam = neddf_amd.Camera(neddf_amd.OrthographicCalib(np.array([scale, scale, w / 2.0, h / 2.0])), pose).to(dev)
    cam.update_transform()
    with pytest.raises(NotImplementedError):
        cam.descriptor()
    idx = torch.arange(w * h, device=dev)
    with torch.no_grad():
        rays = cam.create_rays(torch.stack([idx % w, idx // w], 1))
    R_, T_ = N(cam.R).astype(np.float64), N(cam.T).astype(np.float64)
    rd, ro = N(rays.ray_dir), N(rays.ray_orig)
    assert (rd == rd[0]).all() and np.abs(rd[0] + R_[:, 2]).max() < 1e-6                 # every pixel looks along the camera's -z
    u, v = (np.arange(w) + 0.5 - w / 2.0) / scale, (np.arange(h) + 0.5 - h / 2.0) / scale
    lattice = T_ + u[None, :, None] * R_[:, 0] - v[:, None, None] * R_[:, 1]
    assert np.abs(ro.reshape(h, w, 3) - lattice).max() < 1e-5
    # the mesh view: a sphere about the origin seen from the distance L
    radius, n_lat, n_lon = rc.SPHERE
    vs, ts = gc.uv_sphere(radius, n_lat, n_lon)
    img = r.render_image_mesh(w, h, cam, T(vs, dev), T(ts, dev), ["depth", "transmittance"])
    depth, hit = N(img["depth"]).astype(np.float64), N(img["transmittance"]) == 0
    q = np.hypot(u[None, :], v[:, None])                                                 # the lateral offset of every pixel's ray
    inner = radius - gc.sphere_sagitta(radius, n_lat, n_lon)
    assert abs(np.linalg.norm(T_) - L) < 1e-5 and hit[q < inner - 1e-5].all() and not hit[q > radius + 1e-5].any()
    sure = q < inner - 1e-3
    assert sure.sum() > 100
    t_outer, t_inner = L - np.sqrt(radius ** 2 - q[sure] ** 2), L - np.sqrt(inner ** 2 - q[sure] ** 2)
    assert (depth[sure] >= t_outer - 1e-5).all() and (depth[sure] <= t_inner + 1e-5).all()
    # the volume render through the same camera: the bundle path end to end, against render_bundle on the same rays and uniforms
    torch.manual_seed(4)
    image = r.render_image(w, h, cam, ["color", "depth", "transmittance"], chunk=512)
    assert image["color"].shape == (h, w, 3) and bool(torch.isfinite(image["color"]).all())
    assert float(image["transmittance"].min()) < 0.5 < float(image["transmittance"].max())   # the bunny and the background
    torch.manual_seed(4)
    U_c, U_f = torch.rand(512, SC + 1).to(dev), torch.rand(512, SF + 1).to(dev)         # the first chunk's draws
    head = neddf_amd.Ray(rays.ray_dir[:512].contiguous(), rays.ray_orig[:512].contiguous())
    with torch.no_grad():
        first = r._render(r._ctx(dev), head, None, U_c, U_f, full=False, nan_group=512)
        assert torch.equal(first["color"], image["color"].reshape(-1, 3)[:512]) and torch.equal(first["depth"], image["depth"].reshape(-1)[:512])
        # render_rays with such a camera is render_bundle on its rays
        torch.manual_seed(4)
        a = r.render_bundle(head)
        torch.manual_seed(4)
        same(r.render_rays(torch.stack([idx % w, idx // w], 1)[:512], cam), a, "render_rays, orthographic")
    traced = r.render_image_traced(w, h, cam, ["transmittance"], 0.0275)
    assert traced["transmittance"].shape == (h, w) and 0 < float(traced["transmittance"].mean()) < 1


# ---------------------------------------------------------------------------------------------------------------- 7. trainer
def _trainer(tmp_path, monkeypatch, n=2, **kw):
    from test_host import _make_dataset
    from neddf_amd.config import instantiate
    monkeypatch.chdir(tmp_path)
    _make_dataset(str(tmp_path / "ds"), n=n, w=20, h=16, split="train")
    cfg = _train_cfg(str(tmp_path / "ds"), 32)
    cfg["trainer"].update(kw)
    torch.manual_seed(11)
    tr = instantiate(cfg["trainer"], global_config=cfg, _recursive_=False)
    tr.neural_render.set_iter(0)
    return tr


def test_trainer_mixed_step(dev, tmp_path, monkeypatch):
    tr = _trainer(tmp_path, monkeypatch, batch_views="mixed")
    before = [p.detach().clone() for p in tr.neural_render.get_parameters_list()]
    loss = tr.run_train_step_mixed()
    assert np.isfinite(loss) and loss > 0
    moved = [bool((p.detach() != b).any()) for p, b in zip(tr.neural_render.get_parameters_list(), before)]
    assert all(moved), moved
    assert tr.logger.iteration == 1 and set(tr.logger.last.terms) == LOSS_TERMS
    assert np.isfinite(tr.run_train_step_mixed())


def test_trainer_mixed_step_moves_the_views_it_drew(dev, tmp_path, monkeypatch):
    tr = _trainer(tmp_path, monkeypatch, n=5, batch_views="mixed", optimize_cameras=True, batch_size=4)
    state = torch.get_rng_state()
    drawn = set((torch.rand(4) * 5).to(torch.int64).tolist())
    torch.set_rng_state(state)
    assert 0 < len(drawn) < 5
    assert np.isfinite(tr.run_train_step_mixed())
    for i, cam in enumerate(tr.cameras):
        assert bool(cam.params.detach().any()) == (i in drawn), (i, drawn)
        assert (cam.params.grad is not None) == (i in drawn), (i, drawn)


def test_ground_truth_mixed_rows(dev, tmp_path, monkeypatch):
    """construct_ground_truth_mixed == construct_ground_truth per row, bit for bit: the device stacks and the mixed-size host route."""
    names = ["ColorLoss", "MaskBCELoss", "FieldsConstraintLoss"]
    tr = _trainer(tmp_path, monkeypatch, n=3, batch_views="mixed")
    for route in ("stacks", "host"):
        if route == "host":                 # a second dataset with two sizes: view 1 loses its last rows and columns
            item = dict(tr.dataset[1])
            item["rgb_images"], item["mask_images"] = item["rgb_images"][:13, :17].copy(), item["mask_images"][:13, :17].copy()
            views = [tr.dataset[0], item, tr.dataset[2]]
            tr.dataset = views
            tr._gt_stacks, tr._view_sizes = {}, None
        torch.manual_seed(3)
        tr.batch_size = 64
        view, us, vs = tr.draw_mixed_batch()
        assert len(set(view.tolist())) == 3
        got = tr.construct_ground_truth_mixed(view, us, vs, names)
        assert (tr._ground_truth_stacks(True, True) is not None) == (route == "stacks")
        assert got["color"].shape == (64, 3) and got["mask"].shape == (64,) and got["color"].is_cuda
        assert got["fields_penalty"].shape == (64,) and not got["fields_penalty"].any()
        for b in range(64):
            one = tr.construct_ground_truth(int(view[b]), us[b:b + 1], vs[b:b + 1], names)
            assert torch.equal(got["color"][b:b + 1], one["color"]) and torch.equal(got["mask"][b:b + 1], one["mask"]), (route, b)
        assert float(got["color"].max()) > 0


def test_single_view_step_keeps_the_parent_loss(dev, tmp_path, monkeypatch):
    """batch_views="single" (the default) draws what the parent drew: seed 11, one step on view 0 of the 2-view 20 x 16 dataset gives
    the loss the parent commit gives (recorded by running the parent's run_train_step once; a fixture, not a tolerance)."""
    tr = _trainer(tmp_path, monkeypatch)
    assert tr.batch_views == "single"
    loss = tr.run_train_step(0)
    print("single-view loss, seed 11: %r" % loss)
    assert loss == PARENT_SINGLE_LOSS


# ---------------------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals(dev, bunny_weights):
    import ctypes as C

    from neddf_amd import Context, NeddfError, Ray
    r = make(dev, bunny_weights)
    cam = cameras(dev)[0]
    ctx = r._ctx(dev)
    uv = T(np.array([[3, 4], [5, 6]]), dev)
    rays = bundle_of(ctx, uv, cam)
    packed = torch.cat([rays.ray_dir, rays.ray_orig], 1)
    # NDC plus bundle: the Python layer and the library
    r.ray_space, r.ndc_width, r.ndc_height = "ndc", W, H
    with pytest.raises(NotImplementedError):
        r.render_bundle(rays)
    with pytest.raises(NotImplementedError):
        r.render_rays_mixed(uv, torch.zeros(2, dtype=torch.int64), [cam])
    sentinel = 12345.0
    out = dict(color=torch.full((2, 3), sentinel, device=dev), depth=torch.full((2,), sentinel, device=dev),
               transmittance=torch.full((2,), sentinel, device=dev))
    U = uniforms(dev, 2)
    with pytest.raises(NeddfError, match="NDC"):
        ctx.render_rays(packed, None, r._params(), U[0], U[1], out, bundle=True)
    assert all(bool((v == sentinel).all()) for v in out.values())
    r.ray_space = "world"
    # no pose to differentiate
    with pytest.raises(NeddfError, match="pose"):
        ctx.raygen_backward(rays, cam.descriptor(), torch.ones(2, 3, device=dev), torch.ones(2, 3, device=dev))
    with pytest.raises(NeddfError, match="pose"):
        ctx.raygen_backward(packed, cam.descriptor(), torch.ones(2, 3, device=dev), torch.ones(2, 3, device=dev), bundle=True)
    # a bundle is named, never guessed: a float32 [n, 6] tensor without the keyword is not one, pixels need their camera
    with pytest.raises(NeddfError):
        ctx.raygen(uv, None)
    with pytest.raises(NeddfError):
        ctx.raygen(packed[:, :5].contiguous(), None, bundle=True)
    # uv_type 5 through the raw library
    rd, ro = torch.full((2, 3), sentinel, device=dev), torch.full((2, 3), sentinel, device=dev)
    desc = cam.descriptor()
    rc_ = ctx.lib.neddf_raygen(ctx.h, C.c_void_p(packed.data_ptr()), 5, 2, C.byref(desc), C.c_void_p(rd.data_ptr()), C.c_void_p(ro.data_ptr()),
                               ctx.stream())
    assert rc_ == -1 and b"uv_type" in ctx.lib.neddf_last_error(ctx.h)
    params = r._params()
    from neddf_amd._lib import RenderOutputs
    ro_ = RenderOutputs()
    for k, v in out.items():
        setattr(ro_, k, v.data_ptr())
    for bad in (5, -1):
        rc_ = ctx.lib.neddf_render_rays(ctx.h, C.c_void_p(packed.data_ptr()), bad, 2, C.byref(desc), C.byref(params), C.c_void_p(U[0].data_ptr()),
                                        C.c_void_p(U[1].data_ptr()), C.byref(ro_), ctx.stream())
        assert rc_ == -1
    torch.cuda.synchronize(dev)
    assert bool((rd == sentinel).all()) and bool((ro == sentinel).all()) and all(bool((v == sentinel).all()) for v in out.values())
