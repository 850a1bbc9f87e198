"""Per-row cameras on the GPU: NEDDF_UV_CAMERA_TABLE through neddf_raygen, neddf_raygen_backward and the fused render entry points,
NeRFRender.render_rays_views against render_rays_mixed, the stream contract of the two table launches, the trainer's mixed-view step.

Gates.  Everything the table route computes is defined by the one-camera route: row b of ray generation carries the bits of
neddf_raygen(uv[b], cameras[view[b]]), row v of the backward the bits of neddf_raygen_backward on camera v's rows in batch order (the
table kernel performs that kernel's additions in that kernel's order), and every later stage is the one the bundle route reaches.  So
the gates are bit equality throughout, and +0.0 bits for a camera that owns no row.  The trainer's first mixed step at all-zero pose
parameters composes the poses from products with 0 and 1 only, so its loss is the parent commit's, as a fixture.

Shapes.  Shape A: 1 282 rows over six cameras with (0, 1, 255, 256, 257, 513) rows -- empty, single, either side of the backward's
256-thread stride and of two strides -- shuffled, and sorted by view.  Where two routes must see the same uniforms, test_gpu_bundle's
`hand_out` hands both the same rows."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_bundle import EYES, H, W, _loss, _losses, _targets, _trainer, hand_out, look_at, make, same, uniforms
from test_gpu_train import N, T

pytestmark = pytest.mark.gpu

COUNTS_A = (0, 1, 255, 256, 257, 513)
UV_DTYPES = (torch.float32, torch.int64, torch.int32, torch.int16)
SENTINEL = 12345.0
# batch_views="mixed", seed 11, the first run_train_step_mixed on test_gpu_bundle._trainer(n=5)'s dataset, every pose parameter zero:
# the loss the parent commit returns.  Recorded by running, in a checkout of the parent commit with its library built,
#   python -c "import sys; sys.path[:0] = ['.', 'tests']; import pathlib, tempfile, pytest, test_gpu_bundle as b; \
#              tr = b._trainer(pathlib.Path(tempfile.mkdtemp()), pytest.MonkeyPatch(), n=5, batch_views='mixed'); \
#              print(repr(tr.run_train_step_mixed()))"
PARENT_MIXED_LOSS = 0.23949667811393738


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def six_cameras(dev):
    """Six pinhole views with different poses AND different intrinsics (20 x 16 pixels), non-zero pose parameters."""
    import neddf_amd
    eyes = list(EYES) + [[2.9, 2.2, -1.6], [0.4, -3.9, 0.7]]
    cams = []
    for i, eye in enumerate(eyes):
        calib = neddf_amd.PinholeCalib(np.array([28.0 + 1.5 * i, 27.0 - 0.75 * i, W / 2.0 + 0.25 * i, H / 2.0 - 0.5 * i])).to(dev)
        cam = neddf_amd.Camera(calib, look_at(eye)).to(dev)
        cam.params.data.copy_(torch.tensor([0.01, -0.02, 0.015, 0.03, -0.01, 0.02]) * (i + 1) / 4)
        cam.update_transform()
        cams.append(cam)
    return cams


def table_of(cams):
    """[K,16] rows of (R row-major, T, calib) of the cameras as they stand."""
    with torch.no_grad():
        return torch.stack([torch.cat([c.R.reshape(9), c.T, c.camera_calib.params]).to(torch.float32) for c in cams]).contiguous()


def batch(dev, counts, seed=5, shuffle=True):
    """uv [sum counts, 2] int64 and view int32: counts[k] rows of camera k, shuffled (or sorted by view)."""
    rng = np.random.default_rng(seed)
    view = np.repeat(np.arange(len(counts)), counts)
    if shuffle:
        view = rng.permutation(view)
        assert len(counts) == 1 or not (np.diff(view) >= 0).all()
    uv = np.stack([rng.integers(0, W, view.size), rng.integers(0, H, view.size)], 1)
    return T(uv, dev), T(view.astype(np.int32), dev)


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def world(dev):
    """The cameras, their table and descriptors, and shape A with the per-camera reference of its forward -- computed once."""
    from neddf_amd import Context
    ctx = Context.get(dev)
    cams = six_cameras(dev)
    descs = [c.descriptor() for c in cams]
    uv, view = batch(dev, COUNTS_A)
    return dict(ctx=ctx, cams=cams, descs=descs, table=table_of(cams), uv=uv, view=view)


def per_camera_rays(ctx, uv, view, descs):
    """The reference: every camera's rows through the one-camera neddf_raygen, put back at their batch positions."""
    rd, ro = torch.zeros(uv.shape[0], 3, device=uv.device), torch.zeros(uv.shape[0], 3, device=uv.device)
    for k, desc in enumerate(descs):
        rows = (view == k).nonzero().squeeze(1)
        if rows.numel():
            rd[rows], ro[rows] = ctx.raygen(uv[rows].contiguous(), desc)
    return rd, ro


# ---------------------------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("dtype", UV_DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_forward_equals_per_camera_raygen(world, dev, dtype):
    from neddf_amd._lib import ViewRays
    ctx, descs, table = world["ctx"], world["descs"], world["table"]
    order = torch.argsort(world["view"].long(), stable=True)
    one = batch(dev, (300,), seed=6)
    for what, uv, view, tab, ds in (("shape A", world["uv"], world["view"], table, descs),
                                    ("shape A sorted by view", world["uv"][order], world["view"][order], table, descs),
                                    ("one camera", one[0], one[1], table[3:4].contiguous(), descs[3:4])):
        uv = (uv.to(dtype) + 0.25 if dtype == torch.float32 else uv.to(dtype)).contiguous()
        want = per_camera_rays(ctx, uv, view, ds)
        for index in (view, view.long()):
            got = ctx.raygen(ViewRays(uv, index, tab))
            assert got[0].shape == (uv.shape[0], 3) and got[1].shape == (uv.shape[0], 3)
            assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(bits(got[1]), bits(want[1])), (what, index.dtype)
    assert bool(torch.isfinite(want[0]).all())
    empty = ctx.raygen(ViewRays(world["uv"][:0], world["view"][:0], table))
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3)


# ---------------------------------------------------------------------------------------------------------------- 2. invalid views
def test_invalid_view_rows(world, dev):
    from neddf_amd._lib import ViewRays
    ctx, table, uv = world["ctx"], world["table"], world["uv"]
    V = table.shape[0]
    view = world["view"].clone()
    bad = {3: -1, 257: V, 640: 2 ** 31 - 1, 1281: -2 ** 31}
    for row, value in bad.items():
        view[row] = value
    keep = torch.ones(uv.shape[0], dtype=torch.bool, device=dev)
    keep[list(bad)] = False
    clean = ctx.raygen(ViewRays(uv, world["view"], table))
    for index in (view, view.long(), torch.where(keep, view.long(), torch.tensor(2 ** 40, device=dev))):
        rd, ro = ctx.raygen(ViewRays(uv, index, table))
        assert bool(torch.isnan(rd[~keep]).all()) and bool(torch.isnan(ro[~keep]).all())
        assert torch.equal(bits(rd[keep]), bits(clean[0][keep])) and torch.equal(bits(ro[keep]), bits(clean[1][keep]))
    # the backward: the invalid rows belong to no camera
    g = torch.Generator().manual_seed(8)
    g_rd, g_ro = torch.randn(uv.shape[0], 3, generator=g).to(dev), torch.randn(uv.shape[0], 3, generator=g).to(dev)
    got = ctx.raygen_backward(ViewRays(uv, view, table), None, g_rd, g_ro)
    want = ctx.raygen_backward(ViewRays(uv[keep].contiguous(), view[keep].contiguous(), table), None, g_rd[keep], g_ro[keep])
    assert got.shape == (V, 12) and torch.equal(bits(got), bits(want))
    assert bool(torch.isfinite(got).all())


# ---------------------------------------------------------------------------------------------------------------- 3. backward
def test_backward_equals_per_camera_raygen_backward(world, dev):
    from neddf_amd._lib import ViewRays
    ctx, descs, table, uv, view = (world[k] for k in ("ctx", "descs", "table", "uv", "view"))
    g = torch.Generator().manual_seed(9)
    g_rd, g_ro = torch.randn(uv.shape[0], 3, generator=g).to(dev), torch.randn(uv.shape[0], 3, generator=g).to(dev)
    for dtype in (torch.int64, torch.int16, torch.float32):
        pix = uv.to(dtype).contiguous()
        got = ctx.raygen_backward(ViewRays(pix, view, table), None, g_rd, g_ro)
        assert got.shape == (6, 12) and got.dtype == torch.float32
        for k, desc in enumerate(descs):
            rows = (view == k).nonzero().squeeze(1)                     # ascending: batch order
            assert rows.numel() == COUNTS_A[k]
            g_R, g_T = ctx.raygen_backward(pix[rows].contiguous(), desc, g_rd[rows], g_ro[rows])
            want = torch.cat([g_R.reshape(9), g_T])
            assert torch.equal(bits(got[k]), bits(want)), (dtype, k, float((got[k] - want).abs().max()))
        assert not bits(got[0]).any()                                   # the empty camera: +0.0, not -0.0
        assert bool(got[1:].abs().sum(1).gt(0).all())
        again = ctx.raygen_backward(ViewRays(pix, view, table), None, g_rd, g_ro)
        assert torch.equal(bits(again), bits(got))
    # most cameras empty: 64 rows over 300 cameras
    rng = np.random.default_rng(10)
    wide = T(np.tile(N(table), (50, 1)), dev)
    view_w = T(rng.integers(0, 300, 64).astype(np.int32), dev)
    got = ctx.raygen_backward(ViewRays(uv[:64].contiguous(), view_w, wide), None, g_rd[:64], g_ro[:64])
    assert got.shape == (300, 12)
    for k in range(300):
        rows = (view_w == k).nonzero().squeeze(1)
        if not rows.numel():
            continue
        g_R, g_T = ctx.raygen_backward(uv[rows].contiguous(), descs[k % 6], g_rd[rows], g_ro[rows])
        assert torch.equal(bits(got[k]), bits(torch.cat([g_R.reshape(9), g_T]))), k
    owners = torch.zeros(300, dtype=torch.bool, device=dev)
    owners[view_w.long()] = True
    assert 0 < int(owners.sum()) <= 64 and not bits(got[~owners]).any()
    # no rows at all: every camera's row is written, as zeros
    none = ctx.raygen_backward(ViewRays(uv[:0], view[:0], table), None, g_rd[:0], g_ro[:0])
    assert none.shape == (6, 12) and not bits(none).any()


# ---------------------------------------------------------------------------------------------------------------- 4. fused paths
@pytest.mark.parametrize("coarse", [False, True])
def test_fused_calls_render_the_bundle_bits(world, dev, bunny_weights, coarse):
    """Context.render_rays(ViewRays) against the bundle of the same rays: the two-pass entry (every key, with normals), the
    single-pass entry and both culled variants."""
    from neddf_amd import Ray
    from neddf_amd._lib import SLOT_FINE, ViewRays
    from neddf_amd.occupancy import OccupancyGrid, pack_bits
    B = 257
    r = make(dev, bunny_weights, coarse)
    ctx = r._ctx(dev)
    table = world["table"][:4].contiguous()
    uv, view = batch(dev, (64, 1, 100, 92), seed=12)
    assert uv.shape[0] == B
    U = uniforms(dev, B)
    with torch.no_grad():
        rd, ro = per_camera_rays(ctx, uv, view, world["descs"][:4])
        rays, views = Ray(rd, ro), ViewRays(uv, view, table)
        for normal in (False, True):
            want = r._render(ctx, rays, None, U[0], U[1], full=True, normal=normal)
            got = r._render(ctx, views, None, U[0], U[1], full=True, normal=normal)
            assert int(got["_nan"].item()) == 0 and "weight" in got and ("normal_coarse" in got) == normal
            same(got, want, "two passes, normals=%s" % normal)
        packed = torch.cat([rd, ro], 1)
        R = 16
        z, y, x = np.meshgrid(*(np.arange(R) + 0.5 - R / 2,) * 3, indexing="ij")
        dense = x * x + y * y + z * z < (0.3 * R) ** 2
        occ = OccupancyGrid(T(pack_bits(dense).view(np.int32), dev), R, (-1.1,) * 3, (1.1,) * 3).descriptor()
        want = r._render(ctx, rays, None, U[0], U[1], full=False, normal=True, occupancy=occ)
        got = r._render(ctx, views, None, U[0], U[1], full=False, normal=True, occupancy=occ)
        plain = r._render(ctx, views, None, U[0], U[1], full=False, normal=True)
        same(got, want, "culled")
        assert not torch.equal(plain["color"], want["color"])           # the grid did cull something
        for grid in (None, occ):
            for normal in (False, True):
                outs = []
                for arg, bundle in ((packed, True), (views, False)):
                    o = dict(color=torch.empty(B, 3, device=dev), depth=torch.empty(B, device=dev), transmittance=torch.empty(B, device=dev))
                    if normal:
                        o["normal"] = torch.empty(B, 3, device=dev)
                    flag = torch.zeros(1, device=dev, dtype=torch.int32)
                    ctx.render_rays(arg, None, r._params(), U[0], None, dict(o, nan_flag=flag), single_slot=SLOT_FINE, occupancy=grid,
                                    bundle=bundle)
                    assert int(flag.item()) == 0
                    outs.append(o)
                same(outs[1], outs[0], "single pass, normals=%s, culled=%s" % (normal, grid is not None))


# ---------------------------------------------------------------------------------------------------------------- 5. render_rays_views
def test_render_rays_views_equals_render_rays_mixed(dev, bunny_weights):
    from test_gpu_bundle import cameras
    r = make(dev, bunny_weights)
    uv, view = batch(dev, (37, 80, 1, 58), seed=13)
    view = view.long()
    B = uv.shape[0]
    U = uniforms(dev, B)
    cams = cameras(dev, perturbed=True)
    table = table_of(cams)
    with torch.no_grad():                                               # inference: the fused call
        hand_out(r, U)
        want = r.render_rays_mixed(uv, view, cams)
        hand_out(r, U)
        got = r.render_rays_views(uv, view, table)
        same(got, want, "inference")
        hand_out(r, U)
        same(r.render_rays_views(uv, view.to(torch.int32), table), want, "inference, int32 view")
    hand_out(r, U)                                                      # the training forward
    want = r.render_rays_mixed(uv, view, cams)
    hand_out(r, U)
    got = r.render_rays_views(uv, view, table)
    assert got["color"].requires_grad
    same({k: v.detach() for k, v in got.items()}, {k: v.detach() for k, v in want.items()}, "training forward")
    # pose gradients: the [K,16] table gradient against per-camera RayFunction's (R, T) gradients
    r.pose_gradients = True
    losses, target = _losses(), _targets(dev, B)
    seen = {}
    for cam in cams:
        cam.R.retain_grad()
        cam.T.retain_grad()
    orig = r._render_rays_mixed_per_camera
    hand_out(r, U)
    out = orig(uv, view, cams, [37, 80, 1, 58])                          # the per-camera route: one RayFunction per camera
    _loss(out, target, losses).backward()
    for k, cam in enumerate(cams):
        seen[k] = torch.cat([cam.R.grad.reshape(9), cam.T.grad])
    r.zero_grad()
    leaf = table.clone().requires_grad_(True)
    hand_out(r, U)
    got = r.render_rays_views(uv, view, leaf)
    same({k: v.detach() for k, v in got.items()}, {k: v.detach() for k, v in out.items()}, "pose forward")
    _loss(got, target, losses).backward()
    assert leaf.grad.shape == (4, 16) and not bits(leaf.grad[:, 12:]).any()
    for k in range(4):
        assert torch.equal(bits(leaf.grad[k, :12]), bits(seen[k])), (k, float((leaf.grad[k, :12] - seen[k]).abs().max()))
        assert bool(leaf.grad[k, :12].any())
    # a table that asks for no gradient stays outside the graph
    hand_out(r, U)
    plain = r.render_rays_views(uv, view, table)
    same({k: v.detach() for k, v in plain.items()}, {k: v.detach() for k, v in out.items()}, "pose_gradients, plain table")
    with pytest.raises(ValueError):
        r.render_rays_views(uv, view[:-1], table)
    r.ray_space = "ndc"
    with pytest.raises(NotImplementedError):
        r.render_rays_views(uv, view, table)


# ---------------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_through_the_raw_library(world, dev, bunny_weights):
    from neddf_amd._lib import UV_CAMERA_TABLE, CameraDesc, CameraTableDesc, RenderOutputs
    r = make(dev, bunny_weights)
    ctx = r._ctx(dev)
    lib, table = ctx.lib, world["table"]
    uv, view = world["uv"][:2].contiguous(), world["view"][:2].contiguous()
    rd, ro = torch.full((2, 3), SENTINEL, device=dev), torch.full((2, 3), SENTINEL, device=dev)
    g_RT = torch.full((6, 12), SENTINEL, device=dev)
    ones = torch.ones(2, 3, device=dev)
    out = dict(color=torch.full((2, 3), SENTINEL, device=dev), depth=torch.full((2,), SENTINEL, device=dev),
               transmittance=torch.full((2,), SENTINEL, device=dev))
    ro_ = RenderOutputs()
    for k, v in out.items():
        setattr(ro_, k, v.data_ptr())
    U = uniforms(dev, 2)
    params = r._params()
    p = lambda t: C.c_void_p(t.data_ptr())

    def desc(cameras=table.data_ptr(), views=view.data_ptr(), n=6):
        return C.cast(C.pointer(CameraTableDesc(cameras, views, n)), C.POINTER(CameraDesc))

    def calls(uv_type, d):
        return (lib.neddf_raygen(ctx.h, p(uv), uv_type, 2, d, p(rd), p(ro), ctx.stream()),
                lib.neddf_raygen_backward(ctx.h, p(uv), uv_type, 2, d, p(ones), p(ones), p(g_RT), ctx.stream()),
                lib.neddf_render_rays(ctx.h, p(uv), uv_type, 2, d, C.byref(params), p(U[0]), p(U[1]), C.byref(ro_), ctx.stream()))
    flag = UV_CAMERA_TABLE | 1                                          # int64 pixels
    for what, uv_type, d, word in (("flag on a bundle", UV_CAMERA_TABLE | 4, desc(), b"uv_type"), ("another bit", flag | 0x200, desc(), b"uv_type"),
                                   ("flag | 5", UV_CAMERA_TABLE | 5, desc(), b"uv_type"), ("no cameras", flag, desc(n=0), b"n_cameras"),
                                   ("too many cameras", flag, desc(n=(1 << 20) + 1), b"n_cameras"), ("NULL d_view", flag, desc(views=None), b"NULL"),
                                   ("NULL d_cameras", flag, desc(cameras=None), b"NULL")):
        for rc_ in calls(uv_type, d):
            assert rc_ == -1 and word in lib.neddf_last_error(ctx.h), (what, rc_, lib.neddf_last_error(ctx.h))
    assert lib.neddf_raygen(ctx.h, p(uv), flag, 2, None, p(rd), p(ro), ctx.stream()) == -1
    ndc = r._params()
    ndc.ndc_rays, ndc.ndc_width, ndc.ndc_height, ndc.ndc_near = 1, W, H, 1.0
    assert lib.neddf_render_rays(ctx.h, p(uv), flag, 2, desc(), C.byref(ndc), p(U[0]), p(U[1]), C.byref(ro_), ctx.stream()) == -3
    assert b"NDC" in lib.neddf_last_error(ctx.h)
    torch.cuda.synchronize(dev)
    for t in (rd, ro, g_RT, *out.values()):
        assert bool((t == SENTINEL).all())
    # the same arguments without a mistake are accepted
    assert calls(flag, desc()) == (0, 0, 0)
    torch.cuda.synchronize(dev)
    assert bool(torch.isfinite(rd).all()) and not bool((g_RT == SENTINEL).any()) and not bool((out["color"] == SENTINEL).any())


# ---------------------------------------------------------------------------------------------------------------- 7. stream contract
def test_stream_contract_of_the_table_launches(world, dev):
    """raygen[table] and raygen_backward[table] on a side stream with late inputs, held to tests/stream_check.py as
    tests/test_gpu_streams.py builds it: the two controls first, then the cases."""
    import test_gpu_streams as gs
    from neddf_amd._lib import ViewRays
    from stream_check import StreamCheck
    ctx = world["ctx"]
    st = gs.State()
    st.torch, st.dev, st.ctx, st.h = torch, dev, ctx, StreamCheck(dev)
    rng = np.random.default_rng(20241)
    st.f32 = lambda *shape, lo=0.0, hi=1.0: T(rng.uniform(lo, hi, shape).astype(np.float32), dev)
    uv, view, table = world["uv"], world["view"], world["table"]
    with torch.no_grad():
        st.ray_dir, st.ray_orig = ctx.raygen(uv, world["descs"][2])
        st.dists = ctx.sample_coarse(st.f32(uv.shape[0], 9), 2.0, 6.0)
    torch.cuda.synchronize()
    first = gs._control_streams(st)
    second = gs._control_library(st) if first is None else "inconclusive: the first control did not pass"
    st.h.controls = "; ".join(m for m in (first, second) if m)
    g_rd, g_ro = T(rng.standard_normal((uv.shape[0], 3)).astype(np.float32), dev), T(rng.standard_normal((uv.shape[0], 3)).astype(np.float32), dev)
    st.h.run("raygen[table]", lambda a, b, c: ctx.raygen(ViewRays(a, b, c)), [uv, view, table])
    st.h.run("raygen[table, int64 view]", lambda a, b, c: ctx.raygen(ViewRays(a, b, c)), [uv, view.long(), table])
    st.h.run("raygen_backward[table]", lambda a, b, c, d, e: ctx.raygen_backward(ViewRays(a, b, c), None, d, e), [uv, view, table, g_rd, g_ro])
    assert len(st.h.records) == 3 and all(rec["returned_before_b"] for rec in st.h.records)


# ---------------------------------------------------------------------------------------------------------------- 8. trainer
def test_trainer_mixed_step_has_no_per_view_work(dev, tmp_path, monkeypatch):
    from neddf_amd.camera import Camera
    tr = _trainer(tmp_path, monkeypatch, n=5, batch_views="mixed")
    assert len(tr.camera_set()) == 5                                                     # (built once, with the trainer's cameras)
    counts = {"update_transform": 0, "descriptor": 0, "raygen": 0}

    def counted(name, fn):
        def call(*a, **kw):
            counts[name] += 1
            return fn(*a, **kw)
        return call
    monkeypatch.setattr(Camera, "update_transform", counted("update_transform", Camera.update_transform))
    monkeypatch.setattr(Camera, "descriptor", counted("descriptor", Camera.descriptor))
    from neddf_amd import Context
    ctx = Context.get(dev)

    class Lib:
        def __getattr__(self, name, real=ctx.lib):
            fn = getattr(real, name)
            return counted("raygen", fn) if name == "neddf_raygen" else fn
    monkeypatch.setattr(ctx, "lib", Lib())
    for step in range(3):                                               # three draws
        assert np.isfinite(tr.run_train_step_mixed())
        assert counts == {"update_transform": 0, "descriptor": 0, "raygen": step + 1}, counts


def test_trainer_mixed_step_moves_exactly_the_drawn_views(dev, tmp_path, monkeypatch):
    tr = _trainer(tmp_path, monkeypatch, n=5, batch_views="mixed", optimize_cameras=True, batch_size=4)
    state = torch.get_rng_state()
    drawn = set((torch.rand(4) * 5).to(torch.int64).tolist())
    torch.set_rng_state(state)
    assert 0 < len(drawn) < 5
    assert np.isfinite(tr.run_train_step_mixed())
    for i, cam in enumerate(tr.cameras):
        assert bool(cam.params.detach().any()) == (i in drawn), (i, drawn)
        assert (cam.params.grad is not None) == (i in drawn), (i, drawn)
        if i in drawn:
            assert bool(torch.isfinite(cam.params.grad).all()) and bool(cam.params.grad.any())
    assert tr.camera_set().rebuilds == 0                                # the graph route composes its own table


def test_first_mixed_step_keeps_the_parent_loss(dev, tmp_path, monkeypatch):
    """All pose parameters are zero: the batched poses are the per-camera bits, so the step is the parent's (a fixture, not a tolerance)."""
    tr = _trainer(tmp_path, monkeypatch, n=5, batch_views="mixed")
    assert all(not bool(c.params.any()) for c in tr.cameras)
    loss = tr.run_train_step_mixed()
    print("mixed-view loss, seed 11: %r" % loss)
    assert loss == PARENT_MIXED_LOSS
