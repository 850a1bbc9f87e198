"""Every stream-taking entry point of include/neddf_hip.h on a side stream, with its inputs arriving late (tests/stream_check.py).

The rest of the GPU suite runs on the default stream, where a launch on the null stream, a count read that did not wait for its
stream, a reader that forgets its slot's use mark or a device-wide synchronise in a warm call all give the right answer.  Here each
case makes one Context wrapper call (or one short chain) behind a delay on a side stream whose inputs do not exist yet when the call
is enqueued, and holds the result to the same call on the default stream bit for bit; calls that the header does not document as
synchronising must also return to the host before the delay has ended, the documented ones after it.

TABLE maps every export with a `void *stream` parameter to the test that covers it and to whether the header documents a stream
synchronise; tests/test_streams_host.py holds its keys to the header, test_every_table_row_was_called holds them to what the cases
called (a recording proxy around ctx.lib).  Shapes are the smallest that make every launch of a call happen: more than one block or
tile and a ragged tail.  Every comparison is bit for bit against the default-stream call, which the rest of the suite holds to the
reference; no numerical tolerance appears here.  `pytest -s` prints, per case, the measured host time of the call, the delay chosen
and the delay realised.
"""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

A, S = False, True          # the header's word on the entry point: asynchronous / synchronises `stream`
# export -> (covering test, documented as synchronising)
TABLE = {
    "neddf_raygen": ("test_raygen", A),
    "neddf_sample_coarse": ("test_sample_coarse", A),
    "neddf_sampling": ("test_sampling", A),
    "neddf_sampling_view": ("test_sampling", A),
    "neddf_rays_to_ndc": ("test_rays_to_ndc", A),
    "neddf_composite": ("test_composite", A),
    "neddf_composite_normal": ("test_composite", A),
    "neddf_integrate_penalty": ("test_composite", A),
    "neddf_importance_resample": ("test_importance_resample", A),
    "neddf_op_activation": ("test_layer_ops", A),
    "neddf_op_positional_encoding": ("test_layer_ops", A),
    "neddf_op_pe_weights": ("test_layer_ops", A),
    "neddf_op_linear_grad": ("test_layer_ops", S),
    "neddf_field_forward": ("test_field_forward", A),
    "neddf_field_forward_surface": ("test_field_forward_surface", A),
    "neddf_field_grid": ("test_field_grids", A),
    "neddf_field_grid_coarse": ("test_field_grids", A),
    "neddf_field_bricks": ("test_field_grids", A),
    "neddf_render_rays": ("test_render_rays", A),
    "neddf_render_rays_single": ("test_render_rays", A),
    "neddf_render_rays_surface": ("test_render_rays", A),
    "neddf_render_rays_single_surface": ("test_render_rays", A),
    "neddf_render_rays_culled": ("test_render_rays_culled", S),
    "neddf_render_rays_single_culled": ("test_render_rays_culled", S),
    "neddf_trace_field": ("test_trace_field", S),
    "neddf_train_field_forward": ("test_train_field", A),
    "neddf_train_field_backward": ("test_train_field", A),
    "neddf_train_field_backward_inputs": ("test_train_field", A),
    "neddf_composite_backward": ("test_stage_backwards", A),
    "neddf_sampling_backward": ("test_stage_backwards", A),
    "neddf_raygen_backward": ("test_stage_backwards", A),
    "neddf_marching_cubes": ("test_marching_cubes", S),
    "neddf_brick_select": ("test_brick_pipeline", S),
    "neddf_marching_cubes_bricks": ("test_brick_pipeline", S),
    "neddf_mesh_vertex_normals": ("test_mesh_ops", A),
    "neddf_mesh_components": ("test_mesh_ops", S),
    "neddf_mesh_compact": ("test_mesh_ops", S),
    "neddf_mesh_sample_count": ("test_mesh_sampling", S),
    "neddf_mesh_sample_write": ("test_mesh_sampling", S),
    "neddf_nn_brute": ("test_nearest_neighbours", A),
    "neddf_nn_grid_build": ("test_nearest_neighbours", S),
    "neddf_nn_grid_query": ("test_nearest_neighbours", A),
    "neddf_raycast_brute": ("test_raycast_and_point_mesh_grid", A),
    "neddf_raycast_grid_count": ("test_raycast_and_point_mesh_grid", S),
    "neddf_raycast_grid_build": ("test_raycast_and_point_mesh_grid", S),
    "neddf_raycast_grid_query": ("test_raycast_and_point_mesh_grid", A),
    "neddf_point_mesh_brute": ("test_raycast_and_point_mesh_grid", A),
    "neddf_point_mesh_grid_query": ("test_raycast_and_point_mesh_grid", A),
    "neddf_bvh_keys": ("test_bvh", A),
    "neddf_bvh_build": ("test_bvh", A),
    "neddf_point_mesh_bvh_query": ("test_bvh", A),
    "neddf_raycast_bvh_query": ("test_bvh", A),
    "neddf_raycast_bvh_occluded": ("test_bvh", A),
    "neddf_mesh_simplify_keys": ("test_simplify_steps", A),
    "neddf_mesh_simplify_clusters": ("test_simplify_steps", S),
    "neddf_mesh_simplify_pairs": ("test_simplify_steps", S),
    "neddf_mesh_simplify_place": ("test_simplify_steps", A),
    "neddf_mesh_simplify_attributes": ("test_simplify_steps", A),
    "neddf_mesh_simplify_triangles": ("test_simplify_steps", A),
    "neddf_mesh_simplify_unique": ("test_simplify_steps", A),
    "neddf_occupancy_build": ("test_occupancy", S),
    "neddf_occupancy_classify": ("test_occupancy", A),
    "neddf_occupancy_gather": ("test_occupancy", S),
    "neddf_occupancy_scatter": ("test_occupancy", A),
    "neddf_trace_begin": ("test_trace_steps", A),
    "neddf_trace_compact": ("test_trace_steps", S),
    "neddf_trace_advance": ("test_trace_steps", A),
    "neddf_trace_finish": ("test_trace_steps", A),
    "neddf_trace_bisect_points": ("test_trace_steps", S),
    "neddf_trace_bisect_update": ("test_trace_steps", A),
}
# stream-taking exports without a case here, each with its reason
EXCLUDED = {
    "neddf_gather_pixels": "needs an RCCL communicator; exercised in tests/test_gpu_multi.py",
    "neddf_gather_pixels_granular": "needs an RCCL communicator; exercised in tests/test_gpu_multi.py",
    "neddf_comm_wait": "needs an RCCL communicator; exercised in tests/test_gpu_multi.py",
}

N_POINTS, N_RAYS, N_SAMPLES = 229, 257, 17          # three 64-row tiles and a ragged 37; two blocks of rays and one more
RADIUS = 1.0 / 1111 / math.sqrt(12)
LO, HI = (-1.2, -1.2, -1.2), (1.2, 1.2, 1.2)


class State:
    pass


@pytest.fixture(scope="module")
def st():
    import torch

    import neddf_amd
    import synth
    from conftest import golden
    from neddf_amd._lib import Context
    from stream_check import Recorder, StreamCheck
    assert torch.cuda.is_available()
    s = State()
    s.torch, s.dev = torch, torch.device("cuda:0")
    torch.cuda.set_device(0)
    s.ctx = Context.get(s.dev)
    s.calls, s.by_test, s.passed = set(), {}, set()
    s.real_lib = s.ctx.lib
    s.ctx.lib = Recorder(s.real_lib, s.calls)
    s.h = StreamCheck(s.dev)
    s.T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(s.dev)
    rng = np.random.default_rng(20240)
    s.rng = rng
    s.f32 = lambda *shape, lo=0.0, hi=1.0: s.T(rng.uniform(lo, hi, shape).astype(np.float32))
    s.normal = lambda *shape: s.T(rng.standard_normal(shape).astype(np.float32))
    cls = {"neddf": neddf_amd.NeDDF, "nerf": neddf_amd.NeRF, "neus": neddf_amd.NeuS}

    def module(name, seed=synth.NONFINITE_STATE_SEED):
        kind, kw = synth.NONFINITE_NETS[name]
        net = cls[kind](**kw)
        net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.arch_state(kind, dict(kw), seed).items()})
        net = net.to(s.dev)
        net.set_iter(-1)
        return net
    s.module = module
    s.nets = {"neddf": module("neddf_tanhexp"), "nerf": module("nerf_relu"), "neus": module("neus_relu")}
    (pos, d, var), _ = synth.nonfinite_inputs()
    s.points = [s.T(a.reshape(-1, 3)) for a in (pos, d, var)]
    g = golden("bunny_stages.npz")
    s.g = g
    cam = neddf_amd.Camera(neddf_amd.PinholeCalib(g["calib"].astype(np.float64)), None).to(s.dev)
    cam.R, cam.T = s.T(g["R"]), s.T(g["T"])
    s.camera, s.cam = cam, cam.descriptor()
    idx = torch.arange(N_RAYS, device=s.dev)
    s.uv = torch.stack([idx % 23 * 17, idx // 23 * 31], 1).contiguous()            # int64 pixels of a 400 x 400 view
    with torch.no_grad():
        s.ray_dir, s.ray_orig = s.ctx.raygen(s.uv, s.cam)
        s.dists = s.ctx.sample_coarse(s.f32(N_RAYS, N_SAMPLES), 2.0, 6.0)
        s.pos, s.dir, s.var = s.ctx.sampling(s.ray_dir, s.ray_orig, s.dists, RADIUS)
    torch.cuda.synchronize()
    s.ctl = [_control_streams(s), None]
    s.ctl[1] = _control_library(s) if s.ctl[0] is None else "inconclusive: the first control did not pass"
    s.h.controls = "; ".join(m for m in s.ctl if m)
    yield s
    s.ctx.lib = s.real_lib


@pytest.fixture(autouse=True)
def _record(request, st):
    """Which neddf_* functions the test called, and whether it passed (the later cases that traverse a structure ask for the
    cases that checked its build)."""
    if st.h.dead is not None:          # a device error earlier: nothing more is started
        st.h.require_controls()
    before = set(st.calls)
    st.calls.clear()
    yield
    name = request.node.originalname or request.node.name
    st.by_test.setdefault(name, set()).update(st.calls)
    st.calls.update(before)


def _done(st, request):
    st.passed.add(request.node.originalname or request.node.name)


def _need(st, *tests):
    from stream_check import Inconclusive
    missing = [t for t in tests if t not in st.passed]
    if missing:
        raise Inconclusive("inconclusive: %s did not pass before; the structures this case walks are unchecked" % ", ".join(missing))


# ---------------------------------------------------------------------------------------------------------------- controls
# Both run when the module's state is made, before any case; a case whose controls failed reports inconclusive (StreamCheck.run).
def _control_streams(st):
    """Torch only: delay plus copy pending on the side stream, the buffer read on the default stream straight away still holds zeros --
    side streams of this build do not implicitly order with the default stream, and the delay is effective.  None, or what went wrong."""
    torch, h = st.torch, st.h
    src = st.f32(4096, lo=1.0, hi=2.0)
    dst = torch.zeros_like(src)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(h.side):
        a.record()
        h.enqueue_delay(50.0)
        b.record()
        dst.copy_(src)
    early = dst.clone()                 # default stream, no wait
    torch.cuda.current_stream().synchronize()
    fired = b.query()
    h.side.synchronize()
    realised = a.elapsed_time(b)
    print("control 1: delay asked 50.0 ms, realised %.1f ms" % realised)
    if realised < 50.0:
        return "inconclusive: delay too short (realised %.2f ms of 50)" % realised
    if fired:
        return "inconclusive: delay too short (it had ended when the default stream's read returned)"
    if int((early != 0).sum().item()):
        return "the default stream saw the side stream's copy: side streams are ordered with the default stream on this build"
    return None if bool(torch.equal(dst, src)) else "the side stream's copy did not arrive"


def _control_library(st):
    """Through the library: with delay plus copy pending on the side stream, Context.sampling on the default stream gives what sampling
    of all-zero inputs gives, bit for bit -- a mis-ordered library launch is visible through the comparison every case uses."""
    from stream_check import compare, flatten
    torch, h, ctx = st.torch, st.h, st.ctx
    real = [st.ray_dir, st.ray_orig, st.dists]
    zero_ref = [t.clone() for t in ctx.sampling(*[torch.zeros_like(t) for t in real], RADIUS)]
    real_ref = [t.clone() for t in ctx.sampling(*real, RADIUS)]
    torch.cuda.synchronize()
    if compare(flatten(zero_ref), flatten(real_ref), "sampling") is None:
        return "sampling of zeros equals sampling of the inputs: the control shows nothing"
    late = [torch.zeros_like(t) for t in real]
    b = torch.cuda.Event()
    torch.cuda.synchronize()
    with torch.cuda.stream(h.side):
        h.enqueue_delay(50.0)
        b.record()
        for z, r in zip(late, real):
            z.copy_(r)
    out = [t.clone() for t in ctx.sampling(*late, RADIUS)]          # explicitly on the default stream
    torch.cuda.current_stream().synchronize()
    fired = b.query()
    h.side.synchronize()
    if fired:
        return "inconclusive: delay too short"
    return compare(flatten(out), flatten(zero_ref), "sampling on the default stream ahead of the side stream's copy")


def test_control_side_stream_is_not_ordered_with_the_default_stream(st):
    assert st.ctl[0] is None, st.ctl[0]


def test_control_a_default_stream_library_call_sees_the_zeros(st):
    assert st.ctl[1] is None, st.ctl[1]


# ---------------------------------------------------------------------------------------------------------------- stages
def test_raygen(st, request):
    ctx = st.ctx
    st.h.run("raygen[int64 uv]", lambda uv: ctx.raygen(uv, st.cam), [st.uv])
    st.h.run("raygen[float uv]", lambda uv: ctx.raygen(uv, st.cam), [st.uv.to(st.torch.float32) + 0.25])
    _done(st, request)


def test_sample_coarse(st, request):
    st.h.run("sample_coarse", lambda U: st.ctx.sample_coarse(U, 2.0, 6.0), [st.f32(N_RAYS, N_SAMPLES)])
    _done(st, request)


def test_sampling(st, request):
    ctx, late = st.ctx, [st.ray_dir, st.ray_orig, st.dists]
    st.h.run("sampling[cone]", lambda rd, ro, t: ctx.sampling(rd, ro, t, RADIUS), late)
    st.h.run("sampling[point]", lambda rd, ro, t: ctx.sampling(rd, ro, t, None), late)
    st.h.run("sampling_view", lambda rd, ro, t, vd: ctx.sampling(rd, ro, t, RADIUS, view_dir=vd), late + [st.normal(N_RAYS, 3)])
    _done(st, request)


def test_rays_to_ndc(st, request):
    st.h.run("rays_to_ndc", lambda rd, ro: st.ctx.rays_to_ndc(rd, ro, 400, 400, 500.0, 500.0, 1.0), [st.ray_dir, st.ray_orig])
    _done(st, request)


def test_composite(st, request):
    ctx = st.ctx
    dens, col = st.f32(N_RAYS, N_SAMPLES, hi=3.0), st.f32(N_RAYS, N_SAMPLES, 3)
    st.h.run("composite", lambda t, d, c: ctx.composite(t, d, c, 6.0), [st.dists, dens, col])
    st.h.run("composite_normal", lambda t, d, n: ctx.composite_normal(t, d, n), [st.dists, dens, st.normal(N_RAYS, N_SAMPLES, 3)])
    st.h.run("integrate_penalty", lambda t, p: ctx.integrate_penalty(t, p), [st.dists, st.f32(N_RAYS, N_SAMPLES)])
    _done(st, request)


def test_importance_resample(st, request):
    """The weights are sanitised in place: every run starts from a fresh copy and the sanitised weights are compared too."""
    ctx = st.ctx
    w = st.f32(N_RAYS, N_SAMPLES - 1, lo=-0.1, hi=1.0)

    def fn(t, w, U):
        out, ids = ctx.importance_resample(t, w, U, True, True)
        return out, ids, w
    st.h.run("importance_resample", fn, [st.dists, w, st.f32(N_RAYS, 33)])
    _done(st, request)


def test_layer_ops(st, request):
    ctx, torch = st.ctx, st.torch
    x, J = st.normal(N_POINTS, 128), st.normal(N_POINTS, 3, 128)
    st.h.run("op_activation", lambda x, J: ctx.op_activation(2, x, J), [x, J])
    st.h.run("op_activation[plain]", lambda x: ctx.op_activation(2, x), [x])
    p, Jp, sc = st.normal(N_POINTS, 3), st.normal(N_POINTS, 3, 3), st.f32(N_POINTS, 18)
    st.h.run("op_positional_encoding", lambda p, J, sc: ctx.op_positional_encoding(p, J, sc, 6), [p, Jp, sc])
    st.h.run("op_pe_weights", lambda v: ctx.op_pe_weights(v, 6), [st.points[2]])
    W, b = torch.from_numpy(st.rng.standard_normal((70, 130)).astype(np.float32)), torch.from_numpy(st.rng.standard_normal(130).astype(np.float32))
    # the weights are HOST arrays packed and uploaded per call: the call waits for its stream (include/neddf_hip.h)
    st.h.run("op_linear_grad", lambda x, J: ctx.op_linear_grad(x, J, W, b), [st.normal(N_POINTS, 70), st.normal(N_POINTS, 3, 70)], synchronising=True)
    _done(st, request)


# ---------------------------------------------------------------------------------------------------------------- fields
WANT = {("neddf", "full"): ("distance", "density", "color", "fields_penalty", "aux_grad"), ("neddf", "minimal"): ("distance", "density", "color", "aux_grad"),
        ("nerf", "full"): ("density", "color"), ("nerf", "minimal"): ("density", "color"),
        ("neus", "full"): ("distance", "density", "color"), ("neus", "minimal"): ("distance", "density", "color")}


def _load(st, kind, dtype, slot=2):
    net = st.nets[kind]
    net.weight_dtype = dtype
    net.upload(st.ctx, slot)
    return net


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "f16_split"])
@pytest.mark.parametrize("kind,mode", sorted(WANT))
def test_field_forward(st, request, kind, mode, dtype):
    from neddf_amd._lib import OUT_FULL, OUT_MINIMAL
    _load(st, kind, dtype)
    om, want = OUT_FULL if mode == "full" else OUT_MINIMAL, WANT[kind, mode]
    st.h.run("field_forward[%s,%s,%s]" % (kind, mode, dtype), lambda p, d, v: st.ctx.field_forward(2, p, d, v, om, want), st.points)
    _done(st, request)


@pytest.mark.parametrize("kind", ["neddf", "neus"])
def test_field_forward_surface(st, request, kind):
    from neddf_amd._lib import OUT_MINIMAL
    _load(st, kind, "fp32")
    want = WANT[kind, "full" if kind == "neus" else "minimal"] + ("distance_grad", "normal")
    st.h.run("field_forward_surface[%s]" % kind, lambda p, d, v: st.ctx.field_forward_surface(2, p, d, v, OUT_MINIMAL, want), st.points)
    _done(st, request)


def test_field_grids(st, request):
    """The lattice calls take no device input: their case is the order of the outputs on the stream and that they do not block."""
    ctx = st.ctx
    _load(st, "neddf", "fp32")
    shape = (24, 24, 24)
    st.h.run("field_grid", lambda: ctx.field_grid(2, "distance", (17, 9, 13), LO, HI), [])
    st.h.run("field_grid_coarse", lambda: ctx.field_grid_coarse(2, "distance", shape, 8, LO, HI), [])
    ids = st.T(np.array([0, 5, 13, 26], np.int32))
    st.h.run("field_bricks", lambda: ctx.field_bricks(2, "distance", shape, 8, LO, HI, ids), [])
    _done(st, request)


def _renderer(st, use_coarse=False):
    import synth
    import neddf_amd
    kind, kw = synth.NONFINITE_NETS["neddf_relu"]
    r = neddf_amd.NeRFRender(dict(kw, _target_="neddf.network.NeDDF"), sample_coarse=16, sample_fine=32, dist_near=2.0, dist_far=6.0, max_dist=6.0,
                             use_coarse_network=use_coarse, sampling_type="cone")
    r.network_fine.load_state_dict({k: st.torch.from_numpy(np.asarray(v)) for k, v in synth.nonfinite_state("neddf_relu").items()})
    r.to(st.dev)
    r.set_iter(-1)
    return r


def _render_fn(st, r, single, normal, occupancy=None):
    from neddf_amd.render import SLOT_FINE
    torch, ctx, B, Sc, S2 = st.torch, st.ctx, 64, 16, 16 + 32 + 2
    params = r._params()

    def fn(uv, U_c, U_f):
        buf = lambda *s: torch.empty(*s, device=st.dev, dtype=torch.float32)
        o = dict(color=buf(B, 3), depth=buf(B), transmittance=buf(B))
        if not single:
            o.update(weight=buf(B, S2 - 1), color_coarse=buf(B, 3), depth_coarse=buf(B), transmittance_coarse=buf(B), weight_coarse=buf(B, Sc),
                     dists_coarse=buf(B, Sc + 1), dists_fine=buf(B, S2))
            if occupancy is None:           # (a culled sample has no penalty: the library refuses the output with a grid)
                o.update(fields_penalty=buf(B), fields_penalty_coarse=buf(B))
        if normal:
            o["normal"] = buf(B, 3)
            if not single:
                o["normal_coarse"] = buf(B, 3)
        flag = torch.zeros(1, device=st.dev, dtype=torch.int32)
        ctx.render_rays(uv, st.cam, params, U_c, None if single else U_f, dict(o, nan_flag=flag), single_slot=SLOT_FINE if single else None,
                        occupancy=occupancy)
        return o, flag
    return fn


def _render_inputs(st):
    g = st.g
    return [st.T(g["uv"]), st.T(g["u_coarse"][:, :17]), st.T(g["u_fine"][:, :33])]


def test_render_rays(st, request):
    """The hierarchical route (16 + 32 samples, 64 rays) and the single-pass route, with and without the normal target; the NaN flag
    is among the outputs."""
    r = _renderer(st)
    r._ctx(st.dev)
    late = _render_inputs(st)
    for single in (False, True):
        for normal in (False, True):
            st.h.run("render_rays[%s%s]" % ("single" if single else "hierarchical", ",normal" if normal else ""), _render_fn(st, r, single, normal), late)
    _done(st, request)


def test_render_rays_culled(st, request):
    """render_rays with an occupancy grid: one synchronise of the stream per pass (the host learns the number of kept samples)."""
    from neddf_amd.occupancy import OccupancyGrid
    r = _renderer(st)
    r._ctx(st.dev)
    grid = OccupancyGrid.from_field(r.network_fine, resolution=16, cube_range=1.1, threshold=0.0, dilate=1)
    st.torch.cuda.synchronize()
    occ = grid.descriptor()
    late = _render_inputs(st)
    st.h.run("render_rays_culled", _render_fn(st, r, False, False, occ), late, synchronising=True)
    st.h.run("render_rays_single_culled", _render_fn(st, r, True, False, occ), late, synchronising=True)
    _done(st, request)


def test_trace_field(st, request):
    from neddf_amd.trace import trace_params
    _load(st, "neddf", "fp32")
    o, d = _trace_rays(st)
    p = trace_params(threshold=0.05, t_near=0.5, t_far=6.0, max_steps=8, refine=2)
    st.h.run("trace_field", lambda o, d: st.ctx.trace_field(2, o, d, p), [o, d], synchronising=True)
    _done(st, request)


# ---------------------------------------------------------------------------------------------------------------- training
@pytest.mark.parametrize("kind", ["neddf", "nerf", "neus"])
def test_train_field(st, request, kind):
    """Forward and backward through neddf_amd.autograd under the side stream, the upstream gradients late; NeDDF and NeRF also with the
    gradient of the sample positions (neddf_train_field_backward_inputs)."""
    import synth
    from neddf_amd import Sampling
    torch = st.torch
    net = st.module({"neddf": "neddf_relu", "nerf": "nerf_relu", "neus": "neus_relu"}[kind])
    net.set_iter(2500)
    keys = [k for k in synth.FIELD_KEYS[kind]]
    ups = [st.normal(N_POINTS, 1, 3) if k == "color" else st.normal(N_POINTS, 1) for k in keys]
    params = list(net.parameters())

    def make(inputs_grad):
        def fn(pos, d, var, *up):
            for p in params:
                p.grad = None
            pos = pos.view(N_POINTS, 1, 3).requires_grad_(inputs_grad)
            with torch.enable_grad():
                o = net(Sampling(pos, d.view(N_POINTS, 1, 3), var.view(N_POINTS, 1, 3)))
                loss = sum((o[k] * u).sum() for k, u in zip(keys, up))
                loss.backward()
            return [o[k].detach() for k in keys], [p.grad for p in params], pos.grad
        return fn
    # The parameter gradients (out[1]) are sums by floating-point atomics across workgroups (train_kernels.hip): no two runs on any
    # stream give the same bits, so they are held to the bound of a reordered fp32 sum of N_POINTS terms (stream_check.within_reordering);
    # the forward outputs and the input gradients are bit for bit.  (The autograd engine may wait for nothing here either: the calls it makes are the library's asynchronous ones.)
    loose = lambda n: n.startswith("out[1]")
    st.h.run("train_field[%s]" % kind, make(False), st.points + ups, reordered=loose, n_terms=N_POINTS)
    if kind != "neus":
        st.h.run("train_field[%s,input gradients]" % kind, make(True), st.points + ups, reordered=loose, n_terms=N_POINTS)
    _done(st, request)


def test_stage_backwards(st, request):
    ctx = st.ctx
    dens, col = st.f32(N_RAYS, N_SAMPLES, hi=3.0), st.f32(N_RAYS, N_SAMPLES, 3)
    gs = [st.normal(N_RAYS, N_SAMPLES - 1), st.normal(N_RAYS), st.normal(N_RAYS, 3), st.normal(N_RAYS)]
    st.h.run("composite_backward", lambda t, d, c, *g: ctx.composite_backward(t, d, c, 6.0, *g), [st.dists, dens, col] + gs)
    g3 = [st.normal(N_RAYS, N_SAMPLES, 3) for _ in range(3)]
    st.h.run("sampling_backward", lambda a, b, c, rd, t: ctx.sampling_backward(a, b, c, rd, t, RADIUS), g3 + [st.ray_dir, st.dists])
    st.h.run("raygen_backward", lambda uv, a, b: ctx.raygen_backward(uv, st.cam, a, b), [st.uv, st.normal(N_RAYS, 3), st.normal(N_RAYS, 3)])
    _done(st, request)


# ---------------------------------------------------------------------------------------------------------------- geometry
def _volume(st):
    """|p - c| - r of an off-centre sphere on the 17 x 9 x 13 lattice over LO .. HI, [nz, ny, nx]."""
    x, y, z = (np.linspace(LO[a], HI[a], n) for a, n in enumerate((17, 9, 13)))
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    return st.T((np.sqrt((X - 0.1) ** 2 + (Y + 0.05) ** 2 + (Z - 0.2) ** 2) - 0.8).astype(np.float32))


def _sphere_mesh(st):
    if not hasattr(st, "mesh"):
        v, t = st.ctx.marching_cubes(_volume(st), 0.0, LO, HI)
        st.torch.cuda.synchronize()
        assert t.shape[0] > 256
        st.mesh = (v, t)
    return st.mesh


def _soup(st):
    import raycast_check
    if not hasattr(st, "soup"):
        v, t = raycast_check.soup(300, seed=11)
        o, d = raycast_check.soup_rays(v, t, N_RAYS, seed=12)
        st.soup, st.soup_rays = (st.T(v), st.T(t)), (st.T(o), st.T(d))
    return st.soup + st.soup_rays


def test_marching_cubes(st, request):
    st.h.run("marching_cubes", lambda vol: st.ctx.marching_cubes(vol, 0.0, LO, HI), [_volume(st)], synchronising=True)
    _done(st, request)


def test_brick_pipeline(st, request):
    """brick_select on late corner values; marching_cubes_bricks on late brick values with the id list and slot map, which the kernels
    walk, built before and checked against the default-stream build."""
    ctx, torch = st.ctx, st.torch
    _load(st, "neddf", "fp32")
    shape = (24, 24, 24)
    coarse = ctx.field_grid_coarse(2, "distance", shape, 8, LO, HI)
    iso = float(coarse.median())
    st.h.run("brick_select", lambda c: ctx.brick_select(c, iso, 0.02, 1), [coarse], synchronising=True)
    ref = ctx.brick_select(coarse, iso, 0.02, 1)
    torch.cuda.synchronize()
    slot_map, ids = st.h.build_on_side("brick_select", lambda: ctx.brick_select(coarse, iso, 0.02, 1), ref)
    assert ids.shape[0] >= 2
    values = ctx.field_bricks(2, "distance", shape, 8, LO, HI, ids)
    torch.cuda.synchronize()
    st.h.run("marching_cubes_bricks", lambda v: ctx.marching_cubes_bricks(v, ids, slot_map, shape, 8, iso, LO, HI), [values], synchronising=True)
    _done(st, request)


def test_mesh_ops(st, request):
    ctx = st.ctx
    v, t = _sphere_mesh(st)
    keep = st.T((st.rng.uniform(size=t.shape[0]) < 0.6).astype(np.uint8))
    st.h.run("mesh_vertex_normals", lambda v, t: ctx.mesh_vertex_normals(v, t), [v, t])
    st.h.run("mesh_components", lambda t: ctx.mesh_components(t, v.shape[0]), [t], synchronising=True)
    st.h.run("mesh_compact", lambda v, t, k: ctx.mesh_compact(v, t, k), [v, t, keep], synchronising=True)
    _done(st, request)


def test_mesh_sampling(st, request):
    ctx = st.ctx
    v, t, _, _ = _soup(st)
    n = ctx.mesh_sample_count(v, t, 60.0, 7)
    assert n > 512
    st.h.run("mesh_sample_count", lambda v, t: ctx.mesh_sample_count(v, t, 60.0, 7), [v, t], synchronising=True)
    st.h.run("mesh_sample_write", lambda v, t: ctx.mesh_sample_write(v, t, 60.0, 7, n), [v, t], synchronising=True)
    _done(st, request)


def test_nearest_neighbours(st, request):
    """5000 points: the cross-block scan of the grid build."""
    from stream_check import sort_lists
    ctx, torch = st.ctx, st.torch
    q, tg = st.f32(5000, 3, lo=-1.0, hi=1.0), st.f32(5000, 3, lo=-1.0, hi=1.0)
    cells = (9, 9, 9)
    st.h.run("nn_brute", lambda q, t: ctx.nn_brute(q, t), [q[:1025].contiguous(), tg])
    canon = lambda out: (out[0], sort_lists(out[0], out[1]))        # the order inside a cell may depend on timing (include/neddf_hip.h)
    st.h.run("nn_grid_build", lambda t: ctx.nn_grid_build(t, LO, HI, cells), [tg], synchronising=True, canon=canon)
    ref = ctx.nn_grid_build(tg, LO, HI, cells)
    torch.cuda.synchronize()
    start, order = st.h.build_on_side("nn_grid_build", lambda: ctx.nn_grid_build(tg, LO, HI, cells), ref, canon=canon)
    st.h.run("nn_grid_query", lambda q: ctx.nn_grid_query(q, tg, LO, HI, cells, start, order), [q])
    _done(st, request)


def test_raycast_and_point_mesh_grid(st, request):
    from neddf_amd.raycast import default_pad
    from stream_check import sort_lists
    ctx, torch = st.ctx, st.torch
    v, t, o, d = _soup(st)
    inf, pad, cells = float("inf"), default_pad(LO, HI), (7, 6, 5)
    q = st.f32(N_POINTS, 3, lo=-1.1, hi=1.1)
    st.h.run("raycast_brute", lambda o, d, v, t: ctx.raycast_brute(o, d, v, t, 0.0, inf, pad), [o, d, v, t])
    st.h.run("point_mesh_brute", lambda q, v, t: ctx.point_mesh_brute(q, v, t), [q, v, t])
    st.h.run("raycast_grid_count", lambda v, t: ctx.raycast_grid_count(v, t, LO, HI, cells, pad), [v, t], synchronising=True)
    n = ctx.raycast_grid_count(v, t, LO, HI, cells, pad)
    canon = lambda out: (out[0], sort_lists(out[0], out[1]))        # the order inside a list may depend on timing (include/neddf_hip.h)
    st.h.run("raycast_grid_build", lambda v, t: ctx.raycast_grid_build(v, t, LO, HI, cells, pad, n), [v, t], synchronising=True, canon=canon)
    ref = ctx.raycast_grid_build(v, t, LO, HI, cells, pad, n)
    torch.cuda.synchronize()
    start, items = st.h.build_on_side("raycast_grid_build", lambda: ctx.raycast_grid_build(v, t, LO, HI, cells, pad, n), ref, canon=canon)
    st.h.run("raycast_grid_query", lambda o, d: ctx.raycast_grid_query(o, d, v, t, LO, HI, cells, pad, start, items, 0.0, inf), [o, d])
    st.h.run("point_mesh_grid_query", lambda q: ctx.point_mesh_grid_query(q, v, t, LO, HI, cells, pad, start, items), [q])
    _done(st, request)


def test_bvh(st, request):
    """Keys and build on late vertices and indices (the sorted keys are a structure: resident); the tree is then built under the side
    stream, its sort included, compared with the default-stream tree, and only then walked by the three queries on late rays / points."""
    from neddf_amd.raycast import default_pad
    ctx, torch = st.ctx, st.torch
    v, t, o, d = _soup(st)
    inf, pad = float("inf"), default_pad(LO, HI)
    st.h.run("bvh_keys", lambda v, t: ctx.bvh_keys(v, t, LO, HI), [v, t])
    keys = torch.sort(ctx.bvh_keys(v, t, LO, HI)).values.contiguous()
    torch.cuda.synchronize()
    st.h.run("bvh_build", lambda v, t: ctx.bvh_build(v, t, keys), [v, t])
    ref = ctx.bvh_build(v, t, keys)
    torch.cuda.synchronize()
    tree = st.h.build_on_side("bvh_keys + sort + bvh_build", lambda: ctx.bvh_build(v, t, torch.sort(ctx.bvh_keys(v, t, LO, HI)).values.contiguous()), ref)
    st.tree = tree
    q = st.f32(N_POINTS, 3, lo=-1.1, hi=1.1)
    st.h.run("point_mesh_bvh_query", lambda q: ctx.point_mesh_bvh_query(q, v, t, *tree, return_visits=True), [q])
    st.h.run("raycast_bvh_query", lambda o, d: ctx.raycast_bvh_query(o, d, v, t, *tree, 0.0, inf, pad, return_visits=True), [o, d])
    st.h.run("raycast_bvh_occluded", lambda o, d: ctx.raycast_bvh_occluded(o, d, v, t, *tree, 0.0, inf, pad, return_visits=True), [o, d])
    _done(st, request)


def test_simplify_steps(st, request):
    """Every mesh_simplify_* step on late leaf data; the sorted keys, cluster ranges, sorted pairs and the triangle order come from a
    chain run under the side stream, sorts included, and compared with the default-stream chain first."""
    from neddf_amd._lib import SIMPLIFY_PLACEMENTS
    ctx, torch = st.ctx, st.torch
    v, t = _sphere_mesh(st)
    cells, V = (5, 4, 6), v.shape[0]

    def chain():
        keys = torch.sort(ctx.mesh_simplify_keys(v, LO, HI, cells)).values
        cluster, crange = ctx.mesh_simplify_clusters(keys)
        pairs = torch.sort(ctx.mesh_simplify_pairs(v, t, cluster)).values
        mapped, lowest, tkeys = ctx.mesh_simplify_triangles(t, V, cluster)
        order = torch.sort(tkeys, stable=True).indices
        order = order[torch.sort(lowest[order], stable=True).indices].contiguous()
        return keys, cluster, crange.contiguous(), pairs, mapped, lowest, tkeys, order
    ref = chain()
    torch.cuda.synchronize()
    keys, cluster, crange, pairs, mapped, lowest, tkeys, order = st.h.build_on_side("simplify chain", chain, ref)
    assert 1 < crange.shape[0] < V
    st.h.run("mesh_simplify_keys", lambda v: ctx.mesh_simplify_keys(v, LO, HI, cells), [v])
    st.h.run("mesh_simplify_clusters", lambda: ctx.mesh_simplify_clusters(keys), [], synchronising=True)
    st.h.run("mesh_simplify_pairs", lambda v, t: ctx.mesh_simplify_pairs(v, t, cluster), [v, t], synchronising=True)
    for name, pr in (("mean", None), ("quadric", pairs)):
        st.h.run("mesh_simplify_place[%s]" % name, lambda v: ctx.mesh_simplify_place(v, keys, crange, SIMPLIFY_PLACEMENTS[name], 2.0 ** -10, t, pr), [v])
    st.h.run("mesh_simplify_attributes", lambda a: ctx.mesh_simplify_attributes(a, keys, crange), [st.normal(V, 3)])
    st.h.run("mesh_simplify_triangles", lambda t: ctx.mesh_simplify_triangles(t, V, cluster), [t])
    st.h.run("mesh_simplify_unique", lambda lo, k: ctx.mesh_simplify_unique(lo, k, order), [lowest, tkeys])
    _done(st, request)


def test_occupancy(st, request):
    from neddf_amd.occupancy import OccupancyGrid
    ctx, torch = st.ctx, st.torch
    R = 16
    x = np.linspace(-1.1, 1.1, R + 1)
    Z, Y, X = np.meshgrid(x, x, x, indexing="ij")
    vol = st.T((1.0 - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)).astype(np.float32))          # "density": positive inside the unit sphere
    st.h.run("occupancy_build", lambda vol: ctx.occupancy_build(vol, 0.3, 1), [vol], synchronising=True)
    ref = ctx.occupancy_build(vol, 0.3, 1)
    torch.cuda.synchronize()
    bits, n = st.h.build_on_side("occupancy_build", lambda: ctx.occupancy_build(vol, 0.3, 1), ref)
    assert 0 < n < R ** 3
    occ = OccupancyGrid(bits, R, (-1.1,) * 3, (1.1,) * 3).descriptor()
    pts = st.f32(5000, 3, lo=-1.2, hi=1.2)
    st.h.run("occupancy_classify", lambda p: ctx.occupancy_classify(occ, p), [pts])
    keep = ctx.occupancy_classify(occ, pts)
    rows = [st.normal(5000, 3) for _ in range(3)]
    st.h.run("occupancy_gather", lambda k, a, b, c: ctx.occupancy_gather(k, a, b, c), [keep] + rows, synchronising=True)
    index = ctx.occupancy_gather(keep, *rows)[3].clone()
    torch.cuda.synchronize()
    M = index.shape[0]
    assert 256 < M < 5000
    st.h.run("occupancy_scatter", lambda d, c, n: ctx.occupancy_scatter(index, 5000, d, c, n), [st.f32(M), st.f32(M, 3), st.normal(M, 3)])
    _done(st, request)


def _trace_rays(st, n=1025):
    """n rays from radius 3 towards points near the origin; some miss the sphere of radius 0.5 that _sphere_distance describes."""
    if not hasattr(st, "trace_rays"):
        rng = np.random.default_rng(31)
        o = rng.standard_normal((n, 3))
        o *= 3.0 / np.linalg.norm(o, axis=1, keepdims=True)
        d = rng.uniform(-0.45, 0.45, (n, 3)) - o
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        st.trace_rays = (st.T(o.astype(np.float32)), st.T(d.astype(np.float32)))
    return st.trace_rays


def test_trace_steps(st, request):
    """The stage entry points of the sphere tracer at the states of a run against an analytic sphere.  The per-ray state is leaf data
    and arrives late; the index lists of compact / bisect_points are structures, built before."""
    ctx, torch = st.ctx, st.torch
    o, d = _trace_rays(st)
    thr, t_near, t_far, min_step = 0.01, 0.5, 6.0, 5.5 * 2.0 ** -10
    keys = ("t", "t_lo", "status", "steps", "distance")
    dist = lambda pos: pos.norm(dim=1) - 0.5
    st.h.run("trace_begin", lambda o, d: ctx.trace_begin(o, d, t_near), [o, d])
    s0 = ctx.trace_begin(o, d, t_near)
    st.h.run("trace_compact", lambda o, d, t, status: ctx.trace_compact(o, d, dict(s0, t=t, status=status)), [o, d, s0["t"], s0["status"]], synchronising=True)
    index, pos = (x.clone() for x in ctx.trace_compact(o, d, s0))
    torch.cuda.synchronize()
    assert index.shape[0] > 512

    def advance(D, *state):
        s = dict(zip(keys, state))
        ctx.trace_advance(index, D, s, thr, 1.0, min_step, t_far)
        return s
    st.h.run("trace_advance", advance, [dist(pos)] + [s0[k] for k in keys])
    s = s0
    for _ in range(24):
        idx, p = ctx.trace_compact(o, d, s)
        if idx.shape[0] == 0:
            break
        ctx.trace_advance(idx, dist(p), s, thr, 1.0, min_step, t_far)

    def finish(status):
        ctx.trace_finish(dict(status=status))
        return status
    st.h.run("trace_finish", finish, [s["status"]])
    ctx.trace_finish(s)
    st.h.run("trace_bisect_points", lambda o, d, t, t_lo, status: ctx.trace_bisect_points(o, d, dict(t=t, t_lo=t_lo, status=status)),
             [o, d, s["t"], s["t_lo"], s["status"]], synchronising=True)
    bidx, bpos = (x.clone() for x in ctx.trace_bisect_points(o, d, s))
    torch.cuda.synchronize()
    assert bidx.shape[0] > 0

    def update(D, t, t_lo, distance):
        u = dict(t=t, t_lo=t_lo, distance=distance)
        ctx.trace_bisect_update(bidx, D, u, thr)
        return u
    st.h.run("trace_bisect_update", update, [dist(bpos), s["t"], s["t_lo"], s["distance"]])
    _done(st, request)


# ---------------------------------------------------------------------------------------------------------------- Python layer
# Once each under the side stream, late inputs where the function takes tensors, bit-identical to the default-stream result.  No
# assertion on when they return: these functions legitimately read counts.
def test_python_render_image(st, request):
    torch = st.torch
    r = _renderer(st, use_coarse=True)
    r.rays_per_call = 256

    def fn():
        torch.manual_seed(5)
        return r.render_image(37, 29, st.camera, ["color", "depth", "transmittance"], chunk=128)
    st.h.run("render_image[37x29]", fn, [], check_async=False)
    _done(st, request)


@pytest.mark.parametrize("brick", [0, 8])
def test_python_extract_mesh(st, request, brick):
    net = _load(st, "neddf", "fp32")
    iso = float(st.ctx.field_grid(2, "distance", (24, 24, 24), (-1.1,) * 3, (1.1,) * 3).median())
    st.h.run("extract_mesh[brick=%d]" % brick, lambda: net.extract_mesh("distance", iso, 1.1, 24, brick=brick, normals="geometric"), [], check_async=False)
    _done(st, request)


def test_python_simplify(st, request):
    from neddf_amd.mesh import simplify_mesh
    _need(st, "test_simplify_steps", "test_mesh_ops")
    v, t = _sphere_mesh(st)
    st.h.run("simplify_mesh", lambda v, t: simplify_mesh(v, t, cells=(5, 4, 6), box=(LO, HI), placement="quadric"), [v, t], check_async=False)
    _done(st, request)


def test_python_mesh_distance(st, request):
    from neddf_amd.geometry import mesh_distance
    _need(st, "test_mesh_sampling", "test_nearest_neighbours")
    va, ta = _sphere_mesh(st)
    vb = va * 1.01
    st.h.run("mesh_distance", lambda va, ta, vb: mesh_distance((va, ta), (vb, ta), density=400.0, seed=3, return_samples=True), [va, ta, vb], check_async=False)
    _done(st, request)


def test_python_cast_rays_bvh(st, request):
    """bvh.cast_rays through a tree built under the side stream (build_bvh) and compared with the default-stream tree first."""
    from neddf_amd.bvh import build_bvh, cast_rays
    _need(st, "test_bvh")
    v, t, o, d = _soup(st)
    parts = lambda b: (b.leaf_triangle, b.children, b.boxes, list(b.lo), list(b.hi))
    ref = build_bvh(v, t)
    st.torch.cuda.synchronize()
    box = {}

    def build():
        box["bvh"] = build_bvh(v, t)
        return parts(box["bvh"])
    st.h.build_on_side("build_bvh", build, parts(ref))
    st.h.run("bvh.cast_rays", lambda o, d: cast_rays(o, d, v, t, bvh=box["bvh"]), [o, d], check_async=False)
    _done(st, request)


# ---------------------------------------------------------------------------------------------------------------- weights across streams
def _two_weight_sets(st):
    from neddf_amd._lib import OUT_MINIMAL
    if not hasattr(st, "wsets"):
        nets = [st.module("neddf_tanhexp", seed) for seed in (101, 202, 303)]
        refs = []
        for net in nets:
            net.upload(st.ctx, 3)
            refs.append({k: v.clone() for k, v in st.ctx.field_forward(3, *st.points, OUT_MINIMAL, WANT["neddf", "minimal"]).items()})
        st.torch.cuda.synchronize()
        st.wsets = nets, refs
    return st.wsets


def _eval3(st):
    from neddf_amd._lib import OUT_MINIMAL
    return {k: v.clone() for k, v in st.ctx.field_forward(3, *st.points, OUT_MINIMAL, WANT["neddf", "minimal"]).items()}


def _assert_same(st, got, ref, what):
    from stream_check import compare, flatten
    msg = compare(flatten(got), flatten(ref), what)
    assert msg is None, msg


def test_slot_reuse_waits_for_the_last_reader(st, request):
    """Stream A: delay plus an evaluation of W1.  Without waiting, the host loads W2 into the same slot and evaluates on stream B.  A's
    result is W1's and B's is W2's: neddf_set_field waited for A's use mark, nothing repacked under A's kernels."""
    torch, h = st.torch, st.h
    h.require_controls()
    (n1, n2, _), (r1, r2, _) = _two_weight_sets(st)
    n1.upload(st.ctx, 3)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(h.side):
        a.record()
        h.enqueue_delay(40.0)
        b.record()
        got1 = _eval3(st)
    n2.upload(st.ctx, 3)                # the host: waits for A's evaluation, then repacks
    with torch.cuda.stream(h.side2):
        got2 = _eval3(st)
    torch.cuda.synchronize()
    assert a.elapsed_time(b) >= 40.0, "inconclusive: delay too short"
    _assert_same(st, got1, r1, "stream A (the weights loaded first)")
    _assert_same(st, got2, r2, "stream B (the weights loaded second)")
    _done(st, request)


def test_two_readers_then_a_replacement(st, request):
    """Two streams read one slot back to back, the second ordered after the first by wait_stream; then the weights are replaced and
    read again: the chain of use marks that mark_use describes."""
    torch, h = st.torch, st.h
    h.require_controls()
    (n1, _, n3), (r1, _, r3) = _two_weight_sets(st)
    n1.upload(st.ctx, 3)
    torch.cuda.synchronize()
    with torch.cuda.stream(h.side):
        h.enqueue_delay(40.0)
        got_a = _eval3(st)
    h.side2.wait_stream(h.side)
    with torch.cuda.stream(h.side2):
        got_b = _eval3(st)
    n3.upload(st.ctx, 3)
    with torch.cuda.stream(h.side):
        got_c = _eval3(st)
    torch.cuda.synchronize()
    _assert_same(st, got_a, r1, "the first reader")
    _assert_same(st, got_b, r1, "the second reader")
    _assert_same(st, got_c, r3, "the reader after the replacement")
    _done(st, request)


def test_one_context_on_two_ordered_streams(st, request):
    """One context used from stream A and then from stream B, ordered by B.wait_stream(A) alone, no host synchronisation."""
    torch, h, ctx = st.torch, st.h, st.ctx
    h.require_controls()
    dens, col = st.f32(N_RAYS, N_SAMPLES, hi=3.0), st.f32(N_RAYS, N_SAMPLES, 3)
    (n1, _, _), (r1, _, _) = _two_weight_sets(st)
    n1.upload(ctx, 3)
    ref_c = ctx.composite(st.dists, dens, col, 6.0)
    torch.cuda.synchronize()
    late = [torch.zeros_like(t) for t in st.points]
    with torch.cuda.stream(h.side):
        h.enqueue_delay(40.0)
        for z, p in zip(late, st.points):
            z.copy_(p)
        from neddf_amd._lib import OUT_MINIMAL
        got_a = {k: v.clone() for k, v in ctx.field_forward(3, *late, OUT_MINIMAL, WANT["neddf", "minimal"]).items()}
    h.side2.wait_stream(h.side)
    with torch.cuda.stream(h.side2):
        got_b = {k: v.clone() for k, v in ctx.field_forward(3, *late, OUT_MINIMAL, WANT["neddf", "minimal"]).items()}
        got_c = ctx.composite(st.dists, dens, col, 6.0)
        got_c = ({k: v.clone() for k, v in got_c[0].items()}, got_c[1].clone())
    torch.cuda.synchronize()
    _assert_same(st, got_a, r1, "stream A")
    _assert_same(st, got_b, r1, "stream B after wait_stream(A)")
    _assert_same(st, got_c, ref_c, "composite on stream B")
    _done(st, request)


def test_two_contexts_on_two_unordered_streams(st, request):
    """A 64 x 64 view in four 1024-ray slabs that alternate between two contexts on two streams with no ordering between them
    (tools/two_stream_probe.py): the pixels are those of the one-stream render."""
    from neddf_amd._lib import Context
    from neddf_amd.render import SLOT_FINE
    from stream_check import Recorder
    torch, h = st.torch, st.h
    h.require_controls()
    r = _renderer(st)
    ctxs = [r._ctx(st.dev), Context(0)]
    ctxs[1].lib = Recorder(st.real_lib, st.calls)
    r.network_fine.upload(ctxs[1], SLOT_FINE)
    n = 64 * 64
    idx = torch.arange(n, device=st.dev)
    uv = torch.stack([idx % 64 * 6, idx // 64 * 6], 1).contiguous()
    U = st.f32(n, 17)
    params = r._params()
    streams = [h.side, h.side2]

    def view(two):
        out = dict(color=torch.empty(n, 3, device=st.dev), depth=torch.empty(n, device=st.dev), transmittance=torch.empty(n, device=st.dev))
        flag = torch.zeros(1, device=st.dev, dtype=torch.int32)
        torch.cuda.synchronize()
        for i, lo in enumerate(range(0, n, 1024)):
            k = i & 1 if two else 0
            with torch.cuda.stream(streams[k] if two else torch.cuda.current_stream()):
                ctxs[k].render_rays(uv[lo:lo + 1024], st.cam, params, U[lo:lo + 1024], None,
                                    dict({key: v[lo:lo + 1024] for key, v in out.items()}, nan_flag=flag), single_slot=SLOT_FINE)
        torch.cuda.synchronize()
        return out, flag
    ref = view(False)
    view(True)                          # sizes the second context's workspaces
    got = view(True)
    _assert_same(st, got, ref, "two contexts on two streams")
    ctxs[1].lib = st.real_lib
    _done(st, request)


# ---------------------------------------------------------------------------------------------------------------- completeness
def test_every_table_row_was_called(st):
    """The union of what the cases called through ctx.lib is the table's key set, each export from the test the table names; no case was
    inconclusive (an inconclusive case fails where it runs)."""
    stream_calls = {t: {c for c in calls if c in TABLE} for t, calls in st.by_test.items()}
    missing = sorted(k for k, (test, _) in TABLE.items() if k not in stream_calls.get(test, set()))
    assert not missing, "not called by the test the table names: %s" % missing
    from test_streams_host import HEADER, stream_exports
    called = set().union(*st.by_test.values()) & stream_exports(open(HEADER).read())[0]
    assert called == set(TABLE), "stream-taking exports called without a row: %s" % sorted(called - set(TABLE))
    print("\n%-46s %10s %12s %10s %12s" % ("case", "call ms", "call+sync ms", "delay ms", "realised ms"))
    for r in st.h.records:
        print("%-46s %10.3f %12.3f %10.1f %12.1f" % (r["name"], r["call_ms"], r["call_sync_ms"], r["delay_ms"], r["realised_ms"]))
