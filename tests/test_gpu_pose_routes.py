"""Input gradients on every backward route of the training ABI and at the tile edges of the three pose kernels
(neddf_amd/csrc/pose_kernels.hip) against fp64.

Field routes: tests/golden/pose_grad_routes.npz (gen_pose_goldens.py `routes`) holds the fp64 reference's pos.grad / dir.grad of the
networks whose parameter gradients test_gpu_train.py already gates -- hidden widths 128 / 192 (zero-padded to 256), 256, 384 (padded to
512) and 512, one skip (fused, point-major dZ) and two skips (per layer, kept row-major copies), NeRF at 128 / 384 / 512 -- plus the
encoding ranks at the limits of the kernel's accumulator tiles (60 of 64 S-columns, 120 of 128 U-columns) and at 1.  The inputs are
rebuilt from seeds (synth.pose_route_inputs, pinned by a digest).  Points the generator marked as kinks (the fp32 REFERENCE deviates
from fp64 there by more than a third of the base gate: a ReLU flipped) are left out on both sides.

Samplers and ray generation: fp64 restatements written here (`sampler_restatement`, `raygen_backward_restatement`; test_pose_host.py ties
them to the reference's recorded gradients on the CPU) at the sample counts around the wavefront, ray counts around the workgroup and
every pixel dtype.

Gates: test_gpu_pose.check -- 1e-4 on the norm and on the largest entry, or 3 x the fp32 reference's own deviation where larger.  Every
comparison prints observed / gate.
"""
import itertools
import json

import numpy as np
import pytest
import torch
from conftest import golden
from test_gpu_pose import N, T, check, field_module

pytestmark = pytest.mark.gpu

CASES = ["bunny", "neddf128", "neddf192", "neddf384", "neddf512", "nerf128", "nerf384", "nerf512", "ranks_hi", "nerf_ranks_hi", "ranks_lo"]
MANY = ["bunny_many", "neddf512_many"]
PREFIXES = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65)      # around the 32-point workgroup of enc_input_grad_kernel and the 16-point tiles of the chains
RADIUS = 1.0 / 1111 / np.sqrt(12)


# ------------------------------------------------------------------ fp64 restatements (dtype follows the inputs; importable without a GPU)
def sampler_restatement(ray_orig, ray_dir, dists, radius):
    """Ray.get_sampling_cones / get_sampling_points as device_math.h sample_moments states them: (pos, dir, var), each [B, S, 3].
    radius None: point samples (t_mu = the distance, zero variance)."""
    B, S = dists.shape
    d, o = ray_dir[:, None, :].expand(B, S, 3), ray_orig[:, None, :].expand(B, S, 3)
    if radius is None:
        return o + d * dists[:, :, None], d, torch.zeros_like(o)
    far = torch.cat([dists[:, 1:], 2 * dists[:, -1:] - dists[:, -2:-1]], 1)
    mu, sg = 0.5 * (dists + far), 0.5 * (far - dists)
    mu2, s2 = mu * mu, sg * sg
    s4 = s2 * s2
    minv = 1.0 / (3 * mu2 + s2 + 1e-7)
    t_mu = mu + (2 * mu * s2) * minv
    t_var = (1.0 / 3) * s2 - (4.0 / 15) * s4 * (12 * mu2 - s2) * (minv * minv)
    r_var = radius * radius * (0.25 * mu2 + (5.0 / 12) * s2 - (4.0 / 15) * s4 * minv)
    dsq = d * d
    return o + d * t_mu[:, :, None], d, t_var[:, :, None] * dsq + r_var[:, :, None] * (1.0 - dsq)


def sampler_backward_restatement(ray_orig, ray_dir, dists, radius, g_pos, g_dir, g_var, dtype=torch.float64):
    """(g_ray_dir, g_ray_orig) by autograd through sampler_restatement in `dtype` on the CPU; absent upstream gradients are None."""
    c = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    o, d = c(ray_orig).requires_grad_(True), c(ray_dir).requires_grad_(True)
    with torch.enable_grad():
        outs = sampler_restatement(o, d, c(dists), radius)
        obj = o.sum() * 0 + d.sum() * 0
        for out, g in zip(outs, (g_pos, g_dir, g_var)):
            if g is not None:
                obj = obj + (out * c(g)).sum()
        obj.backward()
    return d.grad.numpy(), o.grad.numpy()


def raygen_backward_restatement(uv, calib, g_rd, g_ro):
    """(g_R [3, 3], g_T [3]) of Camera.create_rays in fp64: c = normalize(((u + 0.5 - cx) / fx, -(v + 0.5 - cy) / fy, -1)),
    g_R = g_rd^T c, g_T = sum g_ro."""
    uv, g_rd, g_ro = (np.asarray(a, np.float64) for a in (uv, g_rd, g_ro))
    fx, fy, cx, cy = (float(x) for x in calib)
    c = np.stack([(uv[:, 0] + 0.5 - cx) / fx, -(uv[:, 1] + 0.5 - cy) / fy, -np.ones(len(uv))], 1)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    return g_rd.T @ c, g_ro.sum(0)


def deviation(a, ref):
    """(norm, entry) deviation of `a` from `ref` relative to ref's norm / largest entry (zero where ref is zero throughout)."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    if not ref.any():
        return 0.0, 0.0
    return abs(np.linalg.norm(a) - np.linalg.norm(ref)) / np.linalg.norm(ref), np.abs(a - ref).max() / np.abs(ref).max()


def check_or_zero(what, got, want, ref_norm=0.0, ref_entry=0.0):
    """`check`; a reference that is zero throughout (no upstream gradient reaches it) must be met exactly."""
    if not np.asarray(want).any():
        assert not np.asarray(got).any(), what
        print("%s: exactly zero on both sides" % what)
        return 0.0
    return check(what, got, want, ref_norm, ref_entry)


# ------------------------------------------------------------------ field routes
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g():
    d = golden("pose_grad_routes.npz")
    return {k: d[k] for k in d.files}


_inputs = {}


def route_inputs(case):
    """The case's flattened inputs, built once: pos, dir, var [n, 3] and the upstream gradients [n] / [n, 3] by key."""
    import synth
    if case not in _inputs:
        pos, d, var, ups = synth.pose_route_inputs(case)
        _inputs[case] = (pos.reshape(-1, 3), d.reshape(-1, 3), var.reshape(-1, 3), {k: v.reshape((-1,) + v.shape[2:]) for k, v in ups.items()})
    return _inputs[case]


def route_module(dev, g, case, bunny_weights):
    import neddf_amd
    import synth
    if case.startswith("bunny"):
        net = field_module(dev, "bunny", bunny_weights)
    else:
        kind, kw = str(g[case + "_kind"]), json.loads(str(g[case + "_config"]))
        net = (neddf_amd.NeRF if kind == "nerf" else neddf_amd.NeDDF)(**kw)
        net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.arch_state(kind, kw, int(g[case + "_state_seed"])).items()})
        net.to(dev)
    net.set_iter(int(g[case + "_iteration"]))
    return net


def route_backward(net, dev, case, n=None, zero_upstream=False):
    """Forward + backward of the first n points of the case, fed as [n, 1, 3]; returns the outputs and the three leaves."""
    from neddf_amd import Sampling
    pos, d, var, ups = route_inputs(case)
    n = len(pos) if n is None else n
    net.zero_grad()
    leaves = [T(a[:n].reshape(n, 1, 3), dev).requires_grad_(True) for a in (pos, d, var)]
    o = net(Sampling(*leaves))
    sum((o[k] * T(v[:n].reshape((n, 1) + v.shape[1:]) * (0.0 if zero_upstream else 1.0), dev)).sum() for k, v in ups.items()).backward()
    return o, leaves


def check_route(g, case, o, leaves, n, what):
    """Outputs at 1e-4 / 2e-5 against the fp32 reference's; pos.grad / dir.grad of the unmarked points against fp64; var.grad zero."""
    ups = route_inputs(case)[3]
    stride = int(g[case + "_out_stride"])
    for k in ups:
        want = g[case + "_out_" + k][:(n + stride - 1) // stride]
        np.testing.assert_allclose(N(o[k]).reshape((n,) + want.shape[1:])[::stride], want, rtol=1e-4, atol=2e-5, err_msg="%s %s" % (what, k))
    keep = ~np.unpackbits(g[case + "_kink"])[:n].astype(bool)
    worst = 0.0
    for leaf, name in zip(leaves[:2], ("pos", "dir")):
        assert leaf.grad is not None and tuple(leaf.grad.shape) == (n, 1, 3)
        worst = max(worst, check("%s d/d%s" % (what, name), N(leaf.grad).reshape(n, 3)[keep], g[case + "_grad64_" + name][:n][keep],
                                 g[case + "_ref32_norm_" + name], g[case + "_ref32_entry_" + name]))
    assert leaves[2].grad is not None and not N(leaves[2].grad).any()     # the reference's cone weights are constants of its autograd
    print("%s: worst observed / gate %.3f" % (what, worst))
    return worst


@pytest.mark.parametrize("case", CASES)
def test_field_routes(dev, g, bunny_weights, case):
    """The 98 points of every case: 4 workgroups of enc_input_grad_kernel, the last one ragged."""
    net = route_module(dev, g, case, bunny_weights)
    o, leaves = route_backward(net, dev, case)
    check_route(g, case, o, leaves, 98, case)


@pytest.mark.parametrize("case", ["bunny", "neddf384", "nerf512"])
def test_field_route_prefixes(dev, g, bunny_weights, case):
    """Point counts around the kernels' tiles.  The gradient of a point does not depend on the other points of the call: the prefix
    of the recorded gradient is the reference."""
    net = route_module(dev, g, case, bunny_weights)
    worst = 0.0
    for n in PREFIXES:
        o, leaves = route_backward(net, dev, case, n)
        worst = max(worst, check_route(g, case, o, leaves, n, "%s n=%d" % (case, n)))
    print("%s prefixes: worst observed / gate %.3f" % (case, worst))


@pytest.mark.parametrize("case", MANY)
def test_field_routes_many_workgroups(dev, g, bunny_weights, case):
    """8231 points: 258 workgroups of enc_input_grad_kernel (more than the device has CUs), the last one with 7 points."""
    net = route_module(dev, g, case, bunny_weights)
    o, leaves = route_backward(net, dev, case)
    check_route(g, case, o, leaves, 8231, case)


@pytest.mark.parametrize("case", ["bunny", "neddf384", "nerf512"])
def test_zero_upstream_gives_zero_input_gradients(dev, g, bunny_weights, case):
    net = route_module(dev, g, case, bunny_weights)
    _, leaves = route_backward(net, dev, case, 33, zero_upstream=True)
    for leaf in leaves:
        assert leaf.grad is not None and np.isfinite(N(leaf.grad)).all() and not N(leaf.grad).any()


@pytest.mark.parametrize("case", ["bunny", "neddf512"])
def test_input_gradients_are_bitwise_repeatable(dev, g, bunny_weights, case):
    """pose_kernels.hip: every reduction in a fixed order, no floating-point atomics -- and nothing upstream of dZ may break that."""
    net = route_module(dev, g, case, bunny_weights)
    _, a = route_backward(net, dev, case)
    _, b = route_backward(net, dev, case)
    assert torch.equal(a[0].grad, b[0].grad) and torch.equal(a[1].grad, b[1].grad)


def test_per_layer_routes_in_subprocess():
    """NEDDF_TRAIN_UNFUSED=1 and NEDDF_TRAIN_WIDE_FUSED=0 are read once per process: a fresh child runs the 256-wide and the
    512-wide one-skip networks through the per-layer routes (row-major kept copies of dZ) at the same gates."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    p = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", "tests/test_gpu_pose_routes.py::test_field_routes[bunny]",
                        "tests/test_gpu_pose_routes.py::test_field_routes[neddf384]"],
                       env=dict(os.environ, NEDDF_TRAIN_UNFUSED="1", NEDDF_TRAIN_WIDE_FUSED="0"), cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    print("\n".join(l for l in p.stdout.splitlines() if "ratio" in l or "worst" in l))
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert "2 passed" in p.stdout, p.stdout[-500:]


# ------------------------------------------------------------------ sampling_backward
def sampling_inputs(B, S, seed):
    """Unit ray directions, stratified jittered distances in [2, 6]; the last ray repeats one distance (a zero-width interval).  Upstream
    gradients on pos / dir / var.  Origins in [-0.25, 0.25]: neither gradient depends on the origin, and the forward comparison is a
    RELATIVE one (1e-6) that fp32 can meet only where o + d t does not cancel -- with |o| <= 0.25 a coordinate either keeps the magnitude
    of d t (relative error of two roundings, 1.2e-7) or is below 0.5 in both terms (absolute error below 6e-8, inside the 1e-7)."""
    rng = np.random.default_rng(seed)
    rd = rng.standard_normal((B, 3))
    rd = (rd / np.linalg.norm(rd, axis=1, keepdims=True)).astype(np.float32)
    ro = rng.uniform(-0.25, 0.25, (B, 3)).astype(np.float32)
    edges = np.linspace(2.0, 6.0, S + 1)
    dists = (edges[:-1] + rng.uniform(0, 1, (B, S)) * (edges[1:] - edges[:-1])).astype(np.float32)
    if S >= 2:
        dists[-1, S // 2] = dists[-1, S // 2 - 1]
    ups = [rng.standard_normal((B, S, 3)).astype(np.float32) for _ in range(3)]
    return rd, ro, dists, ups


def check_sampling_backward(ctx, dev, B, S, cone, present=(True, True, True), seed=0):
    rd, ro, dists, ups = sampling_inputs(B, S, 500 + 1000 * seed + 10 * S + B)
    radius = RADIUS if cone else None
    what = "%s B=%d S=%d%s" % ("cone" if cone else "point", B, S, "" if all(present) else " upstream %s" % (present,))
    # the restatement's forward is the kernel's (which is bit-exact against the oracle in test_gpu_parity.py)
    want = sampler_restatement(*(torch.from_numpy(a).double() for a in (ro, rd, dists)), radius)
    got = ctx.sampling(T(rd, dev), T(ro, dev), T(dists, dev), radius)
    for a, b, k in zip(got, want, ("pos", "dir", "var")):
        np.testing.assert_allclose(N(a), b.numpy(), rtol=1e-6, atol=1e-7, err_msg="%s forward %s" % (what, k))
    gs = [u if p else None for u, p in zip(ups, present)]
    w_rd, w_ro = sampler_backward_restatement(ro, rd, dists, radius, *gs)
    f_rd, f_ro = sampler_backward_restatement(ro, rd, dists, radius, *gs, dtype=torch.float32)
    g_rd, g_ro = ctx.sampling_backward(*(None if u is None else T(u, dev) for u in gs), T(rd, dev), T(dists, dev), radius)
    assert tuple(g_rd.shape) == (B, 3) and tuple(g_ro.shape) == (B, 3)
    return max(check_or_zero(what + " d/dray_dir", N(g_rd), w_rd, *deviation(f_rd, w_rd)),
               check_or_zero(what + " d/dray_orig", N(g_ro), w_ro, *deviation(f_ro, w_ro)))


@pytest.mark.parametrize("cone", [True, False], ids=["cone", "point"])
@pytest.mark.parametrize("B", [1, 3, 4, 5, 9])
def test_sampling_backward_shapes(dev, B, cone):
    """One wave per ray, four rays per workgroup: ray counts that do not fill a workgroup, sample counts around one, two and four
    passes of the wave's loop.  (One sample: point samples only -- the cone sampler refuses it, forward and backward.)"""
    from neddf_amd import Context
    ctx = Context.get(dev)
    worst = 0.0
    for S in ([] if cone else [1]) + [2, 63, 64, 65, 129, 259]:
        worst = max(worst, check_sampling_backward(ctx, dev, B, S, cone))
    print("sampling_backward %s B=%d: worst observed / gate %.3f" % ("cone" if cone else "point", B, worst))


def test_sampling_backward_absent_upstream_gradients(dev):
    """Every non-empty subset of (g_pos, g_dir, g_var), None for the absent ones."""
    from neddf_amd import Context
    ctx = Context.get(dev)
    for present in itertools.product([True, False], repeat=3):
        if any(present):
            check_sampling_backward(ctx, dev, 5, 65, True, present, seed=1)


def test_sampling_backward_no_rays(dev):
    from neddf_amd import Context
    ctx = Context.get(dev)
    z = lambda *s: torch.zeros(*s, device=dev)
    for radius in (RADIUS, None):
        g_rd, g_ro = ctx.sampling_backward(z(0, 7, 3), z(0, 7, 3), z(0, 7, 3), z(0, 3), z(0, 7), radius)
        assert tuple(g_rd.shape) == (0, 3) and tuple(g_ro.shape) == (0, 3)


# ------------------------------------------------------------------ raygen_backward
CALIB = np.array([555.5, 553.1, 200.3, 199.2])


def raygen_camera(dev):
    import neddf_amd
    from scipy.spatial.transform import Rotation
    cam = neddf_amd.Camera(neddf_amd.PinholeCalib(CALIB.copy()), None).to(dev)
    cam.R = T(Rotation.from_rotvec([0.3, -0.7, 0.2]).as_matrix().astype(np.float32), dev)
    cam.T = T(np.array([0.4, -1.1, 3.2], np.float32), dev)
    return cam


@pytest.mark.parametrize("dtype", [np.int64, np.int32, np.int16, np.float32], ids=["int64", "int32", "int16", "float32"])
def test_raygen_backward_shapes_and_pixel_types(dev, dtype):
    """One workgroup of 256 threads, an LDS tree over their partial sums: ray counts below, at and above 256; every pixel dtype of the
    ABI (the float pixels with fractional coordinates).  Each call twice: bitwise repeatable."""
    from neddf_amd import Context
    ctx = Context.get(dev)
    cam = raygen_camera(dev)
    worst = 0.0
    for n in (1, 2, 255, 256, 257, 1000):
        rng = np.random.default_rng(700 + n)
        uv = rng.integers(0, 400, (n, 2)).astype(dtype)
        if dtype is np.float32:
            uv = (uv + rng.uniform(0, 1, (n, 2))).astype(np.float32)
        g_rd, g_ro = rng.standard_normal((n, 3)).astype(np.float32), rng.standard_normal((n, 3)).astype(np.float32)
        wR, wT = raygen_backward_restatement(uv, CALIB, g_rd, g_ro)
        gR, gT = ctx.raygen_backward(T(uv, dev), cam.descriptor(), T(g_rd, dev), T(g_ro, dev))
        worst = max(worst, check("%s n=%d d/dR" % (np.dtype(dtype).name, n), N(gR), wR), check("%s n=%d d/dT" % (np.dtype(dtype).name, n), N(gT), wT))
        gR2, gT2 = ctx.raygen_backward(T(uv, dev), cam.descriptor(), T(g_rd, dev), T(g_ro, dev))
        assert torch.equal(gR, gR2) and torch.equal(gT, gT2)
    print("raygen_backward %s: worst observed / gate %.3f" % (np.dtype(dtype).name, worst))


def test_raygen_backward_no_rays(dev):
    from neddf_amd import Context
    ctx = Context.get(dev)
    cam = raygen_camera(dev)
    for dt in (torch.int64, torch.float32):
        gR, gT = ctx.raygen_backward(torch.zeros(0, 2, device=dev, dtype=dt), cam.descriptor(), torch.zeros(0, 3, device=dev), torch.zeros(0, 3, device=dev))
        assert tuple(gR.shape) == (3, 3) and tuple(gT.shape) == (3,) and not N(gR).any() and not N(gT).any()
