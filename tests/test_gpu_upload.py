"""A field renders with the weights it holds.  The fused inference kernels read the packed copy that BaseNeuralField.upload pushes into a
library slot, never the parameters; upload skips the push when its signature matches the slot's owner (tests/test_upload_host.py pins that
decision on the CPU).  Here the RESULT is held to it on the device: after every way of changing a module, its outputs must be those of a
NEW module built from the changed state_dict and evaluated on a context nothing else has touched -- bit for bit, the kernels are
deterministic -- and within the suite's gates (1e-4 relative + 1e-5 absolute) of the CPU oracle built from the same state.

Every change is large: the oracle before and the oracle after differ by more than 100 x the gate on at least half of the elements of every
gated output (`moved`, computed from the oracle alone), so a stale result cannot pass by being close."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch
from conftest import assert_close

import synth

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5         # the gates of test_neddf_synth / test_nerf_synth / test_neus_synth
KEYS = {("neddf", "full"): ("distance", "density", "color", "fields_penalty", "aux_grad"), ("neddf", "minimal"): ("distance", "density", "color", "aux_grad"),
        ("nerf", None): ("density", "color"), ("neus", None): ("sdf", "density", "color")}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def pts():
    """2 x 33 cone samples: one 64-row tile and a tail of two"""
    return synth.random_sampling(2, 33, seed=21)


def sampling(pts, dev):
    from neddf_amd import Sampling
    return Sampling(*(torch.from_numpy(a).to(dev) for a in pts))


# ------------------------------------------------------------------------------------------------ networks
def arch(kind, width=128, col_width=None, **over):
    """embed ranks 4 / 2, four trunk layers, three colour layers, one skip"""
    wc = width if col_width is None else col_width
    if kind == "neddf":
        kw = dict(embed_pos_rank=4, embed_dir_rank=2, ddf_layer_count=4, ddf_layer_width=width, col_layer_count=3, col_layer_width=wc, d_near=0.01,
                  activation_type="tanhExp", density_activation_type="ReLU", skips=[1], lowpass_alpha_offset=0.0)
    elif kind == "nerf":
        kw = dict(embed_pos_rank=4, embed_dir_rank=2, layer_count=4, layer_width=width, activation_type="ReLU", density_activation_type="tanhExp",
                  skips=[1], lowpass_alpha_offset=0.0)
    else:
        kw = dict(embed_pos_rank=4, embed_dir_rank=2, sdf_layer_count=4, sdf_layer_width=width, col_layer_count=3, col_layer_width=wc,
                  activation_type="tanhExp", init_variance=0.3, skips=[1])
    kw.update(over)
    return kw


def synth_state(kind, kw, seed):
    if kind == "neddf":
        return synth.neddf_state(kw["embed_pos_rank"], kw["embed_dir_rank"], kw["ddf_layer_count"], kw["ddf_layer_width"], kw["col_layer_count"],
                                 kw["col_layer_width"], tuple(kw["skips"]), seed=seed)
    if kind == "nerf":
        return synth.nerf_state(kw["embed_pos_rank"], kw["embed_dir_rank"], kw["layer_count"], kw["layer_width"], tuple(kw["skips"]), seed=seed)
    return synth.neus_state(kw["embed_pos_rank"], kw["embed_dir_rank"], kw["sdf_layer_count"], kw["sdf_layer_width"], kw["col_layer_count"],
                            kw["col_layer_width"], tuple(kw["skips"]), kw["init_variance"], seed=seed)


def build(kind, kw, sd, dev, dtype="fp32", mode=None, it=-1):
    import neddf_amd
    net = {"neddf": neddf_amd.NeDDF, "nerf": neddf_amd.NeRF, "neus": neddf_amd.NeuS}[kind](**kw)
    net.load_state_dict({k: torch.from_numpy(np.array(v, np.float32)) for k, v in sd.items()})
    net.to(dev)
    net.set_iter(it)
    net.weight_dtype = dtype
    if mode is not None:
        net.output_mode = mode
    return net


def state_of(net):
    return {k: v.detach().cpu().numpy().copy() for k, v in net.state_dict().items()}


def oracle_of(orc, kind, kw, sd, pts, it=-1, mode=None):
    o = {"neddf": orc.NeDDFOracle, "nerf": orc.NeRFOracle, "neus": orc.NeuSOracle}[kind](sd, **kw)
    o.set_iter(it)
    ref = o.forward(*pts)
    return {k: ref[k] for k in KEYS[kind, mode]}


def moved(before, after, what):
    """The non-vacuity condition: more than 100 x the gate apart on at least half of the elements of every gated output."""
    for k in after:
        a, b = after[k].astype(np.float64), before[k].astype(np.float64)
        frac = float(np.mean(np.abs(a - b) > 100.0 * (ATOL + RTOL * np.abs(a))))
        assert frac >= 0.5, "%s: only %.0f%% of `%s` moved by more than 100 x the gate -- this change would not expose a stale result" % (what, 100 * frac, k)


@contextlib.contextmanager
def fresh_context(dev):
    """A Context(index) of its own in the place of Context.get(dev)'s for the duration: no slot, blob or workspace is shared with the context the
    module under test lives on -- and none with an earlier fresh evaluation either, each gets a new one."""
    from neddf_amd._lib import Context
    shared = Context.get(dev)
    ctx = Context(dev.index)
    Context._instances[dev.index] = ctx
    try:
        yield ctx
    finally:
        Context._instances[dev.index] = shared
        torch.cuda.synchronize(dev)
        ctx.lib.neddf_destroy(ctx.h)
        ctx.h = None


def run(net, s):
    with torch.no_grad():
        return {k: v.clone() for k, v in net(s).items()}


def fresh_eval(kind, kw, sd, dev, s, dtype="fp32", mode=None, it=-1):
    with fresh_context(dev):
        return run(build(kind, kw, sd, dev, dtype, mode, it), s)


def same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert torch.equal(got[k], want[k]), "%s: `%s` differs from the fresh evaluation in %d of %d elements (max %.3e)" % (
            what, k, int((got[k] != want[k]).sum()), got[k].numel(), float((got[k] - want[k]).abs().max()))


def gated(got, ref, what):
    for k in ref:
        assert_close(got[k].cpu().numpy(), ref[k], RTOL, ATOL, "%s `%s` vs oracle" % (what, k))


class Tracked:
    """One module under test with everything its checks need; check() is the yardstick every test shares."""

    def __init__(self, kind, kw, sd, dev, orc, pts, dtype="fp32", mode=None, it=-1):
        self.kind, self.kw, self.dev, self.orc, self.pts, self.dtype, self.mode, self.it = kind, kw, dev, orc, pts, dtype, mode, it
        self.s = sampling(pts, dev)
        self.net = build(kind, kw, sd, dev, dtype, mode, it)
        self.ref = oracle_of(orc, kind, kw, sd, pts, it, mode)

    def check(self, what, must_move=True):
        sd = state_of(self.net)
        ref = oracle_of(self.orc, self.kind, self.kw, sd, self.pts, self.it, self.mode)
        if must_move:
            moved(self.ref, ref, what)
        got = run(self.net, self.s)
        same(got, fresh_eval(self.kind, self.kw, sd, self.dev, self.s, self.dtype, self.mode, self.it), what)
        if self.dtype == "fp32":
            gated(got, ref, what)
        self.ref = ref
        return got


# ------------------------------------------------------------------------------------------------ the ways to change a module
def hidden(net, i):
    """(weight, bias) of trunk layer i"""
    trunk = getattr(net, "layers_ddf", None) or getattr(net, "layers_sdf", None) or net.layers
    return trunk[i].weight, trunk[i].bias


def r_in_place(net):
    w, b = hidden(net, 1)
    with torch.no_grad():
        w.mul_(0.5)
        b.add_(0.25)
        if hasattr(net, "variance"):
            net.variance.mul_(1.5)


def r_copy(net):
    w, b = hidden(net, 2)
    with torch.no_grad():
        w.copy_(w * 0.5)
        b.copy_(b - 0.25)
        if hasattr(net, "variance"):
            net.variance.copy_(net.variance * 0.6)


def r_load_state_dict(net):
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    name = [k for k in sd if k.endswith("0.weight") and not k.startswith(("layers_col", "outL"))][0]
    sd[name] = sd[name] * 1.8
    sd[name.replace("weight", "bias")] = sd[name.replace("weight", "bias")] + 0.4
    if "variance" in sd:
        sd["variance"] = sd["variance"] * 1.5
    net.load_state_dict(sd)


def signed_sum(outputs, seed=0):
    """sum of every element of every output times a seeded +-1: a loss whose gradients have no common direction, so that an Adam step
    shakes the network instead of driving every output the same way (into a regime where the next change could not show)"""
    g = torch.Generator().manual_seed(seed)
    total = 0.0
    for k in sorted(outputs):
        sign = torch.randint(0, 2, tuple(outputs[k].shape), generator=g).to(torch.float32) * 2.0 - 1.0
        total = total + (outputs[k] * sign.to(outputs[k].device)).sum()
    return total


def r_adam(net, s, lr=0.03, loss=signed_sum):
    """one Adam step after a real backward through the training kernels: every parameter with a gradient moves by about lr"""
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    with torch.enable_grad():
        o = net(s)
        assert all(v.requires_grad for v in o.values())
        loss(o).backward()
    opt.step()
    net.zero_grad(set_to_none=True)


def r_data_assign(net, kind, kw):
    """every parameter gets a new tensor through .data: another synthetic state altogether, so that this change -- and the one after it
    -- shows whatever the optimiser step before has made of the network"""
    sd = synth_state(kind, kw, 100 + SEEDS[kind])
    for name, p in net.named_parameters():
        p.data = torch.from_numpy(np.array(sd[name], np.float32)).to(p.device)


def r_data_mul_invalidate(net):
    w, b = hidden(net, 2)
    w.data.mul_(1.7)
    b.data.add_(0.2)
    if hasattr(net, "variance"):
        net.variance.data.mul_(1.4)
    net.invalidate()


ROUTES = [("no_grad in-place", r_in_place), ("copy_", r_copy), ("load_state_dict", r_load_state_dict), ("Adam step", None),
          ("p.data = tensor", r_data_assign), ("p.data.mul_() + invalidate()", r_data_mul_invalidate)]
SEEDS = {"neddf": 7, "nerf": 11, "neus": 13}


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind,mode", [("neddf", "full"), ("neddf", "minimal"), ("nerf", None), ("neus", None)])
def test_mutation_sweep(dev, orc, pts, kind, mode, dtype):
    """Every route by which parameters change, in sequence on ONE module, each followed by the yardstick."""
    kw = arch(kind)
    t = Tracked(kind, kw, synth_state(kind, kw, SEEDS[kind]), dev, orc, pts, dtype, mode)
    t.check("%s first evaluation" % kind, must_move=False)
    for name, route in ROUTES:
        if route is None:
            r_adam(t.net, t.s)
        elif route is r_data_assign:
            route(t.net, kind, kw)
        else:
            route(t.net)
        t.check("%s %s %s after %s" % (kind, mode or "", dtype, name))


# ------------------------------------------------------------------------------------------------ refused uploads
def refused_modules(dev):
    """One module per architecture that the packer refuses only after neddf_set_field has begun, and the control the library turns away
    at the door (a 640-wide network)."""
    import neddf_amd
    base = dict(embed_pos_rank=4, embed_dir_rank=2, activation_type="ReLU", density_activation_type="ReLU")
    yield "NeDDF 640 wide (the control)", neddf_amd.NeDDF(ddf_layer_count=4, ddf_layer_width=640, col_layer_count=3, col_layer_width=640, skips=[1], **base)
    yield "NeDDF col_layer_width != ddf_layer_width", neddf_amd.NeDDF(ddf_layer_count=4, ddf_layer_width=128, col_layer_count=3, col_layer_width=256, skips=[1], **base)
    yield "NeDDF skip index out of range", neddf_amd.NeDDF(ddf_layer_count=4, ddf_layer_width=128, col_layer_count=3, col_layer_width=128, skips=[5], **base)
    yield "NeDDF five skip connections", neddf_amd.NeDDF(ddf_layer_count=7, ddf_layer_width=128, col_layer_count=3, col_layer_width=128,
                                                        skips=[0, 1, 2, 3, 4], **base)
    yield "NeDDF 13 trunk layers", neddf_amd.NeDDF(ddf_layer_count=14, ddf_layer_width=128, col_layer_count=3, col_layer_width=128, skips=[1], **base)
    yield "NeuS with LeakyReLU", neddf_amd.NeuS(embed_pos_rank=4, embed_dir_rank=2, sdf_layer_count=4, sdf_layer_width=128, col_layer_count=3,
                                               col_layer_width=128, activation_type="LeakyReLU", skips=[1])


def test_refused_upload_leaves_the_previous_owner_working(dev, orc, pts):
    """A renders in the generic slot; an architecture the library refuses tries the same slot and raises; A's next call succeeds with its
    first result.  Before that call the LIBRARY is asked directly: the slot still holds A's field (include/neddf_hip.h, neddf_set_field)."""
    from neddf_amd import NeddfError
    from neddf_amd._lib import OUT_FULL, Context
    kw = arch("neddf")
    t = Tracked("neddf", kw, synth_state("neddf", kw, 7), dev, orc, pts, mode="full")
    first = t.check("A", must_move=False)
    ctx, slot = Context.get(dev), t.net._slot
    pos, d, var = t.s.sample_pos, t.s.sample_dir, t.s.diag_variance
    for what, bad in refused_modules(dev):
        bad.to(dev).set_iter(-1)
        assert bad._slot == slot
        with pytest.raises(NeddfError):
            run(bad, t.s)
        direct = ctx.field_forward(slot, pos, d, var, OUT_FULL, KEYS["neddf", "full"])
        for k, v in direct.items():
            assert torch.equal(v.view(first[k].shape), first[k]), "after %s: the library's slot no longer answers with A's `%s`" % (what, k)
        same(run(t.net, t.s), first, "A after " + what)
    # the same with A's weights changed while the slot was being refused to others
    r_in_place(t.net)
    for what, bad in list(refused_modules(dev))[1:3]:
        bad.to(dev)
        with pytest.raises(NeddfError):
            run(bad, t.s)
    t.check("A changed, after refusals")


def test_refused_set_field_at_the_c_abi(dev, pts):
    """neddf_set_field refused on a loaded slot: neddf_field_forward on that slot returns 0 and writes the same bytes as before."""
    from neddf_amd._lib import Context, FieldDesc, _fp
    ctx, slot = Context.get(dev), 3
    kw = arch("neddf")
    net = build("neddf", kw, synth_state("neddf", kw, 7), dev)
    ws, bs = net._tensors()
    hw = [t.detach().to("cpu", torch.float32).contiguous() for t in ws]
    hb = [t.detach().to("cpu", torch.float32).contiguous() for t in bs]
    n = len(hw)
    wa = (_fp * n)(*[C.cast(t.data_ptr(), _fp) for t in hw])
    ba = (_fp * n)(*[C.cast(t.data_ptr(), _fp) for t in hb])
    good = net._descriptor()
    ctx.slot_owner.pop(slot, None)          # this test loads the slot behind the modules' backs
    assert ctx.lib.neddf_set_field(ctx.h, slot, C.byref(good), wa, ba, n) == 0, ctx.lib.neddf_last_error(ctx.h)
    pos, d, var = (torch.from_numpy(a).to(dev).contiguous() for a in pts)
    N = pos.numel() // 3
    vp = lambda t: C.c_void_p(t.data_ptr())

    def forward():
        out = [torch.full((N * c,), float("nan"), device=dev) for c in (1, 1, 3, 1, 1)]
        rc = ctx.lib.neddf_field_forward(ctx.h, slot, vp(pos), vp(d), vp(var), N, 1, *[vp(o) for o in out], ctx.stream())
        torch.cuda.synchronize(dev)
        return rc, [o.cpu().numpy().tobytes() for o in out]
    rc, first = forward()
    assert rc == 0 and not any(np.isnan(np.frombuffer(b, np.float32)).any() for b in first)

    def desc(**changes):
        bad = FieldDesc.from_buffer_copy(good)
        for k, v in changes.items():
            if k == "skips":
                bad.n_skips = len(v)
                for i, x in enumerate(v):
                    bad.skips[i] = x
            else:
                setattr(bad, k, v)
        return bad
    # refusals that come before the packer reads a weight (the arrays handed over are A's): (descriptor, tensors, code, message)
    refusals = [
        (desc(layer_width=640, col_layer_width=640), n, -3, "hidden widths must be in [1, 512]"),        # the control: refused at the door
        (desc(col_layer_width=256), n, -3, "NeDDF: col_layer_width must equal ddf_layer_width"),
        (desc(layer_count=14), n + 10, -3, "NeDDF: layer count out of range"),
        (desc(skips=[5]), n, -3, "NeDDF: skip index must address"),
        (desc(kind=2, activation=1), n + 1, -3, "NeuS: activation must be ReLU or tanhExp"),
        (good, n - 1, -1, "NeDDF: wrong tensor count"),
        (desc(kind=7), n, -1, "bad field kind"),
    ]
    for bad, count, code, text in refusals:
        assert ctx.lib.neddf_set_field(ctx.h, slot, C.byref(bad), wa, ba, count) == code, text
        assert ctx.lib.neddf_last_error(ctx.h).decode().startswith(text)
        rc, again = forward()
        assert rc == 0, "after '%s': %s" % (text, ctx.lib.neddf_last_error(ctx.h).decode())
        assert again == first, "after '%s': the slot answers with other bytes" % text
    assert ctx.lib.neddf_set_iter(ctx.h, slot, 1.1, 2.0, None) == 0


# ------------------------------------------------------------------------------------------------ one slot, many tenants
def test_slot_reuse_across_shapes_and_kinds(dev, orc, pts):
    """One slot of one context takes, in turn, networks of other engine widths (384 -> 512 columns, 72 -> 128, 200 -> 256), other kinds and
    unequal NeuS widths, then the 72-wide one again: nothing of a tenant -- zero padding, the three-term planes, skip / stash / head
    pointers -- may reach the next one's result."""
    s = sampling(pts, dev)
    tenants = [("neddf", arch("neddf", 384), 31), ("neddf", arch("neddf", 72), 32), ("neddf", arch("neddf", 200), 33), ("nerf", arch("nerf", 128), 34),
               ("neus", arch("neus", 128, 384), 35)]
    nets = []
    for kind, kw, seed in tenants:
        sd = synth_state(kind, kw, seed)
        mode = "minimal" if kind == "neddf" else None          # (minimal: the route that reads the three-term planes)
        nets.append((kind, kw, sd, mode, build(kind, kw, sd, dev, mode=mode)))
    slots = {net._slot for *_, net in nets}
    assert len(slots) == 1
    for kind, kw, sd, mode, net in nets + [nets[1]]:
        what = "%s %s" % (kind, kw.get("ddf_layer_width", kw.get("layer_width", kw.get("sdf_layer_width"))))
        got = run(net, s)
        same(got, fresh_eval(kind, kw, sd, dev, s, mode=mode), what)
        for k, ref in oracle_of(orc, kind, kw, sd, pts, mode=mode).items():      # test_random_architectures_vs_oracle's gate for these widths
            assert_close(got[k].cpu().numpy(), ref, RTOL, 2e-5, "%s `%s` vs oracle" % (what, k))
        if kind == "neddf":                                     # ... and the forward-mode kernels of the same tenant
            net.output_mode = "full"
            same(run(net, s), fresh_eval(kind, kw, sd, dev, s, mode="full"), what + " full")
            net.output_mode = "minimal"


@pytest.mark.parametrize("kind,mode", [("neddf", "minimal"), ("neddf", "full"), ("nerf", None), ("neus", None)])
def test_weight_dtype_round_trip(dev, pts, kind, mode):
    """fp32 -> bf16 -> f16_split -> fp32 on one module: every policy equals its fresh evaluation and the last result is the first."""
    kw = arch(kind)
    sd = synth_state(kind, kw, SEEDS[kind])
    s = sampling(pts, dev)
    net = build(kind, kw, sd, dev, mode=mode)
    results = []
    for dtype in ("fp32", "bf16", "f16_split", "fp32"):
        net.weight_dtype = dtype
        results.append(run(net, s))
        same(results[-1], fresh_eval(kind, kw, sd, dev, s, dtype, mode), "%s as %s" % (kind, dtype))
    same(results[3], results[0], "fp32 after the round trip")
    assert not all(torch.equal(results[1][k], results[0][k]) for k in results[0]), "bf16 operands must show in the result"


# ------------------------------------------------------------------------------------------------ iteration state
@pytest.mark.parametrize("kind,mode", [("neddf", "full"), ("neddf", "minimal"), ("nerf", None)])
def test_iteration_state_follows_set_iter(dev, orc, pts, kind, mode):
    """set_iter changes no weight and uploads nothing, yet every call has to run under the state the module holds now."""
    kw = arch(kind)
    sd = synth_state(kind, kw, SEEDS[kind])
    s = sampling(pts, dev)
    net = build(kind, kw, sd, dev, mode=mode)
    refs = {it: oracle_of(orc, kind, kw, sd, pts, it, mode) for it in (-1, 2500)}
    moved(refs[-1], refs[2500], "%s: iteration 2500 against evaluation" % kind)
    gated(run(net, s), refs[-1], "%s at -1" % kind)
    net.set_iter(2500)
    got = run(net, s)
    gated(got, refs[2500], "%s at 2500" % kind)
    same(got, fresh_eval(kind, kw, sd, dev, s, mode=mode, it=2500), "%s at 2500" % kind)
    net.set_iter(-1)
    got = run(net, s)
    gated(got, refs[-1], "%s back at -1" % kind)
    same(got, fresh_eval(kind, kw, sd, dev, s, mode=mode), "%s back at -1" % kind)


# ------------------------------------------------------------------------------------------------ training and evaluation interleaved
TRAIN_LR = 0.01


@pytest.mark.parametrize("width", [256, 192])
@pytest.mark.parametrize("kind", ["neddf", "neus"])
def test_train_and_evaluate_interleaved(dev, orc, pts, kind, width):
    """forward with autograd, backward, Adam step, no_grad forward -- twice.  Width 192 trains zero-padded to 256: the training call describes
    the slot with the padded network, the evaluation has to put the real one back.  The loss is a regression onto another network's outputs
    (the oracle's, on another synthetic state): steps towards values a network of this kind takes keep the second step in a regime where it
    still moves every output -- under a loss without a target the first step drives most NeDDF densities to the ReLU's zero, where they stay."""
    kw = arch(kind, width)
    mode = "full" if kind == "neddf" else None
    t = Tracked(kind, kw, synth_state(kind, kw, SEEDS[kind] + width), dev, orc, pts, mode=mode)
    assert (t.net._train_layout() is not None) == (width == 192)
    targets = {k: torch.from_numpy(v).to(dev) for k, v in oracle_of(orc, kind, kw, synth_state(kind, kw, 500 + width), pts, mode=mode).items()}

    def regression(o):
        return sum(((o[k] - targets[k]) ** 2).sum() for k in targets)
    for step in range(2):
        r_adam(t.net, t.s, TRAIN_LR, regression)
        got = t.check("%s %d after training step %d" % (kind, width, step))
        with torch.enable_grad():
            trained = t.net(t.s)
        for k in got:       # the gate of test_training_forward_matches_fused_path: two implementations of one function
            assert trained[k].requires_grad
            assert_close(trained[k].detach().cpu().numpy(), got[k].cpu().numpy(), RTOL, ATOL, "%s %d step %d: training forward vs fused `%s`" % (kind, width, step, k))
        same(run(t.net, t.s), got, "%s %d: evaluation after a training forward without a step" % (kind, width))


# ------------------------------------------------------------------------------------------------ renderers
def make_render(dev, seeds, kw=None):
    import neddf_amd
    kw = arch("neddf", 128) if kw is None else kw
    r = neddf_amd.NeRFRender(dict(kw, _target_="neddf.network.NeDDF"), sample_coarse=8, sample_fine=9, dist_near=2.0, dist_far=6.0, max_dist=6.0,
                             use_coarse_network=True, sampling_type="cone")
    for net, seed in zip((r.network_coarse, r.network_fine), seeds):
        net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state("neddf", kw, seed).items()})
    r.to(dev)
    r.set_iter(-1)
    return r


def make_camera(dev):
    import neddf_amd
    cam = neddf_amd.Camera(neddf_amd.PinholeCalib(np.array([40.0, 40.0, 16.0, 16.0])), np.array([0.0, 0.0, 0.0, 0.1, -0.1, 4.0], np.float32))
    return cam.to(dev)


def render(r, uv, cam, seed=5):
    torch.manual_seed(seed)
    with torch.no_grad():
        return {k: v.clone() for k, v in r.render_rays(uv, cam).items()}


def fresh_render(r, dev, uv, cam, seed=5):
    """a new NeRFRender loaded from r's state_dict, on a context of its own"""
    with fresh_context(dev):
        r2 = make_render(dev, (0, 0))
        r2.load_state_dict({k: v.detach().clone() for k, v in r.state_dict().items()})
        r2.to(dev)
        return render(r2, uv, cam, seed)


def uv12(dev):
    rng = np.random.default_rng(3)
    return torch.from_numpy(rng.integers(0, 32, (12, 2)).astype(np.int64)).to(dev)


def test_render_rays_after_an_optimiser_step(dev):
    """render_rays reads SLOT_COARSE and SLOT_FINE: after an Adam step on both networks (a real backward through render_rays) it must be the
    render of a new renderer loaded from the state_dict."""
    r, cam, uv = make_render(dev, (41, 42)), make_camera(dev), uv12(dev)
    before = render(r, uv, cam)
    same(before, fresh_render(r, dev, uv, cam), "first render")
    opt = torch.optim.Adam(r.get_parameters_list(), lr=0.03)
    for step in range(2):
        torch.manual_seed(7)
        with torch.enable_grad():
            o = r.render_rays(uv, cam)
            assert o["color"].requires_grad and o["color_coarse"].requires_grad
            signed_sum({k: o[k] for k in ("color", "depth", "fields_penalty", "color_coarse", "depth_coarse", "fields_penalty_coarse")}, step).backward()
        assert all(net.layers_ddf[0].weight.grad is not None and net.layers_col[0].weight.grad is not None for net in (r.network_coarse, r.network_fine))
        opt.step()
        opt.zero_grad(set_to_none=True)
        after = render(r, uv, cam)
        same(after, fresh_render(r, dev, uv, cam), "render after step %d" % step)
        for k in ("color", "color_coarse"):
            assert float((after[k] - before[k]).abs().max()) > 100.0 * (ATOL + RTOL), "step %d must show in `%s`" % (step, k)
        before = after


def test_two_renderers_alternate_on_one_context(dev):
    """A, B, A, B: both renderers want SLOT_COARSE and SLOT_FINE of the one shared context; each result is that renderer's own first."""
    cam, uv = make_camera(dev), uv12(dev)
    a, b = make_render(dev, (51, 52)), make_render(dev, (53, 54))
    first = {}
    for name, r in (("A", a), ("B", b), ("A", a), ("B", b)):
        got = render(r, uv, cam)
        if name not in first:
            first[name] = got
            same(got, fresh_render(r, dev, uv, cam), "%s's first render" % name)
        else:
            same(got, first[name], "%s's second render" % name)
    assert not torch.equal(first["A"]["color"], first["B"]["color"])


def test_direct_calls_and_render_rays_stay_coherent(dev, orc, pts):
    """network_fine called directly works in the slot render_rays loads: a change made between the two must reach both."""
    r, cam, uv = make_render(dev, (61, 62)), make_camera(dev), uv12(dev)
    kw = arch("neddf", 128)
    s = sampling(pts, dev)
    net = r.network_fine

    def direct_is_fresh(what):
        sd = state_of(net)
        got = run(net, s)
        same(got, fresh_eval("neddf", kw, sd, dev, s, mode="full"), what)
        gated(got, oracle_of(orc, "neddf", kw, sd, pts, mode="full"), what)
    ref = oracle_of(orc, "neddf", kw, state_of(net), pts, mode="full")
    direct_is_fresh("direct call")
    same(render(r, uv, cam), fresh_render(r, dev, uv, cam), "render after a direct call")
    r_in_place(net)                                 # direct call first, then the renderer
    now = oracle_of(orc, "neddf", kw, state_of(net), pts, mode="full")
    moved(ref, now, "in-place change")
    direct_is_fresh("direct call after a change")
    same(render(r, uv, cam), fresh_render(r, dev, uv, cam), "render after the changed direct call")
    r_data_mul_invalidate(net)                      # the renderer first, then the direct call
    moved(now, oracle_of(orc, "neddf", kw, state_of(net), pts, mode="full"), "p.data change + invalidate()")
    same(render(r, uv, cam), fresh_render(r, dev, uv, cam), "render after invalidate()")
    direct_is_fresh("direct call after the render that followed invalidate()")


# ------------------------------------------------------------------------------------------------ the other consumers of a slot
@pytest.mark.parametrize("kind", ["neddf", "neus"])
def test_extract_mesh_and_occupancy_after_a_change(dev, orc, pts, kind):
    """extract_mesh and the occupancy build upload by themselves: each as the FIRST consumer after a change."""
    from neddf_amd.occupancy import OccupancyGrid
    kw = arch(kind)
    field = "distance" if kind == "neddf" else "sdf"
    net = build(kind, kw, synth_state(kind, kw, SEEDS[kind]), dev, mode="full" if kind == "neddf" else None)
    mode = "full" if kind == "neddf" else None

    def levels():
        ref = oracle_of(orc, kind, kw, state_of(net), pts, mode=mode)
        # levels that cut through the volume whatever the weights have become: the median distance, the upper decile of the density
        return ref, float(np.median(ref[field])), float(np.quantile(ref["density"], 0.9))

    def mesh(n, thr):
        v, t = n.extract_mesh(field, threshold=thr, resolution=16)
        return v.clone(), t.clone()

    def occupancy(n, thr):
        return OccupancyGrid.from_field(n, resolution=8, threshold=thr, dilate=0).bits.clone()
    ref0, thr0, dens0 = levels()
    v0, t0 = mesh(net, thr0)
    bits0 = occupancy(net, dens0)
    assert v0.shape[0] > 0 and t0.shape[0] > 0
    for route, first in ((r_in_place, "mesh"), (r_data_mul_invalidate, "occupancy")):
        route(net)
        ref1, thr1, dens1 = levels()
        moved(ref0, ref1, "%s %s" % (kind, route.__name__))
        sd = state_of(net)
        if first == "mesh":
            v1, t1 = mesh(net, thr1)
            bits1 = occupancy(net, dens1)
        else:
            bits1 = occupancy(net, dens1)
            v1, t1 = mesh(net, thr1)
        with fresh_context(dev):
            new = build(kind, kw, sd, dev, mode=mode)
            v2, t2 = mesh(new, thr1)
            grid2 = OccupancyGrid.from_field(new, resolution=8, threshold=dens1, dilate=0)
            bits2, occupied = grid2.bits.clone(), grid2.n_occupied
        assert v2.shape[0] > 0 and 0 < occupied < 8 ** 3, "the levels must cut through the volume (%d vertices, %d cells)" % (v2.shape[0], occupied)
        assert v1.shape == v2.shape and torch.equal(v1, v2) and torch.equal(t1, t2), "%s: the mesh after %s is not the fresh module's" % (kind, route.__name__)
        assert torch.equal(bits1, bits2), "%s: the occupancy grid after %s is not the fresh module's" % (kind, route.__name__)
        assert not (v1.shape == v0.shape and torch.equal(v1, v0)), "the change must show in the mesh"
        assert not torch.equal(bits1, bits0), "the change must show in the occupancy grid"
        ref0, v0, t0, bits0 = ref1, v1, t1, bits1
