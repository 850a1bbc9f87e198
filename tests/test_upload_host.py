"""The upload decision of BaseNeuralField.upload on the CPU.  The fused inference kernels never read a module's parameters: they read the
packed copy that `upload` pushes into a library slot, and `upload` skips the push when its signature matches Context.slot_owner[slot].  A
skip taken wrongly renders the wrong network with finite, plausible numbers, so the decision is pinned here, route by route, for all
three field kinds.  The context is the real Context over a recording stand-in for the library: Context.set_field and Context.set_iter
run as they are, nothing is launched.  (tests/test_gpu_upload.py holds the results to the same table on the device.)"""
import pytest
import torch

import neddf_amd
from neddf_amd._lib import Context, NeddfError

SLOT, OTHER_SLOT = 2, 3


class RecordingLib:
    """neddf_set_field / neddf_set_iter / neddf_last_error as far as Context calls them.  `refuse` makes the next neddf_set_field fail
    AND drop the slot's field -- the worst a failed call may leave behind (include/neddf_hip.h): the Python side has to survive it."""

    def __init__(self):
        self.valid, self.refuse, self.err = set(), False, b""

    def neddf_set_field(self, h, slot, desc, weights, biases, n):
        if self.refuse:
            self.valid.discard(slot)
            self.err = b"refused"
            return -3
        self.valid.add(slot)
        return 0

    def neddf_set_iter(self, h, slot, aux_grad_scale, distance_range_max, lowpass):
        if slot not in self.valid:
            self.err = b"no field in slot"
            return -2
        return 0

    def neddf_last_error(self, h):
        return self.err


class RecordingContext(Context):
    def __init__(self):
        self.lib, self.h, self.slot_owner = RecordingLib(), None, {}
        self.uploads, self.iters = [], []

    def set_field(self, slot, desc, weights, biases, signature):
        self.uploads.append(dict(slot=slot, desc=bytes(desc), w=[t.clone() for t in weights], b=[t.clone() for t in biases]))
        super().set_field(slot, desc, weights, biases, signature)

    def set_iter(self, slot, aux_grad_scale, distance_range_max, lowpass):
        self.iters.append((slot, aux_grad_scale, distance_range_max, list(lowpass)))
        super().set_iter(slot, aux_grad_scale, distance_range_max, lowpass)


KINDS = ("neddf", "nerf", "neus")


def make(kind, width=16, seed=0):
    torch.manual_seed(seed)
    if kind == "neddf":
        net = neddf_amd.NeDDF(embed_pos_rank=4, embed_dir_rank=2, ddf_layer_count=4, ddf_layer_width=width, col_layer_count=3,
                              col_layer_width=width, activation_type="tanhExp", density_activation_type="ReLU", skips=[1], lowpass_alpha_offset=0.0)
    elif kind == "nerf":
        net = neddf_amd.NeRF(embed_pos_rank=4, embed_dir_rank=2, layer_count=4, layer_width=width, skips=[1], lowpass_alpha_offset=0.0)
    else:
        net = neddf_amd.NeuS(embed_pos_rank=4, embed_dir_rank=2, sdf_layer_count=4, sdf_layer_width=width, col_layer_count=2,
                             col_layer_width=width, activation_type="ReLU", skips=[1])
    with torch.no_grad():
        for p in net.parameters():          # no zero bias: every tensor's values show in the record
            if p.dim() == 1:
                p.normal_(0.0, 0.05)
    return net


def uploads(net, ctx, slot=SLOT):
    """How many times one inference-mode upload call reached set_field."""
    n = len(ctx.uploads)
    net.upload(ctx, slot)
    return len(ctx.uploads) - n


def once(net, ctx, what, slot=SLOT):
    """The call uploads exactly once, with the values the module holds NOW, and a repeat is quiet."""
    assert uploads(net, ctx, slot) == 1, what + ": one upload expected"
    rec = ctx.uploads[-1]
    ws, bs = net._tensors()
    assert rec["slot"] == slot and len(rec["w"]) == len(ws) and len(rec["b"]) == len(bs)
    for got, want in zip(rec["w"] + rec["b"], ws + bs):
        assert torch.equal(got, want.detach().to(torch.float32).reshape(got.shape)), what + ": the upload carries other values than the module"
    assert uploads(net, ctx, slot) == 0, what + ": the repeated call uploaded again"


def fill_grads(net):
    for i, p in enumerate(net.parameters()):
        p.grad = torch.full_like(p, 0.01 * (i + 1))


def r_no_grad_mul(net):
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(0.5)


def r_copy(net):
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(p * 1.5 + 0.01)


def r_load_state_dict(net):
    net.load_state_dict({k: v * 0.75 - 0.01 for k, v in net.state_dict().items()})


def r_optimizer(make_opt):
    def route(net):
        fill_grads(net)
        make_opt(net.parameters()).step()
    return route


def r_data_assign(net):
    for p in net.parameters():
        p.data = p.data * 1.25 + 0.02


def r_double_float(net):
    net.double()
    net.float()


def r_weight_dtype(net):
    net.weight_dtype = "bf16" if net.weight_dtype == "fp32" else "fp32"


def r_invalidate(net):
    net.invalidate()


def r_data_mul_then_invalidate(net):
    for p in net.parameters():
        p.data.mul_(1.1)
    net.invalidate()


def r_d_near(net):
    net.d_near = 0.02


def r_penalty_weight(net):
    net.penalty_weight["constraints_color"] = 0.5


def r_skips(net):
    net.skips = [0]


ROUTES = [
    ("no_grad mul_", r_no_grad_mul), ("copy_", r_copy), ("load_state_dict", r_load_state_dict),
    ("Adam.step", r_optimizer(lambda ps: torch.optim.Adam(ps, lr=1e-2))),
    ("Adam(foreach=True).step", r_optimizer(lambda ps: torch.optim.Adam(ps, lr=1e-2, foreach=True))),
    ("Adam(foreach=False).step", r_optimizer(lambda ps: torch.optim.Adam(ps, lr=1e-2, foreach=False))),
    ("SGD.step", r_optimizer(lambda ps: torch.optim.SGD(ps, lr=1e-2))),
    ("p.data = tensor", r_data_assign), (".double().float()", r_double_float), ("weight_dtype", r_weight_dtype),
    ("invalidate()", r_invalidate), ("p.data.mul_() + invalidate()", r_data_mul_then_invalidate),
]
NEDDF_ROUTES = [("d_near", r_d_near), ("penalty_weight entry", r_penalty_weight), ("skips", r_skips)]


@pytest.mark.parametrize("kind", KINDS)
def test_every_mutation_route_uploads_exactly_once(kind):
    ctx, net = RecordingContext(), make(kind)
    once(net, ctx, "first call")
    for name, route in ROUTES + (NEDDF_ROUTES if kind == "neddf" else []):
        route(net)
        once(net, ctx, "%s after %s" % (kind, name))


@pytest.mark.parametrize("kind", KINDS)
def test_modules_and_slots_take_turns(kind):
    ctx, a, b = RecordingContext(), make(kind, seed=1), make(kind, seed=2)
    once(a, ctx, "A")
    once(b, ctx, "B, the same architecture on the same slot")
    once(a, ctx, "A back on the slot B took")
    once(a, ctx, "A on another slot", OTHER_SLOT)
    assert uploads(a, ctx) == 0 and uploads(a, ctx, OTHER_SLOT) == 0, "A owns both slots: nothing to upload"
    assert bytes(a._descriptor()) == bytes(b._descriptor())


@pytest.mark.parametrize("kind", KINDS)
def test_nothing_changed_uploads_nothing(kind):
    ctx, net = RecordingContext(), make(kind)
    once(net, ctx, "first call")
    for _ in range(3):
        assert uploads(net, ctx) == 0
    # the documented blind spot (BaseNeuralField.invalidate): a write through p.data bumps no version counter and moves no storage.
    # Pinned, so that changing it is a decision: whoever closes it turns this into a `once`.
    for p in net.parameters():
        p.data.mul_(0.5)
    assert uploads(net, ctx) == 0, "p.data.mul_() without invalidate() is the documented blind spot"
    net.invalidate()
    once(net, ctx, "invalidate() after p.data.mul_()")


@pytest.mark.parametrize("kind", ("neddf", "nerf"))
def test_set_iter_alone_uploads_nothing_but_is_sent_every_time(kind):
    ctx, net = RecordingContext(), make(kind)
    once(net, ctx, "first call")
    for it in (0, 2500, 7000, -1):
        net.set_iter(it)
        n = len(ctx.iters)
        assert uploads(net, ctx) == 0, "set_iter(%d) is no reason to upload" % it
        assert len(ctx.iters) == n + 1, "every upload call sends the iteration state"
        ags, drm, lp = net._iter_state()
        assert ctx.iters[-1] == (SLOT, ags, drm, list(lp)), "set_iter(%d): the library got another state than the module holds" % it
    states = [net.set_iter(it) or net._iter_state() for it in (0, 2500, -1)]
    assert states[0] != states[1] != states[2], "the iterations above must differ in what they send"


@pytest.mark.parametrize("route", ("version", "storage"))
@pytest.mark.parametrize("kind", KINDS)
def test_every_tensor_counts(kind, route):
    """Each parameter tensor alone -- every bias, the NeuS variance -- changed by a route that only the version counter shows (in-place
    under no_grad) and by one that only the address shows (p.data = tensor): a signature that leaves one tensor out fails here."""
    ctx, net = RecordingContext(), make(kind)
    once(net, ctx, "first call")
    names = [n for n, _ in net.named_parameters()]
    assert len(names) == sum(len(x) for x in net._tensors()) - (1 if kind == "neus" else 0), "a parameter the library never receives"
    for name, p in net.named_parameters():
        if route == "version":
            with torch.no_grad():
                p.add_(0.125)
        else:
            p.data = p.data + 0.125
        once(net, ctx, "%s: %s alone, %s route" % (kind, name, route))


@pytest.mark.parametrize("kind", KINDS)
def test_a_recycled_address_is_not_taken_for_the_packed_tensor(kind):
    """p.data = tensor leaves the version counter alone, so the address is the only witness -- and the allocator hands a freed block out
    again.  Reassign until the first address comes back (or 64 times): the values differ from the packed ones, so one upload is due."""
    ctx, net = RecordingContext(), make(kind, 128)
    once(net, ctx, "first call")
    p = next(q for q in net.parameters() if q.numel() == 128 * 128)      # 64 KiB: a size the host allocator hands straight back
    first = p.data_ptr()
    for i in range(64):
        p.data = torch.full_like(p.data, 0.01 * (i + 2))
        if p.data_ptr() == first:
            break
    once(net, ctx, "p.data reassigned %d times" % (i + 1))


def train_call(net, ctx, slot=SLOT):
    """The upload call of a training-mode forward (NeDDF._forward_with_grad, NeRF.forward, NeuS.forward); returns the descriptor it used."""
    ws, bs = net._tensors()
    desc, pw, pb = net._train_tensors(ws, bs)
    n = len(ctx.uploads)
    net.upload(ctx, slot, weights=False, train=(desc, pw, pb) if net._train_layout() is not None else None)
    return len(ctx.uploads) - n, desc


@pytest.mark.parametrize("kind", KINDS)
def test_training_mode_calls(kind):
    """weights=False: the training kernels read the live tensors, the slot only has to describe the architecture."""
    ctx, a, b = RecordingContext(), make(kind, 256, seed=1), make(kind, 256, seed=2)
    assert a._train_layout() is None
    once(a, ctx, "inference upload")
    assert train_call(a, ctx)[0] == 0, "same module, same architecture: no set_field"
    r_no_grad_mul(a)
    assert train_call(a, ctx)[0] == 0, "a training call does not care about the values"
    once(a, ctx, "the inference call after the weights changed during training")
    assert train_call(b, ctx)[0] == 1, "another module: the slot has to describe it"
    assert train_call(b, ctx)[0] == 0
    assert uploads(b, ctx) == 0, "that set_field carried B's weights: its inference call has nothing to add"
    r_optimizer(lambda ps: torch.optim.Adam(ps, lr=1e-2))(b)
    once(b, ctx, "B's inference call after an optimiser step")
    once(a, ctx, "A back")


@pytest.mark.parametrize("kind", KINDS)
def test_training_mode_zero_padded_width(kind):
    """Width 192 trains zero-padded to 256: the training call describes the slot with the PADDED descriptor, and the inference call
    afterwards has to put the unpadded field back -- once."""
    ctx, net = RecordingContext(), make(kind, 192)
    assert net._train_layout() is not None
    n, desc = train_call(net, ctx)
    assert n == 1 and desc.layer_width == 256
    assert ctx.uploads[-1]["desc"] == bytes(desc) != bytes(net._descriptor())
    shapes = [tuple(t.shape) for t in ctx.uploads[-1]["w"]]
    assert any(256 in s for s in shapes) and not any(192 in s for s in shapes), "the padded tensors describe the slot"
    assert train_call(net, ctx)[0] == 0, "the padded temporaries are new tensors every step: no reason to upload"
    once(net, ctx, "inference after padded training")
    assert ctx.uploads[-1]["desc"] == bytes(net._descriptor())
    assert train_call(net, ctx)[0] == 1, "back to training: the slot describes the unpadded field"
    once(net, ctx, "inference again")


@pytest.mark.parametrize("kind", KINDS)
def test_a_set_field_that_raises_frees_the_slot(kind):
    """B's upload fails and takes the slot's field with it.  A, the previous owner, has to upload again on its next call -- not go
    straight to set_iter on a slot that holds nothing ("no field in slot", until A's weights happen to change)."""
    ctx, a, b = RecordingContext(), make(kind, seed=1), make(kind, seed=2)
    once(a, ctx, "A")
    ctx.lib.refuse = True
    with pytest.raises(NeddfError, match="refused"):
        b.upload(ctx, SLOT)
    with pytest.raises(NeddfError, match="refused"):        # (A asks set_field again: "no field in slot" would come from set_iter)
        a.upload(ctx, SLOT)
    assert SLOT not in ctx.slot_owner, "a failed set_field leaves the slot without an owner"
    ctx.lib.refuse = False
    once(a, ctx, "A after the refused uploads")
    ctx.lib.refuse = True
    with pytest.raises(NeddfError):
        train_call(b, ctx)
    ctx.lib.refuse = False
    assert train_call(a, ctx)[0] == 1, "a training call of the previous owner describes the slot again"
    once(a, ctx, "A's inference call after that (width 16 trains zero-padded: the slot held the padded description)")
