"""Points per field-kernel launch (neddf_capi.hip field_forward): 2^23 by default, except that the three-term fp32 DISTANCE kernel,
whose L2 hit rate falls with the launch size (profiles/r09_alignment.txt), runs a chunk as sub-launches of 2^20 points.  A launch
boundary must not show in the results: an evaluation that crosses one is bit-identical to the same points evaluated piece by piece."""
import os

import numpy as np
import pytest
import torch
from conftest import BUNNY_CFG

import synth

pytestmark = pytest.mark.gpu

N = (1 << 20) + 64 + 17             # one full three-term launch, then one full tile and a ragged one in a second launch
KEYS = ("distance", "density", "color", "aux_grad")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def net(dev, bunny_weights):
    import neddf_amd
    n = neddf_amd.NeDDF(**BUNNY_CFG)
    n.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in bunny_weights.items()})
    n = n.to(dev)
    n.set_iter(-1)
    n.output_mode = "minimal"
    return n


@pytest.fixture(scope="module")
def points(dev):
    pos, d, var = synth.random_sampling(1, N, seed=23)
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (pos, d, var))


def _eval(net, points, lo, hi):
    from neddf_amd import Sampling
    pos, d, var = points
    with torch.no_grad():
        o = net(Sampling(pos[:, lo:hi].contiguous(), d[:, lo:hi].contiguous(), var[:, lo:hi].contiguous()))
    return {k: o[k].clone() for k in KEYS}


def _launches(net, points, dev):
    """(distance launches, colour launches) of one evaluation of all N points, and its outputs."""
    from neddf_amd import Context
    ctx = Context.get(dev)
    ctx.set_timing(True)
    try:
        ctx.get_stage_timings()
        out = _eval(net, points, 0, N)
        st = ctx.get_stage_timings()
    finally:
        ctx.set_timing(False)
    return st["ddf"][1], st["col"][1], out


def _expected(ddf_log2):
    """(distance, colour) launches of N points: 2^23 per launch, the distance kernel of the policy under test 2^ddf_log2;
    NEDDF_FIELD_CHUNK_LOG2 (clamped to 16 .. 25 by the library) sets both."""
    e = os.environ.get("NEDDF_FIELD_CHUNK_LOG2", "").strip()
    if e not in ("", "0"):
        ddf_log2 = col_log2 = min(25, max(16, int(e)))
    else:
        col_log2 = 23
    return -(-N // (1 << ddf_log2)), -(-N // (1 << col_log2))


def test_default_launch_size_is_per_policy(dev, net, points):
    """2^20 + 81 fp32 points on the three-term kernels are two launches of the distance kernel and one of the colour kernel; under bf16
    (and every other policy, the fp32 MFMA of NEDDF_F32_PRODUCTS=mfma among them) they are one of each."""
    three_term = os.environ.get("NEDDF_F32_PRODUCTS", "") != "mfma"
    ddf, col, _ = _launches(net, points, dev)
    assert (ddf, col) == _expected(20 if three_term else 23), (ddf, col)
    net.weight_dtype = "bf16"
    try:
        ddf, col, _ = _launches(net, points, dev)
    finally:
        net.weight_dtype = "fp32"
    assert (ddf, col) == _expected(23), (ddf, col)


def test_launch_boundary_does_not_show_in_the_results(dev, net, points):
    """The same points in one call (whose three-term distance kernel is cut at 2^20) and piece by piece, cut at the boundary and inside the
    first launch: every output bit for bit."""
    whole = _eval(net, points, 0, N)
    for cuts in ((0, 1 << 20, N), (0, 333 * 64 + 5, N)):
        parts = [_eval(net, points, lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
        for k in KEYS:
            assert torch.equal(whole[k], torch.cat([p[k] for p in parts], 1)), (cuts, k)
