"""numpy restatement of the plain-fp16 weight packing (weight_dtype "f16": NEDDF_DTYPE_F16 = 3, operand policy 4 in the argument blocks,
neddf_amd/csrc/field_pack.hip) for tests/test_f16_policy_host.py.  The fragment order is the bf16 policy's (one 16-bit plane, 16 k-values
per super-step: tests/pack_check.py unpack with operands = 1); each weight is np.float16's rounding -- to nearest, ties to even,
subnormals below 2^-14, Inf beyond 65 520.  Everything that is not a fragment-major matrix (biases, heads, scalars) stays fp32 bit for bit,
as under every policy: pack_check.Expect says what each argument block has to hold."""
import numpy as np

import pack_check as pc

DTYPE_F16 = 3       # include/neddf_hip.h NEDDF_DTYPE_F16
OPERANDS_F16 = 4    # neddf_amd/csrc/kernels.h kOperandsH16 (3 is the three-term packing of fp32 fields)
AS_BF16 = 1         # the layout to unpack with


def f16_rne(x):
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(x, np.float32).astype(np.float16).view(np.uint16)


def expected(d, W, B):
    assert d["dtype"] == DTYPE_F16
    if d["kind"] == pc.NEDDF:
        return pc.expect_neddf(d, W, B, OPERANDS_F16)
    return (pc.expect_nerf if d["kind"] == pc.NERF else pc.expect_neus)(d, W, B, OPERANDS_F16)


def check(out, d, W, B):
    """pack_check.check for an accepted f16 case: one argument-block set, no three-term second packing"""
    assert out["rc"] == 0 and out["err"] == "", (out["rc"], out["err"])
    assert out["has3"] == 0
    e, blob, spans = expected(d, W, B), out["blob"], []
    assert out["blob_len"] == blob.size
    for name, want in e.M.items():
        assert name in out["M"], "%s is null or missing" % name
        off, ks, cols, operands = out["M"][name]
        assert (ks * 16, cols, operands) == (want.shape[0], want.shape[1], OPERANDS_F16), (name, out["M"][name], want.shape)
        n = pc.block_floats(ks, cols, AS_BF16)
        assert off % 64 == 0 and 0 <= off and off + n <= blob.size, name
        spans.append((off, off + n, name))
        planes = pc.unpack(blob, off, ks, cols, AS_BF16)
        assert planes.shape[0] == 1
        assert np.array_equal(planes[0], f16_rne(want)), "%s is not the nearest-even fp16 of the state tensor in the bf16 fragment order" % name
    for name, want in e.V.items():
        assert name in out["V"], "%s is null or missing" % name
        off, n = out["V"][name]
        assert n == want.size and off % 64 == 0 and 0 <= off and off + n <= blob.size, (name, off, n, want.size)
        spans.append((off, off + n, name))
        assert np.array_equal(blob[off:off + n].view(np.uint32), want.view(np.uint32)), name
    for name, want in e.S.items():
        got = out["S"][name]
        same = np.float32(got).view(np.uint32) == np.float32(want).view(np.uint32) if isinstance(want, np.floating) else got == want
        assert same, (name, got, want)
    assert set(out["M"]) | set(out["V"]) == set(e.M) | set(e.V), (set(out["M"]) | set(out["V"])) ^ (set(e.M) | set(e.V))
    spans.sort()
    for (a0, a1, an), (b0, b1, bn) in zip(spans, spans[1:]):
        assert a1 <= b0, "%s and %s overlap" % (an, bn)
