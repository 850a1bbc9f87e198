"""The plain fp16 operand policy (weight_dtype "f16", NEDDF_DTYPE_F16 = 3) as far as it can be checked without a device: the enum in the
header and in the ctypes binding, an ABI that stayed at 7, the packer's fp16 fragments against a numpy restatement
(tests/pack_check_f16.py: np.float16 rounding in the bf16 fragment order) on the shipped NeDDF and on padded widths of all three kinds,
and the range refusal -- a finite weight or bias beyond +-65504 would silently become Inf as an fp16 operand, so the packer answers
NEDDF_EUNSUPPORTED and hands back nothing, while Inf and NaN weights pass as under every policy.  The packer is the host-only unit that
neddf_set_field calls BEFORE it touches the slot; that the slot's previous field keeps answering after the refusal is a statement about
the device and is held by tests/test_gpu_f16_policy.py::test_out_of_range_weight_is_refused_and_the_slot_keeps_its_field."""
import os
import re
import subprocess

import numpy as np
import pytest
from conftest import ROOT

import pack_check as pc
import pack_check_f16 as pf
from pack_check import NEDDF, NERF, NEUS

F16 = pf.DTYPE_F16
REFUSAL = "weight_dtype f16: a finite weight or bias beyond +-65504 would become Inf as an fp16 operand"


def test_header_enum_and_binding_agree_and_the_abi_is_still_7():
    from neddf_amd import _lib
    text = open(os.path.join(ROOT, "include", "neddf_hip.h")).read()
    values = {k: int(v) for k, v in re.findall(r"\b(NEDDF_DTYPE_\w+)\s*=\s*(\d+)", text)}
    assert values == {"NEDDF_DTYPE_F32": 0, "NEDDF_DTYPE_BF16": 1, "NEDDF_DTYPE_F16_SPLIT": 2, "NEDDF_DTYPE_F16": 3}
    assert _lib.DTYPE == {"fp32": 0, "bf16": 1, "f16_split": 2, "f16": 3}
    assert re.search(r"#define\s+NEDDF_ABI_VERSION\s+7\b", text) and _lib.ABI_VERSION == 7


def _shipped():
    """descriptor and state tensors of the shipped bunny network, in neddf_set_field's order"""
    import torch

    import neddf_amd
    from neddf_amd.fixtures import BUNNY_SMOKE_CFG as cfg, bunny_smoke_weights
    net = neddf_amd.NeDDF(**cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in bunny_smoke_weights().items()})
    ws, bs = net._tensors()
    W = [w.detach().numpy().astype(np.float32) for w in ws]
    B = [b.detach().numpy().astype(np.float32).reshape(-1) for b in bs]
    d = pc.desc(NEDDF, cfg["embed_pos_rank"], cfg["embed_dir_rank"], cfg["ddf_layer_count"], cfg["ddf_layer_width"], cfg["col_layer_count"],
                cfg["col_layer_width"], skips=cfg["skips"], activation=2, density_activation=1, d_near=cfg["d_near"], dtype=F16)
    assert [(tuple(w.shape), b.size) for w, b in zip(W, B)] == pc.tensor_shapes(d)
    return d, W, B


def _poisoned(seed, tensor, value, bias=False):
    d = pc.desc(NEDDF, 3, 1, 4, 72, 3, 72, skips=(0,), dtype=F16)
    W, B = pc.random_tensors(d, seed)
    (B if bias else W)[tensor].reshape(-1)[5 % (B if bias else W)[tensor].size] = value
    return d, W, B


ACCEPTED = {"neddf-w72": lambda: (pc.desc(NEDDF, 3, 1, 4, 72, 3, 72, skips=(0,), dtype=F16),),       # padded to the 128-wide engine
            "nerf-w72": lambda: (pc.desc(NERF, 3, 1, 3, 72, skips=(1,), dtype=F16),),
            "neus-96-160": lambda: (pc.desc(NEUS, 3, 1, 3, 96, 2, 160, skips=(0,), activation=0, dtype=F16),),
            "shipped": _shipped}
# fp16's edge: 65504 is the largest half, 65519 still rounds to it, 65520 is the first value that rounds to Inf; tiny values go subnormal
EDGE_VALUES = np.array([65504.0, -65504.0, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, -3.0e-6, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11], np.float32)
REFUSED = {"weight-70000": (3, 70000.0, False), "weight-minus-70000": (1, -70000.0, False), "weight-65519": (0, 65519.0, False),
           "bias-70000": (2, 70000.0, True), "head-weight-70000": (5, 70000.0, False), "head-bias-70000": (7, -70000.0, True)}
NONFINITE = {"weight-inf": (2, np.inf), "weight-minus-inf": (0, -np.inf), "weight-nan": (2, np.nan)}        # (tensors whose element 5 is in layer[l].wp)


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    """{case: (descriptor, W, B, parsed output)}: one compile and one run of tests/capi/pack_dump.cpp, host side under ASan + UBSan"""
    tmp = tmp_path_factory.mktemp("pack_f16")
    csrc = os.path.join(ROOT, "neddf_amd", "csrc")
    exe = str(tmp / "pack_dump")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-g", "-I", csrc,
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "capi", "pack_dump.cpp"), os.path.join(csrc, "field_pack.hip"), "-o", exe])
    cases = {}
    for seed, (name, make) in enumerate(ACCEPTED.items()):
        got = make()
        d = got[0]
        W, B = got[1:] if len(got) == 3 else pc.random_tensors(d, 3000 + seed)
        if name == "neddf-w72":
            W[2].reshape(-1)[:EDGE_VALUES.size] = EDGE_VALUES
        cases[name] = (d, W, B)
    for seed, (name, (tensor, value, bias)) in enumerate(REFUSED.items()):
        cases[name] = _poisoned(3100 + seed, tensor, value, bias)
    for seed, (name, (tensor, value)) in enumerate(NONFINITE.items()):
        cases[name] = _poisoned(3200 + seed, tensor, value)
    # the same out-of-range weight under the policies that have the range (bf16, fp32): accepted, as before
    for dtype in (0, 1):
        d, W, B = _poisoned(3300, 3, 70000.0)
        cases["weight-70000-dtype%d" % dtype] = (dict(d, dtype=dtype), W, B)
    for name, (d, W, B) in cases.items():
        pc.write_case(str(tmp / name), d, W, B)
    p = subprocess.run([exe] + [str(tmp / name) for name in cases], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not any(s in p.stderr for s in ("Sanitizer", "runtime error")), p.stderr[-4000:]
    return {name: c + (pc.parse_out(str(tmp / name) + ".out"),) for name, c in cases.items()}


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_fp16_fragments_equal_the_numpy_restatement(packed, name):
    d, W, B, out = packed[name]
    pf.check(out, d, W, B)


def test_edge_values_round_as_ieee_half(packed):
    """the values planted in neddf-w72 reach the blob as np.float16 has them: 65504 stays, subnormals, ties to even"""
    d, W, B, out = packed["neddf-w72"]
    off, ks, cols, _ = out["M"]["ddf.layer[2].wp"]
    got = pc.unpack(out["blob"], off, ks, cols, pf.AS_BF16)[0]
    want = pf.f16_rne(pf.expected(d, W, B).M["ddf.layer[2].wp"])
    assert np.array_equal(got, want)
    halves = set(pf.f16_rne(EDGE_VALUES).tolist())
    assert {0x7bff, 0xfbff, 0x0400, 0x0001, 0x0000, 0x8032, 0x3c00, 0x3c02} <= halves and halves <= set(got.reshape(-1).tolist())


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_a_finite_value_beyond_the_half_range_is_refused(packed, name):
    out = packed[name][3]
    assert (out["rc"], out["err"]) == (-3, REFUSAL) and out["has3"] == 0 and out["blob"].size == 0


@pytest.mark.parametrize("name", sorted(NONFINITE))
def test_inf_and_nan_weights_are_accepted(packed, name):
    d, W, B, out = packed[name]
    assert out["rc"] == 0 and out["err"] == ""
    tensor, value = NONFINITE[name]
    off, ks, cols, _ = out["M"]["ddf.layer[%d].wp" % tensor]
    got = pc.unpack(out["blob"], off, ks, cols, pf.AS_BF16)[0].view(np.float16)
    assert (np.isnan(got).sum() == 1) if np.isnan(value) else ((got == np.float16(value)).sum() == 1)


@pytest.mark.parametrize("dtype", (0, 1))
def test_the_other_policies_keep_taking_that_weight(packed, dtype):
    d, W, B, out = packed["weight-70000-dtype%d" % dtype]
    pc.check(out, d, W, B)
