"""The weight packer behind neddf_set_field (neddf_amd/csrc/field_pack.hip) on the CPU: a stand-alone driver (tests/capi/pack_dump.cpp) packs
small networks of all three kinds under AddressSanitizer + UBSan, and tests/pack_check.py unpacks every block of every argument block by the
layout formula of kernels.h and compares it with the matrix numpy builds from the state tensors: fp32 bit for bit, bf16 the
round-to-nearest-even of the weight, three-term hi + mid + lo == w exactly, split fp16 h = 2^10 w toward zero and m the nearest half of the
rest.  Every pointer the kernels of a kind read is bound, inside the blob, 64-float aligned and overlaps no other."""
import os
import subprocess

import pytest
from conftest import ROOT

import pack_check as pc
from pack_check import NEDDF, NERF, NEUS

# the smallest cases that reach each branch (nothing wider than 256): one skip on every network under every stored policy (the three-term
# policy is the second packing of the fp32 NeDDF field), unequal NeuS widths both ways round, an odd NeRF width, two skips (apart and
# adjacent), encodings that push the engine width up (72 -> 256), and fp32 NeDDF without the second packing
CASES = {}
for dtype in (0, 1, 2):
    CASES["neddf-w72-dtype%d" % dtype] = pc.desc(NEDDF, 3, 1, 4, 72, 3, 72, skips=(0,), dtype=dtype)
    CASES["nerf-w72-dtype%d" % dtype] = pc.desc(NERF, 3, 1, 3, 72, skips=(1,), dtype=dtype)
    CASES["neus-w72-dtype%d" % dtype] = pc.desc(NEUS, 3, 1, 3, 72, 2, 72, skips=(1,), dtype=dtype)
CASES["neus-96-160"] = pc.desc(NEUS, 3, 1, 3, 96, 2, 160, skips=(0,), activation=0)
CASES["neus-160-96"] = pc.desc(NEUS, 4, 2, 2, 160, 1, 96, dtype=2)
CASES["nerf-w73"] = pc.desc(NERF, 3, 1, 3, 73, skips=(0,), activation=1)
CASES["nerf-w73-bf16-no-skip"] = pc.desc(NERF, 1, 1, 1, 73, dtype=1)
CASES["neddf-two-skips"] = pc.desc(NEDDF, 3, 1, 5, 72, 2, 72, skips=(0, 2))
CASES["neus-two-adjacent-skips"] = pc.desc(NEUS, 3, 1, 4, 72, 1, 72, skips=(0, 1), dtype=1)
CASES["nerf-two-skips"] = pc.desc(NERF, 3, 1, 4, 72, skips=(2, 0), dtype=2)
CASES["neddf-long-encodings"] = pc.desc(NEDDF, 10, 12, 3, 72, 2, 72, skips=(0,))
CASES["neddf-minimum-layers"] = pc.desc(NEDDF, 1, 1, 2, 72, 2, 72, dtype=2)
MFMA_CASES = {"neddf-w72-mfma": pc.desc(NEDDF, 3, 1, 4, 72, 3, 72, skips=(0,))}

REFUSALS = {        # descriptor, tensor count handed over -> code, message
    "neddf-col-width": (pc.desc(NEDDF, 3, 1, 4, 72, 3, 96), None, -3, "NeDDF: col_layer_width must equal ddf_layer_width (the reference's layer_col_out takes "
                        "ddf_layer_width inputs, neddf.py:145: its own forward fails otherwise)"),
    "neddf-tensor-count": (pc.desc(NEDDF, 3, 1, 4, 72, 3, 72), 7, -1, "NeDDF: wrong tensor count"),
    "neddf-layer-count": (pc.desc(NEDDF, 3, 1, 14, 72, 3, 72), None, -3, "NeDDF: layer count out of range"),
    "neddf-skip-last": (pc.desc(NEDDF, 3, 1, 4, 72, 3, 72, skips=(2,)), None, -3, "NeDDF: skip index must address a trunk layer followed by another "
                        "(the reference itself fails otherwise)"),
    "neddf-five-skips": (pc.desc(NEDDF, 3, 1, 7, 72, 2, 72, skips=(0, 1, 2, 3, 4)), None, -3, "NeDDF: more than 4 skip connections"),
    "nerf-tensor-count": (pc.desc(NERF, 3, 1, 3, 72), 5, -1, "NeRF: wrong tensor count"),
    "nerf-layer-count": (pc.desc(NERF, 3, 1, 13, 72), None, -3, "NeRF: layer count out of range"),
    "nerf-skip-negative": (pc.desc(NERF, 3, 1, 3, 72, skips=(-1,)), None, -3, "NeRF: skip index must address a layer followed by another"),
    "nerf-four-skips": (pc.desc(NERF, 3, 1, 6, 72, skips=(0, 1, 2, 3)), None, -3, "NeRF: more than 3 skip connections"),
    "neus-tensor-count": (pc.desc(NEUS, 3, 1, 3, 72, 2, 72), 8, -1, "NeuS: wrong tensor count"),
    "neus-layer-count": (pc.desc(NEUS, 3, 1, 3, 72, 13, 72), None, -3, "NeuS: layer count out of range"),
    "neus-leaky": (pc.desc(NEUS, 3, 1, 3, 72, 2, 72, activation=1), None, -3, "NeuS: activation must be ReLU or tanhExp"),
    "neus-skip-last": (pc.desc(NEUS, 3, 1, 3, 72, 2, 72, skips=(2,)), None, -3, "NeuS: skip index must address an sdf layer followed by another"),
    "neus-five-skips": (pc.desc(NEUS, 3, 1, 7, 72, 1, 72, skips=(0, 1, 2, 3, 4)), None, -3, "NeuS: more than 4 skip connections"),
    "bad-kind": (pc.desc(7, 3, 1, 3, 72), 0, -1, "bad field kind"),
}


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    """{case: (descriptor, W, B, parsed output)}: one compile, one run of the driver per environment"""
    tmp = tmp_path_factory.mktemp("pack")
    csrc = os.path.join(ROOT, "neddf_amd", "csrc")
    exe = str(tmp / "pack_dump")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-g", "-I", csrc,
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "capi", "pack_dump.cpp"), os.path.join(csrc, "field_pack.hip"), "-o", exe])
    result = {}
    for env_value, cases in (("split3", {**CASES, **{k: v[0] for k, v in REFUSALS.items()}}), ("mfma", MFMA_CASES)):
        tensors = {}
        for seed, (name, d) in enumerate(cases.items()):
            W, B = ([], []) if d["kind"] == 7 else pc.random_tensors(d, 1000 + seed)
            tensors[name] = (W, B)
            pc.write_case(str(tmp / name), d, W, B, REFUSALS[name][1] if name in REFUSALS else None)
        p = subprocess.run([exe] + [str(tmp / name) for name in cases], env=dict(os.environ, NEDDF_F32_PRODUCTS=env_value),
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and not any(s in p.stderr for s in ("Sanitizer", "runtime error")), p.stderr[-4000:]      # they report nothing
        for name, d in cases.items():
            result[name] = (d,) + tensors[name] + (pc.parse_out(str(tmp / name) + ".out"),)
    return result


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_block_unpacks_to_the_state_tensors(packed, name):
    d, W, B, out = packed[name]
    pc.check(out, d, W, B)


def test_fp32_neddf_without_the_three_term_packing(packed):
    """NEDDF_F32_PRODUCTS=mfma: one packing, has3 off, no pointer of ddf3 / col3 bound"""
    d, W, B, out = packed["neddf-w72-mfma"]
    pc.check(out, d, W, B, split3=False)
    assert out["has3"] == 0 and not any(n.startswith(("ddf3.", "col3.")) for n in list(out["M"]) + list(out["V"]))


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_keep_their_code_and_text(packed, name):
    out = packed[name][3]
    assert (out["rc"], out["err"]) == REFUSALS[name][2:] and out["has3"] == 0 and out["blob"].size == 0
