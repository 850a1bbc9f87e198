#!/usr/bin/env python3
"""What the plain fp16 operand policy (weight_dtype "f16") costs and buys next to bf16, on the shipped bunny -> profiles/f16_policy_cost.json

    python tools/time_f16_policy.py                      # the whole record (both renders, stage timings, PSNR, error ratios)
    NEDDF_LIB_PATH=neddf_amd/csrc/libneddf_hip_v_<tag>.so python tools/time_f16_policy.py --quick --tag <tag> --out <file>
                                                         # one build variant of the policy's elementwise math (tile_engine.h NEDDF_H16_*):
                                                         # C2 only, error ratios, no fp32 frame

  C2            800 x 800, 128 single-pass samples (bench.py's workload)
  hierarchical  800 x 800, 65 coarse + 194 fine samples (render_image)
Both policies run interleaved in ONE process, bf16 / f16 / bf16 / f16 ..., after a warm-up of each; a frame's time is a host clock around
work that ends in a device synchronise; the figure is the median of --reps frames and the spread (min .. max) stays in the record, so that a
difference between the policies can be held against bf16's own repeats.  Kernel times per launch come from neddf_get_stage_timings in a
pass of their own (its events cost a little).  Switching the policy re-packs and uploads the weights (host arithmetic): that happens
before the clock starts.  PSNR is against the fp32 frame drawn with the same uniforms.  The error ratios are those of
tests/test_gpu_f16_policy.py (the cases and evaluation code both share: tests/f16_policy_cases.py), rms(f16 - ref) / rms(bf16 - ref)
per case, mode and output."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import neddf_amd  # noqa: E402
from neddf_amd.fixtures import BUNNY_SMOKE_CFG, BUNNY_SMOKE_RENDER, bunny_smoke_weights  # noqa: E402

W = H = 800
POLICIES = ("bf16", "f16")


def renderer(dev):
    r = neddf_amd.NeRFRender(dict(BUNNY_SMOKE_CFG, _target_="neddf.network.NeDDF"), **BUNNY_SMOKE_RENDER)
    r.network_fine.load_state_dict({k: torch.from_numpy(v) for k, v in bunny_smoke_weights().items()})
    r.to(dev)
    r.set_iter(-1)
    fx = 0.5 * W / np.tan(0.5 * 0.6911112070083618)
    cam = neddf_amd.Camera(neddf_amd.PinholeCalib(np.array([fx, fx, 0.5 * W, 0.5 * H])), None).to(dev)
    cam.R, cam.T = torch.eye(3, device=dev), torch.tensor([0.0, 0.0, 4.0], device=dev)
    return r, cam


def psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return 10.0 * np.log10(1.0 / mse) if mse > 0 else float("inf")


def measure(r, cam, dev, name, frame, prepare, reps, with_fp32):
    """frame(dtype) -> colour tensor [n, 3] / [h, w, 3] of one view under that policy, same uniforms for every policy;
    prepare(dtype): the switch of the policy with its weight upload, outside the clock"""
    ctx = r._ctx(dev)

    def timed(dtype):
        prepare(dtype)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c = frame(dtype)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, c

    color = {d: timed(d)[1] for d in POLICIES}           # warm-up: code objects, workspaces, the packed weights of both policies
    times = {d: [] for d in POLICIES}
    for _ in range(reps):
        for d in POLICIES:                               # interleaved
            times[d].append(timed(d)[0])
    stages = {}
    for d in POLICIES:
        prepare(d)
        frame(d)
        torch.cuda.synchronize()
        ctx.set_timing(True)
        ctx.get_stage_timings()
        frame(d)
        torch.cuda.synchronize()
        st = ctx.get_stage_timings()
        ctx.set_timing(False)
        stages[d] = {k: dict(ms=st[k][0], launches=st[k][1], ms_per_launch=st[k][0] / st[k][1]) for k in ("ddf", "col") if st[k][1]}
    if with_fp32:
        prepare("fp32")
    ref = frame("fp32") if with_fp32 else None
    out = {}
    for d in POLICIES:
        ms = sorted(1e3 * t for t in times[d])
        med = statistics.median(ms)
        out[d] = dict(frame_ms_median=med, frame_ms_min=ms[0], frame_ms_max=ms[-1], frame_ms_all=[1e3 * t for t in times[d]],
                      rays_per_s=W * H / (1e-3 * med), kernels=stages[d])
        if ref is not None:
            out[d]["psnr_db_vs_fp32"] = psnr(color[d], ref)
    b, f = out["bf16"], out["f16"]
    out["f16_over_bf16_time"] = f["frame_ms_median"] / b["frame_ms_median"]
    out["bf16_spread_of_median"] = (b["frame_ms_max"] - b["frame_ms_min"]) / b["frame_ms_median"]
    print("%-12s bf16 %.2f ms (%.2f .. %.2f), f16 %.2f ms (%.2f .. %.2f): f16 / bf16 = %.4f, bf16's own spread %.4f" % (
        name, b["frame_ms_median"], b["frame_ms_min"], b["frame_ms_max"], f["frame_ms_median"], f["frame_ms_min"], f["frame_ms_max"],
        out["f16_over_bf16_time"], out["bf16_spread_of_median"]), flush=True)
    for d in POLICIES:
        print("    %-5s %s%s" % (d, ", ".join("%s %.3f ms/launch x %d" % (k, v["ms_per_launch"], v["launches"]) for k, v in out[d]["kernels"].items()),
                                 ", PSNR %.2f dB" % out[d]["psnr_db_vs_fp32"] if ref is not None else ""), flush=True)
    return out


def error_ratios(dev):
    """rms(f16 - ref) / rms(bf16 - ref) over the cases tests/test_gpu_f16_policy.py gates (tests/f16_policy_cases.py)"""
    import f16_policy_cases as t
    bw, bs = t.bunny()
    rows = []
    with torch.no_grad():
        for name in t.CASES:
            kind, net, pts, exact = t.network_case(name, dev, bw, bs)
            for mode in t.MODES[kind]:
                if kind == "neddf":
                    net.output_mode = mode
                res = {}
                for dtype in ("fp32", "bf16", "f16"):
                    net.weight_dtype = dtype
                    res[dtype] = t.evaluate(net, kind, pts, t.N_MAX, dev)
                for k in res["f16"]:
                    ref = (exact[k] if k in exact else res["fp32"][k]).reshape(res["f16"][k].shape)
                    e16, eb = t.rms(res["f16"][k], ref), t.rms(res["bf16"][k], ref)
                    rows.append(dict(case=name, mode=mode, output=k, ref="fp64" if k in exact else "fp32", rms_f16=e16, rms_bf16=eb,
                                     ratio=e16 / eb if eb > 0 else None, max_f16=float(np.abs(res["f16"][k] - ref).max()),
                                     max_bf16=float(np.abs(res["bf16"][k] - ref).max())))
    worst = max((r for r in rows if r["ratio"] is not None), key=lambda r: r["ratio"])
    print("error ratios: %d outputs, worst %.3f (%s %s %s), median %.3f" % (
        len(rows), worst["ratio"], worst["case"], worst["mode"], worst["output"], statistics.median(r["ratio"] for r in rows if r["ratio"] is not None)), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="C2 and the error ratios only, no fp32 frame: one build variant")
    ap.add_argument("--tag", default="shipped")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f16_policy_cost.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the device: no HIP device, no numbers"
    dev = torch.device("cuda:0")
    r, cam = renderer(dev)
    U = torch.rand(W * H, 128, device=dev)

    def prepare(d):
        r.network_fine.weight_dtype = r.network_coarse.weight_dtype = d
        r._ctx(dev)

    def c2(d):
        return r.render_image_single_pass(W, H, cam, 128, U=U)["color"]

    def hier(d):
        torch.manual_seed(3)
        return r.render_image(W, H, cam, ["color"])["color"]

    rec = dict(tag=args.tag, library=os.environ.get("NEDDF_LIB_PATH", "neddf_amd/csrc/libneddf_hip.so"), device=torch.cuda.get_device_properties(0).gcnArchName,
               reps=args.reps, view="%d x %d, shipped bunny, camera at z = 4" % (W, H),
               method="policies interleaved in one process after a warm-up of each; host clock around a frame that ends in a device synchronise; "
                      "median of reps; kernel ms per launch from neddf_get_stage_timings in a pass of its own; PSNR against the fp32 frame "
                      "with the same uniforms")
    with torch.no_grad():
        rec["c2_single_pass_128"] = measure(r, cam, dev, "C2", c2, prepare, args.reps, not args.quick)
        if not args.quick:
            rec["hierarchical_65_194"] = measure(r, cam, dev, "hierarchical", hier, prepare, args.reps, True)
        rec["error_ratios"] = error_ratios(dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
