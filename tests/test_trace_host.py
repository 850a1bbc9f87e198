"""Sphere tracing without a GPU: the numpy restatement (tests/trace_check.py) against closed-form ray-sphere depths, argument
validation of trace.sphere_trace and NeRFRender.render_image_traced, and the C ABI's new declarations and exports."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch
from conftest import BUNNY_CFG, ROOT

import trace_check as tc

NEW_SYMBOLS = ("neddf_trace_begin", "neddf_trace_compact", "neddf_trace_advance", "neddf_trace_finish", "neddf_trace_bisect_points",
               "neddf_trace_bisect_update", "neddf_trace_field")
T_NEAR, T_FAR, TAU = 1.0, 5.0, 0.02
MIN_STEP = (T_FAR - T_NEAR) * 2.0 ** -10
# a ray that grazes the level set from outside crosses the zone where D - tau < min_step in steps of min_step: a chord of at most
# 2 sqrt(2 (R + tau) min_step) = 0.13, i.e. 33 steps; around it the steps grow geometrically.  256 leaves no such ray EXHAUSTED.
MAX_STEPS = 256


def _sphere(pos):
    p = pos.astype(np.float32)
    return np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2]) - np.float32(tc.SPHERE_R)


def test_restatement_against_closed_form_sphere():
    o, d = tc.sphere_rays(4096)
    st, ev = tc.trace(o, d, _sphere, TAU, T_NEAR, T_FAR, MAX_STEPS, 1.0, MIN_STEP, 4)
    tc.check_sphere_closed_form(o, d, st, TAU, MIN_STEP, 4)
    hit = st["status"] == tc.HIT
    assert set(np.unique(st["status"])) <= {tc.HIT, tc.MISS}
    assert (st["t_lo"][hit] <= st["t"][hit]).all() and (st["distance"][hit] <= np.float32(TAU)).all()
    assert ev >= int(st["steps"].sum()) + int(hit.sum())               # every advance and every hit is one evaluation; bisections add theirs
    # the bracket: the distance at t_lo is still above the threshold wherever the ray advanced at all
    adv = hit & (st["t_lo"] < st["t"])
    assert (_sphere(o[adv] + st["t_lo"][adv, None] * d[adv]) > np.float32(TAU)).all()


def test_restatement_statuses_and_bookkeeping():
    o, d = tc.scene_rays(2048, 2.0, TAU)
    st, _ = tc.trace(o, d, tc.scene_distance, TAU, 2.0, 6.0, 12, 1.0, 4.0 * 2.0 ** -10, 3)
    k = np.arange(2048) % 16
    assert (st["status"][(k >= 6) & (k <= 9)] == tc.INVALID).all() and np.isnan(st["distance"][k == 6]).all()
    assert (st["status"][k == 5] == tc.HIT).all() and (st["steps"][k == 5] == 0).all() and (st["t"][k == 5] == np.float32(2.0)).all()
    for code in (tc.HIT, tc.MISS, tc.EXHAUSTED, tc.INVALID):
        assert (st["status"] == code).any(), code
    assert not (st["status"] == tc.ACTIVE).any() and st["steps"].max() <= 12
    miss = st["status"] == tc.MISS
    assert (st["t"][miss] > np.float32(6.0)).all() and (st["t_lo"][miss] <= np.float32(6.0)).all()
    # a NaN distance ends the ray as INVALID and is kept as the last distance read
    st2 = tc.begin(o[:4], d[:4], 2.0)
    idx, pos = tc.compact(o[:4], d[:4], st2)
    tc.advance(st2, idx, np.array([np.nan, 0.5, 0.01, np.inf], np.float32), TAU, 1.0, 0.01, 6.0)
    assert st2["status"].tolist() == [tc.INVALID, tc.ACTIVE, tc.HIT, tc.MISS] and st2["steps"].tolist() == [0, 1, 0, 1]
    assert st2["t"][1] == np.float32(2.0) + np.float32(1.0) * (np.float32(0.5) - np.float32(TAU)) and st2["t_lo"][1] == np.float32(2.0)


def test_sphere_trace_validates_its_arguments():
    from neddf_amd import NeddfError
    from neddf_amd.trace import default_min_step, sphere_trace, trace_params
    o = torch.zeros(4, 3)
    ok = dict(threshold=0.02, t_near=2.0, t_far=6.0)
    fn = lambda p: p[:, 0]                                            # noqa: E731
    assert default_min_step(2.0, 6.0) == 4.0 * 2.0 ** -10
    p = trace_params(0.02, 2.0, 6.0)
    assert (p.max_steps, p.refine, p.step_scale) == (64, 4, 1.0) and p.min_step == np.float32(4.0 * 2.0 ** -10)
    for bad in (dict(t_near=6.0), dict(t_far=float("nan")), dict(step_scale=0.0), dict(step_scale=1.5), dict(min_step=0.0), dict(min_step=-1.0),
                dict(max_steps=0), dict(max_steps=4097), dict(max_steps=2.5), dict(refine=-1), dict(refine=33), dict(threshold=float("nan"))):
        with pytest.raises(ValueError):
            sphere_trace(o, o, fn, **dict(ok, **bad))
    with pytest.raises(ValueError):
        sphere_trace(o, torch.zeros(5, 3), fn, **ok)
    with pytest.raises(ValueError):
        sphere_trace(torch.zeros(4, 2), torch.zeros(4, 2), fn, **ok)
    with pytest.raises(NeddfError):                                   # CPU tensors: no fallback
        sphere_trace(o, o, fn, **ok)


def _render(target, **kw):
    import neddf_amd
    return neddf_amd.NeRFRender(dict(kw, _target_=target), sample_coarse=8, sample_fine=8, use_coarse_network=False)


def test_render_image_traced_validates_its_arguments():
    import neddf_amd
    cam = neddf_amd.Camera(neddf_amd.PinholeCalib(np.array([10.0, 10.0, 4.0, 4.0])), None)
    render = _render("neddf.network.NeDDF", **BUNNY_CFG)
    with pytest.raises(ValueError):
        render.render_image_traced(8, 8, cam, ["weight"], 0.0275)
    for bad in (dict(step_scale=0.0), dict(min_step=0.0), dict(max_steps=0), dict(refine=40)):
        with pytest.raises(ValueError):
            render.render_image_traced(8, 8, cam, ["color"], 0.0275, **bad)
    render.ray_space = "ndc"
    with pytest.raises(NotImplementedError):
        render.render_image_traced(8, 8, cam, ["color"], 0.0275)
    nerf = _render("neddf.network.NeRF", embed_pos_rank=4, embed_dir_rank=2, layer_count=2, layer_width=64, activation_type="ReLU",
                   density_activation_type="ReLU", skips=[])
    with pytest.raises(NotImplementedError):
        nerf.render_image_traced(8, 8, cam, ["color"], 0.0275)


def test_header_declares_and_library_exports_the_trace_symbols():
    from neddf_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "neddf_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(neddf_[a-z_]+)\s*\(", hdr))
    bound = {name for name, _, _ in _lib.SYMBOLS}
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW_SYMBOLS:
        assert name in declared and name in bound and re.search(r"\bT %s\b" % name, exported), name
    assert "neddf_trace_params" in hdr and all("NEDDF_TRACE_" + k in hdr for k in ("ACTIVE", "HIT", "MISS", "EXHAUSTED", "INVALID"))
    import ctypes as C
    src = '#include "%s"\n#include <stdio.h>\nint main(){printf("%%zu", sizeof(neddf_trace_params)); return 0;}' % \
          os.path.join(ROOT, "include", "neddf_hip.h")
    exe = os.path.join("/tmp", "neddf_trace_sizes_%d" % os.getpid())
    subprocess.run(["gcc", "-x", "c", "-", "-o", exe], input=src.encode(), check=True)
    size = int(subprocess.check_output([exe]))
    os.remove(exe)
    assert size == C.sizeof(_lib.TraceParams)
    lib = _lib.load()                                                 # a NULL context is refused before anything is touched
    assert lib.neddf_trace_field(None, 0, None, None, 0, None, None, None, None, None, None, None, None) == -1
