"""Host half of the pose gradients: ABI 7 and its symbols, configuration plumbing, and the fixture's own consistency
(tests/golden/pose_grad.npz: params.grad is R.grad / T.grad pushed through Camera.update_transform by torch on the CPU;
tests/golden/pose_grad_routes.npz: digests of the regenerated inputs, kink cap, size), and the fp64 restatements of
test_gpu_pose_routes.py against the reference's recorded sampler and ray-generation gradients."""
import os
import re

import numpy as np
import torch
from conftest import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("neddf_train_field_backward_inputs", "neddf_sampling_backward", "neddf_raygen_backward")


def test_abi_7_symbols_match_the_header():
    from neddf_amd import _lib
    header = open(os.path.join(ROOT, "include", "neddf_hip.h")).read()
    assert "#define NEDDF_ABI_VERSION 7" in header and _lib.ABI_VERSION == 7
    declared = set(re.findall(r"^(?:int|int64_t|void|const char \*)\s*(neddf_\w+)\(", header, re.M))
    bound = {name for name, _, _ in _lib.SYMBOLS}
    assert declared == bound, declared ^ bound
    lib = _lib.load()
    assert lib.neddf_abi_version() == 7
    for name in NEW:
        assert name in bound
        args = dict((n, a) for n, _, a in _lib.SYMBOLS)[name]
        proto = re.search(r"int %s\((.*?)\);" % name, header, re.S).group(1)
        assert len(args) == proto.count(",") + 1, name        # one ctypes argument per declared parameter


def test_pose_keywords_reach_render_and_trainer():
    import neddf_amd
    import inspect
    from neddf_amd.render import render_from_config
    cfg = {"_target_": "neddf.render.NeRFRender", "sample_coarse": 4, "sample_fine": 4, "use_coarse_network": False}
    r = render_from_config(dict(cfg, pose_gradients=True), network_config={"_target_": "neddf.network.NeDDF"}, _recursive_=False)
    assert r.pose_gradients is True
    assert render_from_config(cfg, network_config={"_target_": "neddf.network.NeDDF"}, _recursive_=False).pose_gradients is False
    assert neddf_amd.NeRFRender({"_target_": "neddf.network.NeDDF"}, use_coarse_network=False).pose_gradients is False
    sig = inspect.signature(neddf_amd.trainer.NeRFTrainer.__init__)
    assert sig.parameters["optimize_cameras"].default is False and sig.parameters["camera_lr"].default == 1e-3


def test_fixture_params_grad_is_the_chain_rule_of_R_and_T():
    """camera.params.grad of the reference's step = its R.grad / T.grad through update_transform (Rodrigues), by torch on the CPU."""
    import neddf_amd
    g = golden("pose_grad.npz")
    for case in ("cone", "moved"):
        pre = "t_%s_" % case
        cam = neddf_amd.Camera(neddf_amd.PinholeCalib(g[pre + "calib"].astype(np.float64)), g[pre + "initial_params"])
        cam.params.data.copy_(torch.from_numpy(g[pre + "params"]))
        cam.update_transform()
        np.testing.assert_allclose(cam.R.detach().numpy(), g[pre + "R"], rtol=0, atol=2e-6)
        np.testing.assert_allclose(cam.T.detach().numpy(), g[pre + "T"], rtol=0, atol=2e-6)
        ((cam.R * torch.from_numpy(g[pre + "grad_R"])).sum() + (cam.T * torch.from_numpy(g[pre + "grad_T"])).sum()).backward()
        got, want = cam.params.grad.numpy(), g[pre + "grad_params"]
        assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max(), (case, got, want)
    assert np.allclose(g["t_cone_grad_params"], [-0.1247, -0.4908, 0.1734, -0.6848, -0.5081, 0.1267], atol=5e-5)


def test_refine_pose_alias_and_cli():
    import importlib.util
    from neddf_amd.scripts import refine_pose
    spec = importlib.util.spec_from_file_location("refine_pose_alias", os.path.join(ROOT, "neddf", "scripts", "refine_pose.py"))
    alias = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(alias)
    assert alias.main is refine_pose.main
    a = refine_pose.build_parser().parse_args(["runs/x", "--epoch", "12", "--view", "3", "--perturb", "0.1", "0", "0", "0", "-0.2", "0",
                                               "--steps", "5", "--batch", "32"])
    assert (a.epoch, a.view, a.steps, a.batch) == (12, 3, 5, 32) and a.perturb == [0.1, 0, 0, 0, -0.2, 0] and str(a.output_dir) == "runs/x"
    d = refine_pose.build_parser().parse_args(["r"])
    assert d.perturb == [0.0] * 6 and d.view == 0


def test_route_fixture_is_consistent():
    """pose_grad_routes.npz loads, stays under the size limit of a committed file, its inputs regenerate from their seeds to the recorded
    digests, and at most one point in 32 of a case is marked as a kink."""
    import json
    import synth
    from conftest import GOLDEN
    assert os.path.getsize(os.path.join(GOLDEN, "pose_grad_routes.npz")) < 1 << 20
    g = golden("pose_grad_routes.npz")
    assert json.loads(str(g["cases"])) == list(synth.POSE_ROUTE_CASES)
    for case, (kind, rays, samples, _, _) in synth.POSE_ROUTE_CASES.items():
        n = rays * samples
        pos, d, var, ups = synth.pose_route_inputs(case)
        sums, sha = synth.input_digest(pos, d, var, ups)
        assert sha == str(g[case + "_digest_sha256"]), case
        np.testing.assert_array_equal(sums, g[case + "_digest_sums"], err_msg=case)
        assert str(g[case + "_kind"]) == kind and list(ups) == list(synth.FIELD_KEYS[kind])
        bits = np.unpackbits(g[case + "_kink"])
        assert len(bits) >= n and not bits[n:].any()
        assert int(bits[:n].sum()) * 32 <= n, (case, int(bits[:n].sum()))
        stride = int(g[case + "_out_stride"])
        for k in ups:
            assert g[case + "_out_" + k].shape[0] == (n + stride - 1) // stride
        for what in ("pos", "dir"):
            grad = g[case + "_grad64_" + what]
            assert grad.shape == (n, 3) and grad.dtype == np.float32 and np.isfinite(grad).all() and grad.any()
            # deviations over the unmarked points: below the marking threshold by construction
            assert 0 <= float(g[case + "_ref32_entry_" + what]) <= 1e-4 / 3 and 0 <= float(g[case + "_ref32_norm_" + what]) <= 1e-4 / 3


def test_restatements_reproduce_the_reference_gradients():
    """The fp64 restatements of the samplers and of ray generation that test_gpu_pose_routes.py measures the kernels against give the
    reference's own recorded gradients (pose_grad.npz `s_*`, `r_*`: torch autograd in fp32) within 1e-6 of the largest entry."""
    from test_gpu_pose_routes import raygen_backward_restatement, sampler_backward_restatement
    g = golden("pose_grad.npz")

    def same(what, got, want):
        dev = np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max()
        assert dev <= 1e-6, (what, dev)

    for tag, radius in (("cone", float(g["s_radius"])), ("point", None)):
        # (the reference's cone variance is differentiable in the ray direction, its point variance is a constant zero)
        g_rd, g_ro = sampler_backward_restatement(g["s_ro"], g["s_rd"], g["s_dists"], radius, g["s_g_pos"], g["s_g_dir"], g["s_g_var"])
        same(tag + " d/dray_dir", g_rd, g["s_%s_grad_rd" % tag])
        same(tag + " d/dray_orig", g_ro, g["s_%s_grad_ro" % tag])
    gR, gT = raygen_backward_restatement(g["r_uv"], g["r_calib"], g["r_g_rd"], g["r_g_ro"])
    same("d/dR", gR, g["r_grad_R"])
    same("d/dT", gT, g["r_grad_T"])
