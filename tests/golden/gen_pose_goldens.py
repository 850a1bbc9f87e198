#!/usr/bin/env python3
"""Golden vectors of the pose-gradient chain (tests/golden/pose_grad.npz).  Like gen_goldens.py this runs only where the
reference checkout exists; it drives the reference's own autograd and stores inputs and gradients, data only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_pose_goldens.py

Records
  field level  f_<case>_*   NeDDF.forward on cone samples with pos / dir / var as leaves requiring grad, random upstream gradients on all
                            five outputs: pos.grad, dir.grad (var.grad is None in the reference: get_pe_weights runs with gradients
                            disabled, stored as zeros), the same from the fp64 network, and the fp32 reference's own deviation from fp64
  stage level  s_*          get_sampling_cones / get_sampling_points backward on random rays, create_rays backward to R and T
  step level   t_<case>_*   the training step of gen_goldens.gen_train (same seed, rays, targets, losses) with camera.params.grad,
                            camera.R.grad, camera.T.grad; a second case with a non-zero camera.params.  (Point sampling cannot be a
                            step-level case: the reference's NeDDF.forward fails on get_sampling_points' expanded sample_dir --
                            `.view` on a non-contiguous tensor, neddf.py:210 -- so the reference cannot take that step.  The stage-level
                            records cover the point sampler's backward.)  t_<case>_sens_*: the reference's own gradient deviation
                            under a 2e-6 change of R and T (the gate of the tests' end-to-end assertion)
  refinement   rf_*         the reference's Adam trajectory on camera.params for the view of tests/golden/bunny_pose (written here too)
                            from a perturbed pose with the field frozen: settings, initial and final pose error
`python gen_pose_goldens.py step` / `refine` regenerate those parts alone and merge them into the existing fixture.
`python gen_pose_goldens.py routes` writes tests/golden/pose_grad_routes.npz alone (gen_routes: the field's input gradients in fp64 on
every backward route of the training ABI; results only, the inputs are rebuilt from seeds).
"""
import json
import os
import sys

import numpy as np
import torch
import yaml

from gen_goldens import REF, make_camera, npy, save, synth

from neddf.network import NeDDF  # noqa: E402
from neddf.ray import Ray, Sampling  # noqa: E402
from neddf.render import NeRFRender  # noqa: E402

UP_KEYS = ("distance", "density", "color", "fields_penalty", "aux_grad")


def _deviation(a32, a64):
    """(norm, entry) deviation of the fp32 gradient from the fp64 one, relative to the fp64 norm / largest entry."""
    a32, a64 = a32.astype(np.float64), a64.astype(np.float64)
    n64 = np.linalg.norm(a64)
    return abs(np.linalg.norm(a32) - n64) / n64, np.abs(a32 - a64).max() / np.abs(a64).max()


def _field_case(arrs, tag, make, iteration, rays, samples, seed):
    rng = np.random.default_rng(seed)
    pos, dd, var = synth.random_sampling(rays, samples, seed=seed + 1, cone=True)
    ups = {k: rng.standard_normal((rays, samples) + ((3,) if k == "color" else ())).astype(np.float32) for k in UP_KEYS}
    grads = {}
    for dt, name in ((torch.float32, "32"), (torch.float64, "64")):
        torch.set_default_dtype(dt)         # the module's constants (frequencies, scales) are built in the default dtype
        try:
            m = make(dt)
            m.set_iter(iteration)
            leaves = [torch.from_numpy(a).to(dt).requires_grad_(True) for a in (pos, dd, var)]
            with torch.enable_grad():
                o = m(Sampling(*leaves))
                sum((o[k] * torch.from_numpy(ups[k]).to(dt)).sum() for k in UP_KEYS).backward()
        finally:
            torch.set_default_dtype(torch.float32)
        assert leaves[2].grad is None, "the reference differentiates the cone weights after all"
        grads[name] = (npy(leaves[0].grad), npy(leaves[1].grad))
        if name == "32":
            for k in UP_KEYS:
                arrs["f_%s_out_%s" % (tag, k)] = npy(o[k])
    pre = "f_%s_" % tag
    arrs.update({pre + "pos": pos, pre + "dir": dd, pre + "var": var, pre + "iteration": np.int32(iteration)})
    for k in UP_KEYS:
        arrs[pre + "g_" + k] = ups[k]
    for i, what in enumerate(("pos", "dir")):
        arrs[pre + "grad_" + what] = grads["32"][i]
        arrs[pre + "grad64_" + what] = grads["64"][i]
        arrs[pre + "ref32_norm_" + what], arrs[pre + "ref32_entry_" + what] = map(np.float64, _deviation(grads["32"][i], grads["64"][i]))
        print("  %s d/d%s: reference fp32 vs fp64 norm %.2e entry %.2e" % (tag, what, arrs[pre + "ref32_norm_" + what],
                                                                           arrs[pre + "ref32_entry_" + what]))
    arrs[pre + "grad_var"] = np.zeros_like(var)


def gen_field(arrs):
    cfg = yaml.safe_load(open(os.path.join(REF, "pretrained/bunny_smoke/.hydra/config.yaml")))
    ncfg = dict(cfg["network"], density_activation_type="ReLU")
    ncfg.pop("_target_")
    sd = torch.load(os.path.join(REF, "pretrained/bunny_smoke/models/model_02000.pth"), map_location="cpu")

    def bunny(dt):
        net = NeDDF(**ncfg)
        net.load_state_dict({k[len("network_fine."):]: v.to(dt) for k, v in sd.items() if k.startswith("network_fine.")})
        return net

    _field_case(arrs, "bunny", bunny, 1500, 2, 20, 301)
    for tag, kw in (("relu", dict(embed_pos_rank=6, embed_dir_rank=3, ddf_layer_count=6, col_layer_count=3, skips=[1, 3],
                                  activation_type="ReLU", density_activation_type="LeakyReLU")),
                    ("leaky", dict(embed_pos_rank=10, embed_dir_rank=4, ddf_layer_count=8, col_layer_count=4, skips=[4],
                                   activation_type="LeakyReLU", density_activation_type="tanhExp"))):
        def synthetic(dt, kw=kw):
            net = NeDDF(ddf_layer_width=256, col_layer_width=256, d_near=0.01, lowpass_alpha_offset=10,
                        penalty_weight={"constraints_aux_grad": 0.05, "constraints_dDdt": 0.5, "range_color": 0.1}, **kw)
            net.load_state_dict({k: torch.from_numpy(v).to(dt) for k, v in synth.neddf_state(
                embed_pos_rank=kw["embed_pos_rank"], embed_dir_rank=kw["embed_dir_rank"], ddf_layer_count=kw["ddf_layer_count"],
                col_layer_count=kw["col_layer_count"], skips=tuple(kw["skips"]), seed=23).items()})
            return net

        _field_case(arrs, tag, synthetic, 2500, 3, 11, 311)


def gen_field_nerf(arrs):
    """NeRF.forward (value rows only): the `relu250` field of train_nerf.npz, upstream gradients on density and colour."""
    from neddf.network import NeRF
    rng = np.random.default_rng(331)
    pos, dd, var = synth.random_sampling(3, 13, seed=332, cone=True)
    ups = {"density": rng.standard_normal((3, 13)).astype(np.float32), "color": rng.standard_normal((3, 13, 3)).astype(np.float32)}
    grads = {}
    for dt, name in ((torch.float32, "32"), (torch.float64, "64")):
        torch.set_default_dtype(dt)
        try:
            net = NeRF(**synth.NERF_RELU250["kw"])
            net.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(dt) for k, v in synth.nerf_state(**synth.NERF_RELU250["state"]).items()})
            net.set_iter(synth.NERF_RELU250["iteration"])
            leaves = [torch.from_numpy(a).to(dt).requires_grad_(True) for a in (pos, dd, var)]
            with torch.enable_grad():
                o = net(Sampling(*leaves))
                sum((o[k] * torch.from_numpy(ups[k]).to(dt)).sum() for k in ups).backward()
        finally:
            torch.set_default_dtype(torch.float32)
        assert leaves[2].grad is None
        grads[name] = (npy(leaves[0].grad), npy(leaves[1].grad))
        if name == "32":
            for k in ups:
                arrs["f_nerf_out_" + k] = npy(o[k])
    pre = "f_nerf_"
    arrs.update({pre + "pos": pos, pre + "dir": dd, pre + "var": var, pre + "iteration": np.int32(synth.NERF_RELU250["iteration"])})
    for k in ups:
        arrs[pre + "g_" + k] = ups[k]
    for i, what in enumerate(("pos", "dir")):
        arrs[pre + "grad_" + what] = grads["32"][i]
        arrs[pre + "grad64_" + what] = grads["64"][i]
        arrs[pre + "ref32_norm_" + what], arrs[pre + "ref32_entry_" + what] = map(np.float64, _deviation(grads["32"][i], grads["64"][i]))
        print("  nerf d/d%s: reference fp32 vs fp64 norm %.2e entry %.2e" % (what, arrs[pre + "ref32_norm_" + what],
                                                                          arrs[pre + "ref32_entry_" + what]))


POSE_VIEW_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bunny_pose")
POSE_VIEW_SIZE = 48


def pose_error(cam, R_ref, T_ref):
    """(rotation angle between cam.R and R_ref in radians, |cam.T - T_ref|) -- refine_pose.py's measure."""
    rel = npy(cam.R).astype(np.float64) @ R_ref.astype(np.float64).T
    return float(np.arccos(np.clip((np.trace(rel) - 1.0) * 0.5, -1.0, 1.0))), float(np.linalg.norm(npy(cam.T) - T_ref))


def _refine_render():
    cfg = yaml.safe_load(open(os.path.join(REF, "pretrained/bunny_smoke/.hydra/config.yaml")))
    rcfg = dict(cfg["render"]); rcfg.pop("_target_")
    render = NeRFRender(network_config=dict(cfg["network"], density_activation_type="ReLU"), **rcfg)
    render.load_state_dict(torch.load(os.path.join(REF, "pretrained/bunny_smoke/models/model_02000.pth"), map_location="cpu"))
    render.set_iter(-1)
    return render


def gen_pose_view():
    """tests/golden/bunny_pose/: ONE view whose image, intrinsics and pose agree with the shipped field -- frame 3 of bunny_smoke's
    test split as the reference itself renders it (density activation ReLU, the training tests' configuration) at 48 x 48 with the
    dataset's camera_angle_x.  (bunny_mini cannot serve: its 72 x 56 images are crops kept with the full view's camera_angle_x, so no
    pose explains them, and the reference's refinement moves away from the dataset pose there.)  The PNG holds round(256 c) in the
    loader's channel order, alpha 255; read with use_mask = False the loader returns exactly those numbers."""
    from PIL import Image
    tf = json.load(open(os.path.join(REF, "data/bunny_smoke/transforms_test.json")))
    n = POSE_VIEW_SIZE
    cam, _ = make_camera(n, n, tf["frames"][3], tf["camera_angle_x"])
    cam.update_transform()
    torch.manual_seed(5)
    img = _refine_render().render_image(n, n, cam, ["color"], 1, 256)["color"]
    bgr = np.clip(np.rint(npy(img).reshape(n, n, 3) * 256), 0, 255).astype(np.uint8)
    os.makedirs(os.path.join(POSE_VIEW_DIR, "test"), exist_ok=True)
    rgba = np.concatenate([bgr[:, :, ::-1], np.full((n, n, 1), 255, np.uint8)], 2)
    Image.fromarray(rgba, "RGBA").save(os.path.join(POSE_VIEW_DIR, "test", "r_0.png"))
    meta = {"camera_angle_x": tf["camera_angle_x"], "frames": [{"file_path": "./test/r_0", "transform_matrix": tf["frames"][3]["transform_matrix"]}]}
    for split in ("test", "train"):
        json.dump(meta, open(os.path.join(POSE_VIEW_DIR, "transforms_%s.json" % split), "w"))
    print("wrote bunny_pose/ (%d x %d)" % (n, n))


def gen_refine(arrs, steps=60, batch=64, lr=5e-3, seed=21):
    """The reference's own Adam trajectory on camera.params for the view of tests/golden/bunny_pose from a perturbed pose, field frozen:
    per step update_transform, `batch` random pixels drawn as nerf_trainer.py:98-103 draws them, ColorLoss against the image -- the loop
    of neddf_amd/scripts/refine_pose.py.  The settings are chosen so that the reference at least halves both pose errors (asserted)."""
    from neddf.dataset import NeRFSyntheticDataset
    from neddf.loss import ColorLoss
    from neddf.camera import Camera, PinholeCalib
    render = _refine_render()
    ds = NeRFSyntheticDataset(POSE_VIEW_DIR, "test", use_mask=False)
    item = ds[0]
    cam = Camera(PinholeCalib(item["camera_calib_params"]), item["camera_params"])
    cam.update_transform()
    R_ref, T_ref = npy(cam.R), npy(cam.T)
    perturb = np.array([0.03, -0.02, 0.015, 0.06, -0.04, 0.05], np.float32)
    cam.params.data.copy_(torch.from_numpy(perturb))
    cam.update_transform()
    errs = [pose_error(cam, R_ref, T_ref)]
    opt = torch.optim.Adam([cam.params], lr=lr)
    loss_fn = ColorLoss(weight=1.0, weight_coarse=0.1)
    h, w = item["rgb_images"].shape[:2]
    torch.manual_seed(seed)
    traj = [npy(cam.params)]
    for step in range(steps):
        with torch.enable_grad():
            cam.update_transform()
            opt.zero_grad()
            render.zero_grad()
            us = (torch.rand(batch) * (w - 1)).to(torch.int16)
            vs = (torch.rand(batch) * (h - 1)).to(torch.int16)
            target = {"color": torch.from_numpy(((1.0 / 256) * item["rgb_images"][vs.numpy().astype(np.int64), us.numpy().astype(np.int64), :]).astype(np.float32))}
            out = render.render_rays(torch.stack([us, vs], 1), cam)
            loss = torch.sum(torch.stack(list(loss_fn(out, target).values())))
            loss.backward()
            opt.step()
        cam.update_transform()
        traj.append(npy(cam.params))
        errs.append(pose_error(cam, R_ref, T_ref))
        print("  refine step %d loss %.5f error %s" % (step, float(loss), errs[-1]), flush=True)
    e0, e1 = errs[0], errs[-1]
    assert e1[0] <= 0.5 * e0[0] and e1[1] <= 0.5 * e0[1], ("the reference does not halve the pose error with these settings", e0, e1)
    arrs.update(rf_perturb=perturb, rf_steps=np.int32(steps), rf_batch=np.int32(batch), rf_lr=np.float64(lr), rf_seed=np.int32(seed),
                rf_view=np.int32(0), rf_initial_error=np.array(e0), rf_final_error=np.array(e1), rf_trajectory=np.stack(traj),
                rf_errors=np.array(errs))


def gen_stage(arrs):
    rng = np.random.default_rng(401)
    B, S = 9, 70                    # more samples than a wavefront has lanes
    rd = rng.standard_normal((B, 3)).astype(np.float32)
    rd /= np.linalg.norm(rd, axis=1, keepdims=True)
    ro = rng.uniform(-3, 3, (B, 3)).astype(np.float32)
    dists = np.sort(rng.uniform(2, 6, (B, S)).astype(np.float32), axis=1)
    ups = [rng.standard_normal((B, S, 3)).astype(np.float32) for _ in range(3)]
    radius = 1.0 / 1111 / np.sqrt(12)
    arrs.update(s_rd=rd, s_ro=ro, s_dists=dists, s_g_pos=ups[0], s_g_dir=ups[1], s_g_var=ups[2], s_radius=np.float64(radius))
    for tag in ("cone", "point"):
        d_, o_ = torch.from_numpy(rd).requires_grad_(True), torch.from_numpy(ro).requires_grad_(True)
        with torch.enable_grad():
            ray = Ray(d_, o_, torch.zeros(B, 2))
            smp = ray.get_sampling_cones(torch.from_numpy(dists), radius) if tag == "cone" else ray.get_sampling_points(torch.from_numpy(dists))
            obj = (smp.sample_pos * torch.from_numpy(ups[0])).sum() + (smp.sample_dir * torch.from_numpy(ups[1])).sum()
            if smp.diag_variance.requires_grad:
                obj = obj + (smp.diag_variance * torch.from_numpy(ups[2])).sum()
            obj.backward()
        arrs["s_%s_grad_rd" % tag], arrs["s_%s_grad_ro" % tag] = npy(d_.grad), npy(o_.grad)
    # create_rays backward
    tf = json.load(open(os.path.join(REF, "data/bunny_smoke/transforms_test.json")))
    cam, calib = make_camera(400, 400, tf["frames"][5], tf["camera_angle_x"])
    uv = torch.from_numpy(rng.integers(0, 400, (300, 2)).astype(np.int16))     # more rays than the reduction has threads
    g_rd, g_ro = rng.standard_normal((300, 3)).astype(np.float32), rng.standard_normal((300, 3)).astype(np.float32)
    with torch.enable_grad():
        cam.update_transform()
        cam.R.retain_grad(); cam.T.retain_grad()
        rays = cam.create_rays(uv)
        ((rays.ray_dir * torch.from_numpy(g_rd)).sum() + (rays.ray_orig * torch.from_numpy(g_ro)).sum()).backward()
    arrs.update(r_uv=npy(uv), r_calib=calib, r_R=npy(cam.R), r_T=npy(cam.T), r_g_rd=g_rd, r_g_ro=g_ro, r_grad_R=npy(cam.R.grad),
                r_grad_T=npy(cam.T.grad))


def gen_step(arrs):
    from neddf.loss import ColorLoss, FieldsConstraintLoss, MaskBCELoss
    cfg = yaml.safe_load(open(os.path.join(REF, "pretrained/bunny_smoke/.hydra/config.yaml")))
    tf = json.load(open(os.path.join(REF, "data/bunny_smoke/transforms_test.json")))
    ncfg = dict(cfg["network"], density_activation_type="ReLU")
    for tag, params0 in (("cone", np.zeros(6, np.float32)),
                         ("moved", np.array([0.02, -0.015, 0.01, 0.03, -0.02, 0.025], np.float32))):
        rcfg = dict(cfg["render"]); rcfg.pop("_target_")
        render = NeRFRender(network_config=ncfg, **rcfg)
        render.load_state_dict(torch.load(os.path.join(REF, "pretrained/bunny_smoke/models/model_02000.pth"), map_location="cpu"))
        render.set_iter(1500)
        cam, calib = make_camera(400, 400, tf["frames"][3], tf["camera_angle_x"])
        cam.params.data.copy_(torch.from_numpy(params0))
        rng = np.random.default_rng(77)         # gen_train's rays and targets
        uv = torch.from_numpy(rng.integers(140, 260, (12, 2)).astype(np.int16))
        target = {"color": torch.from_numpy(rng.uniform(0, 1, (12, 3)).astype(np.float32)),
                  "mask": torch.from_numpy((rng.uniform(0, 1, 12) > 0.5).astype(np.float32)),
                  "fields_penalty": torch.zeros(12)}
        losses = [ColorLoss(weight=1.0, weight_coarse=0.1), MaskBCELoss(weight=0.05, weight_coarse=0.005),
                  FieldsConstraintLoss(weight=0.01, weight_coarse=0.01)]
        def step(dR=None, dT=None):
            torch.manual_seed(9)
            cam.params.grad = None
            with torch.enable_grad():
                render.zero_grad()
                cam.update_transform()
                if dR is not None:      # the pose as another fp32 Rodrigues would round it; the graph to params stays
                    cam.R, cam.T = cam.R + torch.from_numpy(dR), cam.T + torch.from_numpy(dT)
                cam.R.retain_grad(); cam.T.retain_grad()
                out = render.render_rays(uv, cam)
                ld = {}
                for f in losses:
                    ld.update(f(out, target))
                loss = torch.sum(torch.stack(list(ld.values())))
                loss.backward()
            return loss, (npy(cam.R.grad), npy(cam.T.grad), npy(cam.params.grad))

        # Sensitivity of the reference's own gradients to the rounding of R and T: a device computes Rodrigues in fp32 with other
        # roundings than torch on the CPU (agreement is asserted at 2e-6 in the tests), and the highest encoding frequency turns 1e-6
        # of R into ~3e-3 rad of phase.  Four perturbations of +-2e-6 per entry; the largest (norm, entry) deviation per gradient is
        # recorded and sets the gate of the tests' end-to-end assertion (3 x, like the fp32-vs-fp64 records).
        prng = np.random.default_rng(909)
        pert = [step(prng.uniform(-2e-6, 2e-6, (3, 3)).astype(np.float32), prng.uniform(-2e-6, 2e-6, 3).astype(np.float32))[1]
                for _ in range(4)]
        loss, base = step()
        pre = "t_%s_" % tag
        for i, what in enumerate(("R", "T", "params")):
            devs = [_deviation(pg[i], base[i]) for pg in pert]
            arrs[pre + "sens_norm_" + what] = np.float64(max(d[0] for d in devs))
            arrs[pre + "sens_entry_" + what] = np.float64(max(d[1] for d in devs))
            print("  step %s d/d%s: reference's deviation under a 2e-6 change of R, T: norm %.2e entry %.2e"
                  % (tag, what, arrs[pre + "sens_norm_" + what], arrs[pre + "sens_entry_" + what]))
        arrs.update({pre + "uv": npy(uv), pre + "calib": calib,
                     pre + "params": params0, pre + "R": npy(cam.R), pre + "T": npy(cam.T), pre + "target_color": npy(target["color"]),
                     pre + "target_mask": npy(target["mask"]), pre + "loss": npy(loss), pre + "grad_params": npy(cam.params.grad),
                     pre + "grad_R": npy(cam.R.grad), pre + "grad_T": npy(cam.T.grad), pre + "sampling_type": np.array(rcfg["sampling_type"])})
        m = np.array(tf["frames"][3]["transform_matrix"], dtype=np.float64)
        from scipy.spatial.transform import Rotation
        arrs[pre + "initial_params"] = np.r_[Rotation.from_matrix(m[:3, :3]).as_rotvec(), m[:3, 3]].astype(np.float32)
        print("  step %s: camera.params.grad = %s" % (tag, np.array2string(npy(cam.params.grad), precision=4)))


HERE = os.path.dirname(os.path.abspath(__file__))
ROUTES_MAX_BYTES = 1 << 20          # the size limit of a committed file
KINK_GATE = 1e-4 / 3                # a third of the tests' base gate, of the largest entry
KINK_CAP = 32                       # at most one point in 32 of a case may be marked
ROUTES_OUT_STRIDE = {"bunny_many": 4, "neddf512_many": 4}       # the many-workgroup cases store the outputs of every 4th point (file size)


def _route_networks():
    """case -> (constructor, keywords, state dict (numpy), iteration).  Architectures that already have a parameter-gradient fixture are
    taken from it (stored `*_config`, the state seed of its generator), so these are the networks test_gpu_train.py already gates."""
    from neddf.network import NeRF
    cfg = yaml.safe_load(open(os.path.join(REF, "pretrained/bunny_smoke/.hydra/config.yaml")))
    bunny_kw = dict(cfg["network"], density_activation_type="ReLU")
    bunny_kw.pop("_target_")
    sd = torch.load(os.path.join(REF, "pretrained/bunny_smoke/models/model_02000.pth"), map_location="cpu")
    bunny_sd = {k[len("network_fine."):]: npy(v) for k, v in sd.items() if k.startswith("network_fine.")}
    nets = {"bunny": (NeDDF, bunny_kw, bunny_sd, 1500, -1)}
    for case, fx, seed, it in (("neddf128", "train_widths.npz", 29, 2500), ("neddf192", "train_widths.npz", 29, 2500),
                               ("neddf384", "train_wide.npz", 37, 2500), ("neddf512", "train_wide.npz", 37, 2500),
                               ("nerf128", "train_widths.npz", 31, 1500), ("nerf384", "train_wide_nerf.npz", 41, 1500),
                               ("nerf512", "train_wide_nerf.npz", 41, 1500)):
        kw = json.loads(str(np.load(os.path.join(HERE, fx))[case + "_config"]))
        nets[case] = (NeRF if case.startswith("nerf") else NeDDF, kw, None, it, seed)
    # the encoding limits of the input-gradient kernel: 6 x 10 = 60 of the 64 S-columns, 6 x 20 = 120 of the 128 U-columns; ranks of 1
    nets["ranks_hi"] = (NeDDF, dict(embed_pos_rank=10, embed_dir_rank=10, ddf_layer_count=5, ddf_layer_width=256, col_layer_count=3,
                                    col_layer_width=256, d_near=0.01, activation_type="tanhExp", density_activation_type="ReLU", skips=[1],
                                    lowpass_alpha_offset=10), None, 2500, 43)
    nets["nerf_ranks_hi"] = (NeRF, dict(embed_pos_rank=10, embed_dir_rank=10, layer_count=5, layer_width=256, activation_type="tanhExp",
                                        density_activation_type="ReLU", skips=[2], lowpass_alpha_offset=10), None, 1500, 44)
    nets["ranks_lo"] = (NeDDF, dict(embed_pos_rank=1, embed_dir_rank=1, ddf_layer_count=5, ddf_layer_width=256, col_layer_count=3,
                                    col_layer_width=256, d_near=0.01, activation_type="LeakyReLU", density_activation_type="ReLU", skips=[1],
                                    lowpass_alpha_offset=10), None, 2500, 45)
    nets["bunny_many"], nets["neddf512_many"] = nets["bunny"], nets["neddf512"]
    return nets


def gen_routes():
    """tests/golden/pose_grad_routes.npz: per case of synth.POSE_ROUTE_CASES the fp64 reference's pos.grad / dir.grad (stored as float32: a
    rounding of 6e-8, far below the gates), the fp32 reference's outputs and its own deviation from fp64, the kink mask and the digest
    of the inputs.  Kink points: an fp32 ReLU that flips against fp64 changes one point's gradient by a finite amount, in the reference
    as much as in any fp32 implementation; the points whose fp32 reference gradient deviates from fp64 by more than KINK_GATE of the
    largest entry are marked (packed bits), and the recorded deviations are taken over the unmarked points."""
    arrs = {"cases": np.array(json.dumps(list(synth.POSE_ROUTE_CASES)))}
    nets = _route_networks()
    for case, (kind, rays, samples, _, _) in synth.POSE_ROUTE_CASES.items():
        cls, kw, sd, iteration, state_seed = nets[case]
        if sd is None:
            sd = synth.arch_state(kind, kw, state_seed)
        pos, dd, var, ups = synth.pose_route_inputs(case)
        grads, outs = {}, None
        for dt, name in ((torch.float32, "32"), (torch.float64, "64")):
            torch.set_default_dtype(dt)         # the module's constants (frequencies, scales) are built in the default dtype
            try:
                m = cls(**kw)
                m.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(dt) for k, v in sd.items()})
                m.set_iter(iteration)
                leaves = [torch.from_numpy(a).to(dt).requires_grad_(True) for a in (pos, dd, var)]
                with torch.enable_grad():
                    o = m(Sampling(*leaves))
                    sum((o[k] * torch.from_numpy(ups[k]).to(dt)).sum() for k in ups).backward()
            finally:
                torch.set_default_dtype(torch.float32)
            assert leaves[2].grad is None, "the reference differentiates the cone weights after all"
            grads[name] = [npy(leaves[0].grad).reshape(-1, 3), npy(leaves[1].grad).reshape(-1, 3)]
            if name == "32":
                outs = {k: npy(o[k]) for k in ups}
        n = rays * samples
        dev_pt = np.zeros(n)
        for i in range(2):
            dev_pt = np.maximum(dev_pt, np.abs(grads["32"][i].astype(np.float64) - grads["64"][i]).max(1) / np.abs(grads["64"][i]).max())
        kink = dev_pt > KINK_GATE
        assert kink.sum() * KINK_CAP <= n, ("%s: %d of %d points marked as kinks: change the sampling seed" % (case, kink.sum(), n))
        pre = case + "_"
        sums, sha = synth.input_digest(pos, dd, var, ups)
        arrs.update({pre + "config": np.array(json.dumps(kw)), pre + "kind": np.array(kind), pre + "state_seed": np.int32(state_seed),
                     pre + "iteration": np.int32(iteration), pre + "kink": np.packbits(kink), pre + "digest_sums": sums,
                     pre + "digest_sha256": np.array(sha)})
        stride = ROUTES_OUT_STRIDE.get(case, 1)
        arrs[pre + "out_stride"] = np.int32(stride)
        for k in ups:
            arrs[pre + "out_" + k] = outs[k].reshape((n,) + outs[k].shape[2:])[::stride]
        for i, what in enumerate(("pos", "dir")):
            arrs[pre + "grad64_" + what] = grads["64"][i].astype(np.float32)
            dn, de = _deviation(grads["32"][i][~kink], grads["64"][i][~kink])
            arrs[pre + "ref32_norm_" + what], arrs[pre + "ref32_entry_" + what] = np.float64(dn), np.float64(de)
            print("  %s d/d%s: reference fp32 vs fp64 norm %.2e entry %.2e (%d of %d points marked)" % (case, what, dn, de, kink.sum(), n), flush=True)
    save("pose_grad_routes.npz", **arrs)
    size = os.path.getsize(os.path.join(HERE, "pose_grad_routes.npz"))
    assert size < ROUTES_MAX_BYTES, "pose_grad_routes.npz is %d bytes: above the size limit of a committed file" % size


if __name__ == "__main__":
    arrs = {}
    if len(sys.argv) > 1 and sys.argv[1] == "routes":       # the route fixture alone
        gen_routes()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "refine":       # the slow part alone, merged into the existing fixture
        arrs = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "pose_grad.npz")))
        if not os.path.exists(os.path.join(POSE_VIEW_DIR, "test", "r_0.png")):
            gen_pose_view()
        gen_refine(arrs)
        save("pose_grad.npz", **arrs)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "step":         # the step-level records alone, merged likewise
        arrs = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "pose_grad.npz")))
        gen_step(arrs)
        save("pose_grad.npz", **arrs)
        sys.exit(0)
    gen_field(arrs)
    gen_field_nerf(arrs)
    gen_stage(arrs)
    gen_step(arrs)
    gen_pose_view()
    gen_refine(arrs)
    save("pose_grad.npz", **arrs)
    gen_routes()
