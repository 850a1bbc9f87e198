"""Ray bundles, host side: the header's NEDDF_UV_RAYS against the binding, the orthographic calib against a numpy fp32 restatement, the
optional uv of Ray, and the draw order of the trainer's mixed-view step.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_constant_matches_the_binding():
    from neddf_amd import _lib
    header = open(os.path.join(ROOT, "include", "neddf_hip.h")).read()
    enum = re.search(r"enum\s*\{\s*NEDDF_UV_F32[^}]*\}", header, re.S).group(0)
    enum = re.sub(r"/\*.*?\*/", "", enum, flags=re.S)
    values = {k: int(v) for k, v in re.findall(r"(NEDDF_UV_\w+)\s*=\s*(\d+)", enum)}
    assert values == {"NEDDF_UV_F32": 0, "NEDDF_UV_I64": 1, "NEDDF_UV_I32": 2, "NEDDF_UV_I16": 3, "NEDDF_UV_RAYS": 4}
    assert _lib.UV_RAYS == values["NEDDF_UV_RAYS"]
    assert _lib.UV_TYPES == {torch.float32: 0, torch.int64: 1, torch.int32: 2, torch.int16: 3}       # a bundle is never keyed by dtype
    assert _lib.UV_RAYS not in _lib.UV_TYPES.values()


def test_orthographic_calib_round_trip_and_restatement():
    from neddf_amd.camera import Camera, OrthographicCalib
    w, h = 64, 48
    params = np.array([40.0, 24.0, 31.25, 23.5], np.float32)          # sx, sy, cx, cy: (u - cx) / sx need not be exact
    calib = OrthographicCalib(params)
    cam = Camera(calib, np.array([0.3, -0.2, 0.5, 1.0, -2.0, 3.0], np.float32))
    pix = torch.stack(torch.meshgrid(torch.arange(w), torch.arange(h), indexing="xy"), -1).reshape(-1, 2)
    centre = cam.get_center_of_pixels(pix)
    with torch.no_grad():
        o = calib.unproject_local_origin(centre)
        d = calib.unproject_local(centre)
        back = calib.project_local(o)
        rays = cam.create_rays(pix)
    # the numpy fp32 restatement
    f = np.float32
    c = (f(0.5) + f(1.0) * pix.numpy().astype(f)).astype(f)
    x, y = (c[:, 0] - params[2]) / params[0], (c[:, 1] - params[3]) / params[1]
    want_o = np.stack([x, -y, np.zeros_like(x)], 1).astype(f)
    assert o.dtype == torch.float32 and np.array_equal(o.numpy().view(np.uint32), want_o.view(np.uint32))
    assert np.array_equal(d.numpy(), np.tile(np.array([0.0, 0.0, -1.0], f), (w * h, 1)))
    want_back = np.stack([want_o[:, 0] * params[0] + params[2], (-want_o[:, 1]) * params[1] + params[3]], 1).astype(f)
    assert np.array_equal(back.numpy().view(np.uint32), want_back.view(np.uint32))
    R, T = cam.R.detach().numpy(), cam.T.detach().numpy()

    def rotate(v):
        return (v[:, 0:1] * R[None, :, 0] + v[:, 1:2] * R[None, :, 1] + v[:, 2:3] * R[None, :, 2]).astype(f)
    assert np.array_equal(rays.ray_dir.numpy().view(np.uint32), rotate(d.numpy()).view(np.uint32))
    assert np.array_equal(rays.ray_orig.numpy().view(np.uint32), (rotate(want_o) + T[None, :]).astype(f).view(np.uint32))
    assert rays.ray_dir.dtype == torch.float32 and torch.equal(rays.uv, pix)
    # exact round trip on an integer pixel grid: a power-of-two scale and a half-integer principal point lose nothing
    exact = OrthographicCalib(np.array([32.0, 16.0, w / 2.0, h / 2.0], np.float32))
    with torch.no_grad():
        assert torch.equal(exact.project_local(exact.unproject_local_origin(centre)), centre)
        assert float((back - centre).abs().max()) < 1e-5
    with pytest.raises(NotImplementedError):
        cam.descriptor()


def test_ray_without_uv():
    from neddf_amd import Ray
    rd, ro = torch.zeros(5, 3), torch.ones(5, 3)
    rays = Ray(rd, ro)
    assert rays.uv is None and len(rays) == 5 and not rays.single and rays[2][1].tolist() == [1.0, 1.0, 1.0]
    assert Ray(rd, ro, uv=None).uv is None and Ray(rd[0], ro[0]).single
    assert Ray(rd, ro, torch.zeros(5, 2)).uv.shape == (5, 2)
    with pytest.raises(AssertionError):
        Ray(rd, ro, torch.zeros(4, 2))
    with pytest.raises(AssertionError):
        Ray(rd, ro[:4])


def test_bundles_are_named_not_guessed():
    """The binding types a [n, 6] float tensor as pixels unless told otherwise, and both routes refuse host tensors before any library call."""
    from neddf_amd import Ray
    from neddf_amd._lib import NeddfError, _uv_arg
    with pytest.raises(NeddfError, match="HIP device"):
        _uv_arg(torch.zeros(3, 6), bundle=True)
    with pytest.raises(NeddfError, match="HIP device"):
        _uv_arg(Ray(torch.zeros(3, 3), torch.zeros(3, 3)))
    with pytest.raises(NeddfError, match="HIP device"):
        _uv_arg(torch.zeros(3, 6))


class _Views:
    """Stands in for a dataset: `sizes` (h, w) per view."""

    def __init__(self, sizes):
        self.items = [{"rgb_images": np.zeros((h, w, 3), np.uint8)} for h, w in sizes]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


@pytest.mark.parametrize("sizes", [[(16, 20)] * 3, [(16, 20), (13, 17), (40, 31), (16, 20), (9, 200)]])
def test_mixed_step_draw_order(sizes):
    """view, then u, then v on the CPU generator, u and v scaled by the ray's own view's (w - 1) and (h - 1)."""
    from neddf_amd.trainer import NeRFTrainer
    tr = NeRFTrainer.__new__(NeRFTrainer)          # the draws need the dataset and the batch size only
    tr.dataset, tr.batch_size, tr._view_sizes = _Views(sizes), 257, None
    torch.manual_seed(21)
    view, us, vs = tr.draw_mixed_batch()
    after = torch.rand(3)
    torch.manual_seed(21)
    n = len(sizes)
    want_view = (torch.rand(257) * n).to(torch.int64)
    w1 = torch.tensor([w - 1 for h, w in sizes], dtype=torch.float32)[want_view]
    h1 = torch.tensor([h - 1 for h, w in sizes], dtype=torch.float32)[want_view]
    want_us = (torch.rand(257) * w1).to(torch.int16)
    want_vs = (torch.rand(257) * h1).to(torch.int16)
    assert view.dtype == torch.int64 and us.dtype == torch.int16 and vs.dtype == torch.int16
    assert torch.equal(view, want_view) and torch.equal(us, want_us) and torch.equal(vs, want_vs)
    assert torch.equal(after, torch.rand(3))                            # nothing else was drawn
    assert set(view.tolist()) == set(range(n))
    for k, (h, w) in enumerate(sizes):
        rows = view == k
        assert int(us[rows].max()) <= w - 1 and int(vs[rows].max()) <= h - 1 and int(us[rows].min()) >= 0
    if len(set(sizes)) == 1:        # one size: the single-view step's own expression, (w - 1) as a Python number
        torch.manual_seed(21)
        torch.rand(257)
        assert torch.equal(us, (torch.rand(257) * (sizes[0][1] - 1)).to(torch.int16))


def test_batch_views_keyword():
    from neddf_amd.trainer import NeRFTrainer
    with pytest.raises(ValueError, match="batch_views"):
        NeRFTrainer(batch_views="all", global_config={})
    import inspect
    assert inspect.signature(NeRFTrainer.__init__).parameters["batch_views"].default == "single"


def test_script_options():
    from neddf_amd.scripts import render_mesh, run_eval
    assert render_mesh.build_parser().parse_args(["run", "--ortho", "40"]).ortho == 40.0
    assert run_eval.build_parser().parse_args(["run"]).ortho is None
    assert run_eval.build_parser().parse_args(["run", "--ortho", "12.5"]).ortho == 12.5
