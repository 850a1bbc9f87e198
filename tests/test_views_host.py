"""Per-row cameras, host side: compose_poses (the batched Camera.update_transform) against an fp64 numpy restatement and against
the per-camera autograd, the header's NEDDF_UV_CAMERA_TABLE and neddf_camera_table against the binding, the CameraSet cache and its
host-side view validation.  No GPU.

Gates.  Poses: the yardstick is the existing route, not a constant -- (theta - sin theta) / theta^3 cancels in fp32, so
update_transform itself is off by about 5e-5 at small angles.  compose_poses may be off by at most twice update_transform's largest
error on the same poses, plus 2^-23 max(1, |entry|) (one rounding of the entry).  At a zero rotation both routes multiply by 0 and 1
only, which is exact: there they agree bit for bit.  Gradients: finite everywhere, and tests/test_gpu_pose.py `check`'s gates (norm
and entries within 1e-4) against Camera.update_transform's own autograd."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from neddf_amd.camera import Camera, CameraSet, PinholeCalib, compose_poses      # (the parent commit has neither: ImportError)
from test_gpu_pose import check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = (0.0, 1e-12, 1e-6, 1e-3, 0.05, 1.0, 3.0)
N_POSES = 400


def _hat64(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def pose64(params, R0, T0):
    """Camera.update_transform in fp64 numpy, term for term (fp32 inputs taken as they are)."""
    params, R0, T0 = (np.asarray(a, np.float64) for a in (params, R0, T0))
    eye = np.eye(3)
    rot, trans = params[:3], params[3:]
    theta = np.linalg.norm(rot)
    if theta > 1e-10:
        ti = 1.0 / theta
        w = _hat64(ti * rot)
        ww = w @ w
        c, s = np.cos(theta), np.sin(theta)
        Ri = eye + s * w + (1.0 - c) * ww
        Vi = eye + (1 - c) * ti * ti * w + (theta - s) * ti * ti * ti * ww
    else:
        Ri = eye + _hat64(rot)
        Vi = Ri
    return Ri @ R0, Vi @ trans + Ri @ T0


def _poses(n=N_POSES, seed=31):
    """n cameras with random initial poses; params of pose i are normal draws times SCALES[i % 7].  Rows 7 and 14 keep a zero rotation
    with a non-zero translation."""
    rng = np.random.default_rng(seed)
    calib = PinholeCalib(np.array([28.0, 30.0, 10.0, 8.0]))
    cams = []
    for i in range(n):
        initial = np.concatenate([rng.standard_normal(3), 2.0 * rng.standard_normal(3)]).astype(np.float32)
        cam = Camera(calib, initial)
        p = (rng.standard_normal(6) * SCALES[i % len(SCALES)]).astype(np.float32)
        if i in (7, 14):
            p = np.concatenate([np.zeros(3), rng.standard_normal(3)]).astype(np.float32)
        cam.params.data.copy_(torch.from_numpy(p))
        cams.append(cam)
    return cams


@pytest.fixture(scope="module")
def poses():
    cams = _poses()
    with torch.no_grad():
        for cam in cams:
            cam.update_transform()
    return cams


def test_compose_poses_against_the_fp64_restatement(poses):
    params = torch.stack([c.params.detach() for c in poses])
    R0, T0 = torch.stack([c.R0 for c in poses]), torch.stack([c.T0 for c in poses])
    with torch.no_grad():
        R, T = compose_poses(params, R0, T0)
    assert R.shape == (N_POSES, 3, 3) and T.shape == (N_POSES, 3) and R.dtype == torch.float32
    got = np.concatenate([R.numpy().reshape(N_POSES, 9), T.numpy()], 1)
    old = np.stack([np.concatenate([c.R.numpy().reshape(9), c.T.numpy()]) for c in poses])
    ref = np.stack([np.concatenate([a.reshape(9), b]) for a, b in (pose64(params[i].numpy(), R0[i].numpy(), T0[i].numpy()) for i in range(N_POSES))])
    err_old = np.abs(old.astype(np.float64) - ref).max()
    err_new = np.abs(got.astype(np.float64) - ref)
    print("largest error against fp64: update_transform %.3e, compose_poses %.3e (ratio %.3f)" % (err_old, err_new.max(), err_new.max() / err_old))
    assert err_old > 0
    gate = 2.0 * err_old + 2.0 ** -23 * np.maximum(1.0, np.abs(ref))
    assert (err_new <= gate).all(), (err_new.max(), err_old)
    # a zero rotation: products with 0 and 1 only, the same bits -- params == 0 and the two translation-only rows
    exact = [i for i in range(N_POSES) if not params[i, :3].any()]
    assert {0, 7, 14} <= set(exact) and any(params[i, 3:].any() for i in exact)
    assert np.array_equal(got[exact].view(np.uint32), old[exact].view(np.uint32))
    # elsewhere the two routes agree to rounding, not bit for bit: the gate above is not vacuous
    assert not np.array_equal(got.view(np.uint32), old.view(np.uint32))
    with pytest.raises(ValueError):
        compose_poses(params[:, :5], R0, T0)


def test_compose_poses_gradients_against_the_per_camera_autograd():
    cams = _poses(n=21, seed=32)            # three rounds of SCALES: params == 0 at 0, 7 -> translation only, 14 likewise
    cams[0].params.data.zero_()
    rng = np.random.default_rng(33)
    A = torch.from_numpy(rng.standard_normal((21, 3, 3)).astype(np.float32))
    b = torch.from_numpy(rng.standard_normal((21, 3)).astype(np.float32))
    want = []
    for i, cam in enumerate(cams):
        cam.update_transform()
        ((A[i] * cam.R).sum() + (b[i] * cam.T).sum()).backward()
        want.append(cam.params.grad.clone())
    want = torch.stack(want)
    leaf = torch.stack([c.params.detach() for c in cams]).requires_grad_(True)
    R, T = compose_poses(leaf, torch.stack([c.R0 for c in cams]), torch.stack([c.T0 for c in cams]))
    ((A * R).sum() + (b * T).sum()).backward()
    assert bool(torch.isfinite(leaf.grad).all()) and bool(torch.isfinite(want).all())
    assert not leaf[0].any() and not leaf[7, :3].any() and leaf[7, 3:].any()
    for i in range(21):
        check("pose %d (scale %g) d/dparams" % (i, SCALES[i % len(SCALES)]), leaf.grad[i].numpy(), want[i].numpy())
    check("all poses d/dparams", leaf.grad.numpy(), want.numpy())


def test_constants_match_the_header():
    from neddf_amd import _lib
    header = open(os.path.join(ROOT, "include", "neddf_hip.h")).read()
    value = re.search(r"enum\s*\{\s*NEDDF_UV_CAMERA_TABLE\s*=\s*(0x[0-9a-fA-F]+|\d+)\s*\}", header).group(1)
    assert _lib.UV_CAMERA_TABLE == int(value, 0) == 0x100
    assert all(code & _lib.UV_CAMERA_TABLE == 0 for code in list(_lib.UV_TYPES.values()) + [_lib.UV_RAYS])
    struct = re.search(r"typedef struct \{([^}]*)\}\s*neddf_camera_table;", header).group(1)
    struct = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    fields = re.findall(r"(\w+)\s*;", struct)
    assert fields == ["d_cameras", "d_view", "n_cameras"] == [f[0] for f in _lib.CameraTableDesc._fields_]
    assert C.sizeof(_lib.CameraTableDesc) == 24
    assert [getattr(_lib.CameraTableDesc, f).offset for f in fields] == [0, 8, 16]
    assert C.sizeof(_lib.CameraDesc) == 64          # one table row: 16 floats
    assert _lib.ViewRays._fields == ("uv", "view", "table")
    with pytest.raises(_lib.NeddfError, match="HIP device"):       # host tensors are refused before any library call
        _lib._uv_arg(_lib.ViewRays(torch.zeros(3, 2), torch.zeros(3, dtype=torch.int32), torch.zeros(1, 16)))


def test_camera_set_table_and_cache():
    cams = _poses(n=6, seed=34)
    cams[3].camera_calib = PinholeCalib(np.array([40.0, 41.0, 9.0, 7.5]))      # intrinsics are per row
    for cam in cams:
        cam.update_transform()
    cs = CameraSet(cams)
    assert len(cs) == 6 and cs.rebuilds == 0
    table = cs.table()
    assert table.shape == (6, 16) and table.dtype == torch.float32 and not table.requires_grad and cs.rebuilds == 1
    for i, cam in enumerate(cams):
        assert torch.equal(table[i, 12:], cam.camera_calib.params.detach())
        np.testing.assert_allclose(table[i, :9].numpy(), cam.R.detach().numpy().reshape(9), atol=1e-4)
        np.testing.assert_allclose(table[i, 9:12].numpy(), cam.T.detach().numpy(), atol=1e-4)
    # the initial poses are the cameras' own, bit for bit (the one scipy call)
    assert torch.equal(cs.R0, torch.stack([c.R0 for c in cams])) and torch.equal(cs.T0, torch.stack([c.T0 for c in cams]))
    assert cs.table() is table and cs.rebuilds == 1                    # nothing changed: the cached tensor
    assert torch.equal(cs.table([4, 1]), table[[4, 1]]) and cs.rebuilds == 1
    with torch.no_grad():
        cams[2].params.add_(0.01)                                      # an in-place change, as an optimiser step makes it
    again = cs.table()
    assert cs.rebuilds == 2 and not torch.equal(again[2], table[2])
    assert torch.equal(again[[0, 1, 3, 4, 5]], table[[0, 1, 3, 4, 5]])
    assert cs.table() is again and cs.rebuilds == 2
    # grad=True: the selected cameras' own Parameters receive the gradient, the others none; nothing is cached
    t = cs.table([5, 2], grad=True)
    assert t.requires_grad and t.shape == (2, 16) and cs.rebuilds == 2
    assert torch.equal(t.detach(), again[[5, 2]])
    t[:, :12].sum().backward()
    assert [c.params.grad is not None for c in cams] == [False, False, True, False, False, True]
    assert all(bool(torch.isfinite(c.params.grad).all()) and bool(c.params.grad.any()) for c in (cams[2], cams[5]))
    assert cams[0].camera_calib.params.grad is None                    # the intrinsics are not differentiated
    with pytest.raises(ValueError):
        cs.table([6])
    with pytest.raises(ValueError):
        cs.table([])
    with pytest.raises(ValueError):
        CameraSet([])


def test_camera_set_validates_the_host_view():
    cs = CameraSet(_poses(n=5, seed=35))
    view = torch.tensor([4, 1, 1, 4, 3], dtype=torch.int64)
    cs.check_view(view)
    visited, local = cs.select(view)
    assert visited == [1, 3, 4] and local.dtype == torch.int32 and local.tolist() == [2, 0, 0, 2, 1]
    for bad in ([0, 5], [-1, 2], [2 ** 31 - 1]):
        with pytest.raises(ValueError):
            cs.check_view(torch.tensor(bad, dtype=torch.int64))
        with pytest.raises(ValueError):
            cs.select(torch.tensor(bad, dtype=torch.int64))
    cs.check_view(torch.zeros(0, dtype=torch.int64))


def test_pinhole_cameras_only():
    from neddf_amd.camera import OrthographicCalib
    cam = Camera(OrthographicCalib(np.array([40.0, 40.0, 10.0, 8.0], np.float32)), None)
    with pytest.raises(NotImplementedError):
        CameraSet([cam])
