"""Pinhole camera with an SE(3) pose -- host-side mirror of neddf/camera/.

Pose algebra (camera.py:66-118) stays on the host: it is a handful of 3x3
products per view.  Pixel -> ray (camera.py:155-187, pinhole_calib.py:51-74)
runs in the raygen HIP kernel.

Any other camera model is a calib class with `unproject_local` (and, where its
rays do not start at the camera centre, `unproject_local_origin`): Camera.create_rays
then builds the rays in torch and the renderer takes them as a ray bundle
(NeRFRender.render_bundle).  OrthographicCalib is the one shipped.
"""
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from numpy import ndarray
from scipy.spatial.transform import Rotation
from torch import Tensor, nn

from ._lib import CameraDesc, Context
from .ray import Ray


class BaseCameraCalib(nn.Module):
    def __init__(self, calib_param: ndarray) -> None:
        super().__init__()
        self.params = nn.Parameter(torch.from_numpy(np.asarray(calib_param)).to(torch.float32))

    @property
    def device(self) -> torch.device:
        return self.params.device

    def unproject_local_origin(self, uv: Tensor) -> Tensor:
        """pixels -> where each pixel's ray starts in the camera frame, [B,3]: the camera centre unless a model says otherwise."""
        return torch.zeros(uv.shape[0], 3, dtype=torch.float32, device=uv.device)


class PinholeCalib(BaseCameraCalib):
    """Intrinsics [fx, fy, cx, cy] (pinhole_calib.py:8)."""

    def __init__(self, calib_param: ndarray) -> None:
        assert np.asarray(calib_param).shape == (4,)
        super().__init__(calib_param)

    fx = property(lambda self: self.params[0])
    fy = property(lambda self: self.params[1])
    cx = property(lambda self: self.params[2])
    cy = property(lambda self: self.params[3])

    def project_local(self, xyz: Tensor) -> Tensor:
        """camera-frame (right-up-back) points -> pixels (pinhole_calib.py:26-49)."""
        zi = torch.reciprocal(-xyz[:, 2])
        return torch.stack([self.fx * xyz[:, 0] * zi + self.cx, self.fy * (-xyz[:, 1]) * zi + self.cy], 1)

    def unproject_local(self, uv: Tensor) -> Tensor:
        """pixels -> unit camera-frame directions (pinhole_calib.py:51-74)."""
        x = (1.0 / self.fx) * (uv[:, 0] - self.cx)
        y = (1.0 / self.fy) * (uv[:, 1] - self.cy)
        v = torch.stack([x, -y, -torch.ones_like(x)], 1)
        return nn.functional.normalize(v, p=2, dim=1)


class OrthographicCalib(BaseCameraCalib):
    """Parallel projection [sx, sy, cx, cy] (not a reference model): sx, sy pixels per world unit, (cx, cy) the principal point.
    Every pixel looks along the camera's -z axis (right-up-back frame) from ((u - cx) / sx, -(v - cy) / sy, 0): exact, no
    iteration -- the inspection view of a mesh or field viewer."""

    def __init__(self, calib_param: ndarray) -> None:
        assert np.asarray(calib_param).shape == (4,)
        super().__init__(calib_param)

    sx = property(lambda self: self.params[0])
    sy = property(lambda self: self.params[1])
    cx = property(lambda self: self.params[2])
    cy = property(lambda self: self.params[3])

    def project_local(self, xyz: Tensor) -> Tensor:
        """camera-frame points -> pixels: the inverse of unproject_local_origin, whatever the depth."""
        return torch.stack([xyz[:, 0] * self.sx + self.cx, (-xyz[:, 1]) * self.sy + self.cy], 1)

    def unproject_local(self, uv: Tensor) -> Tensor:
        """pixels -> unit camera-frame directions: (0, 0, -1) for every pixel."""
        d = torch.zeros(uv.shape[0], 3, dtype=torch.float32, device=uv.device)
        d[:, 2] = -1.0
        return d

    def unproject_local_origin(self, uv: Tensor) -> Tensor:
        x = (uv[:, 0] - self.cx) / self.sx
        y = (uv[:, 1] - self.cy) / self.sy
        return torch.stack([x, -y, torch.zeros_like(x)], 1)


def _hat(v: Tensor) -> Tensor:
    z = torch.zeros((), dtype=v.dtype, device=v.device)
    return torch.stack([torch.stack([z, -v[2], v[1]]), torch.stack([v[2], z, -v[0]]), torch.stack([-v[1], v[0], z])])


class Camera(nn.Module):
    """camera.py:13-64.  `params` (6, zero-initialised) perturbs the initial pose."""

    def __init__(self, camera_calib: BaseCameraCalib, initial_camera_param: Optional[ndarray] = None) -> None:
        super().__init__()
        if initial_camera_param is None:
            initial_camera_param = np.zeros(6, dtype=np.float32)
        self.camera_calib = camera_calib
        self.initial_params_np = np.asarray(initial_camera_param)
        self.params = nn.Parameter(torch.zeros(6, dtype=torch.float32))
        self.R = torch.eye(3, dtype=torch.float32)
        self.T = torch.zeros(3, dtype=torch.float32)
        self.update_transform()

    @property
    def device(self) -> torch.device:
        return self.params.device

    @property
    def R0(self) -> Tensor:
        m = Rotation.from_rotvec(self.initial_params_np[:3]).as_matrix().astype(np.float32)
        return torch.from_numpy(m).to(self.device)

    @property
    def T0(self) -> Tensor:
        return torch.from_numpy(self.initial_params_np[3:6].astype(np.float32)).to(self.device)

    def update_transform(self) -> None:
        """[R|T] = exp(params) composed with the initial pose (Rodrigues; camera.py:66-118)."""
        eye = torch.eye(3, dtype=torch.float32, device=self.device)
        rot, trans = self.params[0:3], self.params[3:6]
        theta = torch.norm(rot)
        if theta > 1e-10:
            ti = 1.0 / theta
            w = _hat(ti * rot)
            ww = torch.matmul(w, w)
            c, s = torch.cos(theta), torch.sin(theta)
            Ri = eye + s * w + (1.0 - c) * ww
            Vi = eye + (1 - c) * ti * ti * w + (theta - s) * ti * ti * ti * ww
        else:
            Ri = eye + _hat(rot)
            Vi = Ri
        self.R = torch.matmul(Ri, self.R0)
        self.T = (torch.matmul(Vi, trans[:, None]) + torch.matmul(Ri, self.T0[:, None]))[:, 0]

    def project(self, pos_world: Tensor) -> Tensor:
        pc = torch.matmul(self.R.T, (pos_world[:, :, None] - self.T[None, :, None]))[:, :, 0]
        return self.camera_calib.project_local(pc)

    def unproject(self, uv: Tensor) -> Tensor:
        return torch.matmul(self.R, self.camera_calib.unproject_local(uv).T).T + self.T[None, :]

    def get_center_of_pixels(self, pixel_id: Tensor, scale: float = 1.0) -> Tensor:
        return 0.5 + scale * pixel_id.to(torch.float32)

    def descriptor(self) -> CameraDesc:
        """POD copy of (R, T, intrinsics) for the C ABI: a pinhole camera's.  Any other calib raises -- its rays are made by
        create_rays in torch and reach the library as a bundle."""
        if not isinstance(self.camera_calib, PinholeCalib):
            raise NotImplementedError("Camera.descriptor: the C ABI's camera is a pinhole; a %s makes its rays in create_rays"
                                      % type(self.camera_calib).__name__)
        d = CameraDesc()
        d.R[:] = self.R.detach().reshape(-1).tolist()
        d.T[:] = self.T.detach().tolist()
        d.calib[:] = self.camera_calib.params.detach().tolist()
        return d

    def create_rays(self, uv: Tensor) -> Ray:
        """Pixel indices [B,2] (int64/int32/int16/float) -> rays (camera.py:155-171).  A PinholeCalib goes through the raygen
        kernel; any other calib through its unproject_local / unproject_local_origin at the pixel centres, then R and T, in fp32
        torch ops (differentiable with respect to R and T)."""
        uv = uv.to(self.device)
        if not isinstance(self.camera_calib, PinholeCalib):
            centre = self.get_center_of_pixels(uv)
            d_local = self.camera_calib.unproject_local(centre).to(torch.float32)
            o_local = self.camera_calib.unproject_local_origin(centre).to(torch.float32)
            R, T = self.R.to(torch.float32), self.T.to(torch.float32)

            def rotate(x: Tensor) -> Tensor:        # R x per row, summed left to right as the raygen kernel does (no BLAS call)
                return x[:, 0:1] * R[None, :, 0] + x[:, 1:2] * R[None, :, 1] + x[:, 2:3] * R[None, :, 2]
            return Ray(rotate(d_local), rotate(o_local) + T[None, :], uv)
        ctx = Context.get(self.device)
        rd, ro = ctx.raygen(uv, self.descriptor())
        return Ray(rd, ro, uv)


def _hat_rows(v: Tensor) -> Tensor:
    """_hat of every row: [K,3] -> [K,3,3]."""
    z = torch.zeros_like(v[:, 0])
    return torch.stack([torch.stack([z, -v[:, 2], v[:, 1]], 1), torch.stack([v[:, 2], z, -v[:, 0]], 1),
                        torch.stack([-v[:, 1], v[:, 0], z], 1)], 1)


def compose_poses(params: Tensor, R0: Tensor, T0: Tensor) -> Tuple[Tensor, Tensor]:
    """Camera.update_transform for K cameras at once, differentiable with respect to `params`: params [K,6], R0 [K,3,3],
    T0 [K,3] -> (R [K,3,3], T [K,3]).  The formula is update_transform's, term for term (its (1 - c) * ti * ti coefficient of
    the translation map included, as the reference has it), and so is the choice between Rodrigues' form and the first-order
    one at |rot| <= 1e-10.  Every camera starts at params == 0, so the unselected Rodrigues branch must stay finite there in the
    BACKWARD too: its rows get a fixed unit axis in place of the zero vector before the norm and the reciprocal are taken (a
    torch.where over 1 / theta alone would send 0 * inf = NaN into the gradient).  At a zero rotation the result carries
    update_transform's bits (products with 0 and 1 are exact); elsewhere the two agree to rounding, not bit for bit."""
    if params.dim() != 2 or params.shape[1] != 6 or R0.shape != (params.shape[0], 3, 3) or T0.shape != (params.shape[0], 3):
        raise ValueError("compose_poses: params [K, 6], R0 [K, 3, 3] and T0 [K, 3] expected")
    eye = torch.eye(3, dtype=params.dtype, device=params.device)[None]
    rot, trans = params[:, 0:3], params[:, 3:6]
    small = ~(torch.norm(rot.detach(), dim=1) > 1e-10)
    axis = torch.zeros_like(rot)
    axis[:, 0] = 1.0
    safe = torch.where(small[:, None], axis, rot)
    theta = torch.norm(safe, dim=1)
    ti = 1.0 / theta
    w = _hat_rows(ti[:, None] * safe)
    ww = torch.matmul(w, w)
    c, s = torch.cos(theta), torch.sin(theta)

    def col(x: Tensor) -> Tensor:
        return x[:, None, None]
    Ri_big = eye + col(s) * w + col(1.0 - c) * ww
    Vi_big = eye + col((1 - c) * ti * ti) * w + col((theta - s) * ti * ti * ti) * ww
    Ri_small = eye + _hat_rows(rot)
    Ri = torch.where(col(small), Ri_small, Ri_big)
    Vi = torch.where(col(small), Ri_small, Vi_big)
    R = torch.matmul(Ri, R0)
    T = (torch.matmul(Vi, trans[:, :, None]) + torch.matmul(Ri, T0[:, :, None]))[:, :, 0]
    return R, T


class CameraSet:
    """The cameras of a training set as one device-resident table: [K,16] rows of (R row-major, T, calib), what
    NeRFRender.render_rays_views and the library's per-row-camera ray generation read.  The initial poses (one scipy call per
    camera) and the intrinsics are stacked once; a table is then one batched pose composition (compose_poses) whatever K is.
    Every camera must be a pinhole; the cameras' own R / T attributes are not touched (Camera.update_transform still owns them)."""

    def __init__(self, cameras: Sequence[Camera]) -> None:
        self.cameras: List[Camera] = list(cameras)
        if not self.cameras:
            raise ValueError("CameraSet: no cameras")
        for camera in self.cameras:
            if not isinstance(camera.camera_calib, PinholeCalib):
                raise NotImplementedError("CameraSet: the camera table holds pinhole cameras; a %s makes its rays in create_rays"
                                          % type(camera.camera_calib).__name__)
        self.device = self.cameras[0].device
        initial = np.stack([np.asarray(c.initial_params_np, dtype=np.float64).reshape(6) for c in self.cameras])
        # (the same scipy call and fp32 rounding as Camera.R0 / Camera.T0, once)
        self.R0 = torch.from_numpy(Rotation.from_rotvec(initial[:, :3]).as_matrix().astype(np.float32)).to(self.device)
        self.T0 = torch.from_numpy(np.stack([np.asarray(c.initial_params_np)[3:6].astype(np.float32) for c in self.cameras])).to(self.device)
        self._cached: Optional[Tensor] = None
        self._key: Optional[tuple] = None
        self.rebuilds = 0               # how often the cached table was composed (the cache's own test reads it)

    def __len__(self) -> int:
        return len(self.cameras)

    def _state(self) -> tuple:
        return tuple(c.params._version for c in self.cameras) + tuple(c.camera_calib.params._version for c in self.cameras)

    def _calib(self, indices: Optional[Sequence[int]]) -> Tensor:
        cams = self.cameras if indices is None else [self.cameras[i] for i in indices]
        first = cams[0].camera_calib
        if all(c.camera_calib is first for c in cams):      # one calib shared by every view, as the trainer builds them
            return first.params.detach().to(torch.float32)[None, :].expand(len(cams), 4)
        return torch.stack([c.camera_calib.params.detach().to(torch.float32) for c in cams])

    def table(self, indices: Optional[Sequence[int]] = None, grad: bool = False) -> Tensor:
        """[K,16] rows of the cameras `indices` (all of them: None), at their current `params`.  grad=False: no graph; the table
        of all cameras is cached and composed again only after a camera's (or a calib's) parameters changed in place.  grad=True:
        composed from torch.stack of the selected cameras' `params`, so each of them receives its own gradient through the table
        and a camera that was not selected receives none."""
        if indices is not None:
            indices = [int(i) for i in indices]
            for i in indices:
                if not 0 <= i < len(self.cameras):
                    raise ValueError("CameraSet: camera index %d outside [0, %d)" % (i, len(self.cameras)))
            if not indices:
                raise ValueError("CameraSet: an empty selection has no table")
        if not grad:
            key = self._state()
            if self._cached is None or key != self._key:
                with torch.no_grad():
                    self._cached = self._compose(None)
                self._key = key
                self.rebuilds += 1
            return self._cached if indices is None else self._cached[torch.as_tensor(indices, device=self.device)]
        return self._compose(indices)

    def _compose(self, indices: Optional[Sequence[int]]) -> Tensor:
        cams = self.cameras if indices is None else [self.cameras[i] for i in indices]
        params = torch.stack([c.params for c in cams])
        if indices is None:
            R0, T0 = self.R0, self.T0
        else:
            at = torch.as_tensor(indices, device=self.device)
            R0, T0 = self.R0[at], self.T0[at]
        R, T = compose_poses(params, R0, T0)
        return torch.cat([R.reshape(-1, 9), T, self._calib(indices)], 1)

    def select(self, view: Tensor) -> Tuple[List[int], Tensor]:
        """A HOST view draw [B] -> (the cameras it visits, ascending; the draw renumbered to positions in that list, int32):
        what table(visited, grad=True) and its rays need.  No device is read.  An index outside the set raises ValueError."""
        self.check_view(view)
        visited, local = torch.unique(view.to(torch.int64), sorted=True, return_inverse=True)
        return visited.tolist(), local.to(torch.int32)

    def check_view(self, view: Tensor) -> None:
        """ValueError unless every entry of the HOST view draw names a camera of the set."""
        if view.device.type != "cpu":
            raise ValueError("CameraSet: the view draw is validated on the host (got a %s tensor)" % view.device.type)
        if view.numel() and (int(view.min()) < 0 or int(view.max()) >= len(self.cameras)):
            raise ValueError("CameraSet: view must lie in [0, %d)" % len(self.cameras))

