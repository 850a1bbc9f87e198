"""ctypes binding of libneddf_hip.so (include/neddf_hip.h).

There is deliberately NO fallback: if the HIP library is missing, or a tensor is
not on a HIP device, the product path raises.  (The CPU oracle under oracle/ is
test infrastructure and is never imported from here.)
"""
import ctypes as C
import os
from typing import NamedTuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# NEDDF_LIB_PATH selects another build of the same library (the sanitizer build, `make -C neddf_amd/csrc asan`)
LIB_PATH = os.environ.get("NEDDF_LIB_PATH") or os.path.join(_HERE, "csrc", "libneddf_hip.so")
ABI_VERSION = 7

FIELD_NEDDF, FIELD_NERF, FIELD_NEUS = 0, 1, 2
ACT = {"ReLU": 0, "LeakyReLU": 1, "tanhExp": 2}
DTYPE = {"fp32": 0, "bf16": 1, "f16_split": 2, "f16": 3}       # NEDDF_DTYPE_* (include/neddf_hip.h)
SLOT_COARSE, SLOT_FINE, SLOT_GENERIC = 0, 1, 2
OUT_MINIMAL, OUT_FULL = 0, 1
GRID_FIELDS = {"distance": 0, "density": 1}        # NEDDF_GRID_*
STAGES = ("ddf", "col", "nerf", "raygen", "ndc", "sample_coarse", "sampling", "composite", "penalty", "resample", "gather")
COMM_ID_BYTES = 128
UV_TYPES = {torch.float32: 0, torch.int64: 1, torch.int32: 2, torch.int16: 3}
UV_RAYS = 4         # NEDDF_UV_RAYS: float32 [n, 6] rows of (direction, origin); never inferred from a dtype or a shape
UV_CAMERA_TABLE = 0x100     # NEDDF_UV_CAMERA_TABLE: OR-ed onto a pixel type, a camera per row (ViewRays)
MAX_CAMERAS = 1 << 20
PENALTY_KEYS = ("constraints_aux_grad", "constraints_dDdt", "range_distance", "range_aux_grad",
                "range_color", "constraints_color")     # dict order of neddf.py:260-291

_fp = C.POINTER(C.c_float)
_vp = C.c_void_p
_i64 = C.c_int64
_dp = C.POINTER(C.c_double)


class NeddfError(RuntimeError):
    pass


class ViewRays(NamedTuple):
    """Pixels with a camera per row, in place of (uv, camera): uv [n, 2] pixels, view int32 or int64 [n] the camera of row b,
    table float32 [K, 16] the cameras (R row-major, T, calib: CameraDesc's layout).  Like a Ray it is named by the caller, never
    guessed from shapes.  A row whose view lies outside [0, K) reads no camera and generates NaN rays."""
    uv: torch.Tensor
    view: torch.Tensor
    table: torch.Tensor


def _uv_arg(uv, bundle=False):
    """(contiguous device tensor, NEDDF_UV_* code) of a raygen / render_rays `uv` argument.  Pixels are typed by
    their dtype (UV_TYPES; anything else becomes float32).  A ray bundle is named by the caller, never guessed from a tensor's
    shape: either a Ray (neddf_amd.ray: ray_dir and ray_orig [n, 3], packed here) or, with bundle=True, a float32 [n, 6] tensor
    of (direction, origin) rows.  A ViewRays gives its pixels and their type with UV_CAMERA_TABLE set (_cam_arg takes the rest)."""
    if isinstance(uv, ViewRays):
        if bundle:
            raise NeddfError("a ViewRays holds pixels, not a ray bundle")
        t, code = _uv_arg(uv.uv)
        if t.dim() != 2 or t.shape[1] != 2:
            raise NeddfError("ViewRays: uv must be [n, 2]")
        return t, code | UV_CAMERA_TABLE
    if hasattr(uv, "ray_dir") and hasattr(uv, "ray_orig"):
        rd, ro = uv.ray_dir, uv.ray_orig
        if rd.dim() != 2 or rd.shape[1] != 3 or ro.shape != rd.shape:
            raise NeddfError("a ray bundle needs ray_dir and ray_orig of shape [n, 3]")
        require_device(rd, "ray_dir")
        require_device(ro, "ray_orig")
        return torch.cat([rd.detach().to(torch.float32), ro.detach().to(torch.float32)], 1).contiguous(), UV_RAYS
    require_device(uv, "uv")
    if bundle:
        if uv.dtype != torch.float32 or uv.dim() != 2 or uv.shape[1] != 6:
            raise NeddfError("a ray bundle is a float32 [n, 6] tensor of (direction, origin) rows")
        return uv.contiguous(), UV_RAYS
    if uv.dtype not in UV_TYPES:
        uv = uv.to(torch.float32)
    return uv.contiguous(), UV_TYPES[uv.dtype]


def _cam_arg(cam, uv_type):
    """The h_cam argument: a CameraDesc by reference, or under UV_CAMERA_TABLE the ViewRays itself, whose view and table become a
    CameraTableDesc (the struct keeps the tensors it points to alive)."""
    if uv_type & UV_CAMERA_TABLE:
        if not isinstance(cam, ViewRays):
            raise NeddfError("UV_CAMERA_TABLE needs a ViewRays")
        n = cam.uv.shape[0]
        view, table = cam.view, cam.table
        require_device(view, "view")
        require_device(table, "table")
        if view.dtype not in (torch.int32, torch.int64) or view.dim() != 1 or view.shape[0] != n:
            raise NeddfError("ViewRays: view must be int32 or int64 [n]")
        if table.dtype != torch.float32 or table.dim() != 2 or table.shape[1] != 16 or not 1 <= table.shape[0] <= MAX_CAMERAS:
            raise NeddfError("ViewRays: table must be float32 [K, 16] with 1 <= K <= 2^20")
        if view.device != table.device or view.device != cam.uv.device:
            raise NeddfError("ViewRays: uv, view and table must live on one device")
        if view.dtype == torch.int64:       # every index beyond int32 is invalid anyway: keep it invalid through the narrowing
            view = view.clamp(-1, 2 ** 31 - 1).to(torch.int32)
        view, table = view.contiguous(), table.detach().contiguous()
        desc = CameraTableDesc(table.data_ptr() or None, view.data_ptr() or None, table.shape[0])
        desc._keep = (view, table)
        return C.cast(C.pointer(desc), C.POINTER(CameraDesc))
    if cam is None:
        if uv_type != UV_RAYS:
            raise NeddfError("pixel coordinates need a camera descriptor")
        return None
    return C.byref(cam)


class FieldDesc(C.Structure):
    _fields_ = [("kind", C.c_int), ("embed_pos_rank", C.c_int), ("embed_dir_rank", C.c_int),
                ("layer_count", C.c_int), ("layer_width", C.c_int), ("col_layer_count", C.c_int),
                ("col_layer_width", C.c_int), ("n_skips", C.c_int), ("skips", C.c_int * 8),
                ("activation", C.c_int), ("density_activation", C.c_int), ("d_near", C.c_float),
                ("penalty_weight", C.c_float * 6), ("penalty_has", C.c_int * 6), ("weight_dtype", C.c_int)]


class CameraDesc(C.Structure):
    _fields_ = [("R", C.c_float * 9), ("T", C.c_float * 3), ("calib", C.c_float * 4)]


class CameraTableDesc(C.Structure):
    """neddf_camera_table: a HOST struct naming DEVICE arrays (passed where a CameraDesc goes, under UV_CAMERA_TABLE)."""
    _fields_ = [("d_cameras", _vp), ("d_view", _vp), ("n_cameras", C.c_int32)]


class RenderParams(C.Structure):
    _fields_ = [("sample_coarse", C.c_int), ("sample_fine", C.c_int), ("dist_near", C.c_float),
                ("dist_far", C.c_float), ("max_dist", C.c_float), ("cone_sampling", C.c_int),
                ("ray_radius", C.c_double), ("ndc_rays", C.c_int), ("ndc_width", C.c_int), ("ndc_height", C.c_int),
                ("ndc_near", C.c_float), ("nan_group", C.c_int), ("nan_group_offset", C.c_int)]


class RenderOutputs(C.Structure):
    _fields_ = [(k, _vp) for k in ("color", "depth", "transmittance", "weight", "fields_penalty", "color_coarse",
                                   "depth_coarse", "transmittance_coarse", "weight_coarse", "fields_penalty_coarse",
                                   "dists_coarse", "dists_fine", "nan_flag")]


class Occupancy(C.Structure):
    """neddf_occupancy: an R^3 bitfield over the box lo .. hi (neddf_amd/occupancy.py fills it)."""
    _fields_ = [("d_bits", _vp), ("res", C.c_int), ("lo", C.c_float * 3), ("inv_cell", C.c_float * 3)]


class TraceParams(C.Structure):
    """neddf_trace_params: the constants of one sphere-tracing run (neddf_amd/trace.py validates and fills them)."""
    _fields_ = [("threshold", C.c_float), ("t_near", C.c_float), ("t_far", C.c_float), ("step_scale", C.c_float),
                ("min_step", C.c_float), ("max_steps", C.c_int), ("refine", C.c_int)]


# every symbol include/neddf_hip.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("neddf_abi_version", C.c_int, []),
    ("neddf_create", C.c_int, [C.c_int, C.POINTER(_vp)]),
    ("neddf_destroy", None, [_vp]),
    ("neddf_last_error", C.c_char_p, [_vp]),
    ("neddf_device_cus", C.c_int, [_vp]),
    ("neddf_debug_check_guards", C.c_int, [_vp, C.POINTER(_i64), C.POINTER(_i64)]),
    ("neddf_set_field", C.c_int, [_vp, C.c_int, C.POINTER(FieldDesc), C.POINTER(_fp), C.POINTER(_fp), C.c_int]),
    ("neddf_set_iter", C.c_int, [_vp, C.c_int, C.c_float, C.c_float, _fp]),
    ("neddf_raygen", C.c_int, [_vp, _vp, C.c_int, _i64, C.POINTER(CameraDesc), _vp, _vp, _vp]),
    ("neddf_sample_coarse", C.c_int, [_vp, _vp, _i64, C.c_int, C.c_float, C.c_float, _vp, _vp]),
    ("neddf_sampling", C.c_int, [_vp, _vp, _vp, _vp, _i64, C.c_int, C.c_double, _vp, _vp, _vp, _vp]),
    ("neddf_sampling_view", C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, C.c_int, C.c_double, _vp, _vp, _vp, _vp]),
    ("neddf_rays_to_ndc", C.c_int, [_vp, _vp, _vp, _i64, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, _vp, _vp, _vp]),
    ("neddf_field_forward", C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _i64, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("neddf_composite", C.c_int, [_vp, _vp, _vp, _vp, _i64, C.c_int, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("neddf_integrate_penalty", C.c_int, [_vp, _vp, _vp, _i64, C.c_int, _vp, _vp]),
    ("neddf_importance_resample", C.c_int, [_vp, _vp, _vp, _vp, _i64, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp]),
    ("neddf_render_rays", C.c_int, [_vp, _vp, C.c_int, _i64, C.POINTER(CameraDesc), C.POINTER(RenderParams), _vp, _vp,
                                    C.POINTER(RenderOutputs), _vp]),
    ("neddf_render_rays_single", C.c_int, [_vp, C.c_int, _vp, C.c_int, _i64, C.POINTER(CameraDesc),
                                           C.POINTER(RenderParams), C.c_int, _vp, C.POINTER(RenderOutputs), _vp]),
    ("neddf_op_activation", C.c_int, [_vp, C.c_int, _vp, _vp, _i64, C.c_int, _vp, _vp, _vp]),
    ("neddf_op_positional_encoding", C.c_int, [_vp, _vp, _vp, _vp, _i64, C.c_int, _vp, _vp, _vp]),
    ("neddf_op_pe_weights", C.c_int, [_vp, _vp, _i64, C.c_int, _vp, _vp]),
    ("neddf_op_linear_grad", C.c_int, [_vp, _vp, _vp, _fp, _fp, _i64, C.c_int, C.c_int, _vp, _vp, _vp]),
    ("neddf_set_timing", C.c_int, [_vp, C.c_int]),
    ("neddf_get_timings", C.c_int, [_vp, _fp, C.c_int]),
    ("neddf_get_stage_timings", C.c_int, [_vp, _fp, C.POINTER(C.c_int), C.c_int]),
    ("neddf_comm_unique_id", C.c_int, [_vp, _vp]),
    ("neddf_comm_init", C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    ("neddf_comm_info", C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("neddf_comm_destroy", C.c_int, [_vp]),
    ("neddf_shard_range", None, [_i64, C.c_int, C.c_int, C.POINTER(_i64), C.POINTER(_i64)]),
    ("neddf_shard_range_granular", None, [_i64, _i64, C.c_int, C.c_int, C.POINTER(_i64), C.POINTER(_i64)]),
    ("neddf_gather_pixels", C.c_int, [_vp, _vp, _i64, C.c_int, _vp, _vp]),
    ("neddf_gather_pixels_granular", C.c_int, [_vp, _vp, _i64, _i64, C.c_int, _vp, _vp]),
    ("neddf_comm_wait", C.c_int, [_vp, _vp]),
    ("neddf_comm_wait_host", C.c_int, [_vp, C.c_int]),
    ("neddf_train_workspace_floats", _i64, [_vp, C.c_int, _i64]),
    ("neddf_train_field_forward", C.c_int, [_vp, C.c_int, C.POINTER(_fp), C.POINTER(_fp), C.c_int, _vp, _vp, _vp, _i64, _vp,
                                            _vp, _vp, _vp, _vp, _vp, _vp]),
    ("neddf_train_field_backward", C.c_int, [_vp, C.c_int, C.POINTER(_fp), C.POINTER(_fp), C.c_int, _i64, _vp, _vp, _vp, _vp,
                                             _vp, _vp, C.POINTER(_fp), C.POINTER(_fp), _vp]),
    ("neddf_train_field_backward_inputs", C.c_int, [_vp, C.c_int, C.POINTER(_fp), C.POINTER(_fp), C.c_int, _i64, _vp, _vp, _vp, _vp,
                                                    _vp, _vp, _vp, _vp, _vp, C.POINTER(_fp), C.POINTER(_fp), _vp, _vp, _vp, _vp]),
    ("neddf_sampling_backward", C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, C.c_int, C.c_double, _vp, _vp, _vp]),
    ("neddf_raygen_backward", C.c_int, [_vp, _vp, C.c_int, _i64, C.POINTER(CameraDesc), _vp, _vp, _vp, _vp]),
    ("neddf_composite_backward", C.c_int, [_vp, _vp, _vp, _vp, _i64, C.c_int, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("neddf_field_grid", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _vp, _vp]),
    ("neddf_marching_cubes", C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_float, _vp, _i64, _vp, _i64,
                                       C.POINTER(_i64), C.POINTER(_i64), _vp]),
    ("neddf_field_grid_coarse", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _vp, _vp]),
    ("neddf_brick_select", C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, _vp, _vp, C.POINTER(_i64), _vp]),
    ("neddf_field_bricks", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _vp, _i64, _vp, _vp]),
    ("neddf_marching_cubes_bricks", C.c_int, [_vp, _vp, _vp, _i64, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_float, _vp, _i64,
                                              _vp, _i64, _vp, _vp, C.POINTER(_i64), C.POINTER(_i64), _vp]),
    ("neddf_field_forward_surface", C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _i64, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("neddf_composite_normal", C.c_int, [_vp, _vp, _vp, _vp, _i64, C.c_int, _vp, _vp]),
    ("neddf_render_rays_surface", C.c_int, [_vp, _vp, C.c_int, _i64, C.POINTER(CameraDesc), C.POINTER(RenderParams), _vp, _vp,
                                            C.POINTER(RenderOutputs), _vp, _vp, _vp]),
    ("neddf_render_rays_single_surface", C.c_int, [_vp, C.c_int, _vp, C.c_int, _i64, C.POINTER(CameraDesc),
                                                   C.POINTER(RenderParams), C.c_int, _vp, C.POINTER(RenderOutputs), _vp, _vp]),
    ("neddf_mesh_vertex_normals", C.c_int, [_vp, _vp, _i64, _vp, _i64, _vp, _vp]),
    ("neddf_mesh_components", C.c_int, [_vp, _vp, _i64, _i64, _vp, _vp, _vp, C.POINTER(_i64), _vp]),
    ("neddf_mesh_components_rounds", C.c_int, [_vp]),
    ("neddf_mesh_compact", C.c_int, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, C.POINTER(_i64), C.POINTER(_i64), _vp]),
    ("neddf_occupancy_build", C.c_int, [_vp, _vp, C.c_int, C.c_float, C.c_int, _vp, C.POINTER(_i64), _vp]),
    ("neddf_occupancy_classify", C.c_int, [_vp, C.POINTER(Occupancy), _vp, _i64, _vp, _vp]),
    ("neddf_occupancy_gather", C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, C.POINTER(_i64), _vp]),
    ("neddf_occupancy_scatter", C.c_int, [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("neddf_render_rays_culled", C.c_int, [_vp, _vp, C.c_int, _i64, C.POINTER(CameraDesc), C.POINTER(RenderParams), _vp, _vp,
                                           C.POINTER(RenderOutputs), _vp, _vp, _vp, C.POINTER(Occupancy)]),
    ("neddf_render_rays_single_culled", C.c_int, [_vp, C.c_int, _vp, C.c_int, _i64, C.POINTER(CameraDesc),
                                                  C.POINTER(RenderParams), C.c_int, _vp, C.POINTER(RenderOutputs), _vp, _vp,
                                                  C.POINTER(Occupancy)]),
    ("neddf_cull_stats", C.c_int, [_vp, C.POINTER(_i64), C.POINTER(_i64), C.c_int]),
    ("neddf_trace_begin", C.c_int, [_vp, _vp, _vp, _i64, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("neddf_trace_compact", C.c_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, C.POINTER(_i64), _vp]),
    ("neddf_trace_advance", C.c_int, [_vp, _vp, _vp, _i64, _i64, C.c_float, C.c_float, C.c_float, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("neddf_trace_finish", C.c_int, [_vp, _vp, _i64, _vp]),
    ("neddf_trace_bisect_points", C.c_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i64), _vp]),
    ("neddf_trace_bisect_update", C.c_int, [_vp, _vp, _vp, _i64, _i64, C.c_float, _vp, _vp, _vp, _vp]),
    ("neddf_trace_field", C.c_int, [_vp, C.c_int, _vp, _vp, _i64, C.POINTER(TraceParams), _vp, _vp, _vp, _vp, _vp, C.POINTER(_i64), _vp]),
    # (the uint32 seed travels as a C int: the same 32 bits in the same register; _seed() below folds it into that range)
    ("neddf_mesh_sample_count", C.c_int, [_vp, _vp, _i64, _vp, _i64, C.c_double, C.c_int, C.POINTER(_i64), _vp]),
    ("neddf_mesh_sample_write", C.c_int, [_vp, _vp, _i64, _vp, _i64, C.c_double, C.c_int, _vp, _vp, _i64, C.POINTER(_i64), _vp]),
    ("neddf_nn_brute", C.c_int, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp]),
    ("neddf_nn_grid_build", C.c_int, [_vp, _vp, _i64, _dp, _dp, C.POINTER(C.c_int), _vp, _vp, C.POINTER(_i64), _vp]),
    ("neddf_nn_grid_query", C.c_int, [_vp, _vp, _i64, _vp, _i64, _dp, _dp, C.POINTER(C.c_int), _vp, _vp, _vp, _vp, _vp]),
    ("neddf_raycast_brute", C.c_int, [_vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, C.c_float, C.c_float, C.c_float, _vp, _vp, _vp, _vp, _vp]),
    ("neddf_raycast_grid_count", C.c_int, [_vp, _vp, _i64, _vp, _i64, _dp, _dp, C.POINTER(C.c_int), C.c_float, C.POINTER(_i64), _vp]),
    ("neddf_raycast_grid_build", C.c_int, [_vp, _vp, _i64, _vp, _i64, _dp, _dp, C.POINTER(C.c_int), C.c_float, _vp, _vp, _i64, C.POINTER(_i64), _vp]),
    ("neddf_raycast_grid_query", C.c_int, [_vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _dp, _dp, C.POINTER(C.c_int), C.c_float, _vp, _vp, _i64,
                                           C.c_float, C.c_float, _vp, _vp, _vp, _vp, _vp]),
    ("neddf_point_mesh_brute", C.c_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    ("neddf_point_mesh_grid_query", C.c_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _dp, _dp, C.POINTER(C.c_int), C.c_float, _vp, _vp, _i64,
                                              _vp, _vp, _vp, _vp, _vp]),
    ("neddf_bvh_keys", C.c_int, [_vp, _vp, _i64, _vp, _i64, _dp, _dp, _vp, _vp]),
    ("neddf_bvh_build", C.c_int, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    ("neddf_point_mesh_bvh_query", C.c_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("neddf_raycast_bvh_query", C.c_int, [_vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, C.c_float, C.c_float, C.c_float,
                                          _vp, _vp, _vp, _vp, _vp, _vp]),
    ("neddf_raycast_bvh_occluded", C.c_int, [_vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, C.c_float, C.c_float, C.c_float,
                                             _vp, _vp, _vp]),
    ("neddf_mesh_simplify_keys", C.c_int, [_vp, _vp, _i64, _dp, _dp, C.POINTER(C.c_int), _vp, _vp]),
    ("neddf_mesh_simplify_clusters", C.c_int, [_vp, _vp, _i64, _vp, _vp, C.POINTER(_i64), _vp]),
    ("neddf_mesh_simplify_pairs", C.c_int, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, C.POINTER(_i64), _vp]),
    ("neddf_mesh_simplify_place", C.c_int, [_vp, _vp, _i64, _vp, _vp, _i64, C.c_int, C.c_double, _vp, _i64, _vp, _i64, _vp, _vp]),
    ("neddf_mesh_simplify_attributes", C.c_int, [_vp, _vp, _i64, C.c_int, _vp, _vp, _i64, _vp, _vp]),
    ("neddf_mesh_simplify_triangles", C.c_int, [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp]),
    ("neddf_mesh_simplify_unique", C.c_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp]),
]
SIMPLIFY_PLACEMENTS = {"mean": 0, "quadric": 1}         # NEDDF_SIMPLIFY_*

_lib = None


def load():
    """Load libneddf_hip.so; raises NeddfError if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NeddfError("libneddf_hip.so not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'` "
                             "or `make -C neddf_amd/csrc`; there is no CPU fallback" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.neddf_abi_version() != ABI_VERSION:
            raise NeddfError("libneddf_hip.so ABI %d != binding %d" % (lib.neddf_abi_version(), ABI_VERSION))
        _lib = lib
    return _lib


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _seed(seed):
    """A seed in [0, 2^32) as the signed 32-bit integer with the same bits."""
    seed = int(seed)
    if not 0 <= seed < 2 ** 32:
        raise NeddfError("the seed must fit 32 bits (got %r)" % (seed,))
    return seed - 2 ** 32 if seed >= 2 ** 31 else seed


def require_device(t, what):
    if not t.is_cuda:
        raise NeddfError("%s must live on a HIP device (got %s); the MI355X path has no CPU fallback" % (what, t.device))


# NEDDF_GUARD=1 (the bounds probe, include/neddf_hip.h neddf_debug_check_guards): the buffers the CALLER hands to the training entry
# points -- the workspace and the gradient tensors -- get poisoned bands of their own, checked after every call
def guard_mode():
    """NEDDF_GUARD parsed by ONE rule on both sides of the ABI: the library's atoi(value) != 0 (capi_internal.h guard_mode)."""
    m = __import__("re").match(r"\s*([+-]?\d+)", os.environ.get("NEDDF_GUARD", "0"))
    return bool(m and int(m.group(1)) != 0)


_GUARD = guard_mode()
_GUARD_WORDS, _GUARD_PATTERN = 1024, 0x5AD0BEEF


def _guard_fill(t):
    t.view(torch.int32).fill_(_GUARD_PATTERN)


def _guard_check(t, what):
    bad = int((t.view(torch.int32) != _GUARD_PATTERN).sum().item())
    if bad:
        raise NeddfError("NEDDF_GUARD: %d word(s) written beyond %s" % (bad, what))


def f32c(t):
    return t.contiguous() if t.dtype == torch.float32 else t.to(torch.float32).contiguous()


class Context:
    """A neddf_ctx.  Context.get(device) is the one every module on that device shares; its calls may come from different streams
    as long as the caller orders them.  Work that runs unordered on another stream needs a context of its own, Context(index)
    (include/neddf_hip.h, Conventions)."""
    _instances = {}

    @classmethod
    def get(cls, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise NeddfError("neddf_amd runs on HIP devices only (got %s)" % device)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        if idx not in cls._instances:
            cls._instances[idx] = cls(idx)
        return cls._instances[idx]

    def __init__(self, index):
        self.lib = load()
        self.index = index
        self.device = torch.device("cuda", index)
        h = _vp()
        rc = self.lib.neddf_create(index, C.byref(h))
        if rc != 0:
            raise NeddfError("neddf_create(%d) failed: %s" % (index, self.lib.neddf_last_error(None).decode()))
        self.h = h
        self.slot_owner = {}        # slot -> signature of the field currently loaded
        self._gather_refs = None

    def check(self, rc):
        if rc != 0:
            raise NeddfError("libneddf_hip: %s (code %d)" % (self.lib.neddf_last_error(self.h).decode(), rc))

    @property
    def cus(self):
        return self.lib.neddf_device_cus(self.h)

    def check_guards(self):
        """(bands, overwritten bytes) of the NEDDF_GUARD=1 bounds probe (neddf_debug_check_guards); (0, 0) without it."""
        nb, bad = _i64(0), _i64(0)
        self.check(self.lib.neddf_debug_check_guards(self.h, C.byref(nb), C.byref(bad)))
        return int(nb.value), int(bad.value)

    def stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ------------------------------------------------------------------ fields
    def set_field(self, slot, desc, weights, biases, signature):
        """weights/biases: lists of CPU float32 contiguous tensors in state-dict order.  When the call raises, nobody owns the slot
        any more: whatever the library kept there, the next upload of any module -- the previous owner included -- goes through."""
        n = len(weights)
        wa = (_fp * n)(*[C.cast(w.data_ptr(), _fp) for w in weights])
        ba = (_fp * n)(*[C.cast(b.data_ptr(), _fp) for b in biases])
        try:
            self.check(self.lib.neddf_set_field(self.h, slot, C.byref(desc), wa, ba, n))
        except BaseException:
            self.slot_owner.pop(slot, None)
            raise
        self.slot_owner[slot] = signature

    def set_iter(self, slot, aux_grad_scale, distance_range_max, lowpass):
        arr = (C.c_float * len(lowpass))(*[float(x) for x in lowpass])
        self.check(self.lib.neddf_set_iter(self.h, slot, aux_grad_scale, distance_range_max, arr))

    # ------------------------------------------------------------------ stages
    def raygen(self, uv, cam=None, bundle=False):
        """uv: pixels [n, 2] with a camera descriptor, or a ray bundle (a Ray, or bundle=True with float32 [n, 6] rows of
        (direction, origin); cam may be None): the bundle's rows come back bit for bit.  Or a ViewRays (cam is then not read):
        row b carries the bits that (uv[b], table[view[b]]) gives through the one-camera call."""
        if isinstance(uv, ViewRays):
            cam = uv
        uv, uv_type = _uv_arg(uv, bundle)
        n = uv.shape[0]
        rd = torch.empty(n, 3, device=uv.device, dtype=torch.float32)
        ro = torch.empty_like(rd)
        if n == 0 and (uv_type == UV_RAYS or uv_type & UV_CAMERA_TABLE):    # an empty bundle or table batch (the pointers of empty tensors are NULL)
            return rd, ro
        self.check(self.lib.neddf_raygen(self.h, _ptr(uv), uv_type, n, _cam_arg(cam, uv_type), _ptr(rd), _ptr(ro),
                                         self.stream()))
        return rd, ro

    def sample_coarse(self, U, near, far):
        require_device(U, "U")
        U = f32c(U)
        out = torch.empty_like(U)
        self.check(self.lib.neddf_sample_coarse(self.h, _ptr(U), U.shape[0], U.shape[1], near, far, _ptr(out), self.stream()))
        return out

    def sampling(self, ray_dir, ray_orig, dists, ray_radius, view_dir=None):
        require_device(dists, "dists")
        ray_dir, ray_orig, dists = f32c(ray_dir), f32c(ray_orig), f32c(dists)
        B, S = dists.shape
        pos = torch.empty(B, S, 3, device=dists.device, dtype=torch.float32)
        d = torch.empty_like(pos)
        var = torch.empty_like(pos)
        radius = -1.0 if ray_radius is None else float(ray_radius)
        if view_dir is None:
            self.check(self.lib.neddf_sampling(self.h, _ptr(ray_dir), _ptr(ray_orig), _ptr(dists), B, S, radius, _ptr(pos),
                                               _ptr(d), _ptr(var), self.stream()))
        else:
            view_dir = f32c(view_dir)
            self.check(self.lib.neddf_sampling_view(self.h, _ptr(ray_dir), _ptr(ray_orig), _ptr(view_dir), _ptr(dists), B, S,
                                                    radius, _ptr(pos), _ptr(d), _ptr(var), self.stream()))
        return pos, d, var

    def rays_to_ndc(self, ray_dir, ray_orig, width, height, fx, fy, near):
        """World-space rays -> NDC rays (forward-facing scenes; not a reference function)."""
        require_device(ray_dir, "ray_dir")
        ray_dir, ray_orig = f32c(ray_dir), f32c(ray_orig)
        nd, no = torch.empty_like(ray_dir), torch.empty_like(ray_orig)
        self.check(self.lib.neddf_rays_to_ndc(self.h, _ptr(ray_dir), _ptr(ray_orig), ray_dir.shape[0], int(width), int(height),
                                              float(fx), float(fy), float(near), _ptr(nd), _ptr(no), self.stream()))
        return nd, no

    def field_forward(self, slot, pos, dir, var, out_mode, want):
        """want: iterable of output names; returns dict of flat tensors."""
        require_device(pos, "sample_pos")
        pos, dir, var = f32c(pos), f32c(dir), f32c(var)
        N = pos.numel() // 3
        dev = pos.device
        o = {k: (torch.empty(N * (3 if k == "color" else 1), device=dev, dtype=torch.float32) if k in want else None)
             for k in ("distance", "density", "color", "fields_penalty", "aux_grad")}
        self.check(self.lib.neddf_field_forward(self.h, slot, _ptr(pos), _ptr(dir), _ptr(var), N, out_mode,
                                                _ptr(o["distance"]), _ptr(o["density"]), _ptr(o["color"]),
                                                _ptr(o["fields_penalty"]), _ptr(o["aux_grad"]), self.stream()))
        return {k: v for k, v in o.items() if v is not None}

    def field_forward_surface(self, slot, pos, dir, var, out_mode, want):
        """field_forward plus "distance_grad" / "normal" [N, 3] (neddf_field_forward_surface); NeRF fields raise."""
        require_device(pos, "sample_pos")
        pos, dir, var = f32c(pos), f32c(dir), f32c(var)
        N = pos.numel() // 3
        dev = pos.device
        wide = ("color", "distance_grad", "normal")
        o = {k: (torch.empty(N * (3 if k in wide else 1), device=dev, dtype=torch.float32) if k in want else None)
             for k in ("distance", "density", "color", "fields_penalty", "aux_grad", "distance_grad", "normal")}
        self.check(self.lib.neddf_field_forward_surface(self.h, slot, _ptr(pos), _ptr(dir), _ptr(var), N, out_mode,
                                                        _ptr(o["distance"]), _ptr(o["density"]), _ptr(o["color"]),
                                                        _ptr(o["fields_penalty"]), _ptr(o["aux_grad"]), _ptr(o["distance_grad"]),
                                                        _ptr(o["normal"]), self.stream()))
        return {k: v for k, v in o.items() if v is not None}

    def composite_normal(self, dists, dens, normals):
        """sum_j weight[b, j] * normals[b, j] with composite()'s weights: [B, 3] (neddf_composite_normal)."""
        require_device(dists, "dists")
        dists, dens, normals = f32c(dists), f32c(dens), f32c(normals)
        B, S = dists.shape
        if dens.numel() != B * S or normals.numel() != B * S * 3:
            raise NeddfError("composite_normal: density [B, S] and normals [B, S, 3] expected")
        out = torch.empty(B, 3, device=dists.device, dtype=torch.float32)
        self.check(self.lib.neddf_composite_normal(self.h, _ptr(dists), _ptr(dens), _ptr(normals), B, S, _ptr(out), self.stream()))
        return out

    def mesh_vertex_normals(self, vertices, triangles):
        """Area-weighted geometric vertex normals [V, 3] of an indexed device mesh (neddf_mesh_vertex_normals)."""
        require_device(vertices, "vertices")
        require_device(triangles, "triangles")
        v = f32c(vertices)
        t = triangles.contiguous() if triangles.dtype == torch.int32 else triangles.to(torch.int32).contiguous()
        if v.dim() != 2 or v.shape[1] != 3 or t.dim() != 2 or t.shape[1] != 3:
            raise NeddfError("mesh_vertex_normals: vertices [V, 3] and triangles [T, 3] expected")
        out = torch.empty_like(v)
        self.check(self.lib.neddf_mesh_vertex_normals(self.h, _ptr(v), v.shape[0], _ptr(t), t.shape[0], _ptr(out), self.stream()))
        return out

    # ------------------------------------------------------------------ surface extraction
    @staticmethod
    def _bounds(lo, hi):
        lo, hi = [float(x) for x in lo], [float(x) for x in hi]
        if len(lo) != 3 or len(hi) != 3:
            raise NeddfError("lo / hi must hold three values (x, y, z)")
        return (C.c_double * 3)(*lo), (C.c_double * 3)(*hi)

    def field_grid(self, slot, field, shape, lo, hi):
        """`field` ("distance" / "density") of the field in `slot` on the lattice shape = (nx, ny, nz) between lo and hi
        (np.linspace per axis) -> float32 [nz, ny, nx] on this context's device."""
        if field not in GRID_FIELDS:
            raise NeddfError("field_grid: field must be one of %s (got %r)" % (sorted(GRID_FIELDS), field))
        nx, ny, nz = (int(n) for n in shape)
        blo, bhi = self._bounds(lo, hi)
        vol = torch.empty(max(nz, 0), max(ny, 0), max(nx, 0), device=self.device, dtype=torch.float32)
        self.check(self.lib.neddf_field_grid(self.h, slot, GRID_FIELDS[field], nx, ny, nz, blo, bhi, _ptr(vol), self.stream()))
        return vol

    def marching_cubes(self, volume, iso, lo, hi):
        """Indexed iso-surface of a contiguous float32 [nz, ny, nx] device volume on the lattice lo .. hi:
        (vertices float32 [V, 3], triangles int32 [T, 3]), by a counting call and a writing call of exactly that size."""
        nz, ny, nx = volume.shape
        blo, bhi = self._bounds(lo, hi)
        nv, nt = _i64(0), _i64(0)

        def call(v, t):
            self.check(self.lib.neddf_marching_cubes(self.h, _ptr(volume), nx, ny, nz, blo, bhi, float(iso), _ptr(v),
                                                     0 if v is None else v.shape[0], _ptr(t), 0 if t is None else t.shape[0],
                                                     C.byref(nv), C.byref(nt), self.stream()))
        call(None, None)
        verts = torch.empty(nv.value, 3, device=volume.device, dtype=torch.float32)
        tris = torch.empty(nt.value, 3, device=volume.device, dtype=torch.int32)
        if nv.value and nt.value:
            call(verts, tris)
        return verts, tris

    # ------------------------------------------------------------------ brick-wise surface extraction
    @staticmethod
    def brick_counts(shape, brick):
        """(nbx, nby, nbz): ceil((n - 1) / brick) bricks per axis of the lattice shape = (nx, ny, nz)."""
        return tuple((int(n) - 2 + int(brick)) // int(brick) for n in shape)

    def field_grid_coarse(self, slot, field, shape, brick, lo, hi):
        """field_grid's values at the brick corners, the lattice points min(b * brick, n - 1) per axis: float32 [nbz+1, nby+1, nbx+1]
        (neddf_field_grid_coarse)."""
        if field not in GRID_FIELDS:
            raise NeddfError("field_grid_coarse: field must be one of %s (got %r)" % (sorted(GRID_FIELDS), field))
        nx, ny, nz = (int(n) for n in shape)
        blo, bhi = self._bounds(lo, hi)
        nbx, nby, nbz = (max(n, 0) for n in self.brick_counts((nx, ny, nz), max(int(brick), 1)))
        vol = torch.empty(nbz + 1, nby + 1, nbx + 1, device=self.device, dtype=torch.float32)
        self.check(self.lib.neddf_field_grid_coarse(self.h, slot, GRID_FIELDS[field], nx, ny, nz, int(brick), blo, bhi, _ptr(vol), self.stream()))
        return vol

    def brick_select(self, coarse, iso, band, dilate=0):
        """Active bricks of a contiguous float32 [nbz+1, nby+1, nbx+1] device volume of brick-corner values (neddf_brick_select):
        (slot_map int32 [nbz, nby, nbx], brick_ids int32 [M] ascending)."""
        nbz, nby, nbx = (int(n) - 1 for n in coarse.shape)
        slot_map = torch.empty(max(nbz, 0), max(nby, 0), max(nbx, 0), device=coarse.device, dtype=torch.int32)
        ids = torch.empty(slot_map.numel(), device=coarse.device, dtype=torch.int32)
        m = _i64(0)
        self.check(self.lib.neddf_brick_select(self.h, _ptr(coarse), nbx, nby, nbz, float(iso), float(band), int(dilate), _ptr(slot_map),
                                               _ptr(ids), C.byref(m), self.stream()))
        return slot_map, ids[:m.value].clone()

    def field_bricks(self, slot, field, shape, brick, lo, hi, brick_ids):
        """`field` on the lattices of the listed bricks: float32 [M, (brick + 1)^3], NaN past the fine lattice (neddf_field_bricks)."""
        if field not in GRID_FIELDS:
            raise NeddfError("field_bricks: field must be one of %s (got %r)" % (sorted(GRID_FIELDS), field))
        nx, ny, nz = (int(n) for n in shape)
        blo, bhi = self._bounds(lo, hi)
        require_device(brick_ids, "brick_ids")
        ids = brick_ids.contiguous() if brick_ids.dtype == torch.int32 else brick_ids.to(torch.int32).contiguous()
        vals = torch.empty(ids.shape[0], (int(brick) + 1) ** 3, device=ids.device, dtype=torch.float32)
        self.check(self.lib.neddf_field_bricks(self.h, slot, GRID_FIELDS[field], nx, ny, nz, int(brick), blo, bhi, _ptr(ids), ids.shape[0],
                                               _ptr(vals), self.stream()))
        return vals

    def marching_cubes_bricks(self, values, brick_ids, slot_map, shape, brick, iso, lo, hi):
        """Marching cubes over the listed bricks (neddf_marching_cubes_bricks), by a counting call and a writing call of exactly that
        size: (vertices float32 [V, 3], triangles int32 [T, 3], vertex_key int64 [V], triangle_key int64 [T]) in the library's order."""
        nx, ny, nz = (int(n) for n in shape)
        blo, bhi = self._bounds(lo, hi)
        nv, nt = _i64(0), _i64(0)
        dev = slot_map.device

        def call(v, t, vk, tk):
            self.check(self.lib.neddf_marching_cubes_bricks(self.h, _ptr(values), _ptr(brick_ids), brick_ids.shape[0], _ptr(slot_map), nx, ny, nz,
                                                            int(brick), blo, bhi, float(iso), _ptr(v), 0 if v is None else v.shape[0], _ptr(t),
                                                            0 if t is None else t.shape[0], _ptr(vk), _ptr(tk), C.byref(nv), C.byref(nt),
                                                            self.stream()))
        call(None, None, None, None)
        verts = torch.empty(nv.value, 3, device=dev, dtype=torch.float32)
        tris = torch.empty(nt.value, 3, device=dev, dtype=torch.int32)
        vkey = torch.empty(nv.value, device=dev, dtype=torch.int64)
        tkey = torch.empty(nt.value, device=dev, dtype=torch.int64)
        if nv.value and nt.value:
            call(verts, tris, vkey, tkey)
        return verts, tris, vkey, tkey

    @staticmethod
    def _triangles(triangles, what):
        require_device(triangles, "triangles")
        t = triangles.contiguous() if triangles.dtype == torch.int32 else triangles.to(torch.int32).contiguous()
        if t.dim() != 2 or t.shape[1] != 3:
            raise NeddfError("%s: triangles [T, 3] expected (got %s)" % (what, tuple(t.shape)))
        return t

    def mesh_components(self, triangles, n_vertices):
        """Connected components of an indexed device mesh (neddf_mesh_components): (vertex_label int32 [V], triangle_label int32 [T],
        component_triangles int64 [C]), components numbered by their lowest vertex index, -1 for what belongs to none."""
        t = self._triangles(triangles, "mesh_components")
        V = int(n_vertices)
        if V < 0:
            raise NeddfError("mesh_components: n_vertices must not be negative (got %d)" % V)
        vl = torch.empty(V, device=t.device, dtype=torch.int32)
        tl = torch.empty(t.shape[0], device=t.device, dtype=torch.int32)
        sizes = torch.empty(V, device=t.device, dtype=torch.int64)          # capacity V; the first C entries are written
        nc = _i64(0)
        self.check(self.lib.neddf_mesh_components(self.h, _ptr(t), t.shape[0], V, _ptr(vl), _ptr(tl), _ptr(sizes), C.byref(nc),
                                                  self.stream()))
        return vl, tl, sizes[:nc.value].clone()

    def mesh_components_rounds(self):
        """Union-find rounds of this context's last mesh_components call."""
        return int(self.lib.neddf_mesh_components_rounds(self.h))

    def mesh_compact(self, vertices, triangles, keep_triangle):
        """The kept triangles and the vertices they reference, both in their old order (neddf_mesh_compact), by a counting call and a
        writing call of exactly that size: (vertices float32 [V', 3], triangles int32 [T', 3], vertex_map int32 [V])."""
        require_device(vertices, "vertices")
        t = self._triangles(triangles, "mesh_compact")
        v = f32c(vertices)
        require_device(keep_triangle, "keep_triangle")
        k = keep_triangle.contiguous() if keep_triangle.dtype == torch.uint8 else (keep_triangle != 0).to(torch.uint8).contiguous()
        if v.dim() != 2 or v.shape[1] != 3 or k.dim() != 1 or k.shape[0] != t.shape[0]:
            raise NeddfError("mesh_compact: vertices [V, 3] and keep_triangle [T] expected (got %s, %s)" % (tuple(v.shape), tuple(k.shape)))
        nv, nt = _i64(0), _i64(0)

        def call(ov, ot, vmap):
            self.check(self.lib.neddf_mesh_compact(self.h, _ptr(v), v.shape[0], _ptr(t), t.shape[0], _ptr(k), _ptr(ov),
                                                   0 if ov is None else ov.shape[0], _ptr(ot), 0 if ot is None else ot.shape[0],
                                                   _ptr(vmap), C.byref(nv), C.byref(nt), self.stream()))
        call(None, None, None)
        ov = torch.empty(nv.value, 3, device=v.device, dtype=torch.float32)
        ot = torch.empty(nt.value, 3, device=v.device, dtype=torch.int32)
        if nt.value == 0:           # nothing kept, hence no vertex either
            return ov, ot, torch.full((v.shape[0],), -1, device=v.device, dtype=torch.int32)
        vmap = torch.empty(v.shape[0], device=v.device, dtype=torch.int32)
        call(ov, ot, vmap)
        return ov, ot, vmap

    # ------------------------------------------------------------------ distances between surfaces
    def mesh_sample_count(self, vertices, triangles, density, seed):
        """How many surface samples `density` (per unit area) and `seed` give the mesh (neddf_mesh_sample_count)."""
        require_device(vertices, "vertices")
        t = self._triangles(triangles, "mesh_sample_count")
        v = f32c(vertices)
        n = _i64(0)
        self.check(self.lib.neddf_mesh_sample_count(self.h, _ptr(v), v.shape[0], _ptr(t), t.shape[0], float(density), _seed(seed), C.byref(n),
                                                    self.stream()))
        return int(n.value)

    def mesh_sample_write(self, vertices, triangles, density, seed, n):
        """The n = mesh_sample_count(...) samples (neddf_mesh_sample_write): (points float32 [n, 3], triangle_id int32 [n])."""
        require_device(vertices, "vertices")
        t = self._triangles(triangles, "mesh_sample_write")
        v = f32c(vertices)
        pts = torch.empty(int(n), 3, device=v.device, dtype=torch.float32)
        tid = torch.empty(int(n), device=v.device, dtype=torch.int32)
        got = _i64(0)
        self.check(self.lib.neddf_mesh_sample_write(self.h, _ptr(v), v.shape[0], _ptr(t), t.shape[0], float(density), _seed(seed), _ptr(pts),
                                                    _ptr(tid), int(n), C.byref(got), self.stream()))
        if got.value != int(n):
            raise NeddfError("mesh_sample_write: %d samples counted, %d expected" % (got.value, int(n)))
        return pts, tid

    @staticmethod
    def _grid_args(lo, hi, cells):
        if len(tuple(lo)) != 3 or len(tuple(hi)) != 3 or len(tuple(cells)) != 3:
            raise NeddfError("nearest-neighbour grid: lo, hi and cells must have 3 entries each (got %r, %r, %r)" % (lo, hi, cells))
        return (C.c_double * 3)(*[float(x) for x in lo]), (C.c_double * 3)(*[float(x) for x in hi]), (C.c_int * 3)(*[int(x) for x in cells])

    def nn_brute(self, queries, targets):
        """Exact nearest target of every query by brute force (neddf_nn_brute): (d2 float32 [Q], index int32 [Q])."""
        d2 = torch.empty(queries.shape[0], device=queries.device, dtype=torch.float32)
        idx = torch.empty(queries.shape[0], device=queries.device, dtype=torch.int32)
        self.check(self.lib.neddf_nn_brute(self.h, _ptr(queries), queries.shape[0], _ptr(targets), targets.shape[0], _ptr(d2), _ptr(idx),
                                           self.stream()))
        return d2, idx

    def nn_grid_build(self, targets, lo, hi, cells):
        """The uniform grid of the targets (neddf_nn_grid_build): (cell_start int32 [G + 1], order int32 [N_valid])."""
        blo, bhi, bc = self._grid_args(lo, hi, cells)
        g = int(cells[0]) * int(cells[1]) * int(cells[2])
        start = torch.empty(max(g, 0) + 1, device=targets.device, dtype=torch.int32)
        order = torch.empty(targets.shape[0], device=targets.device, dtype=torch.int32)
        n = _i64(0)
        self.check(self.lib.neddf_nn_grid_build(self.h, _ptr(targets), targets.shape[0], blo, bhi, bc, _ptr(start), _ptr(order), C.byref(n),
                                                self.stream()))
        return start, order[:n.value]

    def nn_grid_query(self, queries, targets, lo, hi, cells, cell_start, order):
        """Exact nearest target of every query through the grid (neddf_nn_grid_query): (d2 float32 [Q], index int32 [Q])."""
        blo, bhi, bc = self._grid_args(lo, hi, cells)
        d2 = torch.empty(queries.shape[0], device=queries.device, dtype=torch.float32)
        idx = torch.empty(queries.shape[0], device=queries.device, dtype=torch.int32)
        self.check(self.lib.neddf_nn_grid_query(self.h, _ptr(queries), queries.shape[0], _ptr(targets), targets.shape[0], blo, bhi, bc,
                                                _ptr(cell_start), _ptr(order), _ptr(d2), _ptr(idx), self.stream()))
        return d2, idx

    # ------------------------------------------------------------------ ray casting on meshes
    @staticmethod
    def _hit_buffers(n, device):
        return (torch.empty(n, device=device, dtype=torch.float32), torch.empty(n, device=device, dtype=torch.int32),
                torch.empty(n, device=device, dtype=torch.float32), torch.empty(n, device=device, dtype=torch.float32))

    def raycast_brute(self, origins, dirs, vertices, triangles, t_min, t_max, pad):
        """The first hit of every ray by brute force (neddf_raycast_brute): (t float32 [R], triangle int32 [R], b1, b2 float32 [R])."""
        t, j, b1, b2 = self._hit_buffers(origins.shape[0], origins.device)
        self.check(self.lib.neddf_raycast_brute(self.h, _ptr(origins), _ptr(dirs), origins.shape[0], _ptr(vertices), vertices.shape[0],
                                                _ptr(triangles), triangles.shape[0], float(t_min), float(t_max), float(pad), _ptr(t), _ptr(j),
                                                _ptr(b1), _ptr(b2), self.stream()))
        return t, j, b1, b2

    def raycast_grid_count(self, vertices, triangles, lo, hi, cells, pad):
        """The number of (list, triangle) pairs of the ray-casting grid (neddf_raycast_grid_count)."""
        blo, bhi, bc = self._grid_args(lo, hi, cells)
        n = _i64(0)
        self.check(self.lib.neddf_raycast_grid_count(self.h, _ptr(vertices), vertices.shape[0], _ptr(triangles), triangles.shape[0], blo, bhi, bc,
                                                     float(pad), C.byref(n), self.stream()))
        return int(n.value)

    def raycast_grid_build(self, vertices, triangles, lo, hi, cells, pad, item_cap):
        """The ray-casting grid (neddf_raycast_grid_build): (cell_start int32 [G + 2], items int32 [item_cap])."""
        blo, bhi, bc = self._grid_args(lo, hi, cells)
        g = int(cells[0]) * int(cells[1]) * int(cells[2])
        start = torch.empty(max(g, 0) + 2, device=vertices.device, dtype=torch.int32)
        items = torch.empty(int(item_cap), device=vertices.device, dtype=torch.int32)
        n = _i64(0)
        self.check(self.lib.neddf_raycast_grid_build(self.h, _ptr(vertices), vertices.shape[0], _ptr(triangles), triangles.shape[0], blo, bhi, bc,
                                                     float(pad), _ptr(start), _ptr(items) if items.numel() else None, int(item_cap), C.byref(n),
                                                     self.stream()))
        return start, items[:n.value]

    def raycast_grid_query(self, origins, dirs, vertices, triangles, lo, hi, cells, pad, cell_start, items, t_min, t_max):
        """The first hit of every ray through the grid (neddf_raycast_grid_query): raycast_brute's result, bit for bit."""
        blo, bhi, bc = self._grid_args(lo, hi, cells)
        t, j, b1, b2 = self._hit_buffers(origins.shape[0], origins.device)
        self.check(self.lib.neddf_raycast_grid_query(self.h, _ptr(origins), _ptr(dirs), origins.shape[0], _ptr(vertices), vertices.shape[0],
                                                     _ptr(triangles), triangles.shape[0], blo, bhi, bc, float(pad), _ptr(cell_start),
                                                     _ptr(items) if items.numel() else None, items.shape[0], float(t_min), float(t_max),
                                                     _ptr(t), _ptr(j), _ptr(b1), _ptr(b2), self.stream()))
        return t, j, b1, b2

    # ------------------------------------------------------------------ point-to-mesh distance
    def point_mesh_brute(self, queries, vertices, triangles):
        """The closest point of the mesh to every query by brute force (neddf_point_mesh_brute): (d2 float32 [Q], triangle int32 [Q],
        b1, b2 float32 [Q])."""
        d2, j, b1, b2 = self._hit_buffers(queries.shape[0], queries.device)
        self.check(self.lib.neddf_point_mesh_brute(self.h, _ptr(queries), queries.shape[0], _ptr(vertices), vertices.shape[0], _ptr(triangles),
                                                   triangles.shape[0], _ptr(d2), _ptr(j), _ptr(b1), _ptr(b2), self.stream()))
        return d2, j, b1, b2

    def point_mesh_grid_query(self, queries, vertices, triangles, lo, hi, cells, pad, cell_start, items):
        """The closest point of the mesh to every query through the ray-casting grid (neddf_point_mesh_grid_query): point_mesh_brute's
        result, bit for bit."""
        blo, bhi, bc = self._grid_args(lo, hi, cells)
        d2, j, b1, b2 = self._hit_buffers(queries.shape[0], queries.device)
        self.check(self.lib.neddf_point_mesh_grid_query(self.h, _ptr(queries), queries.shape[0], _ptr(vertices), vertices.shape[0],
                                                        _ptr(triangles), triangles.shape[0], blo, bhi, bc, float(pad), _ptr(cell_start),
                                                        _ptr(items) if items.numel() else None, items.shape[0], _ptr(d2), _ptr(j), _ptr(b1),
                                                        _ptr(b2), self.stream()))
        return d2, j, b1, b2

    def bvh_keys(self, vertices, triangles, lo, hi):
        """The sort keys of the triangles (neddf_bvh_keys): int64 [T], Morton code of the box centre << 32 | triangle index."""
        blo, bhi, _ = self._grid_args(lo, hi, (1, 1, 1))
        keys = torch.empty(triangles.shape[0], device=vertices.device, dtype=torch.int64)
        self.check(self.lib.neddf_bvh_keys(self.h, _ptr(vertices), vertices.shape[0], _ptr(triangles), triangles.shape[0], blo, bhi,
                                           _ptr(keys) if keys.numel() else None, self.stream()))
        return keys

    def bvh_build(self, vertices, triangles, sorted_keys):
        """The tree over the keys sorted ascending (neddf_bvh_build): (leaf_triangle int32 [T], children int32 [max(T - 1, 0), 2], boxes
        float32 [max(2 T - 1, 0), 6])."""
        n, dev = triangles.shape[0], vertices.device
        leaf = torch.empty(n, device=dev, dtype=torch.int32)
        children = torch.empty(max(n - 1, 0), 2, device=dev, dtype=torch.int32)
        boxes = torch.empty(max(2 * n - 1, 0), 6, device=dev, dtype=torch.float32)
        self.check(self.lib.neddf_bvh_build(self.h, _ptr(vertices), vertices.shape[0], _ptr(triangles), n, _ptr(sorted_keys) if n else None,
                                            _ptr(leaf) if n else None, _ptr(children) if n > 1 else None, _ptr(boxes) if n else None, self.stream()))
        return leaf, children, boxes

    def point_mesh_bvh_query(self, queries, vertices, triangles, leaf_triangle, children, boxes, return_visits=False):
        """The closest point of the mesh to every query through the BVH (neddf_point_mesh_bvh_query): point_mesh_brute's result, bit for
        bit; with return_visits a fifth tensor, the leaves evaluated per query (int32 [Q])."""
        d2, j, b1, b2 = self._hit_buffers(queries.shape[0], queries.device)
        visits = torch.empty(queries.shape[0], device=queries.device, dtype=torch.int32) if return_visits else None
        self.check(self.lib.neddf_point_mesh_bvh_query(self.h, _ptr(queries), queries.shape[0], _ptr(vertices), vertices.shape[0], _ptr(triangles),
                                                       triangles.shape[0], _ptr(leaf_triangle) if leaf_triangle.numel() else None,
                                                       _ptr(children) if children.numel() else None, _ptr(boxes) if boxes.numel() else None,
                                                       leaf_triangle.shape[0], _ptr(d2), _ptr(j), _ptr(b1), _ptr(b2),
                                                       _ptr(visits) if return_visits else None, self.stream()))
        return (d2, j, b1, b2, visits) if return_visits else (d2, j, b1, b2)

    def _raycast_bvh_args(self, origins, dirs, vertices, triangles, leaf_triangle, children, boxes, t_min, t_max, pad):
        return (self.h, _ptr(origins), _ptr(dirs), origins.shape[0], _ptr(vertices), vertices.shape[0], _ptr(triangles), triangles.shape[0],
                _ptr(leaf_triangle) if leaf_triangle.numel() else None, _ptr(children) if children.numel() else None,
                _ptr(boxes) if boxes.numel() else None, leaf_triangle.shape[0], float(t_min), float(t_max), float(pad))

    def raycast_bvh_query(self, origins, dirs, vertices, triangles, leaf_triangle, children, boxes, t_min, t_max, pad, return_visits=False):
        """The first hit of every ray through the BVH (neddf_raycast_bvh_query): raycast_brute's result, bit for bit; with return_visits
        a fifth tensor, the leaves evaluated per ray (int32 [R])."""
        t, j, b1, b2 = self._hit_buffers(origins.shape[0], origins.device)
        visits = torch.empty(origins.shape[0], device=origins.device, dtype=torch.int32) if return_visits else None
        self.check(self.lib.neddf_raycast_bvh_query(*self._raycast_bvh_args(origins, dirs, vertices, triangles, leaf_triangle, children, boxes,
                                                                            t_min, t_max, pad),
                                                    _ptr(t), _ptr(j), _ptr(b1), _ptr(b2), _ptr(visits) if return_visits else None, self.stream()))
        return (t, j, b1, b2, visits) if return_visits else (t, j, b1, b2)

    def raycast_bvh_occluded(self, origins, dirs, vertices, triangles, leaf_triangle, children, boxes, t_min, t_max, pad, return_visits=False):
        """Whether every ray meets the mesh at all, through the BVH (neddf_raycast_bvh_occluded): uint8 [R], 1 where raycast_brute reports
        a triangle; with return_visits a second tensor, the leaves evaluated per ray (int32 [R])."""
        occ = torch.empty(origins.shape[0], device=origins.device, dtype=torch.uint8)
        visits = torch.empty(origins.shape[0], device=origins.device, dtype=torch.int32) if return_visits else None
        self.check(self.lib.neddf_raycast_bvh_occluded(*self._raycast_bvh_args(origins, dirs, vertices, triangles, leaf_triangle, children, boxes,
                                                                               t_min, t_max, pad),
                                                       _ptr(occ), _ptr(visits) if return_visits else None, self.stream()))
        return (occ, visits) if return_visits else occ

    # ------------------------------------------------------------------ mesh simplification (mesh.simplify_mesh orders the steps)
    def mesh_simplify_keys(self, vertices, lo, hi, cells):
        """The sort keys of the vertices (neddf_mesh_simplify_keys): int64 [V], cell << 32 | index, 2^62 | index for a non-finite one."""
        blo, bhi, bc = self._grid_args(lo, hi, cells)
        keys = torch.empty(vertices.shape[0], device=vertices.device, dtype=torch.int64)
        self.check(self.lib.neddf_mesh_simplify_keys(self.h, _ptr(vertices) if keys.numel() else None, vertices.shape[0], blo, bhi, bc,
                                                     _ptr(keys) if keys.numel() else None, self.stream()))
        return keys

    def mesh_simplify_clusters(self, sorted_keys):
        """The clusters of the keys sorted ascending (neddf_mesh_simplify_clusters): (vertex_cluster int32 [V], cluster_range int32 [C, 2])."""
        n, dev = sorted_keys.shape[0], sorted_keys.device
        cluster = torch.empty(n, device=dev, dtype=torch.int32)
        rng = torch.empty(n, 2, device=dev, dtype=torch.int32)
        c = _i64(0)
        self.check(self.lib.neddf_mesh_simplify_clusters(self.h, _ptr(sorted_keys) if n else None, n, _ptr(cluster) if n else None,
                                                         _ptr(rng) if n else None, C.byref(c), self.stream()))
        return cluster, rng[:c.value]

    def mesh_simplify_pairs(self, vertices, triangles, vertex_cluster):
        """The (cluster, triangle) pairs of the valid triangles (neddf_mesh_simplify_pairs), by a counting call and a writing call of
        exactly that size: int64 [P], cluster << 32 | triangle, triangle-major."""
        n = _i64(0)

        def call(pairs):
            self.check(self.lib.neddf_mesh_simplify_pairs(self.h, _ptr(vertices) if vertices.numel() else None, vertices.shape[0],
                                                          _ptr(triangles) if triangles.numel() else None, triangles.shape[0],
                                                          _ptr(vertex_cluster) if vertex_cluster.numel() else None, _ptr(pairs),
                                                          0 if pairs is None else pairs.shape[0], C.byref(n), self.stream()))
        call(None)
        pairs = torch.empty(n.value, device=vertices.device, dtype=torch.int64)
        if n.value:
            call(pairs)
        return pairs

    def mesh_simplify_place(self, vertices, sorted_keys, cluster_range, placement, regularisation, triangles, sorted_pairs):
        """The representative of every cluster (neddf_mesh_simplify_place): float32 [C, 3]."""
        c = cluster_range.shape[0]
        out = torch.empty(c, 3, device=vertices.device, dtype=torch.float32)
        has_pairs = sorted_pairs is not None and sorted_pairs.numel() > 0
        self.check(self.lib.neddf_mesh_simplify_place(self.h, _ptr(vertices) if c else None, vertices.shape[0], _ptr(sorted_keys) if c else None,
                                                      _ptr(cluster_range) if c else None, c, int(placement), float(regularisation),
                                                      _ptr(triangles) if has_pairs else None, triangles.shape[0],
                                                      _ptr(sorted_pairs) if has_pairs else None, sorted_pairs.shape[0] if has_pairs else 0,
                                                      _ptr(out) if c else None, self.stream()))
        return out

    def mesh_simplify_attributes(self, attributes, sorted_keys, cluster_range):
        """The per-cluster mean of every column of float32 [V, k] attributes (neddf_mesh_simplify_attributes): float32 [C, k]."""
        c, k = cluster_range.shape[0], attributes.shape[1]
        out = torch.empty(c, k, device=attributes.device, dtype=torch.float32)
        self.check(self.lib.neddf_mesh_simplify_attributes(self.h, _ptr(attributes) if c else None, attributes.shape[0], k,
                                                           _ptr(sorted_keys) if c else None, _ptr(cluster_range) if c else None, c,
                                                           _ptr(out) if c else None, self.stream()))
        return out

    def mesh_simplify_triangles(self, triangles, n_vertices, vertex_cluster):
        """Corners -> clusters (neddf_mesh_simplify_triangles): (mapped int32 [T, 3] in corner order, lowest int32 [T], keys int64 [T]:
        the triple rotated to its lowest cluster is (lowest, keys >> 31, keys & (2^31 - 1))); -1 for a dropped triangle."""
        n, dev = triangles.shape[0], triangles.device
        mapped = torch.empty(n, 3, device=dev, dtype=torch.int32)
        lowest = torch.empty(n, device=dev, dtype=torch.int32)
        keys = torch.empty(n, device=dev, dtype=torch.int64)
        self.check(self.lib.neddf_mesh_simplify_triangles(self.h, _ptr(triangles) if n else None, n, int(n_vertices),
                                                          _ptr(vertex_cluster) if vertex_cluster.numel() else None, _ptr(mapped) if n else None,
                                                          _ptr(lowest) if n else None, _ptr(keys) if n else None, self.stream()))
        return mapped, lowest, keys

    def mesh_simplify_unique(self, lowest, keys, order):
        """uint8 [T]: 1 for the first of every run of equal rotated triples along `order` (neddf_mesh_simplify_unique)."""
        n = lowest.shape[0]
        keep = torch.empty(n, device=lowest.device, dtype=torch.uint8)
        self.check(self.lib.neddf_mesh_simplify_unique(self.h, _ptr(lowest) if n else None, _ptr(keys) if n else None, n,
                                                       _ptr(order) if n else None, _ptr(keep) if n else None, self.stream()))
        return keep

    def composite(self, dists, dens, col, max_dist):
        require_device(dists, "dists")
        dists, dens, col = f32c(dists), f32c(dens), f32c(col)
        B, S = dists.shape
        dev = dists.device
        w = torch.empty(B, S - 1, device=dev, dtype=torch.float32)
        depth = torch.empty(B, device=dev, dtype=torch.float32)
        color = torch.empty(B, 3, device=dev, dtype=torch.float32)
        trans = torch.empty(B, device=dev, dtype=torch.float32)
        flag = torch.zeros(1, device=dev, dtype=torch.int32)
        self.check(self.lib.neddf_composite(self.h, _ptr(dists), _ptr(dens), _ptr(col), B, S, max_dist, _ptr(w), _ptr(depth),
                                            _ptr(color), _ptr(trans), _ptr(flag), self.stream()))
        return dict(weight=w, depth=depth, color=color, transmittance=trans), flag

    def integrate_penalty(self, dists, pen):
        dists, pen = f32c(dists), f32c(pen)
        out = torch.empty(dists.shape[0], device=dists.device, dtype=torch.float32)
        self.check(self.lib.neddf_integrate_penalty(self.h, _ptr(dists), _ptr(pen), dists.shape[0], dists.shape[1], _ptr(out),
                                                    self.stream()))
        return out

    def importance_resample(self, dists, weights, U, cat_coarse=True, want_ids=False):
        """weights (float32, contiguous, on device) is sanitised in place."""
        require_device(dists, "dists")
        dists, U = f32c(dists), f32c(U)
        assert weights.dtype == torch.float32 and weights.is_contiguous()
        B, n = dists.shape
        nf = U.shape[1]
        out = torch.empty(B, nf + n if cat_coarse else nf, device=dists.device, dtype=torch.float32)
        ids = torch.empty(B, nf, device=dists.device, dtype=torch.int64) if want_ids else None
        self.check(self.lib.neddf_importance_resample(self.h, _ptr(dists), _ptr(weights), _ptr(U), B, n, nf, int(cat_coarse),
                                                      _ptr(out), _ptr(ids), self.stream()))
        return (out, ids) if want_ids else out

    def render_rays(self, uv, cam, params, U_coarse, U_fine, outputs, single_slot=None, occupancy=None, bundle=False):
        """uv: pixels [B, 2], or a ray bundle as in raygen (a Ray, or bundle=True with float32 [B, 6]; cam may then be None).
        outputs: dict name -> preallocated device tensor (subset of RenderOutputs fields, plus "normal" / "normal_coarse"
        [B, 3]: with either present the call goes through the *_surface entry points).  occupancy: an Occupancy struct whose
        bits live on this device -- the call goes through the *_culled entry points (empty-space skipping)."""
        if isinstance(uv, ViewRays):        # a camera per row; cam is not read
            cam = uv
        uv, uv_type = _uv_arg(uv, bundle)
        cam_ref = _cam_arg(cam, uv_type)
        ro = RenderOutputs()
        outputs = dict(outputs)
        normal, normal_coarse = outputs.pop("normal", None), outputs.pop("normal_coarse", None)
        for k, t in outputs.items():
            setattr(ro, k, t.data_ptr())
        if occupancy is not None:
            if single_slot is None:
                self.check(self.lib.neddf_render_rays_culled(self.h, _ptr(uv), uv_type, uv.shape[0], cam_ref,
                                                             C.byref(params), _ptr(U_coarse), _ptr(U_fine), C.byref(ro),
                                                             _ptr(normal), _ptr(normal_coarse), self.stream(), C.byref(occupancy)))
            else:
                self.check(self.lib.neddf_render_rays_single_culled(self.h, single_slot, _ptr(uv), uv_type, uv.shape[0],
                                                                    cam_ref, C.byref(params), U_coarse.shape[1], _ptr(U_coarse),
                                                                    C.byref(ro), _ptr(normal), self.stream(), C.byref(occupancy)))
        elif normal is not None or normal_coarse is not None:
            if single_slot is None:
                self.check(self.lib.neddf_render_rays_surface(self.h, _ptr(uv), uv_type, uv.shape[0], cam_ref,
                                                              C.byref(params), _ptr(U_coarse), _ptr(U_fine), C.byref(ro),
                                                              _ptr(normal), _ptr(normal_coarse), self.stream()))
            else:
                self.check(self.lib.neddf_render_rays_single_surface(self.h, single_slot, _ptr(uv), uv_type, uv.shape[0],
                                                                     cam_ref, C.byref(params), U_coarse.shape[1], _ptr(U_coarse),
                                                                     C.byref(ro), _ptr(normal), self.stream()))
        elif single_slot is None:
            self.check(self.lib.neddf_render_rays(self.h, _ptr(uv), uv_type, uv.shape[0], cam_ref,
                                                  C.byref(params), _ptr(U_coarse), _ptr(U_fine), C.byref(ro), self.stream()))
        else:
            self.check(self.lib.neddf_render_rays_single(self.h, single_slot, _ptr(uv), uv_type, uv.shape[0],
                                                         cam_ref, C.byref(params), U_coarse.shape[1], _ptr(U_coarse),
                                                         C.byref(ro), self.stream()))

    # ------------------------------------------------------------------ empty-space skipping
    def occupancy_build(self, volume, threshold, dilate):
        """Bitfield of the R^3 cells of a contiguous float32 [R+1, R+1, R+1] device volume of corner densities
        (neddf_occupancy_build): (bits int32 [(R^3 + 31) // 32], number of occupied cells)."""
        require_device(volume, "volume")
        if volume.dtype != torch.float32 or not volume.is_contiguous() or volume.dim() != 3 or len(set(volume.shape)) != 1:
            raise NeddfError("occupancy_build: a contiguous float32 [R+1, R+1, R+1] volume expected (got %s)" % (tuple(volume.shape),))
        R = volume.shape[0] - 1
        bits = torch.empty(max((R ** 3 + 31) // 32, 0), device=volume.device, dtype=torch.int32)
        n = _i64(0)
        self.check(self.lib.neddf_occupancy_build(self.h, _ptr(volume), R, float(threshold), int(dilate), _ptr(bits), C.byref(n),
                                                  self.stream()))
        return bits, int(n.value)

    def occupancy_classify(self, occ, points):
        """uint8 [N]: 1 for the points [N, 3] the grid keeps (neddf_occupancy_classify)."""
        require_device(points, "points")
        p = f32c(points).reshape(-1, 3)
        keep = torch.empty(p.shape[0], device=p.device, dtype=torch.uint8)
        self.check(self.lib.neddf_occupancy_classify(self.h, C.byref(occ), _ptr(p), p.shape[0], _ptr(keep), self.stream()))
        return keep

    def occupancy_gather(self, keep, pos, dir, var):
        """Kept rows of pos / dir / var [N, 3] in their old order and their old indices (neddf_occupancy_gather):
        (pos [M, 3], dir [M, 3], var [M, 3], index int32 [M])."""
        require_device(keep, "keep")
        pos, dir, var = f32c(pos).reshape(-1, 3), f32c(dir).reshape(-1, 3), f32c(var).reshape(-1, 3)
        N = pos.shape[0]
        if keep.dtype != torch.uint8 or not keep.is_contiguous() or keep.numel() != N or dir.shape[0] != N or var.shape[0] != N:
            raise NeddfError("occupancy_gather: keep uint8 [N] and pos / dir / var [N, 3] expected")
        out = [torch.empty(N, 3, device=pos.device, dtype=torch.float32) for _ in range(3)]
        index = torch.empty(N, device=pos.device, dtype=torch.int32)
        m = _i64(0)
        self.check(self.lib.neddf_occupancy_gather(self.h, _ptr(keep), _ptr(pos), _ptr(dir), _ptr(var), N, _ptr(out[0]), _ptr(out[1]),
                                                   _ptr(out[2]), _ptr(index), C.byref(m), self.stream()))
        M = int(m.value)
        return out[0][:M], out[1][:M], out[2][:M], index[:M]

    def occupancy_scatter(self, index, n_points, density=None, color=None, normal=None):
        """Compact density [M] / color [M, 3] / normal [M, 3] -> zero-filled [N] / [N, 3] / [N, 3] with row index[k] = row k
        (neddf_occupancy_scatter); None stays None."""
        require_device(index, "index")
        index = index.contiguous()
        M, N = index.shape[0], int(n_points)
        if M == 0:          # nothing kept: all zero (empty tensors have no pointer to hand over)
            z = [None if t is None else torch.zeros(N * w, device=index.device, dtype=torch.float32) for t, w in zip((density, color, normal), (1, 3, 3))]
            return z[0], None if z[1] is None else z[1].view(N, 3), None if z[2] is None else z[2].view(N, 3)
        src = [None if t is None else f32c(t) for t in (density, color, normal)]
        dst = [None if t is None else torch.empty(N * w, device=index.device, dtype=torch.float32) for t, w in zip(src, (1, 3, 3))]
        self.check(self.lib.neddf_occupancy_scatter(self.h, _ptr(index), M, N, _ptr(src[0]), _ptr(src[1]), _ptr(src[2]), _ptr(dst[0]),
                                                    _ptr(dst[1]), _ptr(dst[2]), self.stream()))
        return dst[0], None if dst[1] is None else dst[1].view(N, 3), None if dst[2] is None else dst[2].view(N, 3)

    def cull_stats(self, reset=False):
        """(samples classified, samples kept) over the culled render passes of this context (neddf_cull_stats)."""
        a, b = _i64(0), _i64(0)
        self.check(self.lib.neddf_cull_stats(self.h, C.byref(a), C.byref(b), int(bool(reset))))
        return int(a.value), int(b.value)

    # ------------------------------------------------------------------ sphere tracing
    def trace_state(self, n):
        """Fresh per-ray state arrays on this device: dict t, t_lo, distance float32 [n], status uint8 [n], steps int32 [n]."""
        f = dict(device=self.device, dtype=torch.float32)
        return dict(t=torch.empty(n, **f), t_lo=torch.empty(n, **f), status=torch.empty(n, device=self.device, dtype=torch.uint8),
                    steps=torch.empty(n, device=self.device, dtype=torch.int32), distance=torch.empty(n, **f))

    @staticmethod
    def _rays(origins, dirs, what):
        require_device(origins, "ray origins")
        require_device(dirs, "ray directions")
        o, d = f32c(origins), f32c(dirs)
        if o.dim() != 2 or o.shape[1] != 3 or d.shape != o.shape:
            raise NeddfError("%s: origins and directions [n, 3] expected (got %s, %s)" % (what, tuple(o.shape), tuple(d.shape)))
        return o, d

    def trace_begin(self, origins, dirs, t_near):
        """The state of neddf_trace_begin for the rays origins / dirs [n, 3]."""
        o, d = self._rays(origins, dirs, "trace_begin")
        st = self.trace_state(o.shape[0])
        self.check(self.lib.neddf_trace_begin(self.h, _ptr(o), _ptr(d), o.shape[0], float(t_near), _ptr(st["t"]), _ptr(st["t_lo"]),
                                              _ptr(st["status"]), _ptr(st["steps"]), _ptr(st["distance"]), self.stream()))
        return st

    def trace_compact(self, origins, dirs, st):
        """(index int32 [M], pos [M, 3]) of the ACTIVE rays, ascending (neddf_trace_compact; one stream synchronise)."""
        o, d = self._rays(origins, dirs, "trace_compact")
        n = o.shape[0]
        index, pos = torch.empty(n, device=o.device, dtype=torch.int32), torch.empty(n, 3, device=o.device, dtype=torch.float32)
        m = _i64(0)
        self.check(self.lib.neddf_trace_compact(self.h, _ptr(o), _ptr(d), n, _ptr(st["t"]), _ptr(st["status"]), _ptr(index), _ptr(pos),
                                                C.byref(m), self.stream()))
        return index[:m.value], pos[:m.value]

    @staticmethod
    def _rows(index, distance, what):
        require_device(index, "index")
        require_device(distance, "distances")
        D = f32c(distance).reshape(-1)
        if index.dtype != torch.int32 or not index.is_contiguous() or index.dim() != 1 or D.shape[0] != index.shape[0]:
            raise NeddfError("%s: index int32 [M] and distances [M] expected (got %s, %s)" % (what, tuple(index.shape), tuple(D.shape)))
        return D

    def trace_advance(self, index, distance, st, threshold, step_scale, min_step, t_far):
        """One step of the rays index[k] from the distances distance[k] at their points (neddf_trace_advance); st changes in place."""
        D = self._rows(index, distance, "trace_advance")
        self.check(self.lib.neddf_trace_advance(self.h, _ptr(index), _ptr(D), index.shape[0], st["t"].shape[0], float(threshold), float(step_scale),
                                                float(min_step), float(t_far), _ptr(st["t"]), _ptr(st["t_lo"]), _ptr(st["status"]),
                                                _ptr(st["steps"]), _ptr(st["distance"]), self.stream()))

    def trace_finish(self, st):
        """ACTIVE -> EXHAUSTED (neddf_trace_finish)."""
        self.check(self.lib.neddf_trace_finish(self.h, _ptr(st["status"]), st["status"].shape[0], self.stream()))

    def trace_bisect_points(self, origins, dirs, st):
        """(index int32 [M], pos [M, 3]) of the HIT rays with t_lo < t at 0.5 (t_lo + t) (neddf_trace_bisect_points; one synchronise)."""
        o, d = self._rays(origins, dirs, "trace_bisect_points")
        n = o.shape[0]
        index, pos = torch.empty(n, device=o.device, dtype=torch.int32), torch.empty(n, 3, device=o.device, dtype=torch.float32)
        m = _i64(0)
        self.check(self.lib.neddf_trace_bisect_points(self.h, _ptr(o), _ptr(d), n, _ptr(st["t"]), _ptr(st["t_lo"]), _ptr(st["status"]),
                                                      _ptr(index), _ptr(pos), C.byref(m), self.stream()))
        return index[:m.value], pos[:m.value]

    def trace_bisect_update(self, index, distance, st, threshold):
        """One bisection round from the distances at trace_bisect_points' points (neddf_trace_bisect_update); st changes in place."""
        D = self._rows(index, distance, "trace_bisect_update")
        self.check(self.lib.neddf_trace_bisect_update(self.h, _ptr(index), _ptr(D), index.shape[0], st["t"].shape[0], float(threshold),
                                                      _ptr(st["t"]), _ptr(st["t_lo"]), _ptr(st["distance"]), self.stream()))

    def trace_field(self, slot, origins, dirs, params):
        """The whole loop in the library on the distance of the field in `slot` (neddf_trace_field): (state dict, evaluations)."""
        o, d = self._rays(origins, dirs, "trace_field")
        st = self.trace_state(o.shape[0])
        ev = _i64(0)
        self.check(self.lib.neddf_trace_field(self.h, slot, _ptr(o), _ptr(d), o.shape[0], C.byref(params), _ptr(st["t"]), _ptr(st["t_lo"]),
                                              _ptr(st["status"]), _ptr(st["steps"]), _ptr(st["distance"]), C.byref(ev), self.stream()))
        return st, int(ev.value)

    # ----------------------------------------------------------- stand-alone ops
    def op_activation(self, op, x, J=None):
        require_device(x, "x")
        x = f32c(x)
        y = torch.empty_like(x)
        if J is None:
            self.check(self.lib.neddf_op_activation(self.h, op, _ptr(x), None, x.shape[0], x.shape[1], _ptr(y), None, self.stream()))
            return y
        J = f32c(J)
        G = torch.empty_like(J)
        self.check(self.lib.neddf_op_activation(self.h, op, _ptr(x), _ptr(J), x.shape[0], x.shape[1], _ptr(y), _ptr(G), self.stream()))
        return y, G

    def op_positional_encoding(self, x, J, scale, embed_dim):
        require_device(x, "x")
        x = f32c(x)
        N = x.shape[0]
        if scale is not None:
            scale = f32c(scale.to(x.device).expand(N, 3 * embed_dim))
        y = torch.empty(N, 6 * embed_dim, device=x.device, dtype=torch.float32)
        G = None
        if J is not None:
            J = f32c(J)
            G = torch.empty(N, 3, 6 * embed_dim, device=x.device, dtype=torch.float32)
        self.check(self.lib.neddf_op_positional_encoding(self.h, _ptr(x), _ptr(J), _ptr(scale), N, embed_dim, _ptr(y), _ptr(G),
                                                         self.stream()))
        return y if J is None else (y, G)

    def op_pe_weights(self, var, embed_dim):
        require_device(var, "diag_variance")
        var = f32c(var).reshape(-1, 3)
        w = torch.empty(var.shape[0], 3 * embed_dim, device=var.device, dtype=torch.float32)
        self.check(self.lib.neddf_op_pe_weights(self.h, _ptr(var), var.shape[0], embed_dim, _ptr(w), self.stream()))
        return w

    def op_linear_grad(self, x, J, weight_t, bias):
        require_device(x, "x")
        x, J = f32c(x), f32c(J)
        hw = weight_t.detach().to("cpu", torch.float32).contiguous()
        hb = None if bias is None else bias.detach().to("cpu", torch.float32).contiguous()
        N, cin = x.shape
        cout = hw.shape[1]
        y = torch.empty(N, cout, device=x.device, dtype=torch.float32)
        G = torch.empty(N, 3, cout, device=x.device, dtype=torch.float32)
        self.check(self.lib.neddf_op_linear_grad(self.h, _ptr(x), _ptr(J), C.cast(hw.data_ptr(), _fp),
                                                 None if hb is None else C.cast(hb.data_ptr(), _fp), N, cin, cout, _ptr(y), _ptr(G),
                                                 self.stream()))
        return y, G

    def set_timing(self, on):
        self.check(self.lib.neddf_set_timing(self.h, int(on)))

    # ------------------------------------------------------------------ training step
    @staticmethod
    def _dev_ptrs(tensors, what):
        for t in tensors:
            require_device(t, what)
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise NeddfError("%s must be contiguous float32 device tensors" % what)
        return (_fp * len(tensors))(*[C.cast(t.data_ptr(), _fp) for t in tensors])

    def train_field_forward(self, slot, weights, biases, pos, dir, var, radiance_only=False, sdf=False):
        """Field forward keeping the activations: returns (workspace, distance, density, color, penalty, aux_grad);
        radiance_only (NeRF fields): distance, penalty and aux_grad are None; sdf (NeuS fields): `distance` is the
        sdf, penalty and aux_grad are None."""
        require_device(pos, "sample positions")
        pos, dir, var = f32c(pos).reshape(-1, 3), f32c(dir).reshape(-1, 3), f32c(var).reshape(-1, 3)
        N = pos.shape[0]
        n_ws = self.lib.neddf_train_workspace_floats(self.h, slot, N)
        if n_ws < 0:
            raise NeddfError("libneddf_hip: %s" % self.lib.neddf_last_error(self.h).decode())
        dev = pos.device

        def buf(*shape):
            return torch.empty(*shape, device=dev, dtype=torch.float32)

        n_ws = max(int(n_ws), 1)
        if _GUARD:
            full = buf(n_ws + _GUARD_WORDS)
            _guard_fill(full[n_ws:])
            ws = full[:n_ws]            # ws._base is `full`: train_field_backward checks the band again
        else:
            ws = buf(n_ws)
        density, color = buf(N), buf(N, 3)
        distance, pen, aux = (None, None, None) if radiance_only else ((buf(N), None, None) if sdf else (buf(N), buf(N), buf(N)))
        wa, ba = self._dev_ptrs(weights, "weights"), self._dev_ptrs(biases, "biases")
        self.check(self.lib.neddf_train_field_forward(self.h, slot, wa, ba, len(weights), _ptr(pos), _ptr(dir), _ptr(var), N,
                                                      _ptr(ws), _ptr(distance), _ptr(density), _ptr(color), _ptr(pen), _ptr(aux),
                                                      self.stream()))
        if _GUARD:
            _guard_check(ws._base[n_ws:], "the training workspace (forward)")
        return ws, distance, density, color, pen, aux

    def train_field_backward(self, slot, weights, biases, N, ws, g_distance, g_density, g_color, g_penalty, g_aux, inputs=None):
        """Returns (grad_weights, grad_biases) in the layout of `weights` / `biases`.  `inputs` = the forward's (pos, dir, var):
        additionally returns (g_pos, g_dir, g_var), each [N, 3] (neddf_train_field_backward_inputs)."""
        gs = [None if g is None else f32c(g) for g in (g_distance, g_density, g_color, g_penalty, g_aux)]
        # one zero fill for all gradients (the kernels accumulate into them): views into a flat buffer, 16-byte aligned pieces
        offs, at = [], 0
        gap = 64 if _GUARD else 0       # guard mode: a poisoned band behind every gradient tensor
        for t in list(weights) + list(biases):
            offs.append(at)
            at += ((t.numel() + 3) & ~3) + gap
        flat = torch.zeros(at, device=weights[0].device, dtype=torch.float32)
        views = [flat[o:o + t.numel()].view(t.shape) for o, t in zip(offs, list(weights) + list(biases))]
        if _GUARD:
            for o, t in zip(offs, list(weights) + list(biases)):
                _guard_fill(flat[o + ((t.numel() + 3) & ~3):o + ((t.numel() + 3) & ~3) + gap])
        gw, gb = views[:len(weights)], views[len(weights):]
        wa, ba = self._dev_ptrs(weights, "weights"), self._dev_ptrs(biases, "biases")
        gwa, gba = self._dev_ptrs(gw, "weight gradients"), self._dev_ptrs(gb, "bias gradients")
        g_in = None
        if inputs is None:
            self.check(self.lib.neddf_train_field_backward(self.h, slot, wa, ba, len(weights), N, _ptr(ws), _ptr(gs[0]), _ptr(gs[1]),
                                                           _ptr(gs[2]), _ptr(gs[3]), _ptr(gs[4]), gwa, gba, self.stream()))
        else:
            pos, dir, var = (f32c(t).reshape(-1, 3) for t in inputs)
            if pos.shape[0] != N or dir.shape[0] != N or var.shape[0] != N:
                raise NeddfError("input gradients: pos / dir / var must be the forward call's [N, 3] tensors")
            g_in = tuple(torch.empty(N, 3, device=pos.device, dtype=torch.float32) for _ in range(3))
            self.check(self.lib.neddf_train_field_backward_inputs(self.h, slot, wa, ba, len(weights), N, _ptr(ws), _ptr(pos), _ptr(dir),
                                                                  _ptr(var), _ptr(gs[0]), _ptr(gs[1]), _ptr(gs[2]), _ptr(gs[3]),
                                                                  _ptr(gs[4]), gwa, gba, _ptr(g_in[0]), _ptr(g_in[1]), _ptr(g_in[2]),
                                                                  self.stream()))
        if _GUARD:
            for i, (o, t) in enumerate(zip(offs, list(weights) + list(biases))):
                e = o + ((t.numel() + 3) & ~3)
                _guard_check(flat[e:e + gap], "gradient tensor %d" % i)
            if ws._base is not None:
                _guard_check(ws._base[ws.numel():], "the training workspace (backward)")
        if g_in is not None:
            return gw, gb, g_in
        return gw, gb

    def sampling_backward(self, g_pos, g_dir, g_var, ray_dir, dists, ray_radius):
        """Backward of `sampling` with respect to the ray: [B, S, 3] sample gradients (any may be None) -> g_ray_dir, g_ray_orig [B, 3]."""
        require_device(dists, "dists")
        ray_dir, dists = f32c(ray_dir), f32c(dists)
        B, S = dists.shape
        gs = [None if g is None else f32c(g) for g in (g_pos, g_dir, g_var)]
        for g in gs:
            if g is not None and g.numel() != B * S * 3:
                raise NeddfError("sampling_backward: sample gradients must be [B, S, 3]")
        g_rd = torch.empty(B, 3, device=dists.device, dtype=torch.float32)
        g_ro = torch.empty_like(g_rd)
        radius = -1.0 if ray_radius is None else float(ray_radius)
        self.check(self.lib.neddf_sampling_backward(self.h, _ptr(gs[0]), _ptr(gs[1]), _ptr(gs[2]), _ptr(ray_dir), _ptr(dists), B, S,
                                                    radius, _ptr(g_rd), _ptr(g_ro), self.stream()))
        return g_rd, g_ro

    def raygen_backward(self, uv, cam, g_ray_dir, g_ray_orig, bundle=False):
        """Backward of `raygen` with respect to the pose: g_R [3, 3], g_T [3] (device tensors).  With a ViewRays (cam is then not
        read): [K, 12], row v = (g_R row-major, g_T) of camera v over its own rows in batch order, zeros for a camera without rows."""
        table = isinstance(uv, ViewRays)
        if table:
            cam = uv
        uv, uv_type = _uv_arg(uv, bundle)        # (a bundle is refused by the library: it has no pose)
        g_rd, g_ro = f32c(g_ray_dir), f32c(g_ray_orig)
        if g_rd.shape != (uv.shape[0], 3) or g_ro.shape != (uv.shape[0], 3):
            raise NeddfError("raygen_backward: ray gradients must be [B, 3]")
        if table:
            out = torch.empty(cam.table.shape[0], 12, device=uv.device, dtype=torch.float32)
            self.check(self.lib.neddf_raygen_backward(self.h, _ptr(uv), uv_type, uv.shape[0], _cam_arg(cam, uv_type), _ptr(g_rd),
                                                      _ptr(g_ro), _ptr(out), self.stream()))
            return out
        out = torch.empty(12, device=uv.device, dtype=torch.float32)
        self.check(self.lib.neddf_raygen_backward(self.h, _ptr(uv), uv_type, uv.shape[0], _cam_arg(cam, uv_type), _ptr(g_rd),
                                                  _ptr(g_ro), _ptr(out), self.stream()))
        return out[:9].view(3, 3), out[9:]

    def composite_backward(self, dists, density, color, max_dist, g_weight, g_depth, g_color, g_trans):
        dists, density, color = f32c(dists), f32c(density), f32c(color)
        B, S = dists.shape
        gs = [None if g is None else f32c(g) for g in (g_weight, g_depth, g_color, g_trans)]
        g_density = torch.empty(B, S, device=dists.device, dtype=torch.float32)
        g_pc = torch.empty(B, S, 3, device=dists.device, dtype=torch.float32)
        self.check(self.lib.neddf_composite_backward(self.h, _ptr(dists), _ptr(density), _ptr(color), B, S, float(max_dist),
                                                     _ptr(gs[0]), _ptr(gs[1]), _ptr(gs[2]), _ptr(gs[3]), _ptr(g_density),
                                                     _ptr(g_pc), self.stream()))
        return g_density, g_pc

    def get_stage_timings(self):
        """{stage: (summed ms, launches)} for every NEDDF_STAGE_* since the last call (drains the same events as get_timings)."""
        n = len(STAGES)
        ms, cnt = (C.c_float * n)(), (C.c_int * n)()
        self.check(self.lib.neddf_get_stage_timings(self.h, ms, cnt, n))
        return {k: (ms[i], int(cnt[i])) for i, k in enumerate(STAGES)}

    # ------------------------------------------------------------------ multi-GPU (RCCL communicator owned by the library)
    def comm_unique_id(self):
        buf = C.create_string_buffer(COMM_ID_BYTES)
        self.check(self.lib.neddf_comm_unique_id(self.h, buf))
        return buf.raw

    def comm_init(self, rank, nranks, unique_id):
        assert len(unique_id) == COMM_ID_BYTES
        self.check(self.lib.neddf_comm_init(self.h, rank, nranks, C.create_string_buffer(unique_id, COMM_ID_BYTES)))

    def comm_info(self):
        r, n, v = C.c_int(), C.c_int(), C.c_int()
        self.check(self.lib.neddf_comm_info(self.h, C.byref(r), C.byref(n), C.byref(v)))
        return dict(rank=r.value, nranks=n.value, rccl_version=v.value)

    def comm_destroy(self):
        self.check(self.lib.neddf_comm_destroy(self.h))
        self._gather_refs = None

    def gather_pixels(self, local, n_total, out=None, granule=1):
        """Start the all-gather of this rank's slab [n_rank, C] into out [n_total, C] on the library's communication stream,
        ordered after the current stream's work; returns `out`.  Nothing may touch local / out until comm_wait().
        Slabs are cut on multiples of `granule` rows (neddf_shard_range_granular)."""
        require_device(local, "local pixels")
        local = f32c(local)
        if out is None:
            out = torch.empty(n_total, local.shape[1], device=local.device, dtype=torch.float32)
        self.check(self.lib.neddf_gather_pixels_granular(self.h, _ptr(local), n_total, int(granule), local.shape[1], _ptr(out), self.stream()))
        self._gather_refs = (local, out)       # keep both alive (and out of the caching allocator) until the wait
        return out

    def comm_wait(self):
        """The current stream waits (on the device) for the last gather."""
        self.check(self.lib.neddf_comm_wait(self.h, self.stream()))
        self._gather_refs = None

    def comm_wait_host(self, timeout_ms=60000):
        self.check(self.lib.neddf_comm_wait_host(self.h, int(timeout_ms)))

    def get_timings(self):
        """{'ddf_ms','col_ms','nerf_ms','ddf_launches','col_launches','nerf_launches'} since the last call."""
        arr = (C.c_float * 6)()
        self.check(self.lib.neddf_get_timings(self.h, arr, 6))
        return dict(ddf_ms=arr[0], col_ms=arr[1], nerf_ms=arr[2], ddf_launches=int(arr[3]), col_launches=int(arr[4]),
                    nerf_launches=int(arr[5]))
