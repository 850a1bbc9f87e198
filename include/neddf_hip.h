/*
 * neddf_hip.h -- C ABI of libneddf_hip.so, the MI355X (gfx950) volumetric
 * renderer behind the reference project's Python plugin surface.
 *
 * The reference (ueda0319/neddf) has no FFI: its "plugin API" is the set of
 * Python classes Hydra instantiates.  This header is
 * the boundary those classes' replacements (package neddf_amd, aliased as
 * neddf) call through ctypes.  Each entry point names the reference function
 * it replaces (paths relative to the reference checkout).
 *
 * Conventions
 *   - extern "C", POD only, no torch types.  Every `d_` pointer is a DEVICE
 *     pointer owned by the caller (a torch allocation); `h_` pointers are HOST.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  All
 *     stage calls are asynchronous on that stream; the caller synchronises.
 *     The calls that hand a count back to the host say "synchronises `stream`"
 *     in their comment: they wait for that stream (and for no other) to read it.
 *     No other call blocks the host once the workspaces have grown to its sizes
 *     (a workspace that has to grow is reallocated behind a device synchronise:
 *     the first call of a new, larger size).
 *   - Return 0 on success, a negative NEDDF_E* code otherwise; never throws.
 *     neddf_last_error(ctx) returns a static/ctx-owned message.
 *   - A ctx belongs to one device and owns the packed weights and the scratch
 *     workspaces (the field kernels' `scratch` and tile counters `sched`
 *     included), which ALL its calls share.  Calls into one ctx may come from
 *     different streams, but the caller must order them (an event, a stream
 *     wait): two calls into one ctx that may run at the same time overwrite each
 *     other's workspaces.  Unordered concurrent use needs one ctx per stream;
 *     a device may have any number of them and distinct ctxs are independent.
 *     A ctx is not thread-safe.  The one exception to "the caller orders" is
 *     neddf_set_field: it waits for the last launch that reads the slot it
 *     replaces, on whichever stream that was, and for nothing else.
 */
#ifndef NEDDF_HIP_H
#define NEDDF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libneddf_hip.so is built with -fvisibility=hidden: the entry points declared between this push and the pop at the end of the
 * file are its whole export list (tests/test_host.py holds `nm -D` to exactly these names). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define NEDDF_ABI_VERSION 7

enum { NEDDF_OK = 0, NEDDF_EINVAL = -1, NEDDF_EHIP = -2, NEDDF_EUNSUPPORTED = -3, NEDDF_ENOFIELD = -4,
       NEDDF_ECOMM = -5,      /* RCCL reported an error (message in neddf_last_error) or is not loadable */
       NEDDF_ETIMEOUT = -6 }; /* neddf_comm_wait_host: the collective did not finish in time; the communicator was aborted */
enum { NEDDF_FIELD_NEDDF = 0, NEDDF_FIELD_NERF = 1, NEDDF_FIELD_NEUS = 2 };
enum { NEDDF_ACT_RELU = 0, NEDDF_ACT_LEAKY = 1, NEDDF_ACT_TANHEXP = 2 };
/* operand type of the 256-wide dense layers: fp32 (exact, the parity path) or bf16 weights + bf16 activations with
 * fp32 accumulation on v_mfma_f32_32x32x16_bf16 (BASELINE.json configs[4]); heads, biases, encodings stay fp32 */
enum { NEDDF_DTYPE_F32 = 0, NEDDF_DTYPE_BF16 = 1,
       /* fp32 weights and activations contracted on the fp16 matrix instructions: every operand split into two fp16 terms
        * (21-22 bits), the three products above 2^-22 accumulated in fp32; weights pre-scaled by 2^10 to stay in fp16's normal
        * range.  Errors at the level of the fp32 MFMA path's own, 2.5x its throughput; operands beyond +-65504 saturate */
       NEDDF_DTYPE_F16_SPLIT = 2,
       /* fp16 weights + fp16 activations with fp32 accumulation on v_mfma_f32_32x32x16_f16 (additive to ABI v7): the bf16 policy's
        * kernels and shapes with 11 significant bits per operand instead of 8, within about 4 % of bf16's speed; heads, biases,
        * encodings stay fp32.
        * Inference only: every entry point that evaluates a field (neddf_field_forward, _forward_surface, _grid, _grid_coarse,
        * _bricks, the six neddf_render_rays* calls, neddf_trace_field) takes it for NeDDF, NeRF and NeuS at every width; the
        * training entry points treat it exactly as they treat NEDDF_DTYPE_BF16 -- they do not read the packed weights at all and
        * run fp32 MFMA products on the live fp32 tensors.  fp16 ends at +-65504: a finite OPERAND beyond that (an activation
        * during evaluation) becomes Inf, and neddf_set_field refuses (NEDDF_EUNSUPPORTED, slot untouched) a field with a finite
        * weight or bias beyond it; NaN and Inf weights are accepted as under every policy */
       NEDDF_DTYPE_F16 = 3 };
enum { NEDDF_SLOT_COARSE = 0, NEDDF_SLOT_FINE = 1, NEDDF_NUM_SLOTS = 4 };
/* uv element types accepted by neddf_raygen (the reference takes int64 in
 * render_image, int16 in training, float in its tests) */
enum { NEDDF_UV_F32 = 0, NEDDF_UV_I64 = 1, NEDDF_UV_I32 = 2, NEDDF_UV_I16 = 3,
       /* a ray bundle instead of pixels (additive to ABI v7): d_uv is float [n_rays, 6], each row the ray direction xyz followed by
        * the ray origin xyz in world space, and h_cam is not read (it may be NULL).  neddf_raygen copies the rows to d_ray_dir /
        * d_ray_orig bit for bit -- NaN payloads included, NO normalisation: unit length is the caller's contract, as it is for
        * neddf_sampling -- and neddf_render_rays, _single, _surface, _single_surface, _culled and _single_culled start from the same
        * copy; every later stage is the one the pixel types reach, and the stream contract is that of the call it rides in.
        * Refused, with a neddf_last_error message and nothing written: params->ndc_rays != 0 (NEDDF_EUNSUPPORTED: the NDC map needs
        * a camera's focal lengths) and neddf_raygen_backward (NEDDF_EINVAL: there is no pose to differentiate).  A uv_type
        * is valid in all of these calls when it is 0..4, or 0..3 with NEDDF_UV_CAMERA_TABLE (below) OR-ed on; everything else --
        * 5, a negative value, any other bit, the flag on NEDDF_UV_RAYS -- is NEDDF_EINVAL, and h_cam is not dereferenced. */
       NEDDF_UV_RAYS = 4 };
/* OR-ed onto NEDDF_UV_F32 .. NEDDF_UV_I16 (additive to ABI v7): every row has its own camera.  h_cam then points to a HOST
 * neddf_camera_table (cast to const neddf_camera *), which is read before the call returns; the arrays it names are DEVICE memory
 * read on the stream, so the stream contract is that of the call it rides in.
 *   neddf_raygen and the six neddf_render_rays* calls: row b carries the bits that the call gives for (uv[b], d_cameras[d_view[b]])
 *     without the flag; every later stage is unchanged.  A row whose d_view[b] lies outside [0, n_cameras) reads no camera: its six
 *     ray floats are quiet NaNs, which the fused calls report through nan_flag.
 *   neddf_raygen_backward: d_g_RT is [n_cameras, 12] and EVERY row is written; row v carries the bits that the call gives without
 *     the flag for camera v on the rows with d_view[b] == v, in batch order (+0.0 for a camera that owns no row; a row with an
 *     invalid view belongs to no camera).  One launch, a fixed-order reduction per camera, no floating-point atomics.
 * Refused with a neddf_last_error message before anything is written: the flag with h_cam == NULL, with a NULL array while
 * n_rays > 0 or with n_cameras outside 1 .. 2^20 (NEDDF_EINVAL); the flag with params->ndc_rays != 0 (NEDDF_EUNSUPPORTED: the NDC
 * map takes one camera's focal lengths). */
enum { NEDDF_UV_CAMERA_TABLE = 0x100 };
/* field output selection */
enum { NEDDF_OUT_MINIMAL = 0,   /* density + color (+distance, aux_grad): what compositing consumes */
       NEDDF_OUT_FULL = 1 };    /* + fields_penalty: Jacobian through the colour trunk (neddf.py:243-300) */

typedef struct neddf_ctx neddf_ctx;

/* Architecture of one field network.  Mirrors the constructor keywords of
 * NeDDF (neddf/network/neddf.py:52-66) and NeRF (neddf/network/nerf.py:34-44). */
typedef struct {
    int kind;                 /* NEDDF_FIELD_* */
    int embed_pos_rank;       /* 1..10 */
    int embed_dir_rank;       /* >= 1; both encodings + 32 columns must fit a 512-column tile row (training: <= 10) */
    int layer_count;          /* NeDDF: ddf_layer_count, NeRF: layer_count */
    int layer_width;          /* rendering: 1..512; training: 256 or 512 (other widths zero-padded by the caller) */
    int col_layer_count;      /* NeDDF only */
    int col_layer_width;      /* NeDDF (== layer_width) and NeuS */
    int n_skips;
    int skips[8];
    int activation;           /* NEDDF_ACT_* */
    int density_activation;   /* NEDDF_ACT_* */
    float d_near;             /* NeDDF only */
    /* NeDDF penalty weights in the dict order of neddf.py:260-291:
     * constraints_aux_grad, constraints_dDdt, range_distance, range_aux_grad,
     * range_color, constraints_color; has[i]==0 leaves the term unweighted. */
    float penalty_weight[6];
    int penalty_has[6];
    int weight_dtype;         /* NEDDF_DTYPE_* */
} neddf_field_desc;

/* Pinhole camera: Camera.R / Camera.T (camera.py:117-118) and
 * PinholeCalib [fx, fy, cx, cy] (pinhole_calib.py:8). */
typedef struct {
    float R[9];
    float T[3];
    float calib[4];
} neddf_camera;

/* A camera per row (uv_type | NEDDF_UV_CAMERA_TABLE, above). */
typedef struct {
    const neddf_camera *d_cameras;   /* DEVICE [n_cameras] rows of 16 floats: R row-major, T, calib -- neddf_camera's own layout */
    const int32_t      *d_view;      /* DEVICE [n_rays]: the camera of row b */
    int32_t             n_cameras;   /* 1 .. 2^20 */
} neddf_camera_table;

/* NeRFRender constructor values (neddf/render/nerf_render.py:40-81). */
typedef struct {
    int sample_coarse;
    int sample_fine;
    float dist_near, dist_far, max_dist;
    int cone_sampling;        /* sampling_type == "cone" */
    double ray_radius;        /* 1/1111/sqrt(12), nerf_render.py:144-145 */
    /* forward-facing scenes (not in the reference, see neddf_rays_to_ndc): when ndc_rays != 0 the samples are taken
     * along normalised-device-coordinate rays (dist_near / dist_far are then NDC depths, usually 0 and 1) while the
     * field still receives the world-space unit viewing direction */
    int ndc_rays;
    int ndc_width, ndc_height;
    float ndc_near;
    /* neddf_render_rays on a batch that stands for several render_rays calls of the reference (render_image hands the
     * library many `chunk`s at once): rays [k*nan_group, (k+1)*nan_group) share sample_pdf's NaN fallback decision
     * (base_neural_render.py:105-114 decides per call) and fall back to the linspace of group k's first ray.
     * 0 = the whole batch is one call.  nan_group_offset = index, inside its group, of the batch's first ray (a ray-sharded
     * slab may begin in the middle of a chunk; the leading partial group then falls back to ITS first ray's linspace). */
    int nan_group;
    int nan_group_offset;
} neddf_render_params;

int neddf_abi_version(void);
int neddf_create(int device, neddf_ctx **out);
void neddf_destroy(neddf_ctx *ctx);
const char *neddf_last_error(neddf_ctx *ctx);
/* number of compute units of the ctx's device (for roofline reporting) */
int neddf_device_cus(neddf_ctx *ctx);
/* Bounds probe (ABI v5; no reference counterpart -- the stand-in for a GPU-side sanitizer run).  With NEDDF_GUARD=1 in the environment
 * every workspace of the context is allocated at its exact size between two poisoned 4 KiB bands and every carve of the render arena
 * is followed by a 256 B one; this call synchronises the device and reports how many bands exist and how many of their bytes a kernel
 * has overwritten (0 = no out-of-bounds store reached a band).  Without NEDDF_GUARD it reports 0 bands. */
int neddf_debug_check_guards(neddf_ctx *ctx, int64_t *n_bands, int64_t *n_bad_bytes);

/* Replaces nn.Module.load_state_dict for one network (base_trainer.py:121).
 * h_weights / h_biases: HOST fp32 arrays in state-dict order
 *   NeDDF: layers_ddf.0..n, layers_col.0..m, layer_ddf_out, layer_aux_out, layer_col_out
 *          (LinearGradLayer weights are [in,out], linear.py:113)
 *   NeRF : layers.0..n, outL_density, outL_color.0, outL_color.2
 *          (nn.Linear weights are [out,in], nerf.py:88-103)
 *   NeuS : layers_sdf.0..n-1, layers_col.0..m (m = col_layer_count; last is 256 -> 3), then `variance`
 *          as a 1-element weight with a dummy bias (nn.Linear layout, neus.py:80-99); desc.layer_count =
 *          sdf_layer_count, desc.col_layer_count = col_layer_count, activation ReLU or tanhExp
 * The library packs them into MFMA fragment order and uploads; the caller keeps
 * ownership of the sources.
 * A REFUSED call leaves the slot exactly as it was: every NEDDF_EINVAL / NEDDF_EUNSUPPORTED answer (a descriptor or an
 * architecture the engine does not take) and a device block that cannot be allocated come before the slot is touched, so
 * the field loaded there before keeps answering with the same results.  Only a HIP call that fails once the replacement
 * has begun (NEDDF_EHIP from the copy) leaves the slot without a field; the next call on it then reports NEDDF_ENOFIELD. */
int neddf_set_field(neddf_ctx *ctx, int slot, const neddf_field_desc *desc,
                    const float *const *h_weights, const float *const *h_biases, int n_tensors);
/* Replaces NeDDF.set_iter / NeRF.set_iter (neddf.py:311-326, nerf.py:167-178):
 * h_lowpass[embed_pos_rank] = get_lowpass_scale(lowpass_alpha) per frequency. */
int neddf_set_iter(neddf_ctx *ctx, int slot, float aux_grad_scale, float distance_range_max,
                   const float *h_lowpass);

/* Camera.create_rays (camera.py:155-171) + get_center_of_pixels (:173-187) +
 * PinholeCalib.unproject_local (pinhole_calib.py:51-74). */
int neddf_raygen(neddf_ctx *ctx, const void *d_uv, int uv_type, int64_t n_rays, const neddf_camera *h_cam,
                 float *d_ray_dir, float *d_ray_orig, void *stream);
/* Stratified coarse distances (nerf_render.py:131-140): dists[b,j] =
 * linspace(near,far,S1)[j] + U[b,j]*(far-near)/(S1-1). */
int neddf_sample_coarse(neddf_ctx *ctx, const float *d_U, int64_t n_rays, int S1, float dist_near,
                        float dist_far, float *d_dists, void *stream);
/* Ray.get_sampling_cones (ray.py:128-194) when ray_radius >= 0, else
 * Ray.get_sampling_points (ray.py:88-126).  Outputs [n_rays,S,3] each. */
int neddf_sampling(neddf_ctx *ctx, const float *d_ray_dir, const float *d_ray_orig, const float *d_dists,
                   int64_t n_rays, int S, double ray_radius, float *d_pos, float *d_dir, float *d_var,
                   void *stream);
/* The same with a separate viewing direction [n_rays,3] copied to d_dir (NDC rays: positions follow the NDC ray,
 * the field sees the world-space direction). */
int neddf_sampling_view(neddf_ctx *ctx, const float *d_ray_dir, const float *d_ray_orig, const float *d_view_dir,
                        const float *d_dists, int64_t n_rays, int S, double ray_radius, float *d_pos, float *d_dir,
                        float *d_var, void *stream);
/* World-space rays -> normalised-device-coordinate rays of a width x height pinhole view with focal lengths fx, fy and
 * near plane z = -near (Mildenhall et al. 2020, appendix C; the reference has no NDC code -- parity is pinned on the
 * projective identity NDC(o + t d) = o' + t' d', t' = 1 - oz_near / (oz_near + t dz), checked in tests). */
int neddf_rays_to_ndc(neddf_ctx *ctx, const float *d_ray_dir, const float *d_ray_orig, int64_t n_rays, int width, int height,
                      float fx, float fy, float near_plane, float *d_ndc_dir, float *d_ndc_orig, void *stream);
/* NeDDF.forward (neddf.py:162-309) / NeRF.forward (nerf.py:107-165) on N
 * sample points (pos/dir/var [N,3]).  Any output pointer may be NULL.
 * NeRF fields produce density and color only; NeuS fields (neus.py:101-162) return the sdf in d_distance.
 * NeDDF without a penalty output (NEDDF_OUT_MINIMAL, or d_penalty == NULL) and NeuS: the position gradient of the distance / sdf is taken
 * in reverse mode (one gradient row per point instead of the reference's three forward-mode Jacobian rows, neddf.py:206-230);
 * with a penalty output the Jacobian rows are carried forward as in the reference.  The two agree within rounding (the
 * parity gates of tests/test_gpu_parity.py hold for both).
 * Hidden tanhExp activations (nn_module/with_grad/tanh_exp.py:15-54) are evaluated as x (1 - 2 / (e^(2 e^x) + 1)) for every x: absolute
 * error ~1e-7 |x| where the reference's tanh keeps relative accuracy; network outputs stay as close to an fp64 evaluation as the
 * reference's own fp32 ones.  The stand-alone neddf_op_activation below keeps the reference's form. */
int neddf_field_forward(neddf_ctx *ctx, int slot, const float *d_pos, const float *d_dir, const float *d_var,
                        int64_t n_points, int out_mode, float *d_distance, float *d_density, float *d_color,
                        float *d_fields_penalty, float *d_aux_grad, void *stream);
/* ---- surface normals (additive to ABI v7: new functions only) ----------------------------------------------------
 * neddf_field_forward plus the two quantities the distance trunk hands to the colour trunk, each [N,3], each nullable:
 *   d_distance_grad  NeDDF: distance_grad, the position gradient of the distance (neddf.py:223); NeuS: `gradients`, the
 *                    position gradient of the sdf that the reference takes with torch.autograd.grad (neus.py:135-143)
 *   d_normal         what the colour trunk receives: NeDDF norm_dir = distance_grad / (|distance_grad| + 1e-7) (neddf.py:235,241);
 *                    NeuS the sdf gradient itself, NOT normalised (neus.py:144-145 concatenates `gradients` as they are)
 * Both are read back from the per-point record the distance kernel leaves for the colour kernel, under every operand policy and
 * both output modes (NEDDF_OUT_MINIMAL: reverse-mode gradient, NEDDF_OUT_FULL: forward-mode Jacobian rows); the other outputs are
 * those of neddf_field_forward bit for bit.  NEDDF_EUNSUPPORTED for NeRF fields (no distance, no sdf: nerf.py:107-165). */
int neddf_field_forward_surface(neddf_ctx *ctx, int slot, const float *d_pos, const float *d_dir, const float *d_var,
                                int64_t n_points, int out_mode, float *d_distance, float *d_density, float *d_color,
                                float *d_fields_penalty, float *d_aux_grad, float *d_distance_grad, float *d_normal, void *stream);
/* The normal render target: d_out_normal[b] = sum_j weight[b,j] * d_normals[b,j] over the S-1 intervals and with the weights of
 * neddf_composite (base_neural_render.py:148-160, where color is integrated the same way).  d_normals [n_rays,S,3].  Not
 * normalised: its length is at most 1 - transmittance for unit normals, the background is the zero vector.  One wave per ray,
 * fp64 multiplicative wave scan, fixed reduction order: bitwise repeatable. */
int neddf_composite_normal(neddf_ctx *ctx, const float *d_dists, const float *d_density, const float *d_normals, int64_t n_rays, int S,
                           float *d_out_normal, void *stream);
/* BaseNeuralRender.integrate_volume_render (base_neural_render.py:117-172).
 * d_weight [n_rays,S-1] may be NULL.  *d_nan_flag (int, may be NULL) is set to 1
 * if any weight is NaN (the reference asserts, :155). */
int neddf_composite(neddf_ctx *ctx, const float *d_dists, const float *d_density, const float *d_color,
                    int64_t n_rays, int S, float max_dist, float *d_weight, float *d_depth, float *d_out_color,
                    float *d_transmittance, int *d_nan_flag, void *stream);
/* penalty line integral (nerf_render.py:153-159): out[b] = sum_j (t[j+1]-t[j]) * pen[b,j] */
int neddf_integrate_penalty(neddf_ctx *ctx, const float *d_dists, const float *d_penalty, int64_t n_rays, int S,
                            float *d_out, void *stream);
/* BaseNeuralRender.sample_pdf (base_neural_render.py:27-115) with explicit
 * uniforms d_U [n_rays,n_fine].  d_dists [n_rays,n], d_weights [n_rays,n-1] is
 * sanitised IN PLACE like the reference (:52-55).  d_out [n_rays, n_fine+n]
 * (cat_coarse) or [n_rays,n_fine]; d_ids (int64, may be NULL) receives the
 * searchsorted indices.  The NaN fallback (:105-114) is applied on device, batch-wide
 * (one call of the reference = one call here). */
int neddf_importance_resample(neddf_ctx *ctx, const float *d_dists, float *d_weights, const float *d_U,
                              int64_t n_rays, int n, int n_fine, int cat_coarse, float *d_out, int64_t *d_ids,
                              void *stream);

/* ---- stand-alone layer ops (neddf/nn_module): unit-level counterparts of what the
 * fused field kernels do internally; same device code as their epilogues. ---- */
enum { NEDDF_OP_RELU = 0, NEDDF_OP_LEAKY = 1, NEDDF_OP_TANHEXP = 2, NEDDF_OP_SOFTPLUS = 3, NEDDF_OP_SIGMOID = 4 };
/* {ReLU,LeakyReLU,TanhExp,Softplus,Sigmoid}GradFunction.forward (with_grad/{relu,leaky_relu,tanh_exp,softplus,sigmoid}.py):
 * d_x [N,C], d_J [N,3,C] -> d_y [N,C], d_G [N,3,C].  With d_J == NULL: the plain
 * activation (F.relu / F.leaky_relu / tanhExp, nn_module/tanh_exp.py:15-33). */
int neddf_op_activation(neddf_ctx *ctx, int op, const float *d_x, const float *d_J, int64_t N, int C, float *d_y,
                        float *d_G, void *stream);
/* PositionalEncodingGradLayer.forward (with_grad/positional_encoding.py:34-87) when
 * d_J != NULL, PositionalEncoding.forward (positional_encoding.py:37-65) otherwise.
 * d_x [N,3], d_J [N,3,3], d_scale [N,3E] or NULL -> d_y [N,6E], d_G [N,3,6E]. */
int neddf_op_positional_encoding(neddf_ctx *ctx, const float *d_x, const float *d_J, const float *d_scale, int64_t N,
                                 int embed_dim, float *d_y, float *d_G, void *stream);
/* Sampling.get_pe_weights (sampling.py:44-71): d_var [N,3] -> d_w [N,3E] */
int neddf_op_pe_weights(neddf_ctx *ctx, const float *d_var, int64_t N, int embed_dim, float *d_w, void *stream);
/* LinearGradFunction.forward (with_grad/linear.py:15-46) on the MFMA tile engine:
 * y = xW + b, G = JW.  h_W [Cin,Cout] / h_b [Cout] are HOST arrays (packed + uploaded
 * per call: this op is a test/compat entry point, the renderer keeps weights resident).
 * Synchronises `stream` twice per block of weights: before the upload, which reuses the previous block's buffer, and after it,
 * because the packed block is a host temporary.
 * Any Cin, Cout (round 4): K blocks of 256 input columns accumulate in the outputs, N blocks of 256 / 128 output columns. */
int neddf_op_linear_grad(neddf_ctx *ctx, const float *d_x, const float *d_J, const float *h_W, const float *h_b,
                         int64_t N, int Cin, int Cout, float *d_y, float *d_G, void *stream);

/* Outputs of the fused renderer; every pointer may be NULL. Shapes per ray. */
typedef struct {
    float *color;            /* [3] */
    float *depth;            /* [1] */
    float *transmittance;    /* [1] */
    float *weight;           /* [S_fine-1]   (S_fine = sample_fine+1+sample_coarse+1) */
    float *fields_penalty;   /* [1]  (forces NEDDF_OUT_FULL on NeDDF fields) */
    float *color_coarse, *depth_coarse, *transmittance_coarse;
    float *weight_coarse;    /* [sample_coarse] (sanitised, as the reference returns it) */
    float *fields_penalty_coarse;
    float *dists_coarse;     /* [sample_coarse+1] */
    float *dists_fine;       /* [S_fine] */
    int *nan_flag;           /* single int: NaN weight seen (reference asserts) */
} neddf_render_outputs;

/* NeRFRender.render_rays (nerf_render.py:109-188): raygen -> stratified ->
 * sampling -> field(coarse) -> composite -> sample_pdf -> sampling ->
 * field(fine) -> composite, all on `stream`, no host round trip.
 * d_U_coarse [n_rays, sample_coarse+1], d_U_fine [n_rays, sample_fine+1]: the
 * uniforms the reference draws with torch.rand (nerf_render.py:137,
 * base_neural_render.py:75). */
int neddf_render_rays(neddf_ctx *ctx, const void *d_uv, int uv_type, int64_t n_rays, const neddf_camera *h_cam,
                      const neddf_render_params *params, const float *d_U_coarse, const float *d_U_fine,
                      const neddf_render_outputs *out, void *stream);
/* Single-pass variant (BASELINE.json configs[1]: "128 samples/ray"): raygen ->
 * stratified S1 samples -> sampling -> field(slot) -> composite. */
int neddf_render_rays_single(neddf_ctx *ctx, int slot, const void *d_uv, int uv_type, int64_t n_rays,
                             const neddf_camera *h_cam, const neddf_render_params *params, int S1,
                             const float *d_U, const neddf_render_outputs *out, void *stream);

/* neddf_render_rays / neddf_render_rays_single with the normal target: d_normal [n_rays,3] (fine pass) and d_normal_coarse
 * [n_rays,3] (coarse pass), either may be NULL; per sample the field's d_normal of neddf_field_forward_surface, integrated as by
 * neddf_composite_normal.  Every output of `out` is what the plain call writes, bit for bit.  NEDDF_EUNSUPPORTED when a requested
 * normal would come from a NeRF field. */
int neddf_render_rays_surface(neddf_ctx *ctx, const void *d_uv, int uv_type, int64_t n_rays, const neddf_camera *h_cam,
                              const neddf_render_params *params, const float *d_U_coarse, const float *d_U_fine,
                              const neddf_render_outputs *out, float *d_normal, float *d_normal_coarse, void *stream);
int neddf_render_rays_single_surface(neddf_ctx *ctx, int slot, const void *d_uv, int uv_type, int64_t n_rays,
                                     const neddf_camera *h_cam, const neddf_render_params *params, int S1,
                                     const float *d_U, const neddf_render_outputs *out, float *d_normal, void *stream);

/* Stage timing: hipEvent pairs recorded on the launch stream around every stage kernel launched through this ctx while
 * timing is enabled (neddf_set_timing), drained by either getter (both synchronise on the recorded events).
 * neddf_get_timings: ms[0..2] = summed duration of the distance-trunk / colour-trunk / NeRF kernel launches,
 * ms[3..5] = the corresponding launch counts; n must be >= 6.
 * neddf_get_stage_timings: ms[k], launches[k] for every NEDDF_STAGE_* (n_stages >= NEDDF_STAGE_COUNT). */
enum { NEDDF_STAGE_DDF = 0, NEDDF_STAGE_COL = 1, NEDDF_STAGE_NERF = 2, NEDDF_STAGE_RAYGEN = 3, NEDDF_STAGE_NDC = 4,
       NEDDF_STAGE_SAMPLE_COARSE = 5, NEDDF_STAGE_SAMPLING = 6, NEDDF_STAGE_COMPOSITE = 7, NEDDF_STAGE_PENALTY = 8,
       NEDDF_STAGE_RESAMPLE = 9, NEDDF_STAGE_GATHER = 10, NEDDF_STAGE_COUNT = 11 };
int neddf_set_timing(neddf_ctx *ctx, int enable);
int neddf_get_timings(neddf_ctx *ctx, float *ms, int n);
int neddf_get_stage_timings(neddf_ctx *ctx, float *ms, int *launches, int n_stages);

/* ---- multi-GPU: rays shard, pixels are gathered ----------------------------
 * The reference renders on one device; its rays are independent (nerf_render.py:128-188 has no cross-ray term), so
 * the flat pixel index of a frame (or of several frames) is cut into one contiguous slab per rank and the only
 * exchange is an all-gather of the rendered pixels over RCCL/xGMI.  One process per GPU, one communicator per ctx.
 * RCCL is loaded on first use (dlopen "librccl.so.1": in a torch process that is the copy torch already mapped);
 * a library user that never calls these needs no RCCL.
 *
 * Bootstrap: rank 0 calls neddf_comm_unique_id and hands the NEDDF_COMM_ID_BYTES to every rank by any channel the
 * integrator has (file, socket, MPI, a torch.distributed store); every rank then calls neddf_comm_init -- a blocking
 * collective over the ranks. */
#define NEDDF_COMM_ID_BYTES 128
int neddf_comm_unique_id(neddf_ctx *ctx, void *h_id);
int neddf_comm_init(neddf_ctx *ctx, int rank, int nranks, const void *h_id);
/* rank / nranks of the ctx's communicator (0 / 0 without one) and the RCCL version code (e.g. 22606) */
int neddf_comm_info(neddf_ctx *ctx, int *rank, int *nranks, int *rccl_version);
int neddf_comm_destroy(neddf_ctx *ctx);
/* Slab [lo, hi) of range(n_total) that `rank` of `nranks` owns: contiguous, sizes differ by at most one. */
void neddf_shard_range(int64_t n_total, int rank, int nranks, int64_t *lo, int64_t *hi);
/* The same with slab boundaries on multiples of `granule` rows (the last granule of the range may be short): granule counts per
 * rank differ by at most one.  render_image's chunk is the granule of a sharded frame, so that no chunk -- the unit the reference
 * decides sample_pdf's NaN fallback on, base_neural_render.py:105-114 -- is split between two ranks.  granule = 1 is
 * neddf_shard_range. */
void neddf_shard_range_granular(int64_t n_total, int64_t granule, int rank, int nranks, int64_t *lo, int64_t *hi);
/* All-gather of the per-rank slabs d_local [hi-lo, channels] (fp32, neddf_shard_range order) into d_all
 * [n_total, channels] on every rank.  The collective runs on the ctx's own communication stream, ordered after the
 * work already enqueued on `stream` (the renderer's stream), and returns immediately: the caller keeps rendering the
 * next view on `stream` while the pixels travel.  d_local and d_all must stay untouched until neddf_comm_wait.
 * With equal slabs the gather lands directly in d_all; ragged slabs go through a ctx-owned padded staging buffer. */
int neddf_gather_pixels(neddf_ctx *ctx, const float *d_local, int64_t n_total, int channels, float *d_all, void *stream);
/* ... of slabs cut by neddf_shard_range_granular(n_total, granule, ...). */
int neddf_gather_pixels_granular(neddf_ctx *ctx, const float *d_local, int64_t n_total, int64_t granule, int channels, float *d_all,
                                 void *stream);
/* Make `stream` wait (device-side, no host block) for the last neddf_gather_pixels of this ctx.  NEDDF_ECOMM (once) if the
 * communicator was aborted while that gather was in flight: d_all is incomplete. */
int neddf_comm_wait(neddf_ctx *ctx, void *stream);
/* Host-side wait with a deadline: 0 when the last gather has completed; on an asynchronous RCCL error NEDDF_ECOMM; after
 * timeout_ms without completion the communicator is aborted (ncclCommAbort), the ctx returns to "no communicator"
 * (neddf_comm_info: 0 ranks; neddf_comm_init may be called again) and NEDDF_ETIMEOUT is returned -- a peer died. */
int neddf_comm_wait_host(neddf_ctx *ctx, int timeout_ms);

/* ---- training step -------------------------------------------
 * The reference trains through torch autograd over its with_grad modules
 * (the modules under neddf/nn_module/with_grad: each has a hand-written backward for the
 * (value, Jacobian) pair).  These entry points are that forward + backward for one NeDDF
 * network on N sample points.  NeRF fields (nerf.py:107-165; plain torch autograd in the reference) are
 * supported through the same calls: only density and color are produced / consumed, nn.Linear layout.
 * NeuS fields (neus.py:101-162) likewise: d_distance / d_g_distance carry the sdf, penalty and aux_grad are
 * not touched, d_var is ignored; the last tensor is `variance` (1 element, its bias slot is not read or
 * written).  The reference differentiates NeuS twice (the normal is torch.autograd.grad(create_graph=True));
 * here that is the reverse pass over the (value, Jacobian) rows of the sdf trunk, with the second derivative
 * of tanhExp that torch derives from the plain Function's backward (nn_module/tanh_exp.py:36-60).
 * The parameters are DEVICE fp32 arrays in the reference's
 * state-dict layout and order (see neddf_set_field); gradients are ACCUMULATED into d_gW / d_gB
 * (same shapes).  The slot supplies the architecture and the set_iter state; the weights it was
 * loaded with are not used here.  `d_workspace` (neddf_train_workspace_floats floats, caller-owned)
 * carries the saved activations from the forward call to the matching backward call. */
int64_t neddf_train_workspace_floats(neddf_ctx *ctx, int slot, int64_t n_points);
/* NeDDF.forward (neddf.py:162-309) in training mode: all five outputs ([N] each, color [N,3]); any may be NULL. */
int neddf_train_field_forward(neddf_ctx *ctx, int slot, const float *const *d_W, const float *const *d_B, int n_tensors,
                              const float *d_pos, const float *d_dir, const float *d_var, int64_t n_points,
                              float *d_workspace, float *d_distance, float *d_density, float *d_color,
                              float *d_fields_penalty, float *d_aux_grad, void *stream);
/* Reverse pass: upstream gradients of the five outputs (any may be NULL = zero) -> parameter gradients. */
int neddf_train_field_backward(neddf_ctx *ctx, int slot, const float *const *d_W, const float *const *d_B, int n_tensors,
                               int64_t n_points, const float *d_workspace, const float *d_g_distance,
                               const float *d_g_density, const float *d_g_color, const float *d_g_fields_penalty,
                               const float *d_g_aux_grad, float *const *d_gW, float *const *d_gB, void *stream);
/* ---- pose gradients (ABI v7) --------------------------------------------------------------------------------------
 * In the reference the rays come from camera.R / camera.T through differentiable torch ops, so a loss reaches Camera.params.
 * These three entry points are that chain: field inputs, sampler, ray generation.  Reductions run in a fixed order (no
 * floating-point atomics): the results are bitwise repeatable.
 *
 * neddf_train_field_backward plus the gradients of the forward's sample inputs, d_g_pos / d_g_dir / d_g_var ([n_points, 3],
 * OVERWRITTEN, any may be NULL); d_pos / d_dir / d_var are the arrays the forward call was given.  Differentiates NeDDF.forward
 * (neddf.py:186-257): embed_pos_scaled into distance layer 0 and every skip layer, embed_pos and embed_dir into colour layer 0
 * (value and Jacobian rows, the second-derivative terms of the Jacobian rows included); norm_dir is detached and sample_pos_grad
 * is the constant identity.  d_g_var is ZERO: Sampling.get_pe_weights (ray/sampling.py:44-71) runs with gradients disabled in the
 * reference, which makes the cone weights constants of its autograd.  The parameter gradients are bit for bit those of
 * neddf_train_field_backward.  The new products run on the fp32 MFMA path.  NeRF fields (nerf.py:139-159) take the same call with value
 * rows only: embed_pos into layer 0 and after every skip layer, embed_dir into the colour head.  NEDDF_EUNSUPPORTED for NeuS (a
 * third derivative of the sdf trunk) and for a field loaded under the split-fp16 operand policy. */
int neddf_train_field_backward_inputs(neddf_ctx *ctx, int slot, const float *const *d_W, const float *const *d_B, int n_tensors,
                                      int64_t n_points, const float *d_workspace, const float *d_pos, const float *d_dir,
                                      const float *d_var, const float *d_g_distance, const float *d_g_density,
                                      const float *d_g_color, const float *d_g_fields_penalty, const float *d_g_aux_grad,
                                      float *const *d_gW, float *const *d_gB, float *d_g_pos, float *d_g_dir, float *d_g_var,
                                      void *stream);
/* Backward of neddf_sampling with respect to the ray (Ray.get_sampling_cones ray.py:128-194, get_sampling_points ray.py:88-126):
 * pos = o + d t, dir = d, cone var = t_var d^2 + r_var (1 - d^2).  d_g_pos / d_g_dir / d_g_var [n_rays, S, 3] (any may be NULL)
 * -> d_g_ray_dir, d_g_ray_orig [n_rays, 3].  The distances are not differentiated (the reference draws them under no_grad).
 * radius < 0: point samples. */
int neddf_sampling_backward(neddf_ctx *ctx, const float *d_g_pos, const float *d_g_dir, const float *d_g_var, const float *d_ray_dir,
                            const float *d_dists, int64_t n_rays, int S, double radius, float *d_g_ray_dir, float *d_g_ray_orig,
                            void *stream);
/* Backward of neddf_raygen with respect to the pose (Camera.create_rays camera.py:155-171: ray_dir = R c(uv), ray_orig = T):
 * d_g_RT[12] (DEVICE) = g_R [3][3] row-major = sum_b g_ray_dir[b] (x) c_b, then g_T [3] = sum_b g_ray_orig[b].  The intrinsics
 * are not differentiated.  With uv_type | NEDDF_UV_CAMERA_TABLE: d_g_RT[n_cameras][12], one such row per camera of the table. */
int neddf_raygen_backward(neddf_ctx *ctx, const void *d_uv, int uv_type, int64_t n, const neddf_camera *cam, const float *d_g_ray_dir,
                          const float *d_g_ray_orig, float *d_g_RT, void *stream);
/* Backward of integrate_volume_render (base_neural_render.py:148-171): gradients of weight [n_rays,S-1],
 * depth [n_rays], color [n_rays,3], transmittance [n_rays] (any may be NULL) -> d_g_density [n_rays,S],
 * d_g_point_color [n_rays,S,3]. */
int neddf_composite_backward(neddf_ctx *ctx, const float *d_dists, const float *d_density, const float *d_color,
                             int64_t n_rays, int S, float max_dist, const float *d_g_weight, const float *d_g_depth,
                             const float *d_g_color, const float *d_g_transmittance, float *d_g_density,
                             float *d_g_point_color, void *stream);

/* ---- surface extraction (ABI v6; the reference meshes voxelize()'s cube with PyMCubes inside its Open3D viewer,
 * neddf/scripts/fields_visualizer.py:528-566) -------------------------------------------------------------------
 * Lattice: nx x ny x nz points between h_lo[3] and h_hi[3] (HOST doubles, x y z), coordinate i of an axis =
 * (float)(lo + i * ((hi - lo) / (n - 1))) computed in double and the last one exactly hi: np.linspace's points, so that
 * BaseNeuralField.voxelize (base_neuralfield.py:49-79) evaluates the same ones.  Volumes are [nz][ny][nx], x fastest. */
enum { NEDDF_GRID_DISTANCE = 0, NEDDF_GRID_DENSITY = 1 };
/* Field slot `slot`'s distance (NeuS: sdf) or density on the lattice, dir = (1, 0, 0) and var = 0 as voxelize passes them, under
 * the slot's operand policy; written to d_volume [nz][ny][nx].  The lattice is evaluated in chunks of 2^23 points (the field
 * kernels' launch size).  NEDDF_EINVAL for a dimension below 2, lo >= hi on an axis, or an output the field lacks (NeRF: distance). */
int neddf_field_grid(neddf_ctx *ctx, int slot, int field, int nx, int ny, int nz, const double *h_lo, const double *h_hi, float *d_volume,
                     void *stream);
/* Marching cubes (Lorensen & Cline 1987, Bourke's corner / edge numbering; case table: neddf_amd/csrc/mc_tables.h) over a
 * [nz][ny][nx] volume on the lattice above: an indexed mesh, one vertex per lattice edge the iso-surface crosses.
 *   - a corner is inside when value < iso (NaN is outside); on the edge from lattice point g0 (value v0) to g1 (v1) the vertex is
 *     g0 + t * (g1 - g0), t = (iso - v0) / (v1 - v0) in fp32 (t = 1/2 when that is NaN), the other two coordinates exact
 *   - d_vertices [V][3] float (x, y, z in world units): ordered by the owning (lower) lattice point's linear index, then x, y, z edge
 *   - d_triangles [T][3] int32: ordered by cell, then by table order; (p1 - p0) x (p2 - p0) points from the inside to the outside
 *   - the output does not depend on timing (count / scan / write launches, no atomics)
 * Two calls: with d_vertices or d_triangles NULL, or a cap below its count, only *h_n_vertices / *h_n_triangles are written;
 * otherwise the mesh is too.  Synchronises `stream` once (to read the counts).  NEDDF_EUNSUPPORTED when V >= 2^31. */
int neddf_marching_cubes(neddf_ctx *ctx, const float *d_volume, int nx, int ny, int nz, const double *h_lo, const double *h_hi, float iso,
                         float *d_vertices, int64_t vertex_cap, int32_t *d_triangles, int64_t triangle_cap, int64_t *h_n_vertices,
                         int64_t *h_n_triangles, void *stream);

/* ---- brick-wise surface extraction (additive to ABI v7; no reference counterpart) ------------------------------------
 * The lattice above cut into bricks of B^3 cells, B = `brick` in [2, 16]: nb_a = ceil((n_a - 1) / B) bricks per axis, brick
 * (bx, by, bz) at linear index (bz nby + by) nbx + bx; the last brick of an axis may be partial.  A brick's lattice is (B+1)^3
 * points at local index (lz (B+1) + ly)(B+1) + lx, lattice point b B + l per axis; points past the fine lattice are padding and
 * hold a quiet NaN, and the cells that touch them do not exist.  The coarse lattice is the (nbx+1)(nby+1)(nbz+1) fine lattice
 * points at index min(b B, n - 1) per axis.  Every entry point: NEDDF_EINVAL for a brick size outside [2, 16], a dimension
 * below 2 or lo >= hi on an axis.
 *
 * neddf_field_grid_coarse: neddf_field_grid's values at the coarse lattice points, d_coarse [nbz+1][nby+1][nbx+1]. */
int neddf_field_grid_coarse(neddf_ctx *ctx, int slot, int field, int nx, int ny, int nz, int brick, const double *h_lo, const double *h_hi,
                            float *d_coarse, void *stream);
/* Brick selection from d_coarse [nbz+1][nby+1][nbx+1]: a brick is active when, among its 8 coarse corners, one is NaN, (v < iso)
 * differs between two, or fabsf(v - iso) <= band for one (band >= 0); the active set is then grown by `dilate` bricks (0..4) in the
 * Chebyshev sense, clipped at the grid.  For an L-Lipschitz field band = L * (half the brick's diagonal) misses no brick that holds
 * a piece of the level set.
 *   - d_slot_map int32 [nbz][nby][nbx]: the rank of the brick among the active ones in ascending brick index, or -1
 *   - d_brick_ids int32, capacity nbx nby nbz: the first M entries = the active brick indices, ascending
 *   - *h_n_active (HOST) = M (0 is legal); synchronises `stream` once to read it
 * Count / scan / write launches, no atomics: the result does not depend on timing. */
int neddf_brick_select(neddf_ctx *ctx, const float *d_coarse, int nbx, int nby, int nbz, float iso, float band, int dilate,
                       int32_t *d_slot_map, int32_t *d_brick_ids, int64_t *h_n_active, void *stream);
/* The field on the lattices of the n_bricks bricks listed in d_brick_ids: d_values float [n_bricks][(B+1)^3].  Every value carries
 * the bits neddf_field_grid gives that lattice point (a point shared by several bricks is evaluated once per brick); padding -- and
 * every point of a brick index outside the grid -- gets a quiet NaN.  Points are generated on the device and evaluated in chunks of
 * at most 2^23 (the padding of a partial brick rides along at a clamped lattice point and is overwritten). */
int neddf_field_bricks(neddf_ctx *ctx, int slot, int field, int nx, int ny, int nz, int brick, const double *h_lo, const double *h_hi,
                       const int32_t *d_brick_ids, int64_t n_bricks, float *d_values, void *stream);
/* Marching cubes over the listed bricks: d_values [M][(B+1)^3] as neddf_field_bricks writes them, d_brick_ids [M] strictly ascending,
 * d_slot_map [nbz][nby][nbx] its inverse (-1 for an unlisted brick) -- what neddf_brick_select returns, or any subset built the same way.
 *   - the triangles are exactly neddf_marching_cubes' triangles of the cells that lie in listed bricks, the vertices exactly those
 *     these triangles reference, each once, with neddf_marching_cubes' coordinates bit for bit
 *   - a lattice edge belongs to the listed brick of lowest index whose lattice contains it: an edge on a face or edge shared by
 *     listed bricks gives one vertex, an edge shared with an unlisted brick is still produced
 *   - order: bricks ascending, then lattice points / cells by local index, then x, y, z edge / table order
 *   - d_vertex_key int64 [V] = (the edge's lower lattice point's fine linear index) * 3 + axis; d_triangle_key int64 [T] = (the cell's
 *     corner-0 fine linear index) * 5 + position in the case's table order: sorting by them gives neddf_marching_cubes' order
 *   - the output does not depend on timing (count / scan / write launches, no atomics)
 * Two calls, as neddf_marching_cubes: with an output pointer NULL or a cap below its count only the HOST counts are written.
 * Synchronises `stream` once.  NEDDF_EINVAL also for n_bricks outside [0, nbx nby nbz], a brick index outside the grid, a list that
 * is not strictly ascending or a slot map that is not its inverse (checked on the device); NEDDF_EUNSUPPORTED when V >= 2^31. */
int neddf_marching_cubes_bricks(neddf_ctx *ctx, const float *d_values, const int32_t *d_brick_ids, int64_t n_bricks, const int32_t *d_slot_map,
                                int nx, int ny, int nz, int brick, const double *h_lo, const double *h_hi, float iso, float *d_vertices,
                                int64_t vertex_cap, int32_t *d_triangles, int64_t triangle_cap, int64_t *d_vertex_key, int64_t *d_triangle_key,
                                int64_t *h_n_vertices, int64_t *h_n_triangles, void *stream);

/* Geometric vertex normals of an indexed mesh (no reference counterpart: its .dae export carries none): d_normals[v] = the
 * normalised sum, over the triangles that hold v, of (p1 - p0) x (p2 - p0) -- weighted by area, pointing where the triangles'
 * orientation points (out of the object for neddf_marching_cubes' meshes).  Cross products in fp32, sums in 64-bit fixed point with
 * integer atomics (exact, so the result does not depend on timing), normalisation in fp64; a sum shorter than 1e-20 gives (0,0,0).
 * Triangles with an index outside [0, n_vertices) or a non-finite cross product are ignored. */
int neddf_mesh_vertex_normals(neddf_ctx *ctx, const float *d_vertices, int64_t n_vertices, const int32_t *d_triangles,
                              int64_t n_triangles, float *d_normals, void *stream);

/* ---- mesh clean-up (additive to ABI v7; no reference counterpart) --------------------------------------------------
 * Connected components of an indexed mesh (d_triangles [T][3] int32 over n_vertices vertices): two vertices belong to one
 * component when a chain of triangles sharing vertices joins them.
 *   - components are numbered 0 .. C-1 in the order of their lowest vertex index
 *   - d_vertex_label [V] int32: the component of every vertex; -1 for a vertex no valid triangle references (not a component)
 *   - a triangle with an index outside [0, n_vertices) is ignored and gets label -1 (neddf_mesh_vertex_normals' rule);
 *     degenerate triangles (a, a, b) are valid and counted.  d_triangle_label [T] int32 may be NULL
 *   - d_component_triangles: int64, capacity n_vertices; entry c < C = the number of valid triangles of component c, the rest untouched
 *   - *h_n_components (HOST) = C.  T == 0 and V == 0 are legal and give C = 0
 *   - the output does not depend on timing: union-find on the device whose root is the lowest vertex of the set (atomicMin hooks,
 *     pointer jumping, repeated until a round changes nothing -- a unique fixed point whatever order the atomics land in), dense
 *     labels by flag / scan / gather, counts by integer atomic adds (exact)
 * Synchronises `stream` once per batch of 4 rounds and once at the end.  The iteration ends for every input; should it exceed
 * 256 rounds the call returns NEDDF_EUNSUPPORTED instead of going on (a marching-cubes tube 14 380 triangles long takes 7).
 * NEDDF_EUNSUPPORTED also for V >= 2^31. */
int neddf_mesh_components(neddf_ctx *ctx, const int32_t *d_triangles, int64_t n_triangles, int64_t n_vertices, int32_t *d_vertex_label,
                          int32_t *d_triangle_label, int64_t *d_component_triangles, int64_t *h_n_components, void *stream);
/* Rounds the last neddf_mesh_components call on this context ran (0 for an empty mesh); NEDDF_EINVAL for a NULL context. */
int neddf_mesh_components_rounds(neddf_ctx *ctx);
/* Order-preserving compaction: keeps the triangles whose d_keep_triangle [T] byte is non-zero and whose indices all lie in
 * [0, n_vertices), and exactly the vertices a kept triangle references.
 *   - both keep their relative order; d_out_triangles holds the kept triangles in the new vertex numbering
 *   - vertex coordinates are copied bit for bit (NaN payloads included); d_out_vertices must not overlap d_vertices
 *   - d_vertex_map [V] int32 (may be NULL): the new index of every vertex, -1 for a dropped one
 *   - the output does not depend on timing (count / scan / write launches; no atomics decide a position)
 * Two calls, as neddf_marching_cubes: with d_out_vertices or d_out_triangles NULL, or a cap below its count, only *h_n_vertices /
 * *h_n_triangles (HOST) are written; otherwise the mesh and d_vertex_map are too.  Synchronises `stream` once (to read the counts). */
int neddf_mesh_compact(neddf_ctx *ctx, const float *d_vertices, int64_t n_vertices, const int32_t *d_triangles, int64_t n_triangles,
                       const unsigned char *d_keep_triangle, float *d_out_vertices, int64_t vertex_cap, int32_t *d_out_triangles,
                       int64_t triangle_cap, int32_t *d_vertex_map, int64_t *h_n_vertices, int64_t *h_n_triangles, void *stream);

/* ---- empty-space skipping (additive to ABI v7; no reference counterpart: the reference evaluates every sample) ------
 * An occupancy grid of R^3 cells (R in [1, 1024]) over the box h_lo[3] .. h_hi[3] (HOST doubles), one bit per cell: cell
 * (x, y, z) has bit index (z R + y) R + x, bit i lives in word i >> 5 at position i & 31 of d_bits ((R^3 + 31) / 32 uint32 words),
 * the unused high bits of the last word are 0.  The caller fills the struct: lo = (float)h_lo, inv_cell = (float)(R / (h_hi -
 * h_lo)) per axis, the quotient taken in double. */
typedef struct {
    const uint32_t *d_bits;
    int res;                  /* R */
    float lo[3];
    float inv_cell[3];
} neddf_occupancy;
/* Builds the bitfield from d_volume, the [R+1]^3 lattice of cell-CORNER densities -- what neddf_field_grid(..., NEDDF_GRID_DENSITY,
 * R+1, R+1, R+1, lo, hi, ...) writes.  A cell is occupied when any of its 8 corners satisfies !(v <= threshold): a NaN corner
 * occupies its cells (the grid only ever removes work it is sure about).  The occupied set is then grown by `dilate` cells (0..4)
 * in the Chebyshev (26-neighbour) sense, clipped at the box.  Whole words are written, one lane per word and no atomics: the
 * result does not depend on timing.  *h_n_occupied (HOST) = the population count; synchronises `stream` once to read it. */
int neddf_occupancy_build(neddf_ctx *ctx, const float *d_volume, int R, float threshold, int dilate, uint32_t *d_bits,
                          int64_t *h_n_occupied, void *stream);
/* d_keep[i] (one byte, 0 / 1) for each of the N points d_pos [N,3]: per axis c = (int)floorf((p - lo) * inv_cell) in fp32, in
 * exactly that operation order; a point with a c outside [0, R) or a non-finite coordinate is KEPT (the grid claims nothing about
 * space it never looked at), any other point exactly when its cell's bit is set. */
int neddf_occupancy_classify(neddf_ctx *ctx, const neddf_occupancy *occ, const float *d_pos, int64_t n_points, unsigned char *d_keep,
                             void *stream);
/* Order-preserving compaction of the points whose d_keep byte is non-zero: their d_pos / d_dir / d_var rows ([N,3] each) are
 * copied bit for bit (NaN payloads included) to d_out_pos / d_out_dir / d_out_var and their old index to d_index (int32, strictly
 * increasing); all four need room for N rows.  *h_n_kept (HOST) = M; synchronises `stream` once to read it.  Count / scan / write
 * launches, no atomics.  NEDDF_EUNSUPPORTED for N >= 2^31. */
int neddf_occupancy_gather(neddf_ctx *ctx, const unsigned char *d_keep, const float *d_pos, const float *d_dir, const float *d_var,
                           int64_t n_points, float *d_out_pos, float *d_out_dir, float *d_out_var, int32_t *d_index,
                           int64_t *h_n_kept, void *stream);
/* The inverse: zero-fills d_density [N], d_color [N,3] and d_normal [N,3] (each may be NULL together with its source) and writes
 * row d_index[k] of each from row k < n_kept of the compact d_c_density [M], d_c_color [M,3], d_c_normal [M,3]. */
int neddf_occupancy_scatter(neddf_ctx *ctx, const int32_t *d_index, int64_t n_kept, int64_t n_points, const float *d_c_density,
                            const float *d_c_color, const float *d_c_normal, float *d_density, float *d_color, float *d_normal,
                            void *stream);
/* neddf_render_rays_surface / neddf_render_rays_single_surface with a trailing occupancy grid.  occ == NULL: the plain call.  With
 * a grid every pass writes its sampling tensors (neddf_sampling's kernel), classifies the sample positions, evaluates the field on
 * the kept points only and scatters the results; a culled sample has density 0, colour 0 and normal 0, and a pass in which nothing
 * is kept does not run the field.  Compositing is the plain call's.  One synchronise of `stream` per pass (the host learns the
 * number of kept points).  NEDDF_EUNSUPPORTED when a fields_penalty output is requested together with a grid. */
int neddf_render_rays_culled(neddf_ctx *ctx, const void *d_uv, int uv_type, int64_t n_rays, const neddf_camera *h_cam,
                             const neddf_render_params *params, const float *d_U_coarse, const float *d_U_fine,
                             const neddf_render_outputs *out, float *d_normal, float *d_normal_coarse, void *stream,
                             const neddf_occupancy *occ);
int neddf_render_rays_single_culled(neddf_ctx *ctx, int slot, const void *d_uv, int uv_type, int64_t n_rays,
                                    const neddf_camera *h_cam, const neddf_render_params *params, int S1, const float *d_U,
                                    const neddf_render_outputs *out, float *d_normal, void *stream, const neddf_occupancy *occ);
/* Running totals over the culled passes of this context: samples classified and samples kept (either pointer may be NULL);
 * reset != 0 zeroes them after reading. */
int neddf_cull_stats(neddf_ctx *ctx, int64_t *h_samples, int64_t *h_kept, int reset);

/* ---- sphere tracing (additive to ABI v7; no reference counterpart: the reference renders by volume integration only) ------
 * Rays o + t d march through a distance field D towards the level set D = threshold: where the distance is d the ray may advance
 * by step_scale * (d - threshold) without crossing it (exactly so for a 1-Lipschitz D and step_scale <= 1).  Per-ray state lives in
 * flat DEVICE arrays of n_rays entries, owned by the caller:
 *   d_t       float   current depth along the ray
 *   d_t_lo    float   last depth at which the distance was still above the threshold
 *   d_status  uint8   NEDDF_TRACE_*
 *   d_steps   int32   advances taken
 *   d_dist    float   last distance read
 * Every floating-point step below is one rounded fp32 operation in the order written (no fused multiply-add):
 * tests/trace_check.py restates all of it in numpy, bit for bit.  Compaction is count / scan / write launches with wave ballots, no
 * atomics: no output depends on timing.  Every entry point: NEDDF_EINVAL for a negative count or a NULL array it needs,
 * NEDDF_EUNSUPPORTED for n_rays >= 2^31 (indices are int32). */
enum { NEDDF_TRACE_ACTIVE = 0,      /* still marching */
       NEDDF_TRACE_HIT = 1,         /* reached the level set: D(t) <= threshold */
       NEDDF_TRACE_MISS = 2,        /* t passed t_far */
       NEDDF_TRACE_EXHAUSTED = 3,   /* still active after max_steps iterations */
       NEDDF_TRACE_INVALID = 4 };   /* non-finite origin or direction, or a NaN distance */
typedef struct {
    float threshold;          /* the level set */
    float t_near, t_far;      /* t_near < t_far */
    float step_scale;         /* in (0, 1]; below 1 for a field that is not 1-Lipschitz */
    float min_step;           /* > 0: the least advance */
    int max_steps;            /* 1..4096 marching iterations */
    int refine;               /* 0..32 bisection rounds on the HIT rays */
} neddf_trace_params;
/* t = t_lo = t_near, steps = 0, dist = NaN; status ACTIVE, or INVALID when a component of the ray's origin or direction is not finite. */
int neddf_trace_begin(neddf_ctx *ctx, const float *d_ray_orig, const float *d_ray_dir, int64_t n_rays, float t_near, float *d_t,
                      float *d_t_lo, unsigned char *d_status, int32_t *d_steps, float *d_dist, void *stream);
/* The ACTIVE rays in ascending order: their indices to d_index (int32) and their points pos = o + t * d to d_pos ([.,3]: the rounded
 * product, then the rounded sum); both need room for n_rays rows.  *h_n_active (HOST) = M; synchronises `stream` once to read it. */
int neddf_trace_compact(neddf_ctx *ctx, const float *d_ray_orig, const float *d_ray_dir, int64_t n_rays, const float *d_t,
                        const unsigned char *d_status, int32_t *d_index, float *d_pos, int64_t *h_n_active, void *stream);
/* One step of the rays r = d_index[k], k < n_active, from the distances d = d_distance[k] at their points, in this order:
 *   dist[r] = d;  d NaN: INVALID;  d <= threshold: HIT (t and t_lo stay);  otherwise t_lo = t,
 *   t = t + max(step_scale * (d - threshold), min_step), steps += 1, and MISS when !(t <= t_far).
 * An index outside [0, n_rays) is ignored; the indices must be distinct (neddf_trace_compact's are). */
int neddf_trace_advance(neddf_ctx *ctx, const int32_t *d_index, const float *d_distance, int64_t n_active, int64_t n_rays, float threshold,
                        float step_scale, float min_step, float t_far, float *d_t, float *d_t_lo, unsigned char *d_status, int32_t *d_steps,
                        float *d_dist, void *stream);
/* ACTIVE -> EXHAUSTED: the relabelling after the last marching iteration. */
int neddf_trace_finish(neddf_ctx *ctx, unsigned char *d_status, int64_t n_rays, void *stream);
/* Refinement of the HIT rays with t_lo < t by bisection of [t_lo, t].  _points: their indices (ascending) and the points at
 * mid = 0.5 * (t_lo + t), as neddf_trace_compact does for the ACTIVE rays (*h_n_points = M, one synchronise).  _update, with the
 * distances at those points: d <= threshold or d NaN: t = mid, dist = d; otherwise t_lo = mid.  D(t) <= threshold < D(t_lo) holds
 * after every round for a NaN-free field. */
int neddf_trace_bisect_points(neddf_ctx *ctx, const float *d_ray_orig, const float *d_ray_dir, int64_t n_rays, const float *d_t,
                              const float *d_t_lo, const unsigned char *d_status, int32_t *d_index, float *d_pos, int64_t *h_n_points,
                              void *stream);
int neddf_trace_bisect_update(neddf_ctx *ctx, const int32_t *d_index, const float *d_distance, int64_t n_points, int64_t n_rays,
                              float threshold, float *d_t, float *d_t_lo, float *d_dist, void *stream);
/* The whole loop on the distance (NeuS: sdf) of field slot `slot`: begin; at most max_steps iterations of compact -> field -> advance,
 * ended early once no ray is ACTIVE; finish; at most `refine` rounds of bisect_points -> field -> bisect_update, ended early once no
 * ray is left to refine.  The field is evaluated on the compacted points only, distance output alone (no colour kernel), dir = (1, 0, 0)
 * and var = 0 as neddf_field_grid passes them, under the slot's operand policy, in chunks of at most 2^23 points.  *h_evaluations
 * (HOST, may be NULL) = the number of points evaluated.  One synchronise of `stream` per iteration and per round (the host learns the
 * number of rays left).  NEDDF_EINVAL unless t_near < t_far, 0 < step_scale <= 1, min_step > 0, 1 <= max_steps <= 4096 and
 * 0 <= refine <= 32; NEDDF_EUNSUPPORTED for a NeRF field (no distance). */
int neddf_trace_field(neddf_ctx *ctx, int slot, const float *d_ray_orig, const float *d_ray_dir, int64_t n_rays,
                      const neddf_trace_params *params, float *d_t, float *d_t_lo, unsigned char *d_status, int32_t *d_steps, float *d_dist,
                      int64_t *h_evaluations, void *stream);

/* ---- distances between surfaces (additive to ABI v7; no reference counterpart: its evaluation compares images only) ------
 * Random numbers: hash(seed, t, k, w) = mix(mix(mix(mix(seed + 0x9e3779b9) ^ t) ^ k) + w * 0x85ebca6b) in uint32 arithmetic with
 * mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16; a uniform is (hash >> 8) * 2^-24.
 *
 * Surface samples of an indexed mesh (d_vertices [V][3] float, d_triangles [T][3] int32), `density` samples per unit area:
 *   - triangle t receives floor(A_t * density + u_t) samples, in fp64: A_t = 0.5 sqrt(|e1 x e2|^2) from the fp32 edges e1 = p1 - p0,
 *     e2 = p2 - p0 widened to double, u_t = uniform(seed, t, 0xffffffff, 2): floor(A density) or one more, A density on average
 *   - 0 for a triangle with an index outside [0, V), a non-finite vertex, a zero or non-finite area
 *   - sample k of triangle t: (a, b) = uniform(seed, t, k, 0 / 1), folded (a + b > 1: a = 1 - a, b = 1 - b), p = (p0 + a * e1) + b * e2
 *     per axis, every operation one rounded fp32 operation (no fused multiply-add, no square root)
 *   - order: triangle-major; d_points [N][3] float, d_triangle_id [N] int32.  Count / scan / write launches, no atomics: the output
 *     does not depend on timing or on the launch shape (tests/geometry_check.py restates it in numpy bit for bit)
 * _count writes *h_n_samples (HOST) = N; _write counts again and, with N > 0, needs both outputs and sample_cap >= N (NEDDF_EINVAL
 * otherwise).  Each synchronises `stream` once.  NEDDF_EINVAL also for a density that is negative or not finite and for N >= 2^31
 * (never a wrapped count); NEDDF_EUNSUPPORTED for V >= 2^31. */
int neddf_mesh_sample_count(neddf_ctx *ctx, const float *d_vertices, int64_t n_vertices, const int32_t *d_triangles, int64_t n_triangles,
                            double density, uint32_t seed, int64_t *h_n_samples, void *stream);
int neddf_mesh_sample_write(neddf_ctx *ctx, const float *d_vertices, int64_t n_vertices, const int32_t *d_triangles, int64_t n_triangles,
                            double density, uint32_t seed, float *d_points, int32_t *d_triangle_id, int64_t sample_cap,
                            int64_t *h_n_samples, void *stream);
/* Exact nearest neighbour of every query (d_queries [Q][3]) among the targets (d_targets [N][3]): d_d2 [Q] float, d_index [Q] int32.
 *   - d2 = (dx dx + dy dy) + dz dz with dx = qx - px, every operation one rounded fp32 operation
 *   - the result is the LOWEST target index that attains the minimal d2 (best starts at (+inf, -1); candidate j replaces it when
 *     d2 < best, or d2 == best and j is below the current index, -1 counting as highest): it does not depend on the visiting order
 *   - a target with a non-finite coordinate is never a candidate; a query with one gets (NaN, -1); no valid target: (+inf, -1)
 * neddf_nn_brute: one lane per query visits every target (tiles staged through LDS) -- the yardstick of the grid and the method for
 * small sets.  Q == 0 and N == 0 are legal.  NEDDF_EUNSUPPORTED for 2^31 points or more. */
int neddf_nn_brute(neddf_ctx *ctx, const float *d_queries, int64_t n_queries, const float *d_targets, int64_t n_targets, float *d_d2,
                   int32_t *d_index, void *stream);
/* A uniform grid of h_cells = (gx, gy, gz) cells, each in [1, 1024] and at most 2^24 in all (NEDDF_EINVAL above), over the box h_lo ..
 * h_hi (HOST doubles, finite, hi >= lo).  Per axis lo = (float)h_lo, inv_cell = (float)(g / (h_hi - h_lo)) with the quotient in double,
 * 0 for a zero-extent axis; cell = f >= g ? g - 1 : f > 0 ? (int)f : 0 with f = (p - lo) * inv_cell in fp32 (two rounded operations):
 * points outside the box land in border cells.  Cell (x, y, z) has index (z gy + y) gx + x.
 *   - d_cell_start int32 [G + 1]: the number of finite targets in the cells before each cell, [G] = all of them = *h_n_valid (HOST)
 *   - d_order int32 [capacity N]: the indices of the finite targets grouped by cell.  Histogram and placement use integer atomicAdd:
 *     d_cell_start does not depend on timing, the order INSIDE a cell may -- the query's result does not (the tie rule above)
 * Synchronises `stream` once. */
int neddf_nn_grid_build(neddf_ctx *ctx, const float *d_targets, int64_t n_targets, const double *h_lo, const double *h_hi, const int *h_cells,
                        int32_t *d_cell_start, int32_t *d_order, int64_t *h_n_valid, void *stream);
/* neddf_nn_brute's result, bit for bit, through the grid neddf_nn_grid_build made of the same targets, box and cells (any box, also one
 * that covers only part of the points): one lane per query visits the Chebyshev shells r = 0, 1, 2, ... of cells around the query's
 * (clamped) cell and stops after shell r once (r * safe_cell)^2 > best d2 and >= 1e-30, safe_cell = 0.99 * the smallest cell edge --
 * every target of a later shell is at least r smallest cell edges away, the 1 % covers every fp32 rounding involved -- or when the
 * shell has left the grid on all sides.  d_order may be NULL when the build listed no target (*h_n_valid == 0): every query then gets
 * (+inf, -1). */
int neddf_nn_grid_query(neddf_ctx *ctx, const float *d_queries, int64_t n_queries, const float *d_targets, int64_t n_targets,
                        const double *h_lo, const double *h_hi, const int *h_cells, const int32_t *d_cell_start, const int32_t *d_order,
                        float *d_d2, int32_t *d_index, void *stream);

/* ---- ray casting on meshes (additive to ABI v7; no reference counterpart: the reference looks at meshes through its Open3D viewer) ------
 * The first intersection of rays (d_ray_orig, d_ray_dir [R][3] float, directions of any length) with an indexed mesh (d_vertices [V][3]
 * float, d_triangles [T][3] int32), by the watertight test of Woop, Benthin and Wald (JCGT 2013).  Every operation below is ONE
 * rounded fp32 operation unless stated (no fused multiply-add; `/` is the correctly rounded division); tests/raycast_check.py
 * restates it in numpy bit for bit.
 *   per ray (o, d):  kz = the axis of the largest |d| (the lowest axis among equals), kx = (kz + 1) % 3, ky = (kx + 1) % 3, kx and ky
 *       swapped when d[kz] < 0;  Sz = 1 / d[kz], Sx = d[kx] * Sz, Sy = d[ky] * Sz
 *   per vertex P:    A = P - o;  Ax = A[kx] - Sx * A[kz], Ay = A[ky] - Sy * A[kz], Az = Sz * A[kz]   (B and C alike)
 *   edge functions:  U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax; when any of the three is exactly 0 all three
 *       are computed again with both products and the difference in fp64, then rounded to fp32
 *   the triangle is a CANDIDATE when U, V, W are all >= 0 or all <= 0 (two-sided: no back-face culling), det = (U + V) + W is not 0,
 *       t = ((U * Az + V * Bz) + W * Cz) / det satisfies t_min <= t <= t_max (a NaN fails every comparison), and the hit point
 *       p = o + t * d (per axis a rounded product, then a rounded sum) lies in the triangle's bounding box widened by pad on every
 *       side (the bounds min3 - pad and max3 + pad are one rounded operation each).  The box clause discards the garbage t of a nearly
 *       degenerate triangle, and it is what makes the grid equal to brute force (below)
 *   result per ray:  d_t, d_triangle (int32), d_b1 = V / det, d_b2 = W / det -- the hit point is p0 + b1 (p1 - p0) + b2 (p2 - p0).  The
 *       smallest t wins, among equal t the LOWEST triangle index (best starts at (+inf, -1, 0, 0); a candidate replaces it when
 *       t < best, or t == best and its index is below the current one, -1 counting as highest): the result does not depend on the
 *       visiting order.  No candidate: (+inf, -1, 0, 0).  A ray with a non-finite component or an all-zero direction: (NaN, -1, NaN,
 *       NaN).  A triangle with an index outside [0, V) or a non-finite vertex is never a candidate.
 * pad must be finite and >= 0 (NEDDF_EINVAL).  Every entry point: NEDDF_EINVAL for a negative count or a NULL array it needs,
 * NEDDF_EUNSUPPORTED from 2^31 rays, triangles or vertices on (indices are int32).
 * neddf_raycast_brute: one lane per ray visits every triangle (tiles staged through LDS) -- the yardstick of the grid and the method
 * for small meshes.  R == 0 and T == 0 are legal. */
int neddf_raycast_brute(neddf_ctx *ctx, const float *d_ray_orig, const float *d_ray_dir, int64_t n_rays, const float *d_vertices, int64_t n_vertices,
                        const int32_t *d_triangles, int64_t n_triangles, float t_min, float t_max, float pad, float *d_t, int32_t *d_triangle,
                        float *d_b1, float *d_b2, void *stream);
/* The grid: neddf_nn_grid_build's cells (h_lo, h_hi, h_cells: the same parameters, cell function and limits).  With wlo = (float)h_lo -
 * 2 pad and whi = (float)h_hi + 2 pad per axis (one rounded fp32 operation each; 2 pad is exact):
 *   - a valid triangle whose box widened by 2 pad, [min3 - 2 pad, max3 + 2 pad] (rounded likewise), lies in [wlo, whi] on every axis is
 *     listed in the cells cell(min3 - 2 pad) .. cell(max3 + 2 pad) per axis;
 *   - any other valid triangle is listed once, in the overflow list (index G = gx gy gz), which every ray tests by brute force: the
 *     result is right for ANY box.  A box that holds every vertex -- the mesh's own bounds -- leaves the list empty.
 * d_cell_start int32 [G + 2]: the number of (list, triangle) pairs before each list, [G + 1] = all of them = *h_n_items (HOST);
 * d_items int32 [item_cap]: the triangle indices grouped by list.  Count and placement use integer atomicAdd: d_cell_start does not
 * depend on timing, the order INSIDE a list may -- no result does (the tie rule).  _count returns the number of pairs; _build needs
 * item_cap >= that number (d_items may be NULL when it is 0), counts again, and returns NEDDF_EINVAL when the capacity is short or
 * the number reaches 2^31 (never a wrapped count).  Each of the two synchronises `stream` once.
 *
 * neddf_raycast_grid_query: neddf_raycast_brute's bits with the same pad, for any box, any cell counts and any rays, through the
 * lists _build made of the same mesh, box, cells and pad (n_items = its *h_n_items).  One lane per ray: the overflow list, then the
 * ray's [t_min, t_max] clipped to [wlo, whi] (fp64 slabs) and a 3D-DDA through the cells from the clipped start.  The parameter at
 * which the ray leaves cell i of an axis is computed afresh from the integer index in fp64, ((lo + (i + 1) * edge) - o) / d with
 * edge = 1 / (double)inv_cell, never accumulated; a border cell has no far side (the cell function clamps), so the walk ends at
 * the clipped end of the ray, or early once best t < t_exit - 1e-6 |t_exit|, t_exit the parameter at which the ray leaves the current cell.
 *
 * THE EQUALITY ARGUMENT.  Let a candidate of the brute kernel have parameter t and rounded hit point p.
 *   (1) p lies within pad of the triangle's box B (the box clause); the exact point p* = o + t d lies within eps_p of p, where eps_p <=
 *       2^-24 (|o| + 2 |p|) per axis is the rounding of the product and of the sum.
 *   (2) The triangle is listed in every cell that cell() assigns to a point of B widened by 2 pad (cell() is monotone per axis), or
 *       it is in the overflow list.  A listed triangle has B inside the box, so p* lies inside [wlo, whi] with pad - eps_p to spare
 *       and t inside the clipped range.
 *   (3) The walk's cells tile the clipped range: at parameter t it is in a cell whose ideal interval holds p* per axis up to the fp64
 *       rounding of the exit parameters, and cell()'s steps lie within 3 * 2^-24 of (extent + 4 pad) of the ideal ones.  Call the sum
 *       of the two delta.  As long as delta + eps_p + the rounding of the widened bounds (2^-24 of |coordinate|) < pad, a point within
 *       pad + eps_p of B that the walk places in cell c has c inside the listed range: the triangle is met.
 *   (4) Ending early is safe: a hit with t below the current cell's exit parameter lies in a cell already visited, by (3).
 * Hence NEDDF_EINVAL (_count, _build, _query) for a pad below 2^-16 times the largest of |lo|, |hi| and hi - lo over the axes: delta
 * and the bounds' rounding then stay below 2^-6 pad.  eps_p is the ray's: a ray whose origin has a coordinate beyond
 * 2^21 pad - 2 (that largest value + 2 pad) -- eps_p could pass pad / 8 -- does not walk the grid but visits every triangle.
 * Visiting more triangles, or one twice, never changes the result (the tie rule). */
int neddf_raycast_grid_count(neddf_ctx *ctx, const float *d_vertices, int64_t n_vertices, const int32_t *d_triangles, int64_t n_triangles,
                             const double *h_lo, const double *h_hi, const int *h_cells, float pad, int64_t *h_n_items, void *stream);
int neddf_raycast_grid_build(neddf_ctx *ctx, const float *d_vertices, int64_t n_vertices, const int32_t *d_triangles, int64_t n_triangles,
                             const double *h_lo, const double *h_hi, const int *h_cells, float pad, int32_t *d_cell_start, int32_t *d_items,
                             int64_t item_cap, int64_t *h_n_items, void *stream);
int neddf_raycast_grid_query(neddf_ctx *ctx, const float *d_ray_orig, const float *d_ray_dir, int64_t n_rays, const float *d_vertices, int64_t n_vertices,
                             const int32_t *d_triangles, int64_t n_triangles, const double *h_lo, const double *h_hi, const int *h_cells, float pad,
                             const int32_t *d_cell_start, const int32_t *d_items, int64_t n_items, float t_min, float t_max, float *d_t,
                             int32_t *d_triangle, float *d_b1, float *d_b2, void *stream);

/* ---- point-to-mesh distance (additive to ABI v7; no reference counterpart: its evaluation compares images only) ------
 * The closest point of an indexed mesh (d_vertices [V][3] float, d_triangles [T][3] int32) to every query (d_queries [Q][3] float):
 * d_d2 [Q] float, the squared distance; d_triangle [Q] int32, the closest triangle; d_b1, d_b2 [Q] float -- the closest point is
 * p0 + b1 (p1 - p0) + b2 (p2 - p0).  Every operation below is ONE rounded fp32 operation (no fused multiply-add; `/` is the correctly
 * rounded division); dot(x, y) = (x0 y0 + x1 y1) + x2 y2; tests/pointmesh_check.py restates it in numpy bit for bit.
 *   per valid triangle (indices in [0, V), finite vertices; a, b, c its corners):
 *       e0 = b - a, e1 = c - a, e2 = c - b;  g00 = dot(e0, e0), g01 = dot(e0, e1), g11 = dot(e1, e1), g22 = dot(e2, e2);
 *       r00 = 1 / g00, r11 = 1 / g11, r22 = 1 / g22;  f = e1 - (g01 * r00) * e0 per axis (e1 without its part along e0), gpp = dot(f, f),
 *       rpp = 1 / gpp -- the only four divisions, none per pair
 *   per (query p, triangle):  ap = p - a, bp = p - b, d1 = dot(e0, ap), d2 = dot(e1, ap), d3 = dot(e2, bp);
 *       clamp01(u) = u > 0 ? (u < 1 ? u : 1) : 0 (a NaN gives 0: a zero-length edge, r = inf and h = 0, gives its start point)
 *       edge candidates (s, e, h, r) = (a, e0, d1, r00), (b, e2, d3, r22), (a, e1, d2, r11):  u = clamp01(h * r), q = s + u * e per axis (a
 *           rounded product, then a rounded sum), d = p - q, D2 = dot(d, d); (b1, b2) = (u, 0), (1 - u, u), (0, u)
 *       interior candidate:  solve(x, h) = (v, w) with w = dot(f, x) * rpp, v = (h - w * g01) * r00.  (v, w) = solve(ap, d1);
 *           q = (a + v * e0) + w * e1, d = p - q; ONE step of iterative refinement: (dv, dw) = solve(d, dot(e0, d)), v = v + dv,
 *           w = w + dw, and q, d again.  It exists when gpp > 0, v > 0, w > 0 and v + w < 1;  D2 = dot(d, d), (b1, b2) = (v, w).
 *           (Solving the 2 x 2 Gram system by its determinant g00 * g11 - g01 * g01 squares the triangle's aspect ratio in the error
 *           of (v, w): measured against fp64, samples of a marching-cubes mesh then lie up to 80 * 2^-24 off their OWN triangles, and
 *           2500 * 2^-24 at an aspect of 1:300.  Orthogonalising first -- a QR step in place of the normal equations -- makes the
 *           amplification linear, and the refinement squares what is left: within 4 * 2^-24 down to an aspect of 1:10000.  Thinner
 *           triangles may lose the candidate; the edge candidates are then within the triangle's height of the truth.)
 *       corner candidate:  d = p - c, D2 = dot(d, d), (b1, b2) = (0, 1).  The corners a and b are reached without rounding by u = 0 of
 *           the edges ab and bc; c is reached by no edge candidate exactly (u = g * (1 / g) may round below 1, and a + 1 * (c - a) need
 *           not give c back), so without this candidate a mesh vertex would be at distance 0 of only SOME of its triangles
 *       the pair's result starts at (+inf, 0, 0) and is replaced by the interior candidate, then by the edge candidates in the order
 *           ab, bc, ac, then by the corner candidate, each when its D2 is strictly smaller: a D2 that is NaN (or +inf) never replaces
 *           anything.  A mesh vertex is therefore at distance exactly 0 of every triangle it is a corner of, and the lowest one wins
 *   per query:  the smallest D2 wins, among equal D2 the LOWEST triangle index (best starts at (+inf, -1, 0, 0); a pair replaces it
 *       when D2 < best, or D2 == best and its index is below the current one, -1 counting as highest): the result does not depend on
 *       the visiting order or on how often a triangle is met.  A query with a non-finite coordinate: (NaN, -1, NaN, NaN).  No valid
 *       triangle: (+inf, -1, 0, 0).
 * Every candidate is a point of the triangle up to rounding -- a clamped point of a segment or a convex combination of the corners --
 * so a sliver or a degenerate triangle cannot give a gross underestimate: at worst it loses its interior candidate, and the edge
 * candidates are then within the triangle's smallest height of the truth.
 * Every entry point: NEDDF_EINVAL for a negative count or a NULL array it needs, NEDDF_EUNSUPPORTED from 2^31 queries, triangles or
 * vertices on (indices are int32).
 * neddf_point_mesh_brute: one lane per query visits every triangle; the per-triangle constants are computed once per 256-triangle tile
 * and staged through LDS -- the yardstick of the grid and the method for small meshes.  Q == 0 and T == 0 are legal. */
int neddf_point_mesh_brute(neddf_ctx *ctx, const float *d_queries, int64_t n_queries, const float *d_vertices, int64_t n_vertices,
                           const int32_t *d_triangles, int64_t n_triangles, float *d_d2, int32_t *d_triangle, float *d_b1, float *d_b2, void *stream);
/* neddf_point_mesh_brute's bits, for any box, any cell counts and any queries, through the lists neddf_raycast_grid_build made of the
 * same mesh, box, cells and pad (n_items = its *h_n_items; the pad limit and every other parameter rule are the build's): no build and
 * no list format of its own.  A prepare launch writes the per-triangle constants into a table in the context's workspace (80 bytes
 * per triangle), then one lane per query visits the overflow list and the Chebyshev shells r = 0, 1, 2, ... of cells around the
 * query's (clamped) cell, as neddf_nn_grid_query does, and stops after shell r once (r * safe_cell)^2 > best D2 strictly and
 * (r * safe_cell)^2 >= 1e-30, safe_cell = 0.99 * the smallest cell edge among the axes with an extent, or when the shell has left the
 * grid on all sides.  A triangle listed in several visited cells is evaluated again, which the tie rule makes harmless.
 *
 * THE EQUALITY ARGUMENT.  Let the walk stop after shell r >= 1 with best D2 = B, and let a listed triangle be unvisited.
 *   (1) On some axis its whole listed cell range lies outside [c - r, c + r], c the query's cell.  cell() is monotone and the range
 *       covers cell(min3 - 2 pad) .. cell(max3 + 2 pad), so every point of the triangle lies in a cell at least r + 1 from c along that
 *       axis; cell()'s steps lie within 2^-12 cells of the ideal ones (neddf_nn_grid_build), also for a query outside the box that was
 *       clamped.  Every point of the triangle is therefore more than (r - 2^-12) e from the query, e the smallest cell edge.
 *   (2) A candidate's D2 comes from a point q that carries an ABSOLUTE error: per axis the rounding of the edge (2^-24 |e|, |e| <= 2 W),
 *       of each product and of each sum (2^-24 W each, W the largest |coordinate| of the widened box wlo .. whi, which holds every
 *       vertex of a listed triangle) -- at most nine such terms for the interior candidate, five for an edge candidate, none for the corner; over three
 *       axes less than 2^-20 W < 2^-19 W.  d = p - q and dot(d, d) add relative errors only, below 2^-21 of the distance.  The computed
 *       distance of the unvisited triangle is therefore above (r - 2^-12) e (1 - 2^-21) - 2^-19 W.
 *   (3) The walk stopped because (0.99 r e)^2, computed with relative error below 2^-22, exceeds B.  The unvisited D2 exceeds B as
 *       well -- no tie, no smaller value -- when r e (0.01 - 2^-12 - 2^-20) > 2^-19 W; the bracket exceeds 2^-7, so e >= 2^-12 W would
 *       do.  The query walks the shells only when e >= 2^-10 W (a margin of four); otherwise it visits every list once, the
 *       overflow list included, which is the brute kernel's set of valid triangles.
 * The overflow list is visited before the shells in either case.  Visiting more triangles, or one twice, never changes the result. */
int neddf_point_mesh_grid_query(neddf_ctx *ctx, const float *d_queries, int64_t n_queries, const float *d_vertices, int64_t n_vertices,
                                const int32_t *d_triangles, int64_t n_triangles, const double *h_lo, const double *h_hi, const int *h_cells, float pad,
                                const int32_t *d_cell_start, const int32_t *d_items, int64_t n_items, float *d_d2, int32_t *d_triangle, float *d_b1,
                                float *d_b2, void *stream);

/* ---- a BVH over the triangles, and the point-to-mesh distance through it (additive to ABI v7; no reference counterpart) ------
 * neddf_point_mesh_brute's bits for ANY query, near the surface or far from it, through a linear BVH (Karras 2012) of the mesh.  The
 * per-pair arithmetic, the per-triangle constants and the tie rule are the block's above; only the set of visited triangles differs.
 * Three steps: neddf_bvh_keys, an ascending sort of the keys by the caller (they are distinct, so every correct sort gives one order),
 * neddf_bvh_build.  Argument rules as above: NEDDF_EINVAL for a negative count or a NULL array that is needed, NEDDF_EUNSUPPORTED from
 * 2^31 queries, triangles or vertices on.  T == 0 and Q == 0 are legal everywhere.
 *
 * neddf_bvh_keys: d_keys int64 [T].  A triangle is valid by the rule above (indices in [0, V), finite vertices).  A valid one:
 *     centre = (min3 + max3) * 0.5 per axis (one rounded fp32 sum, an exact halving); cell per axis by neddf_nn_grid_build's cell
 *     function with 1024 cells over the box h_lo .. h_hi (HOST doubles, finite, hi >= lo; any box gives a correct tree -- the cell
 *     function clamps -- the bounds of the valid triangles' vertices the best one); code = the 30-bit Morton code of (cx, cy, cz), bit
 *     3 b + a of the code = bit b of the cell along axis a; key = code << 32 | j.  An invalid one: key = 2^62 | j -- it sorts behind
 *     every valid triangle and stays in the tree (which therefore always has T leaves) with an EMPTY box, which is never entered.
 * neddf_bvh_build, from the keys sorted ascending -- THE TREE, for both traversals (points here, rays in neddf_raycast_bvh_query below):
 *     d_leaf_triangle int32 [T]      the triangle of leaf k: the low 32 bits of sorted key k (Morton order)
 *     d_children int32 [T - 1][2]    left and right child of internal node i (NULL allowed for T <= 1); c >= 0 is internal node c, c < 0
 *                                    is leaf ~c.  Node 0 is the root; T == 1 has no internal node, the root is leaf 0.  Node i covers a
 *                                    contiguous range of leaves, the left child the lower part; depth <= 62 (62 key bits can differ).
 *                                    delta(i, j) = the number of leading bits that the 64-bit keys i and j share, -1 for j outside [0, T)
 *     d_boxes float [2 T - 1][6]     (lo.xyz, hi.xyz): internal node i at row i, leaf k at row T - 1 + k, so row 0 is the root's.  A
 *                                    leaf's box is the exact min / max of its corners, (+inf x 3, -inf x 3) for an invalid triangle;
 *                                    a node's is the min / max of its children's: exact fp32, independent of timing although the
 *                                    boxes are fitted bottom-up with one integer atomic counter per node (the second arriver goes on)
 * neddf_point_mesh_bvh_query: n_leaves must equal n_triangles (NEDDF_EINVAL: a tree of another mesh is refused, not followed).  One
 * lane per query, depth first.  A box (node or leaf) against query p, every operation ONE rounded fp32 operation:
 *     gap_a = max(max(lo_a - p_a, p_a - hi_a), 0) per axis;  lb = sqrt(dot(gap, gap));  m = f * lb - s;  m2 = m * m
 *     f = 1 - 2^-16;  s = 2^-18 * W, W = the largest |coordinate| of the root box
 *     the box is SKIPPED when it is empty (lo.x > hi.x), or when m > 0 and m2 > best D2 strictly and 1e-30 <= m2 < +inf
 * Of two children that are not skipped, the one with the smaller m2 (m <= 0 counting as 0) is entered first, the left one on a tie;
 * the other waits on a stack and is tested again, against the best of that moment, when its turn comes.  A leaf that is entered is
 * evaluated with its ORIGINAL triangle index.  d_visits int32 [Q] (NULL allowed): the leaves evaluated per query (0 for a non-finite
 * query) -- tests/bvh_check.py restates keys, tree and traversal in numpy and reproduces this count exactly.  Child and triangle
 * indices are checked before they are followed and a query handles at most 2 T nodes: a corrupt tree gives a wrong answer, no hang.
 *
 * THE EQUALITY ARGUMENT.  Let a box be skipped by the rule with best D2 = B, and let a valid triangle lie below it.
 *   (1) Boxes are exact min / max of vertex coordinates, so every point of the triangle lies in the box, and its true distance d from
 *       p is at least L, the true distance from p to the box.  The computed lb: each gap is one subtraction (relative error 2^-24; the
 *       max with 0 is exact), dot(gap, gap) is three products and two sums of non-negative terms (relative error below 5 * 2^-24 in
 *       all, the gaps' included), the square root halves that and adds 2^-24: lb <= L (1 + 2^-22).  Underflow only lowers lb.
 *   (2) m = f * lb - s and m2 = m * m add three roundings: with m > 0, sqrt(m2) <= (f L (1 + 2^-22) - s) (1 + 2^-23)
 *       <= L (1 - 2^-16 + 2^-21) - s ((x - s) (1 + e) <= x (1 + e) - s: the roundings only shrink the part of s).  s = 2^-18 W is a
 *       scaling by a power of two, exact.
 *   (3) Step (2) of the grid's argument above: a candidate's computed distance is above d (1 - 2^-21) - 2^-19 W, W the largest
 *       |coordinate| of a box that holds every vertex of the triangles in question -- here the root box, which holds every valid one.
 *   (4) So sqrt(computed D2) - sqrt(m2) > L (2^-16 - 2^-20) + (2^-18 - 2^-19) W > 0: the skipped triangle's D2 exceeds m2,
 *       which exceeds B strictly -- no tie and no smaller value among the skipped, at a relative margin of 2^-16 against roundings of
 *       2^-21.  1e-30 <= m2 keeps the margin above the absolute error of a D2 whose products underflow (3 * 2^-126); m2 < +inf
 *       leaves alone the range where the bound itself has overflowed.
 *   (5) best only decreases, so a box skipped once would be skipped later too; visiting more triangles never changes the result (the
 *       tie rule).  Hence the bits are the brute kernel's, whatever the order.
 * (The grid's factor 0.99 would not do here: 100 mesh sizes away everything is within 1 % of everything else, and a query would
 * visit most of the mesh.  Where rounding dominates -- a mesh of size 2^-8 at offset 1000, s as large as the mesh -- nearly every
 * triangle is visited, as the grid stops walking there.) */
int neddf_bvh_keys(neddf_ctx *ctx, const float *d_vertices, int64_t n_vertices, const int32_t *d_triangles, int64_t n_triangles, const double *h_lo,
                   const double *h_hi, int64_t *d_keys, void *stream);
int neddf_bvh_build(neddf_ctx *ctx, const float *d_vertices, int64_t n_vertices, const int32_t *d_triangles, int64_t n_triangles,
                    const int64_t *d_sorted_keys, int32_t *d_leaf_triangle, int32_t *d_children, float *d_boxes, void *stream);
int neddf_point_mesh_bvh_query(neddf_ctx *ctx, const float *d_queries, int64_t n_queries, const float *d_vertices, int64_t n_vertices,
                               const int32_t *d_triangles, int64_t n_triangles, const int32_t *d_leaf_triangle, const int32_t *d_children,
                               const float *d_boxes, int64_t n_leaves, float *d_d2, int32_t *d_triangle, float *d_b1, float *d_b2, int32_t *d_visits,
                               void *stream);

/* ---- rays through the BVH: first hit and any hit (additive to ABI v7; no reference counterpart) ------
 * neddf_raycast_brute's bits with the same pad, for ANY rays and any pad >= 0, through the tree of neddf_bvh_build: one accelerator for
 * the distance queries above and for ray casts.  The per-pair arithmetic (the hit definition of the ray-casting block) and the tie rule
 * are unchanged; only the set of visited triangles differs.  n_leaves must equal n_triangles.  One lane per ray, depth first, the tree
 * arrays validated and the walk bounded by 2 T nodes exactly as in neddf_point_mesh_bvh_query.
 *
 * THE BOX TEST, all fp64, every operation ONE rounded fp64 operation.  Per ray: rcp_a = 1 / (double)d_a for every axis with d_a != 0.
 * Per box row (lo, hi) and axis a:
 *     wl_a = (double)lo_a - 2 (double)pad,  wh_a = (double)hi_a + 2 (double)pad      (2 (double)pad is exact)
 *     ta = (wl_a - o_a) * rcp_a,  tb = (wh_a - o_a) * rcp_a
 *     an axis with d_a == 0 contributes no ta, tb; it EMPTIES the interval when o_a < wl_a or o_a > wh_a
 *     te = max(t_min, max_a min(ta, tb)),  tx = min(t_max, min_a max(ta, tb))        (max / min that ignore a NaN operand: fmax, fmin)
 * The box is SKIPPED when it is empty (lo.x > hi.x), when the interval is empty, !(te <= tx), or when te > (double)best t strictly.
 * Of two children that are not skipped, the one with the smaller te is entered first, the left one on a tie; the other waits on the
 * stack and is tested again, against the best of that moment, when it is popped.  A leaf that is entered is evaluated with its
 * ORIGINAL triangle index (an invalid triangle has an empty box and is never evaluated).
 *
 * NO WALK.  With W = the largest |coordinate| of the root box (row 0, fp32, read on the device), a ray visits every valid triangle in
 * index order -- the brute kernel's set -- instead of walking the tree when (fp64, one rounded operation each)
 *     pad < 2^-16 W,  or  pad < 2^-126 (zero or subnormal),  or  max_a |o_a| > 2^21 pad - 2 (W + 2 pad).
 * The first and the last are the grid's two conditions (what neddf_raycast_grid_* refuses or routes past its cells); here both are
 * decided per ray on the device, so every pad >= 0 gives the right answer.  An all-invalid mesh has W = +inf: no walk, no visit.
 *
 * neddf_raycast_bvh_query: d_t, d_triangle, d_b1, d_b2 as neddf_raycast_brute writes them; a ray with a non-finite component or an
 * all-zero direction gets (NaN, -1, NaN, NaN).  neddf_raycast_bvh_occluded: the ANY-HIT mode of the same kernel -- the ray stops at
 * its first candidate (in the walk and in the every-triangle route alike); d_occluded uint8 [R] = 1 when there is one, which is
 * exactly `d_triangle >= 0` of neddf_raycast_brute, 0 otherwise and for an invalid ray.  d_visits int32 [R] (NULL allowed): the leaves
 * evaluated -- the valid triangles evaluated on the every-triangle route (all of them for the first hit), 0 for an invalid ray;
 * tests/bvh_raycast_check.py restates the traversal in numpy and reproduces the count exactly.  R == 0 and T == 0 are legal;
 * d_children may be NULL for T <= 1.  Before the first HIP call: NEDDF_EINVAL for a NULL context, a negative count, a NULL array that is
 * needed, n_leaves != n_triangles, a pad that is negative or not finite; NEDDF_EUNSUPPORTED from 2^31 rays, triangles or vertices on.
 *
 * THE EQUALITY ARGUMENT.  Let a ray walk the tree, and let a valid triangle be a candidate of the brute kernel with computed parameter
 * t (fp32, finite: an infinite t fails the box clause) and rounded hit point p.  W holds every coordinate of every valid triangle.
 *   (1) The box clause: p lies within pad of the triangle's box B on every axis, up to the rounding of the bounds min3 - pad and
 *       max3 + pad, at most 2^-24 (W + pad) <= (2^-8 + 2^-24) pad since W <= 2^16 pad.  So |p_a| <= W + 1.01 pad.
 *   (2) The exact point p* = o + t d at the COMPUTED t lies within eps_p of p per axis: the rounding of the product (2^-24 |t d_a| <=
 *       2^-24 (|p_a| (1 + 2^-23) + |o_a|)) and of the sum (2^-24 |p_a|), so eps_p <= 2^-24 (|o_a| + 2.01 |p_a|), plus at most 2^-149 where the
 *       product underflows.  With |o_a| <= 2^21 pad - 2 W - 4 pad: eps_p <= 2^-24 (2^21 pad + 0.01 W) + 2^-149 <= pad / 8 + 2^-14 pad
 *       (pad >= 2^-126 puts the underflow term below 2^-23 pad).
 *   (3) Node boxes are exact min / max of vertex coordinates, so B lies inside the box of every ancestor, the leaf's own included.
 *       wl and wh carry one fp64 rounding each, below 2^-52 (W + 2 pad) <= 2^-35 pad.  Hence on every axis
 *       wl_a + 0.86 pad < p*_a < wh_a - 0.86 pad  (2 - 1 - 2^-8 - 1/8 - 2^-14 - 2^-35 > 0.86): the exact point lies inside every
 *       ancestor's widened box with more than 0.8 pad to spare.
 *   (4) An axis with d_a == 0 has p*_a = o_a, inside [wl_a, wh_a]: it does not empty the interval.  On an axis with d_a != 0, t lies
 *       between the exact (wl_a - o_a) / d_a and (wh_a - o_a) / d_a and is more than 0.8 pad / |d_a| away from both.  The computed ta and tb
 *       carry three fp64 roundings (the difference, the reciprocal, the product): below 2^-51 |wl_a - o_a| / |d_a| <= 2^-51 2^21 pad / |d_a|
 *       = 2^-30 pad / |d_a| -- smaller by eight orders of magnitude.  And t_min <= t <= t_max by the candidate's own range clause, exactly
 *       (a float converts to double without rounding).
 *   (5) Hence (double)t lies inside the computed [te, tx] of every ancestor: no ancestor is skipped for an empty interval, and one that
 *       is skipped with te > best t has t >= te > best t strictly -- the candidate neither ties nor wins.
 *   (6) best t only decreases, so a box skipped once would be skipped later too, and a child dropped when its parent was handled would
 *       have been dropped when popped.  Visiting more triangles, in any order, never changes the result (the tie rule).
 * Hence the walk returns the brute kernel's bits; a ray that does not walk visits the brute kernel's set.  In the any-hit mode best t
 * stays +inf until the ray stops, so no box that holds a candidate is skipped: the flag is 1 exactly when the brute kernel has a
 * candidate at all, that is, when it reports a triangle. */
int neddf_raycast_bvh_query(neddf_ctx *ctx, const float *d_ray_orig, const float *d_ray_dir, int64_t n_rays, const float *d_vertices, int64_t n_vertices,
                            const int32_t *d_triangles, int64_t n_triangles, const int32_t *d_leaf_triangle, const int32_t *d_children,
                            const float *d_boxes, int64_t n_leaves, float t_min, float t_max, float pad, float *d_t, int32_t *d_triangle, float *d_b1,
                            float *d_b2, int32_t *d_visits, void *stream);
int neddf_raycast_bvh_occluded(neddf_ctx *ctx, const float *d_ray_orig, const float *d_ray_dir, int64_t n_rays, const float *d_vertices,
                               int64_t n_vertices, const int32_t *d_triangles, int64_t n_triangles, const int32_t *d_leaf_triangle,
                               const int32_t *d_children, const float *d_boxes, int64_t n_leaves, float t_min, float t_max, float pad,
                               uint8_t *d_occluded, int32_t *d_visits, void *stream);

/* ---- mesh simplification by vertex clustering (additive to ABI v7; no reference counterpart: its users decimated in Open3D) ------
 * Opt-in: a grid of cells is laid over the mesh, the vertices of a cell become one vertex, the triangles that collapse go.  Integer
 * structure by count / scan / write, every floating-point step ONE rounded operation in a fixed order (no fused multiply-add, no float
 * atomic): one answer per input on every run; tests/simplify_check.py restates all of it in numpy bit for bit.  The steps, with the
 * caller's sorts between them (the keys of each sort are distinct or the sort is stable, so every correct sort gives one order):
 *     neddf_mesh_simplify_keys -> sort ascending -> neddf_mesh_simplify_clusters -> [neddf_mesh_simplify_pairs -> sort ascending] ->
 *     neddf_mesh_simplify_place [-> neddf_mesh_simplify_attributes] -> neddf_mesh_simplify_triangles -> order by triple ->
 *     neddf_mesh_simplify_unique -> neddf_mesh_compact(representatives, mapped triangles, keep flags)
 * Input: d_vertices float [V][3], d_triangles int32 [T][3].  V == 0, T == 0 and a result without any triangle are legal everywhere.
 * Every entry point: NEDDF_EINVAL for a negative count, a NULL array it needs or a parameter outside its range, NEDDF_EUNSUPPORTED from
 * 2^31 vertices or triangles on.  An index read from a sorted array is checked before it is followed: arrays that are not what the
 * earlier steps made give a wrong answer, never an access outside them.
 *
 * GRID.  h_cells = (gx, gy, gz), each in [1, 1024], over the box h_lo .. h_hi (HOST doubles, finite, hi >= lo; mesh.simplify_mesh's
 * default: the bounds of the finite vertices).  The cell of a coordinate is neddf_nn_grid_build's cell function unchanged: lo =
 * (float)h_lo, inv_cell = (float)(cells / (h_hi - h_lo)) with the quotient in double, 0 for an axis without extent; f = (p - lo) *
 * inv_cell in two rounded fp32 operations; cell = f >= cells ? cells - 1 : (f > 0 ? (int)f : 0) -- points outside the box are clamped
 * into its border cells.  No per-cell array exists, so that build's limit of 2^24 cells in all does not apply.
 * KEYS (neddf_mesh_simplify_keys: d_keys int64 [V]).  A finite vertex i: ((cz gy + cy) gx + cx) << 32 | i.  A vertex with a non-finite
 * coordinate: 2^62 | i.  The keys are distinct.
 * CLUSTERS (neddf_mesh_simplify_clusters, from the keys sorted ascending).  A cluster is a run of keys with equal high words; a key with
 * bit 62 set is a run of its own (a non-finite vertex is never merged).  Its members appear in ascending vertex index, its head is
 * its lowest vertex index, and clusters are numbered in the order of their heads: when no two vertices share a cell, cluster i is
 * vertex i and the whole simplification is the identity.  d_vertex_cluster int32 [V]: the cluster of every vertex; d_cluster_range
 * int32 [capacity V][2]: the [begin, end) of cluster c among the sorted keys, the first C rows written; *h_n_clusters = C (HOST; the
 * call synchronises `stream` once).
 * PLACEMENT (neddf_mesh_simplify_place: d_out float [C][3]).  A cluster of ONE member, finite or not, gets that vertex' bits.  Otherwise
 *   NEDDF_SIMPLIFY_MEAN:  per axis the members are summed in fp64 in ascending member order (the sum starts at +0.0),
 *       m = sum / (double)count, the result rounded once to fp32.
 *   NEDDF_SIMPLIFY_QUADRIC:  m as above, unrounded.  For every VALID triangle (indices in [0, V), finite corners) with at least one
 *       corner in the cluster, once each, in ascending triangle index, the ones that will collapse included -- the pairs of
 *       neddf_mesh_simplify_pairs sorted ascending -- with p0, p1, p2 its corners converted to fp64:
 *           u = p1 - p0, w = p2 - p0;  n = (u.y w.z - u.z w.y, u.z w.x - u.x w.z, u.x w.y - u.y w.x)
 *           a00 += n.x n.x, a01 += n.x n.y, a02 += n.x n.z, a11 += n.y n.y, a12 += n.y n.z, a22 += n.z n.z
 *           d = (n.x (p0.x - m.x) + n.y (p0.y - m.y)) + n.z (p0.z - m.z);  r += n * d per axis
 *       n is deliberately not normalised: the weight is the squared area, there is no square root, and the only divisions are the
 *       solve's.  Then (A + lambda I) y = r by the adjugate:
 *           tr = (a00 + a11) + a22;  lambda = (regularisation * tr) / 3;  b00 = a00 + lambda, b11 = a11 + lambda, b22 = a22 + lambda
 *           c00 = b11 b22 - a12 a12;  c01 = a02 a12 - a01 b22;  c02 = a01 a12 - a02 b11
 *           c11 = b00 b22 - a02 a02;  c12 = a01 a02 - b00 a12;  c22 = b00 b11 - a01 a01
 *           det = (b00 c00 + a01 c01) + a02 c02
 *           y0 = ((c00 r0 + c01 r1) + c02 r2) / det;  y1 = ((c01 r0 + c11 r1) + c12 r2) / det;  y2 = ((c02 r0 + c12 r1) + c22 r2) / det
 *       x = m + y; x = m instead when tr is 0 or non-finite, det is 0 or non-finite, or a component of y is non-finite.  Each axis of x
 *       is then clamped to the [min, max] of the members' coordinates on that axis (max(x, min) first, then min(., max)) and rounded
 *       to fp32.  regularisation (finite, >= 0; mesh.simplify_mesh's default 2^-10) is a knob, not a tolerance: it pulls x towards m
 *       where the planes of a flat cluster leave a direction undetermined.
 *   neddf_mesh_simplify_pairs: every valid triangle contributes one pair per DISTINCT cluster among its corners, cluster << 32 |
 *       triangle, by count / scan / write in triangle order (within a triangle in corner order); *h_n_pairs = their number (HOST, one
 *       synchronise); nothing is written while d_pairs is NULL or pair_cap is below it (the counting call).
 * ATTRIBUTES (neddf_mesh_simplify_attributes: d_attributes float [V][k] -> d_out float [C][k], 1 <= k <= 1024; normals, colours).  Under
 * either placement: a cluster of one member gets its bits; otherwise each column is the fp64 mean in member order as above, rounded
 * once to fp32, a NaN result written as 0x7fc00000.  Nothing is renormalised.
 * TRIANGLES (neddf_mesh_simplify_triangles: d_mapped int32 [T][3], d_lowest int32 [T], d_keys int64 [T]).  A triangle with an index
 * outside [0, V) is dropped (a non-finite corner does NOT drop it: that vertex is its own cluster).  The corners are replaced by their
 * clusters, d_mapped; a triangle with two equal clusters is dropped.  The rest are rotated cyclically so that the lowest cluster
 * comes first, which keeps the orientation: the rotated triple (a, b, c) is the triangle's IDENTITY, d_lowest = a, d_keys = b << 31 |
 * c.  A dropped one: (-1, -1, -1), -1 and -1.  d_mapped keeps the input's corner order -- the rotation decides which triangles are
 * the same, it does not reorder the output -- so that a simplification that merges nothing returns the triangles as they came.
 *   neddf_mesh_simplify_unique: d_order int64 [T] lists the triangles by ascending (a, b, c), equal triples by ascending index (a
 *   STABLE sort by d_keys, then a stable sort by d_lowest); d_keep_triangle [T] bytes: 1 for the first of every run of equal triples
 *   that is not a dropped one -- among triangles with the same rotated triple only the lowest original index survives.  Opposite
 *   orientations are different triples and both stay.
 * COMPACTION.  neddf_mesh_compact over (d_out of _place as vertices, d_mapped as triangles, d_keep_triangle) drops the clusters that
 * no surviving triangle references and renumbers the rest in order; survivors keep the input order.  With its vertex map M over the
 * clusters, vertex_map[v] = M[d_vertex_cluster[v]] (or -1) and triangle_map[t] = the rank of t among the kept triangles (or -1).
 *
 * THE DISPLACEMENT BOUND.  Let e_a = (h_hi_a - h_lo_a) / cells_a be the cell edges and D = sqrt(e_x^2 + e_y^2 + e_z^2) the diagonal.
 *   (1) A representative lies in the per-axis [min, max] of its members: the mean of numbers lies between them, the clamp enforces
 *       it for the quadric, and the final rounding to fp32 is monotone while min and max are fp32 numbers themselves.
 *   (2) The members of a cluster share a cell.  The cell function's steps lie within 2^-12 cells of the ideal ones
 *       (neddf_nn_grid_build), and its edge 1 / inv_cell within 2^-24 of e_a, so two coordinates INSIDE the box with one cell index
 *       differ by less than (1 + 2^-11 + 2^-23) e_a.  (Points outside the box are clamped into the border cells and may lie further
 *       apart: the bound is for a box that holds the mesh, as the default does.  An axis without extent has e_a = 0 and one cell.)
 *   (3) Hence an input vertex with vertex_map >= 0 lies within (1 + 2^-10) D of its output vertex.
 *   (4) Every output triangle is the image of an input triangle whose corners moved by at most that much; the point with the same
 *       barycentric coordinates moved by a convex combination of the three displacements, so every point of the output surface lies
 *       within (1 + 2^-10) D of the input surface.
 * Nothing is promised in the other direction: a component smaller than a cell vanishes, and that is what clustering means. */
enum { NEDDF_SIMPLIFY_MEAN = 0, NEDDF_SIMPLIFY_QUADRIC = 1 };
int neddf_mesh_simplify_keys(neddf_ctx *ctx, const float *d_vertices, int64_t n_vertices, const double *h_lo, const double *h_hi, const int *h_cells,
                             int64_t *d_keys, void *stream);
int neddf_mesh_simplify_clusters(neddf_ctx *ctx, const int64_t *d_sorted_keys, int64_t n_vertices, int32_t *d_vertex_cluster, int32_t *d_cluster_range,
                                 int64_t *h_n_clusters, void *stream);
int neddf_mesh_simplify_pairs(neddf_ctx *ctx, const float *d_vertices, int64_t n_vertices, const int32_t *d_triangles, int64_t n_triangles,
                              const int32_t *d_vertex_cluster, int64_t *d_pairs, int64_t pair_cap, int64_t *h_n_pairs, void *stream);
int neddf_mesh_simplify_place(neddf_ctx *ctx, const float *d_vertices, int64_t n_vertices, const int64_t *d_sorted_keys, const int32_t *d_cluster_range,
                              int64_t n_clusters, int placement, double regularisation, const int32_t *d_triangles, int64_t n_triangles,
                              const int64_t *d_sorted_pairs, int64_t n_pairs, float *d_out, void *stream);
int neddf_mesh_simplify_attributes(neddf_ctx *ctx, const float *d_attributes, int64_t n_vertices, int n_columns, const int64_t *d_sorted_keys,
                                   const int32_t *d_cluster_range, int64_t n_clusters, float *d_out, void *stream);
int neddf_mesh_simplify_triangles(neddf_ctx *ctx, const int32_t *d_triangles, int64_t n_triangles, int64_t n_vertices, const int32_t *d_vertex_cluster,
                                  int32_t *d_mapped, int32_t *d_lowest, int64_t *d_keys, void *stream);
int neddf_mesh_simplify_unique(neddf_ctx *ctx, const int32_t *d_lowest, const int64_t *d_keys, int64_t n_triangles, const int64_t *d_order,
                               unsigned char *d_keep_triangle, void *stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* NEDDF_HIP_H */
