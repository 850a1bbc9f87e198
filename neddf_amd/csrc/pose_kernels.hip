// pose_kernels.hip -- the input-gradient end of the training backward: what carries the gradient of a loss from the
// fields' pre-activations back to the sample points, the rays and the camera pose (train_kernels.h "pose gradients").
//
//   enc_input_grad_kernel     dZ of the layers that read an encoding  ->  g_pos, g_dir, g_var [N, 3]
//   sampling_backward_kernel  g_pos, g_dir, g_var [B, S, 3]           ->  g_ray_dir, g_ray_orig [B, 3]
//   raygen_backward_kernel    g_ray_dir, g_ray_orig [B, 3]            ->  g_R [3, 3], g_T [3]
//   raygen_table_backward_kernel   the same per camera of a camera table ->  [n_cameras] rows of g_R, g_T
//
// Operand policy: fp32 MFMA (v_mfma_f32_32x32x2_f32) for the products, whatever the field's policy; the C ABI refuses the
// split-fp16 policy for these outputs rather than mixing the two.  Every reduction runs in a fixed order (LDS / wave trees, no
// floating-point atomics): the outputs are bitwise repeatable.
#include "train_kernels.h"
#include "block_scan.h"
#include "device_math.h"
#include <math.h>

namespace neddf {

typedef float pose_f32x16 __attribute__((ext_vector_type(16)));

// ----------------------------------------------------------------------------
// Encoding-segment input gradients fused with the encodings' backward.
//
// NeDDF.forward (neddf.py:186-257) feeds a sample point into the network through
//   embed_pos_scaled (value row y and Jacobian rows G; neddf.py:200-204) -> distance layer 0 and every skip layer (:214-219)
//   embed_pos        (y, G; :205-209) and embed_dir (y; :210)            -> colour layer 0 (:243-253)
// so the gradient on the encodings' rows is, per 4-row point group (value, d/dx, d/dy, d/dz),
//   gS[4, 6E]        = sum over l in {0} + skips of dZ_l x (encoding rows of W_l)^T           (LinearGradFunction.backward linear.py:72-75)
//   gU[4, 6E + 6Ed]  = dZ_col0 x (embed_pos and embed_dir rows of W_col0)^T
// NeRF.forward (nerf.py:139-159) is the same with value rows only: embed_pos (unscaled) into layer 0 and after every skip layer,
// embed_dir into the colour head; its segments all accumulate into the gU tile and the Jacobian rows of the tile stay zero.
// A workgroup takes 32 points (128 rows); each wave forms the 32 x 64 tile of gS and the 32 x 128 tile of gU of its 8 points in
// MFMA accumulators (K = the hidden width, staged 32 features at a time through LDS) and differentiates the encodings on the
// accumulators themselves: in the 32x32 layout a lane holds the four rows of one point for one encoding column.  With J = I3
// (sample_pos_grad is the constant identity, neddf.py:186-191) column (e, axis d) of PositionalEncodingGradLayer.forward
// (with_grad/positional_encoding.py:65-87) is, for p = 2^e x_d and the constant scale s,
//   y_sin = s sin p     G_sin[d] = 2^e s cos p     y_cos = s cos p     G_cos[d] = -2^e s sin p
// hence   g_x_d += gy_sin G_sin - gG_sin 4^e y_sin + gy_cos G_cos - gG_cos 4^e y_cos,
// the second and fourth being the second-derivative terms of G = f s cos(p) J.  s carries pe_grad_scale, the low-pass scale of
// neddf_set_iter and the cone weight exp(-0.5 4^e var); aux_grad_scale reaches this kernel inside dZ.  sin / cos / exp are
// recomputed from pos and var by the forward's own pe_pair (nothing is saved for this in the forward workspace).
// embed_dir = PositionalEncoding(dir): g_dir_d += 2^e (gy_sin cos p - gy_cos sin p).
// g_var is written as ZERO: Sampling.get_pe_weights runs under torch.set_grad_enabled(False) (ray/sampling.py:55), so the
// reference's autograd treats the cone weights as constants and no gradient reaches diag_variance.
// The per-column terms go to LDS and are summed per (point, axis) in column order.
constexpr int kEgPts = 32;                  // points per workgroup
constexpr int kEgKc = 32;                   // features per staged chunk (As + Bs = 34 KB of LDS)
constexpr int kEgLdA = 4 * kEgKc + 8;       // floats per point of the staged dZ chunk: + 8 -> conflict-free A-operand reads
constexpr int kEgLdB = kEgKc + 2;           // floats per encoding column of the staged weight chunk: + 2 -> conflict-free B reads
constexpr int kEgColsS = 64, kEgColsU = 128;
constexpr int kEgLds = kEgPts * kEgLdA + kEgColsU * kEgLdB;

__global__ __launch_bounds__(kThreads) void enc_input_grad_kernel(const EncGradArgs a)
{
    __shared__ float smem[kEgLds];
    float *As = smem, *Bs = smem + kEgPts * kEgLdA;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j32 = lane & 31, h = lane >> 5;
    const int64_t p0 = (int64_t)blockIdx.x * kEgPts;
    pose_f32x16 acc[6];             // [0..1]: gS columns 0..63, [2..5]: gU columns 0..127
#pragma unroll
    for (int t = 0; t < 6; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    for (int sg = 0; sg < a.n_seg; ++sg) {
        const EncGradSeg &g = a.seg[sg];
        const int ncolpad = g.target ? kEgColsU : kEgColsS;
        for (int kc = 0; kc < g.nk / kEgKc; ++kc) {
            __syncthreads();        // the previous chunk's MFMAs are done with As / Bs
            // dZ chunk: As[p][4 k + r] = dZ[row 4 (p0 + p) + r][32 kc + k], zero beyond the last point; two points per pass
            if (g.point_major) {
                const int ps = tid >> 7, idx = tid & 127;           // the chunk of a point is 128 contiguous floats
                for (int p = ps; p < kEgPts; p += 2) {
                    const int64_t n = p0 + p;
                    As[p * kEgLdA + idx] = n < a.N ? g.dZ[n * 4 * g.ld + 4 * kEgKc * kc + idx] : 0.f;
                }
            } else {
                const int ps = tid >> 7, r = (tid >> 5) & 3, k = tid & 31;
                for (int p = ps; p < kEgPts; p += 2) {
                    const int64_t n = p0 + p;
                    As[p * kEgLdA + 4 * k + r] = (n < a.N && r < g.rows) ? g.dZ[(n * g.rows + r) * g.ld + kEgKc * kc + k] : 0.f;
                }
            }
            // weight chunk: Bs[j][k] = W[encoding row row0 + j][feature 32 kc + k], zero beyond the segment's columns
            {
                const int k = tid & 31;
                for (int j = tid >> 5; j < ncolpad; j += 8)
                    Bs[j * kEgLdB + k] = (j >= g.col0 && j < g.col0 + g.ncols) ? g.W[(j - g.col0) * g.sj + (kEgKc * kc + k) * g.sk] : 0.f;
            }
            __syncthreads();
            const float *ap = As + (wave * 8 + (j32 >> 2)) * kEgLdA + (j32 & 3) + 4 * h;
            const float *bp = Bs + j32 * kEgLdB + h;
#pragma unroll 4
            for (int st = 0; st < kEgKc / 2; ++st) {
                const float av = ap[8 * st];
                if (g.target == 0) {
#pragma unroll
                    for (int t = 0; t < 2; ++t)
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bp[(32 * t) * kEgLdB + 2 * st], acc[t], 0, 0, 0);
                } else {
#pragma unroll
                    for (int t = 0; t < 4; ++t)
                        acc[2 + t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bp[(32 * t) * kEgLdB + 2 * st], acc[2 + t], 0, 0, 0);
                }
            }
        }
    }
    __syncthreads();
    // encoding backward on the accumulators: acc[t][4 q + r] = row r of point 8 wave + 2 q + h, column 32 t' + j32
    float *Cs = smem;               // [kEgPts][192]: per-column terms, S columns 0..63, U columns 64..191
    constexpr int kLdC = kEgColsS + kEgColsU;
    const int K3 = 3 * a.enc.E, K3d = 3 * a.enc.Ed, Cpe = 2 * K3;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const bool scaled = t < 2;
        const int col = scaled ? 32 * t + j32 : 32 * (t - 2) + j32;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int p = wave * 8 + 2 * q + h;
            const int64_t n = p0 + p;
            float term = 0.f;
            if (n < a.N) {
                const float gy = acc[t][4 * q], g1 = acc[t][4 * q + 1], g2 = acc[t][4 * q + 2], g3 = acc[t][4 * q + 3];
                if (col < Cpe) {
                    const bool is_cos = col >= K3;
                    const int c = is_cos ? col - K3 : col, e = c / 3, d = c - 3 * e;
                    const float gG = d == 0 ? g1 : (d == 1 ? g2 : g3);
                    const float f = (float)(1 << e);
                    float vs, vc, js, jc;
                    if (scaled) pe_pair<true>(e, a.pos[n * 3 + d], a.var[n * 3 + d], a.enc.lowpass[e], vs, vc, js, jc);
                    else pe_pair<false>(e, a.pos[n * 3 + d], a.var[n * 3 + d], a.enc.lowpass[e], vs, vc, js, jc);
                    // d(vs)/dx = js, d(js)/dx = -4^e vs;  d(vc)/dx = jc, d(jc)/dx = -4^e vc
                    term = is_cos ? gy * jc - gG * ((f * f) * vc) : gy * js - gG * ((f * f) * vs);
                } else if (!scaled && col < Cpe + 2 * K3d) {
                    const int cd = col - Cpe;
                    const bool is_cos = cd >= K3d;
                    const int c = is_cos ? cd - K3d : cd, e = c / 3, d = c - 3 * e;
                    const float f = (float)(1 << e);
                    float sn, cs;
                    sincosf(f * a.dir[n * 3 + d], &sn, &cs);
                    term = is_cos ? -(gy * (f * sn)) : gy * (f * cs);
                }
            }
            Cs[p * kLdC + (scaled ? 0 : kEgColsS) + col] = term;
        }
    }
    __syncthreads();
    if (tid < kEgPts * 3) {
        const int p = tid / 3, d = tid - 3 * p;
        const int64_t n = p0 + p;
        if (n < a.N) {
            const float *c = Cs + p * kLdC;
            float gp = 0.f, gd = 0.f;
            for (int e = 0; e < a.enc.E; ++e) {
                gp += c[3 * e + d];
                gp += c[K3 + 3 * e + d];
                gp += c[kEgColsS + 3 * e + d];
                gp += c[kEgColsS + K3 + 3 * e + d];
            }
            for (int e = 0; e < a.enc.Ed; ++e) {
                gd += c[kEgColsS + Cpe + 3 * e + d];
                gd += c[kEgColsS + Cpe + K3d + 3 * e + d];
            }
            if (a.g_pos) a.g_pos[n * 3 + d] = gp;
            if (a.g_dir) a.g_dir[n * 3 + d] = gd;
            if (a.g_var) a.g_var[n * 3 + d] = 0.f;
        }
    }
}

void launch_enc_input_grad(const EncGradArgs &a, hipStream_t s)
{
    if (a.N <= 0) return;
    hipLaunchKernelGGL(enc_input_grad_kernel, dim3((unsigned)((a.N + kEgPts - 1) / kEgPts)), dim3(kThreads), 0, s, a);
}

// ----------------------------------------------------------------------------
// Backward of Ray.get_sampling_cones (ray.py:128-194) / get_sampling_points (ray.py:88-126) with respect to the ray:
//   pos = o + d t_mu     dir = d     var = t_var d^2 + r_var (1 - d^2)
// (t_mu, t_var, r_var are functions of the distances alone, which are not differentiated: stratified uniforms and sample_pdf
// output under no_grad, nerf_render.py:131-170).  One wave per ray: lanes stride over the samples, then a butterfly sum.
template <bool CONE>
__global__ void sampling_backward_kernel(const float *g_pos, const float *g_dir, const float *g_var, const float *rd, const float *dists,
                                         int64_t n, int S, float r2, float *g_rd, float *g_ro)
{
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b >= n) return;             // (whole waves leave together)
    const float *d = dists + b * S;
    float gd[3] = { 0.f, 0.f, 0.f }, go[3] = { 0.f, 0.f, 0.f };
    for (int j = lane; j < S; j += 64) {
        float t_mu, t_var, r_var;
        sample_moments<CONE>(d, j, S, r2, t_mu, t_var, r_var);
        const int64_t i = b * S + j;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float gp = g_pos ? g_pos[3 * i + k] : 0.f;
            float t = gp * t_mu;
            if (g_dir) t += g_dir[3 * i + k];
            if (CONE && g_var) t += g_var[3 * i + k] * (2.0f * rd[3 * b + k] * (t_var - r_var));
            gd[k] += t;
            go[k] += gp;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            gd[k] += __shfl_xor(gd[k], off, 64);
            go[k] += __shfl_xor(go[k], off, 64);
        }
    if (lane == 0)
        for (int k = 0; k < 3; ++k) { g_rd[3 * b + k] = gd[k]; g_ro[3 * b + k] = go[k]; }
}

void launch_sampling_backward(const float *g_pos, const float *g_dir, const float *g_var, const float *rd, const float *dists, int64_t n, int S,
                              double radius, float *g_rd, float *g_ro, hipStream_t s)
{
    if (n <= 0 || S <= 0) return;
    dim3 g((unsigned)((n + 3) / 4)), b(256);
    if (radius >= 0.0)
        hipLaunchKernelGGL(sampling_backward_kernel<true>, g, b, 0, s, g_pos, g_dir, g_var, rd, dists, n, S, (float)(radius * radius), g_rd, g_ro);
    else
        hipLaunchKernelGGL(sampling_backward_kernel<false>, g, b, 0, s, g_pos, g_dir, g_var, rd, dists, n, S, 0.f, g_rd, g_ro);
}

// ----------------------------------------------------------------------------
// Backward of Camera.create_rays (camera.py:155-171): ray_dir = R c(uv), ray_orig = T with c the unit camera-frame direction of
// the pixel (pinhole_calib.py:51-74; the intrinsics are not differentiated):
//   g_R[i][j] = sum_b g_ray_dir[b][i] c_b[j]        g_T[i] = sum_b g_ray_orig[b][i]
// One workgroup: every thread sums its rays b = tid, tid + 256, .. in order, then an LDS tree over the 256 partial sums.
//
// one ray's terms added to a thread's 12 partial sums (raygen_backward_kernel and raygen_table_backward_kernel)
template <typename T>
__device__ __forceinline__ void raygen_backward_row(const T *uv, int64_t b, float fx, float fy, float cx, float cy, const float *g_rd,
                                                    const float *g_ro, float (&acc)[12])
{
    float u = 0.5f + 1.0f * (float)uv[2 * b + 0];
    float v = 0.5f + 1.0f * (float)uv[2 * b + 1];
    float x = (1.0f / fx) * (u - cx);
    float y = (1.0f / fy) * (v - cy);
    float c[3] = { x, -y, -1.0f };
    float nrm = sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    nrm = nrm < 1e-12f ? 1e-12f : nrm;
    c[0] /= nrm; c[1] /= nrm; c[2] /= nrm;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float gi = g_rd[3 * b + i];
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[3 * i + j] += gi * c[j];
        acc[9 + i] += g_ro[3 * b + i];
    }
}

// the tree over the 256 threads' partial sums; out[12] = g_R | g_T
__device__ __forceinline__ void raygen_backward_tree(const float (&acc)[12], float (*red)[256], float *out)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 12; ++k) red[k][tid] = acc[k];
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w)
#pragma unroll
            for (int k = 0; k < 12; ++k) red[k][tid] += red[k][tid + w];
        __syncthreads();
    }
    if (tid < 12) out[tid] = red[tid][0];
}

template <typename T>
__global__ __launch_bounds__(256) void raygen_backward_kernel(const T *uv, int64_t n, CameraArg cam, const float *g_rd, const float *g_ro, float *out)
{
    __shared__ float red[12][256];
    const int tid = threadIdx.x;
    const float fx = cam.calib[0], fy = cam.calib[1], cx = cam.calib[2], cy = cam.calib[3];
    float acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.f;
    for (int64_t b = tid; b < n; b += 256) raygen_backward_row(uv, b, fx, fy, cx, cy, g_rd, g_ro, acc);
    raygen_backward_tree(acc, red, out);
}

void launch_raygen_backward(const void *uv, int uv_type, int64_t n, const CameraArg &cam, const float *g_rd, const float *g_ro, float *out,
                            hipStream_t s)
{
    dim3 g(1), b(256);
    switch (uv_type) {
    case 0: hipLaunchKernelGGL(raygen_backward_kernel<float>, g, b, 0, s, (const float *)uv, n, cam, g_rd, g_ro, out); break;
    case 1: hipLaunchKernelGGL(raygen_backward_kernel<int64_t>, g, b, 0, s, (const int64_t *)uv, n, cam, g_rd, g_ro, out); break;
    case 2: hipLaunchKernelGGL(raygen_backward_kernel<int32_t>, g, b, 0, s, (const int32_t *)uv, n, cam, g_rd, g_ro, out); break;
    default: hipLaunchKernelGGL(raygen_backward_kernel<int16_t>, g, b, 0, s, (const int16_t *)uv, n, cam, g_rd, g_ro, out); break;
    }
}

// NEDDF_UV_CAMERA_TABLE: one workgroup per camera v = blockIdx.x, out[v][12] = what raygen_backward_kernel gives for camera v on
// the rows with view[b] == v, taken in batch order -- the same bits, because every add happens in the same place: that kernel hands
// the camera's k-th row to thread k mod 256, each thread adds its rows in increasing k, then the tree runs.  Here the batch is walked
// in chunks of 256 rows; a lane whose row belongs to v has rank k = (rows of v in earlier chunks) + (rows of v at lower lanes of this
// chunk) and drops its lane number into LDS slot k mod 256 -- the ranks of one chunk are at most 256 consecutive numbers, so no two
// share a slot -- and after the barrier thread t adds the row in slot t, if any.  Chunks run in order, so every thread meets its
// rows in increasing k.  No sort, no workspace, no atomic; a view outside [0, n_cameras) equals no blockIdx.x and belongs to no
// camera; a camera without rows sums nothing and writes +0.0.  Every workgroup reads the whole view array: O(n_cameras * n) 4-byte
// reads out of L2, nothing next to the field kernels at training sizes.
template <typename T>
__global__ __launch_bounds__(256) void raygen_table_backward_kernel(const T *uv, int64_t n, CameraTableArg table, const float *g_rd,
                                                                    const float *g_ro, float *out)
{
    __shared__ float red[12][256];
    __shared__ int slot[256];
    __shared__ int waves[4];
    const int tid = threadIdx.x;
    const int32_t cam = (int32_t)blockIdx.x;            // < n_cameras: the grid is n_cameras workgroups
    float fx = 1.f, fy = 1.f, cx = 0.f, cy = 0.f;
    if (n > 0) {                                        // (an empty batch may come without a table to read)
        const float *calib = table.cameras + 16 * (int64_t)cam + 12;
        fx = calib[0]; fy = calib[1]; cx = calib[2]; cy = calib[3];
    }
    float acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.f;
    unsigned before = 0;                                // the camera's rows in earlier chunks, mod 2^32 (only mod 256 is used)
    for (int64_t c0 = 0; c0 < n; c0 += 256) {
        slot[tid] = -1;                                 // (this thread alone read slot[tid] in the last round)
        const int64_t b = c0 + tid;
        const bool mine = b < n && table.view[b] == cam;
        const int rank = block_rank(mine, waves);       // barrier: every slot is cleared, the wave counts are in
        if (mine) slot[(before + (unsigned)rank) & 255u] = tid;
        before += (unsigned)(waves[0] + waves[1] + waves[2] + waves[3]);
        __syncthreads();                                // the slots are filled; the wave counts are read
        const int lane = slot[tid];
        if (lane >= 0) raygen_backward_row(uv, c0 + lane, fx, fy, cx, cy, g_rd, g_ro, acc);
    }
    raygen_backward_tree(acc, red, out + 12 * (int64_t)cam);
}

void launch_raygen_table_backward(const void *uv, int uv_type, int64_t n, const CameraTableArg &table, const float *g_rd, const float *g_ro,
                                  float *out, hipStream_t s)
{
    dim3 g((unsigned)table.n_cameras), b(256);
    switch (uv_type) {
    case 0: hipLaunchKernelGGL(raygen_table_backward_kernel<float>, g, b, 0, s, (const float *)uv, n, table, g_rd, g_ro, out); break;
    case 1: hipLaunchKernelGGL(raygen_table_backward_kernel<int64_t>, g, b, 0, s, (const int64_t *)uv, n, table, g_rd, g_ro, out); break;
    case 2: hipLaunchKernelGGL(raygen_table_backward_kernel<int32_t>, g, b, 0, s, (const int32_t *)uv, n, table, g_rd, g_ro, out); break;
    default: hipLaunchKernelGGL(raygen_table_backward_kernel<int16_t>, g, b, 0, s, (const int16_t *)uv, n, table, g_rd, g_ro, out); break;
    }
}

}  // namespace neddf
