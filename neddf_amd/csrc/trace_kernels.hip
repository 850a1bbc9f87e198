// trace_kernels.hip -- sphere tracing of a distance field (no reference counterpart: the reference renders by volume integration only).
//
// Per-ray state lives in flat arrays (kernels.h TraceState): t the current depth, t_lo the last depth at which the distance was still
// above the threshold, status (kTrace*), steps the advances taken, dist the last distance read.
//
//   trace_begin_kernel          t = t_lo = t_near, steps = 0, dist = NaN, status ACTIVE or (non-finite origin / direction) INVALID
//   trace_count_kernel          per block of kOccThreads rays: how many are selected
//   trace_write_kernel          selected rays -> their index (ascending) and the point o + depth * d of each
//   trace_advance_kernel        one step of the compacted rays from their distances
//   trace_bisect_update_kernel  one bisection round of the compacted HIT rays from the distances at their midpoints
//   trace_finish_kernel         ACTIVE -> EXHAUSTED
//
// "Selected" is ACTIVE at depth t (the marching loop) or HIT with t_lo < t at depth 0.5 (t_lo + t) (the refinement).  Placement is decided
// by count -> scan -> write launches as in occupancy_kernels.hip (block_scan.h; launch_scan_totals scans the block totals): no
// atomics, the same output on every run.  Every floating-point step is one
// explicitly rounded operation (__fmul_rn / __fadd_rn / __fsub_rn, never a fused multiply-add), so that tests/trace_check.py restates
// all of it in numpy float32, bit for bit.
//
// Access: the per-ray arrays are SoA and read by consecutive lanes (one 256-byte or 64-byte segment per wave instruction); begin and
// finish, which own whole rays without indirection, move 16 bytes per lane when the arrays are 16-byte aligned.  The [n, 3] rows of
// origins, directions and points are 12 bytes apart: consecutive lanes cover them without gaps.  The compacted kernels reach the state
// through an ascending index, i.e. nearly coalesced.  The cost of tracing lies in the field evaluations between these kernels.
#include "kernels.h"
#include "block_scan.h"

namespace neddf {

__device__ __forceinline__ bool finite3(float x, float y, float z) { return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z); }

__device__ __forceinline__ unsigned char begin_status(const float *o, const float *d)
{
    return finite3(o[0], o[1], o[2]) && finite3(d[0], d[1], d[2]) ? kTraceActive : kTraceInvalid;
}

// four rays per lane; `vec`: every array is 16-byte aligned (status: 4-byte), so full groups move as 16-byte words
__global__ void __launch_bounds__(kMcThreads) trace_begin_kernel(const float *ro, const float *rd, int64_t n, float t_near, TraceState st, int vec)
{
    const int64_t first = ((int64_t)blockIdx.x * kMcThreads + threadIdx.x) * 4;
    if (first >= n) return;
    const float nan = __builtin_nanf("");
    if (vec && first + 4 <= n) {
        alignas(16) float o[12];
        alignas(16) float d[12];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            *(float4 *)(o + 4 * k) = ((const float4 *)(ro + 3 * first))[k];
            *(float4 *)(d + 4 * k) = ((const float4 *)(rd + 3 * first))[k];
        }
        uchar4 code;
        code.x = begin_status(o + 0, d + 0); code.y = begin_status(o + 3, d + 3);
        code.z = begin_status(o + 6, d + 6); code.w = begin_status(o + 9, d + 9);
        *(float4 *)(st.t + first) = make_float4(t_near, t_near, t_near, t_near);
        *(float4 *)(st.t_lo + first) = make_float4(t_near, t_near, t_near, t_near);
        *(float4 *)(st.dist + first) = make_float4(nan, nan, nan, nan);
        *(int4 *)(st.steps + first) = make_int4(0, 0, 0, 0);
        *(uchar4 *)(st.status + first) = code;
        return;
    }
    const int64_t last = first + 4 < n ? first + 4 : n;
    for (int64_t i = first; i < last; ++i) {
        st.t[i] = t_near; st.t_lo[i] = t_near; st.dist[i] = nan; st.steps[i] = 0;
        st.status[i] = begin_status(ro + 3 * i, rd + 3 * i);
    }
}

// the depth at which ray i is evaluated next, or false when the pass does not concern it
template <bool kBisect> __device__ __forceinline__ bool trace_selected(const TraceState &st, int64_t i, float *depth)
{
    if (!kBisect) {
        if (st.status[i] != kTraceActive) return false;
        *depth = st.t[i];
        return true;
    }
    if (st.status[i] != kTraceHit) return false;
    const float lo = st.t_lo[i], hi = st.t[i];
    if (!(lo < hi)) return false;
    *depth = __fmul_rn(0.5f, __fadd_rn(lo, hi));
    return true;
}

template <bool kBisect> __global__ void __launch_bounds__(kOccThreads) trace_count_kernel(TraceState st, int64_t n, int64_t *blk)
{
    const int64_t i = (int64_t)blockIdx.x * kOccThreads + threadIdx.x;
    float depth;
    const int total = __syncthreads_count(i < n && trace_selected<kBisect>(st, i, &depth));
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

template <bool kBisect> __global__ void __launch_bounds__(kOccThreads) trace_write_kernel(const float *ro, const float *rd, TraceState st, int64_t n,
                                                                                         const int64_t *blk, int32_t *index, float *pos)
{
    __shared__ int lds[kOccThreads / 64];
    const int64_t i = (int64_t)blockIdx.x * kOccThreads + threadIdx.x;
    float depth = 0.f;
    const bool k = i < n && trace_selected<kBisect>(st, i, &depth);
    const int rank = block_rank(k, lds);
    if (!k) return;
    const int64_t o = blk[blockIdx.x] + rank;
#pragma unroll
    for (int a = 0; a < 3; ++a) pos[3 * o + a] = __fadd_rn(ro[3 * i + a], __fmul_rn(depth, rd[3 * i + a]));
    index[o] = (int32_t)i;
}

__global__ void __launch_bounds__(kMcThreads) trace_advance_kernel(const int32_t *index, const float *D, int64_t m, int64_t n, float threshold,
                                                                    float step_scale, float min_step, float t_far, TraceState st)
{
    const int64_t k = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    if (k >= m) return;
    const int64_t r = index[k];
    if (r < 0 || r >= n) return;            // an index that is not a ray is ignored
    const float d = D[k];
    st.dist[r] = d;
    if (d != d) { st.status[r] = kTraceInvalid; return; }
    if (d <= threshold) { st.status[r] = kTraceHit; return; }
    const float t0 = st.t[r];
    const float step = fmaxf(__fmul_rn(step_scale, __fsub_rn(d, threshold)), min_step);
    const float t1 = __fadd_rn(t0, step);
    st.t_lo[r] = t0;
    st.t[r] = t1;
    st.steps[r] += 1;
    if (!(t1 <= t_far)) st.status[r] = kTraceMiss;
}

__global__ void __launch_bounds__(kMcThreads) trace_bisect_update_kernel(const int32_t *index, const float *D, int64_t m, int64_t n, float threshold,
                                                                          TraceState st)
{
    const int64_t k = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    if (k >= m) return;
    const int64_t r = index[k];
    if (r < 0 || r >= n) return;
    const float mid = __fmul_rn(0.5f, __fadd_rn(st.t_lo[r], st.t[r]));       // the depth trace_write_kernel<true> evaluated
    const float d = D[k];
    if (d <= threshold || d != d) { st.t[r] = mid; st.dist[r] = d; }
    else st.t_lo[r] = mid;
}

// 16 status bytes per lane: a byte 0 (ACTIVE) becomes 3 (EXHAUSTED), every other byte stays
__device__ __forceinline__ uint32_t exhaust_word(uint32_t w)
{
    const uint32_t zero = ~(((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u;      // 0x80 in exactly the bytes that are 0
    return w | ((zero >> 7) * (uint32_t)kTraceExhausted);
}

__global__ void __launch_bounds__(kMcThreads) trace_finish_kernel(unsigned char *status, int64_t n, int vec)
{
    const int64_t first = ((int64_t)blockIdx.x * kMcThreads + threadIdx.x) * 16;
    if (first >= n) return;
    if (vec && first + 16 <= n) {
        uint4 w = *(const uint4 *)(status + first);
        w.x = exhaust_word(w.x); w.y = exhaust_word(w.y); w.z = exhaust_word(w.z); w.w = exhaust_word(w.w);
        *(uint4 *)(status + first) = w;
        return;
    }
    const int64_t last = first + 16 < n ? first + 16 : n;
    for (int64_t i = first; i < last; ++i)
        if (status[i] == kTraceActive) status[i] = kTraceExhausted;
}

// one float4 per lane over the 3 n floats of each array (their base is a workspace carve: 16-byte aligned); dir repeats 1 0 0
__global__ void __launch_bounds__(kMcThreads) trace_unit_inputs_kernel(float *dir, float *var, int64_t n_floats)
{
    const int64_t q = ((int64_t)blockIdx.x * kMcThreads + threadIdx.x) * 4;
    if (q >= n_floats) return;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (q + j) % 3 == 0 ? 1.f : 0.f;
    if (q + 4 <= n_floats) {
        *(float4 *)(dir + q) = make_float4(v[0], v[1], v[2], v[3]);
        *(float4 *)(var + q) = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    for (int j = 0; q + j < n_floats; ++j) { dir[q + j] = v[j]; var[q + j] = 0.f; }
}

static inline bool aligned_to(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

void launch_trace_begin(const float *ro, const float *rd, int64_t n, float t_near, const TraceState &st, hipStream_t s)
{
    if (n <= 0) return;
    const int vec = aligned_to(ro, 16) && aligned_to(rd, 16) && aligned_to(st.t, 16) && aligned_to(st.t_lo, 16) && aligned_to(st.dist, 16) &&
                    aligned_to(st.steps, 16) && aligned_to(st.status, 4);
    hipLaunchKernelGGL(trace_begin_kernel, dim3((unsigned)mc_blocks((n + 3) / 4)), dim3(kMcThreads), 0, s, ro, rd, n, t_near, st, vec);
}

void launch_trace_compact(const float *ro, const float *rd, int64_t n, const TraceState &st, int bisect, int64_t *blk, int32_t *index, float *pos,
                          hipStream_t s)
{
    const int64_t nb = occ_blocks(n);
    if (nb > 0) {
        if (bisect) hipLaunchKernelGGL(trace_count_kernel<true>, dim3((unsigned)nb), dim3(kOccThreads), 0, s, st, n, blk);
        else hipLaunchKernelGGL(trace_count_kernel<false>, dim3((unsigned)nb), dim3(kOccThreads), 0, s, st, n, blk);
    }
    launch_scan_totals(blk, nb, s);
    if (nb > 0) {
        if (bisect) hipLaunchKernelGGL(trace_write_kernel<true>, dim3((unsigned)nb), dim3(kOccThreads), 0, s, ro, rd, st, n, (const int64_t *)blk, index, pos);
        else hipLaunchKernelGGL(trace_write_kernel<false>, dim3((unsigned)nb), dim3(kOccThreads), 0, s, ro, rd, st, n, (const int64_t *)blk, index, pos);
    }
}

void launch_trace_advance(const int32_t *index, const float *D, int64_t m, int64_t n, float threshold, float step_scale, float min_step, float t_far,
                          const TraceState &st, hipStream_t s)
{
    if (m <= 0) return;
    hipLaunchKernelGGL(trace_advance_kernel, dim3((unsigned)mc_blocks(m)), dim3(kMcThreads), 0, s, index, D, m, n, threshold, step_scale, min_step,
                       t_far, st);
}

void launch_trace_bisect_update(const int32_t *index, const float *D, int64_t m, int64_t n, float threshold, const TraceState &st, hipStream_t s)
{
    if (m <= 0) return;
    hipLaunchKernelGGL(trace_bisect_update_kernel, dim3((unsigned)mc_blocks(m)), dim3(kMcThreads), 0, s, index, D, m, n, threshold, st);
}

void launch_trace_finish(unsigned char *status, int64_t n, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(trace_finish_kernel, dim3((unsigned)mc_blocks((n + 15) / 16)), dim3(kMcThreads), 0, s, status, n, (int)aligned_to(status, 16));
}

void launch_trace_unit_inputs(float *dir, float *var, int64_t n, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(trace_unit_inputs_kernel, dim3((unsigned)mc_blocks((3 * n + 3) / 4)), dim3(kMcThreads), 0, s, dir, var, 3 * n);
}

}  // namespace neddf
