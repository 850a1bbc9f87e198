// block_scan.h -- the workgroup primitives of deterministic, atomic-free stream compaction (mesh_kernels.hip,
// occupancy_kernels.hip, trace_kernels.hip): count per workgroup, scan the block totals in one workgroup (launch_scan_totals),
// write at block base + rank inside the block.
//
//   a 0/1 predicate    count: __syncthreads_count(keep)           write: block_rank(keep, lds)
//   a count per thread count: block_sum(v, lds)                   write: block_exclusive_scan(v, lds, &total)
//
// The rule they all share: EVERY thread of the workgroup calls them, before any divergent `return` (they hold barriers).  The
// workgroup is a whole number of wave64s (blockDim.x a multiple of 64; kMcThreads = 256 and kOccThreads = 1024 are in use).
#pragma once
#include <hip/hip_runtime.h>

namespace neddf {

// sum of one integer (int, or int64_t where a total may pass 2^31) per thread over the workgroup (every thread receives it);
// lds: blockDim.x / 64 values, free again on return
template <typename T>
__device__ __forceinline__ T block_sum(T v, T *lds)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) lds[wave] = v;
    __syncthreads();
    T t = 0;
    for (int w = 0; w < n_waves; ++w) t += lds[w];
    __syncthreads();
    return t;
}

// exclusive scan of one value per thread over the workgroup; *total = the sum of all; lds: blockDim.x values, free again on return
template <typename T>
__device__ T block_exclusive_scan(T v, T *lds, T *total)
{
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int d = 1; d < (int)blockDim.x; d <<= 1) {
        const T add = t >= d ? lds[t - d] : (T)0;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    const T incl = lds[t];
    *total = lds[blockDim.x - 1];
    __syncthreads();                // lds may be reused by the caller's next scan
    return incl - v;
}

// how many threads of the workgroup with a LOWER thread index keep: a wave64 ballot and the population count of the lower lanes,
// plus the totals of the waves before this one.  lds: blockDim.x / 64 ints; one barrier, none behind the reads -- a second call
// on the same array needs a __syncthreads() of the caller's in between
__device__ __forceinline__ int block_rank(bool keep, int *lds)
{
    const unsigned long long ballot = __ballot(keep);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) lds[wave] = (int)__popcll(ballot);
    __syncthreads();
    int before = (int)__popcll(ballot & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) before += lds[w];
    return before;
}

}  // namespace neddf
