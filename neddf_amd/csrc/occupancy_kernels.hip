// occupancy_kernels.hip -- empty-space skipping for the renderer (no reference counterpart: the reference evaluates every sample).
//
//   occ_cell_kernel      per cell of the R^3 grid: one byte, set when any of its 8 corner densities satisfies !(v <= threshold)
//                        (a NaN corner sets it: the grid only removes work it is sure about)
//   launch_dilate        the Chebyshev dilation (a box maximum is separable: x, then y, then z; dilate_axis_kernel of mesh_kernels.hip)
//   occ_pack_kernel      one lane per 32-bit word: bit i of the grid lives in word i >> 5 at position i & 31, whole words stored,
//                        unused high bits of the last word 0; per-block population counts
//   occ_classify_kernel  per point: keep byte (outside the box or non-finite: keep; inside: the cell's bit)
//   occ_count_kernel     per block of kOccThreads points: how many are kept
//   occ_gather_kernel    kept rows of pos / dir / var -> compact arrays in their old order, and the old index of each
//   occ_scatter_kernel   compact density / colour / normal rows -> their old places
//
// Placement is decided by count -> scan -> write launches (block_scan.h; launch_scan_totals of mesh_kernels.hip scans the block
// totals): no atomics, so every output is the same on every run (tests/occupancy_check.py restates all of it in numpy, bit for bit).
#include "kernels.h"
#include "block_scan.h"

namespace neddf {

__device__ __forceinline__ bool corner_occupied(float v, float threshold) { return !(v <= threshold); }

__global__ void __launch_bounds__(kMcThreads) occ_cell_kernel(const float *vol, int R, int64_t n_cells, float threshold, unsigned char *cell)
{
    const int64_t c = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    if (c >= n_cells) return;
    const int x = (int)(c % R), y = (int)((c / R) % R), z = (int)(c / ((int64_t)R * R));
    const int64_t L = (int64_t)R + 1;               // corners per axis
    const int64_t p = ((int64_t)z * L + y) * L + x;
    bool occ = false;
#pragma unroll
    for (int b = 0; b < 8; ++b) occ |= corner_occupied(vol[p + (b & 1) + ((b >> 1) & 1) * L + (b >> 2) * L * L], threshold);
    cell[c] = occ ? 1 : 0;
}

__global__ void __launch_bounds__(kMcThreads) occ_pack_kernel(const unsigned char *cell, int64_t n_cells, int64_t n_words, uint32_t *bits,
                                                               int64_t *blk)
{
    __shared__ int lds[kMcThreads / 64];
    const int64_t w = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    uint32_t word = 0;
    if (w < n_words) {
        const int64_t first = w << 5;
        const int n = n_cells - first < 32 ? (int)(n_cells - first) : 32;
        for (int k = 0; k < n; ++k) word |= (uint32_t)(cell[first + k] != 0) << k;
        bits[w] = word;
    }
    const int total = block_sum((int)__popc(word), lds);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

// cell coordinate of one axis in fp32, in this operation order; false when the point lies outside [0, R) there or is not finite
__device__ __forceinline__ bool cell_coord(float p, float lo, float inv_cell, int R, int *c)
{
    const float f = floorf((p - lo) * inv_cell);
    if (!(f >= 0.f && f < (float)R)) return false;          // NaN and +-Inf land here too
    *c = (int)f;
    return true;
}

__global__ void __launch_bounds__(kMcThreads) occ_classify_kernel(OccGrid g, const float *pos, int64_t n, unsigned char *keep)
{
    const int64_t i = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    if (i >= n) return;
    int x, y, z;
    bool k = true;          // outside the box, or not finite: evaluated as before
    if (cell_coord(pos[3 * i + 0], g.lo[0], g.inv_cell[0], g.res, &x) && cell_coord(pos[3 * i + 1], g.lo[1], g.inv_cell[1], g.res, &y) &&
        cell_coord(pos[3 * i + 2], g.lo[2], g.inv_cell[2], g.res, &z)) {
        const int64_t bit = ((int64_t)z * g.res + y) * g.res + x;
        k = (g.bits[bit >> 5] >> (bit & 31)) & 1u;
    }
    keep[i] = k ? 1 : 0;
}

__global__ void __launch_bounds__(kOccThreads) occ_count_kernel(const unsigned char *keep, int64_t n, int64_t *blk)
{
    const int64_t i = (int64_t)blockIdx.x * kOccThreads + threadIdx.x;
    const int total = __syncthreads_count(i < n && keep[i]);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kOccThreads) occ_gather_kernel(const unsigned char *keep, const uint32_t *pos, const uint32_t *dir,
                                                                  const uint32_t *var, int64_t n, const int64_t *blk, uint32_t *cpos,
                                                                  uint32_t *cdir, uint32_t *cvar, int32_t *index)
{
    __shared__ int lds[kOccThreads / 64];
    const int64_t i = (int64_t)blockIdx.x * kOccThreads + threadIdx.x;
    const bool k = i < n && keep[i];
    const int rank = block_rank(k, lds);
    if (!k) return;
    const int64_t o = blk[blockIdx.x] + rank;       // bit copies: NaN payloads survive
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        cpos[3 * o + a] = pos[3 * i + a];
        cdir[3 * o + a] = dir[3 * i + a];
        cvar[3 * o + a] = var[3 * i + a];
    }
    index[o] = (int32_t)i;
}

__global__ void __launch_bounds__(kMcThreads) occ_scatter_kernel(const int32_t *index, int64_t m, int64_t n, const uint32_t *cdens,
                                                                  const uint32_t *ccol, const uint32_t *cnrm, uint32_t *dens, uint32_t *col,
                                                                  uint32_t *nrm)
{
    const int64_t k = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    if (k >= m) return;
    const int64_t i = index[k];
    if (i < 0 || i >= n) return;            // an index that is not a row of the outputs is ignored
    if (dens) dens[i] = cdens[k];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (col) col[3 * i + a] = ccol[3 * k + a];
        if (nrm) nrm[3 * i + a] = cnrm[3 * k + a];
    }
}

void launch_occ_build(const float *vol, int R, float threshold, int dilate, unsigned char *cell_a, unsigned char *cell_b, uint32_t *bits,
                      int64_t *blk, hipStream_t s)
{
    const int64_t n_cells = (int64_t)R * R * R, n_words = occ_words(R);
    const unsigned grid = (unsigned)mc_blocks(n_cells);
    hipLaunchKernelGGL(occ_cell_kernel, dim3(grid), dim3(kMcThreads), 0, s, vol, R, n_cells, threshold, cell_a);
    const unsigned char *cell = launch_dilate(cell_a, cell_b, R, R, R, dilate, s);
    const int64_t nb = mc_blocks(n_words);
    hipLaunchKernelGGL(occ_pack_kernel, dim3((unsigned)nb), dim3(kMcThreads), 0, s, cell, n_cells, n_words, bits, blk);
    launch_scan_totals(blk, nb, s);
}

void launch_occ_classify(const OccGrid &g, const float *pos, int64_t n, unsigned char *keep, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(occ_classify_kernel, dim3((unsigned)mc_blocks(n)), dim3(kMcThreads), 0, s, g, pos, n, keep);
}

void launch_occ_count(const unsigned char *keep, int64_t n, int64_t *blk, hipStream_t s)
{
    const int64_t nb = occ_blocks(n);
    if (nb > 0) hipLaunchKernelGGL(occ_count_kernel, dim3((unsigned)nb), dim3(kOccThreads), 0, s, keep, n, blk);
    launch_scan_totals(blk, nb, s);
}

void launch_occ_gather(const unsigned char *keep, const float *pos, const float *dir, const float *var, int64_t n, const int64_t *blk,
                       float *cpos, float *cdir, float *cvar, int32_t *index, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(occ_gather_kernel, dim3((unsigned)occ_blocks(n)), dim3(kOccThreads), 0, s, keep, (const uint32_t *)pos,
                       (const uint32_t *)dir, (const uint32_t *)var, n, blk, (uint32_t *)cpos, (uint32_t *)cdir, (uint32_t *)cvar, index);
}

void launch_occ_scatter(const int32_t *index, int64_t m, int64_t n, const float *cdens, const float *ccol, const float *cnrm, float *dens,
                        float *col, float *nrm, hipStream_t s)
{
    if (m <= 0) return;
    hipLaunchKernelGGL(occ_scatter_kernel, dim3((unsigned)mc_blocks(m)), dim3(kMcThreads), 0, s, index, m, n, (const uint32_t *)cdens,
                       (const uint32_t *)ccol, (const uint32_t *)cnrm, (uint32_t *)dens, (uint32_t *)col, (uint32_t *)nrm);
}

}  // namespace neddf
