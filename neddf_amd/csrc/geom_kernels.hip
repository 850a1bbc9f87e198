// geom_kernels.hip -- distances between surfaces (no reference counterpart: the reference's evaluation compares images only).
//
//   sample_count_kernel   per block of kMcThreads triangles: how many surface samples they receive
//   sample_write_kernel   the samples of each triangle at block base + offset inside the block, triangle-major
//   nn_brute_kernel       one lane per query, every target, target tiles staged through LDS
//   grid_hist_kernel      the cell of every finite target, one integer atomicAdd per target into its cell's count
//   grid_block_kernel / grid_start_kernel   cell counts -> cell_start (count -> scan -> write over the cells, block_scan.h)
//   grid_place_kernel     target indices grouped by cell (an integer atomicAdd on the cell's cursor)
//   nn_grid_kernel        one lane per query, Chebyshev shells of cells around the query's cell
//
// THE HASH.  Every random number is a pure function of (seed, triangle t, sample k, which w), all uint32, in 32-bit arithmetic:
//     mix(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
//     hash(seed, t, k, w) = mix(mix(mix(mix(seed + 0x9e3779b9) ^ t) ^ k) + w * 0x85ebca6b)
//     uniform = (hash >> 8) * 2^-24            (the top 24 bits: exact in float and in double, in [0, 1))
// w = 0, 1: the barycentric pair (a, b) of sample k of triangle t;  w = 2 with k = 0xffffffff: the rounding uniform u_t of triangle t.
// Nothing depends on the launch shape or on timing.
//
// SAMPLING.  count(t) = floor(A_t * density + u_t) in fp64, A_t = 0.5 sqrt(|e1 x e2|^2) with e1 = p1 - p0, e2 = p2 - p0 rounded fp32
// differences widened to double (mesh_normal_*'s choice), every double operation singly rounded, none fused; 0 for an index outside [0, V), a
// non-finite vertex, a non-finite or zero area; 2^31 (which the host refuses) from 2^31 on.  Sample k of triangle t: (a, b) folded
// into the triangle (a + b > 1: a = 1 - a, b = 1 - b), p = (p0 + a * e1) + b * e2 per axis, each operation one rounded fp32 operation.
// Placement is count -> scan -> write, no atomics; inside a block the samples are dealt to the lanes one by one (a binary search in
// the block's 256 offsets finds a sample's triangle), so a large triangle's samples are written by the whole workgroup, coalesced.
//
// NEAREST NEIGHBOUR.  d2 = (dx dx + dy dy) + dz dz with dx = qx - px, single-rounded fp32.  best = (+inf, -1); candidate j replaces it
// when d2 < best, or d2 == best and j is below the current index (-1 counts as highest: the compare is unsigned) -- the lowest index
// that attains the minimum wins WHATEVER the visiting order, which is what makes the grid's answer independent of the order inside a
// cell (that order comes from atomics and depends on timing).  A target with a non-finite coordinate is never a candidate (the brute
// kernel stages it as NaN, whose d2 compares false; the grid never lists it); a query with one returns (NaN, -1).
//
// THE GRID.  cell(p) per axis: f = (p - lo) * inv_cell (two rounded fp32 operations), c = f >= g ? g - 1 : f > 0 ? (int)f : 0 (NaN: 0).
// Every step is monotone in p, so cell() is a monotone step function of each coordinate whose steps lie within 2^-23 g cells of the
// ideal ones: two points whose cells differ by k along an axis are more than (k - 1 - 2^-12) cells apart along it (g <= 1024) --
// also when either lies outside the box and was clamped.  After shell r every unvisited target is in a shell >= r + 1, hence at
// least r * safe_cell away, safe_cell = 0.99 * the smallest cell edge (the 1 % covers the step error above and the rounding of d2 and
// of the bound itself, each below 1e-6): the walk stops once (r * safe_cell)^2 > best -- strictly, so an unvisited tie cannot exist --
// and (r * safe_cell)^2 >= 1e-30 (below that d2 may underflow and the bound proves nothing).
#include "kernels.h"
#include "block_scan.h"

namespace neddf {

__device__ __forceinline__ uint32_t geom_mix(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// the top 24 bits of the hash
__device__ __forceinline__ uint32_t geom_bits(uint32_t seed, uint32_t t, uint32_t k, uint32_t w)
{
    return geom_mix(geom_mix(geom_mix(geom_mix(seed + 0x9e3779b9u) ^ t) ^ k) + w * 0x85ebca6bu) >> 8;
}

__device__ __forceinline__ bool geom_finite3(float x, float y, float z) { return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z); }

struct SampleTri {
    float p0[3], e1[3], e2[3];
};

// the corners of triangle t; false for an index outside [0, V) or a non-finite vertex
__device__ __forceinline__ bool sample_triangle(const float *v, int64_t V, const int32_t *tri, int64_t t, SampleTri *s)
{
    const int64_t i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
    if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) return false;
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p0 = v[3 * i0 + a], p1 = v[3 * i1 + a], p2 = v[3 * i2 + a];
        ok = ok && __builtin_isfinite(p0) && __builtin_isfinite(p1) && __builtin_isfinite(p2);
        s->p0[a] = p0;
        s->e1[a] = __fsub_rn(p1, p0);
        s->e2[a] = __fsub_rn(p2, p0);
    }
    return ok;
}

__device__ __forceinline__ int64_t sample_count(const float *v, int64_t V, const int32_t *tri, int64_t t, double density, uint32_t seed)
{
    SampleTri s;
    if (!sample_triangle(v, V, tri, t, &s)) return 0;
    const double ax = s.e1[0], ay = s.e1[1], az = s.e1[2], bx = s.e2[0], by = s.e2[1], bz = s.e2[2];
    const double cx = __dsub_rn(__dmul_rn(ay, bz), __dmul_rn(az, by));
    const double cy = __dsub_rn(__dmul_rn(az, bx), __dmul_rn(ax, bz));
    const double cz = __dsub_rn(__dmul_rn(ax, by), __dmul_rn(ay, bx));
    const double area = __dmul_rn(0.5, __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(cx, cx), __dmul_rn(cy, cy)), __dmul_rn(cz, cz))));
    if (!(area > 0.0) || !__builtin_isfinite(area)) return 0;
    const double u = (double)geom_bits(seed, (uint32_t)t, 0xffffffffu, 2u) * 0x1p-24;
    const double x = __dadd_rn(__dmul_rn(area, density), u);
    if (!(x < 2147483648.0)) return (int64_t)1 << 31;
    return (int64_t)floor(x);
}

__global__ void __launch_bounds__(kMcThreads) sample_count_kernel(const float *v, int64_t V, const int32_t *tri, int64_t T, double density,
                                                                  uint32_t seed, int64_t *blk)
{
    __shared__ int64_t lds[kMcThreads / 64];
    const int64_t t = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    const int64_t total = block_sum(t < T ? sample_count(v, V, tri, t, density, seed) : (int64_t)0, lds);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kMcThreads) sample_write_kernel(const float *v, int64_t V, const int32_t *tri, int64_t T, double density,
                                                                  uint32_t seed, const int64_t *blk, float *points, int32_t *triangle_id)
{
    __shared__ int64_t lds[kMcThreads];
    __shared__ int64_t off[kMcThreads];
    const int64_t first = (int64_t)blockIdx.x * kMcThreads, t = first + threadIdx.x;
    const int64_t c = t < T ? sample_count(v, V, tri, t, density, seed) : 0;
    int64_t total;
    off[threadIdx.x] = block_exclusive_scan(c, lds, &total);
    __syncthreads();
    const int64_t base = blk[blockIdx.x];
    for (int64_t j = threadIdx.x; j < total; j += kMcThreads) {
        int lo = 0, hi = kMcThreads - 1;                // the last triangle of the block whose offset is <= j: the one that owns sample j
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (off[mid] <= j) lo = mid; else hi = mid - 1;
        }
        const int64_t tt = first + lo;
        const uint32_t k = (uint32_t)(j - off[lo]);
        SampleTri s;
        (void)sample_triangle(v, V, tri, tt, &s);
        float a = (float)geom_bits(seed, (uint32_t)tt, k, 0u) * 0x1p-24f;
        float b = (float)geom_bits(seed, (uint32_t)tt, k, 1u) * 0x1p-24f;
        if (__fadd_rn(a, b) > 1.f) { a = __fsub_rn(1.f, a); b = __fsub_rn(1.f, b); }
        const int64_t o = base + j;
#pragma unroll
        for (int x = 0; x < 3; ++x)
            points[3 * o + x] = __fadd_rn(__fadd_rn(s.p0[x], __fmul_rn(a, s.e1[x])), __fmul_rn(b, s.e2[x]));
        triangle_id[o] = (int32_t)tt;
    }
}

// ---- nearest neighbour ----
struct Best {
    float d2;
    int32_t j;
};

__device__ __forceinline__ void nn_visit(Best *best, float qx, float qy, float qz, float px, float py, float pz, int32_t j)
{
    const float dx = __fsub_rn(qx, px), dy = __fsub_rn(qy, py), dz = __fsub_rn(qz, pz);
    const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
    if (d2 < best->d2 || (d2 == best->d2 && (uint32_t)j < (uint32_t)best->j)) { best->d2 = d2; best->j = j; }
}

constexpr int kNnThreads = 256;          // queries per workgroup and targets per LDS tile

__global__ void __launch_bounds__(kNnThreads) nn_brute_kernel(const float *q, int64_t nq, const float *p, int64_t np, float *out_d2, int32_t *out_j)
{
    __shared__ float4 tile[kNnThreads];
    const int64_t i = (int64_t)blockIdx.x * kNnThreads + threadIdx.x;
    const bool live = i < nq;
    const float qx = live ? q[3 * i] : 0.f, qy = live ? q[3 * i + 1] : 0.f, qz = live ? q[3 * i + 2] : 0.f;
    const float nan = __builtin_nanf("");
    Best best{ __builtin_inff(), -1 };
    for (int64_t base = 0; base < np; base += kNnThreads) {
        const int64_t j = base + threadIdx.x;
        float4 t = make_float4(nan, nan, nan, 0.f);
        if (j < np) {
            const float x = p[3 * j], y = p[3 * j + 1], z = p[3 * j + 2];
            if (geom_finite3(x, y, z)) t = make_float4(x, y, z, 0.f);       // a non-finite target stays NaN: its d2 compares false
        }
        __syncthreads();                 // the tile of the round before has been read by everyone
        tile[threadIdx.x] = t;
        __syncthreads();
        const int n = (int)(np - base < kNnThreads ? np - base : kNnThreads);
#pragma unroll 4
        for (int k = 0; k < n; ++k) {
            const float4 c = tile[k];    // one address for the whole wave: a broadcast read
            nn_visit(&best, qx, qy, qz, c.x, c.y, c.z, (int32_t)(base + k));
        }
    }
    if (!live) return;
    if (!geom_finite3(qx, qy, qz)) { best.d2 = nan; best.j = -1; }
    out_d2[i] = best.d2;
    out_j[i] = best.j;
}

// (grid_axis_cell: kernels.h -- raycast_kernels.hip lists triangles by the same cell function)
__device__ __forceinline__ int grid_cell(const NnGrid &g, float x, float y, float z, int *cx, int *cy, int *cz)
{
    *cx = grid_axis_cell(x, g.lo[0], g.inv_cell[0], g.n[0]);
    *cy = grid_axis_cell(y, g.lo[1], g.inv_cell[1], g.n[1]);
    *cz = grid_axis_cell(z, g.lo[2], g.inv_cell[2], g.n[2]);
    return (*cz * g.n[1] + *cy) * g.n[0] + *cx;
}

// cell_of[j] = the cell of target j or -1 for a non-finite one; count[cell] += 1
__global__ void __launch_bounds__(kMcThreads) grid_hist_kernel(NnGrid g, const float *p, int64_t np, int32_t *cell_of, int32_t *count)
{
    const int64_t j = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    if (j >= np) return;
    const float x = p[3 * j], y = p[3 * j + 1], z = p[3 * j + 2];
    int32_t c = -1;
    if (geom_finite3(x, y, z)) {
        int cx, cy, cz;
        c = grid_cell(g, x, y, z, &cx, &cy, &cz);
        atomicAdd(count + c, 1);
    }
    cell_of[j] = c;
}

__global__ void __launch_bounds__(kMcThreads) grid_block_kernel(const int32_t *count, int64_t n_cells, int64_t *blk)
{
    __shared__ int lds[kMcThreads / 64];
    const int64_t c = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    const int total = block_sum(c < n_cells ? (int)count[c] : 0, lds);          // at most N < 2^31 in all
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

// cell_start[c] = the number of targets in the cells before c, cell_start[n_cells] = all of them; count is zeroed: the cursors of grid_place_kernel
__global__ void __launch_bounds__(kMcThreads) grid_start_kernel(int32_t *count, int64_t n_cells, const int64_t *blk, int64_t n_blocks, int32_t *cell_start)
{
    __shared__ int lds[kMcThreads];
    const int64_t c = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    int total;
    const int e = block_exclusive_scan(c < n_cells ? (int)count[c] : 0, lds, &total);
    if (c < n_cells) {
        cell_start[c] = (int32_t)(blk[blockIdx.x] + e);
        count[c] = 0;
    }
    if (c == n_cells - 1) cell_start[n_cells] = (int32_t)blk[n_blocks];
}

__global__ void __launch_bounds__(kMcThreads) grid_place_kernel(const int32_t *cell_of, int64_t np, const int32_t *cell_start, int32_t *cursor, int32_t *order)
{
    const int64_t j = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    if (j >= np) return;
    const int32_t c = cell_of[j];
    if (c < 0) return;
    order[cell_start[c] + atomicAdd(cursor + c, 1)] = (int32_t)j;
}

__global__ void __launch_bounds__(kNnThreads) nn_grid_kernel(NnGrid g, const float *q, int64_t nq, const float *p, int64_t np,
                                                             const int32_t *cell_start, const int32_t *order, float *out_d2, int32_t *out_j)
{
    const int64_t i = (int64_t)blockIdx.x * kNnThreads + threadIdx.x;
    if (i >= nq) return;
    const float qx = q[3 * i], qy = q[3 * i + 1], qz = q[3 * i + 2];
    if (!geom_finite3(qx, qy, qz)) { out_d2[i] = __builtin_nanf(""); out_j[i] = -1; return; }
    int cx, cy, cz;
    (void)grid_cell(g, qx, qy, qz, &cx, &cy, &cz);
    const int gx = g.n[0], gy = g.n[1], gz = g.n[2];
    // the last shell that still touches the grid
    const int r_max = max(max(max(cx, gx - 1 - cx), max(cy, gy - 1 - cy)), max(cz, gz - 1 - cz));
    Best best{ __builtin_inff(), -1 };
    for (int r = 0; r <= r_max; ++r) {
        const int z0 = max(cz - r, 0), z1 = min(cz + r, gz - 1), y0 = max(cy - r, 0), y1 = min(cy + r, gy - 1);
        const int x0 = max(cx - r, 0), x1 = min(cx + r, gx - 1);
        for (int z = z0; z <= z1; ++z)
            for (int y = y0; y <= y1; ++y) {
                const int64_t row = ((int64_t)z * gy + y) * gx;
                const bool face = z - cz == r || cz - z == r || y - cy == r || cy - y == r;
                // a row on the shell's z or y face: all its cells, one contiguous range of `order`; otherwise the two cells at x = cx -+ r
                for (int side = 0; side < (face ? 1 : 2); ++side) {
                    int xa, xb;
                    if (face) { xa = x0; xb = x1; }
                    else {
                        xa = xb = side == 0 ? cx - r : cx + r;
                        if (xa < 0 || xa >= gx) continue;
                    }
                    // (a range or an index that neddf_nn_grid_build cannot have written is not followed: no read outside `order` or `p`)
                    const int64_t e = min((int64_t)cell_start[row + xb + 1], np);
                    for (int64_t k = max(cell_start[row + xa], 0); k < e; ++k) {
                        const int32_t j = order[k];
                        if (j < 0 || j >= np) continue;
                        nn_visit(&best, qx, qy, qz, p[3 * (int64_t)j], p[3 * (int64_t)j + 1], p[3 * (int64_t)j + 2], j);
                    }
                }
            }
        const float lb = __fmul_rn((float)r, g.safe_cell);
        const float lb2 = __fmul_rn(lb, lb);
        if (lb2 > best.d2 && lb2 >= 1e-30f) break;          // every unvisited target is farther than the best one (header)
    }
    out_d2[i] = best.d2;
    out_j[i] = best.j;
}

void launch_sample_count(const float *v, int64_t V, const int32_t *tri, int64_t T, double density, uint32_t seed, int64_t *blk, hipStream_t s)
{
    const int64_t nb = mc_blocks(T);
    if (nb > 0) hipLaunchKernelGGL(sample_count_kernel, dim3((unsigned)nb), dim3(kMcThreads), 0, s, v, V, tri, T, density, seed, blk);
    launch_scan_totals(blk, nb, s);
}

void launch_sample_write(const float *v, int64_t V, const int32_t *tri, int64_t T, double density, uint32_t seed, const int64_t *blk, float *points,
                         int32_t *triangle_id, hipStream_t s)
{
    if (T <= 0) return;
    hipLaunchKernelGGL(sample_write_kernel, dim3((unsigned)mc_blocks(T)), dim3(kMcThreads), 0, s, v, V, tri, T, density, seed, blk, points, triangle_id);
}

void launch_nn_brute(const float *q, int64_t nq, const float *p, int64_t np, float *d2, int32_t *index, hipStream_t s)
{
    if (nq <= 0) return;
    hipLaunchKernelGGL(nn_brute_kernel, dim3((unsigned)((nq + kNnThreads - 1) / kNnThreads)), dim3(kNnThreads), 0, s, q, nq, p, np, d2, index);
}

void launch_nn_grid_build(const NnGrid &g, const float *p, int64_t np, int32_t *cell_of, int32_t *count, int64_t *blk, int32_t *cell_start,
                          int32_t *order, hipStream_t s)
{
    const int64_t n_cells = (int64_t)g.n[0] * g.n[1] * g.n[2], nb = mc_blocks(n_cells);
    (void)hipMemsetAsync(count, 0, (size_t)n_cells * sizeof(int32_t), s);
    if (np > 0) hipLaunchKernelGGL(grid_hist_kernel, dim3((unsigned)mc_blocks(np)), dim3(kMcThreads), 0, s, g, p, np, cell_of, count);
    hipLaunchKernelGGL(grid_block_kernel, dim3((unsigned)nb), dim3(kMcThreads), 0, s, (const int32_t *)count, n_cells, blk);
    launch_scan_totals(blk, nb, s);
    hipLaunchKernelGGL(grid_start_kernel, dim3((unsigned)nb), dim3(kMcThreads), 0, s, count, n_cells, (const int64_t *)blk, nb, cell_start);
    if (np > 0)
        hipLaunchKernelGGL(grid_place_kernel, dim3((unsigned)mc_blocks(np)), dim3(kMcThreads), 0, s, (const int32_t *)cell_of, np,
                           (const int32_t *)cell_start, count, order);
}

void launch_nn_grid_query(const NnGrid &g, const float *q, int64_t nq, const float *p, int64_t np, const int32_t *cell_start, const int32_t *order,
                          float *d2, int32_t *index, hipStream_t s)
{
    if (nq <= 0) return;
    hipLaunchKernelGGL(nn_grid_kernel, dim3((unsigned)((nq + kNnThreads - 1) / kNnThreads)), dim3(kNnThreads), 0, s, g, q, nq, p, np, cell_start, order,
                       d2, index);
}

}  // namespace neddf
