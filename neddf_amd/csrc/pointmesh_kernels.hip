// pointmesh_kernels.hip -- the distance from points to the SURFACE of an indexed triangle mesh: the closest point of the closest
// triangle (no reference counterpart: the reference's evaluation compares images only).
//
//   pm_brute_kernel       one lane per query, every triangle; the per-triangle constants are computed once per tile by the staging
//                         lanes and staged through LDS, the inner loop is selects only
//   pm_prepare_kernel     one lane per triangle: the same constants into a table, once per query launch
//   pm_grid_kernel        one lane per query: the overflow list, then Chebyshev shells of the ray-casting grid's cells around the
//                         query's cell (or every list once: the header says when), the constants gathered from the table
//
// THE DISTANCE (include/neddf_hip.h states it; tests/pointmesh_check.py restates it in numpy bit for bit).  Per triangle the edges
// e0 = b - a, e1 = c - a, e2 = c - b, three Gram entries' reciprocals, and f = e1 without its part along e0 with 1 / |f|^2 -- four
// divisions, none of them per pair.  Per pair five candidates, each a point of the triangle up to rounding: the clamped foot on each
// edge, q = s + clamp01(h r) e, the corner c, and the interior point (a + v e0) + w e1 when v > 0, w > 0 and v + w < 1, (v, w) solved
// through f (a QR step: the error grows with the triangle's aspect ratio, not with its square) and refined once on the residual.
// Every operation is one rounded fp32 operation, none fused (-ffp-contract=off and the __f*_rn intrinsics below).  best =
// (+inf, -1, 0, 0); a pair replaces it when D2 < best, or D2 == best and its index is below the current one (-1 counts as highest:
// the compare is unsigned): the lowest index that attains the smallest D2 wins WHATEVER the visiting order and however often a
// triangle is met, which is what lets the grid return the brute kernel's bits.
//
// THE TABLE.  Five float4 per triangle: (a, valid), (b, g01), (c, r00), (f, rpp), (r11, r22, -, -).  The edges are three subtractions
// each and are recomputed per pair (the same rounded operation gives the same bits): with them the table would need seven float4 and
// a 256-triangle tile 28 KB of LDS instead of 20.  rpp is stored as NaN when gpp > 0 fails: v and w are then NaN and the interior
// candidate fails its own comparisons, which is the stated rule without a flag of its own.  The grid query gathers 80 bytes per visit
// from this table instead of three indices, nine floats and four correctly rounded divisions (about 40 instructions) per visit; the
// prepare launch costs one pass over the mesh.
//
// The per-pair code (pm_constants, pm_visit, pm_store) lives in pointmesh_device.h: bvh_kernels.hip visits triangles with the same
// functions, which is what makes its result the brute kernel's.
#include "kernels.h"
#include "pointmesh_device.h"

namespace neddf {

__global__ void __launch_bounds__(kPmThreads) pm_brute_kernel(const float *q, int64_t nq, const float *v, int64_t V, const int32_t *tri, int64_t T,
                                                              float *out_d2, int32_t *out_j, float *out_b1, float *out_b2)
{
    __shared__ float4 tile[kPmVec][kPmThreads];         // 20 KB
    const int64_t i = (int64_t)blockIdx.x * kPmThreads + threadIdx.x;
    const bool live = i < nq;
    float px = live ? q[3 * i] : 0.f, py = live ? q[3 * i + 1] : 0.f, pz = live ? q[3 * i + 2] : 0.f;
    const bool ok = pm_finite3(px, py, pz);
    if (!ok) px = py = pz = 0.f;
    PmBest best{ __builtin_inff(), -1, 0.f, 0.f };
    for (int64_t base = 0; base < T; base += kPmThreads) {
        const int64_t j = base + threadIdx.x;
        float4 c[kPmVec];
        if (j < T) pm_constants(v, V, tri, j, c);
        else {
#pragma unroll
            for (int a = 0; a < kPmVec; ++a) c[a] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __syncthreads();                 // the tile of the round before has been read by everyone
#pragma unroll
        for (int a = 0; a < kPmVec; ++a) tile[a][threadIdx.x] = c[a];
        __syncthreads();
        const int n = (int)(T - base < kPmThreads ? T - base : kPmThreads);
        for (int k = 0; k < n; ++k)      // one address per read for the whole wave: broadcast reads
            pm_visit(px, py, pz, tile[0][k], tile[1][k], tile[2][k], tile[3][k], tile[4][k], (int32_t)(base + k), &best);
    }
    if (live) pm_store(ok, best, i, out_d2, out_j, out_b1, out_b2);
}

__global__ void __launch_bounds__(kPmThreads) pm_prepare_kernel(const float *v, int64_t V, const int32_t *tri, int64_t T, float4 *table)
{
    const int64_t j = (int64_t)blockIdx.x * kPmThreads + threadIdx.x;
    if (j >= T) return;
    float4 c[kPmVec];
    pm_constants(v, V, tri, j, c);
#pragma unroll
    for (int a = 0; a < kPmVec; ++a) table[kPmVec * j + a] = c[a];
}

// the triangles items[k0 .. k1) against one query (a range or an index that neddf_raycast_grid_build cannot have written is not followed)
__device__ __forceinline__ void pm_visit_items(float px, float py, float pz, const float4 *table, int64_t T, const int32_t *items, int64_t n_items,
                                                  int64_t k0, int64_t k1, PmBest *best)
{
    k0 = k0 > 0 ? k0 : 0;
    k1 = k1 < n_items ? k1 : n_items;
    for (int64_t k = k0; k < k1; ++k) {
        const int32_t j = items[k];
        if (j < 0 || j >= T) continue;
        const float4 *c = table + kPmVec * (int64_t)j;
        pm_visit(px, py, pz, c[0], c[1], c[2], c[3], c[4], j, best);
    }
}

__global__ void __launch_bounds__(kPmThreads) pm_grid_kernel(PmGrid g, const float *q, int64_t nq, const float4 *table, int64_t T,
                                                             const int32_t *cell_start, const int32_t *items, int64_t n_items, float *out_d2,
                                                             int32_t *out_j, float *out_b1, float *out_b2)
{
    const int64_t i = (int64_t)blockIdx.x * kPmThreads + threadIdx.x;
    if (i >= nq) return;
    const float px = q[3 * i], py = q[3 * i + 1], pz = q[3 * i + 2];
    PmBest best{ __builtin_inff(), -1, 0.f, 0.f };
    if (!pm_finite3(px, py, pz)) {
        pm_store(false, best, i, out_d2, out_j, out_b1, out_b2);
        return;
    }
    const int gx = g.nn.n[0], gy = g.nn.n[1], gz = g.nn.n[2];
    const int64_t G = (int64_t)gx * gy * gz;
    if (!g.walk) {
        // cells so small against the coordinates that the stopping rule's slack no longer covers a candidate's rounding: every list once
        pm_visit_items(px, py, pz, table, T, items, n_items, 0, n_items, &best);
    } else {
        pm_visit_items(px, py, pz, table, T, items, n_items, cell_start[G], cell_start[G + 1], &best);           // the overflow list
        const int cx = grid_axis_cell(px, g.nn.lo[0], g.nn.inv_cell[0], gx), cy = grid_axis_cell(py, g.nn.lo[1], g.nn.inv_cell[1], gy);
        const int cz = grid_axis_cell(pz, g.nn.lo[2], g.nn.inv_cell[2], gz);
        // the last shell that still touches the grid
        const int r_max = max(max(max(cx, gx - 1 - cx), max(cy, gy - 1 - cy)), max(cz, gz - 1 - cz));
        for (int r = 0; r <= r_max; ++r) {
            const int z0 = max(cz - r, 0), z1 = min(cz + r, gz - 1), y0 = max(cy - r, 0), y1 = min(cy + r, gy - 1);
            const int x0 = max(cx - r, 0), x1 = min(cx + r, gx - 1);
            for (int z = z0; z <= z1; ++z)
                for (int y = y0; y <= y1; ++y) {
                    const int64_t row = ((int64_t)z * gy + y) * gx;
                    const bool face = z - cz == r || cz - z == r || y - cy == r || cy - y == r;
                    // a row on the shell's z or y face: all its cells, one contiguous range of `items`; otherwise the two cells at x = cx -+ r
                    for (int side = 0; side < (face ? 1 : 2); ++side) {
                        int xa, xb;
                        if (face) { xa = x0; xb = x1; }
                        else {
                            xa = xb = side == 0 ? cx - r : cx + r;
                            if (xa < 0 || xa >= gx) continue;
                        }
                        pm_visit_items(px, py, pz, table, T, items, n_items, cell_start[row + xa], cell_start[row + xb + 1], &best);
                    }
                }
            const float lb = __fmul_rn((float)r, g.nn.safe_cell);
            const float lb2 = __fmul_rn(lb, lb);
            if (lb2 > best.d2 && lb2 >= 1e-30f) break;          // every unvisited triangle is farther than the best one (header)
        }
    }
    pm_store(true, best, i, out_d2, out_j, out_b1, out_b2);
}

void launch_point_mesh_brute(const float *q, int64_t nq, const float *v, int64_t V, const int32_t *tri, int64_t T, float *d2, int32_t *triangle, float *b1,
                             float *b2, hipStream_t s)
{
    if (nq <= 0) return;
    hipLaunchKernelGGL(pm_brute_kernel, dim3((unsigned)((nq + kPmThreads - 1) / kPmThreads)), dim3(kPmThreads), 0, s, q, nq, v, V, tri, T, d2, triangle,
                       b1, b2);
}

void launch_point_mesh_prepare(const float *v, int64_t V, const int32_t *tri, int64_t T, float *table, hipStream_t s)
{
    if (T > 0)
        hipLaunchKernelGGL(pm_prepare_kernel, dim3((unsigned)((T + kPmThreads - 1) / kPmThreads)), dim3(kPmThreads), 0, s, v, V, tri, T, (float4 *)table);
}

void launch_point_mesh_grid_query(const PmGrid &g, const float *q, int64_t nq, const float *v, int64_t V, const int32_t *tri, int64_t T, float *table,
                                  const int32_t *cell_start, const int32_t *items, int64_t n_items, float *d2, int32_t *triangle, float *b1, float *b2,
                                  hipStream_t s)
{
    if (nq <= 0) return;
    launch_point_mesh_prepare(v, V, tri, T, table, s);
    hipLaunchKernelGGL(pm_grid_kernel, dim3((unsigned)((nq + kPmThreads - 1) / kPmThreads)), dim3(kPmThreads), 0, s, g, q, nq, (const float4 *)table, T,
                       cell_start, items, n_items, d2, triangle, b1, b2);
}

}  // namespace neddf
