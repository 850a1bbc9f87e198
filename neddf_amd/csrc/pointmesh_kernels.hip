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
#include "kernels.h"

namespace neddf {

constexpr int kPmThreads = 256;          // queries per workgroup and triangles per LDS tile
constexpr int kPmVec = 5;                // float4 per triangle

struct PmBest {
    float d2;
    int32_t j;
    float b1, b2;
};

__device__ __forceinline__ float pm_dot(float x0, float x1, float x2, float y0, float y1, float y2)
{
    return __fadd_rn(__fadd_rn(__fmul_rn(x0, y0), __fmul_rn(x1, y1)), __fmul_rn(x2, y2));
}

__device__ __forceinline__ float pm_clamp01(float u) { return u > 0.f ? (u < 1.f ? u : 1.f) : 0.f; }          // a NaN gives 0

// the constants of triangle j; an index outside [0, V) or a non-finite vertex gives valid = 0 and harmless zeros
__device__ __forceinline__ void pm_constants(const float *v, int64_t V, const int32_t *tri, int64_t j, float4 *out)
{
    const int64_t i0 = tri[3 * j], i1 = tri[3 * j + 1], i2 = tri[3 * j + 2];
    float p[9] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
    bool ok = !(i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V);
    if (ok) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            p[a] = v[3 * i0 + a]; p[3 + a] = v[3 * i1 + a]; p[6 + a] = v[3 * i2 + a];
            ok = ok && __builtin_isfinite(p[a]) && __builtin_isfinite(p[3 + a]) && __builtin_isfinite(p[6 + a]);
        }
    }
    if (!ok) {
#pragma unroll
        for (int a = 0; a < 9; ++a) p[a] = 0.f;
    }
    const float e0x = __fsub_rn(p[3], p[0]), e0y = __fsub_rn(p[4], p[1]), e0z = __fsub_rn(p[5], p[2]);
    const float e1x = __fsub_rn(p[6], p[0]), e1y = __fsub_rn(p[7], p[1]), e1z = __fsub_rn(p[8], p[2]);
    const float e2x = __fsub_rn(p[6], p[3]), e2y = __fsub_rn(p[7], p[4]), e2z = __fsub_rn(p[8], p[5]);
    const float g00 = pm_dot(e0x, e0y, e0z, e0x, e0y, e0z), g01 = pm_dot(e0x, e0y, e0z, e1x, e1y, e1z);
    const float g11 = pm_dot(e1x, e1y, e1z, e1x, e1y, e1z), g22 = pm_dot(e2x, e2y, e2z, e2x, e2y, e2z);
    const float r00 = __fdiv_rn(1.f, g00), m = __fmul_rn(g01, r00);
    const float fx = __fsub_rn(e1x, __fmul_rn(m, e0x)), fy = __fsub_rn(e1y, __fmul_rn(m, e0y)), fz = __fsub_rn(e1z, __fmul_rn(m, e0z));
    const float gpp = pm_dot(fx, fy, fz, fx, fy, fz);
    const float rpp = gpp > 0.f ? __fdiv_rn(1.f, gpp) : __builtin_nanf("");
    out[0] = make_float4(p[0], p[1], p[2], ok ? 1.f : 0.f);
    out[1] = make_float4(p[3], p[4], p[5], g01);
    out[2] = make_float4(p[6], p[7], p[8], r00);
    out[3] = make_float4(fx, fy, fz, rpp);
    out[4] = make_float4(__fdiv_rn(1.f, g11), __fdiv_rn(1.f, g22), 0.f, 0.f);
}

// one edge candidate: the clamped foot of p on s + u e; replaces (D2, b1, b2) when strictly smaller (a NaN compares false)
__device__ __forceinline__ void pm_edge(float px, float py, float pz, float sx, float sy, float sz, float ex, float ey, float ez, float h, float r, int which,
                                        float *D2, float *b1, float *b2)
{
    const float u = pm_clamp01(__fmul_rn(h, r));
    const float dx = __fsub_rn(px, __fadd_rn(sx, __fmul_rn(u, ex))), dy = __fsub_rn(py, __fadd_rn(sy, __fmul_rn(u, ey)));
    const float dz = __fsub_rn(pz, __fadd_rn(sz, __fmul_rn(u, ez)));
    const float d = pm_dot(dx, dy, dz, dx, dy, dz);
    const bool take = d < *D2;
    *D2 = take ? d : *D2;
    *b1 = take ? (which == 0 ? u : (which == 1 ? __fsub_rn(1.f, u) : 0.f)) : *b1;
    *b2 = take ? (which == 0 ? 0.f : u) : *b2;
}

// triangle j (its five float4) against one query: selects only
__device__ __forceinline__ void pm_visit(float px, float py, float pz, const float4 &c0, const float4 &c1, const float4 &c2, const float4 &c3, const float4 &c4,
                                         int32_t j, PmBest *best)
{
    const float ax = c0.x, ay = c0.y, az = c0.z, bx = c1.x, by = c1.y, bz = c1.z;
    const float g01 = c1.w, r00 = c2.w, fx = c3.x, fy = c3.y, fz = c3.z, rpp = c3.w, r11 = c4.x, r22 = c4.y;
    const float e0x = __fsub_rn(bx, ax), e0y = __fsub_rn(by, ay), e0z = __fsub_rn(bz, az);
    const float e1x = __fsub_rn(c2.x, ax), e1y = __fsub_rn(c2.y, ay), e1z = __fsub_rn(c2.z, az);
    const float e2x = __fsub_rn(c2.x, bx), e2y = __fsub_rn(c2.y, by), e2z = __fsub_rn(c2.z, bz);
    const float apx = __fsub_rn(px, ax), apy = __fsub_rn(py, ay), apz = __fsub_rn(pz, az);
    const float bpx = __fsub_rn(px, bx), bpy = __fsub_rn(py, by), bpz = __fsub_rn(pz, bz);
    const float d1 = pm_dot(e0x, e0y, e0z, apx, apy, apz), d2 = pm_dot(e1x, e1y, e1z, apx, apy, apz), d3 = pm_dot(e2x, e2y, e2z, bpx, bpy, bpz);
    // the interior candidate (rpp is NaN unless gpp > 0): solve, then one step of iterative refinement on the residual
    float ww = __fmul_rn(pm_dot(fx, fy, fz, apx, apy, apz), rpp);
    float vv = __fmul_rn(__fsub_rn(d1, __fmul_rn(ww, g01)), r00);
    float ix = __fsub_rn(px, __fadd_rn(__fadd_rn(ax, __fmul_rn(vv, e0x)), __fmul_rn(ww, e1x)));
    float iy = __fsub_rn(py, __fadd_rn(__fadd_rn(ay, __fmul_rn(vv, e0y)), __fmul_rn(ww, e1y)));
    float iz = __fsub_rn(pz, __fadd_rn(__fadd_rn(az, __fmul_rn(vv, e0z)), __fmul_rn(ww, e1z)));
    const float dw = __fmul_rn(pm_dot(fx, fy, fz, ix, iy, iz), rpp);
    const float dv = __fmul_rn(__fsub_rn(pm_dot(e0x, e0y, e0z, ix, iy, iz), __fmul_rn(dw, g01)), r00);
    vv = __fadd_rn(vv, dv);
    ww = __fadd_rn(ww, dw);
    ix = __fsub_rn(px, __fadd_rn(__fadd_rn(ax, __fmul_rn(vv, e0x)), __fmul_rn(ww, e1x)));
    iy = __fsub_rn(py, __fadd_rn(__fadd_rn(ay, __fmul_rn(vv, e0y)), __fmul_rn(ww, e1y)));
    iz = __fsub_rn(pz, __fadd_rn(__fadd_rn(az, __fmul_rn(vv, e0z)), __fmul_rn(ww, e1z)));
    const float Di = pm_dot(ix, iy, iz, ix, iy, iz);
    const bool inside = vv > 0.f && ww > 0.f && __fadd_rn(vv, ww) < 1.f && Di < __builtin_inff();
    float D2 = inside ? Di : __builtin_inff(), b1 = inside ? vv : 0.f, b2 = inside ? ww : 0.f;
    pm_edge(px, py, pz, ax, ay, az, e0x, e0y, e0z, d1, r00, 0, &D2, &b1, &b2);
    pm_edge(px, py, pz, bx, by, bz, e2x, e2y, e2z, d3, r22, 1, &D2, &b1, &b2);
    pm_edge(px, py, pz, ax, ay, az, e1x, e1y, e1z, d2, r11, 2, &D2, &b1, &b2);
    // the corner c: a and b are reached exactly by u = 0 of ab and bc, c only through a product that may round (header)
    const float cpx = __fsub_rn(px, c2.x), cpy = __fsub_rn(py, c2.y), cpz = __fsub_rn(pz, c2.z);
    const float Dc = pm_dot(cpx, cpy, cpz, cpx, cpy, cpz);
    const bool corner = Dc < D2;
    D2 = corner ? Dc : D2;
    b1 = corner ? 0.f : b1;
    b2 = corner ? 1.f : b2;
    const bool take = c0.w != 0.f && (D2 < best->d2 || (D2 == best->d2 && (uint32_t)j < (uint32_t)best->j));
    best->d2 = take ? D2 : best->d2;
    best->j = take ? j : best->j;
    best->b1 = take ? b1 : best->b1;
    best->b2 = take ? b2 : best->b2;
}

__device__ __forceinline__ void pm_store(bool ok, const PmBest &best, int64_t i, float *out_d2, int32_t *out_j, float *out_b1, float *out_b2)
{
    const float nan = __builtin_nanf("");
    out_d2[i] = ok ? best.d2 : nan;
    out_j[i] = ok ? best.j : -1;
    out_b1[i] = ok ? best.b1 : nan;
    out_b2[i] = ok ? best.b2 : nan;
}

__device__ __forceinline__ bool pm_finite3(float x, float y, float z) { return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z); }

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

void launch_point_mesh_grid_query(const PmGrid &g, const float *q, int64_t nq, const float *v, int64_t V, const int32_t *tri, int64_t T, float *table,
                                  const int32_t *cell_start, const int32_t *items, int64_t n_items, float *d2, int32_t *triangle, float *b1, float *b2,
                                  hipStream_t s)
{
    if (nq <= 0) return;
    if (T > 0)
        hipLaunchKernelGGL(pm_prepare_kernel, dim3((unsigned)((T + kPmThreads - 1) / kPmThreads)), dim3(kPmThreads), 0, s, v, V, tri, T, (float4 *)table);
    hipLaunchKernelGGL(pm_grid_kernel, dim3((unsigned)((nq + kPmThreads - 1) / kPmThreads)), dim3(kPmThreads), 0, s, g, q, nq, (const float4 *)table, T,
                       cell_start, items, n_items, d2, triangle, b1, b2);
}

}  // namespace neddf
