// raycast_kernels.hip -- the first intersection of rays with an indexed triangle mesh (no reference counterpart: the reference looks at
// meshes through its Open3D viewer).
//
//   rc_brute_kernel       one lane per ray, every triangle, triangle tiles (nine floats and a validity flag) staged through LDS
//   rc_hist_kernel        one lane per triangle: one integer atomicAdd into the count of every cell it is listed in
//   rc_block_kernel / rc_start_kernel   cell counts -> cell_start (count -> scan -> write over the G + 1 lists, block_scan.h)
//   rc_place_kernel       triangle indices grouped by list (an integer atomicAdd on the list's cursor)
//   rc_grid_kernel        one lane per ray: the overflow list, then a 3D-DDA through the cells
//
// THE HIT (include/neddf_hip.h states it; tests/raycast_check.py restates it in numpy bit for bit).  The watertight test of Woop,
// Benthin and Wald (JCGT 2013): the ray is sheared onto its dominant axis, the three edge functions are differences of two rounded
// products, and the edge functions of two triangles over a shared edge are exact negations of each other -- as long as no
// multiply-add is fused (-ffp-contract=off and the __f*_rn intrinsics below) a ray cannot slip between them.  Every operation of
// rc_visit is one rounded fp32 operation, except the fp64 recomputation of edge functions that came out exactly 0.  best = (+inf, -1);
// a candidate replaces it when t < best, or t == best and its index is below the current one (-1 counts as highest: the compare is
// unsigned): the lowest index that attains the smallest t wins WHATEVER the visiting order, which makes the grid's answer
// independent of the order inside a cell (that order comes from atomics and depends on timing) and of how often a triangle is met.
//
// THE GRID.  Cells and cell function are neddf_nn_grid_build's (kernels.h grid_axis_cell: monotone in p, points outside the box land in
// border cells).  A valid triangle whose box, widened by 2 pad, lies inside the grid's box widened by 2 pad is listed in the cells
// cell(min3 - 2 pad) .. cell(max3 + 2 pad) per axis; any other valid triangle goes into the overflow list (index G), which every ray
// tests by brute force.  The walk covers the ray inside the box widened by 2 pad; border cells reach out to infinity, so the walk
// never leaves the grid -- it ends at the clipped end of the ray, or once the best t lies before the exit of the current cell.  The
// exit parameter of a cell is computed afresh from its integer index in fp64, never accumulated.  Why this returns the brute
// kernel's bits: include/neddf_hip.h, "the equality argument".
#include "kernels.h"
#include "block_scan.h"
#include "raycast_device.h"           // rc_ray_setup, rc_visit, rc_triangle, rc_store: the per-pair arithmetic, shared with bvh_kernels.hip

namespace neddf {

constexpr int kRcThreads = 256;          // rays per workgroup and triangles per LDS tile

__global__ void __launch_bounds__(kRcThreads) rc_brute_kernel(const float *ro, const float *rd, int64_t nr, const float *v, int64_t V, const int32_t *tri,
                                                              int64_t T, float t_min, float t_max, float pad, float *out_t, int32_t *out_j,
                                                              float *out_b1, float *out_b2)
{
    __shared__ float4 tile[3][kRcThreads];      // (p0, valid), (p1, -), (p2, -)
    const int64_t i = (int64_t)blockIdx.x * kRcThreads + threadIdx.x;
    const bool live = i < nr;
    RcRay r;
    const bool ok = rc_ray_setup(live ? ro[3 * i] : 0.f, live ? ro[3 * i + 1] : 0.f, live ? ro[3 * i + 2] : 0.f, live ? rd[3 * i] : 0.f,
                                 live ? rd[3 * i + 1] : 0.f, live ? rd[3 * i + 2] : 1.f, &r);
    RcHit best{ __builtin_inff(), -1, 0.f, 0.f };
    for (int64_t base = 0; base < T; base += kRcThreads) {
        const int64_t j = base + threadIdx.x;
        float p[9] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
        const bool valid = j < T && rc_triangle(v, V, tri, j, p);
        __syncthreads();                 // the tile of the round before has been read by everyone
        tile[0][threadIdx.x] = make_float4(p[0], p[1], p[2], valid ? 1.f : 0.f);
        tile[1][threadIdx.x] = make_float4(p[3], p[4], p[5], 0.f);
        tile[2][threadIdx.x] = make_float4(p[6], p[7], p[8], 0.f);
        __syncthreads();
        const int n = (int)(T - base < kRcThreads ? T - base : kRcThreads);
        for (int k = 0; k < n; ++k) {
            const float4 a = tile[0][k];         // one address for the whole wave: a broadcast read
            if (a.w == 0.f) continue;            // (uniform over the workgroup)
            const float4 b = tile[1][k], c = tile[2][k];
            rc_visit(r, t_min, t_max, pad, a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z, (int32_t)(base + k), &best);
        }
    }
    if (live) rc_store(ok, best, i, out_t, out_j, out_b1, out_b2);
}

// ---- the grid ----
// where triangle j is listed: 0 = nowhere (invalid), 1 = the cells c0 .. c1 per axis, 2 = the overflow list
__device__ __forceinline__ int rc_triangle_cells(const RcGrid &g, const float *v, int64_t V, const int32_t *tri, int64_t j, int *c0, int *c1)
{
    float p[9];
    if (!rc_triangle(v, V, tri, j, p)) return 0;
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float lo = __fsub_rn(fminf(fminf(p[a], p[3 + a]), p[6 + a]), g.pad2), hi = __fadd_rn(fmaxf(fmaxf(p[a], p[3 + a]), p[6 + a]), g.pad2);
        inside = inside && lo >= g.wlo[a] && hi <= g.whi[a];
        c0[a] = grid_axis_cell(lo, g.nn.lo[a], g.nn.inv_cell[a], g.nn.n[a]);
        c1[a] = grid_axis_cell(hi, g.nn.lo[a], g.nn.inv_cell[a], g.nn.n[a]);
    }
    return inside ? 1 : 2;
}

// count[c] += 1 for every list c triangle j belongs to (place == 0), or items[cell_start[c] + cursor[c]++] = j (place != 0)
__global__ void __launch_bounds__(kMcThreads) rc_list_kernel(RcGrid g, const float *v, int64_t V, const int32_t *tri, int64_t T, int place,
                                                             const int32_t *cell_start, int32_t *count, int32_t *items)
{
    const int64_t j = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    if (j >= T) return;
    int c0[3], c1[3];
    const int where = rc_triangle_cells(g, v, V, tri, j, c0, c1);
    if (where == 0) return;
    const int64_t G = (int64_t)g.nn.n[0] * g.nn.n[1] * g.nn.n[2];
    if (where == 2) {
        const int32_t k = atomicAdd(count + G, 1);
        if (place) items[cell_start[G] + k] = (int32_t)j;
        return;
    }
    for (int z = c0[2]; z <= c1[2]; ++z)
        for (int y = c0[1]; y <= c1[1]; ++y)
            for (int x = c0[0]; x <= c1[0]; ++x) {
                const int64_t c = ((int64_t)z * g.nn.n[1] + y) * g.nn.n[0] + x;
                const int32_t k = atomicAdd(count + c, 1);
                if (place) items[cell_start[c] + k] = (int32_t)j;
            }
}

// (a list holds at most T < 2^31 triangles, 256 lists may hold more: the block totals are int64)
__global__ void __launch_bounds__(kMcThreads) rc_block_kernel(const int32_t *count, int64_t n_lists, int64_t *blk)
{
    __shared__ int64_t lds[kMcThreads / 64];
    const int64_t c = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    const int64_t total = block_sum(c < n_lists ? (int64_t)count[c] : (int64_t)0, lds);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

// cell_start[c] = the number of pairs in the lists before c, cell_start[n_lists] = all of them (the caller has checked that they fit
// int32); count is zeroed: the cursors of the placing launch
__global__ void __launch_bounds__(kMcThreads) rc_start_kernel(int32_t *count, int64_t n_lists, const int64_t *blk, int64_t n_blocks, int32_t *cell_start)
{
    __shared__ int64_t lds[kMcThreads];
    const int64_t c = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    int64_t total;
    const int64_t e = block_exclusive_scan(c < n_lists ? (int64_t)count[c] : (int64_t)0, lds, &total);
    if (c < n_lists) {
        cell_start[c] = (int32_t)(blk[blockIdx.x] + e);
        count[c] = 0;
    }
    if (c == n_lists - 1) cell_start[n_lists] = (int32_t)blk[n_blocks];
}

// the triangles items[k0 .. k1) against one ray (a range or an index that neddf_raycast_grid_build cannot have written is not followed)
__device__ __forceinline__ void rc_visit_items(const RcRay &r, float t_min, float t_max, float pad, const float *v, int64_t V, const int32_t *tri,
                                               int64_t T, const int32_t *items, int64_t n_items, int64_t k0, int64_t k1, RcHit *best)
{
    k1 = k1 < n_items ? k1 : n_items;
    for (int64_t k = k0 > 0 ? k0 : 0; k < k1; ++k) {
        const int32_t j = items[k];
        float p[9];
        if (j < 0 || j >= T || !rc_triangle(v, V, tri, j, p)) continue;
        rc_visit(r, t_min, t_max, pad, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], j, best);
    }
}

__global__ void __launch_bounds__(kRcThreads) rc_grid_kernel(RcGrid g, const float *ro, const float *rd, int64_t nr, const float *v, int64_t V,
                                                             const int32_t *tri, int64_t T, const int32_t *cell_start, const int32_t *items,
                                                             int64_t n_items, float t_min, float t_max, float *out_t, int32_t *out_j,
                                                             float *out_b1, float *out_b2)
{
    const int64_t i = (int64_t)blockIdx.x * kRcThreads + threadIdx.x;
    if (i >= nr) return;
    RcRay r;
    RcHit best{ __builtin_inff(), -1, 0.f, 0.f };
    if (!rc_ray_setup(ro[3 * i], ro[3 * i + 1], ro[3 * i + 2], rd[3 * i], rd[3 * i + 1], rd[3 * i + 2], &r)) {
        rc_store(false, best, i, out_t, out_j, out_b1, out_b2);
        return;
    }
    const float pad = g.pad;
    if (!(fmaxf(fmaxf(fabsf(r.ox), fabsf(r.oy)), fabsf(r.oz)) <= g.far_origin)) {
        // an origin so far away that the rounding of o + t d is no longer small against pad: every triangle, as the brute kernel
        for (int64_t j = 0; j < T; ++j) {
            float p[9];
            if (rc_triangle(v, V, tri, j, p)) rc_visit(r, t_min, t_max, pad, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], (int32_t)j, &best);
        }
        rc_store(true, best, i, out_t, out_j, out_b1, out_b2);
        return;
    }
    const int gn[3] = { g.nn.n[0], g.nn.n[1], g.nn.n[2] };
    const int64_t G = (int64_t)gn[0] * gn[1] * gn[2];
    rc_visit_items(r, t_min, t_max, pad, v, V, tri, T, items, n_items, cell_start[G], cell_start[G + 1], &best);          // the overflow list
    // the ray inside the box widened by 2 pad (slabs, fp64)
    const double o[3] = { (double)r.ox, (double)r.oy, (double)r.oz }, d[3] = { (double)r.dx, (double)r.dy, (double)r.dz };
    double t0 = (double)t_min, t1 = (double)t_max;
    bool empty = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double wl = (double)g.wlo[a], wh = (double)g.whi[a];
        if (d[a] == 0.0) empty = empty || o[a] < wl || o[a] > wh;
        else {
            const double ta = (wl - o[a]) / d[a], tb = (wh - o[a]) / d[a];
            t0 = fmax(t0, fmin(ta, tb));
            t1 = fmin(t1, fmax(ta, tb));
        }
    }
    if (!empty && t0 <= t1) {
        int c[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            c[a] = 0;
            if (g.edge[a] > 0.0) {              // (an axis without extent is one layer of cells: the cell function puts every point into cell 0)
                const double f = ((o[a] + t0 * d[a]) - g.lo[a]) / g.edge[a];
                c[a] = f >= (double)gn[a] ? gn[a] - 1 : (f > 0.0 ? (int)f : 0);
            }
        }
        const int max_steps = gn[0] + gn[1] + gn[2];        // every step moves one index towards a border and none moves back
        for (int step = 0; step <= max_steps; ++step) {
            const int64_t cell = ((int64_t)c[2] * gn[1] + c[1]) * gn[0] + c[0];
            rc_visit_items(r, t_min, t_max, pad, v, V, tri, T, items, n_items, cell_start[cell], cell_start[cell + 1], &best);
            // where the ray leaves this cell, afresh from the integer index; a border cell has no far side
            double t_next = __builtin_inf();
            int axis = -1;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (!(g.edge[a] > 0.0) || d[a] == 0.0) continue;
                const bool up = d[a] > 0.0;
                if (up ? c[a] + 1 >= gn[a] : c[a] <= 0) continue;
                const double t_exit = ((g.lo[a] + (double)(up ? c[a] + 1 : c[a]) * g.edge[a]) - o[a]) / d[a];
                if (t_exit < t_next) { t_next = t_exit; axis = a; }
            }
            if (axis < 0 || !(t_next < t1)) break;
            if ((double)best.t < t_next - 1e-6 * fabs(t_next)) break;      // every triangle hit before t_next is listed in a cell already visited
            c[axis] += d[axis] > 0.0 ? 1 : -1;
        }
    }
    rc_store(true, best, i, out_t, out_j, out_b1, out_b2);
}

void launch_raycast_brute(const float *ro, const float *rd, int64_t nr, const float *v, int64_t V, const int32_t *tri, int64_t T, float t_min,
                          float t_max, float pad, float *t, int32_t *triangle, float *b1, float *b2, hipStream_t s)
{
    if (nr <= 0) return;
    hipLaunchKernelGGL(rc_brute_kernel, dim3((unsigned)((nr + kRcThreads - 1) / kRcThreads)), dim3(kRcThreads), 0, s, ro, rd, nr, v, V, tri, T, t_min,
                       t_max, pad, t, triangle, b1, b2);
}

void launch_raycast_grid_count(const RcGrid &g, const float *v, int64_t V, const int32_t *tri, int64_t T, int32_t *count, int64_t *blk, hipStream_t s)
{
    const int64_t n_lists = (int64_t)g.nn.n[0] * g.nn.n[1] * g.nn.n[2] + 1, nb = mc_blocks(n_lists);
    (void)hipMemsetAsync(count, 0, (size_t)n_lists * sizeof(int32_t), s);
    if (T > 0)
        hipLaunchKernelGGL(rc_list_kernel, dim3((unsigned)mc_blocks(T)), dim3(kMcThreads), 0, s, g, v, V, tri, T, 0, (const int32_t *)nullptr, count,
                           (int32_t *)nullptr);
    hipLaunchKernelGGL(rc_block_kernel, dim3((unsigned)nb), dim3(kMcThreads), 0, s, (const int32_t *)count, n_lists, blk);
    launch_scan_totals(blk, nb, s);
}

void launch_raycast_grid_place(const RcGrid &g, const float *v, int64_t V, const int32_t *tri, int64_t T, int32_t *count, const int64_t *blk,
                               int32_t *cell_start, int32_t *items, hipStream_t s)
{
    const int64_t n_lists = (int64_t)g.nn.n[0] * g.nn.n[1] * g.nn.n[2] + 1, nb = mc_blocks(n_lists);
    hipLaunchKernelGGL(rc_start_kernel, dim3((unsigned)nb), dim3(kMcThreads), 0, s, count, n_lists, blk, nb, cell_start);
    if (T > 0 && items)
        hipLaunchKernelGGL(rc_list_kernel, dim3((unsigned)mc_blocks(T)), dim3(kMcThreads), 0, s, g, v, V, tri, T, 1, (const int32_t *)cell_start, count,
                           items);
}

void launch_raycast_grid_query(const RcGrid &g, const float *ro, const float *rd, int64_t nr, const float *v, int64_t V, const int32_t *tri, int64_t T,
                               const int32_t *cell_start, const int32_t *items, int64_t n_items, float t_min, float t_max, float *t, int32_t *triangle,
                               float *b1, float *b2, hipStream_t s)
{
    if (nr <= 0) return;
    hipLaunchKernelGGL(rc_grid_kernel, dim3((unsigned)((nr + kRcThreads - 1) / kRcThreads)), dim3(kRcThreads), 0, s, g, ro, rd, nr, v, V, tri, T,
                       cell_start, items, n_items, t_min, t_max, t, triangle, b1, b2);
}

}  // namespace neddf
