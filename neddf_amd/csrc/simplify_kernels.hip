// simplify_kernels.hip -- mesh simplification by vertex clustering (no reference counterpart: the reference's users decimated in
// Open3D).  include/neddf_hip.h states the contract and the displacement bound; tests/simplify_check.py restates every kernel in numpy
// bit for bit.
//
//   simp_keys_kernel          one lane per vertex: cell of neddf_nn_grid_build's cell function << 32 | index, 2^62 | index when non-finite
//   (torch.sort of the keys: plumbing, as bvh.py and mesh.py sort theirs)
//   simp_head_*, simp_run_*   one lane per sorted key: a run of equal high words is a cluster, a non-finite vertex one of its own; run
//                             heads by count / scan / write (block_scan.h); the heads ranked again BY VERTEX INDEX give the cluster ids
//   simp_assign_kernel        one lane per sorted key: the cluster of every vertex, the [begin, end) of every cluster in the sorted keys
//   simp_pair_*               one lane per triangle: its distinct corner clusters as keys cluster << 32 | triangle, count / scan / write
//   (torch.sort of the pairs)
//   simp_place_kernel         one lane per cluster: the fp64 mean of its members in ascending vertex index, or the quadric solve
//   simp_attr_kernel          one lane per (cluster, column): the fp64 ordered mean of an attribute column
//   simp_triangle_kernel      one lane per triangle: corners -> clusters, collapsed ones dropped; the triple with its lowest id rotated
//                             to the front is the triangle's identity
//   (two stable torch.sorts of the triples)
//   simp_unique_kernel        one lane per sorted triple: the first of a run of equal triples is kept
// neddf_mesh_compact then drops the clusters nothing references.
//
// MAPPING.  The contract fixes the ORDER of every floating-point sum (ascending member index, ascending triangle index), and fp64
// addition is not associative: a tree over the lanes of a sub-wave group would compute another number.  So a cluster is one lane's,
// which walks its members (a cell K lattice steps wide holds about K^2 marching-cubes vertices: 4 to 64) with one 12-byte gather
// each; neighbouring clusters' members are neighbouring keys, their vertices near each other in marching cubes' order, so the
// gathers of a wave fall into few cache lines.  The degenerate input -- everything in one cell -- is one lane's loop over V members:
// slow, never wrong.  No float atomic anywhere: every sum has one owner.  The accumulators are scalars (a00 .. a22, r0 .. r2, three
// sums, three minima, three maxima), no array is indexed dynamically: the private segment of every kernel here is 0 bytes.
//
// Every index read from an array the caller sorted is checked before it is followed (a vertex index against V, a triangle index
// against T, a range against the key count): arrays that are not what the earlier steps made give a wrong answer, never an access
// outside them.
#include "kernels.h"
#include "block_scan.h"

namespace neddf {

constexpr int64_t kSimpNonFinite = (int64_t)1 << 62;

__device__ __forceinline__ bool simp_finite3(float x, float y, float z)
{
    return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
}

__global__ void __launch_bounds__(kMcThreads) simp_keys_kernel(NnGrid g, const float *v, int64_t V, int64_t *keys)
{
    const int64_t i = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    if (i >= V) return;
    const float x = v[3 * i], y = v[3 * i + 1], z = v[3 * i + 2];
    if (!simp_finite3(x, y, z)) {
        keys[i] = kSimpNonFinite | i;
        return;
    }
    const int64_t cx = grid_axis_cell(x, g.lo[0], g.inv_cell[0], g.n[0]), cy = grid_axis_cell(y, g.lo[1], g.inv_cell[1], g.n[1]),
                  cz = grid_axis_cell(z, g.lo[2], g.inv_cell[2], g.n[2]);
    keys[i] = (((cz * g.n[1] + cy) * g.n[0] + cx) << 32) | i;
}

// sorted key i starts a cluster: the first key, a non-finite vertex, or another cell than the key before
__device__ __forceinline__ bool simp_is_head(const int64_t *keys, int64_t i, int64_t V)
{
    if (i >= V) return false;
    if (i == 0) return true;
    const int64_t k = keys[i];
    return (k & kSimpNonFinite) != 0 || (k >> 32) != (keys[i - 1] >> 32);
}

// the vertex of a key, -1 for one no keys kernel can have written
__device__ __forceinline__ int64_t simp_vertex(int64_t key, int64_t V)
{
    const int64_t v = key & 0xffffffffll;
    return v < V ? v : -1;
}

// head_of_vertex [V] zeroed by the caller; sblk [mc_blocks(V) + 1]
__global__ void __launch_bounds__(kMcThreads) simp_head_count_kernel(const int64_t *keys, int64_t V, unsigned char *head_of_vertex, int64_t *sblk)
{
    const int64_t i = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    const bool head = simp_is_head(keys, i, V);
    if (head) {
        const int64_t v = simp_vertex(keys[i], V);
        if (v >= 0) head_of_vertex[v] = 1;
    }
    const int n = __syncthreads_count(head);
    if (threadIdx.x == 0) sblk[blockIdx.x] = n;
}

// run_start [V + 1]: the sorted position at which run r begins, [number of runs] = V
__global__ void __launch_bounds__(kMcThreads) simp_run_start_kernel(const int64_t *keys, int64_t V, const int64_t *sblk, int64_t nb, int32_t *run_start)
{
    __shared__ int lds[kMcThreads / 64];
    const int64_t i = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    const bool head = simp_is_head(keys, i, V);
    const int rank = block_rank(head, lds);
    if (head) run_start[sblk[blockIdx.x] + rank] = (int32_t)i;
    if (i == V - 1) run_start[sblk[nb]] = (int32_t)V;
}

__global__ void __launch_bounds__(kMcThreads) simp_head_rank_count_kernel(const unsigned char *head_of_vertex, int64_t V, int64_t *vblk)
{
    const int64_t v = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    const int n = __syncthreads_count(v < V && head_of_vertex[v]);
    if (threadIdx.x == 0) vblk[blockIdx.x] = n;
}

// the heads get their cluster id: their rank among the heads in VERTEX order; the other vertices are filled in by simp_assign_kernel
__global__ void __launch_bounds__(kMcThreads) simp_head_id_kernel(const unsigned char *head_of_vertex, int64_t V, const int64_t *vblk, int32_t *vertex_cluster)
{
    __shared__ int lds[kMcThreads / 64];
    const int64_t v = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    const bool head = v < V && head_of_vertex[v];
    const int rank = block_rank(head, lds);
    if (head) vertex_cluster[v] = (int32_t)(vblk[blockIdx.x] + rank);
}

// a member reads its head's entry, which the launch before wrote and this one leaves alone; cluster_range [C][2] from the heads
__global__ void __launch_bounds__(kMcThreads) simp_assign_kernel(const int64_t *keys, int64_t V, const int64_t *sblk, int64_t nb, const int32_t *run_start,
                                                                 int32_t *vertex_cluster, int32_t *cluster_range)
{
    __shared__ int lds[kMcThreads / 64];
    const int64_t i = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    const bool head = simp_is_head(keys, i, V);
    const int rank = block_rank(head, lds);
    if (i >= V) return;
    const int64_t runs = sblk[nb], r = sblk[blockIdx.x] + rank - (head ? 0 : 1);
    if (r < 0 || r >= runs) return;
    const int64_t b = run_start[r], e = run_start[r + 1];
    if (b < 0 || b >= V) return;
    const int64_t hv = simp_vertex(keys[b], V);
    if (hv < 0) return;
    const int32_t c = vertex_cluster[hv];
    if (head) {
        if (c < 0 || c >= runs) return;
        cluster_range[2 * (int64_t)c] = (int32_t)b;
        cluster_range[2 * (int64_t)c + 1] = (int32_t)e;
        return;
    }
    const int64_t v = simp_vertex(keys[i], V);
    if (v >= 0) vertex_cluster[v] = c;
}

// ---- cluster -> triangle pairs ---------------------------------------------------------------------------------------------------
// a triangle is valid when its indices lie in [0, V) and its corners are finite; cl[0 .. n) = the distinct clusters of its corners in
// corner order
__device__ __forceinline__ int simp_pair_clusters(const float *v, int64_t V, const int32_t *tri, int64_t T, int64_t t, const int32_t *vertex_cluster, int32_t cl[3])
{
    if (t >= T) return 0;
    const int64_t i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
    if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) return 0;
    if (!simp_finite3(v[3 * i0], v[3 * i0 + 1], v[3 * i0 + 2]) || !simp_finite3(v[3 * i1], v[3 * i1 + 1], v[3 * i1 + 2]) ||
        !simp_finite3(v[3 * i2], v[3 * i2 + 1], v[3 * i2 + 2]))
        return 0;
    const int32_t c0 = vertex_cluster[i0], c1 = vertex_cluster[i1], c2 = vertex_cluster[i2];
    int n = 0;
    cl[n++] = c0;
    if (c1 != c0) cl[n++] = c1;
    if (c2 != c0 && c2 != c1) cl[n++] = c2;
    return n;
}

__global__ void __launch_bounds__(kMcThreads) simp_pair_count_kernel(const float *v, int64_t V, const int32_t *tri, int64_t T, const int32_t *vertex_cluster,
                                                                     int64_t *pblk)
{
    __shared__ int lds[kMcThreads / 64];
    const int64_t t = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    int32_t cl[3];
    const int total = block_sum(simp_pair_clusters(v, V, tri, T, t, vertex_cluster, cl), lds);
    if (threadIdx.x == 0) pblk[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kMcThreads) simp_pair_write_kernel(const float *v, int64_t V, const int32_t *tri, int64_t T, const int32_t *vertex_cluster,
                                                                     const int64_t *pblk, int64_t *pairs)
{
    __shared__ int lds[kMcThreads];
    const int64_t t = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    int32_t cl[3] = { 0, 0, 0 };
    const int n = simp_pair_clusters(v, V, tri, T, t, vertex_cluster, cl);
    int total;
    const int off = block_exclusive_scan(n, lds, &total);
    const int64_t o = pblk[blockIdx.x] + off;
    if (n > 0) pairs[o] = ((int64_t)cl[0] << 32) | t;
    if (n > 1) pairs[o + 1] = ((int64_t)cl[1] << 32) | t;
    if (n > 2) pairs[o + 2] = ((int64_t)cl[2] << 32) | t;
}

// ---- placement ---------------------------------------------------------------------------------------------------------------------
struct SimpClusters {
    const int64_t *keys;                 // [V] sorted
    const int32_t *range;                // [C][2]
    int64_t V, C;
};

// the first position of pairs [0, P) whose key is not below `key`
__device__ __forceinline__ int64_t simp_lower_bound(const int64_t *pairs, int64_t P, int64_t key)
{
    int64_t lo = 0, hi = P;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (pairs[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(kMcThreads) simp_place_kernel(SimpClusters k, const float *v, const int32_t *tri, int64_t T, const int64_t *pairs, int64_t P,
                                                                int quadric, double reg, float *out)
{
    const int64_t c = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    if (c >= k.C) return;
    unsigned *o = (unsigned *)out + 3 * c;
    const int64_t b = k.range[2 * c], e = k.range[2 * c + 1];
    o[0] = o[1] = o[2] = 0u;
    if (b < 0 || e > k.V || b >= e) return;
    if (e - b == 1) {                                    // a singleton, non-finite ones included: its own bits
        const int64_t i = simp_vertex(k.keys[b], k.V);
        if (i < 0) return;
        const unsigned *src = (const unsigned *)v + 3 * i;
        o[0] = src[0]; o[1] = src[1]; o[2] = src[2];
        return;
    }
    double sx = 0.0, sy = 0.0, sz = 0.0, lx = 0.0, ly = 0.0, lz = 0.0, hx = 0.0, hy = 0.0, hz = 0.0;
    for (int64_t j = b; j < e; ++j) {
        const int64_t i = simp_vertex(k.keys[j], k.V);
        if (i < 0) return;
        const double x = (double)v[3 * i], y = (double)v[3 * i + 1], z = (double)v[3 * i + 2];
        sx += x; sy += y; sz += z;                       // from +0.0, in member order
        if (j == b) {
            lx = hx = x; ly = hy = y; lz = hz = z;
        } else {
            lx = fmin(lx, x); ly = fmin(ly, y); lz = fmin(lz, z);
            hx = fmax(hx, x); hy = fmax(hy, y); hz = fmax(hz, z);
        }
    }
    const double cnt = (double)(e - b);
    const double mx = sx / cnt, my = sy / cnt, mz = sz / cnt;
    double px = mx, py = my, pz = mz;
    if (quadric) {
        double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, r0 = 0.0, r1 = 0.0, r2 = 0.0;
        const int64_t first = simp_lower_bound(pairs, P, c << 32), last = simp_lower_bound(pairs, P, (c + 1) << 32);
        for (int64_t j = first; j < last; ++j) {
            const int64_t t = pairs[j] & 0xffffffffll;
            if (t >= T) continue;
            const int64_t i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
            if (i0 < 0 || i0 >= k.V || i1 < 0 || i1 >= k.V || i2 < 0 || i2 >= k.V) continue;
            const double p0x = (double)v[3 * i0], p0y = (double)v[3 * i0 + 1], p0z = (double)v[3 * i0 + 2];
            const double ux = (double)v[3 * i1] - p0x, uy = (double)v[3 * i1 + 1] - p0y, uz = (double)v[3 * i1 + 2] - p0z;
            const double wx = (double)v[3 * i2] - p0x, wy = (double)v[3 * i2 + 1] - p0y, wz = (double)v[3 * i2 + 2] - p0z;
            const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
            a00 += nx * nx; a01 += nx * ny; a02 += nx * nz; a11 += ny * ny; a12 += ny * nz; a22 += nz * nz;
            const double d = (nx * (p0x - mx) + ny * (p0y - my)) + nz * (p0z - mz);
            r0 += nx * d; r1 += ny * d; r2 += nz * d;
        }
        const double tr = (a00 + a11) + a22;
        if (tr != 0.0 && __builtin_isfinite(tr)) {
            const double lam = (reg * tr) / 3.0;
            const double b00 = a00 + lam, b11 = a11 + lam, b22 = a22 + lam;
            const double c00 = b11 * b22 - a12 * a12, c01 = a02 * a12 - a01 * b22, c02 = a01 * a12 - a02 * b11;
            const double c11 = b00 * b22 - a02 * a02, c12 = a01 * a02 - b00 * a12, c22 = b00 * b11 - a01 * a01;
            const double det = (b00 * c00 + a01 * c01) + a02 * c02;
            if (det != 0.0 && __builtin_isfinite(det)) {
                const double y0 = ((c00 * r0 + c01 * r1) + c02 * r2) / det;
                const double y1 = ((c01 * r0 + c11 * r1) + c12 * r2) / det;
                const double y2 = ((c02 * r0 + c12 * r1) + c22 * r2) / det;
                if (__builtin_isfinite(y0) && __builtin_isfinite(y1) && __builtin_isfinite(y2)) {
                    px = mx + y0; py = my + y1; pz = mz + y2;
                }
            }
        }
        px = fmin(fmax(px, lx), hx); py = fmin(fmax(py, ly), hy); pz = fmin(fmax(pz, lz), hz);
    }
    out[3 * c] = (float)px; out[3 * c + 1] = (float)py; out[3 * c + 2] = (float)pz;
}

// attr [V][K] -> out [C][K]: a singleton's bits, otherwise the fp64 mean in member order, rounded once; a NaN result is 0x7fc00000
__global__ void __launch_bounds__(kMcThreads) simp_attr_kernel(SimpClusters k, const float *attr, int K, float *out)
{
    const int64_t q = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    if (q >= k.C * K) return;
    const int64_t c = q / K, col = q % K;
    const int64_t b = k.range[2 * c], e = k.range[2 * c + 1];
    unsigned *o = (unsigned *)out + q;
    *o = 0u;
    if (b < 0 || e > k.V || b >= e) return;
    if (e - b == 1) {
        const int64_t i = simp_vertex(k.keys[b], k.V);
        if (i >= 0) *o = ((const unsigned *)attr)[i * K + col];
        return;
    }
    double s = 0.0;
    for (int64_t j = b; j < e; ++j) {
        const int64_t i = simp_vertex(k.keys[j], k.V);
        if (i < 0) return;
        s += (double)attr[i * K + col];
    }
    const float m = (float)(s / (double)(e - b));
    *o = m != m ? 0x7fc00000u : __float_as_uint(m);
}

// ---- triangles -----------------------------------------------------------------------------------------------------------------------
// mapped [T][3]: the clusters of the corners in corner order, (-1, -1, -1) for a triangle with an index outside [0, V) or two corners
// in one cluster.  The triple rotated cyclically so that its lowest cluster comes first (the orientation stays) is (a, b, c):
// lowest [T] = a, key [T] = b << 31 | c; both -1 for a dropped one
__global__ void __launch_bounds__(kMcThreads) simp_triangle_kernel(const int32_t *tri, int64_t T, int64_t V, const int32_t *vertex_cluster, int32_t *mapped,
                                                                   int32_t *lowest, int64_t *key)
{
    const int64_t t = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    if (t >= T) return;
    const int64_t i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
    int32_t c0 = -1, c1 = -1, c2 = -1, a = -1, b = -1, c = -1;
    if (!(i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V)) {
        c0 = vertex_cluster[i0]; c1 = vertex_cluster[i1]; c2 = vertex_cluster[i2];
        if (c0 != c1 && c1 != c2 && c0 != c2 && c0 >= 0 && c1 >= 0 && c2 >= 0) {
            if (c0 < c1 && c0 < c2) { a = c0; b = c1; c = c2; }
            else if (c1 < c0 && c1 < c2) { a = c1; b = c2; c = c0; }
            else { a = c2; b = c0; c = c1; }
        } else {
            c0 = c1 = c2 = -1;
        }
    }
    mapped[3 * t] = c0; mapped[3 * t + 1] = c1; mapped[3 * t + 2] = c2;
    lowest[t] = a;
    key[t] = a < 0 ? (int64_t)-1 : (((int64_t)b << 31) | (int64_t)c);
}

// order [T]: the triangles sorted by their rotated triple, equal triples in ascending index; keep [T]: 1 for the first of each run of
// equal triples that is not a dropped one
__global__ void __launch_bounds__(kMcThreads) simp_unique_kernel(const int32_t *lowest, const int64_t *key, int64_t T, const int64_t *order, unsigned char *keep)
{
    const int64_t i = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    if (i >= T) return;
    const int64_t t = order[i];
    if (t < 0 || t >= T) return;
    const int32_t a = lowest[t];
    bool first = a >= 0;
    if (first && i > 0) {
        const int64_t p = order[i - 1];
        if (p >= 0 && p < T) first = !(lowest[p] == a && key[p] == key[t]);
    }
    keep[t] = first ? 1 : 0;
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------
void launch_simplify_keys(const NnGrid &g, const float *v, int64_t V, int64_t *keys, hipStream_t s)
{
    if (V <= 0) return;
    hipLaunchKernelGGL(simp_keys_kernel, dim3((unsigned)mc_blocks(V)), dim3(kMcThreads), 0, s, g, v, V, keys);
}

void launch_simplify_clusters(const int64_t *keys, int64_t V, unsigned char *head_of_vertex, int32_t *run_start, int64_t *sblk, int64_t *vblk,
                              int32_t *vertex_cluster, int32_t *cluster_range, hipStream_t s)
{
    const int64_t nb = mc_blocks(V);
    const dim3 grid((unsigned)nb), block(kMcThreads);
    if (V > 0) {
        (void)hipMemsetAsync(head_of_vertex, 0, (size_t)V, s);
        hipLaunchKernelGGL(simp_head_count_kernel, grid, block, 0, s, keys, V, head_of_vertex, sblk);
    }
    launch_scan_totals(sblk, nb, s);
    if (V <= 0) return;
    hipLaunchKernelGGL(simp_run_start_kernel, grid, block, 0, s, keys, V, (const int64_t *)sblk, nb, run_start);
    hipLaunchKernelGGL(simp_head_rank_count_kernel, grid, block, 0, s, (const unsigned char *)head_of_vertex, V, vblk);
    launch_scan_totals(vblk, nb, s);
    hipLaunchKernelGGL(simp_head_id_kernel, grid, block, 0, s, (const unsigned char *)head_of_vertex, V, (const int64_t *)vblk, vertex_cluster);
    hipLaunchKernelGGL(simp_assign_kernel, grid, block, 0, s, keys, V, (const int64_t *)sblk, nb, (const int32_t *)run_start, vertex_cluster, cluster_range);
}

void launch_simplify_pair_count(const float *v, int64_t V, const int32_t *tri, int64_t T, const int32_t *vertex_cluster, int64_t *pblk, hipStream_t s)
{
    const int64_t nb = mc_blocks(T);
    if (T > 0) hipLaunchKernelGGL(simp_pair_count_kernel, dim3((unsigned)nb), dim3(kMcThreads), 0, s, v, V, tri, T, vertex_cluster, pblk);
    launch_scan_totals(pblk, nb, s);
}

void launch_simplify_pair_write(const float *v, int64_t V, const int32_t *tri, int64_t T, const int32_t *vertex_cluster, const int64_t *pblk, int64_t *pairs,
                                hipStream_t s)
{
    if (T > 0) hipLaunchKernelGGL(simp_pair_write_kernel, dim3((unsigned)mc_blocks(T)), dim3(kMcThreads), 0, s, v, V, tri, T, vertex_cluster, pblk, pairs);
}

void launch_simplify_place(const int64_t *keys, int64_t V, const int32_t *cluster_range, int64_t C, const float *v, const int32_t *tri, int64_t T,
                           const int64_t *pairs, int64_t P, int quadric, double reg, float *out, hipStream_t s)
{
    if (C <= 0) return;
    const SimpClusters k{ keys, cluster_range, V, C };
    hipLaunchKernelGGL(simp_place_kernel, dim3((unsigned)mc_blocks(C)), dim3(kMcThreads), 0, s, k, v, tri, T, pairs, P, quadric, reg, out);
}

void launch_simplify_attributes(const int64_t *keys, int64_t V, const int32_t *cluster_range, int64_t C, const float *attr, int K, float *out, hipStream_t s)
{
    if (C <= 0 || K <= 0) return;
    const SimpClusters k{ keys, cluster_range, V, C };
    hipLaunchKernelGGL(simp_attr_kernel, dim3((unsigned)mc_blocks(C * K)), dim3(kMcThreads), 0, s, k, attr, K, out);
}

void launch_simplify_triangles(const int32_t *tri, int64_t T, int64_t V, const int32_t *vertex_cluster, int32_t *mapped, int32_t *lowest, int64_t *key,
                               hipStream_t s)
{
    if (T > 0) hipLaunchKernelGGL(simp_triangle_kernel, dim3((unsigned)mc_blocks(T)), dim3(kMcThreads), 0, s, tri, T, V, vertex_cluster, mapped, lowest, key);
}

void launch_simplify_unique(const int32_t *lowest, const int64_t *key, int64_t T, const int64_t *order, unsigned char *keep, hipStream_t s)
{
    if (T <= 0) return;
    (void)hipMemsetAsync(keep, 0, (size_t)T, s);         // an `order` that is no permutation leaves no flag unwritten
    hipLaunchKernelGGL(simp_unique_kernel, dim3((unsigned)mc_blocks(T)), dim3(kMcThreads), 0, s, lowest, key, T, order, keep);
}

}  // namespace neddf
