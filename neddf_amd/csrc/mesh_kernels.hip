// mesh_kernels.hip -- surface extraction (no reference kernel: the reference meshes on the host with PyMCubes,
// neddf/scripts/fields_visualizer.py:528-566).
//
//   grid_points_kernel   the lattice of neddf_field_grid: np.linspace coordinates per axis, x fastest
//   mc_count_kernel      per lattice point: which of the three edges it owns are crossed (one byte); per block: vertex and
//                        triangle totals
//   scan_totals_kernel   one workgroup: exclusive scan of an array of block totals (in place, the grand total behind them)
//   mc_vertex_kernel     per point: its first vertex id (block scan + block base), the vertices of its crossed edges
//   mc_triangle_kernel   per cell: its first triangle id (block scan + block base), the triangles of its case
//   mesh_normal_*        geometric vertex normals of an indexed mesh: area-weighted sums of the incident triangles' cross products,
//                        accumulated in 64-bit fixed point with INTEGER atomics (exact, hence order-independent), then normalised
//   cc_*                 connected components of an indexed mesh: union-find with atomicMin hooks and pointer jumps, dense labels
//   compact_*            order-preserving removal of triangles and of the vertices nothing references any more
//
// Placement is decided by count -> scan -> write launches only (block_scan.h): no atomics, no exchange between workgroups inside
// a launch, so the output is the same on every run (tests/mesh_check.py restates it in numpy bit for bit).  A corner is inside when
// value < iso; NaN compares false and is outside.  A vertex on an edge with a NaN end (t = NaN) sits at the edge's middle.
#include "kernels.h"
#include "block_scan.h"
#include "mc_tables.h"

namespace neddf {

// np.linspace(lo, hi, n)[i] rounded to float: lo + i * ((hi - lo) / (n - 1)) in double, the last one exactly hi
__device__ __forceinline__ float lattice_coord(double lo, double hi, int n, int i)
{
    if (i == n - 1) return (float)hi;
    const double step = (hi - lo) / (double)(n - 1);
    return (float)(lo + (double)i * step);
}

// the constant inputs of a point that is evaluated for its position alone (base_neuralfield.py:49-79): dir (1, 0, 0), var 0
__device__ __forceinline__ void unit_inputs(int64_t q, float *dir, float *var)
{
    dir[3 * q + 0] = 1.f; dir[3 * q + 1] = 0.f; dir[3 * q + 2] = 0.f;
    var[3 * q + 0] = 0.f; var[3 * q + 1] = 0.f; var[3 * q + 2] = 0.f;
}

__global__ void __launch_bounds__(kMcThreads) grid_points_kernel(McGrid g, int64_t first, int64_t n, float *pos, float *dir, float *var)
{
    const int64_t q = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    if (q >= n) return;
    const int64_t p = first + q;
    const int i = (int)(p % g.nx), j = (int)((p / g.nx) % g.ny), k = (int)(p / ((int64_t)g.nx * g.ny));
    pos[3 * q + 0] = lattice_coord(g.lo[0], g.hi[0], g.nx, i);
    pos[3 * q + 1] = lattice_coord(g.lo[1], g.hi[1], g.ny, j);
    pos[3 * q + 2] = lattice_coord(g.lo[2], g.hi[2], g.nz, k);
    unit_inputs(q, dir, var);
}

__device__ __forceinline__ bool inside(float v, float iso) { return v < iso; }

__device__ __forceinline__ int point_mask(const McGrid &g, int64_t p, int i, int j, int k)
{
    const bool in0 = inside(g.vol[p], g.iso);
    int m = 0;
    if (i + 1 < g.nx && inside(g.vol[p + 1], g.iso) != in0) m |= 1;
    if (j + 1 < g.ny && inside(g.vol[p + g.nx], g.iso) != in0) m |= 2;
    if (k + 1 < g.nz && inside(g.vol[p + (int64_t)g.nx * g.ny], g.iso) != in0) m |= 4;
    return m;
}

// case index of the cell whose corner 0 is v[0], in values with strides 1 / sy / sz (Bourke's corner numbering, mc_tables.h)
template <typename I> __device__ __forceinline__ int cell_case(const float *v, I sy, I sz, float iso)
{
    const I sx = 1;
    const I off[8] = { 0, sx, sx + sy, sy, sz, sx + sz, sx + sy + sz, sy + sz };
    int c = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) c |= inside(v[off[b]], iso) << b;
    return c;
}

__device__ __forceinline__ int dense_cell_case(const McGrid &g, int64_t p) { return cell_case(g.vol + p, (int64_t)g.nx, (int64_t)g.nx * g.ny, g.iso); }

__device__ __forceinline__ int case_triangles(int c)
{
    int n = 0;
    while (n < kMcMaxTris && kMcTriTable[c][3 * n] >= 0) ++n;
    return n;
}

// The vertices of the crossed edges `m` (bit a: the edge along axis a) of the fine lattice point idx[], written at ids id, id + 1, ...
// in axis order.  v0 = the point's value, next(a) = the value one step along axis a; vertex_key (or NULL) receives 3 p + a.
template <typename Next>
__device__ __forceinline__ void edge_vertices(const McGrid &g, const int idx[3], int m, float v0, Next next, int64_t id, float *vertices,
                                              int64_t *vertex_key)
{
    const int dim[3] = { g.nx, g.ny, g.nz };
    const float c[3] = { lattice_coord(g.lo[0], g.hi[0], g.nx, idx[0]), lattice_coord(g.lo[1], g.hi[1], g.ny, idx[1]),
                         lattice_coord(g.lo[2], g.hi[2], g.nz, idx[2]) };
    const int64_t p = ((int64_t)idx[2] * g.ny + idx[1]) * g.nx + idx[0];
    for (int a = 0; a < 3; ++a) {
        if (!(m >> a & 1)) continue;
        const float v1 = next(a);
        float t = (g.iso - v0) / (v1 - v0);
        if (t != t) t = 0.5f;
        const float g0 = c[a], g1 = lattice_coord(g.lo[a], g.hi[a], dim[a], idx[a] + 1);
        float out[3] = { c[0], c[1], c[2] };
        out[a] = g0 + t * (g1 - g0);
        vertices[3 * id + 0] = out[0];
        vertices[3 * id + 1] = out[1];
        vertices[3 * id + 2] = out[2];
        if (vertex_key) vertex_key[id] = 3 * p + a;
        ++id;
    }
}

// The vertex id of one triangle corner.  own (kMcEdgeOwner): the corner's edge runs along axis own >> 3 from the cell's point at offset
// (own & 1, own >> 1 & 1, own >> 2 & 1); point(dx, dy, dz, axis) = where that point's entries of vbase / mask are.  The id is the point's
// first vertex plus its crossed edges of lower axis.
template <typename Point>
__device__ __forceinline__ int32_t corner_vertex(int own, const int32_t *vbase, const unsigned char *mask, Point point)
{
    const int axis = own >> 3;
    const int64_t q = point(own & 1, (own >> 1) & 1, (own >> 2) & 1, axis);
    return vbase[q] + (int32_t)__popc(mask[q] & ((1 << axis) - 1));
}

__global__ void __launch_bounds__(kMcThreads) mc_count_kernel(McGrid g, unsigned char *mask, int64_t *vblk, int64_t *tblk)
{
    __shared__ int lds[kMcThreads / 64];
    const int64_t p = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    int nv = 0, nt = 0;
    if (p < g.n) {
        const int i = (int)(p % g.nx), j = (int)((p / g.nx) % g.ny), k = (int)(p / ((int64_t)g.nx * g.ny));
        const int m = point_mask(g, p, i, j, k);
        mask[p] = (unsigned char)m;
        nv = (int)__popc(m);
        if (i + 1 < g.nx && j + 1 < g.ny && k + 1 < g.nz) nt = case_triangles(dense_cell_case(g, p));
    }
    const int tv = block_sum(nv, lds), tt = block_sum(nt, lds);
    if (threadIdx.x == 0) { vblk[blockIdx.x] = tv; tblk[blockIdx.x] = tt; }
}

__global__ void __launch_bounds__(kMcThreads) mc_vertex_kernel(McGrid g, const unsigned char *mask, const int64_t *vblk, int32_t *vbase,
                                                               float *vertices)
{
    __shared__ int lds[kMcThreads];
    const int64_t p = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    const int m = p < g.n ? mask[p] : 0;
    int total;
    const int off = block_exclusive_scan((int)__popc(m), lds, &total);
    if (p >= g.n) return;
    const int64_t id = vblk[blockIdx.x] + off;
    vbase[p] = (int32_t)id;
    if (!m) return;
    const int idx[3] = { (int)(p % g.nx), (int)((p / g.nx) % g.ny), (int)(p / ((int64_t)g.nx * g.ny)) };
    const int64_t stride[3] = { 1, g.nx, (int64_t)g.nx * g.ny };
    edge_vertices(g, idx, m, g.vol[p], [&](int a) { return g.vol[p + stride[a]]; }, id, vertices, nullptr);
}

__global__ void __launch_bounds__(kMcThreads) mc_triangle_kernel(McGrid g, const unsigned char *mask, const int64_t *tblk,
                                                                 const int32_t *vbase, int32_t *tris)
{
    __shared__ int lds[kMcThreads];
    const int64_t p = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    int c = 0, nt = 0;
    if (p < g.n) {
        const int i = (int)(p % g.nx), j = (int)((p / g.nx) % g.ny), k = (int)(p / ((int64_t)g.nx * g.ny));
        if (i + 1 < g.nx && j + 1 < g.ny && k + 1 < g.nz) {
            c = dense_cell_case(g, p);
            nt = case_triangles(c);
        }
    }
    int total;
    const int off = block_exclusive_scan(nt, lds, &total);
    if (!nt) return;
    const int64_t first = tblk[blockIdx.x] + off;
    const int64_t sy = g.nx, sz = (int64_t)g.nx * g.ny;
    for (int e = 0; e < 3 * nt; ++e)
        tris[3 * first + e] = corner_vertex(kMcEdgeOwner[kMcTriTable[c][e]], vbase, mask,
                                            [&](int dx, int dy, int dz, int) { return p + dx + dy * sy + dz * sz; });
}

// ---- geometric vertex normals ------------------------------------------------------------------------------------------------
// n_v = normalise(sum over the triangles t that hold v of (p1 - p0) x (p2 - p0)): the cross product's length is twice the triangle's
// area, so the sum is area-weighted.  The cross product is taken in fp32 (differences, then products and one subtraction per
// component, no fma: the file is compiled with -ffp-contract=off), scaled by a power of two that puts the largest component of the
// whole mesh at 2^52 and rounded to an integer: below 2^-52 of the largest triangle a contribution is dropped, everything above is
// exact, and integer sums do not depend on the order the atomics land in.  Triangles with a vertex index outside [0, V) or a
// non-finite cross product contribute nothing.
__device__ __forceinline__ bool tri_cross(const float *v, const int32_t *tris, int64_t t, int64_t V, int32_t id[3], float c[3])
{
    id[0] = tris[3 * t]; id[1] = tris[3 * t + 1]; id[2] = tris[3 * t + 2];
    for (int k = 0; k < 3; ++k)
        if (id[k] < 0 || id[k] >= V) return false;
    const float *p0 = v + 3 * (int64_t)id[0], *p1 = v + 3 * (int64_t)id[1], *p2 = v + 3 * (int64_t)id[2];
    const float a0 = p1[0] - p0[0], a1 = p1[1] - p0[1], a2 = p1[2] - p0[2];
    const float b0 = p2[0] - p0[0], b1 = p2[1] - p0[1], b2 = p2[2] - p0[2];
    c[0] = a1 * b2 - a2 * b1;
    c[1] = a2 * b0 - a0 * b2;
    c[2] = a0 * b1 - a1 * b0;
    const float m = fmaxf(fabsf(c[0]), fmaxf(fabsf(c[1]), fabsf(c[2])));
    return m < INFINITY && c[0] == c[0] && c[1] == c[1] && c[2] == c[2];
}

// largest |component| of any cross product, as the bit pattern of a non-negative float (ordered like the value: an integer max)
__global__ void __launch_bounds__(kMcThreads) mesh_normal_max_kernel(const float *v, int64_t V, const int32_t *tris, int64_t T, unsigned *maxbits)
{
    const int64_t t = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    if (t >= T) return;
    int32_t id[3];
    float c[3];
    if (!tri_cross(v, tris, t, V, id, c)) return;
    const float m = fmaxf(fabsf(c[0]), fmaxf(fabsf(c[1]), fabsf(c[2])));
    atomicMax(maxbits, __float_as_uint(m));
}

// 2^(52 - e) with 2^e <= max < 2^(e+1) (frexp's exponent minus one); max = 0 (or a subnormal scale overflow) is handled by the callers
__device__ __forceinline__ double mesh_normal_scale(unsigned maxbits)
{
    int e;
    (void)frexpf(__uint_as_float(maxbits), &e);
    return ldexp(1.0, 53 - e);
}

__global__ void __launch_bounds__(kMcThreads) mesh_normal_accum_kernel(const float *v, int64_t V, const int32_t *tris, int64_t T,
                                                                       const unsigned *maxbits, unsigned long long *acc)
{
    const int64_t t = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    if (t >= T || *maxbits == 0) return;
    int32_t id[3];
    float c[3];
    if (!tri_cross(v, tris, t, V, id, c)) return;
    const double scale = mesh_normal_scale(*maxbits);
    for (int d = 0; d < 3; ++d) {
        const long long q = (long long)rint((double)c[d] * scale);      // |q| <= 2^53
        if (!q) continue;
        for (int k = 0; k < 3; ++k) atomicAdd(acc + 3 * (int64_t)id[k] + d, (unsigned long long)q);     // two's complement: signed sums
    }
}

__global__ void __launch_bounds__(kMcThreads) mesh_normal_finish_kernel(int64_t V, const unsigned *maxbits, const unsigned long long *acc,
                                                                        float *normals)
{
    const int64_t i = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    if (i >= V) return;
    float out[3] = { 0.f, 0.f, 0.f };
    if (*maxbits) {
        const double inv = 1.0 / mesh_normal_scale(*maxbits);
        const double x = (double)(long long)acc[3 * i] * inv, y = (double)(long long)acc[3 * i + 1] * inv, z = (double)(long long)acc[3 * i + 2] * inv;
        const double len = sqrt(x * x + y * y + z * z);
        if (len >= 1e-20) { out[0] = (float)(x / len); out[1] = (float)(y / len); out[2] = (float)(z / len); }
    }
    normals[3 * i] = out[0]; normals[3 * i + 1] = out[1]; normals[3 * i + 2] = out[2];
}

// acc: [3 V] 64-bit words followed by one 32-bit word (the max), zeroed here
void launch_mesh_normals(const float *vertices, int64_t V, const int32_t *tris, int64_t T, unsigned long long *acc, float *normals, hipStream_t s)
{
    if (V <= 0) return;
    unsigned *maxbits = (unsigned *)(acc + 3 * V);
    (void)hipMemsetAsync(acc, 0, (size_t)(3 * V + 1) * sizeof(unsigned long long), s);
    if (T > 0) {
        const unsigned tb = (unsigned)((T + kMcThreads - 1) / kMcThreads);
        hipLaunchKernelGGL(mesh_normal_max_kernel, dim3(tb), dim3(kMcThreads), 0, s, vertices, V, tris, T, maxbits);
        hipLaunchKernelGGL(mesh_normal_accum_kernel, dim3(tb), dim3(kMcThreads), 0, s, vertices, V, tris, T, maxbits, acc);
    }
    hipLaunchKernelGGL(mesh_normal_finish_kernel, dim3((unsigned)((V + kMcThreads - 1) / kMcThreads)), dim3(kMcThreads), 0, s, V, maxbits, acc, normals);
}

// ---- mesh clean-up: connected components and compaction ---------------------------------------------------------------------
// Components: union-find over the vertices with parent[v] <= v throughout, so that a set's root is its LOWEST vertex index.
//   cc_hook_kernel   per valid triangle: m = the lowest of its three vertices' parents; the other parents (the heads of the higher
//                    trees) and the vertices themselves are put under m with atomicMin -- whatever order the atomics land in, a
//                    parent only ever DEcreases and always names a vertex of the same component
//   cc_jump_kernel   per vertex: parent[v] = parent[parent[parent[v]]] (two pointer jumps)
// Both are loop-free; the host repeats the pair until a round changes nothing (neddf_capi.hip).  A round that changes nothing leaves
// parent[a] == parent[b] == parent[c] on every valid triangle and parent[parent[v]] == parent[v] everywhere: all vertices of a component
// then share ONE parent r with parent[r] == r, r <= each of them and r inside the component -- r is the component's lowest vertex.  That
// fixed point is unique, so the labels do not depend on timing (only the number of rounds may).  While it is not reached a round
// strictly lowers some parent (if no jump can, every parent is a root, and a triangle with two parents hooks the higher root), so the
// iteration ends for every input.  parent[] only ever holds indices in [0, V): no load leaves the array.
// Dense labels: flag the roots (used and parent[v] == v), count / scan / write as marching cubes does, gather through parent[].
// Triangle counts per component: integer atomic adds (exact, so order-independent), one per workgroup for the label its first
// triangle has -- neighbouring triangles of a marching-cubes mesh share their component.
// Compaction: keep flags -> used vertices -> per-block totals -> scans -> writes: no atomics decide a position.
__device__ __forceinline__ bool tri_ids(const int32_t *tris, int64_t t, int64_t V, int32_t id[3])
{
    id[0] = tris[3 * t]; id[1] = tris[3 * t + 1]; id[2] = tris[3 * t + 2];
    return id[0] >= 0 && id[0] < V && id[1] >= 0 && id[1] < V && id[2] >= 0 && id[2] < V;
}

// parent[] is read while other lanes lower it: a relaxed agent-scope load, never a value the compiler kept in a register
__device__ __forceinline__ int32_t cc_load(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ void __launch_bounds__(kMcThreads) cc_init_kernel(int32_t *parent, unsigned char *used, int64_t V)
{
    const int64_t v = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    if (v >= V) return;
    parent[v] = (int32_t)v;
    used[v] = 0;
}

__global__ void __launch_bounds__(kMcThreads) cc_mark_kernel(const int32_t *tris, int64_t T, int64_t V, unsigned char *used)
{
    const int64_t t = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    int32_t id[3];
    if (t >= T || !tri_ids(tris, t, V, id)) return;
    used[id[0]] = 1; used[id[1]] = 1; used[id[2]] = 1;        // every writer stores the same byte
}

__global__ void __launch_bounds__(kMcThreads) cc_hook_kernel(int32_t *parent, const int32_t *tris, int64_t T, int64_t V, int *changed)
{
    const int64_t t = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    int32_t id[3];
    if (t >= T || !tri_ids(tris, t, V, id)) return;
    const int32_t p0 = cc_load(parent + id[0]), p1 = cc_load(parent + id[1]), p2 = cc_load(parent + id[2]);
    const int32_t p[3] = { p0, p1, p2 };
    const int32_t m = min(p0, min(p1, p2));
    if (p0 == m && p1 == m && p2 == m) return;
    *changed = 1;
    for (int k = 0; k < 3; ++k)
        if (p[k] > m) {
            atomicMin(parent + p[k], m);           // the head of the higher tree
            atomicMin(parent + id[k], m);          // and the vertex itself (a shortcut: the jump would get there too)
        }
}

__global__ void __launch_bounds__(kMcThreads) cc_jump_kernel(int32_t *parent, int64_t V, int *changed)
{
    const int64_t v = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    if (v >= V) return;
    const int32_t p = cc_load(parent + v);
    const int32_t g = cc_load(parent + cc_load(parent + p));     // this launch's only writer of parent[v] is this thread
    if (g == p) return;
    __hip_atomic_store(parent + v, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *changed = 1;
}

// a single workgroup: a[0..n) -> exclusive prefix sums in place, a[n] = the total
__global__ void __launch_bounds__(kMcScanThreads) scan_totals_kernel(int64_t *a, int64_t n)
{
    __shared__ int64_t lds[kMcScanThreads];
    int64_t carry = 0;
    for (int64_t base = 0; base < n; base += kMcScanThreads) {
        const int64_t q = base + threadIdx.x;
        const int64_t v = q < n ? a[q] : 0;
        int64_t total;
        const int64_t e = block_exclusive_scan(v, lds, &total);
        if (q < n) a[q] = carry + e;
        carry += total;
    }
    if (threadIdx.x == 0) a[n] = carry;
}

__global__ void __launch_bounds__(kMcThreads) cc_root_count_kernel(const int32_t *parent, const unsigned char *used, int64_t V, int64_t *blk)
{
    const int64_t v = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    const int n = __syncthreads_count(v < V && used[v] && parent[v] == (int32_t)v);
    if (threadIdx.x == 0) blk[blockIdx.x] = n;
}

// roots get their dense label, unused vertices -1; the other vertices are filled in by cc_gather_kernel
__global__ void __launch_bounds__(kMcThreads) cc_root_label_kernel(const int32_t *parent, const unsigned char *used, int64_t V, const int64_t *blk,
                                                                   int32_t *vertex_label)
{
    __shared__ int lds[kMcThreads / 64];
    const int64_t v = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    const bool use = v < V && used[v];
    const bool root = use && parent[v] == (int32_t)v;
    const int off = block_rank(root, lds);
    if (v >= V) return;
    if (!use) vertex_label[v] = -1;
    else if (root) vertex_label[v] = (int32_t)(blk[blockIdx.x] + off);
}

// a non-root reads its root's entry, which the launch before wrote and this one leaves alone; the first C counts are zeroed here
__global__ void __launch_bounds__(kMcThreads) cc_gather_kernel(const int32_t *parent, const unsigned char *used, int64_t V, const int64_t *n_components,
                                                               int32_t *vertex_label, int64_t *component_triangles)
{
    const int64_t v = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    if (v >= V) return;
    if (v < *n_components) component_triangles[v] = 0;
    const int32_t p = parent[v];
    if (used[v] && p != (int32_t)v) vertex_label[v] = vertex_label[p];
}

__global__ void __launch_bounds__(kMcThreads) cc_triangle_kernel(const int32_t *tris, int64_t T, int64_t V, const int32_t *vertex_label,
                                                                 int32_t *triangle_label, unsigned long long *component_triangles)
{
    __shared__ int head;
    const int64_t t = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    int32_t id[3], label = -1;
    if (t < T && tri_ids(tris, t, V, id)) label = vertex_label[id[0]];
    if (t < T && triangle_label) triangle_label[t] = label;
    if (threadIdx.x == 0) head = label;
    __syncthreads();
    const bool same = label >= 0 && label == head;
    const int n = __syncthreads_count(same);
    if (threadIdx.x == 0 && n) atomicAdd(component_triangles + head, (unsigned long long)n);
    if (label >= 0 && !same) atomicAdd(component_triangles + label, 1ULL);
}

__device__ __forceinline__ bool compact_kept(const int32_t *tris, int64_t t, int64_t T, int64_t V, const unsigned char *keep, int32_t id[3])
{
    return t < T && keep[t] && tri_ids(tris, t, V, id);
}

__global__ void __launch_bounds__(kMcThreads) compact_mark_kernel(const int32_t *tris, int64_t T, int64_t V, const unsigned char *keep,
                                                                  unsigned char *used, int64_t *tblk)
{
    const int64_t t = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    int32_t id[3];
    const bool kept = compact_kept(tris, t, T, V, keep, id);
    if (kept) { used[id[0]] = 1; used[id[1]] = 1; used[id[2]] = 1; }
    const int n = __syncthreads_count(kept);
    if (threadIdx.x == 0) tblk[blockIdx.x] = n;
}

__global__ void __launch_bounds__(kMcThreads) compact_vertex_count_kernel(const unsigned char *used, int64_t V, int64_t *vblk)
{
    const int64_t v = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    const int n = __syncthreads_count(v < V && used[v]);
    if (threadIdx.x == 0) vblk[blockIdx.x] = n;
}

__global__ void __launch_bounds__(kMcThreads) compact_vertex_kernel(const unsigned *vertices, int64_t V, const unsigned char *used, const int64_t *vblk,
                                                                    int32_t *vmap, unsigned *out_vertices)
{
    __shared__ int lds[kMcThreads / 64];
    const int64_t v = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    const bool use = v < V && used[v];
    const int off = block_rank(use, lds);
    if (v >= V) return;
    if (!use) { vmap[v] = -1; return; }
    const int64_t o = vblk[blockIdx.x] + off;
    vmap[v] = (int32_t)o;
    out_vertices[3 * o] = vertices[3 * v];                // as 32-bit words: every bit pattern survives, NaN payloads included
    out_vertices[3 * o + 1] = vertices[3 * v + 1];
    out_vertices[3 * o + 2] = vertices[3 * v + 2];
}

__global__ void __launch_bounds__(kMcThreads) compact_triangle_kernel(const int32_t *tris, int64_t T, int64_t V, const unsigned char *keep,
                                                                      const int64_t *tblk, const int32_t *vmap, int32_t *out_tris)
{
    __shared__ int lds[kMcThreads / 64];
    const int64_t t = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    int32_t id[3];
    const bool kept = compact_kept(tris, t, T, V, keep, id);
    const int off = block_rank(kept, lds);
    if (!kept) return;
    const int64_t o = tblk[blockIdx.x] + off;
    out_tris[3 * o] = vmap[id[0]];
    out_tris[3 * o + 1] = vmap[id[1]];
    out_tris[3 * o + 2] = vmap[id[2]];
}

void launch_cc_init(int32_t *parent, unsigned char *used, int64_t V, const int32_t *tris, int64_t T, hipStream_t s)
{
    if (V > 0) hipLaunchKernelGGL(cc_init_kernel, dim3((unsigned)mc_blocks(V)), dim3(kMcThreads), 0, s, parent, used, V);
    if (V > 0 && T > 0) hipLaunchKernelGGL(cc_mark_kernel, dim3((unsigned)mc_blocks(T)), dim3(kMcThreads), 0, s, tris, T, V, used);
}

void launch_cc_round(int32_t *parent, int64_t V, const int32_t *tris, int64_t T, int *changed, hipStream_t s)
{
    if (V <= 0 || T <= 0) return;
    hipLaunchKernelGGL(cc_hook_kernel, dim3((unsigned)mc_blocks(T)), dim3(kMcThreads), 0, s, parent, tris, T, V, changed);
    hipLaunchKernelGGL(cc_jump_kernel, dim3((unsigned)mc_blocks(V)), dim3(kMcThreads), 0, s, parent, V, changed);
}

void launch_scan_totals(int64_t *a, int64_t n, hipStream_t s)
{
    hipLaunchKernelGGL(scan_totals_kernel, dim3(1), dim3(kMcScanThreads), 0, s, a, n);
}

void launch_cc_labels(const int32_t *parent, const unsigned char *used, int64_t V, const int32_t *tris, int64_t T, int64_t *blk,
                      int32_t *vertex_label, int32_t *triangle_label, int64_t *component_triangles, hipStream_t s)
{
    const int64_t nb = mc_blocks(V);
    if (V > 0) hipLaunchKernelGGL(cc_root_count_kernel, dim3((unsigned)nb), dim3(kMcThreads), 0, s, parent, used, V, blk);
    launch_scan_totals(blk, nb, s);
    if (V > 0) {
        hipLaunchKernelGGL(cc_root_label_kernel, dim3((unsigned)nb), dim3(kMcThreads), 0, s, parent, used, V, blk, vertex_label);
        hipLaunchKernelGGL(cc_gather_kernel, dim3((unsigned)nb), dim3(kMcThreads), 0, s, parent, used, V, blk + nb, vertex_label, component_triangles);
    }
    if (T > 0)          // with V == 0 every triangle is invalid: label -1, nothing counted
        hipLaunchKernelGGL(cc_triangle_kernel, dim3((unsigned)mc_blocks(T)), dim3(kMcThreads), 0, s, tris, T, V, vertex_label, triangle_label,
                           (unsigned long long *)component_triangles);
}

void launch_compact_count(const int32_t *tris, int64_t T, int64_t V, const unsigned char *keep, unsigned char *used, int64_t *vblk,
                          int64_t *tblk, hipStream_t s)
{
    const int64_t nbv = mc_blocks(V), nbt = mc_blocks(T);
    if (V > 0) (void)hipMemsetAsync(used, 0, (size_t)V, s);
    if (T > 0) hipLaunchKernelGGL(compact_mark_kernel, dim3((unsigned)nbt), dim3(kMcThreads), 0, s, tris, T, V, keep, used, tblk);
    if (V > 0) hipLaunchKernelGGL(compact_vertex_count_kernel, dim3((unsigned)nbv), dim3(kMcThreads), 0, s, used, V, vblk);
    launch_scan_totals(vblk, nbv, s);
    launch_scan_totals(tblk, nbt, s);
}

void launch_compact_write(const float *vertices, int64_t V, const int32_t *tris, int64_t T, const unsigned char *keep,
                          const unsigned char *used, const int64_t *vblk, const int64_t *tblk, int32_t *vmap, float *out_vertices,
                          int32_t *out_tris, hipStream_t s)
{
    if (V > 0) hipLaunchKernelGGL(compact_vertex_kernel, dim3((unsigned)mc_blocks(V)), dim3(kMcThreads), 0, s, (const unsigned *)vertices, V, used, vblk,
                                  vmap, (unsigned *)out_vertices);
    if (T > 0) hipLaunchKernelGGL(compact_triangle_kernel, dim3((unsigned)mc_blocks(T)), dim3(kMcThreads), 0, s, tris, T, V, keep, tblk, vmap, out_tris);
}

void launch_grid_points(const McGrid &g, int64_t first, int64_t n, float *pos, float *dir, float *var, hipStream_t s)
{
    const unsigned blocks = (unsigned)((n + kMcThreads - 1) / kMcThreads);
    hipLaunchKernelGGL(grid_points_kernel, dim3(blocks), dim3(kMcThreads), 0, s, g, first, n, pos, dir, var);
}

void launch_mc_count(const McGrid &g, unsigned char *mask, int64_t *vblk, int64_t *tblk, hipStream_t s)
{
    hipLaunchKernelGGL(mc_count_kernel, dim3((unsigned)mc_blocks(g.n)), dim3(kMcThreads), 0, s, g, mask, vblk, tblk);
}

void launch_mc_vertices(const McGrid &g, const unsigned char *mask, const int64_t *vblk, int32_t *vbase, float *vertices, hipStream_t s)
{
    hipLaunchKernelGGL(mc_vertex_kernel, dim3((unsigned)mc_blocks(g.n)), dim3(kMcThreads), 0, s, g, mask, vblk, vbase, vertices);
}

void launch_mc_triangles(const McGrid &g, const unsigned char *mask, const int64_t *tblk, const int32_t *vbase, int32_t *tris, hipStream_t s)
{
    hipLaunchKernelGGL(mc_triangle_kernel, dim3((unsigned)mc_blocks(g.n)), dim3(kMcThreads), 0, s, g, mask, tblk, vbase, tris);
}

// ---- brick-wise marching cubes -------------------------------------------------------------------------------------------------
// The fine lattice is cut into bricks of B^3 cells (kernels.h BrickGrid); only the listed ("active") bricks carry values, [M][P] floats.
//   coarse_points_kernel    the brick corners: fine lattice points min(b B, n - 1) per axis
//   brick_flag_kernel       a brick is active when one of its 8 corners is NaN, two of them lie on different sides of iso, or one
//                           is within `band` of it; dilate_axis_kernel grows the set along one axis (three launches: a Chebyshev ball)
//   brick_count / _list     active bricks per workgroup (scan_totals_kernel in between), then slot map and ascending list by
//                           block_rank: the rank of a brick among the active ones is its position in both
//   brick_points / _pad     the lattice points of the listed bricks for the field kernels; NaN over what lies past the fine lattice
//   brick_mc_*              one workgroup per brick, the brick's values in LDS: count (the owned crossed edges of every point, the
//                           brick's totals), vertices, triangles -- dense marching cubes' arithmetic on the same lattice points
// Ownership: a lattice edge with lower point p along axis a lies in the lattice of brick p[a] / B on that axis and, on each other axis
// c, of brick p[c] / B and -- when p[c] is a multiple of B -- of the brick below it.  The edge belongs to the ACTIVE brick of lowest
// index among these (up to four); every brick finds the same owner from the slot map alone, so that an edge on a face or edge shared
// by active bricks gives one vertex, and one next to an inactive brick is still produced.  A triangle corner is the owner's first
// vertex id of the edge's lower point (vbase [M][P]) plus the owned crossed edges of lower axis there (mask [M][P]).
// Order: bricks ascending, points / cells by local index, then x / y / z edge / table order; the keys (fine linear index of the lower
// point * 3 + axis, of the cell's corner 0 * 5 + position) sort it into the dense kernel's order.
__device__ __forceinline__ void brick_coords(const BrickGrid &bg, int32_t id, int b[3])
{
    b[0] = id % bg.nbx; b[1] = (id / bg.nbx) % bg.nby; b[2] = id / (bg.nbx * bg.nby);
}

// last valid local index per axis: B, less in the last brick of an axis the bricks do not divide
__device__ __forceinline__ void brick_extent(const BrickGrid &bg, const int b[3], int e[3])
{
    const int dim[3] = { bg.g.nx, bg.g.ny, bg.g.nz };
    for (int a = 0; a < 3; ++a) e[a] = min(bg.B, dim[a] - 1 - b[a] * bg.B);
}

__global__ void __launch_bounds__(kMcThreads) coarse_points_kernel(BrickGrid bg, int64_t first, int64_t n, float *pos, float *dir, float *var)
{
    const int64_t q = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    if (q >= n) return;
    const int64_t p = first + q;
    const int cx = (int)(p % (bg.nbx + 1)), cy = (int)((p / (bg.nbx + 1)) % (bg.nby + 1)), cz = (int)(p / ((int64_t)(bg.nbx + 1) * (bg.nby + 1)));
    pos[3 * q + 0] = lattice_coord(bg.g.lo[0], bg.g.hi[0], bg.g.nx, min(cx * bg.B, bg.g.nx - 1));
    pos[3 * q + 1] = lattice_coord(bg.g.lo[1], bg.g.hi[1], bg.g.ny, min(cy * bg.B, bg.g.ny - 1));
    pos[3 * q + 2] = lattice_coord(bg.g.lo[2], bg.g.hi[2], bg.g.nz, min(cz * bg.B, bg.g.nz - 1));
    unit_inputs(q, dir, var);
}

// fine indices of point p of the [M][P] brick lattices; false for padding (and for a brick index outside the grid), then clamped
__device__ __forceinline__ bool brick_point(const BrickGrid &bg, const int32_t *ids, int64_t p, int idx[3])
{
    const int32_t id = ids[p / bg.P];
    const int l = (int)(p % bg.P), L = bg.B + 1;
    const int loc[3] = { l % L, (l / L) % L, l / (L * L) };
    const int dim[3] = { bg.g.nx, bg.g.ny, bg.g.nz };
    if (id < 0 || id >= bg.nb) { idx[0] = idx[1] = idx[2] = 0; return false; }
    int b[3];
    brick_coords(bg, id, b);
    bool valid = true;
    for (int a = 0; a < 3; ++a) {
        idx[a] = b[a] * bg.B + loc[a];
        if (idx[a] > dim[a] - 1) { idx[a] = dim[a] - 1; valid = false; }
    }
    return valid;
}

__global__ void __launch_bounds__(kMcThreads) brick_points_kernel(BrickGrid bg, const int32_t *ids, int64_t first, int64_t n, float *pos, float *dir,
                                                                   float *var)
{
    const int64_t q = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    if (q >= n) return;
    int idx[3];
    (void)brick_point(bg, ids, first + q, idx);
    pos[3 * q + 0] = lattice_coord(bg.g.lo[0], bg.g.hi[0], bg.g.nx, idx[0]);
    pos[3 * q + 1] = lattice_coord(bg.g.lo[1], bg.g.hi[1], bg.g.ny, idx[1]);
    pos[3 * q + 2] = lattice_coord(bg.g.lo[2], bg.g.hi[2], bg.g.nz, idx[2]);
    unit_inputs(q, dir, var);
}

__global__ void __launch_bounds__(kMcThreads) brick_pad_kernel(BrickGrid bg, const int32_t *ids, int64_t first, int64_t n, float *out)
{
    const int64_t q = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    if (q >= n) return;
    int idx[3];
    if (!brick_point(bg, ids, first + q, idx)) out[q] = __uint_as_float(0x7fc00000u);
}

__global__ void __launch_bounds__(kMcThreads) brick_flag_kernel(const float *coarse, int nbx, int nby, int nbz, int64_t nb, float iso, float band,
                                                                 unsigned char *flag)
{
    const int64_t c = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    if (c >= nb) return;
    const int x = (int)(c % nbx), y = (int)((c / nbx) % nby), z = (int)(c / ((int64_t)nbx * nby));
    const int64_t sy = nbx + 1, sz = (int64_t)(nbx + 1) * (nby + 1);
    const int64_t p = z * sz + y * sy + x;
    bool any = false;
    int in = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const float v = coarse[p + (b & 1) + ((b >> 1) & 1) * sy + (b >> 2) * sz];
        any |= v != v || fabsf(v - iso) <= band;
        in += inside(v, iso);
    }
    flag[c] = any || (in != 0 && in != 8) ? 1 : 0;
}

// dst = maximum of src over [i - d, i + d] along one axis of an [nz][ny][nx] byte grid of n cells, clipped to the grid (the bricks
// of launch_brick_select, the cells of launch_occ_build)
__global__ void __launch_bounds__(kMcThreads) dilate_axis_kernel(const unsigned char *src, unsigned char *dst, int nx, int ny, int nz, int64_t n_cells,
                                                                  int d, int axis)
{
    const int64_t c = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    if (c >= n_cells) return;
    const int64_t stride = axis == 0 ? 1 : (axis == 1 ? (int64_t)nx : (int64_t)nx * ny);
    const int n = axis == 0 ? nx : (axis == 1 ? ny : nz);
    const int i = (int)((c / stride) % n);
    const int a = i - d < 0 ? 0 : i - d, b = i + d > n - 1 ? n - 1 : i + d;
    unsigned char m = 0;
    for (int j = a; j <= b; ++j) m |= src[c + (int64_t)(j - i) * stride];
    dst[c] = m;
}

__global__ void __launch_bounds__(kMcThreads) brick_count_kernel(const unsigned char *flag, int64_t nb, int64_t *blk)
{
    const int64_t c = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    const int n = __syncthreads_count(c < nb && flag[c]);
    if (threadIdx.x == 0) blk[blockIdx.x] = n;
}

__global__ void __launch_bounds__(kMcThreads) brick_list_kernel(const unsigned char *flag, int64_t nb, const int64_t *blk, int32_t *slot_map,
                                                                 int32_t *ids)
{
    __shared__ int lds[kMcThreads / 64];
    const int64_t c = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    const bool k = c < nb && flag[c];
    const int rank = block_rank(k, lds);
    if (c >= nb) return;
    const int64_t o = blk[blockIdx.x] + rank;
    slot_map[c] = k ? (int32_t)o : -1;
    if (k) ids[o] = (int32_t)c;
}

__global__ void __launch_bounds__(kMcThreads) brick_check_kernel(BrickMesh k, int *bad)
{
    const int64_t t = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    bool wrong = false;
    if (t < k.M) {
        const int32_t id = k.ids[t];
        if (id < 0 || id >= k.bg.nb) wrong = true;
        else wrong = k.slot_map[id] != (int32_t)t || (t > 0 && k.ids[t - 1] >= id);
    }
    if (t < k.bg.nb) {
        const int32_t s = k.slot_map[t];
        if (s != -1 && (s < 0 || s >= k.M || k.ids[s] != (int32_t)t)) wrong = true;
    }
    if (wrong) *bad = 1;            // every writer stores the same word
}

// the brick that owns the edge from local point l of brick b (slot `self`) along `axis`, and the edge's lower point in that brick's lattice
__device__ __forceinline__ int64_t edge_owner(const BrickMesh &k, const int b[3], const int l[3], int axis, int64_t self, int ol[3])
{
    const BrickGrid &bg = k.bg;
    const int c1 = axis == 0 ? 1 : 0, c2 = axis == 2 ? 1 : 2;          // the other two axes, c2 the slower one
    const int nbs[3] = { bg.nbx, bg.nby, bg.nbz };
    // on a face of the brick the edge also lies in the neighbour's lattice (l == B only occurs in a full brick)
    const int lo1 = b[c1] - (l[c1] == 0 && b[c1] > 0), hi1 = b[c1] + (l[c1] == bg.B && b[c1] + 1 < nbs[c1]);
    const int lo2 = b[c2] - (l[c2] == 0 && b[c2] > 0), hi2 = b[c2] + (l[c2] == bg.B && b[c2] + 1 < nbs[c2]);
    ol[0] = l[0]; ol[1] = l[1]; ol[2] = l[2];
    for (int o2 = lo2; o2 <= hi2; ++o2)
        for (int o1 = lo1; o1 <= hi1; ++o1) {         // ascending brick index
            if (o1 == b[c1] && o2 == b[c2]) return self;
            int o[3] = { b[0], b[1], b[2] };
            o[c1] = o1; o[c2] = o2;
            const int32_t s = k.slot_map[((int64_t)o[2] * bg.nby + o[1]) * bg.nbx + o[0]];
            if (s >= 0 && s < k.M) {
                ol[c1] = l[c1] + (b[c1] - o1) * bg.B;
                ol[c2] = l[c2] + (b[c2] - o2) * bg.B;
                return s;
            }
        }
    return self;            // (bricks above this one never own: it is active and lower)
}

// what every brick kernel starts with: the brick's coordinates and extent (false: an index outside the grid, nothing to do), its values in LDS
__device__ __forceinline__ bool brick_stage(const BrickMesh &k, int64_t m, int b[3], int e[3], float *val)
{
    const int32_t id = k.ids[m];
    if (id < 0 || id >= k.bg.nb) return false;
    brick_coords(k.bg, id, b);
    brick_extent(k.bg, b, e);
    for (int l = threadIdx.x; l < k.bg.P; l += kMcThreads) val[l] = k.values[m * k.bg.P + l];
    __syncthreads();
    return true;
}

__global__ void __launch_bounds__(kMcThreads) brick_mc_count_kernel(BrickMesh k, unsigned char *mask, int64_t *vblk, int64_t *tblk)
{
    __shared__ float val[kBrickMaxPoints];
    __shared__ int lds[kMcThreads / 64];
    const int64_t m = blockIdx.x;
    const int L = k.bg.B + 1, P = k.bg.P;
    const float iso = k.bg.g.iso;
    int b[3], e[3], nv = 0, nt = 0;
    const bool ok = brick_stage(k, m, b, e, val);           // uniform over the workgroup
    for (int l = threadIdx.x; l < P; l += kMcThreads) {
        const int loc[3] = { l % L, (l / L) % L, l / (L * L) };
        const int stride[3] = { 1, L, L * L };
        int msk = 0;
        if (ok && loc[0] <= e[0] && loc[1] <= e[1] && loc[2] <= e[2]) {
            const bool in0 = inside(val[l], iso);
            for (int a = 0; a < 3; ++a) {
                int ol[3];
                if (loc[a] < e[a] && inside(val[l + stride[a]], iso) != in0 && edge_owner(k, b, loc, a, m, ol) == m) msk |= 1 << a;
            }
            if (loc[0] < e[0] && loc[1] < e[1] && loc[2] < e[2]) nt += case_triangles(cell_case(val + l, L, L * L, iso));
        }
        mask[m * P + l] = (unsigned char)msk;
        nv += (int)__popc(msk);
    }
    const int tv = block_sum(nv, lds), tt = block_sum(nt, lds);
    if (threadIdx.x == 0) { vblk[m] = tv; tblk[m] = tt; }
}

__global__ void __launch_bounds__(kMcThreads) brick_mc_vertex_kernel(BrickMesh k, const unsigned char *mask, const int64_t *vblk, int32_t *vbase,
                                                                      float *vertices, int64_t *vertex_key)
{
    __shared__ float val[kBrickMaxPoints];
    __shared__ int lds[kMcThreads];
    const int64_t m = blockIdx.x;
    const int L = k.bg.B + 1, P = k.bg.P;
    const McGrid &g = k.bg.g;
    int b[3], e[3];
    if (!brick_stage(k, m, b, e, val)) return;
    int64_t carry = vblk[m];
    for (int base = 0; base < P; base += kMcThreads) {
        const int l = base + threadIdx.x;
        const int msk = l < P ? mask[m * P + l] : 0;
        int total;
        const int off = block_exclusive_scan((int)__popc(msk), lds, &total);
        const int64_t id = carry + off;
        carry += total;
        if (l >= P) continue;
        vbase[m * P + l] = (int32_t)id;
        if (!msk) continue;
        const int loc[3] = { l % L, (l / L) % L, l / (L * L) };
        const int idx[3] = { b[0] * k.bg.B + loc[0], b[1] * k.bg.B + loc[1], b[2] * k.bg.B + loc[2] };
        const int stride[3] = { 1, L, L * L };
        edge_vertices(g, idx, msk, val[l], [&](int a) { return val[l + stride[a]]; }, id, vertices, vertex_key);
    }
}

__global__ void __launch_bounds__(kMcThreads) brick_mc_triangle_kernel(BrickMesh k, const unsigned char *mask, const int64_t *tblk,
                                                                        const int32_t *vbase, int32_t *tris, int64_t *triangle_key)
{
    __shared__ float val[kBrickMaxPoints];
    __shared__ int lds[kMcThreads];
    const int64_t m = blockIdx.x;
    const int L = k.bg.B + 1, P = k.bg.P;
    const McGrid &g = k.bg.g;
    int b[3], e[3];
    if (!brick_stage(k, m, b, e, val)) return;
    int64_t carry = tblk[m];
    for (int base = 0; base < P; base += kMcThreads) {
        const int l = base + threadIdx.x;
        const int loc[3] = { l % L, (l / L) % L, l / (L * L) };
        int c = 0, nt = 0;
        if (l < P && loc[0] < e[0] && loc[1] < e[1] && loc[2] < e[2]) {
            c = cell_case(val + l, L, L * L, g.iso);
            nt = case_triangles(c);
        }
        int total;
        const int off = block_exclusive_scan(nt, lds, &total);
        const int64_t first = carry + off;
        carry += total;
        if (!nt) continue;
        const int64_t p = ((int64_t)(b[2] * k.bg.B + loc[2]) * g.ny + (b[1] * k.bg.B + loc[1])) * g.nx + (b[0] * k.bg.B + loc[0]);
        for (int i = 0; i < 3 * nt; ++i)
            tris[3 * first + i] = corner_vertex(kMcEdgeOwner[kMcTriTable[c][i]], vbase, mask, [&](int dx, int dy, int dz, int axis) {
                const int ql[3] = { loc[0] + dx, loc[1] + dy, loc[2] + dz };
                int ol[3];
                const int64_t s = edge_owner(k, b, ql, axis, m, ol);         // the brick whose lattice holds the vertex
                return s * P + (ol[2] * L + ol[1]) * L + ol[0];
            });
        for (int i = 0; i < nt; ++i) triangle_key[first + i] = 5 * p + i;
    }
}

void launch_coarse_points(const BrickGrid &bg, int64_t first, int64_t n, float *pos, float *dir, float *var, hipStream_t s)
{
    hipLaunchKernelGGL(coarse_points_kernel, dim3((unsigned)mc_blocks(n)), dim3(kMcThreads), 0, s, bg, first, n, pos, dir, var);
}

void launch_brick_points(const BrickGrid &bg, const int32_t *ids, int64_t first, int64_t n, float *pos, float *dir, float *var, hipStream_t s)
{
    hipLaunchKernelGGL(brick_points_kernel, dim3((unsigned)mc_blocks(n)), dim3(kMcThreads), 0, s, bg, ids, first, n, pos, dir, var);
}

void launch_brick_pad(const BrickGrid &bg, const int32_t *ids, int64_t first, int64_t n, float *out, hipStream_t s)
{
    hipLaunchKernelGGL(brick_pad_kernel, dim3((unsigned)mc_blocks(n)), dim3(kMcThreads), 0, s, bg, ids, first, n, out);
}

const unsigned char *launch_dilate(unsigned char *a, unsigned char *b, int nx, int ny, int nz, int d, hipStream_t s)
{
    const int64_t n = (int64_t)nx * ny * nz;
    for (int axis = 0; axis < 3 && d > 0; ++axis) {
        hipLaunchKernelGGL(dilate_axis_kernel, dim3((unsigned)mc_blocks(n)), dim3(kMcThreads), 0, s, (const unsigned char *)a, b, nx, ny, nz, n, d, axis);
        unsigned char *t = a; a = b; b = t;
    }
    return a;
}

void launch_brick_select(const float *coarse, int nbx, int nby, int nbz, float iso, float band, int dilate, unsigned char *flag_a,
                         unsigned char *flag_b, int64_t *blk, int32_t *slot_map, int32_t *ids, hipStream_t s)
{
    const int64_t nb = (int64_t)nbx * nby * nbz, blocks = mc_blocks(nb);
    hipLaunchKernelGGL(brick_flag_kernel, dim3((unsigned)blocks), dim3(kMcThreads), 0, s, coarse, nbx, nby, nbz, nb, iso, band, flag_a);
    const unsigned char *src = launch_dilate(flag_a, flag_b, nbx, nby, nbz, dilate, s);
    hipLaunchKernelGGL(brick_count_kernel, dim3((unsigned)blocks), dim3(kMcThreads), 0, s, src, nb, blk);
    launch_scan_totals(blk, blocks, s);
    hipLaunchKernelGGL(brick_list_kernel, dim3((unsigned)blocks), dim3(kMcThreads), 0, s, src, nb, blk, slot_map, ids);
}

void launch_brick_check(const BrickMesh &k, int *bad, hipStream_t s)
{
    const int64_t n = k.M > k.bg.nb ? k.M : k.bg.nb;
    hipLaunchKernelGGL(brick_check_kernel, dim3((unsigned)mc_blocks(n)), dim3(kMcThreads), 0, s, k, bad);
}

void launch_brick_mc_count(const BrickMesh &k, unsigned char *mask, int64_t *vblk, int64_t *tblk, hipStream_t s)
{
    hipLaunchKernelGGL(brick_mc_count_kernel, dim3((unsigned)k.M), dim3(kMcThreads), 0, s, k, mask, vblk, tblk);
}

void launch_brick_mc_vertices(const BrickMesh &k, const unsigned char *mask, const int64_t *vblk, int32_t *vbase, float *vertices,
                              int64_t *vertex_key, hipStream_t s)
{
    hipLaunchKernelGGL(brick_mc_vertex_kernel, dim3((unsigned)k.M), dim3(kMcThreads), 0, s, k, mask, vblk, vbase, vertices, vertex_key);
}

void launch_brick_mc_triangles(const BrickMesh &k, const unsigned char *mask, const int64_t *tblk, const int32_t *vbase, int32_t *tris,
                               int64_t *triangle_key, hipStream_t s)
{
    hipLaunchKernelGGL(brick_mc_triangle_kernel, dim3((unsigned)k.M), dim3(kMcThreads), 0, s, k, mask, tblk, vbase, tris, triangle_key);
}

}  // namespace neddf
