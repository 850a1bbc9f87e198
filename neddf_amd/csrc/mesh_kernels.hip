// mesh_kernels.hip -- surface extraction (no reference kernel: the reference meshes on the host with PyMCubes,
// neddf/scripts/fields_visualizer.py:528-566).
//
//   grid_points_kernel   the lattice of neddf_field_grid: np.linspace coordinates per axis, x fastest
//   mc_count_kernel      per lattice point: which of the three edges it owns are crossed (one byte); per block: vertex and
//                        triangle totals
//   mc_scan_kernel       one workgroup: exclusive scans of the block totals (in place, the grand totals behind them)
//   mc_vertex_kernel     per point: its first vertex id (block scan + block base), the vertices of its crossed edges
//   mc_triangle_kernel   per cell: its first triangle id (block scan + block base), the triangles of its case
//   mesh_normal_*        geometric vertex normals of an indexed mesh: area-weighted sums of the incident triangles' cross products,
//                        accumulated in 64-bit fixed point with INTEGER atomics (exact, hence order-independent), then normalised
//
// Placement is decided by count -> scan -> write launches only: no atomics, no exchange between workgroups inside a launch,
// so the output is the same on every run (tests/mesh_check.py restates it in numpy bit for bit).  A corner is inside when
// value < iso; NaN compares false and is outside.  A vertex on an edge with a NaN end (t = NaN) sits at the edge's middle.
#include "kernels.h"
#include "mc_tables.h"

namespace neddf {

// np.linspace(lo, hi, n)[i] rounded to float: lo + i * ((hi - lo) / (n - 1)) in double, the last one exactly hi
__device__ __forceinline__ float lattice_coord(double lo, double hi, int n, int i)
{
    if (i == n - 1) return (float)hi;
    const double step = (hi - lo) / (double)(n - 1);
    return (float)(lo + (double)i * step);
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
    dir[3 * q + 0] = 1.f; dir[3 * q + 1] = 0.f; dir[3 * q + 2] = 0.f;          // base_neuralfield.py:49-79: dir (1, 0, 0), var 0
    var[3 * q + 0] = 0.f; var[3 * q + 1] = 0.f; var[3 * q + 2] = 0.f;
}

// exclusive scan of one value per thread over the workgroup; *total = the sum of all
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

// case index of the cell whose corner 0 is lattice point p (Bourke's corner numbering, mc_tables.h)
__device__ __forceinline__ int cell_case(const McGrid &g, int64_t p)
{
    const int64_t sx = 1, sy = g.nx, sz = (int64_t)g.nx * g.ny;
    const int64_t off[8] = { 0, sx, sx + sy, sy, sz, sx + sz, sx + sy + sz, sy + sz };
    int c = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) c |= inside(g.vol[p + off[b]], g.iso) << b;
    return c;
}

__device__ __forceinline__ int case_triangles(int c)
{
    int n = 0;
    while (n < kMcMaxTris && kMcTriTable[c][3 * n] >= 0) ++n;
    return n;
}

__global__ void __launch_bounds__(kMcThreads) mc_count_kernel(McGrid g, unsigned char *mask, int64_t *vblk, int64_t *tblk)
{
    __shared__ int lds[kMcThreads];
    const int64_t p = (int64_t)blockIdx.x * kMcThreads + threadIdx.x;
    int nv = 0, nt = 0;
    if (p < g.n) {
        const int i = (int)(p % g.nx), j = (int)((p / g.nx) % g.ny), k = (int)(p / ((int64_t)g.nx * g.ny));
        const int m = point_mask(g, p, i, j, k);
        mask[p] = (unsigned char)m;
        nv = (int)__popc(m);
        if (i + 1 < g.nx && j + 1 < g.ny && k + 1 < g.nz) nt = case_triangles(cell_case(g, p));
    }
    int tv, tt;
    (void)block_exclusive_scan(nv, lds, &tv);
    (void)block_exclusive_scan(nt, lds, &tt);
    if (threadIdx.x == 0) { vblk[blockIdx.x] = tv; tblk[blockIdx.x] = tt; }
}

// a single workgroup: a[0..n) -> exclusive prefix sums in place, a[n] = the total (for both arrays)
__global__ void __launch_bounds__(kMcScanThreads) mc_scan_kernel(int64_t *va, int64_t *ta, int64_t n)
{
    __shared__ int64_t lds[kMcScanThreads];
    int64_t vcarry = 0, tcarry = 0;
    for (int64_t base = 0; base < n; base += kMcScanThreads) {
        const int64_t q = base + threadIdx.x;
        const int64_t v = q < n ? va[q] : 0, t = q < n ? ta[q] : 0;
        int64_t vt, tt;
        const int64_t ve = block_exclusive_scan(v, lds, &vt);
        const int64_t te = block_exclusive_scan(t, lds, &tt);
        if (q < n) { va[q] = vcarry + ve; ta[q] = tcarry + te; }
        vcarry += vt; tcarry += tt;
    }
    if (threadIdx.x == 0) { va[n] = vcarry; ta[n] = tcarry; }
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
    int64_t id = vblk[blockIdx.x] + off;
    vbase[p] = (int32_t)id;
    if (!m) return;
    const int i = (int)(p % g.nx), j = (int)((p / g.nx) % g.ny), k = (int)(p / ((int64_t)g.nx * g.ny));
    const float c[3] = { lattice_coord(g.lo[0], g.hi[0], g.nx, i), lattice_coord(g.lo[1], g.hi[1], g.ny, j),
                         lattice_coord(g.lo[2], g.hi[2], g.nz, k) };
    const int idx[3] = { i, j, k }, dim[3] = { g.nx, g.ny, g.nz };
    const int64_t stride[3] = { 1, g.nx, (int64_t)g.nx * g.ny };
    const float v0 = g.vol[p];
    for (int a = 0; a < 3; ++a) {
        if (!(m >> a & 1)) continue;
        const float v1 = g.vol[p + stride[a]];
        float t = (g.iso - v0) / (v1 - v0);
        if (t != t) t = 0.5f;
        const float g0 = c[a], g1 = lattice_coord(g.lo[a], g.hi[a], dim[a], idx[a] + 1);
        float out[3] = { c[0], c[1], c[2] };
        out[a] = g0 + t * (g1 - g0);
        vertices[3 * id + 0] = out[0];
        vertices[3 * id + 1] = out[1];
        vertices[3 * id + 2] = out[2];
        ++id;
    }
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
            c = cell_case(g, p);
            nt = case_triangles(c);
        }
    }
    int total;
    const int off = block_exclusive_scan(nt, lds, &total);
    if (!nt) return;
    const int64_t first = tblk[blockIdx.x] + off;
    const int64_t sy = g.nx, sz = (int64_t)g.nx * g.ny;
    for (int e = 0; e < 3 * nt; ++e) {
        const int own = kMcEdgeOwner[kMcTriTable[c][e]];
        const int64_t q = p + (own & 1) + ((own >> 1) & 1) * sy + ((own >> 2) & 1) * sz;
        const int axis = own >> 3;
        tris[3 * first + e] = vbase[q] + (int32_t)__popc(mask[q] & ((1 << axis) - 1));
    }
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

void launch_grid_points(const McGrid &g, int64_t first, int64_t n, float *pos, float *dir, float *var, hipStream_t s)
{
    const unsigned blocks = (unsigned)((n + kMcThreads - 1) / kMcThreads);
    hipLaunchKernelGGL(grid_points_kernel, dim3(blocks), dim3(kMcThreads), 0, s, g, first, n, pos, dir, var);
}

void launch_mc_count(const McGrid &g, unsigned char *mask, int64_t *vblk, int64_t *tblk, hipStream_t s)
{
    hipLaunchKernelGGL(mc_count_kernel, dim3((unsigned)mc_blocks(g.n)), dim3(kMcThreads), 0, s, g, mask, vblk, tblk);
}

void launch_mc_scan(int64_t *vblk, int64_t *tblk, int64_t nblocks, hipStream_t s)
{
    hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(kMcScanThreads), 0, s, vblk, tblk, nblocks);
}

void launch_mc_vertices(const McGrid &g, const unsigned char *mask, const int64_t *vblk, int32_t *vbase, float *vertices, hipStream_t s)
{
    hipLaunchKernelGGL(mc_vertex_kernel, dim3((unsigned)mc_blocks(g.n)), dim3(kMcThreads), 0, s, g, mask, vblk, vbase, vertices);
}

void launch_mc_triangles(const McGrid &g, const unsigned char *mask, const int64_t *tblk, const int32_t *vbase, int32_t *tris, hipStream_t s)
{
    hipLaunchKernelGGL(mc_triangle_kernel, dim3((unsigned)mc_blocks(g.n)), dim3(kMcThreads), 0, s, g, mask, tblk, vbase, tris);
}

}  // namespace neddf
