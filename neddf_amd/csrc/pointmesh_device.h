// pointmesh_device.h -- the per-pair arithmetic of the point-to-mesh distance (pointmesh_kernels.hip states it), shared by every kernel that
// visits triangles: the brute and grid queries (pointmesh_kernels.hip) and the BVH query (bvh_kernels.hip).  One definition, one set of bits.
#pragma once
#include "kernels.h"

namespace neddf {

constexpr int kPmThreads = 256;          // queries per workgroup and triangles per LDS tile
constexpr int kPmVec = 5;                // float4 per triangle
static_assert(kPmTableFloats == 4 * kPmVec, "the table the C ABI sizes (kernels.h) is the one these kernels index");

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

}  // namespace neddf
