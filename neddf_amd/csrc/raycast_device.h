// raycast_device.h -- the per-pair arithmetic of the ray casts (raycast_kernels.hip states it), shared by every kernel that tests rays
// against triangles: the brute and grid queries (raycast_kernels.hip) and the BVH traversal (bvh_kernels.hip).  One definition, one set
// of bits.
#pragma once
#include "kernels.h"

namespace neddf {

struct RcRay {
    float ox, oy, oz, dx, dy, dz;
    float Sx, Sy, Sz;
    int kx, ky, kz;
};

struct RcHit {
    float t;
    int32_t j;
    float b1, b2;
};

__device__ __forceinline__ float rc_sel(float x, float y, float z, int k) { return k == 0 ? x : (k == 1 ? y : z); }

__device__ __forceinline__ bool rc_finite3(float x, float y, float z) { return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z); }

// the per-ray constants; false for a non-finite component or an all-zero direction (the ray is then filled with a harmless stand-in)
__device__ __forceinline__ bool rc_ray_setup(float ox, float oy, float oz, float dx, float dy, float dz, RcRay *r)
{
    const bool ok = rc_finite3(ox, oy, oz) && rc_finite3(dx, dy, dz) && (dx != 0.f || dy != 0.f || dz != 0.f);
    if (!ok) { ox = oy = oz = 0.f; dx = dy = 0.f; dz = 1.f; }
    r->ox = ox; r->oy = oy; r->oz = oz; r->dx = dx; r->dy = dy; r->dz = dz;
    const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
    int kz = 0;
    float m = ax;
    if (ay > m) { kz = 1; m = ay; }
    if (az > m) kz = 2;
    int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
    const float dk = rc_sel(dx, dy, dz, kz);
    if (dk < 0.f) { const int s = kx; kx = ky; ky = s; }
    r->kx = kx; r->ky = ky; r->kz = kz;
    r->Sz = __fdiv_rn(1.f, dk);
    r->Sx = __fmul_rn(rc_sel(dx, dy, dz, kx), r->Sz);
    r->Sy = __fmul_rn(rc_sel(dx, dy, dz, ky), r->Sz);
    return ok;
}

// an edge function that came out exactly 0, again: both products (exact in double) and their difference in fp64, rounded to fp32
__device__ __forceinline__ float rc_edge64(float a, float b, float c, float d)
{
    return (float)__dsub_rn(__dmul_rn((double)a, (double)b), __dmul_rn((double)c, (double)d));
}

// one finite triangle (p0, p1, p2) with index j against one ray
__device__ __forceinline__ void rc_visit(const RcRay &r, float t_min, float t_max, float pad, float p0x, float p0y, float p0z, float p1x, float p1y,
                                         float p1z, float p2x, float p2y, float p2z, int32_t j, RcHit *best)
{
    const float a0 = __fsub_rn(p0x, r.ox), a1 = __fsub_rn(p0y, r.oy), a2 = __fsub_rn(p0z, r.oz);
    const float b0 = __fsub_rn(p1x, r.ox), b1 = __fsub_rn(p1y, r.oy), b2 = __fsub_rn(p1z, r.oz);
    const float c0 = __fsub_rn(p2x, r.ox), c1 = __fsub_rn(p2y, r.oy), c2 = __fsub_rn(p2z, r.oz);
    const float Akz = rc_sel(a0, a1, a2, r.kz), Bkz = rc_sel(b0, b1, b2, r.kz), Ckz = rc_sel(c0, c1, c2, r.kz);
    const float Ax = __fsub_rn(rc_sel(a0, a1, a2, r.kx), __fmul_rn(r.Sx, Akz)), Ay = __fsub_rn(rc_sel(a0, a1, a2, r.ky), __fmul_rn(r.Sy, Akz));
    const float Bx = __fsub_rn(rc_sel(b0, b1, b2, r.kx), __fmul_rn(r.Sx, Bkz)), By = __fsub_rn(rc_sel(b0, b1, b2, r.ky), __fmul_rn(r.Sy, Bkz));
    const float Cx = __fsub_rn(rc_sel(c0, c1, c2, r.kx), __fmul_rn(r.Sx, Ckz)), Cy = __fsub_rn(rc_sel(c0, c1, c2, r.ky), __fmul_rn(r.Sy, Ckz));
    float U = __fsub_rn(__fmul_rn(Cx, By), __fmul_rn(Cy, Bx));
    float V = __fsub_rn(__fmul_rn(Ax, Cy), __fmul_rn(Ay, Cx));
    float W = __fsub_rn(__fmul_rn(Bx, Ay), __fmul_rn(By, Ax));
    if (U == 0.f || V == 0.f || W == 0.f) {
        U = rc_edge64(Cx, By, Cy, Bx);
        V = rc_edge64(Ax, Cy, Ay, Cx);
        W = rc_edge64(Bx, Ay, By, Ax);
    }
    if (!((U >= 0.f && V >= 0.f && W >= 0.f) || (U <= 0.f && V <= 0.f && W <= 0.f))) return;         // two-sided; a NaN fails both
    const float det = __fadd_rn(__fadd_rn(U, V), W);
    if (det == 0.f) return;
    const float Az = __fmul_rn(r.Sz, Akz), Bz = __fmul_rn(r.Sz, Bkz), Cz = __fmul_rn(r.Sz, Ckz);
    const float t = __fdiv_rn(__fadd_rn(__fadd_rn(__fmul_rn(U, Az), __fmul_rn(V, Bz)), __fmul_rn(W, Cz)), det);
    if (!(t >= t_min && t <= t_max)) return;
    // the rounded hit point inside the triangle's box widened by pad: discards the garbage t of a nearly degenerate triangle, and is
    // what ties a candidate to the cells it is listed in
    const float px = __fadd_rn(r.ox, __fmul_rn(t, r.dx)), py = __fadd_rn(r.oy, __fmul_rn(t, r.dy)), pz = __fadd_rn(r.oz, __fmul_rn(t, r.dz));
    if (!(px >= __fsub_rn(fminf(fminf(p0x, p1x), p2x), pad) && px <= __fadd_rn(fmaxf(fmaxf(p0x, p1x), p2x), pad))) return;
    if (!(py >= __fsub_rn(fminf(fminf(p0y, p1y), p2y), pad) && py <= __fadd_rn(fmaxf(fmaxf(p0y, p1y), p2y), pad))) return;
    if (!(pz >= __fsub_rn(fminf(fminf(p0z, p1z), p2z), pad) && pz <= __fadd_rn(fmaxf(fmaxf(p0z, p1z), p2z), pad))) return;
    if (t < best->t || (t == best->t && (uint32_t)j < (uint32_t)best->j)) {
        best->t = t;
        best->j = j;
        best->b1 = __fdiv_rn(V, det);
        best->b2 = __fdiv_rn(W, det);
    }
}

// the corners of triangle j (nine floats, vertex-major); false for an index outside [0, V) or a non-finite vertex
__device__ __forceinline__ bool rc_triangle(const float *v, int64_t V, const int32_t *tri, int64_t j, float *p)
{
    const int64_t i0 = tri[3 * j], i1 = tri[3 * j + 1], i2 = tri[3 * j + 2];
    if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) return false;
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        p[a] = v[3 * i0 + a]; p[3 + a] = v[3 * i1 + a]; p[6 + a] = v[3 * i2 + a];
        ok = ok && __builtin_isfinite(p[a]) && __builtin_isfinite(p[3 + a]) && __builtin_isfinite(p[6 + a]);
    }
    return ok;
}

__device__ __forceinline__ void rc_store(bool ok, const RcHit &best, int64_t i, float *out_t, int32_t *out_j, float *out_b1, float *out_b2)
{
    const float nan = __builtin_nanf("");
    out_t[i] = ok ? best.t : nan;
    out_j[i] = ok ? best.j : -1;
    out_b1[i] = ok ? best.b1 : nan;
    out_b2[i] = ok ? best.b2 : nan;
}

}  // namespace neddf
