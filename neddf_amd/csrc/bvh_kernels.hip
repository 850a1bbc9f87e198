// bvh_kernels.hip -- a linear BVH (Karras 2012) over the triangles of an indexed mesh, built and traversed on the GPU, and the
// point-to-mesh query through it: the brute kernel's bits for a query anywhere, near the surface or far from it (no reference
// counterpart).  include/neddf_hip.h states the arrays and the equality argument; tests/bvh_check.py restates every kernel in numpy.
//
//   bvh_keys_kernel       one lane per triangle: the 30-bit Morton code of the centre of its box, and its index, as one int64 key
//   (torch.sort of the keys between the two entry points: plumbing, as mesh.py sorts its keys)
//   bvh_topology_kernel   one lane per internal node: Karras' construction over the sorted keys -- integers only
//   bvh_fit_kernel        one lane per leaf: its box, then upwards; the second arriver at a node combines both children
//   pm_bvh_kernel         one lane per query: depth-first, the nearer child first, a box skipped by the pruning rule below
//   rc_bvh_kernel         one lane per ray: the same walk with the ray's slab test; first hit, or (any-hit) the first candidate
//
// INVALID TRIANGLES (an index outside [0, V) or a non-finite vertex: pm_constants' rule) stay in the tree, so that it always has T
// leaves and its sizes can be checked against the mesh: their key has bit 62 set and sorts behind every valid one, their box is EMPTY
// (lo = +inf, hi = -inf: the neutral element of min / max), and an empty box (lo.x > hi.x) is never entered.  A subtree of invalid
// triangles is therefore skipped at its root, and none is ever evaluated.
//
// KEYS.  centre = (min3 + max3) * 0.5 per axis (one rounded sum; the halving is exact), cell = grid_axis_cell(centre) with 1024 cells
// per axis over the caller's box (bvh.py: the bounds of the valid triangles' vertices; any box gives a correct tree, the cell function
// clamps), code = the bits of (cx, cy, cz) interleaved with x lowest, key = code << 32 | index.  Bits 0-30 hold the index, bit 31 is 0,
// bits 32-61 the code, bit 62 the invalid flag: 62 bits can differ, keys are distinct, the depth of the tree is at most 62.
//
// TOPOLOGY.  delta(i, j) = clz64(key_i ^ key_j), -1 for j outside [0, T).  Node i covers the leaves between i and its other end j;
// children int32 [T - 1][2]: c >= 0 is internal node c, c < 0 is leaf ~c; node 0 is the root; T == 1 has no internal node and the root
// is leaf 0.  parent int32 [2 T - 1] (workspace): internal nodes first, then the leaves.
//
// BOXES float [2 T - 1][6] = (lo.xyz, hi.xyz): internal node i at row i, leaf k at row T - 1 + k, so row 0 is always the root.  Exact
// fp32 min / max of vertex coordinates: associative and commutative, the result does not depend on which lane arrives when.  Each lane
// writes its box, __threadfence(), bumps the node's counter; the first arriver stops, the second fences again, reads the sibling's box
// (agent-scope loads) and goes on with the union in registers.  No lane waits for another: no spin, no loop whose exit depends on
// another workgroup.  The climb is bounded by 64 steps whatever `parent` holds.
//
// THE QUERY.  A box (node or leaf) against query p, every operation one rounded fp32 operation:
//     gap_a = max(max(lo_a - p_a, p_a - hi_a), 0);  lb2 = pm_dot(gap, gap);  lb = sqrt(lb2);  m = f * lb - s;  m2 = m * m
//     f = 1 - 2^-16,  s = 2^-18 * W,  W = the largest |coordinate| of the root box
//     SKIPPED when it is empty, or when m > 0 and m2 > best.d2 strictly and 1e-30 <= m2 < +inf (a NaN compares false: visited)
// The header's equality argument shows that a skipped triangle's computed D2 exceeds best.d2 strictly.  Order: the child with the
// smaller m2 (m <= 0 counts as 0) is followed first, the left one on a tie; the other is pushed and tested AGAIN when it is popped,
// against the best of that moment.  (Equivalent to "push both, pop, test": the near child would be popped at once, with an unchanged
// best.)  Every child index is validated before it is followed, every leaf's triangle index before it is gathered, and the loop handles
// at most 2 T nodes (a tree has 2 T - 1): a corrupt tree gives a wrong answer, never a hang or an access outside the arrays.
//
// THE STACK holds at most depth + 1 <= 63 entries.  It lives in LDS as [level][lane] -- the lanes of a wave read one row, 64 distinct
// banks -- 64 levels x 64 lanes x 4 B = 16 KB per one-wave workgroup, ten workgroups per CU.  No dynamically indexed private array: the
// kernel's private segment size in the gfx950 code object's metadata is 0 bytes (.private_segment_fixed_size: 0, no scratch).
//
// RAYS (rc_bvh_kernel<any-hit>) walk the same arrays in the same shape -- one lane per ray, one wave per workgroup, the same LDS stack, the
// same validation and the same 2 T bound -- with another pruning rule: an fp64 slab test of the ray against the box widened by 2 pad
// (rb_skip; include/neddf_hip.h, neddf_raycast_bvh_query, states it and why the result has neddf_raycast_brute's bits).  The per-pair
// arithmetic is raycast_device.h's, the one the brute and grid kernels use.  A ray for which the argument does not hold (a pad that is
// small against the root box, an origin that is far away against pad) visits every triangle in index order instead.
#include "kernels.h"
#include "pointmesh_device.h"
#include "raycast_device.h"

namespace neddf {

constexpr int kBvhThreads = 64;          // queries per workgroup: one wave
constexpr int kBvhStack = 64;            // levels of the traversal stack (depth + 1 <= 63)

__device__ __forceinline__ uint32_t bvh_spread(uint32_t x)          // 10 bits -> every third bit
{
    x &= 0x3ffu;
    x = (x | (x << 16)) & 0x030000ffu;
    x = (x | (x << 8)) & 0x0300f00fu;
    x = (x | (x << 4)) & 0x030c30c3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

// the corners of triangle j into p[9]; false for an index outside [0, V) or a non-finite vertex (pm_constants' rule)
__device__ __forceinline__ bool bvh_corners(const float *v, int64_t V, const int32_t *tri, int64_t j, float *p)
{
    const int64_t i0 = tri[3 * j], i1 = tri[3 * j + 1], i2 = tri[3 * j + 2];
    bool ok = !(i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V);
    if (ok) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            p[a] = v[3 * i0 + a]; p[3 + a] = v[3 * i1 + a]; p[6 + a] = v[3 * i2 + a];
            ok = ok && __builtin_isfinite(p[a]) && __builtin_isfinite(p[3 + a]) && __builtin_isfinite(p[6 + a]);
        }
    }
    return ok;
}

__global__ void __launch_bounds__(kPmThreads) bvh_keys_kernel(NnGrid g, const float *v, int64_t V, const int32_t *tri, int64_t T, int64_t *keys)
{
    const int64_t j = (int64_t)blockIdx.x * kPmThreads + threadIdx.x;
    if (j >= T) return;
    float p[9];
    if (!bvh_corners(v, V, tri, j, p)) {
        keys[j] = ((int64_t)1 << 62) | j;
        return;
    }
    uint32_t code = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float lo = fminf(fminf(p[a], p[3 + a]), p[6 + a]), hi = fmaxf(fmaxf(p[a], p[3 + a]), p[6 + a]);
        const float c = __fmul_rn(__fadd_rn(lo, hi), 0.5f);
        code |= bvh_spread((uint32_t)grid_axis_cell(c, g.lo[a], g.inv_cell[a], g.n[a])) << a;
    }
    keys[j] = ((int64_t)code << 32) | j;
}

// the common-prefix length of keys i and j; -1 for j outside the range (equal keys -- the sort's input never holds any -- give 64)
__device__ __forceinline__ int bvh_delta(const int64_t *keys, int64_t T, int64_t i, int64_t j)
{
    if (j < 0 || j >= T) return -1;
    const uint64_t x = (uint64_t)(keys[i] ^ keys[j]);
    return x ? __builtin_clzll(x) : 64;
}

__global__ void __launch_bounds__(kPmThreads) bvh_topology_kernel(const int64_t *keys, int64_t T, int32_t *leaf_tri, int32_t *children, int32_t *parent,
                                                                  int32_t *counter)
{
    const int64_t i = (int64_t)blockIdx.x * kPmThreads + threadIdx.x;
    if (i >= T) return;
    leaf_tri[i] = (int32_t)(keys[i] & 0x7fffffff);
    if (i == 0) parent[0] = -1;                           // the root: node 0, or leaf 0 of a one-triangle mesh (row T - 1 + 0 = 0)
    if (i >= T - 1) return;
    counter[i] = 0;
    const int64_t d = bvh_delta(keys, T, i, i + 1) - bvh_delta(keys, T, i, i - 1) >= 0 ? 1 : -1;
    const int dmin = bvh_delta(keys, T, i, i - d);
    int64_t lmax = 2;
    while (lmax < 2 * T && bvh_delta(keys, T, i, i + lmax * d) > dmin) lmax *= 2;
    int64_t l = 0;
    for (int64_t t = lmax / 2; t >= 1; t /= 2)
        if (bvh_delta(keys, T, i, i + (l + t) * d) > dmin) l += t;
    const int64_t j = i + l * d;
    const int dnode = bvh_delta(keys, T, i, j);
    int64_t s = 0, t = l;
    do {
        t = (t + 1) >> 1;
        if (bvh_delta(keys, T, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int64_t gamma = i + s * d + (d < 0 ? -1 : 0);
    const int64_t first = i < j ? i : j, last = i < j ? j : i;
    const int32_t left = first == gamma ? ~(int32_t)gamma : (int32_t)gamma;
    const int32_t right = last == gamma + 1 ? ~(int32_t)(gamma + 1) : (int32_t)(gamma + 1);
    children[2 * i] = left;
    children[2 * i + 1] = right;
    parent[first == gamma ? T - 1 + gamma : gamma] = (int32_t)i;
    parent[last == gamma + 1 ? T - 1 + gamma + 1 : gamma + 1] = (int32_t)i;
}

__global__ void __launch_bounds__(kPmThreads) bvh_fit_kernel(const float *v, int64_t V, const int32_t *tri, int64_t T, const int32_t *leaf_tri,
                                                             const int32_t *children, const int32_t *parent, int32_t *counter, float *boxes)
{
    const int64_t k = (int64_t)blockIdx.x * kPmThreads + threadIdx.x;
    if (k >= T) return;
    const float inf = __builtin_inff();
    float b[6] = { inf, inf, inf, -inf, -inf, -inf };
    const int64_t j = leaf_tri[k];
    float p[9];
    if (j >= 0 && j < T && bvh_corners(v, V, tri, j, p)) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            b[a] = fminf(fminf(p[a], p[3 + a]), p[6 + a]);
            b[3 + a] = fmaxf(fmaxf(p[a], p[3 + a]), p[6 + a]);
        }
    }
    int64_t row = T - 1 + k;
    int32_t me = ~(int32_t)k;
    for (int up = 0; up < 64; ++up) {
#pragma unroll
        for (int a = 0; a < 6; ++a) boxes[6 * row + a] = b[a];
        const int64_t node = parent[row];
        if (node < 0 || node >= T - 1) return;                      // the root is done (or `parent` is not a tree's)
        __threadfence();                                            // the box is visible before the counter says so
        if (atomicAdd(&counter[node], 1) == 0) return;              // the first arriver stops; nobody waits
        __threadfence();
        const int32_t c0 = children[2 * node], c1 = children[2 * node + 1];
        const int32_t sib = c0 == me ? c1 : c0;
        const int64_t srow = sib >= 0 ? (int64_t)sib : T - 1 + (int64_t)~sib;
        if (srow < 0 || srow >= 2 * T - 1) return;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            b[a] = fminf(b[a], __hip_atomic_load(&boxes[6 * srow + a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            b[3 + a] = fmaxf(b[3 + a], __hip_atomic_load(&boxes[6 * srow + 3 + a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        }
        row = node;
        me = (int32_t)node;
    }
}

// the pruning rule: true when box `row` need not be entered; *key = m2 (0 for m <= 0), what orders two children
__device__ __forceinline__ bool bvh_skip(const float *boxes, int64_t row, float px, float py, float pz, float s, float best_d2, float *key)
{
    const float *b = boxes + 6 * row;
    const float lx = b[0], ly = b[1], lz = b[2], hx = b[3], hy = b[4], hz = b[5];
    const float gx = fmaxf(fmaxf(__fsub_rn(lx, px), __fsub_rn(px, hx)), 0.f);
    const float gy = fmaxf(fmaxf(__fsub_rn(ly, py), __fsub_rn(py, hy)), 0.f);
    const float gz = fmaxf(fmaxf(__fsub_rn(lz, pz), __fsub_rn(pz, hz)), 0.f);
    const float lb = __fsqrt_rn(pm_dot(gx, gy, gz, gx, gy, gz));
    const float m = __fsub_rn(__fmul_rn(0.9999847412109375f, lb), s);           // f = 1 - 2^-16
    const float m2 = __fmul_rn(m, m);
    const bool pos = m > 0.f;
    *key = pos ? m2 : 0.f;
    return lx > hx || (pos && m2 > best_d2 && m2 >= 1e-30f && m2 < __builtin_inff());
}

// child c of an internal node: its row of `boxes`, or -1 for an index no build can have written
__device__ __forceinline__ int64_t bvh_row(int32_t c, int64_t T)
{
    if (c >= 0) return c < T - 1 ? (int64_t)c : -1;
    const int64_t k = (int64_t)~c;
    return k < T ? T - 1 + k : -1;
}

__global__ void __launch_bounds__(kBvhThreads) pm_bvh_kernel(const float *q, int64_t nq, const float4 *table, int64_t T, const int32_t *leaf_tri,
                                                             const int32_t *children, const float *boxes, float *out_d2, int32_t *out_j, float *out_b1,
                                                             float *out_b2, int32_t *out_visits)
{
    __shared__ int32_t stack[kBvhStack][kBvhThreads];           // 16 KB, [level][lane]
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kBvhThreads + lane;
    if (i >= nq) return;
    const float px = q[3 * i], py = q[3 * i + 1], pz = q[3 * i + 2];
    PmBest best{ __builtin_inff(), -1, 0.f, 0.f };
    if (!pm_finite3(px, py, pz)) {
        pm_store(false, best, i, out_d2, out_j, out_b1, out_b2);
        if (out_visits) out_visits[i] = 0;
        return;
    }
    int32_t visits = 0;
    if (T > 0) {
        float w = 0.f;
#pragma unroll
        for (int a = 0; a < 6; ++a) w = fmaxf(w, fabsf(boxes[a]));              // the root box is row 0 (inf when it is empty: skipped below)
        const float s = __fmul_rn(0x1p-18f, w);
        int32_t cur = T == 1 ? ~0 : 0;
        float key;
        bool have = !bvh_skip(boxes, 0, px, py, pz, s, best.d2, &key);
        int sp = 0;
        for (int64_t step = 0; step < 2 * T; ++step) {
            if (!have) {
                if (sp == 0) break;
                cur = stack[--sp][lane];
                if (bvh_skip(boxes, bvh_row(cur, T), px, py, pz, s, best.d2, &key)) continue;          // (pushed entries were validated)
            }
            have = false;
            if (cur < 0) {
                const int32_t j = leaf_tri[~cur];
                if (j >= 0 && j < T) {
                    const float4 *c = table + kPmVec * (int64_t)j;
                    pm_visit(px, py, pz, c[0], c[1], c[2], c[3], c[4], j, &best);
                    ++visits;
                }
                continue;
            }
            const int32_t c0 = children[2 * (int64_t)cur], c1 = children[2 * (int64_t)cur + 1];
            const int64_t r0 = bvh_row(c0, T), r1 = bvh_row(c1, T);
            float k0 = 0.f, k1 = 0.f;
            const bool go0 = r0 >= 0 && !bvh_skip(boxes, r0, px, py, pz, s, best.d2, &k0);
            const bool go1 = r1 >= 0 && !bvh_skip(boxes, r1, px, py, pz, s, best.d2, &k1);
            if (go0 && go1) {
                const bool swap = k1 < k0;                       // the left child first on a tie
                if (sp < kBvhStack) stack[sp++][lane] = swap ? c0 : c1;
                cur = swap ? c1 : c0;
                have = true;
            } else if (go0 || go1) {
                cur = go0 ? c0 : c1;
                have = true;
            }
        }
    }
    pm_store(true, best, i, out_d2, out_j, out_b1, out_b2);
    if (out_visits) out_visits[i] = visits;
}

// ---- rays through the same tree (include/neddf_hip.h: neddf_raycast_bvh_query states the rule and the equality argument) ----
struct RbRay {                      // what the box test needs of a ray, all fp64: origin, 1 / d per axis (unused where d == 0), [t_min, t_max]
    double ox, oy, oz, rx, ry, rz;
    bool zx, zy, zz;                // d_a == 0
    double t0, t1;
};

// one axis of the slab test against the bounds widened by 2 pad: every operation one rounded fp64 operation
__device__ __forceinline__ void rb_axis(float lo, float hi, double pad2, double o, double rcp, bool zero, double *te, double *tx, bool *out)
{
    const double wl = __dsub_rn((double)lo, pad2), wh = __dadd_rn((double)hi, pad2);
    if (zero) {
        *out = *out || o < wl || o > wh;
    } else {
        const double ta = __dmul_rn(__dsub_rn(wl, o), rcp), tb = __dmul_rn(__dsub_rn(wh, o), rcp);
        *te = fmax(*te, fmin(ta, tb));
        *tx = fmin(*tx, fmax(ta, tb));
    }
}

// the pruning rule of the ray traversal: true when box `row` need not be entered; *key = te, what orders two children
__device__ __forceinline__ bool rb_skip(const float *boxes, int64_t row, const RbRay &q, double pad2, float best_t, double *key)
{
    const float *b = boxes + 6 * row;
    const float lx = b[0], ly = b[1], lz = b[2], hx = b[3], hy = b[4], hz = b[5];
    double te = q.t0, tx = q.t1;
    bool out = false;
    rb_axis(lx, hx, pad2, q.ox, q.rx, q.zx, &te, &tx, &out);
    rb_axis(ly, hy, pad2, q.oy, q.ry, q.zy, &te, &tx, &out);
    rb_axis(lz, hz, pad2, q.oz, q.rz, q.zz, &te, &tx, &out);
    *key = te;
    return lx > hx || out || !(te <= tx) || te > (double)best_t;
}

// kAny == false: the first hit (out_t, out_j, out_b1, out_b2).  kAny == true: the ray stops at its first candidate, out_occ = 1 with one.
template <bool kAny>
__global__ void __launch_bounds__(kBvhThreads) rc_bvh_kernel(const float *ro, const float *rd, int64_t nr, const float *v, int64_t V, const int32_t *tri,
                                                             int64_t T, const int32_t *leaf_tri, const int32_t *children, const float *boxes,
                                                             float t_min, float t_max, float pad, float *out_t, int32_t *out_j, float *out_b1,
                                                             float *out_b2, uint8_t *out_occ, int32_t *out_visits)
{
    __shared__ int32_t stack[kBvhStack][kBvhThreads];           // 16 KB, [level][lane]
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kBvhThreads + lane;
    if (i >= nr) return;
    RcRay r;
    RcHit best{ __builtin_inff(), -1, 0.f, 0.f };
    const bool ok = rc_ray_setup(ro[3 * i], ro[3 * i + 1], ro[3 * i + 2], rd[3 * i], rd[3 * i + 1], rd[3 * i + 2], &r);
    int32_t visits = 0;
    if (ok && T > 0) {
        float w = 0.f;
#pragma unroll
        for (int a = 0; a < 6; ++a) w = fmaxf(w, fabsf(boxes[a]));              // the root box is row 0 (inf when it is empty: no walk)
        const double pd = (double)pad, wd = (double)w;
        const double far = __dsub_rn(__dmul_rn(0x1p21, pd), __dmul_rn(2.0, __dadd_rn(wd, __dmul_rn(2.0, pd))));
        const double omax = (double)fmaxf(fmaxf(fabsf(r.ox), fabsf(r.oy)), fabsf(r.oz));
        const bool walk = pad >= 0x1p-126f && pd >= __dmul_rn(0x1p-16, wd) && omax <= far;
        if (!walk) {
            // the rounding of o + t d is not small against pad (or pad against the boxes' rounding): every triangle, as the brute kernel
            for (int64_t j = 0; j < T; ++j) {
                float p[9];
                if (!rc_triangle(v, V, tri, j, p)) continue;
                rc_visit(r, t_min, t_max, pad, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], (int32_t)j, &best);
                ++visits;
                if (kAny && best.j >= 0) break;
            }
        } else {
            RbRay q;
            q.ox = (double)r.ox; q.oy = (double)r.oy; q.oz = (double)r.oz;
            q.zx = r.dx == 0.f; q.zy = r.dy == 0.f; q.zz = r.dz == 0.f;
            q.rx = q.zx ? 0.0 : __ddiv_rn(1.0, (double)r.dx);
            q.ry = q.zy ? 0.0 : __ddiv_rn(1.0, (double)r.dy);
            q.rz = q.zz ? 0.0 : __ddiv_rn(1.0, (double)r.dz);
            q.t0 = (double)t_min; q.t1 = (double)t_max;
            const double pad2 = __dmul_rn(2.0, pd);
            int32_t cur = T == 1 ? ~0 : 0;
            double key;
            bool have = !rb_skip(boxes, 0, q, pad2, best.t, &key);
            int sp = 0;
            for (int64_t step = 0; step < 2 * T; ++step) {
                if (!have) {
                    if (sp == 0) break;
                    cur = stack[--sp][lane];
                    if (rb_skip(boxes, bvh_row(cur, T), q, pad2, best.t, &key)) continue;          // (pushed entries were validated)
                }
                have = false;
                if (cur < 0) {
                    const int32_t j = leaf_tri[~cur];
                    float p[9];
                    if (j >= 0 && j < T && rc_triangle(v, V, tri, j, p)) {
                        rc_visit(r, t_min, t_max, pad, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], j, &best);
                        ++visits;
                        if (kAny && best.j >= 0) break;
                    }
                    continue;
                }
                const int32_t c0 = children[2 * (int64_t)cur], c1 = children[2 * (int64_t)cur + 1];
                const int64_t r0 = bvh_row(c0, T), r1 = bvh_row(c1, T);
                double k0 = 0.0, k1 = 0.0;
                const bool go0 = r0 >= 0 && !rb_skip(boxes, r0, q, pad2, best.t, &k0);
                const bool go1 = r1 >= 0 && !rb_skip(boxes, r1, q, pad2, best.t, &k1);
                if (go0 && go1) {
                    const bool swap = k1 < k0;                       // the left child first on a tie
                    if (sp < kBvhStack) stack[sp++][lane] = swap ? c0 : c1;
                    cur = swap ? c1 : c0;
                    have = true;
                } else if (go0 || go1) {
                    cur = go0 ? c0 : c1;
                    have = true;
                }
            }
        }
    }
    if (kAny) out_occ[i] = ok && best.j >= 0 ? 1 : 0;
    else rc_store(ok, best, i, out_t, out_j, out_b1, out_b2);
    if (out_visits) out_visits[i] = visits;
}

void launch_raycast_bvh(bool any_hit, const float *ro, const float *rd, int64_t nr, const float *v, int64_t V, const int32_t *tri, int64_t T,
                        const int32_t *leaf_tri, const int32_t *children, const float *boxes, float t_min, float t_max, float pad, float *t,
                        int32_t *triangle, float *b1, float *b2, uint8_t *occluded, int32_t *visits, hipStream_t s)
{
    if (nr <= 0) return;
    const dim3 grid((unsigned)((nr + kBvhThreads - 1) / kBvhThreads));
    if (any_hit)
        hipLaunchKernelGGL(rc_bvh_kernel<true>, grid, dim3(kBvhThreads), 0, s, ro, rd, nr, v, V, tri, T, leaf_tri, children, boxes, t_min, t_max, pad, t,
                           triangle, b1, b2, occluded, visits);
    else
        hipLaunchKernelGGL(rc_bvh_kernel<false>, grid, dim3(kBvhThreads), 0, s, ro, rd, nr, v, V, tri, T, leaf_tri, children, boxes, t_min, t_max, pad, t,
                           triangle, b1, b2, occluded, visits);
}

void launch_bvh_keys(const NnGrid &g, const float *v, int64_t V, const int32_t *tri, int64_t T, int64_t *keys, hipStream_t s)
{
    if (T <= 0) return;
    hipLaunchKernelGGL(bvh_keys_kernel, dim3((unsigned)((T + kPmThreads - 1) / kPmThreads)), dim3(kPmThreads), 0, s, g, v, V, tri, T, keys);
}

void launch_bvh_build(const int64_t *keys, const float *v, int64_t V, const int32_t *tri, int64_t T, int32_t *leaf_tri, int32_t *children, float *boxes,
                      int32_t *parent, int32_t *counter, hipStream_t s)
{
    if (T <= 0) return;
    const dim3 grid((unsigned)((T + kPmThreads - 1) / kPmThreads));
    hipLaunchKernelGGL(bvh_topology_kernel, grid, dim3(kPmThreads), 0, s, keys, T, leaf_tri, children, parent, counter);
    hipLaunchKernelGGL(bvh_fit_kernel, grid, dim3(kPmThreads), 0, s, v, V, tri, T, (const int32_t *)leaf_tri, (const int32_t *)children,
                       (const int32_t *)parent, counter, boxes);
}

void launch_point_mesh_bvh_query(const float *q, int64_t nq, const float *v, int64_t V, const int32_t *tri, int64_t T, float *table, const int32_t *leaf_tri,
                                 const int32_t *children, const float *boxes, float *d2, int32_t *triangle, float *b1, float *b2, int32_t *visits,
                                 hipStream_t s)
{
    if (nq <= 0) return;
    launch_point_mesh_prepare(v, V, tri, T, table, s);
    hipLaunchKernelGGL(pm_bvh_kernel, dim3((unsigned)((nq + kBvhThreads - 1) / kBvhThreads)), dim3(kBvhThreads), 0, s, q, nq, (const float4 *)table, T,
                       leaf_tri, children, boxes, d2, triangle, b1, b2, visits);
}

}  // namespace neddf
