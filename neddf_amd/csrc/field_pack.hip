// field_pack.hip -- see field_pack.h.  One trunk packer, one transpose packer and one colour-trunk loop serve the three networks; what
// really differs between them (small-input maps, heads, the NeRF colour head) stays in pack_neddf / pack_neus / pack_nerf.
#include "field_pack.h"

#include <initializer_list>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using namespace neddf;

// round-to-nearest-even fp32 -> bf16 bit pattern (what v_cvt_pk_bf16_f32 does on the device)
static inline uint16_t bf16_bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);      // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// fp32 -> IEEE half bit pattern, round to nearest even (toward_zero = false) or toward zero (true; never overflows to inf)
static inline uint16_t f16_bits(float f, bool toward_zero)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    const uint32_t sign = (u >> 16) & 0x8000u;
    u &= 0x7fffffffu;
    if (u >= 0x7f800000u) return (uint16_t)(sign | (u > 0x7f800000u ? 0x7e00u : (toward_zero ? 0x7bffu : 0x7c00u)));
    if (u >= 0x477ff000u) {                                     // >= 65520: beyond the largest half
        if (toward_zero || u < 0x477ff000u) return (uint16_t)(sign | 0x7bffu);
        return (uint16_t)(sign | (toward_zero ? 0x7bffu : 0x7c00u));
    }
    if (u < 0x33000000u) return (uint16_t)sign;                 // < 2^-25: rounds to zero
    int e = (int)(u >> 23) - 127;
    uint32_t man = (u & 0x7fffffu) | 0x800000u;                 // 24-bit significand
    int shift = e >= -14 ? 13 : 13 + (-14 - e);                 // bits dropped (subnormal halves drop more)
    uint32_t q = man >> shift, rem = man & ((1u << shift) - 1), halfway = 1u << (shift - 1);
    if (!toward_zero && (rem > halfway || (rem == halfway && (q & 1)))) ++q;
    uint32_t h = e >= -14 ? (uint32_t)((e + 15) << 10) + (q - 0x400u) : q;      // q carries into the exponent on overflow
    return (uint16_t)(sign | h);
}

static inline float f16_value(uint16_t h)
{
    const int e = (h >> 10) & 31, m = h & 0x3ff;
    float v = e == 0 ? ldexpf((float)m, -24) : ldexpf((float)(m | 0x400), e - 25);
    return (h & 0x8000) ? -v : v;
}

static inline float bf16_value(uint16_t b)
{
    const uint32_t u = (uint32_t)b << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// w = hi + mid + lo in bf16 (tile_engine.h OpsF32x3T): each term the bf16 rounding of what the previous ones left.  Exact for every
// finite fp32 w that bf16 does not round up to infinity -- checked here for every packed weight, not assumed
static inline bool bf16x3_split(float w, uint16_t t[3])
{
    t[0] = bf16_bits(w);
    const float r1 = w - bf16_value(t[0]);
    t[1] = bf16_bits(r1);
    const float r2 = r1 - bf16_value(t[1]);
    t[2] = bf16_bits(r2);
    return bf16_value(t[2]) == r2 && (double)bf16_value(t[0]) + (double)bf16_value(t[1]) + (double)bf16_value(t[2]) == (double)w;
}

// a finite value that fp16 rounds to infinity (NaN and Inf themselves keep their class in fp16, as under every policy)
static inline bool beyond_f16(float v) { return isfinite(v) && fabsf(v) > 65504.0f; }

// fragment-major packing, see kernels.h LayerW.  kmap is padded to a whole number of super-steps: 8 k-values for fp32 fragments
// (4 floats per lane half), 16 for the 16-bit ones (8 per lane half).
size_t pack_layer(std::vector<float> &blob, const Src &src, std::vector<int> kmap, int nout, int operands, int *ksteps_out, bool *split_exact)
{
    // operands == 2 (split fp16): two fp16 planes of 2^10 w (h toward zero, m = remainder to nearest), 32 bytes per lane and super-step
    // operands == 3 (fp32 as three bf16 terms): planes hi, mid, lo of the 32x32x16 fragment, 48 bytes per lane and super-step
    // operands == 4 (kOperandsH16, plain fp16): the bf16 fragment with every weight rounded to the nearest-even half instead; split_exact
    // is cleared by a finite weight beyond +-65504
    const int step = operands ? 16 : 8, half = step / 2, tiles = nout / 32, planes = operands == 2 ? 2 : (operands == 3 ? 3 : 1);
    while (kmap.size() % step) kmap.push_back(-1);
    const int ks = (int)kmap.size() / step;
    if (ksteps_out) *ksteps_out = ks;
    size_t off = roundup((int)blob.size(), 64);
    const size_t elems = (size_t)ks * step * nout;
    blob.resize(off + (operands ? elems * planes / 2 : elems), 0.f);
    float *dst = blob.data() + off;
    uint16_t *dst16 = (uint16_t *)dst;
    for (int tile = 0; tile < tiles; ++tile)            // tile-major: tile = wave * NT + t in the kernels
        for (int S = 0; S < ks; ++S)
            for (int lane = 0; lane < 64; ++lane)
                for (int r = 0; r < half; ++r) {
                    int n = tile * 32 + (lane & 31);
                    int k = kmap[step * S + half * (lane >> 5) + r];
                    float v = (k < 0 || n >= src.cols) ? 0.f : src.at(k, n);
                    size_t frag = (((size_t)tile * ks + S) * 64 + lane);
                    if (operands == 3) {
                        uint16_t t[3];
                        if (!bf16x3_split(v, t) && split_exact) *split_exact = false;
                        for (int pl = 0; pl < 3; ++pl) dst16[(frag * 3 + pl) * half + r] = t[pl];
                    } else if (operands == 2) {
                        const float sv = v * 1024.0f;
                        uint16_t h = f16_bits(sv, true);
                        dst16[(frag * 2 + 0) * half + r] = h;
                        dst16[(frag * 2 + 1) * half + r] = f16_bits(sv - f16_value(h), false);
                    } else if (operands == kOperandsH16) {
                        if (beyond_f16(v) && split_exact) *split_exact = false;
                        dst16[frag * half + r] = f16_bits(v, false);
                    } else if (operands) dst16[frag * half + r] = bf16_bits(v);
                    else dst[frag * half + r] = v;
                }
    return off;
}

size_t put(std::vector<float> &blob, const float *p, size_t n, size_t n_padded)
{
    size_t off = roundup((int)blob.size(), 64);
    blob.resize(off + (n_padded > n ? n_padded : n), 0.f);
    memcpy(blob.data() + off, p, n * sizeof(float));
    return off;
}

// engine columns of a hidden state of `width` features (zero-padded to the engine width wp) -> reference weight row base + k
static std::vector<int> hidden_map(int width, int wp, int base)
{
    std::vector<int> m;
    for (int k = 0; k < wp; ++k) m.push_back(k < width ? base + k : -1);
    return m;
}

// engine width of a hidden width: the next multiple of 128 (four waves x 32-column MFMA tiles).  The padding columns carry zero
// weights and biases, so they hold a(0) = 0 under every activation of the reference and feed zero rows downstream: exact.
// A tile row also has to hold both encodings next to a 32-column block (enc_columns): a narrow network with long encodings takes the next
// engine width that does
int enc_columns(const neddf_field_desc &d) { return 2 * roundup(3 * d.embed_pos_rank, 4) + 2 * roundup(3 * d.embed_dir_rank, 4) + 32; }
static int engine_width(int width, const neddf_field_desc &d)
{
    int w = roundup(width, 128);
    while (w < enc_columns(d)) w += 128;
    return w;
}

// engine columns of the [sin half | cos half] encoding -> reference feature index base+...
static void enc_map(std::vector<int> &m, int rank, int K, int base)
{
    for (int q = 0; q < K; ++q) m.push_back(q < 3 * rank ? base + q : -1);
    for (int q = 0; q < K; ++q) m.push_back(q < 3 * rank ? base + 3 * rank + q : -1);
}

// How fp32 NeDDF fields take their products on the eval-minimal route (reverse-mode distance kernel + colour kernel), read once:
//   NEDDF_F32_PRODUCTS=split3 (default)  three-term bf16 splits on v_mfma_f32_32x32x16_bf16 (tile_engine.h OpsF32x3T): fp32-accurate
//   NEDDF_F32_PRODUCTS=mfma              v_mfma_f32_32x32x2_f32, the exact-fp32 route of earlier versions, bit for bit
// The forward-mode kernels (full outputs, NEDDF_DDF_REVERSE=0), NeRF, NeuS and the training kernels take the fp32 MFMA either way.
static bool f32_products_split3()
{
    static const bool v = [] {
        const char *e = getenv("NEDDF_F32_PRODUCTS");
        if (e && *e && strcmp(e, "mfma") != 0 && strcmp(e, "split3") != 0)
            fprintf(stderr, "neddf: NEDDF_F32_PRODUCTS=%s is neither 'split3' nor 'mfma'; taking split3\n", e);
        return !e || strcmp(e, "mfma") != 0;
    }();
    return v;
}

// One packing pass: appends under one operand policy and binds the pointer that will read each block where the block is appended
struct Packer {
    PackedField &out;
    const neddf_field_desc &d;
    const float *const *W, *const *B;
    std::string &err;
    int operands;
    bool *exact;                // pack_layer's split_exact (fp16: cleared by a finite value beyond +-65504, in a matrix, a vector or a scalar)
    const int E = d.embed_pos_rank, Ed = d.embed_dir_rank, KH = roundup(3 * E, 4), KD = roundup(3 * Ed, 4), Cpe = 6 * E, Cdir = 6 * Ed;
    void layer(const float *&slot, const Src &src, const std::vector<int> &kmap, int nout, int *ksteps)
    {
        out.fixes.push_back({ &slot, pack_layer(out.blob, src, kmap, nout, operands, ksteps, exact) });
    }
    void vec(const float *&slot, const float *p, size_t n, size_t n_padded = 0)
    {
        if (operands == kOperandsH16 && exact)
            for (size_t i = 0; i < n; ++i) if (beyond_f16(p[i])) *exact = false;
        out.fixes.push_back({ &slot, put(out.blob, p, n, n_padded) });
    }
    void scalars(std::initializer_list<float> v)         // the biases and the NeuS variance that travel in the argument blocks themselves
    {
        if (operands == kOperandsH16 && exact)
            for (float x : v) if (beyond_f16(x)) *exact = false;
    }
    int fail(int code, const std::string &msg) { err = msg; return code; }
};

// What differs between the trunks of the three networks
struct Trunk {
    const char *name, *skip_rule;       // for the refusals
    bool transposed;                    // storage [out][in] (nn.Linear) instead of LinearGradLayer's [in][out]
    bool enc_first;                     // a skip layer's input is cat([encoding, h]) instead of cat([h, encoding])
    int max_stash;                      // skip connections the kernel has stash slots for
};
static const Trunk kNeddfTrunk{ "NeDDF", "a trunk layer followed by another (the reference itself fails otherwise)", false, true, kMaxStash };
static const Trunk kNeusTrunk{ "NeuS", "an sdf layer followed by another", true, false, kMaxStash };
static const Trunk kNerfTrunk{ "NeRF", "a layer followed by another", true, false, kMaxStash - 1 };      // (the colour head's direction segment takes the last slot)

// Layers 0 .. n-1 of a trunk of `width` features on engine width WP: layer 0 through the encoding map, the later ones through the hidden
// map, the encoding rows of a skip layer into a stash slot, biases zero-padded
template <class Args>
static int pack_trunk(Packer &p, const Trunk &t, Args &a, int n, int width, int WP)
{
    for (int i = 0; i < p.d.n_skips; ++i)
        if (p.d.skips[i] < 0 || p.d.skips[i] >= n - 1) return p.fail(NEDDF_EUNSUPPORTED, std::string(t.name) + ": skip index must address " + t.skip_rule);
    std::vector<int> pe0, pes;
    enc_map(pe0, p.E, p.KH, 0);
    enc_map(pes, p.E, p.KH, t.enc_first ? 0 : width);
    a.n_layers = n; a.n_stash = 0;
    for (int l = 0; l < n; ++l) {
        const bool wide = l > 0 && in_skips(p.d, l - 1);
        Src src{ p.W[l], l == 0 ? p.Cpe : (wide ? width + p.Cpe : width), width, t.transposed };
        a.layer[l].stash = -1;
        p.layer(a.layer[l].wp, src, l == 0 ? pe0 : hidden_map(width, WP, wide && t.enc_first ? p.Cpe : 0), WP, &a.layer[l].ksteps);
        if (wide) {
            if (a.n_stash >= t.max_stash) return p.fail(NEDDF_EUNSUPPORTED, std::string(t.name) + ": more than " + std::to_string(t.max_stash) + " skip connections");
            p.layer(a.stash[a.n_stash].wp, src, pes, WP, &a.stash[a.n_stash].ksteps);
            a.stash[a.n_stash].col0 = 0;
            a.layer[l].stash = a.n_stash++;
        }
        p.vec(a.layer[l].bias, p.B[l], width, WP);
    }
    return 0;
}

// Reverse-mode gradient (ddf_rev_kernel): the transposes.  dL/dH_{l-1} = g_l x (hidden rows of W_l)^T is a dense product with
// B[k][n] = W_l[in = row0 + n][out = k]; the gradient of the encoding collects g_0 x W_0^T and g_skip x (encoding rows of W_skip)^T,
// 64 engine columns wide (same [sin half | cos half] order as the forward encoding in LDS)
static void pack_transposes(Packer &p, const Trunk &t, DdfArgs &a, int n, int width, int WP)
{
    const std::vector<int> kall = hidden_map(width, WP, 0);
    // narrow transposes: column j of the engine's encoding layout is input feature cols[j] of the layer (or padding)
    auto pack_pe_T = [&](const float *&slot, const float *Wl, int cin, int base) {
        std::vector<int> cols;
        enc_map(cols, p.E, p.KH, base);
        std::vector<float> tmp((size_t)width * 64, 0.f);           // [k][j] row-major, j < 64
        for (int j = 0; j < (int)cols.size() && j < 64; ++j)
            if (cols[j] >= 0)
                for (int k = 0; k < width; ++k) tmp[(size_t)k * 64 + j] = t.transposed ? Wl[(size_t)k * cin + cols[j]] : Wl[(size_t)cols[j] * width + k];
        p.layer(slot, Src{ tmp.data(), width, 64, false }, kall, 64, nullptr);
    };
    a.skip_layer = -1;
    for (int l = 1; l < n; ++l) {
        const bool wide = in_skips(p.d, l - 1);
        const int cin = wide ? width + p.Cpe : width, row0 = wide && t.enc_first ? p.Cpe : 0;
        // nn.Linear's [out][in] storage is B itself (row stride cin); [in][out] storage is B^T from row row0 on
        p.layer(a.wT[l], t.transposed ? Src{ p.W[l] + row0, width, width, false, cin } : Src{ p.W[l] + (size_t)row0 * width, width, width, true }, kall, WP, nullptr);
        if (wide) { a.skip_layer = l; pack_pe_T(a.wT_pe_skip[a.layer[l].stash], p.W[l], cin, t.enc_first ? 0 : width); }
    }
    pack_pe_T(a.wT_pe0, p.W[0], p.Cpe, 0);
}

// Colour trunk behind a distance / sdf trunk of `feat` features: layer 0 = the small-input segment (engine columns `small`) + the
// feature segment (input rows from feat_row on), then n - 1 hidden layers; W / B start at the colour trunk's first tensor
static void pack_col_trunk(Packer &p, const Trunk &t, ColArgs &c, const float *const *W, const float *const *B, int n, const std::vector<int> &small,
                           int feat_row, int feat, int width, int WP)
{
    p.layer(c.wp_a, Src{ W[0], feat_row + feat, width, t.transposed }, small, WP, &c.ksteps_a);
    c.n_layers = n;
    for (int l = 0; l < n; ++l) {
        Src src{ W[l], l == 0 ? feat_row + feat : width, width, t.transposed };
        p.layer(c.layer[l].wp, src, l == 0 ? hidden_map(feat, WP, feat_row) : hidden_map(width, WP, 0), WP, &c.layer[l].ksteps);
        c.layer[l].stash = -1;
        p.vec(c.layer[l].bias, B[l], width, WP);
    }
}

// NeDDF (neddf/network/neddf.py): the argument blocks of one operand policy
static int pack_neddf(Packer &p, DdfArgs &a, ColArgs &c)
{
    const neddf_field_desc &d = p.d;
    const int n_trunk = d.layer_count - 1, n_col = d.col_layer_count - 1, Wd = d.layer_width, WP = engine_width(Wd, d);
    a = DdfArgs{}; c = ColArgs{};
    if (int rc = pack_trunk(p, kNeddfTrunk, a, n_trunk, Wd, WP)) return rc;
    const int i_ddf = n_trunk + n_col, i_aux = i_ddf + 1, i_cout = i_ddf + 2;
    p.vec(a.w_ddf_out, p.W[i_ddf], Wd, WP);
    p.vec(a.w_aux_out, p.W[i_aux], Wd, WP);
    a.b_ddf_out = p.B[i_ddf][0]; a.b_aux_out = p.B[i_aux][0];
    p.scalars({ a.b_ddf_out, a.b_aux_out, p.B[i_cout][0], p.B[i_cout][1], p.B[i_cout][2] });
    pack_transposes(p, kNeddfTrunk, a, n_trunk, Wd, WP);
    std::vector<int> ka;        // engine columns [pos sin KH | pos cos KH | dir sin KD | dir cos KD | normal 3]
    enc_map(ka, p.E, p.KH, 0);
    enc_map(ka, p.Ed, p.KD, p.Cpe);
    for (int k = 0; k < 3; ++k) ka.push_back(p.Cpe + p.Cdir + k);
    pack_col_trunk(p, kNeddfTrunk, c, p.W + n_trunk, p.B + n_trunk, n_col, ka, p.Cpe + p.Cdir + 3, Wd, Wd, WP);
    p.vec(c.w_out, p.W[i_cout], (size_t)Wd * 3, (size_t)WP * 3);
    for (int k = 0; k < 3; ++k) c.b_out[k] = p.B[i_cout][k];
    a.ks_hidden = WP / (p.operands ? 16 : 8);
    a.width = c.width = WP;
    a.activation = c.activation = d.activation;
    a.density_activation = d.density_activation;
    a.d_near = d.d_near;
    a.operands = c.operands = p.operands;
    c.final_act = -1;
    for (int k = 0; k < 6; ++k) { c.penalty_weight[k] = d.penalty_weight[k]; c.penalty_has[k] = d.penalty_has[k]; }
    return 0;
}

// NeuS (neddf/network/neus.py): sdf trunk with Jacobian rows on the distance kernel (forward-mode replaces the
// reference's torch.autograd.grad), colour trunk on the colour kernel.
static int pack_neus(Packer &p, DdfArgs &a, ColArgs &c)
{
    const neddf_field_desc &d = p.d;
    // sdf and colour trunks may have different widths (neus.py:80-99); both run on one engine width, zero-padded
    const int n_sdf = d.layer_count, n_col = d.col_layer_count, Ws = d.layer_width, Wc = d.col_layer_width, WP = engine_width(Ws > Wc ? Ws : Wc, d);
    a = DdfArgs{}; c = ColArgs{};
    if (int rc = pack_trunk(p, kNeusTrunk, a, n_sdf, Ws, WP)) return rc;
    // Reverse-mode normal (ddf_rev_kernel): the sdf is feature 0 of the last activated layer, so the seed of the reverse pass is
    // e_0 * y'_L -- the "distance head" of the kernel becomes the unit vector e_0 with zero bias, the aux head is zero
    pack_transposes(p, kNeusTrunk, a, n_sdf, Ws, WP);
    std::vector<float> e0(WP, 0.f), zero(WP, 0.f);
    e0[0] = 1.0f;
    p.vec(a.w_ddf_out, e0.data(), WP);
    p.vec(a.w_aux_out, zero.data(), WP);
    a.b_ddf_out = 0.f; a.b_aux_out = 0.f;
    std::vector<int> ka;        // engine columns [pos 3 | gradient 3 | pad 2 | dir sin KD | dir cos KD]
    for (int k = 0; k < 3; ++k) ka.push_back(k);
    for (int k = 0; k < 3; ++k) ka.push_back(3 + p.Cdir + k);
    ka.push_back(-1); ka.push_back(-1);
    enc_map(ka, p.Ed, p.KD, 3);
    pack_col_trunk(p, kNeusTrunk, c, p.W + n_sdf, p.B + n_sdf, n_col, ka, 6 + p.Cdir, Ws, Wc, WP);
    std::vector<float> wout((size_t)WP * 3, 0.f);         // [3][Wc] -> [WP][3]
    for (int k = 0; k < Wc; ++k)
        for (int o = 0; o < 3; ++o) wout[k * 3 + o] = p.W[n_sdf + n_col][(size_t)o * Wc + k];
    p.vec(c.w_out, wout.data(), wout.size());
    for (int k = 0; k < 3; ++k) c.b_out[k] = p.B[n_sdf + n_col][k];
    a.ks_hidden = WP / (p.operands ? 16 : 8);
    a.width = c.width = WP;
    a.activation = c.activation = d.activation;
    a.neus = 1;
    a.operands = c.operands = p.operands;
    a.neus_v10 = p.W[n_sdf + n_col + 1][0] * 10.0f;
    p.scalars({ c.b_out[0], c.b_out[1], c.b_out[2], p.W[n_sdf + n_col + 1][0] });
    c.mode = 1;
    c.final_act = d.activation;
    return 0;
}

static int pack_nerf(Packer &p, NerfArgs &a)
{
    const neddf_field_desc &d = p.d;
    const int n = d.layer_count, step = p.operands ? 16 : 8, Wn = d.layer_width, WP = engine_width(Wn, d);
    const int Wh = Wn / 2, HC = roundup(Wh > 0 ? Wh : 1, 128);      // colour head's hidden layer (nerf.py:99-103: layer_width // 2) and its engine width
    a = NerfArgs{};
    if (int rc = pack_trunk(p, kNerfTrunk, a, n, Wn, WP)) return rc;
    p.vec(a.w_density, p.W[n], Wn, WP);
    a.b_density = p.B[n][0];
    // colour head: Linear(layer_width + dir, layer_width // 2), the direction encoding as one more early partial
    Src sc{ p.W[n + 1], Wn + p.Cdir, Wh, true };
    std::vector<int> kd;
    enc_map(kd, p.Ed, p.KD, Wn);
    p.layer(a.col0.wp, sc, hidden_map(Wn, WP, 0), HC, &a.col0.ksteps);
    a.col0.stash = a.col_stash = a.n_stash++;
    p.layer(a.stash[a.col_stash].wp, sc, kd, HC, &a.stash[a.col_stash].ksteps);
    a.stash[a.col_stash].col0 = roundup(2 * p.KH, step);          // direction encoding: first super-step boundary after the position encoding
    p.vec(a.col0.bias, p.B[n + 1], Wh, HC);
    std::vector<float> w1((size_t)3 * HC, 0.f);               // [3][Wh] -> [3][HC]
    for (int o = 0; o < 3; ++o) memcpy(&w1[(size_t)o * HC], p.W[n + 2] + (size_t)o * Wh, (size_t)Wh * sizeof(float));
    p.vec(a.w_col1, w1.data(), w1.size());
    for (int k = 0; k < 3; ++k) a.b_col1[k] = p.B[n + 2][k];
    p.scalars({ a.b_density, a.b_col1[0], a.b_col1[1], a.b_col1[2] });
    a.activation = d.activation;
    a.density_activation = d.density_activation;
    a.operands = p.operands;
    a.width = WP;
    return 0;
}

int pack_field(const neddf_field_desc &d, const float *const *W, const float *const *B, int n_tensors, PackedField &out, std::string &err)
{
    // the operand policy of a weight_dtype: 0 fp32, 1 bf16, 2 split fp16 as they are; plain fp16 is kOperandsH16 (3 is the three-term packing)
    bool in_range = true;
    const bool h16 = d.weight_dtype == NEDDF_DTYPE_F16;
    Packer p{ out, d, W, B, err, h16 ? kOperandsH16 : d.weight_dtype, h16 ? &in_range : nullptr };
    const auto done = [&](int rc) {
        if (rc == 0 && !in_range)
            return p.fail(NEDDF_EUNSUPPORTED, "weight_dtype f16: a finite weight or bias beyond +-65504 would become Inf as an fp16 operand");
        return rc;
    };
    const int n = d.layer_count, n_col = d.col_layer_count;
    out.has3 = false;
    if (d.kind == NEDDF_FIELD_NEDDF) {
        if (d.col_layer_width != d.layer_width)
            return p.fail(NEDDF_EUNSUPPORTED, "NeDDF: col_layer_width must equal ddf_layer_width (the reference's layer_col_out takes ddf_layer_width inputs, "
                                              "neddf.py:145: its own forward fails otherwise)");
        if (n_tensors != n + n_col + 1) return p.fail(NEDDF_EINVAL, "NeDDF: wrong tensor count");
        if (n < 2 || n - 1 > kMaxLayers || n_col < 2 || n_col - 1 > kMaxLayers) return p.fail(NEDDF_EUNSUPPORTED, "NeDDF: layer count out of range");
        if (int rc = done(pack_neddf(p, out.ddf, out.col))) return rc;
        // fp32 fields: the reverse-mode distance kernel and the colour kernel of the eval-minimal route take their products as three-term
        // bf16 splits (operands 3, tile_engine.h OpsF32x3T) from a second packing of the same weights; the forward-mode kernels keep the first
        if (d.weight_dtype == NEDDF_DTYPE_F32 && f32_products_split3()) {
            bool exact = true;
            const size_t n_fixes = out.fixes.size();
            Packer p3{ out, d, W, B, err, 3, &exact };
            if (int rc = pack_neddf(p3, out.ddf3, out.col3)) return rc;
            if (!exact) out.fixes.resize(n_fixes);      // a weight that does not split: the packing is never read, its pointers stay null
            out.has3 = exact;
        }
        return 0;
    }
    if (d.kind == NEDDF_FIELD_NERF) {
        if (n_tensors != n + 3) return p.fail(NEDDF_EINVAL, "NeRF: wrong tensor count");
        if (n < 1 || n > kMaxLayers) return p.fail(NEDDF_EUNSUPPORTED, "NeRF: layer count out of range");
        return done(pack_nerf(p, out.nerf));
    }
    if (d.kind == NEDDF_FIELD_NEUS) {
        if (n_tensors != n + n_col + 2) return p.fail(NEDDF_EINVAL, "NeuS: wrong tensor count");
        if (n < 1 || n > kMaxLayers || n_col < 1 || n_col > kMaxLayers) return p.fail(NEDDF_EUNSUPPORTED, "NeuS: layer count out of range");
        if (d.activation == NEDDF_ACT_LEAKY) return p.fail(NEDDF_EUNSUPPORTED, "NeuS: activation must be ReLU or tanhExp");
        return done(pack_neus(p, out.ddf, out.col));
    }
    return p.fail(NEDDF_EINVAL, "bad field kind");
}
