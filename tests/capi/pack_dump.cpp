// pack_dump.cpp -- stand-alone driver of the host-only weight packer (neddf_amd/csrc/field_pack.hip) for tests/test_pack_host.py: no
// GPU, no Python, no library.  Built by the test together with field_pack.hip, the host side under AddressSanitizer + UBSan.
//
//   pack_dump <case file>...      writes <case file>.out for each
//
// Case file (little-endian, 4-byte words): neddf_field_desc | n_tensors handed to pack_field | tensors present | per tensor:
// weight count, bias count, the weights, the biases.
// Output: text lines, then the blob's bytes.  The argument blocks are read the way the kernels read them, after resolve(blob base):
//   rc <code> / err <text> / has3 <0|1> / blob <floats>
//   M <name> <offset> <super-steps> <columns> <operand policy>     a fragment-major matrix
//   V <name> <offset> <floats>                                      a float vector
//   N <name>                                                        a null pointer
//   S <name> <value>                                                a scalar (floats as f<bits>)
//   end
#include "field_pack.h"      // -I neddf_amd/csrc

#include <stdio.h>
#include <string.h>

using namespace neddf;

struct Dump {
    FILE *fp;
    const float *base;
    void mat(const std::string &name, const float *p, int ksteps, int cols, int operands)
    {
        if (!p) fprintf(fp, "N %s\n", name.c_str());
        else fprintf(fp, "M %s %td %d %d %d\n", name.c_str(), p - base, ksteps, cols, operands);
    }
    void vec(const std::string &name, const float *p, int n)
    {
        if (!p) fprintf(fp, "N %s\n", name.c_str());
        else fprintf(fp, "V %s %td %d\n", name.c_str(), p - base, n);
    }
    void i(const std::string &name, long long v) { fprintf(fp, "S %s %lld\n", name.c_str(), v); }
    void f(const std::string &name, float v)
    {
        uint32_t u;
        memcpy(&u, &v, 4);
        fprintf(fp, "S %s f%08x\n", name.c_str(), u);
    }
    void layer(const std::string &name, const LayerW &l, int cols, int operands)
    {
        mat(name + ".wp", l.wp, l.ksteps, cols, operands);
        vec(name + ".bias", l.bias, cols);
        i(name + ".ksteps", l.ksteps);
        i(name + ".stash", l.stash);
    }
    void stash(const std::string &name, const StashW &s, int cols, int operands)
    {
        mat(name + ".wp", s.wp, s.ksteps, cols, operands);
        i(name + ".col0", s.col0);
        i(name + ".ksteps", s.ksteps);
    }
    void enc(const std::string &name, const EncodeDesc &e)
    {
        i(name + ".E", e.E); i(name + ".Ed", e.Ed); i(name + ".KH", e.KH); i(name + ".KD", e.KD);
        for (int k = 0; k < 10; ++k) f(name + ".lowpass[" + std::to_string(k) + "]", e.lowpass[k]);
    }
};

static std::string idx(const char *name, int k) { return std::string(name) + "[" + std::to_string(k) + "]"; }

static void dump_ddf(Dump &o, const std::string &n, const DdfArgs &a)
{
    o.i(n + ".caller_pointers", !!a.pos + !!a.dir + !!a.var + !!a.scratch + !!a.rev_scratch + !!a.sched + !!a.features + !!a.ptaux + !!a.distance +
                                    !!a.density + !!a.aux_grad + !!a.rays.rd + !!a.rays.ro + !!a.rays.view + !!a.rays.dists + !!a.stamps);
    o.i(n + ".n_points", a.n_points); o.enc(n + ".enc", a.enc);
    o.i(n + ".n_layers", a.n_layers); o.i(n + ".activation", a.activation); o.i(n + ".density_activation", a.density_activation);
    for (int l = 0; l < kMaxLayers; ++l) o.layer(n + idx(".layer", l), a.layer[l], a.width, a.operands);
    o.i(n + ".n_stash", a.n_stash);
    for (int s = 0; s < kMaxStash; ++s) o.stash(n + idx(".stash", s), a.stash[s], a.width, a.operands);
    o.i(n + ".width", a.width);
    o.vec(n + ".w_ddf_out", a.w_ddf_out, a.width); o.vec(n + ".w_aux_out", a.w_aux_out, a.width);
    o.f(n + ".b_ddf_out", a.b_ddf_out); o.f(n + ".b_aux_out", a.b_aux_out); o.f(n + ".d_near", a.d_near); o.f(n + ".aux_grad_scale", a.aux_grad_scale);
    o.i(n + ".operands", a.operands); o.i(n + ".neus", a.neus); o.f(n + ".neus_v10", a.neus_v10);
    for (int l = 0; l < kMaxLayers; ++l) o.mat(n + idx(".wT", l), a.wT[l], a.ks_hidden, a.width, a.operands);
    o.mat(n + ".wT_pe0", a.wT_pe0, a.ks_hidden, 64, a.operands);
    for (int s = 0; s < kMaxStash; ++s) o.mat(n + idx(".wT_pe_skip", s), a.wT_pe_skip[s], a.ks_hidden, 64, a.operands);
    o.i(n + ".skip_layer", a.skip_layer); o.i(n + ".ks_hidden", a.ks_hidden); o.i(n + ".sched_flags", a.sched_flags); o.i(n + ".feat_rows", a.feat_rows);
    o.i(n + ".rays.S", a.rays.S); o.f(n + ".rays.r2", a.rays.r2); o.i(n + ".rays.cone", a.rays.cone); o.i(n + ".rays.base", a.rays.base);
}

static void dump_col(Dump &o, const std::string &n, const ColArgs &c)
{
    o.i(n + ".caller_pointers", !!c.pos + !!c.dir + !!c.var + !!c.features + !!c.ptaux + !!c.sched + !!c.color + !!c.penalty + !!c.stamps);
    o.i(n + ".n_points", c.n_points); o.enc(n + ".enc", c.enc);
    o.i(n + ".n_layers", c.n_layers); o.i(n + ".activation", c.activation); o.i(n + ".mode", c.mode); o.i(n + ".final_act", c.final_act);
    o.i(n + ".operands", c.operands); o.i(n + ".width", c.width); o.i(n + ".ksteps_a", c.ksteps_a);
    o.mat(n + ".wp_a", c.wp_a, c.ksteps_a, c.width, c.operands);
    for (int l = 0; l < kMaxLayers; ++l) o.layer(n + idx(".layer", l), c.layer[l], c.width, c.operands);
    o.vec(n + ".w_out", c.w_out, 3 * c.width);
    for (int k = 0; k < 3; ++k) o.f(n + idx(".b_out", k), c.b_out[k]);
    o.i(n + ".feat_rows", c.feat_rows); o.i(n + ".sched_flags", c.sched_flags); o.i(n + ".rays", c.rays); o.f(n + ".distance_range_max", c.distance_range_max);
    for (int k = 0; k < 6; ++k) { o.f(n + idx(".penalty_weight", k), c.penalty_weight[k]); o.i(n + idx(".penalty_has", k), c.penalty_has[k]); }
}

static void dump_nerf(Dump &o, const std::string &n, const NerfArgs &a, int head_cols)      // head_cols: engine width of the colour head's hidden layer
{
    o.i(n + ".caller_pointers", !!a.pos + !!a.dir + !!a.var + !!a.scratch + !!a.density + !!a.color);
    o.i(n + ".n_points", a.n_points); o.enc(n + ".enc", a.enc);
    o.i(n + ".n_layers", a.n_layers); o.i(n + ".activation", a.activation); o.i(n + ".density_activation", a.density_activation);
    for (int l = 0; l < kMaxLayers; ++l) o.layer(n + idx(".layer", l), a.layer[l], a.width, a.operands);
    o.i(n + ".n_stash", a.n_stash); o.i(n + ".col_stash", a.col_stash);
    for (int s = 0; s < kMaxStash; ++s) o.stash(n + idx(".stash", s), a.stash[s], a.n_stash && s == a.col_stash ? head_cols : a.width, a.operands);
    o.vec(n + ".w_density", a.w_density, a.width); o.f(n + ".b_density", a.b_density);
    o.layer(n + ".col0", a.col0, head_cols, a.operands);
    o.vec(n + ".w_col1", a.w_col1, 3 * head_cols);
    for (int k = 0; k < 3; ++k) o.f(n + idx(".b_col1", k), a.b_col1[k]);
    o.i(n + ".operands", a.operands); o.i(n + ".width", a.width);
}

static bool read_words(FILE *fp, void *p, size_t n) { return fread(p, 4, n, fp) == n; }

static int run_case(const char *path)
{
    FILE *in = fopen(path, "rb");
    if (!in) { fprintf(stderr, "pack_dump: cannot open %s\n", path); return 1; }
    neddf_field_desc d;
    int n_tensors = 0, n_present = 0;
    bool ok = read_words(in, &d, sizeof(d) / 4) && read_words(in, &n_tensors, 1) && read_words(in, &n_present, 1) && n_present >= 0 && n_present < 64;
    std::vector<std::vector<float>> w(ok ? n_present : 0), b(ok ? n_present : 0);
    for (int t = 0; ok && t < n_present; ++t) {
        int nw = 0, nb = 0;
        ok = read_words(in, &nw, 1) && read_words(in, &nb, 1) && nw >= 0 && nb >= 0;
        if (!ok) break;
        w[t].resize(nw); b[t].resize(nb);
        ok = read_words(in, w[t].data(), nw) && read_words(in, b[t].data(), nb);
    }
    fclose(in);
    if (!ok) { fprintf(stderr, "pack_dump: %s is not a case file\n", path); return 1; }
    std::vector<const float *> W, B;
    for (int t = 0; t < n_present; ++t) { W.push_back(w[t].data()); B.push_back(b[t].data()); }

    PackedField pk;
    std::string err;
    const int rc = pack_field(d, W.data(), B.data(), n_tensors, pk, err);
    FILE *fp = fopen((std::string(path) + ".out").c_str(), "wb");
    if (!fp) { fprintf(stderr, "pack_dump: cannot write %s.out\n", path); return 1; }
    fprintf(fp, "rc %d\nerr %s\nhas3 %d\n", rc, err.c_str(), pk.has3 ? 1 : 0);
    if (rc == 0) {          // (a refused field: nothing is uploaded and no argument block is taken over)
        pk.resolve(pk.blob.data());
        Dump o{ fp, pk.blob.data() };
        fprintf(fp, "blob %zu\n", pk.blob.size());
        dump_ddf(o, "ddf", pk.ddf); dump_col(o, "col", pk.col);
        dump_ddf(o, "ddf3", pk.ddf3); dump_col(o, "col3", pk.col3);
        const int wh = d.layer_width / 2;
        dump_nerf(o, "nerf", pk.nerf, ((wh > 0 ? wh : 1) + 127) / 128 * 128);
        fprintf(fp, "end\n");
        fwrite(pk.blob.data(), sizeof(float), pk.blob.size(), fp);
    } else fprintf(fp, "end\n");
    fclose(fp);
    return 0;
}

int main(int argc, char **argv)
{
    for (int k = 1; k < argc; ++k)
        if (run_case(argv[k])) return 1;
    return 0;
}
