// field_pack.h -- weight packing of neddf_set_field: the state tensors of a NeDDF, NeRF or NeuS network -> one host blob in MFMA fragment
// order (kernels.h LayerW) and the argument blocks that point into it.  Host arithmetic only (field_pack.hip): no kernel, no HIP runtime
// call, no context -- neddf_capi.hip uploads the blob and resolves the pointers.  Not installed.
#pragma once
#include "../../include/neddf_hip.h"
#include "kernels.h"

#include <string>
#include <vector>

static inline int roundup(int x, int m) { return (x + m - 1) / m * m; }

static inline bool in_skips(const neddf_field_desc &d, int id)
{
    for (int i = 0; i < d.n_skips; ++i) if (d.skips[i] == id) return true;
    return false;
}

// a weight matrix, logical [in = rows][out = cols]; ld = storage stride (0: dense)
struct Src {
    const float *w;
    int rows, cols;
    bool transposed;      // storage is [out][in] (nn.Linear)
    int ld;
    Src(const float *w, int rows, int cols, bool transposed, int ld = 0) : w(w), rows(rows), cols(cols), transposed(transposed), ld(ld ? ld : (transposed ? rows : cols)) {}
    float at(int k, int n) const { return transposed ? w[(size_t)n * ld + k] : w[(size_t)k * ld + n]; }
};

// Appends to `blob` at the next 64-float boundary and returns the offset.  pack_layer: fragment-major under an operand policy (0 fp32,
// 1 bf16, 2 split fp16, 3 fp32 as three bf16 terms, 4 plain fp16; split_exact is cleared when a weight does not split exactly under 3
// or is finite and beyond fp16's range under 4), kmap = engine
// column -> weight row (-1 = zero), nout a multiple of 32.  put: n floats, zero-padded to n_padded.
size_t pack_layer(std::vector<float> &blob, const Src &src, std::vector<int> kmap, int nout, int operands, int *ksteps_out, bool *split_exact = nullptr);
size_t put(std::vector<float> &blob, const float *p, size_t n, size_t n_padded = 0);

// columns of a tile row that both encodings and one 32-column block take (neddf_set_field refuses descriptors beyond kMaxWidth)
int enc_columns(const neddf_field_desc &d);

// everything neddf_set_field stores in a Field besides the device block
struct PackedField {
    std::vector<float> blob;
    neddf::DdfArgs ddf{}, ddf3{};
    neddf::ColArgs col{}, col3{};
    neddf::NerfArgs nerf{};
    bool has3 = false;      // ddf3 / col3 hold the three-term second packing of an fp32 NeDDF field (NEDDF_F32_PRODUCTS)
    // every weight pointer of the argument blocks = base + its offset in the blob.  Each is bound where its data is appended (fixes point
    // into this object: it is not copyable)
    void resolve(const float *base) { for (const Fix &f : fixes) *f.slot = base + f.off; }
    struct Fix { const float **slot; size_t off; };
    std::vector<Fix> fixes;
    PackedField() = default;
    PackedField(const PackedField &) = delete;
    PackedField &operator=(const PackedField &) = delete;
};

// 0, or the NEDDF_E* code with its message in err
int pack_field(const neddf_field_desc &d, const float *const *W, const float *const *B, int n_tensors, PackedField &out, std::string &err);
