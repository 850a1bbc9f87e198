// field_plan.h -- how field_forward (neddf_capi.hip) cuts N points into launches, as plain functions over plain numbers: no HIP call, no
// getenv, host only.  tests/capi/field_plan.cpp drives it on the CPU under AddressSanitizer + UBSan (tests/test_field_plan.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace neddf {

struct FieldPlanIn {
    bool full;                  // the four-row Jacobian route (penalties): 2^19 points per launch
    bool use3;                  // the three-term fp32 policy (reverse-mode NeDDF only): its distance kernel runs in sub-launches
    int64_t N;
    int chunk_env;              // NEDDF_FIELD_CHUNK_LOG2 as parsed (0: not set); clamped to 16..25 here
    size_t feat_row, aux_row;   // bytes per hand-off point: features, per-point record
    size_t feat_cap, aux_cap;   // what the two hand-off buffers hold now
    size_t cache_row;           // a launch size settled earlier (`cache_chunk` > 0) for a hand-off of `cache_row` bytes per point
    int64_t cache_chunk;
};

struct FieldPlan {
    int64_t chunk;              // points per launch of the colour kernel (and per hand-off)
    int64_t ddf_sub;            // points per launch of the distance kernel inside a chunk
    bool probed;                // the free-memory probe was asked
    bool cache;                 // the probe shrank the chunk: the caller remembers (feat_row + aux_row, chunk)
};

// Points per launch of the field kernels.  Every launch boundary drains the persistent grid (workgroups finish up to one tile
// apart) and refills it: at 2^21 points a 65 536-ray x 128-sample call was four launch pairs, at 2^23 it is one -- fp32 +0.8 %,
// split fp16 +0.7 %, bf16 +2.8 % (profiles/r04_launch_size.txt).  The hand-off buffers grow with it (1 088 B per point
// eval-minimal: 9.1 GB at 2^23 of the 288 GB); NEDDF_FIELD_CHUNK_LOG2 overrides.
// `probe(size_t &free_bytes) -> bool` asks the device for its free memory (false: it could not tell); it is called at most once, and
// only when a hand-off buffer would have to grow.
template <class Probe>
inline FieldPlan field_plan(const FieldPlanIn &in, Probe &&probe)
{
    const int env = !in.chunk_env ? 0 : (in.chunk_env < 16 ? 16 : (in.chunk_env > 25 ? 25 : in.chunk_env));
    FieldPlan p{};
    // The three-term fp32 DISTANCE kernel is the exception: its L2 hit rate FALLS with the launch size (per 2^23 points: 83 % of the
    // TCC requests hit in 2^19-point launches, 74 % at 2^21, 65 % at 2^23; fabric reads 42 / 83 / 125 M KB) and it is fastest in
    // launches of 2^20 points (profiles/r09_alignment.txt, r09_launch_size_ab.txt).  The colour kernel behind it and every other policy
    // still prefer the large launch.  So a chunk's distance kernel runs as sub-launches of 2^20 points into the chunk's hand-off, and
    // the colour kernel once over the chunk.  With NEDDF_FIELD_CHUNK_LOG2 set, both kernels take launches of that size as before.
    p.ddf_sub = (in.use3 && !env) ? ((int64_t)1 << 20) : ((int64_t)1 << 25);
    const int64_t cap = in.full ? ((int64_t)1 << 19) : ((int64_t)1 << (env ? env : 23));
    int64_t chunk = in.N < cap ? in.N : cap;
    // The hand-off of one launch (features + per-point record: 1 088 B per point eval-minimal at width 256, 9.1 GB at 2^23 points,
    // twice that at engine width 512) is bounded by what the DEVICE has free, not by a constant: several contexts or ranks on one
    // device, or a part with less HBM, get smaller launches (-0.8 .. -2.8 % each halving, profiles/r04_launch_size.txt) instead
    // of NEDDF_EHIP -- at most a quarter of the free memory (counting what this context's own blocks give back when they grow).
    const size_t per_point = in.feat_row + in.aux_row;
    // a launch size settled earlier for this row size stands (the probe is a driver call: not on the hot path of every evaluation)
    if (in.cache_row == per_point && in.cache_chunk > 0 && chunk > in.cache_chunk) chunk = in.cache_chunk;
    if (in.feat_cap < (size_t)chunk * in.feat_row || in.aux_cap < (size_t)chunk * in.aux_row) {
        size_t free_b = 0;
        p.probed = true;
        if (probe(free_b)) {
            free_b += in.feat_cap + in.aux_cap;
            const int64_t asked = chunk;
            while (chunk > (1 << 16) && (size_t)chunk * per_point + (size_t)chunk * per_point / 8 > free_b / 4) chunk >>= 1;
            p.cache = chunk < asked;
        }
    }
    p.chunk = chunk;
    return p;
}

// [0, total) in pieces of at most `step`, in order: f(offset, length) -> int, the first non-zero result ends the walk and is returned.
// field_forward walks the chunks of a call with it, and inside each chunk the distance kernel's sub-launches.
template <class F>
inline int each_span(int64_t total, int64_t step, F &&f)
{
    for (int64_t off = 0; off < total; off += step)
        if (int rc = f(off, total - off < step ? total - off : step)) return rc;
    return 0;
}

}  // namespace neddf
