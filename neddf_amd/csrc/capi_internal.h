// capi_internal.h -- context layout and helpers shared by the C-ABI translation units (neddf_capi.hip: context, fields, render, surface
// extraction, occupancy, tracing; geom_capi.hip: meshes and point geometry; train_capi.hip: training step; comm_capi.hip: multi-GPU).
// The host-only weight packer has its own header, field_pack.h (included here for roundup / in_skips).  Not installed.
#pragma once
#include "../../include/neddf_hip.h"
#include "kernels.h"
#include "field_pack.h"

#include <stdlib.h>
#include <initializer_list>
#include <string>
#include <vector>

using namespace neddf;

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    void *base = nullptr;       // NEDDF_GUARD=1: the allocation starts one guard band in front of p
};

// NEDDF_GUARD=1 (a debug mode, tests/test_gpu_multi.py::test_workspace_guard_bands): every workspace of a context is allocated at its
// EXACT requested size between two poisoned guard bands, every carve of the render arena is followed by one, and
// neddf_debug_check_guards() counts the band bytes a kernel has overwritten -- the bounds probe that stands in for a GPU-side
// AddressSanitizer run (ROCm's ASan runtime does not start beside an uninstrumented python on this image, tools/asan_probe.sh).
constexpr size_t kGuardBytes = 4096, kCarveGuardBytes = 256;
constexpr int kGuardByte = 0xA5;
static inline bool guard_mode()
{
    static const bool on = [] { const char *e = getenv("NEDDF_GUARD"); return e && atoi(e) != 0; }();
    return on;
}
struct GuardBand { const void *p; size_t bytes; };

struct Field {
    bool valid = false;
    neddf_field_desc d{};
    float aux_grad_scale = 1.1f, distance_range_max = 2.0f;
    float lowpass[10];
    DevBuf blob;
    hipEvent_t last_use = nullptr;       // recorded after the last launch that reads `blob` (neddf_set_field waits on it)
    bool last_use_recorded = false;      // ... and the stream that recorded it last: another stream waits for it before re-recording
    hipStream_t last_use_stream = nullptr;
    DdfArgs ddf{};
    ColArgs col{};
    NerfArgs nerf{};
    // NeDDF in fp32: the same network with three-term bf16 products (operands 3), taken by the eval-minimal route's reverse-mode
    // distance kernel and colour kernel (NEDDF_F32_PRODUCTS, field_pack.hip)
    bool has3 = false;
    DdfArgs ddf3{};
    ColArgs col3{};
};

struct EventPair {
    hipEvent_t a, b;
    int which;                   // NEDDF_STAGE_*
};

// Multi-GPU state of a context (comm_capi.hip): one RCCL communicator, a communication stream of its own and the event
// pair that orders it against the caller's compute stream.
struct CommState {
    void *comm = nullptr;        // ncclComm_t
    int rank = 0, nranks = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ready = nullptr;  // recorded on the compute stream: the local slab is complete
    hipEvent_t done = nullptr;   // recorded on the communication stream: the gathered pixels are complete
    bool pending = false;
    bool lost = false;           // the communicator was aborted with a gather in flight: the next wait reports it
    DevBuf pad;                  // [nranks * pad_rows * channels] staging for ragged slabs
    bool in_place = false;       // ragged slabs by one grouped set of broadcasts instead of the padded staging route: decided ONCE
                                 // at neddf_comm_init from every rank's own capability / NEDDF_GATHER_INPLACE (all ranks must agree)
    bool force_ragged = false;   // NEDDF_GATHER_FORCE_RAGGED=1 (test hook): equal slabs take the ragged route too
};

// Every entry point that launches or allocates runs on the ctx's device and leaves the caller's current device as it
// found it (a torch process may have another device current).
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

struct neddf_ctx {
    int device = 0;
    int cus = 256;
    std::string err;
    Field field[NEDDF_NUM_SLOTS];
    DevBuf features, ptaux, scratch, arena, flags, sched;
    int64_t handoff_chunk = 0;   // field_forward: launch size last settled for a hand-off of `handoff_row` bytes per point (0: none yet) --
    size_t handoff_row = 0;      // the free-memory probe runs when the hand-off would have to GROW, not on every call
    DevBuf rflags;               // importance resampling: one NaN-fallback flag per group of rays
    DevBuf rev_scratch;          // reverse-mode distance kernel: per-workgroup y' of every layer + encoding Jacobian
    DevBuf tpack, ttmp;          // training step: packed weights of the layer in flight, gradient ping-pong buffers
    DevBuf tamax;                // training step: max |dZ| of every gradient matrix of a backward pass (split-fp16 operand range)
    DevBuf grid_pts;             // neddf_field_grid: pos / dir / var of one chunk of the lattice
    DevBuf mc_mask, mc_vbase, mc_blk;         // neddf_marching_cubes: crossed-edge byte and first vertex id per lattice point, block bases
    DevBuf mc_nacc;              // neddf_mesh_vertex_normals: 64-bit fixed-point sums [3 V] + the scale word
    DevBuf cc_parent, cc_used, cc_blk;        // neddf_mesh_components / neddf_mesh_compact: parent (or new index) and used byte per vertex,
                                              // block totals followed by the "changed" words of one batch of rounds.  Borrowed by
                                              // neddf_mesh_simplify_clusters (run starts [V + 1], head byte per vertex, the block totals of
                                              // its two scans) and neddf_mesh_simplify_pairs (cc_blk alone)
    int cc_rounds = 0;           // union-find rounds of the last neddf_mesh_components call
    DevBuf occ_cells, occ_blk;   // neddf_occupancy_build: two byte planes of R^3 cells; block totals of build / gather
    DevBuf brick_flags, brick_blk;            // neddf_brick_select: two byte planes of one flag per brick, block totals
    DevBuf brick_mask, brick_vbase;           // neddf_marching_cubes_bricks: owned crossed edges and first vertex id per brick lattice point
    DevBuf trace_blk, trace_ws;  // sphere tracing: block totals of the compactions; neddf_trace_field's index / points / distances / constant inputs
    DevBuf geom_blk, geom_ws;    // geom_capi.hip, one call at a time.  geom_blk: the block totals of neddf_mesh_sample_*, neddf_nn_grid_build and
                                 // neddf_raycast_grid_count / _build.  geom_ws: the cell of every target and the count of every cell
                                 // (neddf_nn_grid_build), the pairs of every list (neddf_raycast_grid_*), the per-triangle table
                                 // [kPmTableFloats T] (neddf_point_mesh_grid_query / _bvh_query), parents and counters (neddf_bvh_build)
    int64_t cull_samples = 0, cull_kept = 0;  // neddf_cull_stats: samples classified / kept by the culled render passes
    std::vector<GuardBand> carve_guards;      // NEDDF_GUARD=1: the bands behind the carves of the last render call
    bool timing = false;
    std::vector<EventPair> events;
    std::vector<EventPair> pool;
    CommState comm;
};

// Every DevBuf of a context (the fields' blobs and the communicator's staging aside): what neddf_destroy frees and the bounds probe
// checks.  A workspace added to neddf_ctx joins this list.
static inline std::vector<DevBuf *> workspaces(neddf_ctx *ctx)
{
    return { &ctx->features, &ctx->ptaux, &ctx->scratch, &ctx->arena, &ctx->flags, &ctx->rflags, &ctx->rev_scratch, &ctx->sched, &ctx->tpack, &ctx->ttmp,
             &ctx->tamax, &ctx->grid_pts, &ctx->mc_mask, &ctx->mc_vbase, &ctx->mc_blk, &ctx->mc_nacc, &ctx->cc_parent, &ctx->cc_used, &ctx->cc_blk,
             &ctx->occ_cells, &ctx->occ_blk, &ctx->brick_flags, &ctx->brick_blk, &ctx->brick_mask, &ctx->brick_vbase, &ctx->trace_blk, &ctx->trace_ws,
             &ctx->geom_blk, &ctx->geom_ws };
}

// hipEvent pair around one stage launch (only while neddf_set_timing is on); `which` = NEDDF_STAGE_*
static inline void tick(neddf_ctx *ctx, hipStream_t s, int which, bool begin)
{
    if (!ctx->timing) return;
    if (begin) {
        EventPair e;
        if (!ctx->pool.empty()) { e = ctx->pool.back(); ctx->pool.pop_back(); }
        else { (void)hipEventCreate(&e.a); (void)hipEventCreate(&e.b); }
        e.which = which;
        (void)hipEventRecord(e.a, s);
        ctx->events.push_back(e);
    } else {
        (void)hipEventRecord(ctx->events.back().b, s);
    }
}

#define HIPCHK(call)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);                     \
            return NEDDF_EHIP;                                                                \
        }                                                                                     \
    } while (0)

static inline int fail(neddf_ctx *ctx, int code, const std::string &msg)
{
    ctx->err = msg;
    return code;
}

// uv_type as the ray-generating calls take it (neddf_raygen, the six neddf_render_rays*, neddf_raygen_backward): an element type
// 0..4, and under NEDDF_UV_CAMERA_TABLE (element types 0..3 only) h_cam is a HOST neddf_camera_table naming a camera per row.
// Everything is checked here, before the caller writes anything.
struct UvSpec {
    int elem;                       // NEDDF_UV_F32 .. NEDDF_UV_RAYS
    neddf::CameraTableArg table;    // cameras == nullptr: no table
};
static inline int parse_uv(neddf_ctx *ctx, int uv_type, int64_t n, const neddf_camera *cam, bool ndc, UvSpec *u)
{
    u->elem = uv_type & ~(int)NEDDF_UV_CAMERA_TABLE;
    u->table = neddf::CameraTableArg{ nullptr, nullptr, 0 };
    if (uv_type < 0 || u->elem > NEDDF_UV_RAYS) return fail(ctx, NEDDF_EINVAL, "bad uv_type");
    if (!(uv_type & NEDDF_UV_CAMERA_TABLE)) return 0;
    if (u->elem == NEDDF_UV_RAYS) return fail(ctx, NEDDF_EINVAL, "bad uv_type: NEDDF_UV_CAMERA_TABLE goes with the pixel types, a ray bundle has no camera");
    if (!cam) return fail(ctx, NEDDF_EINVAL, "NEDDF_UV_CAMERA_TABLE: h_cam must point to a neddf_camera_table");
    const neddf_camera_table *t = (const neddf_camera_table *)cam;
    if (t->n_cameras < 1 || t->n_cameras > (1 << 20)) return fail(ctx, NEDDF_EINVAL, "NEDDF_UV_CAMERA_TABLE: n_cameras must be in 1 .. 2^20");
    if (n > 0 && (!t->d_cameras || !t->d_view)) return fail(ctx, NEDDF_EINVAL, "NEDDF_UV_CAMERA_TABLE: d_cameras and d_view must not be NULL");
    if (ndc) return fail(ctx, NEDDF_EUNSUPPORTED, "NEDDF_UV_CAMERA_TABLE: the NDC map takes one camera's focal lengths (ndc_rays must be 0)");
    u->table = neddf::CameraTableArg{ (const float *)t->d_cameras, t->d_view, t->n_cameras };
    return 0;
}

static inline int ensure(neddf_ctx *ctx, DevBuf &b, size_t bytes)
{
    if (b.cap >= bytes && !(guard_mode() && b.cap != ((bytes + 15) & ~(size_t)15))) return 0;
    if (b.p) {
        HIPCHK(hipDeviceSynchronize());      // nothing in flight may still use the old block
        HIPCHK(hipFree(b.base ? b.base : b.p));
        b.p = nullptr; b.cap = 0; b.base = nullptr;
        if (&b == &ctx->arena) ctx->carve_guards.clear();      // the bands behind the last render's carves lived in the freed block
    }
    if (guard_mode()) {         // exact size (rounded to 16 B) between two poisoned bands: one element past either end lands in a band
        const size_t want = (bytes + 15) & ~(size_t)15;
        HIPCHK(hipMalloc(&b.base, want + 2 * kGuardBytes));
        HIPCHK(hipMemset(b.base, kGuardByte, kGuardBytes));
        HIPCHK(hipMemset((char *)b.base + kGuardBytes + want, kGuardByte, kGuardBytes));
        b.p = (char *)b.base + kGuardBytes;
        b.cap = want;
        return 0;
    }
    size_t want = bytes + bytes / 8;
    HIPCHK(hipMalloc(&b.p, want));
    b.cap = want;
    return 0;
}

// The end of every count -> scan pass: the launches before are checked, the grand totals (8 bytes each, behind their block bases; at
// most three) and an optional flag word come back on the stream, then ONE synchronise.
struct TotalRead { int64_t *host; const int64_t *dev; };
static inline int read_totals(neddf_ctx *ctx, hipStream_t s, std::initializer_list<TotalRead> totals, int *h_flag = nullptr, const int *d_flag = nullptr)
{
    HIPCHK(hipGetLastError());
    for (const TotalRead &t : totals) HIPCHK(hipMemcpyAsync(t.host, t.dev, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    if (h_flag) HIPCHK(hipMemcpyAsync(h_flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

static inline void fill_enc(EncodeDesc &e, const Field &f)
{
    e.E = f.d.embed_pos_rank; e.Ed = f.d.embed_dir_rank;
    e.KH = roundup(3 * e.E, 4); e.KD = roundup(3 * e.Ed, 4);
    for (int i = 0; i < 10; ++i) e.lowpass[i] = f.lowpass[i];
}
