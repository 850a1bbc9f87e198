// neddf_capi.hip -- C ABI of libneddf_hip.so (include/neddf_hip.h), the part around the fields: context, upload of the packed weights,
// workspaces, stage entry points, the fused render_rays orchestration (all launches on the caller's stream, no host
// round trip inside a call), and what evaluates a field or shares the render path's helpers: surface extraction, the occupancy tools
// and sphere tracing.  Weight packing into MFMA fragment order: field_pack.hip (host only); meshes and point geometry: geom_capi.hip;
// the training step: train_capi.hip; multi-GPU: comm_capi.hip.
#include "../../include/neddf_hip.h"
#include "kernels.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <string>
#include <vector>

using namespace neddf;

#include "capi_internal.h"
#include "field_plan.h"

// one stage launch, bracketed by a hipEvent pair while timing is on
#define STAGE(ctx, stream, which, launch) \
    do { tick((ctx), (stream), (which), true); launch; tick((ctx), (stream), (which), false); } while (0)

static char g_err[256] = "no context";

void neddf_comm_release(neddf_ctx *ctx);       // comm_capi.hip

static int sched_flags() { return 2; }       // bit 1: dynamic tile queue (kernels.h DdfArgs::sched_flags)

// ---------------------------------------------------------------------------
// the slot's packed weights were just read by work enqueued on `s`: neddf_set_field waits for exactly this before it repacks
static int mark_use(neddf_ctx *ctx, Field &f, hipStream_t s)
{
    if (!f.last_use) HIPCHK(hipEventCreateWithFlags(&f.last_use, hipEventDisableTiming));
    // one event per slot, shared by every stream that reads it: a stream that takes the event over first waits for the previous
    // holder's mark, so the waits chain and the event always lies behind EVERY earlier reader (two streams reading one slot)
    if (f.last_use_recorded && f.last_use_stream != s) HIPCHK(hipStreamWaitEvent(s, f.last_use, 0));
    HIPCHK(hipEventRecord(f.last_use, s));
    f.last_use_recorded = true;
    f.last_use_stream = s;
    return 0;
}

// marks the slot on every way out of a function that may have launched readers of it (error returns after a chunk included)
struct UseMark {
    neddf_ctx *ctx; Field &f; hipStream_t s;
    ~UseMark() { (void)mark_use(ctx, f, s); }
};

// Eval-minimal NeDDF needs the gradient of one scalar (the distance) only: reverse mode halves the matrix work
// (NEDDF_DDF_REVERSE=0 keeps the forward-mode Jacobian rows, which the penalties of the full mode need anyway)
static bool ddf_reverse(const Field &f, bool full)
{
    static const bool rev_enabled = [] { const char *e = getenv("NEDDF_DDF_REVERSE"); return !e || atoi(e) != 0; }();
    // (all three operand policies gain: fp32 27.5 vs 51.8 ms per 2^21 points, split fp16 12.4 vs 19.9 ms, bf16 6.4 vs 7.4 ms)
    return rev_enabled && !full && (f.d.kind == NEDDF_FIELD_NEDDF || f.d.kind == NEDDF_FIELD_NEUS);
}

// Sample points straight from the rays (the cone moments in the field prologue): the reverse-mode distance
// kernel derives them in its prologue and hands them to the colour kernel in the per-point record; NEDDF_RAYS_IN_FIELD=0 keeps the
// sampling tensors (the A/B partner: tests/test_gpu_parity.py holds both routes bit-identical)
// (read per call, a few times per frame: the bit-identity test flips it inside one process)
// (a rays-sourced launch parks the sample position in the record's gradient slots, kernels.h PA_R_POS: not when the gradient is asked for)
static bool rays_in_field(const Field &f, bool full, bool dgrad)
{
    const char *rif = getenv("NEDDF_RAYS_IN_FIELD");
    return (!rif || atoi(rif) != 0) && ddf_reverse(f, full) && f.d.kind == NEDDF_FIELD_NEDDF && !dgrad;
}

// -DNEDDF_STAMP builds (`make stamp`): the phase stamps of a field kernel.  One device block per argument type -- the distance and the
// colour kernel each have their own -- allocated once and cleared before every launch group ...
#ifdef NEDDF_STAMP
constexpr size_t kStampBytes = ((size_t)kStampBlocks * 8 * kStampSlots * kStampPairTiles + 4 * kStampWgTail) * sizeof(unsigned long long);
#endif
template <class Args>
static int stamp_arm(neddf_ctx *ctx, Args &a, hipStream_t s)
{
#ifdef NEDDF_STAMP
    static unsigned long long *d_stamps = nullptr;
    if (!d_stamps) HIPCHK(hipMalloc((void **)&d_stamps, kStampBytes));
    HIPCHK(hipMemsetAsync(d_stamps, 0, kStampBytes, s));
    a.stamps = d_stamps;
#endif
    return 0;
}

// ... and the LAST launch's stamps written to the path that `env` names (a diagnostic build: synchronising here is fine)
static int stamp_dump(neddf_ctx *ctx, const unsigned long long *d_stamps, const char *env, hipStream_t s)
{
#ifdef NEDDF_STAMP
    if (const char *path = getenv(env)) {
        HIPCHK(hipStreamSynchronize(s));
        std::vector<unsigned long long> h(kStampBytes / sizeof(unsigned long long));
        HIPCHK(hipMemcpy(h.data(), d_stamps, kStampBytes, hipMemcpyDeviceToHost));
        if (FILE *fp = fopen(path, "wb")) { fwrite(h.data(), 1, kStampBytes, fp); fclose(fp); }
    }
#endif
    return 0;
}

// The one place that knows where a launch's pointers start.  `a` holds the whole call: its inputs and outputs at point 0, the hand-off
// buffers at their heads.  The launch of `n` points at point `so` of the chunk at `off` reads and writes the call's arrays at off + so
// and the chunk's hand-off at so -- whether the points come from the rays or from the sampling tensors.
static DdfArgs ddf_at(const DdfArgs &a, int wid, int64_t off, int64_t so, int64_t n)
{
    DdfArgs b = a;
    const int64_t at = off + so;
    b.n_points = n;
    if (a.rays.rd) b.rays.base = a.rays.base + at;
    else { b.pos = a.pos + at * 3; b.dir = a.dir + at * 3; b.var = a.var + at * 3; }
    if (a.features) b.features = a.features + (size_t)so * a.feat_rows * wid;
    b.ptaux = a.ptaux + (size_t)so * kPtAux;
    if (a.distance) b.distance = a.distance + at;
    if (a.density) b.density = a.density + at;
    if (a.aux_grad) b.aux_grad = a.aux_grad + at;
    return b;
}

// the NeRF field: one kernel, one launch over all N points
static int nerf_forward(neddf_ctx *ctx, Field &f, const float *pos, const float *dir, const float *var, int64_t N, float *density, float *color,
                        hipStream_t s)
{
    NerfArgs a = f.nerf;
    fill_enc(a.enc, f);
    a.pos = pos; a.dir = dir; a.var = var; a.n_points = N;
    a.scratch = (float *)ctx->scratch.p;
    DevBuf &tmp = ctx->ptaux;   // NeRF needs no hand-off buffers; reuse ptaux for optional sinks
    if (!density || !color) {
        if (int rc = ensure(ctx, tmp, (size_t)N * 4 * sizeof(float))) return rc;
    }
    a.density = density ? density : (float *)tmp.p;
    a.color = color ? color : (float *)tmp.p + N;
    const int grid_cap = ctx->cus * nerf_wgs_per_cu(f.nerf.width);
    int64_t tiles = (N + nerf_points_per_tile(f.nerf.width) - 1) / nerf_points_per_tile(f.nerf.width);
    STAGE(ctx, s, NEDDF_STAGE_NERF, launch_nerf(a, (int)(tiles < grid_cap ? tiles : grid_cap), s));
    HIPCHK(hipGetLastError());
    return 0;
}

// rays != NULL (neddf_render_rays): the N points are the [B, Se] grid of these rays' evaluated samples (Se = S unless the caller skips
// each ray's last one, which only a rays_in_field() route can); pos / dir / var are then WORKSPACE -- filled by the sampling kernel when
// the route cannot take its points from the rays, untouched when it can (kernels.h RaySrc)
static int field_forward(neddf_ctx *ctx, int slot, const float *pos, const float *dir, const float *var, int64_t N,
                         int out_mode, float *distance, float *density, float *color, float *penalty, float *aux,
                         hipStream_t s, const RaySrc *rays = nullptr, float *dgrad = nullptr, float *normal = nullptr)
{
    if (slot < 0 || slot >= NEDDF_NUM_SLOTS || !ctx->field[slot].valid) return fail(ctx, NEDDF_ENOFIELD, "no field in slot");
    if (N <= 0) return 0;
    Field &f = ctx->field[slot];
    // dgrad / normal [N, 3] (the surface entry points): read back from the per-point record after each distance-trunk launch
    if ((dgrad || normal) && f.d.kind == NEDDF_FIELD_NERF)
        return fail(ctx, NEDDF_EUNSUPPORTED, "a NeRF field has no distance or sdf: no gradient and no normal (nerf.py:107-165)");
    UseMark mark{ ctx, f, s };
    const int dt = f.d.kind == NEDDF_FIELD_NERF ? f.nerf.operands : f.ddf.operands;      // the slot's operand policy (kernels.h DdfArgs::operands)
    const int wid = f.d.kind == NEDDF_FIELD_NERF ? f.nerf.width : f.ddf.width;        // engine width
    // persistent grids: every workgroup slot of the device filled once (all 512 are resident, two per CU: tools/residency_probe.hip)
    const int grid_cap = ctx->cus * nerf_wgs_per_cu(wid);
    const int grid_cap_ddf = ctx->cus * field_wgs_per_cu(dt, wid);
    const int grid_cap_col = ctx->cus * col_wgs_per_cu(dt, wid);
    const int n_parked = f.d.kind == NEDDF_FIELD_NERF ? f.nerf.n_stash : f.ddf.n_stash;      // early partials a kernel may park per workgroup
    if (int rc = ensure(ctx, ctx->scratch, (size_t)(grid_cap > grid_cap_ddf ? grid_cap : grid_cap_ddf) * (n_parked > 1 ? n_parked : 1) * kStashFloatsPerWg * sizeof(float))) return rc;
    auto sample_now = [&]() {       // the sampling tensors after all (a route that reads them)
        STAGE(ctx, s, NEDDF_STAGE_SAMPLING, launch_sampling(rays->rd, rays->ro, rays->view, rays->dists, N / rays->S, rays->S,
                                                              rays->radius, (float *)pos, (float *)dir, (float *)var, s));
    };
    if (f.d.kind == NEDDF_FIELD_NERF) {
        if (rays) sample_now();
        return nerf_forward(ctx, f, pos, dir, var, N, density, color, s);
    }
    // ---- the route ----
    const bool full = (out_mode == NEDDF_OUT_FULL) && penalty && f.d.kind == NEDDF_FIELD_NEDDF;
    const int fr = full ? 4 : 1;
    const bool reverse = ddf_reverse(f, full);
    const bool use_rays = rays && rays_in_field(f, full, dgrad != nullptr);
    if (rays && !use_rays && rays->Se && rays->Se != rays->S)
        return fail(ctx, NEDDF_EINVAL, "field_forward: the sampling tensors hold every sample of a ray (RaySrc::Se)");
    if (rays && !use_rays) sample_now();
    // fp32 products as three-term bf16 splits (f32_products_split3): the reverse-mode kernel and the colour kernel behind it only
    const bool use3 = f.has3 && reverse && f.d.kind == NEDDF_FIELD_NEDDF;
    // NEDDF_X3_L2 (read per call: the A/B runs flip it inside one library): an L2 residency mechanism of the three-term distance
    // kernel (tile_engine.h OpsF32x3L2T) -- `stream` (the default: y' read back non-temporal), `wb` (a write-back every
    // NEDDF_X3_L2_PERIOD tiles of an XCD, default 16), `both`; `0`: the plain kernel.  The sub-launches of the plan stay: `stream` lifts a
    // 2^23-point launch from 61 to 69 % hits, the 2^20-point ones from 77 to 82 %, and is faster with them (docs/lab_notebook.md R11.1)
    int l2_mode = 0, l2_period = 0;
    if (use3) {
        const char *e = getenv("NEDDF_X3_L2");
        l2_mode = !e ? 1 : !strcmp(e, "0") ? 0 : !strcmp(e, "wb") ? 2 : !strcmp(e, "both") ? 3 : 1;
        const char *r = getenv("NEDDF_X3_L2_PERIOD");
        const int v = r && *r ? atoi(r) : 16;
        l2_period = v < 1 ? 1 : (v > 4096 ? 4096 : v);
    }
    // ---- the plan: points per launch of either kernel (field_plan.h has the rules and their reasons) ----
    static const int chunk_env = [] { const char *e = getenv("NEDDF_FIELD_CHUNK_LOG2"); return e && *e ? atoi(e) : 0; }();
    const FieldPlanIn in{ full, use3, N, chunk_env, (size_t)fr * wid * sizeof(float), kPtAux * sizeof(float),
                          ctx->features.cap, ctx->ptaux.cap, ctx->handoff_row, ctx->handoff_chunk };
    const FieldPlan plan = field_plan(in, [](size_t &free_b) { size_t total_b = 0; return hipMemGetInfo(&free_b, &total_b) == hipSuccess; });
    if (plan.cache) { ctx->handoff_row = in.feat_row + in.aux_row; ctx->handoff_chunk = plan.chunk; }
    // ---- the buffers ----
    // activations' element type and planes: fp32 1024 B, bf16 512 B, split bf16 (two planes) 1024 B per row
    if (int rc = ensure(ctx, ctx->features, (size_t)plan.chunk * in.feat_row)) return rc;
    if (int rc = ensure(ctx, ctx->ptaux, (size_t)plan.chunk * in.aux_row)) return rc;
    if (int rc = ensure(ctx, ctx->sched, 2 * kSchedInts * sizeof(int))) return rc;
    DdfArgs a0 = use3 ? f.ddf3 : f.ddf;
    // one scalar's gradient: reverse mode, 64 or 32 points per tile (field_kernels.hip ddf_rev_kernel)
    const int pts = reverse ? ddf_rev_points(dt, wid) : ddf_points_per_tile(dt, wid);
    const int wgs = reverse ? ddf_rev_wgs_per_cu(dt, wid) * ctx->cus : grid_cap_ddf;
    if (reverse)
        if (int rc = ensure(ctx, ctx->rev_scratch, (size_t)wgs * ddf_rev_scratch_floats_per_wg(a0.n_layers, pts, wid) * sizeof(float))) return rc;
    // penalty requested without colour: park colour in the (already consumed) head of ptaux? no -- own sink
    if (full && !color)
        if (int rc = ensure(ctx, ctx->arena, (size_t)plan.chunk * 3 * sizeof(float))) return rc;
    // ---- the whole call's arguments; every launch takes its piece of them (ddf_at) ----
    fill_enc(a0.enc, f);
    a0.pos = pos; a0.dir = dir; a0.var = var;
    if (use_rays) {
        a0.pos = a0.dir = a0.var = nullptr;
        a0.rays = *rays;
        if (!a0.rays.Se) a0.rays.Se = rays->S;
    }
    a0.aux_grad_scale = f.aux_grad_scale;
    a0.scratch = (float *)ctx->scratch.p;
    a0.features = (color || full) ? (float *)ctx->features.p : nullptr;      // no colour kernel follows: no hand-off
    a0.feat_rows = fr;
    a0.ptaux = (float *)ctx->ptaux.p;
    if (reverse) a0.rev_scratch = (float *)ctx->rev_scratch.p;
    a0.distance = distance; a0.density = density; a0.aux_grad = aux;
    a0.sched = (int *)ctx->sched.p;
    a0.sched_flags = sched_flags();
    if (l2_mode) a0.sched_flags |= (l2_mode << kSchedL2ModeShift) | (l2_period << kSchedL2PeriodShift);
    int rc = each_span(N, plan.chunk, [&](int64_t off, int64_t n) -> int {
        if (reverse)
            if (int rc = stamp_arm(ctx, a0, s)) return rc;
        // the distance kernel (one launch per chunk, except for the three-term policy: FieldPlan::ddf_sub), each on a fresh tile queue
        if (int rc = each_span(n, plan.ddf_sub, [&](int64_t so, int64_t n_sub) -> int {
                const DdfArgs b = ddf_at(a0, wid, off, so, n_sub);
                HIPCHK(hipMemsetAsync(b.sched, 0, kSchedInts * sizeof(int), s));
                const int64_t tiles = (n_sub + pts - 1) / pts;
                const int grid = (int)(tiles < wgs ? tiles : wgs);
                if (reverse) STAGE(ctx, s, NEDDF_STAGE_DDF, launch_ddf_rev(b, grid, s));
                else STAGE(ctx, s, NEDDF_STAGE_DDF, launch_ddf(b, grid, s));
                return 0;
            })) return rc;
        if (reverse)
            if (int rc = stamp_dump(ctx, a0.stamps, "NEDDF_STAMP_FILE", s)) return rc;
        const DdfArgs a = ddf_at(a0, wid, off, 0, n);
        if (dgrad || normal)
            launch_surface_gather(a.ptaux, n, f.d.kind == NEDDF_FIELD_NEUS, dgrad ? dgrad + off * 3 : nullptr, normal ? normal + off * 3 : nullptr, s);
        if (!(color || full)) return 0;
        ColArgs c = use3 ? f.col3 : f.col;
        fill_enc(c.enc, f);
        c.pos = a.pos; c.dir = a.dir; c.var = a.var; c.n_points = n;
        c.rays = use_rays ? 1 : 0;
        c.features = a.features; c.feat_rows = fr; c.ptaux = a.ptaux;
        c.distance_range_max = f.distance_range_max;
        c.penalty = full ? penalty + off : nullptr;
        c.color = color ? color + off * 3 : (float *)ctx->arena.p;
        int ppt = col_points_per_tile(full, dt, wid);
        int64_t ctiles = (n + ppt - 1) / ppt;
        c.sched = (int *)ctx->sched.p + kSchedInts;
        c.sched_flags = sched_flags();
        HIPCHK(hipMemsetAsync(c.sched, 0, kSchedInts * sizeof(int), s));
        if (int rc = stamp_arm(ctx, c, s)) return rc;
        STAGE(ctx, s, NEDDF_STAGE_COL, launch_col(c, (int)(ctiles < grid_cap_col ? ctiles : grid_cap_col), full, s));
        return stamp_dump(ctx, c.stamps, "NEDDF_STAMP_FILE_COL", s);       // (tools/stamp_timeline_col.py)
    });
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    return 0;           // (the slot is marked by `mark` on every way out)
}

// ---------------------------------------------------------------------------
extern "C" {

int neddf_abi_version(void) { return NEDDF_ABI_VERSION; }

const char *neddf_last_error(neddf_ctx *ctx) { return ctx ? ctx->err.c_str() : g_err; }

int neddf_create(int device, neddf_ctx **out)
{
    if (!out) return NEDDF_EINVAL;
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || device < 0 || device >= count) {
        snprintf(g_err, sizeof(g_err), "neddf_create: no HIP device %d (%s)", device, hipGetErrorString(e));
        return NEDDF_EHIP;
    }
    neddf_ctx *ctx = new neddf_ctx();
    ctx->device = device;
    DeviceGuard guard_(device);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) ctx->cus = prop.multiProcessorCount;
    if (ctx->cus <= 0) ctx->cus = 256;
    void *p = nullptr;
    if (hipMalloc(&p, 256) != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "neddf_create: hipMalloc failed");
        delete ctx;
        return NEDDF_EHIP;
    }
    (void)hipMemset(p, 0, 256);
    ctx->flags.p = p; ctx->flags.cap = 256;
    *out = ctx;
    return 0;
}

void neddf_destroy(neddf_ctx *ctx)
{
    if (!ctx) return;
    DeviceGuard guard_(ctx->device);
    (void)hipDeviceSynchronize();
    neddf_comm_release(ctx);
    for (auto &f : ctx->field) {
        if (f.blob.p) (void)hipFree(f.blob.p);
        if (f.last_use) (void)hipEventDestroy(f.last_use);
    }
    for (DevBuf *b : workspaces(ctx))
        if (b->p) (void)hipFree(b->base ? b->base : b->p);
    for (auto &e : ctx->events) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    for (auto &e : ctx->pool) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    delete ctx;
}

int neddf_device_cus(neddf_ctx *ctx) { return ctx ? ctx->cus : 0; }

int neddf_debug_check_guards(neddf_ctx *ctx, int64_t *n_bands, int64_t *n_bad_bytes)
{
    if (!ctx) return NEDDF_EINVAL;
    if (n_bands) *n_bands = 0;
    if (n_bad_bytes) *n_bad_bytes = 0;
    if (!guard_mode()) return 0;            // bands exist only under NEDDF_GUARD=1
    DeviceGuard guard_(ctx->device);
    HIPCHK(hipDeviceSynchronize());
    std::vector<GuardBand> bands = ctx->carve_guards;
    for (DevBuf *b : workspaces(ctx))
        if (b->base) {
            bands.push_back(GuardBand{ b->base, kGuardBytes });
            bands.push_back(GuardBand{ (char *)b->p + b->cap, kGuardBytes });
        }
    // NEDDF_GUARD_SELFTEST=1: overwrite one byte of the last band first -- the test of the probe itself
    if (const char *e = getenv("NEDDF_GUARD_SELFTEST")) if (atoi(e) && !bands.empty()) HIPCHK(hipMemset((void *)bands.back().p, 0, 1));
    std::vector<unsigned char> h(kGuardBytes);
    int64_t bad = 0;
    for (const GuardBand &g : bands) {
        HIPCHK(hipMemcpy(h.data(), g.p, g.bytes, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < g.bytes; ++i) bad += h[i] != (unsigned char)kGuardByte;
    }
    if (n_bands) *n_bands = (int64_t)bands.size();
    if (n_bad_bytes) *n_bad_bytes = bad;
    return 0;
}

int neddf_set_field(neddf_ctx *ctx, int slot, const neddf_field_desc *desc, const float *const *W, const float *const *B, int n)
{
    if (!ctx || !desc || !W || !B) return NEDDF_EINVAL;
    if (slot < 0 || slot >= NEDDF_NUM_SLOTS) return fail(ctx, NEDDF_EINVAL, "bad slot");
    DeviceGuard guard_(ctx->device);
    // Hidden widths: any (neddf.py:52-66, nerf.py:34-44, neus.py:80-99 take any); the engine runs them zero-padded to the next
    // multiple of 128, up to 512 (beyond that one 32-row tile no longer fits two workgroups into a CU's LDS).
    // Encoding ranks: the position encoding owns one 64-column block of the tile (2 x roundup(3 E, 4) <= 64, and ten low-pass
    // factors in the argument block) -> E <= 10, the reference's default and the largest frequency (2^9) that still resolves fp32
    // scene coordinates; the direction encoding only has to fit the tile row next to it.
    const int wmax = desc->kind == NEDDF_FIELD_NERF ? desc->layer_width
                                                    : (desc->layer_width > desc->col_layer_width ? desc->layer_width : desc->col_layer_width);
    if (desc->layer_width < 1 || (desc->kind != NEDDF_FIELD_NERF && desc->col_layer_width < 1) || wmax > kMaxWidth)
        return fail(ctx, NEDDF_EUNSUPPORTED, "hidden widths must be in [1, 512]");
    if (desc->kind == NEDDF_FIELD_NERF && desc->layer_width < 2) return fail(ctx, NEDDF_EUNSUPPORTED, "NeRF: layer_width must be at least 2 (the colour head is layer_width // 2 wide)");
    if (desc->embed_pos_rank < 1 || desc->embed_pos_rank > 10 || desc->embed_dir_rank < 1)
        return fail(ctx, NEDDF_EUNSUPPORTED, "embed_pos_rank must be in [1,10] and embed_dir_rank >= 1");
    if (enc_columns(*desc) > kMaxWidth)
        return fail(ctx, NEDDF_EUNSUPPORTED, "embed_dir_rank: the encodings do not fit one tile row of the widest engine (512 columns)");
    if (desc->n_skips < 0 || desc->n_skips > 8) return fail(ctx, NEDDF_EINVAL, "bad n_skips");
    if (desc->activation < 0 || desc->activation > 2 || desc->density_activation < 0 || desc->density_activation > 2)
        return fail(ctx, NEDDF_EINVAL, "bad activation id");
    if (desc->weight_dtype < NEDDF_DTYPE_F32 || desc->weight_dtype > NEDDF_DTYPE_F16) return fail(ctx, NEDDF_EINVAL, "bad weight_dtype");
    // Everything that can refuse the field comes BEFORE the slot is touched (include/neddf_hip.h): the packer's refusals -- it is host
    // arithmetic into a local block -- and the allocation of a larger device block, which is made beside the old one
    PackedField pk;
    if (int rc = pack_field(*desc, W, B, n, pk, ctx->err)) return rc;
    Field &f = ctx->field[slot];
    const size_t bytes = pk.blob.size() * sizeof(float);
    DevBuf grown;
    if (!(f.blob.cap >= bytes && !(guard_mode() && f.blob.cap != ((bytes + 15) & ~(size_t)15))))
        if (int rc = ensure(ctx, grown, bytes)) {
            if (grown.p) (void)hipFree(grown.base ? grown.base : grown.p);
            return rc;
        }
    // the packed weights of this slot are about to be overwritten: wait for the LAST launch that reads them (an event recorded
    // on its stream by field_forward), not for the whole device -- other streams and other slots keep running
    if (f.last_use)
        if (hipError_t e = hipEventSynchronize(f.last_use)) {
            if (grown.p) (void)hipFree(grown.base ? grown.base : grown.p);
            ctx->err = std::string("hipEventSynchronize(f.last_use): ") + hipGetErrorString(e);
            return NEDDF_EHIP;
        }
    // from here on the slot holds no field until the new one is complete (only a failing HIP call can leave it that way)
    f.valid = false;
    f.has3 = false;
    if (grown.p) {
        if (f.blob.p) HIPCHK(hipFree(f.blob.base ? f.blob.base : f.blob.p));
        f.blob = grown;
    }
    f.d = *desc;
    f.aux_grad_scale = 1.1f; f.distance_range_max = 2.0f;
    for (int i = 0; i < 10; ++i) f.lowpass[i] = 1.0f;
    HIPCHK(hipMemcpy(f.blob.p, pk.blob.data(), bytes, hipMemcpyHostToDevice));
    pk.resolve((const float *)f.blob.p);
    f.ddf = pk.ddf; f.col = pk.col; f.nerf = pk.nerf;
    f.ddf3 = pk.ddf3; f.col3 = pk.col3; f.has3 = pk.has3;
    f.valid = true;
    return 0;
}

int neddf_set_iter(neddf_ctx *ctx, int slot, float aux_grad_scale, float distance_range_max, const float *h_lowpass)
{
    if (!ctx) return NEDDF_EINVAL;
    if (slot < 0 || slot >= NEDDF_NUM_SLOTS || !ctx->field[slot].valid) return fail(ctx, NEDDF_ENOFIELD, "no field in slot");
    Field &f = ctx->field[slot];
    f.aux_grad_scale = aux_grad_scale;
    f.distance_range_max = distance_range_max;
    for (int i = 0; i < f.d.embed_pos_rank; ++i) f.lowpass[i] = h_lowpass ? h_lowpass[i] : 1.0f;
    return 0;
}

static CameraArg cam_arg(const neddf_camera *c)
{
    CameraArg a{};
    if (!c) return a;           // NEDDF_UV_RAYS: the copy kernel reads no camera
    memcpy(a.R, c->R, sizeof(a.R)); memcpy(a.T, c->T, sizeof(a.T)); memcpy(a.calib, c->calib, sizeof(a.calib));
    return a;
}

int neddf_raygen(neddf_ctx *ctx, const void *uv, int uv_type, int64_t n, const neddf_camera *cam, float *rd, float *ro, void *stream)
{
    if (!ctx || !uv || !rd || !ro) return NEDDF_EINVAL;
    UvSpec u;
    if (int rc = parse_uv(ctx, uv_type, n, cam, false, &u)) return rc;
    if (!cam && u.elem != NEDDF_UV_RAYS) return NEDDF_EINVAL;
    DeviceGuard guard_(ctx->device);
    STAGE(ctx, (hipStream_t)stream, NEDDF_STAGE_RAYGEN,
          launch_raygen(uv, u.elem, n, cam_arg(u.table.cameras ? nullptr : cam), u.table, rd, ro, (hipStream_t)stream));
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_sample_coarse(neddf_ctx *ctx, const float *U, int64_t n, int S1, float near_, float far_, float *dists, void *stream)
{
    if (!ctx || !U || !dists || S1 < 2) return NEDDF_EINVAL;
    DeviceGuard guard_(ctx->device);
    STAGE(ctx, (hipStream_t)stream, NEDDF_STAGE_SAMPLE_COARSE, launch_sample_coarse(U, n, S1, near_, far_, dists, (hipStream_t)stream));
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_sampling(neddf_ctx *ctx, const float *rd, const float *ro, const float *dists, int64_t n, int S, double radius,
                   float *pos, float *dir, float *var, void *stream)
{
    if (!ctx || !rd || !ro || !dists || !pos || !dir || !var) return NEDDF_EINVAL;
    if (radius >= 0.0 && S < 2) return fail(ctx, NEDDF_EINVAL, "cone sampling needs at least 2 samples");
    DeviceGuard guard_(ctx->device);
    STAGE(ctx, (hipStream_t)stream, NEDDF_STAGE_SAMPLING, launch_sampling(rd, ro, nullptr, dists, n, S, radius, pos, dir, var, (hipStream_t)stream));
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_sampling_view(neddf_ctx *ctx, const float *rd, const float *ro, const float *view, const float *dists, int64_t n, int S,
                        double radius, float *pos, float *dir, float *var, void *stream)
{
    if (!ctx || !rd || !ro || !view || !dists || !pos || !dir || !var) return NEDDF_EINVAL;
    if (radius >= 0.0 && S < 2) return fail(ctx, NEDDF_EINVAL, "cone sampling needs at least 2 samples");
    DeviceGuard guard_(ctx->device);
    STAGE(ctx, (hipStream_t)stream, NEDDF_STAGE_SAMPLING, launch_sampling(rd, ro, view, dists, n, S, radius, pos, dir, var, (hipStream_t)stream));
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_rays_to_ndc(neddf_ctx *ctx, const float *rd, const float *ro, int64_t n, int width, int height, float fx, float fy,
                      float near_plane, float *nd, float *no, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (n <= 0) return 0;
    if (!rd || !ro || !nd || !no || width < 1 || height < 1 || !(fx > 0.f) || !(fy > 0.f)) return fail(ctx, NEDDF_EINVAL, "rays_to_ndc: bad argument");
    DeviceGuard guard_(ctx->device);
    STAGE(ctx, (hipStream_t)stream, NEDDF_STAGE_NDC, launch_ndc(rd, ro, n, (float)width, (float)height, fx, fy, near_plane, nd, no, (hipStream_t)stream));
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_field_forward(neddf_ctx *ctx, int slot, const float *pos, const float *dir, const float *var, int64_t N, int out_mode,
                        float *distance, float *density, float *color, float *penalty, float *aux, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (N <= 0) return 0;
    if (!pos || !dir || !var) return NEDDF_EINVAL;
    DeviceGuard guard_(ctx->device);
    return field_forward(ctx, slot, pos, dir, var, N, out_mode, distance, density, color, penalty, aux, (hipStream_t)stream);
}

int neddf_field_forward_surface(neddf_ctx *ctx, int slot, const float *pos, const float *dir, const float *var, int64_t N, int out_mode,
                                float *distance, float *density, float *color, float *penalty, float *aux, float *dgrad, float *normal,
                                void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (N <= 0) return 0;
    if (!pos || !dir || !var) return NEDDF_EINVAL;
    DeviceGuard guard_(ctx->device);
    if (slot >= 0 && slot < NEDDF_NUM_SLOTS && ctx->field[slot].valid && ctx->field[slot].d.kind == NEDDF_FIELD_NERF)
        return fail(ctx, NEDDF_EUNSUPPORTED, "field_forward_surface: a NeRF field has no distance or sdf, hence no gradient and no normal");
    return field_forward(ctx, slot, pos, dir, var, N, out_mode, distance, density, color, penalty, aux, (hipStream_t)stream, nullptr, dgrad, normal);
}

int neddf_composite_normal(neddf_ctx *ctx, const float *dists, const float *dens, const float *nrm, int64_t n, int S, float *normal,
                           void *stream)
{
    if (!ctx || !dists || !dens || !nrm || !normal || S < 2) return NEDDF_EINVAL;
    DeviceGuard guard_(ctx->device);
    STAGE(ctx, (hipStream_t)stream, NEDDF_STAGE_COMPOSITE, launch_composite_normal(dists, dens, nrm, n, S, normal, (hipStream_t)stream));
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_composite(neddf_ctx *ctx, const float *dists, const float *dens, const float *col, int64_t n, int S, float max_dist,
                    float *w, float *depth, float *color, float *trans, int *nan_flag, void *stream)
{
    if (!ctx || !dists || !dens || !col || !depth || !color || !trans || S < 2) return NEDDF_EINVAL;
    DeviceGuard guard_(ctx->device);
    STAGE(ctx, (hipStream_t)stream, NEDDF_STAGE_COMPOSITE, launch_composite(dists, dens, col, n, S, max_dist, w, depth, color, trans, nan_flag, (hipStream_t)stream));
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_integrate_penalty(neddf_ctx *ctx, const float *dists, const float *pen, int64_t n, int S, float *out, void *stream)
{
    if (!ctx || !dists || !pen || !out) return NEDDF_EINVAL;
    DeviceGuard guard_(ctx->device);
    STAGE(ctx, (hipStream_t)stream, NEDDF_STAGE_PENALTY, launch_integrate_penalty(dists, pen, n, S, out, (hipStream_t)stream));
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_importance_resample(neddf_ctx *ctx, const float *dists, float *weights, const float *U, int64_t n_rays, int n, int nf,
                              int cat, float *out, int64_t *ids, void *stream)
{
    if (!ctx || !dists || !weights || !U || !out || n < 2 || nf < 1) return NEDDF_EINVAL;
    if (n + nf > 8192) return fail(ctx, NEDDF_EUNSUPPORTED, "importance_resample: n + n_fine must be <= 8192");
    DeviceGuard guard_(ctx->device);
    STAGE(ctx, (hipStream_t)stream, NEDDF_STAGE_RESAMPLE, launch_resample(dists, weights, U, n_rays, n, nf, cat, out, ids, (int *)ctx->flags.p + 1, 0, 0, (hipStream_t)stream));
    HIPCHK(hipGetLastError());
    return 0;
}

// carve helper for the render arena
// NEDDF_GUARD=1: a carve ends exactly at its last element and is followed by a poisoned band (capi_internal.h guard_mode)
// p == NULL measures: the same layout function runs once on such a Carver for the byte count (`off`, no memset, no band recorded)
// and once on the block of that size, so what is reserved is what is carved
struct Carver {
    char *p;
    neddf_ctx *ctx = nullptr;       // NULL: no bands between the carves
    hipStream_t s = nullptr;
    size_t off = 0;
    float *take(size_t n_floats)
    {
        float *r = p ? (float *)(p + off) : nullptr;
        size_t used = n_floats * sizeof(float);
        if (guard_mode() && ctx) {
            used = (used + 15) & ~(size_t)15;
            if (p) {
                (void)hipMemsetAsync(p + off + used, kGuardByte, kCarveGuardBytes, s);
                ctx->carve_guards.push_back(GuardBand{ p + off + used, kCarveGuardBytes });
            }
            used += kCarveGuardBytes;
        }
        off += (used + 255) & ~(size_t)255;
        return r;
    }
};

// ---- empty-space skipping: the workspace of one culled render call (carved from the arena, sized for its longest pass) ----
struct OccWork {
    OccGrid grid;
    unsigned char *keep;            // [N]
    int32_t *index;                 // [N]
    int64_t *blk;                   // [occ_blocks(N) + 1]
    float *cpos, *cdir, *cvar;      // [N, 3] each: the kept points
    float *cdens, *ccol, *cnrm;     // [N], [N, 3], [N, 3] (cnrm only with a normal target): their results
};

// ---- the workspace of one render call: described once, here; counted and carved by running this function twice (Carver) ----
struct RenderWork {
    float *rd, *ro;                         // [B, 3] the rays
    float *nd, *no;                         // [B, 3] their NDC map (ndc_rays only)
    float *dc, *df;                         // [B, Sc1] coarse distances (two passes only), [B, S] the last pass's
    float *pos, *dir, *var;                 // [B, S, 3] sampling tensors of one pass
    float *dens, *pen, *col, *nrm;          // [B, S], [B, S], [B, S, 3], [B, S, 3] (nrm only with a normal target): the field's results
    float *wc;                              // [B, Sc1 - 1] coarse weights for the resampling
    float *depth_c, *color_c, *trans_c;     // coarse pixels: only when the caller asked for one of them (render_rays); render_image does not
    float *depth, *color, *trans;           // the pixels of the last pass
    OccWork occ;
    const OccWork *ow;                      // &occ with an occupancy grid, else NULL
};

// Sc1: samples of the coarse pass of a hierarchical call, 0 for a single pass; S: samples of the last (the longest) pass.
// A pointer the caller supplied in `out` replaces the carve.
static void render_layout(Carver &cv, int64_t B, int Sc1, int S, const neddf_render_outputs *out, bool normals, bool ndc,
                          const neddf_occupancy *occ, RenderWork &w)
{
    w = RenderWork{};
    w.rd = cv.take(B * 3); w.ro = cv.take(B * 3);
    if (Sc1) w.dc = out->dists_coarse ? out->dists_coarse : cv.take(B * Sc1);
    w.df = out->dists_fine ? out->dists_fine : cv.take(B * S);
    w.pos = cv.take(B * S * 3); w.dir = cv.take(B * S * 3); w.var = cv.take(B * S * 3);
    w.dens = cv.take(B * S); w.pen = cv.take(B * S); w.col = cv.take(B * S * 3);
    if (Sc1) {
        w.wc = out->weight_coarse ? out->weight_coarse : cv.take(B * (Sc1 - 1));
        const bool coarse_px = out->depth_coarse || out->color_coarse || out->transmittance_coarse || out->fields_penalty_coarse;
        w.depth_c = out->depth_coarse ? out->depth_coarse : (coarse_px ? cv.take(B) : nullptr);
        w.color_c = out->color_coarse ? out->color_coarse : (coarse_px ? cv.take(B * 3) : nullptr);
        w.trans_c = out->transmittance_coarse ? out->transmittance_coarse : (coarse_px ? cv.take(B) : nullptr);
    }
    w.depth = out->depth ? out->depth : cv.take(B);
    w.color = out->color ? out->color : cv.take(B * 3);
    w.trans = out->transmittance ? out->transmittance : cv.take(B);
    if (normals) w.nrm = cv.take(B * S * 3);           // the per-sample normals of one pass
    if (occ) {
        const size_t N = (size_t)B * S;
        OccWork &o = w.occ;
        o.grid.bits = occ->d_bits; o.grid.res = occ->res;
        for (int a = 0; a < 3; ++a) { o.grid.lo[a] = occ->lo[a]; o.grid.inv_cell[a] = occ->inv_cell[a]; }
        o.keep = (unsigned char *)cv.take((N + 3) / 4);
        o.index = (int32_t *)cv.take(N);
        o.blk = (int64_t *)cv.take((size_t)(occ_blocks(N) + 1) * 2);
        o.cpos = cv.take(N * 3); o.cdir = cv.take(N * 3); o.cvar = cv.take(N * 3);
        o.cdens = cv.take(N); o.ccol = cv.take(N * 3);
        if (normals) o.cnrm = cv.take(N * 3);
        w.ow = &w.occ;
    }
    if (ndc) { w.nd = cv.take(B * 3); w.no = cv.take(B * 3); }
}

static bool occ_ok(const neddf_occupancy *occ) { return occ->d_bits && occ->res >= 1 && occ->res <= kOccMaxRes; }

// kept points of keep[0..n) -> compact rows + index; *m = their number (one stream synchronise)
static int occ_compact(neddf_ctx *ctx, const unsigned char *keep, const float *pos, const float *dir, const float *var, int64_t n, int64_t *blk,
                       float *cpos, float *cdir, float *cvar, int32_t *index, int64_t *m, hipStream_t s)
{
    launch_occ_count(keep, n, blk, s);
    launch_occ_gather(keep, pos, dir, var, n, blk, cpos, cdir, cvar, index, s);
    return read_totals(ctx, s, { { m, blk + occ_blocks(n) } });
}

// The field of one culled pass: sampling tensors -> classify -> gather -> field on the kept points -> scatter into zero-filled outputs.
// dens [B, S]; col / nrm [B, S, 3] or NULL.  A culled sample has density 0, colour 0 and normal 0.
static int culled_field(neddf_ctx *ctx, int slot, const RaySrc &rays, int64_t B, int S, float *pos, float *dir, float *var, float *dens, float *col,
                        float *nrm, const OccWork &w, hipStream_t s)
{
    const int64_t N = B * S;
    STAGE(ctx, s, NEDDF_STAGE_SAMPLING, launch_sampling(rays.rd, rays.ro, rays.view, rays.dists, B, S, rays.radius, pos, dir, var, s));
    launch_occ_classify(w.grid, pos, N, w.keep, s);
    int64_t M = 0;
    if (int rc = occ_compact(ctx, w.keep, pos, dir, var, N, w.blk, w.cpos, w.cdir, w.cvar, w.index, &M, s)) return rc;
    ctx->cull_samples += N;
    ctx->cull_kept += M;
    HIPCHK(hipMemsetAsync(dens, 0, (size_t)N * sizeof(float), s));
    if (col) HIPCHK(hipMemsetAsync(col, 0, (size_t)N * 3 * sizeof(float), s));
    if (nrm) HIPCHK(hipMemsetAsync(nrm, 0, (size_t)N * 3 * sizeof(float), s));
    if (M == 0) return 0;           // nothing kept: the field does not run
    if (int rc = field_forward(ctx, slot, w.cpos, w.cdir, w.cvar, M, NEDDF_OUT_MINIMAL, nullptr, w.cdens, col ? w.ccol : nullptr, nullptr, nullptr, s,
                               nullptr, nullptr, nrm ? w.cnrm : nullptr)) return rc;
    launch_occ_scatter(w.index, M, N, w.cdens, col ? w.ccol : nullptr, nrm ? w.cnrm : nullptr, dens, col, nrm, s);
    HIPCHK(hipGetLastError());
    return 0;
}

// one pass of a render call: its rays and distances, the call's workspace, and where this pass's results go (NULL: not asked for)
struct RenderPass {
    const float *rd, *ro, *view;
    const float *dists;             // [B, S]
    int64_t B;
    int S;
    const RenderWork *ws;           // pos / dir / var / dens / col / pen / nrm, and ow: an occupancy grid and its workspace (the culled pass)
    float *w, *depth, *color, *trans, *pen_out;
    float *normal_out;              // [B, 3] (the normal target)
    int *nan_flag;
};

static int render_pass(neddf_ctx *ctx, int slot, const neddf_render_params *rp, const RenderPass &p, hipStream_t s)
{
    const RenderWork &k = *p.ws;
    const int64_t B = p.B;
    const int S = p.S;
    RaySrc rays;
    rays.rd = p.rd; rays.ro = p.ro; rays.view = p.view; rays.dists = p.dists; rays.S = S;
    rays.cone = rp->cone_sampling ? 1 : 0;
    rays.radius = rp->cone_sampling ? rp->ray_radius : -1.0;
    rays.r2 = (float)(rp->ray_radius * rp->ray_radius);          // launch_sampling's own (float)(radius * radius)
    const bool want_pen = p.pen_out && ctx->field[slot].d.kind == NEDDF_FIELD_NEDDF;
    // a pass whose pixels nobody asked for (the coarse pass of render_image: only its resampling weights are consumed) needs the
    // densities only -- the colour trunk is skipped (the reference evaluates and discards it)
    const bool want_col = p.depth || p.color || p.trans || want_pen;
    float *col = want_col ? k.col : nullptr, *nrm = p.normal_out ? k.nrm : nullptr;
    if (k.ow) {
        if (int rc = culled_field(ctx, slot, rays, B, S, k.pos, k.dir, k.var, k.dens, col, nrm, *k.ow, s)) return rc;
        STAGE(ctx, s, NEDDF_STAGE_COMPOSITE, launch_composite(p.dists, k.dens, col, B, S, rp->max_dist, p.w, p.depth, p.color, p.trans, p.nan_flag, s));
        if (nrm) STAGE(ctx, s, NEDDF_STAGE_COMPOSITE, launch_composite_normal(p.dists, k.dens, nrm, B, S, p.normal_out, s));
        return 0;
    }
    // dens / col / nrm are workspaces of the caller (render_rays_body) and the two compositors below are their only
    // readers: of a ray's last sample they read the distance alone, so the field skips it where it takes its points from the rays (RaySrc::Se;
    // the arrays are then [B, S - 1] rows).  The penalty route integrates a per-sample array of its own and keeps all S samples, and so
    // does the sampling-tensor route (NeRF, NeuS, NEDDF_RAYS_IN_FIELD=0, NEDDF_DDF_REVERSE=0) and the culled pass above.
    const int Se = !want_pen && rays_in_field(ctx->field[slot], false, false) ? S - 1 : S;
    rays.Se = Se;
    int rc = field_forward(ctx, slot, k.pos, k.dir, k.var, B * Se, want_pen ? NEDDF_OUT_FULL : NEDDF_OUT_MINIMAL, nullptr, k.dens, col,
                           want_pen ? k.pen : nullptr, nullptr, s, &rays, nullptr, nrm);
    if (rc) return rc;
    STAGE(ctx, s, NEDDF_STAGE_COMPOSITE, launch_composite(p.dists, k.dens, col, B, S, rp->max_dist, p.w, p.depth, p.color, p.trans, p.nan_flag, s, Se));
    if (nrm) STAGE(ctx, s, NEDDF_STAGE_COMPOSITE, launch_composite_normal(p.dists, k.dens, nrm, B, S, p.normal_out, s, Se));
    if (want_pen) STAGE(ctx, s, NEDDF_STAGE_PENALTY, launch_integrate_penalty(p.dists, k.pen, B, S, p.pen_out, s));
    return 0;
}

// what the fused entry points ask of (uv_type, camera): a ray bundle (NEDDF_UV_RAYS) needs no camera and cannot be mapped to NDC,
// and neither can a camera table (NEDDF_UV_CAMERA_TABLE)
static int check_uv(neddf_ctx *ctx, int uv_type, int64_t B, const neddf_camera *cam, const neddf_render_params *rp, UvSpec *u)
{
    if (int rc = parse_uv(ctx, uv_type, B, cam, rp->ndc_rays != 0, u)) return rc;
    if (u->elem != NEDDF_UV_RAYS) return cam ? 0 : NEDDF_EINVAL;
    if (rp->ndc_rays) return fail(ctx, NEDDF_EUNSUPPORTED, "NEDDF_UV_RAYS: the NDC map needs a camera's focal lengths (ndc_rays must be 0)");
    return 0;
}

// What one fused call is, beyond the arguments every entry point shares.  A single-pass call (neddf_render_rays_single*) is the
// hierarchical one that stops after its first pass, which then runs on the caller's slot with S1 samples and writes the final outputs.
struct RenderCall {
    const char *name;               // the prefix of the culled entry points' refusals
    bool two;                       // coarse pass -> importance resampling -> fine pass
    int slot, S1;                   // a single pass: its field and its samples per ray
    const float *Uc, *Uf;           // [B, S] uniforms of the first draw, [B, sample_fine + 1] of the resampling (two passes)
    float *normal, *normal_coarse;  // [B, 3] normal targets or NULL
    const neddf_occupancy *occ;     // an occupancy grid: the culled passes
};

static int render_rays_body(neddf_ctx *ctx, const RenderCall &c, const void *uv, int uv_type, int64_t B, const neddf_camera *cam,
                            const neddf_render_params *rp, const neddf_render_outputs *out, void *stream)
{
    const neddf_occupancy *occ = c.occ;
    if (!ctx) return NEDDF_EINVAL;
    if (B <= 0) return 0;           // empty batch: nothing to do (pointers of empty tensors may be NULL)
    if (!uv || !rp || !c.Uc || !out || (c.two ? !c.Uf : c.S1 < 2)) return NEDDF_EINVAL;
    UvSpec u;
    if (int rc = check_uv(ctx, uv_type, B, cam, rp, &u)) return rc;
    auto refuse = [&](int code, const char *why, const char *more = "") { return fail(ctx, code, std::string(c.name) + why + more); };
    if (occ && !occ_ok(occ)) return refuse(NEDDF_EINVAL, ": the grid needs its bits and a resolution in [1, 1024]");
    if (occ && (out->fields_penalty || (c.two && out->fields_penalty_coarse)))
        return refuse(NEDDF_EUNSUPPORTED, ": no fields_penalty output with an occupancy grid (a culled sample has no penalty)");
    DeviceGuard guard_(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    // samples per ray of the first pass, of the resampling, of the last pass
    const int Sc1 = c.two ? rp->sample_coarse + 1 : c.S1, Sf1 = rp->sample_fine + 1, S = c.two ? Sc1 + Sf1 : c.S1;
    if (c.two) {
        if (!ctx->field[NEDDF_SLOT_COARSE].valid || !ctx->field[NEDDF_SLOT_FINE].valid) return fail(ctx, NEDDF_ENOFIELD, "render_rays needs coarse and fine fields");
    } else if (c.slot < 0 || c.slot >= NEDDF_NUM_SLOTS || !ctx->field[c.slot].valid) return fail(ctx, NEDDF_ENOFIELD, "no field in slot");
    if (occ && B * S >= ((int64_t)1 << 31))
        return refuse(NEDDF_EUNSUPPORTED, c.two ? ": 2^31 samples or more in one pass" : ": 2^31 samples or more", " (compaction indices are int32)");
    // the workspace: measured, reserved, carved -- all by render_layout
    // (the arena is also used by field_forward as a colour sink only when colour is not requested; never the case here)
    RenderWork w;
    auto layout = [&](Carver cv) { render_layout(cv, B, c.two ? Sc1 : 0, S, out, c.normal || c.normal_coarse, rp->ndc_rays != 0, occ, w); return cv.off; };
    if (int rc = ensure(ctx, ctx->arena, layout(Carver{ nullptr, ctx, s }))) return rc;
    ctx->carve_guards.clear();
    layout(Carver{ (char *)ctx->arena.p, ctx, s });
    int *nan_flag = out->nan_flag ? out->nan_flag : (int *)ctx->flags.p;

    STAGE(ctx, s, NEDDF_STAGE_RAYGEN, launch_raygen(uv, u.elem, B, cam_arg(u.table.cameras ? nullptr : cam), u.table, w.rd, w.ro, s));
    float *d1 = c.two ? w.dc : w.df;        // the first draw
    RenderPass p{ w.rd, w.ro, nullptr, d1, B, Sc1, &w };
    if (rp->ndc_rays) {         // positions follow the NDC ray, the field keeps the world-space viewing direction
        STAGE(ctx, s, NEDDF_STAGE_NDC, launch_ndc(w.rd, w.ro, B, (float)rp->ndc_width, (float)rp->ndc_height, cam->calib[0], cam->calib[1], rp->ndc_near, w.nd, w.no, s));
        p.view = w.rd; p.rd = w.nd; p.ro = w.no;
    }
    p.nan_flag = nan_flag;
    STAGE(ctx, s, NEDDF_STAGE_SAMPLE_COARSE, launch_sample_coarse(c.Uc, B, Sc1, rp->dist_near, rp->dist_far, d1, s));
    if (c.two) {
        p.w = w.wc; p.depth = w.depth_c; p.color = w.color_c; p.trans = w.trans_c;
        p.pen_out = out->fields_penalty_coarse; p.normal_out = c.normal_coarse;
        if (int rc = render_pass(ctx, NEDDF_SLOT_COARSE, rp, p, s)) return rc;
        // the reference takes the NaN-fallback decision of sample_pdf per render_rays call, i.e. per `chunk` rays of render_image
        const int64_t group = rp->nan_group > 0 ? rp->nan_group : B;
        const int64_t goff = rp->nan_group > 0 && rp->nan_group_offset > 0 ? rp->nan_group_offset % group : 0;
        if (int rc = ensure(ctx, ctx->rflags, (size_t)((B + goff + group - 1) / group) * sizeof(int))) return rc;
        STAGE(ctx, s, NEDDF_STAGE_RESAMPLE, launch_resample(w.dc, w.wc, c.Uf, B, Sc1, Sf1, 1, w.df, nullptr, (int *)ctx->rflags.p, group, goff, s));
        p.dists = w.df; p.S = S;
    }
    p.w = out->weight; p.depth = w.depth; p.color = w.color; p.trans = w.trans;
    p.pen_out = out->fields_penalty; p.normal_out = c.normal;
    if (int rc = render_pass(ctx, c.two ? NEDDF_SLOT_FINE : c.slot, rp, p, s)) return rc;
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_render_rays(neddf_ctx *ctx, const void *uv, int uv_type, int64_t B, const neddf_camera *cam, const neddf_render_params *rp,
                      const float *Uc, const float *Uf, const neddf_render_outputs *out, void *stream)
{
    return render_rays_body(ctx, { "render_rays_culled", true, 0, 0, Uc, Uf, nullptr, nullptr, nullptr }, uv, uv_type, B, cam, rp, out, stream);
}

int neddf_render_rays_surface(neddf_ctx *ctx, const void *uv, int uv_type, int64_t B, const neddf_camera *cam, const neddf_render_params *rp,
                              const float *Uc, const float *Uf, const neddf_render_outputs *out, float *normal, float *normal_coarse,
                              void *stream)
{
    return render_rays_body(ctx, { "render_rays_culled", true, 0, 0, Uc, Uf, normal, normal_coarse, nullptr }, uv, uv_type, B, cam, rp, out, stream);
}

int neddf_render_rays_single(neddf_ctx *ctx, int slot, const void *uv, int uv_type, int64_t B, const neddf_camera *cam,
                             const neddf_render_params *rp, int S1, const float *U, const neddf_render_outputs *out, void *stream)
{
    return render_rays_body(ctx, { "render_rays_single_culled", false, slot, S1, U, nullptr, nullptr, nullptr, nullptr }, uv, uv_type, B, cam, rp, out, stream);
}

int neddf_render_rays_single_surface(neddf_ctx *ctx, int slot, const void *uv, int uv_type, int64_t B, const neddf_camera *cam,
                                     const neddf_render_params *rp, int S1, const float *U, const neddf_render_outputs *out, float *normal,
                                     void *stream)
{
    return render_rays_body(ctx, { "render_rays_single_culled", false, slot, S1, U, nullptr, normal, nullptr, nullptr }, uv, uv_type, B, cam, rp, out, stream);
}

int neddf_op_activation(neddf_ctx *ctx, int op, const float *x, const float *J, int64_t N, int C, float *y, float *G, void *stream)
{
    if (!ctx || !x || !y || op < 0 || op > 4 || (J && !G)) return NEDDF_EINVAL;
    if (!J && op > 2) return fail(ctx, NEDDF_EINVAL, "softplus/sigmoid exist only as (value, Jacobian) ops in the reference");
    if (J && op == 4 && C != 1) return fail(ctx, NEDDF_EUNSUPPORTED, "SigmoidGradFunction is defined for one channel (sigmoid.py:42)");
    launch_op_activation(op, x, J, N, C, y, G, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_op_positional_encoding(neddf_ctx *ctx, const float *x, const float *J, const float *scale, int64_t N, int E, float *y,
                                 float *G, void *stream)
{
    if (!ctx || !x || !y || E < 1 || E > 30 || (J && !G)) return NEDDF_EINVAL;
    launch_op_pe(x, J, scale, N, E, y, G, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_op_pe_weights(neddf_ctx *ctx, const float *var, int64_t N, int E, float *w, void *stream)
{
    if (!ctx || !var || !w || E < 1 || E > 30) return NEDDF_EINVAL;
    launch_op_pe_weights(var, N, E, w, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_op_linear_grad(neddf_ctx *ctx, const float *x, const float *J, const float *W, const float *b, int64_t N, int Cin,
                         int Cout, float *y, float *G, void *stream)
{
    if (!ctx || !x || !J || !W || !y || !G) return NEDDF_EINVAL;
    if (Cin < 1 || Cout < 1 || Cin > 65536 || Cout > 65536) return fail(ctx, NEDDF_EINVAL, "op_linear_grad: bad Cin / Cout");
    if (N <= 0) return 0;
    DeviceGuard guard_(ctx->device);
    // any (Cin, Cout) (with_grad/linear.py:87-133 takes any): the product is cut into K blocks of <= 256 input columns (accumulated in
    // the outputs) and N blocks of 256 / 128 output columns (a last partial block runs zero-padded and stores only its valid columns)
    hipStream_t s = (hipStream_t)stream;
    const int64_t tiles = (N + 31) / 32;
    const int grid = (int)(tiles < ctx->cus ? tiles : ctx->cus);
    for (int n0 = 0; n0 < Cout; n0 += 256) {
        const int nvalid = Cout - n0 < 256 ? Cout - n0 : 256, nblk = nvalid > 128 ? 256 : 128;
        for (int k0 = 0; k0 < Cin; k0 += 256) {
            const int kc = Cin - k0 < 256 ? Cin - k0 : 256;
            std::vector<float> blob;
            std::vector<int> km;
            for (int k = 0; k < roundup(kc, 8); ++k) km.push_back(k < kc ? k0 + k : -1);
            // the block's weights [kc, nblk]: columns n0 .. n0 + nvalid of W (row stride Cout), zero beyond
            std::vector<float> wblk((size_t)Cin * nblk, 0.f);              // (W and b are HOST arrays, include/neddf_hip.h)
            for (int k = k0; k < k0 + kc; ++k)
                for (int n = 0; n < nvalid; ++n) wblk[(size_t)k * nblk + n] = W[(size_t)k * Cout + n0 + n];
            Src src{ wblk.data(), Cin, nblk, false };
            size_t o_w = pack_layer(blob, src, km, nblk, 0, nullptr);
            std::vector<float> bv(nblk, 0.f);
            if (b && k0 == 0) memcpy(bv.data(), b + n0, (size_t)nvalid * sizeof(float));
            size_t o_b = put(blob, bv.data(), nblk);
            if (int rc = ensure(ctx, ctx->features, blob.size() * sizeof(float))) return rc;
            HIPCHK(hipStreamSynchronize(s));                  // the previous block's launch is done with the buffer; blob is a host temporary
            HIPCHK(hipMemcpyAsync(ctx->features.p, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice, s));
            HIPCHK(hipStreamSynchronize(s));
            const float *base = (const float *)ctx->features.p;
            launch_linear_grad(x + k0, J + k0, N, kc, Cin, nblk, (int)km.size() / 8, base + o_w, base + o_b, y + n0, G + n0, Cout, nvalid, k0 > 0, grid, s);
        }
    }
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_set_timing(neddf_ctx *ctx, int enable)
{
    if (!ctx) return NEDDF_EINVAL;
    ctx->timing = enable != 0;
    return 0;
}

static int drain_events(neddf_ctx *ctx, float *ms, int *launches)
{
    for (auto &e : ctx->events) {
        HIPCHK(hipEventSynchronize(e.b));
        float t = 0.f;
        HIPCHK(hipEventElapsedTime(&t, e.a, e.b));
        ms[e.which] += t;
        launches[e.which] += 1;
        ctx->pool.push_back(e);
    }
    ctx->events.clear();
    return 0;
}

int neddf_get_timings(neddf_ctx *ctx, float *ms, int n)
{
    if (!ctx || !ms || n < 6) return NEDDF_EINVAL;
    DeviceGuard guard_(ctx->device);
    float t[NEDDF_STAGE_COUNT] = { 0 };
    int c[NEDDF_STAGE_COUNT] = { 0 };
    for (int i = 0; i < n; ++i) ms[i] = 0.f;
    if (int rc = drain_events(ctx, t, c)) return rc;
    for (int k = 0; k < 3; ++k) { ms[k] = t[k]; ms[3 + k] = (float)c[k]; }      // distance trunk, colour trunk, NeRF field
    return 0;
}

int neddf_get_stage_timings(neddf_ctx *ctx, float *ms, int *launches, int n_stages)
{
    if (!ctx || !ms || !launches || n_stages < NEDDF_STAGE_COUNT) return NEDDF_EINVAL;
    DeviceGuard guard_(ctx->device);
    for (int i = 0; i < n_stages; ++i) { ms[i] = 0.f; launches[i] = 0; }
    return drain_events(ctx, ms, launches);
}

// ---- surface extraction (no reference counterpart inside the library: fields_visualizer.py:528-566 meshes on the host) ----
static bool lattice_ok(int nx, int ny, int nz, const double *lo, const double *hi)
{
    if (nx < 2 || ny < 2 || nz < 2) return false;
    for (int a = 0; a < 3; ++a)
        if (!(lo[a] < hi[a])) return false;      // NaN bounds fail too
    return true;
}

static McGrid mc_grid(const float *vol, int nx, int ny, int nz, const double *lo, const double *hi, float iso)
{
    McGrid g{};
    g.vol = vol; g.nx = nx; g.ny = ny; g.nz = nz;
    g.n = (int64_t)nx * ny * nz;
    g.iso = iso;
    for (int a = 0; a < 3; ++a) { g.lo[a] = lo[a]; g.hi[a] = hi[a]; }
    return g;
}

static int grid_field_ok(neddf_ctx *ctx, int slot, int field, const char *what)
{
    if (field != NEDDF_GRID_DISTANCE && field != NEDDF_GRID_DENSITY)
        return fail(ctx, NEDDF_EINVAL, std::string(what) + ": field must be NEDDF_GRID_DISTANCE or NEDDF_GRID_DENSITY");
    if (slot < 0 || slot >= NEDDF_NUM_SLOTS || !ctx->field[slot].valid) return fail(ctx, NEDDF_ENOFIELD, "no field in slot");
    if (field == NEDDF_GRID_DISTANCE && ctx->field[slot].d.kind == NEDDF_FIELD_NERF)
        return fail(ctx, NEDDF_EINVAL, std::string(what) + ": a NeRF field has no distance output");
    return 0;
}

// `total` generated points through the field in chunks: points(first, n, pos, dir, var) fills a chunk, after(first, n, out) runs behind
// its evaluation.  One chunk = one launch of field_forward at its own launch size (2^23 points): 302 MB of pos / dir / var
static int eval_generated(neddf_ctx *ctx, int slot, int field, int64_t total, float *d_out, hipStream_t s,
                          const std::function<void(int64_t, int64_t, float *, float *, float *)> &points,
                          const std::function<void(int64_t, int64_t, float *)> &after)
{
    const int64_t chunk = total < ((int64_t)1 << 23) ? total : ((int64_t)1 << 23);
    if (int rc = ensure(ctx, ctx->grid_pts, (size_t)chunk * 9 * sizeof(float))) return rc;
    float *pos = (float *)ctx->grid_pts.p, *dir = pos + chunk * 3, *var = dir + chunk * 3;
    for (int64_t off = 0; off < total; off += chunk) {
        const int64_t n = total - off < chunk ? total - off : chunk;
        points(off, n, pos, dir, var);
        HIPCHK(hipGetLastError());
        float *out = d_out + off;
        // no colour: the colour kernel and its hand-off are skipped (field_forward, a.features)
        if (int rc = field_forward(ctx, slot, pos, dir, var, n, NEDDF_OUT_MINIMAL, field == NEDDF_GRID_DISTANCE ? out : nullptr,
                                   field == NEDDF_GRID_DENSITY ? out : nullptr, nullptr, nullptr, nullptr, s)) return rc;
        after(off, n, out);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

int neddf_field_grid(neddf_ctx *ctx, int slot, int field, int nx, int ny, int nz, const double *h_lo, const double *h_hi, float *d_volume,
                     void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (!h_lo || !h_hi || !d_volume) return fail(ctx, NEDDF_EINVAL, "field_grid: NULL bounds or volume");
    if (!lattice_ok(nx, ny, nz, h_lo, h_hi)) return fail(ctx, NEDDF_EINVAL, "field_grid: every dimension must be >= 2 and lo < hi on every axis");
    if (int rc = grid_field_ok(ctx, slot, field, "field_grid")) return rc;
    DeviceGuard guard_(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    const McGrid g = mc_grid(nullptr, nx, ny, nz, h_lo, h_hi, 0.f);
    return eval_generated(ctx, slot, field, g.n, d_volume, s,
                          [&](int64_t first, int64_t n, float *pos, float *dir, float *var) { launch_grid_points(g, first, n, pos, dir, var, s); },
                          [](int64_t, int64_t, float *) {});
}

int neddf_marching_cubes(neddf_ctx *ctx, const float *d_volume, int nx, int ny, int nz, const double *h_lo, const double *h_hi, float iso,
                         float *d_vertices, int64_t vertex_cap, int32_t *d_triangles, int64_t triangle_cap, int64_t *h_n_vertices,
                         int64_t *h_n_triangles, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (!d_volume || !h_lo || !h_hi || !h_n_vertices || !h_n_triangles) return fail(ctx, NEDDF_EINVAL, "marching_cubes: NULL volume, bounds or count");
    if (!lattice_ok(nx, ny, nz, h_lo, h_hi)) return fail(ctx, NEDDF_EINVAL, "marching_cubes: every dimension must be >= 2 and lo < hi on every axis");
    DeviceGuard guard_(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    const McGrid g = mc_grid(d_volume, nx, ny, nz, h_lo, h_hi, iso);
    const int64_t nb = mc_blocks(g.n);
    if (nb > 0x7fffffff) return fail(ctx, NEDDF_EUNSUPPORTED, "marching_cubes: lattice too large");
    if (int rc = ensure(ctx, ctx->mc_mask, (size_t)g.n)) return rc;
    if (int rc = ensure(ctx, ctx->mc_blk, (size_t)2 * (nb + 1) * sizeof(int64_t))) return rc;
    unsigned char *mask = (unsigned char *)ctx->mc_mask.p;
    int64_t *vblk = (int64_t *)ctx->mc_blk.p, *tblk = vblk + nb + 1;
    launch_mc_count(g, mask, vblk, tblk, s);
    launch_scan_totals(vblk, nb, s);
    launch_scan_totals(tblk, nb, s);
    int64_t counts[2];
    if (int rc = read_totals(ctx, s, { { &counts[0], vblk + nb }, { &counts[1], tblk + nb } })) return rc;
    *h_n_vertices = counts[0];
    *h_n_triangles = counts[1];
    if (counts[0] >= ((int64_t)1 << 31)) return fail(ctx, NEDDF_EUNSUPPORTED, "marching_cubes: 2^31 vertices or more (triangle indices are int32)");
    if (!d_vertices || !d_triangles || vertex_cap < counts[0] || triangle_cap < counts[1]) return 0;     // the counting call
    if (int rc = ensure(ctx, ctx->mc_vbase, (size_t)g.n * sizeof(int32_t))) return rc;
    int32_t *vbase = (int32_t *)ctx->mc_vbase.p;
    launch_mc_vertices(g, mask, vblk, vbase, d_vertices, s);
    launch_mc_triangles(g, mask, tblk, vbase, d_triangles, s);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- brick-wise surface extraction ----
static bool brick_ok(int brick) { return brick >= kBrickMin && brick <= kBrickMax; }

static BrickGrid brick_grid(int nx, int ny, int nz, int brick, const double *lo, const double *hi, float iso)
{
    BrickGrid bg{};
    bg.g = mc_grid(nullptr, nx, ny, nz, lo, hi, iso);
    bg.B = brick;
    bg.P = (brick + 1) * (brick + 1) * (brick + 1);
    bg.nbx = (nx - 2 + brick) / brick; bg.nby = (ny - 2 + brick) / brick; bg.nbz = (nz - 2 + brick) / brick;
    bg.nb = (int64_t)bg.nbx * bg.nby * bg.nbz;
    return bg;
}

int neddf_field_grid_coarse(neddf_ctx *ctx, int slot, int field, int nx, int ny, int nz, int brick, const double *h_lo, const double *h_hi,
                            float *d_coarse, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (!h_lo || !h_hi || !d_coarse) return fail(ctx, NEDDF_EINVAL, "field_grid_coarse: NULL bounds or volume");
    if (!lattice_ok(nx, ny, nz, h_lo, h_hi)) return fail(ctx, NEDDF_EINVAL, "field_grid_coarse: every dimension must be >= 2 and lo < hi on every axis");
    if (!brick_ok(brick)) return fail(ctx, NEDDF_EINVAL, "field_grid_coarse: the brick size must lie in [2, 16]");
    if (int rc = grid_field_ok(ctx, slot, field, "field_grid_coarse")) return rc;
    DeviceGuard guard_(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    const BrickGrid bg = brick_grid(nx, ny, nz, brick, h_lo, h_hi, 0.f);
    const int64_t total = (int64_t)(bg.nbx + 1) * (bg.nby + 1) * (bg.nbz + 1);
    return eval_generated(ctx, slot, field, total, d_coarse, s,
                          [&](int64_t first, int64_t n, float *pos, float *dir, float *var) { launch_coarse_points(bg, first, n, pos, dir, var, s); },
                          [](int64_t, int64_t, float *) {});
}

int neddf_brick_select(neddf_ctx *ctx, const float *d_coarse, int nbx, int nby, int nbz, float iso, float band, int dilate, int32_t *d_slot_map,
                       int32_t *d_brick_ids, int64_t *h_n_active, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (!d_coarse || !d_slot_map || !d_brick_ids || !h_n_active) return fail(ctx, NEDDF_EINVAL, "brick_select: NULL volume, slot map, list or count");
    if (nbx < 1 || nby < 1 || nbz < 1) return fail(ctx, NEDDF_EINVAL, "brick_select: every axis needs at least one brick");
    if (!(band >= 0.f)) return fail(ctx, NEDDF_EINVAL, "brick_select: the band must not be negative");
    if (dilate < 0 || dilate > kBrickMaxDilate) return fail(ctx, NEDDF_EINVAL, "brick_select: dilate must lie in [0, 4]");
    const int64_t nb = (int64_t)nbx * nby * nbz, blocks = mc_blocks(nb);
    if (nb >= ((int64_t)1 << 31)) return fail(ctx, NEDDF_EUNSUPPORTED, "brick_select: 2^31 bricks or more (brick indices are int32)");
    DeviceGuard guard_(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = ensure(ctx, ctx->brick_flags, (size_t)2 * nb)) return rc;
    if (int rc = ensure(ctx, ctx->brick_blk, (size_t)(blocks + 1) * sizeof(int64_t))) return rc;
    unsigned char *flags = (unsigned char *)ctx->brick_flags.p;
    int64_t *blk = (int64_t *)ctx->brick_blk.p;
    launch_brick_select(d_coarse, nbx, nby, nbz, iso, band, dilate, flags, flags + nb, blk, d_slot_map, d_brick_ids, s);
    return read_totals(ctx, s, { { h_n_active, blk + blocks } });
}

int neddf_field_bricks(neddf_ctx *ctx, int slot, int field, int nx, int ny, int nz, int brick, const double *h_lo, const double *h_hi,
                       const int32_t *d_brick_ids, int64_t n_bricks, float *d_values, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (!h_lo || !h_hi) return fail(ctx, NEDDF_EINVAL, "field_bricks: NULL bounds");
    if (!lattice_ok(nx, ny, nz, h_lo, h_hi)) return fail(ctx, NEDDF_EINVAL, "field_bricks: every dimension must be >= 2 and lo < hi on every axis");
    if (!brick_ok(brick)) return fail(ctx, NEDDF_EINVAL, "field_bricks: the brick size must lie in [2, 16]");
    const BrickGrid bg = brick_grid(nx, ny, nz, brick, h_lo, h_hi, 0.f);
    if (n_bricks < 0 || n_bricks > bg.nb) return fail(ctx, NEDDF_EINVAL, "field_bricks: the number of bricks must lie in [0, the bricks of the grid]");
    if (bg.nb >= ((int64_t)1 << 31)) return fail(ctx, NEDDF_EUNSUPPORTED, "field_bricks: 2^31 bricks or more (brick indices are int32)");
    if (n_bricks > 0 && (!d_brick_ids || !d_values)) return fail(ctx, NEDDF_EINVAL, "field_bricks: NULL brick list or values");
    if (int rc = grid_field_ok(ctx, slot, field, "field_bricks")) return rc;
    if (n_bricks == 0) return 0;
    DeviceGuard guard_(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    return eval_generated(ctx, slot, field, n_bricks * bg.P, d_values, s,
                          [&](int64_t first, int64_t n, float *pos, float *dir, float *var) { launch_brick_points(bg, d_brick_ids, first, n, pos, dir, var, s); },
                          [&](int64_t first, int64_t n, float *out) { launch_brick_pad(bg, d_brick_ids, first, n, out, s); });
}

int neddf_marching_cubes_bricks(neddf_ctx *ctx, const float *d_values, const int32_t *d_brick_ids, int64_t n_bricks, const int32_t *d_slot_map,
                                int nx, int ny, int nz, int brick, const double *h_lo, const double *h_hi, float iso, float *d_vertices,
                                int64_t vertex_cap, int32_t *d_triangles, int64_t triangle_cap, int64_t *d_vertex_key, int64_t *d_triangle_key,
                                int64_t *h_n_vertices, int64_t *h_n_triangles, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (!d_slot_map || !h_lo || !h_hi || !h_n_vertices || !h_n_triangles) return fail(ctx, NEDDF_EINVAL, "marching_cubes_bricks: NULL slot map, bounds or count");
    if (!lattice_ok(nx, ny, nz, h_lo, h_hi)) return fail(ctx, NEDDF_EINVAL, "marching_cubes_bricks: every dimension must be >= 2 and lo < hi on every axis");
    if (!brick_ok(brick)) return fail(ctx, NEDDF_EINVAL, "marching_cubes_bricks: the brick size must lie in [2, 16]");
    BrickMesh k{};
    k.bg = brick_grid(nx, ny, nz, brick, h_lo, h_hi, iso);
    k.values = d_values; k.ids = d_brick_ids; k.slot_map = d_slot_map; k.M = n_bricks;
    const int64_t M = n_bricks;
    if (M < 0 || M > k.bg.nb) return fail(ctx, NEDDF_EINVAL, "marching_cubes_bricks: the number of bricks must lie in [0, the bricks of the grid]");
    if (k.bg.nb >= ((int64_t)1 << 31)) return fail(ctx, NEDDF_EUNSUPPORTED, "marching_cubes_bricks: 2^31 bricks or more (brick indices are int32)");
    if (M > 0 && (!d_values || !d_brick_ids)) return fail(ctx, NEDDF_EINVAL, "marching_cubes_bricks: NULL values or brick list");
    DeviceGuard guard_(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    // block totals of both kinds (each with its grand total behind it), then the word the list / slot-map check raises
    if (int rc = ensure(ctx, ctx->brick_blk, (size_t)2 * (M + 1) * sizeof(int64_t) + sizeof(int))) return rc;
    if (int rc = ensure(ctx, ctx->brick_mask, (size_t)(M > 0 ? M * k.bg.P : 1))) return rc;
    unsigned char *mask = (unsigned char *)ctx->brick_mask.p;
    int64_t *vblk = (int64_t *)ctx->brick_blk.p, *tblk = vblk + M + 1;
    int *bad = (int *)(tblk + M + 1);
    HIPCHK(hipMemsetAsync(bad, 0, sizeof(int), s));
    launch_brick_check(k, bad, s);
    if (M > 0) launch_brick_mc_count(k, mask, vblk, tblk, s);
    launch_scan_totals(vblk, M, s);
    launch_scan_totals(tblk, M, s);
    int64_t counts[2];
    int h_bad = 0;
    if (int rc = read_totals(ctx, s, { { &counts[0], vblk + M }, { &counts[1], tblk + M } }, &h_bad, bad)) return rc;
    if (h_bad) return fail(ctx, NEDDF_EINVAL, "marching_cubes_bricks: the brick list must be strictly ascending inside the grid and the slot map its inverse");
    *h_n_vertices = counts[0];
    *h_n_triangles = counts[1];
    if (counts[0] >= ((int64_t)1 << 31)) return fail(ctx, NEDDF_EUNSUPPORTED, "marching_cubes_bricks: 2^31 vertices or more (triangle indices are int32)");
    if (!d_vertices || !d_triangles || !d_vertex_key || !d_triangle_key || vertex_cap < counts[0] || triangle_cap < counts[1]) return 0;     // the counting call
    if (M == 0) return 0;
    if (int rc = ensure(ctx, ctx->brick_vbase, (size_t)M * k.bg.P * sizeof(int32_t))) return rc;
    int32_t *vbase = (int32_t *)ctx->brick_vbase.p;
    launch_brick_mc_vertices(k, mask, vblk, vbase, d_vertices, d_vertex_key, s);
    launch_brick_mc_triangles(k, mask, tblk, vbase, d_triangles, d_triangle_key, s);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- empty-space skipping (occupancy_kernels.hip) ----
int neddf_render_rays_culled(neddf_ctx *ctx, const void *uv, int uv_type, int64_t B, const neddf_camera *cam, const neddf_render_params *rp,
                             const float *Uc, const float *Uf, const neddf_render_outputs *out, float *normal, float *normal_coarse,
                             void *stream, const neddf_occupancy *occ)
{
    return render_rays_body(ctx, { "render_rays_culled", true, 0, 0, Uc, Uf, normal, normal_coarse, occ }, uv, uv_type, B, cam, rp, out, stream);
}

int neddf_render_rays_single_culled(neddf_ctx *ctx, int slot, const void *uv, int uv_type, int64_t B, const neddf_camera *cam,
                                    const neddf_render_params *rp, int S1, const float *U, const neddf_render_outputs *out, float *normal,
                                    void *stream, const neddf_occupancy *occ)
{
    return render_rays_body(ctx, { "render_rays_single_culled", false, slot, S1, U, nullptr, normal, nullptr, occ }, uv, uv_type, B, cam, rp, out, stream);
}

int neddf_cull_stats(neddf_ctx *ctx, int64_t *h_samples, int64_t *h_kept, int reset)
{
    if (!ctx) return NEDDF_EINVAL;
    if (h_samples) *h_samples = ctx->cull_samples;
    if (h_kept) *h_kept = ctx->cull_kept;
    if (reset) ctx->cull_samples = ctx->cull_kept = 0;
    return 0;
}

int neddf_occupancy_build(neddf_ctx *ctx, const float *d_volume, int R, float threshold, int dilate, uint32_t *d_bits, int64_t *h_n_occupied,
                          void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (!d_volume || !d_bits || !h_n_occupied) return fail(ctx, NEDDF_EINVAL, "occupancy_build: NULL volume, bits or count");
    if (R < 1 || R > kOccMaxRes) return fail(ctx, NEDDF_EINVAL, "occupancy_build: the resolution must be in [1, 1024]");
    if (dilate < 0 || dilate > kOccMaxDilate) return fail(ctx, NEDDF_EINVAL, "occupancy_build: dilate must be in [0, 4]");
    DeviceGuard guard_(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_cells = (int64_t)R * R * R, nb = mc_blocks(occ_words(R));
    if (int rc = ensure(ctx, ctx->occ_cells, (size_t)2 * n_cells)) return rc;
    if (int rc = ensure(ctx, ctx->occ_blk, (size_t)(nb + 1) * sizeof(int64_t))) return rc;
    unsigned char *cells = (unsigned char *)ctx->occ_cells.p;
    int64_t *blk = (int64_t *)ctx->occ_blk.p;
    launch_occ_build(d_volume, R, threshold, dilate, cells, cells + n_cells, d_bits, blk, s);
    return read_totals(ctx, s, { { h_n_occupied, blk + nb } });
}

int neddf_occupancy_classify(neddf_ctx *ctx, const neddf_occupancy *occ, const float *d_pos, int64_t n_points, unsigned char *d_keep,
                             void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (!occ || !occ_ok(occ)) return fail(ctx, NEDDF_EINVAL, "occupancy_classify: the grid needs its bits and a resolution in [1, 1024]");
    if (n_points < 0) return fail(ctx, NEDDF_EINVAL, "occupancy_classify: negative count");
    if (n_points == 0) return 0;
    if (!d_pos || !d_keep) return fail(ctx, NEDDF_EINVAL, "occupancy_classify: NULL points or keep bytes");
    if (mc_blocks(n_points) > 0x7fffffff) return fail(ctx, NEDDF_EUNSUPPORTED, "occupancy_classify: too many points for one launch");
    DeviceGuard guard_(ctx->device);
    OccGrid g{};
    g.bits = occ->d_bits; g.res = occ->res;
    for (int a = 0; a < 3; ++a) { g.lo[a] = occ->lo[a]; g.inv_cell[a] = occ->inv_cell[a]; }
    launch_occ_classify(g, d_pos, n_points, d_keep, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_occupancy_gather(neddf_ctx *ctx, const unsigned char *d_keep, const float *d_pos, const float *d_dir, const float *d_var,
                           int64_t n_points, float *d_out_pos, float *d_out_dir, float *d_out_var, int32_t *d_index, int64_t *h_n_kept,
                           void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (!h_n_kept || n_points < 0) return fail(ctx, NEDDF_EINVAL, "occupancy_gather: NULL count or negative size");
    *h_n_kept = 0;
    if (n_points == 0) return 0;
    if (!d_keep || !d_pos || !d_dir || !d_var || !d_out_pos || !d_out_dir || !d_out_var || !d_index)
        return fail(ctx, NEDDF_EINVAL, "occupancy_gather: NULL keep bytes, rows, outputs or index");
    if (n_points >= ((int64_t)1 << 31)) return fail(ctx, NEDDF_EUNSUPPORTED, "occupancy_gather: 2^31 points or more (indices are int32)");
    DeviceGuard guard_(ctx->device);
    if (int rc = ensure(ctx, ctx->occ_blk, (size_t)(occ_blocks(n_points) + 1) * sizeof(int64_t))) return rc;
    return occ_compact(ctx, d_keep, d_pos, d_dir, d_var, n_points, (int64_t *)ctx->occ_blk.p, d_out_pos, d_out_dir, d_out_var, d_index, h_n_kept,
                       (hipStream_t)stream);
}

int neddf_occupancy_scatter(neddf_ctx *ctx, const int32_t *d_index, int64_t n_kept, int64_t n_points, const float *d_c_density,
                            const float *d_c_color, const float *d_c_normal, float *d_density, float *d_color, float *d_normal, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (n_kept < 0 || n_points < n_kept) return fail(ctx, NEDDF_EINVAL, "occupancy_scatter: 0 <= n_kept <= n_points expected");
    if ((n_kept > 0 && !d_index) || (!d_c_density != !d_density) || (!d_c_color != !d_color) || (!d_c_normal != !d_normal))
        return fail(ctx, NEDDF_EINVAL, "occupancy_scatter: NULL index, or an output without its source");
    if (n_points >= ((int64_t)1 << 31)) return fail(ctx, NEDDF_EUNSUPPORTED, "occupancy_scatter: 2^31 points or more (indices are int32)");
    DeviceGuard guard_(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    if (d_density && n_points) HIPCHK(hipMemsetAsync(d_density, 0, (size_t)n_points * sizeof(float), s));
    if (d_color && n_points) HIPCHK(hipMemsetAsync(d_color, 0, (size_t)n_points * 3 * sizeof(float), s));
    if (d_normal && n_points) HIPCHK(hipMemsetAsync(d_normal, 0, (size_t)n_points * 3 * sizeof(float), s));
    launch_occ_scatter(d_index, n_kept, n_points, d_c_density, d_c_color, d_c_normal, d_density, d_color, d_normal, s);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- sphere tracing (trace_kernels.hip) ----
static TraceState trace_state(const float *t, const float *t_lo, const unsigned char *status, const int32_t *steps, const float *dist)
{
    return TraceState{ (float *)t, (float *)t_lo, (float *)dist, (unsigned char *)status, (int32_t *)steps };
}

static int trace_count_ok(neddf_ctx *ctx, int64_t n, const char *what)
{
    if (n < 0) return fail(ctx, NEDDF_EINVAL, std::string(what) + ": negative count");
    if (n >= ((int64_t)1 << 31)) return fail(ctx, NEDDF_EUNSUPPORTED, std::string(what) + ": 2^31 rays or more (indices are int32)");
    return 0;
}

// selected rays -> index + points; *m = their number (one stream synchronise)
static int trace_compact(neddf_ctx *ctx, const float *ro, const float *rd, int64_t n, const TraceState &st, int bisect, int32_t *index, float *pos,
                         int64_t *m, hipStream_t s)
{
    *m = 0;
    if (n == 0) return 0;
    if (int rc = ensure(ctx, ctx->trace_blk, (size_t)(occ_blocks(n) + 1) * sizeof(int64_t))) return rc;
    int64_t *blk = (int64_t *)ctx->trace_blk.p;
    launch_trace_compact(ro, rd, n, st, bisect, blk, index, pos, s);
    return read_totals(ctx, s, { { m, blk + occ_blocks(n) } });
}

int neddf_trace_begin(neddf_ctx *ctx, const float *d_ray_orig, const float *d_ray_dir, int64_t n_rays, float t_near, float *d_t, float *d_t_lo,
                      unsigned char *d_status, int32_t *d_steps, float *d_dist, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (int rc = trace_count_ok(ctx, n_rays, "trace_begin")) return rc;
    if (n_rays == 0) return 0;
    if (!d_ray_orig || !d_ray_dir || !d_t || !d_t_lo || !d_status || !d_steps || !d_dist) return fail(ctx, NEDDF_EINVAL, "trace_begin: NULL rays or state");
    DeviceGuard guard_(ctx->device);
    launch_trace_begin(d_ray_orig, d_ray_dir, n_rays, t_near, trace_state(d_t, d_t_lo, d_status, d_steps, d_dist), (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_trace_compact(neddf_ctx *ctx, const float *d_ray_orig, const float *d_ray_dir, int64_t n_rays, const float *d_t,
                        const unsigned char *d_status, int32_t *d_index, float *d_pos, int64_t *h_n_active, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (!h_n_active) return fail(ctx, NEDDF_EINVAL, "trace_compact: NULL count");
    if (int rc = trace_count_ok(ctx, n_rays, "trace_compact")) return rc;
    *h_n_active = 0;
    if (n_rays == 0) return 0;
    if (!d_ray_orig || !d_ray_dir || !d_t || !d_status || !d_index || !d_pos) return fail(ctx, NEDDF_EINVAL, "trace_compact: NULL rays, state or outputs");
    DeviceGuard guard_(ctx->device);
    return trace_compact(ctx, d_ray_orig, d_ray_dir, n_rays, trace_state(d_t, nullptr, d_status, nullptr, nullptr), 0, d_index, d_pos, h_n_active,
                         (hipStream_t)stream);
}

int neddf_trace_advance(neddf_ctx *ctx, const int32_t *d_index, const float *d_distance, int64_t n_active, int64_t n_rays, float threshold,
                        float step_scale, float min_step, float t_far, float *d_t, float *d_t_lo, unsigned char *d_status, int32_t *d_steps,
                        float *d_dist, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (int rc = trace_count_ok(ctx, n_rays, "trace_advance")) return rc;
    if (n_active < 0 || n_active > n_rays) return fail(ctx, NEDDF_EINVAL, "trace_advance: 0 <= n_active <= n_rays expected");
    if (n_active == 0) return 0;
    if (!d_index || !d_distance || !d_t || !d_t_lo || !d_status || !d_steps || !d_dist) return fail(ctx, NEDDF_EINVAL, "trace_advance: NULL index, distances or state");
    DeviceGuard guard_(ctx->device);
    launch_trace_advance(d_index, d_distance, n_active, n_rays, threshold, step_scale, min_step, t_far,
                         trace_state(d_t, d_t_lo, d_status, d_steps, d_dist), (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_trace_finish(neddf_ctx *ctx, unsigned char *d_status, int64_t n_rays, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (int rc = trace_count_ok(ctx, n_rays, "trace_finish")) return rc;
    if (n_rays == 0) return 0;
    if (!d_status) return fail(ctx, NEDDF_EINVAL, "trace_finish: NULL status");
    DeviceGuard guard_(ctx->device);
    launch_trace_finish(d_status, n_rays, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_trace_bisect_points(neddf_ctx *ctx, const float *d_ray_orig, const float *d_ray_dir, int64_t n_rays, const float *d_t, const float *d_t_lo,
                              const unsigned char *d_status, int32_t *d_index, float *d_pos, int64_t *h_n_points, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (!h_n_points) return fail(ctx, NEDDF_EINVAL, "trace_bisect_points: NULL count");
    if (int rc = trace_count_ok(ctx, n_rays, "trace_bisect_points")) return rc;
    *h_n_points = 0;
    if (n_rays == 0) return 0;
    if (!d_ray_orig || !d_ray_dir || !d_t || !d_t_lo || !d_status || !d_index || !d_pos)
        return fail(ctx, NEDDF_EINVAL, "trace_bisect_points: NULL rays, state or outputs");
    DeviceGuard guard_(ctx->device);
    return trace_compact(ctx, d_ray_orig, d_ray_dir, n_rays, trace_state(d_t, d_t_lo, d_status, nullptr, nullptr), 1, d_index, d_pos, h_n_points,
                         (hipStream_t)stream);
}

int neddf_trace_bisect_update(neddf_ctx *ctx, const int32_t *d_index, const float *d_distance, int64_t n_points, int64_t n_rays, float threshold,
                              float *d_t, float *d_t_lo, float *d_dist, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (int rc = trace_count_ok(ctx, n_rays, "trace_bisect_update")) return rc;
    if (n_points < 0 || n_points > n_rays) return fail(ctx, NEDDF_EINVAL, "trace_bisect_update: 0 <= n_points <= n_rays expected");
    if (n_points == 0) return 0;
    if (!d_index || !d_distance || !d_t || !d_t_lo || !d_dist) return fail(ctx, NEDDF_EINVAL, "trace_bisect_update: NULL index, distances or state");
    DeviceGuard guard_(ctx->device);
    launch_trace_bisect_update(d_index, d_distance, n_points, n_rays, threshold, trace_state(d_t, d_t_lo, nullptr, nullptr, d_dist), (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_trace_field(neddf_ctx *ctx, int slot, const float *d_ray_orig, const float *d_ray_dir, int64_t n_rays, const neddf_trace_params *p,
                      float *d_t, float *d_t_lo, unsigned char *d_status, int32_t *d_steps, float *d_dist, int64_t *h_evaluations, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (!p) return fail(ctx, NEDDF_EINVAL, "trace_field: NULL parameters");
    if (int rc = trace_count_ok(ctx, n_rays, "trace_field")) return rc;
    if (!(p->t_near < p->t_far)) return fail(ctx, NEDDF_EINVAL, "trace_field: t_near < t_far expected");
    if (!(p->step_scale > 0.f && p->step_scale <= 1.f)) return fail(ctx, NEDDF_EINVAL, "trace_field: step_scale must lie in (0, 1]");
    if (!(p->min_step > 0.f)) return fail(ctx, NEDDF_EINVAL, "trace_field: min_step must be positive");
    if (p->max_steps < 1 || p->max_steps > 4096) return fail(ctx, NEDDF_EINVAL, "trace_field: max_steps must lie in [1, 4096]");
    if (p->refine < 0 || p->refine > 32) return fail(ctx, NEDDF_EINVAL, "trace_field: refine must lie in [0, 32]");
    if (slot < 0 || slot >= NEDDF_NUM_SLOTS || !ctx->field[slot].valid) return fail(ctx, NEDDF_ENOFIELD, "no field in slot");
    if (ctx->field[slot].d.kind == NEDDF_FIELD_NERF) return fail(ctx, NEDDF_EUNSUPPORTED, "trace_field: a NeRF field has no distance to trace");
    if (h_evaluations) *h_evaluations = 0;
    if (n_rays == 0) return 0;
    if (!d_ray_orig || !d_ray_dir || !d_t || !d_t_lo || !d_status || !d_steps || !d_dist) return fail(ctx, NEDDF_EINVAL, "trace_field: NULL rays or state");
    DeviceGuard guard_(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    // workspace: index [n], points [n, 3], distances [n], and dir / var of one field chunk (at most 2^23 points, the field kernels' launch size)
    const int64_t chunk = n_rays < ((int64_t)1 << 23) ? n_rays : ((int64_t)1 << 23);
    int32_t *index;
    float *D, *pos, *dir, *var;
    auto layout = [&](Carver cv) {                  // (no bands between the carves: the block's own two stand at its ends)
        index = (int32_t *)cv.take((size_t)n_rays);
        D = cv.take((size_t)n_rays); pos = cv.take((size_t)n_rays * 3); dir = cv.take((size_t)chunk * 3); var = cv.take((size_t)chunk * 3);
        return cv.off;
    };
    if (int rc = ensure(ctx, ctx->trace_ws, layout(Carver{ nullptr }))) return rc;
    layout(Carver{ (char *)ctx->trace_ws.p });
    launch_trace_unit_inputs(dir, var, chunk, s);
    const TraceState st = trace_state(d_t, d_t_lo, d_status, d_steps, d_dist);
    launch_trace_begin(d_ray_orig, d_ray_dir, n_rays, p->t_near, st, s);
    HIPCHK(hipGetLastError());
    int64_t evaluations = 0;
    auto distances = [&](int64_t M) -> int {        // the field on the M compacted points, distance output only: no colour kernel runs
        for (int64_t off = 0; off < M; off += chunk) {
            const int64_t n = M - off < chunk ? M - off : chunk;
            if (int rc = field_forward(ctx, slot, pos + off * 3, dir, var, n, NEDDF_OUT_MINIMAL, D + off, nullptr, nullptr, nullptr, nullptr, s)) return rc;
        }
        evaluations += M;
        return 0;
    };
    for (int it = 0; it < p->max_steps; ++it) {
        int64_t M = 0;
        if (int rc = trace_compact(ctx, d_ray_orig, d_ray_dir, n_rays, st, 0, index, pos, &M, s)) return rc;
        if (M == 0) break;
        if (int rc = distances(M)) return rc;
        launch_trace_advance(index, D, M, n_rays, p->threshold, p->step_scale, p->min_step, p->t_far, st, s);
    }
    launch_trace_finish(d_status, n_rays, s);
    for (int round = 0; round < p->refine; ++round) {
        int64_t M = 0;
        if (int rc = trace_compact(ctx, d_ray_orig, d_ray_dir, n_rays, st, 1, index, pos, &M, s)) return rc;
        if (M == 0) break;
        if (int rc = distances(M)) return rc;
        launch_trace_bisect_update(index, D, M, n_rays, p->threshold, st, s);
    }
    HIPCHK(hipGetLastError());
    if (h_evaluations) *h_evaluations = evaluations;
    return 0;
}

}  // extern "C"
