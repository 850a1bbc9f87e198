// geom_capi.hip -- C ABI of the mesh and point-geometry entry points (include/neddf_hip.h): vertex normals, connected components and
// compaction, surface sampling, nearest neighbours, ray casting, point-to-mesh distance through the grid and the BVH, the BVH build, rays
// through the BVH and mesh simplification.  What belongs here takes no field slot and never touches a Field, the render arena, stage timing or occupancy
// state: argument checks, workspaces of the context and launches on the caller's stream.
#include "capi_internal.h"

#include <math.h>

#include <algorithm>

extern "C" {

// ---- the argument checks the entry points share (every one before the first HIP call) ----
// n points and, for the entry points with two sets of them (queries and targets), n2 more
static int point_counts_ok(neddf_ctx *ctx, const char *what, int64_t n, const float *p, int64_t n2 = 0, const float *p2 = nullptr)
{
    if (n < 0 || n2 < 0) return fail(ctx, NEDDF_EINVAL, std::string(what) + ": negative count");
    if ((n > 0 && !p) || (n2 > 0 && !p2)) return fail(ctx, NEDDF_EINVAL, std::string(what) + ": NULL points");
    if (n >= ((int64_t)1 << 31) || n2 >= ((int64_t)1 << 31)) return fail(ctx, NEDDF_EUNSUPPORTED, std::string(what) + ": 2^31 points or more (indices are int32)");
    return 0;
}

// V vertices and T triangles and, for the entry points that have them, n rays or query points (have_points: every array of them is
// there).  The words are the ray casts'; the point-to-mesh and BVH entry points say the same of their queries and of a mesh alone.
static int mesh_counts_ok(neddf_ctx *ctx, int64_t V, const float *v, int64_t T, const int32_t *tri, const char *what, int64_t n = 0, bool have_points = true)
{
    if (n < 0 || V < 0 || T < 0) return fail(ctx, NEDDF_EINVAL, std::string(what) + ": negative count");
    if ((n > 0 && !have_points) || (V > 0 && !v) || (T > 0 && !tri)) return fail(ctx, NEDDF_EINVAL, std::string(what) + ": NULL rays, vertices or triangles");
    if (n >= ((int64_t)1 << 31) || V >= ((int64_t)1 << 31) || T >= ((int64_t)1 << 31))
        return fail(ctx, NEDDF_EUNSUPPORTED, std::string(what) + ": 2^31 rays, triangles or vertices or more (indices are int32)");
    return 0;
}

static int pad_ok(neddf_ctx *ctx, float pad, const char *what)
{
    if (!(pad >= 0.f) || !std::isfinite(pad)) return fail(ctx, NEDDF_EINVAL, std::string(what) + ": pad must be finite and not negative");
    return 0;
}

// the four per-query outputs of a ray cast or a point-to-mesh query; the lists of neddf_raycast_grid_build as a query receives them
static bool outputs_ok(int64_t n, const void *d_first, const void *d_triangle, const void *d_b1, const void *d_b2) { return n <= 0 || (d_first && d_triangle && d_b1 && d_b2); }
static bool cell_lists_ok(const int32_t *d_cell_start, const int32_t *d_items, int64_t n_items) { return d_cell_start && n_items >= 0 && n_items <= 0x7fffffff && (n_items == 0 || d_items); }

// THE cell function of a box ("neddf_nn_grid_build's cells" of the header): n = cells, lo = (float)h_lo, inv_cell = (float)(cells /
// (h_hi - h_lo)) with the quotient in double (0 for a zero-extent axis); safe_cell = 0, for the users that follow no lists.  The limit
// of 2^24 cells in all is the lists', not the cell function's (nn_grid).
static int cell_grid(neddf_ctx *ctx, const double *h_lo, const double *h_hi, const int *cells, NnGrid *g, const char *what)
{
    for (int a = 0; a < 3; ++a) {
        if (cells[a] < 1 || cells[a] > kNnMaxAxis) return fail(ctx, NEDDF_EINVAL, std::string(what) + ": 1 to 1024 cells per axis");
        if (!std::isfinite(h_lo[a]) || !std::isfinite(h_hi[a]) || !(h_hi[a] >= h_lo[a])) return fail(ctx, NEDDF_EINVAL, std::string(what) + ": a finite box with hi >= lo expected");
        g->n[a] = cells[a];
        g->lo[a] = (float)h_lo[a];
        const double ext = h_hi[a] - h_lo[a];
        g->inv_cell[a] = ext > 0.0 ? (float)((double)cells[a] / ext) : 0.f;
        if (!std::isfinite(g->lo[a]) || !std::isfinite(g->inv_cell[a])) return fail(ctx, NEDDF_EINVAL, std::string(what) + ": the box does not fit fp32");
    }
    g->safe_cell = 0.f;
    return 0;
}

// ---- mesh normals, connected components, compaction (mesh_kernels.hip) ----
int neddf_mesh_vertex_normals(neddf_ctx *ctx, const float *d_vertices, int64_t n_vertices, const int32_t *d_triangles, int64_t n_triangles,
                              float *d_normals, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (n_vertices < 0 || n_triangles < 0) return fail(ctx, NEDDF_EINVAL, "mesh_vertex_normals: negative count");
    if (n_vertices == 0) return 0;
    if (!d_vertices || !d_normals || (n_triangles > 0 && !d_triangles)) return fail(ctx, NEDDF_EINVAL, "mesh_vertex_normals: NULL vertices, triangles or normals");
    if (n_vertices >= ((int64_t)1 << 31)) return fail(ctx, NEDDF_EUNSUPPORTED, "mesh_vertex_normals: 2^31 vertices or more (triangle indices are int32)");
    DeviceGuard guard_(ctx->device);
    if (int rc = ensure(ctx, ctx->mc_nacc, (size_t)(3 * n_vertices + 1) * sizeof(unsigned long long))) return rc;
    launch_mesh_normals(d_vertices, n_vertices, d_triangles, n_triangles, (unsigned long long *)ctx->mc_nacc.p, d_normals, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

// block totals of nbv vertex blocks and nbt triangle blocks (each with its grand total behind it), then kCcBatch "changed" words
static int mesh_workspace(neddf_ctx *ctx, int64_t V, int64_t nbv, int64_t nbt)
{
    if (int rc = ensure(ctx, ctx->cc_parent, (size_t)(V > 0 ? V : 1) * sizeof(int32_t))) return rc;
    if (int rc = ensure(ctx, ctx->cc_used, (size_t)(V > 0 ? V : 1))) return rc;
    return ensure(ctx, ctx->cc_blk, (size_t)(nbv + nbt + 2) * sizeof(int64_t) + kCcBatch * sizeof(int));
}

int neddf_mesh_components(neddf_ctx *ctx, const int32_t *d_triangles, int64_t n_triangles, int64_t n_vertices, int32_t *d_vertex_label,
                          int32_t *d_triangle_label, int64_t *d_component_triangles, int64_t *h_n_components, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    const int64_t V = n_vertices, T = n_triangles;
    if (V < 0 || T < 0) return fail(ctx, NEDDF_EINVAL, "mesh_components: negative count");
    if (!h_n_components || (T > 0 && !d_triangles) || (V > 0 && (!d_vertex_label || !d_component_triangles)))
        return fail(ctx, NEDDF_EINVAL, "mesh_components: NULL triangles, vertex labels, component counts or count");
    const int64_t nbv = mc_blocks(V), nbt = mc_blocks(T);
    if (V >= ((int64_t)1 << 31) || nbt > 0x7fffffff) return fail(ctx, NEDDF_EUNSUPPORTED, "mesh_components: 2^31 vertices or more, or too many triangles");
    DeviceGuard guard_(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = mesh_workspace(ctx, V, nbv, 0)) return rc;
    int32_t *parent = (int32_t *)ctx->cc_parent.p;
    unsigned char *used = (unsigned char *)ctx->cc_used.p;
    int64_t *blk = (int64_t *)ctx->cc_blk.p;
    int *changed = (int *)(blk + nbv + 2);
    launch_cc_init(parent, used, V, d_triangles, T, s);
    HIPCHK(hipGetLastError());
    // rounds of (hook, jump) until one changes nothing; the "changed" words are read once per batch of kCcBatch rounds
    ctx->cc_rounds = 0;
    for (bool done = V == 0 || T == 0; !done;) {
        if (ctx->cc_rounds >= kCcMaxRounds) return fail(ctx, NEDDF_EUNSUPPORTED, "mesh_components: no fixed point within the round limit");
        int h_changed[kCcBatch];
        HIPCHK(hipMemsetAsync(changed, 0, sizeof(h_changed), s));
        for (int r = 0; r < kCcBatch; ++r) launch_cc_round(parent, V, d_triangles, T, changed + r, s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h_changed, changed, sizeof(h_changed), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (int r = 0; r < kCcBatch && !done; ++r) {
            ++ctx->cc_rounds;
            done = h_changed[r] == 0;
        }
    }
    launch_cc_labels(parent, used, V, d_triangles, T, blk, d_vertex_label, d_triangle_label, d_component_triangles, s);
    return read_totals(ctx, s, { { h_n_components, blk + nbv } });
}

int neddf_mesh_components_rounds(neddf_ctx *ctx)
{
    return ctx ? ctx->cc_rounds : NEDDF_EINVAL;
}

int neddf_mesh_compact(neddf_ctx *ctx, const float *d_vertices, int64_t n_vertices, const int32_t *d_triangles, int64_t n_triangles,
                       const unsigned char *d_keep_triangle, float *d_out_vertices, int64_t vertex_cap, int32_t *d_out_triangles,
                       int64_t triangle_cap, int32_t *d_vertex_map, int64_t *h_n_vertices, int64_t *h_n_triangles, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    const int64_t V = n_vertices, T = n_triangles;
    if (V < 0 || T < 0) return fail(ctx, NEDDF_EINVAL, "mesh_compact: negative count");
    if (!h_n_vertices || !h_n_triangles || (V > 0 && !d_vertices) || (T > 0 && (!d_triangles || !d_keep_triangle)))
        return fail(ctx, NEDDF_EINVAL, "mesh_compact: NULL vertices, triangles, keep flags or count");
    const int64_t nbv = mc_blocks(V), nbt = mc_blocks(T);
    if (V >= ((int64_t)1 << 31) || nbt > 0x7fffffff) return fail(ctx, NEDDF_EUNSUPPORTED, "mesh_compact: 2^31 vertices or more, or too many triangles");
    DeviceGuard guard_(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = mesh_workspace(ctx, V, nbv, nbt)) return rc;
    unsigned char *used = (unsigned char *)ctx->cc_used.p;
    int64_t *vblk = (int64_t *)ctx->cc_blk.p, *tblk = vblk + nbv + 1;
    launch_compact_count(d_triangles, T, V, d_keep_triangle, used, vblk, tblk, s);
    int64_t counts[2];
    if (int rc = read_totals(ctx, s, { { &counts[0], vblk + nbv }, { &counts[1], tblk + nbt } })) return rc;
    *h_n_vertices = counts[0];
    *h_n_triangles = counts[1];
    if (!d_out_vertices || !d_out_triangles || vertex_cap < counts[0] || triangle_cap < counts[1]) return 0;     // the counting call
    launch_compact_write(d_vertices, V, d_triangles, T, d_keep_triangle, used, vblk, tblk, d_vertex_map ? d_vertex_map : (int32_t *)ctx->cc_parent.p,
                         d_out_vertices, d_out_triangles, s);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- distances between surfaces (geom_kernels.hip) ----
// (the sampling entry points share one prefix and keep a checker of their own: its NULL test covers the count, its limit the triangles' blocks)
static int sample_args_ok(neddf_ctx *ctx, const float *v, int64_t V, const int32_t *tri, int64_t T, double density, const int64_t *h_n)
{
    if (V < 0 || T < 0) return fail(ctx, NEDDF_EINVAL, "mesh_sample: negative count");
    if (!h_n || (T > 0 && !tri) || (V > 0 && !v)) return fail(ctx, NEDDF_EINVAL, "mesh_sample: NULL vertices, triangles or count");
    if (!(density >= 0.0) || !std::isfinite(density)) return fail(ctx, NEDDF_EINVAL, "mesh_sample: the density must be finite and not negative");
    if (V >= ((int64_t)1 << 31) || mc_blocks(T) > 0x7fffffff) return fail(ctx, NEDDF_EUNSUPPORTED, "mesh_sample: 2^31 vertices or more, or too many triangles");
    return 0;
}

// count -> scan -> one synchronise; *n = the number of samples, NEDDF_EINVAL when it does not fit int32
static int sample_total(neddf_ctx *ctx, const float *v, int64_t V, const int32_t *tri, int64_t T, double density, uint32_t seed, int64_t *n, hipStream_t s)
{
    if (int rc = ensure(ctx, ctx->geom_blk, (size_t)(mc_blocks(T) + 1) * sizeof(int64_t))) return rc;
    int64_t *blk = (int64_t *)ctx->geom_blk.p;
    launch_sample_count(v, V, tri, T, density, seed, blk, s);
    if (int rc = read_totals(ctx, s, { { n, blk + mc_blocks(T) } })) return rc;
    if (*n > 0x7fffffff) return fail(ctx, NEDDF_EINVAL, "mesh_sample: the density gives 2^31 samples or more (indices are int32)");
    return 0;
}

int neddf_mesh_sample_count(neddf_ctx *ctx, const float *d_vertices, int64_t n_vertices, const int32_t *d_triangles, int64_t n_triangles, double density,
                            uint32_t seed, int64_t *h_n_samples, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (int rc = sample_args_ok(ctx, d_vertices, n_vertices, d_triangles, n_triangles, density, h_n_samples)) return rc;
    DeviceGuard guard_(ctx->device);
    return sample_total(ctx, d_vertices, n_vertices, d_triangles, n_triangles, density, seed, h_n_samples, (hipStream_t)stream);
}

int neddf_mesh_sample_write(neddf_ctx *ctx, const float *d_vertices, int64_t n_vertices, const int32_t *d_triangles, int64_t n_triangles, double density,
                            uint32_t seed, float *d_points, int32_t *d_triangle_id, int64_t sample_cap, int64_t *h_n_samples, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (int rc = sample_args_ok(ctx, d_vertices, n_vertices, d_triangles, n_triangles, density, h_n_samples)) return rc;
    DeviceGuard guard_(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = sample_total(ctx, d_vertices, n_vertices, d_triangles, n_triangles, density, seed, h_n_samples, s)) return rc;
    if (*h_n_samples == 0) return 0;
    if (!d_points || !d_triangle_id || sample_cap < *h_n_samples) return fail(ctx, NEDDF_EINVAL, "mesh_sample_write: NULL outputs or a capacity below the count");
    launch_sample_write(d_vertices, n_vertices, d_triangles, n_triangles, density, seed, (const int64_t *)ctx->geom_blk.p, d_points, d_triangle_id, s);
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_nn_brute(neddf_ctx *ctx, const float *d_queries, int64_t n_queries, const float *d_targets, int64_t n_targets, float *d_d2, int32_t *d_index,
                   void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (int rc = point_counts_ok(ctx, "nn_brute", n_queries, d_queries, n_targets, d_targets)) return rc;
    if (n_queries > 0 && (!d_d2 || !d_index)) return fail(ctx, NEDDF_EINVAL, "nn_brute: NULL outputs");
    DeviceGuard guard_(ctx->device);
    launch_nn_brute(d_queries, n_queries, d_targets, n_targets, d_d2, d_index, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

// the grid of cell lists over a box: cell_grid's cells, at most 2^24 of them, and safe_cell = 0.99 / max(inv_cell) rounded to float
static int nn_grid(neddf_ctx *ctx, const double *h_lo, const double *h_hi, const int *h_cells, NnGrid *g, const char *what)
{
    if (!h_lo || !h_hi || !h_cells) return fail(ctx, NEDDF_EINVAL, std::string(what) + ": NULL box or cells");
    if (int rc = cell_grid(ctx, h_lo, h_hi, h_cells, g, what)) return rc;
    if ((int64_t)g->n[0] * g->n[1] * g->n[2] > kNnMaxCells) return fail(ctx, NEDDF_EINVAL, std::string(what) + ": more than 2^24 cells");
    const float inv_max = std::max(g->inv_cell[0], std::max(g->inv_cell[1], g->inv_cell[2]));
    const double safe = inv_max > 0.f ? 0.99 / (double)inv_max : 3.0e38;
    g->safe_cell = safe < 3.0e38 ? (float)safe : 3.0e38f;
    return 0;
}

int neddf_nn_grid_build(neddf_ctx *ctx, const float *d_targets, int64_t n_targets, const double *h_lo, const double *h_hi, const int *h_cells,
                        int32_t *d_cell_start, int32_t *d_order, int64_t *h_n_valid, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (int rc = point_counts_ok(ctx, "nn_grid_build", n_targets, d_targets)) return rc;
    NnGrid g;
    if (int rc = nn_grid(ctx, h_lo, h_hi, h_cells, &g, "nn_grid_build")) return rc;
    if (!d_cell_start || !h_n_valid || (n_targets > 0 && !d_order)) return fail(ctx, NEDDF_EINVAL, "nn_grid_build: NULL cell_start, order or count");
    DeviceGuard guard_(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_cells = (int64_t)g.n[0] * g.n[1] * g.n[2], nb = mc_blocks(n_cells);
    if (int rc = ensure(ctx, ctx->geom_blk, (size_t)(nb + 1) * sizeof(int64_t))) return rc;
    if (int rc = ensure(ctx, ctx->geom_ws, (size_t)(n_targets + n_cells) * sizeof(int32_t))) return rc;
    int32_t *cell_of = (int32_t *)ctx->geom_ws.p, *count = cell_of + n_targets;
    int64_t *blk = (int64_t *)ctx->geom_blk.p;
    launch_nn_grid_build(g, d_targets, n_targets, cell_of, count, blk, d_cell_start, d_order, s);
    return read_totals(ctx, s, { { h_n_valid, blk + nb } });
}

int neddf_nn_grid_query(neddf_ctx *ctx, const float *d_queries, int64_t n_queries, const float *d_targets, int64_t n_targets, const double *h_lo,
                        const double *h_hi, const int *h_cells, const int32_t *d_cell_start, const int32_t *d_order, float *d_d2, int32_t *d_index,
                        void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (int rc = point_counts_ok(ctx, "nn_grid_query", n_queries, d_queries, n_targets, d_targets)) return rc;
    NnGrid g;
    if (int rc = nn_grid(ctx, h_lo, h_hi, h_cells, &g, "nn_grid_query")) return rc;
    if (!d_cell_start || (n_queries > 0 && (!d_d2 || !d_index))) return fail(ctx, NEDDF_EINVAL, "nn_grid_query: NULL cell_start or outputs");
    DeviceGuard guard_(ctx->device);
    // a NULL order is the empty list of a build that found no finite target: no range of it is followed
    launch_nn_grid_query(g, d_queries, n_queries, d_targets, d_order ? n_targets : 0, d_cell_start, d_order, d_d2, d_index, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- ray casting on meshes (raycast_kernels.hip) ----
// the grid of a box, its cell counts and pad (checked here): neddf_nn_grid_build's cells, the box widened by 2 pad, the walk's fp64
// cells and the limits the equality argument of the header needs
static int rc_grid(neddf_ctx *ctx, const double *h_lo, const double *h_hi, const int *h_cells, float pad, RcGrid *g, const char *what)
{
    if (int rc = pad_ok(ctx, pad, what)) return rc;
    if (int rc = nn_grid(ctx, h_lo, h_hi, h_cells, &g->nn, what)) return rc;
    double scale = 0.0;
    for (int a = 0; a < 3; ++a) scale = std::max(std::max(scale, std::fabs(h_lo[a])), std::max(std::fabs(h_hi[a]), h_hi[a] - h_lo[a]));
    if (!((double)pad >= scale * 0x1p-16))
        return fail(ctx, NEDDF_EINVAL, std::string(what) + ": pad below 2^-16 of the largest of |lo|, |hi| and the box extent (the grid would lose hits to rounding)");
    g->pad = pad;
    g->pad2 = 2.f * pad;
    if (!std::isfinite(g->pad2)) return fail(ctx, NEDDF_EINVAL, std::string(what) + ": 2 pad does not fit fp32");
    for (int a = 0; a < 3; ++a) {
        const float hi = (float)h_hi[a];
        g->wlo[a] = g->nn.lo[a] - g->pad2;
        g->whi[a] = hi + g->pad2;
        if (!std::isfinite(g->wlo[a]) || !std::isfinite(g->whi[a])) return fail(ctx, NEDDF_EINVAL, std::string(what) + ": the widened box does not fit fp32");
        g->lo[a] = (double)g->nn.lo[a];
        g->edge[a] = g->nn.inv_cell[a] > 0.f ? 1.0 / (double)g->nn.inv_cell[a] : 0.0;
    }
    // the rounding of o + t d, at most 2^-24 (|o| + 2 |p|) per axis, stays below pad / 8 for an origin inside this limit
    const double far = (double)pad * 0x1p21 - 2.0 * (scale + 2.0 * (double)pad);
    g->far_origin = far > 0.0 ? (far < 3.0e38 ? (float)far : 3.0e38f) : 0.f;
    return 0;
}

int neddf_raycast_brute(neddf_ctx *ctx, const float *d_ray_orig, const float *d_ray_dir, int64_t n_rays, const float *d_vertices, int64_t n_vertices,
                        const int32_t *d_triangles, int64_t n_triangles, float t_min, float t_max, float pad, float *d_t, int32_t *d_triangle,
                        float *d_b1, float *d_b2, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (int rc = mesh_counts_ok(ctx, n_vertices, d_vertices, n_triangles, d_triangles, "raycast_brute", n_rays, d_ray_orig && d_ray_dir)) return rc;
    if (int rc = pad_ok(ctx, pad, "raycast_brute")) return rc;
    if (!outputs_ok(n_rays, d_t, d_triangle, d_b1, d_b2)) return fail(ctx, NEDDF_EINVAL, "raycast_brute: NULL outputs");
    DeviceGuard guard_(ctx->device);
    launch_raycast_brute(d_ray_orig, d_ray_dir, n_rays, d_vertices, n_vertices, d_triangles, n_triangles, t_min, t_max, pad, d_t, d_triangle, d_b1,
                         d_b2, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

// count -> scan -> one synchronise; *n = the number of (list, triangle) pairs, NEDDF_EINVAL when it does not fit int32
static int rc_total(neddf_ctx *ctx, const RcGrid &g, const float *v, int64_t V, const int32_t *tri, int64_t T, int64_t *n, hipStream_t s, const char *what)
{
    const int64_t n_lists = (int64_t)g.nn.n[0] * g.nn.n[1] * g.nn.n[2] + 1, nb = mc_blocks(n_lists);
    if (int rc = ensure(ctx, ctx->geom_blk, (size_t)(nb + 1) * sizeof(int64_t))) return rc;
    if (int rc = ensure(ctx, ctx->geom_ws, (size_t)n_lists * sizeof(int32_t))) return rc;
    int64_t *blk = (int64_t *)ctx->geom_blk.p;
    launch_raycast_grid_count(g, v, V, tri, T, (int32_t *)ctx->geom_ws.p, blk, s);
    if (int rc = read_totals(ctx, s, { { n, blk + nb } })) return rc;
    if (*n > 0x7fffffff) return fail(ctx, NEDDF_EINVAL, std::string(what) + ": 2^31 (cell, triangle) pairs or more (offsets are int32): fewer cells, or a smaller pad");
    return 0;
}

int neddf_raycast_grid_count(neddf_ctx *ctx, const float *d_vertices, int64_t n_vertices, const int32_t *d_triangles, int64_t n_triangles,
                             const double *h_lo, const double *h_hi, const int *h_cells, float pad, int64_t *h_n_items, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (int rc = mesh_counts_ok(ctx, n_vertices, d_vertices, n_triangles, d_triangles, "raycast_grid_count")) return rc;
    RcGrid g;
    if (int rc = rc_grid(ctx, h_lo, h_hi, h_cells, pad, &g, "raycast_grid_count")) return rc;
    if (!h_n_items) return fail(ctx, NEDDF_EINVAL, "raycast_grid_count: NULL count");
    DeviceGuard guard_(ctx->device);
    return rc_total(ctx, g, d_vertices, n_vertices, d_triangles, n_triangles, h_n_items, (hipStream_t)stream, "raycast_grid_count");
}

int neddf_raycast_grid_build(neddf_ctx *ctx, const float *d_vertices, int64_t n_vertices, const int32_t *d_triangles, int64_t n_triangles,
                             const double *h_lo, const double *h_hi, const int *h_cells, float pad, int32_t *d_cell_start, int32_t *d_items,
                             int64_t item_cap, int64_t *h_n_items, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (int rc = mesh_counts_ok(ctx, n_vertices, d_vertices, n_triangles, d_triangles, "raycast_grid_build")) return rc;
    RcGrid g;
    if (int rc = rc_grid(ctx, h_lo, h_hi, h_cells, pad, &g, "raycast_grid_build")) return rc;
    if (!d_cell_start || !h_n_items) return fail(ctx, NEDDF_EINVAL, "raycast_grid_build: NULL cell_start or count");
    DeviceGuard guard_(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = rc_total(ctx, g, d_vertices, n_vertices, d_triangles, n_triangles, h_n_items, s, "raycast_grid_build")) return rc;
    if (*h_n_items > 0 && (!d_items || item_cap < *h_n_items)) return fail(ctx, NEDDF_EINVAL, "raycast_grid_build: NULL items or a capacity below the count");
    launch_raycast_grid_place(g, d_vertices, n_vertices, d_triangles, n_triangles, (int32_t *)ctx->geom_ws.p, (const int64_t *)ctx->geom_blk.p,
                              d_cell_start, *h_n_items > 0 ? d_items : nullptr, s);
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_raycast_grid_query(neddf_ctx *ctx, const float *d_ray_orig, const float *d_ray_dir, int64_t n_rays, const float *d_vertices, int64_t n_vertices,
                             const int32_t *d_triangles, int64_t n_triangles, const double *h_lo, const double *h_hi, const int *h_cells, float pad,
                             const int32_t *d_cell_start, const int32_t *d_items, int64_t n_items, float t_min, float t_max, float *d_t,
                             int32_t *d_triangle, float *d_b1, float *d_b2, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (int rc = mesh_counts_ok(ctx, n_vertices, d_vertices, n_triangles, d_triangles, "raycast_grid_query", n_rays, d_ray_orig && d_ray_dir)) return rc;
    RcGrid g;
    if (int rc = rc_grid(ctx, h_lo, h_hi, h_cells, pad, &g, "raycast_grid_query")) return rc;
    if (!cell_lists_ok(d_cell_start, d_items, n_items) || !outputs_ok(n_rays, d_t, d_triangle, d_b1, d_b2))
        return fail(ctx, NEDDF_EINVAL, "raycast_grid_query: NULL cell_start, items or outputs, or an item count outside [0, 2^31)");
    DeviceGuard guard_(ctx->device);
    launch_raycast_grid_query(g, d_ray_orig, d_ray_dir, n_rays, d_vertices, n_vertices, d_triangles, n_triangles, d_cell_start, d_items, n_items, t_min,
                              t_max, d_t, d_triangle, d_b1, d_b2, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- point-to-mesh distance (pointmesh_kernels.hip) ----
int neddf_point_mesh_brute(neddf_ctx *ctx, const float *d_queries, int64_t n_queries, const float *d_vertices, int64_t n_vertices,
                           const int32_t *d_triangles, int64_t n_triangles, float *d_d2, int32_t *d_triangle, float *d_b1, float *d_b2, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (int rc = mesh_counts_ok(ctx, n_vertices, d_vertices, n_triangles, d_triangles, "point_mesh_brute", n_queries, d_queries != nullptr)) return rc;
    if (!outputs_ok(n_queries, d_d2, d_triangle, d_b1, d_b2)) return fail(ctx, NEDDF_EINVAL, "point_mesh_brute: NULL outputs");
    DeviceGuard guard_(ctx->device);
    launch_point_mesh_brute(d_queries, n_queries, d_vertices, n_vertices, d_triangles, n_triangles, d_d2, d_triangle, d_b1, d_b2, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_point_mesh_grid_query(neddf_ctx *ctx, const float *d_queries, int64_t n_queries, const float *d_vertices, int64_t n_vertices,
                                const int32_t *d_triangles, int64_t n_triangles, const double *h_lo, const double *h_hi, const int *h_cells, float pad,
                                const int32_t *d_cell_start, const int32_t *d_items, int64_t n_items, float *d_d2, int32_t *d_triangle, float *d_b1,
                                float *d_b2, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (int rc = mesh_counts_ok(ctx, n_vertices, d_vertices, n_triangles, d_triangles, "point_mesh_grid_query", n_queries, d_queries != nullptr)) return rc;
    RcGrid rg;
    if (int rc = rc_grid(ctx, h_lo, h_hi, h_cells, pad, &rg, "point_mesh_grid_query")) return rc;
    if (!cell_lists_ok(d_cell_start, d_items, n_items) || !outputs_ok(n_queries, d_d2, d_triangle, d_b1, d_b2))
        return fail(ctx, NEDDF_EINVAL, "point_mesh_grid_query: NULL cell_start, items or outputs, or an item count outside [0, 2^31)");
    PmGrid g;
    g.nn = rg.nn;
    // the shells are walked when the smallest cell edge is at least 2^-10 of the largest |coordinate| of the widened box (the header's
    // equality argument, part 3); a grid without any extent is one cell
    float inv_max = 0.f;
    double w = 0.0;
    for (int a = 0; a < 3; ++a) {
        inv_max = std::max(inv_max, rg.nn.inv_cell[a]);
        w = std::max(w, std::max(std::fabs((double)rg.wlo[a]), std::fabs((double)rg.whi[a])));
    }
    g.walk = (inv_max == 0.f || 1.0 / (double)inv_max >= 0x1p-10 * w) ? 1 : 0;
    DeviceGuard guard_(ctx->device);
    if (n_queries > 0 && n_triangles > 0)
        if (int rc = ensure(ctx, ctx->geom_ws, (size_t)n_triangles * kPmTableFloats * sizeof(float))) return rc;
    launch_point_mesh_grid_query(g, d_queries, n_queries, d_vertices, n_vertices, d_triangles, n_triangles, (float *)ctx->geom_ws.p, d_cell_start, d_items,
                                 n_items, d_d2, d_triangle, d_b1, d_b2, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- a BVH over the triangles, and the point-to-mesh distance through it (bvh_kernels.hip) ----
int neddf_bvh_keys(neddf_ctx *ctx, const float *d_vertices, int64_t n_vertices, const int32_t *d_triangles, int64_t n_triangles, const double *h_lo,
                   const double *h_hi, int64_t *d_keys, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (int rc = mesh_counts_ok(ctx, n_vertices, d_vertices, n_triangles, d_triangles, "bvh_keys")) return rc;
    if (!h_lo || !h_hi) return fail(ctx, NEDDF_EINVAL, "bvh_keys: NULL box");
    if (n_triangles > 0 && !d_keys) return fail(ctx, NEDDF_EINVAL, "bvh_keys: NULL keys");
    const int cells[3] = { kNnMaxAxis, kNnMaxAxis, kNnMaxAxis };        // always in range: the cell check of cell_grid never speaks here
    NnGrid g;
    if (int rc = cell_grid(ctx, h_lo, h_hi, cells, &g, "bvh_keys")) return rc;
    DeviceGuard guard_(ctx->device);
    launch_bvh_keys(g, d_vertices, n_vertices, d_triangles, n_triangles, d_keys, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_bvh_build(neddf_ctx *ctx, const float *d_vertices, int64_t n_vertices, const int32_t *d_triangles, int64_t n_triangles,
                    const int64_t *d_sorted_keys, int32_t *d_leaf_triangle, int32_t *d_children, float *d_boxes, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (int rc = mesh_counts_ok(ctx, n_vertices, d_vertices, n_triangles, d_triangles, "bvh_build")) return rc;
    if (n_triangles > 0 && (!d_sorted_keys || !d_leaf_triangle || !d_boxes || (n_triangles > 1 && !d_children)))
        return fail(ctx, NEDDF_EINVAL, "bvh_build: NULL keys, leaf_triangle, children or boxes");
    if (n_triangles == 0) return 0;
    DeviceGuard guard_(ctx->device);
    if (int rc = ensure(ctx, ctx->geom_ws, (size_t)(3 * n_triangles) * sizeof(int32_t))) return rc;
    int32_t *parent = (int32_t *)ctx->geom_ws.p, *counter = parent + (2 * n_triangles - 1);
    launch_bvh_build(d_sorted_keys, d_vertices, n_vertices, d_triangles, n_triangles, d_leaf_triangle, d_children, d_boxes, parent, counter,
                     (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_point_mesh_bvh_query(neddf_ctx *ctx, const float *d_queries, int64_t n_queries, const float *d_vertices, int64_t n_vertices,
                               const int32_t *d_triangles, int64_t n_triangles, const int32_t *d_leaf_triangle, const int32_t *d_children,
                               const float *d_boxes, int64_t n_leaves, float *d_d2, int32_t *d_triangle, float *d_b1, float *d_b2, int32_t *d_visits,
                               void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (int rc = mesh_counts_ok(ctx, n_vertices, d_vertices, n_triangles, d_triangles, "point_mesh_bvh_query", n_queries, d_queries != nullptr)) return rc;
    if (n_leaves != n_triangles) return fail(ctx, NEDDF_EINVAL, "point_mesh_bvh_query: the tree's leaves are not this mesh's triangles (n_leaves != n_triangles)");
    if (n_triangles > 0 && (!d_leaf_triangle || !d_boxes || (n_triangles > 1 && !d_children)))
        return fail(ctx, NEDDF_EINVAL, "point_mesh_bvh_query: NULL leaf_triangle, children or boxes");
    if (!outputs_ok(n_queries, d_d2, d_triangle, d_b1, d_b2)) return fail(ctx, NEDDF_EINVAL, "point_mesh_bvh_query: NULL outputs");
    DeviceGuard guard_(ctx->device);
    if (n_queries > 0 && n_triangles > 0)
        if (int rc = ensure(ctx, ctx->geom_ws, (size_t)n_triangles * kPmTableFloats * sizeof(float))) return rc;
    launch_point_mesh_bvh_query(d_queries, n_queries, d_vertices, n_vertices, d_triangles, n_triangles, (float *)ctx->geom_ws.p, d_leaf_triangle, d_children,
                                d_boxes, d_d2, d_triangle, d_b1, d_b2, d_visits, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- rays through the BVH (bvh_kernels.hip): the first hit and the any-hit flag share every check but the outputs' ----
static int raycast_bvh_args_ok(neddf_ctx *ctx, const char *what, const float *d_ray_orig, const float *d_ray_dir, int64_t n_rays, const float *d_vertices,
                               int64_t n_vertices, const int32_t *d_triangles, int64_t n_triangles, const int32_t *d_leaf_triangle,
                               const int32_t *d_children, const float *d_boxes, int64_t n_leaves, float pad)
{
    if (int rc = mesh_counts_ok(ctx, n_vertices, d_vertices, n_triangles, d_triangles, what, n_rays, d_ray_orig && d_ray_dir)) return rc;
    if (n_leaves != n_triangles) return fail(ctx, NEDDF_EINVAL, std::string(what) + ": the tree's leaves are not this mesh's triangles (n_leaves != n_triangles)");
    if (n_triangles > 0 && (!d_leaf_triangle || !d_boxes || (n_triangles > 1 && !d_children)))
        return fail(ctx, NEDDF_EINVAL, std::string(what) + ": NULL leaf_triangle, children or boxes");
    return pad_ok(ctx, pad, what);
}

int neddf_raycast_bvh_query(neddf_ctx *ctx, const float *d_ray_orig, const float *d_ray_dir, int64_t n_rays, const float *d_vertices, int64_t n_vertices,
                            const int32_t *d_triangles, int64_t n_triangles, const int32_t *d_leaf_triangle, const int32_t *d_children,
                            const float *d_boxes, int64_t n_leaves, float t_min, float t_max, float pad, float *d_t, int32_t *d_triangle, float *d_b1,
                            float *d_b2, int32_t *d_visits, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (int rc = raycast_bvh_args_ok(ctx, "raycast_bvh_query", d_ray_orig, d_ray_dir, n_rays, d_vertices, n_vertices, d_triangles, n_triangles,
                                     d_leaf_triangle, d_children, d_boxes, n_leaves, pad))
        return rc;
    if (!outputs_ok(n_rays, d_t, d_triangle, d_b1, d_b2)) return fail(ctx, NEDDF_EINVAL, "raycast_bvh_query: NULL outputs");
    DeviceGuard guard_(ctx->device);
    launch_raycast_bvh(false, d_ray_orig, d_ray_dir, n_rays, d_vertices, n_vertices, d_triangles, n_triangles, d_leaf_triangle, d_children, d_boxes, t_min,
                       t_max, pad, d_t, d_triangle, d_b1, d_b2, nullptr, d_visits, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_raycast_bvh_occluded(neddf_ctx *ctx, const float *d_ray_orig, const float *d_ray_dir, int64_t n_rays, const float *d_vertices,
                               int64_t n_vertices, const int32_t *d_triangles, int64_t n_triangles, const int32_t *d_leaf_triangle,
                               const int32_t *d_children, const float *d_boxes, int64_t n_leaves, float t_min, float t_max, float pad,
                               uint8_t *d_occluded, int32_t *d_visits, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (int rc = raycast_bvh_args_ok(ctx, "raycast_bvh_occluded", d_ray_orig, d_ray_dir, n_rays, d_vertices, n_vertices, d_triangles, n_triangles,
                                     d_leaf_triangle, d_children, d_boxes, n_leaves, pad))
        return rc;
    if (n_rays > 0 && !d_occluded) return fail(ctx, NEDDF_EINVAL, "raycast_bvh_occluded: NULL outputs");
    DeviceGuard guard_(ctx->device);
    launch_raycast_bvh(true, d_ray_orig, d_ray_dir, n_rays, d_vertices, n_vertices, d_triangles, n_triangles, d_leaf_triangle, d_children, d_boxes, t_min,
                       t_max, pad, nullptr, nullptr, nullptr, nullptr, d_occluded, d_visits, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- mesh simplification by vertex clustering (simplify_kernels.hip) ----
// (counts alone: every step names its own arrays after its own range checks, and this wording has no rays)
static int simplify_counts_ok(neddf_ctx *ctx, int64_t V, int64_t T, const char *what)
{
    if (V < 0 || T < 0) return fail(ctx, NEDDF_EINVAL, std::string(what) + ": negative count");
    if (V >= ((int64_t)1 << 31) || T >= ((int64_t)1 << 31)) return fail(ctx, NEDDF_EUNSUPPORTED, std::string(what) + ": 2^31 vertices or triangles or more (indices are int32)");
    return 0;
}

int neddf_mesh_simplify_keys(neddf_ctx *ctx, const float *d_vertices, int64_t n_vertices, const double *h_lo, const double *h_hi, const int *h_cells,
                             int64_t *d_keys, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (int rc = simplify_counts_ok(ctx, n_vertices, 0, "mesh_simplify_keys")) return rc;
    if (!h_lo || !h_hi || !h_cells) return fail(ctx, NEDDF_EINVAL, "mesh_simplify_keys: NULL box or cells");
    if (n_vertices > 0 && (!d_vertices || !d_keys)) return fail(ctx, NEDDF_EINVAL, "mesh_simplify_keys: NULL vertices or keys");
    NnGrid g;
    if (int rc = cell_grid(ctx, h_lo, h_hi, h_cells, &g, "mesh_simplify_keys")) return rc;
    DeviceGuard guard_(ctx->device);
    launch_simplify_keys(g, d_vertices, n_vertices, d_keys, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_mesh_simplify_clusters(neddf_ctx *ctx, const int64_t *d_sorted_keys, int64_t n_vertices, int32_t *d_vertex_cluster, int32_t *d_cluster_range,
                                 int64_t *h_n_clusters, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    const int64_t V = n_vertices;
    if (int rc = simplify_counts_ok(ctx, V, 0, "mesh_simplify_clusters")) return rc;
    if (!h_n_clusters || (V > 0 && (!d_sorted_keys || !d_vertex_cluster || !d_cluster_range)))
        return fail(ctx, NEDDF_EINVAL, "mesh_simplify_clusters: NULL keys, vertex clusters, cluster ranges or count");
    DeviceGuard guard_(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    const int64_t nb = mc_blocks(V);
    if (int rc = ensure(ctx, ctx->cc_parent, (size_t)(V + 1) * sizeof(int32_t))) return rc;
    if (int rc = ensure(ctx, ctx->cc_used, (size_t)(V > 0 ? V : 1))) return rc;
    if (int rc = ensure(ctx, ctx->cc_blk, (size_t)(2 * nb + 2) * sizeof(int64_t))) return rc;
    int64_t *sblk = (int64_t *)ctx->cc_blk.p, *vblk = sblk + nb + 1;
    launch_simplify_clusters(d_sorted_keys, V, (unsigned char *)ctx->cc_used.p, (int32_t *)ctx->cc_parent.p, sblk, vblk, d_vertex_cluster, d_cluster_range, s);
    return read_totals(ctx, s, { { h_n_clusters, sblk + nb } });
}

int neddf_mesh_simplify_pairs(neddf_ctx *ctx, const float *d_vertices, int64_t n_vertices, const int32_t *d_triangles, int64_t n_triangles,
                              const int32_t *d_vertex_cluster, int64_t *d_pairs, int64_t pair_cap, int64_t *h_n_pairs, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    const int64_t V = n_vertices, T = n_triangles;
    if (int rc = simplify_counts_ok(ctx, V, T, "mesh_simplify_pairs")) return rc;
    if (!h_n_pairs || (V > 0 && (!d_vertices || !d_vertex_cluster)) || (T > 0 && !d_triangles))
        return fail(ctx, NEDDF_EINVAL, "mesh_simplify_pairs: NULL vertices, triangles, vertex clusters or count");
    DeviceGuard guard_(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    const int64_t nb = mc_blocks(T);
    if (int rc = ensure(ctx, ctx->cc_blk, (size_t)(nb + 1) * sizeof(int64_t))) return rc;
    int64_t *pblk = (int64_t *)ctx->cc_blk.p;
    launch_simplify_pair_count(d_vertices, V, d_triangles, T, d_vertex_cluster, pblk, s);
    if (int rc = read_totals(ctx, s, { { h_n_pairs, pblk + nb } })) return rc;
    if (!d_pairs || pair_cap < *h_n_pairs) return 0;                 // the counting call
    launch_simplify_pair_write(d_vertices, V, d_triangles, T, d_vertex_cluster, pblk, d_pairs, s);
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_mesh_simplify_place(neddf_ctx *ctx, const float *d_vertices, int64_t n_vertices, const int64_t *d_sorted_keys, const int32_t *d_cluster_range,
                              int64_t n_clusters, int placement, double regularisation, const int32_t *d_triangles, int64_t n_triangles,
                              const int64_t *d_sorted_pairs, int64_t n_pairs, float *d_out, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    const int64_t V = n_vertices, T = n_triangles, C = n_clusters;
    if (int rc = simplify_counts_ok(ctx, V, T, "mesh_simplify_place")) return rc;
    if (C < 0 || C > V || n_pairs < 0 || n_pairs > 3 * T) return fail(ctx, NEDDF_EINVAL, "mesh_simplify_place: 0 <= clusters <= vertices and 0 <= pairs <= 3 triangles expected");
    if (placement != NEDDF_SIMPLIFY_MEAN && placement != NEDDF_SIMPLIFY_QUADRIC) return fail(ctx, NEDDF_EINVAL, "mesh_simplify_place: unknown placement");
    if (!(regularisation >= 0.0) || !std::isfinite(regularisation)) return fail(ctx, NEDDF_EINVAL, "mesh_simplify_place: the regularisation must be finite and not negative");
    if (C > 0 && (!d_vertices || !d_sorted_keys || !d_cluster_range || !d_out)) return fail(ctx, NEDDF_EINVAL, "mesh_simplify_place: NULL vertices, keys, ranges or output");
    if (placement == NEDDF_SIMPLIFY_QUADRIC && n_pairs > 0 && (!d_triangles || !d_sorted_pairs))
        return fail(ctx, NEDDF_EINVAL, "mesh_simplify_place: NULL triangles or pairs");
    DeviceGuard guard_(ctx->device);
    launch_simplify_place(d_sorted_keys, V, d_cluster_range, C, d_vertices, d_triangles, T, d_sorted_pairs, n_pairs, placement == NEDDF_SIMPLIFY_QUADRIC,
                          regularisation, d_out, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_mesh_simplify_attributes(neddf_ctx *ctx, const float *d_attributes, int64_t n_vertices, int n_columns, const int64_t *d_sorted_keys,
                                   const int32_t *d_cluster_range, int64_t n_clusters, float *d_out, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    const int64_t V = n_vertices, C = n_clusters;
    if (int rc = simplify_counts_ok(ctx, V, 0, "mesh_simplify_attributes")) return rc;
    if (C < 0 || C > V || n_columns < 1 || n_columns > 1024) return fail(ctx, NEDDF_EINVAL, "mesh_simplify_attributes: 0 <= clusters <= vertices and 1 to 1024 columns expected");
    if (C > 0 && (!d_attributes || !d_sorted_keys || !d_cluster_range || !d_out)) return fail(ctx, NEDDF_EINVAL, "mesh_simplify_attributes: NULL attributes, keys, ranges or output");
    DeviceGuard guard_(ctx->device);
    launch_simplify_attributes(d_sorted_keys, V, d_cluster_range, C, d_attributes, n_columns, d_out, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_mesh_simplify_triangles(neddf_ctx *ctx, const int32_t *d_triangles, int64_t n_triangles, int64_t n_vertices, const int32_t *d_vertex_cluster,
                                  int32_t *d_mapped, int32_t *d_lowest, int64_t *d_keys, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (int rc = simplify_counts_ok(ctx, n_vertices, n_triangles, "mesh_simplify_triangles")) return rc;
    if ((n_triangles > 0 && (!d_triangles || !d_mapped || !d_lowest || !d_keys)) || (n_triangles > 0 && n_vertices > 0 && !d_vertex_cluster))
        return fail(ctx, NEDDF_EINVAL, "mesh_simplify_triangles: NULL triangles, vertex clusters or outputs");
    DeviceGuard guard_(ctx->device);
    launch_simplify_triangles(d_triangles, n_triangles, n_vertices, d_vertex_cluster, d_mapped, d_lowest, d_keys, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

int neddf_mesh_simplify_unique(neddf_ctx *ctx, const int32_t *d_lowest, const int64_t *d_keys, int64_t n_triangles, const int64_t *d_order,
                               unsigned char *d_keep_triangle, void *stream)
{
    if (!ctx) return NEDDF_EINVAL;
    if (int rc = simplify_counts_ok(ctx, 0, n_triangles, "mesh_simplify_unique")) return rc;
    if (n_triangles > 0 && (!d_lowest || !d_keys || !d_order || !d_keep_triangle)) return fail(ctx, NEDDF_EINVAL, "mesh_simplify_unique: NULL triples, order or keep flags");
    DeviceGuard guard_(ctx->device);
    launch_simplify_unique(d_lowest, d_keys, n_triangles, d_order, d_keep_triangle, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"
