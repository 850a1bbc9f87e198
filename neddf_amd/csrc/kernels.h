// kernels.h -- argument blocks shared by the HIP kernels and the C-ABI host code.
// gfx950 only (wave64, f32 MFMA 32x32x2); no portability layer on purpose.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace neddf {

constexpr int kWaves = 4;            // waves per workgroup (one per SIMD)
constexpr int kThreads = 64 * kWaves;
constexpr int kActLd = 260;          // LDS row stride (floats): 256 + 4 -> conflict-free ds_read_b128 of MFMA A fragments
constexpr int kWidth = 256;          // engine width of the shipped configurations (and of the training kernels); other hidden widths run on 128 / 384 / 512
constexpr int kMaxWidth = 512;
constexpr int kMaxLayers = 12;
constexpr int kMaxStash = 4;         // early partials per field: skip connections (+ the NeRF colour head's direction segment)
constexpr int kSchedInts = 16;          // tile-queue head (+ padding)
constexpr int kSchedXcd = 8, kSchedXcds = 8;     // ... and behind it one count of started tiles per XCD (tile_inputs.h l2_writeback_tick)
// DdfArgs::sched_flags of the three-term distance kernel also carries its L2 residency mechanism (NEDDF_X3_L2; inside the flags word, so
// that the argument block of every kernel keeps its layout): bits 4-5 the mode (1 stream, 2 wb, 3 both), bits 8-20 the write-back period
constexpr int kSchedL2ModeShift = 4, kSchedL2PeriodShift = 8;
constexpr int kPtAux = 16;           // floats per point handed from the distance kernel to the colour kernel
// floats of one stash slot of one workgroup: 4 waves x (MT=4 x NT=2 x 4 float4) x 64 lanes x 4
constexpr size_t kStashFloatsPerWg = (size_t)kWaves * (4 * 2 * 4) * 64 * 4;

// Sample points taken straight from the rays (round 5: SURVEY section 7 step 6, the cone moments in the field prologue): the
// reverse-mode distance kernel derives position / variance / direction of point i from ray i / S and its distances
// (device_math.h sample_moments: the stand-alone sampling kernel's own arithmetic, bit for bit) and hands them to the colour
// kernel INSIDE the per-point record it writes anyway -- the [N, 3] x 3 sampling tensors (36 B per point written and 60 B read)
// and the sampling launch disappear from neddf_render_rays' eval-minimal route.
// Se < S: only the first Se samples of every ray are points of the launch, numbered compactly (point i = sample i % Se of ray i / Se, and
// every per-point output is indexed by i).  The volume integral reads density / colour / normal of samples 0 .. S - 2 and of sample S - 1
// its distance alone (render_kernels.hip composite_kernel), so a render pass whose per-sample arrays never leave the library evaluates
// Se = S - 1 samples per ray (neddf_capi.hip render_pass).  A sample's moments do not depend on Se: dists keeps its row stride S.
struct RaySrc {
    const float *rd = nullptr, *ro = nullptr, *view = nullptr, *dists = nullptr;   // [B, 3], [B, 3], [B, 3] or NULL, [B, S]
    int S = 0;              // samples per ray
    int Se = 0;             // samples per ray that are evaluated: 1 .. S, or 0 for all S of them
    float r2 = 0.f;         // ray_radius^2 (cone sampling)
    int cone = 0;
    int64_t base = 0;       // index of this launch's first point in the [B, Se] grid
    double radius = -1.0;   // host side: the caller's ray radius as given (launch_sampling squares it itself), < 0 for point samples
};

// per-point record written by the distance-trunk kernel (float index); with RaySrc in eval-minimal mode the slots the colour kernel
// does not read there carry the sample point: PA_R_DIR (0..2), PA_R_POS (8..10), PA_R_VAR (11..13)
enum { PA_R_DIR = 0, PA_R_POS = 8, PA_R_VAR = 11 };
enum { PA_D = 0, PA_RHO = 1, PA_AUX = 2, PA_N0 = 3, PA_N1 = 4, PA_N2 = 5, PA_DDF_RAW = 6, PA_AUX_RAW = 7,
       PA_DG0 = 8, PA_DG1 = 9, PA_DG2 = 10, PA_AGG0 = 11, PA_AGG1 = 12, PA_AGG2 = 13, PA_DGN = 14, PA_DDDT = 15 };

// One dense layer in "fragment-major" packing (see pack_layer() in field_pack.hip):
//   wp[(((wave*NT + t)*ksteps + S)*64 + lane)*4 + r] = W[k = 8S + 4*(lane>>5) + r][n = (wave*NT + t)*32 + (lane&31)]
// so that one global_load_dwordx4 per lane yields the B operands of four
// v_mfma_f32_32x32x2_f32 k-steps, and a wave's load is 1 KiB contiguous.
struct LayerW {
    const float *wp;       // packed weights of the act-segment (K = 8*ksteps)
    const float *bias;     // [nout]
    int ksteps;            // super-steps of 8 k's
    int stash;             // -1, or index of the early partial (input-feature segment of a skip layer) to add
};

struct StashW {
    const float *wp;       // packed weights of the input-feature segment
    int col0;              // first act column of the segment (multiple of 8)
    int ksteps;
};

constexpr int kOperandsH16 = 4;
inline bool plain16(int operands) { return operands == 1 || operands == kOperandsH16; }      // one 16-bit plane: bf16's tile geometry

struct EncodeDesc {
    int E, Ed;             // embed_pos_rank, embed_dir_rank
    int KH, KD;            // padded half-widths: roundup(3E,4), roundup(3Ed,4)
    float lowpass[10];     // get_lowpass_scale per frequency
};

// Distance trunk of NeDDF (neddf.py:193-241): PE -> n_layers x (LinearGrad + activation) with
// (value, d/dx, d/dy, d/dz) rows -> distance / aux-gradient heads -> density, normal.
struct DdfArgs {
    const float *pos, *dir, *var;
    int64_t n_points;
    EncodeDesc enc;
    int n_layers;
    int activation, density_activation;
    LayerW layer[kMaxLayers];
    int n_stash;
    StashW stash[kMaxStash];
    int width;                            // engine width: hidden width padded to 128 / 256 / 384 / 512 (padding = zero weights: exact)
    const float *w_ddf_out, *w_aux_out;   // [width] each
    float b_ddf_out, b_aux_out;
    float d_near, aux_grad_scale;
    int operands;                         // 0 fp32 (32x32x2 f32 MFMA), 1 bf16, 2 split fp16 (three fp16 products per multiply-add), 3 fp32 with
                                          // three-term bf16 products (OpsF32x3T: reverse-mode distance + colour kernels only), 4 = kOperandsH16
                                          // plain fp16 (NEDDF_DTYPE_F16; the value 3 was taken), see tile_engine.h
    int neus;                             // 1: NeuS sdf trunk (neus.py:118-145): plain PE, no heads, sdf = feature 0
    float neus_v10;                       // variance * 10
    float *scratch;                       // per-workgroup stash area
    // reverse-mode distance gradient (ddf_rev_kernel, eval-minimal): transposed weights and a per-workgroup scratch
    const float *wT[kMaxLayers];          // [l >= 1] packed (hidden rows of W_l)^T, width x width
    const float *wT_pe0;                  // packed [width x 64]: W_0^T (engine column order of the encoding)
    const float *wT_pe_skip[kMaxStash];   // ... and the encoding rows^T of the skip layer that owns stash[s]
    int skip_layer;                       // a trunk layer whose input is cat([encoding, h]) (the last one), or -1
    int ks_hidden;                        // super-steps of a width-wide product under this operand policy
    float *rev_scratch;                   // per workgroup: y' of every layer [n_layers][P][width] + encoding Jacobian, copy and parked gradient [P][192]
    int *sched;                           // [0] tile queue head (zeroed before each launch)
    int sched_flags;                      // bit 1: dynamic tile queue (always set by the library); operands == 3: kSchedL2* below
    float *features;                      // [n_points][feat_rows][width]
    int feat_rows;                        // 1 (value row) or 4 (value + Jacobian rows)
    float *ptaux;                         // [n_points][kPtAux]
    float *distance, *density, *aux_grad; // optional outputs [n_points]
    RaySrc rays;                          // rays.rd != NULL: pos / dir / var are NULL, the points come from the rays (ddf_rev_kernel)
    unsigned long long *stamps = nullptr; // -DNEDDF_STAMP builds only (`make stamp`, tools/stamp_timeline.py): phase time stamps of a few workgroups
};
#ifndef NEDDF_STAMP_TILE_INDEX
#define NEDDF_STAMP_TILE_INDEX 6
#endif
constexpr int kStampBlocks = 8, kStampSlots = 160, kStampTile = NEDDF_STAMP_TILE_INDEX;      // workgroups stamped, stamps per wave, which tile of the workgroup
// (-DNEDDF_STAMP_TILE_INDEX=<k>, `make stamp STAMP_TILE=<k>`: a tile in the middle or at the end of a launch instead of its 7th)
constexpr int kStampWgTail = 4096;     // behind the stamps, four arrays of one word per workgroup: tiles it took | XCC_ID << 20 | HW_ID << 24; its first / last moment on the 100 MHz clock; its shader cycles between the two (tools/stamp_tiles.py)
constexpr int kStampPairTiles = 4;     // NEDDF_STAMP_PAIRS builds: tiles kStampTile .. + 3 of workgroups {0..3, 256..259} (a CU's two workgroups), slot 0 = HW_ID

// Colour trunk of NeDDF (neddf.py:243-300).
struct ColArgs {
    const float *pos, *dir, *var;
    int64_t n_points;
    EncodeDesc enc;
    int n_layers;                         // hidden layers (NeDDF: col_layer_count - 1, NeuS: col_layer_count)
    int activation;
    int mode;                             // 0 NeDDF inputs [embed_pos | embed_dir | normal], 1 NeuS inputs [pos | gradient | embed_dir]
    int final_act;                        // activation id applied to the 3 outputs (NeuS, neus.py:150-152) or -1
    int operands;                         // as DdfArgs::operands
    int width;                            // as DdfArgs::width
    int ksteps_a;                         // super-steps of layer 0's small-input segment [pe_pos | pe_dir | normal]
    const float *wp_a;                    // its packed weights
    LayerW layer[kMaxLayers];             // layer[0] = feature segment of layer 0
    const float *w_out;                   // [width][3] row-major (layer_col_out.weight)
    float b_out[3];
    const float *features;                // from DdfArgs
    int feat_rows;
    const float *ptaux;
    int *sched;                           // as DdfArgs::sched
    int sched_flags;
    float *color;                         // [n_points][3]
    int rays;                             // 1: pos / var / dir are read from the per-point record (PA_R_*), the pointers above are NULL
    float *penalty;                       // [n_points] (full mode) or NULL
    float distance_range_max;
    float penalty_weight[6];
    int penalty_has[6];
    unsigned long long *stamps = nullptr; // -DNEDDF_STAMP builds only: phase time stamps of the colour kernel (NEDDF_STAMP_FILE_COL, tools/stamp_timeline_col.py)
};

// Plain NeRF field (nerf.py:107-165), value rows only.
struct NerfArgs {
    const float *pos, *dir, *var;
    int64_t n_points;
    EncodeDesc enc;
    int n_layers;
    int activation, density_activation;
    LayerW layer[kMaxLayers];
    int n_stash;
    StashW stash[kMaxStash];              // [0..] skip partials, last = colour-head dir partial
    int col_stash;                        // stash index of the colour head's dir segment
    const float *w_density;               // [width]
    float b_density;
    LayerW col0;                          // outL_color.0: layer_width (+dir) -> layer_width / 2, padded to HC = a multiple of 128 columns
    const float *w_col1;                  // [3][HC] (nn.Linear layout, zero-padded)
    float b_col1[3];
    int operands;                         // as DdfArgs::operands
    int width;                            // as DdfArgs::width
    float *scratch;
    float *density, *color;
};

struct CameraArg {
    float R[9], T[3], calib[4];
};
// NEDDF_UV_CAMERA_TABLE: a camera per row.  cameras [n_cameras] rows of 16 floats in CameraArg's own layout, view [n] the camera
// of row b -- both DEVICE memory.  cameras == nullptr: no table, the call has one camera (or a ray bundle).
struct CameraTableArg {
    const float *cameras;
    const int32_t *view;
    int32_t n_cameras;
};

size_t field_lds_bytes(int mt);
void launch_ddf(const DdfArgs &a, int grid, hipStream_t s);
void launch_ddf_rev(const DdfArgs &a, int grid, hipStream_t s);
size_t ddf_rev_scratch_floats_per_wg(int n_layers, int points, int width);
int ddf_rev_points(int operands, int width);        // sample points per tile of ddf_rev_kernel under an operand policy / engine width
int ddf_rev_wgs_per_cu(int operands, int width);
void launch_col(const ColArgs &a, int grid, bool rows4, hipStream_t s);
void launch_nerf(const NerfArgs &a, int grid, hipStream_t s);
int ddf_points_per_tile(int operands, int width);
int col_points_per_tile(bool rows4, int operands, int width);
int nerf_points_per_tile(int width);
int nerf_wgs_per_cu(int width);
int field_wgs_per_cu(int operands, int width);
int col_wgs_per_cu(int operands, int width);

// uv_type: the element type 0..4 (the table flag already taken off); with a table (element types 0..3) cam is not read
void launch_raygen(const void *uv, int uv_type, int64_t n, const CameraArg &cam, const CameraTableArg &table, float *dir, float *orig,
                   hipStream_t s);
void launch_sample_coarse(const float *U, int64_t n, int S1, float near_, float far_, float *dists, hipStream_t s);
void launch_sampling(const float *rd, const float *ro, const float *view, const float *dists, int64_t n, int S, double radius,
                     float *pos, float *dir, float *var, hipStream_t s);
void launch_ndc(const float *rd, const float *ro, int64_t n, float width, float height, float fx, float fy, float near_, float *nd,
                float *no, hipStream_t s);
// ld: row stride of dens / col / nrm in samples (0: S; S - 1 where the field evaluated RaySrc::Se = S - 1 samples per ray)
void launch_composite(const float *dists, const float *dens, const float *col, int64_t n, int S, float max_dist,
                      float *w, float *depth, float *color, float *trans, int *nan_flag, hipStream_t s, int ld = 0);
// sum_j weight[b, j] * nrm[b, j] with launch_composite's weights (render_kernels.hip composite_normal_kernel); nrm [n, ld, 3], normal [n, 3]
void launch_composite_normal(const float *dists, const float *dens, const float *nrm, int64_t n, int S, float *normal, hipStream_t s, int ld = 0);
// [n, 3] position gradient / normal out of the per-point record of a distance-trunk launch (either may be NULL)
void launch_surface_gather(const float *ptaux, int64_t n, int neus, float *dgrad, float *normal, hipStream_t s);
void launch_integrate_penalty(const float *dists, const float *pen, int64_t n, int S, float *out, hipStream_t s);
void launch_resample(const float *dists, float *weights, const float *U, int64_t n_rays, int n, int nf, int cat,
                     float *out, int64_t *ids, int *flag, int64_t group, int64_t offset, hipStream_t s);

// Surface extraction (mesh_kernels.hip): a [nz][ny][nx] volume on the lattice lo .. hi (np.linspace per axis, x fastest)
constexpr int kMcThreads = 256;          // lattice points per workgroup of the count / vertex / triangle kernels
constexpr int kMcScanThreads = 1024;     // the one workgroup of the block-total scan
struct McGrid {
    const float *vol;                    // [nz][ny][nx] (NULL for grid_points_kernel)
    int nx, ny, nz;
    int64_t n;                           // nx * ny * nz
    float iso;
    double lo[3], hi[3];
};
static inline int64_t mc_blocks(int64_t n) { return (n + kMcThreads - 1) / kMcThreads; }
void launch_grid_points(const McGrid &g, int64_t first, int64_t n, float *pos, float *dir, float *var, hipStream_t s);
// per-block vertex / triangle totals (vblk / tblk [mc_blocks(n) + 1]) and the crossed-edge byte of every lattice point;
// launch_scan_totals on each turns them into block bases, [mc_blocks(n)] = the vertex / triangle count of the mesh
void launch_mc_count(const McGrid &g, unsigned char *mask, int64_t *vblk, int64_t *tblk, hipStream_t s);
void launch_mc_vertices(const McGrid &g, const unsigned char *mask, const int64_t *vblk, int32_t *vbase, float *vertices, hipStream_t s);
void launch_mc_triangles(const McGrid &g, const unsigned char *mask, const int64_t *tblk, const int32_t *vbase, int32_t *tris,
                         hipStream_t s);
// geometric vertex normals of an indexed mesh; acc: workspace of (3 V + 1) 64-bit words
void launch_mesh_normals(const float *vertices, int64_t V, const int32_t *tris, int64_t T, unsigned long long *acc, float *normals, hipStream_t s);

// Mesh clean-up (mesh_kernels.hip): connected components by union-find on the device, order-preserving compaction.
// Every launcher takes V >= 0 and T >= 0 and launches nothing over an empty range.
constexpr int kCcBatch = 4;              // union-find rounds between two reads of the "changed" words (one stream synchronise each)
constexpr int kCcMaxRounds = 256;        // neddf_mesh_components gives up (NEDDF_EUNSUPPORTED) after this many rounds
// parent[v] = v, used[v] = 0; then used[v] = 1 for the vertices of the valid triangles
void launch_cc_init(int32_t *parent, unsigned char *used, int64_t V, const int32_t *tris, int64_t T, hipStream_t s);
// one round: hook (per triangle, atomicMin) and one pointer jump (per vertex); *changed is set when either did anything
void launch_cc_round(int32_t *parent, int64_t V, const int32_t *tris, int64_t T, int *changed, hipStream_t s);
// one workgroup: a[0..n) -> exclusive prefix sums in place, a[n] = the total: the block totals of every count kernel (block_scan.h)
// -> block bases, the grand total behind them
void launch_scan_totals(int64_t *a, int64_t n, hipStream_t s);
// Chebyshev dilation by d cells of an [nz][ny][nx] byte grid held in a (b: as large, scratch): one launch per axis, each clipped to
// the grid.  Returns the buffer that holds the result (a itself for d <= 0).
const unsigned char *launch_dilate(unsigned char *a, unsigned char *b, int nx, int ny, int nz, int d, hipStream_t s);
// roots (parent[v] == v, used) -> dense labels in vertex order; vertex / triangle labels and the triangle count of every component.
// blk: [mc_blocks(V) + 1], blk[mc_blocks(V)] = the number of components afterwards
void launch_cc_labels(const int32_t *parent, const unsigned char *used, int64_t V, const int32_t *tris, int64_t T, int64_t *blk,
                      int32_t *vertex_label, int32_t *triangle_label, int64_t *component_triangles, hipStream_t s);
// kept = keep flag set and every index in [0, V): used[] of their vertices, per-block totals of both, scanned
// (vblk [mc_blocks(V) + 1], tblk [mc_blocks(T) + 1], the totals behind the bases)
void launch_compact_count(const int32_t *tris, int64_t T, int64_t V, const unsigned char *keep, unsigned char *used, int64_t *vblk,
                          int64_t *tblk, hipStream_t s);
void launch_compact_write(const float *vertices, int64_t V, const int32_t *tris, int64_t T, const unsigned char *keep,
                          const unsigned char *used, const int64_t *vblk, const int64_t *tblk, int32_t *vmap, float *out_vertices,
                          int32_t *out_tris, hipStream_t s);

// Brick-wise surface extraction (mesh_kernels.hip): the fine lattice of McGrid cut into bricks of B^3 cells, brick (bx, by, bz) at linear
// index (bz nby + by) nbx + bx, its lattice (B+1)^3 points at local index (lz (B+1) + ly)(B+1) + lx; the last brick of an axis may be
// partial (its points past the fine lattice are padding).
constexpr int kBrickMin = 2, kBrickMax = 16, kBrickMaxDilate = 4;
constexpr int kBrickMaxPoints = (kBrickMax + 1) * (kBrickMax + 1) * (kBrickMax + 1);
struct BrickGrid {
    McGrid g;                            // the fine lattice; vol unused
    int B, P;                            // cells per brick and axis; (B + 1)^3
    int nbx, nby, nbz;                   // ceil((n - 1) / B) per axis
    int64_t nb;                          // nbx * nby * nbz
};
struct BrickMesh {
    BrickGrid bg;
    const float *values;                 // [M][P]
    const int32_t *ids;                  // [M], strictly ascending brick indices
    const int32_t *slot_map;             // [nb]: the rank of a brick in ids, or -1
    int64_t M;
};
// the (nbx+1)(nby+1)(nbz+1) fine lattice points at index min(b B, n - 1) per axis, x fastest
void launch_coarse_points(const BrickGrid &bg, int64_t first, int64_t n, float *pos, float *dir, float *var, hipStream_t s);
// points first .. first + n of the [M][P] brick lattices (padding: the clamped lattice point); brick_pad writes NaN over the padding's results
void launch_brick_points(const BrickGrid &bg, const int32_t *ids, int64_t first, int64_t n, float *pos, float *dir, float *var, hipStream_t s);
void launch_brick_pad(const BrickGrid &bg, const int32_t *ids, int64_t first, int64_t n, float *out, hipStream_t s);
// coarse: [nbz+1][nby+1][nbx+1]; flag_a / flag_b: nb bytes each (workspace); blk: [mc_blocks(nb) + 1], the number of active bricks behind
// the block bases afterwards; slot_map [nb], ids [capacity nb]
void launch_brick_select(const float *coarse, int nbx, int nby, int nbz, float iso, float band, int dilate, unsigned char *flag_a,
                         unsigned char *flag_b, int64_t *blk, int32_t *slot_map, int32_t *ids, hipStream_t s);
// *bad = 1 unless ids is strictly ascending inside [0, nb) and slot_map is exactly its inverse (-1 elsewhere)
void launch_brick_check(const BrickMesh &k, int *bad, hipStream_t s);
// mask [M][P]: the crossed edges each brick lattice point OWNS; vblk / tblk [M + 1]: per-brick vertex / triangle totals (launch_scan_totals next)
void launch_brick_mc_count(const BrickMesh &k, unsigned char *mask, int64_t *vblk, int64_t *tblk, hipStream_t s);
void launch_brick_mc_vertices(const BrickMesh &k, const unsigned char *mask, const int64_t *vblk, int32_t *vbase, float *vertices,
                              int64_t *vertex_key, hipStream_t s);
void launch_brick_mc_triangles(const BrickMesh &k, const unsigned char *mask, const int64_t *tblk, const int32_t *vbase, int32_t *tris,
                               int64_t *triangle_key, hipStream_t s);

// Empty-space skipping (occupancy_kernels.hip): an R^3 bitfield over the box lo .. hi, bit (z R + y) R + x of cell (x, y, z) in
// 32-bit words; classification of sample points against it and order-preserving compaction of the kept ones.
constexpr int kOccThreads = 1024;        // points per workgroup of the count / gather kernels (16 waves: block_rank offsets)
constexpr int kOccMaxRes = 1024, kOccMaxDilate = 4;
struct OccGrid {
    const uint32_t *bits;
    int res;
    float lo[3], inv_cell[3];
};
static inline int64_t occ_words(int R) { return ((int64_t)R * R * R + 31) >> 5; }
static inline int64_t occ_blocks(int64_t n) { return (n + kOccThreads - 1) / kOccThreads; }
// vol: [R+1]^3 corner densities; cell_a / cell_b: R^3 bytes each (workspace); bits: occ_words(R) words;
// blk: [mc_blocks(occ_words(R)) + 1], the population count behind the block bases afterwards
void launch_occ_build(const float *vol, int R, float threshold, int dilate, unsigned char *cell_a, unsigned char *cell_b, uint32_t *bits,
                      int64_t *blk, hipStream_t s);
void launch_occ_classify(const OccGrid &g, const float *pos, int64_t n, unsigned char *keep, hipStream_t s);
// kept points per block, scanned (launch_scan_totals): blk [occ_blocks(n) + 1], blk[occ_blocks(n)] = the number of kept points
void launch_occ_count(const unsigned char *keep, int64_t n, int64_t *blk, hipStream_t s);
// gather: rows of the kept points, order preserved, and their old index; scatter: compact results back to rows index[k] < n (any may be NULL)
void launch_occ_gather(const unsigned char *keep, const float *pos, const float *dir, const float *var, int64_t n, const int64_t *blk,
                       float *cpos, float *cdir, float *cvar, int32_t *index, hipStream_t s);
void launch_occ_scatter(const int32_t *index, int64_t m, int64_t n, const float *cdens, const float *ccol, const float *cnrm, float *dens,
                        float *col, float *nrm, hipStream_t s);

// Sphere tracing (trace_kernels.hip): per-ray state in flat arrays -- t, t_lo, dist float [n], status uint8 [n], steps int32 [n].
enum { kTraceActive = 0, kTraceHit = 1, kTraceMiss = 2, kTraceExhausted = 3, kTraceInvalid = 4 };
struct TraceState {
    float *t, *t_lo, *dist;
    unsigned char *status;
    int32_t *steps;
};
// t = t_lo = t_near, steps = 0, dist = NaN, status ACTIVE (INVALID for a non-finite origin or direction component)
void launch_trace_begin(const float *ro, const float *rd, int64_t n, float t_near, const TraceState &st, hipStream_t s);
// Order-preserving compaction of the selected rays: bisect == 0 the ACTIVE ones at depth t, bisect != 0 the HIT ones with t_lo < t at
// depth 0.5 (t_lo + t).  index [n] int32, pos [n, 3] = o + depth * d (a rounded product, then a rounded sum);
// blk [occ_blocks(n) + 1], blk[occ_blocks(n)] = the number of selected rays afterwards
void launch_trace_compact(const float *ro, const float *rd, int64_t n, const TraceState &st, int bisect, int64_t *blk, int32_t *index,
                          float *pos, hipStream_t s);
// one sphere-tracing step of rays index[k] < n with the distances D[k], k < m
void launch_trace_advance(const int32_t *index, const float *D, int64_t m, int64_t n, float threshold, float step_scale, float min_step,
                          float t_far, const TraceState &st, hipStream_t s);
// one bisection round of rays index[k] < n with the distances D[k] at their midpoints, k < m
void launch_trace_bisect_update(const int32_t *index, const float *D, int64_t m, int64_t n, float threshold, const TraceState &st, hipStream_t s);
// ACTIVE -> EXHAUSTED
void launch_trace_finish(unsigned char *status, int64_t n, hipStream_t s);
// dir = (1, 0, 0), var = 0 for n rows: the constant field inputs of a distance-only evaluation
void launch_trace_unit_inputs(float *dir, float *var, int64_t n, hipStream_t s);

// Distances between surfaces (geom_kernels.hip): area-weighted surface samples of an indexed mesh, exact nearest neighbours by brute
// force and through a uniform grid.  Every launcher takes counts >= 0 and launches nothing over an empty range.
constexpr int kNnMaxAxis = 1024;                         // cells per axis of the grid (the stopping rule's error bound assumes it)
constexpr int64_t kNnMaxCells = (int64_t)1 << 24;        // cells in all: 64 MiB of cell_start
struct NnGrid {
    int n[3];                            // cells per axis (x, y, z); cell (x, y, z) at linear index (z n[1] + y) n[0] + x
    float lo[3], inv_cell[3];            // cell = (p - lo) * inv_cell per axis, clamped to the grid; inv_cell 0 for a zero-extent axis
    float safe_cell;                     // 0.99 * the smallest cell edge over the axes with an extent (FLT_MAX when there is none)
};
// the cell of coordinate p along one axis: two rounded fp32 operations, monotone in p, clamped to the grid (NaN: 0)
__device__ __forceinline__ int grid_axis_cell(float p, float lo, float inv_cell, int g)
{
    const float f = __fmul_rn(__fsub_rn(p, lo), inv_cell);
    return f >= (float)g ? g - 1 : (f > 0.f ? (int)f : 0);
}
// per-block sample totals of the triangles, scanned: blk [mc_blocks(T) + 1], blk[mc_blocks(T)] = the number of samples afterwards
void launch_sample_count(const float *v, int64_t V, const int32_t *tri, int64_t T, double density, uint32_t seed, int64_t *blk, hipStream_t s);
// points [N, 3] and triangle_id [N], triangle-major (N < 2^31: the caller has read the total)
void launch_sample_write(const float *v, int64_t V, const int32_t *tri, int64_t T, double density, uint32_t seed, const int64_t *blk, float *points,
                         int32_t *triangle_id, hipStream_t s);
void launch_nn_brute(const float *q, int64_t nq, const float *p, int64_t np, float *d2, int32_t *index, hipStream_t s);
// cell_of [np], count [cells] (workspace); blk [mc_blocks(cells) + 1], blk[mc_blocks(cells)] = the number of finite targets afterwards;
// cell_start [cells + 1], order [capacity np]
void launch_nn_grid_build(const NnGrid &g, const float *p, int64_t np, int32_t *cell_of, int32_t *count, int64_t *blk, int32_t *cell_start,
                          int32_t *order, hipStream_t s);
void launch_nn_grid_query(const NnGrid &g, const float *q, int64_t nq, const float *p, int64_t np, const int32_t *cell_start, const int32_t *order,
                          float *d2, int32_t *index, hipStream_t s);

// Ray casting on meshes (raycast_kernels.hip): the first watertight hit of every ray by brute force and through the uniform grid of
// NnGrid's cells, each listing the triangles whose box, widened by 2 pad, overlaps it; list G holds the triangles that leave the box.
struct RcGrid {
    NnGrid nn;
    float pad, pad2;                     // pad and 2 pad
    float wlo[3], whi[3];                // the box widened by 2 pad: (float)h_lo - pad2 and (float)h_hi + pad2, one rounded operation each
    float far_origin;                    // a ray whose origin has a larger |coordinate| visits every triangle instead of walking the grid
    double lo[3], edge[3];               // the walk's cells: (double)nn.lo and 1 / (double)nn.inv_cell (0 for an axis without extent)
};
void launch_raycast_brute(const float *ro, const float *rd, int64_t nr, const float *v, int64_t V, const int32_t *tri, int64_t T, float t_min,
                          float t_max, float pad, float *t, int32_t *triangle, float *b1, float *b2, hipStream_t s);
// count [G + 1] (workspace): the pairs of every list; blk [mc_blocks(G + 1) + 1], blk[mc_blocks(G + 1)] = the number of pairs afterwards
void launch_raycast_grid_count(const RcGrid &g, const float *v, int64_t V, const int32_t *tri, int64_t T, int32_t *count, int64_t *blk, hipStream_t s);
// after launch_raycast_grid_count and once the total is known to fit int32 and items: cell_start [G + 2], items [total]
void launch_raycast_grid_place(const RcGrid &g, const float *v, int64_t V, const int32_t *tri, int64_t T, int32_t *count, const int64_t *blk,
                               int32_t *cell_start, int32_t *items, hipStream_t s);
void launch_raycast_grid_query(const RcGrid &g, const float *ro, const float *rd, int64_t nr, const float *v, int64_t V, const int32_t *tri, int64_t T,
                               const int32_t *cell_start, const int32_t *items, int64_t n_items, float t_min, float t_max, float *t, int32_t *triangle,
                               float *b1, float *b2, hipStream_t s);

// Point-to-mesh distance (pointmesh_kernels.hip): the closest point of the closest triangle to every query, by brute force and through
// the lists of the ray-casting grid.
struct PmGrid {
    NnGrid nn;
    int walk;                            // 1: Chebyshev shells with the stopping rule; 0: every list once (include/neddf_hip.h says when)
};
void launch_point_mesh_brute(const float *q, int64_t nq, const float *v, int64_t V, const int32_t *tri, int64_t T, float *d2, int32_t *triangle, float *b1,
                             float *b2, hipStream_t s);
constexpr int kPmTableFloats = 20;       // floats per triangle of the table below (pointmesh_device.h: kPmVec float4)
// table [kPmTableFloats T] floats, 16-byte aligned (workspace): the per-triangle constants, written by a prepare launch in front of the query
void launch_point_mesh_grid_query(const PmGrid &g, const float *q, int64_t nq, const float *v, int64_t V, const int32_t *tri, int64_t T, float *table,
                                  const int32_t *cell_start, const int32_t *items, int64_t n_items, float *d2, int32_t *triangle, float *b1, float *b2,
                                  hipStream_t s);
// the table alone: [kPmTableFloats T] floats, 16-byte aligned (nothing is launched for T <= 0)
void launch_point_mesh_prepare(const float *v, int64_t V, const int32_t *tri, int64_t T, float *table, hipStream_t s);

// A linear BVH over the triangles and the point-to-mesh query through it (bvh_kernels.hip; include/neddf_hip.h states the arrays).
// keys int64 [T]: Morton code of the box centre (g: 1024 cells per axis) << 32 | triangle index; bit 62 set for an invalid triangle
void launch_bvh_keys(const NnGrid &g, const float *v, int64_t V, const int32_t *tri, int64_t T, int64_t *keys, hipStream_t s);
// keys sorted ascending -> leaf_tri [T], children [T - 1][2], boxes [2 T - 1][6]; parent [2 T - 1] and counter [T - 1] are workspace
void launch_bvh_build(const int64_t *keys, const float *v, int64_t V, const int32_t *tri, int64_t T, int32_t *leaf_tri, int32_t *children, float *boxes,
                      int32_t *parent, int32_t *counter, hipStream_t s);
// table [kPmTableFloats T] floats (workspace, written by a prepare launch in front of the query); visits [nq] or NULL
void launch_point_mesh_bvh_query(const float *q, int64_t nq, const float *v, int64_t V, const int32_t *tri, int64_t T, float *table, const int32_t *leaf_tri,
                                 const int32_t *children, const float *boxes, float *d2, int32_t *triangle, float *b1, float *b2, int32_t *visits,
                                 hipStream_t s);
// rays through the tree: the first hit (t, triangle, b1, b2), or with any_hit the flag `occluded` [nr] alone; visits [nr] or NULL
void launch_raycast_bvh(bool any_hit, const float *ro, const float *rd, int64_t nr, const float *v, int64_t V, const int32_t *tri, int64_t T,
                        const int32_t *leaf_tri, const int32_t *children, const float *boxes, float t_min, float t_max, float pad, float *t,
                        int32_t *triangle, float *b1, float *b2, uint8_t *occluded, int32_t *visits, hipStream_t s);

// Mesh simplification by vertex clustering (simplify_kernels.hip; include/neddf_hip.h states the contract).
// keys int64 [V]: cell of g (neddf_nn_grid_build's cell function) << 32 | vertex index; 2^62 | index for a non-finite vertex
void launch_simplify_keys(const NnGrid &g, const float *v, int64_t V, int64_t *keys, hipStream_t s);
// keys sorted ascending -> vertex_cluster [V], cluster_range [C][2] (the [begin, end) of each cluster in the sorted keys); workspace:
// head_of_vertex [V] bytes, run_start [V + 1], sblk / vblk [mc_blocks(V) + 1] each, sblk[mc_blocks(V)] = the number of clusters afterwards
void launch_simplify_clusters(const int64_t *keys, int64_t V, unsigned char *head_of_vertex, int32_t *run_start, int64_t *sblk, int64_t *vblk,
                              int32_t *vertex_cluster, int32_t *cluster_range, hipStream_t s);
// the (cluster, triangle) pairs of the valid triangles: pblk [mc_blocks(T) + 1], pblk[mc_blocks(T)] = the number of pairs afterwards;
// pairs [that number] = cluster << 32 | triangle, triangle-major
void launch_simplify_pair_count(const float *v, int64_t V, const int32_t *tri, int64_t T, const int32_t *vertex_cluster, int64_t *pblk, hipStream_t s);
void launch_simplify_pair_write(const float *v, int64_t V, const int32_t *tri, int64_t T, const int32_t *vertex_cluster, const int64_t *pblk, int64_t *pairs,
                                hipStream_t s);
// out [C][3]: the representative of every cluster; quadric != 0 reads the pairs sorted ascending
void launch_simplify_place(const int64_t *keys, int64_t V, const int32_t *cluster_range, int64_t C, const float *v, const int32_t *tri, int64_t T,
                           const int64_t *pairs, int64_t P, int quadric, double reg, float *out, hipStream_t s);
// attr [V][K] -> out [C][K]
void launch_simplify_attributes(const int64_t *keys, int64_t V, const int32_t *cluster_range, int64_t C, const float *attr, int K, float *out, hipStream_t s);
// mapped [T][3], lowest [T], key [T]; then, with order [T] = the triangles sorted by (lowest, key) (ties by index), keep [T]
void launch_simplify_triangles(const int32_t *tri, int64_t T, int64_t V, const int32_t *vertex_cluster, int32_t *mapped, int32_t *lowest, int64_t *key,
                               hipStream_t s);
void launch_simplify_unique(const int32_t *lowest, const int64_t *key, int64_t T, const int64_t *order, unsigned char *keep, hipStream_t s);

void launch_linear_grad(const float *x, const float *J, int64_t n, int cin, int ldx, int cout_block, int ksteps, const float *wp,
                        const float *bias, float *y, float *G, int ldo, int nvalid, int accumulate, int grid, hipStream_t s);
void launch_op_activation(int kind, const float *x, const float *J, int64_t N, int C, float *y, float *G, hipStream_t s);
void launch_op_pe(const float *x, const float *J, const float *scale, int64_t N, int E, float *y, float *G, hipStream_t s);
void launch_op_pe_weights(const float *var, int64_t N, int E, float *w, hipStream_t s);

}  // namespace neddf
