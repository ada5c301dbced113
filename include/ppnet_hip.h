/* ppnet_hip.h — C ABI of libppnet_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the two data-parallel loops of AdamQLMeng/PPNet.  The reference has no
 * FFI layer of its own (it is pure Python); each entry point below names the reference
 * interface it replaces (paths relative to the reference repo).  INTEGRATION.md shows the
 * ctypes binding a maintainer would add under EDaGe-PP/ and GenNet/.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller unless the comment says "host";
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous
 *     on that stream and never synchronise;
 *   - return value: PPN_OK or a negative PPN_E_* code; nothing throws or aborts;
 *   - no global mutable state: calls are re-entrant (constant tables are built once, lazily,
 *     under a lock);
 *   - points are (row, col) doubles; obstacles are [col, row, radius] doubles, as in the
 *     reference (EDaGe-PP/Path.py:495, MapGenerate.py:143);
 *   - R must be a multiple of 32 and 32 <= R <= 512.
 */
#ifndef PPNET_HIP_H
#define PPNET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPN_OK             0
#define PPN_E_INVALID     -1   /* bad argument (NULL where required, R not a multiple of 32, ...) */
#define PPN_E_HIP         -2   /* a HIP runtime call failed; see ppn_last_hip_error() */
#define PPN_E_UNSUPPORTED -3

/* fixed geometry of the generator (EDaGe-PP/MapGenerate.py:21-23, PathSeg.py:22-23) */
#define PPN_SEGS            10
#define PPN_POLY             5          /* degree-4 coefficients, highest power first */
#define PPN_PATH_POINTS   1000
#define PPN_BOUNDARY_POINTS 1100
#define PPN_DRAWS_PER_SEG 1002          /* [straight flag][1000 samples][end abscissa] */
#define PPN_DRAWS_PER_PATH (1 + PPN_SEGS * PPN_DRAWS_PER_SEG)
#define PPN_MAX_HULL        64
#define PPN_MAX_ISLES       16
#define PPN_MAX_POCKET      64          /* pocket obstacles per path */
#define PPN_POCKET_TRY_CAP 256          /* per-isle cap on set_obstacles iterations */
#define PPN_PLACE_TRY_CAP 4096          /* per-map cap on placement attempts */
#define PPN_MAX_WAYPOINTS 2048          /* extract_path step cap (replaces the 1 s wall-clock timeout) */

/* occupancy grid codes (u8) */
#define PPN_GRID_OBST   0
#define PPN_GRID_FREE 255
#define PPN_GRID_MARK 128               /* start / goal marker squares */

/* per-instance flag bits */
#define PPN_FLAG_POCKET_CAP   1u        /* reference would loop forever (Path.py:478) */
#define PPN_FLAG_PLACE_CAP    2u        /* reference: "Repeated over 1000000 times" (MapGenerate.py:60-62) */
#define PPN_FLAG_EMPTY_ISLE   4u        /* reference raises IndexError (Path.py:529) */
#define PPN_FLAG_HULL_CAP     8u        /* more than PPN_MAX_HULL hull vertices */
#define PPN_FLAG_ISLE_CAP    16u
#define PPN_FLAG_POCKET_FULL 32u        /* more than PPN_MAX_POCKET pocket obstacles */
#define PPN_FLAG_CORRIDOR_PASS 64u       /* informational: an obstacle may touch the corridor, the raster ran its compose pass */
#define PPN_FLAG_POCKET_DRAWS 128u       /* caller-fed pocket draws ran out (pocket_stride too small): the path's pocket
                                            obstacles are not the reference's — call again with a larger buffer
                                            (3 * PPN_POCKET_TRY_CAP * PPN_MAX_ISLES floats always suffice) */

/* ABI version of this header.  ppn_version() returns the PPN_ABI_VERSION the LIBRARY was built with; a caller compares the two
 * before its first real call (ppnet_amd/_lib.py does, INTEGRATION.md shows the check) — argument lists are plain pointers and
 * sizes, so a caller built against another header would link and pass, say, a batch size where a workspace pointer is expected.
 * Bumped whenever an entry point's argument list changes or an entry point is removed: 100 = rounds 1-3; 101 = round 4
 * (ppn_conv3x3_relu_classify2_bf16 gained `partial`); 105 = round 5; 106 = ppn_swin_wmsa_fwd; 107 = ppn_upsample2x_concat_nhwc;
 * 108 = ppn_mhsa_fwd; 109 = ppn_mhsa_bwd, ppn_mhsa_bwd_workspace; 110 = ppn_swin_wmsa_bwd, ppn_swin_wmsa_bwd_workspace;
 * 111 = ppn_na2d_bwd_vpad, ppn_na2d_bwd_vpad_workspace.  ppn_resize_ce_workspace, ppn_resize_ce_fwd and ppn_resize_ce_bwd joined at
 * 111 too, and so did ppn_seg_eval and ppn_augment_params / ppn_augment_codes / ppn_augment_rgb: new symbols change no existing
 * argument list and remove nothing, which is all the version guards against.  ppn_ohem_ce_workspace, ppn_ohem_ce_fwd and
 * ppn_ohem_ce_bwd joined at 111 in the same way, and so did ppn_resize_dice_workspace, ppn_resize_dice_fwd and ppn_resize_dice_bwd, and
 * ppn_upsample2x_nhwc_bwd, ppn_upsample2x_concat_nhwc_bwd and ppn_resize_concat_nhwc_bwd, and ppn_residual_layernorm_train_fwd,
 * ppn_residual_layernorm_bwd_workspace and ppn_residual_layernorm_bwd, and ppn_patch_merge_ln_fwd, ppn_patch_merge_ln_bwd_workspace,
 * ppn_patch_merge_ln_bwd, ppn_patch_merge_ln_rows and ppn_patch_merge_ln_max_blocks, and ppn_seg_tta, and ppn_gennet_stem_train_workspace,
 * ppn_gennet_stem_train_fwd, ppn_gennet_stem_train_bwd, ppn_gennet_stem_train_tile and ppn_gennet_stem_train_max_blocks, and
 * ppn_gennet_tail_train_workspace, ppn_gennet_tail_train_fwd, ppn_gennet_tail_train_bwd, ppn_gennet_tail_train_tile and
 * ppn_gennet_tail_train_max_blocks, and ppn_gennet_s2_tile, ppn_gennet_s2_max_blocks, ppn_gennet_s2_wgrad_workspace, ppn_gennet_s2_down,
 * ppn_gennet_s2_up and ppn_gennet_s2_wgrad, and ppn_wmsa_fwd. */
#define PPN_ABI_VERSION 111
int         ppn_version(void);
const char* ppn_error_string(int code);
int         ppn_last_hip_error(void);   /* hipError_t of the most recent PPN_E_HIP on this thread */

/* Host-side constant: the 4 x 1000 least-squares operator W with Poly[0..3] = W . y for
 * x = arange(1000)/100, degree 4 (replaces the per-call np.polyfit at PathSeg.py:24; the
 * constant coefficient is overwritten with 0 at PathSeg.py:28 so its row is not needed).
 * `out` is a HOST buffer of 4*1000 doubles. */
int ppn_polyfit_table(double* out);

/* ---------------------------------------------------------------------------------------------
 * Stage A — target paths.  Replaces PathGroup.generate (PathGenerate.py:33-50) =
 * Path.generate + Path.draw_boundary + Path.path_obstacles (Path.py:78-98, 318-356, 144-155,
 * 113-142, 157-193, 388-404, 463-537) for n_paths independent paths.
 * Optional outputs may be NULL. */
typedef struct ppn_paths {
    double*   seg_poly;         /* [n][10][5]                                          */
    double*   seg_endpoint;     /* [n][10]                                             */
    double*   seg_rotation;     /* [n][10]   PathSeg.Rotation after Path.transform      */
    double*   seg_translation;  /* [n][10][2]                                          */
    double*   seg_length;       /* [n][10]   optional                                  */
    int32_t*  seg_straight;     /* [n][10]                                             */
    double*   segpoint_world;   /* [n][11][2]                                          */
    double*   pathpoint_world;  /* [n][1000][2]                                        */
    double*   boundary_world;   /* [n][1100][2] optional (Path.BoundaryPoint)          */
    uint32_t* canvas_bits;      /* [n][(2R*2R)/32] optional: pre-rotation corridor canvas, bit = row*2R+col */
    double*   hull_raw;         /* [n][64][2] optional: integer hull before normalisation */
    double*   hull;             /* [n][64][2] Path.ConvexHull after space_normalization */
    int32_t*  hull_n;           /* [n]                                                 */
    double*   rotation;         /* [n]  Path.Rotation (degrees)                        */
    double*   trans_rc;         /* [n][2] (t_row, t_col); Path.Translation = [t_col, t_row] */
    double*   segpoint_image;   /* [n][11][2]  Path.SegPointImage                      */
    double*   pathpoint_image;  /* [n][1000][2] Path.PathPoint after normalisation      */
    uint32_t* space_bits;       /* [n][R*R/32] Path.Space as a bit mask, bit = row*R+col */
    int32_t*  isles;            /* [n][16][2] slice bounds into PathPoint              */
    int32_t*  n_isles;          /* [n]                                                 */
    double*   obstacles;        /* [n][64][3] Path.obstacles as [col,row,r]            */
    int32_t*  n_obstacles;      /* [n]                                                 */
    double*   length;           /* [n] Path.Length                                     */
    int32_t*  straight;         /* [n] path-level is_straight                          */
    uint32_t* flags;            /* [n] PPN_FLAG_*                                      */
    double*   max_step_px;      /* [n] largest distance between consecutive path points (and the last one to
                                   the end point), in pixels; stage B uses it to prove that an obstacle cannot
                                   touch the corridor and skip the compose for it */
    double*   seg_grad;         /* [n][10][2] optional: PathSeg.GradSt, GradEnd (PathSeg.py:43-47)      */
    int32_t*  pocket_draws_used;/* [n] optional: torch.rand draws consumed by set_obstacles           */
} ppn_paths_t;

/* draws        : [n_paths][PPN_DRAWS_PER_PATH] uniform doubles in the fixed layout
 *                [path straight][seg0: flag, 1000 samples, end]...[seg9] or NULL = Philox4x32-10
 *                keyed by (seed, stream PATH, first_path_id + p, draw index);
 * pocket_draws : [n_paths][pocket_stride] uniform floats consumed in torch.rand order by
 *                set_obstacles, or NULL = Philox (stream POCKET). */
int ppn_edage_paths(int32_t n_paths, uint64_t first_path_id, int32_t R, double map_size,
                    double clearance, uint64_t seed,
                    const double* draws, const float* pocket_draws, int32_t pocket_stride,
                    const ppn_paths_t* out, void* stream);

/* Same, with the path-level is_straight flag supplied by the caller (Path(is_straight=...), Path.py:53):
 * force_straight[n] int8, -1 = decide from draw 0 as PathGroup.generate does, 0 / 1 = forced. May be NULL. */
int ppn_edage_paths_ex(int32_t n_paths, uint64_t first_path_id, int32_t R, double map_size,
                       double clearance, uint64_t seed,
                       const double* draws, const float* pocket_draws, int32_t pocket_stride,
                       const int8_t* force_straight, const ppn_paths_t* out, void* stream);

/* Same, with the hull's first vertex supplied by the caller: hull_start[n] int32 = index into the canonical vertex cycle
 * (lexicographically smallest lattice point first, counter-clockwise) at which the cycle is to begin, -1 = canonical; may be
 * NULL.  scipy.spatial.ConvexHull (Qhull, Path.py:392-393) returns the same cycle from an implementation-defined start, and
 * Path.search_isle / Path.set_obstacles (Path.py:463-537) walk the hull edges — and draw torch.rand — in that order: a caller
 * that replays the reference's random streams computes Qhull's start on the host and passes it here (dropin/Path.py). */
int ppn_edage_paths_ex2(int32_t n_paths, uint64_t first_path_id, int32_t R, double map_size,
                        double clearance, uint64_t seed,
                        const double* draws, const float* pocket_draws, int32_t pocket_stride,
                        const int8_t* force_straight, const int32_t* hull_start,
                        const ppn_paths_t* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Stage B — maps.  Replaces the body of MapGenerate.generate (MapGenerate.py:48-124) incl.
 * Path.boundary_check (Path.py:100-111), generate_map_randomly (MapGenerate.py:126-151), the
 * obstacle raster (Path.plot_obstacles, Path.py:36-49 — explicit rule) and
 * add_init_end_single (process_map.py:119-145).  Map m uses target path m / placements. */
typedef struct ppn_maps {
    uint8_t*  grid;             /* [n][R][R]  PPN_GRID_* codes                          */
    double*   angle;            /* [n]  degrees, U(-180,180)                           */
    int32_t*  translation;      /* [n][2] as drawn (MapGenerate.py:64-65)              */
    int32_t*  attempts;         /* [n]  placement attempts used                        */
    double*   segpoint;         /* [n][11][2] label                                     */
    double*   pathpoint;        /* [n][1000][2] label, optional                         */
    uint8_t*  accept;           /* [n][K] clearance-filter mask of the K random obstacles, optional */
    double*   obstacles;        /* [n][K+64][3] kept random obstacles then pocket obstacles */
    int32_t*  n_obstacles;      /* [n][2] (total, of which random)                      */
    uint32_t* flags;            /* [n]                                                  */
    double*   records;          /* [n][PPN_RECORD_WIDTH] optional: angle, flags, translation[2], segpoint[11][2] as doubles —
                                   the fixed-size per-instance record the ranks all-gather at the end of a batch
                                   (SURVEY 8e), written by the kernel so that no pack pass precedes the collective */
} ppn_maps_t;
#define PPN_RECORD_WIDTH 26

/* place_draws : [n_maps][3] (angle, t0, t1 uniforms of the ACCEPTED attempt) or NULL = Philox
 *               rejection loop (stream PLACE, draw index 3*attempt+i);
 * obst_draws  : [n_maps][3K] in the reference's draw order (K x, K y, K size) or NULL = Philox. */
int ppn_edage_maps(const ppn_paths_t* paths, int32_t n_paths, int32_t placements,
                   uint64_t first_map_id, int32_t R, double map_size, double obstacles_size,
                   int32_t K, double clearance, uint64_t seed,
                   const double* place_draws, const double* obst_draws,
                   const ppn_maps_t* out, void* stream);

/* The per-map label images written right after generation (process_map.py:148-191), for the n = n_paths*placements
 * maps of a ppn_edage_maps call:
 *   mask_path [n][R][R] u8 : generate_gen_path — every 5th label point with 0 < round(p) < bound set to 255;
 *   mask_space[n][R][R] u8 : generate_seg_space — the target path's Space rotated by -angle and translated, {0,1}.
 * `bound` is the reference's hard-coded 224 (pass R for other resolutions). Either output may be NULL. */
int ppn_label_masks(const ppn_paths_t* paths, const ppn_maps_t* maps, int32_t n_paths, int32_t placements,
                    int32_t R, int32_t bound, uint8_t* mask_path, uint8_t* mask_space, void* stream);

/* The two halves of ppn_edage_maps as separate launches (same arguments): `_place` runs the rejection loop, the label
 * transforms and the clearance filter and writes every output except `grid`; `_raster` turns the obstacle lists it
 * left into `grid`.  ppn_edage_maps == _place then _raster on one stream.  Apart they let the compute-bound half of
 * one batch overlap the store-bound half of another on different streams (double-buffer the ppn_maps_t). */
int ppn_edage_maps_place(const ppn_paths_t* paths, int32_t n_paths, int32_t placements,
                         uint64_t first_map_id, int32_t R, double map_size, double obstacles_size,
                         int32_t K, double clearance, uint64_t seed,
                         const double* place_draws, const double* obst_draws,
                         const ppn_maps_t* out, void* stream);
int ppn_edage_maps_raster(const ppn_paths_t* paths, int32_t n_paths, int32_t placements, int32_t R, int32_t K,
                          const ppn_maps_t* out, void* stream);

/* Path.boundary_check (Path.py:100-111) for n (angle, translation) pairs against one hull.
 * angle_deg[n] is the angle passed by the caller (MapGenerate passes -angle), translation_rc
 * [n][2] is (row, col).  ok[n] u8. */
int ppn_boundary_check(const double* hull, int32_t hull_n, const double* angle_deg,
                       const double* translation_rc, int32_t n, int32_t R, uint8_t* ok,
                       void* stream);
/* same, also returning the transformed hulls hull_out[n][hull_n][2] (second element of the reference's tuple) */
int ppn_boundary_check_ex(const double* hull, int32_t hull_n, const double* angle_deg,
                          const double* translation_rc, int32_t n, int32_t R, uint8_t* ok,
                          double* hull_out, void* stream);

/* The accept loop of MapGenerate.generate_map_randomly (MapGenerate.py:128-143) on its own: draws[n][3K]
 * (K x, K y, K size uniforms), pathpoint[n][1000][2]; accept[n][K] u8, obstacles[n][K][3] kept ones
 * compacted in draw order as [col,row,r], counts[n]. */
int ppn_obstacle_filter(const double* pathpoint, const double* draws, int32_t n, int32_t K, int32_t R,
                        double map_size, double obstacles_size, double clearance, uint8_t* accept,
                        double* obstacles, int32_t* counts, void* stream);

/* add_init_end_single (process_map.py:119-145) on n u8 grids [n][R][R]: PPN_GRID_MARK in the 7x7 squares
 * centred on the rounded init[n][2] and end[n][2] (row, col), clipped. */
int ppn_paint_markers(uint8_t* grid, int32_t n, int32_t R, const double* init, const double* end,
                      void* stream);

/* Obstacle raster rule standing in for plot_obstacles (Path.py:36-49): n_maps grids of R x R,
 * grid = PPN_GRID_OBST where the data point the pixel centre shows in the reference's cropped matplotlib figure
 * (X = (j + 0.5) * 444 / 446.4 + R / 446.4, Y = (i + 0.5) * 330 / 332.64 + 1.16 * R / 332.64) lies in the ellipse a stroked
 * circle (cx, cy, r) inks (semi-axes r + 0.625 R / 446.4 and r + 0.625 R / 332.64), else PPN_GRID_FREE; unfused IEEE double,
 * bit-exact against oracle/edage_np.py disc_raster.  obstacles [n_maps][stride][3] = (col, row, r), counts[n_maps]. */
int ppn_disc_raster(const double* obstacles, const int32_t* counts, int32_t stride,
                    int32_t n_maps, int32_t R, uint8_t* grid, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Planner tail (loop B).  collision_check_circle_edge (process_map.py:383-425) for n_seg
 * segments; segment i belongs to problem prob[i] whose obstacles are
 * obs[obs_off[p] .. obs_off[p+1]) as [ox, oy, size] floats.  hit[n_seg] u8. */
int ppn_collision_segments(const float* s, const float* e, const int32_t* prob, int32_t n_seg,
                           const float* obs, const int32_t* obs_off, float clearance,
                           uint8_t* hit, void* stream);
/* The reference's bounds test hard-codes its 224-pixel maps (process_map.py:384-387: a segment with a negative row or a
 * column above 224 is a collision); ppn_collision_segments keeps that constant.  `_bound` takes the map's resolution
 * instead, for maps of another size (configs 3 and 5: 256 and 512). */
int ppn_collision_segments_bound(const float* s, const float* e, const int32_t* prob, int32_t n_seg,
                                 const float* obs, const int32_t* obs_off, float clearance, float bound,
                                 uint8_t* hit, void* stream);

/* extract_path (process_map.py:293-365) on n heat maps `heat` [n][H][W] float32 already
 * down-sampled; init/end [n][2] doubles in down-sampled coordinates.  wp [n][max_wp][2] doubles,
 * wp_n[n], ok[n].  The 1 s wall-clock timeout becomes the max_wp step cap (<= PPN_MAX_WAYPOINTS).  One wave per problem;
 * the revisit rule runs on a bitmap of visited lattice offsets, and a heat map whose values are exactly k/255 is walked
 * from its 8-bit codes in LDS (any other values: from the float map in memory) — same waypoints either way.
 * Square maps only (H == W, else PPN_E_UNSUPPORTED): the reference's bounds test swaps the axes (process_map.py:318). */
int ppn_extract_paths(const float* heat, int32_t n, int32_t H, int32_t W, const double* init,
                      const double* end, int32_t max_wp, double* wp, int32_t* wp_n, uint8_t* ok,
                      void* stream);

/* Fused neighbourhood attention forward (replaces natten2dqkrpb + softmax + natten2dav behind
 * natten.NeighborhoodAttention2D, SegNet/nat.py:111-120,144).  qkv is the qkv Linear's output viewed as
 * [B][H][W][3][heads][32]; rpb [heads][13][13] float32; out [B][H][W][heads*32] (what `proj` consumes).
 * kernel size 7, head dim 32, dilation >= 1 with H, W >= 7*dilation (the module pads first, as NATTEN does).
 * dtype: 0 = float32, 1 = bfloat16 (float32 accumulation). q is multiplied by `scale` before QK. */
int ppn_na2d_fwd(const void* qkv, const float* rpb, void* out, int32_t B, int32_t H, int32_t W, int32_t heads,
                 int32_t dilation, float scale, int32_t dtype, void* stream);
/* Same for a zero-padded token grid: qkv covers the padded H x W grid (the padded tokens' q/k/v are the qkv bias, as
 * when NATTEN's module pads before its projection); only the Hr x Wr real tokens are queries and out is the cropped
 * [B][Hr][Wr][heads*32] tensor.  Hr <= H, Wr <= W. */
int ppn_na2d_fwd_padded(const void* qkv, const float* rpb, void* out, int32_t B, int32_t H, int32_t W, int32_t Hr,
                        int32_t Wr, int32_t heads, int32_t dilation, float scale, int32_t dtype, void* stream);
/* The same result without materialising the padded grid ("virtual padding"): qkv is [B][Hr][Wr][3][heads][32] (real
 * tokens only) and every padded position of the H x W grid has k / v = pad_kv[3][heads][32] — the qkv projection's bias
 * in the activation dtype (zeros when it has none), which is what projecting a zero-padded token yields.  Saves the
 * projection and the reads of the 1.7-3x larger padded grid on DiNAT's dilated layers. */
int ppn_na2d_fwd_vpad(const void* qkv, const void* pad_kv, const float* rpb, void* out, int32_t B, int32_t H, int32_t W,
                      int32_t Hr, int32_t Wr, int32_t heads, int32_t dilation, float scale, int32_t dtype, void* stream);

/* Swin's window / shifted-window multi-head self-attention, forward (replaces the body of mmseg's ShiftWindowMSA.forward and
 * WindowMSA.forward between the qkv and the proj Linear, SegNet/mmseg/backbones/swin.py:80-118,179-253: pad, roll, window
 * partition, q k^T + relative position bias (+ region mask), softmax, . v, window reverse, reverse roll, crop).
 * qkv [B][H][W][3][heads][32], real tokens only; pad_kv [3][heads][32] the k / v of every padded position (the qkv bias in the
 * activation dtype, zeros without one: mmseg pads before the projection); rpb [heads][13][13] float32 = mmseg's
 * relative_position_bias_table [169][heads] transposed, indexed [h][dy + 6][dx + 6] with (dy, dx) = query minus key inside the
 * window; out [B][H][W][heads*32], only real tokens written.  The grid is padded to Hp = ceil(H/7)*7, Wp likewise (also when
 * H or W < 7); window (wy, wx) slot (i, j) holds padded position ((7 wy + i + shift) mod Hp, (7 wx + j + shift) mod Wp).  With
 * shift > 0, slots of different regions (per axis of the shifted frame: y < Hp-7, Hp-7 <= y < Hp-shift, the rest) get -100
 * added to the logit (not -inf).  Logit = (q * scale) . k + bias.  window must be 7 and shift 0 or 3 (else
 * PPN_E_UNSUPPORTED); buffers 16-byte aligned, B * windows < 2^31, heads <= 65535 (else PPN_E_INVALID, no launch).
 * dtype 0 = float32, 1 = bfloat16 (float32 accumulation, matrix cores). */
int ppn_swin_wmsa_fwd(const void* qkv, const void* pad_kv, const float* rpb, void* out, int32_t B, int32_t H, int32_t W,
                      int32_t heads, int32_t window, int32_t shift, float scale, int32_t dtype, void* stream);

/* The same forward generalised over (window w, head dim d), for GenNet's AESwin (GenNet/networks/vanilla_swin.py:239-284,325-376,
 * 429-454 between the qkv and the proj Linear; csrc/wmsa_gen.hip).  qkv [B][H][W][3][heads][d], real tokens only; pad_kv
 * [3][heads][d] the k / v of every padded position; rpb [heads][2w-1][2w-1] float32 = the relative_position_bias_table
 * [(2w-1)^2][heads] transposed, indexed [h][dy + w-1][dx + w-1] with (dy, dx) = query minus key inside the window; out
 * [B][H][W][heads*d], only real tokens written.  The grid is padded to Hp = ceil(H/w)*w, Wp likewise (also when H or W < w);
 * window (wy, wx) slot (i, j) holds padded position ((w wy + i + shift) mod Hp, (w wx + j + shift) mod Wp).  With shift > 0, slots
 * of different regions (per axis of the shifted frame: y < Hp-w, Hp-w <= y < Hp-shift, the rest) get -100 added to the logit (not
 * -inf) - also when one window covers the whole grid (a 14 x 14 grid under w = 14, shift 7 is one window with four regions).
 * Logit = (q * scale) . k + bias.  (w, d) must be (14, 8), (14, 16), (14, 32), (7, 8), (7, 16) or (7, 32) - the last is
 * forwarded to ppn_swin_wmsa_fwd's kernels, bit for bit - and shift 0 or w / 2 (7 or 3), else PPN_E_UNSUPPORTED.  NULL pointers,
 * B / H / W / heads <= 0, heads > 65535, a non-finite or non-positive scale, a dtype other than 0 / 1, any of the four buffers not
 * 16-byte aligned and a launch of 2^31 work-items or more (B * windows * heads * 256, or * 64 at w = 7) return PPN_E_INVALID; all
 * of it before any HIP call.  dtype 0 = float32, 1 = bfloat16 (converted on load, float32 softmax and accumulation with the
 * maximum taken before any exponential, the output rounded once; one VALU kernel form serves both). */
int ppn_wmsa_fwd(const void* qkv, const void* pad_kv, const float* rpb, void* out, int32_t B, int32_t H, int32_t W, int32_t heads,
                 int32_t head_dim, int32_t window, int32_t shift, float scale, int32_t dtype, void* stream);

/* Backward of ppn_swin_wmsa_fwd, in its layouts and index arithmetic.  Per (image, window, head), over the 49 slots, with the
 * logit L_ij = scale q_i . k_j + rpb[h][rel(i, j)] + mask_ij (the -100 region mask of a shifted layer, not -inf):
 *   P = softmax_j(L);  dP_ij = dO_i . v_j;  delta_i = sum_j P_ij dP_ij (= rowsum(dO o O): the forward's output is not an input);
 *   dS_ij = P_ij (dP_ij - delta_i);  dV_j = sum_i P_ij dO_i;  dQ_i = scale sum_j dS_ij k_j;  dK_j = scale sum_i dS_ij q_i.
 * dout [B][H][W][heads*32] (real tokens; a padded query has dO = 0 and contributes nothing).  Outputs, all fully WRITTEN and never
 * accumulated into: dqkv in qkv's layout and dtype; dpad_kv [3][heads][32] float32 — a padded key / value slot's dK / dV belongs
 * to pad_kv (the qkv bias): its k and v thirds are the sums of dK / dV over all padded positions of all images, its q third is
 * exactly 0, and all of it is 0 when H and W are multiples of 7; drpb [heads][13][13] float32 with drpb[h][dy + 6][dx + 6] = the
 * sum of dS_ij over images, windows and slot pairs with query-minus-key offset (dy, dx), padded keys included (the mask does not
 * change it).  One (window, head) is computed end to end by one wave (bfloat16) or workgroup (float32), so dqkv has one writer per
 * element; drpb and dpad_kv are summed per workgroup over the windows it walks and then over the workgroups by a second kernel, in
 * a fixed order and without atomics: the gradients are bitwise reproducible.  workspace: ppn_swin_wmsa_bwd_workspace(...) floats
 * (the per-workgroup partial sums: the size depends on the current device), 16-byte aligned; workspace_floats is what the caller
 * allocated and is checked.  NULL pointers, B / H / W / heads <= 0, heads > 65535, a non-finite or non-positive scale, a dtype
 * other than 0 / 1, any buffer not 16-byte aligned, a workspace that is too small and B * windows >= 2^31 return PPN_E_INVALID,
 * window != 7 or shift not in {0, 3} PPN_E_UNSUPPORTED, before any HIP launch (the workspace check comes last: its size is the one
 * thing that asks the runtime, for the device's compute-unit count).  dtype 0 = float32 (VALU), 1 = bfloat16 (matrix
 * cores: float32 softmax arithmetic and accumulation, P and dS rounded to bfloat16 once each as operands, dqkv rounded once). */
int64_t ppn_swin_wmsa_bwd_workspace(int32_t B, int32_t H, int32_t W, int32_t heads);     /* floats; < 0: invalid shape */
int ppn_swin_wmsa_bwd(const void* qkv, const void* pad_kv, const float* rpb, const void* dout,
                      void* dqkv, float* dpad_kv, float* drpb, float* workspace, int64_t workspace_floats,
                      int32_t B, int32_t H, int32_t W, int32_t heads, int32_t window, int32_t shift,
                      float scale, int32_t dtype, void* stream);

/* Global multi-head self-attention, forward (the body of nn.MultiheadAttention between in_proj and out_proj, which mmseg's
 * VisionTransformer calls through mmcv's MultiheadAttention, SegNet/mmseg/backbones/vit.py:63-70,92-95):
 * out[b][n][h][:] = softmax_m(scale * q[b][n][h] . k[b][m][h]) . v[b][m][h], the sum over all N keys m of image b.
 * qkv [B][N][3][heads][head_dim] (each token row q | k | v: the order of in_proj_weight), out [B][N][heads][head_dim].
 * head_dim must be 64 or 8 (else PPN_E_UNSUPPORTED); any N >= 1.  NULL pointers, B / N / heads <= 0, a non-finite or non-positive
 * scale, a dtype other than 0 / 1, buffers not 16-byte aligned and grids of 2^31 work-items or more return PPN_E_INVALID
 * before any HIP call.  head_dim 64 (mmseg's ViT): dtype 0 = float32 (VALU), 1 = bfloat16 (flash-style on the matrix cores:
 * float32 online softmax and accumulation, the output rounded once).  head_dim 8 (GenNet's AE-ViT, csrc/mhsa_d8.hip): both data
 * types on one flash-style VALU kernel, a query per lane with its 8 channels in registers, float32 online softmax and
 * accumulation (bfloat16 converted on load, the output rounded once); nothing of size N x N reaches memory. */
int ppn_mhsa_fwd(const void* qkv, void* out, int32_t B, int32_t N, int32_t heads, int32_t head_dim, float scale, int32_t dtype,
                 void* stream);

/* Backward of ppn_mhsa_fwd: with P = softmax(scale q k^T) per (batch, head), dV = P^T dO, dS = P o (dO V^T - rowsum(dO o O)),
 * dQ = scale dS K, dK = scale dS^T Q.  qkv and out as in the forward (out is what ppn_mhsa_fwd returned for this qkv), dout
 * [B][N][heads][head_dim]; dqkv has qkv's layout and is fully WRITTEN (all three thirds of every row), never accumulated into.
 * Three passes (per-query softmax statistics and rowsum(dO o O) into the workspace; dK / dV per key block; dQ per query block):
 * P is recomputed, nothing of size N x N is stored, every output element has one writer and no atomics are used, so the
 * gradients are bitwise reproducible.  workspace: ppn_mhsa_bwd_workspace(B, N, heads) floats (2 * B * heads * N), 16-byte
 * aligned; workspace_floats is what the caller allocated and is checked.  head_dim must be 64 or 8 (else PPN_E_UNSUPPORTED); any
 * N >= 1.  NULL pointers, B / N / heads <= 0, a non-finite or non-positive scale, a dtype other than 0 / 1, buffers not 16-byte
 * aligned, a workspace that is too small and launches of 2^31 work-items or more return PPN_E_INVALID before any HIP call.
 * dtype 0 = float32 (VALU), 1 = bfloat16 (matrix cores: float32 softmax arithmetic and accumulation, P and dS rounded to
 * bfloat16 once each as operands, dqkv rounded once).  head_dim 8 (csrc/mhsa_d8.hip) runs the same three passes in the same
 * workspace on VALU kernels for both data types: float32 arithmetic throughout (bfloat16 converted on load, P and dS never
 * rounded, dqkv rounded once), the launch-size check against those kernels' own workgroup (256 rows, 128 work-items). */
int64_t ppn_mhsa_bwd_workspace(int32_t B, int32_t N, int32_t heads);      /* floats; < 0: invalid shape */
int ppn_mhsa_bwd(const void* qkv, const void* out, const void* dout, void* dqkv, float* workspace, int64_t workspace_floats,
                 int32_t B, int32_t N, int32_t heads, int32_t head_dim, float scale, int32_t dtype, void* stream);

/* Training loss of a segmentation head without the resized logits: bilinear resize (torch's F.interpolate, align_corners=False,
 * size given) of logit [B][C][h][w] (NCHW contiguous) to H x W, then cross-entropy against label [B][H][W] — what mmseg's
 * BaseDecodeHead.losses composes from resize + CrossEntropyLoss + accuracy (decode_head.py:231-265).  Per full-resolution pixel:
 * the C interpolated logits z_c, lse = log sum_c exp z_c (maximum subtracted), argmax (ties to the lowest class), loss lse - z_label.
 * *loss = the sum over the valid pixels divided by ALL B H W pixels (an ignored pixel adds 0 and still counts in the divisor, as
 * mmseg's mean does); *correct = the number of valid pixels whose argmax equals the label (an ignored pixel is never correct).
 * A label equal to ignore_index OR outside [0, C) is ignored everywhere and never indexes memory — the one deliberate difference
 * from the library, which raises a device-side assert on an out-of-range label.  lse [B][H][W] float32 is the only per-pixel
 * state the backward needs; pass NULL when no backward is wanted and it is not written.  The sums have a fixed order (a tree per
 * workgroup of 1024 pixels into the workspace, then one workgroup in double / int64) and no atomics: bitwise reproducible.
 * workspace: ppn_resize_ce_workspace(B, H, W) floats = 2 * ceil(B * H * W / 1024) (a float32 loss sum and an int32 count per
 * workgroup of 1024 pixels); workspace_floats is what the caller allocated and is checked.
 * ppn_resize_ce_bwd: dlogit[b][c][y][x] = *grad_out / (B H W) * the sum over the valid pixels (Y, X) whose taps touch (y, x) of
 * wy wx (exp(z_c(Y, X) - lse[Y][X]) - [label == c]), in gather form: one writer per element, dlogit (logit's layout and dtype) fully
 * WRITTEN, fixed-order sums, no atomics.  logit, label and lse are what the forward read and wrote; grad_out is ONE float32 on the
 * DEVICE (no host synchronisation).  Both calls use the same tap function, so they see the same z bit for bit.  float32 arithmetic
 * for both logit dtypes (0 = float32, 1 = bfloat16: widened on load, dlogit rounded once); label_dtype 0 = uint8, 1 = int64.  Any
 * C >= 1 and any sizes, up- or down-sampling.  NULL pointers (lse in the forward excepted), logit / dlogit / lse / workspace not
 * 16-byte aligned, label / loss / correct / grad_out not naturally aligned, an extent <= 0, B C h w or B H W >= 2^31, a launch of
 * 2^31 work-items or more, a dtype other than 0 / 1 and a workspace that is too small return PPN_E_INVALID before any HIP call. */
int64_t ppn_resize_ce_workspace(int B, int H, int W);           /* floats; < 0 for invalid sizes */
int ppn_resize_ce_fwd(const void* logit, const void* label, float* lse /* may be NULL: no backward wanted */,
                      float* loss /* 1 */, int64_t* correct /* 1 */, float* workspace, int64_t workspace_floats,
                      int B, int C, int h, int w, int H, int W, int ignore_index,
                      int logit_dtype /* 0 f32, 1 bf16 */, int label_dtype /* 0 u8, 1 i64 */, void* stream);
int ppn_resize_ce_bwd(const void* logit, const void* label, const float* lse, const float* grad_out /* device, 1 */,
                      void* dlogit, int B, int C, int h, int w, int H, int W, int ignore_index,
                      int logit_dtype, int label_dtype, void* stream);

/* Evaluation of a segmentation head without the resized logits: the three per-class area histograms that mmseg's mIoU / mDice /
 * mFscore are computed from (intersect_and_union, core/evaluation/metrics.py:26-86).  Per full-resolution pixel: the C logits of
 * logit [B][C][h][w] (NCHW contiguous) interpolated bilinearly to H x W with ppn_resize_ce_fwd's own tap arithmetic (torch's float32
 * align_corners=False rule, one shared inline function), and their argmax in ONE sweep over the channels with no exponentials (the
 * argmax of the softmax is the argmax of the logits); ties go to the lowest class, so the prediction is bit for bit the argmax that
 * ppn_resize_ce_fwd counts in *correct.  A NaN logit never wins (all NaN: class 0) — the one difference from torch.argmax, which
 * treats NaN as the maximum.  areas [3][C] int64: areas[0][c] = valid pixels with pred == label == c (intersect), areas[1][c] =
 * valid pixels with pred == c, areas[2][c] = valid pixels with label == c; union = areas[1] + areas[2] - areas[0].  A label equal
 * to ignore_index OR outside [0, C) is ignored: it adds to none of the three and never indexes memory (mmseg masks by
 * label != ignore_index only, so an out-of-range label that is not ignore_index would still count in ITS prediction histogram — the
 * deliberate difference, ppn_resize_ce_fwd's rule).  pred [B][H][W] uint8, when not NULL, is WRITTEN for every pixel, ignored or
 * not (any alignment; four pixels per store where the address allows).  areas is zeroed on the stream inside the call and needs no
 * workspace; counts are integers (int32 per workgroup in LDS — wave ballots and popcounts per class for C <= 8, LDS integer atomics
 * above —, then one 64-bit global atomic add per non-zero bin), so the result does not depend on the order: bitwise reproducible.
 * float32 arithmetic for both logit dtypes (0 = float32, 1 = bfloat16: widened on load); label_dtype 0 = uint8, 1 = int64.  Any
 * sizes, up- or down-sampling.  NULL logit / label / areas, logit not 16-byte aligned, areas not 8-byte aligned, label not naturally
 * aligned, an extent <= 0, C > 256 (pred is uint8, the LDS histogram is fixed), B C h w or B H W >= 2^31, a launch of 2^31
 * work-items or more and a dtype other than 0 / 1 return PPN_E_INVALID before any HIP call. */
int ppn_seg_eval(const void* logit /* [B][C][h][w] f32 | bf16 */, const void* label /* [B][H][W] u8 | i64 */,
                 uint8_t* pred /* [B][H][W], may be NULL */, int64_t* areas /* [3][C]: intersect | pred | label */,
                 int B, int C, int h, int w, int H, int W, int ignore_index,
                 int logit_dtype /* 0 f32, 1 bf16 */, int label_dtype /* 0 u8, 1 i64 */, void* stream);

/* The merge of a multi-scale + flip test-time augmentation (mmseg's aug_test, encoder_decoder.py:200-285: per augmentation resize to
 * the augmentation's image size, resize to ori_shape, softmax, flip back, add; then / len(imgs) and argmax) in ONE launch, from the
 * heads' LOW-resolution logits of up to PPN_SEG_TTA_MAX_AUGS augmentations to labels.  For output pixel (Y, X) and augmentation a:
 * the source pixel (Ys, Xs) is (Y, X), (Y, W-1-X) for flip 1 (horizontal) or (H-1-Y, X) for flip 2 (vertical); the logit of a class
 * is the two bilinear resizes (h,w) -> (hm,wm) -> (H,W) composed, both align_corners=False with ppn_resize_ce_fwd's own tap arithmetic
 * (torch's float32 rule, one shared inline function): stage 2's taps of Ys in hm / Xs in wm name up to 2 x 2 mid-grid positions, each
 * a stage-1 interpolation on the (h,w) plane (at most 4 x 4 loads per class), combined in the same order; softmax = maximum,
 * expf(z - m), 1 / s; the probabilities are summed over the augmentations in index order and divided by (float)n_augs.  pred [B][H][W]
 * uint8, when not NULL, is the argmax of that mean, WRITTEN for every pixel at any alignment (four pixels per store where the address
 * allows): ties go to the lowest class, a NaN never wins and all NaN is class 0 (ppn_seg_eval's rule; a NaN logit makes every
 * probability of its pixel NaN).  prob [B][C][H][W] float32, when not NULL, receives the mean probabilities.  float32 throughout for
 * both logit dtypes (0 = float32, 1 = bfloat16: widened on load, nothing is rounded to bfloat16 in between — the library composition
 * rounds every tensor it materialises).  With one augmentation, hm = H, wm = W, flip 0 and finite logits stage 2 is 1 z + 0 z' and
 * pred is ppn_seg_eval's pred bit for bit.  C <= PPN_SEG_TTA_REG_CLASSES: the per-class sums are registers and prob may be NULL;
 * larger C, up to 256: prob is required and is the accumulator (one work-item owns its pixels for every augmentation: no atomics, no
 * race, no zeroing by the caller).  Every result is bitwise reproducible.  augs is a HOST array, copied into a by-value kernel
 * argument: no device allocation and no synchronisation in the call; each augmentation has its own (h, w), all share B, C and the
 * dtype.  NULL augs, n_augs outside [1, PPN_SEG_TTA_MAX_AUGS], a NULL or not 16-byte aligned logit, an extent <= 0, a flip outside
 * {0, 1, 2}, C > 256, C > PPN_SEG_TTA_REG_CLASSES with NULL prob, pred and prob both NULL, B C h w, B C H W or B H W >= 2^31 and a
 * dtype other than 0 / 1 return PPN_E_INVALID before any HIP call. */
#define PPN_SEG_TTA_MAX_AUGS    16
#define PPN_SEG_TTA_REG_CLASSES 8
typedef struct ppn_tta_aug {
    const void* logit;          /* [B][C][h][w] f32 | bf16, device                                            */
    int32_t     h, w;           /* the head's resolution for this augmentation                                */
    int32_t     hm, wm;         /* the augmentation's image size (encode_decode's resize target)              */
    int32_t     flip;           /* 0 none, 1 horizontal, 2 vertical                                           */
} ppn_tta_aug;
int ppn_seg_tta(const ppn_tta_aug* augs /* HOST array */, int n_augs, uint8_t* pred /* [B][H][W], may be NULL */,
                float* prob /* [B][C][H][W], may be NULL when C <= PPN_SEG_TTA_REG_CLASSES */,
                int B, int C, int H, int W, int logit_dtype /* 0 f32, 1 bf16 */, void* stream);

/* ppn_resize_ce_fwd / _bwd with mmseg's OHEMPixelSampler (core/seg/sampler/ohem_pixel_sampler.py:32-85) and CrossEntropyLoss's
 * class_weight (losses/cross_entropy_loss.py:10-33): the same bilinear resize of logit [B][C][h][w] to H x W (the same tap
 * arithmetic, so the same interpolated logits bit for bit), per valid pixel ce = lse - z_label and p = exp(z_label - lse), and a
 * SELECTION of the hard pixels instead of the reference's softmax + gather + sort.  cw = class_weight [C] float32 on the device, or
 * NULL = all ones.  With n_valid valid pixels and batch_kept = min_kept * B:
 *   mode 1 (thresh given)  score = p;  t = max(ascending_sorted(p)[min(batch_kept, n_valid - 1)], thresh);  selected = p < t;
 *                          n_valid == 0: t = thresh and nothing is selected
 *   mode 2 (thresh None)   score = cw[label] ce;  t = the batch_kept-th largest score (the smallest when batch_kept >= n_valid);
 *                          selected = score >= t: pixels that TIE with the cut are all kept — the reference keeps exactly batch_kept
 *                          and leaves the choice among ties to an unstable sort, the one deliberate difference;  n_valid == 0: t = +inf
 *   mode 0 (no sampler)    score = cw[label] ce;  t = -inf;  every valid pixel is selected (class weights only)
 * *loss = 1 / (B H W) * the sum over the selected pixels of cw[label] ce — the mean over ALL pixels, as weight_reduce_loss with
 * avg_factor None takes it.  counts [3] int64 = {correct (valid pixels whose argmax, ties to the lowest class, equals the label: not
 * changed by the sampling), n_valid, n_kept (selected pixels)}.  *threshold = t, float32, computed and kept on the DEVICE: nothing is
 * read back to the host.  mask [B][H][W] uint8, when not NULL, is WRITTEN for every pixel: 1 selected, 0 not.  lse and score
 * [B][H][W] float32 are WRITTEN for every pixel and are what the backward reads; an ignored pixel (label == ignore_index or outside
 * [0, C), which never indexes memory) has the score NaN — no comparison with it is true, so it is never selected, and the histograms
 * skip it — a valid pixel's score that comes out NaN is stored as +inf, and -0 as +0.  The selection is a radix select of the k-th
 * smallest score over a 32-bit key that orders as the floats do, in three digits of 11 | 11 | 10 bits: integer histograms in LDS (the
 * bin of a wave's first live lane is added once per wave by a ballot, twice over, the lanes left one by one), one global integer
 * atomic per non-zero bin and workgroup; the later passes read score only.  Every sum of floats has a fixed order (a tree per
 * workgroup, then one workgroup in double / int64) and every atomic is an integer add: loss, threshold, mask and dlogit are bitwise
 * reproducible.  workspace: ppn_ohem_ce_workspace(B, H, W) BYTES (the same for every valid size), 16-byte aligned, needs NO
 * initialisation by the caller; workspace_bytes is what the caller allocated and is checked.
 * ppn_ohem_ce_bwd: dlogit[b][c][y][x] = *grad_out / (B H W) * the sum over the SELECTED pixels (Y, X) whose taps touch (y, x) of
 * wy wx cw[label] (exp(z_c - lse) - [label == c]), in ppn_resize_ce_bwd's gather form: one writer per element, dlogit fully WRITTEN,
 * fixed-order sums, no atomics; `selected` is recomputed from score and *threshold (device), no weight tensor exists.  Same
 * class_weight, mode and ignore_index as the forward.  float32 arithmetic for both logit dtypes (0 = float32, 1 = bfloat16: widened on
 * load, dlogit rounded once); label_dtype 0 = uint8, 1 = int64.  NULL pointers (class_weight and mask excepted), logit / dlogit /
 * lse / score / workspace not 16-byte aligned, the others not naturally aligned, an extent <= 0, B C h w or B H W >= 2^31, a launch
 * of 2^31 work-items or more, a dtype other than 0 / 1, a mode other than 0 / 1 / 2, min_kept < 1 (modes 1, 2), thresh outside (0, 1]
 * or NaN (mode 1) and a workspace that is too small return PPN_E_INVALID before any HIP call. */
int64_t ppn_ohem_ce_workspace(int B, int H, int W);             /* bytes; < 0 for invalid sizes */
int ppn_ohem_ce_fwd(const void* logit, const void* label, const float* class_weight /* [C] device, may be NULL */,
                    float* lse /* [B][H][W] */, float* score /* [B][H][W] */, float* loss /* 1 */,
                    int64_t* counts /* 3: correct, n_valid, n_kept */, float* threshold /* 1 */, uint8_t* mask /* [B][H][W], may be NULL */,
                    void* workspace, int64_t workspace_bytes, int B, int C, int h, int w, int H, int W, int ignore_index,
                    int mode /* 0 none, 1 thresh, 2 top-k */, float thresh, int min_kept,
                    int logit_dtype /* 0 f32, 1 bf16 */, int label_dtype /* 0 u8, 1 i64 */, void* stream);
int ppn_ohem_ce_bwd(const void* logit, const void* label, const float* class_weight, const float* lse, const float* score,
                    const float* threshold /* device, 1 */, const float* grad_out /* device, 1 */, void* dlogit,
                    int B, int C, int h, int w, int H, int W, int ignore_index, int mode, int logit_dtype, int label_dtype, void* stream);

/* mmseg's DiceLoss (models/losses/dice_loss.py, exponent 2) of a segmentation head without the resized logits, their softmax or a
 * one-hot tensor: logit [B][C][h][w] resized bilinearly to H x W with ppn_resize_ce_fwd's own tap arithmetic (the same interpolated
 * logits bit for bit), per pixel p_i = exp(z_i - lse), v = the label is valid (not ignore_index and inside [0, C)), tc = the label
 * clamped into [0, C - 1], and per image and class
 *   I = sum_px p_i [tc == i] v,   P2 = sum_px p_i^2,   T = #{px: tc == i}  (not masked: the reference's denominator counts an ignored
 *   label as the class its clamp lands on),   N = 2 I + smooth,   Den = P2 + T + smooth,
 *   *loss = 1 / (C B) sum_b sum_{i != ignore_index} cw_i (1 - N / Den)       (cw = class_weight [C] float32 on the device, NULL = ones;
 *   the loss's own loss_weight stays with the caller).  sums [B][C][3] float64 = I | P2 | T (T an exact integer), WRITTEN; *correct =
 * valid pixels whose argmax (ties to the lowest class) equals the label, ppn_resize_ce_fwd's count; lse [B][H][W] float32, when not
 * NULL, is WRITTEN for every pixel and is the only per-pixel state the backward reads.  A label never indexes memory.
 * ppn_resize_dice_bwd: dlogit[b][c][y][x] = the sum over the pixels (Y, X) whose taps touch (y, x) of wy wx p_c (g_c - s), g_i =
 * a[b][i] [tc == i] v + b[b][i] p_i, s = sum_i g_i p_i, a = -2 k_i / Den, b = 2 k_i N / Den^2, k_i = *grad_out cw_i / (C B), 0 for
 * i == ignore_index — the coefficients are derived on the device from sums, smooth, class_weight and *grad_out (nothing is read back);
 * a first pass writes s, one float32 per pixel, into the workspace, then ppn_resize_ce_bwd's gather: one writer per element, dlogit
 * fully WRITTEN.  Same class_weight, smooth and ignore_index as the forward.  No atomics anywhere and every sum has a fixed order
 * (per-tile partials in a fixed tree, then in double): sums, loss, correct and dlogit are bitwise reproducible.
 * workspace: ppn_resize_dice_workspace(B, C, H, W) = 4 * max(B * ceil(H W / 1024) * (3 C + 1), B H W + 4 B C) BYTES, 16-byte aligned,
 * needs NO initialisation; both calls use it from its start (the backward overwrites what the forward left).  float32 arithmetic
 * for both logit dtypes (0 = float32, 1 = bfloat16: widened on load, dlogit rounded once); label_dtype 0 = uint8, 1 = int64.  NULL
 * pointers (class_weight, and lse in the forward, excepted), logit / dlogit / lse / workspace not 16-byte aligned, the others not
 * naturally aligned, an extent <= 0, C > 256, B C h w or B H W >= 2^31, a launch of 2^31 work-items or more, a dtype other than 0 / 1
 * and smooth negative, NaN or infinite return PPN_E_INVALID before any HIP call. */
int64_t ppn_resize_dice_workspace(int B, int C, int H, int W);  /* bytes; < 0 for invalid sizes */
int ppn_resize_dice_fwd(const void* logit, const void* label, const float* class_weight /* [C] device, may be NULL */, void* workspace,
                        float* lse /* [B][H][W], may be NULL */, double* sums /* [B][C][3]: I | P2 | T */, float* loss /* 1 */,
                        int64_t* correct /* 1 */, int B, int C, int h, int w, int H, int W, int ignore_index, float smooth,
                        int logit_dtype /* 0 f32, 1 bf16 */, int label_dtype /* 0 u8, 1 i64 */, void* stream);
int ppn_resize_dice_bwd(const void* logit, const void* label, const float* lse, const double* sums, const float* class_weight,
                        const float* grad_out /* device, 1 */, void* workspace, void* dlogit,
                        int B, int C, int h, int w, int H, int W, int ignore_index, float smooth,
                        int logit_dtype, int label_dtype, void* stream);

/* Backward of ppn_na2d_fwd (the gradient NATTEN's natten2dqkrpb / natten2dav backward kernels compute; first brick of the
 * training step, GenNet/train.py:93-147, SegNet/mmseg/apis/train.py:67-167).  qkv [B][H][W][3][heads][32] and rpb as in the
 * forward, dout [B][H][W][heads*32]; outputs dqkv (same layout as qkv) and drpb [heads][13][13] float32, both fully WRITTEN (the
 * rpb gradient is summed in a fixed order: bit-reproducible).  Two passes over 8 x 8 regions staged through LDS, the
 * probabilities recomputed in the second; workspace: ppn_na2d_bwd_workspace(...) floats, 16-byte aligned (softmax statistics of
 * every query, 4 floats, + 169 partial sums of drpb per region and head) — workspace_floats is what the caller allocated and is
 * checked.  H, W >= 7 * dilation (the training module pads the tokens itself, as NATTEN's does).  dtype 0 = float32,
 * 1 = bfloat16 (float32 arithmetic). */
int64_t ppn_na2d_bwd_workspace(int32_t B, int32_t H, int32_t W, int32_t heads, int32_t dilation);   /* floats; < 0: invalid shape */
int ppn_na2d_bwd(const void* qkv, const float* rpb, const void* dout, void* dqkv, float* drpb, float* workspace, int64_t workspace_floats,
                 int32_t B, int32_t H, int32_t W, int32_t heads, int32_t dilation, float scale, int32_t dtype, void* stream);

/* Backward of ppn_na2d_fwd_vpad: ppn_na2d_bwd on the grid that the virtual padding defines, without building it.  H, W name the
 * padded grid and Hr, Wr the real tokens, in ppn_na2d_fwd_vpad's argument order.  qkv [B][Hr][Wr][3][heads][32] (real tokens only);
 * every position of the H x W grid outside Hr x Wr has k, v = pad_kv[3][heads][32] (in qkv's dtype; its q third is not read); only
 * real tokens are queries; dout [B][Hr][Wr][heads*32].  Outputs, all fully WRITTEN and never accumulated into: dqkv in qkv's layout
 * and dtype (real tokens only); drpb [heads][13][13] float32, padded keys included, as in the materialised form; dpad_kv
 * [3][heads][32] float32 — its k third is the sum of dK over all padded positions of all images, its v third the sum of dV over the
 * same positions, its q third exactly 0 (a padded query is cropped: dO = 0), and all of it exactly 0 when Hr == H and Wr == W.
 * float32 arithmetic for both dtypes; the probabilities are recomputed in the key pass from 16 bytes of statistics per real query;
 * all padded keys of a query's window share one k and one v, so their dK / dV are formed per query from two scalars (sum p, sum dS
 * over those keys) and summed per workgroup in query order; a key's range of queries ends at the last real one (a padded query has
 * no statistics); one writer per dqkv element, no atomics, fixed-order sums: the three outputs are bitwise reproducible.
 * workspace: ppn_na2d_bwd_vpad_workspace(...) floats, 16-byte aligned = 4 * B * heads * Hr * Wr (statistics of the real queries)
 * + 233 * heads * workgroups (169 drpb bins + 2 x 32 dpad_kv sums each), workgroups = B * dilation^2 * ceil(ceil(H / dilation) / 8)
 * * ceil(ceil(W / dilation) / 8); workspace_floats is what the caller allocated and is checked.  NULL pointers, B / Hr / Wr / heads
 * <= 0, Hr > H or Wr > W, H or W < 7 * dilation, heads > 65535, a non-finite or non-positive scale, a dtype other than 0 / 1, any
 * buffer not 16-byte aligned, a workspace that is too small and 2^31 workgroups or more return PPN_E_INVALID before any HIP call
 * (ppn_na2d_bwd_vpad_workspace returns < 0 for such a shape). */
int64_t ppn_na2d_bwd_vpad_workspace(int32_t B, int32_t H, int32_t W, int32_t Hr, int32_t Wr, int32_t heads, int32_t dilation);
int ppn_na2d_bwd_vpad(const void* qkv, const void* pad_kv, const float* rpb, const void* dout, void* dqkv, float* dpad_kv,
                      float* drpb, float* workspace, int64_t workspace_floats, int32_t B, int32_t H, int32_t W, int32_t Hr,
                      int32_t Wr, int32_t heads, int32_t dilation, float scale, int32_t dtype, void* stream);

/* Fused residual + LayerScale + LayerNorm around the NAT layer's dense ops (SegNet/nat.py:140-153):
 *   a == NULL : y_out = LayerNorm(x)                                   (x_out ignored)
 *   a != NULL : x_out = x + gamma * a  (gamma NULL = 1);  y_out = LayerNorm(x_out) unless y_out is NULL.
 * rows x C row-major, C a multiple of 8 with C/8 a power of two <= 64 (one pass of C/8 lanes), or C = 1024 (two passes of 64 lanes),
 * or C/8 = 3 * 2^k with 2^k <= 64 (three passes of 2^k lanes: 96, 192, 384, 768, 1536 — and 24, 48 on the padded form), or any
 * C <= 64 on the unpadded forms; every other width returns PPN_E_UNSUPPORTED before any launch, from this entry, from
 * ppn_layernorm_offset and from ppn_residual_layernorm_padded alike.  w, b, gamma are [C] in the same dtype (0 = float32,
 * 1 = bfloat16; statistics in float32). x_out may alias x. */
int ppn_residual_layernorm(const void* x, const void* a, const void* gamma, const void* w, const void* b, void* x_out,
                           void* y_out, int64_t rows, int32_t C, float eps, int32_t dtype, void* stream);
/* y_out = LayerNorm(x + xoff) with a per-channel float32 offset xoff [C] (NULL = none; float32 whatever dtype x has): for a residual stream whose constant
 * (bias) part is carried outside the tensor — the projections then accumulate straight into x through the GEMM's
 * beta * C term and the residual add needs no pass of its own. */
int ppn_layernorm_offset(const void* x, const float* xoff, const void* w, const void* b, void* y_out, int64_t rows,
                         int32_t C, float eps, int32_t dtype, void* stream);
/* Same, with y_out scattered into a zero-padded token grid: rows = B*Hr*Wr tokens in [B][Hr][Wr] order are written to
 * y_out laid out [B][Hp][Wp][C] (the pad region is left untouched: the caller zero-fills it once). */
int ppn_residual_layernorm_padded(const void* x, const void* a, const void* gamma, const void* w, const void* b,
                                  void* x_out, void* y_out, int64_t rows, int32_t C, float eps, int32_t dtype,
                                  int32_t Hr, int32_t Wr, int32_t Hp, int32_t Wp, void* stream);

/* The TRAINING pair of ppn_residual_layernorm (csrc/residual_ln_bwd.hip): stochastic depth folded in, row statistics kept, and the
 * backward of all of it in one pass over the rows.
 *
 * ppn_residual_layernorm_train_fwd:
 *   a != NULL : x_out = x + scale[b] * gamma * a  (gamma NULL = 1; scale NULL = 1);  y_out = LayerNorm(x_out) unless y_out is NULL
 *   a == NULL : y_out = LayerNorm(x)                                                  (x_out, gamma, scale ignored)
 * scale [rows / rows_per_image] float32: image b owns rows_per_image consecutive rows; 0 drops the image's branch, 1 / keep scales
 * it (timm's DropPath).  With y_out, stats [rows][2] float32 receives (mean, rstd) of every row; without, nothing is written to it.
 * For bfloat16 the LayerNorm sees the rounded x_out.  x_out must not alias x when autograd keeps x.
 *
 * ppn_residual_layernorm_bwd: gy = the gradient at y_out (NULL: none, or no LayerNorm), gx = the gradient that arrives at x_out from
 * its other consumers (NULL: none); at least one is given.  xn = the forward's x_out (x for a plain LayerNorm), stats its statistics
 * (both needed with gy only).  With xhat = (xn - mean) rstd, g = gy w, G = gx + rstd (g - mean_c(g) - xhat mean_c(g xhat)):
 *   dx = G        da = scale[b] gamma G        dgamma_c = sum_rows scale[b] a G        dw_c = sum_rows gy xhat        dbeta_c = sum_rows gy
 * Every output pointer may be NULL (not wanted) except dx with gy; dgamma needs a and gamma, dw / dbeta need gy.  dx, da are rows x C
 * of `dtype`, dgamma / dw / dbeta [C] of `dtype`: summed in float32 without atomics (one partial per workgroup in `workspace`, added
 * in a fixed order by a second kernel) and rounded once, so two calls give the same bits.  workspace holds
 * ppn_residual_layernorm_bwd_workspace(rows, C) floats (< 0: a width the kernels do not take).
 *
 * Widths as ppn_residual_layernorm.  PPN_E_INVALID before any HIP call for a NULL required pointer, rows <= 0, a dtype outside {0, 1},
 * rows % rows_per_image != 0 with a scale, a workspace that is too small; PPN_E_UNSUPPORTED for another width or 2^31 rows and more. */
int64_t ppn_residual_layernorm_bwd_workspace(int64_t rows, int32_t C);
int ppn_residual_layernorm_train_fwd(const void* x, const void* a, const void* gamma, const float* scale, const void* w, const void* b,
                                     void* x_out, void* y_out, float* stats, int64_t rows, int64_t rows_per_image, int32_t C, float eps,
                                     int32_t dtype, void* stream);
int ppn_residual_layernorm_bwd(const void* gy, const void* gx, const void* xn, const void* a, const void* gamma, const float* scale,
                               const void* w, const float* stats, void* dx, void* da, void* dgamma, void* dw, void* dbeta, float* workspace,
                               int64_t workspace_floats, int64_t rows, int64_t rows_per_image, int32_t C, int32_t dtype, void* stream);

/* DiNAT_s's PatchMerging in front of its reduction GEMM (csrc/patch_merge_ln.hip; reference SegNet/dinats.py:74-104): the 2 x 2 gather
 * of a token grid fused with the LayerNorm over the gathered 4C values, forward and backward.
 *
 * x [B][H][W][C] contiguous NHWC of `dtype` (0 = float32, 1 = bfloat16); Ho = ceil(H / 2), Wo = ceil(W / 2), rows = B Ho Wo.
 * ppn_patch_merge_ln_fwd: row (b, i, j) of y [B][Ho][Wo][4C] is LayerNorm_{4C}(concat_q x[b, 2i + (q & 1), 2j + (q >> 1), :], q = 0..3)
 *   with biased variance and `eps`, scaled by gamma and shifted by beta (each [4C] of `dtype`), rounded once.  A token outside the grid
 *   (odd H or W) reads as zeros and enters the statistics as zeros.  Statistics are float32, mean first and then the centred squares.
 *   stats [rows][2] float32 receives (mean, rstd) of every row; NULL = not wanted (inference).
 * ppn_patch_merge_ln_bwd: with xhat = (row - mean) rstd and g = gy gamma, quadrant q of rstd (g - mean(g) - xhat mean(g xhat)) is stored
 *   to dx[b, 2i + (q & 1), 2j + (q >> 1), :] (every element of dx [B][H][W][C] is written exactly once; the gradient of a padded position
 *   is dropped), dgamma = sum_rows gy xhat and dbeta = sum_rows gy ([4C] of `dtype`; NULL = not wanted) are summed in float32 without
 *   atomics — one [2][4C] partial per workgroup in `workspace`, added in a fixed order by a second kernel — and rounded once: two calls
 *   give the same bits.  gy [B][Ho][Wo][4C] of `dtype`; x, stats and gamma as in the forward.
 * ppn_patch_merge_ln_bwd_workspace(B, H, W, C): the bytes `workspace` holds,
 *   4 * min(ceil(rows / ppn_patch_merge_ln_rows(C)), ppn_patch_merge_ln_max_blocks()) * 2 * 4C; < 0 for sizes the entry points refuse.
 * ppn_patch_merge_ln_rows(C): the rows of one workgroup tile, 256 / (C / 8); 0 for a width outside the set.
 * ppn_patch_merge_ln_max_blocks(): the most workgroups of a launch; past that many tiles a workgroup strides over several.
 *
 * C in {8, 16, 32, 64, 128, 256, 512}.  Before any HIP call: PPN_E_INVALID for a NULL required pointer, a tensor pointer that is not
 * 16-byte aligned (stats: 4), an extent below 1, a dtype outside {0, 1}, an eps that is negative or not finite, 2^31 elements and more
 * in x or in the gathered rows; PPN_E_UNSUPPORTED for another width. */
int     ppn_patch_merge_ln_rows(int C);
int     ppn_patch_merge_ln_max_blocks(void);
int     ppn_patch_merge_ln_fwd(const void* x, const void* gamma, const void* beta, void* y, float* stats /* may be NULL */,
                               int B, int H, int W, int C, float eps, int dtype, void* stream);
int64_t ppn_patch_merge_ln_bwd_workspace(int B, int H, int W, int C);   /* bytes; < 0 for invalid sizes */
int     ppn_patch_merge_ln_bwd(const void* gy, const void* x, const float* stats, const void* gamma, void* workspace,
                               void* dx, void* dgamma /* may be NULL */, void* dbeta /* may be NULL */,
                               int B, int H, int W, int C, int dtype, void* stream);

/* The training pair of GenNet's stem (csrc/gennet_stem_train.hip; reference GenNet/networks/ae_vit.py conv_first): Conv2d(1, C, 3, 1, 1) ->
 * BatchNorm2d on the batch statistics -> LeakyReLU at full resolution, forward and backward, in one write of z and one read of dz.
 *
 * x [B][H][W] float32 (one input channel); w [C][9] (tap 3 dy + dx), bias, gamma, beta [C] float32; z and dz [B][C][H][W] contiguous NCHW
 * of `dtype` (0 = float32, 1 = bfloat16).  N = B H W.  All arithmetic is float32 from the float32 x and parameters, the moments and the
 * two finishing steps float64; bfloat16 is only the rounding of z on store and the widening of dz on load.
 * ppn_gennet_stem_train_fwd: with p(n) the zero-padded 3 x 3 patch of x at pixel n, moments [54] float64 receives S1 = sum_n p (9) and
 *   the lower triangle of S2 = sum_n p p^T (45, element (i, j <= i) at 9 + i (i + 1) / 2 + j), summed in float64 — one partial per
 *   workgroup in `workspace`, added in a fixed order.  stats [3][C] float32 receives mean_c = w_c . S1 / N + bias_c, the biased variance
 *   var_c = w_c^T (S2 / N - S1 S1^T / N^2) w_c and rstd_c = 1 / sqrt(var_c + eps).  z = leaky_relu(gamma ((conv(x) + bias - mean) rstd)
 *   + beta, negative_slope), rounded once.  The convolution's output is never written.
 * ppn_gennet_stem_train_bwd: recomputes xhat and the pre-activation u from x with the forward's own instructions (the LeakyReLU mask
 *   is the forward's bit for bit), g = dz (u > 0 ? 1 : negative_slope); dbeta_c = sum g, dgamma_c = sum g xhat and, with G_c = sum g p,
 *   dw_c = gamma_c rstd_c (G_c - (dbeta_c / N) S1 - (dgamma_c / N) X_c), X_c = rstd_c (S2 w_c + (bias_c - mean_c) S1), each [C] or [C][9]
 *   float32.  The sums are float32 per workgroup (one partial each in `workspace`), added in a fixed order and finished in float64, rounded
 *   once: one writer per element, two calls give the same bits.  The gradient of bias is exactly 0 and is not written.  x, w, bias, gamma,
 *   beta, stats and moments as in (and from) the forward.
 * ppn_gennet_stem_train_workspace(B, H, W, C): the bytes `workspace` holds (either call),
 *   max(54 * 8, C * 11 * 4) * min(ceil(N / ppn_gennet_stem_train_tile()), ppn_gennet_stem_train_max_blocks()); < 0 for sizes the entry
 *   points refuse.
 * ppn_gennet_stem_train_tile(): the pixels of one workgroup tile (1024: 256 work-items x 4 consecutive pixels).
 * ppn_gennet_stem_train_max_blocks(): the most workgroups (in x) of the summing kernels; past that many tiles a workgroup strides.
 *
 * C in {8, 16, 24, 32}.  Before any HIP call: PPN_E_INVALID for a NULL required pointer, a pointer that is not 16-byte aligned
 * (moments: 8, stats: 4), an extent below 1 or N < 2, a dtype outside {0, 1}, an eps or negative_slope that is negative or not finite,
 * 2^31 elements and more in z; PPN_E_UNSUPPORTED for another C. */
int     ppn_gennet_stem_train_tile(void);
int     ppn_gennet_stem_train_max_blocks(void);
int64_t ppn_gennet_stem_train_workspace(int B, int H, int W, int C);   /* bytes; < 0 for invalid sizes */
int     ppn_gennet_stem_train_fwd(const float* x, const float* w, const float* bias /* may be NULL = 0 */, const float* gamma,
                                  const float* beta, void* z, float* stats, double* moments, void* workspace,
                                  int B, int H, int W, int C, float eps, float negative_slope, int dtype, void* stream);
int     ppn_gennet_stem_train_bwd(const void* dz, const float* x, const float* w, const float* bias /* may be NULL = 0 */,
                                  const float* gamma, const float* beta, const float* stats, const double* moments, void* workspace,
                                  float* dw, float* dgamma, float* dbeta,
                                  int B, int H, int W, int C, float negative_slope, int dtype, void* stream);

/* The training pair of GenNet's tail (csrc/gennet_tail_train.hip; reference GenNet/networks/ae_vit.py, the last dec_conv stage's BatchNorm2d
 * and LeakyReLU followed by conv_final): BatchNorm2d on the batch statistics -> LeakyReLU -> Conv2d(C, 1, 3, 1, 1) at full resolution,
 * forward and backward, in two reads of y forward and two reads of y plus one write of dy backward.  Neither the BatchNorm's output, the
 * activation z nor its gradient is ever written.
 *
 * y and dy [B][C][H][W], out and dout [B][1][H][W], contiguous NCHW of `dtype` (0 = float32, 1 = bfloat16); gamma, beta [C], wf [C][9]
 * (tap 3 dy + dx), bf [1], stats [3][C] and every parameter gradient float32.  N = B H W.  All arithmetic is float32 (the statistics and
 * the two finishing steps float64); bfloat16 is only the widening of y and dout on load and the rounding of out and dy on store.
 * ppn_gennet_tail_train_fwd: stats receives mean_c = sum y / N, the biased variance var_c = sum y^2 / N - mean_c^2 (never negative; 0
 *   exactly for a constant plane) and rstd_c = 1 / sqrt(var_c + eps), from float64 sums — one partial per workgroup in `workspace`, added
 *   in a fixed order.  With xhat = (y - mean) rstd, u = gamma xhat + beta and z = u > 0 ? u : negative_slope u inside the image and
 *   z = 0 outside it (the convolution's zero padding): out(p) = bf + sum_c sum_tap wf[c][tap] z_c(p + tap), rounded once.
 * ppn_gennet_tail_train_bwd: recomputes xhat and u from y with the forward's own instructions (the LeakyReLU mask is the forward's bit
 *   for bit).  With d = dout, zero outside the image: dz_c(q) = sum_tap wf[c][tap] d(q - tap), g = dz (u > 0 ? 1 : negative_slope);
 *   dbeta_c = sum g, dgamma_c = sum g xhat, dwf[c][tap] = sum_q z_c(q) d(q - tap), dbf = sum d (not written when dbf is NULL), and
 *   dy = gamma rstd (g - dbeta / N - xhat dgamma / N) in a second pass (skipped when dy is NULL).  The sums are float32 per workgroup
 *   (one partial each in `workspace`), added in a fixed order and finished in float64, rounded once: one writer per element, no atomics,
 *   two calls give the same bits.  y, gamma, beta, wf and stats as in (and from) the forward.
 * ppn_gennet_tail_train_workspace(B, H, W, C): the bytes `workspace` holds (either call),
 *   max(C * 2 * 8, (C * 11 + 1) * 4) * min(ceil(N / ppn_gennet_tail_train_tile()), ppn_gennet_tail_train_max_blocks()); < 0 for sizes the
 *   entry points refuse.
 * ppn_gennet_tail_train_tile(): the pixels of one workgroup tile (1024: 256 work-items x 4 consecutive pixels).
 * ppn_gennet_tail_train_max_blocks(): the most workgroups (in x) of the summing kernels; past that many tiles a workgroup strides.
 *
 * C in {8, 16, 24, 32}.  Before any HIP call: PPN_E_INVALID for a NULL required pointer, a pointer that is not 16-byte aligned (stats,
 * bf, dbf: 4), an extent below 1 or N < 2, a dtype outside {0, 1}, an eps or negative_slope that is negative or not finite, 2^31
 * elements and more in y; PPN_E_UNSUPPORTED for another C. */
int     ppn_gennet_tail_train_tile(void);
int     ppn_gennet_tail_train_max_blocks(void);
int64_t ppn_gennet_tail_train_workspace(int B, int H, int W, int C);   /* bytes; < 0 for invalid sizes */
int     ppn_gennet_tail_train_fwd(const void* y, const float* gamma, const float* beta, const float* wf, const float* bf /* may be NULL = 0 */,
                                  void* out, float* stats, void* workspace,
                                  int B, int H, int W, int C, float eps, float negative_slope, int dtype, void* stream);
int     ppn_gennet_tail_train_bwd(const void* dout, const void* y, const float* gamma, const float* beta, const float* wf, const float* stats,
                                  void* workspace, void* dy /* may be NULL */, float* dgamma, float* dbeta, float* dwf,
                                  float* dbf /* may be NULL */,
                                  int B, int H, int W, int C, float negative_slope, int dtype, void* stream);

/* The training kernels of GenNet's 24 -> 24 stride-2 stages (csrc/gennet_s2_train.hip; reference GenNet/networks/ae_vit.py, enc_conv's
 * Conv2d(C, C, 3, 2, 1) and dec_conv's ConvTranspose2d(C, C, 3, 2, 1, output_padding=1)): one adjoint pair and one reduction serve both
 * layer types, forward and backward, with the weights as the modules store them — nothing is flipped, transposed or repacked.
 *
 * H x W is always the BIG grid, the small one is Hs x Ws = ceil(H / 2) x ceil(W / 2); outside either grid everything is zero.
 *   D, ppn_gennet_s2_down:  small[b,o,i,j] = bias[o] + sum_{c,ky,kx} w[o][c][ky][kx] big[b,c,2i+ky-1,2j+kx-1];  w is [out][in][3][3].
 *   U, ppn_gennet_s2_up:    big[b,c,Y,X] = bias[c] + sum_{a,ky,kx : Y = 2i-1+ky, X = 2j-1+kx} w[a][c][ky][kx] small[b,a,i,j];  w is
 *      [in][out][3][3]; gather form (even Y takes ky = 1, odd Y takes ky = 0 and ky = 2, X alike): one writer per element.  Each axis of
 *      the big extent is 2 Hs or 2 Hs - 1, as passed.
 *   W, ppn_gennet_s2_wgrad: dw[a][c][ky][kx] = sum_{b,i,j} small[b,a,i,j] big[b,c,2i+ky-1,2j+kx-1], [small channel][big channel][3][3];
 *      sum_small[a] = sum_{b,i,j} small[b,a,i,j] and sum_big[c] = sum_{b,Y,X} big[b,c,Y,X] in the same pass (either may be NULL).
 * Conv2d (weight [co][ci]): forward D(x, w) + bias; input gradient U(dy, w) at x's extent; weight gradient W(small = dy, big = x), bias
 * gradient sum_small.  ConvTranspose2d (weight [ci][co]): forward U(x, w) + bias at 2H x 2W; input gradient D(dy, w); weight gradient
 * W(small = x, big = dy), bias gradient sum_big.
 *
 * big [B][C][H][W] and small [B][C][Hs][Ws] contiguous NCHW of `dtype` (0 = float32, 1 = bfloat16); w [C][C][3][3], bias [C], dw, sum_small
 * and sum_big float32.  Products and sums are float32 FMAs in both data types (bfloat16 is only the widening on load and the one rounding
 * on store).  W keeps one float32 partial [C C 9 + 2 C] per workgroup in `workspace`; a finishing kernel adds the partials in a fixed
 * order in float64 and rounds once.  No atomics anywhere: two calls give the same bits.
 * ppn_gennet_s2_wgrad_workspace(B, Hs, Ws) — of the SMALL grid: the bytes `workspace` holds,
 *   (24 * 24 * 9 + 2 * 24) * 4 * min(ceil(B Hs Ws / ppn_gennet_s2_tile()), ppn_gennet_s2_max_blocks()); < 0 for sizes the entry refuses.
 * ppn_gennet_s2_tile(): the small pixels of one workgroup tile (512).  ppn_gennet_s2_max_blocks(): the most workgroups of W; past that
 * many tiles a workgroup strides.
 *
 * C = 24 only.  Before any HIP call: PPN_E_INVALID for a NULL required pointer, a tensor, weight or workspace pointer that is not 16-byte
 * aligned (bias, sum_small, sum_big: 4), an extent below 1, a dtype outside {0, 1}, 2^31 elements and more in big; PPN_E_UNSUPPORTED for
 * another C. */
int     ppn_gennet_s2_tile(void);
int     ppn_gennet_s2_max_blocks(void);
int64_t ppn_gennet_s2_wgrad_workspace(int B, int Hs, int Ws);            /* bytes; < 0 for sizes the entry refuses */
int     ppn_gennet_s2_down (const void* big, const float* w, const float* bias /* may be NULL */, void* small,
                            int B, int H, int W, int C, int dtype, void* stream);
int     ppn_gennet_s2_up   (const void* small, const float* w, const float* bias /* may be NULL */, void* big,
                            int B, int H, int W, int C, int dtype, void* stream);          /* H, W: the BIG extent */
int     ppn_gennet_s2_wgrad(const void* small, const void* big, void* workspace, float* dw,
                            float* sum_small /* may be NULL */, float* sum_big /* may be NULL */,
                            int B, int H, int W, int C, int dtype, void* stream);

/* Bilinear x2 up-sampling of an NHWC tensor x [B][H][W][C] -> y [B][2H][2W][C] with PyTorch's
 * F.interpolate(scale_factor=2, mode="bilinear", align_corners=False) arithmetic (the SETR-UP head's Upsample,
 * SegNet/mmseg/ops/wrappers.py:30-51); relu != 0 applies max(x, 0) to the input first (the ConvModule's ReLU,
 * setr_up_head.py:53-66). C a multiple of 8; dtype 0 = float32, 1 = bfloat16. */
int ppn_upsample2x_nhwc(const void* x, void* y, int32_t B, int32_t H, int32_t W, int32_t C, int32_t relu,
                        int32_t dtype, void* stream);
/* Same with a per-channel bias [C] added before the ReLU: the preceding convolution then runs without its (BatchNorm-
 * folded) bias and its separate add pass (mmcv ConvModule conv -> bn -> ReLU -> Upsample, setr_up_head.py:56-66). */
int ppn_upsample2x_nhwc_bias(const void* x, const void* bias, void* y, int32_t B, int32_t H, int32_t W, int32_t C,
                             int32_t relu, int32_t dtype, void* stream);
/* y = add + (x resized x2): the FPN's top-down step (uper_head.py:103-108: `laterals[i - 1] += resize(laterals[i], size=prev_shape,
 * mode='bilinear', align_corners=False)`) when the finer level is exactly twice the coarser one.  x [B][H][W][C], add and y
 * [B][2H][2W][C]; add may be y.  The resized value is rounded to the tensor's type before the sum, as the two separate kernels do. */
int ppn_upsample2x_add_nhwc(const void* x, const void* add, void* y, int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype, void* stream);
/* UPerPUPHead's FPN output assembly (SegNet/mmseg/decode_heads/uper_pup_head.py:121-128: the last `Upsample(scale_factor=2,
 * mode='bilinear', align_corners=False)` of every FPN chain, then `torch.cat(fpn_outs, dim=1)`) in one pass: n <= 8 NHWC tensors
 * x[l] [B][H][W][channels[l]] of ONE size (HOST arrays of pointers / channel counts; channels % 8 == 0), each up-sampled x2 with
 * ppn_upsample2x_nhwc's arithmetic into channels [off_l, off_l + channels[l]) of out [B][2H][2W][sum channels], off_l the sum of the
 * channels before it.  64-bit offsets: out may pass 2^32 bytes.  n outside 1..8, a NULL pointer, a bad size or dtype, or a grid past
 * the launch limits (B (H + 1) >= 2^31; (W + 1) max(channels) / 8 > 65535 * 256) return PPN_E_INVALID before any HIP call.
 * dtype 0 = float32, 1 = bfloat16. */
int ppn_upsample2x_concat_nhwc(const void* const* x, const int32_t* channels, int32_t n, void* out, int32_t B, int32_t H, int32_t W, int32_t dtype,
                               void* stream);
/* UPerHead's FPN output assembly (mmseg/decode_heads/uper_head.py:117-127: `resize(fpn_outs[i], size=fpn_outs[0].shape[2:],
 * mode='bilinear', align_corners=False)` for i = 1..3, then `torch.cat(fpn_outs, dim=1)`) in one pass over NHWC tensors:
 * out [B][H0][W0][4 C], channels [l C, (l + 1) C) = level l resized to H0 x W0 (level 0 copied).  x_l is [B][hw[2 l]][hw[2 l + 1]][C]
 * (host array hw[8], no level larger than level 0); PyTorch's upsample_bilinear2d arithmetic per output.  C % 8 == 0; dtype 0
 * float32, 1 bfloat16. */
int ppn_resize_concat4_nhwc(const void* x0, const void* x1, const void* x2, const void* x3, const int32_t* hw, void* out, int32_t B, int32_t C,
                            int32_t dtype, void* stream);
/* The general form: n <= 8 NHWC tensors x[l] [B][hw[2 l]][hw[2 l + 1]][channels[l]] (HOST arrays of pointers / sizes; channels % 8 == 0),
 * each resized (bilinear, align_corners False; a tensor of level 0's size is copied) to level 0's size and written to its channel
 * range of out [B][H0][W0][sum channels].  Also the pyramid pooling module's output, psp_head.py:48-60 + uper_head.py:76-84:
 * `torch.cat([x] + [resize(ppm(x), size=x.shape[2:], mode='bilinear')...], dim=1)` with the pooled maps smaller than x. */
int ppn_resize_concat_nhwc(const void* const* x, const int32_t* hw, const int32_t* channels, int32_t n, void* out, int32_t B, int32_t dtype,
                           void* stream);
/* The backward of the three up-sampling entries above, for training the decode heads on them.  All are gathers: one writer per dx
 * element, no atomics, float32 sums in a fixed order, one rounding to the tensor type — two calls on the same inputs give the same
 * bits — and every dx element is written (no zero-filled buffer is assumed).  NHWC, channels % 8 == 0, dtype 0 = float32,
 * 1 = bfloat16, 64-bit offsets.  Every argument check returns PPN_E_INVALID before any HIP call.
 *
 * ppn_upsample2x_nhwc_bwd: dy [B][2H][2W][C] -> dx [B][H][W][C], the exact transpose of ppn_upsample2x_nhwc: input row r gathers
 * output rows 2r-1, 2r, 2r+1, 2r+2 with weights 0.25 [r >= 1], w0, w1, 0.25 [r <= H-2], w0 = 1 if r == 0 else 0.75, w1 = 1 if
 * r == H-1 else 0.75 (the clamped borders fold onto the edge rows), the same along x: 16 taps per element.  x, when not NULL, is the
 * forward's input BEFORE its folded ReLU ([B][H][W][C]): dx is zeroed where x <= 0.  Also the backward of ppn_upsample2x_add_nhwc with
 * respect to its coarse operand (x = NULL; with respect to `add` it is the identity).  H == 1 and W == 1 are valid.  Limits, as the
 * forward's: B (H + 1) < 2^31, (W + 1) C / 8 <= 65535 * 256, H and W < 2^30. */
int ppn_upsample2x_nhwc_bwd(const void* dy, const void* x, void* dx, int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype, void* stream);
/* The backward of ppn_upsample2x_concat_nhwc: dx[l] [B][H][W][channels[l]] = the transpose above applied to channels
 * [off_l, off_l + channels[l]) of dout [B][2H][2W][sum channels] (HOST arrays of n = 1..8 pointers / channel counts), one launch.
 * The forward entry's limits. */
int ppn_upsample2x_concat_nhwc_bwd(const void* dout, void* const* dx, const int32_t* channels, int32_t n, int32_t B, int32_t H, int32_t W,
                                   int32_t dtype, void* stream);
/* The backward of ppn_resize_concat_nhwc: dx[l] [B][hw[2 l]][hw[2 l + 1]][channels[l]] from dout [B][hw[0]][hw[1]][sum channels].  A
 * level of level 0's size receives a copy of its channel slice; otherwise input pixel (r, q) gathers every output pixel whose taps
 * (y0, y1) x (x0, x1) include it, with the weights the forward kernel's own float32 formula gives that output, so forward and
 * backward agree on every tap.  No level may be larger than level 0 (PPN_E_INVALID); B hw[0] hw[1] < 2^31 and fewer than 2^31
 * blocks of 256 threads (B hw[0] hw[1] max(channels) / 8 work-items at most). */
int ppn_resize_concat_nhwc_bwd(const void* dout, void* const* dx, const int32_t* hw, const int32_t* channels, int32_t n, int32_t B, int32_t dtype,
                               void* stream);
/* The pyramid pooling module's pools (psp_head.py:33-38: `nn.AdaptiveAvgPool2d(s)` for each pool scale) of one NHWC tensor
 * x [B][H][W][C] in one launch: y[k] [B][scales[k]][scales[k]][C], k < n <= 4 (HOST arrays), PyTorch's bins
 * (rows floor(i H / s) .. ceil((i + 1) H / s) - 1), summed in float32.  C % 8 == 0. */
int ppn_adaptive_pools_nhwc(const void* x, void* const* y, const int32_t* scales, int32_t n, int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype,
                            void* stream);
/* SegNet's input straight from stage B's occupancy codes: img [n_pixels][3] (NHWC) = (rgb - mean3) / std3 with rgb = (255,255,255)
 * for PPN_GRID_FREE, (255,0,0) for PPN_GRID_MARK, (0,0,0) otherwise (process_map.py:120,128; planning_seg.py:12-41).
 * mean3 / std3 are HOST pointers to three floats; n_pixels a multiple of 8. */
int ppn_grid_to_image(const uint8_t* grid, void* img, int64_t n_pixels, const float* mean3, const float* std3, int32_t dtype,
                      void* stream);
/* SegNet's TRAINING input: the reference's train_pipeline (SegNet/configs/_base_/datasets/planning_seg.py:18-27) RandomFlip(0.5) ->
 * PhotoMetricDistortion -> Normalize -> Pad(size, pad_val 0, seg_pad_val 255) on the device, image and labels together.
 *
 * Per-image parameters: params [B][PPN_AUG_PARAM_WORDS] 32-bit words = { flags (PPN_AUG_* bits), beta float32 (brightness),
 * alpha float32 (contrast), alpha_s float32 (saturation), delta int32 (hue), 0, 0, 0 }; any caller may fill them, ppn_augment_params
 * draws them.  The colour function on one BGR u8 pixel, in this order (mmseg/datasets/pipelines/transforms.py:835-940):
 * brightness convert(x, 1, beta); contrast convert(x, alpha, 0) here unless PPN_AUG_CONTRAST_LAST; saturation BGR -> HSV,
 * S = convert(S, alpha_s, 0), HSV -> BGR; hue BGR -> HSV, H = (H + delta) mod 180 (non-negative), HSV -> BGR (a second round trip, as
 * in the reference); contrast when PPN_AUG_CONTRAST_LAST.  A step whose flag is off is skipped entirely.  convert(x, a, b) =
 * float32(x) * a + b as two separately rounded float32 operations, clipped to [0, 255], truncated toward zero.  HSV is the documented
 * OpenCV 8-bit form (H in [0, 180)) in exact integer arithmetic with round-half-up (DESIGN.md 18 states it; OpenCV's own roundings
 * are NOT pinned against it).  Then channel c of RGB: (float32(v) - mean3[c]) / std3[c], IEEE float32 (ppn_grid_to_image's
 * expression), rounded to bfloat16 for dtype 1.  With PPN_AUG_FLIP output column x shows source column W - 1 - x, image and label
 * alike.  img_out [B][Ho][Wo][3] (NHWC) and label_out [B][Ho][Wo] are WRITTEN for every pixel: outside the H x W source the image is
 * 0.0 and the label seg_pad_val (its low 8 bits).  Labels: label_in [B][H][W] u8 and label_out both given, or both NULL.
 * mean3 / std3 are HOST pointers to three floats.  W % 8 == 0, Wo % 8 == 0, Ho >= H, Wo >= W.
 *
 * ppn_augment_params: one work-item per image; draws d0..d9 = Philox doubles (numpy recipe) of (seed, stream 5, instance
 * first_instance + b), fixed slots: d0 < flip_ratio flip; d1 < 0.5 brightness on, beta = -brightness_delta + 2 brightness_delta d2;
 * d3 < 0.5 contrast first (else PPN_AUG_CONTRAST_LAST); d4 < 0.5 contrast on, alpha = contrast_lo + (contrast_hi - contrast_lo) d5;
 * d6 < 0.5 saturation on, alpha_s likewise from d7; d8 < 0.5 hue on, delta = -hue_delta + floor(2 hue_delta d9) (the upper bound is
 * excluded, as numpy.random.randint does).  Double arithmetic, stored as float32 / int32.  The reference's defaults: 0.5, 32,
 * 0.5, 1.5, 0.5, 1.5, 18.
 * ppn_augment_codes: grid [B][H][W] u8 occupancy codes, rendered with ppn_grid_to_image's palette (free white, marker red, anything
 * else black).  A distorted palette image still has three colours per image: each workgroup distorts the three colours once and a
 * pixel costs selects only.  With flags 0 and Ho == H, Wo == W the image is bit for bit ppn_grid_to_image's.
 * ppn_augment_rgb: rgb [B][H][W][3] u8, channel order RGB; the same colour function per pixel.
 * NULL grid / rgb / params / img_out / mean3 / std3, one label pointer without the other, a size <= 0, W % 8 or Wo % 8 != 0, Ho < H,
 * Wo < W, a dtype other than 0 / 1, grid / rgb / label_in / label_out not 8-byte aligned, img_out / params not 16-byte aligned,
 * B Ho Wo 3 >= 2^31 or a launch of 2^31 work-items or more return PPN_E_INVALID before any HIP call; so do, for ppn_augment_params,
 * NULL / misaligned params, B <= 0 and a setting outside flip_ratio in [0, 1], brightness_delta in [0, 255],
 * 0 <= lo <= hi <= 255, hue_delta in [0, 180]. */
#define PPN_AUG_FLIP            1u
#define PPN_AUG_BRIGHTNESS      2u
#define PPN_AUG_CONTRAST        4u
#define PPN_AUG_CONTRAST_LAST   8u
#define PPN_AUG_SATURATION     16u
#define PPN_AUG_HUE            32u
#define PPN_AUG_PARAM_WORDS     8
int ppn_augment_params(uint64_t seed, uint64_t first_instance, int B, double flip_ratio, double brightness_delta, double contrast_lo,
                       double contrast_hi, double saturation_lo, double saturation_hi, int hue_delta,
                       uint32_t* params /* [B][8] */, void* stream);
int ppn_augment_codes(const uint8_t* grid /* [B][H][W] */, const uint8_t* label_in /* [B][H][W], may be NULL */,
                      const uint32_t* params /* [B][8] */, void* img_out /* [B][Ho][Wo][3] f32 | bf16 */,
                      uint8_t* label_out /* [B][Ho][Wo], NULL with label_in */, int B, int H, int W, int Ho, int Wo,
                      const float* mean3, const float* std3, int seg_pad_val, int dtype /* 0 f32, 1 bf16 */, void* stream);
int ppn_augment_rgb(const uint8_t* rgb /* [B][H][W][3] */, const uint8_t* label_in /* [B][H][W], may be NULL */,
                    const uint32_t* params /* [B][8] */, void* img_out /* [B][Ho][Wo][3] f32 | bf16 */,
                    uint8_t* label_out /* [B][Ho][Wo], NULL with label_in */, int B, int H, int W, int Ho, int Wo,
                    const float* mean3, const float* std3, int seg_pad_val, int dtype /* 0 f32, 1 bf16 */, void* stream);
/* The segmentor's output tail for two classes (setr_up_head.py:78-80, encoder_decoder.py:76-79,242,257): logits [B][2][h][w]
 * (NCHW) -> bilinear x2 -> bilinear to [Ho][Wo] (both align_corners=False, each rounded to the logits' dtype as the
 * materialised tensors are) -> float32 softmax -> argmax, labels u8 [B][Ho][Wo] in {0,1}. */
int ppn_seg_labels_2class(const void* logits, uint8_t* labels, int32_t B, int32_t h, int32_t w, int32_t Ho, int32_t Wo,
                          int32_t dtype, void* stream);
/* In place x = leaky_relu(x + bias[c], negative_slope) on n elements of an NHWC tensor with C channels (C % 8 == 0;
 * slope 0 = ReLU, 1 = bias only): bias + BatchNorm(folded) + LeakyReLU of GenNet's conv stages (ae_vit.py:17-55) as
 * one pass behind a bias-free library convolution. */
int ppn_bias_act_nhwc(void* x, const void* bias, int64_t n, int32_t C, float negative_slope, int32_t dtype, void* stream);

/* The single-channel 3x3 convolutions at the two ends of GenNet's AE-ViT (ae_vit.py:17-20,58; stride 1, padding 1) as
 * direct kernels, float32 accumulation, weights and bias float32 on the device:
 *   _c1  : x [B][H][W] -> y [B][H][W][Cout] (NHWC), y = leaky_relu(conv(x, w[Cout][1][3][3]) + bias[Cout], negative_slope)
 *          (the BatchNorm folded into w / bias by the caller), Cout in {8,16,24,32};
 *   _to1 : x [B][H][W][Cin] (NHWC) -> y [B][H][W], y = conv(x, w[1][Cin][3][3]) + bias, Cin in {8,16,24,32}. */
int ppn_conv3x3_c1_nhwc(const void* x, const float* w, const float* bias, void* y, int32_t B, int32_t H, int32_t W,
                        int32_t Cout, float negative_slope, int32_t dtype, void* stream);
int ppn_conv3x3_to1_nhwc(const void* x, const float* w, float bias, void* y, int32_t B, int32_t H, int32_t W, int32_t Cin,
                         int32_t dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * bf16 MFMA kernels (v_mfma_f32_16x16x32_bf16, float32 accumulation; ppnet_amd/csrc/mfma_gemm.h).
 *
 * 3x3 convolution, padding 1, stride 1 or 2, as an implicit GEMM on NHWC bfloat16: x [B][H][W][Cin] -> y [B][Ho][Wo][Cout],
 * y = act(conv(x, w) + bias), act = ReLU when relu != 0.  w is [Cout][3][3][Cin] (the torch weight [Cout][Cin][3][3]
 * permuted to (0, 2, 3, 1)); bias [Cout] float32 (zeros for a bias-free convolution).  Cin % 64 == 0, Cout % 8 == 0.
 * Replaces mmcv's ConvModule conv -> (folded) BatchNorm -> ReLU of the SETR-UP head (setr_up_head.py:53-66) and the bias-free
 * stride-2 convolution of NAT's ConvDownsampler (SegNet/nat.py:48-59). */
int ppn_conv3x3_mfma_bf16(const void* x, const void* w, const float* bias, void* y, int32_t B, int32_t H, int32_t W, int32_t Cin,
                          int32_t Cout, int32_t stride, int32_t relu, void* stream);
/* The head's last stage (setr_up_head.py:78-80 with the 1x1 classifier commuted in front of the last up-sampling):
 * logits[m][c] += sum_n max(conv(x, w)[m][n] + bias[n], 0) * w2[c][n] for the B*H*W pixels m and c = 0, 1.
 * logits [B*H*W][2] float32 must hold the classifier's bias on entry; w2 [2][Cout] float32.  The Cout-channel activation is
 * never written: a workgroup adds the sums of its 256-column block in a fixed order (through LDS) and, when Cout <= 256, onto the
 * logits directly — ppn_conv3x3_relu_classify2_slots(Cout) is then 0 and `partial` may be NULL.  Wider convolutions leave one partial
 * sum per pixel, class and 256-column block in partial [ppn_conv3x3_relu_classify2_slots(Cout)][B*H*W][2] float32 (caller-owned
 * workspace, every element written; 16 bytes per pixel at Cout = 512 — round 4: 32) and a second launch adds the slots to logits in
 * slot order.  No atomics anywhere: bit-reproducible. */
int32_t ppn_conv3x3_relu_classify2_slots(int32_t Cout);
int ppn_conv3x3_relu_classify2_bf16(const void* x, const void* w, const float* bias, const float* w2, float* logits, float* partial, int32_t B,
                                    int32_t H, int32_t W, int32_t Cin, int32_t Cout, void* stream);
/* GenNet's 24-channel stride-2 stages on MFMA, NHWC bfloat16, BatchNorm folded by the caller, bias + LeakyReLU fused:
 *   transposed == 0 (ae_vit.py:24-36, Conv2d(24, 24, 3, 2, 1)): x [B][H][W][24] -> y [B][H/2][W/2][24];
 *        w [32][224] bfloat16, row co (24..31 zero), column (ky*3+kx)*24 + ci (216..223 zero);
 *   transposed != 0 (ae_vit.py:44-55, ConvTranspose2d(24, 24, 3, 2, 1, output_padding=1)): x [B][H][W][24] -> y [B][2H][2W][24];
 *        w [4][32][96] bfloat16: output parity class (oy & 1) * 2 + (ox & 1), row co, column (dy*2+dx)*24 + ci over the 2x2
 *        input block under the 2x2 output block, zero where the class has no tap (ppnet_amd/gennet.py packs both).
 * bias [32] float32 (24..31 zero). */
int ppn_gennet_conv_s2_bf16(const void* x, const void* w, const float* bias, void* y, int32_t B, int32_t H, int32_t W, float negative_slope,
                            int32_t transposed, void* stream);
/* GenNet's LAST decoder stage fused with its final convolution (ae_vit.py:44-58: ConvTranspose2d(24, 24, 3, 2, 1, output_padding=1) + BN +
 * LeakyReLU, then Conv2d(24, 1, 3, 1, 1)): x [B][H][W][24] bfloat16 -> y [B][2H][2W] bfloat16; the 24-channel tensor at the output
 * resolution never reaches memory.  w / bias / negative_slope: the decoder stage as for ppn_gennet_conv_s2_bf16 (transposed form);
 * w_final [24][9] float32 (input channel, tap ky*3+kx) = the final convolution's weight [1][24][3][3]; bias_final its bias.
 * Bit-identical to ppn_gennet_conv_s2_bf16 followed by ppn_conv3x3_to1_nhwc on bfloat16 tensors. */
int ppn_gennet_dec_final_bf16(const void* x, const void* w, const float* bias, float negative_slope, const float* w_final, float bias_final, void* y,
                              int32_t B, int32_t H, int32_t W, void* stream);
/* GenNet's first convolution fused into its first encoder stage (ae_vit.py:24-36: Conv2d(1, 24, 3, 1, 1) + BN + LeakyReLU, then
 * Conv2d(24, 24, 3, 2, 1) + BN + LeakyReLU; BatchNorms folded by the caller): x1 [B][H][W] bfloat16 -> y [B][H/2][W/2][24] bfloat16, the
 * 24-channel full-resolution tensor in between never reaches memory.  H, W even.
 *   w1 [2][16][32] bfloat16: row = channel (24..31 zero), columns 0..8 = bfloat16(w[c][tap]) (hi), 16..24 = bfloat16(w - hi) (lo),
 *       columns 9 / 25 = hi / lo of the bias (the kernel feeds a constant 1 there), else 0;  b1 [32] float32: unused, kept for the layout;
 *   the first LeakyReLU's slope must be <= 1;
 *   wk2 [2][9][16][32] bfloat16: [co tile][tap ky*3+kx][co row][k-slot], slot 8g + e = input channel 4g + e (e < 4) or
 *       16 + 4g + e - 4 (e >= 4, g < 2; zero for g >= 2);  bias2 [32] float32.  ppnet_amd/gennet.py packs all four. */
int ppn_gennet_first_enc_bf16(const void* x1, const void* w1, const float* b1, const void* wk2, const float* bias2, void* y, int32_t B, int32_t H, int32_t W,
                              float slope1, float slope2, void* stream);
/* The ViT blocks of GenNet's AE-ViT (ae_vit.py:38-42,68-70; vit.py:88-161: pre-LN attention + MLP residual blocks, dim 24, 3 heads,
 * MLP x4, LayerNorm eps 1e-6, erf GELU) as one kernel: x, y [B][N][24] bfloat16 token rows (the NHWC feature map), N <= 1024,
 * N % 8 == 0.  One workgroup per problem holds the residual stream in registers (float32) across all n_blocks blocks and the
 * block's K / V in LDS.  params: [n_blocks][PPN_GENNET_BLOCK_PARAMS] float32, per block in this order:
 *   norm1.weight[24] norm1.bias[24] attn.qkv.weight[72][24] attn.qkv.bias[72] attn.proj.weight[24][24] attn.proj.bias[24]
 *   norm2.weight[24] norm2.bias[24] mlp.fc1.weight[96][24] mlp.fc1.bias[96] mlp.fc2.weight TRANSPOSED [96][24] mlp.fc2.bias[24] */
#define PPN_GENNET_BLOCK_PARAMS 7224
int ppn_gennet_trunk_bf16(const void* x, void* y, const float* params, int32_t B, int32_t N, int32_t n_blocks, void* stream);
/* extract_path's result as a fixed-size polyline per problem (process_map.py:355-359): full[b] = [init[b]] + wp[b][:wp_n[b]] * rate +
 * [end[b]] in a [n][max_wp + 2][2] float64 array (rows beyond the plan: wp * rate, i.e. zeros), counts[b] = ok[b] ? wp_n[b] + 2 : 0.
 * wp [n][max_wp][2] / wp_n / ok are ppn_extract_paths' outputs, init / end the full-resolution states. */
int ppn_assemble_paths(const double* wp, const int32_t* wp_n, const uint8_t* ok, const double* init, const double* end, double rate, int32_t n,
                       int32_t max_wp, double* full, int32_t* counts, void* stream);
/* collision[b] = any consecutive-waypoint segment i < counts[b] - 1 of plan b hits any of its first n_obstacles[b] obstacle rows
 * (process_map.py:491-495 over collision_check_circle_edge, :383-425; same float32 arithmetic as ppn_collision_segments_bound).
 * waypoints [B][M][2] float64; obstacles [B][S][3] rows (ox, oy, size), float32 or float64 (obstacles_f64 != 0). */
int ppn_plan_collision(const double* waypoints, const int32_t* counts, const void* obstacles, int32_t obstacles_f64, const int32_t* n_obstacles,
                       int32_t B, int32_t M, int32_t S, float clearance, float bound, uint8_t* collision, void* stream);
/* GenNet's output -> 8-bit heat map, per sample (GenNet/predict.py:95-102): out[b][i] = (uint8)(((y[b][i] - min_b) / (max_b - min_b)) * 255),
 * float32 arithmetic in that order (bit-identical to the torch composition), y [B][n] float32 (dtype 0) or bfloat16 (1). */
int ppn_heatmap_u8(const void* y, uint8_t* out, int32_t B, int32_t n, int32_t dtype, void* stream);
/* SegNet's first tokenizer convolution (SegNet/nat.py:24-40, Conv2d(3, 64, 3, stride 2, padding 1)) straight from the occupancy
 * codes grid [B][H][W] u8: the input image is a 3-colour palette (see ppn_grid_to_image), so the convolution is a 64 x 28 table
 * times a one-hot column per output pixel.  lut [2][64][32] bfloat16: hi and lo halves of the float32 table
 * L[co][3 * (ky * 3 + kx) + colour] = sum_ci w[co][ci][ky][kx] * image_ci(colour)  (colour 0 free, 1 marker, 2 other), column 27 =
 * bias (hi half only), 28..31 zero.  out [B][H/2][W/2][64] bfloat16.  H even, W % 32 == 0 (else PPN_E_UNSUPPORTED). */
int ppn_tokenizer_conv1_codes_bf16(const uint8_t* grid, const void* lut, void* out, int32_t B, int32_t H, int32_t W, void* stream);
/* SegNet's whole tokenizer (SegNet/nat.py:17-46: Conv2d(3, 64, 3, 2, 1) -> Conv2d(64, 128, 3, 2, 1) -> LayerNorm(128)) from the occupancy
 * codes grid [B][H][W] u8 in one kernel: tokens [B][H/4][W/4][128] bfloat16.  H % 4 == 0, W % 64 == 0 (else PPN_E_UNSUPPORTED).
 *   lut [2][64][32] bfloat16: the palette table of ppn_tokenizer_conv1_codes_bf16 with rows in natural channel order;
 *   w2p [8][9][2][16][32] bfloat16: the second convolution's weight as MFMA A fragments — [output tile nt][tap ky*3+kx][k-step s][row i][slot],
 *       row (nt, i) = output channel (nt>>2)*64 + 16*(i>>2) + 4*(nt&3) + (i&3), slot 8g + e = input channel (2s + (e>>2))*16 + 4g + (e&3);
 *   vec [3][128] float32: the second convolution's bias, the LayerNorm weight, the LayerNorm bias.  ppnet_amd/fused.py packs all three. */
int ppn_tokenizer_codes_bf16(const uint8_t* grid, const void* lut, const void* w2p, const float* vec, void* tokens, int32_t B, int32_t H, int32_t W,
                             float eps, void* stream);
/* The dense half of a 128-channel NAT layer (DiNAT-B level 0) as two token-streaming kernels with the weights resident in LDS
 * (SegNet/nat.py:101-153), bfloat16 token rows, float32 accumulation.  tokens % 16 == 0 (else PPN_E_UNSUPPORTED).
 *   ppn_nat128_ln_qkv_bf16:  qkv[tokens][384] = LN(s + offset) . w[384][128]^T + bias     (norm1 -> attn.qkv; offset, bias may be NULL)
 *   ppn_nat128_ln_mlp_bf16:  s[tokens][128] += GELU(LN(s + offset) . w1[256][128]^T + b1) . w2[128][256]^T   in place
 *                            (norm2 -> mlp.fc1 -> erf GELU -> mlp.fc2 -> residual; fc2's bias is carried by the caller's offset)
 *   ppn_nat128_ln_mlp_add_bf16: the same with final_add [128] float32 (may be NULL) added to the result — the last layer of a level
 *                            gives the residual stream its accumulated constant back here instead of in a separate pass over the tensor
 * offset [128] float32 is the constant part of the residual stream carried outside the tensor (ppn_layernorm_offset). */
int ppn_nat128_ln_qkv_bf16(const void* s, const float* offset, const void* ln_w, const void* ln_b, const void* w, const void* bias, void* qkv,
                           int64_t tokens, float eps, void* stream);
int ppn_nat128_ln_mlp_bf16(void* s, const float* offset, const void* ln_w, const void* ln_b, const void* w1, const void* b1, const void* w2,
                           int64_t tokens, float eps, void* stream);
int ppn_nat128_ln_mlp_add_bf16(void* s, const float* offset, const void* ln_w, const void* ln_b, const void* w1, const void* b1, const void* w2,
                               const float* final_add, int64_t tokens, float eps, void* stream);
/* s[tokens][128] += a[tokens][128] . w[128][128]^T in place, bfloat16 (the output projection + residual of a 128-channel NAT layer,
 * SegNet/nat.py:144-146, LayerScale folded into w by the caller, no bias): one streaming kernel, w resident in LDS.  tokens % 16 == 0. */
int ppn_nat128_proj_add_bf16(void* s, const void* a, const void* w, int64_t tokens, void* stream);

/* Dense projection c[M][N] = epilogue(a[M][K] . w[N][K]^T) on bfloat16 (torch.nn.Linear layout; SegNet/nat.py:62-85,111-120).
 * epilogue: 0 = + bias[n]; 1 = gelu(+ bias[n]) (erf form); 2 = c += (the residual stream accumulates, bias unused);
 * 3 = max(+ bias[n], 0) (a 1x1 ConvModule: convolution + folded BatchNorm + ReLU, mmseg/models/decode_heads/uper_head.py:40-63).
 * K % 64 == 0, K >= 128, N % 8 == 0.  persistent_blocks: 0 = one tile per workgroup; else the number of workgroups (a multiple
 * of 8, normally the CU count) that walk the tiles with the LDS-DMA stream running across tile boundaries (M, N % 256 == 0).
 * Few rows (fewer than 64 tiles of 256 x 256, N % 64 == 0: batches of 1-16 problems) go to a kernel of their own whatever
 * persistent_blocks says: a workgroup per 32 x 64 block of c, its four waves splitting K (csrc/gemm_small.hip). */
int ppn_gemm_bf16(const void* a, const void* w, const float* bias, void* c, int64_t M, int32_t N, int32_t K, int32_t epilogue,
                  int32_t persistent_blocks, void* stream);

/* Row-statistics partials per row that the accumulating mode of ppn_nat_gemm_bf16 writes for a residual stream of width C (and
 * that the LayerNorm modes expect to read for K = C): one per 128 columns at C = 256 (what ppn_nat_mlp_bf16 emits there too), one per
 * 256 columns for wider streams (round 4: per 128 up to C = 512).  C % 256 == 0; < 0: invalid. */
int32_t ppn_nat_gemm_partials(int32_t C);

/* The dense half of a NAT layer at C = 256 / 512 / 1024 with everything between two projections in the GEMMs' epilogues
 * (SegNet/nat.py:62-85 `Mlp.forward`, :140-153 `NATLayer.forward`; csrc/mfma_gemm.h, csrc/mfma_gemm.hip).  a [M][K], w [N][K]
 * (torch Linear layout), c [M][N], all bfloat16; M, N % 256 == 0, K % 64 == 0, K >= 128.
 *   mode 0: c = LN(a) w0^T + b0 computed from the RAW rows of a: the caller passes w = w0 diag(gamma), bias = b0 + w0 beta,
 *           colsum[n] = sum_k w[n][k] (of the bfloat16 values), and stats_in [partials_in][M][2] = partial (sum, sum of squares) of
 *           every row of a (1 <= partials_in <= 4, summed in order; the LayerNorm is over the K features, eps as given):
 *           c = rstd (a w^T - mean colsum) + bias.  K >= 192.
 *   mode 1: c = gelu(mode 0) (erf form; evaluated through a logistic fit of erf, |error| < 3e-5).
 *   mode 2: c += a w^T + bias IN PLACE, and stats_out [P][M][2], P = ppn_nat_gemm_partials(N), receives per column tile (sum, sum of
 *           squares) of every row of the NEW c over the tile's columns — of the bfloat16 values stored: what mode 0 / 1 of the
 *           next projection reads as stats_in with partials_in = P.  colsum / stats_in unused.  K >= 128.
 *   The partials of a row are summed in a fixed tree (lane quarter q takes partial q), not in index order: bit-reproducible, and
 *   equal to any other order to float32 rounding.
 * Behind it: ONE kernel, the persistent 256 x 256 core of csrc/mfma_gemm.h with these three epilogues (mode 2 reads the old c in
 * its epilogue).  The core addresses a and w with 32-bit byte offsets: M * K * 2 >= 2^32 or N * K * 2 >= 2^32 returns
 * PPN_E_UNSUPPORTED (as ppn_gemm_bf16).  Bit-reproducible (no atomics). */
int ppn_nat_gemm_bf16(const void* a, const void* w, const float* bias, const float* colsum, const float* stats_in, int32_t partials_in,
                      float* stats_out, void* c, int64_t M, int32_t N, int32_t K, int32_t mode, float eps, void* stream);

/* The MLP half of a NAT layer as ONE kernel (SegNet/nat.py:62-85 `Mlp.forward`, :147-153 of `NATLayer.forward`; csrc/nat_mlp.hip):
 *     s += gelu(LN(s) W1^T + b1) W2^T + b2        in place on the residual stream s [M][C] (bfloat16),
 * the hidden activation [M][HID] never written: it is produced and consumed chunk by chunk inside the compute unit.
 * ppn_nat_mlp_supported: 1 when (M, C, HID) is served (C = 256, M % 128 == 0 — a workgroup pass is 4 wave pairs x 32 rows —, 64 <= HID <= 2048, HID % 32 == 0), else 0 — callers fall back to two
 *   ppn_nat_gemm_bf16 calls (modes 1 and 2).
 * ppn_nat_mlp_pack_bf16: wpk [2 * C * HID] bfloat16 <- the two weights in the kernel's streaming order; w1 [HID][C] with the
 *   LayerNorm folded in (w1 = W1 diag(gamma)), w2 [C][HID] with LayerScale folded in (torch Linear layouts).  Once per weight change.
 * ppn_nat_mlp_bf16: hb [HID][2] float32 = (colsum_k w1[h][k] of the bfloat16 values, b1[h] + W1[h] . beta); b2 [C] float32;
 *   stats_out [C / 128][M][2] (or null) receives (sum, sum of squares) of every row of the NEW s per 128 columns, of the bfloat16
 *   values stored — the stats_in of the next ppn_nat_gemm_bf16 mode-0 call.  LayerNorm over the C features with `eps`; erf-GELU
 *   as x (1/2 + x~ q(x~^2)) with x~ = clamp(x, -4.25, 4.25) and q an odd-polynomial fit of (Phi(x) - 1/2) / x of degree 15 in x
 *   (no transcendental instruction; |gelu error| <= 9.2e-5 absolute, three times the 3e-5 of ppn_nat_gemm_bf16 mode 1's logistic
 *   fit — the bound bench.py's PARITY_TOLERANCE is sized against).  Bit-reproducible (no atomics). */
int32_t ppn_nat_mlp_supported(int64_t M, int32_t C, int32_t HID);
int ppn_nat_mlp_pack_bf16(const void* w1, const void* w2, void* wpk, int32_t C, int32_t HID, void* stream);
int ppn_nat_mlp_bf16(void* s, const void* wpk, const float* hb, const float* b2, float* stats_out, int64_t M, int32_t C, int32_t HID,
                     float eps, void* stream);

/* stats[rows][2] = (sum, sum of squares) of every row of the bfloat16 tensor x [rows][C], C % 8 == 0 in [64, 1024]: the
 * stats_in (partials_in = 1) of a level's first projection, whose input no mode-2 GEMM produced. */
int ppn_row_stats_bf16(const void* x, int64_t rows, int32_t C, float* stats, void* stream);

/* PIL.Image.resize(size, BILINEAR) for 8-bit single-channel images, bit-exact: Pillow's ImagingResample
 * (support = max(scale,1), 22-bit fixed-point coefficients, horizontal pass then vertical pass, each rounded
 * to 8 bits).  Used by extract_path's down-sampling (process_map.py:301).  in [n][H][W], tmp [n][H][outW],
 * out [n][outH][outW], all u8. */
int ppn_resize_bilinear_u8(const uint8_t* in, int32_t n, int32_t H, int32_t W, int32_t outH, int32_t outW,
                           uint8_t* tmp, uint8_t* out, void* stream);

/* `count` uniform doubles of Philox4x32-10 stream (seed, stream, instance), draw indices first..first+count-1,
 * exactly as the generator kernels draw them (tests pin this against oracle/philox_np.py). out[count] device. */
int ppn_philox_doubles(uint64_t seed, uint32_t stream_id, uint64_t instance, uint32_t first, int32_t count,
                       double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PPNET_HIP_H */
