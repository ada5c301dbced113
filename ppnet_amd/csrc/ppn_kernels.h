// ppn_kernels.h — kernel parameter blocks and launch prototypes (internal to libppnet_hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include "../../include/ppnet_hip.h"

#ifndef PPN_PATHS_THREADS
#define PPN_PATHS_THREADS 256
#endif

namespace ppn {

// ---- per-device launcher state.  Function attributes, device-resident constants and CU counts belong to the device that is
// current at the call; a process that drives several GPUs gets one slot per device ordinal (nothing here is shared between
// devices, and nothing is keyed by "first caller").
constexpr int PPN_MAX_DEVICES = 64;
inline int current_device() {
    int d = 0;
    return (hipGetDevice(&d) == hipSuccess && d >= 0 && d < PPN_MAX_DEVICES) ? d : -1;
}
struct DeviceOnce { std::atomic<int> done[PPN_MAX_DEVICES]; };       // static storage: zero-initialised
struct DeviceBuffer { std::atomic<void*> p[PPN_MAX_DEVICES]; };
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel, device): 0 or the HIP error
inline int dynamic_lds_once(DeviceOnce& o, const void* fn, int bytes) {
    const int d = current_device();
    if (d < 0) return (int)hipErrorInvalidDevice;
    if (o.done[d].load(std::memory_order_acquire)) return 0;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return (int)e;
    o.done[d].store(1, std::memory_order_release);
    return 0;
}
// Region size (16 / 8 / 4 queries a side) of the matrix-core neighbourhood-attention kernels for a dilation group of hq x wq queries:
// the cheapest cover, priced per covered query cell.  Measured on 11 x 11 groups (DiNAT-B's dilation-3 layers at 32 x 32 tokens,
// batch 256: tools/na_timing_512.py): 16 x 16 regions 0.52 ms (47 % of the cells used), 8 x 8 0.97 ms, 4 x 4 1.56 ms (84 % used; the
// v_dot2 kernel 2.23 ms) — per cell 1 : 1.9 : 5.3.  Rounds 2-3 chose by lane utilisation alone and took the 4 x 4 form here.
inline int na_region_size(int hq, int wq) {
    auto cells = [&](int t) { return (double)((hq + t - 1) / t * t) * (double)((wq + t - 1) / t * t); };
    const double c16 = cells(16), c8 = 1.9 * cells(8), c4 = 5.3 * cells(4);
    return (c16 <= c8 && c16 <= c4) ? 16 : (c8 <= c4 ? 8 : 4);
}

// compute units of the current device (cached per device; 0 when the query fails)
inline int device_cu_count() {
    static std::atomic<int> cus[PPN_MAX_DEVICES];
    const int d = current_device();
    if (d < 0) return 0;
    int v = cus[d].load(std::memory_order_relaxed);
    if (!v) {
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || v <= 0) return 0;
        cus[d].store(v, std::memory_order_relaxed);
    }
    return v;
}

struct PathsParams {
    ppn_paths_t out;
    int n_paths;
    uint64_t first_id;
    int R;
    double map_size, clearance;
    uint64_t seed;
    const double* draws;       // [n][PPN_DRAWS_PER_PATH] or null
    const float* pocket;       // [n][pocket_stride] or null
    int pocket_stride;
    const double* W;           // [4][1000] least-squares operator (device)
    const int8_t* force_straight;  // [n] or null
    const int32_t* hull_start;     // [n] or null: first hull vertex as an index into the canonical cycle (-1 / null = canonical)
};

struct MapsParams {
    ppn_paths_t paths;
    ppn_maps_t out;
    int n_paths, placements, n_maps;
    uint64_t first_map_id;
    int R;
    double map_size, obstacles_size, clearance;
    int K;
    uint64_t seed;
    const double* place_draws; // [n_maps][3] or null
    const double* obst_draws;  // [n_maps][3K] or null
    int force_compose;         // validation: never skip the corridor compose
};

__global__ void edage_paths_kernel(PathsParams prm);
// phase: 1 = placement / labels / filter, 2 = obstacle lists -> grid, 3 = both in one kernel
int edage_maps_launch(int phase, const MapsParams& prm, hipStream_t stream);
__global__ void boundary_check_kernel(const double* hull, int hull_n, const double* angle_deg,
                                      const double* trans_rc, int n, int R, uint8_t* ok, double* hull_out);
__global__ void obstacle_filter_kernel(const double* pathpoint, const double* draws, int n, int K, int R,
                                       double map_size, double obstacles_size, double clearance, uint8_t* accept,
                                       double* obstacles, int32_t* counts);
__global__ void paint_markers_kernel(uint8_t* grid, int n, int R, const double* init, const double* end);
__global__ void disc_raster_kernel(const double* obstacles, const int32_t* counts, int stride,
                                   int n_maps, int R, uint8_t* grid);
__global__ void collision_segments_kernel(const float* s, const float* e, const int32_t* prob, int n_seg,
                                          const float* obs, const int32_t* obs_off, float clearance,
                                          float bound, uint8_t* hit);
__global__ void extract_paths_kernel(const float* heat, int n, int H, int W, const double* init,
                                     const double* end, int max_wp, double* wp, int32_t* wp_n, uint8_t* ok, int vis_dim, int stage_heat);

constexpr int PPN_RESIZE_REP = 16;      // lines / images one thread of resize_pass_kernel walks with its filter weights
__global__ void resize_pass_kernel(const uint8_t* in, int n, int inH, int inW, int outH, int outW, int horizontal,
                                   uint8_t* out);
__global__ void philox_doubles_kernel(uint64_t seed, uint32_t stream_id, uint64_t instance, uint32_t first, int count,
                                      double* out);

int na2d_launch(const void* qkv, const void* pad_kv, const float* rpb, void* out, int B, int H, int W, int Hr, int Wr, int heads, int dil,
                float scale, int dtype, hipStream_t stream);

const void* zero_line();
int na2d_mfma_launch(const void* qkv, const void* pad_kv, const float* rpb, void* out, int B, int H, int W, int Hr, int Wr, int heads, int dil,
                     float scale, hipStream_t stream);
int na2d_halo16_launch(const void* qkv, const void* pad_kv, const float* rpb, void* out, int B, int H, int W, int Hr, int Wr, int heads, int dil,
                       float scale, const void* zero, hipStream_t stream);
long long na2d_bwd_workspace_floats(int B, int H, int W, int heads, int dil);
int na2d_bwd_launch(const void* qkv, const float* rpb, const void* dout, void* dqkv, float* drpb, float* workspace, int B, int H, int W, int heads,
                    int dil, float scale, int dtype, hipStream_t stream);
long long na2d_bwd_vpad_workspace_floats(int B, int H, int W, int Hr, int Wr, int heads, int dil);
int na2d_bwd_vpad_launch(const void* qkv, const void* pad_kv, const float* rpb, const void* dout, void* dqkv, float* dpad_kv, float* drpb,
                         float* workspace, int B, int H, int W, int Hr, int Wr, int heads, int dil, float scale, int dtype, hipStream_t stream);

int norm_launch(const void* x, const void* a, const void* gamma, const void* w, const void* b, void* x_out, void* y_out,
                long long rows, int C, float eps, int dtype, int Hr, int Wr, int Hp, int Wp, const void* xoff, hipStream_t stream);

// residual_ln_bwd.hip: the training pair of norm_launch's residual form (scale [rows / rows_per_image] float32 or null; -1 = a width the
// kernels do not take; the workspace holds residual_ln_bwd_workspace_floats(rows, C) floats)
long long residual_ln_bwd_workspace_floats(long long rows, int C);
int residual_ln_train_fwd_launch(const void* x, const void* a, const void* gamma, const float* scale, const void* w, const void* b, void* x_out,
                                 void* y_out, float* stats, long long rows, long long rows_per_image, int C, float eps, int dtype, hipStream_t stream);
int residual_ln_bwd_launch(const void* gy, const void* gx, const void* xn, const float* stats, const void* a, const void* gamma, const float* scale,
                           const void* w, void* dx, void* da, void* dgamma, void* dw, void* dbeta, float* workspace, long long rows,
                           long long rows_per_image, int C, int dtype, hipStream_t stream);

// patch_merge_ln.hip: DiNAT_s's 2 x 2 patch gather fused with the LayerNorm over 4C, forward and backward; rows per workgroup tile
// (0 = a width the kernels do not take), the workgroup cap, the backward's workspace in bytes (-1 = not taken).  Launches: -1 = width
int patch_merge_ln_rows(int C);
int patch_merge_ln_max_blocks();
long long patch_merge_ln_bwd_workspace_bytes(long long rows, int C);
int patch_merge_ln_fwd_launch(const void* x, const void* gamma, const void* beta, void* y, float* stats, int B, int H, int W, int C, float eps,
                              int dtype, hipStream_t stream);
int patch_merge_ln_bwd_launch(const void* gy, const void* x, const float* stats, const void* gamma, float* workspace, void* dx, void* dgamma,
                              void* dbeta, int B, int H, int W, int C, int dtype, hipStream_t stream);

// gennet_stem_train.hip: the training pair of GenNet's stem (Conv2d(1, C, 3, 1, 1) + BatchNorm2d on batch statistics + LeakyReLU), C in
// {8, 16, 24, 32}; pixels per workgroup tile, the workgroup cap of the reducing kernels, the workspace in bytes for n = B H W pixels
// (-1 = not taken).  Launches: -1 = a channel count the kernels do not take
int gennet_stem_channels_ok(int C);
int gennet_stem_tile();
int gennet_stem_max_blocks();
long long gennet_stem_train_workspace_bytes(long long n, int C);
int gennet_stem_train_fwd_launch(const float* x, const float* w, const float* bias, const float* gamma, const float* beta, void* z, float* stats,
                                 double* moments, void* workspace, int B, int H, int W, int C, float eps, float slope, int dtype, hipStream_t stream);
int gennet_stem_train_bwd_launch(const void* dz, const float* x, const float* w, const float* bias, const float* gamma, const float* beta,
                                 const float* stats, const double* moments, void* workspace, float* dw, float* dgamma, float* dbeta, int B, int H, int W,
                                 int C, float slope, int dtype, hipStream_t stream);

// gennet_tail_train.hip: the training pair of GenNet's tail (BatchNorm2d on batch statistics + LeakyReLU + Conv2d(C, 1, 3, 1, 1)), C in
// {8, 16, 24, 32}; the same conventions as the stem's.  bf, dbf and dy may be null (no bias; no input gradient wanted)
int gennet_tail_channels_ok(int C);
int gennet_tail_tile();
int gennet_tail_max_blocks();
long long gennet_tail_train_workspace_bytes(long long n, int C);
int gennet_tail_train_fwd_launch(const void* y, const float* gamma, const float* beta, const float* wf, const float* bf, void* out, float* stats,
                                 void* workspace, int B, int H, int W, int C, float eps, float slope, int dtype, hipStream_t stream);
int gennet_tail_train_bwd_launch(const void* dout, const void* y, const float* gamma, const float* beta, const float* wf, const float* stats,
                                 void* workspace, void* dy, float* dgamma, float* dbeta, float* dwf, float* dbf, int B, int H, int W, int C,
                                 float slope, int dtype, hipStream_t stream);

// gennet_s2_train.hip: the training kernels of GenNet's 24 -> 24 stride-2 stages — D (big -> small), U (small -> big, gather form) and W
// (the weight gradient and both channel sums) on contiguous NCHW float32 / bfloat16 with the weights as stored; H, W: the big extent,
// the small one ceil(H / 2) x ceil(W / 2); ns = B Hs Ws.  bias, sum_small and sum_big may be null.  -1: C is not 24
int gennet_s2_tile();
int gennet_s2_max_blocks();
long long gennet_s2_wgrad_workspace_bytes(long long ns);
int gennet_s2_down_launch(const void* big, const float* w, const float* bias, void* small, int B, int H, int W, int C, int dtype, hipStream_t stream);
int gennet_s2_up_launch(const void* small, const float* w, const float* bias, void* big, int B, int H, int W, int C, int dtype, hipStream_t stream);
int gennet_s2_wgrad_launch(const void* small, const void* big, void* workspace, float* dw, float* sum_small, float* sum_big, int B, int H, int W,
                           int C, int dtype, hipStream_t stream);

int resize_concat_launch(const void* const* x, const int* hw, const int* ch, int n, void* out, int B, int dtype, hipStream_t stream);
int adaptive_pools_launch(const void* x, void* const* y, const int* scales, int n, int B, int H, int W, int C, int dtype, hipStream_t stream);
int upsample2x_launch(const void* x, const void* bias, const void* add, void* y, int B, int H, int W, int C, int relu, int dtype, hipStream_t stream);
int upsample2x_concat_launch(const void* const* x, const int* ch, int n, void* y, int B, int H, int W, int dtype, hipStream_t stream);
// upsample_bwd.hip: the transposes of the three launches above (x may be null: no folded ReLU)
int upsample2x_bwd_launch(const void* dy, const void* x, void* dx, int B, int H, int W, int C, int dtype, hipStream_t stream);
int upsample2x_concat_bwd_launch(const void* dout, void* const* dx, const int* ch, int n, int B, int H, int W, int dtype, hipStream_t stream);
int resize_concat_bwd_launch(const void* dout, void* const* dx, const int* hw, const int* ch, int n, int B, int dtype, hipStream_t stream);
int conv3x3_c1_launch(const void* x, const float* w, const float* bias, void* y, int B, int H, int W, int Cout, float slope, int dtype,
                      hipStream_t stream);
int conv3x3_to1_launch(const void* x, const float* w, float bias, void* y, int B, int H, int W, int Cin, int dtype, hipStream_t stream);
int seg_labels_launch(const void* lo, uint8_t* labels, int B, int h, int w, int Ho, int Wo, int dtype, hipStream_t stream);
int grid_image_launch(const uint8_t* grid, void* img, long long n, const float* mean, const float* stdv, int dtype, hipStream_t stream);
int bias_act_launch(void* x, const void* bias, long long n, int C, float slope, int dtype, hipStream_t stream);

int conv3x3_mfma_launch(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int Cin, int Cout, int stride,
                        int relu, const float* w2, float* logits, float* partial, hipStream_t stream);
int gennet_enc_conv_launch(const void* x, const void* wk, const float* bias, void* y, int B, int H, int W, float slope, hipStream_t stream);
int gennet_dec_conv_launch(const void* x, const void* wt, const float* bias, void* y, int B, int H, int W, float slope, hipStream_t stream);
int assemble_paths_launch(const double* wp, const int32_t* wp_n, const uint8_t* ok, const double* init, const double* end, double rate, int n, int max_wp,
                          double* full, int32_t* counts, hipStream_t stream);
int plan_collision_launch(const double* full, const int32_t* counts, const void* obstacles, int obs_f64, const int32_t* n_obs, int B, int M, int S,
                          float clearance, float bound, uint8_t* collision, hipStream_t stream);
int mhsa_launch(const void* qkv, void* out, int B, int N, int heads, float scale, int dtype, hipStream_t stream);
long long mhsa_bwd_workspace_floats(int B, int N, int heads);
int mhsa_bwd_launch(const void* qkv, const void* out, const void* dout, void* dqkv, float* workspace, int B, int N, int heads, float scale, int dtype,
                    hipStream_t stream);
// head dim 8 (mhsa_d8.hip): the same layouts and workspace; rows and work-items per workgroup of every one of its kernels
int mhsa_d8_block_rows();
int mhsa_d8_block_threads();
int mhsa_d8_launch(const void* qkv, void* out, int B, int N, int heads, float scale, int dtype, hipStream_t stream);
int mhsa_d8_bwd_launch(const void* qkv, const void* out, const void* dout, void* dqkv, float* workspace, int B, int N, int heads, float scale,
                       int dtype, hipStream_t stream);
int swin_wmsa_launch(const void* qkv, const void* pad_kv, const float* rpb, void* out, int B, int H, int W, int heads, int shift, float scale,
                     int dtype, hipStream_t stream);
// wmsa_gen.hip: the same forward for window 14 with head dim 8 / 16 / 32 and window 7 with head dim 8 / 16 ((7, 32) is forwarded to
// swin_wmsa_launch); work-items per workgroup of its kernels (one workgroup per (image, window, head))
int wmsa_gen_threads(int window);
int wmsa_gen_launch(const void* qkv, const void* pad_kv, const float* rpb, void* out, int B, int H, int W, int heads, int head_dim, int window,
                    int shift, float scale, int dtype, hipStream_t stream);
long long swin_wmsa_bwd_workspace_floats(int heads);
int swin_wmsa_bwd_launch(const void* qkv, const void* pad_kv, const float* rpb, const void* dout, void* dqkv, float* dpad_kv, float* drpb,
                         float* workspace, int B, int H, int W, int heads, int shift, float scale, int dtype, hipStream_t stream);
// resize_ce.hip: bilinear resize + cross-entropy loss of a segmentation head, forward and backward; pixels per forward workgroup,
// work-items per workgroup of every kernel, and the lanes that share one output of the backward (1 / 8 / 64 by the resize ratio: the
// rule of ohem_ce.hip's and resize_dice.hip's backward too).  What this file, seg_eval.hip, ohem_ce.hip and resize_dice.hip share —
// taps, softmax sweep, reductions, the backward's gather, the dtype and lane dispatch — is inline code in resize_tap.h, not declared here
int resize_ce_fwd_pixels();
int resize_ce_threads();
int resize_ce_bwd_lanes(int h, int w, int H, int W);
long long resize_ce_workspace_floats(int B, int H, int W);
int resize_ce_fwd_launch(const void* logit, const void* label, float* lse, float* loss, int64_t* correct, float* workspace, int B, int C, int h,
                         int w, int H, int W, int ignore_index, int logit_dtype, int label_dtype, hipStream_t stream);
int resize_ce_bwd_launch(const void* logit, const void* label, const float* lse, const float* grad_out, void* dlogit, int B, int C, int h, int w,
                         int H, int W, int ignore_index, int logit_dtype, int label_dtype, hipStream_t stream);
// seg_eval.hip: bilinear resize + argmax + the three per-class area histograms of a segmentation evaluation; pixels per tile,
// work-items per workgroup, the largest grid (a workgroup strides over the tiles) and the largest C (pred is uint8, the LDS
// histogram is fixed).  Taps and dtype dispatch: resize_tap.h; the argmax sweep (from -inf) is its own
int seg_eval_pixels();
int seg_eval_threads();
int seg_eval_max_groups();
int seg_eval_max_classes();
int seg_eval_launch(const void* logit, const void* label, uint8_t* pred, int64_t* areas, int B, int C, int h, int w, int H, int W, int ignore_index,
                    int logit_dtype, int label_dtype, hipStream_t stream);
// seg_tta.hip: the merge of a multi-scale + flip test-time augmentation — per augmentation two composed bilinear resizes, softmax and
// un-flip, then the mean and its argmax — in one launch; pixels per tile, work-items per workgroup (one workgroup per tile) and the
// largest C (pred is uint8).  Taps and interp: resize_tap.h.  augs is a host array, passed on as one by-value kernel argument
int seg_tta_pixels();
int seg_tta_threads();
int seg_tta_max_classes();
int seg_tta_launch(const ppn_tta_aug* augs, int n_augs, uint8_t* pred, float* prob, int B, int C, int H, int W, int logit_dtype, hipStream_t stream);
// ohem_ce.hip: resize_ce.hip's loss with online hard example mining (a radix select of the k-th score) and class weights, forward and
// backward; pixels per tile, work-items per workgroup, the largest grid (a workgroup strides over the tiles) and the workspace (bytes,
// the same for every size).  mode 0 = no sampler, 1 = threshold on the label's probability, 2 = the batch_kept largest losses.
// Sweep, reductions and gather: resize_tap.h
int ohem_ce_pixels();
int ohem_ce_threads();
int ohem_ce_max_groups();
long long ohem_ce_workspace_bytes();
int ohem_ce_fwd_launch(const void* logit, const void* label, const float* class_weight, float* lse, float* score, float* loss, int64_t* counts,
                       float* threshold, uint8_t* mask, void* workspace, int B, int C, int h, int w, int H, int W, int ignore_index, int mode,
                       float thresh, uint32_t batch_kept, int logit_dtype, int label_dtype, hipStream_t stream);
int ohem_ce_bwd_launch(const void* logit, const void* label, const float* class_weight, const float* lse, const float* score, const float* threshold,
                       const float* grad_out, void* dlogit, int B, int C, int h, int w, int H, int W, int ignore_index, int mode, int logit_dtype,
                       int label_dtype, hipStream_t stream);
// resize_dice.hip: bilinear resize + Dice loss (mmseg's DiceLoss, exponent 2) of a segmentation head, forward and backward; pixels per
// tile (a tile lies inside one image), work-items per workgroup, the largest C (LDS arrays are fixed) and the workspace in bytes.
// Sweep, final reduction and gather: resize_tap.h
int resize_dice_pixels();
int resize_dice_threads();
int resize_dice_max_classes();
long long resize_dice_workspace_bytes(int B, int C, int H, int W);
int resize_dice_fwd_launch(const void* logit, const void* label, const float* class_weight, void* workspace, float* lse, double* sums, float* loss,
                           int64_t* correct, int B, int C, int h, int w, int H, int W, int ignore_index, float smooth, int logit_dtype,
                           int label_dtype, hipStream_t stream);
int resize_dice_bwd_launch(const void* logit, const void* label, const float* lse, const double* sums, const float* class_weight,
                           const float* grad_out, void* workspace, void* dlogit, int B, int C, int h, int w, int H, int W, int ignore_index,
                           float smooth, int logit_dtype, int label_dtype, hipStream_t stream);
// augment.hip: SegNet's training input (flip + photometric distortion + normalise + pad) from occupancy codes or u8 RGB images;
// work-items per workgroup and output pixels per workgroup (a workgroup serves one image)
int augment_threads();
int augment_pixels();
int augment_params_launch(uint64_t seed, uint64_t first_instance, int B, double flip_ratio, double brightness_delta, double contrast_lo,
                          double contrast_hi, double saturation_lo, double saturation_hi, int hue_delta, uint32_t* params, hipStream_t stream);
int augment_launch(int rgb, const uint8_t* in, const uint8_t* label_in, const uint32_t* params, void* img, uint8_t* label_out, int B, int H, int W,
                   int Ho, int Wo, const float* mean, const float* stdv, int seg_pad_val, int dtype, hipStream_t stream);
int na2d_dense7_launch(const void* qkv, const void* pad_kv, const float* rpb, void* out, int B, int H, int W, int Hr, int Wr, int heads, int dil,
                       float scale, hipStream_t stream);
int gennet_dec_final_launch(const void* x, const void* wt, const float* bias, float slope, const float* w1, float bias1, void* y, int B, int H, int W,
                            hipStream_t stream);
int gennet_first_enc_launch(const void* x1, const void* w1, const float* b1, const void* wk2, const float* bias2, void* y, int B, int H, int W, float slope1,
                            float slope2, hipStream_t stream);
int heatmap_u8_launch(const void* y, uint8_t* out, int B, int n, int dtype, hipStream_t stream);
int tokenizer_fused_launch(const uint8_t* grid, const void* lut, const void* w2p, const float* vec, void* out, int B, int H, int W, float eps,
                           hipStream_t stream);
int tokenizer_codes_launch(const uint8_t* grid, const void* lut, void* out, int B, int H, int W, hipStream_t stream);
int nat128_ln_qkv_launch(const void* s, const float* off, const void* lnw, const void* lnb, const void* w, const void* bias, void* qkv, long long tokens,
                         float eps, hipStream_t stream);
int nat128_ln_mlp_launch(void* s, const float* off, const void* lnw, const void* lnb, const void* w1, const void* b1, const void* w2, const float* add,
                         long long tokens, float eps, hipStream_t stream);
int nat128_proj_add_launch(void* s, const void* a, const void* w, long long tokens, hipStream_t stream);
int gennet_trunk_launch(const void* x, void* y, const float* params, int B, int N, int n_blocks, hipStream_t stream);
bool gemm_small_wanted(long long M, int N, int K);
int gemm_small_launch(const void* a, const void* w, const float* bias, void* c, long long M, int N, int K, int epilogue, hipStream_t stream);
// nat_mlp.hip: the fused MLP of a NAT layer (LN -> fc1 -> GELU -> fc2 -> residual, hidden activation never leaves the CU)
bool nat_mlp_supported(long long M, int C, int HID);
int nat_mlp_pack_launch(const void* w1, const void* w2, void* wpk, int C, int HID, hipStream_t stream);
int nat_mlp_launch(void* s, const void* wpk, const float* hb, const float* b2, float* stats_out, long long M, int C, int HID, float eps, hipStream_t stream);
bool nat_stats_p128(int C);
int row_stats_launch(const void* x, long long rows, int C, float* stats, hipStream_t stream);
int gemm_acc_stats_launch(const void* a, const void* w, const float* bias, float* stats, void* c, long long M, int N, int K, int n_cu,
                          hipStream_t stream);
int gemm_ln_launch(const void* a, const void* w, const float* bias, const float* colsum, const float* stats, int parts, void* c, long long M,
                   int N, int K, int gelu, float eps, int n_cu, hipStream_t stream);
int gemm_mfma_launch(const void* a, const void* w, const float* bias, void* c, long long M, int N, int K, int epi, int persistent,
                     hipStream_t stream);

__global__ void label_masks_kernel(ppn_paths_t paths, ppn_maps_t maps, int placements, int R, int bound, uint8_t* mask_path,
                                   uint8_t* mask_space);

}  // namespace ppn
