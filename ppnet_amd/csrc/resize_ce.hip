// resize_ce.hip — bilinear resize + cross-entropy of a segmentation head's training loss, forward and backward, without the resized
// logits: what SegNet.forward_train composed from F.interpolate(bilinear, align_corners=False) and
// F.cross_entropy(ignore_index, reduction='none').mean() (mmseg decode_head.py:231-265, losses/cross_entropy_loss.py:20-31).
//
//   z_c(Y, X) = a0 (b0 z00 + b1 z01) + a1 (b0 z10 + b1 z11)       the four taps of the low-resolution logit [B][C][h][w]
//   lse(Y, X) = log sum_c exp z_c(Y, X)                           the only per-pixel state: one float32 [B][H][W]
//   loss      = 1 / (B H W) sum_{valid (Y, X)} (lse - z_label)    an ignored pixel adds 0 and still counts in the divisor
//   dlogit[b][c][y][x] = g / (B H W) sum_{valid (Y, X) whose taps touch (y, x)} wy wx (exp(z_c - lse) - [label == c])
//
// One inline function (bilinear_tap, resize_tap.h) gives the taps of a destination index to every kernel of the file — torch's float32 rule for
// align_corners=False with the size given — so the forward and the backward see the same interpolated logit bit for bit (the build
// has -ffp-contract=off: no kernel fuses the products differently).  All arithmetic is float32 — only the sums over many pixels (the
// last stage of the loss, a dlogit element's footprint) are kept in double and rounded once; bfloat16 logits are widened on load
// (exact) and dlogit is rounded once on store, as na2d_bwd.hip and mhsa_d8.hip do.  Labels are uint8 or int64.  A label that is
// ignore_index, or outside [0, C), is IGNORED everywhere and never indexes memory (the one deliberate difference from the library,
// which raises a device-side assert on an out-of-range label).
//
//   forward   a work-item per full-resolution pixel, RCE_FWD_PX pixels per workgroup: two sweeps over the C channels (maximum,
//             argmax with ties to the lowest class and z_label; then the sum of exponentials), no per-channel registers.  The loss
//             terms and the count of argmax == label are summed per workgroup in a fixed tree into the workspace
//             ([2][workgroups]: float32 loss sums | int32 counts); one more workgroup sums those in double / int64 in a fixed order.
//   backward  gather, one writer per dlogit element.  The pixels whose taps touch source row y are a run of consecutive Y (the
//             source index is monotone in Y): a conservative candidate range from the ratio, widened by one (and by the float32
//             error of the source index at very large sizes), is scanned with bilinear_tap itself for the first and the last member,
//             so rounding can neither drop nor double a pixel; where both taps of a pixel fall on y (the high border) their weights
//             add.  RCE_LANES lanes share an output (1, 8 or 64 by the footprint, about (2 H/h)(2 W/w) pixels), lanes across the
//             footprint, and are summed by a fixed xor tree.  No atomics: every result is bitwise reproducible.
//
// No kernel holds a runtime-C array: every one loops over the channels (ScratchSize 0).  Element offsets are 64-bit; the caller
// (capi.hip) rejects B C h w, B H W and launches of 2^31 or more.
//
// What ohem_ce.hip and resize_dice.hip do the same way lives in resize_tap.h, once: the taps (Tap, bilinear_tap, ldf, stf, interp,
// valid_label), the forward's softmax_sweep, group_sum and final_sum, the backward's tap_range, tap_weight and Gather, and the host's
// dispatch_types and dispatch_lanes.  This file keeps its kernels, its constants and what is the cross-entropy's own: the loss term,
// the gather's per-pixel term and its store.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include "ppn_device.h"
#include "ppn_kernels.h"
#include "resize_tap.h"

namespace ppn {

namespace {
constexpr int RCE_THREADS = 256;                       // work-items per workgroup, every kernel
constexpr int RCE_FWD_PER_THREAD = 4;
constexpr int RCE_FWD_PX = RCE_THREADS * RCE_FWD_PER_THREAD;   // pixels per forward workgroup

template <typename T, typename LT>
__global__ __launch_bounds__(RCE_THREADS) void resize_ce_fwd_kernel(const T* __restrict__ logit, const LT* __restrict__ label,
                                                                     float* __restrict__ lse, float* __restrict__ ws, int n_groups,
                                                                     int n_px, int C, int h, int w, int H, int W, int ignore_index) {
    __shared__ float s_loss[RCE_THREADS / 64];
    __shared__ int s_cnt[RCE_THREADS / 64];
    const int tid = threadIdx.x;
    const size_t plane = (size_t)h * w;
    float loss = 0.f;
    int cnt = 0;
    for (int k = 0; k < RCE_FWD_PER_THREAD; ++k) {
        const long long pl = (long long)blockIdx.x * RCE_FWD_PX + k * RCE_THREADS + tid;
        if (pl >= n_px) break;
        const int p = (int)pl;
        const int b = p / (H * W), r = p - b * (H * W), Y = r / W, X = r - Y * W;
        const Tap ty = bilinear_tap(Y, h, H), tx = bilinear_tap(X, w, W);
        const int r0 = ty.i0 * w, r1 = ty.i1 * w;
        const T* img = logit + (size_t)b * C * plane;
        const int lab = valid_label(label, (size_t)p, C, ignore_index);
        const Sweep sw = softmax_sweep(img, plane, C, r0, r1, ty, tx, lab);
        const float l = sw.m + logf(sw.s);
        if (lse) lse[p] = l;
        if (lab >= 0) {
            loss += l - sw.zl;
            cnt += (sw.arg == lab);
        }
    }
    const FloatInt sum = group_sum<RCE_THREADS>(loss, cnt, s_loss, s_cnt);   // a fixed tree
    if (tid == 0) {
        ws[blockIdx.x] = sum.a;
        reinterpret_cast<int*>(ws)[(size_t)n_groups + blockIdx.x] = sum.n;
    }
}

// one workgroup: the partial sums in double / int64, each work-item a strided share in order, then a fixed tree through LDS
__global__ __launch_bounds__(RCE_THREADS) void resize_ce_final_kernel(const float* __restrict__ ws, int n_groups, double n_px,
                                                                       float* __restrict__ loss, long long* __restrict__ correct) {
    __shared__ double s_a[RCE_THREADS];
    __shared__ long long s_n[RCE_THREADS];
    const int tid = threadIdx.x;
    const int* cnt = reinterpret_cast<const int*>(ws) + n_groups;
    double a = 0.0;
    long long n = 0;
    for (int i = tid; i < n_groups; i += RCE_THREADS) { a += (double)ws[i]; n += cnt[i]; }
    final_sum<RCE_THREADS>(a, n, s_a, s_n);
    if (tid == 0) { *loss = (float)(a / n_px); *correct = n; }
}

template <typename T, typename LT, int LANES>
__global__ __launch_bounds__(RCE_THREADS) void resize_ce_bwd_kernel(const T* __restrict__ logit, const LT* __restrict__ label,
                                                                     const float* __restrict__ lse, const float* __restrict__ grad_out,
                                                                     T* __restrict__ dlogit, long long n_out, int C, int h, int w, int H,
                                                                     int W, int ignore_index, float inv_px) {
    const Gather<RCE_THREADS, LANES> out(n_out, C, h, w);
    const T* plane = logit + (size_t)out.bc * h * w;
    const double acc = out.sum(true, h, w, H, W, [&](double& sum, size_t p, int Y, int X) {
        const int lab = valid_label(label, p, C, ignore_index);
        if (lab < 0) return;
        const Tap ty = bilinear_tap(Y, h, H), tx = bilinear_tap(X, w, W);
        const float z = interp(plane, ty.i0 * w, ty.i1 * w, ty, tx);
        const float g = expf(z - lse[p]) - (lab == out.c ? 1.f : 0.f);
        sum += (double)(tap_weight(ty, out.y) * tap_weight(tx, out.x) * g);   // a float32 product, rounded once, then widened
    });
    if (out.live && out.lane() == 0) stf(dlogit + out.o, (float)acc * (*grad_out * inv_px));
}

template <typename T, typename LT>
int fwd_typed(const void* logit, const void* label, float* lse, float* loss, int64_t* correct, float* ws, int B, int C, int h, int w, int H,
              int W, int ignore_index, hipStream_t stream) {
    const long long n_px = (long long)B * H * W;
    const int groups = (int)((n_px + RCE_FWD_PX - 1) / RCE_FWD_PX);
    hipLaunchKernelGGL((resize_ce_fwd_kernel<T, LT>), dim3((unsigned)groups), dim3(RCE_THREADS), 0, stream, (const T*)logit, (const LT*)label, lse,
                       ws, groups, (int)n_px, C, h, w, H, W, ignore_index);
    hipLaunchKernelGGL(resize_ce_final_kernel, dim3(1), dim3(RCE_THREADS), 0, stream, (const float*)ws, groups, (double)n_px, loss,
                       (long long*)correct);
    return (int)hipGetLastError();
}

template <typename T, typename LT>
int bwd_typed(const void* logit, const void* label, const float* lse, const float* grad_out, void* dlogit, int B, int C, int h, int w, int H, int W,
              int ignore_index, hipStream_t stream) {
    const long long n_out = (long long)B * C * h * w;
    dispatch_lanes(RCE_THREADS, n_out, h, w, H, W, [&](auto lanes, dim3 grid) {
        hipLaunchKernelGGL((resize_ce_bwd_kernel<T, LT, decltype(lanes)::value>), grid, dim3(RCE_THREADS), 0, stream, (const T*)logit,
                           (const LT*)label, lse, grad_out, (T*)dlogit, n_out, C, h, w, H, W, ignore_index, 1.0f / (float)((long long)B * H * W));
    });
    return (int)hipGetLastError();
}
}  // namespace

int resize_ce_fwd_pixels() { return RCE_FWD_PX; }
int resize_ce_threads() { return RCE_THREADS; }

// lanes that share one dlogit element: by the footprint (2 H/h)(2 W/w) of an output, the pixels whose taps touch it
int resize_ce_bwd_lanes(int h, int w, int H, int W) {
    const double fy = 2.0 * (H > h ? (double)H / h : 1.0), fx = 2.0 * (W > w ? (double)W / w : 1.0);
    const double f = fy * fx;
    return f <= 16.0 ? 1 : (f <= 128.0 ? 8 : 64);
}

// workspace [2][groups]: loss sums (float32) | counts (int32), groups = ceil(B H W / RCE_FWD_PX)
long long resize_ce_workspace_floats(int B, int H, int W) {
    return 2 * (((long long)B * H * W + RCE_FWD_PX - 1) / RCE_FWD_PX);
}

// extents >= 1, B C h w and B H W and the launches below 2^31, aligned non-null buffers: checked by the caller (capi.hip)
int resize_ce_fwd_launch(const void* logit, const void* label, float* lse, float* loss, int64_t* correct, float* ws, int B, int C, int h, int w,
                         int H, int W, int ignore_index, int logit_dtype, int label_dtype, hipStream_t stream) {
    return dispatch_types(logit_dtype, label_dtype, [&](auto t, auto lt) {
        return fwd_typed<decltype(t), decltype(lt)>(logit, label, lse, loss, correct, ws, B, C, h, w, H, W, ignore_index, stream);
    });
}

int resize_ce_bwd_launch(const void* logit, const void* label, const float* lse, const float* grad_out, void* dlogit, int B, int C, int h, int w,
                         int H, int W, int ignore_index, int logit_dtype, int label_dtype, hipStream_t stream) {
    return dispatch_types(logit_dtype, label_dtype, [&](auto t, auto lt) {
        return bwd_typed<decltype(t), decltype(lt)>(logit, label, lse, grad_out, dlogit, B, C, h, w, H, W, ignore_index, stream);
    });
}

}  // namespace ppn
