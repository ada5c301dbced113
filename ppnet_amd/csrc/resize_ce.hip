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

// Tap, bilinear_tap, ldf, interp and valid_label: resize_tap.h (shared with seg_eval.hip, whose argmax is this file's)

template <typename T>
__device__ __forceinline__ void stf(T* p, float v) {
    if constexpr (sizeof(T) == 4) *p = v;
    else *p = (__bf16)v;                                                                       // rounded to nearest even, once
}

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
        float m = interp(img, r0, r1, ty, tx), zl = m;
        int arg = 0;
        for (int c = 1; c < C; ++c) {
            const float z = interp(img + c * plane, r0, r1, ty, tx);
            if (z > m) { m = z; arg = c; }                         // ties keep the lowest class
            if (c == lab) zl = z;
        }
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += expf(interp(img + c * plane, r0, r1, ty, tx) - m);
        const float l = m + logf(s);
        if (lse) lse[p] = l;
        if (lab >= 0) {
            loss += l - zl;
            cnt += (arg == lab);
        }
    }
    // fixed tree: xor shuffles within the wave, then the four waves in order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        loss += __shfl_xor(loss, o, 64);
        cnt += __shfl_xor(cnt, o, 64);
    }
    if ((tid & 63) == 0) { s_loss[tid >> 6] = loss; s_cnt[tid >> 6] = cnt; }
    __syncthreads();
    if (tid == 0) {
        float a = s_loss[0];
        int n = s_cnt[0];
#pragma unroll
        for (int i = 1; i < RCE_THREADS / 64; ++i) { a += s_loss[i]; n += s_cnt[i]; }
        ws[blockIdx.x] = a;
        reinterpret_cast<int*>(ws)[(size_t)n_groups + blockIdx.x] = n;
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
    s_a[tid] = a;
    s_n[tid] = n;
    __syncthreads();
    for (int o = RCE_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) { s_a[tid] += s_a[tid + o]; s_n[tid] += s_n[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) { *loss = (float)(s_a[0] / n_px); *correct = s_n[0]; }
}

// first / last destination index in [0, n_out) whose taps touch source index y (first > last: none).  The exact range is
// ((y - 1 + 0.5) n_out / n_in - 0.5, (y + 1 + 0.5) n_out / n_in - 0.5); the scan decides membership with bilinear_tap itself.
__device__ __forceinline__ void tap_range(int y, int n_in, int n_out, int& first, int& last) {
    const double r = (double)n_out / (double)n_in;
    const double lo = floor(((double)y - 0.5) * r - 0.5), hi = ceil(((double)y + 1.5) * r - 0.5);
    const double margin = 1.0 + floor(hi * 1.0e-6);        // one, plus the float32 error of the source index (< 2.4e-7 of it)
    const int c0 = (int)fmax(lo - margin, 0.0), c1 = (int)fmin(hi + margin, (double)(n_out - 1));
    first = c1 + 1;
    last = c0 - 1;
    for (int Y = c0; Y <= c1; ++Y) {
        const Tap t = bilinear_tap(Y, n_in, n_out);
        if (t.i0 == y || t.i1 == y) {
            if (first > c1) first = Y;
            last = Y;
        }
    }
}

__device__ __forceinline__ float tap_weight(const Tap& t, int y) { return (t.i0 == y ? t.l0 : 0.f) + (t.i1 == y ? t.l1 : 0.f); }

template <typename T, typename LT, int LANES>
__global__ __launch_bounds__(RCE_THREADS) void resize_ce_bwd_kernel(const T* __restrict__ logit, const LT* __restrict__ label,
                                                                     const float* __restrict__ lse, const float* __restrict__ grad_out,
                                                                     T* __restrict__ dlogit, long long n_out, int C, int h, int w, int H,
                                                                     int W, int ignore_index, float inv_px) {
    constexpr int OUTS = RCE_THREADS / LANES;              // outputs per workgroup
    const int lane = threadIdx.x % LANES;
    const long long o = (long long)blockIdx.x * OUTS + threadIdx.x / LANES;
    const bool live = o < n_out;                           // the lanes of an output agree; no early return before the shuffles
    double acc = 0.0;                                      // a footprint of ~1000 signed terms that cancel: summed in double, rounded once
    if (live) {
        const int x = (int)(o % w), y = (int)((o / w) % h);
        const int bc = (int)(o / ((long long)w * h)), b = bc / C, c = bc - b * C;
        int Y0, Y1, X0, X1;
        tap_range(y, h, H, Y0, Y1);
        tap_range(x, w, W, X0, X1);
        const int ny = Y1 - Y0 + 1, nx = X1 - X0 + 1;
        if (ny > 0 && nx > 0) {
            const T* plane = logit + (size_t)bc * h * w;
            const size_t px0 = (size_t)b * H * W;
            const int n = ny * nx;                         // < 2^31: a subset of one image's H W pixels
            for (int i = lane; i < n; i += LANES) {
                const int dy = i / nx, Y = Y0 + dy, X = X0 + (i - dy * nx);
                const size_t p = px0 + (size_t)Y * W + X;
                const int lab = valid_label(label, p, C, ignore_index);
                if (lab < 0) continue;
                const Tap ty = bilinear_tap(Y, h, H), tx = bilinear_tap(X, w, W);
                const float z = interp(plane, ty.i0 * w, ty.i1 * w, ty, tx);
                const float g = expf(z - lse[p]) - (lab == c ? 1.f : 0.f);
                acc += (double)(tap_weight(ty, y) * tap_weight(tx, x) * g);
            }
        }
    }
#pragma unroll
    for (int s = LANES / 2; s > 0; s >>= 1) acc += __shfl_xor(acc, s, LANES);
    if (live && lane == 0) stf(dlogit + o, (float)acc * (*grad_out * inv_px));
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

template <typename T, typename LT, int LANES>
void bwd_lanes(const void* logit, const void* label, const float* lse, const float* grad_out, void* dlogit, int B, int C, int h, int w, int H,
               int W, int ignore_index, hipStream_t stream) {
    const long long n_out = (long long)B * C * h * w, outs = RCE_THREADS / LANES;
    hipLaunchKernelGGL((resize_ce_bwd_kernel<T, LT, LANES>), dim3((unsigned)((n_out + outs - 1) / outs)), dim3(RCE_THREADS), 0, stream,
                       (const T*)logit, (const LT*)label, lse, grad_out, (T*)dlogit, n_out, C, h, w, H, W, ignore_index,
                       1.0f / (float)((long long)B * H * W));
}

template <typename T, typename LT>
int bwd_typed(const void* logit, const void* label, const float* lse, const float* grad_out, void* dlogit, int B, int C, int h, int w, int H, int W,
              int ignore_index, hipStream_t stream) {
    const int lanes = resize_ce_bwd_lanes(h, w, H, W);
    if (lanes == 1) bwd_lanes<T, LT, 1>(logit, label, lse, grad_out, dlogit, B, C, h, w, H, W, ignore_index, stream);
    else if (lanes == 8) bwd_lanes<T, LT, 8>(logit, label, lse, grad_out, dlogit, B, C, h, w, H, W, ignore_index, stream);
    else bwd_lanes<T, LT, 64>(logit, label, lse, grad_out, dlogit, B, C, h, w, H, W, ignore_index, stream);
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
    if (logit_dtype == 0)
        return label_dtype == 0 ? fwd_typed<float, uint8_t>(logit, label, lse, loss, correct, ws, B, C, h, w, H, W, ignore_index, stream)
                                : fwd_typed<float, int64_t>(logit, label, lse, loss, correct, ws, B, C, h, w, H, W, ignore_index, stream);
    return label_dtype == 0 ? fwd_typed<__bf16, uint8_t>(logit, label, lse, loss, correct, ws, B, C, h, w, H, W, ignore_index, stream)
                            : fwd_typed<__bf16, int64_t>(logit, label, lse, loss, correct, ws, B, C, h, w, H, W, ignore_index, stream);
}

int resize_ce_bwd_launch(const void* logit, const void* label, const float* lse, const float* grad_out, void* dlogit, int B, int C, int h, int w,
                         int H, int W, int ignore_index, int logit_dtype, int label_dtype, hipStream_t stream) {
    if (logit_dtype == 0)
        return label_dtype == 0 ? bwd_typed<float, uint8_t>(logit, label, lse, grad_out, dlogit, B, C, h, w, H, W, ignore_index, stream)
                                : bwd_typed<float, int64_t>(logit, label, lse, grad_out, dlogit, B, C, h, w, H, W, ignore_index, stream);
    return label_dtype == 0 ? bwd_typed<__bf16, uint8_t>(logit, label, lse, grad_out, dlogit, B, C, h, w, H, W, ignore_index, stream)
                            : bwd_typed<__bf16, int64_t>(logit, label, lse, grad_out, dlogit, B, C, h, w, H, W, ignore_index, stream);
}

}  // namespace ppn
