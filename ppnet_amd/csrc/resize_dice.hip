// resize_dice.hip — bilinear resize + Dice loss of a segmentation head, forward and backward, without the resized logits, their
// softmax or a one-hot tensor: what mmseg composes from resize + DiceLoss (models/losses/dice_loss.py: F.softmax, F.one_hot of the
// clamped labels, a valid mask, per class binary_dice_loss with exponent 2 under @weighted_loss, i.e. the mean over the batch).
//
//   z_i(Y, X) = the four taps of logit [B][C][h][w] (resize_tap.h: resize_ce.hip's own interpolated logit, bit for bit)
//   lse = log sum_i exp z_i,   p_i = exp(z_i - lse)                the only per-pixel state kept for the backward: lse, one float32
//   v  = label is valid (not ignore_index and inside [0, C): this build's rule),   tc = the label clamped into [0, C - 1]
//   I[b][i]  = sum_px p_i [tc == i] v        P2[b][i] = sum_px p_i^2        T[b][i] = #{px: tc == i}   (NOT masked: the reference's
//              denominator counts an ignored label as the class its clamp lands on — 255 as class C - 1)
//   N = 2 I + smooth,   Den = P2 + T + smooth
//   loss = 1 / (C B) sum_b sum_{i != ignore_index} cw_i (1 - N / Den)                  (loss_weight stays with the caller)
//   dloss/dz_k(px) = p_k (g_k - s),   g_i = a[b][i] [tc == i] v + b[b][i] p_i,   s = sum_i g_i p_i,
//              a = -2 k_i / Den,   b = 2 k_i N / Den^2,   k_i = grad_out cw_i / (C B), 0 for i == ignore_index
//   dlogit[b][c][y][x] = sum_{(Y, X) whose taps touch (y, x)} wy wx p_c (g_c - s)      (EVERY pixel: an ignored one still has p)
//
//   kernels   dice_fwd      a workgroup per tile of DICE_PX pixels of ONE image (tiles never straddle images), four pixels per
//                           work-item: maximum + argmax (ties to the lowest class), sum of exponentials, lse; then a sweep with the
//                           class OUTSIDE and the four pixels inside, so that a class's three sums are reduced over the workgroup in
//                           a fixed tree (xor shuffles, then the four waves in order through LDS) and written as one partial
//                           [tile][C][3] (float32 I | float32 P2 | int32 T) + the tile's count of argmax == label
//             dice_sums     a workgroup per image: the tiles' partials in tile order in double (T: int64) -> sums [B][C][3] float64
//             dice_loss     one workgroup: the B C terms in double, a strided share in order and a fixed tree; loss, correct
//             dice_bwd_px   per pixel s(px) -> workspace (one float32 per pixel); a[b][.] and b[b][.] are derived in LDS from sums,
//                           smooth, the class weights and the device scalar grad_out by every workgroup, and the first tile of an
//                           image records them ([B][C][2] float64 in front of the per-pixel buffer) for the gather
//             dice_bwd      resize_ce_bwd_kernel's gather (resize_tap.h's Gather: one writer per dlogit element, resize_ce_bwd_lanes
//                           lanes per element, a fixed xor tree, no atomics).  Its own: the term (double)(wy wx) (p_c (g_c - s)), the
//                           product with g in double, of EVERY pixel (the clamped label skips none), and a store without a scale
//             a, b, g and s are combined in DOUBLE from the float32 p: where a pixel is confidently right N / Den is close to 1, a and
//             b p nearly cancel (g and s are ~20 x smaller than a) and g - s is smaller again — in float32 that chain lost 5e-6 of a
//             one-pixel image's gradient.  s itself is small, so its one rounding to float32 for the workspace costs 6e-8 of |s|.
//             s is taken as the p-weighted MEAN sum_i g_i p_i / sum_i p_i: exp(z_i - lse) sums to 1 only within the rounding of the
//             float32 lse (half an ulp of |lse|: 1e-7 at |lse| = 2, 4e-6 at 80), and g_k - s has to vanish as p_k -> 1 whatever that
//             rounding was — with the plain sum the residue a p_t delta stayed, up to 3e-6 of a small image's gradient.
//             The FORWARD takes p_i = exp(z_i - lse) from lse's two parts before they are added, exp(z_i - max) / sum exp(z - max):
//             rounded to one float32, lse scales every p of a pixel by 1 + delta (delta up to 4e-6 at |lse| = 80), I and P2 inherit
//             it, and the cancellation above multiplies it in a and b — 2.9e-6 of the gradient at +-80 logits on the device, 1.3e-6
//             in a float32 emulation once the sums are taken from the normalised p.
//             C = 1: the softmax is the constant 1 and the gradient identically 0; the gather writes 0 without the sum.
//             Three launches forward, two backward; no atomics at all and every sum has a fixed order: sums, loss, correct and
//             dlogit are bitwise reproducible.  Nothing is read back to the host.
//
// Per-pixel arithmetic is float32 up to p (bfloat16 logits are widened on load, dlogit is rounded once on store); sums over many pixels and the backward's combination of a, b, p end in
// double.  No kernel holds a runtime-C array: every one loops over the channels (ScratchSize 0).  Element offsets are 64-bit; the
// caller (capi.hip) rejects C > DICE_MAX_C, B C h w, B H W and launches of 2^31 or more.  A label never indexes memory.
//
// What this file does as resize_ce.hip does is not copied but included (resize_tap.h): the taps, dice_fwd's softmax_sweep (it takes
// the maximum and 1 / sum before lse is rounded, and wants no z_label), dice_loss's final_sum, dice_bwd's Gather with tap_range and
// tap_weight, stf, and the host's dispatch_types and dispatch_lanes.  dice_fwd's per-class triple reduction is its own and stays here.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include "ppn_device.h"
#include "ppn_kernels.h"
#include "resize_tap.h"

namespace ppn {

namespace {
constexpr int DICE_THREADS = 256;                      // work-items per workgroup, every kernel
constexpr int DICE_PER_THREAD = 4;
constexpr int DICE_PX = DICE_THREADS * DICE_PER_THREAD;   // pixels per tile (of one image)
constexpr int DICE_MAX_C = 256;                        // the LDS partials and coefficients are fixed arrays
constexpr int DICE_WAVES = DICE_THREADS / 64;

// the label clamped into [0, C - 1] (what the reference one-hot encodes), and whether it is valid (this build's rule)
template <typename LT>
__device__ __forceinline__ int clamped_label(const LT* label, size_t p, int C, int ignore_index, bool& valid) {
    const long long v = (long long)label[p];
    valid = !(v == (long long)ignore_index || v < 0 || v >= (long long)C);
    return v < 0 ? 0 : (v >= (long long)C ? C - 1 : (int)v);
}

template <typename T, typename LT>
__global__ __launch_bounds__(DICE_THREADS) void dice_fwd_kernel(const T* __restrict__ logit, const LT* __restrict__ label,
                                                                 float* __restrict__ lse, uint32_t* __restrict__ ws, int tiles_per_image,
                                                                 long long n_tiles, int C, int h, int w, int H, int W, int ignore_index) {
    __shared__ uint32_t s_part[DICE_MAX_C * 3 * DICE_WAVES];
    __shared__ int s_cnt[DICE_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / tiles_per_image, tile = blockIdx.x - b * tiles_per_image;
    const int HW = H * W;
    const size_t plane = (size_t)h * w;
    const T* img = logit + (size_t)b * C * plane;
    const size_t px0 = (size_t)b * HW;
    Tap ty[DICE_PER_THREAD], tx[DICE_PER_THREAD];
    float mx[DICE_PER_THREAD], inv[DICE_PER_THREAD];       // the maximum and 1 / sum exp(z - max): lse before its rounding to one float
    int tc[DICE_PER_THREAD];                               // -1: no pixel (past the image's end)
    bool ok[DICE_PER_THREAD];
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < DICE_PER_THREAD; ++k) {
        const int r = tile * DICE_PX + k * DICE_THREADS + tid;
        tc[k] = -1;
        ok[k] = false;
        mx[k] = 0.f;
        inv[k] = 0.f;
        ty[k] = tx[k] = Tap{0, 0, 0.f, 0.f};
        if (r < HW) {
            const int Y = r / W, X = r - Y * W;
            ty[k] = bilinear_tap(Y, h, H);
            tx[k] = bilinear_tap(X, w, W);
            const int r0 = ty[k].i0 * w, r1 = ty[k].i1 * w;
            const Sweep sw = softmax_sweep(img, plane, C, r0, r1, ty[k], tx[k], -1);   // no z_label wanted
            mx[k] = sw.m;
            inv[k] = 1.f / sw.s;
            if (lse) lse[px0 + r] = sw.m + logf(sw.s);
            tc[k] = clamped_label(label, px0 + r, C, ignore_index, ok[k]);
            cnt += (ok[k] && sw.arg == tc[k]);
        }
    }
    // the class outside, the pixels inside: a class's three sums over the workgroup, a fixed tree
    for (int c = 0; c < C; ++c) {
        float vi = 0.f, vp = 0.f;
        int vt = 0;
#pragma unroll
        for (int k = 0; k < DICE_PER_THREAD; ++k) {
            if (tc[k] >= 0) {
                const float p = expf(interp(img + c * plane, ty[k].i0 * w, ty[k].i1 * w, ty[k], tx[k]) - mx[k]) * inv[k];
                vp += p * p;
                if (tc[k] == c) {
                    vt += 1;
                    if (ok[k]) vi += p;
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            vi += __shfl_xor(vi, o, 64);
            vp += __shfl_xor(vp, o, 64);
            vt += __shfl_xor(vt, o, 64);
        }
        if (lane == 0) {
            s_part[(c * 3 + 0) * DICE_WAVES + wave] = __float_as_uint(vi);
            s_part[(c * 3 + 1) * DICE_WAVES + wave] = __float_as_uint(vp);
            s_part[(c * 3 + 2) * DICE_WAVES + wave] = (uint32_t)vt;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    uint32_t* out = ws + (size_t)blockIdx.x * (3 * C);
    for (int i = tid; i < 3 * C; i += DICE_THREADS) {       // the four waves in order
        const uint32_t* q = s_part + i * DICE_WAVES;
        if (i % 3 == 2) {
            uint32_t n = q[0];
#pragma unroll
            for (int j = 1; j < DICE_WAVES; ++j) n += q[j];
            out[i] = n;
        } else {
            float a = __uint_as_float(q[0]);
#pragma unroll
            for (int j = 1; j < DICE_WAVES; ++j) a += __uint_as_float(q[j]);
            out[i] = __float_as_uint(a);
        }
    }
    if (tid == 0) {
        int n = s_cnt[0];
#pragma unroll
        for (int j = 1; j < DICE_WAVES; ++j) n += s_cnt[j];
        ws[(size_t)n_tiles * (3 * C) + blockIdx.x] = (uint32_t)n;
    }
}

// a workgroup per image: every (class, sum) over the image's tiles in tile order, in double (the counts in int64, exact)
__global__ __launch_bounds__(DICE_THREADS) void dice_sums_kernel(const uint32_t* __restrict__ ws, int tiles_per_image, int C,
                                                                  double* __restrict__ sums) {
    const int b = blockIdx.x;
    const uint32_t* part = ws + (size_t)b * tiles_per_image * (3 * C);
    for (int i = threadIdx.x; i < 3 * C; i += DICE_THREADS) {
        double a = 0.0;
        long long n = 0;
        if (i % 3 == 2) {
            for (int t = 0; t < tiles_per_image; ++t) n += (long long)part[(size_t)t * (3 * C) + i];
            a = (double)n;
        } else {
            for (int t = 0; t < tiles_per_image; ++t) a += (double)__uint_as_float(part[(size_t)t * (3 * C) + i]);
        }
        sums[(size_t)b * (3 * C) + i] = a;
    }
}

// one workgroup: the B C terms cw_i (1 - N / Den) and the tiles' counts, each work-item a strided share in order, then a fixed tree
__global__ __launch_bounds__(DICE_THREADS) void dice_loss_kernel(const double* __restrict__ sums, const uint32_t* __restrict__ cnt,
                                                                  const float* __restrict__ cw, long long n_tiles, int B, int C,
                                                                  int ignore_index, double smooth, float* __restrict__ loss,
                                                                  long long* __restrict__ correct) {
    __shared__ double s_a[DICE_THREADS];
    __shared__ long long s_n[DICE_THREADS];
    const int tid = threadIdx.x;
    double a = 0.0;
    long long n = 0;
    const long long terms = (long long)B * C;
    for (long long i = tid; i < terms; i += DICE_THREADS) {
        const int c = (int)(i % C);
        if (c == ignore_index) continue;
        const double* q = sums + i * 3;
        const double t = 1.0 - (2.0 * q[0] + smooth) / (q[1] + q[2] + smooth);
        a += cw ? (double)cw[c] * t : t;
    }
    for (long long i = tid; i < n_tiles; i += DICE_THREADS) n += (long long)cnt[i];
    final_sum<DICE_THREADS>(a, n, s_a, s_n);
    if (tid == 0) { *loss = (float)(a / ((double)C * (double)B)); *correct = n; }
}

// first pass of the backward: s(px) = (a[b][tc] v p_tc + sum_i b[b][i] p_i^2) / sum_i p_i, one float32 per pixel; the coefficients in LDS
template <typename T, typename LT>
__global__ __launch_bounds__(DICE_THREADS) void dice_bwd_px_kernel(const T* __restrict__ logit, const LT* __restrict__ label,
                                                                    const float* __restrict__ lse, const double* __restrict__ sums,
                                                                    const float* __restrict__ cw, const float* __restrict__ grad_out,
                                                                    float* __restrict__ spx, double* __restrict__ coef, int tiles_per_image,
                                                                    int B, int C, int h, int w, int H, int W, int ignore_index, double smooth) {
    __shared__ double s_a[DICE_MAX_C], s_b[DICE_MAX_C];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / tiles_per_image, tile = blockIdx.x - b * tiles_per_image;
    const double go = (double)*grad_out;
    for (int c = tid; c < C; c += DICE_THREADS) {
        const double* q = sums + ((size_t)b * C + c) * 3;
        const double k = c == ignore_index ? 0.0 : go * (cw ? (double)cw[c] : 1.0) / ((double)C * (double)B);
        const double N = 2.0 * q[0] + smooth, Den = q[1] + q[2] + smooth;
        const double a = -2.0 * k / Den, bb = 2.0 * k * N / (Den * Den);
        s_a[c] = a;
        s_b[c] = bb;
        if (tile == 0) {
            coef[((size_t)b * C + c) * 2] = a;
            coef[((size_t)b * C + c) * 2 + 1] = bb;
        }
    }
    __syncthreads();
    const int HW = H * W;
    const size_t plane = (size_t)h * w;
    const T* img = logit + (size_t)b * C * plane;
    const size_t px0 = (size_t)b * HW;
    for (int k = 0; k < DICE_PER_THREAD; ++k) {
        const int r = tile * DICE_PX + k * DICE_THREADS + tid;
        if (r >= HW) break;
        const int Y = r / W, X = r - Y * W;
        const Tap ty = bilinear_tap(Y, h, H), tx = bilinear_tap(X, w, W);
        const int r0 = ty.i0 * w, r1 = ty.i1 * w;
        bool ok;
        const int tc = clamped_label(label, px0 + r, C, ignore_index, ok);
        const float l = lse[px0 + r];
        double sb = 0.0, pt = 0.0, sp = 0.0;
        for (int c = 0; c < C; ++c) {
            const double p = (double)expf(interp(img + c * plane, r0, r1, ty, tx) - l);
            sb += s_b[c] * (p * p);
            sp += p;
            if (c == tc) pt = p;
        }
        // the p-WEIGHTED MEAN of g: sp is 1 only within the rounding of lse.  tc is inside [0, C): an LDS index, never a global one
        spx[px0 + r] = (float)(((ok ? s_a[tc] * pt : 0.0) + sb) / sp);
    }
}

template <typename T, typename LT, int LANES>
__global__ __launch_bounds__(DICE_THREADS) void dice_bwd_kernel(const T* __restrict__ logit, const LT* __restrict__ label,
                                                                 const float* __restrict__ lse, const float* __restrict__ spx,
                                                                 const double* __restrict__ coef, T* __restrict__ dlogit, long long n_out, int C,
                                                                 int h, int w, int H, int W, int ignore_index) {
    const Gather<DICE_THREADS, LANES> out(n_out, C, h, w);
    const T* plane = logit + (size_t)out.bc * h * w;
    const double ca = out.live ? coef[(size_t)out.bc * 2] : 0.0, cb = out.live ? coef[(size_t)out.bc * 2 + 1] : 0.0;
    // C = 1: p is the constant 1, the gradient identically 0.  No pixel is skipped: an ignored one still has p
    const double acc = out.sum(C > 1, h, w, H, W, [&](double& sum, size_t p, int Y, int X) {
        bool ok;
        const int tc = clamped_label(label, p, C, ignore_index, ok);
        const Tap ty = bilinear_tap(Y, h, H), tx = bilinear_tap(X, w, W);
        const double pc = (double)expf(interp(plane, ty.i0 * w, ty.i1 * w, ty, tx) - lse[p]);
        const double g = ((ok && tc == out.c) ? ca : 0.0) + cb * pc;
        sum += (double)(tap_weight(ty, out.y) * tap_weight(tx, out.x)) * (pc * (g - (double)spx[p]));   // the product with g in double
    });
    if (out.live && out.lane() == 0) stf(dlogit + out.o, (float)acc);
}

__host__ inline int tiles_of(int H, int W) { return (int)(((long long)H * W + DICE_PX - 1) / DICE_PX); }

template <typename T, typename LT>
int fwd_typed(const void* logit, const void* label, const float* cw, uint32_t* ws, float* lse, double* sums, float* loss, int64_t* correct, int B,
              int C, int h, int w, int H, int W, int ignore_index, float smooth, hipStream_t stream) {
    const int tpi = tiles_of(H, W);
    const long long tiles = (long long)B * tpi;
    hipLaunchKernelGGL((dice_fwd_kernel<T, LT>), dim3((unsigned)tiles), dim3(DICE_THREADS), 0, stream, (const T*)logit, (const LT*)label, lse, ws,
                       tpi, tiles, C, h, w, H, W, ignore_index);
    hipLaunchKernelGGL(dice_sums_kernel, dim3((unsigned)B), dim3(DICE_THREADS), 0, stream, (const uint32_t*)ws, tpi, C, sums);
    hipLaunchKernelGGL(dice_loss_kernel, dim3(1), dim3(DICE_THREADS), 0, stream, (const double*)sums, (const uint32_t*)(ws + (size_t)tiles * (3 * C)),
                       cw, tiles, B, C, ignore_index, (double)smooth, loss, (long long*)correct);
    return (int)hipGetLastError();
}

template <typename T, typename LT>
int bwd_typed(const void* logit, const void* label, const float* lse, const double* sums, const float* cw, const float* grad_out, float* ws,
              void* dlogit, int B, int C, int h, int w, int H, int W, int ignore_index, float smooth, hipStream_t stream) {
    const int tpi = tiles_of(H, W);
    double* coef = (double*)ws;                            // [B][C][2] float64 first (the workspace is 16-byte aligned), then a float32 per pixel
    float* spx = ws + 4 * (size_t)B * C;
    hipLaunchKernelGGL((dice_bwd_px_kernel<T, LT>), dim3((unsigned)((long long)B * tpi)), dim3(DICE_THREADS), 0, stream, (const T*)logit,
                       (const LT*)label, lse, sums, cw, grad_out, spx, coef, tpi, B, C, h, w, H, W, ignore_index, (double)smooth);
    const long long n_out = (long long)B * C * h * w;
    dispatch_lanes(DICE_THREADS, n_out, h, w, H, W, [&](auto lanes, dim3 grid) {
        hipLaunchKernelGGL((dice_bwd_kernel<T, LT, decltype(lanes)::value>), grid, dim3(DICE_THREADS), 0, stream, (const T*)logit, (const LT*)label,
                           lse, spx, coef, (T*)dlogit, n_out, C, h, w, H, W, ignore_index);
    });
    return (int)hipGetLastError();
}
}  // namespace

int resize_dice_pixels() { return DICE_PX; }
int resize_dice_threads() { return DICE_THREADS; }
int resize_dice_max_classes() { return DICE_MAX_C; }

// 32-bit words: the larger of the forward's partials ([tiles][C][3] + [tiles] counts, tiles = B ceil(H W / DICE_PX)) and the
// backward's coefficients + per-pixel buffer (4 B C + B H W); both calls start at the workspace's first word
long long resize_dice_workspace_bytes(int B, int C, int H, int W) {
    const long long tiles = (long long)B * tiles_of(H, W);
    const long long fwd = tiles * (3LL * C + 1), bwd = (long long)B * H * W + 4LL * B * C;
    return 4 * (fwd > bwd ? fwd : bwd);
}

// extents >= 1, C <= DICE_MAX_C, B C h w and B H W and the launches below 2^31, aligned non-null buffers: checked by the caller
// (capi.hip)
int resize_dice_fwd_launch(const void* logit, const void* label, const float* class_weight, void* workspace, float* lse, double* sums, float* loss,
                           int64_t* correct, int B, int C, int h, int w, int H, int W, int ignore_index, float smooth, int logit_dtype,
                           int label_dtype, hipStream_t stream) {
    uint32_t* ws = (uint32_t*)workspace;
    return dispatch_types(logit_dtype, label_dtype, [&](auto t, auto lt) {
        return fwd_typed<decltype(t), decltype(lt)>(logit, label, class_weight, ws, lse, sums, loss, correct, B, C, h, w, H, W, ignore_index, smooth,
                                                    stream);
    });
}

int resize_dice_bwd_launch(const void* logit, const void* label, const float* lse, const double* sums, const float* class_weight,
                           const float* grad_out, void* workspace, void* dlogit, int B, int C, int h, int w, int H, int W, int ignore_index,
                           float smooth, int logit_dtype, int label_dtype, hipStream_t stream) {
    float* ws = (float*)workspace;
    return dispatch_types(logit_dtype, label_dtype, [&](auto t, auto lt) {
        return bwd_typed<decltype(t), decltype(lt)>(logit, label, lse, sums, class_weight, grad_out, ws, dlogit, B, C, h, w, H, W, ignore_index,
                                                    smooth, stream);
    });
}

}  // namespace ppn
