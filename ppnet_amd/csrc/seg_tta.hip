// seg_tta.hip — the merge of a multi-scale + flip test-time augmentation in one launch: what mmseg's aug_test composes per
// augmentation from resize to the augmentation's image size, resize to ori_shape, softmax, flip back and add
// (encoder_decoder.py:200-285), from the heads' LOW-resolution logits to labels.
//
//   (Ys, Xs)    = (Y, X) | (Y, W-1-X) horizontal | (H-1-Y, X) vertical        the un-flip: output pixel (Y, X) reads the flipped source
//   z_c(a)      = the two bilinear resizes (h,w) -> (hm,wm) -> (H,W) composed: stage 2 takes bilinear_tap(Ys, hm, H) and
//                 bilinear_tap(Xs, wm, W); each of the up to 2 x 2 mid-grid positions they name is resize_tap.h's interp on the
//                 (h,w) plane with bilinear_tap(mid index, h, hm) / (.., w, wm) — at most 4 x 4 loads per class — and stage 2
//                 combines the four with the same interp (on a register array): both stages are torch's float32 rule
//   p_c(a)      = expf(z_c - m) * (1 / s),  m = max_c z_c,  s = sum_c expf(z_c - m)
//   mean_c      = (p_c(0) + p_c(1) + ... in index order) / (float)n_augs
//   pred(Y, X)  = the lowest c with mean_c = max_c mean_c; the sweep starts from -inf, so a NaN never wins and all NaN is class 0
//                 (seg_eval.hip's rule).  A NaN logit makes every p_c of its pixel NaN, hence every mean_c: class 0.
//
// float32 throughout; bfloat16 is widened on load and nothing is rounded to bfloat16 in between (the library composition rounds every
// tensor it materialises: the documented difference).  With one augmentation, hm = H, wm = W and no flip, stage 2 is 1 z + 0 z', so
// for finite logits z_c is seg_eval.hip's interpolated logit bit for bit and pred is ppn_seg_eval's pred.
//
//   geometry  seg_eval.hip's: ST_THREADS work-items, tiles of ST_PX pixels, ST_PER_THREAD consecutive pixels per work-item, so pred goes
//             out as one 32-bit store where the address allows.  One workgroup per tile and no stride: there is no per-workgroup state
//             to amortise (seg_eval.hip caps its grid to bound its global atomics; this kernel has none).  The row taps of an
//             augmentation are computed for a work-item's first pixel and again only where the row changes inside its four.
//   classes   C <= ST_REG_C  seg_tta_reg_kernel<T, C>, one instance per class count: the per-class sums of the four pixels are
//                            registers (every loop over c is unrolled, no accumulator is indexed dynamically); prob is optional
//             above          seg_tta_acc_kernel<T, ZLDS>: prob [B][C][H][W] is required and IS the accumulator.  The first augmentation
//                            writes it, the later ones add, the last divides and takes the argmax.  A work-item owns its pixels for
//                            every augmentation: no atomics, no race, nothing to zero before.  Three sweeps over the classes per
//                            augmentation and pixel (maximum, sum, probabilities) and no per-class registers:
//                              C <= ST_LDS_C  the first sweep keeps the pixel's C logits in LDS ([C][ST_THREADS] floats, a column per
//                                             work-item: no bank conflict, no barrier), the second replaces them by the exponentials,
//                                             the third reads those — 16 loads per class, not 48 (12 augmentations, C = 19 at
//                                             16 x 512^2: 14.9 ms with three sweeps of loads)
//                              above          every sweep interpolates again (C floats per work-item no longer fit 64 KB)
//                            The two forms compute the same floats in the same order.
//   arguments the augmentations travel as one by-value kernel argument (ST_MAX_AUGS x 32 bytes): no device allocation, no copy, no
//             synchronisation in the call.  The kernels read them with a uniform index.
//
// Every sum has a fixed order and one writer: bitwise reproducible.  Element offsets are 64-bit; the caller (capi.hip) rejects
// B C h w, B C H W and B H W of 2^31 or more, C > ST_MAX_C and more than ST_MAX_AUGS augmentations.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include "ppn_device.h"
#include "ppn_kernels.h"
#include "resize_tap.h"

namespace ppn {

namespace {
constexpr int ST_THREADS = 256;                        // work-items per workgroup
constexpr int ST_PER_THREAD = 4;                       // consecutive pixels of a work-item: one packed pred store
constexpr int ST_PX = ST_THREADS * ST_PER_THREAD;      // pixels per tile
constexpr int ST_MAX_AUGS = PPN_SEG_TTA_MAX_AUGS;      // augmentations of one launch
constexpr int ST_REG_C = PPN_SEG_TTA_REG_CLASSES;      // up to here the per-class sums are registers; above, prob accumulates
constexpr int ST_LDS_C = 64;                           // up to here the accumulating kernel keeps a pixel's logits in LDS (64 KB)
constexpr int ST_MAX_C = 256;                          // pred is uint8
static_assert(ST_PER_THREAD == 4, "the packed pred store writes four pixels as one uint32");
static_assert(sizeof(ppn_tta_aug) == 32, "the by-value argument block is ST_MAX_AUGS x 32 bytes");

struct TtaArgs { ppn_tta_aug a[ST_MAX_AUGS]; };

// one axis of the composed resize: the stage-2 tap on the mid grid and the stage-1 taps of the two mid positions it names
struct Tap2 { Tap s2, a, b; };

__device__ __forceinline__ Tap2 tta_taps(int P, int n_in, int n_mid, int n_out) {
    Tap2 t;
    t.s2 = bilinear_tap(P, n_mid, n_out);
    t.a = bilinear_tap(t.s2.i0, n_in, n_mid);
    t.b = bilinear_tap(t.s2.i1, n_in, n_mid);
    return t;
}

// the composed logit of one class: four stage-1 values by interp on the (h,w) plane, stage 2 by interp on the four
template <typename T>
__device__ __forceinline__ float tta_logit(const T* plane, int w, const Tap2& ty, const Tap2& tx) {
    const int a0 = ty.a.i0 * w, a1 = ty.a.i1 * w, b0 = ty.b.i0 * w, b1 = ty.b.i1 * w;
    float v[4];                                                            // the 2 x 2 mid-grid values, rows of two
    v[0] = interp(plane, a0, a1, ty.a, tx.a);
    v[1] = interp(plane, a0, a1, ty.a, tx.b);
    v[2] = interp(plane, b0, b1, ty.b, tx.a);
    v[3] = interp(plane, b0, b1, ty.b, tx.b);
    const Tap cx{0, 1, tx.s2.l0, tx.s2.l1};
    return interp(v, 0, 2, ty.s2, cx);
}

// a work-item's four pixels: batch index, row, column; past the end of the pixels: live false
struct Px { int b[ST_PER_THREAD], Y[ST_PER_THREAD], X[ST_PER_THREAD]; bool live[ST_PER_THREAD]; };

__device__ __forceinline__ Px decode_pixels(long long p0, int n_px, int H, int W) {
    Px q;
    const int HW = H * W;
#pragma unroll
    for (int k = 0; k < ST_PER_THREAD; ++k) {
        q.live[k] = p0 + k < n_px;
        const int p = q.live[k] ? (int)(p0 + k) : 0;
        q.b[k] = p / HW;
        const int r = p - q.b[k] * HW;
        q.Y[k] = r / W;
        q.X[k] = r - q.Y[k] * W;
    }
    return q;
}

__device__ __forceinline__ void store_pred(uint8_t* pred, long long p0, int n_px, const int (&arg)[ST_PER_THREAD]) {
    uint8_t* q = pred + p0;
    if (p0 + ST_PER_THREAD <= n_px && ((uintptr_t)q & 3) == 0) {
        *reinterpret_cast<uint32_t*>(q) = (uint32_t)arg[0] | ((uint32_t)arg[1] << 8) | ((uint32_t)arg[2] << 16) | ((uint32_t)arg[3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < ST_PER_THREAD; ++k)
            if (p0 + k < n_px) q[k] = (uint8_t)arg[k];
    }
}

template <typename T, int NC>
__global__ __launch_bounds__(ST_THREADS) void seg_tta_reg_kernel(const TtaArgs args, int n_augs, uint8_t* __restrict__ pred,
                                                                  float* __restrict__ prob, int n_px, int H, int W) {
    const long long p0 = (long long)blockIdx.x * ST_PX + threadIdx.x * ST_PER_THREAD;
    if (p0 >= n_px) return;
    const Px px = decode_pixels(p0, n_px, H, W);
    float acc[ST_PER_THREAD][NC];
#pragma unroll
    for (int k = 0; k < ST_PER_THREAD; ++k)
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[k][c] = 0.f;
    for (int a = 0; a < n_augs; ++a) {
        const ppn_tta_aug g = args.a[a];                                   // uniform: scalar loads of the argument block
        const size_t plane = (size_t)g.h * g.w;
        Tap2 ty = {};
        int Yprev = -1;
#pragma unroll
        for (int k = 0; k < ST_PER_THREAD; ++k) {
            if (!px.live[k]) continue;
            if (px.Y[k] != Yprev) {
                ty = tta_taps(g.flip == 2 ? H - 1 - px.Y[k] : px.Y[k], g.h, g.hm, H);
                Yprev = px.Y[k];
            }
            const Tap2 tx = tta_taps(g.flip == 1 ? W - 1 - px.X[k] : px.X[k], g.w, g.wm, W);
            const T* img = (const T*)g.logit + (size_t)px.b[k] * NC * plane;
            float z[NC], m = -INFINITY;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                z[c] = tta_logit(img + c * plane, g.w, ty, tx);
                if (z[c] > m) m = z[c];
            }
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                z[c] = expf(z[c] - m);
                s += z[c];
            }
            const float inv = 1.f / s;
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[k][c] += z[c] * inv;
            // the four pixels are independent and the scheduler would interleave all their 16 NC loads: one pixel's at a time keeps
            // the live registers at one pixel's taps and logits
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    const float n = (float)n_augs;
    int arg[ST_PER_THREAD];
#pragma unroll
    for (int k = 0; k < ST_PER_THREAD; ++k) {
        float m = -INFINITY;
        arg[k] = 0;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            acc[k][c] = acc[k][c] / n;
            if (acc[k][c] > m) { m = acc[k][c]; arg[k] = c; }              // ties keep the lowest class; a NaN never wins
        }
    }
    if (pred) store_pred(pred, p0, n_px, arg);
    if (prob) {
        const size_t HW = (size_t)H * W;
        // four pixels of one row (hence of one image) whose address allows: one 128-bit store per class
        const bool row = px.live[ST_PER_THREAD - 1] && px.X[0] + ST_PER_THREAD - 1 < W;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            float* q = prob + ((size_t)px.b[0] * NC + c) * HW + (size_t)px.Y[0] * W + px.X[0];
            if (row && ((uintptr_t)q & 15) == 0) {
                *reinterpret_cast<float4*>(q) = make_float4(acc[0][c], acc[1][c], acc[2][c], acc[3][c]);
            } else {
#pragma unroll
                for (int k = 0; k < ST_PER_THREAD; ++k)
                    if (px.live[k]) prob[((size_t)px.b[k] * NC + c) * HW + (size_t)px.Y[k] * W + px.X[k]] = acc[k][c];
            }
        }
    }
}

template <typename T, bool ZLDS>
__global__ __launch_bounds__(ST_THREADS) void seg_tta_acc_kernel(const TtaArgs args, int n_augs, uint8_t* __restrict__ pred,
                                                                  float* __restrict__ prob, int n_px, int C, int H, int W) {
    extern __shared__ float s_z[];                                         // ZLDS: [C][ST_THREADS], column threadIdx.x is this work-item's
    const long long p0 = (long long)blockIdx.x * ST_PX + threadIdx.x * ST_PER_THREAD;
    if (p0 >= n_px) return;                                                // (no barrier below)
    const Px px = decode_pixels(p0, n_px, H, W);
    const size_t HW = (size_t)H * W;
    const float n = (float)n_augs;
    float* zc = s_z + threadIdx.x;
    int arg[ST_PER_THREAD] = {0, 0, 0, 0};
    for (int a = 0; a < n_augs; ++a) {
        const ppn_tta_aug g = args.a[a];                                   // uniform: scalar loads of the argument block
        const size_t plane = (size_t)g.h * g.w;
        const bool first = a == 0, last = a == n_augs - 1;
        Tap2 ty = {};
        int Yprev = -1;
#pragma unroll
        for (int k = 0; k < ST_PER_THREAD; ++k) {
            if (!px.live[k]) continue;
            if (px.Y[k] != Yprev) {
                ty = tta_taps(g.flip == 2 ? H - 1 - px.Y[k] : px.Y[k], g.h, g.hm, H);
                Yprev = px.Y[k];
            }
            const Tap2 tx = tta_taps(g.flip == 1 ? W - 1 - px.X[k] : px.X[k], g.w, g.wm, W);
            const T* img = (const T*)g.logit + (size_t)px.b[k] * C * plane;
            float m = -INFINITY;
            for (int c = 0; c < C; ++c) {
                const float z = tta_logit(img + c * plane, g.w, ty, tx);
                if constexpr (ZLDS) zc[c * ST_THREADS] = z;
                if (z > m) m = z;
            }
            float s = 0.f;
            for (int c = 0; c < C; ++c) {
                float e;
                if constexpr (ZLDS) {
                    e = expf(zc[c * ST_THREADS] - m);
                    zc[c * ST_THREADS] = e;
                } else {
                    e = expf(tta_logit(img + c * plane, g.w, ty, tx) - m);
                }
                s += e;
            }
            const float inv = 1.f / s;
            float* q = prob + (size_t)px.b[k] * C * HW + (size_t)px.Y[k] * W + px.X[k];      // this pixel's class 0; classes HW apart
            float best = -INFINITY;
            int ak = 0;
            for (int c = 0; c < C; ++c) {
                float v;
                if constexpr (ZLDS) v = zc[c * ST_THREADS] * inv;
                else v = expf(tta_logit(img + c * plane, g.w, ty, tx) - m) * inv;
                if (!first) v = q[c * HW] + v;                             // the sum so far: this work-item wrote it
                if (last) {
                    v = v / n;
                    if (v > best) { best = v; ak = c; }                    // ties keep the lowest class; a NaN never wins
                }
                q[c * HW] = v;
            }
            arg[k] = ak;
        }
    }
    if (pred) store_pred(pred, p0, n_px, arg);
}

template <typename T, int NC>
void launch_reg(int C, const TtaArgs& args, int n_augs, uint8_t* pred, float* prob, int groups, int n_px, int H, int W, hipStream_t stream) {
    if constexpr (NC > ST_REG_C) {
        return;                                                            // C <= ST_REG_C: checked by the caller
    } else {
        if (C == NC)
            hipLaunchKernelGGL((seg_tta_reg_kernel<T, NC>), dim3((unsigned)groups), dim3(ST_THREADS), 0, stream, args, n_augs, pred, prob, n_px, H, W);
        else
            launch_reg<T, NC + 1>(C, args, n_augs, pred, prob, groups, n_px, H, W, stream);
    }
}

template <typename T>
int tta_typed(const TtaArgs& args, int n_augs, uint8_t* pred, float* prob, int B, int C, int H, int W, hipStream_t stream) {
    const long long n_px = (long long)B * H * W;
    const int groups = (int)((n_px + ST_PX - 1) / ST_PX);
    if (C <= ST_REG_C)
        launch_reg<T, 1>(C, args, n_augs, pred, prob, groups, (int)n_px, H, W, stream);
    else if (C <= ST_LDS_C)
        hipLaunchKernelGGL((seg_tta_acc_kernel<T, true>), dim3((unsigned)groups), dim3(ST_THREADS), sizeof(float) * ST_THREADS * (size_t)C, stream, args,
                           n_augs, pred, prob, (int)n_px, C, H, W);
    else
        hipLaunchKernelGGL((seg_tta_acc_kernel<T, false>), dim3((unsigned)groups), dim3(ST_THREADS), 0, stream, args, n_augs, pred, prob, (int)n_px, C, H, W);
    return (int)hipGetLastError();
}
}  // namespace

int seg_tta_pixels() { return ST_PX; }
int seg_tta_threads() { return ST_THREADS; }
int seg_tta_max_classes() { return ST_MAX_C; }

// 1 <= n_augs <= ST_MAX_AUGS, extents >= 1, flips in {0, 1, 2}, C <= ST_MAX_C, prob non-null for C > ST_REG_C, pred or prob non-null,
// B C h w, B C H W and B H W below 2^31, aligned non-null logits: checked by the caller (capi.hip)
int seg_tta_launch(const ppn_tta_aug* augs, int n_augs, uint8_t* pred, float* prob, int B, int C, int H, int W, int logit_dtype, hipStream_t stream) {
    TtaArgs args = {};
    for (int a = 0; a < n_augs; ++a) args.a[a] = augs[a];
    for (int a = n_augs; a < ST_MAX_AUGS; ++a) args.a[a] = augs[0];       // never read: valid values all the same
    return logit_dtype == 0 ? tta_typed<float>(args, n_augs, pred, prob, B, C, H, W, stream)
                            : tta_typed<__bf16>(args, n_augs, pred, prob, B, C, H, W, stream);
}

}  // namespace ppn
