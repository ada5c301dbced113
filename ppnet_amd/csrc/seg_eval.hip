// seg_eval.hip — the area histograms of a segmentation evaluation without the resized logits: what mmseg's evaluation composes from
// resize + softmax + argmax (encoder_decoder.py:200-265) and intersect_and_union (core/evaluation/metrics.py:26-86).
//
//   z_c(Y, X)  = a0 (b0 z00 + b1 z01) + a1 (b0 z10 + b1 z11)      resize_tap.h: resize_ce.hip's own taps of logit [B][C][h][w]
//   pred(Y, X) = the lowest c with z_c = max_c z_c                one sweep over the channels, no exponentials (the argmax of the
//                                                                 softmax is the argmax of the logits); a NaN logit never wins
//   areas[0][c] = #{valid (Y, X): pred == label == c}             intersect
//   areas[1][c] = #{valid (Y, X): pred == c}                      prediction
//   areas[2][c] = #{valid (Y, X): label == c}                     label            (union = areas[1] + areas[2] - areas[0])
//
// The interpolated logit is resize_ce.hip's bit for bit (the same inline functions, -ffp-contract=off), and the sweep keeps the first
// maximum as resize_ce_fwd_kernel's does, so the sum of areas[0] is the `correct` of ppn_resize_ce_fwd.  The sweep starts from -inf
// instead of class 0's logit: the same argmax for every input without a NaN, and a NaN (no comparison with it is true) can neither
// win nor block a later class — torch.argmax treats NaN as the maximum, the one difference.  A label that is ignore_index, or outside
// [0, C), is ignored (valid_label): it adds to none of the three histograms and never indexes memory.  mmseg masks by
// label != ignore_index only, so an out-of-range label would still count in its prediction histogram: the deliberate difference.
//
//   counting  a work-item takes SE_PER_THREAD consecutive pixels of a tile of SE_PX (so pred goes out as one 32-bit store per
//             work-item where the address allows), a workgroup strides over the tiles (at most SE_MAX_GROUPS workgroups: the number
//             of global atomics is bounded by the grid, not by the image) and counts into int32 LDS bins [3][C]:
//               C <= SE_BALLOT_C  per class and pixel slot three wave ballots, their popcounts summed in scalar registers, and one
//                                 LDS add per wave, class and histogram — 64 lanes adding into two bins would serialise (the
//                                 project's own workload is C = 2);
//               above             an LDS integer atomic per valid pixel and histogram.
//             At the end one 64-bit global atomic add per non-zero bin into areas, which the launch zeroes on the stream first.
//             Integers only: the result does not depend on the order of the adds and is bitwise reproducible.
//
// No kernel holds a runtime-C array: the sweep loops over the channels, the per-slot state is four registers (ScratchSize 0).  Element
// offsets are 64-bit; the caller (capi.hip) rejects B C h w and B H W of 2^31 or more and C > SE_MAX_C.  A workgroup counts at most
// ceil(tiles / groups) * SE_PX < 2^31 pixels, so an int32 bin cannot overflow.
//
// From resize_tap.h: the taps (Tap, bilinear_tap, ldf, interp, valid_label) and the host's dispatch_types.  The header's softmax_sweep
// is NOT used here: this sweep starts from -inf (above) and needs neither z_label nor the exponentials.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include "ppn_device.h"
#include "ppn_kernels.h"
#include "resize_tap.h"

namespace ppn {

namespace {
constexpr int SE_THREADS = 256;                        // work-items per workgroup
constexpr int SE_PER_THREAD = 4;                       // consecutive pixels of a work-item: one packed pred store
constexpr int SE_PX = SE_THREADS * SE_PER_THREAD;      // pixels per tile
constexpr int SE_MAX_GROUPS = 1024;                    // 4 workgroups per CU of a 256-CU device; more tiles are strided over
constexpr int SE_BALLOT_C = 8;                         // up to here wave ballots; above, LDS atomics
constexpr int SE_MAX_C = 256;                          // pred is uint8; s_hist is [3][SE_MAX_C]
static_assert(SE_PER_THREAD == 4, "the packed pred store writes four pixels as one uint32");

template <typename T, typename LT, bool BALLOT>
__global__ __launch_bounds__(SE_THREADS) void seg_eval_kernel(const T* __restrict__ logit, const LT* __restrict__ label,
                                                               uint8_t* __restrict__ pred, unsigned long long* __restrict__ areas, int n_tiles,
                                                               int n_px, int C, int h, int w, int H, int W, int ignore_index) {
    __shared__ int s_hist[3 * SE_MAX_C];               // [3][C]: intersect | pred | label
    const int tid = threadIdx.x;
    for (int i = tid; i < 3 * C; i += SE_THREADS) s_hist[i] = 0;
    __syncthreads();
    const size_t plane = (size_t)h * w;
    const int HW = H * W;
    for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) {                // uniform over the workgroup: the ballots below see whole waves
        const long long p0 = (long long)t * SE_PX + tid * SE_PER_THREAD;
        int arg[SE_PER_THREAD], lab[SE_PER_THREAD];
#pragma unroll
        for (int k = 0; k < SE_PER_THREAD; ++k) {
            arg[k] = 0;
            lab[k] = -1;                                                   // past the end: ignored
            if (p0 + k < n_px) {
                const int p = (int)(p0 + k);
                const int b = p / HW, r = p - b * HW, Y = r / W, X = r - Y * W;
                const Tap ty = bilinear_tap(Y, h, H), tx = bilinear_tap(X, w, W);
                const int r0 = ty.i0 * w, r1 = ty.i1 * w;
                const T* img = logit + (size_t)b * C * plane;
                float m = -INFINITY;
                int a = 0;
                for (int c = 0; c < C; ++c) {
                    const float z = interp(img + c * plane, r0, r1, ty, tx);
                    if (z > m) { m = z; a = c; }                           // ties keep the lowest class; a NaN never wins
                }
                arg[k] = a;
                lab[k] = valid_label(label, (size_t)p, C, ignore_index);
            }
        }
        if (pred) {
            uint8_t* q = pred + p0;
            if (p0 + SE_PER_THREAD <= n_px && ((uintptr_t)q & 3) == 0) {
                *reinterpret_cast<uint32_t*>(q) = (uint32_t)arg[0] | ((uint32_t)arg[1] << 8) | ((uint32_t)arg[2] << 16) | ((uint32_t)arg[3] << 24);
            } else {
#pragma unroll
                for (int k = 0; k < SE_PER_THREAD; ++k)
                    if (p0 + k < n_px) q[k] = (uint8_t)arg[k];
            }
        }
        if constexpr (BALLOT) {
            for (int c = 0; c < C; ++c) {
                int ni = 0, np = 0, nl = 0;                                // wave-uniform
#pragma unroll
                for (int k = 0; k < SE_PER_THREAD; ++k) {
                    const bool lc = lab[k] == c, pc = lab[k] >= 0 && arg[k] == c;
                    ni += __popcll(__ballot(lc && pc));
                    np += __popcll(__ballot(pc));
                    nl += __popcll(__ballot(lc));
                }
                if ((tid & 63) == 0) {
                    if (ni) atomicAdd(&s_hist[c], ni);
                    if (np) atomicAdd(&s_hist[C + c], np);
                    if (nl) atomicAdd(&s_hist[2 * C + c], nl);
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < SE_PER_THREAD; ++k) {
                if (lab[k] >= 0) {                                         // lab < C and arg < C: inside [3][C]
                    if (arg[k] == lab[k]) atomicAdd(&s_hist[arg[k]], 1);
                    atomicAdd(&s_hist[C + arg[k]], 1);
                    atomicAdd(&s_hist[2 * C + lab[k]], 1);
                }
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < 3 * C; i += SE_THREADS) {
        const int v = s_hist[i];
        if (v) atomicAdd(areas + i, (unsigned long long)v);
    }
}

template <typename T, typename LT>
int eval_typed(const void* logit, const void* label, uint8_t* pred, int64_t* areas, int B, int C, int h, int w, int H, int W, int ignore_index,
               hipStream_t stream) {
    const long long n_px = (long long)B * H * W;
    const int tiles = (int)((n_px + SE_PX - 1) / SE_PX);
    const int groups = tiles < SE_MAX_GROUPS ? tiles : SE_MAX_GROUPS;
    const hipError_t e = hipMemsetAsync(areas, 0, sizeof(int64_t) * 3 * (size_t)C, stream);
    if (e != hipSuccess) return (int)e;
    if (C <= SE_BALLOT_C)
        hipLaunchKernelGGL((seg_eval_kernel<T, LT, true>), dim3((unsigned)groups), dim3(SE_THREADS), 0, stream, (const T*)logit, (const LT*)label, pred,
                           (unsigned long long*)areas, tiles, (int)n_px, C, h, w, H, W, ignore_index);
    else
        hipLaunchKernelGGL((seg_eval_kernel<T, LT, false>), dim3((unsigned)groups), dim3(SE_THREADS), 0, stream, (const T*)logit, (const LT*)label, pred,
                           (unsigned long long*)areas, tiles, (int)n_px, C, h, w, H, W, ignore_index);
    return (int)hipGetLastError();
}
}  // namespace

int seg_eval_pixels() { return SE_PX; }
int seg_eval_threads() { return SE_THREADS; }
int seg_eval_max_groups() { return SE_MAX_GROUPS; }
int seg_eval_max_classes() { return SE_MAX_C; }

// extents >= 1, C <= SE_MAX_C, B C h w and B H W below 2^31, aligned non-null buffers: checked by the caller (capi.hip)
int seg_eval_launch(const void* logit, const void* label, uint8_t* pred, int64_t* areas, int B, int C, int h, int w, int H, int W, int ignore_index,
                    int logit_dtype, int label_dtype, hipStream_t stream) {
    return dispatch_types(logit_dtype, label_dtype, [&](auto t, auto lt) {
        return eval_typed<decltype(t), decltype(lt)>(logit, label, pred, areas, B, C, h, w, H, W, ignore_index, stream);
    });
}

}  // namespace ppn
