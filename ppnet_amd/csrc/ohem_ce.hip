// ohem_ce.hip — a segmentation head's training loss with online hard example mining and class weights, forward and backward, without
// the resized logits: what mmseg composes from resize + OHEMPixelSampler.sample (core/seg/sampler/ohem_pixel_sampler.py:32-85: a
// softmax, a gather, a boolean index and a full sort of the valid pixels) + CrossEntropyLoss(class_weight)(weight=seg_weight)
// (losses/cross_entropy_loss.py:10-33, losses/utils.py:47-76).  Here the sampler is a SELECTION: the k-th order statistic of one
// float32 score per pixel, found by a radix select over integer histograms, on top of the per-pixel state resize_ce.hip computes.
//
//   z_c(Y, X) = the four taps of logit [B][C][h][w] (resize_tap.h: resize_ce.hip's own interpolated logit, bit for bit)
//   lse = log sum_c exp z_c,   ce = lse - z_label,   p = exp(z_label - lse),   cw = class_weight or all ones
//   score     = p (mode 1: `thresh` given)  |  cw[label] ce (mode 2: top-k; mode 0: no sampler)
//               an IGNORED pixel (label == ignore_index or outside [0, C)) gets the sentinel NaN: no comparison with it is true, so it
//               is never selected, and the histograms skip it, so it is never counted.  A valid pixel's score that comes out NaN
//               (NaN logits) is stored as +inf and -0 as +0, so the 32-bit key below orders exactly as the float comparison does.
//   mode 1    t = max(asc_sorted(p)[min(batch_kept, n_valid - 1)], thresh);  selected = p < t;  n_valid == 0: t = thresh
//   mode 2    t = asc_sorted(score)[n_valid - min(batch_kept, n_valid)];     selected = score >= t — ties at the cut are ALL kept (the
//             reference leaves the choice among them to an unstable sort: the one deliberate difference);  n_valid == 0: t = +inf
//   mode 0    t = -inf;  selected = score >= t: every valid pixel
//   loss      = 1 / (B H W) sum_selected cw[label] ce          (weight_reduce_loss with avg_factor None: the mean over ALL pixels)
//   dlogit[b][c][y][x] = g / (B H W) sum_{selected (Y, X) whose taps touch (y, x)} wy wx cw[label] (exp(z_c - lse) - [label == c])
//
//   key       the float's bits with the sign flipped (negative: all bits flipped): unsigned order = float order.  Three digits,
//             OH_BITS1 | OH_BITS2 | OH_BITS3 = 11 | 11 | 10 bits: 2048 int32 LDS bins (8 KB, a quarter of what lets four workgroups share
//             a CU's LDS) and three passes — 8-bit digits would need four, 16-bit digits 256 KB of bins.  Scores crowd: a trained
//             head's p sits in [0.5, 1), ONE exponent, so the first digit (sign, exponent, two mantissa bits) sends a wave's 64 adds to
//             a handful of bins and an LDS atomic serialises per address.  hist_add therefore peels the two most likely bins per wave
//             first — the bin of the first live lane, a ballot of the lanes that share it, one add of the popcount, twice — and
//             only the lanes left add one by one; on spread digits (the second and third, uniform inside a bin) the two rounds cost
//             two ballots.  A workgroup then adds its non-zero bins to the global histogram with one integer atomic each.
//   kernels   ohem_score    a work-item per pixel (grid-stride over tiles of OH_PX, at most OH_MAX_GROUPS workgroups): lse, score,
//                           correct, n_valid, first-digit histogram
//             ohem_hist<2>  every workgroup finds the first digit's bin of rank k from the global histogram (the same integers: the
//                           same bin), then histograms the second digit of the scores inside it; ohem_hist<3> likewise.  Only
//                           `score` is read, 4 bytes per pixel; the bin and the remaining rank stay on the device (workgroup 0 records them)
//             ohem_reduce   finds the third digit — the key is complete, t is a float — and sums cw ce over the selected pixels per
//                           workgroup in a fixed tree; writes mask when asked
//             ohem_final    one workgroup: the partial sums in double / int64 in a fixed order; loss, counts, threshold
//             ohem_bwd      resize_ce_bwd_kernel's gather (resize_tap.h's Gather: one writer per dlogit element, a fixed xor tree, no
//                           atomics) with the factor (selected ? cw[label] : 0), `selected` recomputed from score and the device
//                           threshold; a pixel that is not selected is skipped before its label is read
//             Six launches and one memset forward (mode 0: four), one backward.  Every sum of floats has a fixed order and every
//             atomic is an integer add: loss, threshold, mask and dlogit are bitwise reproducible.  Nothing is read back to the host.
//
// No kernel holds a runtime-C array (ScratchSize 0).  Element offsets are 64-bit; the caller (capi.hip) rejects B C h w, B H W and
// launches of 2^31 or more.  n_valid <= B H W < 2^31 fits every uint32 bin and rank.
//
// What this file does as resize_ce.hip does is not copied but included (resize_tap.h): the taps, ohem_score's softmax_sweep,
// ohem_reduce's group_sum, ohem_final's final_sum, ohem_bwd's Gather with tap_range and tap_weight, stf, and the host's dispatch_types
// and dispatch_lanes.  Here stay the select (keys, histograms, select_bin), the score and the gather's per-pixel term.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include "ppn_device.h"
#include "ppn_kernels.h"
#include "resize_tap.h"

namespace ppn {

namespace {
constexpr int OH_THREADS = 256;                        // work-items per workgroup, every kernel
constexpr int OH_PER_THREAD = 4;
constexpr int OH_PX = OH_THREADS * OH_PER_THREAD;      // pixels per tile
constexpr int OH_MAX_GROUPS = 1024;                    // 4 workgroups per CU of a 256-CU device; more tiles are strided over
constexpr int OH_BITS1 = 11;
constexpr int OH_BITS2 = 11;
constexpr int OH_BITS3 = 10;
static_assert(OH_BITS1 + OH_BITS2 + OH_BITS3 == 32, "the three digits make the key");
constexpr int OH_BINS = 1 << OH_BITS1;                 // LDS bins of a pass (the widest digit)
static_assert(OH_BITS2 <= OH_BITS1 && OH_BITS3 <= OH_BITS1 && OH_BINS % OH_THREADS == 0 && (1 << OH_BITS3) % OH_THREADS == 0, "select_bin's shares");
// workspace, in 32-bit words: three global histograms | state | per-workgroup partial loss sums (float32) | kept counts (int32)
constexpr int OH_HIST2 = OH_BINS, OH_HIST3 = 2 * OH_BINS, OH_STATE = 3 * OH_BINS;
constexpr int OH_ST_VALID = 0, OH_ST_CORRECT = 1, OH_ST_BIN1 = 2, OH_ST_RANK1 = 3, OH_ST_BIN2 = 4, OH_ST_RANK2 = 5, OH_ST_THRESHOLD = 6;
constexpr int OH_HEADER = OH_STATE + 16;               // zeroed on the stream by every forward call
constexpr int OH_PARTIAL = OH_HEADER, OH_KEPT = OH_PARTIAL + OH_MAX_GROUPS, OH_WORDS = OH_KEPT + OH_MAX_GROUPS;

__device__ __forceinline__ uint32_t score_key(float s) {
    const uint32_t u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float key_score(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ bool selected(float s, float t, int mode) { return mode == 1 ? s < t : s >= t; }   // false for the NaN sentinel

// rank of the cut among the n_valid ascending scores (n_valid >= 1)
__device__ __forceinline__ uint32_t cut_rank(uint32_t n_valid, uint32_t batch_kept, int mode) {
    return mode == 1 ? min(batch_kept, n_valid - 1u) : n_valid - min(batch_kept, n_valid);
}

// `on` lanes add 1 to s_hist[bin]; every lane of the wave calls it.  Two rounds peel the bin of the first live lane with one add of a
// popcount; the lanes left add one by one.
__device__ __forceinline__ void hist_add(uint32_t* s_hist, bool on, uint32_t bin) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const unsigned long long todo = __ballot(on);
        if (todo == 0) return;                                               // wave-uniform
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t b = (uint32_t)__shfl((int)bin, leader, 64);
        const bool same = on && bin == b;
        const unsigned long long m = __ballot(same);
        if (lane == leader) atomicAdd(&s_hist[b], (uint32_t)__popcll(m));
        on = on && !same;
    }
    if (on) atomicAdd(&s_hist[bin], 1u);
}

__device__ __forceinline__ void hist_flush(const uint32_t* s_hist, uint32_t* g_hist, int bins) {
    for (int i = threadIdx.x; i < bins; i += OH_THREADS) {
        const uint32_t v = s_hist[i];
        if (v) atomicAdd(g_hist + i, v);
    }
}

// the bin of NB that holds rank k of the histogram, and k's rank inside it; the same for every work-item.  A work-item takes NB /
// OH_THREADS consecutive bins; their sums are scanned over the workgroup.  k below the histogram's total (the caller's n_valid >= 1).
template <int NB>
__device__ __forceinline__ void select_bin(const uint32_t* __restrict__ hist, uint32_t k, uint32_t* s_tmp /* [8] */, uint32_t& bin, uint32_t& rem) {
    constexpr int PER = NB / OH_THREADS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t c[PER], sum = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) { c[i] = hist[tid * PER + i]; sum += c[i]; }
    uint32_t inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)inc, o, 64);
        if (lane >= o) inc += v;
    }
    if (lane == 63) s_tmp[wave] = inc;
    if (tid == 0) { s_tmp[4] = 0; s_tmp[5] = 0; }
    __syncthreads();
    uint32_t excl = inc - sum;
    for (int i = 0; i < wave; ++i) excl += s_tmp[i];
    if (sum > 0 && k >= excl && k - excl < sum) {                           // one work-item
        uint32_t r = k - excl, b = 0, found = 0;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            if (!found) {
                if (r < c[i]) { b = (uint32_t)(tid * PER + i); found = 1; }
                else r -= c[i];
            }
        }
        s_tmp[4] = b;
        s_tmp[5] = r;
    }
    __syncthreads();
    bin = s_tmp[4];
    rem = s_tmp[5];
    __syncthreads();                                                         // s_tmp may be reused
}

template <typename T, typename LT>
__global__ __launch_bounds__(OH_THREADS) void ohem_score_kernel(const T* __restrict__ logit, const LT* __restrict__ label,
                                                                 const float* __restrict__ cw, float* __restrict__ lse,
                                                                 float* __restrict__ score, uint32_t* __restrict__ ws, int n_tiles, int n_px,
                                                                 int C, int h, int w, int H, int W, int ignore_index, int mode) {
    __shared__ uint32_t s_hist[OH_BINS];
    __shared__ int s_cnt[2 * (OH_THREADS / 64)];
    const int tid = threadIdx.x;
    for (int i = tid; i < OH_BINS; i += OH_THREADS) s_hist[i] = 0;
    __syncthreads();
    const size_t plane = (size_t)h * w;
    const int HW = H * W;
    int correct = 0, n_valid = 0;
    for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) {                  // uniform over the workgroup: hist_add sees whole waves
#pragma unroll 1
        for (int k = 0; k < OH_PER_THREAD; ++k) {
            const long long pl = (long long)t * OH_PX + k * OH_THREADS + tid;
            bool on = false;
            uint32_t key = 0;
            if (pl < n_px) {
                const int p = (int)pl;
                const int b = p / HW, r = p - b * HW, Y = r / W, X = r - Y * W;
                const Tap ty = bilinear_tap(Y, h, H), tx = bilinear_tap(X, w, W);
                const int r0 = ty.i0 * w, r1 = ty.i1 * w;
                const T* img = logit + (size_t)b * C * plane;
                const int lab = valid_label(label, (size_t)p, C, ignore_index);
                const Sweep sw = softmax_sweep(img, plane, C, r0, r1, ty, tx, lab);
                const float l = sw.m + logf(sw.s);
                lse[p] = l;
                float sc = __uint_as_float(0x7fc00000u);                     // ignored: the NaN sentinel
                if (lab >= 0) {
                    sc = mode == 1 ? expf(sw.zl - l) : (cw ? cw[lab] : 1.f) * (l - sw.zl);
                    sc = (sc != sc) ? INFINITY : sc + 0.f;                   // a valid pixel is never NaN; -0 becomes +0
                    correct += (sw.arg == lab);
                    n_valid += 1;
                    on = mode != 0;
                    key = score_key(sc);
                }
                score[p] = sc;
            }
            hist_add(s_hist, on, key >> (32 - OH_BITS1));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        correct += __shfl_xor(correct, o, 64);
        n_valid += __shfl_xor(n_valid, o, 64);
    }
    if ((tid & 63) == 0) { s_cnt[tid >> 6] = correct; s_cnt[OH_THREADS / 64 + (tid >> 6)] = n_valid; }
    __syncthreads();
    if (tid == 0) {
        int a = 0, n = 0;
#pragma unroll
        for (int i = 0; i < OH_THREADS / 64; ++i) { a += s_cnt[i]; n += s_cnt[OH_THREADS / 64 + i]; }
        if (a) atomicAdd(ws + OH_STATE + OH_ST_CORRECT, (uint32_t)a);
        if (n) atomicAdd(ws + OH_STATE + OH_ST_VALID, (uint32_t)n);
    }
    if (mode != 0) hist_flush(s_hist, ws, OH_BINS);
}

// DIGIT 2: the bin of the first digit from the first histogram, then the second digit's histogram of the scores inside it;
// DIGIT 3: the bin of the second digit from the second histogram (and the recorded first), then the third digit's histogram.
template <int DIGIT>
__global__ __launch_bounds__(OH_THREADS) void ohem_hist_kernel(const float* __restrict__ score, uint32_t* __restrict__ ws, int n_tiles, int n_px,
                                                                uint32_t batch_kept, int mode) {
    __shared__ uint32_t s_hist[OH_BINS];
    __shared__ uint32_t s_tmp[8];
    const int tid = threadIdx.x;
    const uint32_t n_valid = ws[OH_STATE + OH_ST_VALID];
    if (n_valid == 0) return;                                                // uniform: nothing to select
    constexpr int BINS = 1 << (DIGIT == 2 ? OH_BITS2 : OH_BITS3);
    constexpr int SHIFT = DIGIT == 2 ? OH_BITS3 : 0;                         // of this pass's digit
    constexpr int PSHIFT = DIGIT == 2 ? 32 - OH_BITS1 : OH_BITS3;            // of the prefix found so far
    for (int i = tid; i < BINS; i += OH_THREADS) s_hist[i] = 0;
    uint32_t bin, rem, prefix;
    if constexpr (DIGIT == 2) {
        select_bin<OH_BINS>(ws, cut_rank(n_valid, batch_kept, mode), s_tmp, bin, rem);
        prefix = bin;
        if (blockIdx.x == 0 && tid == 0) { ws[OH_STATE + OH_ST_BIN1] = bin; ws[OH_STATE + OH_ST_RANK1] = rem; }
    } else {
        select_bin<(1 << OH_BITS2)>(ws + OH_HIST2, ws[OH_STATE + OH_ST_RANK1], s_tmp, bin, rem);
        prefix = (ws[OH_STATE + OH_ST_BIN1] << OH_BITS2) | bin;
        if (blockIdx.x == 0 && tid == 0) { ws[OH_STATE + OH_ST_BIN2] = prefix; ws[OH_STATE + OH_ST_RANK2] = rem; }
    }                                                                        // (select_bin ends on a barrier: s_hist is zero for all)
    for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) {
#pragma unroll 1
        for (int k = 0; k < OH_PER_THREAD; ++k) {
            const long long pl = (long long)t * OH_PX + k * OH_THREADS + tid;
            bool on = false;
            uint32_t key = 0;
            if (pl < n_px) {
                const float s = score[pl];
                key = score_key(s);
                on = s == s && (key >> PSHIFT) == prefix;
            }
            hist_add(s_hist, on, (key >> SHIFT) & (uint32_t)(BINS - 1));
        }
    }
    __syncthreads();
    hist_flush(s_hist, ws + (DIGIT == 2 ? OH_HIST2 : OH_HIST3), BINS);
}

template <typename T, typename LT>
__global__ __launch_bounds__(OH_THREADS) void ohem_reduce_kernel(const T* __restrict__ logit, const LT* __restrict__ label,
                                                                  const float* __restrict__ cw, const float* __restrict__ lse,
                                                                  const float* __restrict__ score, uint8_t* __restrict__ mask,
                                                                  uint32_t* __restrict__ ws, int n_tiles, int n_px, int C, int h, int w, int H,
                                                                  int W, int ignore_index, int mode, float thresh) {
    __shared__ uint32_t s_tmp[8];
    __shared__ float s_loss[OH_THREADS / 64];
    __shared__ int s_kept[OH_THREADS / 64];
    const int tid = threadIdx.x;
    const uint32_t n_valid = ws[OH_STATE + OH_ST_VALID];
    float t;
    if (mode == 0) t = -INFINITY;
    else if (n_valid == 0) t = mode == 1 ? thresh : INFINITY;
    else {
        uint32_t bin, rem;
        select_bin<(1 << OH_BITS3)>(ws + OH_HIST3, ws[OH_STATE + OH_ST_RANK2], s_tmp, bin, rem);
        t = key_score((ws[OH_STATE + OH_ST_BIN2] << OH_BITS3) | bin);
        if (mode == 1) t = fmaxf(t, thresh);
    }
    if (blockIdx.x == 0 && tid == 0) ws[OH_STATE + OH_ST_THRESHOLD] = __float_as_uint(t);
    const size_t plane = (size_t)h * w;
    const int HW = H * W;
    float loss = 0.f;
    int kept = 0;
    for (int tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
#pragma unroll 1
        for (int k = 0; k < OH_PER_THREAD; ++k) {
            const long long pl = (long long)tl * OH_PX + k * OH_THREADS + tid;
            if (pl >= n_px) continue;
            const int p = (int)pl;
            const bool sel = selected(score[p], t, mode);
            if (mask) mask[p] = sel ? 1 : 0;
            if (!sel) continue;
            const int lab = valid_label(label, (size_t)p, C, ignore_index);
            if (lab < 0) continue;                                           // (its score is the sentinel: never selected)
            const int b = p / HW, r = p - b * HW, Y = r / W, X = r - Y * W;
            const Tap ty = bilinear_tap(Y, h, H), tx = bilinear_tap(X, w, W);
            const float zl = interp(logit + ((size_t)b * C + lab) * plane, ty.i0 * w, ty.i1 * w, ty, tx);   // the score pass's z_label, bit for bit
            loss += (cw ? cw[lab] : 1.f) * (lse[p] - zl);
            kept += 1;
        }
    }
    const FloatInt sum = group_sum<OH_THREADS>(loss, kept, s_loss, s_kept);  // a fixed tree
    if (tid == 0) {
        reinterpret_cast<float*>(ws)[OH_PARTIAL + blockIdx.x] = sum.a;
        reinterpret_cast<int*>(ws)[OH_KEPT + blockIdx.x] = sum.n;
    }
}

// one workgroup: the partial sums in double / int64, each work-item a strided share in order, then a fixed tree through LDS
__global__ __launch_bounds__(OH_THREADS) void ohem_final_kernel(const uint32_t* __restrict__ ws, int n_groups, double n_px, float* __restrict__ loss,
                                                                 long long* __restrict__ counts, float* __restrict__ threshold) {
    __shared__ double s_a[OH_THREADS];
    __shared__ long long s_n[OH_THREADS];
    const int tid = threadIdx.x;
    const float* part = reinterpret_cast<const float*>(ws) + OH_PARTIAL;
    const int* kept = reinterpret_cast<const int*>(ws) + OH_KEPT;
    double a = 0.0;
    long long n = 0;
    for (int i = tid; i < n_groups; i += OH_THREADS) { a += (double)part[i]; n += kept[i]; }
    final_sum<OH_THREADS>(a, n, s_a, s_n);
    if (tid == 0) {
        *loss = (float)(a / n_px);
        counts[0] = (long long)ws[OH_STATE + OH_ST_CORRECT];
        counts[1] = (long long)ws[OH_STATE + OH_ST_VALID];
        counts[2] = n;
        *threshold = __uint_as_float(ws[OH_STATE + OH_ST_THRESHOLD]);
    }
}

template <typename T, typename LT, int LANES>
__global__ __launch_bounds__(OH_THREADS) void ohem_bwd_kernel(const T* __restrict__ logit, const LT* __restrict__ label,
                                                               const float* __restrict__ cw, const float* __restrict__ lse,
                                                               const float* __restrict__ score, const float* __restrict__ threshold,
                                                               const float* __restrict__ grad_out, T* __restrict__ dlogit, long long n_out, int C,
                                                               int h, int w, int H, int W, int ignore_index, int mode, float inv_px) {
    const Gather<OH_THREADS, LANES> out(n_out, C, h, w);
    const T* plane = logit + (size_t)out.bc * h * w;
    const float t = *threshold;
    const double acc = out.sum(true, h, w, H, W, [&](double& sum, size_t p, int Y, int X) {
        if (!selected(score[p], t, mode)) return;          // before the label is read
        const int lab = valid_label(label, p, C, ignore_index);
        if (lab < 0) return;
        const Tap ty = bilinear_tap(Y, h, H), tx = bilinear_tap(X, w, W);
        const float z = interp(plane, ty.i0 * w, ty.i1 * w, ty, tx);
        const float g = (cw ? cw[lab] : 1.f) * (expf(z - lse[p]) - (lab == out.c ? 1.f : 0.f));
        sum += (double)(tap_weight(ty, out.y) * tap_weight(tx, out.x) * g);   // a float32 product, rounded once, then widened
    });
    if (out.live && out.lane() == 0) stf(dlogit + out.o, (float)acc * (*grad_out * inv_px));
}

template <typename T, typename LT>
int fwd_typed(const void* logit, const void* label, const float* cw, float* lse, float* score, float* loss, int64_t* counts, float* threshold,
              uint8_t* mask, uint32_t* ws, int B, int C, int h, int w, int H, int W, int ignore_index, int mode, float thresh, uint32_t batch_kept,
              hipStream_t stream) {
    const long long n_px = (long long)B * H * W;
    const int tiles = (int)((n_px + OH_PX - 1) / OH_PX);
    const int groups = tiles < OH_MAX_GROUPS ? tiles : OH_MAX_GROUPS;
    const hipError_t e = hipMemsetAsync(ws, 0, sizeof(uint32_t) * OH_HEADER, stream);
    if (e != hipSuccess) return (int)e;
    const dim3 grid((unsigned)groups), block(OH_THREADS);
    hipLaunchKernelGGL((ohem_score_kernel<T, LT>), grid, block, 0, stream, (const T*)logit, (const LT*)label, cw, lse, score, ws, tiles, (int)n_px, C, h,
                       w, H, W, ignore_index, mode);
    if (mode != 0) {
        hipLaunchKernelGGL(ohem_hist_kernel<2>, grid, block, 0, stream, (const float*)score, ws, tiles, (int)n_px, batch_kept, mode);
        hipLaunchKernelGGL(ohem_hist_kernel<3>, grid, block, 0, stream, (const float*)score, ws, tiles, (int)n_px, batch_kept, mode);
    }
    hipLaunchKernelGGL((ohem_reduce_kernel<T, LT>), grid, block, 0, stream, (const T*)logit, (const LT*)label, cw, (const float*)lse,
                       (const float*)score, mask, ws, tiles, (int)n_px, C, h, w, H, W, ignore_index, mode, thresh);
    hipLaunchKernelGGL(ohem_final_kernel, dim3(1), block, 0, stream, (const uint32_t*)ws, groups, (double)n_px, loss, (long long*)counts, threshold);
    return (int)hipGetLastError();
}

template <typename T, typename LT>
int bwd_typed(const void* logit, const void* label, const float* cw, const float* lse, const float* score, const float* threshold,
              const float* grad_out, void* dlogit, int B, int C, int h, int w, int H, int W, int ignore_index, int mode, hipStream_t stream) {
    const long long n_out = (long long)B * C * h * w;
    dispatch_lanes(OH_THREADS, n_out, h, w, H, W, [&](auto lanes, dim3 grid) {
        hipLaunchKernelGGL((ohem_bwd_kernel<T, LT, decltype(lanes)::value>), grid, dim3(OH_THREADS), 0, stream, (const T*)logit, (const LT*)label,
                           cw, lse, score, threshold, grad_out, (T*)dlogit, n_out, C, h, w, H, W, ignore_index, mode,
                           1.0f / (float)((long long)B * H * W));
    });
    return (int)hipGetLastError();
}
}  // namespace

int ohem_ce_pixels() { return OH_PX; }
int ohem_ce_threads() { return OH_THREADS; }
int ohem_ce_max_groups() { return OH_MAX_GROUPS; }

// three histograms, the state, and a partial loss sum and a kept count per workgroup: the same for every size
long long ohem_ce_workspace_bytes() { return (long long)sizeof(uint32_t) * OH_WORDS; }

// extents >= 1, B C h w and B H W and the launches below 2^31, aligned non-null buffers, mode 0 / 1 / 2, batch_kept >= 1: checked by
// the caller (capi.hip)
int ohem_ce_fwd_launch(const void* logit, const void* label, const float* class_weight, float* lse, float* score, float* loss, int64_t* counts,
                       float* threshold, uint8_t* mask, void* workspace, int B, int C, int h, int w, int H, int W, int ignore_index, int mode,
                       float thresh, uint32_t batch_kept, int logit_dtype, int label_dtype, hipStream_t stream) {
    uint32_t* ws = (uint32_t*)workspace;
    return dispatch_types(logit_dtype, label_dtype, [&](auto t, auto lt) {
        return fwd_typed<decltype(t), decltype(lt)>(logit, label, class_weight, lse, score, loss, counts, threshold, mask, ws, B, C, h, w, H, W,
                                                    ignore_index, mode, thresh, batch_kept, stream);
    });
}

int ohem_ce_bwd_launch(const void* logit, const void* label, const float* class_weight, const float* lse, const float* score, const float* threshold,
                       const float* grad_out, void* dlogit, int B, int C, int h, int w, int H, int W, int ignore_index, int mode, int logit_dtype,
                       int label_dtype, hipStream_t stream) {
    return dispatch_types(logit_dtype, label_dtype, [&](auto t, auto lt) {
        return bwd_typed<decltype(t), decltype(lt)>(logit, label, class_weight, lse, score, threshold, grad_out, dlogit, B, C, h, w, H, W,
                                                    ignore_index, mode, stream);
    });
}

}  // namespace ppn
