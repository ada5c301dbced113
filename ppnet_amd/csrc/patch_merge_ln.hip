// patch_merge_ln.hip — DiNAT_s's PatchMerging (reference SegNet/dinats.py:74-104) in front of its reduction GEMM on gfx950: the 2 x 2
// gather of the token grid fused with the LayerNorm over the gathered 4C values, forward and backward.
//
//   pm_ln_fwd_kernel     y[b,i,j, q C + c] = LN_{4C}( x[b, 2i + (q & 1), 2j + (q >> 1), c] ) ;  stats[row] = (mean, rstd)   (x in; y out)
//   pm_ln_bwd_kernel     dx[b, 2i + (q & 1), 2j + (q >> 1), c] = LN'(gy)[b,i,j, q C + c] ;  per-channel sums      (gy, x in; dx out)
//   pm_ln_colsum_kernel  dgamma, dbeta from the workgroups' partial sums
//
// x [B][H][W][C] NHWC, Ho = ceil(H / 2), Wo = ceil(W / 2), rows = B Ho Wo.  A token outside the grid (odd H or W) reads as zeros and
// enters the statistics and the channel sums as zeros — the reference zero-pads before it gathers — and its gradient is dropped.  The
// gathered, un-normalised row is never written.  Every token belongs to exactly one output row: each element of dx has one writer,
// no zero-fill, no atomics.
//
// Row ownership: C / 8 lanes per row (lpr = 1 .. 64, a power of two), each lane holding FOUR 8-element pieces, one per quadrant: piece q
// of lane li is channels li * 8 .. + 7 of quadrant q, position q C + li * 8 of the row.  At C = 512 a row is one wave with 32 row
// registers per lane; narrower rows share a wave.  Inputs float32 or bfloat16, every statistic and sum float32 (mean first, then the
// centred squares, as fused_norm.hip / residual_ln_bwd.hip), every output rounded once.
//
// Channel sums without atomics, residual_ln_bwd.hip's scheme: a workgroup (256 threads = 256 / lpr rows per tile) walks tiles
// blockIdx.x, blockIdx.x + gridDim.x, ... (at most PM_MAX_BLOCKS workgroups), each lane adding its rows' terms to its own channels in
// registers in that order; at the end the lanes that hold the same channels are added through LDS in thread order and the workgroup
// writes ONE [2][4C] float32 partial.  pm_ln_colsum_kernel adds the partials in a fixed order (PM_SLICES contiguous index ranges in
// index order, then the range sums in order) and rounds once: the gradients are bitwise reproducible.
#include <hip/hip_bf16.h>
#include "ppn_device.h"
#include "ppn_kernels.h"
#include "norm_vec.h"

namespace ppn {

constexpr int PM_THREADS = 256;        // work-items per workgroup of every kernel of this file
constexpr int PM_MAX_BLOCKS = 1024;    // 4 workgroups per CU of the 256; the partials stay small (1024 x 2 x 4C floats: 16 MB at C = 512)
constexpr int PM_SLICES = 32;          // index ranges of the partials summed side by side in pm_ln_colsum_kernel

int patch_merge_ln_rows(int C) {       // rows per workgroup tile; 0 = a width the kernels do not take
    if (C < 8 || C > 512 || (C & 7) != 0) return 0;
    const int lpr = C / 8;
    return (lpr & (lpr - 1)) == 0 ? PM_THREADS / lpr : 0;
}
int patch_merge_ln_max_blocks() { return PM_MAX_BLOCKS; }

namespace {

unsigned pm_tiles(long long rows, int rpt) { return (unsigned)((rows + rpt - 1) / rpt); }
unsigned pm_blocks(long long rows, int rpt) { const unsigned t = pm_tiles(rows, rpt); return t < (unsigned)PM_MAX_BLOCKS ? t : (unsigned)PM_MAX_BLOCKS; }

// the grid of one call; (b, i, j) of an output row and the token behind each of its quadrants
struct PmGrid {
    uint32_t H, W, Ho, Wo, C;
    __device__ __forceinline__ void place(uint32_t row, uint32_t& b, uint32_t& h0, uint32_t& w0) const {
        const uint32_t per = Ho * Wo;
        b = row / per;
        const uint32_t r = row - b * per, i = r / Wo;
        h0 = 2u * i; w0 = 2u * (r - i * Wo);
    }
    __device__ __forceinline__ bool inside(uint32_t h0, uint32_t w0, int q) const { return h0 + (uint32_t)(q & 1) < H && w0 + (uint32_t)(q >> 1) < W; }
    __device__ __forceinline__ size_t token(uint32_t b, uint32_t h0, uint32_t w0, int q) const {
        return (((size_t)b * H + h0 + (uint32_t)(q & 1)) * W + w0 + (uint32_t)(q >> 1)) * C;
    }
};

}  // namespace

template <typename T>
__global__ __launch_bounds__(PM_THREADS) void pm_ln_fwd_kernel(const T* __restrict__ x, const T* __restrict__ gamma, const T* __restrict__ beta,
                                                               T* __restrict__ y, float* __restrict__ stats, PmGrid g, uint32_t rows, int lpr,
                                                               float eps, uint32_t ntiles) {
    const int li = (int)threadIdx.x & (lpr - 1);
    const uint32_t rpt = (uint32_t)PM_THREADS / (uint32_t)lpr, rit = threadIdx.x / (uint32_t)lpr;
    const uint32_t C = g.C;
    const float inv_n = 1.0f / (float)(4u * C);                              // 4C is a power of two: exact
    // per-channel vectors are the same for every row: loaded once, every tile of the workgroup reuses them
    float wv[4][8], bv[4][8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        Vec8<T>::load(gamma + (size_t)q * C + li * 8, wv[q]);
        Vec8<T>::load(beta + (size_t)q * C + li * 8, bv[q]);
    }
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t row = tile * rpt + rit;
        const bool live = row < rows;                                        // dead lanes still join the shuffles
        uint32_t b = 0, h0 = 0, w0 = 0;
        if (live) g.place(row, b, h0, w0);
        float v[4][8];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (live && g.inside(h0, w0, q)) {
                Vec8<T>::load(x + g.token(b, h0, w0, q) + li * 8, v[q]);
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) v[q][k] = 0.0f;
            }
        }
        // a lane's 32 values are summed piece by piece (chains of 8, then 4), and 1 / sqrt is the correctly rounded pair, not the
        // reciprocal-square-root approximation: rstd scales every value of the row, here and in the backward, so its error is the
        // one that does not average out
        float s = 0.0f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float sp = 0.0f;
#pragma unroll
            for (int k = 0; k < 8; ++k) sp += v[q][k];
            s += sp;
        }
        const float mean = group_sum(s, lpr) * inv_n;
        float sq = 0.0f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float sp = 0.0f;
#pragma unroll
            for (int k = 0; k < 8; ++k) { const float d = v[q][k] - mean; sp = fmaf(d, d, sp); }
            sq += sp;
        }
        const float rstd = 1.0f / sqrtf(group_sum(sq, lpr) * inv_n + eps);
        if (!live) continue;
        if (stats && li == 0) { stats[2 * (size_t)row] = mean; stats[2 * (size_t)row + 1] = rstd; }
        const size_t at = (size_t)row * 4u * C;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = fmaf((v[q][k] - mean) * rstd, wv[q][k], bv[q][k]);
            Vec8<T>::store(y + at + (size_t)q * C + li * 8, o);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(PM_THREADS) void pm_ln_bwd_kernel(const T* __restrict__ gy, const T* __restrict__ x, const float* __restrict__ stats,
                                                               const T* __restrict__ gamma, T* __restrict__ dx, float* __restrict__ partial,
                                                               PmGrid g, uint32_t rows, int lpr, uint32_t ntiles) {
    __shared__ __align__(16) float red[PM_THREADS * 32];
    const int li = (int)threadIdx.x & (lpr - 1);
    const uint32_t rpt = (uint32_t)PM_THREADS / (uint32_t)lpr, rit = threadIdx.x / (uint32_t)lpr;
    const uint32_t C = g.C;
    const float inv_n = 1.0f / (float)(4u * C);
    float acc_w[4][8], acc_b[4][8], wv[4][8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int k = 0; k < 8; ++k) { acc_w[q][k] = 0.0f; acc_b[q][k] = 0.0f; }
        Vec8<T>::load(gamma + (size_t)q * C + li * 8, wv[q]);
    }
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t row = tile * rpt + rit;
        const bool live = row < rows;                                        // dead lanes carry zeros through the shuffles
        uint32_t b = 0, h0 = 0, w0 = 0;
        float mean = 0.0f, rstd = 0.0f;
        if (live) { g.place(row, b, h0, w0); mean = stats[2 * (size_t)row]; rstd = stats[2 * (size_t)row + 1]; }
        const size_t at = (size_t)row * 4u * C;
        float xh[4][8], gg[4][8];
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (live) {
                float gyv[8], p1 = 0.0f, p2 = 0.0f;                          // the row sums piece by piece, as in the forward
                if (g.inside(h0, w0, q)) {
                    Vec8<T>::load(x + g.token(b, h0, w0, q) + li * 8, xh[q]);
                } else {                                                     // the padded token: zeros in the row, part of every sum
#pragma unroll
                    for (int k = 0; k < 8; ++k) xh[q][k] = 0.0f;
                }
                Vec8<T>::load(gy + at + (size_t)q * C + li * 8, gyv);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    xh[q][k] = (xh[q][k] - mean) * rstd;
                    acc_w[q][k] = fmaf(gyv[k], xh[q][k], acc_w[q][k]);
                    acc_b[q][k] += gyv[k];
                    gg[q][k] = gyv[k] * wv[q][k];
                    p1 += gg[q][k];
                    p2 = fmaf(gg[q][k], xh[q][k], p2);
                }
                s1 += p1; s2 += p2;
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) { xh[q][k] = 0.0f; gg[q][k] = 0.0f; }
            }
        }
        const float m1 = group_sum(s1, lpr) * inv_n, m2 = group_sum(s2, lpr) * inv_n;
        if (!live) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!g.inside(h0, w0, q)) continue;                              // the gradient of a padded position is dropped
            float o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = rstd * (gg[q][k] - m1 - xh[q][k] * m2);
            Vec8<T>::store(dx + g.token(b, h0, w0, q) + li * 8, o);
        }
    }
    if (!partial) return;                                                    // neither dgamma nor dbeta wanted (uniform over the grid)
    // the workgroup's partial: for each of the two sums, every lane's registers to LDS, then thread c adds column c's
    // 256 / lpr holders in thread order
    const int groups = PM_THREADS / lpr, C4 = 4 * (int)C;
    float* out = partial + (size_t)blockIdx.x * 2 * C4;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        float (&acc)[4][8] = t == 0 ? acc_w : acc_b;
#pragma unroll
        for (int q = 0; q < 4; ++q) Vec8<float>::store(red + (size_t)threadIdx.x * 32 + q * 8, acc[q]);
        __syncthreads();
        for (int c = (int)threadIdx.x; c < C4; c += PM_THREADS) {
            const int piece = c >> 3, q = piece / lpr, l = piece & (lpr - 1);
            float s = 0.0f;
            for (int gi = 0; gi < groups; ++gi) s += red[(gi * lpr + l) * 32 + q * 8 + (c & 7)];
            out[t * C4 + c] = s;
        }
        __syncthreads();
    }
}

namespace {
template <typename T> __device__ __forceinline__ void pm_store_one(T* p, float v);
template <> __device__ __forceinline__ void pm_store_one<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void pm_store_one<__hip_bfloat16>(__hip_bfloat16* p, float v) { *p = __float2bfloat16(v); }
}  // namespace

// dgamma / dbeta [4C] of dtype T from `nparts` partials [nparts][2][4C]: 8 columns x PM_SLICES index ranges per workgroup; a NULL
// output is skipped.
template <typename T>
__global__ __launch_bounds__(PM_THREADS) void pm_ln_colsum_kernel(const float* __restrict__ partial, int nparts, int C4, T* __restrict__ dgamma,
                                                                  T* __restrict__ dbeta) {
    __shared__ float red[PM_SLICES][8];
    const int cl = (int)threadIdx.x & 7, slice = (int)threadIdx.x >> 3;
    const int col = (int)blockIdx.x * 8 + cl;                                 // 2 x 4C columns, a multiple of 8
    const int per = (nparts + PM_SLICES - 1) / PM_SLICES;
    const int g0 = slice * per, g1 = min(g0 + per, nparts);
    float s = 0.0f;
    for (int gi = g0; gi < g1; ++gi) s += partial[(size_t)gi * 2 * C4 + col];
    red[slice][cl] = s;
    __syncthreads();
    if (slice != 0) return;
    float t = 0.0f;
#pragma unroll
    for (int i = 0; i < PM_SLICES; ++i) t += red[i][cl];
    const int which = col / C4, c = col - which * C4;
    T* dst = which == 0 ? dgamma : dbeta;
    if (dst) pm_store_one<T>(dst + c, t);
}

long long patch_merge_ln_bwd_workspace_bytes(long long rows, int C) {
    const int rpt = patch_merge_ln_rows(C);
    if (rows <= 0 || rows > 0x7fffffffLL || rpt == 0) return -1;
    return (long long)pm_blocks(rows, rpt) * 2 * 4 * C * (long long)sizeof(float);
}

template <typename T>
static int launch_pm_fwd(const void* x, const void* gamma, const void* beta, void* y, float* stats, int B, int H, int W, int C, float eps,
                         hipStream_t stream) {
    const int rpt = patch_merge_ln_rows(C);
    if (rpt == 0) return -1;
    const PmGrid g{(uint32_t)H, (uint32_t)W, (uint32_t)((H + 1) / 2), (uint32_t)((W + 1) / 2), (uint32_t)C};
    const long long rows = (long long)B * g.Ho * g.Wo;
    hipLaunchKernelGGL((pm_ln_fwd_kernel<T>), dim3(pm_blocks(rows, rpt)), dim3(PM_THREADS), 0, stream, (const T*)x, (const T*)gamma, (const T*)beta,
                       (T*)y, stats, g, (uint32_t)rows, C / 8, eps, pm_tiles(rows, rpt));
    return (int)hipGetLastError();
}

int patch_merge_ln_fwd_launch(const void* x, const void* gamma, const void* beta, void* y, float* stats, int B, int H, int W, int C, float eps,
                              int dtype, hipStream_t stream) {
    return dtype == 0 ? launch_pm_fwd<float>(x, gamma, beta, y, stats, B, H, W, C, eps, stream)
                      : launch_pm_fwd<__hip_bfloat16>(x, gamma, beta, y, stats, B, H, W, C, eps, stream);
}

template <typename T>
static int launch_pm_bwd(const void* gy, const void* x, const float* stats, const void* gamma, float* workspace, void* dx, void* dgamma,
                         void* dbeta, int B, int H, int W, int C, hipStream_t stream) {
    const int rpt = patch_merge_ln_rows(C);
    if (rpt == 0) return -1;
    const PmGrid g{(uint32_t)H, (uint32_t)W, (uint32_t)((H + 1) / 2), (uint32_t)((W + 1) / 2), (uint32_t)C};
    const long long rows = (long long)B * g.Ho * g.Wo;
    const unsigned blocks = pm_blocks(rows, rpt);
    const bool sums = dgamma || dbeta;
    hipLaunchKernelGGL((pm_ln_bwd_kernel<T>), dim3(blocks), dim3(PM_THREADS), 0, stream, (const T*)gy, (const T*)x, stats, (const T*)gamma, (T*)dx,
                       sums ? workspace : nullptr, g, (uint32_t)rows, C / 8, pm_tiles(rows, rpt));
    const int e = (int)hipGetLastError();
    if (e != 0 || !sums) return e;
    hipLaunchKernelGGL((pm_ln_colsum_kernel<T>), dim3((unsigned)(2 * 4 * C / 8)), dim3(PM_THREADS), 0, stream, (const float*)workspace, (int)blocks,
                       4 * C, (T*)dgamma, (T*)dbeta);
    return (int)hipGetLastError();
}

int patch_merge_ln_bwd_launch(const void* gy, const void* x, const float* stats, const void* gamma, float* workspace, void* dx, void* dgamma,
                              void* dbeta, int B, int H, int W, int C, int dtype, hipStream_t stream) {
    return dtype == 0 ? launch_pm_bwd<float>(gy, x, stats, gamma, workspace, dx, dgamma, dbeta, B, H, W, C, stream)
                      : launch_pm_bwd<__hip_bfloat16>(gy, x, stats, gamma, workspace, dx, dgamma, dbeta, B, H, W, C, stream);
}

}  // namespace ppn
