// gennet_tail_train.hip — the training pair of GenNet's tail on gfx950: BatchNorm2d (batch statistics) -> LeakyReLU -> Conv2d(C, 1, 3, 1, 1)
// at full resolution behind the last ConvTranspose2d, forward and backward, without ever writing the BatchNorm's output, the
// activation z or the gradient dz: the mirror image of gennet_stem_train.hip.
//
//   tail_stats_kernel         sum y, sum y^2 per channel and workgroup, float64                                   (y in; partials out)
//   tail_stats_finish_kernel  the partials in a fixed order -> stats [3][C] = (mean, biased var, rstd), float32
//   tail_apply_kernel         out = b_f + sum_c sum_tap w_f[c][tap] z_c(p + tap), z recomputed from y with its halo  (y in; out out)
//   tail_bwd_reduce_kernel    sum g, sum g xhat, sum_q z_c(q) d(q - tap) per channel, sum d, per workgroup         (y, d in; partials out)
//   tail_bwd_finish_kernel    the partials in a fixed order in float64 -> dbeta, dgamma, dW_f, db_f, rounded once
//   tail_bwd_apply_kernel     dy = gamma rstd (g - dbeta / N - xhat dgamma / N)                                    (y, d in; dy out)
//
// xhat = (y - mean) rstd, u = gamma xhat + beta, z = u > 0 ? u : slope u; z is ZERO outside the image (the convolution's padding).  The
// convolution has one output channel, so everything that flows back through it is a 3 x 3 stencil of the one-channel d = dL/d out:
// dz_c(q) = sum_tap w_f[c][tap] d(q - tap), g = dz (u > 0 ? 1 : slope), with d zero outside the image.  Forward and backward form xhat
// and u in tl_preact: one function, explicit FMA, the file is built with -ffp-contract=off — the backward's mask is the forward's.
//
// y, dy [B][C][H][W], out, d [B][1][H][W] float32 or bfloat16; gamma, beta [C], w_f [C][9] (tap 3 dy + dx), b_f [1] float32.  All
// arithmetic is float32 (the statistics and the two finishing steps: float64); bfloat16 is only the widening of y and d on load and the
// rounding of out and dy on store.
//
// Work split, as in the stem's file: pixels are numbered n = (b H + h) W + w over the batch — the index into out and d; a work-item owns
// TL_PPT = 4 consecutive ones, a workgroup TL_TILE = 1024.  Four pixels of one row share a 3 x 6 window (of y per channel forward, of d
// backward) which comes from L1 / L2 (an aligned vector and two single values per row when W is a multiple of 4); a work-item whose
// four pixels cross a row end takes 3 x 3 patches pixel by pixel.  When H W is a multiple of 4 the four pixels of a channel plane are
// one aligned vector of y and dy.  The apply kernel walks all C channels (one output channel: nothing to split); the others split
// channels over blockIdx.y — TL_STAT_CH = TL_BWD_CH = 4, TL_DY_CH = 8.  The summing
// kernels walk tiles blockIdx.x, + gridDim.x, ... with at most TL_MAX_BLOCKS workgroups in x; each work-item adds in its own registers
// in that order, a wave by shuffles, the four waves through LDS in wave order, and the workgroup writes ONE partial.  The finishing
// kernels add the partials in index order in float64.  One writer per output element, no atomics: two calls give the same bits.
#include <hip/hip_bf16.h>
#include "ppn_device.h"
#include "ppn_kernels.h"

namespace ppn {

constexpr int TL_THREADS = 256;        // work-items per workgroup of every kernel of this file
constexpr int TL_PPT = 4;              // consecutive pixels per work-item: the line unit of the vector loads and stores
constexpr int TL_TILE = 1024;          // pixels per workgroup tile (TL_THREADS * TL_PPT)
constexpr int TL_MAX_BLOCKS = 512;     // workgroups in x of the summing kernels: past that many tiles a workgroup strides
constexpr int TL_SUMS = 11;            // per channel: sum g, sum g xhat, sum z d(. - tap) for 9 taps
constexpr int TL_STAT_CH = 4;          // channels per work-item of the statistics kernel
constexpr int TL_BWD_CH = 4;           // channels per work-item of the reduce kernel (4 x 11 running sums)
constexpr int TL_DY_CH = 8;            // channels per work-item of the backward's apply kernel
constexpr int TL_MAX_CH = 32;          // the widest channel count (coefficients of all channels in LDS forward)
constexpr int TL_SLICES = 16;          // index ranges of the partials summed side by side in the backward's finishing kernel
constexpr int TL_COEF = 16;            // floats per channel in LDS: w_f[9], mean, rstd, gamma, beta, dbeta / N, dgamma / N, gamma rstd

int gennet_tail_channels_ok(int C) { return C == 8 || C == 16 || C == 24 || C == 32; }
int gennet_tail_tile() { return TL_TILE; }
int gennet_tail_max_blocks() { return TL_MAX_BLOCKS; }

namespace {

unsigned tl_tiles(long long n) { return (unsigned)((n + TL_TILE - 1) / TL_TILE); }
unsigned tl_blocks(long long n) { const unsigned t = tl_tiles(n); return t < (unsigned)TL_MAX_BLOCKS ? t : (unsigned)TL_MAX_BLOCKS; }

struct TlGrid { uint32_t H, W, HW, N; };                                     // N = B H W; B C H W < 2^31

template <typename T> struct TlIO;
template <> struct TlIO<float> {
    static __device__ __forceinline__ void store4(float* p, const float (&v)[4]) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
    static __device__ __forceinline__ void store1(float* p, float v) { *p = v; }
    static __device__ __forceinline__ void load4(const float* p, float (&v)[4]) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
    static __device__ __forceinline__ float load1(const float* p) { return *p; }
};
template <> struct TlIO<__hip_bfloat16> {
    static __device__ __forceinline__ void store4(__hip_bfloat16* p, const float (&v)[4]) {
        *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
    }
    static __device__ __forceinline__ void store1(__hip_bfloat16* p, float v) { *p = __float2bfloat16(v); }
    static __device__ __forceinline__ void load4(const __hip_bfloat16* p, float (&v)[4]) {
        const uint2 t = *reinterpret_cast<const uint2*>(p);
        v[0] = __uint_as_float(t.x << 16); v[1] = __uint_as_float(t.x & 0xffff0000u);
        v[2] = __uint_as_float(t.y << 16); v[3] = __uint_as_float(t.y & 0xffff0000u);
    }
    static __device__ __forceinline__ float load1(const __hip_bfloat16* p) { return __bfloat162float(*p); }
};

// Where the pixels n0 .. n0 + 3 of a work-item lie.  row: all four in one image row (then b[0], h[0], w[0] place the first and the
// others follow it); otherwise each has its own image, row and column, and a pixel at or past N is not live.
struct TlPix {
    uint32_t b[TL_PPT], h[TL_PPT], w[TL_PPT];
    bool live[TL_PPT], row;
};

__device__ __forceinline__ void tl_place(const TlGrid& g, uint32_t n0, TlPix& px) {
#pragma unroll
    for (int k = 0; k < TL_PPT; ++k) {
        const uint32_t n = n0 + k;
        px.live[k] = n < g.N;
        const uint32_t b = px.live[k] ? n / g.HW : 0u, q = px.live[k] ? n - b * g.HW : 0u;
        px.b[k] = b; px.h[k] = q / g.W; px.w[k] = q - px.h[k] * g.W;
    }
    px.row = px.live[TL_PPT - 1] && px.w[0] + (TL_PPT - 1) < g.W;             // n0 + 3 < N and no row end inside: one row of one image
}

// The 3 x 6 window around four pixels of one row of the plane `img` (H x W): win[r][j] = img(h + r - 1, w + j - 1), 0 outside the plane.
// When W is a multiple of 4 (then w is one too, and so is the plane's offset) the middle four of a row are one aligned vector.
template <typename T>
__device__ __forceinline__ void tl_window(const T* __restrict__ img, const TlGrid& g, uint32_t h, uint32_t w, float (&win)[3][TL_PPT + 2]) {
    if ((g.W & (TL_PPT - 1)) == 0) {                                         // uniform
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int hh = (int)h + r - 1;
            const bool row = hh >= 0 && hh < (int)g.H;
            const T* line = img + (size_t)(row ? hh : 0) * g.W + w;
            float mid[TL_PPT] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (row) TlIO<T>::load4(line, mid);
#pragma unroll
            for (int j = 0; j < TL_PPT; ++j) win[r][1 + j] = mid[j];
            win[r][0] = (row && w > 0) ? TlIO<T>::load1(line - 1) : 0.0f;
            win[r][TL_PPT + 1] = (row && w + TL_PPT < g.W) ? TlIO<T>::load1(line + TL_PPT) : 0.0f;
        }
        return;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int hh = (int)h + r - 1;
        const bool row = hh >= 0 && hh < (int)g.H;
#pragma unroll
        for (int j = 0; j < TL_PPT + 2; ++j) {
            const int ww = (int)w + j - 1;
            win[r][j] = (row && ww >= 0 && ww < (int)g.W) ? TlIO<T>::load1(img + (size_t)hh * g.W + ww) : 0.0f;
        }
    }
}

// The 3 x 3 patch around one pixel of the plane `img`: p[3 r + j] = img(h + r - 1, w + j - 1), 0 outside the plane or when not live.
template <typename T>
__device__ __forceinline__ void tl_patch(const T* __restrict__ img, const TlGrid& g, uint32_t h, uint32_t w, bool live, float (&p)[9]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int hh = (int)h + r - 1, ww = (int)w + j - 1;
            p[3 * r + j] = (live && hh >= 0 && hh < (int)g.H && ww >= 0 && ww < (int)g.W) ? TlIO<T>::load1(img + (size_t)hh * g.W + ww) : 0.0f;
        }
}

// The patches of the one-channel d around the four pixels: p[k][3 r + j] = d(h_k + r - 1, w_k + j - 1), zero outside the pixel's image.
template <typename T>
__device__ __forceinline__ void tl_d_patches(const T* __restrict__ d, const TlGrid& g, const TlPix& px, float (&p)[TL_PPT][9]) {
    if (px.row) {
        float win[3][TL_PPT + 2];
        tl_window<T>(d + (size_t)px.b[0] * g.HW, g, px.h[0], px.w[0], win);
#pragma unroll
        for (int k = 0; k < TL_PPT; ++k)
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int j = 0; j < 3; ++j) p[k][3 * r + j] = win[r][k + j];
        return;
    }
#pragma unroll
    for (int k = 0; k < TL_PPT; ++k) tl_patch<T>(d + (size_t)px.b[k] * g.HW, g, px.h[k], px.w[k], px.live[k], p[k]);
}

// The four values of channel plane c at the work-item's pixels (a pixel that is not live: 0).  vec: H W is a multiple of 4, so the
// four lie in one plane, aligned, and n0 + 3 < N.
template <typename T>
__device__ __forceinline__ void tl_load_line(const T* __restrict__ y, const TlGrid& g, const TlPix& px, int C, int c, bool vec, float (&v)[TL_PPT]) {
    if (vec) {
        TlIO<T>::load4(y + ((size_t)px.b[0] * C + c) * g.HW + (size_t)px.h[0] * g.W + px.w[0], v);
        return;
    }
#pragma unroll
    for (int k = 0; k < TL_PPT; ++k)
        v[k] = px.live[k] ? TlIO<T>::load1(y + ((size_t)px.b[k] * C + c) * g.HW + (size_t)px.h[k] * g.W + px.w[k]) : 0.0f;
}

// xhat and the pre-activation u of one value of y from its channel's coefficients: forward and backward call this one function
// (explicit FMA, no contraction), so u > 0 decides alike in both.
__device__ __forceinline__ void tl_preact(float y, const float (&cf)[TL_COEF], float& xh, float& u) {
    xh = (y - cf[9]) * cf[10];
    u = fmaf(cf[11], xh, cf[12]);
}

__device__ __forceinline__ float tl_act(float y, const float (&cf)[TL_COEF], float slope) {
    float xh, u;
    tl_preact(y, cf, xh, u);
    return u > 0.0f ? u : u * slope;
}

// the coefficients of channels c0 .. c0 + n - 1 into LDS (work-item t < n loads channel c0 + t); dgamma, dbeta: NULL forward
__device__ __forceinline__ void tl_load_coef(float (*coef)[TL_COEF], int c0, int n, int C, const float* __restrict__ wf, const float* __restrict__ gamma,
                                             const float* __restrict__ beta, const float* __restrict__ stats, const float* __restrict__ dgamma,
                                             const float* __restrict__ dbeta, double count) {
    const int t = (int)threadIdx.x;
    if (t < n) {
        const int c = c0 + t;
#pragma unroll
        for (int j = 0; j < 9; ++j) coef[t][j] = wf[c * 9 + j];
        coef[t][9] = stats[c];
        coef[t][10] = stats[2 * C + c];
        coef[t][11] = gamma[c];
        coef[t][12] = beta[c];
        coef[t][13] = dbeta ? (float)((double)dbeta[c] / count) : 0.0f;
        coef[t][14] = dgamma ? (float)((double)dgamma[c] / count) : 0.0f;
        coef[t][15] = gamma[c] * stats[2 * C + c];
    }
    __syncthreads();
}

__device__ __forceinline__ void tl_coef(const float (*coef)[TL_COEF], int ci, float (&cf)[TL_COEF]) {
    const float4* s = reinterpret_cast<const float4*>(coef[ci]);
#pragma unroll
    for (int i = 0; i < TL_COEF / 4; ++i) { const float4 v = s[i]; cf[4 * i] = v.x; cf[4 * i + 1] = v.y; cf[4 * i + 2] = v.z; cf[4 * i + 3] = v.w; }
}

__device__ __forceinline__ float tl_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;                                                                // valid in lane 0
}

}  // namespace

// partial [gridDim.x][C][2] float64: sum y and sum y^2 of the tiles this workgroup walked, channels c0 .. c0 + 3
template <typename T>
__global__ __launch_bounds__(TL_THREADS) void tail_stats_kernel(const T* __restrict__ y, double* __restrict__ partial, TlGrid g, int C, uint32_t ntiles) {
    __shared__ double red[TL_THREADS / 64][TL_STAT_CH * 2];
    const int c0 = (int)blockIdx.y * TL_STAT_CH;
    const bool vec = (g.HW & (TL_PPT - 1)) == 0;
    double acc[TL_STAT_CH][2];
#pragma unroll
    for (int ci = 0; ci < TL_STAT_CH; ++ci) acc[ci][0] = acc[ci][1] = 0.0;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t n0 = tile * (uint32_t)TL_TILE + threadIdx.x * (uint32_t)TL_PPT;
        if (n0 >= g.N) continue;
        TlPix px;
        tl_place(g, n0, px);
#pragma unroll
        for (int ci = 0; ci < TL_STAT_CH; ++ci) {
            float v[TL_PPT];
            tl_load_line<T>(y, g, px, C, c0 + ci, vec, v);                   // a pixel past N is 0: it adds nothing
#pragma unroll
            for (int k = 0; k < TL_PPT; ++k) {
                const double d = (double)v[k];
                acc[ci][0] += d;
                acc[ci][1] = fma(d, d, acc[ci][1]);
            }
        }
    }
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
#pragma unroll
    for (int ci = 0; ci < TL_STAT_CH; ++ci)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const double v = wave_sum(acc[ci][j]);
            if (lane == 0) red[wave][ci * 2 + j] = v;
        }
    __syncthreads();
    if (threadIdx.x < TL_STAT_CH * 2) {
        double s = red[0][threadIdx.x];
#pragma unroll
        for (int wv = 1; wv < TL_THREADS / 64; ++wv) s += red[wv][threadIdx.x];
        partial[((size_t)blockIdx.x * C + c0) * 2 + threadIdx.x] = s;
    }
}

// One workgroup: the 2 C sums = the partials added in 4 contiguous index ranges in index order, then the range sums in order; then
// channel c's mean, biased variance and rstd in float64, rounded once.
__global__ __launch_bounds__(TL_THREADS) void tail_stats_finish_kernel(const double* __restrict__ partial, int nparts, int C, double count, float eps,
                                                                       float* __restrict__ stats) {
    __shared__ double red[TL_THREADS / 64][64];
    __shared__ double tot[64];
    const int col = (int)threadIdx.x & 63, slice = (int)threadIdx.x >> 6;      // 4 ranges x 64 columns (2 C live)
    const int per = (nparts + TL_THREADS / 64 - 1) / (TL_THREADS / 64);
    const int g0 = slice * per, g1 = min(g0 + per, nparts);
    double s = 0.0;
    if (col < 2 * C)
#pragma unroll 8
        for (int gi = g0; gi < g1; ++gi) s += partial[(size_t)gi * C * 2 + col];
    red[slice][col] = s;
    __syncthreads();
    if (threadIdx.x < 64) {
        double t = red[0][threadIdx.x];
#pragma unroll
        for (int i = 1; i < TL_THREADS / 64; ++i) t += red[i][threadIdx.x];
        tot[threadIdx.x] = t;
    }
    __syncthreads();
    const int c = (int)threadIdx.x;
    if (c >= C) return;
    const double mean = tot[2 * c] / count;
    double var = tot[2 * c + 1] / count - mean * mean;
    if (var < 0.0) var = 0.0;                                                // a nearly constant plane: rounding may leave -1e-17
    stats[c] = (float)mean;
    stats[C + c] = (float)var;
    stats[2 * C + c] = (float)(1.0 / sqrt(var + (double)eps));
}

template <typename T>
__global__ __launch_bounds__(TL_THREADS) void tail_apply_kernel(const T* __restrict__ y, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                const float* __restrict__ wf, const float* __restrict__ bf,
                                                                const float* __restrict__ stats, T* __restrict__ out, TlGrid g, int C, float slope) {
    __shared__ __align__(16) float coef[TL_MAX_CH][TL_COEF];
    tl_load_coef(coef, 0, C, C, wf, gamma, beta, stats, nullptr, nullptr, 1.0);
    const uint32_t n0 = blockIdx.x * (uint32_t)TL_TILE + threadIdx.x * (uint32_t)TL_PPT;
    if (n0 >= g.N) return;
    TlPix px;
    tl_place(g, n0, px);
    const float b0 = bf ? bf[0] : 0.0f;
    float o[TL_PPT];
#pragma unroll
    for (int k = 0; k < TL_PPT; ++k) o[k] = b0;
    if (px.row) {
        const uint32_t h = px.h[0], w = px.w[0];
        bool in[3][TL_PPT + 2];                                              // z is zero outside the image, not leaky(beta)
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int j = 0; j < TL_PPT + 2; ++j) {
                const int hh = (int)h + r - 1, ww = (int)w + j - 1;
                in[r][j] = hh >= 0 && hh < (int)g.H && ww >= 0 && ww < (int)g.W;
            }
#pragma unroll 2
        for (int c = 0; c < C; ++c) {
            float cf[TL_COEF], win[3][TL_PPT + 2];
            tl_coef(coef, c, cf);
            tl_window<T>(y + ((size_t)px.b[0] * C + c) * g.HW, g, h, w, win);
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int j = 0; j < TL_PPT + 2; ++j) win[r][j] = in[r][j] ? tl_act(win[r][j], cf, slope) : 0.0f;
#pragma unroll
            for (int k = 0; k < TL_PPT; ++k)
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int j = 0; j < 3; ++j) o[k] = fmaf(cf[3 * r + j], win[r][k + j], o[k]);
        }
        TlIO<T>::store4(out + n0, o);                                        // out has one channel: pixel n is element n
        return;
    }
#pragma unroll
    for (int k = 0; k < TL_PPT; ++k) {
        if (!px.live[k]) continue;
        const uint32_t h = px.h[k], w = px.w[k];
        for (int c = 0; c < C; ++c) {
            float cf[TL_COEF], p[9];
            tl_coef(coef, c, cf);
            tl_patch<T>(y + ((size_t)px.b[k] * C + c) * g.HW, g, h, w, true, p);
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int hh = (int)h + r - 1, ww = (int)w + j - 1;
                    const bool in = hh >= 0 && hh < (int)g.H && ww >= 0 && ww < (int)g.W;
                    o[k] = fmaf(cf[3 * r + j], in ? tl_act(p[3 * r + j], cf, slope) : 0.0f, o[k]);
                }
        }
        TlIO<T>::store1(out + n0 + k, o[k]);
    }
}

// partial: [gridDim.x][C][11] float32, then [gridDim.x] float32 (sum d, written by the workgroups of channel group 0)
template <typename T>
__global__ __launch_bounds__(TL_THREADS) void tail_bwd_reduce_kernel(const T* __restrict__ d, const T* __restrict__ y, const float* __restrict__ gamma,
                                                                     const float* __restrict__ beta, const float* __restrict__ wf,
                                                                     const float* __restrict__ stats, float* __restrict__ partial, TlGrid g, int C,
                                                                     float slope, uint32_t ntiles) {
    __shared__ __align__(16) float coef[TL_BWD_CH][TL_COEF];
    __shared__ float red[TL_THREADS / 64][TL_BWD_CH * TL_SUMS + 1];
    const int c0 = (int)blockIdx.y * TL_BWD_CH;
    tl_load_coef(coef, c0, TL_BWD_CH, C, wf, gamma, beta, stats, nullptr, nullptr, 1.0);
    const bool hw4 = (g.HW & (TL_PPT - 1)) == 0;
    float acc[TL_BWD_CH][TL_SUMS], sd = 0.0f;
#pragma unroll
    for (int ci = 0; ci < TL_BWD_CH; ++ci)
#pragma unroll
        for (int j = 0; j < TL_SUMS; ++j) acc[ci][j] = 0.0f;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t n0 = tile * (uint32_t)TL_TILE + threadIdx.x * (uint32_t)TL_PPT;
        if (n0 >= g.N) continue;
        TlPix px;
        tl_place(g, n0, px);
        float p[TL_PPT][9];                                                  // p[k][t] = d(q_k + tap t): d(q_k - tap t) is p[k][8 - t]
        tl_d_patches<T>(d, g, px, p);
#pragma unroll
        for (int k = 0; k < TL_PPT; ++k) sd += p[k][4];                      // a pixel past N: 0
#pragma unroll
        for (int ci = 0; ci < TL_BWD_CH; ++ci) {
            float cf[TL_COEF], v[TL_PPT];
            tl_coef(coef, ci, cf);
            tl_load_line<T>(y, g, px, C, c0 + ci, hw4, v);
#pragma unroll
            for (int k = 0; k < TL_PPT; ++k) {
                float xh, u;
                tl_preact(v[k], cf, xh, u);
                const float z = u > 0.0f ? u : u * slope;
                float dz = cf[0] * p[k][8];
#pragma unroll
                for (int t = 1; t < 9; ++t) dz = fmaf(cf[t], p[k][8 - t], dz);
                const float gk = u > 0.0f ? dz : dz * slope;
                acc[ci][0] += gk;
                acc[ci][1] = fmaf(gk, xh, acc[ci][1]);
#pragma unroll
                for (int t = 0; t < 9; ++t) acc[ci][2 + t] = fmaf(z, p[k][8 - t], acc[ci][2 + t]);   // a pixel past N: its patch is 0
            }
        }
    }
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
#pragma unroll
    for (int ci = 0; ci < TL_BWD_CH; ++ci)
#pragma unroll
        for (int j = 0; j < TL_SUMS; ++j) {
            const float v = tl_wave_sum(acc[ci][j]);
            if (lane == 0) red[wave][ci * TL_SUMS + j] = v;
        }
    {
        const float v = tl_wave_sum(sd);
        if (lane == 0) red[wave][TL_BWD_CH * TL_SUMS] = v;
    }
    __syncthreads();
    if (threadIdx.x < TL_BWD_CH * TL_SUMS + 1) {
        float s = red[0][threadIdx.x];
#pragma unroll
        for (int wv = 1; wv < TL_THREADS / 64; ++wv) s += red[wv][threadIdx.x];
        if (threadIdx.x < TL_BWD_CH * TL_SUMS) {
            const int ci = (int)threadIdx.x / TL_SUMS, j = (int)threadIdx.x - ci * TL_SUMS;
            partial[((size_t)blockIdx.x * C + c0 + ci) * TL_SUMS + j] = s;
        } else if (blockIdx.y == 0) {
            partial[(size_t)gridDim.x * C * TL_SUMS + blockIdx.x] = s;
        }
    }
}

// Workgroup c < C: channel c's 11 sums from the partials (TL_SLICES contiguous index ranges in index order, then the range sums in
// order, float64), rounded once into dbeta, dgamma and dW_f.  Workgroup C (launched when db_f is wanted): sum d in column 0.
__global__ __launch_bounds__(TL_THREADS) void tail_bwd_finish_kernel(const float* __restrict__ partial, int nparts, int C, float* __restrict__ dgamma,
                                                                     float* __restrict__ dbeta, float* __restrict__ dwf, float* __restrict__ dbf) {
    __shared__ double red[TL_SLICES][16];
    const int c = (int)blockIdx.x;
    const int col = (int)threadIdx.x & 15, slice = (int)threadIdx.x >> 4;
    const int per = (nparts + TL_SLICES - 1) / TL_SLICES;
    const int g0 = slice * per, g1 = min(g0 + per, nparts);
    const float* sums_d = partial + (size_t)nparts * C * TL_SUMS;
    double s = 0.0;
    if (c < C) {
        if (col < TL_SUMS)
#pragma unroll 8
            for (int gi = g0; gi < g1; ++gi) s += (double)partial[((size_t)gi * C + c) * TL_SUMS + col];
    } else if (col == 0) {
#pragma unroll 8
        for (int gi = g0; gi < g1; ++gi) s += (double)sums_d[gi];
    }
    red[slice][col] = s;
    __syncthreads();
    const int t = (int)threadIdx.x;
    if (t >= TL_SUMS) return;
    double tot = red[0][t];
#pragma unroll
    for (int i = 1; i < TL_SLICES; ++i) tot += red[i][t];
    if (c >= C) { if (t == 0) dbf[0] = (float)tot; return; }
    if (t == 0) dbeta[c] = (float)tot;
    else if (t == 1) dgamma[c] = (float)tot;
    else dwf[c * 9 + (t - 2)] = (float)tot;
}

template <typename T>
__global__ __launch_bounds__(TL_THREADS) void tail_bwd_apply_kernel(const T* __restrict__ d, const T* __restrict__ y, const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, const float* __restrict__ wf,
                                                                    const float* __restrict__ stats, const float* __restrict__ dgamma,
                                                                    const float* __restrict__ dbeta, T* __restrict__ dy, TlGrid g, int C, float slope) {
    __shared__ __align__(16) float coef[TL_DY_CH][TL_COEF];
    const int c0 = (int)blockIdx.y * TL_DY_CH;
    tl_load_coef(coef, c0, TL_DY_CH, C, wf, gamma, beta, stats, dgamma, dbeta, (double)g.N);
    const uint32_t n0 = blockIdx.x * (uint32_t)TL_TILE + threadIdx.x * (uint32_t)TL_PPT;
    if (n0 >= g.N) return;
    const bool hw4 = (g.HW & (TL_PPT - 1)) == 0;
    TlPix px;
    tl_place(g, n0, px);
    float p[TL_PPT][9];
    tl_d_patches<T>(d, g, px, p);
#pragma unroll 2
    for (int ci = 0; ci < TL_DY_CH; ++ci) {
        float cf[TL_COEF], v[TL_PPT], o[TL_PPT];
        tl_coef(coef, ci, cf);
        tl_load_line<T>(y, g, px, C, c0 + ci, hw4, v);
#pragma unroll
        for (int k = 0; k < TL_PPT; ++k) {
            float xh, u;
            tl_preact(v[k], cf, xh, u);
            float dz = cf[0] * p[k][8];
#pragma unroll
            for (int t = 1; t < 9; ++t) dz = fmaf(cf[t], p[k][8 - t], dz);
            const float gk = u > 0.0f ? dz : dz * slope;
            o[k] = cf[15] * ((gk - cf[13]) - xh * cf[14]);
        }
        if (hw4) {
            TlIO<T>::store4(dy + ((size_t)px.b[0] * C + c0 + ci) * g.HW + (size_t)px.h[0] * g.W + px.w[0], o);
        } else {
#pragma unroll
            for (int k = 0; k < TL_PPT; ++k)
                if (px.live[k]) TlIO<T>::store1(dy + ((size_t)px.b[k] * C + c0 + ci) * g.HW + (size_t)px.h[k] * g.W + px.w[k], o[k]);
        }
    }
}

long long gennet_tail_train_workspace_bytes(long long n, int C) {
    if (n < 2 || n > 0x7fffffffLL || !gennet_tail_channels_ok(C)) return -1;
    const long long a = (long long)C * 2 * (long long)sizeof(double), b = ((long long)C * TL_SUMS + 1) * (long long)sizeof(float);
    return (a > b ? a : b) * (long long)tl_blocks(n);
}

int gennet_tail_train_fwd_launch(const void* y, const float* gamma, const float* beta, const float* wf, const float* bf, void* out, float* stats,
                                 void* workspace, int B, int H, int W, int C, float eps, float slope, int dtype, hipStream_t stream) {
    if (!gennet_tail_channels_ok(C)) return -1;
    const long long n = (long long)B * H * W;
    const TlGrid g{(uint32_t)H, (uint32_t)W, (uint32_t)(H * W), (uint32_t)n};
    const unsigned blocks = tl_blocks(n), tiles = tl_tiles(n);
    const dim3 sgrid(blocks, (unsigned)(C / TL_STAT_CH));
    if (dtype == 0)
        hipLaunchKernelGGL((tail_stats_kernel<float>), sgrid, dim3(TL_THREADS), 0, stream, (const float*)y, (double*)workspace, g, C, tiles);
    else
        hipLaunchKernelGGL((tail_stats_kernel<__hip_bfloat16>), sgrid, dim3(TL_THREADS), 0, stream, (const __hip_bfloat16*)y, (double*)workspace, g, C,
                           tiles);
    int e = (int)hipGetLastError();
    if (e != 0) return e;
    hipLaunchKernelGGL(tail_stats_finish_kernel, dim3(1), dim3(TL_THREADS), 0, stream, (const double*)workspace, (int)blocks, C, (double)n, eps, stats);
    e = (int)hipGetLastError();
    if (e != 0) return e;
    if (dtype == 0)
        hipLaunchKernelGGL((tail_apply_kernel<float>), dim3(tiles), dim3(TL_THREADS), 0, stream, (const float*)y, gamma, beta, wf, bf,
                           (const float*)stats, (float*)out, g, C, slope);
    else
        hipLaunchKernelGGL((tail_apply_kernel<__hip_bfloat16>), dim3(tiles), dim3(TL_THREADS), 0, stream, (const __hip_bfloat16*)y, gamma, beta, wf, bf,
                           (const float*)stats, (__hip_bfloat16*)out, g, C, slope);
    return (int)hipGetLastError();
}

int gennet_tail_train_bwd_launch(const void* dout, const void* y, const float* gamma, const float* beta, const float* wf, const float* stats,
                                 void* workspace, void* dy, float* dgamma, float* dbeta, float* dwf, float* dbf, int B, int H, int W, int C,
                                 float slope, int dtype, hipStream_t stream) {
    if (!gennet_tail_channels_ok(C)) return -1;
    const long long n = (long long)B * H * W;
    const TlGrid g{(uint32_t)H, (uint32_t)W, (uint32_t)(H * W), (uint32_t)n};
    const unsigned blocks = tl_blocks(n), tiles = tl_tiles(n);
    const dim3 rgrid(blocks, (unsigned)(C / TL_BWD_CH));
    if (dtype == 0)
        hipLaunchKernelGGL((tail_bwd_reduce_kernel<float>), rgrid, dim3(TL_THREADS), 0, stream, (const float*)dout, (const float*)y, gamma, beta, wf,
                           stats, (float*)workspace, g, C, slope, tiles);
    else
        hipLaunchKernelGGL((tail_bwd_reduce_kernel<__hip_bfloat16>), rgrid, dim3(TL_THREADS), 0, stream, (const __hip_bfloat16*)dout,
                           (const __hip_bfloat16*)y, gamma, beta, wf, stats, (float*)workspace, g, C, slope, tiles);
    int e = (int)hipGetLastError();
    if (e != 0) return e;
    hipLaunchKernelGGL(tail_bwd_finish_kernel, dim3((unsigned)C + (dbf ? 1u : 0u)), dim3(TL_THREADS), 0, stream, (const float*)workspace, (int)blocks, C,
                       dgamma, dbeta, dwf, dbf);
    e = (int)hipGetLastError();
    if (e != 0 || !dy) return e;
    const dim3 agrid(tiles, (unsigned)(C / TL_DY_CH));
    if (dtype == 0)
        hipLaunchKernelGGL((tail_bwd_apply_kernel<float>), agrid, dim3(TL_THREADS), 0, stream, (const float*)dout, (const float*)y, gamma, beta, wf, stats,
                           (const float*)dgamma, (const float*)dbeta, (float*)dy, g, C, slope);
    else
        hipLaunchKernelGGL((tail_bwd_apply_kernel<__hip_bfloat16>), agrid, dim3(TL_THREADS), 0, stream, (const __hip_bfloat16*)dout,
                           (const __hip_bfloat16*)y, gamma, beta, wf, stats, (const float*)dgamma, (const float*)dbeta, (__hip_bfloat16*)dy, g, C, slope);
    return (int)hipGetLastError();
}

}  // namespace ppn
