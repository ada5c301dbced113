// gennet_stem_train.hip — the training pair of GenNet's stem on gfx950: Conv2d(1, C, 3, 1, 1) -> BatchNorm2d (batch statistics) ->
// LeakyReLU at full resolution, forward and backward, without ever writing the convolution's output or the BatchNorm's.
//
//   stem_moments_kernel     S1 = sum_n p(n), S2 = sum_n p(n) p(n)^T per workgroup, float64                      (x in; partials out)
//   stem_stats_kernel       the partials in a fixed order -> moments [54] float64, stats [3][C] = (mean, biased var, rstd)
//   stem_apply_kernel       z = leaky_relu(gamma ((conv(x) + b - mean) rstd) + beta), rounded once              (x in; z out)
//   stem_bwd_reduce_kernel  g = dz (u > 0 ? 1 : slope);  sum g, sum g xhat, sum g p_t per channel and workgroup  (dz, x in; partials out)
//   stem_bwd_finish_kernel  the partials in a fixed order, then dW, dgamma, dbeta in float64, rounded once
//
// p(n) is the zero-padded 3 x 3 patch of the one-channel input at pixel n (9 values, tap t = 3 dy + dx).  With m = S1 / N and
// Cov = S2 / N - m m^T the batch statistics of y = conv(x) + b are mean_c = w_c . m + b_c and var_c = w_c^T Cov w_c: one pass over the
// 1-channel input, none over y.  The backward recomputes xhat and u from x (9 FMAs per channel and pixel, st_preact: the SAME function
// as the forward, so the LeakyReLU mask is the forward's bit for bit) and needs one pass over dz:
//   dbeta_c = sum g,  dgamma_c = sum g xhat,  G_c = sum g p,
//   dW_c = gamma_c rstd_c (G_c - (dbeta_c / N) S1 - (dgamma_c / N) X_c),  X_c = sum xhat_c p = rstd_c (S2 w_c + (b_c - mean_c) S1);
// the convolution bias has gradient 0 exactly (the sum of a BatchNorm input gradient).
//
// x [B][H][W] float32; w [C][9], bias, gamma, beta [C] float32; z, dz [B][C][H][W] float32 or bfloat16.  All arithmetic is float32
// from the float32 x and parameters (moments and the two finishing steps: float64); bfloat16 is only the rounding of z on store and
// the widening of dz on load.
//
// Work split: pixels are numbered n = (b H + h) W + w over the whole batch; a work-item owns ST_PPT = 4 consecutive ones, a workgroup
// ST_TILE = 1024.  When H W is a multiple of 4 the four lie in one channel plane, 16-byte aligned (8 for bfloat16), and go out / come
// in as one vector per channel: a wave writes 1 KiB (512 B) of contiguous plane per instruction.  Otherwise element by element.
// Channels are split over blockIdx.y — ST_FWD_CH = 8 per work-item forward, ST_BWD_CH = 4 backward (4 x 11 running sums) — so batch 8
// at 224 x 224 launches 1176 / 2352 workgroups.  The moments and the backward sums walk tiles blockIdx.x, + gridDim.x, ... with at
// most ST_MAX_BLOCKS workgroups in x; each work-item adds in its own registers in that order, a wave by shuffles, the four waves
// through LDS in wave order, and the workgroup writes ONE partial.  The finishing kernels add the partials in index order in float64.
// One writer per output element and a fixed order everywhere: two calls give the same bits.
#include <hip/hip_bf16.h>
#include "ppn_device.h"
#include "ppn_kernels.h"

namespace ppn {

constexpr int ST_THREADS = 256;        // work-items per workgroup of every kernel of this file
constexpr int ST_PPT = 4;              // consecutive pixels per work-item: the line unit of the vector loads and stores
constexpr int ST_TILE = 1024;          // pixels per workgroup tile (ST_THREADS * ST_PPT) of the moments, apply and reduce kernels
constexpr int ST_MAX_BLOCKS = 512;     // workgroups in x of the moments and reduce kernels: past that many tiles a workgroup strides
constexpr int ST_MOMENTS = 54;         // S1 (9) then the lower triangle of S2 (45, index i (i + 1) / 2 + j for j <= i)
constexpr int ST_SUMS = 11;            // per channel: sum g, sum g xhat, sum g p_0 .. p_8
constexpr int ST_FWD_CH = 8;           // channels per work-item of the apply kernel
constexpr int ST_BWD_CH = 4;           // channels per work-item of the reduce kernel
constexpr int ST_SLICES = 16;          // index ranges of the partials summed side by side in the finishing kernels
constexpr int ST_COEF = 16;            // floats per channel in LDS: w[9], b - mean, rstd, gamma, beta, 3 unused

int gennet_stem_channels_ok(int C) { return C == 8 || C == 16 || C == 24 || C == 32; }
int gennet_stem_tile() { return ST_TILE; }
int gennet_stem_max_blocks() { return ST_MAX_BLOCKS; }

namespace {

unsigned st_tiles(long long n) { return (unsigned)((n + ST_TILE - 1) / ST_TILE); }
unsigned st_blocks(long long n) { const unsigned t = st_tiles(n); return t < (unsigned)ST_MAX_BLOCKS ? t : (unsigned)ST_MAX_BLOCKS; }

struct StGrid { uint32_t H, W, HW, N; };                                     // N = B H W < 2^31

// The patches of the pixels n0 .. n0 + 3 (n0 < N); a pixel at or past N gets zeros.  Four pixels of one row share a 3 x 6 window.
// b0, q0: image and in-plane offset of pixel n0.
__device__ __forceinline__ void st_patches(const float* __restrict__ x, const StGrid& g, uint32_t n0, float (&p)[ST_PPT][9], uint32_t& b0, uint32_t& q0) {
    const uint32_t b = n0 / g.HW, q = n0 - b * g.HW, h = q / g.W, w = q - h * g.W;
    b0 = b; q0 = q;
    if (w + (ST_PPT - 1) < g.W) {
        const float* img = x + (size_t)b * g.HW;
        float win[3][ST_PPT + 2];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int hh = (int)h + dy - 1;
            const bool row = hh >= 0 && hh < (int)g.H;
#pragma unroll
            for (int j = 0; j < ST_PPT + 2; ++j) {
                const int ww = (int)w + j - 1;
                win[dy][j] = (row && ww >= 0 && ww < (int)g.W) ? img[(size_t)hh * g.W + ww] : 0.0f;
            }
        }
#pragma unroll
        for (int k = 0; k < ST_PPT; ++k)
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) p[k][dy * 3 + dx] = win[dy][k + dx];
        return;
    }
#pragma unroll
    for (int k = 0; k < ST_PPT; ++k) {
        const uint32_t n = n0 + k;
        const bool live = n < g.N;
        const uint32_t bk = live ? n / g.HW : 0u, qk = live ? n - bk * g.HW : 0u, hk = qk / g.W, wk = qk - hk * g.W;
        const float* img = x + (size_t)bk * g.HW;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int hh = (int)hk + dy - 1, ww = (int)wk + dx - 1;
                p[k][dy * 3 + dx] = (live && hh >= 0 && hh < (int)g.H && ww >= 0 && ww < (int)g.W) ? img[(size_t)hh * g.W + ww] : 0.0f;
            }
    }
}

// xhat and the pre-activation u of one pixel and channel from its patch and the channel's coefficients: forward and backward call
// this one function (explicit FMAs, the file is built with -ffp-contract=off), so u > 0 decides alike in both.
__device__ __forceinline__ void st_preact(const float (&p)[9], const float (&cf)[ST_COEF], float& xh, float& u) {
    float y = cf[0] * p[0];
#pragma unroll
    for (int t = 1; t < 9; ++t) y = fmaf(cf[t], p[t], y);
    xh = (y + cf[9]) * cf[10];
    u = fmaf(cf[11], xh, cf[12]);
}

// the coefficients of channels c0 .. c0 + n - 1 into LDS (work-item t < n loads channel c0 + t)
__device__ __forceinline__ void st_load_coef(float (*coef)[ST_COEF], int c0, int n, int C, const float* __restrict__ w, const float* __restrict__ bias,
                                             const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ stats) {
    const int t = (int)threadIdx.x;
    if (t < n) {
        const int c = c0 + t;
#pragma unroll
        for (int j = 0; j < 9; ++j) coef[t][j] = w[c * 9 + j];
        coef[t][9] = (bias ? bias[c] : 0.0f) - stats[c];
        coef[t][10] = stats[2 * C + c];
        coef[t][11] = gamma[c];
        coef[t][12] = beta[c];
        coef[t][13] = coef[t][14] = coef[t][15] = 0.0f;
    }
    __syncthreads();
}

__device__ __forceinline__ void st_coef(const float (*coef)[ST_COEF], int ci, float (&cf)[ST_COEF]) {
    const float4* s = reinterpret_cast<const float4*>(coef[ci]);
#pragma unroll
    for (int i = 0; i < ST_COEF / 4; ++i) { const float4 v = s[i]; cf[4 * i] = v.x; cf[4 * i + 1] = v.y; cf[4 * i + 2] = v.z; cf[4 * i + 3] = v.w; }
}

template <typename T> struct StIO;
template <> struct StIO<float> {
    static __device__ __forceinline__ void store4(float* p, const float (&v)[4]) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
    static __device__ __forceinline__ void store1(float* p, float v) { *p = v; }
    static __device__ __forceinline__ void load4(const float* p, float (&v)[4]) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
    static __device__ __forceinline__ float load1(const float* p) { return *p; }
};
template <> struct StIO<__hip_bfloat16> {
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

__device__ __forceinline__ float st_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;                                                                // valid in lane 0
}

}  // namespace

__global__ __launch_bounds__(ST_THREADS) void stem_moments_kernel(const float* __restrict__ x, double* __restrict__ partial, StGrid g, uint32_t ntiles) {
    __shared__ double red[ST_THREADS / 64][ST_MOMENTS];
    double acc[ST_MOMENTS];
#pragma unroll
    for (int i = 0; i < ST_MOMENTS; ++i) acc[i] = 0.0;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t n0 = tile * (uint32_t)ST_TILE + threadIdx.x * (uint32_t)ST_PPT;
        if (n0 >= g.N) continue;
        float p[ST_PPT][9];
        uint32_t b0, q0;
        st_patches(x, g, n0, p, b0, q0);
#pragma unroll
        for (int k = 0; k < ST_PPT; ++k) {                                   // a pixel past N is all zeros: it adds nothing
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                const double pi = (double)p[k][i];
                acc[i] += pi;
#pragma unroll
                for (int j = 0; j <= i; ++j) acc[9 + i * (i + 1) / 2 + j] = fma(pi, (double)p[k][j], acc[9 + i * (i + 1) / 2 + j]);
            }
        }
    }
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < ST_MOMENTS; ++i) {
        const double v = wave_sum(acc[i]);
        if (lane == 0) red[wave][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < ST_MOMENTS) {
        double s = red[0][threadIdx.x];
#pragma unroll
        for (int wv = 1; wv < ST_THREADS / 64; ++wv) s += red[wv][threadIdx.x];
        partial[(size_t)blockIdx.x * ST_MOMENTS + threadIdx.x] = s;
    }
}

// One workgroup: moments = the partials added in ST_SLICES contiguous index ranges in index order, then the range sums in order;
// then channel c's mean, biased variance and rstd in float64, rounded once.
__global__ __launch_bounds__(ST_THREADS) void stem_stats_kernel(const double* __restrict__ partial, int nparts, const float* __restrict__ w,
                                                                const float* __restrict__ bias, int C, double count, float eps,
                                                                double* __restrict__ moments, float* __restrict__ stats) {
    __shared__ double red[ST_THREADS / 64][64];
    __shared__ double mom[ST_MOMENTS];
    const int col = (int)threadIdx.x & 63, slice = (int)threadIdx.x >> 6;      // 4 ranges x 64 columns (54 live)
    const int per = (nparts + ST_THREADS / 64 - 1) / (ST_THREADS / 64);
    const int g0 = slice * per, g1 = min(g0 + per, nparts);
    double s = 0.0;
    if (col < ST_MOMENTS)
#pragma unroll 8
        for (int gi = g0; gi < g1; ++gi) s += partial[(size_t)gi * ST_MOMENTS + col];
    red[slice][col] = s;
    __syncthreads();
    if (threadIdx.x < ST_MOMENTS) {
        double t = red[0][threadIdx.x];
#pragma unroll
        for (int i = 1; i < ST_THREADS / 64; ++i) t += red[i][threadIdx.x];
        mom[threadIdx.x] = t;
        moments[threadIdx.x] = t;
    }
    __syncthreads();
    const int c = (int)threadIdx.x;
    if (c >= C) return;
    double m[9], wc[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) { m[i] = mom[i] / count; wc[i] = (double)w[c * 9 + i]; }
    double mean = bias ? (double)bias[c] : 0.0, var = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        mean = fma(wc[i], m[i], mean);
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            const double cov = mom[9 + i * (i + 1) / 2 + j] / count - m[i] * m[j];
            var = fma(wc[i] * wc[j] * (i == j ? 1.0 : 2.0), cov, var);
        }
    }
    if (var < 0.0) var = 0.0;                                                // a constant image: rounding may leave -1e-17
    stats[c] = (float)mean;
    stats[C + c] = (float)var;
    stats[2 * C + c] = (float)(1.0 / sqrt(var + (double)eps));
}

template <typename T>
__global__ __launch_bounds__(ST_THREADS) void stem_apply_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                const float* __restrict__ stats, T* __restrict__ z, StGrid g, int C, float slope) {
    __shared__ __align__(16) float coef[ST_FWD_CH][ST_COEF];
    const int c0 = (int)blockIdx.y * ST_FWD_CH;
    st_load_coef(coef, c0, ST_FWD_CH, C, w, bias, gamma, beta, stats);
    const uint32_t n0 = blockIdx.x * (uint32_t)ST_TILE + threadIdx.x * (uint32_t)ST_PPT;
    if (n0 >= g.N) return;
    float p[ST_PPT][9];
    uint32_t b0, q0;
    st_patches(x, g, n0, p, b0, q0);
    const bool vec = (g.HW & (ST_PPT - 1)) == 0;                             // uniform: the four pixels are one aligned piece of a plane
#pragma unroll 2
    for (int ci = 0; ci < ST_FWD_CH; ++ci) {
        float cf[ST_COEF], o[ST_PPT];
        st_coef(coef, ci, cf);
#pragma unroll
        for (int k = 0; k < ST_PPT; ++k) {
            float xh, u;
            st_preact(p[k], cf, xh, u);
            o[k] = u > 0.0f ? u : u * slope;
        }
        if (vec) {
            StIO<T>::store4(z + ((size_t)b0 * C + c0 + ci) * g.HW + q0, o);
        } else {
#pragma unroll
            for (int k = 0; k < ST_PPT; ++k) {                               // the next image begins where q0 + k reaches H W
                uint32_t bk = b0, qk = q0 + k;
                while (qk >= g.HW) { qk -= g.HW; ++bk; }                     // at most k images further (H W < 4: one pixel each)
                if (n0 + k < g.N) StIO<T>::store1(z + ((size_t)bk * C + c0 + ci) * g.HW + qk, o[k]);
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(ST_THREADS) void stem_bwd_reduce_kernel(const T* __restrict__ dz, const float* __restrict__ x, const float* __restrict__ w,
                                                                     const float* __restrict__ bias, const float* __restrict__ gamma,
                                                                     const float* __restrict__ beta, const float* __restrict__ stats,
                                                                     float* __restrict__ partial, StGrid g, int C, float slope, uint32_t ntiles) {
    __shared__ __align__(16) float coef[ST_BWD_CH][ST_COEF];
    __shared__ float red[ST_THREADS / 64][ST_BWD_CH * ST_SUMS];
    const int c0 = (int)blockIdx.y * ST_BWD_CH;
    st_load_coef(coef, c0, ST_BWD_CH, C, w, bias, gamma, beta, stats);
    const bool vec = (g.HW & (ST_PPT - 1)) == 0;
    float acc[ST_BWD_CH][ST_SUMS];
#pragma unroll
    for (int ci = 0; ci < ST_BWD_CH; ++ci)
#pragma unroll
        for (int j = 0; j < ST_SUMS; ++j) acc[ci][j] = 0.0f;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t n0 = tile * (uint32_t)ST_TILE + threadIdx.x * (uint32_t)ST_PPT;
        if (n0 >= g.N) continue;
        float p[ST_PPT][9];
        uint32_t b0, q0;
        st_patches(x, g, n0, p, b0, q0);
#pragma unroll
        for (int ci = 0; ci < ST_BWD_CH; ++ci) {
            float cf[ST_COEF], d[ST_PPT];
            st_coef(coef, ci, cf);
            if (vec) {
                StIO<T>::load4(dz + ((size_t)b0 * C + c0 + ci) * g.HW + q0, d);
            } else {
#pragma unroll
                for (int k = 0; k < ST_PPT; ++k) {
                    uint32_t bk = b0, qk = q0 + k;
                    while (qk >= g.HW) { qk -= g.HW; ++bk; }
                    d[k] = n0 + k < g.N ? StIO<T>::load1(dz + ((size_t)bk * C + c0 + ci) * g.HW + qk) : 0.0f;
                }
            }
#pragma unroll
            for (int k = 0; k < ST_PPT; ++k) {
                float xh, u;
                st_preact(p[k], cf, xh, u);
                const float gk = u > 0.0f ? d[k] : d[k] * slope;
                acc[ci][0] += gk;
                acc[ci][1] = fmaf(gk, xh, acc[ci][1]);
#pragma unroll
                for (int t = 0; t < 9; ++t) acc[ci][2 + t] = fmaf(gk, p[k][t], acc[ci][2 + t]);
            }
        }
    }
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
#pragma unroll
    for (int ci = 0; ci < ST_BWD_CH; ++ci)
#pragma unroll
        for (int j = 0; j < ST_SUMS; ++j) {
            const float v = st_wave_sum(acc[ci][j]);
            if (lane == 0) red[wave][ci * ST_SUMS + j] = v;
        }
    __syncthreads();
    if (threadIdx.x < ST_BWD_CH * ST_SUMS) {
        float s = red[0][threadIdx.x];
#pragma unroll
        for (int wv = 1; wv < ST_THREADS / 64; ++wv) s += red[wv][threadIdx.x];
        const int ci = (int)threadIdx.x / ST_SUMS, j = (int)threadIdx.x - ci * ST_SUMS;
        partial[((size_t)blockIdx.x * C + c0 + ci) * ST_SUMS + j] = s;
    }
}

// One workgroup per channel: its 11 sums from the partials (ST_SLICES contiguous index ranges in index order, then the range sums in
// order, float64), then dW_c [9], dgamma_c and dbeta_c by the formulas at the top in float64, rounded once.
__global__ __launch_bounds__(ST_THREADS) void stem_bwd_finish_kernel(const float* __restrict__ partial, int nparts, const float* __restrict__ w,
                                                                     const float* __restrict__ bias, const float* __restrict__ gamma,
                                                                     const float* __restrict__ stats, const double* __restrict__ moments, int C,
                                                                     double count, float* __restrict__ dw, float* __restrict__ dgamma,
                                                                     float* __restrict__ dbeta) {
    __shared__ double red[ST_SLICES][16];
    __shared__ double tot[16];
    const int c = (int)blockIdx.x;
    const int col = (int)threadIdx.x & 15, slice = (int)threadIdx.x >> 4;
    const int per = (nparts + ST_SLICES - 1) / ST_SLICES;
    const int g0 = slice * per, g1 = min(g0 + per, nparts);
    double s = 0.0;
    if (col < ST_SUMS)
#pragma unroll 8
        for (int gi = g0; gi < g1; ++gi) s += (double)partial[((size_t)gi * C + c) * ST_SUMS + col];
    red[slice][col] = s;
    __syncthreads();
    if (threadIdx.x < 16) {
        double t = red[0][threadIdx.x];
#pragma unroll
        for (int i = 1; i < ST_SLICES; ++i) t += red[i][threadIdx.x];
        tot[threadIdx.x] = t;
    }
    __syncthreads();
    const int t = (int)threadIdx.x;
    if (t >= ST_SUMS) return;
    const double db = tot[0], dg = tot[1];
    if (t == 9) { dgamma[c] = (float)dg; return; }
    if (t == 10) { dbeta[c] = (float)db; return; }
    // tap t of dW_c; xhat was formed from the float32 (b - mean) and rstd, so X_c uses those very values
    const double rstd = (double)stats[2 * C + c], bm = (double)((bias ? bias[c] : 0.0f) - stats[c]);
    double xs = bm * moments[t];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const int hi = t > j ? t : j, lo = t > j ? j : t;
        xs = fma(moments[9 + hi * (hi + 1) / 2 + lo], (double)w[c * 9 + j], xs);
    }
    const double X = rstd * xs;
    dw[c * 9 + t] = (float)((double)gamma[c] * rstd * (tot[2 + t] - (db / count) * moments[t] - (dg / count) * X));
}

long long gennet_stem_train_workspace_bytes(long long n, int C) {
    if (n < 2 || n > 0x7fffffffLL || !gennet_stem_channels_ok(C)) return -1;
    const long long a = ST_MOMENTS * (long long)sizeof(double), b = (long long)C * ST_SUMS * (long long)sizeof(float);
    return (a > b ? a : b) * (long long)st_blocks(n);
}

int gennet_stem_train_fwd_launch(const float* x, const float* w, const float* bias, const float* gamma, const float* beta, void* z, float* stats,
                                 double* moments, void* workspace, int B, int H, int W, int C, float eps, float slope, int dtype, hipStream_t stream) {
    if (!gennet_stem_channels_ok(C)) return -1;
    const long long n = (long long)B * H * W;
    const StGrid g{(uint32_t)H, (uint32_t)W, (uint32_t)(H * W), (uint32_t)n};
    const unsigned blocks = st_blocks(n), tiles = st_tiles(n);
    hipLaunchKernelGGL(stem_moments_kernel, dim3(blocks), dim3(ST_THREADS), 0, stream, x, (double*)workspace, g, tiles);
    int e = (int)hipGetLastError();
    if (e != 0) return e;
    hipLaunchKernelGGL(stem_stats_kernel, dim3(1), dim3(ST_THREADS), 0, stream, (const double*)workspace, (int)blocks, w, bias, C, (double)n, eps, moments,
                       stats);
    e = (int)hipGetLastError();
    if (e != 0) return e;
    const dim3 grid(tiles, (unsigned)(C / ST_FWD_CH));
    if (dtype == 0)
        hipLaunchKernelGGL((stem_apply_kernel<float>), grid, dim3(ST_THREADS), 0, stream, x, w, bias, gamma, beta, (const float*)stats, (float*)z, g, C, slope);
    else
        hipLaunchKernelGGL((stem_apply_kernel<__hip_bfloat16>), grid, dim3(ST_THREADS), 0, stream, x, w, bias, gamma, beta, (const float*)stats,
                           (__hip_bfloat16*)z, g, C, slope);
    return (int)hipGetLastError();
}

int gennet_stem_train_bwd_launch(const void* dz, const float* x, const float* w, const float* bias, const float* gamma, const float* beta,
                                 const float* stats, const double* moments, void* workspace, float* dw, float* dgamma, float* dbeta, int B, int H, int W,
                                 int C, float slope, int dtype, hipStream_t stream) {
    if (!gennet_stem_channels_ok(C)) return -1;
    const long long n = (long long)B * H * W;
    const StGrid g{(uint32_t)H, (uint32_t)W, (uint32_t)(H * W), (uint32_t)n};
    const unsigned blocks = st_blocks(n), tiles = st_tiles(n);
    const dim3 grid(blocks, (unsigned)(C / ST_BWD_CH));
    if (dtype == 0)
        hipLaunchKernelGGL((stem_bwd_reduce_kernel<float>), grid, dim3(ST_THREADS), 0, stream, (const float*)dz, x, w, bias, gamma, beta, stats,
                           (float*)workspace, g, C, slope, tiles);
    else
        hipLaunchKernelGGL((stem_bwd_reduce_kernel<__hip_bfloat16>), grid, dim3(ST_THREADS), 0, stream, (const __hip_bfloat16*)dz, x, w, bias, gamma, beta,
                           stats, (float*)workspace, g, C, slope, tiles);
    const int e = (int)hipGetLastError();
    if (e != 0) return e;
    hipLaunchKernelGGL(stem_bwd_finish_kernel, dim3((unsigned)C), dim3(ST_THREADS), 0, stream, (const float*)workspace, (int)blocks, w, bias, gamma, stats,
                       moments, C, (double)n, dw, dgamma, dbeta);
    return (int)hipGetLastError();
}

}  // namespace ppn
