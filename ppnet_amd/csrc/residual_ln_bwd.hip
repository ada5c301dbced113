// residual_ln_bwd.hip — the TRAINING pair of fused_norm.hip's residual + LayerScale + LayerNorm kernel on gfx950: the residual stream
// of a NAT / DiNAT block (reference SegNet/nat.py:140-153) with stochastic depth folded in, forward and backward.
//
//   rln_train_fwd_kernel   x' = x + s[b] * gamma * a ;  y = LN(x') ;  stats[row] = (mean, rstd)      4 tensor passes (x, a in; x', y out)
//   rln_bwd_kernel         G = gx + LN'(gy) ;  dx = G ;  da = s[b] * gamma * G ;  per-channel sums    6 (gy, gx, x', a in; dx, da out)
//   rln_colsum_kernel      dgamma, dw, dbeta from the workgroups' partial sums
//
// s [B] float32 is the per-image stochastic-depth scale (0 = dropped, 1 / keep otherwise; NULL = 1), image b owns rows_per_image
// consecutive rows; gamma NULL = 1; a NULL = a plain LayerNorm; y NULL = no LayerNorm behind the residual (no statistics).
//
// Row ownership is norm_kernel's: C <= 64 one THREAD per row (lpr = 1, C / 8 pieces per lane), otherwise C / 8 lanes per row (16, 32
// or 64), C = 1024 two pieces per lane.  Piece p of lane li holds channels (p * lpr + li) * 8 .. + 7.  Inputs float32 or bfloat16,
// every statistic and sum float32, every output rounded once.
//
// Channel sums without atomics: a workgroup (256 threads = 256 / lpr rows per tile) walks tiles blockIdx.x, blockIdx.x + gridDim.x, ...
// (at most RLN_MAX_BLOCKS workgroups), each lane adding its rows' terms to its own channels in registers in that order; at the end
// the lanes that hold the same channels are added through LDS in thread order and the workgroup writes ONE [3][C] float32 partial.
// rln_colsum_kernel adds the partials in a fixed order (32 contiguous index ranges in index order, then the 32 range sums in order)
// and rounds once: the gradients are bitwise reproducible.
#include <hip/hip_bf16.h>
#include "ppn_device.h"
#include "ppn_kernels.h"
#include "norm_vec.h"

namespace ppn {

constexpr int RLN_MAX_BLOCKS = 1024;   // 4 workgroups per CU of the 256: every CU busy, and the partials stay a few MB (1024 x 3 x C floats)
constexpr int RLN_SLICES = 32;         // index ranges of the partials summed side by side in rln_colsum_kernel

namespace {

// nv pieces per lane and lpr lanes per row for a row of C channels; false = a width the kernels do not take
bool rln_geometry(int C, int& nv, int& lpr) {
    if (C <= 0 || C % 8 != 0) return false;
    if (C <= 64) { nv = C / 8; lpr = 1; return true; }
    int l = C / 8, n = 1;
    if (l > 64) { n = l / 64; l = 64; }
    if (n > 2 || (l & (l - 1)) != 0 || l * 8 * n != C) return false;
    nv = n; lpr = l;
    return true;
}

unsigned rln_tiles(long long rows, int lpr) { const long long rpt = 256 / lpr; return (unsigned)((rows + rpt - 1) / rpt); }
unsigned rln_blocks(long long rows, int lpr) { const unsigned t = rln_tiles(rows, lpr); return t < (unsigned)RLN_MAX_BLOCKS ? t : (unsigned)RLN_MAX_BLOCKS; }

template <typename T> __device__ __forceinline__ void round_through(float (&v)[8]) {
    if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int k = 0; k < 8; k += 2) {
            const uint32_t u = Vec8<__hip_bfloat16>::pack(v[k], v[k + 1]);
            v[k] = __uint_as_float(u << 16); v[k + 1] = __uint_as_float(u & 0xffff0000u);
        }
    }
}

}  // namespace

template <typename T, int NV>
__global__ __launch_bounds__(256) void rln_train_fwd_kernel(const T* __restrict__ x, const T* __restrict__ a, const T* __restrict__ gamma,
                                                            const float* __restrict__ scale, const T* __restrict__ w, const T* __restrict__ b,
                                                            T* __restrict__ x_out, T* __restrict__ y_out, float* __restrict__ stats, uint32_t rows,
                                                            uint32_t rows_per_image, int C, int lpr, float eps, uint32_t ntiles) {
    const int li = (int)threadIdx.x & (lpr - 1);
    const uint32_t rpt = 256u / (uint32_t)lpr, rit = threadIdx.x / (uint32_t)lpr;
    // per-channel vectors are the same for every row: loaded once, every tile of the workgroup reuses them
    float gv[NV][8], wv[NV][8], bv[NV][8];
#pragma unroll
    for (int p = 0; p < NV; ++p) {
        const int c0 = (p * lpr + li) * 8;
        if (a && gamma) Vec8<T>::load(gamma + c0, gv[p]);
        if (y_out) { Vec8<T>::load(w + c0, wv[p]); Vec8<T>::load(b + c0, bv[p]); }
    }
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t row = tile * rpt + rit;
        const bool live = row < rows;                                        // dead lanes still join the shuffles
        const size_t at = (size_t)row * C;
        float v[NV][8];
        if (live) {
            const float sc = (a && scale) ? scale[row / rows_per_image] : 1.0f;
#pragma unroll
            for (int p = 0; p < NV; ++p) {
                const int c0 = (p * lpr + li) * 8;
                Vec8<T>::load(x + at + c0, v[p]);
                if (a) {
                    float av[8];
                    Vec8<T>::load(a + at + c0, av);
                    if (gamma) {                                             // scale NULL: sc * gamma is gamma itself, the inference kernel's bits
#pragma unroll
                        for (int k = 0; k < 8; ++k) v[p][k] = fmaf(sc * gv[p][k], av[k], v[p][k]);
                    } else if (scale) {
#pragma unroll
                        for (int k = 0; k < 8; ++k) v[p][k] = fmaf(sc, av[k], v[p][k]);
                    } else {
#pragma unroll
                        for (int k = 0; k < 8; ++k) v[p][k] += av[k];
                    }
                    Vec8<T>::store(x_out + at + c0, v[p]);
                    round_through<T>(v[p]);                                  // LN sees what the next op reads back: the rounded stream
                }
            }
        } else {
#pragma unroll
            for (int p = 0; p < NV; ++p)
#pragma unroll
                for (int k = 0; k < 8; ++k) v[p][k] = 0.0f;
        }
        if (!y_out) continue;                                                // residual only (last sub-layer of a level)
        float s = 0.0f;
#pragma unroll
        for (int p = 0; p < NV; ++p)
#pragma unroll
            for (int k = 0; k < 8; ++k) s += v[p][k];
        const float mean = group_sum(s, lpr) / (float)C;
        float q = 0.0f;
#pragma unroll
        for (int p = 0; p < NV; ++p)
#pragma unroll
            for (int k = 0; k < 8; ++k) { const float d = v[p][k] - mean; q = fmaf(d, d, q); }
        const float rstd = rsqrtf(group_sum(q, lpr) / (float)C + eps);
        if (!live) continue;
        if (li == 0) *reinterpret_cast<float2*>(stats + 2 * (size_t)row) = make_float2(mean, rstd);
#pragma unroll
        for (int p = 0; p < NV; ++p) {
            const int c0 = (p * lpr + li) * 8;
            float o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = fmaf((v[p][k] - mean) * rstd, wv[p][k], bv[p][k]);
            Vec8<T>::store(y_out + at + c0, o);
        }
    }
}

// gy NULL: no LayerNorm term (xn, stats, w unused).  gx NULL: nothing arrives at x' from later consumers.  dx NULL: not wanted (with gy NULL
// it would be gx itself).  da NULL: not wanted (a plain LayerNorm, or neither gamma nor scale: da is dx).  a is read only for dgamma.
template <typename T, int NV>
__global__ __launch_bounds__(256) void rln_bwd_kernel(const T* __restrict__ gy, const T* __restrict__ gx, const T* __restrict__ xn,
                                                      const float* __restrict__ stats, const T* __restrict__ a, const T* __restrict__ gamma,
                                                      const float* __restrict__ scale, const T* __restrict__ w, T* __restrict__ dx, T* __restrict__ da,
                                                      float* __restrict__ partial, uint32_t rows, uint32_t rows_per_image, int C, int lpr,
                                                      uint32_t ntiles) {
    __shared__ __align__(16) float red[256 * NV * 8];
    const int li = (int)threadIdx.x & (lpr - 1);
    const uint32_t rpt = 256u / (uint32_t)lpr, rit = threadIdx.x / (uint32_t)lpr;
    const bool want_dgamma = a && gamma;
    // gamma and w: kept in registers where a lane holds one or two pieces; the thread-per-row forms with more (every lane the same
    // channels: a broadcast from L1) load them where they are used, or the three sums' registers would spill
    constexpr bool KEEP = NV <= 2;
    float acc_g[NV][8], acc_w[NV][8], acc_b[NV][8], gv[KEEP ? NV : 1][8], wv[KEEP ? NV : 1][8];
#pragma unroll
    for (int p = 0; p < NV; ++p) {
        const int c0 = (p * lpr + li) * 8;
#pragma unroll
        for (int k = 0; k < 8; ++k) { acc_g[p][k] = 0.0f; acc_w[p][k] = 0.0f; acc_b[p][k] = 0.0f; }
        if constexpr (KEEP) {
            if (gamma) Vec8<T>::load(gamma + c0, gv[p]);
            if (gy) Vec8<T>::load(w + c0, wv[p]);
        }
    }
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t row = tile * rpt + rit;
        const bool live = row < rows;                                        // dead lanes carry zeros through the shuffles
        const size_t at = (size_t)row * C;
        float G[NV][8];
#pragma unroll
        for (int p = 0; p < NV; ++p) {
            if (gx && live) {
                Vec8<T>::load(gx + at + (p * lpr + li) * 8, G[p]);
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) G[p][k] = 0.0f;
            }
        }
        if (gy) {
            float xh[NV][8], g[NV][8];
            float mean = 0.0f, rstd = 0.0f;
            if (live) { const float2 st = *reinterpret_cast<const float2*>(stats + 2 * (size_t)row); mean = st.x; rstd = st.y; }
            float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
            for (int p = 0; p < NV; ++p) {
                if (live) {
                    const int c0 = (p * lpr + li) * 8;
                    float gyv[8], wl[8];
                    if constexpr (!KEEP) Vec8<T>::load(w + c0, wl);
                    Vec8<T>::load(xn + at + c0, xh[p]);
                    Vec8<T>::load(gy + at + c0, gyv);
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        xh[p][k] = (xh[p][k] - mean) * rstd;
                        acc_w[p][k] = fmaf(gyv[k], xh[p][k], acc_w[p][k]);
                        acc_b[p][k] += gyv[k];
                        g[p][k] = gyv[k] * (KEEP ? wv[KEEP ? p : 0][k] : wl[k]);
                        s1 += g[p][k];
                        s2 = fmaf(g[p][k], xh[p][k], s2);
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 8; ++k) { xh[p][k] = 0.0f; g[p][k] = 0.0f; }
                }
            }
            const float m1 = group_sum(s1, lpr) / (float)C, m2 = group_sum(s2, lpr) / (float)C;
#pragma unroll
            for (int p = 0; p < NV; ++p)
#pragma unroll
                for (int k = 0; k < 8; ++k) G[p][k] += rstd * (g[p][k] - m1 - xh[p][k] * m2);
        }
        if (!live) continue;
        const float sc = scale ? scale[row / rows_per_image] : 1.0f;
#pragma unroll
        for (int p = 0; p < NV; ++p) {
            const int c0 = (p * lpr + li) * 8;
            if (dx) Vec8<T>::store(dx + at + c0, G[p]);
            if (da) {
                float o[8], gl[8];
                if constexpr (!KEEP) { if (gamma) Vec8<T>::load(gamma + c0, gl); }
#pragma unroll
                for (int k = 0; k < 8; ++k) o[k] = (gamma ? sc * (KEEP ? gv[KEEP ? p : 0][k] : gl[k]) : sc) * G[p][k];
                Vec8<T>::store(da + at + c0, o);
            }
            if (want_dgamma) {
                float av[8];
                Vec8<T>::load(a + at + c0, av);
#pragma unroll
                for (int k = 0; k < 8; ++k) acc_g[p][k] = fmaf(sc * av[k], G[p][k], acc_g[p][k]);
            }
        }
    }
    // the workgroup's partial: for each of the three sums, every lane's registers to LDS, then thread c adds channel c's
    // 256 / lpr holders in thread order
    const int groups = 256 / lpr;
    float* out = partial + (size_t)blockIdx.x * 3 * C;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        float (&acc)[NV][8] = q == 0 ? acc_g : (q == 1 ? acc_w : acc_b);
#pragma unroll
        for (int p = 0; p < NV; ++p) Vec8<float>::store(red + (size_t)threadIdx.x * (NV * 8) + p * 8, acc[p]);
        __syncthreads();
        for (int c = (int)threadIdx.x; c < C; c += 256) {
            const int piece = c >> 3, p = piece / lpr, l = piece & (lpr - 1);
            float s = 0.0f;
            for (int gi = 0; gi < groups; ++gi) s += red[(gi * lpr + l) * (NV * 8) + p * 8 + (c & 7)];
            out[q * C + c] = s;
        }
        __syncthreads();
    }
}

// dgamma / dw / dbeta [C] of dtype T from `nparts` partials [nparts][3][C]: 8 columns x RLN_SLICES index ranges per workgroup; a NULL output
// is skipped.
template <typename T> __device__ __forceinline__ void store_one(T* p, float v);
template <> __device__ __forceinline__ void store_one<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void store_one<__hip_bfloat16>(__hip_bfloat16* p, float v) { *p = __float2bfloat16(v); }

template <typename T>
__global__ __launch_bounds__(256) void rln_colsum_kernel(const float* __restrict__ partial, int nparts, int C, T* __restrict__ dgamma,
                                                         T* __restrict__ dw, T* __restrict__ dbeta) {
    __shared__ float red[RLN_SLICES][8];
    const int cl = (int)threadIdx.x & 7, slice = (int)threadIdx.x >> 3;
    const int col = (int)blockIdx.x * 8 + cl;                                 // 3 C columns, a multiple of 8
    const int per = (nparts + RLN_SLICES - 1) / RLN_SLICES;
    const int g0 = slice * per, g1 = min(g0 + per, nparts);
    float s = 0.0f;
    for (int g = g0; g < g1; ++g) s += partial[(size_t)g * 3 * C + col];
    red[slice][cl] = s;
    __syncthreads();
    if (slice != 0) return;
    float t = 0.0f;
#pragma unroll
    for (int i = 0; i < RLN_SLICES; ++i) t += red[i][cl];
    const int q = col / C, c = col - q * C;
    T* dst = q == 0 ? dgamma : (q == 1 ? dw : dbeta);
    if (dst) store_one<T>(dst + c, t);
}

long long residual_ln_bwd_workspace_floats(long long rows, int C) {
    int nv, lpr;
    if (rows <= 0 || rows > 0x7fffffffLL || !rln_geometry(C, nv, lpr)) return -1;
    return (long long)rln_blocks(rows, lpr) * 3 * C;
}

template <typename T>
static int launch_rln_fwd(const void* x, const void* a, const void* gamma, const float* scale, const void* w, const void* b, void* x_out, void* y_out,
                          float* stats, long long rows, long long rows_per_image, int C, float eps, hipStream_t stream) {
    int nv, lpr;
    if (rows > 0x7fffffffLL || !rln_geometry(C, nv, lpr)) return -1;
    const unsigned ntiles = rln_tiles(rows, lpr);
    const dim3 grid(rln_blocks(rows, lpr));
#define PPN_RLN_FWD(NV) hipLaunchKernelGGL((rln_train_fwd_kernel<T, NV>), grid, dim3(256), 0, stream, (const T*)x, (const T*)a, (const T*)gamma, \
    scale, (const T*)w, (const T*)b, (T*)x_out, (T*)y_out, stats, (uint32_t)rows, (uint32_t)rows_per_image, C, lpr, eps, ntiles)
    switch (nv) {
        case 1: PPN_RLN_FWD(1); break; case 2: PPN_RLN_FWD(2); break; case 3: PPN_RLN_FWD(3); break; case 4: PPN_RLN_FWD(4); break;
        case 5: PPN_RLN_FWD(5); break; case 6: PPN_RLN_FWD(6); break; case 7: PPN_RLN_FWD(7); break; default: PPN_RLN_FWD(8); break;
    }
#undef PPN_RLN_FWD
    return (int)hipGetLastError();
}

int residual_ln_train_fwd_launch(const void* x, const void* a, const void* gamma, const float* scale, const void* w, const void* b, void* x_out,
                                 void* y_out, float* stats, long long rows, long long rows_per_image, int C, float eps, int dtype, hipStream_t stream) {
    return dtype == 0 ? launch_rln_fwd<float>(x, a, gamma, scale, w, b, x_out, y_out, stats, rows, rows_per_image, C, eps, stream)
                      : launch_rln_fwd<__hip_bfloat16>(x, a, gamma, scale, w, b, x_out, y_out, stats, rows, rows_per_image, C, eps, stream);
}

template <typename T>
static int launch_rln_bwd(const void* gy, const void* gx, const void* xn, const float* stats, const void* a, const void* gamma, const float* scale,
                          const void* w, void* dx, void* da, void* dgamma, void* dw, void* dbeta, float* workspace, long long rows,
                          long long rows_per_image, int C, hipStream_t stream) {
    int nv, lpr;
    if (rows > 0x7fffffffLL || !rln_geometry(C, nv, lpr)) return -1;
    const unsigned ntiles = rln_tiles(rows, lpr), blocks = rln_blocks(rows, lpr);
#define PPN_RLN_BWD(NV) hipLaunchKernelGGL((rln_bwd_kernel<T, NV>), dim3(blocks), dim3(256), 0, stream, (const T*)gy, (const T*)gx, (const T*)xn, stats, \
    (const T*)a, (const T*)gamma, scale, (const T*)w, (T*)dx, (T*)da, workspace, (uint32_t)rows, (uint32_t)rows_per_image, C, lpr, ntiles)
    switch (nv) {
        case 1: PPN_RLN_BWD(1); break; case 2: PPN_RLN_BWD(2); break; case 3: PPN_RLN_BWD(3); break; case 4: PPN_RLN_BWD(4); break;
        case 5: PPN_RLN_BWD(5); break; case 6: PPN_RLN_BWD(6); break; case 7: PPN_RLN_BWD(7); break; default: PPN_RLN_BWD(8); break;
    }
#undef PPN_RLN_BWD
    int e = (int)hipGetLastError();
    if (e != 0) return e;
    if (dgamma || dw || dbeta)
        hipLaunchKernelGGL((rln_colsum_kernel<T>), dim3((unsigned)(3 * C / 8)), dim3(256), 0, stream, (const float*)workspace, (int)blocks, C, (T*)dgamma,
                           (T*)dw, (T*)dbeta);
    return (int)hipGetLastError();
}

int residual_ln_bwd_launch(const void* gy, const void* gx, const void* xn, const float* stats, const void* a, const void* gamma, const float* scale,
                           const void* w, void* dx, void* da, void* dgamma, void* dw, void* dbeta, float* workspace, long long rows,
                           long long rows_per_image, int C, int dtype, hipStream_t stream) {
    return dtype == 0 ? launch_rln_bwd<float>(gy, gx, xn, stats, a, gamma, scale, w, dx, da, dgamma, dw, dbeta, workspace, rows, rows_per_image, C, stream)
                      : launch_rln_bwd<__hip_bfloat16>(gy, gx, xn, stats, a, gamma, scale, w, dx, da, dgamma, dw, dbeta, workspace, rows, rows_per_image,
                                                       C, stream);
}

}  // namespace ppn
