// mhsa_d8.hip — global multi-head self-attention at head dim 8, forward and backward: GenNet's AE-ViT blocks (dim 24, 3 heads, 784 or
// 1024 tokens; reference GenNet/networks/vit.py:71-161).  The math and the layouts are ppn_mhsa_fwd's and ppn_mhsa_bwd's (mhsa.hip,
// mhsa_bwd.hip) with 8 in place of 64: qkv and dqkv [B][N][3][heads][8], out and dout [B][N][heads][8].
//
//   P = softmax(scale S), S = q k^T;  O = P V;  dV = P^T dO;  dP = dO V^T;  delta = rowsum(dO o O);  dS = P o (dP - delta);
//   dQ = scale dS K;  dK = scale dS^T Q.
//
// At head dim 8 a dot product is 8 FMAs and a row is 32 bytes of float32: the work is the N^2 exponentials per head, and the matrix
// cores have nothing to chew on.  Every kernel here is plain VALU in float32 (bfloat16 is converted on load and rounded once on
// store, as ppn_na2d_bwd does), one shape throughout: a lane owns D8_R rows (queries, or keys in the dK / dV pass) with their 8
// channels in registers; the other side comes through LDS in tiles of D8_KT rows (double-buffered, one barrier per tile) and is
// read as broadcasts — one LDS read serves the lane's D8_R rows.  Nothing of size N x N touches memory.
//
//   forward     online softmax: logits of 16 keys at a time in registers, one rescale per 16 keys, the 16 keys' sums formed apart
//               before they join the running ones (rounding grows with 16 + N / 16 terms, not N).
//   statistics  per (b, h, query): L2 = log2 sum_j 2^(c S_j), c = scale log2 e, and delta, into the caller's workspace
//               ([2][B][heads][N] float32: ppn_mhsa_bwd_workspace).  With L2, p = exp2(c S - L2) needs no maximum.
//   dK / dV     one workgroup per (b, h, block of keys) sweeping all query tiles (c Q, dO, L2, delta through LDS).
//   dQ          one workgroup per (b, h, block of queries) sweeping all key tiles (K, V through LDS).
//
// q is multiplied by c once where it is loaded (every pass the same product, so every pass sees the same logits bit for bit) and
// the logit is the 8-term FMA chain in the order of the channels.  delta and dP use that same chain, so where O = V (one key)
// dP - delta is exactly 0.  Every output element has one writer, there are no atomics and every sum has a fixed order: repeated
// calls are bitwise equal.  Tail keys contribute nothing (a finite "absent" logit in the forward and the statistics, a select in
// dQ, a statistic that makes p exactly 0 in dK / dV); tail rows of a lane are never summed across lanes and never stored.
// The absent logit and the running maximum's start are -1e30 in the exp2 domain: every real logit c q.k must lie far above that,
// which any finite float32 q and k with a sane scale give (|c q.k| of 1e30 would overflow the softmax in any form).
//
// Element offsets are 64-bit; the caller (capi.hip) rejects launches of 2^31 work-items or more.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include "ppn_device.h"
#include "ppn_kernels.h"

namespace ppn {

namespace {
constexpr int D8 = 8;                          // head dim
constexpr int D8_THREADS = 128;                // work-items per workgroup
constexpr int D8_R = 2;                        // rows (queries or keys) a lane owns
constexpr int D8_RB = D8_THREADS * D8_R;       // rows a workgroup owns
constexpr int D8_KT = D8_THREADS;              // rows per LDS tile: every thread stages one
constexpr int D8_CH = 16;                      // rows of a tile whose sums are formed apart
constexpr float D8_LOG2E = 1.4426950408889634f;
constexpr float D8_LN2 = 0.6931471805599453f;
constexpr float D8_ABSENT = -1.0e30f;          // logit of a key that does not exist

// 8 consecutive elements -> float32 registers (bfloat16: the upper half of a float32, exact); zeros where the row does not exist
template <typename T>
__device__ __forceinline__ void load8(float* r, const T* src, bool valid) {
    if constexpr (sizeof(T) == 4) {
        const float4 a = valid ? *reinterpret_cast<const float4*>(src) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 b = valid ? *reinterpret_cast<const float4*>(src + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w; r[4] = b.x; r[5] = b.y; r[6] = b.z; r[7] = b.w;
    } else {
        const uint4 u = valid ? *reinterpret_cast<const uint4*>(src) : make_uint4(0, 0, 0, 0);
        r[0] = __uint_as_float(u.x << 16); r[1] = __uint_as_float(u.x & 0xffff0000u);
        r[2] = __uint_as_float(u.y << 16); r[3] = __uint_as_float(u.y & 0xffff0000u);
        r[4] = __uint_as_float(u.z << 16); r[5] = __uint_as_float(u.z & 0xffff0000u);
        r[6] = __uint_as_float(u.w << 16); r[7] = __uint_as_float(u.w & 0xffff0000u);
    }
}

// 8 float32 registers -> 8 consecutive elements (bfloat16: rounded to nearest even, once)
template <typename T>
__device__ __forceinline__ void store8(T* dst, const float* r) {
    if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<float4*>(dst) = make_float4(r[0], r[1], r[2], r[3]);
        *reinterpret_cast<float4*>(dst + 4) = make_float4(r[4], r[5], r[6], r[7]);
    } else {
        *reinterpret_cast<uint4*>(dst) = make_uint4(pack_bf16x2(r[0], r[1]), pack_bf16x2(r[2], r[3]), pack_bf16x2(r[4], r[5]), pack_bf16x2(r[6], r[7]));
    }
}

// a row of an LDS tile [row][8] float32: two 16-byte reads, the same address in every lane
__device__ __forceinline__ void lds8(float* r, const float* tile, int i) {
    const float4 a = *reinterpret_cast<const float4*>(tile + i * D8), b = *reinterpret_cast<const float4*>(tile + i * D8 + 4);
    r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w; r[4] = b.x; r[5] = b.y; r[6] = b.z; r[7] = b.w;
}

__device__ __forceinline__ void put8(float* tile, int i, const float* r) {
    *reinterpret_cast<float4*>(tile + i * D8) = make_float4(r[0], r[1], r[2], r[3]);
    *reinterpret_cast<float4*>(tile + i * D8 + 4) = make_float4(r[4], r[5], r[6], r[7]);
}

// the one dot product of this file: the channels in order, one rounding per step
__device__ __forceinline__ float dot8(const float* a, const float* b) {
    float acc = a[0] * b[0];
#pragma unroll
    for (int d = 1; d < D8; ++d) acc = __builtin_fmaf(a[d], b[d], acc);
    return acc;
}

struct D8Block {
    int blk, bh, h, b;
};
__device__ __forceinline__ D8Block d8_block(int heads, int blocks) {
    D8Block k;
    k.blk = (int)(blockIdx.x % (unsigned)blocks);
    k.bh = (int)(blockIdx.x / (unsigned)blocks);
    k.h = k.bh % heads;
    k.b = k.bh / heads;
    return k;
}
}  // namespace

// ------------------------------------------------------------------------------------------------ forward
template <typename T>
__global__ __launch_bounds__(D8_THREADS) void mhsa_d8_fwd_kernel(const T* __restrict__ qkv, T* __restrict__ out, int N, int heads, int qblocks,
                                                                  float scale) {
    __shared__ __attribute__((aligned(16))) float kv_lds[2][2][D8_KT * D8];            // [buffer][K, V][key][dim]
    const int tid = threadIdx.x;
    const D8Block id = d8_block(heads, qblocks);
    const size_t row = (size_t)3 * heads * D8, C = (size_t)heads * D8;
    const T* base = qkv + (size_t)id.b * N * row;
    const size_t hoff = (size_t)id.h * D8;
    const float sl2 = scale * D8_LOG2E;

    float qv[D8_R][D8], o[D8_R][D8], m[D8_R], l[D8_R];
#pragma unroll
    for (int r = 0; r < D8_R; ++r) {
        const int q = id.blk * D8_RB + r * D8_THREADS + tid;
        load8(qv[r], base + (size_t)(q < N ? q : 0) * row + hoff, q < N);
#pragma unroll
        for (int d = 0; d < D8; ++d) {
            qv[r][d] *= sl2;
            o[r][d] = 0.0f;
        }
        m[r] = D8_ABSENT;
        l[r] = 0.0f;
    }

    const int ntiles = (N + D8_KT - 1) / D8_KT;
    float sk[D8], sv[D8];
    auto fetch = [&](int tile) {
        const int n = tile * D8_KT + tid;
        const T* src = base + (size_t)(n < N ? n : 0) * row + hoff;
        load8(sk, src + C, n < N);
        load8(sv, src + 2 * C, n < N);
    };
    auto put = [&](int buf) {
        put8(kv_lds[buf][0], tid, sk);
        put8(kv_lds[buf][1], tid, sv);
    };
    fetch(0);
    put(0);
    __syncthreads();

    for (int tile = 0; tile < ntiles; ++tile) {
        const int buf = tile & 1;
        if (tile + 1 < ntiles) fetch(tile + 1);
        const float* kl = kv_lds[buf][0];
        const float* vl = kv_lds[buf][1];
        const int kvalid = N - tile * D8_KT < D8_KT ? N - tile * D8_KT : D8_KT;        // keys of this tile that exist (>= 1)
        for (int c0 = 0; c0 < kvalid; c0 += D8_CH) {
            float s[D8_R][D8_CH];
#pragma unroll
            for (int c = 0; c < D8_CH; ++c) {
                float kr[D8];
                lds8(kr, kl, c0 + c);
#pragma unroll
                for (int r = 0; r < D8_R; ++r) s[r][c] = dot8(qv[r], kr);
            }
            if (kvalid - c0 < D8_CH) {                                                 // (workgroup-uniform) absent keys out
#pragma unroll
                for (int c = 0; c < D8_CH; ++c)
#pragma unroll
                    for (int r = 0; r < D8_R; ++r) s[r][c] = c0 + c < kvalid ? s[r][c] : D8_ABSENT;
            }
            float alpha[D8_R], lt[D8_R], ot[D8_R][D8];
#pragma unroll
            for (int r = 0; r < D8_R; ++r) {
                float mx = m[r];
#pragma unroll
                for (int c = 0; c < D8_CH; ++c) mx = fmaxf(mx, s[r][c]);
                alpha[r] = __builtin_amdgcn_exp2f(m[r] - mx);
                m[r] = mx;
                lt[r] = 0.0f;
#pragma unroll
                for (int d = 0; d < D8; ++d) ot[r][d] = 0.0f;
            }
#pragma unroll
            for (int c = 0; c < D8_CH; ++c) {
                float vr[D8];
                lds8(vr, vl, c0 + c);
#pragma unroll
                for (int r = 0; r < D8_R; ++r) {
                    const float p = __builtin_amdgcn_exp2f(s[r][c] - m[r]);
                    lt[r] += p;
#pragma unroll
                    for (int d = 0; d < D8; ++d) ot[r][d] = __builtin_fmaf(p, vr[d], ot[r][d]);
                }
            }
#pragma unroll
            for (int r = 0; r < D8_R; ++r) {
                l[r] = __builtin_fmaf(l[r], alpha[r], lt[r]);
#pragma unroll
                for (int d = 0; d < D8; ++d) o[r][d] = __builtin_fmaf(o[r][d], alpha[r], ot[r][d]);
            }
        }
        if (tile + 1 < ntiles) put(buf ^ 1);                                           // the other buffer: every wave left it at the last barrier
        __syncthreads();
    }

    T* obase = out + (size_t)id.b * N * C + hoff;
#pragma unroll
    for (int r = 0; r < D8_R; ++r) {
        const int q = id.blk * D8_RB + r * D8_THREADS + tid;
        if (q < N) {
            const float inv = 1.0f / l[r];
            float res[D8];
#pragma unroll
            for (int d = 0; d < D8; ++d) res[d] = o[r][d] * inv;
            store8(obase + (size_t)q * C, res);
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward: statistics
template <typename T>
__global__ __launch_bounds__(D8_THREADS) void mhsa_d8_stats_kernel(const T* __restrict__ qkv, const T* __restrict__ out, const T* __restrict__ dout,
                                                                    float* __restrict__ lse2, float* __restrict__ delta, int N, int heads,
                                                                    int qblocks, float scale) {
    __shared__ __attribute__((aligned(16))) float k_lds[2][D8_KT * D8];                // [buffer][key][dim]
    const int tid = threadIdx.x;
    const D8Block id = d8_block(heads, qblocks);
    const size_t row = (size_t)3 * heads * D8, C = (size_t)heads * D8;
    const T* base = qkv + (size_t)id.b * N * row;
    const size_t hoff = (size_t)id.h * D8;
    const float sl2 = scale * D8_LOG2E;

    float qv[D8_R][D8], m[D8_R], l[D8_R];
#pragma unroll
    for (int r = 0; r < D8_R; ++r) {
        const int q = id.blk * D8_RB + r * D8_THREADS + tid;
        load8(qv[r], base + (size_t)(q < N ? q : 0) * row + hoff, q < N);
#pragma unroll
        for (int d = 0; d < D8; ++d) qv[r][d] *= sl2;
        m[r] = D8_ABSENT;
        l[r] = 0.0f;
    }

    const int ntiles = (N + D8_KT - 1) / D8_KT;
    float sk[D8];
    auto fetch = [&](int tile) {
        const int n = tile * D8_KT + tid;
        load8(sk, base + (size_t)(n < N ? n : 0) * row + C + hoff, n < N);
    };
    fetch(0);
    put8(k_lds[0], tid, sk);
    __syncthreads();

    for (int tile = 0; tile < ntiles; ++tile) {
        const int buf = tile & 1;
        if (tile + 1 < ntiles) fetch(tile + 1);
        const float* kl = k_lds[buf];
        const int kvalid = N - tile * D8_KT < D8_KT ? N - tile * D8_KT : D8_KT;
        for (int c0 = 0; c0 < kvalid; c0 += D8_CH) {
            float s[D8_R][D8_CH];
#pragma unroll
            for (int c = 0; c < D8_CH; ++c) {
                float kr[D8];
                lds8(kr, kl, c0 + c);
#pragma unroll
                for (int r = 0; r < D8_R; ++r) s[r][c] = dot8(qv[r], kr);
            }
            if (kvalid - c0 < D8_CH) {
#pragma unroll
                for (int c = 0; c < D8_CH; ++c)
#pragma unroll
                    for (int r = 0; r < D8_R; ++r) s[r][c] = c0 + c < kvalid ? s[r][c] : D8_ABSENT;
            }
#pragma unroll
            for (int r = 0; r < D8_R; ++r) {
                float mx = m[r];
#pragma unroll
                for (int c = 0; c < D8_CH; ++c) mx = fmaxf(mx, s[r][c]);
                float lt = 0.0f;
#pragma unroll
                for (int c = 0; c < D8_CH; ++c) lt += __builtin_amdgcn_exp2f(s[r][c] - mx);
                l[r] = __builtin_fmaf(l[r], __builtin_amdgcn_exp2f(m[r] - mx), lt);
                m[r] = mx;
            }
        }
        if (tile + 1 < ntiles) put8(k_lds[buf ^ 1], tid, sk);
        __syncthreads();
    }

#pragma unroll
    for (int r = 0; r < D8_R; ++r) {
        const int q = id.blk * D8_RB + r * D8_THREADS + tid;
        if (q < N) {
            float ov[D8], dv[D8];
            const size_t off = ((size_t)id.b * N + q) * C + hoff;
            load8(ov, out + off, true);
            load8(dv, dout + off, true);
            lse2[(size_t)id.bh * N + q] = m[r] + log2f(l[r]);
            delta[(size_t)id.bh * N + q] = dot8(dv, ov);
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward: dK, dV
// A lane owns D8_R keys; the tile's queries come as (c q, dO, L2, delta).  Queries past N are zero rows with delta 0 and a statistic
// that makes their p exactly 0.
template <typename T>
__global__ __launch_bounds__(D8_THREADS) void mhsa_d8_dkdv_kernel(const T* __restrict__ qkv, const T* __restrict__ dout,
                                                                   const float* __restrict__ lse2, const float* __restrict__ delta,
                                                                   T* __restrict__ dqkv, int N, int heads, int kblocks, float scale) {
    __shared__ __attribute__((aligned(16))) float qd_lds[2][2][D8_KT * D8];            // [buffer][c Q, dO][query][dim]
    __shared__ __attribute__((aligned(16))) float st_lds[2][D8_KT * 2];                // [buffer][query][L2, delta]
    const int tid = threadIdx.x;
    const D8Block id = d8_block(heads, kblocks);
    const size_t row = (size_t)3 * heads * D8, C = (size_t)heads * D8;
    const T* base = qkv + (size_t)id.b * N * row;
    const T* dbase = dout + (size_t)id.b * N * C;
    const size_t hoff = (size_t)id.h * D8;
    const float* lrow = lse2 + (size_t)id.bh * N;
    const float* drow = delta + (size_t)id.bh * N;
    const float sl2 = scale * D8_LOG2E;

    float kr[D8_R][D8], vr[D8_R][D8], dk[D8_R][D8], dv[D8_R][D8];
#pragma unroll
    for (int r = 0; r < D8_R; ++r) {
        const int key = id.blk * D8_RB + r * D8_THREADS + tid;
        const T* src = base + (size_t)(key < N ? key : 0) * row + hoff;
        load8(kr[r], src + C, key < N);
        load8(vr[r], src + 2 * C, key < N);
#pragma unroll
        for (int d = 0; d < D8; ++d) dk[r][d] = dv[r][d] = 0.0f;
    }

    const int ntiles = (N + D8_KT - 1) / D8_KT;
    float sq[D8], sd[D8], sl = 0.0f, sdl = 0.0f;
    auto fetch = [&](int tile) {
        const int n = tile * D8_KT + tid;
        const int nn = n < N ? n : 0;
        load8(sq, base + (size_t)nn * row + hoff, n < N);
        load8(sd, dbase + (size_t)nn * C + hoff, n < N);
#pragma unroll
        for (int d = 0; d < D8; ++d) sq[d] *= sl2;
        sl = n < N ? lrow[nn] : -D8_ABSENT;
        sdl = n < N ? drow[nn] : 0.0f;
    };
    auto put = [&](int buf) {
        put8(qd_lds[buf][0], tid, sq);
        put8(qd_lds[buf][1], tid, sd);
        *reinterpret_cast<float2*>(&st_lds[buf][2 * tid]) = make_float2(sl, sdl);
    };
    fetch(0);
    put(0);
    __syncthreads();

    for (int tile = 0; tile < ntiles; ++tile) {
        const int buf = tile & 1;
        if (tile + 1 < ntiles) fetch(tile + 1);
        const float* ql = qd_lds[buf][0];
        const float* dl = qd_lds[buf][1];
        const float* st = st_lds[buf];
        const int qvalid = N - tile * D8_KT < D8_KT ? N - tile * D8_KT : D8_KT;
        for (int c0 = 0; c0 < qvalid; c0 += D8_CH) {
            // the 16 queries' sums apart, then folded in
            float dkt[D8_R][D8], dvt[D8_R][D8];
#pragma unroll
            for (int r = 0; r < D8_R; ++r)
#pragma unroll
                for (int d = 0; d < D8; ++d) dkt[r][d] = dvt[r][d] = 0.0f;
#pragma unroll
            for (int c = 0; c < D8_CH; ++c) {
                float qi[D8], di[D8];
                lds8(qi, ql, c0 + c);
                lds8(di, dl, c0 + c);
                const float2 ld = *reinterpret_cast<const float2*>(&st[2 * (c0 + c)]);
#pragma unroll
                for (int r = 0; r < D8_R; ++r) {
                    const float p = __builtin_amdgcn_exp2f(dot8(qi, kr[r]) - ld.x);
                    const float ds = p * (dot8(di, vr[r]) - ld.y);
#pragma unroll
                    for (int d = 0; d < D8; ++d) {
                        dvt[r][d] = __builtin_fmaf(p, di[d], dvt[r][d]);
                        dkt[r][d] = __builtin_fmaf(ds, qi[d], dkt[r][d]);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < D8_R; ++r)
#pragma unroll
                for (int d = 0; d < D8; ++d) {
                    dk[r][d] += dkt[r][d];
                    dv[r][d] += dvt[r][d];
                }
        }
        if (tile + 1 < ntiles) put(buf ^ 1);
        __syncthreads();
    }

    T* gbase = dqkv + (size_t)id.b * N * row + hoff;
#pragma unroll
    for (int r = 0; r < D8_R; ++r) {
        const int key = id.blk * D8_RB + r * D8_THREADS + tid;
        if (key < N) {
            // the sums ran over c q = scale log2 e q: dK = scale sum dS q = ln 2 sum dS (c q)
#pragma unroll
            for (int d = 0; d < D8; ++d) dk[r][d] *= D8_LN2;
            store8(gbase + (size_t)key * row + C, dk[r]);
            store8(gbase + (size_t)key * row + 2 * C, dv[r]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward: dQ
template <typename T>
__global__ __launch_bounds__(D8_THREADS) void mhsa_d8_dq_kernel(const T* __restrict__ qkv, const T* __restrict__ dout,
                                                                 const float* __restrict__ lse2, const float* __restrict__ delta,
                                                                 T* __restrict__ dqkv, int N, int heads, int qblocks, float scale) {
    __shared__ __attribute__((aligned(16))) float kv_lds[2][2][D8_KT * D8];            // [buffer][K, V][key][dim]
    const int tid = threadIdx.x;
    const D8Block id = d8_block(heads, qblocks);
    const size_t row = (size_t)3 * heads * D8, C = (size_t)heads * D8;
    const T* base = qkv + (size_t)id.b * N * row;
    const size_t hoff = (size_t)id.h * D8;
    const float sl2 = scale * D8_LOG2E;

    float qv[D8_R][D8], dov[D8_R][D8], dq[D8_R][D8], L[D8_R], D[D8_R];
#pragma unroll
    for (int r = 0; r < D8_R; ++r) {
        const int q = id.blk * D8_RB + r * D8_THREADS + tid;
        const int qq = q < N ? q : 0;
        load8(qv[r], base + (size_t)qq * row + hoff, q < N);
        load8(dov[r], dout + ((size_t)id.b * N + qq) * C + hoff, q < N);
#pragma unroll
        for (int d = 0; d < D8; ++d) {
            qv[r][d] *= sl2;
            dq[r][d] = 0.0f;
        }
        L[r] = q < N ? lse2[(size_t)id.bh * N + qq] : 0.0f;
        D[r] = q < N ? delta[(size_t)id.bh * N + qq] : 0.0f;
    }

    const int ntiles = (N + D8_KT - 1) / D8_KT;
    float sk[D8], sv[D8];
    auto fetch = [&](int tile) {
        const int n = tile * D8_KT + tid;
        const T* src = base + (size_t)(n < N ? n : 0) * row + hoff;
        load8(sk, src + C, n < N);
        load8(sv, src + 2 * C, n < N);
    };
    auto put = [&](int buf) {
        put8(kv_lds[buf][0], tid, sk);
        put8(kv_lds[buf][1], tid, sv);
    };
    fetch(0);
    put(0);
    __syncthreads();

    for (int tile = 0; tile < ntiles; ++tile) {
        const int buf = tile & 1;
        if (tile + 1 < ntiles) fetch(tile + 1);
        const float* kl = kv_lds[buf][0];
        const float* vl = kv_lds[buf][1];
        const int kvalid = N - tile * D8_KT < D8_KT ? N - tile * D8_KT : D8_KT;
        for (int c0 = 0; c0 < kvalid; c0 += D8_CH) {
            const bool tail = kvalid - c0 < D8_CH;                                     // workgroup-uniform
            float dqt[D8_R][D8];
#pragma unroll
            for (int r = 0; r < D8_R; ++r)
#pragma unroll
                for (int d = 0; d < D8; ++d) dqt[r][d] = 0.0f;
#pragma unroll
            for (int c = 0; c < D8_CH; ++c) {
                float kj[D8], vj[D8];
                lds8(kj, kl, c0 + c);
                lds8(vj, vl, c0 + c);
                const bool absent = tail && c0 + c >= kvalid;
#pragma unroll
                for (int r = 0; r < D8_R; ++r) {
                    const float p = __builtin_amdgcn_exp2f(dot8(qv[r], kj) - L[r]);
                    float ds = p * (dot8(dov[r], vj) - D[r]);
                    ds = absent ? 0.0f : ds;                                           // a select: p of an absent key may be anything
#pragma unroll
                    for (int d = 0; d < D8; ++d) dqt[r][d] = __builtin_fmaf(ds, kj[d], dqt[r][d]);
                }
            }
#pragma unroll
            for (int r = 0; r < D8_R; ++r)
#pragma unroll
                for (int d = 0; d < D8; ++d) dq[r][d] += dqt[r][d];
        }
        if (tile + 1 < ntiles) put(buf ^ 1);
        __syncthreads();
    }

    T* gbase = dqkv + (size_t)id.b * N * row + hoff;
#pragma unroll
    for (int r = 0; r < D8_R; ++r) {
        const int q = id.blk * D8_RB + r * D8_THREADS + tid;
        if (q < N) {
#pragma unroll
            for (int d = 0; d < D8; ++d) dq[r][d] *= scale;
            store8(gbase + (size_t)q * row, dq[r]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ host
// rows and work-items per workgroup of every kernel above (capi.hip checks the launch size with them)
int mhsa_d8_block_rows() { return D8_RB; }
int mhsa_d8_block_threads() { return D8_THREADS; }

// B, N, heads > 0, 16-byte aligned buffers, launches below 2^31 work-items: checked by the caller (capi.hip)
int mhsa_d8_launch(const void* qkv, void* out, int B, int N, int heads, float scale, int dtype, hipStream_t stream) {
    const int blocks = (N + D8_RB - 1) / D8_RB;
    const dim3 grid((unsigned)((long long)B * heads * blocks)), thr(D8_THREADS);
    if (dtype == 0)
        hipLaunchKernelGGL(mhsa_d8_fwd_kernel<float>, grid, thr, 0, stream, (const float*)qkv, (float*)out, N, heads, blocks, scale);
    else
        hipLaunchKernelGGL(mhsa_d8_fwd_kernel<__bf16>, grid, thr, 0, stream, (const __bf16*)qkv, (__bf16*)out, N, heads, blocks, scale);
    return (int)hipGetLastError();
}

// the workspace is mhsa_bwd_workspace_floats(B, N, heads) = 2 B heads N floats: L2 | delta
template <typename T>
static int d8_bwd(const void* qkv, const void* out, const void* dout, void* dqkv, float* ws, int B, int N, int heads, float scale,
                  hipStream_t stream) {
    float* lse = ws;
    float* delta = ws + (size_t)B * heads * N;
    const int blocks = (N + D8_RB - 1) / D8_RB;
    const dim3 grid((unsigned)((long long)B * heads * blocks)), thr(D8_THREADS);
    hipLaunchKernelGGL(mhsa_d8_stats_kernel<T>, grid, thr, 0, stream, (const T*)qkv, (const T*)out, (const T*)dout, lse, delta, N, heads, blocks,
                       scale);
    hipLaunchKernelGGL(mhsa_d8_dkdv_kernel<T>, grid, thr, 0, stream, (const T*)qkv, (const T*)dout, (const float*)lse, (const float*)delta,
                       (T*)dqkv, N, heads, blocks, scale);
    hipLaunchKernelGGL(mhsa_d8_dq_kernel<T>, grid, thr, 0, stream, (const T*)qkv, (const T*)dout, (const float*)lse, (const float*)delta, (T*)dqkv,
                       N, heads, blocks, scale);
    return (int)hipGetLastError();
}

int mhsa_d8_bwd_launch(const void* qkv, const void* out, const void* dout, void* dqkv, float* ws, int B, int N, int heads, float scale, int dtype,
                       hipStream_t stream) {
    return dtype == 0 ? d8_bwd<float>(qkv, out, dout, dqkv, ws, B, N, heads, scale, stream)
                      : d8_bwd<__bf16>(qkv, out, dout, dqkv, ws, B, N, heads, scale, stream);
}

}  // namespace ppn
