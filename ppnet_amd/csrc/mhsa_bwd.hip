// mhsa_bwd.hip — global multi-head self-attention, backward: the gradient of out = softmax(scale q k^T) v per (batch, head) in
// ppn_mhsa_fwd's layouts (mhsa.hip): qkv and dqkv [B][N][3][heads][64], out and dout [B][N][heads][64].
//
//   P = softmax(scale S), S = q k^T;  dV = P^T dO;  dP = dO V^T;  delta = rowsum(dO o O);  dS = P o (dP - delta);
//   dQ = scale dS K;  dK = scale dS^T Q.
//
// Nothing of size N x N touches memory: P is recomputed from q, k and one number per query.  Three passes, every output element
// written by exactly one workgroup (no atomics, no hand-off between workgroups: the gradients are bitwise reproducible):
//
//   statistics  per (b, h, query): the log-sum-exp of the scaled logits and delta, into the caller's workspace
//               ([2][B][heads][N] float32).  The forward kernel keeps neither, and mhsa.hip is not touched: like ppn_na2d_bwd the
//               backward recomputes what it needs.
//   dK / dV     one workgroup per (b, h, block of keys); the block's K and V stay in registers, dK^T and dV^T accumulate in
//               registers while the workgroup sweeps all query tiles (Q, dO and the two statistics staged through LDS).
//   dQ          one workgroup per (b, h, block of queries) sweeping all key tiles (K, V through LDS), like the forward.
//
//   bfloat16: v_mfma_f32_16x16x32_bf16, float32 accumulation and softmax arithmetic, 4 waves per workgroup, tiles of 64 staged in
//             LDS (double-buffered, one barrier per tile).  The statistic is kept in the exp2 domain (L2 = log2 sum 2^(c S),
//             c = scale log2 e), so p = exp2(c S - L2) needs no maximum.  In the dK / dV pass the key sits on the MFMA column
//             (S = Q K^T, dP = dO V^T with K, V as B operands), so the P and dS accumulators are, rounded to bfloat16 once, directly
//             the B operands of dV^T += dO^T P and dK^T += Q^T dS; dO^T and Q^T come out of the same LDS image by
//             ds_read_b64_tr_b16.  The dQ pass mirrors it with the query on the column (S^T = K Q^T, dP^T = V dO^T,
//             dQ^T += K^T dS^T), as the forward does.  Tail keys contribute nothing; tail queries are neither summed nor stored.
//   float32:  plain VALU kernels (the parity path), two lanes per query (or key), each owning 32 of the 64 dims: the two halves of
//             a dot product meet through one lane exchange; sums over a tile are formed apart before they join the running ones.
//
// Element offsets are 64-bit; the caller (capi.hip) rejects launches of 2^31 work-items or more.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include "ppn_device.h"
#include "ppn_kernels.h"

namespace ppn {

namespace {
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
constexpr int HD = 64;                         // head dim
constexpr int KT = 64;                         // rows (keys or queries) per LDS tile
constexpr int BW_WAVES = 4, BW_RW = 32;        // waves per workgroup, rows (queries or keys) a wave owns
constexpr int BW_RB = BW_WAVES * BW_RW;        // rows a workgroup owns (bfloat16)
constexpr int PITCH = 144;                     // LDS row pitch in bytes (128 + 16: rows start 4 banks apart)
constexpr int TILE_BYTES = KT * PITCH;
constexpr int F32_RB = 64, F32_THREADS = 128;  // float32: rows per workgroup, two lanes per row
constexpr float LOG2E = 1.4426950408889634f;
constexpr float ABSENT = -1.0e30f;             // logit of a key that does not exist

// rows 32 ks .. 32 ks + 31 of an LDS image [row][64 bf16] as the A operand of a product over rows: operand row = dim 16 cb + j,
// k slot (g, e) = row 32 ks + 16 (e >> 2) + 4 g + (e & 3) — the order in which two S accumulators packed side by side hold them
__device__ __forceinline__ bf16x8 read_transposed(const unsigned char* img, int ks, int cb, int g, int q4, int p4) {
    const unsigned char* a = img + (32 * ks + 4 * g + q4) * PITCH + 8 * p4 + cb * 32;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a + 16 * PITCH));
    const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
}

__device__ __forceinline__ bf16x8 pack8(const f32x4 a, const f32x4 b) {
    return bf16x8{(__bf16)a[0], (__bf16)a[1], (__bf16)a[2], (__bf16)a[3], (__bf16)b[0], (__bf16)b[1], (__bf16)b[2], (__bf16)b[3]};
}

}  // namespace

// ================================================================================================ bfloat16, matrix cores
// ------------------------------------------------------------------------------------------------ statistics
// One workgroup per (b, h, 128 queries); S^T = K Q^T as in the forward (a query's keys in one lane column).  Every lane keeps a
// running maximum and sum over its own 16 keys of each tile; the query's four lanes join once, after the last tile.
__global__ __launch_bounds__(64 * BW_WAVES) void mhsa_bwd_stats_bf16_kernel(const __bf16* __restrict__ qkv, const __bf16* __restrict__ out,
                                                                           const __bf16* __restrict__ dout, float* __restrict__ lse2,
                                                                           float* __restrict__ delta, int N, int heads, int qblocks, float scale) {
    __shared__ __attribute__((aligned(16))) unsigned char k_lds[2][TILE_BYTES];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int j = lane & 15, g = lane >> 4;
    const int qb = (int)(blockIdx.x % (unsigned)qblocks);
    const int bh = (int)(blockIdx.x / (unsigned)qblocks);
    const int h = bh % heads, b = bh / heads;
    const size_t rowb = (size_t)3 * heads * HD * 2, outb = (size_t)heads * HD * 2;
    const unsigned char* base = reinterpret_cast<const unsigned char*>(qkv) + (size_t)b * N * rowb;
    const size_t qoff = (size_t)h * HD * 2, koff = (size_t)(heads + h) * HD * 2;

    const int q0 = qb * BW_RB + wave * BW_RW;
    bf16x8 qf[2][2];
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
        const int q = q0 + 16 * sb + j;
#pragma unroll
        for (int st = 0; st < 2; ++st)
            qf[sb][st] = q < N ? *reinterpret_cast<const bf16x8*>(base + (size_t)q * rowb + qoff + 16 * g + 64 * st) : bf16x8{};
    }

    // staging: 64 keys x 8 pieces of 16 bytes = 512 pieces, 2 per thread; keys past N are zeros
    const int ntiles = (N + KT - 1) / KT;
    uint4 stage[2];
    auto fetch = [&](int tile) {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int c = it * 256 + (int)threadIdx.x, key = c >> 3, ch = c & 7;
            const int n = tile * KT + key;
            stage[it] = n < N ? *reinterpret_cast<const uint4*>(base + (size_t)n * rowb + koff + 16 * ch) : make_uint4(0, 0, 0, 0);
        }
    };
    auto put = [&](int buf) {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int c = it * 256 + (int)threadIdx.x, key = c >> 3, ch = c & 7;
            *reinterpret_cast<uint4*>(&k_lds[buf][key * PITCH + 16 * ch]) = stage[it];
        }
    };
    fetch(0);
    put(0);
    __syncthreads();

    const float sl2 = scale * LOG2E;
    float m[2] = {ABSENT, ABSENT}, l[2] = {0.0f, 0.0f};
    for (int tile = 0; tile < ntiles; ++tile) {
        const int buf = tile & 1;
        if (tile + 1 < ntiles) fetch(tile + 1);
        const unsigned char* kl = k_lds[buf];
        bf16x8 kf[4][2];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int st = 0; st < 2; ++st) kf[t][st] = *reinterpret_cast<const bf16x8*>(kl + (16 * t + j) * PITCH + 16 * g + 64 * st);
        const int kvalid = N - tile * KT;
#pragma unroll
        for (int sb = 0; sb < 2; ++sb) {
            f32x4 s[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[t][0], qf[sb][0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[t][1], qf[sb][1], s[t], 0, 0, 0);
            }
            if (kvalid < KT) {
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int e = 0; e < 4; ++e) s[t][e] = 16 * t + 4 * g + e < kvalid ? s[t][e] : ABSENT;
            }
            float mx = m[sb];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) mx = fmaxf(mx, s[t][e]);
            // (s - mx) first: a lane whose keys so far are all absent has s = mx = ABSENT, and fma(s, c, -mx c) would leave the
            // product's rounding error (1e22) in the exponent
            float lt = 0.0f;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) lt += __builtin_amdgcn_exp2f((s[t][e] - mx) * sl2);
            l[sb] = __builtin_fmaf(l[sb], __builtin_amdgcn_exp2f((m[sb] - mx) * sl2), lt);
            m[sb] = mx;
        }
        if (tile + 1 < ntiles) put(buf ^ 1);
        __syncthreads();
    }

    const unsigned char* oc = reinterpret_cast<const unsigned char*>(out) + (size_t)b * N * outb + (size_t)h * HD * 2;
    const unsigned char* dc = reinterpret_cast<const unsigned char*>(dout) + (size_t)b * N * outb + (size_t)h * HD * 2;
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
        const int q = q0 + 16 * sb + j;
        // the query's four lanes (lane ^ 16, lane ^ 32): a lane whose keys were all absent holds m = ABSENT and adds 0
        float mq = fmaxf(m[sb], __shfl_xor(m[sb], 16));
        mq = fmaxf(mq, __shfl_xor(mq, 32));
        float lq = l[sb] * __builtin_amdgcn_exp2f((m[sb] - mq) * sl2);
        lq += __shfl_xor(lq, 16);
        lq += __shfl_xor(lq, 32);
        // delta on the matrix core, with dO and the dims in the k slots the dP products of the two other passes use: where O = V
        // (one key) dP - delta is then exactly 0.  O rows x dO columns; the diagonal element of query j is row 4 g + e = j
        f32x4 dd = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            const bf16x8 oa = q < N ? *reinterpret_cast<const bf16x8*>(oc + (size_t)q * outb + 16 * g + 64 * st) : bf16x8{};
            const bf16x8 db = q < N ? *reinterpret_cast<const bf16x8*>(dc + (size_t)q * outb + 16 * g + 64 * st) : bf16x8{};
            dd = __builtin_amdgcn_mfma_f32_16x16x32_bf16(oa, db, dd, 0, 0, 0);
        }
        const int e = j & 3;
        const float dl = e == 0 ? dd[0] : e == 1 ? dd[1] : e == 2 ? dd[2] : dd[3];
        if (q < N && g == 0) lse2[(size_t)bh * N + q] = __builtin_fmaf(mq, sl2, log2f(lq));
        if (q < N && g == (j >> 2)) delta[(size_t)bh * N + q] = dl;
    }
}

// ------------------------------------------------------------------------------------------------ dK, dV
// One workgroup per (b, h, 128 keys), each wave 32 keys (two 16-key MFMA tiles) held as B operands; query tiles of 64 through LDS.
__global__ __launch_bounds__(64 * BW_WAVES) void mhsa_bwd_dkdv_bf16_kernel(const __bf16* __restrict__ qkv, const __bf16* __restrict__ dout,
                                                                          const float* __restrict__ lse2, const float* __restrict__ delta,
                                                                          __bf16* __restrict__ dqkv, int N, int heads, int kblocks, float scale) {
    __shared__ __attribute__((aligned(16))) unsigned char qd_lds[2][2][TILE_BYTES];   // [buffer][Q, dO][query row]
    __shared__ __attribute__((aligned(16))) float st_lds[2][2][KT];                   // [buffer][L2, delta][query]
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int j = lane & 15, g = lane >> 4, q4 = j >> 2, p4 = j & 3;
    const int kb = (int)(blockIdx.x % (unsigned)kblocks);
    const int bh = (int)(blockIdx.x / (unsigned)kblocks);
    const int h = bh % heads, b = bh / heads;
    const size_t rowb = (size_t)3 * heads * HD * 2, outb = (size_t)heads * HD * 2;
    const unsigned char* base = reinterpret_cast<const unsigned char*>(qkv) + (size_t)b * N * rowb;
    const unsigned char* dbase = reinterpret_cast<const unsigned char*>(dout) + (size_t)b * N * outb + (size_t)h * HD * 2;
    const float* lrow = lse2 + (size_t)bh * N;
    const float* drow = delta + (size_t)bh * N;
    const size_t qoff = (size_t)h * HD * 2, koff = (size_t)(heads + h) * HD * 2, voff = (size_t)(2 * heads + h) * HD * 2;

    // K and V of this wave's two 16-key tiles as MFMA B operands: column = key, k = dims 8 g .. 8 g + 7 (+ 32 on the second step)
    const int k0 = kb * BW_RB + wave * BW_RW;
    bf16x8 kf[2][2], vf[2][2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
        const int key = k0 + 16 * kt + j;
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            kf[kt][st] = key < N ? *reinterpret_cast<const bf16x8*>(base + (size_t)key * rowb + koff + 16 * g + 64 * st) : bf16x8{};
            vf[kt][st] = key < N ? *reinterpret_cast<const bf16x8*>(base + (size_t)key * rowb + voff + 16 * g + 64 * st) : bf16x8{};
        }
    }

    // staging: 64 queries x (Q, dO) x 8 pieces of 16 bytes = 1024 pieces, 4 per thread, and 2 x 64 statistics; queries past N
    // are zero rows with delta 0 and a statistic that makes their p exactly 0
    const int ntiles = (N + KT - 1) / KT;
    uint4 stage[4];
    float sstat = 0.0f;
    auto fetch = [&](int tile) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int c = it * 256 + (int)threadIdx.x, row = c >> 4, part = (c >> 3) & 1, ch = c & 7;
            const int n = tile * KT + row;
            stage[it] = n < N ? *reinterpret_cast<const uint4*>(part ? dbase + (size_t)n * outb + 16 * ch : base + (size_t)n * rowb + qoff + 16 * ch)
                              : make_uint4(0, 0, 0, 0);
        }
        if (threadIdx.x < 2 * KT) {
            const int which = (int)threadIdx.x >> 6, n = tile * KT + ((int)threadIdx.x & 63);
            sstat = n < N ? (which ? drow[n] : lrow[n]) : (which ? 0.0f : -ABSENT);
        }
    };
    auto put = [&](int buf) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int c = it * 256 + (int)threadIdx.x, row = c >> 4, part = (c >> 3) & 1, ch = c & 7;
            *reinterpret_cast<uint4*>(&qd_lds[buf][part][row * PITCH + 16 * ch]) = stage[it];
        }
        if (threadIdx.x < 2 * KT) st_lds[buf][(int)threadIdx.x >> 6][(int)threadIdx.x & 63] = sstat;
    };
    fetch(0);
    put(0);
    __syncthreads();

    const float sl2 = scale * LOG2E;
    f32x4 dkT[2][4], dvT[2][4];                    // [key tile][dims 16 cb ..]: row = dim 16 cb + 4 g + e, column = key j
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) dkT[kt][cb] = dvT[kt][cb] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int tile = 0; tile < ntiles; ++tile) {
        const int buf = tile & 1;
        if (tile + 1 < ntiles) fetch(tile + 1);
        const unsigned char* ql = qd_lds[buf][0];
        const unsigned char* dl = qd_lds[buf][1];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {          // 32 queries: two 16-query MFMA tiles t = 2 ks, 2 ks + 1
            bf16x8 qa[2][2], da[2][2], qT[4], dT[4];
            f32x4 L[2], D[2];
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                const int r = 16 * (2 * ks + tt);
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    qa[tt][st] = *reinterpret_cast<const bf16x8*>(ql + (r + j) * PITCH + 16 * g + 64 * st);
                    da[tt][st] = *reinterpret_cast<const bf16x8*>(dl + (r + j) * PITCH + 16 * g + 64 * st);
                }
                L[tt] = *reinterpret_cast<const f32x4*>(&st_lds[buf][0][r + 4 * g]);      // queries r + 4 g + e: the accumulator's rows
                D[tt] = *reinterpret_cast<const f32x4*>(&st_lds[buf][1][r + 4 * g]);
            }
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                qT[cb] = read_transposed(ql, ks, cb, g, q4, p4);
                dT[cb] = read_transposed(dl, ks, cb, g, q4, p4);
            }
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                f32x4 s[2], dp[2];
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {
                    s[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[tt][0], kf[kt][0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                    s[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[tt][1], kf[kt][1], s[tt], 0, 0, 0);
                    dp[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(da[tt][0], vf[kt][0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                    dp[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(da[tt][1], vf[kt][1], dp[tt], 0, 0, 0);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        s[tt][e] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[tt][e], sl2, -L[tt][e]));    // p
                        dp[tt][e] = s[tt][e] * (dp[tt][e] - D[tt][e]);                                 // dS
                    }
                }
                const bf16x8 pf = pack8(s[0], s[1]), dsf = pack8(dp[0], dp[1]);
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) {
                    dvT[kt][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dT[cb], pf, dvT[kt][cb], 0, 0, 0);
                    dkT[kt][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qT[cb], dsf, dkT[kt][cb], 0, 0, 0);
                }
            }
        }
        if (tile + 1 < ntiles) put(buf ^ 1);
        __syncthreads();
    }

    unsigned char* gbase = reinterpret_cast<unsigned char*>(dqkv) + (size_t)b * N * rowb;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
        const int key = k0 + 16 * kt + j;
        if (key < N) {
            unsigned char* dk = gbase + (size_t)key * rowb + koff + 8 * g;
            unsigned char* dv = gbase + (size_t)key * rowb + voff + 8 * g;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                *reinterpret_cast<uint2*>(dk + cb * 32) = make_uint2(pack_bf16x2(dkT[kt][cb][0] * scale, dkT[kt][cb][1] * scale),
                                                                     pack_bf16x2(dkT[kt][cb][2] * scale, dkT[kt][cb][3] * scale));
                *reinterpret_cast<uint2*>(dv + cb * 32) = make_uint2(pack_bf16x2(dvT[kt][cb][0], dvT[kt][cb][1]),
                                                                     pack_bf16x2(dvT[kt][cb][2], dvT[kt][cb][3]));
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ dQ
// One workgroup per (b, h, 128 queries), each wave 32 queries with Q and dO as B operands; key tiles of 64 (K, V) through LDS.
__global__ __launch_bounds__(64 * BW_WAVES) void mhsa_bwd_dq_bf16_kernel(const __bf16* __restrict__ qkv, const __bf16* __restrict__ dout,
                                                                        const float* __restrict__ lse2, const float* __restrict__ delta,
                                                                        __bf16* __restrict__ dqkv, int N, int heads, int qblocks, float scale) {
    __shared__ __attribute__((aligned(16))) unsigned char kv_lds[2][2][TILE_BYTES];   // [buffer][K, V][key row]
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int j = lane & 15, g = lane >> 4, q4 = j >> 2, p4 = j & 3;
    const int qb = (int)(blockIdx.x % (unsigned)qblocks);
    const int bh = (int)(blockIdx.x / (unsigned)qblocks);
    const int h = bh % heads, b = bh / heads;
    const size_t rowb = (size_t)3 * heads * HD * 2, outb = (size_t)heads * HD * 2;
    const unsigned char* base = reinterpret_cast<const unsigned char*>(qkv) + (size_t)b * N * rowb;
    const unsigned char* dbase = reinterpret_cast<const unsigned char*>(dout) + (size_t)b * N * outb + (size_t)h * HD * 2;
    const size_t qoff = (size_t)h * HD * 2, koff = (size_t)(heads + h) * HD * 2, voff = (size_t)(2 * heads + h) * HD * 2;

    const int q0 = qb * BW_RB + wave * BW_RW;
    bf16x8 qf[2][2], df[2][2];
    float Lq[2], Dq[2];
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
        const int q = q0 + 16 * sb + j;
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            qf[sb][st] = q < N ? *reinterpret_cast<const bf16x8*>(base + (size_t)q * rowb + qoff + 16 * g + 64 * st) : bf16x8{};
            df[sb][st] = q < N ? *reinterpret_cast<const bf16x8*>(dbase + (size_t)q * outb + 16 * g + 64 * st) : bf16x8{};
        }
        Lq[sb] = q < N ? lse2[(size_t)bh * N + q] : 0.0f;
        Dq[sb] = q < N ? delta[(size_t)bh * N + q] : 0.0f;
    }

    const int ntiles = (N + KT - 1) / KT;
    uint4 stage[4];
    auto fetch = [&](int tile) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int c = it * 256 + (int)threadIdx.x, key = c >> 4, part = (c >> 3) & 1, ch = c & 7;
            const int n = tile * KT + key;
            stage[it] = n < N ? *reinterpret_cast<const uint4*>(base + (size_t)n * rowb + (part ? voff : koff) + 16 * ch) : make_uint4(0, 0, 0, 0);
        }
    };
    auto put = [&](int buf) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int c = it * 256 + (int)threadIdx.x, key = c >> 4, part = (c >> 3) & 1, ch = c & 7;
            *reinterpret_cast<uint4*>(&kv_lds[buf][part][key * PITCH + 16 * ch]) = stage[it];
        }
    };
    fetch(0);
    put(0);
    __syncthreads();

    const float sl2 = scale * LOG2E;
    f32x4 dqT[2][4];                               // row = dim 16 cb + 4 g + e, column = query j
#pragma unroll
    for (int sb = 0; sb < 2; ++sb)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) dqT[sb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int tile = 0; tile < ntiles; ++tile) {
        const int buf = tile & 1;
        if (tile + 1 < ntiles) fetch(tile + 1);
        const unsigned char* kl = kv_lds[buf][0];
        const unsigned char* vl = kv_lds[buf][1];
        const int kvalid = N - tile * KT;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {          // 32 keys: two 16-key MFMA tiles
            bf16x8 ka[2][2], va[2][2], kT[4];
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                const int r = 16 * (2 * ks + tt);
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    ka[tt][st] = *reinterpret_cast<const bf16x8*>(kl + (r + j) * PITCH + 16 * g + 64 * st);
                    va[tt][st] = *reinterpret_cast<const bf16x8*>(vl + (r + j) * PITCH + 16 * g + 64 * st);
                }
            }
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) kT[cb] = read_transposed(kl, ks, cb, g, q4, p4);
#pragma unroll
            for (int sb = 0; sb < 2; ++sb) {
                f32x4 s[2], dp[2];
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {
                    s[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka[tt][0], qf[sb][0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                    s[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka[tt][1], qf[sb][1], s[tt], 0, 0, 0);
                    dp[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va[tt][0], df[sb][0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                    dp[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va[tt][1], df[sb][1], dp[tt], 0, 0, 0);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[tt][e], sl2, -Lq[sb]));
                        const float ds = p * (dp[tt][e] - Dq[sb]);
                        dp[tt][e] = 16 * (2 * ks + tt) + 4 * g + e < kvalid ? ds : 0.0f;              // absent keys add nothing
                    }
                }
                const bf16x8 dsf = pack8(dp[0], dp[1]);
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) dqT[sb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kT[cb], dsf, dqT[sb][cb], 0, 0, 0);
            }
        }
        if (tile + 1 < ntiles) put(buf ^ 1);
        __syncthreads();
    }

    unsigned char* gbase = reinterpret_cast<unsigned char*>(dqkv) + (size_t)b * N * rowb + qoff;
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
        const int q = q0 + 16 * sb + j;
        if (q < N) {
            unsigned char* dst = gbase + (size_t)q * rowb + 8 * g;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
                *reinterpret_cast<uint2*>(dst + cb * 32) = make_uint2(pack_bf16x2(dqT[sb][cb][0] * scale, dqT[sb][cb][1] * scale),
                                                                      pack_bf16x2(dqT[sb][cb][2] * scale, dqT[sb][cb][3] * scale));
        }
    }
}

// ================================================================================================ float32, VALU (parity path)
// 128 threads own 64 rows: thread = (wave w, row w * 32 + (lane & 31), half = lane >> 5) holds dims 32 half .. 32 half + 31 of
// its row; a 64-term dot product is the sum of the two halves' 32 terms, exchanged with lane ^ 32 (both lanes get the same bits).
namespace {
struct F32Id {
    int row, d0;
};
__device__ __forceinline__ F32Id f32_id() {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    return F32Id{w * 32 + (lane & 31), (lane >> 5) * 32};
}
__device__ __forceinline__ void load32(float* r, const float* src, bool valid) {
#pragma unroll
    for (int d = 0; d < 32; d += 4) {
        const float4 v = valid ? *reinterpret_cast<const float4*>(src + d) : make_float4(0.f, 0.f, 0.f, 0.f);
        r[d] = v.x; r[d + 1] = v.y; r[d + 2] = v.z; r[d + 3] = v.w;
    }
}
// a tile of up to 64 rows x 64 floats, rows `src + n * stride`, into LDS [row][64]; rows past `rows` are zeros
__device__ __forceinline__ void stage_f32(float* lds, const float* src, size_t stride, int rows) {
    for (int i = threadIdx.x; i < KT * 16; i += F32_THREADS) {
        const int r = i >> 4, c4 = i & 15;
        const float4 v = r < rows ? *reinterpret_cast<const float4*>(src + (size_t)r * stride + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(&lds[r * HD + 4 * c4]) = v;
    }
}
__device__ __forceinline__ float half_dot(const float* r, const float* lds_row) {
    float acc = 0.0f;
#pragma unroll
    for (int d = 0; d < 32; ++d) acc = __builtin_fmaf(r[d], lds_row[d], acc);
    return acc + __shfl_xor(acc, 32);
}
}  // namespace

// statistics: L = log sum exp(scale S) (natural logarithm: this path uses expf, as the forward's does) and delta
__global__ __launch_bounds__(F32_THREADS) void mhsa_bwd_stats_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ out,
                                                                        const float* __restrict__ dout, float* __restrict__ lse,
                                                                        float* __restrict__ delta, int N, int heads, int qblocks, float scale) {
    __shared__ __attribute__((aligned(16))) float kt_lds[KT * HD];
    __shared__ float sc[KT * F32_THREADS];                            // logits [key][thread]
    const F32Id id = f32_id();
    const int qb = (int)(blockIdx.x % (unsigned)qblocks);
    const int bh = (int)(blockIdx.x / (unsigned)qblocks);
    const int h = bh % heads, b = bh / heads;
    const size_t row = (size_t)3 * heads * HD, C = (size_t)heads * HD;
    const float* base = qkv + (size_t)b * N * row;
    const int q = qb * F32_RB + id.row;
    const bool qvalid = q < N;
    float qv[32];
    load32(qv, base + (size_t)(qvalid ? q : 0) * row + (size_t)h * HD + id.d0, qvalid);
    float m = -3.0e38f, l = 0.0f;
    for (int k0 = 0; k0 < N; k0 += KT) {
        const int kn = N - k0 < KT ? N - k0 : KT;
        stage_f32(kt_lds, base + (size_t)k0 * row + C + (size_t)h * HD, row, kn);
        __syncthreads();
        float mx = m;
        for (int k = 0; k < kn; ++k) {
            const float s = half_dot(qv, &kt_lds[k * HD + id.d0]) * scale;
            sc[k * F32_THREADS + threadIdx.x] = s;
            mx = fmaxf(mx, s);
        }
        const float alpha = expf(m - mx);
        m = mx;
        float lt = 0.0f;
        for (int k = 0; k < kn; ++k) lt += expf(sc[k * F32_THREADS + threadIdx.x] - m);
        l = __builtin_fmaf(l, alpha, lt);
        __syncthreads();
    }
    float dov[32];
    const size_t orow = ((size_t)b * N + (qvalid ? q : 0)) * C + (size_t)h * HD + id.d0;
    load32(dov, dout + orow, qvalid);
    const float dl = half_dot(dov, out + orow);                        // the lane exchange needs every lane: a tail row reads row 0
    if (qvalid && id.d0 == 0) {
        lse[(size_t)bh * N + q] = m + logf(l);
        delta[(size_t)bh * N + q] = dl;
    }
}

// dK, dV: one workgroup per (b, h, 64 keys); query tiles of 64 (Q, dO, statistics) through LDS
__global__ __launch_bounds__(F32_THREADS) void mhsa_bwd_dkdv_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                                       const float* __restrict__ lse, const float* __restrict__ delta,
                                                                       float* __restrict__ dqkv, int N, int heads, int kblocks, float scale) {
    __shared__ __attribute__((aligned(16))) float qd_lds[2][KT * HD];   // [Q, dO][query][dim]
    __shared__ float st_lds[2][KT];                                     // [L, delta][query]
    const F32Id id = f32_id();
    const int kb = (int)(blockIdx.x % (unsigned)kblocks);
    const int bh = (int)(blockIdx.x / (unsigned)kblocks);
    const int h = bh % heads, b = bh / heads;
    const size_t row = (size_t)3 * heads * HD, C = (size_t)heads * HD;
    const float* base = qkv + (size_t)b * N * row;
    const float* dbase = dout + (size_t)b * N * C + (size_t)h * HD;
    const int key = kb * F32_RB + id.row;
    const bool kvalid = key < N;
    float kv[32], vv[32], dk[32], dv[32];
    load32(kv, base + (size_t)(kvalid ? key : 0) * row + C + (size_t)h * HD + id.d0, kvalid);
    load32(vv, base + (size_t)(kvalid ? key : 0) * row + 2 * C + (size_t)h * HD + id.d0, kvalid);
#pragma unroll
    for (int d = 0; d < 32; ++d) dk[d] = dv[d] = 0.0f;
    for (int q0 = 0; q0 < N; q0 += KT) {
        const int qn = N - q0 < KT ? N - q0 : KT;
        stage_f32(qd_lds[0], base + (size_t)q0 * row + (size_t)h * HD, row, qn);
        stage_f32(qd_lds[1], dbase + (size_t)q0 * C, C, qn);
        if (threadIdx.x < 2 * KT) {
            const int which = threadIdx.x >> 6, i = threadIdx.x & 63;
            st_lds[which][i] = i < qn ? (which ? delta : lse)[(size_t)bh * N + q0 + i] : 0.0f;
        }
        __syncthreads();
        // the tile's sums apart, then folded in: rounding grows with 64 + N / 64 terms, not N
        float dkt[32], dvt[32];
#pragma unroll
        for (int d = 0; d < 32; ++d) dkt[d] = dvt[d] = 0.0f;
        for (int i = 0; i < qn; ++i) {
            const float* qr = &qd_lds[0][i * HD + id.d0];
            const float* dr = &qd_lds[1][i * HD + id.d0];
            const float s = half_dot(kv, qr), dp = half_dot(vv, dr);
            const float p = expf(s * scale - st_lds[0][i]);             // the statistics pass rounds s * scale the same way
            const float ds = p * (dp - st_lds[1][i]);
#pragma unroll
            for (int d = 0; d < 32; ++d) {
                dvt[d] = __builtin_fmaf(p, dr[d], dvt[d]);
                dkt[d] = __builtin_fmaf(ds, qr[d], dkt[d]);
            }
        }
#pragma unroll
        for (int d = 0; d < 32; ++d) {
            dk[d] += dkt[d];
            dv[d] += dvt[d];
        }
        __syncthreads();
    }
    if (!kvalid) return;
    float* gk = dqkv + ((size_t)b * N + key) * row + C + (size_t)h * HD + id.d0;
    float* gv = gk + C;
#pragma unroll
    for (int d = 0; d < 32; d += 4) {
        *reinterpret_cast<float4*>(gk + d) = make_float4(dk[d] * scale, dk[d + 1] * scale, dk[d + 2] * scale, dk[d + 3] * scale);
        *reinterpret_cast<float4*>(gv + d) = make_float4(dv[d], dv[d + 1], dv[d + 2], dv[d + 3]);
    }
}

// dQ: one workgroup per (b, h, 64 queries); key tiles of 64 (K, V) through LDS
__global__ __launch_bounds__(F32_THREADS) void mhsa_bwd_dq_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                                     const float* __restrict__ lse, const float* __restrict__ delta,
                                                                     float* __restrict__ dqkv, int N, int heads, int qblocks, float scale) {
    __shared__ __attribute__((aligned(16))) float kv_lds[2][KT * HD];   // [K, V][key][dim]
    const F32Id id = f32_id();
    const int qb = (int)(blockIdx.x % (unsigned)qblocks);
    const int bh = (int)(blockIdx.x / (unsigned)qblocks);
    const int h = bh % heads, b = bh / heads;
    const size_t row = (size_t)3 * heads * HD, C = (size_t)heads * HD;
    const float* base = qkv + (size_t)b * N * row;
    const int q = qb * F32_RB + id.row;
    const bool qvalid = q < N;
    float qv[32], dov[32], dq[32];
    load32(qv, base + (size_t)(qvalid ? q : 0) * row + (size_t)h * HD + id.d0, qvalid);
    load32(dov, dout + ((size_t)b * N + (qvalid ? q : 0)) * C + (size_t)h * HD + id.d0, qvalid);
    const float L = qvalid ? lse[(size_t)bh * N + q] : 0.0f, D = qvalid ? delta[(size_t)bh * N + q] : 0.0f;
#pragma unroll
    for (int d = 0; d < 32; ++d) dq[d] = 0.0f;
    for (int k0 = 0; k0 < N; k0 += KT) {
        const int kn = N - k0 < KT ? N - k0 : KT;
        stage_f32(kv_lds[0], base + (size_t)k0 * row + C + (size_t)h * HD, row, kn);
        stage_f32(kv_lds[1], base + (size_t)k0 * row + 2 * C + (size_t)h * HD, row, kn);
        __syncthreads();
        float dqt[32];
#pragma unroll
        for (int d = 0; d < 32; ++d) dqt[d] = 0.0f;
        for (int k = 0; k < kn; ++k) {
            const float* kr = &kv_lds[0][k * HD + id.d0];
            const float s = half_dot(qv, kr), dp = half_dot(dov, &kv_lds[1][k * HD + id.d0]);
            const float ds = expf(s * scale - L) * (dp - D);
#pragma unroll
            for (int d = 0; d < 32; ++d) dqt[d] = __builtin_fmaf(ds, kr[d], dqt[d]);
        }
#pragma unroll
        for (int d = 0; d < 32; ++d) dq[d] += dqt[d];
        __syncthreads();
    }
    if (!qvalid) return;
    float* gq = dqkv + ((size_t)b * N + q) * row + (size_t)h * HD + id.d0;
#pragma unroll
    for (int d = 0; d < 32; d += 4) *reinterpret_cast<float4*>(gq + d) = make_float4(dq[d] * scale, dq[d + 1] * scale, dq[d + 2] * scale, dq[d + 3] * scale);
}

// ================================================================================================ host
long long mhsa_bwd_workspace_floats(int B, int N, int heads) { return 2LL * B * heads * N; }

// B, N, heads > 0, 16-byte aligned buffers, a workspace of mhsa_bwd_workspace_floats, launches below 2^31 work-items: checked by
// the caller (capi.hip)
int mhsa_bwd_launch(const void* qkv, const void* out, const void* dout, void* dqkv, float* ws, int B, int N, int heads, float scale, int dtype,
                    hipStream_t stream) {
    float* lse = ws;
    float* delta = ws + (size_t)B * heads * N;
    if (dtype == 0) {
        const int blocks = (N + F32_RB - 1) / F32_RB;
        const dim3 grid((unsigned)((long long)B * heads * blocks)), thr(F32_THREADS);
        hipLaunchKernelGGL(mhsa_bwd_stats_f32_kernel, grid, thr, 0, stream, (const float*)qkv, (const float*)out, (const float*)dout, lse, delta, N,
                           heads, blocks, scale);
        hipLaunchKernelGGL(mhsa_bwd_dkdv_f32_kernel, grid, thr, 0, stream, (const float*)qkv, (const float*)dout, (const float*)lse,
                           (const float*)delta, (float*)dqkv, N, heads, blocks, scale);
        hipLaunchKernelGGL(mhsa_bwd_dq_f32_kernel, grid, thr, 0, stream, (const float*)qkv, (const float*)dout, (const float*)lse,
                           (const float*)delta, (float*)dqkv, N, heads, blocks, scale);
        return (int)hipGetLastError();
    }
    const int blocks = (N + BW_RB - 1) / BW_RB;
    const dim3 grid((unsigned)((long long)B * heads * blocks)), thr(64 * BW_WAVES);
    hipLaunchKernelGGL(mhsa_bwd_stats_bf16_kernel, grid, thr, 0, stream, (const __bf16*)qkv, (const __bf16*)out, (const __bf16*)dout, lse, delta,
                       N, heads, blocks, scale);
    hipLaunchKernelGGL(mhsa_bwd_dkdv_bf16_kernel, grid, thr, 0, stream, (const __bf16*)qkv, (const __bf16*)dout, (const float*)lse,
                       (const float*)delta, (__bf16*)dqkv, N, heads, blocks, scale);
    hipLaunchKernelGGL(mhsa_bwd_dq_bf16_kernel, grid, thr, 0, stream, (const __bf16*)qkv, (const __bf16*)dout, (const float*)lse,
                       (const float*)delta, (__bf16*)dqkv, N, heads, blocks, scale);
    return (int)hipGetLastError();
}

}  // namespace ppn
