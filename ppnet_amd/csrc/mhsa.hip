// mhsa.hip — global multi-head self-attention, forward: out[b, n, h, :] = softmax(scale q[b,n,h] . k[b,:,h]^T) . v[b,:,h], the sum
// over all N keys of the image (the body of nn.MultiheadAttention between in_proj and out_proj, as mmseg's VisionTransformer calls
// it through mmcv's MultiheadAttention: reference SegNet/mmseg/backbones/vit.py:63-70,92-95).
//
// qkv [B][N][3][heads][64] (one row per token: q | k | v, each [heads][64] — the order of nn.MultiheadAttention's in_proj_weight,
// so the qkv GEMM's output is read as it stands), out [B][N][heads][64].  Tail keys of the last key tile add nothing to the
// softmax; tail query slots are never stored.
//
//   bfloat16: flash-style, one workgroup per (batch, head, block of 128 queries), 4 waves of 32 queries (two 16-query MFMA tiles).
//             Q stays in registers as the B operand; K and V tiles of 64 keys are staged through LDS (double-buffered, one barrier
//             per tile).  S^T = K . Q^T puts a query's keys in one lane column, so the online softmax (float32 running max and
//             denominator per query, scale * log2 e folded into exp2) stays in registers; O^T = V^T . P^T takes the S^T registers
//             in place with V read by ds_read_b64_tr_b16, and the denominator is an all-ones MFMA over the same bf16 P.  The output
//             is rounded to bfloat16 once.
//   float32:  a plain VALU kernel (the parity path): one query per lane, K / V tiles of 64 keys in LDS, the same online softmax
//             with each tile's sums formed apart before they join the running ones.
//
// Element offsets are 64-bit; the launcher's caller (capi.hip) rejects grids of 2^31 work-items or more.
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
constexpr int KT = 64;                         // keys per LDS tile
constexpr int MH_WAVES = 4, MH_QW = 32;        // waves per workgroup, queries per wave
constexpr int MH_QB = MH_WAVES * MH_QW;        // queries per workgroup
constexpr int PITCH = 144;                     // LDS row pitch in bytes (128 + 16: rows start 4 banks apart)
constexpr int TILE_BYTES = KT * PITCH;
}  // namespace

// ------------------------------------------------------------------------------------------------ bfloat16, matrix cores
__global__ __launch_bounds__(64 * MH_WAVES, 2) void mhsa_bf16_kernel(const __bf16* __restrict__ qkv, __bf16* __restrict__ out, int N, int heads,
                                                                    int qblocks, float scale) {
    __shared__ __attribute__((aligned(16))) unsigned char kv_lds[2][2][TILE_BYTES];   // [buffer][K, V][key row]
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int j = lane & 15, g = lane >> 4, q4 = j >> 2, p4 = j & 3;
    const int qb = (int)(blockIdx.x % (unsigned)qblocks);
    const int bh = (int)(blockIdx.x / (unsigned)qblocks);
    const int h = bh % heads, b = bh / heads;
    const size_t rowb = (size_t)3 * heads * HD * 2, outb = (size_t)heads * HD * 2;      // bytes per qkv / out row
    const unsigned char* base = reinterpret_cast<const unsigned char*>(qkv) + (size_t)b * N * rowb;
    const size_t qoff = (size_t)h * HD * 2, koff = (size_t)(heads + h) * HD * 2, voff = (size_t)(2 * heads + h) * HD * 2;

    // Q of this wave's two 16-query tiles as MFMA B operands: column = query, k = dims 8 g .. 8 g + 7 (+ 32 on the second step)
    const int q0 = qb * MH_QB + wave * MH_QW;
    bf16x8 qf[2][2];
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
        const int q = q0 + 16 * sb + j;
#pragma unroll
        for (int st = 0; st < 2; ++st)
            qf[sb][st] = q < N ? *reinterpret_cast<const bf16x8*>(base + (size_t)q * rowb + qoff + 16 * g + 64 * st) : bf16x8{};
    }

    // staging: 64 keys x (K, V) x 8 pieces of 16 bytes = 1024 pieces, 4 per thread; keys past N are zeros
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

    const float sl2 = scale * 1.4426950408889634f;
    const bf16x8 ones = {(__bf16)1.0f, (__bf16)1.0f, (__bf16)1.0f, (__bf16)1.0f, (__bf16)1.0f, (__bf16)1.0f, (__bf16)1.0f, (__bf16)1.0f};
    f32x4 o[2][4], lsum[2];
    float m[2] = {-1.0e30f, -1.0e30f};
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
        lsum[sb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) o[sb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    for (int tile = 0; tile < ntiles; ++tile) {
        const int buf = tile & 1;
        if (tile + 1 < ntiles) fetch(tile + 1);                           // in flight under this tile's MFMAs
        const unsigned char* kl = kv_lds[buf][0];
        const unsigned char* vl = kv_lds[buf][1];
        // K as A operands: row = key 16 t + j, k = dims 8 g .. (+ 32 on step 1)
        bf16x8 kf[4][2];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int st = 0; st < 2; ++st) kf[t][st] = *reinterpret_cast<const bf16x8*>(kl + (16 * t + j) * PITCH + 16 * g + 64 * st);
        // V^T as A operands by transposed reads: k slot (g, e) of step ks is key 32 ks + 16 (e >> 2) + 4 g + (e & 3), row = dim 16 cb + j
        bf16x8 vf[2][4];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                const unsigned char* va = vl + (32 * ks + 4 * g + q4) * PITCH + 8 * p4 + cb * 32;
                const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(va));
                const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(va + 16 * PITCH));
                const s16x8 vv = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                vf[ks][cb] = __builtin_bit_cast(bf16x8, vv);
            }
        const int kvalid = N - tile * KT;                                 // keys of this tile that exist (>= 1)
#pragma unroll
        for (int sb = 0; sb < 2; ++sb) {
            f32x4 s[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[t][0], qf[sb][0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[t][1], qf[sb][1], s[t], 0, 0, 0);
            }
            if (kvalid < KT) {                                            // (workgroup-uniform) the tail tile: absent keys out
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int e = 0; e < 4; ++e) s[t][e] = 16 * t + 4 * g + e < kvalid ? s[t][e] : -1.0e30f;
            }
            float mx = s[0][0];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) mx = fmaxf(mx, s[t][e]);
            {   // the query's other three lane quarters (lane ^ 16, lane ^ 32)
                auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
                mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
                sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
                mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
            }
            const float mn = fmaxf(m[sb], mx);
            const float alpha = __builtin_amdgcn_exp2f((m[sb] - mn) * sl2);
            m[sb] = mn;
            const float nm = -mn * sl2;                                   // p = 2^((S - max) * scale * log2 e)
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) s[t][e] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[t][e], sl2, nm));
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                lsum[sb][e] *= alpha;
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) o[sb][cb][e] *= alpha;
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const f32x4 pa = s[2 * ks], pb = s[2 * ks + 1];
                const bf16x8 pf = {(__bf16)pa[0], (__bf16)pa[1], (__bf16)pa[2], (__bf16)pa[3], (__bf16)pb[0], (__bf16)pb[1], (__bf16)pb[2], (__bf16)pb[3]};
                lsum[sb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, pf, lsum[sb], 0, 0, 0);
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) o[sb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[ks][cb], pf, o[sb][cb], 0, 0, 0);
            }
        }
        if (tile + 1 < ntiles) put(buf ^ 1);                              // the other buffer: every wave left it at the last barrier
        __syncthreads();
    }

    // O^T[dim 16 cb + 4 g + e][query j] / l -> 4 bf16 per (cb) at out row q, dims 16 cb + 4 g
    unsigned char* outc = reinterpret_cast<unsigned char*>(out) + (size_t)b * N * outb + (size_t)h * HD * 2;
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
        const int q = q0 + 16 * sb + j;
        if (q < N) {
            const float inv = 1.0f / lsum[sb][0];
            unsigned char* dst = outc + (size_t)q * outb + 8 * g;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
                *reinterpret_cast<uint2*>(dst + cb * 32) = make_uint2(pack_bf16x2(o[sb][cb][0] * inv, o[sb][cb][1] * inv),
                                                                      pack_bf16x2(o[sb][cb][2] * inv, o[sb][cb][3] * inv));
        }
    }
}

// ------------------------------------------------------------------------------------------------ float32, VALU (parity path)
__global__ __launch_bounds__(64) void mhsa_f32_kernel(const float* __restrict__ qkv, float* __restrict__ out, int N, int heads, int qblocks,
                                                     float scale) {
    __shared__ __attribute__((aligned(16))) float kv[2][KT * HD];       // [K, V][key][dim]
    __shared__ float sc[KT * 64];                                       // logits [key][query lane]
    const int lane = threadIdx.x;
    const int qb = (int)(blockIdx.x % (unsigned)qblocks);
    const int bh = (int)(blockIdx.x / (unsigned)qblocks);
    const int h = bh % heads, b = bh / heads;
    const size_t row = (size_t)3 * heads * HD, C = (size_t)heads * HD;
    const float* base = qkv + (size_t)b * N * row;
    const int q = qb * 64 + lane;
    const bool qvalid = q < N;
    float qv[HD], o[HD];
#pragma unroll
    for (int d = 0; d < HD; d += 4) {
        const float4 v = qvalid ? *reinterpret_cast<const float4*>(base + (size_t)q * row + (size_t)h * HD + d) : make_float4(0.f, 0.f, 0.f, 0.f);
        qv[d] = v.x; qv[d + 1] = v.y; qv[d + 2] = v.z; qv[d + 3] = v.w;
        o[d] = o[d + 1] = o[d + 2] = o[d + 3] = 0.0f;
    }
    float m = -3.0e38f, l = 0.0f;
    for (int k0 = 0; k0 < N; k0 += KT) {
        const int kn = N - k0 < KT ? N - k0 : KT;
        for (int i = lane; i < KT * 32; i += 64) {                      // (key, K / V, 4-float piece)
            const int key = i >> 5, t = (i >> 4) & 1, c4 = i & 15;
            const float4 v = key < kn ? *reinterpret_cast<const float4*>(base + (size_t)(k0 + key) * row + (size_t)(1 + t) * C + (size_t)h * HD + 4 * c4)
                                      : make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(&kv[t][key * HD + 4 * c4]) = v;
        }
        __syncthreads();
        float mx = m;
        for (int k = 0; k < kn; ++k) {
            float acc = 0.0f;
#pragma unroll
            for (int d = 0; d < HD; ++d) acc = __builtin_fmaf(qv[d], kv[0][k * HD + d], acc);
            acc *= scale;
            sc[k * 64 + lane] = acc;
            mx = fmaxf(mx, acc);
        }
        const float alpha = expf(m - mx);
        m = mx;
        // the tile's sums apart, then folded in: rounding grows with 64 + N / 64 terms, not N
        float lt = 0.0f, ot[HD];
#pragma unroll
        for (int d = 0; d < HD; ++d) ot[d] = 0.0f;
        for (int k = 0; k < kn; ++k) {
            const float p = expf(sc[k * 64 + lane] - m);
            lt += p;
#pragma unroll
            for (int d = 0; d < HD; ++d) ot[d] = __builtin_fmaf(p, kv[1][k * HD + d], ot[d]);
        }
        l = __builtin_fmaf(l, alpha, lt);
#pragma unroll
        for (int d = 0; d < HD; ++d) o[d] = __builtin_fmaf(o[d], alpha, ot[d]);
        __syncthreads();
    }
    if (!qvalid) return;
    const float inv = 1.0f / l;
    float* dst = out + ((size_t)b * N + q) * C + (size_t)h * HD;
#pragma unroll
    for (int d = 0; d < HD; d += 4) *reinterpret_cast<float4*>(dst + d) = make_float4(o[d] * inv, o[d + 1] * inv, o[d + 2] * inv, o[d + 3] * inv);
}

// B, N, heads > 0, 16-byte aligned buffers, grid below 2^31 work-items: checked by the caller (capi.hip)
int mhsa_launch(const void* qkv, void* out, int B, int N, int heads, float scale, int dtype, hipStream_t stream) {
    if (dtype == 0) {
        const int qblocks = (N + 63) / 64;
        hipLaunchKernelGGL(mhsa_f32_kernel, dim3((unsigned)((long long)B * heads * qblocks)), dim3(64), 0, stream, (const float*)qkv, (float*)out,
                           N, heads, qblocks, scale);
        return (int)hipGetLastError();
    }
    const int qblocks = (N + MH_QB - 1) / MH_QB;
    hipLaunchKernelGGL(mhsa_bf16_kernel, dim3((unsigned)((long long)B * heads * qblocks)), dim3(64 * MH_WAVES), 0, stream, (const __bf16*)qkv,
                       (__bf16*)out, N, heads, qblocks, scale);
    return (int)hipGetLastError();
}

}  // namespace ppn
