// swin_wmsa_bwd.hip — Swin's (shifted-)window multi-head self-attention, backward: the gradient of ppn_swin_wmsa_fwd (swin_wmsa.hip,
// whose layouts, slot arithmetic, bias table and -100 region mask are used unchanged) with respect to qkv, pad_kv and the bias table.
//
// Per (image, window, head), over the 49 slots, with L_ij = scale q_i . k_j + rpb[h][rel(i, j)] + mask_ij:
//   P = softmax_j(L);  dP_ij = dO_i . v_j;  delta_i = sum_j P_ij dP_ij (= rowsum(dO o O): the forward's output is not needed);
//   dS_ij = P_ij (dP_ij - delta_i);  dV_j = sum_i P_ij dO_i;  dQ_i = scale sum_j dS_ij k_j;  dK_j = scale sum_i dS_ij q_i.
// A padded query has dO = 0 and adds nothing.  A padded key / value slot's dK / dV belongs to pad_kv (the qkv bias): dpad_kv's k and
// v thirds are the sums over every padded position of every image, its q third is 0.  drpb[h][dy + 6][dx + 6] = the sum of dS_ij
// over images, windows and slot pairs with query-minus-key offset (dy, dx), padded keys included.
//
// A window is self-contained (every token is in exactly one window per layer), so one item = (window, head) is owned end to end:
// dq / dk / dv have one writer per element.  drpb and dpad_kv: every workgroup keeps one head and a running float32 sum of dS
// (64 x 64 per wave) and of the padded slots' dK / dV over the windows it walks, folds them once at the end in a fixed order into
// its 256 floats of the caller's workspace (169 bins + 2 x 32), and swin_wmsa_bwd_reduce_kernel sums the workgroups' partials in
// ascending order.  No atomics of any kind; the gradients are bitwise reproducible.
//
//   bfloat16: one WAVE per item on the matrix cores.  K, Q and dO rows go to the wave's LDS image by LDS-DMA; V stays in registers.
//             Both orientations are computed from registers (no P / dS hand-off through LDS):
//             pass 1, query on the MFMA column as in the forward: S^T = K Q^T on the bias table (+ mask), exact softmax over 64
//                     slots in float32, dP^T = V dO^T, delta, dS^T, and dQ^T += K^T dS^T with K^T by ds_read_b64_tr_b16; the
//                     query's log-sum-exp (exp2 domain) and delta go to 2 x 64 floats of LDS;
//             pass 2, key on the column: S = Q K^T and dP = dO V^T again (16 MFMAs each), P and dS from the saved statistics, and
//                     dV^T += dO^T P, dK^T += Q^T dS with dO^T / Q^T transposed out of the same images.
//             P and dS are rounded to bfloat16 once each as operands; the outputs are rounded once.
//   float32:  a VALU kernel of the same arithmetic (the parity path): one workgroup of 64 lanes per item, q / k / v / dO staged in
//             LDS; a lane owns a query (P, dS, dQ), then a key (dV, dK).
//
// Offsets of tokens are 64-bit; window numbers are 32-bit (the caller rejects B * windows >= 2^31).
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include <algorithm>
#include "ppn_device.h"
#include "ppn_kernels.h"

namespace ppn {

namespace {
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
constexpr int SB_HD = 32, SB_WAVES = 4, SB_TP = 68;     // head dim, waves per workgroup (bfloat16), bias-table row pitch (floats)
constexpr int SB_IMG = 64 * 64;                         // one LDS image: 64 slots x 32 bf16
constexpr int SB_WAVE_LDS = 3 * SB_IMG + 2 * 64 * 4;    // K, Q, dO images and the two per-query statistics
constexpr int SB_PART = 256;                            // floats per workgroup in the workspace: 169 bins, 32 dK, 32 dV (23 unused)
constexpr int SB_RESIDENT = 2;                          // workgroups per CU the geometry (and the workspace) counts on at most
constexpr int SF_P = 65;                                // float32: pitch of the [key][query] LDS matrices

// token index (b, py, px) of window slot `sl` (0..48), or -1 when the slot is a padded position (as swin_wmsa.hip)
__device__ __forceinline__ long long slot_token(int sl, int b, int wy, int wx, int H, int W, int Hp, int Wp, int shift) {
    const int kr = sl / 7, kc = sl - 7 * (sl / 7);
    int py = 7 * wy + kr + shift, px = 7 * wx + kc + shift;
    py -= py >= Hp ? Hp : 0;
    px -= px >= Wp ? Wp : 0;
    if (py >= H || px >= W) return -1;
    return ((long long)b * H + py) * W + px;
}

// rows 32 ks .. 32 ks + 31 of an LDS image [slot][32 bf16] as the A operand of a product over slots: operand row = dim 16 cb + j,
// k slot (g, e) = slot 32 ks + 16 (e >> 2) + 4 g + (e & 3) — the order in which two accumulators packed side by side hold them
__device__ __forceinline__ bf16x8 read_transposed(const unsigned char* img, int ks, int cb, int g, int q4, int p4) {
    const unsigned char* a = img + (32 * ks + 4 * g + q4) * 64 + 8 * p4 + cb * 32;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a + 16 * 64));
    const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
}

__device__ __forceinline__ bf16x8 pack8(const f32x4 a, const f32x4 b) {
    return bf16x8{(__bf16)a[0], (__bf16)a[1], (__bf16)a[2], (__bf16)a[3], (__bf16)b[0], (__bf16)b[1], (__bf16)b[2], (__bf16)b[3]};
}

// a value of the query's four lanes (lane ^ 16, lane ^ 32) summed: every lane gets the same bits (each step adds the same pair)
__device__ __forceinline__ float quad_sum(float v) {
    v += __shfl_xor(v, 16);
    return v + __shfl_xor(v, 32);
}

// One workgroup's partial sums: bin t of drpb = the sum over its waves' dS matrices ds[w][query][key] (pitch `qp` floats per query,
// `wp` per wave) of the pairs with query-minus-key offset (t / 13 - 6, t % 13 - 6), waves, query rows and columns ascending.
__device__ __forceinline__ float fold_bin(const float* ds, int waves, int wp, int qp, int kp, int t) {
    const int dy = t / 13 - 6, dx = t - 13 * (t / 13) - 6;
    float a = 0.0f;
    for (int w = 0; w < waves; ++w)
        for (int u = 0; u < 7; ++u) {
            const int kr = u - dy;
            if (kr < 0 || kr > 6) continue;
            for (int v = 0; v < 7; ++v) {
                const int kc = v - dx;
                if (kc < 0 || kc > 6) continue;
                a += ds[w * wp + (7 * u + v) * qp + (7 * kr + kc) * kp];
            }
        }
    return a;
}
}  // namespace

// ------------------------------------------------------------------------------------------------ bfloat16, matrix cores
__global__ __launch_bounds__(64 * SB_WAVES, 2) void swin_wmsa_bwd_bf16_kernel(const __bf16* __restrict__ qkv, const __bf16* __restrict__ pad_kv,
                                                                              const float* __restrict__ rpb, const __bf16* __restrict__ dout,
                                                                              __bf16* __restrict__ dqkv, float* __restrict__ partial, int H, int W,
                                                                              int Hp, int Wp, int heads, int shift, float scale, int n_items,
                                                                              const __bf16* __restrict__ zero) {
    __shared__ __attribute__((aligned(16))) unsigned char img_all[SB_WAVES][SB_WAVE_LDS];
    __shared__ __attribute__((aligned(16))) float tl[49 * SB_TP];                        // this workgroup's head: bias table [query][slot]
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    unsigned char* kimg = img_all[wave];
    unsigned char* qimg = kimg + SB_IMG;
    unsigned char* dimg = kimg + 2 * SB_IMG;
    float* st = reinterpret_cast<float*>(kimg + 3 * SB_IMG);                             // [0][slot] log-sum-exp (exp2 domain), [1][slot] delta
    const int j = lane & 15, g = lane >> 4, q4 = j >> 2, p4 = j & 3;
    const int h = (int)((blockIdx.x >> 3) % heads);
    const int slot0 = (int)(blockIdx.x / (8 * heads)) * 8 + (blockIdx.x & 7), nslots = (int)(gridDim.x / (8 * heads)) * 8;
    const float inv_scale = 1.0f / scale;
    // T[query slot][key slot] = rpb[h][qr - kr + 6][qc - kc + 6] / scale, -1e30 on key slots 49..63 (as the forward)
    for (int i = threadIdx.x; i < 49 * 64; i += 64 * SB_WAVES) {
        const int sl = i & 63, qp = i >> 6;
        float v = -1.0e30f;
        if (sl < 49) {
            const int u = qp / 7, w = qp - 7 * (qp / 7), kr = sl / 7, kc = sl - 7 * (sl / 7);
            v = rpb[(size_t)h * 169 + (u - kr + 6) * 13 + (w - kc + 6)] * inv_scale;
        }
        tl[qp * SB_TP + sl] = v;
    }
    __syncthreads();

    const size_t tokb = (size_t)3 * heads * SB_HD * 2, outb = (size_t)heads * SB_HD * 2;   // bytes per qkv / dout token row
    const uint32_t qh = (uint32_t)h * (SB_HD * 2), kh = (uint32_t)(heads + h) * (SB_HD * 2), vh = (uint32_t)(2 * heads + h) * (SB_HD * 2);
    const unsigned char* qkvb = reinterpret_cast<const unsigned char*>(qkv);
    const unsigned char* padb = reinterpret_cast<const unsigned char*>(pad_kv);
    const unsigned char* zerob = reinterpret_cast<const unsigned char*>(zero);
    const unsigned char* doutb = reinterpret_cast<const unsigned char*>(dout);
    unsigned char* gout = reinterpret_cast<unsigned char*>(dqkv);
    const float sl2 = scale * 1.4426950408889634f, mneg = -100.0f * inv_scale;
    const bf16x8 vpad = *reinterpret_cast<const bf16x8*>(padb + vh + 16 * g);
    // region bits of the slots 16 t + 4 g + e this lane's accumulator rows hold: row (SY) / column (SX) < 7 - shift
    const int thr = 7 - shift;
    uint32_t SY = 0, SX = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int sl = 16 * t + 4 * g + e;
            SY |= (uint32_t)(sl < 49 && sl / 7 < thr) << (4 * t + e);
            SX |= (uint32_t)(sl < 49 && sl % 7 < thr) << (4 * t + e);
        }
    const int nWx = Wp / 7, nWy = Hp / 7, nW = nWx * nWy;

    // running sum of dS: [key tile][query tile], row = query 16 t + 4 g + e, column = key j; of query tile 3 only slot 48 exists (e = 0)
    f32x4 acc[4][3];
    float acc3[4];
    f32x4 padk[2], padv[2];                        // running sums of the padded key slots' dK^T / dV^T (this lane's column's)
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        acc3[a] = 0.0f;
#pragma unroll
        for (int t = 0; t < 3; ++t) acc[a][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) padk[cb] = padv[cb] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (long long item = slot0 * SB_WAVES + wave; item < n_items; item += nslots * SB_WAVES) {   // 64-bit: the step may pass 2^31
        const int grp = (int)item;
        const int b = grp / nW, wi = grp - b * nW, wy = wi / nWx, wx = wi - wy * nWx;
        const bool lastr = shift > 0 && wy == nWy - 1, lastc = shift > 0 && wx == nWx - 1;
        // K, Q, dO rows -> LDS by LDS-DMA: piece p = slot * 4 + chunk at byte 16 p; padded slots read pad_kv (K) or the zero line
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int sl = (it * 64 + lane) >> 2;
            const long long tv = sl < 49 ? slot_token(sl, b, wy, wx, H, W, Hp, Wp, shift) : -1;
            const unsigned char* ks = tv >= 0 ? qkvb + (size_t)tv * tokb + kh : (sl < 49 ? padb + kh : zerob);
            const unsigned char* qs = tv >= 0 ? qkvb + (size_t)tv * tokb + qh : zerob;
            const unsigned char* ds = tv >= 0 ? doutb + (size_t)tv * outb + qh : zerob;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ks + 16 * (lane & 3)),
                                             (__attribute__((address_space(3))) void*)(kimg + it * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(qs + 16 * (lane & 3)),
                                             (__attribute__((address_space(3))) void*)(qimg + it * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ds + 16 * (lane & 3)),
                                             (__attribute__((address_space(3))) void*)(dimg + it * 1024), 16, 0, 0);
        }
        // this lane's slot 16 t + j: its token and its V row (an A operand in pass 1, a B operand in pass 2: the same registers)
        const long long tok0 = (long long)b * H * W;
        int tq[4];                                 // within the image (H * W < 2^31: the caller checked), -1 = padded or no slot
        bf16x8 vf[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int sl = 16 * t + j;
            tq[t] = sl < 49 ? (int)slot_token(sl, 0, wy, wx, H, W, Hp, Wp, shift) : -1;
            if (tq[t] >= 0) vf[t] = *reinterpret_cast<const bf16x8*>(qkvb + (size_t)(tok0 + tq[t]) * tokb + vh + 16 * g);
            else vf[t] = sl < 49 ? vpad : bf16x8{};
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // the DMAs of this window have landed (same wave: no barrier)
        // operand rows (slot 16 t + j, dims 8 g ..) come out of the images where they are needed: fewer live registers
        auto frag = [&](const unsigned char* img, int t) { return *reinterpret_cast<const bf16x8*>(img + (16 * t + j) * 64 + 16 * g); };

        // ---- pass 1: query 16 qt + j on the column; rows = keys 16 t + 4 g + e
        {
        bf16x8 kf[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) kf[t] = frag(kimg, t);
#pragma unroll 1
        for (int qt = 0; qt < 4; ++qt) {
            const bf16x8 qfq = frag(qimg, qt), dfq = frag(dimg, qt);
            const int qs = 16 * qt + j;
            const int qtok = qt == 0 ? tq[0] : qt == 1 ? tq[1] : qt == 2 ? tq[2] : tq[3];
            const int qp = qs < 49 ? qs : 48, u = qp / 7, v = qp - 7 * (qp / 7);
            const float* tb = tl + qp * SB_TP + 4 * g;
            f32x4 s[4], dp[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) s[t] = *reinterpret_cast<const f32x4*>(tb + 16 * t);
            if (lastr || lastc) {                                             // (wave-uniform) the region mask joins the table
                const uint32_t m = (lastr ? (u < thr ? ~SY : SY) : 0u) | (lastc ? (v < thr ? ~SX : SX) : 0u);
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int e = 0; e < 4; ++e) s[t][e] += ((m >> (4 * t + e)) & 1u) ? mneg : 0.0f;
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[t], qfq, s[t], 0, 0, 0);
                dp[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[t], dfq, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
            }
            float mx = s[0][0];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) mx = fmaxf(mx, s[t][e]);
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float nm = -mx * sl2;                                       // p = 2^((S' - max) * scale * log2 e)
            float l = 0.0f;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    s[t][e] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[t][e], sl2, nm));
                    l += s[t][e];
                }
            l = quad_sum(l);
            const float inv = 1.0f / l;
            float dl = 0.0f;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    s[t][e] *= inv;                                           // P
                    dl = __builtin_fmaf(s[t][e], dp[t][e], dl);
                }
            dl = quad_sum(dl);                                                // delta
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) dp[t][e] = s[t][e] * (dp[t][e] - dl);   // dS^T
            if (g == 0) {                                                     // slots 49..63 are no queries: their P is 0 in pass 2
                st[qs] = qs < 49 ? __builtin_fmaf(mx, sl2, log2f(l)) : 3.0e38f;
                st[64 + qs] = dl;
            }
            // dQ^T = K^T . dS^T: k slot (g, e) of step ks is key 4 g + (e & 3) of tile 2 ks + (e >> 2) — the registers in place
            f32x4 dq[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bf16x8 dsf = pack8(dp[2 * ks], dp[2 * ks + 1]);
#pragma unroll
                for (int cb = 0; cb < 2; ++cb)
                    dq[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(read_transposed(kimg, ks, cb, g, q4, p4), dsf, dq[cb], 0, 0, 0);
            }
            if (qtok >= 0) {
                unsigned char* dst = gout + ((size_t)(tok0 + qtok) * tokb + qh + 8 * g);
#pragma unroll
                for (int cb = 0; cb < 2; ++cb)
                    *reinterpret_cast<uint2*>(dst + cb * 32) = make_uint2(pack_bf16x2(dq[cb][0] * scale, dq[cb][1] * scale),
                                                                          pack_bf16x2(dq[cb][2] * scale, dq[cb][3] * scale));
            }
        }

        }
        // ---- pass 2: key 16 kt + j on the column; rows = queries 16 t + 4 g + e (statistics of pass 1: this wave's own LDS writes)
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            const bf16x8 kfk = frag(kimg, kt);
            const int ksl = 16 * kt + j;
            const int ktok = tq[kt];
            const int kp = ksl < 49 ? ksl : 48, kr = kp / 7, kc = kp - 7 * (kp / 7);
            const uint32_t m = (lastr ? (kr < thr ? ~SY : SY) : 0u) | (lastc ? (kc < thr ? ~SX : SX) : 0u);
            f32x4 dk[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}}, dv[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {      // 32 queries: the two 16-query tiles t = 2 ks, 2 ks + 1 that one operand packs
                f32x4 p[2], ds[2];
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {
                    const int t = 2 * ks + tt;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int qs = 16 * t + 4 * g + e;
                        p[tt][e] = tl[(qs < 49 ? qs : 48) * SB_TP + ksl] + (((m >> (4 * t + e)) & 1u) ? mneg : 0.0f);
                    }
                    p[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(qimg, t), kfk, p[tt], 0, 0, 0);
                    ds[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(dimg, t), vf[kt], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                    const f32x4 L = *reinterpret_cast<const f32x4*>(st + 16 * t + 4 * g);
                    const f32x4 D = *reinterpret_cast<const f32x4*>(st + 64 + 16 * t + 4 * g);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        p[tt][e] = __builtin_amdgcn_exp2f(__builtin_fmaf(p[tt][e], sl2, -L[e]));
                        ds[tt][e] = p[tt][e] * (ds[tt][e] - D[e]);
                        if (t < 3) acc[kt][t][e] += ds[tt][e];
                    }
                    if (t == 3) acc3[kt] += ds[tt][0];
                }
                const bf16x8 pf = pack8(p[0], p[1]), dsf = pack8(ds[0], ds[1]);
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    dv[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(read_transposed(dimg, ks, cb, g, q4, p4), pf, dv[cb], 0, 0, 0);
                    dk[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(read_transposed(qimg, ks, cb, g, q4, p4), dsf, dk[cb], 0, 0, 0);
                }
            }
            if (ktok >= 0) {
                unsigned char* dst = gout + ((size_t)(tok0 + ktok) * tokb + 8 * g);
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    *reinterpret_cast<uint2*>(dst + kh + cb * 32) = make_uint2(pack_bf16x2(dk[cb][0] * scale, dk[cb][1] * scale),
                                                                               pack_bf16x2(dk[cb][2] * scale, dk[cb][3] * scale));
                    *reinterpret_cast<uint2*>(dst + vh + cb * 32) = make_uint2(pack_bf16x2(dv[cb][0], dv[cb][1]), pack_bf16x2(dv[cb][2], dv[cb][3]));
                }
            } else if (ksl < 49) {                                            // a padded position: its gradient is pad_kv's
#pragma unroll
                for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        padk[cb][e] += dk[cb][e] * scale;
                        padv[cb][e] += dv[cb][e];
                    }
            }
        }
        // the next window's DMAs overwrite this wave's images: its reads must have returned (wave-local ordering)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }

    // ---- the workgroup's partial sums, in a fixed order.  First the padded slots': [k, v][dim][column j] floats per wave
    float* wf = reinterpret_cast<float*>(kimg);
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            wf[(16 * cb + 4 * g + e) * 16 + j] = padk[cb][e];
            wf[(32 + 16 * cb + 4 * g + e) * 16 + j] = padv[cb][e];
        }
    __syncthreads();
    float* mine = partial + (size_t)blockIdx.x * SB_PART;
    if (threadIdx.x < 64) {
        float a = 0.0f;
        for (int w = 0; w < SB_WAVES; ++w) {
            const float* src = reinterpret_cast<const float*>(img_all[w]) + threadIdx.x * 16;
            for (int c = 0; c < 16; ++c) a += src[c];
        }
        mine[169 + threadIdx.x] = a;
    }
    __syncthreads();
    // then dS: [query][key] floats per wave (49 x 49 of the 64 x 64)
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int qs = 16 * t + 4 * g + e, ksl = 16 * kt + j;
                if (qs < 49 && ksl < 49) wf[qs * 49 + ksl] = t < 3 ? acc[kt][t][e] : acc3[kt];
            }
    __syncthreads();
    if (threadIdx.x < 169) mine[threadIdx.x] = fold_bin(reinterpret_cast<const float*>(&img_all[0][0]), SB_WAVES, SB_WAVE_LDS / 4, 49, 1, threadIdx.x);
}

// ------------------------------------------------------------------------------------------------ float32, VALU (parity path)
__global__ __launch_bounds__(64) void swin_wmsa_bwd_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ pad_kv,
                                                              const float* __restrict__ rpb, const float* __restrict__ dout,
                                                              float* __restrict__ dqkv, float* __restrict__ partial, int H, int W, int Hp, int Wp,
                                                              int heads, int shift, float scale, int n_items) {
    __shared__ __attribute__((aligned(16))) float rows[4][49 * SB_HD];  // q, k, v, dO [slot][dim]; later the padded slots' dK | dV
    __shared__ float pm[49 * SF_P];                                     // P   [key][query lane]
    __shared__ float dsm[49 * SF_P];                                    // dS  [key][query lane]
    __shared__ float accm[49 * SF_P];                                   // running sum of dS over this workgroup's windows
    __shared__ long long tokl[49];
    const int lane = threadIdx.x;
    const int h = (int)((blockIdx.x >> 3) % heads);
    const int slot0 = (int)(blockIdx.x / (8 * heads)) * 8 + (blockIdx.x & 7), nslots = (int)(gridDim.x / (8 * heads)) * 8;
    const int nWx = Wp / 7, nWy = Hp / 7, nW = nWx * nWy;
    const size_t C = (size_t)heads * SB_HD;
    const int u = lane / 7, v = lane % 7, thr = 7 - shift;
    const float* tb = rpb + (size_t)h * 169;
    for (int i = lane; i < 49 * SF_P; i += 64) accm[i] = 0.0f;
    float padsum = 0.0f;                                               // lane d < 32: dK[d] of the padded slots, lane 32 + d: dV[d]

    for (long long item = slot0; item < n_items; item += nslots) {     // 64-bit: the step may pass 2^31
        const int grp = (int)item;
        const int b = grp / nW, wi = grp - b * nW, wy = wi / nWx, wx = wi - wy * nWx;
        const bool lastr = shift > 0 && wy == nWy - 1, lastc = shift > 0 && wx == nWx - 1;
        __syncthreads();                                               // the previous window's readers are done
        if (lane < 49) tokl[lane] = slot_token(lane, b, wy, wx, H, W, Hp, Wp, shift);
        for (int i = lane; i < 49 * 32; i += 64) {                     // (slot, q / k / v / dO, 4-float chunk)
            const int sl = i >> 5, t = (i >> 3) & 3, c4 = i & 7;
            const long long tok = slot_token(sl, b, wy, wx, H, W, Hp, Wp, shift);
            float4 val = make_float4(0.f, 0.f, 0.f, 0.f);              // a padded slot's q and dO
            if (t == 3) {
                if (tok >= 0) val = *reinterpret_cast<const float4*>(dout + (size_t)tok * C + (size_t)h * SB_HD + 4 * c4);
            } else if (tok >= 0) {
                val = *reinterpret_cast<const float4*>(qkv + (size_t)tok * 3 * C + t * C + (size_t)h * SB_HD + 4 * c4);
            } else if (t > 0) {
                val = *reinterpret_cast<const float4*>(pad_kv + t * C + (size_t)h * SB_HD + 4 * c4);
            }
            *reinterpret_cast<float4*>(&rows[t][sl * SB_HD + 4 * c4]) = val;
        }
        __syncthreads();
        bool anypad = false;
        for (int k = 0; k < 49; ++k) anypad |= tokl[k] < 0;            // workgroup-uniform
        if (lane < 49) {                                               // ---- this lane's query: P, dS, dQ
            float q[SB_HD], d[SB_HD], dq[SB_HD];
#pragma unroll
            for (int c = 0; c < SB_HD; ++c) {
                q[c] = rows[0][lane * SB_HD + c] * scale;              // q = q * scale first, as the forward
                d[c] = rows[3][lane * SB_HD + c];
                dq[c] = 0.0f;
            }
            float mx = -3.0e38f;
            for (int k = 0; k < 49; ++k) {
                const int kr = k / 7, kc = k - 7 * (k / 7);
                float a = 0.0f, dp = 0.0f;
#pragma unroll
                for (int c = 0; c < SB_HD; ++c) {
                    a = __builtin_fmaf(q[c], rows[1][k * SB_HD + c], a);
                    dp = __builtin_fmaf(d[c], rows[2][k * SB_HD + c], dp);
                }
                a += tb[(u - kr + 6) * 13 + (v - kc + 6)];
                if ((lastr && ((u < thr) != (kr < thr))) || (lastc && ((v < thr) != (kc < thr)))) a += -100.0f;
                pm[k * SF_P + lane] = a;
                dsm[k * SF_P + lane] = dp;
                mx = fmaxf(mx, a);
            }
            float sum = 0.0f;
            for (int k = 0; k < 49; ++k) {
                const float p = expf(pm[k * SF_P + lane] - mx);
                pm[k * SF_P + lane] = p;
                sum += p;
            }
            const float inv = 1.0f / sum;
            float dl = 0.0f;
            for (int k = 0; k < 49; ++k) {
                const float p = pm[k * SF_P + lane] * inv;
                pm[k * SF_P + lane] = p;
                dl = __builtin_fmaf(p, dsm[k * SF_P + lane], dl);
            }
            for (int k = 0; k < 49; ++k) {
                const float ds = pm[k * SF_P + lane] * (dsm[k * SF_P + lane] - dl);
                dsm[k * SF_P + lane] = ds;
                accm[k * SF_P + lane] += ds;                           // this lane's own column: no other writer
#pragma unroll
                for (int c = 0; c < SB_HD; ++c) dq[c] = __builtin_fmaf(ds, rows[1][k * SB_HD + c], dq[c]);
            }
            const long long qtok = tokl[lane];
            if (qtok >= 0) {
                float* dst = dqkv + (size_t)qtok * 3 * C + (size_t)h * SB_HD;
#pragma unroll
                for (int c = 0; c < SB_HD; c += 4)
                    *reinterpret_cast<float4*>(dst + c) = make_float4(dq[c] * scale, dq[c + 1] * scale, dq[c + 2] * scale, dq[c + 3] * scale);
            }
        }
        __syncthreads();
        float dk[SB_HD], dv[SB_HD];
        if (lane < 49) {                                               // ---- this lane's key: dV, dK
#pragma unroll
            for (int c = 0; c < SB_HD; ++c) dk[c] = dv[c] = 0.0f;
            for (int i = 0; i < 49; ++i) {
                const float p = pm[lane * SF_P + i], ds = dsm[lane * SF_P + i];
#pragma unroll
                for (int c = 0; c < SB_HD; ++c) {
                    dv[c] = __builtin_fmaf(p, rows[3][i * SB_HD + c], dv[c]);
                    dk[c] = __builtin_fmaf(ds, rows[0][i * SB_HD + c], dk[c]);
                }
            }
            const long long ktok = tokl[lane];
            if (ktok >= 0) {
                float* gk = dqkv + (size_t)ktok * 3 * C + C + (size_t)h * SB_HD;
#pragma unroll
                for (int c = 0; c < SB_HD; c += 4) {
                    *reinterpret_cast<float4*>(gk + c) = make_float4(dk[c] * scale, dk[c + 1] * scale, dk[c + 2] * scale, dk[c + 3] * scale);
                    *reinterpret_cast<float4*>(gk + C + c) = make_float4(dv[c], dv[c + 1], dv[c + 2], dv[c + 3]);
                }
            }
        }
        if (anypad) {                                                  // the padded slots' dK | dV join the running sums, slots ascending
            __syncthreads();                                           // q and k rows are read no more: their LDS takes [slot][64]
            float* stage = &rows[0][0];
            if (lane < 49 && tokl[lane] < 0) {
#pragma unroll
                for (int c = 0; c < SB_HD; ++c) {
                    stage[lane * 64 + c] = dk[c] * scale;
                    stage[lane * 64 + 32 + c] = dv[c];
                }
            }
            __syncthreads();
            for (int k = 0; k < 49; ++k)
                if (tokl[k] < 0) padsum += stage[k * 64 + lane];
        }
    }
    __syncthreads();
    float* mine = partial + (size_t)blockIdx.x * SB_PART;
    mine[169 + lane] = padsum;
    for (int t = lane; t < 169; t += 64) mine[t] = fold_bin(accm, 1, 0, 1, SF_P, t);
}

// ------------------------------------------------------------------------------------------------ the workgroups' partials -> drpb, dpad_kv
// One workgroup per head; workgroup (s * heads + h) * 8 + x of the main kernel kept head h: its partials are summed with s, x ascending.
__global__ __launch_bounds__(256) void swin_wmsa_bwd_reduce_kernel(const float* __restrict__ partial, float* __restrict__ drpb,
                                                                  float* __restrict__ dpad_kv, int heads, int sets) {
    const int h = blockIdx.x, t = threadIdx.x;
    if (t < 32) dpad_kv[(size_t)h * SB_HD + t] = 0.0f;                 // the q third
    if (t >= 169 + 64) return;
    float a = 0.0f;
    for (int s = 0; s < sets; ++s)
        for (int x = 0; x < 8; ++x) a += partial[((size_t)(s * heads + h) * 8 + x) * SB_PART + t];
    if (t < 169) drpb[(size_t)h * 169 + t] = a;
    else dpad_kv[(size_t)(1 + ((t - 169) >> 5)) * heads * SB_HD + (size_t)h * SB_HD + ((t - 169) & 31)] = a;
}

// ================================================================================================ host
// Workgroups come in sets of 8 * heads (one head each, as the forward's): at most what SB_RESIDENT workgroups per CU hold, at least one.
static long long bwd_max_sets(int heads) {
    const int cus = device_cu_count() > 0 ? device_cu_count() : 256;
    return std::max<long long>(1, ((long long)cus * SB_RESIDENT) / (8LL * heads));
}

// SB_PART floats per workgroup of the largest grid the launcher may choose on this device
long long swin_wmsa_bwd_workspace_floats(int heads) { return bwd_max_sets(heads) * 8LL * heads * SB_PART; }

// B, H, W, heads > 0, shift in {0, 3}, 16-byte aligned buffers, B * windows < 2^31, a workspace of swin_wmsa_bwd_workspace_floats:
// checked by the caller (capi.hip)
int swin_wmsa_bwd_launch(const void* qkv, const void* pad_kv, const float* rpb, const void* dout, void* dqkv, float* dpad_kv, float* drpb, float* ws,
                         int B, int H, int W, int heads, int shift, float scale, int dtype, hipStream_t stream) {
    const int Hp = (H + 6) / 7 * 7, Wp = (W + 6) / 7 * 7;
    const long long windows = (long long)B * (Hp / 7) * (Wp / 7);
    long long sets;
    if (dtype == 0) {
        sets = std::min<long long>((windows + 7) / 8, bwd_max_sets(heads));
        hipLaunchKernelGGL(swin_wmsa_bwd_f32_kernel, dim3((unsigned)(sets * 8 * heads)), dim3(64), 0, stream, (const float*)qkv,
                           (const float*)pad_kv, rpb, (const float*)dout, (float*)dqkv, ws, H, W, Hp, Wp, heads, shift, scale, (int)windows);
    } else {
        const __bf16* zero = (const __bf16*)zero_line();
        if (!zero) return (int)hipErrorOutOfMemory;
        // asked once per process (as the forward does) while the workspace is sized per device: the clamp to SB_RESIDENT, which the
        // workspace counts on, keeps the two in agreement whatever a second device would answer
        static const int resident = [] {
            int n = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)swin_wmsa_bwd_bf16_kernel, 64 * SB_WAVES, 0) != hipSuccess || n < 1)
                n = SB_RESIDENT;
            return std::min(n, SB_RESIDENT);
        }();
        const int cus = device_cu_count() > 0 ? device_cu_count() : 256;
        const long long want_sets = ((windows + SB_WAVES - 1) / SB_WAVES + 7) / 8;
        sets = std::max<long long>(1, std::min<long long>(want_sets, ((long long)cus * resident) / (8LL * heads)));
        hipLaunchKernelGGL(swin_wmsa_bwd_bf16_kernel, dim3((unsigned)(sets * 8 * heads)), dim3(64 * SB_WAVES), 0, stream, (const __bf16*)qkv,
                           (const __bf16*)pad_kv, rpb, (const __bf16*)dout, (__bf16*)dqkv, ws, H, W, Hp, Wp, heads, shift, scale, (int)windows,
                           zero);
    }
    hipLaunchKernelGGL(swin_wmsa_bwd_reduce_kernel, dim3((unsigned)heads), dim3(256), 0, stream, (const float*)ws, drpb, dpad_kv, heads, (int)sets);
    return (int)hipGetLastError();
}

}  // namespace ppn
