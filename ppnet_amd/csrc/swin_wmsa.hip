// swin_wmsa.hip — Swin's (shifted-)window multi-head self-attention, forward: the body of mmseg's ShiftWindowMSA.forward /
// WindowMSA.forward between the qkv and the proj Linear (reference SegNet/mmseg/backbones/swin.py:80-118,179-253) as ONE launch.
//
// The padding to multiples of the window (F.pad), the cyclic shift (torch.roll), window_partition, window_reverse, the reverse roll
// and the crop are index arithmetic: window (wy, wx), slot (i, j) is the padded-grid position ((7 wy + i + shift) mod Hp,
// (7 wx + j + shift) mod Wp), and only real tokens are read or written.  A padded position is a key / value whose k, v are pad_kv
// (mmseg pads BEFORE the qkv Linear, so a padded token's k / v is the projection's bias: "virtual padding", as ppn_na2d_fwd_vpad).
// Logit = (q scale) . k + rpb[h][dy + 6][dx + 6] (dy, dx = query minus key inside the window: swin.py:64-68,97-104) and, on the
// last window row / column of a shifted layer, -100 (NOT -inf, swin.py:216-219) between slots of different regions.
//
//   bfloat16: one WAVE per (window, head) on the matrix cores, the structure of na2d_dense7.hip (a 7 x 7 window is a dense 49-key
//             attention): S^T = K . Q^T with the head's bias table (and the region mask) as the initial accumulator, an exact softmax
//             over 64 slots (49 keys, 15 at -1e30), O^T = V^T . P^T from the S^T registers in place, the denominator by an all-ones
//             MFMA.  A workgroup keeps one head; its 8 waves walk windows.
//   float32:  a plain VALU kernel (the parity path): one workgroup per (window, head), K / V staged in LDS, one query per lane.
//
// Offsets of tokens are 64-bit; window numbers are 32-bit (the launcher rejects B * windows >= 2^31).
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
constexpr int SW_HD = 32, SW_WAVES = 8, SW_TP = 68;                       // head dim, waves per workgroup, bias-table row pitch (floats)

// token index (b, py, px) of window slot `sl` (0..48), or -1 when the slot is a padded position
__device__ __forceinline__ long long slot_token(int sl, int b, int wy, int wx, int H, int W, int Hp, int Wp, int shift) {
    const int kr = sl / 7, kc = sl - 7 * (sl / 7);
    int py = 7 * wy + kr + shift, px = 7 * wx + kc + shift;
    py -= py >= Hp ? Hp : 0;
    px -= px >= Wp ? Wp : 0;
    if (py >= H || px >= W) return -1;
    return ((long long)b * H + py) * W + px;
}

// region label inside the last window row / column of a shifted layer: slot row / column < 7 - shift is region 1, the rest region 2
// (swin.py:199-211: slices (-7, -shift) and (-shift, None) of the padded grid, which the window partition sees unshifted)
}  // namespace

// ------------------------------------------------------------------------------------------------ bfloat16, matrix cores
__global__ __launch_bounds__(64 * SW_WAVES, 4) void swin_wmsa_bf16_kernel(const __bf16* __restrict__ qkv, const __bf16* __restrict__ pad_kv,
                                                                          const float* __restrict__ rpb, __bf16* __restrict__ out, int H, int W, int Hp,
                                                                          int Wp, int heads, int shift, float scale, int n_items,
                                                                          const __bf16* __restrict__ zero) {
    __shared__ __attribute__((aligned(16))) unsigned char vimg_all[SW_WAVES][64 * 64];   // per wave: 64 key slots x 32 bf16 of V
    __shared__ __attribute__((aligned(16))) float tl[49 * SW_TP];                        // this workgroup's head: bias table [query][slot]
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    unsigned char* vimg = vimg_all[wave];
    const int j = lane & 15, g = lane >> 4, q4 = j >> 2, p4 = j & 3;
    const int h = (int)((blockIdx.x >> 3) % heads);
    const int slot0 = (int)(blockIdx.x / (8 * heads)) * 8 + (blockIdx.x & 7), nslots = (int)(gridDim.x / (8 * heads)) * 8;
    const float inv_scale = 1.0f / scale;
    // T[query slot][key slot] = rpb[h][qr - kr + 6][qc - kc + 6] / scale (the units of the raw product q . k: the table is the
    // logits' initial accumulator), -1e30 on key slots 49..63
    for (int i = threadIdx.x; i < 49 * 64; i += 64 * SW_WAVES) {
        const int sl = i & 63, qp = i >> 6;
        float v = -1.0e30f;
        if (sl < 49) {
            const int u = qp / 7, w = qp - 7 * (qp / 7), kr = sl / 7, kc = sl - 7 * (sl / 7);
            v = rpb[(size_t)h * 169 + (u - kr + 6) * 13 + (w - kc + 6)] * inv_scale;
        }
        tl[qp * SW_TP + sl] = v;
    }
    __syncthreads();

    const size_t tokb = (size_t)3 * heads * SW_HD * 2, outb = (size_t)heads * SW_HD * 2;   // bytes per qkv / out token row
    const uint32_t qh = (uint32_t)h * (SW_HD * 2), kh = (uint32_t)(heads + h) * (SW_HD * 2), vh = (uint32_t)(2 * heads + h) * (SW_HD * 2);
    const unsigned char* qkvb = reinterpret_cast<const unsigned char*>(qkv);
    const unsigned char* padb = reinterpret_cast<const unsigned char*>(pad_kv);
    const unsigned char* zerob = reinterpret_cast<const unsigned char*>(zero);
    unsigned char* outc = reinterpret_cast<unsigned char*>(out);
    const float sl2 = scale * 1.4426950408889634f, mneg = -100.0f * inv_scale;
    const bf16x8 kpad = *reinterpret_cast<const bf16x8*>(padb + kh + 16 * g);
    // key-slot region bits of this lane's S^T rows: bit 4 t + e <-> key slot 16 t + 4 g + e has row (KY) / column (KX) < 7 - shift
    const int thr = 7 - shift;
    uint32_t KY = 0, KX = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int sl = 16 * t + 4 * g + e;
            KY |= (uint32_t)(sl < 49 && sl / 7 < thr) << (4 * t + e);
            KX |= (uint32_t)(sl < 49 && sl % 7 < thr) << (4 * t + e);
        }
    const int nWx = Wp / 7, nWy = Hp / 7, nW = nWx * nWy;
    const bf16x8 ones = {(__bf16)1.0f, (__bf16)1.0f, (__bf16)1.0f, (__bf16)1.0f, (__bf16)1.0f, (__bf16)1.0f, (__bf16)1.0f, (__bf16)1.0f};

    for (int grp = slot0 * SW_WAVES + wave; grp < n_items; grp += nslots * SW_WAVES) {
        const int b = grp / nW, wi = grp - b * nW, wy = wi / nWx, wx = wi - wy * nWx;
        const bool lastr = shift > 0 && wy == nWy - 1, lastc = shift > 0 && wx == nWx - 1;
        // this lane's slot 16 t + j: a K row (MFMA A operand) and, in query tile t, its query
        long long tq[4];
        bf16x8 kf[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int sl = 16 * t + j;
            tq[t] = sl < 49 ? slot_token(sl, b, wy, wx, H, W, Hp, Wp, shift) : -1;
            if (tq[t] >= 0) kf[t] = *reinterpret_cast<const bf16x8*>(qkvb + (size_t)tq[t] * tokb + kh + 16 * g);
            else kf[t] = sl < 49 ? kpad : bf16x8{};
        }
        // V rows -> LDS by LDS-DMA: piece p = slot * 4 + chunk at byte 16 p; padded slots read pad_kv, slots 49..63 the zero line
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int sl = (it * 64 + lane) >> 2;
            const long long tv = sl < 49 ? slot_token(sl, b, wy, wx, H, W, Hp, Wp, shift) : -1;
            const unsigned char* src = tv >= 0 ? qkvb + (size_t)tv * tokb + vh : (sl < 49 ? padb + vh : zerob);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + 16 * (lane & 3)),
                                             (__attribute__((address_space(3))) void*)(vimg + it * 1024), 16, 0, 0);
        }
        for (int qt = 0; qt < 4; ++qt) {
            const int qs = 16 * qt + j;
            const long long qtok = tq[qt];
            const bool qvalid = qtok >= 0;
            const bf16x8 qf = qvalid ? *reinterpret_cast<const bf16x8*>(qkvb + (size_t)qtok * tokb + qh + 16 * g) : bf16x8{};
            const int qp = qs < 49 ? qs : 48, u = qp / 7, v = qp - 7 * (qp / 7);
            const float* tb = tl + qp * SW_TP + 4 * g;
            f32x4 s[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) s[t] = *reinterpret_cast<const f32x4*>(tb + 16 * t);
            if (lastr || lastc) {                                             // (wave-uniform) the region mask joins the table
                const uint32_t m = (lastr ? (u < thr ? ~KY : KY) : 0u) | (lastc ? (v < thr ? ~KX : KX) : 0u);
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int e = 0; e < 4; ++e) s[t][e] += ((m >> (4 * t + e)) & 1u) ? mneg : 0.0f;
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[t], qf, s[t], 0, 0, 0);
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
            const float nm = -mx * sl2;                                       // p = 2^((S' - max) * scale * log2 e)
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) s[t][e] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[t][e], sl2, nm));
            if (qt == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the V DMAs of this window have landed (same wave: no barrier)
            // O^T = V^T . P^T: k slot (g, e) of step ks is key 4 g + (e & 3) of tile 2 ks + (e >> 2) — the S^T registers in place
            f32x4 o[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}}, lsum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const f32x4 pa = s[2 * ks], pb = s[2 * ks + 1];
                const bf16x8 pf = {(__bf16)pa[0], (__bf16)pa[1], (__bf16)pa[2], (__bf16)pa[3], (__bf16)pb[0], (__bf16)pb[1], (__bf16)pb[2], (__bf16)pb[3]};
                lsum = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, pf, lsum, 0, 0, 0);
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    const unsigned char* va = vimg + (32 * ks + 4 * g + q4) * 64 + 8 * p4 + cb * 32;
                    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(va));
                    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(va + 16 * 64));
                    const s16x8 vv = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    o[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vv), pf, o[cb], 0, 0, 0);
                }
            }
            if (qvalid) {
                const float inv = 1.0f / lsum[0];
                unsigned char* dst = outc + ((size_t)qtok * outb + qh + 8 * g);
#pragma unroll
                for (int cb = 0; cb < 2; ++cb)
                    *reinterpret_cast<uint2*>(dst + cb * 32) = make_uint2(pack_bf16x2(o[cb][0] * inv, o[cb][1] * inv), pack_bf16x2(o[cb][2] * inv, o[cb][3] * inv));
            }
        }
        // the next window's DMAs overwrite this wave's V image: its transposed reads must have returned (wave-local ordering)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}

// ------------------------------------------------------------------------------------------------ float32, VALU (parity path)
__global__ __launch_bounds__(64) void swin_wmsa_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ pad_kv,
                                                          const float* __restrict__ rpb, float* __restrict__ out, int H, int W, int Hp, int Wp,
                                                          int heads, int shift, float scale) {
    __shared__ __attribute__((aligned(16))) float kv[2][49 * SW_HD];
    __shared__ float sc[49 * 64];                                      // logits [key][query lane]
    const int lane = threadIdx.x, h = blockIdx.y;
    const int nWx = Wp / 7, nWy = Hp / 7, nW = nWx * nWy;
    const int grp = blockIdx.x, b = grp / nW, wi = grp - b * nW, wy = wi / nWx, wx = wi - wy * nWx;
    const size_t C = (size_t)heads * SW_HD;
    for (int i = lane; i < 49 * 16; i += 64) {                         // (slot, k / v, 4-float chunk)
        const int sl = i >> 4, t = (i >> 3) & 1, c4 = i & 7;
        const long long tok = slot_token(sl, b, wy, wx, H, W, Hp, Wp, shift);
        const float* src = (tok >= 0 ? qkv + (size_t)tok * 3 * C : pad_kv) + (1 + t) * C + (size_t)h * SW_HD + 4 * c4;
        *reinterpret_cast<float4*>(&kv[t][sl * SW_HD + 4 * c4]) = *reinterpret_cast<const float4*>(src);
    }
    __syncthreads();
    if (lane >= 49) return;
    const long long qtok = slot_token(lane, b, wy, wx, H, W, Hp, Wp, shift);
    if (qtok < 0) return;                                              // a padded query: cropped by the reference, never written
    float q[SW_HD];
    const float* qs = qkv + (size_t)qtok * 3 * C + (size_t)h * SW_HD;
#pragma unroll
    for (int d = 0; d < SW_HD; ++d) q[d] = qs[d] * scale;              // q = q * scale first (swin.py:94)
    const int u = lane / 7, v = lane % 7, thr = 7 - shift;
    const bool lastr = shift > 0 && wy == nWy - 1, lastc = shift > 0 && wx == nWx - 1;
    const float* tb = rpb + (size_t)h * 169;
    float mx = -3.0e38f;
    for (int k = 0; k < 49; ++k) {                                     // logits -> this lane's column of sc
        const int kr = k / 7, kc = k - 7 * (k / 7);
        float acc = 0.0f;
#pragma unroll
        for (int d = 0; d < SW_HD; ++d) acc = __builtin_fmaf(q[d], kv[0][k * SW_HD + d], acc);
        acc += tb[(u - kr + 6) * 13 + (v - kc + 6)];
        if ((lastr && ((u < thr) != (kr < thr))) || (lastc && ((v < thr) != (kc < thr)))) acc += -100.0f;
        sc[k * 64 + lane] = acc;
        mx = fmaxf(mx, acc);
    }
    float sum = 0.0f, o[SW_HD];
#pragma unroll
    for (int d = 0; d < SW_HD; ++d) o[d] = 0.0f;
    for (int k = 0; k < 49; ++k) {
        const float p = expf(sc[k * 64 + lane] - mx);
        sum += p;
#pragma unroll
        for (int d = 0; d < SW_HD; ++d) o[d] = __builtin_fmaf(p, kv[1][k * SW_HD + d], o[d]);
    }
    const float inv = 1.0f / sum;
    float* dst = out + (size_t)qtok * C + (size_t)h * SW_HD;
#pragma unroll
    for (int d = 0; d < SW_HD; d += 4) *reinterpret_cast<float4*>(dst + d) = make_float4(o[d] * inv, o[d + 1] * inv, o[d + 2] * inv, o[d + 3] * inv);
}

// B, H, W, heads > 0, shift in [0, 7), 16-byte aligned buffers, B * windows < 2^31: checked by the caller (capi.hip)
int swin_wmsa_launch(const void* qkv, const void* pad_kv, const float* rpb, void* out, int B, int H, int W, int heads, int shift, float scale,
                     int dtype, hipStream_t stream) {
    const int Hp = (H + 6) / 7 * 7, Wp = (W + 6) / 7 * 7;
    const long long windows = (long long)B * (Hp / 7) * (Wp / 7);
    if (dtype == 0) {
        hipLaunchKernelGGL(swin_wmsa_f32_kernel, dim3((unsigned)windows, (unsigned)heads), dim3(64), 0, stream, (const float*)qkv,
                           (const float*)pad_kv, rpb, (float*)out, H, W, Hp, Wp, heads, shift, scale);
        return (int)hipGetLastError();
    }
    const __bf16* zero = (const __bf16*)zero_line();
    if (!zero) return (int)hipErrorOutOfMemory;
    // workgroups come in sets of 8 * heads (one head each): as many sets as the windows need, at most what fills the CUs
    static const int resident = [] {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)swin_wmsa_bf16_kernel, 64 * SW_WAVES, 0) != hipSuccess || n < 1) n = 2;
        return n > 3 ? 3 : n;
    }();
    const int cus = device_cu_count() > 0 ? device_cu_count() : 256;
    const long long per_set = 8LL * heads, want_sets = ((windows + SW_WAVES - 1) / SW_WAVES + 7) / 8;
    const long long sets = std::max<long long>(1, std::min<long long>(want_sets, ((long long)cus * resident) / per_set));
    hipLaunchKernelGGL(swin_wmsa_bf16_kernel, dim3((unsigned)(sets * per_set)), dim3(64 * SW_WAVES), 0, stream, (const __bf16*)qkv,
                       (const __bf16*)pad_kv, rpb, (__bf16*)out, H, W, Hp, Wp, heads, shift, scale, (int)windows, zero);
    return (int)hipGetLastError();
}

}  // namespace ppn
