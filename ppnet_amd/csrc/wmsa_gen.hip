// wmsa_gen.hip — (shifted-)window multi-head self-attention, forward, for the windows and head dims of GenNet's AESwin (reference
// GenNet/networks/vanilla_swin.py:239-284,325-376,429-454 between the qkv and the proj Linear): swin_wmsa.hip's semantics and index
// arithmetic generalised over (window w, head dim d).  w = 14 with d in {8, 16, 32} and w = 7 with d in {8, 16} run here; (7, 32)
// is Swin-B's shape and stays on swin_wmsa.hip (the launcher below forwards it).
//
// The padding to multiples of the window, the cyclic shift, window_partition, window_reverse, the reverse roll and the crop are
// index arithmetic: window (wy, wx), slot (i, j) is the padded-grid position ((w wy + i + shift) mod Hp, (w wx + j + shift) mod Wp),
// and only real tokens are read or written.  A padded position is a key / value whose k, v are pad_kv (the reference pads BEFORE
// the qkv Linear, so a padded token's k / v is the projection's bias).  Logit = (q scale) . k + rpb[h][dy + w-1][dx + w-1] (dy, dx
// = query minus key inside the window) and, on the last window row / column of a shifted layer, -100 (NOT -inf,
// vanilla_swin.py:453) between slots of different regions.  The reference keeps the shift when one window covers the whole grid: a
// 14 x 14 grid under window 14, shift 7 is one window with four mask regions.
//
// One kernel form for both data types (the float32 kernel of swin_wmsa.hip and the kernels of mhsa_d8.hip are the models): one
// workgroup per (image, window, head), one query slot per lane (196 live lanes of 256 at w = 14, 49 of 64 at w = 7).  The window's
// K and V are staged in LDS as float32 (w = 14, d = 32: 196 x 32 x 2 x 4 B = 49 KB; bfloat16 is converted on load), padded slots
// from pad_kv, and so is the head's (2w-1)^2 bias table (2.8 KB).  A lane keeps its scaled q row and its output row in registers
// and walks the keys twice: the first walk takes the maximum of the logits, the second recomputes each logit with the same
// operations in the same order (bit-equal, so every exponent is <= 0), exponentiates and accumulates P . V.  Every lane reads the
// same K / V address at a time (an LDS broadcast).  Nothing of size N x N exists anywhere; no atomics; one writer per output
// element; the output is rounded once.
//
// Offsets of tokens are 64-bit; window numbers are 32-bit (the caller rejects launches of 2^31 work-items or more).
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include "ppn_device.h"
#include "ppn_kernels.h"

namespace ppn {

namespace {
template <int WN>
struct WmsaShape {
    static constexpr int N = WN * WN, T = 2 * WN - 1, THREADS = N <= 64 ? 64 : 256;
};

// token index (b, py, px) of window slot `sl` (0 .. w^2 - 1), or -1 when the slot is a padded position
template <int WN>
__device__ __forceinline__ long long gen_slot_token(int sl, int b, int wy, int wx, int H, int W, int Hp, int Wp, int shift) {
    const int kr = sl / WN, kc = sl - WN * kr;
    int py = WN * wy + kr + shift, px = WN * wx + kc + shift;           // < 2 Hp, < 2 Wp: shift < w <= Hp, Wp
    py -= py >= Hp ? Hp : 0;
    px -= px >= Wp ? Wp : 0;
    if (py >= H || px >= W) return -1;
    return ((long long)b * H + py) * W + px;
}

// four consecutive elements at element offset `off` (a multiple of 4) as float32
template <bool BF16>
__device__ __forceinline__ float4 load4(const void* base, size_t off) {
    if constexpr (BF16) {
        const uint2 r = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(base) + off);
        return make_float4(__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xffff0000u), __uint_as_float(r.y << 16),
                           __uint_as_float(r.y & 0xffff0000u));
    } else {
        return *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(base) + off);
    }
}

template <bool BF16>
__device__ __forceinline__ void store4(void* base, size_t off, float a, float b, float c, float d) {
    if constexpr (BF16)
        *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(base) + off) = make_uint2(pack_bf16x2(a, b), pack_bf16x2(c, d));
    else
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(base) + off) = make_float4(a, b, c, d);
}
}  // namespace

template <int WN, int D, bool BF16>
__global__ __launch_bounds__(WmsaShape<WN>::THREADS) void wmsa_gen_kernel(const void* __restrict__ qkv, const void* __restrict__ pad_kv,
                                                                         const float* __restrict__ rpb, void* __restrict__ out, int H, int W,
                                                                         int Hp, int Wp, int heads, int shift, float scale) {
    constexpr int N = WmsaShape<WN>::N, T = WmsaShape<WN>::T, NT = WmsaShape<WN>::THREADS, CH = D / 4;
    __shared__ __attribute__((aligned(16))) float kv[2][N * D];        // K and V of the window, float32, [slot][d]
    __shared__ float tb[T * T];                                        // this head's bias table [dy + w-1][dx + w-1]
    const int lane = threadIdx.x, h = blockIdx.y;
    const int nWx = Wp / WN, nWy = Hp / WN, nW = nWx * nWy;
    const int grp = blockIdx.x, b = grp / nW, wi = grp - b * nW, wy = wi / nWx, wx = wi - wy * nWx;
    const size_t C = (size_t)heads * D;
    for (int i = lane; i < N * 2 * CH; i += NT) {                      // (slot, k / v, 4-element chunk)
        const int c4 = i % CH, t = (i / CH) & 1, sl = i / (2 * CH);
        const long long tok = gen_slot_token<WN>(sl, b, wy, wx, H, W, Hp, Wp, shift);
        const size_t off = (size_t)(1 + t) * C + (size_t)h * D + 4 * c4;
        const float4 x = tok >= 0 ? load4<BF16>(qkv, (size_t)tok * 3 * C + off) : load4<BF16>(pad_kv, off);
        *reinterpret_cast<float4*>(&kv[t][sl * D + 4 * c4]) = x;
    }
    for (int i = lane; i < T * T; i += NT) tb[i] = rpb[(size_t)h * (T * T) + i];
    __syncthreads();
    if (lane >= N) return;
    const long long qtok = gen_slot_token<WN>(lane, b, wy, wx, H, W, Hp, Wp, shift);
    if (qtok < 0) return;                                              // a padded query: cropped by the reference, never written
    float q[D];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const float4 x = load4<BF16>(qkv, (size_t)qtok * 3 * C + (size_t)h * D + 4 * c);
        q[4 * c] = x.x * scale, q[4 * c + 1] = x.y * scale, q[4 * c + 2] = x.z * scale, q[4 * c + 3] = x.w * scale;   // q * scale first
    }
    const int u = lane / WN, v = lane - WN * u, thr = WN - shift;
    const bool lastr = shift > 0 && wy == nWy - 1, lastc = shift > 0 && wx == nWx - 1;
    const bool qr = u < thr, qc = v < thr;                             // the query's region on each axis of a last window row / column
    const float* tq = tb + (u + WN - 1) * T + (v + WN - 1);            // + bias of key (kr, kc) at tq[-(kr T + kc)]
    // the logit of key slot k = (kr, kc): both walks call this, so the two values are bit-equal
    auto logit = [&](int k, int kr, int kc) {
        const float* kp = &kv[0][k * D];
        float acc = 0.0f;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const float4 x = *reinterpret_cast<const float4*>(kp + 4 * c);
            acc = __builtin_fmaf(q[4 * c], x.x, acc);
            acc = __builtin_fmaf(q[4 * c + 1], x.y, acc);
            acc = __builtin_fmaf(q[4 * c + 2], x.z, acc);
            acc = __builtin_fmaf(q[4 * c + 3], x.w, acc);
        }
        acc += tq[-(kr * T + kc)];
        if ((lastr && (qr != (kr < thr))) || (lastc && (qc != (kc < thr)))) acc += -100.0f;
        return acc;
    };
    float mx = -3.0e38f;
#pragma unroll 1                                                       // one window row of keys at a time: 49 unrolled keys take 400 registers
    for (int kr = 0, k = 0; kr < WN; ++kr)
        for (int kc = 0; kc < WN; ++kc, ++k) mx = fmaxf(mx, logit(k, kr, kc));
    float sum = 0.0f, o[D];
#pragma unroll
    for (int d = 0; d < D; ++d) o[d] = 0.0f;
#pragma unroll 1
    for (int kr = 0, k = 0; kr < WN; ++kr)
        for (int kc = 0; kc < WN; ++kc, ++k) {
            const float p = expf(logit(k, kr, kc) - mx);
            sum += p;
            const float* vp = &kv[1][k * D];
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const float4 x = *reinterpret_cast<const float4*>(vp + 4 * c);
                o[4 * c] = __builtin_fmaf(p, x.x, o[4 * c]);
                o[4 * c + 1] = __builtin_fmaf(p, x.y, o[4 * c + 1]);
                o[4 * c + 2] = __builtin_fmaf(p, x.z, o[4 * c + 2]);
                o[4 * c + 3] = __builtin_fmaf(p, x.w, o[4 * c + 3]);
            }
        }
    const float inv = 1.0f / sum;
    const size_t dst = (size_t)qtok * C + (size_t)h * D;
#pragma unroll
    for (int d = 0; d < D; d += 4) store4<BF16>(out, dst + d, o[d] * inv, o[d + 1] * inv, o[d + 2] * inv, o[d + 3] * inv);
}

int wmsa_gen_threads(int window) { return window == 7 ? WmsaShape<7>::THREADS : WmsaShape<14>::THREADS; }

namespace {
template <int WN, int D>
int launch_wd(const void* qkv, const void* pad_kv, const float* rpb, void* out, int B, int H, int W, int heads, int shift, float scale, int dtype,
              hipStream_t stream) {
    const int Hp = (H + WN - 1) / WN * WN, Wp = (W + WN - 1) / WN * WN;
    const long long windows = (long long)B * (Hp / WN) * (Wp / WN);
    const dim3 grid((unsigned)windows, (unsigned)heads), block(WmsaShape<WN>::THREADS);
    if (dtype == 0)
        hipLaunchKernelGGL((wmsa_gen_kernel<WN, D, false>), grid, block, 0, stream, qkv, pad_kv, rpb, out, H, W, Hp, Wp, heads, shift, scale);
    else
        hipLaunchKernelGGL((wmsa_gen_kernel<WN, D, true>), grid, block, 0, stream, qkv, pad_kv, rpb, out, H, W, Hp, Wp, heads, shift, scale);
    return (int)hipGetLastError();
}
}  // namespace

// B, H, W, heads > 0, (window, head_dim) in the supported set, shift in {0, window / 2}, 16-byte aligned buffers and a launch below
// 2^31 work-items: checked by the caller (capi.hip)
int wmsa_gen_launch(const void* qkv, const void* pad_kv, const float* rpb, void* out, int B, int H, int W, int heads, int head_dim, int window,
                    int shift, float scale, int dtype, hipStream_t stream) {
    if (window == 7 && head_dim == 32) return swin_wmsa_launch(qkv, pad_kv, rpb, out, B, H, W, heads, shift, scale, dtype, stream);
    if (window == 14 && head_dim == 8) return launch_wd<14, 8>(qkv, pad_kv, rpb, out, B, H, W, heads, shift, scale, dtype, stream);
    if (window == 14 && head_dim == 16) return launch_wd<14, 16>(qkv, pad_kv, rpb, out, B, H, W, heads, shift, scale, dtype, stream);
    if (window == 14 && head_dim == 32) return launch_wd<14, 32>(qkv, pad_kv, rpb, out, B, H, W, heads, shift, scale, dtype, stream);
    if (window == 7 && head_dim == 8) return launch_wd<7, 8>(qkv, pad_kv, rpb, out, B, H, W, heads, shift, scale, dtype, stream);
    if (window == 7 && head_dim == 16) return launch_wd<7, 16>(qkv, pad_kv, rpb, out, B, H, W, heads, shift, scale, dtype, stream);
    return (int)hipErrorInvalidValue;
}

}  // namespace ppn
