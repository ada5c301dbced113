// upsample_bwd.hip — the backward of the decode heads' bilinear up-sampling kernels of fused_norm.hip (upsample2x_kernel,
// upsample2x_concat_kernel, resize_concat_kernel), so that the heads train on the kernels they infer with:
//
//   upsample2x_bwd_kernel         dx = U^T dy, U the x2 bilinear operator of upsample2x_block; optionally masked by the folded ReLU
//   upsample2x_concat_bwd_kernel  the same on the channel ranges of one dout, level = blockIdx.z
//   resize_concat_bwd_kernel      dx_l = R_l^T dout[..., off_l : off_l + C_l], R_l the forward kernel's float32 taps; level = blockIdx.y
//
// All three are GATHERS: a thread owns 8 channels of its dx elements, reads every dy element that the forward wrote from them, sums in
// float32 in a fixed order and rounds once.  No atomics, no zero-filled buffer, every dx element written exactly once: two runs give the
// same bits (the library's upsample_bilinear2d_backward scatters with atomics: its sums depend on arrival order and, in bfloat16,
// round after every add).
#include <hip/hip_bf16.h>
#include "ppn_device.h"
#include "ppn_kernels.h"
#include "resize_tap.h"

namespace ppn {

namespace {

template <typename T> struct V8;
template <> struct V8<float> {
    static __device__ __forceinline__ void load(const float* p, float (&v)[8]) {
        const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
    static __device__ __forceinline__ void store(float* p, const float (&v)[8]) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
};
template <> struct V8<__hip_bfloat16> {
    static __device__ __forceinline__ void load(const __hip_bfloat16* p, float (&v)[8]) {
        const uint4 u = *reinterpret_cast<const uint4*>(p);
        v[0] = __uint_as_float(u.x << 16); v[1] = __uint_as_float(u.x & 0xffff0000u);
        v[2] = __uint_as_float(u.y << 16); v[3] = __uint_as_float(u.y & 0xffff0000u);
        v[4] = __uint_as_float(u.z << 16); v[5] = __uint_as_float(u.z & 0xffff0000u);
        v[6] = __uint_as_float(u.w << 16); v[7] = __uint_as_float(u.w & 0xffff0000u);
    }
    static __device__ __forceinline__ void store(__hip_bfloat16* p, const float (&v)[8]) {
        *reinterpret_cast<uint4*>(p) = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
    }
};

// Weight of input index r (of n) in output index 2 r + d of the x2 operator: output 2 r - 1 and 2 r + 2 take 0.25 of it, 2 r and
// 2 r + 1 take 0.75 — and the whole of it on the two border outputs, where the forward's clamped neighbour is r itself (output 0:
// weights (1, 0) on rows (0, 1); output 2 n - 1: rows (n - 1, n - 1) with 0.75 + 0.25).  Outputs outside [0, 2 n) do not exist: the
// caller skips them, so d = -1 is only asked for r >= 1 and d = 2 for r <= n - 2.
__device__ __forceinline__ float up2_weight(int d, int r, int n) {
    return d == -1 || d == 2 ? 0.25f : d == 0 ? (r == 0 ? 1.0f : 0.75f) : d == 1 ? (r == n - 1 ? 1.0f : 0.75f) : 0.0f;
}

// The body of one thread, shared by upsample2x_bwd_kernel and upsample2x_concat_bwd_kernel: dy [B][2H][2W][Cy] read at channels
// [yoff, yoff + C), dx [B][H][W][C] written.  The mirror of upsample2x_block: one thread per 8 channels of a 2 x 2 INPUT block
// (rows 2 ib, 2 ib + 1, columns 2 jb, 2 jb + 1).  Its four pixels gather from the 6 x 6 output patch (rows 4 ib - 1 .. 4 ib + 4): 36
// 16-byte loads for four 16-byte stores, 9 per dx pixel instead of the 16 of a pixel-per-thread gather.  The operator is separable: a
// patch row is first summed along x with the column weights (4 taps per input column), then added to the two input rows with the row
// weights — 16 taps per dx element, every weight and weight product exact in float32, a fixed order of sums.
// grid: x = (image, block row) = b * ceil(H / 2) + ib, y = 256-thread pieces of a block row (ceil(W / 2) blocks x C/8 groups).
template <typename T, bool RELU>
__device__ __forceinline__ void upsample2x_bwd_block(const T* __restrict__ dy, const T* __restrict__ x, T* __restrict__ dx, int H, int W, int C,
                                                     int Cy, int yoff) {
    const uint32_t cg = (uint32_t)C >> 3, wb = ((uint32_t)W + 1u) >> 1, hb = ((uint32_t)H + 1u) >> 1;
    const uint32_t e = blockIdx.y * 256u + threadIdx.x;
    if (e >= wb * cg) return;
    const uint32_t jb = e / cg;
    const int c0 = (int)(e - jb * cg) * 8;
    const int b = (int)(blockIdx.x / hb), ib = (int)(blockIdx.x - (uint32_t)b * hb);
    const int r0 = 2 * ib, q0 = 2 * (int)jb;                                 // r0 < H and q0 < W; r0 + 1 / q0 + 1 may be one past the image
    const T* src = dy + (size_t)b * 2 * H * 2 * W * Cy + (yoff + c0);
    float acc[2][2][8];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[a][d][k] = 0.0f;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        const int oy = 2 * r0 - 1 + a;
        if (oy < 0 || oy >= 2 * H) continue;
        float h0[8], h1[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) h0[k] = h1[k] = 0.0f;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const int ox = 2 * q0 - 1 + c;
            if (ox < 0 || ox >= 2 * W) continue;
            float v[8];
            V8<T>::load(src + ((size_t)oy * 2 * W + ox) * Cy, v);
            if (c <= 3) {
                const float w = up2_weight(c - 1, q0, W);
#pragma unroll
                for (int k = 0; k < 8; ++k) h0[k] += w * v[k];
            }
            if (c >= 2) {
                const float w = up2_weight(c - 3, q0 + 1, W);
#pragma unroll
                for (int k = 0; k < 8; ++k) h1[k] += w * v[k];
            }
        }
        if (a <= 3) {
            const float w = up2_weight(a - 1, r0, H);
#pragma unroll
            for (int k = 0; k < 8; ++k) { acc[0][0][k] += w * h0[k]; acc[0][1][k] += w * h1[k]; }
        }
        if (a >= 2) {
            const float w = up2_weight(a - 3, r0 + 1, H);
#pragma unroll
            for (int k = 0; k < 8; ++k) { acc[1][0][k] += w * h0[k]; acc[1][1][k] += w * h1[k]; }
        }
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        if (r0 + a >= H) continue;
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            if (q0 + d >= W) continue;
            const size_t at = (((size_t)b * H + (r0 + a)) * W + (q0 + d)) * C + c0;
            if (RELU) {                                                     // the forward's folded ReLU: grad * (x > 0)
                float xv[8];
                V8<T>::load(x + at, xv);
#pragma unroll
                for (int k = 0; k < 8; ++k) acc[a][d][k] = xv[k] > 0.0f ? acc[a][d][k] : 0.0f;
            }
            V8<T>::store(dx + at, acc[a][d]);
        }
    }
}

}  // namespace

template <typename T, bool RELU>
__global__ __launch_bounds__(256) void upsample2x_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x, T* __restrict__ dx, int H, int W,
                                                             int C) {
    upsample2x_bwd_block<T, RELU>(dy, x, dx, H, W, C, C, 0);
}

struct Up2xConcatBwdParams {
    void* dx[8];
    int C[8], off[8];
};
template <typename T>
__global__ __launch_bounds__(256) void upsample2x_concat_bwd_kernel(Up2xConcatBwdParams p, const T* __restrict__ dout, int H, int W, int Ctot) {
    const int l = (int)blockIdx.z;
    upsample2x_bwd_block<T, false>(dout, nullptr, reinterpret_cast<T*>(p.dx[l]), H, W, p.C[l], Ctot, p.off[l]);
}

int upsample2x_bwd_launch(const void* dy, const void* x, void* dx, int B, int H, int W, int C, int dtype, hipStream_t stream) {
    const long long per_row = (((long long)W + 1) / 2) * (C / 8), rows = (long long)B * ((H + 1) / 2);
    if ((per_row + 255) / 256 > 65535 || rows >= (1LL << 31)) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)rows, (unsigned)((per_row + 255) / 256));
#define PPN_UPB(T, R) hipLaunchKernelGGL((upsample2x_bwd_kernel<T, R>), grid, dim3(256), 0, stream, (const T*)dy, (const T*)x, (T*)dx, H, W, C)
    if (dtype == 0) { if (x) PPN_UPB(float, true); else PPN_UPB(float, false); }
    else { if (x) PPN_UPB(__hip_bfloat16, true); else PPN_UPB(__hip_bfloat16, false); }
#undef PPN_UPB
    return (int)hipGetLastError();
}

int upsample2x_concat_bwd_launch(const void* dout, void* const* dx, const int* ch, int n, int B, int H, int W, int dtype, hipStream_t stream) {
    Up2xConcatBwdParams p;
    int off = 0, cmax = 0;
    for (int l = 0; l < 8; ++l) {
        const int k = l < n ? l : 0;
        p.dx[l] = dx[k]; p.C[l] = ch[k]; p.off[l] = off;
        if (l < n) { off += ch[l]; cmax = ch[l] > cmax ? ch[l] : cmax; }
    }
    const long long per_row = (((long long)W + 1) / 2) * (cmax / 8), rows = (long long)B * ((H + 1) / 2);
    if ((per_row + 255) / 256 > 65535 || rows >= (1LL << 31)) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)rows, (unsigned)((per_row + 255) / 256), (unsigned)n);
    if (dtype == 0) hipLaunchKernelGGL(upsample2x_concat_bwd_kernel<float>, grid, dim3(256), 0, stream, p, (const float*)dout, H, W, off);
    else hipLaunchKernelGGL(upsample2x_concat_bwd_kernel<__hip_bfloat16>, grid, dim3(256), 0, stream, p, (const __hip_bfloat16*)dout, H, W, off);
    return (int)hipGetLastError();
}

// The transpose of resize_concat_kernel: one thread per 8 channels of one INPUT pixel (r, q) of level l = blockIdx.y.  A level of
// level 0's size copies its channel slice.  Otherwise the thread walks the output rows / columns that can name r / q as a tap — the
// exact range is src in (r - 1, r + 1), i.e. (2 i + 1) H_l in ((2 r - 1) H_0, (2 r + 3) H_0), taken one wider on both sides — and
// decides every candidate with the FORWARD's float32 arithmetic.  resize_concat_kernel (fused_norm.hip) carries that arithmetic inline;
// bilinear_tap (resize_tap.h) is the same sequence of float32 operations — scale = in / out, source index scale (dst + 0.5) - 0.5
// clamped at 0, truncation, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1 — and the build has -ffp-contract=off, so the two give
// the same floats (tests/test_gpu_upsample_bwd.py compares the backward with the forward kernel's own weights, read out through
// one-hot images): forward and backward agree on every tap, also where the float32 source index falls on an integer.
// A tap clamped onto r twice (the last row: y1 = y0) enters with both weights.  Row sums along x first, then the row weight: a fixed
// order.  A 1 x 1 level gathers the whole H_0 x W_0 image per thread — the pyramid's sizes (at most 64 x 64) keep that short.
struct ConcatBwdParams {
    void* dx[8];
    int H[8], W[8], C[8], off[8];
    int Ctot;
};

namespace {
// the candidates only, in integers: the kernel tests each one itself (resize_tap.h's tap_range scans for the exact first / last member)
__device__ __forceinline__ void candidate_range(int r, int n_in, int n_out, int& lo, int& hi) {
    const long long a = ((2LL * r - 1) * n_out - n_in) / (2LL * n_in) - 1, b = ((2LL * r + 3) * n_out - n_in) / (2LL * n_in) + 1;
    lo = (int)(a < 0 ? 0 : a);
    hi = (int)(b > n_out - 1 ? n_out - 1 : b);
}
// tap_weight: resize_tap.h
}  // namespace

template <typename T>
__global__ __launch_bounds__(256) void resize_concat_bwd_kernel(ConcatBwdParams p, const T* __restrict__ dout, int B) {
    const int l = (int)blockIdx.y;
    const int Hl = p.H[l], Wl = p.W[l], C = p.C[l], cg = C >> 3;
    const int H0 = p.H[0], W0 = p.W[0];
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)B * Hl * Wl * cg) return;
    const int g = (int)(idx % cg);
    const long long pix = idx / cg;
    const int q = (int)(pix % Wl), r = (int)((pix / Wl) % Hl), b = (int)(pix / ((long long)Wl * Hl));
    const T* src = dout + (size_t)b * H0 * W0 * p.Ctot + p.off[l] + g * 8;
    T* dst = reinterpret_cast<T*>(p.dx[l]) + (size_t)pix * C + g * 8;
    float acc[8];
    if (Hl == H0 && Wl == W0) {
        V8<T>::load(src + ((size_t)r * W0 + q) * p.Ctot, acc);
    } else {
        int i_lo, i_hi, j_lo, j_hi;
        candidate_range(r, Hl, H0, i_lo, i_hi);
        candidate_range(q, Wl, W0, j_lo, j_hi);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = 0.0f;
        for (int i = i_lo; i <= i_hi; ++i) {
            const Tap ty = bilinear_tap(i, Hl, H0);
            if (ty.i0 != r && ty.i1 != r) continue;
            const float wy = tap_weight(ty, r);
            float row[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) row[k] = 0.0f;
            const T* line = src + (size_t)i * W0 * p.Ctot;
            for (int j = j_lo; j <= j_hi; ++j) {
                const Tap tx = bilinear_tap(j, Wl, W0);
                if (tx.i0 != q && tx.i1 != q) continue;
                const float wx = tap_weight(tx, q);
                float v[8];
                V8<T>::load(line + (size_t)j * p.Ctot, v);
#pragma unroll
                for (int k = 0; k < 8; ++k) row[k] += wx * v[k];
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] += wy * row[k];
        }
    }
    V8<T>::store(dst, acc);
}

int resize_concat_bwd_launch(const void* dout, void* const* dx, const int* hw, const int* ch, int n, int B, int dtype, hipStream_t stream) {
    ConcatBwdParams p;
    int off = 0;
    long long most = 0;
    for (int l = 0; l < 8; ++l) {
        const int k = l < n ? l : 0;
        p.dx[l] = dx[k]; p.H[l] = hw[2 * k]; p.W[l] = hw[2 * k + 1]; p.C[l] = ch[k]; p.off[l] = off;
        if (l < n) {
            off += ch[l];
            const long long t = (long long)B * hw[2 * l] * hw[2 * l + 1] * (ch[l] / 8);
            most = t > most ? t : most;
        }
    }
    p.Ctot = off;
    if ((most + 255) / 256 >= (1LL << 31)) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)((most + 255) / 256), (unsigned)n);
    if (dtype == 0) hipLaunchKernelGGL(resize_concat_bwd_kernel<float>, grid, dim3(256), 0, stream, p, (const float*)dout, B);
    else hipLaunchKernelGGL(resize_concat_bwd_kernel<__hip_bfloat16>, grid, dim3(256), 0, stream, p, (const __hip_bfloat16*)dout, B);
    return (int)hipGetLastError();
}

}  // namespace ppn
