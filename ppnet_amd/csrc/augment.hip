// augment.hip — SegNet's training input: the reference's RandomFlip + PhotoMetricDistortion + Normalize + Pad
// (SegNet/configs/_base_/datasets/planning_seg.py:18-27, mmseg/datasets/pipelines/transforms.py:835-940) on the device.
//
// PhotoMetricDistortion is a per-pixel colour function with per-image parameters, so the distorted palette image of stage B's
// occupancy codes still has three colours per image: ppn_augment_codes distorts the three palette colours once per workgroup and
// expands the codes with selects, as grid_image_kernel (fused_norm.hip) does.  ppn_augment_rgb runs the same device function on
// every pixel of a u8 RGB image.  ppn_augment_params draws the per-image parameters from Philox (stream STREAM_AUG, instance =
// global image index, ten fixed draw slots).
//
// The colour function is integer / float32 arithmetic that the host restates exactly (ppnet_amd/augment.py):
// convert = two separately rounded float32 operations, clip, truncate; 8-bit HSV in exact integer arithmetic, round half up.
#include <hip/hip_bf16.h>
#include "ppn_device.h"
#include "ppn_kernels.h"

namespace ppn {

namespace {

constexpr int AUG_THREADS = 256;
constexpr int AUG_PX = 8;                       // consecutive output pixels of a row per work-item

struct AugParams { uint32_t flags; float beta, alpha, alpha_s; int delta; };

__device__ __forceinline__ AugParams load_params(const uint32_t* __restrict__ params, int b) {
    const uint4 w0 = *reinterpret_cast<const uint4*>(params + (size_t)b * PPN_AUG_PARAM_WORDS);
    const uint32_t w4 = params[(size_t)b * PPN_AUG_PARAM_WORDS + 4];
    AugParams p;
    p.flags = w0.x; p.beta = __uint_as_float(w0.y); p.alpha = __uint_as_float(w0.z); p.alpha_s = __uint_as_float(w0.w);
    p.delta = (int)w4;
    return p;
}

// PhotoMetricDistortion.convert (transforms.py:865-869): float32(x) * alpha + beta, clipped to [0, 255], truncated
__device__ __forceinline__ int convert(int x, float alpha, float beta) {
    const float f = __fadd_rn(__fmul_rn((float)x, alpha), beta);
    return (int)fminf(fmaxf(f, 0.0f), 255.0f);              // fmaxf(NaN, 0) = 0: whatever the parameters hold, the result is in [0, 255]
}

// 8-bit HSV (H in [0, 180)), exact integers, round half up
__device__ __forceinline__ void bgr2hsv(int b, int g, int r, int& h, int& s, int& v) {
    v = max(r, max(g, b));
    const int m = min(r, min(g, b)), d = v - m;
    s = v ? (int)((uint32_t)(2 * 255 * d + v) / (uint32_t)(2 * v)) : 0;
    int n = (v == r) ? g - b : (v == g) ? b - r + 2 * d : r - g + 4 * d;
    if (n < 0) n += 6 * d;
    h = d ? (int)(((uint32_t)(60 * n + d) / (uint32_t)(2 * d)) % 180u) : 0;
}

__device__ __forceinline__ int rdiv(int a, int b) { return (int)((uint32_t)(2 * a + b) / (uint32_t)(2 * b)); }

__device__ __forceinline__ void hsv2bgr(int h, int s, int v, int& b, int& g, int& r) {
    const int sec = h / 30, f = h - sec * 30;
    const int p = rdiv(v * (255 - s), 255), q = rdiv(v * (7650 - s * f), 7650), t = rdiv(v * (7650 - s * (30 - f)), 7650);
    r = (sec == 0 || sec == 5) ? v : (sec == 1) ? q : (sec == 4) ? t : p;
    g = (sec == 1 || sec == 2) ? v : (sec == 0) ? t : (sec == 3) ? q : p;
    b = (sec == 3 || sec == 4) ? v : (sec == 2) ? t : (sec == 5) ? q : p;
}

// PhotoMetricDistortion.__call__ on one BGR pixel; every branch is uniform over the image
__device__ __forceinline__ void distort(const AugParams& p, int& b, int& g, int& r) {
    if (p.flags & PPN_AUG_BRIGHTNESS) { b = convert(b, 1.0f, p.beta); g = convert(g, 1.0f, p.beta); r = convert(r, 1.0f, p.beta); }
    const bool contrast = (p.flags & PPN_AUG_CONTRAST) != 0, last = (p.flags & PPN_AUG_CONTRAST_LAST) != 0;
    if (contrast && !last) { b = convert(b, p.alpha, 0.0f); g = convert(g, p.alpha, 0.0f); r = convert(r, p.alpha, 0.0f); }
    if (p.flags & PPN_AUG_SATURATION) {
        int h, s, v;
        bgr2hsv(b, g, r, h, s, v);
        s = convert(s, p.alpha_s, 0.0f);
        hsv2bgr(h, s, v, b, g, r);
    }
    if (p.flags & PPN_AUG_HUE) {
        int h, s, v;
        bgr2hsv(b, g, r, h, s, v);
        h = (h + p.delta % 180) % 180;                      // delta reduced first: no overflow for any int32 a caller writes
        if (h < 0) h += 180;
        hsv2bgr(h, s, v, b, g, r);
    }
    if (contrast && last) { b = convert(b, p.alpha, 0.0f); g = convert(g, p.alpha, 0.0f); r = convert(r, p.alpha, 0.0f); }
}

// Normalize: grid_image_launch's expression
__device__ __forceinline__ float normalise(int v, float mean, float stdv) { return __fdiv_rn(__fsub_rn((float)v, mean), stdv); }

struct Norm { float mean[3], stdv[3]; };

// the 24 values of a work-item's eight pixels, in memory order
__device__ __forceinline__ void store24(float* out, const float (&v)[24]) {
#pragma unroll
    for (int q = 0; q < 6; ++q) *reinterpret_cast<float4*>(out + 4 * q) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}
__device__ __forceinline__ void store24(__hip_bfloat16* out, const float (&v)[24]) {
#pragma unroll
    for (int q = 0; q < 3; ++q)
        *reinterpret_cast<uint4*>(out + 8 * q) = make_uint4(pack_bf16x2(v[8 * q], v[8 * q + 1]), pack_bf16x2(v[8 * q + 2], v[8 * q + 3]),
                                                             pack_bf16x2(v[8 * q + 4], v[8 * q + 5]), pack_bf16x2(v[8 * q + 6], v[8 * q + 7]));
}

// eight bytes in reversed order
__device__ __forceinline__ uint2 reverse8(uint2 g) { return make_uint2(__builtin_bswap32(g.y), __builtin_bswap32(g.x)); }

// Where a work-item's eight output pixels come from.  The workgroup's image is b; `inside` = the pixels lie in the H x W source
// (W and Wo are multiples of 8, so a group of eight is inside or outside as a whole); src = offset of the eight source pixels in
// their [H][W] image (the mirrored group when flipped: its pixels are then taken in reversed order).
struct Place { bool active, inside; long long out_px; int src; };
__device__ __forceinline__ Place place(int groups_per_image, int H, int W, int Ho, int Wo, bool flip, int& b) {
    b = (int)(blockIdx.x / (unsigned)groups_per_image);
    const int gi = (int)(blockIdx.x - (unsigned)b * (unsigned)groups_per_image) * AUG_THREADS + (int)threadIdx.x;
    const int wo8 = Wo / AUG_PX;
    Place pl;
    pl.active = gi < Ho * wo8;
    const int y = gi / wo8, x0 = (gi - y * wo8) * AUG_PX;
    pl.inside = pl.active && y < H && x0 < W;
    pl.out_px = ((long long)b * Ho + y) * Wo + x0;
    pl.src = y * W + (flip ? W - AUG_PX - x0 : x0);
    return pl;
}

// the eight labels of a work-item, flipped and padded like its pixels (read before the workgroup's barrier, written after it)
__device__ __forceinline__ uint2 get_labels(const uint8_t* __restrict__ label_in, const uint8_t* label_out, const Place& pl, int b, int H, int W,
                                            bool flip, int seg_pad_val) {
    const uint32_t pad = (uint32_t)(seg_pad_val & 0xff) * 0x01010101u;
    uint2 l = make_uint2(pad, pad);
    if (label_out && pl.inside) {
        l = *reinterpret_cast<const uint2*>(label_in + (long long)b * H * W + pl.src);
        if (flip) l = reverse8(l);
    }
    return l;
}
__device__ __forceinline__ void put_labels(uint8_t* __restrict__ label_out, const Place& pl, uint2 l) {
    if (label_out) *reinterpret_cast<uint2*>(label_out + pl.out_px) = l;
}

}  // namespace

// One work-item per image: the ten draws of (seed, STREAM_AUG, first_instance + b) and the eight parameter words.
__global__ __launch_bounds__(AUG_THREADS) void augment_params_kernel(uint64_t seed, uint64_t first_instance, int B, double flip_ratio,
                                                                     double brightness_delta, double contrast_lo, double contrast_hi,
                                                                     double saturation_lo, double saturation_hi, int hue_delta,
                                                                     uint32_t* __restrict__ params) {
    const int b = (int)(blockIdx.x * AUG_THREADS + threadIdx.x);
    if (b >= B) return;
    double d[10];
#pragma unroll
    for (int k = 0; k < 5; ++k) philox_double2(seed, STREAM_AUG, first_instance + (uint64_t)b, (uint32_t)k, d[2 * k], d[2 * k + 1]);
    uint32_t flags = 0;
    if (d[0] < flip_ratio) flags |= PPN_AUG_FLIP;
    if (d[1] < 0.5) flags |= PPN_AUG_BRIGHTNESS;
    if (!(d[3] < 0.5)) flags |= PPN_AUG_CONTRAST_LAST;
    if (d[4] < 0.5) flags |= PPN_AUG_CONTRAST;
    if (d[6] < 0.5) flags |= PPN_AUG_SATURATION;
    if (d[8] < 0.5) flags |= PPN_AUG_HUE;
    const float beta = (float)(-brightness_delta + (2.0 * brightness_delta) * d[2]);
    const float alpha = (float)(contrast_lo + (contrast_hi - contrast_lo) * d[5]);
    const float alpha_s = (float)(saturation_lo + (saturation_hi - saturation_lo) * d[7]);
    const int delta = -hue_delta + (int)floor((double)(2 * hue_delta) * d[9]);
    uint4* out = reinterpret_cast<uint4*>(params + (size_t)b * PPN_AUG_PARAM_WORDS);
    out[0] = make_uint4(flags, __float_as_uint(beta), __float_as_uint(alpha), __float_as_uint(alpha_s));
    out[1] = make_uint4((uint32_t)delta, 0u, 0u, 0u);
}

// Occupancy codes -> distorted, normalised, flipped, padded palette image (+ labels).  Prologue: lanes 0..2 distort the palette
// colours free / marker / obstacle and leave their normalised RGB values in LDS; afterwards a pixel costs selects only.
template <typename T>
__global__ __launch_bounds__(AUG_THREADS) void augment_codes_kernel(const uint8_t* __restrict__ grid, const uint8_t* __restrict__ label_in,
                                                                    const uint32_t* __restrict__ params, T* __restrict__ img,
                                                                    uint8_t* __restrict__ label_out, int groups_per_image, int H, int W, int Ho,
                                                                    int Wo, Norm nm, int seg_pad_val) {
    __shared__ float pal[3][3];
    int b;
    const AugParams prm = load_params(params, (int)(blockIdx.x / (unsigned)groups_per_image));
    const bool flip = (prm.flags & PPN_AUG_FLIP) != 0;
    const Place pl = place(groups_per_image, H, W, Ho, Wo, flip, b);
    // the work-item's loads go out before the prologue and its barrier: they depend on the flip flag only
    uint2 g = make_uint2(0u, 0u);
    if (pl.inside) {
        g = *reinterpret_cast<const uint2*>(grid + (long long)b * H * W + pl.src);
        if (flip) g = reverse8(g);
    }
    const uint2 lab = get_labels(label_in, label_out, pl, b, H, W, flip, seg_pad_val);
    if (threadIdx.x < 3) {
        // BGR of the palette (process_map.py:120,128): free white, marker red, obstacle black
        int pb = threadIdx.x == 0 ? 255 : 0, pg = pb, pr = threadIdx.x == 2 ? 0 : 255;
        distort(prm, pb, pg, pr);
        pal[threadIdx.x][0] = normalise(pr, nm.mean[0], nm.stdv[0]);
        pal[threadIdx.x][1] = normalise(pg, nm.mean[1], nm.stdv[1]);
        pal[threadIdx.x][2] = normalise(pb, nm.mean[2], nm.stdv[2]);
    }
    __syncthreads();
    if (!pl.active) return;
    float v[24];
    if (pl.inside) {
        const float f0 = pal[0][0], f1 = pal[0][1], f2 = pal[0][2], m0 = pal[1][0], m1 = pal[1][1], m2 = pal[1][2];
        const float o0 = pal[2][0], o1 = pal[2][1], o2 = pal[2][2];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t code = ((k < 4 ? g.x : g.y) >> (8 * (k & 3))) & 0xffu;
            const bool free_ = code == PPN_GRID_FREE, mark = code == PPN_GRID_MARK;
            v[3 * k] = free_ ? f0 : mark ? m0 : o0;
            v[3 * k + 1] = free_ ? f1 : mark ? m1 : o1;
            v[3 * k + 2] = free_ ? f2 : mark ? m2 : o2;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 24; ++k) v[k] = 0.0f;
    }
    store24(img + pl.out_px * 3, v);
    put_labels(label_out, pl, lab);
}

// u8 RGB image -> the same output; the colour function runs per pixel, Normalize is a 3 x 256 table in LDS.
template <typename T>
__global__ __launch_bounds__(AUG_THREADS) void augment_rgb_kernel(const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ label_in,
                                                                  const uint32_t* __restrict__ params, T* __restrict__ img,
                                                                  uint8_t* __restrict__ label_out, int groups_per_image, int H, int W, int Ho,
                                                                  int Wo, Norm nm, int seg_pad_val) {
    __shared__ float table[3][256];
    static_assert(AUG_THREADS == 256, "one table column per work-item");
    int b;
    const AugParams prm = load_params(params, (int)(blockIdx.x / (unsigned)groups_per_image));
    const bool flip = (prm.flags & PPN_AUG_FLIP) != 0;
    const Place pl = place(groups_per_image, H, W, Ho, Wo, flip, b);
    // loads before the table and its barrier, as in the codes kernel
    uint2 s0 = make_uint2(0u, 0u), s1 = s0, s2 = s0;
    if (pl.inside) {
        const uint2* src = reinterpret_cast<const uint2*>(rgb + ((long long)b * H * W + pl.src) * 3);
        s0 = src[0]; s1 = src[1]; s2 = src[2];
    }
    const uint2 lab = get_labels(label_in, label_out, pl, b, H, W, flip, seg_pad_val);
#pragma unroll
    for (int c = 0; c < 3; ++c) table[c][threadIdx.x] = normalise((int)threadIdx.x, nm.mean[c], nm.stdv[c]);
    __syncthreads();
    if (!pl.active) return;
    float v[24];
    if (pl.inside) {
        const uint32_t w[6] = {s0.x, s0.y, s1.x, s1.y, s2.x, s2.y};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            int ch[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int fwd = 3 * k + c, rev = 3 * (7 - k) + c;           // byte of the 24, both known at compile time
                const uint32_t a = (w[fwd >> 2] >> (8 * (fwd & 3))) & 0xffu, z = (w[rev >> 2] >> (8 * (rev & 3))) & 0xffu;
                ch[c] = (int)(flip ? z : a);
            }
            int r = ch[0], g = ch[1], bl = ch[2];
            distort(prm, bl, g, r);
            v[3 * k] = table[0][r];
            v[3 * k + 1] = table[1][g];
            v[3 * k + 2] = table[2][bl];
        }
    } else {
#pragma unroll
        for (int k = 0; k < 24; ++k) v[k] = 0.0f;
    }
    store24(img + pl.out_px * 3, v);
    put_labels(label_out, pl, lab);
}

int augment_threads() { return AUG_THREADS; }
int augment_pixels() { return AUG_THREADS * AUG_PX; }

int augment_params_launch(uint64_t seed, uint64_t first_instance, int B, double flip_ratio, double brightness_delta, double contrast_lo,
                          double contrast_hi, double saturation_lo, double saturation_hi, int hue_delta, uint32_t* params, hipStream_t stream) {
    hipLaunchKernelGGL(augment_params_kernel, dim3((unsigned)((B + AUG_THREADS - 1) / AUG_THREADS)), dim3(AUG_THREADS), 0, stream, seed,
                       first_instance, B, flip_ratio, brightness_delta, contrast_lo, contrast_hi, saturation_lo, saturation_hi, hue_delta, params);
    return (int)hipGetLastError();
}

int augment_launch(int rgb, const uint8_t* in, const uint8_t* label_in, const uint32_t* params, void* img, uint8_t* label_out, int B, int H, int W,
                   int Ho, int Wo, const float* mean, const float* stdv, int seg_pad_val, int dtype, hipStream_t stream) {
    const int per = augment_pixels(), groups = (int)(((long long)Ho * Wo + per - 1) / per);
    const dim3 g((unsigned)((long long)B * groups)), t(AUG_THREADS);
    Norm nm;
    for (int c = 0; c < 3; ++c) { nm.mean[c] = mean[c]; nm.stdv[c] = stdv[c]; }
    if (rgb) {
        if (dtype == 0) hipLaunchKernelGGL((augment_rgb_kernel<float>), g, t, 0, stream, in, label_in, params, (float*)img, label_out, groups, H, W, Ho, Wo, nm, seg_pad_val);
        else hipLaunchKernelGGL((augment_rgb_kernel<__hip_bfloat16>), g, t, 0, stream, in, label_in, params, (__hip_bfloat16*)img, label_out, groups, H, W, Ho, Wo, nm, seg_pad_val);
    } else {
        if (dtype == 0) hipLaunchKernelGGL((augment_codes_kernel<float>), g, t, 0, stream, in, label_in, params, (float*)img, label_out, groups, H, W, Ho, Wo, nm, seg_pad_val);
        else hipLaunchKernelGGL((augment_codes_kernel<__hip_bfloat16>), g, t, 0, stream, in, label_in, params, (__hip_bfloat16*)img, label_out, groups, H, W, Ho, Wo, nm, seg_pad_val);
    }
    return (int)hipGetLastError();
}

}  // namespace ppn
