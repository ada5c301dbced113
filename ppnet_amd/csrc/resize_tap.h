// resize_tap.h — what the kernels on a bilinearly resized logit share: resize_ce.hip (the heads' cross-entropy), seg_eval.hip (the
// evaluation's area histograms), ohem_ce.hip (cross-entropy under OHEM), resize_dice.hip (the Dice loss); upsample_bwd.hip takes the
// taps and tap_weight.  One definition of each piece, so that a fix reaches every kernel at once:
//   taps      Tap, bilinear_tap — torch's float32 rule for F.interpolate(bilinear, align_corners=False) with the size given —, ldf / stf,
//             interp, valid_label: the interpolated logit of a pixel, and with it the argmax, is the same float in every kernel of every
//             file (the build has -ffp-contract=off: no kernel fuses the products differently)
//   forward   softmax_sweep (maximum, argmax, z_label, sum of exponentials), group_sum (a workgroup's (float, int) partial) and
//             final_sum (the last workgroup's (double, int64) tree)
//   backward  tap_range, tap_weight and Gather, the one-writer gather of a dlogit element: forward and backward of every loss agree
//             on which pixels exist
//   host      dispatch_types (the C ABI's dtype codes -> the template's types) and dispatch_lanes (the gather's LANES instance)
// Everything is inline, in an anonymous namespace: the kernels, their names and their launches stay in their own files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "ppn_kernels.h"

namespace ppn {

namespace {
struct Tap { int i0, i1; float l0, l1; };

// torch's area_pixel_compute_source_index (align_corners=False, no scale factor given) in float32, and upsample_bilinear2d's taps
__device__ __forceinline__ Tap bilinear_tap(int X, int n_in, int n_out) {
    const float scale = (float)n_in / (float)n_out;
    float src = scale * ((float)X + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    Tap t;
    t.i0 = min((int)src, n_in - 1);                    // (int)src <= n_in - 1 in exact arithmetic; the min keeps every index inside
    t.i1 = t.i0 + (t.i0 < n_in - 1 ? 1 : 0);
    t.l1 = src - (float)t.i0;
    t.l0 = 1.f - t.l1;
    return t;
}

template <typename T>
__device__ __forceinline__ float ldf(const T* p) {
    if constexpr (sizeof(T) == 4) return *p;
    else return __uint_as_float((uint32_t)(*reinterpret_cast<const uint16_t*>(p)) << 16);      // bfloat16: the upper half, exact
}

template <typename T>
__device__ __forceinline__ void stf(T* p, float v) {
    if constexpr (sizeof(T) == 4) *p = v;
    else *p = (__bf16)v;                                                                       // rounded to nearest even, once
}

// the one interpolated logit of every file: plane = logit[b][c], rows r0 / r1 = i0 * w / i1 * w of the Y tap
template <typename T>
__device__ __forceinline__ float interp(const T* plane, int r0, int r1, const Tap& ty, const Tap& tx) {
    const float z00 = ldf(plane + r0 + tx.i0), z01 = ldf(plane + r0 + tx.i1);
    const float z10 = ldf(plane + r1 + tx.i0), z11 = ldf(plane + r1 + tx.i1);
    return ty.l0 * (tx.l0 * z00 + tx.l1 * z01) + ty.l1 * (tx.l0 * z10 + tx.l1 * z11);
}

// label of a pixel, or -1 when it is ignored (ignore_index, or outside [0, C))
template <typename LT>
__device__ __forceinline__ int valid_label(const LT* label, size_t p, int C, int ignore_index) {
    const long long v = (long long)label[p];
    return (v == (long long)ignore_index || v < 0 || v >= (long long)C) ? -1 : (int)v;
}

// first / last destination index in [0, n_out) whose taps touch source index y (first > last: none).  The exact range is
// ((y - 1 + 0.5) n_out / n_in - 0.5, (y + 1 + 0.5) n_out / n_in - 0.5); the scan decides membership with bilinear_tap itself, so
// rounding can neither drop nor double a pixel.
__device__ __forceinline__ void tap_range(int y, int n_in, int n_out, int& first, int& last) {
    const double r = (double)n_out / (double)n_in;
    const double lo = floor(((double)y - 0.5) * r - 0.5), hi = ceil(((double)y + 1.5) * r - 0.5);
    const double margin = 1.0 + floor(hi * 1.0e-6);        // one, plus the float32 error of the source index (< 2.4e-7 of it)
    const int c0 = (int)fmax(lo - margin, 0.0), c1 = (int)fmin(hi + margin, (double)(n_out - 1));
    first = c1 + 1;
    last = c0 - 1;
    for (int Y = c0; Y <= c1; ++Y) {
        const Tap t = bilinear_tap(Y, n_in, n_out);
        if (t.i0 == y || t.i1 == y) {
            if (first > c1) first = Y;
            last = Y;
        }
    }
}

// the weight of source index y in a destination pixel's taps; where both taps fall on y (the high border) they add
__device__ __forceinline__ float tap_weight(const Tap& t, int y) { return (t.i0 == y ? t.l0 : 0.f) + (t.i1 == y ? t.l1 : 0.f); }

// the softmax sweep of one pixel over the C channels of img = logit[b] (rows r0 / r1 of the Y tap): the maximum m, its class arg (ties
// keep the lowest), z_label zl (lab < 0: of no use) and s = sum_c exp(z_c - m), in two passes and with no per-channel registers.  The
// caller forms lse = m + logf(s) or 1 / s.  seg_eval_kernel's sweep is NOT this one: it starts from -inf so that a NaN never wins.
struct Sweep { float m, s, zl; int arg; };

template <typename T>
__device__ __forceinline__ Sweep softmax_sweep(const T* img, size_t plane, int C, int r0, int r1, const Tap& ty, const Tap& tx, int lab) {
    Sweep r;
    r.m = r.zl = interp(img, r0, r1, ty, tx);
    r.arg = 0;
    for (int c = 1; c < C; ++c) {
        const float z = interp(img + c * plane, r0, r1, ty, tx);
        if (z > r.m) { r.m = z; r.arg = c; }                   // ties keep the lowest class
        if (c == lab) r.zl = z;
    }
    r.s = 0.f;
    for (int c = 0; c < C; ++c) r.s += expf(interp(img + c * plane, r0, r1, ty, tx) - r.m);
    return r;
}

// a (float, int) pair summed over a workgroup of THREADS in a fixed tree: xor shuffles within the wave, then the waves in order through
// the caller's LDS (s_a, s_n: THREADS / 64 each).  Every work-item calls it; work-item 0 gets the sums, the others zeros.  By value and
// by return: updating the caller's accumulators through references cost resize_ce_fwd_kernel two VGPRs and a vector loop counter.
struct FloatInt { float a; int n; };

template <int THREADS>
__device__ __forceinline__ FloatInt group_sum(float a, int n, float* s_a, int* s_n) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        n += __shfl_xor(n, o, 64);
    }
    if ((tid & 63) == 0) { s_a[tid >> 6] = a; s_n[tid >> 6] = n; }
    __syncthreads();
    FloatInt r{0.f, 0};
    if (tid == 0) {
        r.a = s_a[0];
        r.n = s_n[0];
#pragma unroll
        for (int i = 1; i < THREADS / 64; ++i) { r.a += s_a[i]; r.n += s_n[i]; }
    }
    return r;
}

// the last stage of a loss, one workgroup of THREADS: each work-item brings its strided share (a in double, n in int64, summed in
// order), a fixed tree through the caller's LDS (s_a, s_n: THREADS each) adds them.  Every work-item calls it; the sums are in work-item 0.
template <int THREADS>
__device__ __forceinline__ void final_sum(double& a, long long& n, double* s_a, long long* s_n) {
    const int tid = threadIdx.x;
    s_a[tid] = a;
    s_n[tid] = n;
    __syncthreads();
    for (int o = THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) { s_a[tid] += s_a[tid + o]; s_n[tid] += s_n[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) { a = s_a[0]; n = s_n[0]; }
}

// The one-writer gather of a backward: dlogit element o = [b][c][y][x] is the sum over the full-resolution pixels whose taps touch
// (y, x).  Those are a run of consecutive Y and of consecutive X (tap_range); LANES lanes share an output, lanes across the footprint,
// each summing its terms in double (a footprint of ~1000 signed terms that cancel), and a fixed xor tree adds the lanes: no atomics,
// every result is bitwise reproducible.  A workgroup of THREADS holds THREADS / LANES outputs.  The kernel constructs it, calls sum
// with its per-pixel term, and stores where live && lane() == 0.
template <int THREADS, int LANES>
struct Gather {
    long long o;                                           // the dlogit element
    int bc, b, c, y, x;                                    // o decoded (zeros where not live)
    bool live;                                             // the lanes of an output agree; no early return before the shuffles

    // the lane within the output.  Not a member: read back from the struct, the compiler no longer sees that the footprint index
    // i = lane + k LANES is non-negative, and the i / nx of every pixel costs three more instructions
    __device__ __forceinline__ static int lane() { return threadIdx.x % LANES; }

    __device__ __forceinline__ Gather(long long n_out, int C, int h, int w)
        : o((long long)blockIdx.x * (THREADS / LANES) + threadIdx.x / LANES), bc(0), b(0), c(0), y(0), x(0), live(o < n_out) {
        if (live) {
            x = (int)(o % w);
            y = (int)((o / w) % h);
            bc = (int)(o / ((long long)w * h));
            b = bc / C;
            c = bc - b * C;
        }
    }

    // term(acc, p, Y, X) adds pixel p = (b, Y, X)'s share to acc, or returns early to skip it — before it computes the taps.  `on` false
    // (uniform over the output's lanes): the sum is 0 without a pixel read.  Every lane of the workgroup calls sum; all get the total.
    template <typename F>
    __device__ __forceinline__ double sum(bool on, int h, int w, int H, int W, F&& term) const {
        double acc = 0.0;
        if (live && on) {
            int Y0, Y1, X0, X1;
            tap_range(y, h, H, Y0, Y1);
            tap_range(x, w, W, X0, X1);
            const int ny = Y1 - Y0 + 1, nx = X1 - X0 + 1;
            if (ny > 0 && nx > 0) {
                const size_t px0 = (size_t)b * H * W;
                const int n = ny * nx;                     // < 2^31: a subset of one image's H W pixels
                for (int i = lane(); i < n; i += LANES) {
                    const int dy = i / nx, Y = Y0 + dy, X = X0 + (i - dy * nx);
                    term(acc, px0 + (size_t)Y * W + X, Y, X);
                }
            }
        }
#pragma unroll
        for (int s = LANES / 2; s > 0; s >>= 1) acc += __shfl_xor(acc, s, LANES);
        return acc;
    }
};

// host: the (logit, label) type pair of a launch from the C ABI's dtype codes (logit 0 float32 / 1 bfloat16, label 0 uint8 / 1 int64,
// checked by capi.hip): f is a generic lambda called with one value of each type, `[&](auto t, auto lt) { return typed<decltype(t),
// decltype(lt)>(...); }`
template <typename F>
int dispatch_types(int logit_dtype, int label_dtype, F&& f) {
    if (logit_dtype == 0) return label_dtype == 0 ? f(float{}, uint8_t{}) : f(float{}, int64_t{});
    return label_dtype == 0 ? f(__bf16{}, uint8_t{}) : f(__bf16{}, int64_t{});
}

// host: the LANES instance of a backward gather, 1 / 8 / 64 by resize_ce_bwd_lanes (the footprint of a dlogit element is the same for
// every loss), and its grid of `threads` / LANES outputs per workgroup: f(std::integral_constant<int, LANES>, grid) launches
template <typename F>
void dispatch_lanes(int threads, long long n_out, int h, int w, int H, int W, F&& f) {
    const int lanes = resize_ce_bwd_lanes(h, w, H, W);
    const long long outs = threads / lanes;
    const dim3 grid((unsigned)((n_out + outs - 1) / outs));
    if (lanes == 1) f(std::integral_constant<int, 1>{}, grid);
    else if (lanes == 8) f(std::integral_constant<int, 8>{}, grid);
    else f(std::integral_constant<int, 64>{}, grid);
}
}  // namespace

}  // namespace ppn
