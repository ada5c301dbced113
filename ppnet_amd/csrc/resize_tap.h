// resize_tap.h — the bilinear tap arithmetic that resize_ce.hip (the heads' training loss) and seg_eval.hip (the evaluation's area
// histograms) share: torch's float32 rule for F.interpolate(bilinear, align_corners=False) with the size given.  One definition, so
// the interpolated logit of a pixel — and with it the argmax — is the same float in every kernel of both files (the build has
// -ffp-contract=off: no kernel fuses the products differently).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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

// the one interpolated logit of both files: plane = logit[b][c], rows r0 / r1 = i0 * w / i1 * w of the Y tap
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
}  // namespace

}  // namespace ppn
