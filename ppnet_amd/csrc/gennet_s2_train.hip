// gennet_s2_train.hip — the training kernels of GenNet's 24 -> 24 stride-2 stages on gfx950: one adjoint pair and one reduction serve
// Conv2d(24, 24, 3, 2, 1) and ConvTranspose2d(24, 24, 3, 2, 1, output_padding=1) alike, with the weights as the modules store them.
//
//   s2_down_kernel          D: y[b,o,i,j]   = bias[o] + sum_{c,ky,kx} w[o][c][ky][kx] x[b,c,2i+ky-1,2j+kx-1]                  big -> small
//   s2_up_kernel            U: o[b,c,Y,X]   = bias[c] + sum_{a,ky,kx : Y = 2i-1+ky, X = 2j-1+kx} w[a][c][ky][kx] s[b,a,i,j]    small -> big
//   s2_wgrad_kernel         W: dw[a][c][ky][kx] = sum_{b,i,j} s[b,a,i,j] big[b,c,2i+ky-1,2j+kx-1], sum_b,i,j s[a], sum_b,Y,X big[c]
//   s2_wgrad_finish_kernel  the workgroups' partials in index order, float64, rounded once
//
// The big grid is H x W, the small one Hs x Ws = ceil(H / 2) x ceil(W / 2); everything outside either grid is zero (the padding).
// Conv2d: forward D(x, w), input gradient U(dy, w) at x's extent, weight gradient W(small = dy, big = x), bias gradient sum_small.
// ConvTranspose2d: forward U(x, w) at 2H x 2W, input gradient D(dy, w), weight gradient W(small = x, big = dy), bias gradient sum_big.
// No weight is flipped, transposed or repacked on the host: D reads w as [out][in][3][3], U as [in][out][3][3], W writes
// [small channel][big channel][3][3] — the stored layout of the layer it serves.
//
// Activations are contiguous NCHW, float32 or bfloat16; weights, bias, dw and the channel sums float32.  All products and sums are
// float32 FMAs on the vector unit in both data types (bfloat16 is only the widening on load and the one rounding on store); the
// finishing kernel adds in float64.
//
// Work split: small pixels are numbered n = (b Hs + i) Ws + j over the batch.  A workgroup of S2_THREADS work-items owns a tile of
// S2_TILE = 512 consecutive ones.  In D and U a work-item owns the S2_PPT = 2 pixels n0 + t and n0 + 256 + t of the tile (lanes along
// j: its loads and stores walk a row), each placed and bounds-checked on its own, so rows and images may end anywhere in a tile (a
// value outside a grid is a load of the plane's element 0 replaced by zero: no branch around a load, nothing waits for one).  The
// weights lie in LDS, reduced channel major, the 24 (U: 12) output channels of one (channel, tap) contiguous, and are read as
// broadcast 16-byte vectors: one read feeds 4 FMAs of each pixel.  D: 48 running sums per work-item.  U in gather form: the 2 x 2
// output block of small position (i, j) takes s(i..i+1, j..j+1) and each of the nine taps exactly once (even Y: ky = 1; odd Y: ky = 0
// from i + 1 and ky = 2 from i; X alike) — 4 x 12 sums per pixel, the output channels split in two halves over blockIdx.y; an even W
// stores the two columns of a block as one pair.  Every output element has one writer.
// W: a workgroup walks tiles blockIdx.x, + gridDim.x, ... (at most S2_MAX_BLOCKS workgroups) in chunks of S2_CHUNK = 32 pixels: the
// chunk's 24 small values and 216 patch values per pixel go through registers (loaded while the chunk before is summed) to LDS (zero
// outside the grids and past the last pixel), then work-item t < 216
// adds its 4 x 6 block of the 24 x 216 products over the chunk's pixels in pixel order, and work-items 216 .. 239 the channel
// sums (sum_big from taps (1,1), (1,2), (2,1), (2,2): the four big pixels 2i + {0,1}, 2j + {0,1} — every big pixel exactly once).
// Each sum has one owner, so the workgroup writes ONE partial [5184 + 48] without any exchange; the finishing kernel adds the partials
// in S2_SLICES contiguous index ranges in index order, then the range sums in order.  No atomics: two calls give the same bits.
#include <hip/hip_bf16.h>
#include "ppn_device.h"
#include "ppn_kernels.h"

namespace ppn {

constexpr int S2_C = 24;               // the one width
constexpr int S2_THREADS = 256;        // work-items per workgroup of every kernel of this file
constexpr int S2_PPT = 2;              // small pixels per work-item of D and U, S2_THREADS apart
constexpr int S2_TILE = 512;           // small pixels per workgroup tile (S2_THREADS * S2_PPT)
constexpr int S2_MAX_BLOCKS = 768;     // workgroups of W (three per CU, what its registers allow): past that many tiles one strides
constexpr int S2_CHUNK = 32;           // small pixels per LDS chunk of W
constexpr int S2_ROW = 36;             // floats per LDS row of W (S2_CHUNK + 4: rows 6 apart start in different banks)
constexpr int S2_KT = 216;             // taps x channels: 9 * S2_C
constexpr int S2_DW = 5184;            // S2_C * S2_KT
constexpr int S2_PART = 5232;          // floats per partial of W: dw, sum_small [24], sum_big [24]
constexpr int S2_SLICES = 16;          // index ranges of the partials summed side by side in the finishing kernel
constexpr int S2_UCH = 12;             // output channels per work-item of U

int gennet_s2_tile() { return S2_TILE; }
int gennet_s2_max_blocks() { return S2_MAX_BLOCKS; }

namespace {

struct S2Grid { uint32_t H, W, Hs, Ws, HW, HWs, NS; };                       // NS = B Hs Ws; B 24 H W < 2^31

unsigned s2_tiles(long long ns) { return (unsigned)((ns + S2_TILE - 1) / S2_TILE); }

// raw_t: an element as loaded, kept in a register until it is needed (W loads a chunk ahead: widening at once would wait for the load)
template <typename T> struct S2IO;
template <> struct S2IO<float> {
    typedef float raw_t;
    static __device__ __forceinline__ raw_t load_raw(const float* p) { return *p; }
    static __device__ __forceinline__ float widen(raw_t r) { return r; }
    static __device__ __forceinline__ float load(const float* p) { return *p; }
    static __device__ __forceinline__ void store(float* p, float v) { *p = v; }
    static __device__ __forceinline__ void store2(float* p, float a, float b) { *reinterpret_cast<float2*>(p) = make_float2(a, b); }
};
template <> struct S2IO<__hip_bfloat16> {
    typedef uint16_t raw_t;
    static __device__ __forceinline__ raw_t load_raw(const __hip_bfloat16* p) { return *reinterpret_cast<const uint16_t*>(p); }
    static __device__ __forceinline__ float widen(raw_t r) { return __uint_as_float((uint32_t)r << 16); }
    static __device__ __forceinline__ float load(const __hip_bfloat16* p) { return widen(load_raw(p)); }
    static __device__ __forceinline__ void store(__hip_bfloat16* p, float v) {     // round to nearest even, as pack_bf16x2 does
        *reinterpret_cast<uint16_t*>(p) = __builtin_bit_cast(uint16_t, (__bf16)v);
    }
    static __device__ __forceinline__ void store2(__hip_bfloat16* p, float a, float b) { *reinterpret_cast<uint32_t*>(p) = pack_bf16x2(a, b); }
};

// small pixel n -> image b, row i, column j (n < NS)
__device__ __forceinline__ void s2_place(const S2Grid& g, uint32_t n, uint32_t& b, uint32_t& i, uint32_t& j) {
    b = n / g.HWs;
    const uint32_t q = n - b * g.HWs;
    i = q / g.Ws;
    j = q - i * g.Ws;
}

// offsets inside a big plane of the 3 x 3 patch of small pixel (i, j): off[3 ky + kx] = (2i + ky - 1) W + 2j + kx - 1, -1 outside
__device__ __forceinline__ void s2_patch_offsets(const S2Grid& g, bool live, uint32_t i, uint32_t j, int (&off)[9]) {
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int Y = 2 * (int)i + ky - 1, X = 2 * (int)j + kx - 1;
            off[3 * ky + kx] = (live && Y >= 0 && Y < (int)g.H && X >= 0 && X < (int)g.W) ? Y * (int)g.W + X : -1;
        }
}

}  // namespace

template <typename T>
__global__ __launch_bounds__(S2_THREADS) void s2_down_kernel(const T* __restrict__ big, const float* __restrict__ w, const float* __restrict__ bias,
                                                             T* __restrict__ small, S2Grid g) {
    __shared__ __align__(16) float wl[S2_DW];                                // [c][tap][o]: wl[(9 c + t) 24 + o] = w[o][c][t]
    for (int s = (int)threadIdx.x; s < S2_DW; s += S2_THREADS) {
        const int o = s / S2_KT, rem = s - o * S2_KT;
        wl[rem * S2_C + o] = w[s];
    }
    __syncthreads();
    uint32_t b[S2_PPT], q[S2_PPT];
    bool live[S2_PPT];
    int off[S2_PPT][9];
    float acc[S2_PPT][S2_C];
#pragma unroll
    for (int k = 0; k < S2_PPT; ++k) {
        const uint32_t n = blockIdx.x * (uint32_t)S2_TILE + (uint32_t)k * S2_THREADS + threadIdx.x;
        live[k] = n < g.NS;
        uint32_t i = 0, j = 0;
        b[k] = 0;
        if (live[k]) s2_place(g, n, b[k], i, j);
        q[k] = i * g.Ws + j;
        s2_patch_offsets(g, live[k], i, j, off[k]);
#pragma unroll
        for (int o = 0; o < S2_C; ++o) acc[k][o] = bias ? bias[o] : 0.0f;
    }
    const float4* wl4 = reinterpret_cast<const float4*>(wl);
#pragma unroll 1
    for (int c = 0; c < S2_C; ++c) {
        float p[S2_PPT][9];
#pragma unroll
        for (int k = 0; k < S2_PPT; ++k) {
            const T* plane = big + ((size_t)b[k] * S2_C + c) * g.HW;
#pragma unroll
            for (int t = 0; t < 9; ++t) {                                    // always a load (element 0 stands in outside): no branch, no wait
                const float v = S2IO<T>::load(plane + max(off[k][t], 0));
                p[k][t] = off[k][t] >= 0 ? v : 0.0f;
            }
        }
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int o4 = 0; o4 < S2_C / 4; ++o4) {
                const float4 wv = wl4[(c * 9 + t) * (S2_C / 4) + o4];
#pragma unroll
                for (int k = 0; k < S2_PPT; ++k) {
                    acc[k][4 * o4 + 0] = fmaf(wv.x, p[k][t], acc[k][4 * o4 + 0]);
                    acc[k][4 * o4 + 1] = fmaf(wv.y, p[k][t], acc[k][4 * o4 + 1]);
                    acc[k][4 * o4 + 2] = fmaf(wv.z, p[k][t], acc[k][4 * o4 + 2]);
                    acc[k][4 * o4 + 3] = fmaf(wv.w, p[k][t], acc[k][4 * o4 + 3]);
                }
            }
    }
#pragma unroll
    for (int k = 0; k < S2_PPT; ++k) {
        if (!live[k]) continue;
        T* dst = small + (size_t)b[k] * S2_C * g.HWs + q[k];
#pragma unroll
        for (int o = 0; o < S2_C; ++o) S2IO<T>::store(dst + (size_t)o * g.HWs, acc[k][o]);
    }
}

template <typename T>
__global__ __launch_bounds__(S2_THREADS) void s2_up_kernel(const T* __restrict__ small, const float* __restrict__ w, const float* __restrict__ bias,
                                                           T* __restrict__ big, S2Grid g) {
    __shared__ __align__(16) float wl[S2_KT * S2_UCH];                       // [a][tap][c - c0]: wl[(9 a + t) 12 + c - c0] = w[a][c][t]
    const int c0 = (int)blockIdx.y * S2_UCH;
    for (int s = (int)threadIdx.x; s < S2_DW; s += S2_THREADS) {
        const int a = s / S2_KT, rem = s - a * S2_KT, c = rem / 9, t = rem - c * 9;
        if (c >= c0 && c < c0 + S2_UCH) wl[(a * 9 + t) * S2_UCH + c - c0] = w[s];
    }
    __syncthreads();
    uint32_t b[S2_PPT], ii[S2_PPT], jj[S2_PPT];
    bool live[S2_PPT];
    int so[S2_PPT][4];                                                       // offsets inside a small plane of s(i + di, j + dj), -1 outside
    float acc[S2_PPT][4][S2_UCH];                                            // [pixel][2 (Y - 2i) + X - 2j][channel]
#pragma unroll
    for (int k = 0; k < S2_PPT; ++k) {
        const uint32_t n = blockIdx.x * (uint32_t)S2_TILE + (uint32_t)k * S2_THREADS + threadIdx.x;
        live[k] = n < g.NS;
        b[k] = ii[k] = jj[k] = 0;
        if (live[k]) s2_place(g, n, b[k], ii[k], jj[k]);
#pragma unroll
        for (int di = 0; di < 2; ++di)
#pragma unroll
            for (int dj = 0; dj < 2; ++dj)
                so[k][2 * di + dj] = (live[k] && ii[k] + di < g.Hs && jj[k] + dj < g.Ws) ? (int)((ii[k] + di) * g.Ws + jj[k] + dj) : -1;
#pragma unroll
        for (int qd = 0; qd < 4; ++qd)
#pragma unroll
            for (int c = 0; c < S2_UCH; ++c) acc[k][qd][c] = bias ? bias[c0 + c] : 0.0f;
    }
    const float4* wl4 = reinterpret_cast<const float4*>(wl);
#pragma unroll 1
    for (int a = 0; a < S2_C; ++a) {
        float sv[S2_PPT][4];
#pragma unroll
        for (int k = 0; k < S2_PPT; ++k) {
            const T* plane = small + ((size_t)b[k] * S2_C + a) * g.HWs;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const float v = S2IO<T>::load(plane + max(so[k][d], 0));
                sv[k][d] = so[k][d] >= 0 ? v : 0.0f;
            }
        }
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                // Y = 2 i' - 1 + ky: ky = 1 -> Y = 2i from i; ky = 2 -> Y = 2i + 1 from i; ky = 0 -> Y = 2i + 1 from i + 1 (X alike)
                const int qa = ky == 1 ? 0 : 1, di = ky == 0 ? 1 : 0, qb = kx == 1 ? 0 : 1, dj = kx == 0 ? 1 : 0;
#pragma unroll
                for (int c4 = 0; c4 < S2_UCH / 4; ++c4) {
                    const float4 wv = wl4[(a * 9 + 3 * ky + kx) * (S2_UCH / 4) + c4];
#pragma unroll
                    for (int k = 0; k < S2_PPT; ++k) {
                        const float s = sv[k][2 * di + dj];
                        float (&o)[S2_UCH] = acc[k][2 * qa + qb];
                        o[4 * c4 + 0] = fmaf(wv.x, s, o[4 * c4 + 0]);
                        o[4 * c4 + 1] = fmaf(wv.y, s, o[4 * c4 + 1]);
                        o[4 * c4 + 2] = fmaf(wv.z, s, o[4 * c4 + 2]);
                        o[4 * c4 + 3] = fmaf(wv.w, s, o[4 * c4 + 3]);
                    }
                }
            }
    }
    const bool pair = (g.W & 1u) == 0;                                       // uniform; then 2j + 1 < W and every pair is aligned
#pragma unroll
    for (int k = 0; k < S2_PPT; ++k) {
        if (!live[k]) continue;
#pragma unroll
        for (int qa = 0; qa < 2; ++qa) {
            const uint32_t Y = 2 * ii[k] + qa, X = 2 * jj[k];
            if (Y >= g.H) continue;
            T* dst = big + ((size_t)b[k] * S2_C + c0) * g.HW + (size_t)Y * g.W + X;
#pragma unroll
            for (int c = 0; c < S2_UCH; ++c) {
                if (pair) {
                    S2IO<T>::store2(dst + (size_t)c * g.HW, acc[k][2 * qa][c], acc[k][2 * qa + 1][c]);
                } else {
                    S2IO<T>::store(dst + (size_t)c * g.HW, acc[k][2 * qa][c]);
                    if (X + 1 < g.W) S2IO<T>::store(dst + (size_t)c * g.HW + 1, acc[k][2 * qa + 1][c]);
                }
            }
        }
    }
}

// partial [gridDim.x][S2_PART] float32: the sums of the tiles this workgroup walked
template <typename T>
__global__ __launch_bounds__(S2_THREADS) void s2_wgrad_kernel(const T* __restrict__ small, const T* __restrict__ big, float* __restrict__ partial,
                                                              S2Grid g, uint32_t ntiles) {
    __shared__ __align__(16) float sS[S2_C * S2_ROW];                        // [a][pixel]
    __shared__ __align__(16) float sB[S2_KT * S2_ROW];                       // [9 c + t][pixel]
    const int tid = (int)threadIdx.x;
    const int p = tid & (S2_CHUNK - 1), grp = tid / S2_CHUNK;                // loading: pixel of the chunk, channels grp, grp + 8, grp + 16
    const bool mac = tid < S2_KT, sums = tid >= S2_KT && tid < S2_KT + S2_C;
    const int ag = tid / 36, ctg = tid - ag * 36;                            // summing: rows 4 ag .. + 3 of s, 6 ctg .. + 5 of the patches
    const int ch = tid - S2_KT;                                              // the channel of a work-item that keeps the channel sums
    float acc[4][6], cs = 0.0f, cb = 0.0f;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 6; ++v) acc[u][v] = 0.0f;
    constexpr int LCH = S2_C / (S2_THREADS / S2_CHUNK), CHUNKS = S2_TILE / S2_CHUNK;
    typename S2IO<T>::raw_t rb[LCH][9], rs[LCH];                             // the next chunk's values of this work-item, on their way to LDS
    // chunk q of this workgroup: tile blockIdx.x + (q / CHUNKS) gridDim.x, pixels base .. base + 31; bases grow with q
    auto chunk_base = [&](uint32_t q) -> uint64_t {
        const uint64_t tile = (uint64_t)blockIdx.x + (uint64_t)(q / CHUNKS) * gridDim.x;
        return tile < ntiles ? tile * S2_TILE + (uint64_t)(q % CHUNKS) * S2_CHUNK : (uint64_t)g.NS;
    };
    auto fetch = [&](uint64_t base) {
        const uint32_t n = (uint32_t)base + (uint32_t)p;
        const bool live = n < g.NS;
        uint32_t b = 0, i = 0, j = 0;
        if (live) s2_place(g, n, b, i, j);
        int off[9];
        s2_patch_offsets(g, live, i, j, off);
#pragma unroll
        for (int cc = 0; cc < LCH; ++cc) {
            const int c = grp + cc * (S2_THREADS / S2_CHUNK);
            const T* plane = big + ((size_t)b * S2_C + c) * g.HW;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const typename S2IO<T>::raw_t v = S2IO<T>::load_raw(plane + max(off[t], 0));
                rb[cc][t] = off[t] >= 0 ? v : (typename S2IO<T>::raw_t)0;
            }
            const typename S2IO<T>::raw_t sv = S2IO<T>::load_raw(small + ((size_t)b * S2_C + c) * g.HWs + (size_t)i * g.Ws + j);   // not live: pixel 0
            rs[cc] = live ? sv : (typename S2IO<T>::raw_t)0;
        }
    };
    uint64_t base = chunk_base(0);
    if (base < g.NS) fetch(base);
    for (uint32_t q = 0; base < g.NS; ++q) {                                 // uniform
#pragma unroll
        for (int cc = 0; cc < LCH; ++cc) {
            const int c = grp + cc * (S2_THREADS / S2_CHUNK);
#pragma unroll
            for (int t = 0; t < 9; ++t) sB[(c * 9 + t) * S2_ROW + p] = S2IO<T>::widen(rb[cc][t]);
            sS[c * S2_ROW + p] = S2IO<T>::widen(rs[cc]);
        }
        __syncthreads();
        base = chunk_base(q + 1);
        if (base < g.NS) fetch(base);                                        // in flight while this chunk is summed
        if (mac) {
#pragma unroll 2
            for (int p4 = 0; p4 < S2_CHUNK; p4 += 4) {
                float4 sa[4], bb[6];
#pragma unroll
                for (int u = 0; u < 4; ++u) sa[u] = *reinterpret_cast<const float4*>(&sS[(4 * ag + u) * S2_ROW + p4]);
#pragma unroll
                for (int v = 0; v < 6; ++v) bb[v] = *reinterpret_cast<const float4*>(&sB[(6 * ctg + v) * S2_ROW + p4]);
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int v = 0; v < 6; ++v) {
                        acc[u][v] = fmaf(sa[u].x, bb[v].x, acc[u][v]);
                        acc[u][v] = fmaf(sa[u].y, bb[v].y, acc[u][v]);
                        acc[u][v] = fmaf(sa[u].z, bb[v].z, acc[u][v]);
                        acc[u][v] = fmaf(sa[u].w, bb[v].w, acc[u][v]);
                    }
            }
        } else if (sums) {
            for (int p4 = 0; p4 < S2_CHUNK; p4 += 4) {
                const float4 s = *reinterpret_cast<const float4*>(&sS[ch * S2_ROW + p4]);
                cs += s.x; cs += s.y; cs += s.z; cs += s.w;
#pragma unroll
                for (int t = 4; t < 9; ++t) {
                    if (t == 6) continue;                                    // taps (1,1), (1,2), (2,1), (2,2)
                    const float4 v = *reinterpret_cast<const float4*>(&sB[(ch * 9 + t) * S2_ROW + p4]);
                    cb += v.x; cb += v.y; cb += v.z; cb += v.w;
                }
            }
        }
        __syncthreads();
    }
    float* out = partial + (size_t)blockIdx.x * S2_PART;
    if (mac) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 6; ++v) out[(4 * ag + u) * S2_KT + 6 * ctg + v] = acc[u][v];
    } else if (sums) {
        out[S2_DW + ch] = cs;
        out[S2_DW + S2_C + ch] = cb;
    }
}

// Sum idx = 16 blockIdx.x + col of the S2_PART: the partials in S2_SLICES contiguous index ranges in index order, then the range sums in
// order, float64, rounded once into dw, sum_small or sum_big (the last two where wanted).
__global__ __launch_bounds__(S2_THREADS) void s2_wgrad_finish_kernel(const float* __restrict__ partial, int nparts, float* __restrict__ dw,
                                                                     float* __restrict__ sum_small, float* __restrict__ sum_big) {
    __shared__ double red[S2_SLICES][16];
    const int col = (int)threadIdx.x & 15, slice = (int)threadIdx.x >> 4;
    const int idx = (int)blockIdx.x * 16 + col;                              // S2_PART is a multiple of 16
    const int per = (nparts + S2_SLICES - 1) / S2_SLICES;
    const int g0 = slice * per, g1 = min(g0 + per, nparts);
    double s = 0.0;
#pragma unroll 8
    for (int gi = g0; gi < g1; ++gi) s += (double)partial[(size_t)gi * S2_PART + idx];
    red[slice][col] = s;
    __syncthreads();
    if (threadIdx.x >= 16) return;
    double tot = red[0][col];
#pragma unroll
    for (int i = 1; i < S2_SLICES; ++i) tot += red[i][col];
    if (idx < S2_DW) dw[idx] = (float)tot;
    else if (idx < S2_DW + S2_C) { if (sum_small) sum_small[idx - S2_DW] = (float)tot; }
    else if (sum_big) sum_big[idx - S2_DW - S2_C] = (float)tot;
}

namespace {

S2Grid s2_grid(int B, int H, int W) {
    const uint32_t Hs = (uint32_t)((H + 1) / 2), Ws = (uint32_t)((W + 1) / 2);
    return S2Grid{(uint32_t)H, (uint32_t)W, Hs, Ws, (uint32_t)H * (uint32_t)W, Hs * Ws, (uint32_t)B * Hs * Ws};
}

unsigned s2_wgrad_blocks(long long ns) { const unsigned t = s2_tiles(ns); return t < (unsigned)S2_MAX_BLOCKS ? t : (unsigned)S2_MAX_BLOCKS; }

}  // namespace

long long gennet_s2_wgrad_workspace_bytes(long long ns) {
    if (ns < 1 || ns > 0x7fffffffLL) return -1;
    return (long long)S2_PART * (long long)sizeof(float) * (long long)s2_wgrad_blocks(ns);
}

int gennet_s2_down_launch(const void* big, const float* w, const float* bias, void* small, int B, int H, int W, int C, int dtype, hipStream_t stream) {
    if (C != S2_C) return -1;
    const S2Grid g = s2_grid(B, H, W);
    const dim3 grid(s2_tiles(g.NS));
    if (dtype == 0)
        hipLaunchKernelGGL((s2_down_kernel<float>), grid, dim3(S2_THREADS), 0, stream, (const float*)big, w, bias, (float*)small, g);
    else
        hipLaunchKernelGGL((s2_down_kernel<__hip_bfloat16>), grid, dim3(S2_THREADS), 0, stream, (const __hip_bfloat16*)big, w, bias,
                           (__hip_bfloat16*)small, g);
    return (int)hipGetLastError();
}

int gennet_s2_up_launch(const void* small, const float* w, const float* bias, void* big, int B, int H, int W, int C, int dtype, hipStream_t stream) {
    if (C != S2_C) return -1;
    const S2Grid g = s2_grid(B, H, W);
    const dim3 grid(s2_tiles(g.NS), (unsigned)(S2_C / S2_UCH));
    if (dtype == 0)
        hipLaunchKernelGGL((s2_up_kernel<float>), grid, dim3(S2_THREADS), 0, stream, (const float*)small, w, bias, (float*)big, g);
    else
        hipLaunchKernelGGL((s2_up_kernel<__hip_bfloat16>), grid, dim3(S2_THREADS), 0, stream, (const __hip_bfloat16*)small, w, bias,
                           (__hip_bfloat16*)big, g);
    return (int)hipGetLastError();
}

int gennet_s2_wgrad_launch(const void* small, const void* big, void* workspace, float* dw, float* sum_small, float* sum_big, int B, int H, int W,
                           int C, int dtype, hipStream_t stream) {
    if (C != S2_C) return -1;
    const S2Grid g = s2_grid(B, H, W);
    const unsigned blocks = s2_wgrad_blocks(g.NS), tiles = s2_tiles(g.NS);
    if (dtype == 0)
        hipLaunchKernelGGL((s2_wgrad_kernel<float>), dim3(blocks), dim3(S2_THREADS), 0, stream, (const float*)small, (const float*)big,
                           (float*)workspace, g, tiles);
    else
        hipLaunchKernelGGL((s2_wgrad_kernel<__hip_bfloat16>), dim3(blocks), dim3(S2_THREADS), 0, stream, (const __hip_bfloat16*)small,
                           (const __hip_bfloat16*)big, (float*)workspace, g, tiles);
    const int e = (int)hipGetLastError();
    if (e != 0) return e;
    hipLaunchKernelGGL(s2_wgrad_finish_kernel, dim3(S2_PART / 16), dim3(S2_THREADS), 0, stream, (const float*)workspace, (int)blocks, dw, sum_small,
                       sum_big);
    return (int)hipGetLastError();
}

}  // namespace ppn
