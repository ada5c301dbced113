// capi.hip — the extern "C" boundary of libppnet_hip.so (declared in include/ppnet_hip.h).
// Argument validation, constant tables, kernel launches.  No torch types, no exceptions.
#include <hip/hip_runtime.h>
#include <math.h>
#include <mutex>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include <cstdlib>
#include "ppn_kernels.h"

namespace {

thread_local int g_last_hip = 0;

inline int hip_fail(hipError_t e) {
    g_last_hip = (int)e;
    return PPN_E_HIP;
}
#define PPN_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return hip_fail(e_); } while (0)

inline bool bad_R(int R) { return R < 32 || R > 512 || (R % 32) != 0; }

// Least-squares operator for np.polyfit(arange(1000)/100, y, 4): W = pinv(V)[0:4], V[i][k] = x_i^(4-k).
// Built once in extended precision (modified Gram-Schmidt with re-orthogonalisation), so the
// device fit is a constant 4 x 1000 matrix-vector product instead of a per-call LAPACK solve.
void build_polyfit_table(double* out) {
    const int N = PPN_PATH_POINTS, M = 5;
    std::vector<long double> q((size_t)M * N);
    long double Rm[5][5] = {};
    for (int i = 0; i < N; ++i) {
        const long double x = (long double)i / 100.0L;
        long double pw = 1.0L;
        for (int k = M - 1; k >= 0; --k) { q[(size_t)k * N + i] = pw; pw *= x; }
    }
    for (int k = 0; k < M; ++k) {
        long double* qk = &q[(size_t)k * N];
        for (int pass = 0; pass < 2; ++pass)
            for (int j = 0; j < k; ++j) {
                const long double* qj = &q[(size_t)j * N];
                long double r = 0.0L;
                for (int i = 0; i < N; ++i) r += qj[i] * qk[i];
                for (int i = 0; i < N; ++i) qk[i] -= r * qj[i];
                Rm[j][k] += r;
            }
        long double nn = 0.0L;
        for (int i = 0; i < N; ++i) nn += qk[i] * qk[i];
        nn = sqrtl(nn);
        Rm[k][k] = nn;
        for (int i = 0; i < N; ++i) qk[i] /= nn;
    }
    for (int i = 0; i < N; ++i) {                 // W[:, i] = R^-1 (Q^T e_i)
        long double w[5];
        for (int k = M - 1; k >= 0; --k) {
            long double v = q[(size_t)k * N + i];
            for (int j = k + 1; j < M; ++j) v -= Rm[k][j] * w[j];
            w[k] = v / Rm[k][k];
        }
        for (int k = 0; k < 4; ++k) out[(size_t)k * N + i] = (double)w[k];
    }
}

std::mutex g_tab_mu;
double* g_tab_dev[64] = {};

int polyfit_table_device(const double** out) {
    int dev = 0;
    PPN_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return PPN_E_INVALID;
    std::lock_guard<std::mutex> lk(g_tab_mu);
    if (!g_tab_dev[dev]) {
        std::vector<double> host(4 * PPN_PATH_POINTS);
        build_polyfit_table(host.data());
        double* d = nullptr;
        PPN_HIP(hipMalloc((void**)&d, host.size() * sizeof(double)));
        hipError_t e = hipMemcpy(d, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(d); return hip_fail(e); }
        g_tab_dev[dev] = d;
    }
    *out = g_tab_dev[dev];
    return PPN_OK;
}

}  // namespace

extern "C" {

int ppn_version(void) { return PPN_ABI_VERSION; }

const char* ppn_error_string(int code) {
    switch (code) {
        case PPN_OK: return "ok";
        case PPN_E_INVALID: return "invalid argument";
        case PPN_E_HIP: return "HIP runtime error";
        case PPN_E_UNSUPPORTED: return "unsupported";
        default: return "unknown error";
    }
}

int ppn_last_hip_error(void) { return g_last_hip; }

int ppn_polyfit_table(double* out) {
    if (!out) return PPN_E_INVALID;
    build_polyfit_table(out);
    return PPN_OK;
}

int ppn_edage_paths(int32_t n_paths, uint64_t first_path_id, int32_t R, double map_size, double clearance,
                    uint64_t seed, const double* draws, const float* pocket_draws, int32_t pocket_stride,
                    const ppn_paths_t* out, void* stream) {
    return ppn_edage_paths_ex(n_paths, first_path_id, R, map_size, clearance, seed, draws, pocket_draws, pocket_stride,
                              nullptr, out, stream);
}

int ppn_edage_paths_ex(int32_t n_paths, uint64_t first_path_id, int32_t R, double map_size, double clearance,
                       uint64_t seed, const double* draws, const float* pocket_draws, int32_t pocket_stride,
                       const int8_t* force_straight, const ppn_paths_t* out, void* stream) {
    return ppn_edage_paths_ex2(n_paths, first_path_id, R, map_size, clearance, seed, draws, pocket_draws, pocket_stride,
                               force_straight, nullptr, out, stream);
}

int ppn_edage_paths_ex2(int32_t n_paths, uint64_t first_path_id, int32_t R, double map_size, double clearance,
                        uint64_t seed, const double* draws, const float* pocket_draws, int32_t pocket_stride,
                        const int8_t* force_straight, const int32_t* hull_start, const ppn_paths_t* out, void* stream) {
    if (n_paths < 0 || bad_R(R) || !out || !(map_size > 0.0) || !(clearance > 0.0)) return PPN_E_INVALID;
    if (pocket_draws && pocket_stride <= 0) return PPN_E_INVALID;
    if (n_paths == 0) return PPN_OK;                           // an empty batch has no buffers to validate
    const ppn_paths_t& o = *out;
    if (!o.seg_poly || !o.seg_endpoint || !o.seg_rotation || !o.seg_translation || !o.seg_straight ||
        !o.segpoint_world || !o.pathpoint_world || !o.hull || !o.hull_n || !o.rotation || !o.trans_rc ||
        !o.segpoint_image || !o.pathpoint_image || !o.space_bits || !o.isles || !o.n_isles || !o.obstacles ||
        !o.n_obstacles || !o.length || !o.straight || !o.flags || !o.max_step_px)
        return PPN_E_INVALID;
    if (n_paths == 0) return PPN_OK;
    ppn::PathsParams prm;
    prm.out = o;
    prm.n_paths = n_paths;
    prm.first_id = first_path_id;
    prm.R = R;
    prm.map_size = map_size;
    prm.clearance = clearance;
    prm.seed = seed;
    prm.draws = draws;
    prm.pocket = pocket_draws;
    prm.pocket_stride = pocket_stride;
    prm.force_straight = force_straight;
    prm.hull_start = hull_start;
    int rc = polyfit_table_device(&prm.W);
    if (rc != PPN_OK) return rc;
    const size_t lds = (size_t)PPN_PATH_POINTS * 24 + (size_t)(2 * R) * (2 * R) / 8;      // path points + lattice + canvas bits
    PPN_HIP(hipFuncSetAttribute((const void*)ppn::edage_paths_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(ppn::edage_paths_kernel, dim3(n_paths), dim3(PPN_PATHS_THREADS), lds, (hipStream_t)stream, prm);
    PPN_HIP(hipGetLastError());
    return PPN_OK;
}

// phase: 1 = placement half, 2 = raster half, 3 = both in one kernel
static int maps_launch(int phase, const ppn_paths_t* paths, int32_t n_paths, int32_t placements, uint64_t first_map_id,
                       int32_t R, double map_size, double obstacles_size, int32_t K, double clearance, uint64_t seed,
                       const double* place_draws, const double* obst_draws, const ppn_maps_t* out, void* stream) {
    if (!paths || !out || n_paths < 0 || placements < 0 || bad_R(R) || K < 0 || K > 256) return PPN_E_INVALID;
    if ((phase & 1) && !(map_size > 0.0)) return PPN_E_INVALID;
    if ((long long)n_paths * placements == 0) return PPN_OK;   // an empty batch has no buffers to validate
    const ppn_paths_t& p = *paths;
    const ppn_maps_t& o = *out;
    if ((phase & 1) && (!p.hull || !p.hull_n || !p.segpoint_image || !p.pathpoint_image || !p.obstacles ||
                        !p.n_obstacles || !p.flags || !p.max_step_px))
        return PPN_E_INVALID;
    if (!p.space_bits) return PPN_E_INVALID;
    if (!o.grid || !o.angle || !o.translation || !o.attempts || !o.segpoint || !o.obstacles || !o.n_obstacles || !o.flags)
        return PPN_E_INVALID;
    const long long n_maps = (long long)n_paths * placements;
    if (n_maps > 0x7fffffffLL) return PPN_E_INVALID;
    ppn::MapsParams prm;
    prm.paths = p;
    prm.out = o;
    prm.n_paths = n_paths;
    prm.placements = placements;
    prm.n_maps = (int)n_maps;
    prm.first_map_id = first_map_id;
    prm.R = R;
    prm.map_size = map_size;
    prm.obstacles_size = obstacles_size;
    prm.clearance = clearance;
    prm.K = K;
    prm.seed = seed;
    prm.place_draws = place_draws;
    prm.obst_draws = obst_draws;
    {   // validation knob: always run the corridor compose pass (tests compare it with the proven skip)
        const char* f = getenv("PPN_FORCE_COMPOSE");
        prm.force_compose = (f && f[0] == '1') ? 1 : 0;
    }
    {
        const int rc = ppn::edage_maps_launch(phase, prm, (hipStream_t)stream);
        if (rc == PPN_E_HIP) g_last_hip = (int)hipGetLastError();
        if (rc != PPN_OK) return rc;
    }
    return PPN_OK;
}

int ppn_edage_maps(const ppn_paths_t* paths, int32_t n_paths, int32_t placements, uint64_t first_map_id, int32_t R,
                   double map_size, double obstacles_size, int32_t K, double clearance, uint64_t seed,
                   const double* place_draws, const double* obst_draws, const ppn_maps_t* out, void* stream) {
    return maps_launch(3, paths, n_paths, placements, first_map_id, R, map_size, obstacles_size, K, clearance, seed,
                       place_draws, obst_draws, out, stream);
}

int ppn_edage_maps_place(const ppn_paths_t* paths, int32_t n_paths, int32_t placements, uint64_t first_map_id, int32_t R,
                         double map_size, double obstacles_size, int32_t K, double clearance, uint64_t seed,
                         const double* place_draws, const double* obst_draws, const ppn_maps_t* out, void* stream) {
    return maps_launch(1, paths, n_paths, placements, first_map_id, R, map_size, obstacles_size, K, clearance, seed,
                       place_draws, obst_draws, out, stream);
}

int ppn_edage_maps_raster(const ppn_paths_t* paths, int32_t n_paths, int32_t placements, int32_t R, int32_t K,
                          const ppn_maps_t* out, void* stream) {
    return maps_launch(2, paths, n_paths, placements, 0, R, 0.0, 0.0, K, 0.0, 0, nullptr, nullptr, out, stream);
}

int ppn_label_masks(const ppn_paths_t* paths, const ppn_maps_t* maps, int32_t n_paths, int32_t placements, int32_t R,
                    int32_t bound, uint8_t* mask_path, uint8_t* mask_space, void* stream) {
    if (!paths || !maps || n_paths < 0 || placements < 0 || bad_R(R) || bound <= 0) return PPN_E_INVALID;
    if (mask_space && (!paths->space_bits || !maps->angle || !maps->translation)) return PPN_E_INVALID;
    if (mask_path && !maps->pathpoint) return PPN_E_INVALID;
    const long long n = (long long)n_paths * placements;
    if (n == 0 || (!mask_path && !mask_space)) return PPN_OK;
    if (n > 0x7fffffffLL) return PPN_E_INVALID;
    hipLaunchKernelGGL(ppn::label_masks_kernel, dim3((unsigned)n), dim3(256), (size_t)R * R / 8, (hipStream_t)stream, *paths, *maps,
                       placements, R, bound, mask_path, mask_space);
    PPN_HIP(hipGetLastError());
    return PPN_OK;
}

int ppn_boundary_check(const double* hull, int32_t hull_n, const double* angle_deg, const double* translation_rc,
                       int32_t n, int32_t R, uint8_t* ok, void* stream) {
    return ppn_boundary_check_ex(hull, hull_n, angle_deg, translation_rc, n, R, ok, nullptr, stream);
}

int ppn_boundary_check_ex(const double* hull, int32_t hull_n, const double* angle_deg, const double* translation_rc,
                          int32_t n, int32_t R, uint8_t* ok, double* hull_out, void* stream) {
    if (!hull || hull_n <= 0 || !angle_deg || !translation_rc || n < 0 || R <= 0 || !ok) return PPN_E_INVALID;
    if (n == 0) return PPN_OK;
    hipLaunchKernelGGL(ppn::boundary_check_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, hull, hull_n,
                       angle_deg, translation_rc, n, R, ok, hull_out);
    PPN_HIP(hipGetLastError());
    return PPN_OK;
}

int ppn_obstacle_filter(const double* pathpoint, const double* draws, int32_t n, int32_t K, int32_t R, double map_size,
                        double obstacles_size, double clearance, uint8_t* accept, double* obstacles, int32_t* counts,
                        void* stream) {
    if (!pathpoint || !draws || n < 0 || K <= 0 || K > 256 || R <= 0 || !(map_size > 0.0) || !obstacles || !counts)
        return PPN_E_INVALID;
    if (n == 0) return PPN_OK;
    hipLaunchKernelGGL(ppn::obstacle_filter_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, pathpoint, draws, n, K, R,
                       map_size, obstacles_size, clearance, accept, obstacles, counts);
    PPN_HIP(hipGetLastError());
    return PPN_OK;
}

int ppn_paint_markers(uint8_t* grid, int32_t n, int32_t R, const double* init, const double* end, void* stream) {
    if (!grid || n < 0 || R <= 0 || !init || !end) return PPN_E_INVALID;
    if (n == 0) return PPN_OK;
    hipLaunchKernelGGL(ppn::paint_markers_kernel, dim3(n), dim3(128), 0, (hipStream_t)stream, grid, n, R, init, end);
    PPN_HIP(hipGetLastError());
    return PPN_OK;
}

int ppn_disc_raster(const double* obstacles, const int32_t* counts, int32_t stride, int32_t n_maps, int32_t R,
                    uint8_t* grid, void* stream) {
    if (!obstacles || !counts || stride <= 0 || n_maps < 0 || R <= 0 || (R % 16) != 0 || !grid) return PPN_E_INVALID;
    if (n_maps == 0) return PPN_OK;
    hipLaunchKernelGGL(ppn::disc_raster_kernel, dim3(n_maps), dim3(256), 0, (hipStream_t)stream, obstacles, counts,
                       stride, n_maps, R, grid);
    PPN_HIP(hipGetLastError());
    return PPN_OK;
}

int ppn_collision_segments_bound(const float* s, const float* e, const int32_t* prob, int32_t n_seg, const float* obs,
                                 const int32_t* obs_off, float clearance, float bound, uint8_t* hit, void* stream) {
    if (!s || !e || !prob || n_seg < 0 || !obs || !obs_off || !hit || !(bound > 0.0f)) return PPN_E_INVALID;
    if (n_seg == 0) return PPN_OK;
    hipLaunchKernelGGL(ppn::collision_segments_kernel, dim3((n_seg + 255) / 256), dim3(256), 0, (hipStream_t)stream, s,
                       e, prob, n_seg, obs, obs_off, clearance, bound, hit);
    PPN_HIP(hipGetLastError());
    return PPN_OK;
}

int ppn_collision_segments(const float* s, const float* e, const int32_t* prob, int32_t n_seg, const float* obs,
                           const int32_t* obs_off, float clearance, uint8_t* hit, void* stream) {
    return ppn_collision_segments_bound(s, e, prob, n_seg, obs, obs_off, clearance, 224.0f, hit, stream);
}

int ppn_extract_paths(const float* heat, int32_t n, int32_t H, int32_t W, const double* init, const double* end,
                      int32_t max_wp, double* wp, int32_t* wp_n, uint8_t* ok, void* stream) {
    if (!heat || n < 0 || H <= 0 || W <= 0 || !init || !end || max_wp <= 0 || max_wp > PPN_MAX_WAYPOINTS || !wp || !wp_n || !ok)
        return PPN_E_INVALID;
    // the walk keeps the reference's bounds test (process_map.py:318 checks the row against size[0] = width and the column
    // against the height), which only indexes inside the map when it is square
    if (H != W) return PPN_E_UNSUPPORTED;
    if (n == 0) return PPN_OK;
    // visited bitmap over the lattice offsets (-M .. M per axis, M = max(H, W)); none (history scan) if it would not fit in LDS
    int vis_dim = 2 * (H > W ? H : W) + 4;
    size_t lds = (((size_t)vis_dim * vis_dim + 31) / 32) * 4;
    if (lds > 48 * 1024) { vis_dim = 0; lds = 0; }
    // the heat map as 8-bit codes behind the bitmap when both fit beside the 8 KB history (values must be k/255: the
    // caller's ToTensor of an 8-bit image, process_map.py:302); H*W a multiple of 4 for the 16-byte staging loads
    const int stage_heat = ((size_t)H * W % 4 == 0 && lds + (size_t)H * W <= 52 * 1024 && ((uintptr_t)heat % 16) == 0 && ((size_t)H * W * 4) % 16 == 0) ? 1 : 0;
    if (stage_heat) lds += (size_t)H * W;
    hipLaunchKernelGGL(ppn::extract_paths_kernel, dim3(n), dim3(64), lds, (hipStream_t)stream, heat, n, H, W, init, end,
                       max_wp, wp, wp_n, ok, vis_dim, stage_heat);
    PPN_HIP(hipGetLastError());
    return PPN_OK;
}

int ppn_na2d_fwd(const void* qkv, const float* rpb, void* out, int32_t B, int32_t H, int32_t W, int32_t heads,
                 int32_t dilation, float scale, int32_t dtype, void* stream) {
    return ppn_na2d_fwd_padded(qkv, rpb, out, B, H, W, H, W, heads, dilation, scale, dtype, stream);
}

int64_t ppn_na2d_bwd_workspace(int32_t B, int32_t H, int32_t W, int32_t heads, int32_t dilation) {
    if (B <= 0 || heads <= 0 || heads > 65535 || dilation < 1 || H < 7 * dilation || W < 7 * dilation) return -1;
    if ((long long)B * heads * H * W >= (1LL << 40)) return -1;
    return ppn::na2d_bwd_workspace_floats(B, H, W, heads, dilation);
}

int ppn_na2d_bwd(const void* qkv, const float* rpb, const void* dout, void* dqkv, float* drpb, float* workspace, int64_t workspace_floats,
                 int32_t B, int32_t H, int32_t W, int32_t heads, int32_t dilation, float scale, int32_t dtype, void* stream) {
    if (!qkv || !rpb || !dout || !dqkv || !drpb || !workspace || (dtype != 0 && dtype != 1)) return PPN_E_INVALID;
    const int64_t need = ppn_na2d_bwd_workspace(B, H, W, heads, dilation);
    if (need < 0 || workspace_floats < need || (reinterpret_cast<uintptr_t>(workspace) & 15)) return PPN_E_INVALID;
    const int e = ppn::na2d_bwd_launch(qkv, rpb, dout, dqkv, drpb, workspace, B, H, W, heads, dilation, scale, dtype, (hipStream_t)stream);
    if (e == -1) return PPN_E_INVALID;
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int64_t ppn_na2d_bwd_vpad_workspace(int32_t B, int32_t H, int32_t W, int32_t Hr, int32_t Wr, int32_t heads, int32_t dilation) {
    if (B <= 0 || Hr <= 0 || Wr <= 0 || heads <= 0 || heads > 65535 || dilation < 1) return -1;
    if (Hr > H || Wr > W || H < 7 * (long long)dilation || W < 7 * (long long)dilation) return -1;
    if ((long long)B * heads * Hr * Wr >= (1LL << 40)) return -1;
    // one workgroup per 8 x 8 region of the largest dilation group's padded sub-image, image and group: the grid's x extent
    const long long hs = (H + (long long)dilation - 1) / dilation, ws = (W + (long long)dilation - 1) / dilation;
    if (((hs + 7) / 8) * ((ws + 7) / 8) * B * dilation * dilation >= (1LL << 31)) return -1;
    return ppn::na2d_bwd_vpad_workspace_floats(B, H, W, Hr, Wr, heads, dilation);
}

int ppn_na2d_bwd_vpad(const void* qkv, const void* pad_kv, const float* rpb, const void* dout, void* dqkv, float* dpad_kv, float* drpb,
                      float* workspace, int64_t workspace_floats, int32_t B, int32_t H, int32_t W, int32_t Hr, int32_t Wr, int32_t heads,
                      int32_t dilation, float scale, int32_t dtype, void* stream) {
    if (!qkv || !pad_kv || !rpb || !dout || !dqkv || !dpad_kv || !drpb || !workspace) return PPN_E_INVALID;
    if (dtype != 0 && dtype != 1) return PPN_E_INVALID;
    if (!(scale > 0.0f) || scale > 3.0e38f) return PPN_E_INVALID;                        // NaN, inf, zero, negative
    if ((((uintptr_t)qkv | (uintptr_t)pad_kv | (uintptr_t)rpb | (uintptr_t)dout | (uintptr_t)dqkv | (uintptr_t)dpad_kv | (uintptr_t)drpb |
          (uintptr_t)workspace) & 15) != 0)
        return PPN_E_INVALID;
    const int64_t need = ppn_na2d_bwd_vpad_workspace(B, H, W, Hr, Wr, heads, dilation);  // every shape check lives there
    if (need < 0 || workspace_floats < need) return PPN_E_INVALID;
    const int e = ppn::na2d_bwd_vpad_launch(qkv, pad_kv, rpb, dout, dqkv, dpad_kv, drpb, workspace, B, H, W, Hr, Wr, heads, dilation, scale, dtype,
                                            (hipStream_t)stream);
    if (e == -1) return PPN_E_INVALID;
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

static int na2d_checked(const void* qkv, const void* pad_kv, const float* rpb, void* out, int32_t B, int32_t H, int32_t W, int32_t Hr,
                        int32_t Wr, int32_t heads, int32_t dilation, float scale, int32_t dtype, void* stream) {
    if (!qkv || !rpb || !out || B <= 0 || heads <= 0 || dilation < 1 || (dtype != 0 && dtype != 1)) return PPN_E_INVALID;
    if (Hr <= 0 || Wr <= 0 || Hr > H || Wr > W) return PPN_E_INVALID;
    if (H < 7 * dilation || W < 7 * dilation) return PPN_E_INVALID;      // caller pads, like NATTEN's module
    {
        const long long hs = (H + dilation - 1) / dilation, ws = (W + dilation - 1) / dilation;
        if (((hs + 15) / 16) * ((ws + 15) / 16) * (long long)B * dilation * dilation > 0x7fffffffLL) return PPN_E_INVALID;
    }
    const int e = ppn::na2d_launch(qkv, pad_kv, rpb, out, B, H, W, Hr, Wr, heads, dilation, scale, dtype, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_na2d_fwd_padded(const void* qkv, const float* rpb, void* out, int32_t B, int32_t H, int32_t W, int32_t Hr, int32_t Wr,
                        int32_t heads, int32_t dilation, float scale, int32_t dtype, void* stream) {
    return na2d_checked(qkv, nullptr, rpb, out, B, H, W, Hr, Wr, heads, dilation, scale, dtype, stream);
}

int ppn_na2d_fwd_vpad(const void* qkv, const void* pad_kv, const float* rpb, void* out, int32_t B, int32_t H, int32_t W, int32_t Hr,
                      int32_t Wr, int32_t heads, int32_t dilation, float scale, int32_t dtype, void* stream) {
    if (!pad_kv) return PPN_E_INVALID;
    return na2d_checked(qkv, pad_kv, rpb, out, B, H, W, Hr, Wr, heads, dilation, scale, dtype, stream);
}

int ppn_swin_wmsa_fwd(const void* qkv, const void* pad_kv, const float* rpb, void* out, int32_t B, int32_t H, int32_t W, int32_t heads,
                      int32_t window, int32_t shift, float scale, int32_t dtype, void* stream) {
    if (!qkv || !pad_kv || !rpb || !out || B <= 0 || H <= 0 || W <= 0 || heads <= 0 || (dtype != 0 && dtype != 1)) return PPN_E_INVALID;
    if (window <= 0 || shift < 0 || shift >= window || !(scale > 0.0f) || scale > 3.0e38f) return PPN_E_INVALID;
    if (window != 7 || (shift != 0 && shift != 3)) return PPN_E_UNSUPPORTED;             // Swin-B's window; shift = window // 2
    if ((((uintptr_t)qkv | (uintptr_t)pad_kv | (uintptr_t)out) & 15) != 0) return PPN_E_INVALID;   // 16-byte loads / stores
    if (heads > 65535) return PPN_E_INVALID;
    const long long windows = (long long)B * ((H + 6) / 7) * ((W + 6) / 7);
    if (windows >= 0x7fffffffLL || (long long)H * W >= 0x7fffffffLL) return PPN_E_INVALID;    // window numbers are 32-bit (token offsets 64-bit)
    const int e = ppn::swin_wmsa_launch(qkv, pad_kv, rpb, out, B, H, W, heads, shift, scale, dtype, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_wmsa_fwd(const void* qkv, const void* pad_kv, const float* rpb, void* out, int32_t B, int32_t H, int32_t W, int32_t heads,
                 int32_t head_dim, int32_t window, int32_t shift, float scale, int32_t dtype, void* stream) {
    if (!qkv || !pad_kv || !rpb || !out || B <= 0 || H <= 0 || W <= 0 || heads <= 0 || heads > 65535 || (dtype != 0 && dtype != 1))
        return PPN_E_INVALID;
    if (!(scale > 0.0f) || scale > 3.0e38f) return PPN_E_INVALID;                        // NaN, inf, zero, negative
    const bool w14 = window == 14 && (head_dim == 8 || head_dim == 16 || head_dim == 32);   // AESwin's inner stages
    const bool w7 = window == 7 && (head_dim == 8 || head_dim == 16 || head_dim == 32);     // 32: Swin-B's kernel (swin_wmsa.hip)
    if ((!w14 && !w7) || (shift != 0 && shift != window / 2)) return PPN_E_UNSUPPORTED;
    if ((((uintptr_t)qkv | (uintptr_t)pad_kv | (uintptr_t)rpb | (uintptr_t)out) & 15) != 0) return PPN_E_INVALID;   // 16-byte loads / stores
    // window numbers are 32-bit (token offsets 64-bit); in steps, each within 64 bits: H W < 2^31, so windows per image < 2^31, then
    // B x that, then x heads x the workgroup's work-items
    if ((long long)H * W >= 0x7fffffffLL) return PPN_E_INVALID;
    const long long per_image = (((long long)H + window - 1) / window) * (((long long)W + window - 1) / window);
    if (per_image >= 0x7fffffffLL || (long long)B * per_image >= 0x7fffffffLL) return PPN_E_INVALID;
    if ((long long)B * per_image * heads >= 0x7fffffffLL / ppn::wmsa_gen_threads(window)) return PPN_E_INVALID;
    const int e = ppn::wmsa_gen_launch(qkv, pad_kv, rpb, out, B, H, W, heads, head_dim, window, shift, scale, dtype, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int64_t ppn_swin_wmsa_bwd_workspace(int32_t B, int32_t H, int32_t W, int32_t heads) {
    if (B <= 0 || H <= 0 || W <= 0 || heads <= 0 || heads > 65535) return -1;
    return ppn::swin_wmsa_bwd_workspace_floats(heads);
}

int ppn_swin_wmsa_bwd(const void* qkv, const void* pad_kv, const float* rpb, const void* dout, void* dqkv, float* dpad_kv, float* drpb,
                      float* workspace, int64_t workspace_floats, int32_t B, int32_t H, int32_t W, int32_t heads, int32_t window, int32_t shift,
                      float scale, int32_t dtype, void* stream) {
    if (!qkv || !pad_kv || !rpb || !dout || !dqkv || !dpad_kv || !drpb || !workspace) return PPN_E_INVALID;
    if (B <= 0 || H <= 0 || W <= 0 || heads <= 0 || heads > 65535 || (dtype != 0 && dtype != 1)) return PPN_E_INVALID;
    if (!(scale > 0.0f) || scale > 3.0e38f) return PPN_E_INVALID;                        // NaN, inf, zero, negative
    if (window != 7 || (shift != 0 && shift != 3)) return PPN_E_UNSUPPORTED;             // Swin-B's window; shift = window // 2
    if ((((uintptr_t)qkv | (uintptr_t)pad_kv | (uintptr_t)rpb | (uintptr_t)dout | (uintptr_t)dqkv | (uintptr_t)dpad_kv | (uintptr_t)drpb |
          (uintptr_t)workspace) & 15) != 0)
        return PPN_E_INVALID;
    // window numbers are 32-bit (token offsets 64-bit); in steps, each within 64 bits: H W < 2^31, so windows per image < 2^31, then B x that
    if ((long long)H * W >= 0x7fffffffLL) return PPN_E_INVALID;
    const long long per_image = ((H + 6LL) / 7) * ((W + 6LL) / 7);
    if (per_image >= 0x7fffffffLL || (long long)B * per_image >= 0x7fffffffLL) return PPN_E_INVALID;
    const int64_t need = ppn_swin_wmsa_bwd_workspace(B, H, W, heads);                    // per device: the one check that asks the runtime
    if (need < 0 || workspace_floats < need) return PPN_E_INVALID;
    const int e = ppn::swin_wmsa_bwd_launch(qkv, pad_kv, rpb, dout, dqkv, dpad_kv, drpb, workspace, B, H, W, heads, shift, scale, dtype,
                                            (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_mhsa_fwd(const void* qkv, void* out, int32_t B, int32_t N, int32_t heads, int32_t head_dim, float scale, int32_t dtype,
                 void* stream) {
    if (!qkv || !out || B <= 0 || N <= 0 || heads <= 0 || head_dim <= 0 || (dtype != 0 && dtype != 1)) return PPN_E_INVALID;
    if (!(scale > 0.0f) || scale > 3.0e38f) return PPN_E_INVALID;                        // NaN, inf, zero, negative
    if (head_dim != 64 && head_dim != 8) return PPN_E_UNSUPPORTED;
    if ((((uintptr_t)qkv | (uintptr_t)out) & 15) != 0) return PPN_E_INVALID;              // 16-byte loads / stores
    const bool d8 = head_dim == 8;                                                         // mhsa_d8.hip: one block shape, both dtypes
    const long long qblock = d8 ? ppn::mhsa_d8_block_rows() : dtype == 0 ? 64 : 128;       // queries / work-items per workgroup
    const long long threads = d8 ? ppn::mhsa_d8_block_threads() : dtype == 0 ? 64 : 256;
    if ((long long)B * heads * ((N + qblock - 1) / qblock) * threads >= 0x7fffffffLL) return PPN_E_INVALID;
    const int e = d8 ? ppn::mhsa_d8_launch(qkv, out, B, N, heads, scale, dtype, (hipStream_t)stream)
                     : ppn::mhsa_launch(qkv, out, B, N, heads, scale, dtype, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int64_t ppn_mhsa_bwd_workspace(int32_t B, int32_t N, int32_t heads) {
    if (B <= 0 || N <= 0 || heads <= 0) return -1;
    if ((long long)B * heads >= (1LL << 40) / N) return -1;                                // statistics of fewer than 2^40 queries
    return ppn::mhsa_bwd_workspace_floats(B, N, heads);
}

int ppn_mhsa_bwd(const void* qkv, const void* out, const void* dout, void* dqkv, float* workspace, int64_t workspace_floats,
                 int32_t B, int32_t N, int32_t heads, int32_t head_dim, float scale, int32_t dtype, void* stream) {
    if (!qkv || !out || !dout || !dqkv || !workspace || B <= 0 || N <= 0 || heads <= 0 || head_dim <= 0 || (dtype != 0 && dtype != 1))
        return PPN_E_INVALID;
    if (!(scale > 0.0f) || scale > 3.0e38f) return PPN_E_INVALID;                        // NaN, inf, zero, negative
    if (head_dim != 64 && head_dim != 8) return PPN_E_UNSUPPORTED;
    if ((((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)dout | (uintptr_t)dqkv | (uintptr_t)workspace) & 15) != 0) return PPN_E_INVALID;
    const bool d8 = head_dim == 8;                                                         // mhsa_d8.hip: one block shape, both dtypes
    const long long block = d8 ? ppn::mhsa_d8_block_rows() : dtype == 0 ? 64 : 128;        // rows / work-items per workgroup, every pass
    const long long threads = d8 ? ppn::mhsa_d8_block_threads() : dtype == 0 ? 128 : 256;
    if ((long long)B * heads * ((N + block - 1) / block) * threads >= 0x7fffffffLL) return PPN_E_INVALID;
    const int64_t need = ppn_mhsa_bwd_workspace(B, N, heads);
    if (need < 0 || workspace_floats < need) return PPN_E_INVALID;
    const int e = d8 ? ppn::mhsa_d8_bwd_launch(qkv, out, dout, dqkv, workspace, B, N, heads, scale, dtype, (hipStream_t)stream)
                     : ppn::mhsa_bwd_launch(qkv, out, dout, dqkv, workspace, B, N, heads, scale, dtype, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int64_t ppn_resize_ce_workspace(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return -1;
    if ((long long)H * W >= 0x80000000LL || (long long)B * ((long long)H * W) >= 0x80000000LL) return -1;      // pixel numbers are 32-bit
    return ppn::resize_ce_workspace_floats(B, H, W);
}

// B C h w < 2^31, in steps that each stay within 64 bits
static bool resize_ce_sizes_ok(int B, int C, int h, int w, int H, int W) {
    if (B <= 0 || C <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return false;
    const long long hw = (long long)h * w;
    if (hw >= 0x80000000LL || (long long)C * hw >= 0x80000000LL || (long long)B * ((long long)C * hw) >= 0x80000000LL) return false;
    return ppn_resize_ce_workspace(B, H, W) >= 0;
}

// work-items of a backward gather's launch: 1, 8 or 64 lanes per dlogit element in whole workgroups of `threads`, below 2^31
static bool gather_launch_ok(int threads, int B, int C, int h, int w, int H, int W) {
    const long long per = threads / ppn::resize_ce_bwd_lanes(h, w, H, W);
    return (((long long)B * C * h * w + per - 1) / per) * threads < 0x7fffffffLL;
}

int ppn_resize_ce_fwd(const void* logit, const void* label, float* lse, float* loss, int64_t* correct, float* workspace, int64_t workspace_floats,
                      int B, int C, int h, int w, int H, int W, int ignore_index, int logit_dtype, int label_dtype, void* stream) {
    if (!logit || !label || !loss || !correct || !workspace) return PPN_E_INVALID;                    // lse may be NULL: no backward wanted
    if ((logit_dtype != 0 && logit_dtype != 1) || (label_dtype != 0 && label_dtype != 1)) return PPN_E_INVALID;
    if ((((uintptr_t)logit | (uintptr_t)lse | (uintptr_t)workspace) & 15) != 0) return PPN_E_INVALID;
    if (((uintptr_t)loss & 3) != 0 || ((uintptr_t)correct & 7) != 0 || (label_dtype == 1 && ((uintptr_t)label & 7) != 0)) return PPN_E_INVALID;
    if (!resize_ce_sizes_ok(B, C, h, w, H, W)) return PPN_E_INVALID;
    // work-items of the forward launch: one per pixel in whole workgroups
    const long long px = ppn::resize_ce_fwd_pixels(), groups = ((long long)B * H * W + px - 1) / px;
    if (groups * ppn::resize_ce_threads() >= 0x7fffffffLL) return PPN_E_INVALID;
    const int64_t need = ppn_resize_ce_workspace(B, H, W);
    if (need < 0 || workspace_floats < need) return PPN_E_INVALID;
    const int e = ppn::resize_ce_fwd_launch(logit, label, lse, loss, correct, workspace, B, C, h, w, H, W, ignore_index, logit_dtype, label_dtype,
                                            (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_resize_ce_bwd(const void* logit, const void* label, const float* lse, const float* grad_out, void* dlogit, int B, int C, int h, int w,
                      int H, int W, int ignore_index, int logit_dtype, int label_dtype, void* stream) {
    if (!logit || !label || !lse || !grad_out || !dlogit) return PPN_E_INVALID;
    if ((logit_dtype != 0 && logit_dtype != 1) || (label_dtype != 0 && label_dtype != 1)) return PPN_E_INVALID;
    if ((((uintptr_t)logit | (uintptr_t)lse | (uintptr_t)dlogit) & 15) != 0) return PPN_E_INVALID;
    if (((uintptr_t)grad_out & 3) != 0 || (label_dtype == 1 && ((uintptr_t)label & 7) != 0)) return PPN_E_INVALID;
    if (!resize_ce_sizes_ok(B, C, h, w, H, W)) return PPN_E_INVALID;
    if (!gather_launch_ok(ppn::resize_ce_threads(), B, C, h, w, H, W)) return PPN_E_INVALID;
    const int e = ppn::resize_ce_bwd_launch(logit, label, lse, grad_out, dlogit, B, C, h, w, H, W, ignore_index, logit_dtype, label_dtype,
                                            (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_seg_eval(const void* logit, const void* label, uint8_t* pred, int64_t* areas, int B, int C, int h, int w, int H, int W, int ignore_index,
                 int logit_dtype, int label_dtype, void* stream) {
    if (!logit || !label || !areas) return PPN_E_INVALID;                                             // pred may be NULL: histograms only
    if ((logit_dtype != 0 && logit_dtype != 1) || (label_dtype != 0 && label_dtype != 1)) return PPN_E_INVALID;
    if (((uintptr_t)logit & 15) != 0 || ((uintptr_t)areas & 7) != 0 || (label_dtype == 1 && ((uintptr_t)label & 7) != 0)) return PPN_E_INVALID;
    if (!resize_ce_sizes_ok(B, C, h, w, H, W) || C > ppn::seg_eval_max_classes()) return PPN_E_INVALID;
    // work-items of the launch: a workgroup per tile of pixels, at most seg_eval_max_groups of them
    const long long px = ppn::seg_eval_pixels(), tiles = ((long long)B * H * W + px - 1) / px;
    const long long groups = tiles < ppn::seg_eval_max_groups() ? tiles : ppn::seg_eval_max_groups();
    if (tiles >= 0x7fffffffLL || groups * ppn::seg_eval_threads() >= 0x7fffffffLL) return PPN_E_INVALID;
    const int e = ppn::seg_eval_launch(logit, label, pred, areas, B, C, h, w, H, W, ignore_index, logit_dtype, label_dtype, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_seg_tta(const ppn_tta_aug* augs, int n_augs, uint8_t* pred, float* prob, int B, int C, int H, int W, int logit_dtype, void* stream) {
    if (!augs || n_augs < 1 || n_augs > PPN_SEG_TTA_MAX_AUGS) return PPN_E_INVALID;
    if ((!pred && !prob) || (logit_dtype != 0 && logit_dtype != 1)) return PPN_E_INVALID;             // either output may be NULL, not both
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || C > ppn::seg_tta_max_classes()) return PPN_E_INVALID;
    if (C > PPN_SEG_TTA_REG_CLASSES && !prob) return PPN_E_INVALID;                                    // prob is the accumulator
    if (((uintptr_t)prob & 3) != 0) return PPN_E_INVALID;
    // B H W and B C H W < 2^31, in steps that each stay within 64 bits
    const long long HW = (long long)H * W;
    if (HW >= 0x80000000LL || (long long)B * HW >= 0x80000000LL || (long long)C * HW >= 0x80000000LL ||
        (long long)B * ((long long)C * HW) >= 0x80000000LL)
        return PPN_E_INVALID;
    for (int a = 0; a < n_augs; ++a) {
        const ppn_tta_aug& g = augs[a];
        if (!g.logit || ((uintptr_t)g.logit & 15) != 0 || g.flip < 0 || g.flip > 2) return PPN_E_INVALID;
        if (g.h <= 0 || g.w <= 0 || g.hm <= 0 || g.wm <= 0) return PPN_E_INVALID;
        const long long hw = (long long)g.h * g.w;
        if (hw >= 0x80000000LL || (long long)C * hw >= 0x80000000LL || (long long)B * ((long long)C * hw) >= 0x80000000LL) return PPN_E_INVALID;
    }
    // work-items of the launch: a workgroup per tile of pixels
    const long long px = ppn::seg_tta_pixels(), tiles = ((long long)B * HW + px - 1) / px;
    if (tiles * ppn::seg_tta_threads() >= 0x7fffffffLL) return PPN_E_INVALID;
    const int e = ppn::seg_tta_launch(augs, n_augs, pred, prob, B, C, H, W, logit_dtype, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int64_t ppn_ohem_ce_workspace(int B, int H, int W) {
    if (ppn_resize_ce_workspace(B, H, W) < 0) return -1;                                               // the same limits on B, H, W
    return ppn::ohem_ce_workspace_bytes();
}

// what both OHEM entry points check alike: sizes, dtypes, mode, and the buffers they share
static bool ohem_ce_common_ok(const void* logit, const void* label, const float* class_weight, const float* lse, const float* score, int B, int C,
                              int h, int w, int H, int W, int mode, int logit_dtype, int label_dtype) {
    if (!logit || !label || !lse || !score) return false;                                              // class_weight may be NULL: all ones
    if ((logit_dtype != 0 && logit_dtype != 1) || (label_dtype != 0 && label_dtype != 1) || mode < 0 || mode > 2) return false;
    if ((((uintptr_t)logit | (uintptr_t)lse | (uintptr_t)score) & 15) != 0 || ((uintptr_t)class_weight & 3) != 0) return false;
    if (label_dtype == 1 && ((uintptr_t)label & 7) != 0) return false;
    return resize_ce_sizes_ok(B, C, h, w, H, W);
}

int ppn_ohem_ce_fwd(const void* logit, const void* label, const float* class_weight, float* lse, float* score, float* loss, int64_t* counts,
                    float* threshold, uint8_t* mask, void* workspace, int64_t workspace_bytes, int B, int C, int h, int w, int H, int W,
                    int ignore_index, int mode, float thresh, int min_kept, int logit_dtype, int label_dtype, void* stream) {
    if (!loss || !counts || !threshold || !workspace) return PPN_E_INVALID;                            // mask may be NULL: not wanted
    if (!ohem_ce_common_ok(logit, label, class_weight, lse, score, B, C, h, w, H, W, mode, logit_dtype, label_dtype)) return PPN_E_INVALID;
    if (((uintptr_t)workspace & 15) != 0 || (((uintptr_t)loss | (uintptr_t)threshold) & 3) != 0 || ((uintptr_t)counts & 7) != 0) return PPN_E_INVALID;
    if (mode != 0 && min_kept < 1) return PPN_E_INVALID;
    if (mode == 1 && !(thresh > 0.0f && thresh <= 1.0f)) return PPN_E_INVALID;                         // NaN included
    const long long n_px = (long long)B * H * W, px = ppn::ohem_ce_pixels(), tiles = (n_px + px - 1) / px;
    const long long groups = tiles < ppn::ohem_ce_max_groups() ? tiles : ppn::ohem_ce_max_groups();
    if (tiles >= 0x7fffffffLL || groups * ppn::ohem_ce_threads() >= 0x7fffffffLL) return PPN_E_INVALID;
    const int64_t need = ppn_ohem_ce_workspace(B, H, W);
    if (need < 0 || workspace_bytes < need) return PPN_E_INVALID;
    // batch_kept = min_kept * B, capped at the pixel count (beyond n_valid every value means the same)
    const long long kept = mode == 0 ? n_px : ((long long)min_kept * B < n_px ? (long long)min_kept * B : n_px);
    const int e = ppn::ohem_ce_fwd_launch(logit, label, class_weight, lse, score, loss, counts, threshold, mask, workspace, B, C, h, w, H, W,
                                          ignore_index, mode, thresh, (uint32_t)kept, logit_dtype, label_dtype, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_ohem_ce_bwd(const void* logit, const void* label, const float* class_weight, const float* lse, const float* score, const float* threshold,
                    const float* grad_out, void* dlogit, int B, int C, int h, int w, int H, int W, int ignore_index, int mode, int logit_dtype,
                    int label_dtype, void* stream) {
    if (!threshold || !grad_out || !dlogit) return PPN_E_INVALID;
    if (!ohem_ce_common_ok(logit, label, class_weight, lse, score, B, C, h, w, H, W, mode, logit_dtype, label_dtype)) return PPN_E_INVALID;
    if (((uintptr_t)dlogit & 15) != 0 || (((uintptr_t)threshold | (uintptr_t)grad_out) & 3) != 0) return PPN_E_INVALID;
    if (!gather_launch_ok(ppn::ohem_ce_threads(), B, C, h, w, H, W)) return PPN_E_INVALID;
    const int e = ppn::ohem_ce_bwd_launch(logit, label, class_weight, lse, score, threshold, grad_out, dlogit, B, C, h, w, H, W, ignore_index, mode,
                                          logit_dtype, label_dtype, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int64_t ppn_resize_dice_workspace(int B, int C, int H, int W) {
    if (C <= 0 || C > ppn::resize_dice_max_classes() || ppn_resize_ce_workspace(B, H, W) < 0) return -1;  // the same limits on B, H, W
    return ppn::resize_dice_workspace_bytes(B, C, H, W);
}

// what both Dice entry points check alike: the buffers they share, dtypes, sizes, smooth
static bool resize_dice_common_ok(const void* logit, const void* label, const float* class_weight, const void* workspace, const float* lse,
                                  const double* sums, int B, int C, int h, int w, int H, int W, float smooth, int logit_dtype, int label_dtype) {
    if (!logit || !label || !workspace || !sums) return false;                                         // class_weight may be NULL: all ones
    if ((logit_dtype != 0 && logit_dtype != 1) || (label_dtype != 0 && label_dtype != 1)) return false;
    if ((((uintptr_t)logit | (uintptr_t)workspace | (uintptr_t)lse) & 15) != 0) return false;
    if (((uintptr_t)class_weight & 3) != 0 || ((uintptr_t)sums & 7) != 0 || (label_dtype == 1 && ((uintptr_t)label & 7) != 0)) return false;
    if (!(smooth >= 0.0f) || smooth > 3.0e38f) return false;                                           // NaN, negative, inf
    if (!resize_ce_sizes_ok(B, C, h, w, H, W) || C > ppn::resize_dice_max_classes()) return false;
    // work-items of the per-pixel launches: a workgroup per tile of an image's pixels
    const long long px = ppn::resize_dice_pixels(), tiles = (long long)B * (((long long)H * W + px - 1) / px);
    return tiles * ppn::resize_dice_threads() < 0x7fffffffLL;
}

int ppn_resize_dice_fwd(const void* logit, const void* label, const float* class_weight, void* workspace, float* lse, double* sums, float* loss,
                        int64_t* correct, int B, int C, int h, int w, int H, int W, int ignore_index, float smooth, int logit_dtype,
                        int label_dtype, void* stream) {
    if (!loss || !correct) return PPN_E_INVALID;                                                       // lse may be NULL: no backward wanted
    if (!resize_dice_common_ok(logit, label, class_weight, workspace, lse, sums, B, C, h, w, H, W, smooth, logit_dtype, label_dtype))
        return PPN_E_INVALID;
    if (((uintptr_t)loss & 3) != 0 || ((uintptr_t)correct & 7) != 0) return PPN_E_INVALID;
    const int e = ppn::resize_dice_fwd_launch(logit, label, class_weight, workspace, lse, sums, loss, correct, B, C, h, w, H, W, ignore_index, smooth,
                                              logit_dtype, label_dtype, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_resize_dice_bwd(const void* logit, const void* label, const float* lse, const double* sums, const float* class_weight,
                        const float* grad_out, void* workspace, void* dlogit, int B, int C, int h, int w, int H, int W, int ignore_index,
                        float smooth, int logit_dtype, int label_dtype, void* stream) {
    if (!lse || !grad_out || !dlogit) return PPN_E_INVALID;
    if (!resize_dice_common_ok(logit, label, class_weight, workspace, lse, sums, B, C, h, w, H, W, smooth, logit_dtype, label_dtype))
        return PPN_E_INVALID;
    if (((uintptr_t)dlogit & 15) != 0 || ((uintptr_t)grad_out & 3) != 0) return PPN_E_INVALID;
    if (!gather_launch_ok(ppn::resize_dice_threads(), B, C, h, w, H, W)) return PPN_E_INVALID;
    const int e = ppn::resize_dice_bwd_launch(logit, label, lse, sums, class_weight, grad_out, workspace, dlogit, B, C, h, w, H, W, ignore_index,
                                              smooth, logit_dtype, label_dtype, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_residual_layernorm(const void* x, const void* a, const void* gamma, const void* w, const void* b, void* x_out,
                           void* y_out, int64_t rows, int32_t C, float eps, int32_t dtype, void* stream) {
    return ppn_residual_layernorm_padded(x, a, gamma, w, b, x_out, y_out, rows, C, eps, dtype, 0, 0, 0, 0, stream);
}

int ppn_residual_layernorm_padded(const void* x, const void* a, const void* gamma, const void* w, const void* b, void* x_out,
                                  void* y_out, int64_t rows, int32_t C, float eps, int32_t dtype, int32_t Hr, int32_t Wr,
                                  int32_t Hp, int32_t Wp, void* stream) {
    if (Hp != 0 && (Hr <= 0 || Wr <= 0 || Hp < Hr || Wp < Wr || rows % ((int64_t)Hr * Wr) != 0)) return PPN_E_INVALID;
    if (!x || rows < 0 || C <= 0 || (C % 8) != 0 || (dtype != 0 && dtype != 1)) return PPN_E_INVALID;
    if (a && !x_out) return PPN_E_INVALID;
    if (!a && !y_out) return PPN_E_INVALID;
    if (y_out && (!w || !b)) return PPN_E_INVALID;
    if (rows == 0) return PPN_OK;
    const int e = ppn::norm_launch(x, a, gamma, w, b, x_out, y_out, rows, C, eps, dtype, Hr, Wr, Hp, Wp, nullptr, (hipStream_t)stream);
    if (e == -1) return PPN_E_UNSUPPORTED;
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_layernorm_offset(const void* x, const float* xoff, const void* w, const void* b, void* y_out, int64_t rows, int32_t C, float eps,
                         int32_t dtype, void* stream) {
    if (!x || !y_out || !w || !b || rows < 0 || C <= 0 || (C % 8) != 0 || (dtype != 0 && dtype != 1)) return PPN_E_INVALID;
    if (rows == 0) return PPN_OK;
    const int e = ppn::norm_launch(x, nullptr, nullptr, w, b, nullptr, y_out, rows, C, eps, dtype, 0, 0, 0, 0, xoff, (hipStream_t)stream);
    if (e == -1) return PPN_E_UNSUPPORTED;
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int64_t ppn_residual_layernorm_bwd_workspace(int64_t rows, int32_t C) {
    return ppn::residual_ln_bwd_workspace_floats(rows, C);
}

int ppn_residual_layernorm_train_fwd(const void* x, const void* a, const void* gamma, const float* scale, const void* w, const void* b, void* x_out,
                                     void* y_out, float* stats, int64_t rows, int64_t rows_per_image, int32_t C, float eps, int32_t dtype,
                                     void* stream) {
    if (!x || rows <= 0 || (dtype != 0 && dtype != 1)) return PPN_E_INVALID;
    if (a ? !x_out : !y_out) return PPN_E_INVALID;                           // nothing to write
    if (y_out && (!w || !b || !stats)) return PPN_E_INVALID;
    if (scale && (rows_per_image <= 0 || rows % rows_per_image != 0)) return PPN_E_INVALID;
    if (ppn::residual_ln_bwd_workspace_floats(rows, C) < 0) return PPN_E_UNSUPPORTED;      // the width (or 2^31 rows and more)
    const int e = ppn::residual_ln_train_fwd_launch(x, a, gamma, scale, w, b, x_out, y_out, stats, rows, scale ? rows_per_image : 1, C, eps, dtype,
                                                    (hipStream_t)stream);
    if (e == -1) return PPN_E_UNSUPPORTED;
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_residual_layernorm_bwd(const void* gy, const void* gx, const void* xn, const void* a, const void* gamma, const float* scale, const void* w,
                               const float* stats, void* dx, void* da, void* dgamma, void* dw, void* dbeta, float* workspace,
                               int64_t workspace_floats, int64_t rows, int64_t rows_per_image, int32_t C, int32_t dtype, void* stream) {
    if ((!gy && !gx) || !workspace || rows <= 0 || (dtype != 0 && dtype != 1)) return PPN_E_INVALID;
    if (gy && (!xn || !stats || !w || !dx)) return PPN_E_INVALID;            // the LayerNorm term needs its inputs and changes dx
    if (dgamma && (!a || !gamma)) return PPN_E_INVALID;
    if ((dw || dbeta) && !gy) return PPN_E_INVALID;
    if (!dx && !da && !dgamma) return PPN_E_INVALID;                         // nothing to write
    if (scale && (rows_per_image <= 0 || rows % rows_per_image != 0)) return PPN_E_INVALID;
    const long long need = ppn::residual_ln_bwd_workspace_floats(rows, C);
    if (need < 0) return PPN_E_UNSUPPORTED;                                  // the width (or 2^31 rows and more)
    if (workspace_floats < need) return PPN_E_INVALID;
    const int e = ppn::residual_ln_bwd_launch(gy, gx, xn, stats, dgamma ? a : nullptr, gamma, scale, w, dx, da, dgamma, dw, dbeta, workspace, rows,
                                              scale ? rows_per_image : 1, C, dtype, (hipStream_t)stream);
    if (e == -1) return PPN_E_UNSUPPORTED;
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_patch_merge_ln_rows(int C) { return ppn::patch_merge_ln_rows(C); }
int ppn_patch_merge_ln_max_blocks(void) { return ppn::patch_merge_ln_max_blocks(); }

// what the three patch-merge entry points check alike: extents, width, element counts.  PPN_OK, PPN_E_INVALID or PPN_E_UNSUPPORTED
static int patch_merge_sizes(int B, int H, int W, int C) {
    if (B < 1 || H < 1 || W < 1 || C < 1) return PPN_E_INVALID;
    if (ppn::patch_merge_ln_rows(C) == 0) return PPN_E_UNSUPPORTED;            // C outside {8, 16, 32, 64, 128, 256, 512}
    const long long Ho = ((long long)H + 1) / 2, Wo = ((long long)W + 1) / 2;
    // x and the gathered rows (the padded grid: a little more than x at odd sizes) stay below 2^31 elements; overflow-safe in this order
    if ((long long)B * H >= 0x7fffffffLL || (long long)B * H * W >= 0x7fffffffLL || (long long)B * H * W * C >= 0x7fffffffLL) return PPN_E_INVALID;
    if (B * Ho * Wo * 4 * C >= 0x7fffffffLL) return PPN_E_INVALID;
    return PPN_OK;
}

int64_t ppn_patch_merge_ln_bwd_workspace(int B, int H, int W, int C) {
    if (patch_merge_sizes(B, H, W, C) != PPN_OK) return -1;
    return ppn::patch_merge_ln_bwd_workspace_bytes((long long)B * ((H + 1) / 2) * ((W + 1) / 2), C);
}

int ppn_patch_merge_ln_fwd(const void* x, const void* gamma, const void* beta, void* y, float* stats, int B, int H, int W, int C, float eps,
                           int dtype, void* stream) {
    if (!x || !gamma || !beta || !y) return PPN_E_INVALID;                                               // stats may be NULL: inference
    if ((((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)y) & 15) != 0 || ((uintptr_t)stats & 3) != 0) return PPN_E_INVALID;
    if (dtype != 0 && dtype != 1) return PPN_E_INVALID;
    if (!(eps >= 0.0f) || eps > 3.0e38f) return PPN_E_INVALID;                                           // NaN, negative, inf
    const int ok = patch_merge_sizes(B, H, W, C);
    if (ok != PPN_OK) return ok;
    const int e = ppn::patch_merge_ln_fwd_launch(x, gamma, beta, y, stats, B, H, W, C, eps, dtype, (hipStream_t)stream);
    if (e == -1) return PPN_E_UNSUPPORTED;
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_patch_merge_ln_bwd(const void* gy, const void* x, const float* stats, const void* gamma, void* workspace, void* dx, void* dgamma,
                           void* dbeta, int B, int H, int W, int C, int dtype, void* stream) {
    if (!gy || !x || !stats || !gamma || !workspace || !dx) return PPN_E_INVALID;                        // dgamma, dbeta may be NULL: not wanted
    if ((((uintptr_t)gy | (uintptr_t)x | (uintptr_t)gamma | (uintptr_t)workspace | (uintptr_t)dx | (uintptr_t)dgamma | (uintptr_t)dbeta) & 15) != 0 ||
        ((uintptr_t)stats & 3) != 0)
        return PPN_E_INVALID;
    if (dtype != 0 && dtype != 1) return PPN_E_INVALID;
    const int ok = patch_merge_sizes(B, H, W, C);
    if (ok != PPN_OK) return ok;
    const int e = ppn::patch_merge_ln_bwd_launch(gy, x, stats, gamma, (float*)workspace, dx, dgamma, dbeta, B, H, W, C, dtype, (hipStream_t)stream);
    if (e == -1) return PPN_E_UNSUPPORTED;
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

// what the three stem-training entry points check alike: extents, the pixel count, the channel set, z's element count
static int stem_train_sizes(int B, int H, int W, int C) {
    if (B < 1 || H < 1 || W < 1 || C < 1) return PPN_E_INVALID;
    if ((long long)B * H > 0x7fffffffLL || (long long)B * H * W > 0x7fffffffLL) return PPN_E_INVALID;     // overflow-safe in this order
    if ((long long)B * H * W < 2) return PPN_E_INVALID;                       // one value per channel has no batch variance
    if (!ppn::gennet_stem_channels_ok(C)) return PPN_E_UNSUPPORTED;           // C outside {8, 16, 24, 32}
    if ((long long)B * H * W * C >= 0x80000000LL) return PPN_E_INVALID;       // z: 2^31 elements or more
    return PPN_OK;
}

static bool stem_scalar_ok(float v) { return v >= 0.0f && v <= 3.0e38f; }     // not NaN, not negative, not inf

int64_t ppn_gennet_stem_train_workspace(int B, int H, int W, int C) {
    if (stem_train_sizes(B, H, W, C) != PPN_OK) return -1;
    return ppn::gennet_stem_train_workspace_bytes((long long)B * H * W, C);
}

int ppn_gennet_stem_train_fwd(const float* x, const float* w, const float* bias, const float* gamma, const float* beta, void* z, float* stats,
                              double* moments, void* workspace, int B, int H, int W, int C, float eps, float negative_slope, int dtype,
                              void* stream) {
    if (!x || !w || !gamma || !beta || !z || !stats || !moments || !workspace) return PPN_E_INVALID;     // bias may be NULL: none
    if ((((uintptr_t)x | (uintptr_t)w | (uintptr_t)bias | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)z | (uintptr_t)workspace) & 15) != 0 ||
        ((uintptr_t)moments & 7) != 0 || ((uintptr_t)stats & 3) != 0)
        return PPN_E_INVALID;
    if (dtype != 0 && dtype != 1) return PPN_E_INVALID;
    if (!stem_scalar_ok(eps) || !stem_scalar_ok(negative_slope)) return PPN_E_INVALID;
    const int ok = stem_train_sizes(B, H, W, C);
    if (ok != PPN_OK) return ok;
    const int e = ppn::gennet_stem_train_fwd_launch(x, w, bias, gamma, beta, z, stats, moments, workspace, B, H, W, C, eps, negative_slope, dtype,
                                                    (hipStream_t)stream);
    if (e == -1) return PPN_E_UNSUPPORTED;
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_gennet_stem_train_bwd(const void* dz, const float* x, const float* w, const float* bias, const float* gamma, const float* beta,
                              const float* stats, const double* moments, void* workspace, float* dw, float* dgamma, float* dbeta, int B, int H,
                              int W, int C, float negative_slope, int dtype, void* stream) {
    if (!dz || !x || !w || !gamma || !beta || !stats || !moments || !workspace || !dw || !dgamma || !dbeta) return PPN_E_INVALID;
    if ((((uintptr_t)dz | (uintptr_t)x | (uintptr_t)w | (uintptr_t)bias | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)workspace | (uintptr_t)dw |
          (uintptr_t)dgamma | (uintptr_t)dbeta) & 15) != 0 || ((uintptr_t)moments & 7) != 0 || ((uintptr_t)stats & 3) != 0)
        return PPN_E_INVALID;
    if (dtype != 0 && dtype != 1) return PPN_E_INVALID;
    if (!stem_scalar_ok(negative_slope)) return PPN_E_INVALID;
    const int ok = stem_train_sizes(B, H, W, C);
    if (ok != PPN_OK) return ok;
    const int e = ppn::gennet_stem_train_bwd_launch(dz, x, w, bias, gamma, beta, stats, moments, workspace, dw, dgamma, dbeta, B, H, W, C,
                                                    negative_slope, dtype, (hipStream_t)stream);
    if (e == -1) return PPN_E_UNSUPPORTED;
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_gennet_stem_train_tile(void) { return ppn::gennet_stem_tile(); }
int ppn_gennet_stem_train_max_blocks(void) { return ppn::gennet_stem_max_blocks(); }

// what the three tail-training entry points check alike: extents, the pixel count, the channel set, y's element count
static int tail_train_sizes(int B, int H, int W, int C) {
    if (B < 1 || H < 1 || W < 1 || C < 1) return PPN_E_INVALID;
    if ((long long)B * H > 0x7fffffffLL || (long long)B * H * W > 0x7fffffffLL) return PPN_E_INVALID;     // overflow-safe in this order
    if ((long long)B * H * W < 2) return PPN_E_INVALID;                       // one value per channel has no batch variance
    if (!ppn::gennet_tail_channels_ok(C)) return PPN_E_UNSUPPORTED;           // C outside {8, 16, 24, 32}
    if ((long long)B * H * W * C >= 0x80000000LL) return PPN_E_INVALID;       // y: 2^31 elements or more
    return PPN_OK;
}

int64_t ppn_gennet_tail_train_workspace(int B, int H, int W, int C) {
    if (tail_train_sizes(B, H, W, C) != PPN_OK) return -1;
    return ppn::gennet_tail_train_workspace_bytes((long long)B * H * W, C);
}

int ppn_gennet_tail_train_fwd(const void* y, const float* gamma, const float* beta, const float* wf, const float* bf, void* out, float* stats,
                              void* workspace, int B, int H, int W, int C, float eps, float negative_slope, int dtype, void* stream) {
    if (!y || !gamma || !beta || !wf || !out || !stats || !workspace) return PPN_E_INVALID;              // bf may be NULL: no bias
    if ((((uintptr_t)y | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)wf | (uintptr_t)out | (uintptr_t)workspace) & 15) != 0 ||
        (((uintptr_t)bf | (uintptr_t)stats) & 3) != 0)
        return PPN_E_INVALID;
    if (dtype != 0 && dtype != 1) return PPN_E_INVALID;
    if (!stem_scalar_ok(eps) || !stem_scalar_ok(negative_slope)) return PPN_E_INVALID;
    const int ok = tail_train_sizes(B, H, W, C);
    if (ok != PPN_OK) return ok;
    const int e = ppn::gennet_tail_train_fwd_launch(y, gamma, beta, wf, bf, out, stats, workspace, B, H, W, C, eps, negative_slope, dtype,
                                                    (hipStream_t)stream);
    if (e == -1) return PPN_E_UNSUPPORTED;
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_gennet_tail_train_bwd(const void* dout, const void* y, const float* gamma, const float* beta, const float* wf, const float* stats,
                              void* workspace, void* dy, float* dgamma, float* dbeta, float* dwf, float* dbf, int B, int H, int W, int C,
                              float negative_slope, int dtype, void* stream) {
    if (!dout || !y || !gamma || !beta || !wf || !stats || !workspace || !dgamma || !dbeta || !dwf) return PPN_E_INVALID;   // dy, dbf may be NULL
    if ((((uintptr_t)dout | (uintptr_t)y | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)wf | (uintptr_t)workspace | (uintptr_t)dy |
          (uintptr_t)dgamma | (uintptr_t)dbeta | (uintptr_t)dwf) & 15) != 0 || (((uintptr_t)dbf | (uintptr_t)stats) & 3) != 0)
        return PPN_E_INVALID;
    if (dtype != 0 && dtype != 1) return PPN_E_INVALID;
    if (!stem_scalar_ok(negative_slope)) return PPN_E_INVALID;
    const int ok = tail_train_sizes(B, H, W, C);
    if (ok != PPN_OK) return ok;
    const int e = ppn::gennet_tail_train_bwd_launch(dout, y, gamma, beta, wf, stats, workspace, dy, dgamma, dbeta, dwf, dbf, B, H, W, C,
                                                    negative_slope, dtype, (hipStream_t)stream);
    if (e == -1) return PPN_E_UNSUPPORTED;
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_gennet_tail_train_tile(void) { return ppn::gennet_tail_tile(); }
int ppn_gennet_tail_train_max_blocks(void) { return ppn::gennet_tail_max_blocks(); }

// what the stride-2 entry points check alike: extents, the width, the big tensor's element count (H, W: the big extent)
static int s2_sizes(int B, int H, int W, int C, int dtype) {
    if (dtype != 0 && dtype != 1) return PPN_E_INVALID;
    if (B < 1 || H < 1 || W < 1 || C < 1) return PPN_E_INVALID;
    if (C != 24) return PPN_E_UNSUPPORTED;
    if ((long long)B * H > 0x7fffffffLL || (long long)B * H * W > 0x7fffffffLL) return PPN_E_INVALID;     // overflow-safe in this order
    if ((long long)B * H * W * C >= 0x80000000LL) return PPN_E_INVALID;       // the big tensor: 2^31 elements or more
    return PPN_OK;
}

int ppn_gennet_s2_tile(void) { return ppn::gennet_s2_tile(); }
int ppn_gennet_s2_max_blocks(void) { return ppn::gennet_s2_max_blocks(); }

int64_t ppn_gennet_s2_wgrad_workspace(int B, int Hs, int Ws) {
    if (B < 1 || Hs < 1 || Ws < 1) return -1;
    if ((long long)B * Hs > 0x7fffffffLL || (long long)B * Hs * Ws > 0x7fffffffLL) return -1;
    if ((long long)B * Hs * Ws * 24 >= 0x80000000LL) return -1;               // the small tensor alone is past what the entry takes
    return ppn::gennet_s2_wgrad_workspace_bytes((long long)B * Hs * Ws);
}

int ppn_gennet_s2_down(const void* big, const float* w, const float* bias, void* small, int B, int H, int W, int C, int dtype, void* stream) {
    if (!big || !w || !small) return PPN_E_INVALID;                           // bias may be NULL: none
    if ((((uintptr_t)big | (uintptr_t)w | (uintptr_t)small) & 15) != 0 || ((uintptr_t)bias & 3) != 0) return PPN_E_INVALID;
    const int ok = s2_sizes(B, H, W, C, dtype);
    if (ok != PPN_OK) return ok;
    const int e = ppn::gennet_s2_down_launch(big, w, bias, small, B, H, W, C, dtype, (hipStream_t)stream);
    if (e == -1) return PPN_E_UNSUPPORTED;
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_gennet_s2_up(const void* small, const float* w, const float* bias, void* big, int B, int H, int W, int C, int dtype, void* stream) {
    if (!small || !w || !big) return PPN_E_INVALID;                           // bias may be NULL: none
    if ((((uintptr_t)small | (uintptr_t)w | (uintptr_t)big) & 15) != 0 || ((uintptr_t)bias & 3) != 0) return PPN_E_INVALID;
    const int ok = s2_sizes(B, H, W, C, dtype);
    if (ok != PPN_OK) return ok;
    const int e = ppn::gennet_s2_up_launch(small, w, bias, big, B, H, W, C, dtype, (hipStream_t)stream);
    if (e == -1) return PPN_E_UNSUPPORTED;
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_gennet_s2_wgrad(const void* small, const void* big, void* workspace, float* dw, float* sum_small, float* sum_big, int B, int H, int W,
                        int C, int dtype, void* stream) {
    if (!small || !big || !workspace || !dw) return PPN_E_INVALID;            // sum_small, sum_big may be NULL: not wanted
    if ((((uintptr_t)small | (uintptr_t)big | (uintptr_t)workspace | (uintptr_t)dw) & 15) != 0 ||
        (((uintptr_t)sum_small | (uintptr_t)sum_big) & 3) != 0)
        return PPN_E_INVALID;
    const int ok = s2_sizes(B, H, W, C, dtype);
    if (ok != PPN_OK) return ok;
    const int e = ppn::gennet_s2_wgrad_launch(small, big, workspace, dw, sum_small, sum_big, B, H, W, C, dtype, (hipStream_t)stream);
    if (e == -1) return PPN_E_UNSUPPORTED;
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_upsample2x_nhwc(const void* x, void* y, int32_t B, int32_t H, int32_t W, int32_t C, int32_t relu, int32_t dtype,
                        void* stream) {
    return ppn_upsample2x_nhwc_bias(x, nullptr, y, B, H, W, C, relu, dtype, stream);
}

int ppn_upsample2x_nhwc_bias(const void* x, const void* bias, void* y, int32_t B, int32_t H, int32_t W, int32_t C, int32_t relu,
                             int32_t dtype, void* stream) {
    if (!x || !y || B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C % 8) != 0 || (dtype != 0 && dtype != 1)) return PPN_E_INVALID;
    const int e = ppn::upsample2x_launch(x, bias, nullptr, y, B, H, W, C, relu, dtype, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_upsample2x_add_nhwc(const void* x, const void* add, void* y, int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype, void* stream) {
    if (!x || !add || !y || B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C % 8) != 0 || (dtype != 0 && dtype != 1)) return PPN_E_INVALID;
    const int e = ppn::upsample2x_launch(x, nullptr, add, y, B, H, W, C, 0, dtype, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_upsample2x_concat_nhwc(const void* const* x, const int32_t* channels, int32_t n, void* out, int32_t B, int32_t H, int32_t W, int32_t dtype,
                               void* stream) {
    if (!x || !channels || !out || n <= 0 || n > 8 || B <= 0 || H <= 0 || W <= 0 || (dtype != 0 && dtype != 1)) return PPN_E_INVALID;
    int ch[8];
    long long total = 0, cmax = 0;
    for (int l = 0; l < n; ++l) {
        if (!x[l] || channels[l] <= 0 || (channels[l] % 8) != 0) return PPN_E_INVALID;
        ch[l] = channels[l];
        total += channels[l];
        cmax = channels[l] > cmax ? channels[l] : cmax;
    }
    // launch geometry (upsample2x_concat_launch): B (H + 1) block rows < 2^31, at most 65535 pieces of 256 threads per block row;
    // 2H, 2W and the channel offsets stay 32-bit
    if (total > 0x7fffffffLL || H >= (1 << 30) || W >= (1 << 30) || (long long)B * (H + 1) >= (1LL << 31) ||
        (((long long)W + 1) * (cmax / 8) + 255) / 256 > 65535)
        return PPN_E_INVALID;
    const int e = ppn::upsample2x_concat_launch(x, ch, n, out, B, H, W, dtype, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_resize_concat4_nhwc(const void* x0, const void* x1, const void* x2, const void* x3, const int32_t* hw, void* out, int32_t B, int32_t C,
                            int32_t dtype, void* stream) {
    if (!x0 || !x1 || !x2 || !x3 || !hw || !out || B <= 0 || C <= 0 || (C % 8) != 0 || (dtype != 0 && dtype != 1)) return PPN_E_INVALID;
    const void* x[4] = {x0, x1, x2, x3};
    const int32_t ch[4] = {C, C, C, C};
    return ppn_resize_concat_nhwc(x, hw, ch, 4, out, B, dtype, stream);
}

int ppn_resize_concat_nhwc(const void* const* x, const int32_t* hw, const int32_t* channels, int32_t n, void* out, int32_t B, int32_t dtype, void* stream) {
    if (!x || !hw || !channels || !out || n <= 0 || n > 8 || B <= 0 || (dtype != 0 && dtype != 1)) return PPN_E_INVALID;
    int h[16], ch[8];
    for (int l = 0; l < n; ++l) {
        if (!x[l] || hw[2 * l] <= 0 || hw[2 * l + 1] <= 0 || channels[l] <= 0 || (channels[l] % 8) != 0) return PPN_E_INVALID;
        h[2 * l] = hw[2 * l]; h[2 * l + 1] = hw[2 * l + 1]; ch[l] = channels[l];
    }
    const int e = ppn::resize_concat_launch(x, h, ch, n, out, B, dtype, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

// The launch limits of the x2 kernels, forward and backward (the backward's grid is the smaller one: it walks 2 x 2 input blocks):
// B (H + 1) block rows < 2^31, at most 65535 pieces of 256 threads per block row; 2H, 2W stay 32-bit.
static bool up2x_grid_ok(int32_t B, int32_t H, int32_t W, long long cmax) {
    return H < (1 << 30) && W < (1 << 30) && (long long)B * (H + 1) < (1LL << 31) && (((long long)W + 1) * (cmax / 8) + 255) / 256 <= 65535;
}

int ppn_upsample2x_nhwc_bwd(const void* dy, const void* x, void* dx, int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype, void* stream) {
    if (!dy || !dx || B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C % 8) != 0 || (dtype != 0 && dtype != 1)) return PPN_E_INVALID;
    if (!up2x_grid_ok(B, H, W, C)) return PPN_E_INVALID;
    const int e = ppn::upsample2x_bwd_launch(dy, x, dx, B, H, W, C, dtype, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_upsample2x_concat_nhwc_bwd(const void* dout, void* const* dx, const int32_t* channels, int32_t n, int32_t B, int32_t H, int32_t W,
                                   int32_t dtype, void* stream) {
    if (!dout || !dx || !channels || n <= 0 || n > 8 || B <= 0 || H <= 0 || W <= 0 || (dtype != 0 && dtype != 1)) return PPN_E_INVALID;
    int ch[8];
    long long total = 0, cmax = 0;
    for (int l = 0; l < n; ++l) {
        if (!dx[l] || channels[l] <= 0 || (channels[l] % 8) != 0) return PPN_E_INVALID;
        ch[l] = channels[l];
        total += channels[l];
        cmax = channels[l] > cmax ? channels[l] : cmax;
    }
    if (total > 0x7fffffffLL || !up2x_grid_ok(B, H, W, cmax)) return PPN_E_INVALID;
    const int e = ppn::upsample2x_concat_bwd_launch(dout, dx, ch, n, B, H, W, dtype, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_resize_concat_nhwc_bwd(const void* dout, void* const* dx, const int32_t* hw, const int32_t* channels, int32_t n, int32_t B, int32_t dtype,
                               void* stream) {
    if (!dout || !dx || !hw || !channels || n <= 0 || n > 8 || B <= 0 || (dtype != 0 && dtype != 1)) return PPN_E_INVALID;
    int h[16], ch[8];
    long long total = 0, cmax = 0;
    for (int l = 0; l < n; ++l) {
        if (!dx[l] || hw[2 * l] <= 0 || hw[2 * l + 1] <= 0 || channels[l] <= 0 || (channels[l] % 8) != 0) return PPN_E_INVALID;
        if (hw[2 * l] > hw[0] || hw[2 * l + 1] > hw[1]) return PPN_E_INVALID;          // no level larger than level 0
        h[2 * l] = hw[2 * l]; h[2 * l + 1] = hw[2 * l + 1]; ch[l] = channels[l];
        total += channels[l];
        cmax = channels[l] > cmax ? channels[l] : cmax;
    }
    // launch geometry (resize_concat_bwd_launch): one thread per 8 channels of an input pixel, fewer than 2^31 blocks of 256 per level
    // (levels are no larger than level 0, so its pixel count bounds them all); the channel offsets stay 32-bit
    if (total > 0x7fffffffLL || (long long)hw[0] * hw[1] >= (1LL << 31) || (long long)B * hw[0] * hw[1] >= (1LL << 31) ||
        ((long long)B * hw[0] * hw[1] * (cmax / 8) + 255) / 256 >= (1LL << 31))
        return PPN_E_INVALID;
    const int e = ppn::resize_concat_bwd_launch(dout, dx, h, ch, n, B, dtype, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_adaptive_pools_nhwc(const void* x, void* const* y, const int32_t* scales, int32_t n, int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype,
                            void* stream) {
    if (!x || !y || !scales || n <= 0 || n > 4 || B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C % 8) != 0 || (dtype != 0 && dtype != 1)) return PPN_E_INVALID;
    int sc[4];
    for (int k = 0; k < n; ++k) { if (!y[k] || scales[k] <= 0) return PPN_E_INVALID; sc[k] = scales[k]; }
    const int e = ppn::adaptive_pools_launch(x, y, sc, n, B, H, W, C, dtype, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_grid_to_image(const uint8_t* grid, void* img, int64_t n_pixels, const float* mean3, const float* std3, int32_t dtype, void* stream) {
    if (!grid || !img || !mean3 || !std3 || n_pixels < 0 || (n_pixels % 8) != 0 || (dtype != 0 && dtype != 1)) return PPN_E_INVALID;
    if (n_pixels == 0) return PPN_OK;
    const int e = ppn::grid_image_launch(grid, img, n_pixels, mean3, std3, dtype, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

// B H W, B Ho Wo and the image's B Ho Wo 3 elements below 2^31, in steps that each stay within 64 bits
static bool augment_args_ok(const void* in, const uint8_t* label_in, const uint32_t* params, const void* img_out, const uint8_t* label_out, int B,
                            int H, int W, int Ho, int Wo, const float* mean3, const float* std3, int dtype) {
    if (!in || !params || !img_out || !mean3 || !std3) return false;
    if ((label_in == nullptr) != (label_out == nullptr)) return false;                                // labels: both or neither
    if (B <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0 || (W % 8) != 0 || (Wo % 8) != 0 || Ho < H || Wo < W) return false;
    if (dtype != 0 && dtype != 1) return false;
    if ((((uintptr_t)in | (uintptr_t)label_in | (uintptr_t)label_out) & 7) != 0) return false;        // eight pixels per load / store
    if ((((uintptr_t)img_out | (uintptr_t)params) & 15) != 0) return false;
    const long long px = (long long)Ho * Wo;
    if (px >= 0x80000000LL || (long long)B * px >= 0x80000000LL || 3 * ((long long)B * px) >= 0x80000000LL) return false;
    // work-items of the launch: whole workgroups per image
    const long long per = ppn::augment_pixels(), groups = (px + per - 1) / per;
    return (long long)B * groups * ppn::augment_threads() < 0x7fffffffLL;
}

int ppn_augment_params(uint64_t seed, uint64_t first_instance, int B, double flip_ratio, double brightness_delta, double contrast_lo,
                       double contrast_hi, double saturation_lo, double saturation_hi, int hue_delta, uint32_t* params, void* stream) {
    if (!params || ((uintptr_t)params & 15) != 0 || B <= 0 || (long long)B * PPN_AUG_PARAM_WORDS >= 0x80000000LL) return PPN_E_INVALID;
    if (!(flip_ratio >= 0.0 && flip_ratio <= 1.0) || !(brightness_delta >= 0.0 && brightness_delta <= 255.0)) return PPN_E_INVALID;
    if (!(contrast_lo >= 0.0 && contrast_hi >= contrast_lo && contrast_hi <= 255.0)) return PPN_E_INVALID;
    if (!(saturation_lo >= 0.0 && saturation_hi >= saturation_lo && saturation_hi <= 255.0)) return PPN_E_INVALID;
    if (hue_delta < 0 || hue_delta > 180) return PPN_E_INVALID;
    const int e = ppn::augment_params_launch(seed, first_instance, B, flip_ratio, brightness_delta, contrast_lo, contrast_hi, saturation_lo,
                                             saturation_hi, hue_delta, params, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_augment_codes(const uint8_t* grid, const uint8_t* label_in, const uint32_t* params, void* img_out, uint8_t* label_out, int B, int H, int W,
                      int Ho, int Wo, const float* mean3, const float* std3, int seg_pad_val, int dtype, void* stream) {
    if (!augment_args_ok(grid, label_in, params, img_out, label_out, B, H, W, Ho, Wo, mean3, std3, dtype)) return PPN_E_INVALID;
    const int e = ppn::augment_launch(0, grid, label_in, params, img_out, label_out, B, H, W, Ho, Wo, mean3, std3, seg_pad_val, dtype,
                                      (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_augment_rgb(const uint8_t* rgb, const uint8_t* label_in, const uint32_t* params, void* img_out, uint8_t* label_out, int B, int H, int W,
                    int Ho, int Wo, const float* mean3, const float* std3, int seg_pad_val, int dtype, void* stream) {
    if (!augment_args_ok(rgb, label_in, params, img_out, label_out, B, H, W, Ho, Wo, mean3, std3, dtype)) return PPN_E_INVALID;
    const int e = ppn::augment_launch(1, rgb, label_in, params, img_out, label_out, B, H, W, Ho, Wo, mean3, std3, seg_pad_val, dtype,
                                      (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_seg_labels_2class(const void* logits, uint8_t* labels, int32_t B, int32_t h, int32_t w, int32_t Ho, int32_t Wo, int32_t dtype,
                          void* stream) {
    if (!logits || !labels || B <= 0 || h <= 0 || w <= 0 || Ho <= 0 || Wo <= 0 || (dtype != 0 && dtype != 1)) return PPN_E_INVALID;
    const int e = ppn::seg_labels_launch(logits, labels, B, h, w, Ho, Wo, dtype, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_bias_act_nhwc(void* x, const void* bias, int64_t n, int32_t C, float negative_slope, int32_t dtype, void* stream) {
    if (!x || !bias || n < 0 || C <= 0 || (C % 8) != 0 || (n % C) != 0 || (dtype != 0 && dtype != 1)) return PPN_E_INVALID;
    if (n == 0) return PPN_OK;
    const int e = ppn::bias_act_launch(x, bias, n, C, negative_slope, dtype, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_conv3x3_c1_nhwc(const void* x, const float* w, const float* bias, void* y, int32_t B, int32_t H, int32_t W, int32_t Cout,
                        float negative_slope, int32_t dtype, void* stream) {
    if (!x || !w || !bias || !y || B <= 0 || H <= 0 || W <= 0 || Cout <= 0 || Cout > 32 || (Cout % 8) != 0 || (dtype != 0 && dtype != 1))
        return PPN_E_INVALID;
    const int e = ppn::conv3x3_c1_launch(x, w, bias, y, B, H, W, Cout, negative_slope, dtype, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_conv3x3_to1_nhwc(const void* x, const float* w, float bias, void* y, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t dtype,
                         void* stream) {
    if (!x || !w || !y || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cin > 32 || (Cin % 8) != 0 || (dtype != 0 && dtype != 1))
        return PPN_E_INVALID;
    const int e = ppn::conv3x3_to1_launch(x, w, bias, y, B, H, W, Cin, dtype, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_conv3x3_mfma_bf16(const void* x, const void* w, const float* bias, void* y, int32_t B, int32_t H, int32_t W, int32_t Cin,
                          int32_t Cout, int32_t stride, int32_t relu, void* stream) {
    if (!x || !w || !bias || !y || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || (Cin % 64) != 0 || Cout <= 0 || (Cout % 8) != 0 ||
        (stride != 1 && stride != 2))
        return PPN_E_INVALID;
    // 32-bit byte offsets inside the kernel: the image and the weights must stay below 4 GiB
    if ((long long)B * H * W * Cin * 2 >= (1LL << 32) || (long long)Cout * 9 * Cin * 2 >= (1LL << 32) || (long long)B * H * W >= (1LL << 31))
        return PPN_E_UNSUPPORTED;
    const int e = ppn::conv3x3_mfma_launch(x, w, bias, y, B, H, W, Cin, Cout, stride, relu, nullptr, nullptr, nullptr, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

// workspace slots: one per 256-column block, none when there is a single block (the kernel then adds straight onto the logits)
int32_t ppn_conv3x3_relu_classify2_slots(int32_t Cout) { return Cout > 0 ? (Cout > 256 ? (Cout + 255) / 256 : 0) : -1; }

int ppn_conv3x3_relu_classify2_bf16(const void* x, const void* w, const float* bias, const float* w2, float* logits, float* partial, int32_t B,
                                    int32_t H, int32_t W, int32_t Cin, int32_t Cout, void* stream) {
    if (!x || !w || !bias || !w2 || !logits || (!partial && Cout > 256) || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || (Cin % 64) != 0 || Cout <= 0 || (Cout % 8) != 0)
        return PPN_E_INVALID;
    if ((long long)B * H * W * Cin * 2 >= (1LL << 32) || (long long)Cout * 9 * Cin * 2 >= (1LL << 32) || (long long)B * H * W >= (1LL << 31))
        return PPN_E_UNSUPPORTED;
    const int e = ppn::conv3x3_mfma_launch(x, w, bias, nullptr, B, H, W, Cin, Cout, 1, 1, w2, logits, partial, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_gennet_conv_s2_bf16(const void* x, const void* w, const float* bias, void* y, int32_t B, int32_t H, int32_t W, float negative_slope,
                            int32_t transposed, void* stream) {
    if (!x || !w || !bias || !y || B <= 0 || H <= 0 || W <= 0 || (!transposed && ((H | W) & 1))) return PPN_E_INVALID;
    if ((long long)B * H * W * 4 >= (1LL << 31)) return PPN_E_UNSUPPORTED;          // 32-bit pixel indices inside
    const int e = transposed ? ppn::gennet_dec_conv_launch(x, w, bias, y, B, H, W, negative_slope, (hipStream_t)stream)
                             : ppn::gennet_enc_conv_launch(x, w, bias, y, B, H, W, negative_slope, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_gennet_first_enc_bf16(const void* x1, const void* w1, const float* b1, const void* wk2, const float* bias2, void* y, int32_t B, int32_t H, int32_t W,
                              float slope1, float slope2, void* stream) {
    if (!x1 || !w1 || !b1 || !wk2 || !bias2 || !y || B <= 0 || H <= 0 || W <= 0 || ((H | W) & 1)) return PPN_E_INVALID;
    const int e = ppn::gennet_first_enc_launch(x1, w1, b1, wk2, bias2, y, B, H, W, slope1, slope2, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_gennet_dec_final_bf16(const void* x, const void* w, const float* bias, float negative_slope, const float* w_final, float bias_final, void* y,
                              int32_t B, int32_t H, int32_t W, void* stream) {
    if (!x || !w || !bias || !w_final || !y || B <= 0 || H <= 0 || W <= 0) return PPN_E_INVALID;
    if ((long long)B * H * W * 4 * 24 >= (1LL << 32)) return PPN_E_UNSUPPORTED;     // 32-bit element offsets inside one image batch
    const int e = ppn::gennet_dec_final_launch(x, w, bias, negative_slope, w_final, bias_final, y, B, H, W, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_gennet_trunk_bf16(const void* x, void* y, const float* params, int32_t B, int32_t N, int32_t n_blocks, void* stream) {
    if (!x || !y || !params || B <= 0 || N <= 0 || N > 1024 || (N % 8) != 0 || n_blocks <= 0) return PPN_E_INVALID;
    const int e = ppn::gennet_trunk_launch(x, y, params, B, N, n_blocks, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_assemble_paths(const double* wp, const int32_t* wp_n, const uint8_t* ok, const double* init, const double* end, double rate, int32_t n,
                       int32_t max_wp, double* full, int32_t* counts, void* stream) {
    if (!wp || !wp_n || !ok || !init || !end || !full || !counts || n <= 0 || max_wp <= 0) return PPN_E_INVALID;
    const int e = ppn::assemble_paths_launch(wp, wp_n, ok, init, end, rate, n, max_wp, full, counts, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_plan_collision(const double* waypoints, const int32_t* counts, const void* obstacles, int32_t obstacles_f64, const int32_t* n_obstacles,
                       int32_t B, int32_t M, int32_t S, float clearance, float bound, uint8_t* collision, void* stream) {
    if (!waypoints || !counts || !n_obstacles || !collision || B <= 0 || M < 2 || S < 0 || (S > 0 && !obstacles)) return PPN_E_INVALID;
    const int e = ppn::plan_collision_launch(waypoints, counts, obstacles, obstacles_f64, n_obstacles, B, M, S, clearance, bound, collision,
                                             (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_heatmap_u8(const void* y, uint8_t* out, int32_t B, int32_t n, int32_t dtype, void* stream) {
    if (!y || !out || B <= 0 || n <= 0 || (dtype != 0 && dtype != 1)) return PPN_E_INVALID;
    const int e = ppn::heatmap_u8_launch(y, out, B, n, dtype, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_tokenizer_conv1_codes_bf16(const uint8_t* grid, const void* lut, void* out, int32_t B, int32_t H, int32_t W, void* stream) {
    if (!grid || !lut || !out || B <= 0 || H <= 0 || W <= 0) return PPN_E_INVALID;
    if ((H & 1) || (W % 32)) return PPN_E_UNSUPPORTED;
    const int e = ppn::tokenizer_codes_launch(grid, lut, out, B, H, W, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_tokenizer_codes_bf16(const uint8_t* grid, const void* lut, const void* w2p, const float* vec, void* tokens, int32_t B, int32_t H, int32_t W,
                             float eps, void* stream) {
    if (!grid || !lut || !w2p || !vec || !tokens || B <= 0 || H <= 0 || W <= 0) return PPN_E_INVALID;
    if ((H % 4) || (W % 64)) return PPN_E_UNSUPPORTED;
    const int e = ppn::tokenizer_fused_launch(grid, lut, w2p, vec, tokens, B, H, W, eps, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_nat128_ln_qkv_bf16(const void* s, const float* offset, const void* ln_w, const void* ln_b, const void* w, const void* bias, void* qkv,
                           int64_t tokens, float eps, void* stream) {
    if (!s || !ln_w || !ln_b || !w || !qkv || tokens <= 0) return PPN_E_INVALID;
    if (tokens % 16) return PPN_E_UNSUPPORTED;
    const int e = ppn::nat128_ln_qkv_launch(s, offset, ln_w, ln_b, w, bias, qkv, tokens, eps, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_nat128_ln_mlp_add_bf16(void* s, const float* offset, const void* ln_w, const void* ln_b, const void* w1, const void* b1, const void* w2,
                               const float* final_add, int64_t tokens, float eps, void* stream) {
    if (!s || !ln_w || !ln_b || !w1 || !b1 || !w2 || tokens <= 0) return PPN_E_INVALID;
    if (tokens % 16) return PPN_E_UNSUPPORTED;
    const int e = ppn::nat128_ln_mlp_launch(s, offset, ln_w, ln_b, w1, b1, w2, final_add, tokens, eps, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_nat128_ln_mlp_bf16(void* s, const float* offset, const void* ln_w, const void* ln_b, const void* w1, const void* b1, const void* w2,
                           int64_t tokens, float eps, void* stream) {
    return ppn_nat128_ln_mlp_add_bf16(s, offset, ln_w, ln_b, w1, b1, w2, nullptr, tokens, eps, stream);
}

int ppn_nat128_proj_add_bf16(void* s, const void* a, const void* w, int64_t tokens, void* stream) {
    if (!s || !a || !w || tokens <= 0 || (tokens % 16) != 0) return PPN_E_INVALID;
    const int e = ppn::nat128_proj_add_launch(s, a, w, tokens, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_gemm_bf16(const void* a, const void* w, const float* bias, void* c, int64_t M, int32_t N, int32_t K, int32_t epilogue,
                  int32_t persistent_blocks, void* stream) {
    if (!a || !w || !c || M <= 0 || M >= (1LL << 31) || N <= 0 || (N % 8) != 0 || K < 128 || (K % 64) != 0 || epilogue < 0 || epilogue > 3 ||
        (epilogue != 2 && !bias) || persistent_blocks < 0 || (persistent_blocks % 8) != 0)
        return PPN_E_INVALID;
    if (M * K * 2 >= (1LL << 32) || (long long)N * K * 2 >= (1LL << 32)) return PPN_E_UNSUPPORTED;
    // few rows (small batches): the wave-per-block kernel of gemm_small.hip instead of a handful of 256 x 256 tiles
    static const bool no_small = getenv("PPNET_NO_SMALL_GEMM") != nullptr;       // A/B
    const int e = (!no_small && ppn::gemm_small_wanted(M, N, K))
                      ? ppn::gemm_small_launch(a, w, bias, c, M, N, K, epilogue, (hipStream_t)stream)
                      : ppn::gemm_mfma_launch(a, w, bias, c, M, N, K, epilogue, persistent_blocks, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_nat_gemm_bf16(const void* a, const void* w, const float* bias, const float* colsum, const float* stats_in, int32_t partials_in,
                      float* stats_out, void* c, int64_t M, int32_t N, int32_t K, int32_t mode, float eps, void* stream) {
    if (!a || !w || !c || !bias || M <= 0 || M >= (1LL << 31) || (M % 256) != 0 || N <= 0 || (N % 256) != 0 || K < 128 || (K % 64) != 0 ||
        mode < 0 || mode > 2)
        return PPN_E_INVALID;
    if (mode != 2 && (!colsum || !stats_in || partials_in < 1 || partials_in > 4 || K / 64 < 3)) return PPN_E_INVALID;
    if (mode == 2 && !stats_out) return PPN_E_INVALID;
    if (M * K * 2 >= (1LL << 32) || (long long)N * K * 2 >= (1LL << 32)) return PPN_E_UNSUPPORTED;     // the core's 32-bit operand offsets
    // the 256 x 256 core of mfma_gemm.h: mode 2 reads the old c in its epilogue, modes 0 / 1 fold the LayerNorm into theirs
    const int n_cu = ppn::device_cu_count();
    if (!n_cu) return hip_fail(hipErrorInvalidDevice);
    const int e = mode == 2 ? ppn::gemm_acc_stats_launch(a, w, bias, stats_out, c, M, N, K, n_cu, (hipStream_t)stream)
                            : ppn::gemm_ln_launch(a, w, bias, colsum, stats_in, partials_in, c, M, N, K, mode == 1, eps, n_cu, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int32_t ppn_nat_gemm_partials(int32_t C) {
    if (C <= 0 || (C % 256) != 0) return -1;
    return ppn::nat_stats_p128(C) ? C / 128 : C / 256;
}

int32_t ppn_nat_mlp_supported(int64_t M, int32_t C, int32_t HID) { return ppn::nat_mlp_supported(M, C, HID) ? 1 : 0; }

int ppn_nat_mlp_pack_bf16(const void* w1, const void* w2, void* wpk, int32_t C, int32_t HID, void* stream) {
    if (!w1 || !w2 || !wpk || HID <= 0 || (HID % 32) != 0) return PPN_E_INVALID;
    const int e = ppn::nat_mlp_pack_launch(w1, w2, wpk, C, HID, (hipStream_t)stream);
    if (e == -1) return PPN_E_UNSUPPORTED;
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_nat_mlp_bf16(void* s, const void* wpk, const float* hb, const float* b2, float* stats_out, int64_t M, int32_t C, int32_t HID,
                     float eps, void* stream) {
    if (!s || !wpk || !hb || !b2 || M <= 0 || M >= (1LL << 31)) return PPN_E_INVALID;
    if (!ppn::nat_mlp_supported(M, C, HID)) return PPN_E_UNSUPPORTED;
    const int e = ppn::nat_mlp_launch(s, wpk, hb, b2, stats_out, M, C, HID, eps, (hipStream_t)stream);
    if (e == -1) return PPN_E_UNSUPPORTED;
    if (e == -2) return hip_fail(hipErrorInvalidDevice);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_row_stats_bf16(const void* x, int64_t rows, int32_t C, float* stats, void* stream) {
    if (!x || !stats || rows < 0 || C < 64 || C > 1024 || (C % 8) != 0) return PPN_E_INVALID;
    if (rows == 0) return PPN_OK;
    const int e = ppn::row_stats_launch(x, rows, C, stats, (hipStream_t)stream);
    if (e != 0) return hip_fail((hipError_t)e);
    return PPN_OK;
}

int ppn_resize_bilinear_u8(const uint8_t* in, int32_t n, int32_t H, int32_t W, int32_t outH, int32_t outW, uint8_t* tmp,
                           uint8_t* out, void* stream) {
    if (!in || n < 0 || H <= 0 || W <= 0 || outH <= 0 || outW <= 0 || !tmp || !out) return PPN_E_INVALID;
    if (n == 0) return PPN_OK;
    // a thread computes its output coordinate's filter weights once and walks PPN_RESIZE_REP lines (pass 1) / images (pass 2)
    const long long g1 = ((long long)n * H + ppn::PPN_RESIZE_REP - 1) / ppn::PPN_RESIZE_REP;
    const long long g2 = (((long long)n + ppn::PPN_RESIZE_REP - 1) / ppn::PPN_RESIZE_REP) * outH;
    if (g1 >= (1LL << 31) || g2 >= (1LL << 31) || (outW + 255) / 256 > 65535) return PPN_E_UNSUPPORTED;
    hipLaunchKernelGGL(ppn::resize_pass_kernel, dim3((unsigned)g1, (unsigned)((outW + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in, n, H, W,
                       H, outW, 1, tmp);
    hipLaunchKernelGGL(ppn::resize_pass_kernel, dim3((unsigned)g2, (unsigned)((outW + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const uint8_t*)tmp, n, H, outW, outH, outW, 0, out);
    PPN_HIP(hipGetLastError());
    return PPN_OK;
}

int ppn_philox_doubles(uint64_t seed, uint32_t stream_id, uint64_t instance, uint32_t first, int32_t count, double* out,
                       void* stream) {
    if (count < 0 || !out) return PPN_E_INVALID;
    if (count == 0) return PPN_OK;
    hipLaunchKernelGGL(ppn::philox_doubles_kernel, dim3((count + 255) / 256), dim3(256), 0, (hipStream_t)stream, seed,
                       stream_id, instance, first, count, out);
    PPN_HIP(hipGetLastError());
    return PPN_OK;
}

}  // extern "C"
