// Image-pair inlier scoring (include/insfm_pairs.h): ImagePairInliersCount on the GPU.
//
//   1. k_check_pairs / k_check_matches -- pair_ptr, the kinds and every feature number are validated on the device
//      before anything is written (the scoring kernel gathers through them); one flag word comes back to the host.
//   2. k_pair_inliers -- one wave per pair, walking its matches 64 at a time.  Each lane gathers its two features,
//      widens them to float64 and evaluates the match; a 64-bit __ballot and a popcount of the lanes below give the
//      ordered compaction into inlier_idx; the score is a per-lane sum over the walk, reduced across the wave in a
//      fixed order at the end (no atomics: the bytes are the same from run to run).  The fundamental kind walks twice:
//      the first walk counts the orientation votes of the pre-inliers, the second recomputes each match and selects
//      the majority side, so nothing is stashed in the output and a tied pair writes no index at all.
// The per-pair constants (32 doubles) are read at a wave-uniform address; no LDS, no scratch buffers besides the flag
// word, which a StageTemps (stage_device.h) owns.  The word is read back into a local, not a pinned block: the call
// takes 0.5 ms, and allocating and freeing pinned memory would add 0.2 ms to it.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/insfm_ba.h"
#include "../../include/insfm_pairs.h"
#include "../../include/insfm_tracks.h"
#include "stage_device.h"

namespace {

using namespace insfm;

constexpr int kWaves = kT / 64;
constexpr int kG = INSFM_PAIR_GEOM_STRIDE;
constexpr double kEps = 1e-10;  // EPSILON of two_view_geometry.py:4
constexpr int kBadPtr = 1, kBadKind = 2, kBadMatch = 4, kHasEssential = 8;

__global__ __launch_bounds__(kT) void k_check_pairs(int64_t np, int64_t nm, const int64_t* __restrict__ ptr,
                                                    const int32_t* __restrict__ kind, int* __restrict__ flags) {
    const int64_t p = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (p >= np) return;
    const int64_t a = ptr[p], b = ptr[p + 1];
    int f = 0;
    if (a < 0 || b < a || b > nm) f |= kBadPtr;
    const int k = kind[p];
    if (k < INSFM_PAIR_SKIP || k > INSFM_PAIR_ESSENTIAL) f |= kBadKind;
    if (k == INSFM_PAIR_ESSENTIAL) f |= kHasEssential;
    if (f) atomicOr(flags, f);
}

__global__ __launch_bounds__(kT) void k_check_matches(int64_t nm, int64_t nf, const int32_t* __restrict__ ma,
                                                      const int32_t* __restrict__ mb, int* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (i >= nm) return;
    const int64_t a = ma[i], b = mb[i];
    if (a < 0 || a >= nf || b < 0 || b >= nf) atomicOr(flags, kBadMatch);
}

struct V3 {
    double x, y, z;
};

__device__ inline double dot(const V3& a, const V3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
// rows / columns of a row-major 3x3 at g
__device__ inline V3 row(const double* g, int i) { return {g[3 * i], g[3 * i + 1], g[3 * i + 2]}; }
__device__ inline V3 col(const double* g, int j) { return {g[j], g[3 + j], g[6 + j]}; }

__device__ inline V3 pixel(const void* xy, int f32, int64_t i) {
    V3 p = {0.0, 0.0, 1.0};
    load_xy(xy, f32, i, p.x, p.y);
    return p;
}

__device__ inline V3 ray(const void* rays, int f32, int64_t i) {
    if (f32) {
        const float* p = static_cast<const float*>(rays) + 3 * i;
        return {(double)p[0], (double)p[1], (double)p[2]};
    }
    const double* p = static_cast<const double*>(rays) + 3 * i;
    return {p[0], p[1], p[2]};
}

// two_view_geometry.py:24-34
__device__ inline double sampson(const double* E, const V3& x1, const V3& x2) {
    const double d1 = x1.z + kEps, d2 = x2.z + kEps;
    const V3 Ex1 = {dot(row(E, 0), x1) / d1, dot(row(E, 1), x1) / d1, dot(row(E, 2), x1) / d1};
    const double Etx2_0 = dot(col(E, 0), x2) / d2, Etx2_1 = dot(col(E, 1), x2) / d2;
    const double C = dot(x2, Ex1);
    const double Cx = Ex1.x * Ex1.x + Ex1.y * Ex1.y;
    const double Cy = Etx2_0 * Etx2_0 + Etx2_1 * Etx2_1;
    return C * C / (Cx + Cy);
}

// two_view_geometry.py:54-57
__device__ inline double homography(const double* H, const V3& x1, const V3& x2) {
    const double d = dot(row(H, 2), x1) + kEps;
    const double u = dot(row(H, 0), x1) / d - x2.x, v = dot(row(H, 1), x1) / d - x2.y;
    return u * u + v * v;
}

// two_view_geometry.py:49-52
__device__ inline double orientation(const double* F, const double* epipole, const V3& x1, const V3& x2) {
    const double s1 = F[0] * x2.x + F[3] * x2.y + F[6];
    const double s2 = epipole[1] - epipole[2] * x1.y;
    return s1 * s2;
}

// The three checks of score_error_essential (:96-110) after r2 < thr^2, in the reference's order and senses.
__device__ inline bool essential_checks(const double* g, const V3& x1, const V3& x2) {
    const double* R = g + 16;
    const V3 t = {g[25], g[26], g[27]};
    const V3 Rx1 = {dot(row(R, 0), x1), dot(row(R, 1), x1), dot(row(R, 2), x1)};
    const V3 nRx1 = {-Rx1.x, -Rx1.y, -Rx1.z};
    const double a = dot(nRx1, x2), b1 = dot(nRx1, t), b2 = dot(t, x2);  // check_cheirality (:36-47)
    const double l1 = b1 - a * b2, l2 = -a * b1 + b2;
    const double lo = g[30] * (1 - a * a), hi = g[31] * (1 - a * a);
    if (!(l1 > lo && l2 > lo && l1 < hi && l2 < hi)) return false;
    const V3 Rtx2 = {dot(col(R, 0), x2), dot(col(R, 1), x2), dot(col(R, 2), x2)};  // inv(R) x2
    if (dot(x1, Rtx2) > g[29]) return false;
    const V3 e12 = {g[10], g[11], g[12]}, e21 = {g[13], g[14], g[15]};
    if (dot(x1, e21) > g[28] || dot(x2, e12) > g[28]) return false;
    return true;
}

__device__ inline double wave_sum(double s) {
    for (int o = 32; o; o >>= 1) s += __shfl_down(s, o, 64);
    return s;
}

__global__ __launch_bounds__(kT) void k_pair_inliers(int64_t np, const int64_t* __restrict__ ptr,
                                                     const int32_t* __restrict__ ma, const int32_t* __restrict__ mb,
                                                     const void* __restrict__ xy, int xy_f32,
                                                     const void* __restrict__ rays, int rays_f32,
                                                     const int32_t* __restrict__ kind, const double* __restrict__ geom,
                                                     int32_t* __restrict__ idx, int32_t* __restrict__ count,
                                                     double* __restrict__ score, int32_t* __restrict__ touched) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * kWaves + wave;
    if (p >= np) return;  // (the whole wave leaves together)
    const int k = kind[p];
    const int64_t begin = ptr[p];
    const int n = (int)(ptr[p + 1] - begin);
    const double* g = geom + p * kG;
    const double thr2 = g[9];
    const unsigned long long below = (1ull << lane) - 1;
    double s = 0.0;
    int cnt = 0, wrote = 1;

    if (k == INSFM_PAIR_SKIP) {
        wrote = 0;
    } else if (k == INSFM_PAIR_FUNDAMENTAL) {
        int pre_n = 0, pos_n = 0;
        for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            bool pre = false, pos = false;
            if (i < n) {
                const V3 x1 = pixel(xy, xy_f32, ma[begin + i]), x2 = pixel(xy, xy_f32, mb[begin + i]);
                pre = sampson(g, x1, x2) < thr2;
                pos = pre && orientation(g, g + 10, x1, x2) > 0;
            }
            pre_n += __popcll(__ballot(pre));
            pos_n += __popcll(__ballot(pos));
        }
        const int neg_n = pre_n - pos_n;
        if (pos_n == neg_n) {
            wrote = 0;
        } else {
            const bool want = pos_n > neg_n;
            for (int base = 0; base < n; base += 64) {
                const int i = base + lane;
                bool ok = false;
                if (i < n) {
                    const V3 x1 = pixel(xy, xy_f32, ma[begin + i]), x2 = pixel(xy, xy_f32, mb[begin + i]);
                    const double r2 = sampson(g, x1, x2);
                    if (r2 < thr2) {
                        ok = (orientation(g, g + 10, x1, x2) > 0) == want;
                        s += ok ? r2 : thr2;
                    }
                }
                const unsigned long long m = __ballot(ok);
                if (ok) idx[begin + cnt + __popcll(m & below)] = i;
                cnt += __popcll(m);
            }
        }
    } else {
        const bool ess = k == INSFM_PAIR_ESSENTIAL;
        for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            bool ok = false;
            if (i < n) {
                double r2;
                if (ess) {
                    const V3 x1 = ray(rays, rays_f32, ma[begin + i]), x2 = ray(rays, rays_f32, mb[begin + i]);
                    r2 = sampson(g, x1, x2);
                    ok = r2 < thr2 && essential_checks(g, x1, x2);
                } else {
                    r2 = homography(g, pixel(xy, xy_f32, ma[begin + i]), pixel(xy, xy_f32, mb[begin + i]));
                    ok = r2 < thr2;
                }
                s += ok ? r2 : thr2;
            }
            const unsigned long long m = __ballot(ok);
            if (ok) idx[begin + cnt + __popcll(m & below)] = i;
            cnt += __popcll(m);
        }
    }
    s = wave_sum(s);
    if (lane == 0) {
        count[p] = cnt;
        score[p] = wrote ? s : 0.0;
        touched[p] = wrote;
    }
}

}  // namespace

extern "C" int insfm_pair_inliers(int64_t n_pairs, const int64_t* pair_ptr, int64_t n_matches, const int32_t* match_a,
                                  const int32_t* match_b, int64_t n_features, const void* xy, int32_t xy_f32,
                                  const void* rays, int32_t rays_f32, const int32_t* pair_kind, const double* pair_geom,
                                  int32_t* inlier_idx, int32_t* inlier_count, double* score, int32_t* touched,
                                  void* stream) {
    constexpr int64_t kMax = (int64_t)1 << 31;
    if (n_pairs < 0 || n_pairs >= kMax || n_matches < 0 || n_matches >= kMax || n_features < 0 || n_features >= kMax)
        return INSFM_BA_EINVAL;
    if (n_pairs == 0) return INSFM_BA_OK;
    if (!pair_ptr || !pair_kind || !pair_geom || !inlier_count || !score || !touched) return INSFM_BA_EINVAL;
    if (n_matches > 0 && (!match_a || !match_b || !xy || !inlier_idx || n_features == 0)) return INSFM_BA_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int host_flags = 0;
    StageTemps w(s, /*pinned=*/false);
    int* flags = w.get<int>(1);
    if (!w.ok()) return INSFM_BA_ENOMEM;
    INSFM_HIP(hipMemsetAsync(flags, 0, sizeof(int), s));
    launch(k_check_pairs, n_pairs, s, n_pairs, n_matches, pair_ptr, pair_kind, flags);
    launch(k_check_matches, n_matches, s, n_matches, n_features, match_a, match_b, flags);
    INSFM_HIP(hipMemcpyAsync(&host_flags, flags, sizeof(int), hipMemcpyDeviceToHost, s));
    INSFM_HIP(settle(s));
    if (host_flags & (kBadPtr | kBadKind | kBadMatch)) return INSFM_BA_EINVAL;
    if ((host_flags & kHasEssential) && !rays) return INSFM_BA_EINVAL;
    launch<kWaves>(k_pair_inliers, n_pairs, s, n_pairs, pair_ptr, match_a, match_b, xy, xy_f32, rays, rays_f32, pair_kind,
                   pair_geom, inlier_idx, inlier_count, score, touched);
    INSFM_HIP(settle(s));
    return INSFM_BA_OK;
}
