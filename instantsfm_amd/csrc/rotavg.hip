// Rotation averaging (include/insfm_rotavg.h): RotationEstimator's L1 / IRLS solve and FilterRotations' angles.
//
// The reference's A is B (x) I3 (B: signed incidence of the pairs plus one gauge row), so every solve is the n x n
// system M = B^T W B with three right-hand sides.  One call
//   1. prepare()    -- validates the pairs on the device (k_check_pairs, a sort of the pairs' {a, b} keys and
//      k_dup for repeated pairs) and builds the per-image CSR of incident pairs: the 2 P (image, entry) pairs, entry
//      e = 2 k + side, stably sorted by image, so a row lists its pairs in pair order; one flag word comes back;
//   2. k_system     -- one workgroup per row of M: clears it, writes -w_k at the partners, thread 0 sums the diagonal
//      in pair order; the rows past n are the identity padding ba_gj.h wants, d = 1 / sqrt(diag) its equilibration;
//   3. launch_gj_unit (ba_gj.h) -- the explicit inverse by blocked f64-MFMA Gauss-Jordan;
//   4. per ADMM iteration k_gather (A^T v per image, through the CSR), k_matvec (one wave per row of M^-1),
//      k_admm_rows (shrinkage, dual update, four partial norms), k_gather_norms (the two dual norms), k_finish (the
//      partials summed in block order) and one 48-byte copy; the host applies the reference's stopping tests;
//   5. per IRLS iteration k_weights, 2, 3, k_gather with the weights, k_matvec, k_update, k_residuals, k_step_stats
//      and one 64-byte copy.
// No floating-point atomics anywhere: every sum has one owner and a fixed order.  The elementwise kernels are plain
// one-thread-per-item C++; the rotation maps are documented in the header.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <utility>

#include "../../include/insfm_ba.h"
#include "../../include/insfm_rotavg.h"
#include "../../include/insfm_tracks.h"
#include "ba_common.h"
#include "stage_device.h"

namespace {

using namespace ::insfm;

// ba_gj.h defines its kernels with external linkage, and ba_kernels.hip, a source of the same library, includes it too.
// Its text is therefore included inside this file's unnamed namespace: everything it needs (the HIP runtime,
// <utility>, ba_common.h) is included above, so only its own definitions land here, as (unnamed)::insfm::k_gj_step and
// so on -- copies private to this translation unit, with the BA's translation unit and the header left as they are.
#include "ba_gj.h"
using namespace insfm;  // (the unnamed namespace's insfm: kGB, gj_steps, launch_gj_unit)

constexpr int kBadIndex = 1, kBadSelf = 2, kBadDup = 4;
constexpr double kSmallAngle = 1e-3;  // scipy's series threshold
constexpr double kRad2Deg = 57.295779513082320876798154814105;

// ---------------------------------------------------------------------------------------------------------------------
// rotation maps
// ---------------------------------------------------------------------------------------------------------------------
struct Quat {
    double x, y, z, w;
};

__device__ inline Quat qmul(const Quat& a, const Quat& b) {  // Hamilton product: R(a b) = R(a) R(b)
    return {a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x,
            a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}

__device__ inline Quat qconj(const Quat& a) { return {-a.x, -a.y, -a.z, a.w}; }

__device__ inline Quat q_exp(double vx, double vy, double vz) {
    const double a2 = vx * vx + vy * vy + vz * vz, a = sqrt(a2);
    const double s = a <= kSmallAngle ? 0.5 - a2 / 48.0 + a2 * a2 / 3840.0 : sin(0.5 * a) / a;
    return {s * vx, s * vy, s * vz, cos(0.5 * a)};
}

__device__ inline Quat q_exp(const double* v) { return q_exp(v[0], v[1], v[2]); }

__device__ inline void q_log(Quat q, double sign, double* out) {  // out = sign * Log(q)
    if (q.w < 0.0) q = {-q.x, -q.y, -q.z, -q.w};
    const double nv = sqrt(q.x * q.x + q.y * q.y + q.z * q.z);
    const double a = 2.0 * atan2(nv, q.w);
    const double a2 = a * a;
    const double s = sign * (a <= kSmallAngle ? 2.0 + a2 / 12.0 + 7.0 * a2 * a2 / 2880.0 : a / nv);
    out[0] = s * q.x;
    out[1] = s * q.y;
    out[2] = s * q.z;
}

__device__ inline Quat load_quat(const double* q) {  // normalised, as Rotation.from_quat does
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double inv = 1.0 / sqrt(x * x + y * y + z * z + w * w);
    return {x * inv, y * inv, z * inv, w * inv};
}

// ---------------------------------------------------------------------------------------------------------------------
// validation and the per-image CSR
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void k_check_pairs(int64_t P, int64_t n, const int32_t* __restrict__ pi,
                                                    const int32_t* __restrict__ pj, int64_t* __restrict__ key,
                                                    int32_t* __restrict__ ent_img, int32_t* __restrict__ ent_id,
                                                    int* __restrict__ flags) {
    const int64_t k = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (k >= P) return;
    int64_t a = pi[k], b = pj[k];
    int f = 0;
    if (a < 0 || a >= n || b < 0 || b >= n) {
        f = kBadIndex;
        a = b = 0;  // (keeps everything derived from them in range; the call is refused anyway)
    } else if (a == b) {
        f = kBadSelf;
    }
    key[k] = (a < b ? a : b) * n + (a < b ? b : a);
    ent_img[2 * k] = (int32_t)a;
    ent_img[2 * k + 1] = (int32_t)b;
    ent_id[2 * k] = (int32_t)(2 * k);
    ent_id[2 * k + 1] = (int32_t)(2 * k + 1);
    if (f) atomicOr(flags, f);
}

__global__ __launch_bounds__(kT) void k_dup(int64_t P, const int64_t* __restrict__ sorted, int* __restrict__ flags) {
    const int64_t k = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (k + 1 >= P) return;
    if (sorted[k] == sorted[k + 1]) atomicOr(flags, kBadDup);
}

// row_ptr[a] = first entry whose image is >= a (a = 0 .. n), over the E sorted images
__global__ __launch_bounds__(kT) void k_row_ptr(int64_t n, int64_t E, const int32_t* __restrict__ img,
                                                int32_t* __restrict__ row_ptr) {
    const int64_t a = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (a > n) return;
    int64_t lo = 0, hi = E;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (img[mid] < a) lo = mid + 1; else hi = mid;
    }
    row_ptr[a] = (int32_t)lo;
}

struct Graph {
    int64_t n = 0, P = 0;
    const int32_t *pi = nullptr, *pj = nullptr;
    int32_t* row_ptr = nullptr;  // [n + 1]
    int32_t* ent = nullptr;      // [2 P] entries 2 k + side, grouped by image, ascending inside a row
    int64_t fixed = 0;
};

bool sizes_ok(int64_t n, int64_t P) {
    return n >= 0 && P >= 0 && n <= INSFM_ROTAVG_MAX_IMAGES && P < ((int64_t)1 << 30) && !(n == 0 && P > 0);
}

// Validates the pairs and builds g.row_ptr / g.ent (scratch of w).  n >= 1.
int prepare(StageTemps& w, int64_t n, int64_t P, const int32_t* pi, const int32_t* pj, int64_t fixed, Graph& g) {
    hipStream_t s = w.stream();
    g.n = n;
    g.P = P;
    g.pi = pi;
    g.pj = pj;
    g.fixed = fixed;
    g.row_ptr = w.get<int32_t>(n + 1);
    g.ent = w.get<int32_t>(2 * P);
    int32_t* img_sorted = w.get<int32_t>(2 * P);
    if (P > 0) {
        const int nE = (int)(2 * P);
        int64_t *key = w.get<int64_t>(P), *key_sorted = w.get<int64_t>(P);
        int32_t *ent_img = w.get<int32_t>(2 * P), *ent_id = w.get<int32_t>(2 * P);
        int* flags = w.get<int>(1);
        TempBytes tb;
        INSFM_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, tb.next(), key, key_sorted, (int)P, 0, bits_for(n * n), s));
        INSFM_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb.next(), ent_img, img_sorted, ent_id, g.ent, nE, 0,
                                                     bits_for(n), s));
        size_t bytes = tb.bytes();
        void* tmp = w.get<char>(bytes);
        if (!w.ok()) return INSFM_BA_ENOMEM;
        INSFM_HIP(hipMemsetAsync(flags, 0, sizeof(int), s));
        launch(k_check_pairs, P, s, P, n, pi, pj, key, ent_img, ent_id, flags);
        INSFM_HIP(hipcub::DeviceRadixSort::SortKeys(tmp, bytes, key, key_sorted, (int)P, 0, bits_for(n * n), s));
        launch(k_dup, P, s, P, key_sorted, flags);
        INSFM_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, ent_img, img_sorted, ent_id, g.ent, nE, 0, bits_for(n),
                                                     s));
        int host_flags = 0;
        INSFM_HIP(hipMemcpyAsync(&host_flags, flags, sizeof(int), hipMemcpyDeviceToHost, s));
        INSFM_HIP(settle(s));
        if (host_flags) return INSFM_BA_EINVAL;
    }
    if (!w.ok()) return INSFM_BA_ENOMEM;
    launch(k_row_ptr, n + 1, s, n, 2 * P, img_sorted, g.row_ptr);
    return INSFM_BA_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// residuals, update, pair errors
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void k_residuals(int64_t P, const int32_t* __restrict__ pi,
                                                  const int32_t* __restrict__ pj, const double* __restrict__ quat,
                                                  const double* __restrict__ rot, int64_t fixed,
                                                  const double* __restrict__ fixed_rot, double* __restrict__ res) {
    const int64_t k = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (k > P) return;
    if (k == P) {  // the gauge row: Log(R_fixed^T R_f)
        q_log(qmul(qconj(q_exp(fixed_rot)), q_exp(rot + 3 * fixed)), 1.0, res + 3 * P);
        return;
    }
    const Quat q1 = q_exp(rot + 3 * (int64_t)pi[k]), q2 = q_exp(rot + 3 * (int64_t)pj[k]);
    q_log(qmul(qconj(q2), qmul(load_quat(quat + 4 * k), q1)), -1.0, res + 3 * k);
}

__global__ __launch_bounds__(kT) void k_update(int64_t n, double* __restrict__ rot, const double* __restrict__ step) {
    const int64_t a = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (a >= n) return;
    const double* st = step + 3 * a;
    q_log(qmul(q_exp(rot + 3 * a), q_exp(-st[0], -st[1], -st[2])), 1.0, rot + 3 * a);
}

__global__ __launch_bounds__(kT) void k_pair_errors(int64_t P, const int32_t* __restrict__ pi,
                                                    const int32_t* __restrict__ pj, const double* __restrict__ quat,
                                                    const double* __restrict__ Rw, double* __restrict__ angle) {
    const int64_t k = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (k >= P) return;
    const double *R1 = Rw + 9 * (int64_t)pi[k], *R2 = Rw + 9 * (int64_t)pj[k];
    const Quat q = load_quat(quat + 4 * k);
    const double x = q.x, y = q.y, z = q.z, w = q.w;
    const double Rr[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w),     2 * (x * z + y * w),
                          2 * (x * y + z * w),     1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                          2 * (x * z - y * w),     2 * (y * z + x * w),     1 - 2 * (x * x + y * y)};
    // trace((R2 R1^T)^T Rr) = sum_ab (R2 R1^T)_ab Rr_ab
    double tr = 0.0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            const double m = R2[3 * a] * R1[3 * b] + R2[3 * a + 1] * R1[3 * b + 1] + R2[3 * a + 2] * R1[3 * b + 2];
            tr += m * Rr[3 * a + b];
        }
    double c = (tr - 1.0) / 2.0;
    c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);  // (a NaN stays a NaN, like np.clip)
    angle[k] = acos(c) * kRad2Deg;
}

// ---------------------------------------------------------------------------------------------------------------------
// the system
// ---------------------------------------------------------------------------------------------------------------------
// Row blockIdx.x of M (row stride ld, `rows` rows; rows and columns past n are the identity).  wt null: unit weights.
// d (optional, [rows]): 1 / sqrt(M_aa), 1 where the diagonal is not positive (the inversion then reports the pivot).
__global__ __launch_bounds__(kT) void k_system(int64_t n, int64_t ld, const int32_t* __restrict__ row_ptr,
                                               const int32_t* __restrict__ ent, const int32_t* __restrict__ pi,
                                               const int32_t* __restrict__ pj, const double* __restrict__ wt,
                                               int64_t fixed, double* __restrict__ M, double* __restrict__ d) {
    const int64_t a = blockIdx.x;
    double* row = M + a * ld;
    for (int64_t c = threadIdx.x; c < ld; c += kT) row[c] = 0.0;
    __syncthreads();
    if (a >= n) {
        if (threadIdx.x == 0) {
            row[a] = 1.0;
            if (d) d[a] = 1.0;
        }
        return;
    }
    const int begin = row_ptr[a], end = row_ptr[a + 1];
    for (int e = begin + threadIdx.x; e < end; e += kT) {  // (the pairs are unique: one writer per entry)
        const int id = ent[e], k = id >> 1;
        row[(id & 1) ? pi[k] : pj[k]] = -(wt ? wt[k] : 1.0);
    }
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int e = begin; e < end; ++e) s += wt ? wt[ent[e] >> 1] : 1.0;
        if (a == fixed) s += 1.0;
        row[a] = s;
        if (d) d[a] = s > 0.0 ? 1.0 / sqrt(s) : 1.0;
    }
}

// Geman-McClure weights (rotation_averaging.py:135-148); counts the NaN weights.
__global__ __launch_bounds__(kT) void k_weights(int64_t P, const double* __restrict__ res, double sigma2,
                                                double* __restrict__ wt, int* __restrict__ nan_count) {
    const int64_t k = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (k >= P) return;
    const double* r = res + 3 * k;
    const double tmp = r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + sigma2;
    const double v = sigma2 / (tmp * tmp);
    wt[k] = v;
    if (v != v) atomicAdd(nan_count, 1);
}

// out[a] = (A^T W v)[a] = sum over a's pairs, in pair order, of sign w_k v[k], plus v[P] at the fixed image.
__device__ inline void gather(int64_t a, const Graph& g, const double* __restrict__ v, const double* __restrict__ wt,
                              double* out) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    const int begin = g.row_ptr[a], end = g.row_ptr[a + 1];
    for (int e = begin; e < end; ++e) {
        const int id = g.ent[e], k = id >> 1;
        const double c = ((id & 1) ? 1.0 : -1.0) * (wt ? wt[k] : 1.0);
        s0 += c * v[3 * (int64_t)k];
        s1 += c * v[3 * (int64_t)k + 1];
        s2 += c * v[3 * (int64_t)k + 2];
    }
    if (a == g.fixed) {
        s0 += v[3 * g.P];
        s1 += v[3 * g.P + 1];
        s2 += v[3 * g.P + 2];
    }
    out[0] = s0;
    out[1] = s1;
    out[2] = s2;
}

__global__ __launch_bounds__(kT) void k_gather(Graph g, const double* __restrict__ v, const double* __restrict__ wt,
                                               double* __restrict__ out) {
    const int64_t a = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (a >= g.n) return;
    gather(a, g, v, wt, out + 3 * a);
}

// x = Minv t: one wave per row, the lanes stride over the columns, a butterfly sum at the end.
__global__ __launch_bounds__(kT) void k_matvec(int64_t n, const double* __restrict__ Minv, const double* __restrict__ t,
                                               double* __restrict__ x) {
    const int64_t a = (int64_t)blockIdx.x * (kT / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (a >= n) return;  // (the whole wave leaves together)
    const double* row = Minv + a * n;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int64_t c = lane; c < n; c += 64) {
        const double m = row[c];
        s0 += m * t[3 * c];
        s1 += m * t[3 * c + 1];
        s2 += m * t[3 * c + 2];
    }
    wave_sum3(s0, s1, s2);
    if (lane == 0) {
        x[3 * a] = s0;
        x[3 * a + 1] = s1;
        x[3 * a + 2] = s2;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// ADMM (l1_solver.py:20-38)
// ---------------------------------------------------------------------------------------------------------------------
// Rows k = 0 .. P (P = the gauge row): a_times_x, ax_hat, the shrinkage, the dual update; dz = z - z_old and
// tv = rhs + z - u (the next iteration's right-hand side before A^T) are stored; part[q][block] receives the block's
// sums of |a_times_x - z - rhs|^2, |a_times_x|^2, |z|^2, |rhs|^2.
__global__ __launch_bounds__(kT) void k_admm_rows(Graph g, double alpha, double kappa, const double* __restrict__ rhs,
                                                  const double* __restrict__ x, double* __restrict__ z,
                                                  double* __restrict__ u, double* __restrict__ dz,
                                                  double* __restrict__ tv, double* __restrict__ part) {
    __shared__ double sh[4 * kT / 64];
    const int64_t k = (int64_t)blockIdx.x * kT + threadIdx.x;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (k <= g.P) {
        const double* xa = k < g.P ? x + 3 * (int64_t)g.pi[k] : nullptr;
        const double* xb = x + 3 * (k < g.P ? (int64_t)g.pj[k] : g.fixed);
        for (int c = 0; c < 3; ++c) {
            const int64_t o = 3 * k + c;
            const double ax = xa ? xb[c] - xa[c] : xb[c];
            const double r = rhs[o], zo = z[o], uo = u[o];
            const double axh = alpha * ax + (1.0 - alpha) * (zo + r);
            const double v = axh - r + uo;
            const double zn = fmax(0.0, v - kappa) - fmax(0.0, -v - kappa);
            const double un = uo + (axh - zn - r);
            z[o] = zn;
            u[o] = un;
            dz[o] = zn - zo;
            tv[o] = r + zn - un;
            const double pr = ax - zn - r;
            acc[0] += pr * pr;
            acc[1] += ax * ax;
            acc[2] += zn * zn;
            acc[3] += r * r;
        }
    }
    block_sum<4, kT>(acc, sh);
    if (threadIdx.x == 0)
        for (int q = 0; q < 4; ++q) part[(int64_t)q * gridDim.x + blockIdx.x] = acc[q];
}

// part[q][block]: the block's sums of |rho A^T dz|^2 and |rho A^T u|^2 over its images.
__global__ __launch_bounds__(kT) void k_gather_norms(Graph g, double rho, const double* __restrict__ dz,
                                                     const double* __restrict__ u, double* __restrict__ part) {
    __shared__ double sh[2 * kT / 64];
    const int64_t a = (int64_t)blockIdx.x * kT + threadIdx.x;
    double acc[2] = {0.0, 0.0};
    if (a < g.n) {
        double s[3], t[3];
        gather(a, g, dz, nullptr, s);
        gather(a, g, u, nullptr, t);
        for (int c = 0; c < 3; ++c) {
            acc[0] += (rho * s[c]) * (rho * s[c]);
            acc[1] += (rho * t[c]) * (rho * t[c]);
        }
    }
    block_sum<2, kT>(acc, sh);
    if (threadIdx.x == 0)
        for (int q = 0; q < 2; ++q) part[(int64_t)q * gridDim.x + blockIdx.x] = acc[q];
}

// out[0..3] = the sums of part_rows[q][0 .. nb_rows), out[4..5] = those of part_img[q][0 .. nb_img): thread t adds the
// blocks t, t + 256, .. in order, then the threads' sums are reduced in a fixed order (one workgroup).
__global__ __launch_bounds__(kT) void k_finish(int nb_rows, const double* __restrict__ part_rows, int nb_img,
                                               const double* __restrict__ part_img, double* __restrict__ out) {
    __shared__ double sh[6 * kT / 64];
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int q = 0; q < 4; ++q)
        for (int b = threadIdx.x; b < nb_rows; b += kT) acc[q] += part_rows[(int64_t)q * nb_rows + b];
    for (int q = 0; q < 2; ++q)
        for (int b = threadIdx.x; b < nb_img; b += kT) acc[4 + q] += part_img[(int64_t)q * nb_img + b];
    block_sum<6, kT>(acc, sh);
    if (threadIdx.x == 0)
        for (int q = 0; q < 6; ++q) out[q] = acc[q];
}

__global__ __launch_bounds__(kT) void k_admm_init(int64_t m3, const double* __restrict__ rhs, double* __restrict__ z,
                                                  double* __restrict__ u, double* __restrict__ tv) {
    const int64_t o = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (o >= m3) return;
    z[o] = 0.0;
    u[o] = 0.0;
    tv[o] = rhs[o];
}

// out[0] = |step|^2, out[1] = sum over the images of |step_a| (ComputeAverageStepSize's numerator), out[2] = NaN
// components, out[3] = NaN weights (nan_w, optional), out[4] = the inversion's ok word (optional; 1 when absent).
// One workgroup: thread t takes the images t, t + 256, ..
__global__ __launch_bounds__(kT) void k_step_stats(int64_t n, const double* __restrict__ step,
                                                   const int* __restrict__ nan_w, const int* __restrict__ ok,
                                                   double* __restrict__ out) {
    __shared__ double sh[3 * kT / 64];
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t a = threadIdx.x; a < n; a += kT) {
        const double x = step[3 * a], y = step[3 * a + 1], z = step[3 * a + 2];
        const double s2 = x * x + y * y + z * z;
        acc[0] += s2;
        acc[1] += sqrt(s2);
        acc[2] += (x != x) + (y != y) + (z != z);
    }
    block_sum<3, kT>(acc, sh);
    if (threadIdx.x == 0) {
        out[0] = acc[0];
        out[1] = acc[1];
        out[2] = acc[2];
        out[3] = nan_w ? (double)nan_w[0] : 0.0;
        out[4] = ok ? (double)ok[0] : 1.0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
struct Dense {
    int64_t n = 0, ld = 0;
    double *E = nullptr, *W = nullptr, *inv = nullptr, *d = nullptr, *piv = nullptr;
    int* ok = nullptr;
    void alloc(StageTemps& w, int64_t n_) {
        n = n_;
        ld = (int64_t)gj_steps((int)n) * kGB;
        E = w.get<double>(ld * ld);
        W = w.get<double>(ld * ld);
        inv = w.get<double>(n * n);
        d = w.get<double>(ld);
        piv = w.get<double>(2 * kGB * kGB);
        ok = w.get<int>(1);
    }
};

// M = B^T W B into the padded buffer, then its inverse into D.inv (D.ok[0] = 0 for a non-positive pivot).
void build_and_invert(const Graph& g, const Dense& D, const double* wt, hipStream_t s) {
    k_system<<<(unsigned)D.ld, kT, 0, s>>>(g.n, D.ld, g.row_ptr, g.ent, g.pi, g.pj, wt, g.fixed, D.E, D.d);
    for (int u = 0; u <= gj_steps((int)g.n); ++u) launch_gj_unit(u, (int)g.n, D.E, D.W, D.piv, D.d, D.inv, D.ok, s);
}

bool finite_nonneg(double v) { return std::isfinite(v) && v >= 0.0; }

bool options_ok(const insfm_rotavg_options* o) {
    return o->max_num_l1_iterations >= 0 && o->max_num_irls_iterations >= 0 &&
           finite_nonneg(o->l1_step_convergence_threshold) && finite_nonneg(o->irls_step_convergence_threshold) &&
           finite_nonneg(o->irls_loss_parameter_sigma) && std::isfinite(o->rho) && o->rho > 0.0 &&
           std::isfinite(o->alpha) && finite_nonneg(o->absolute_tolerance) && finite_nonneg(o->relative_tolerance);
}

int solve(int64_t n, int64_t P, const int32_t* pi, const int32_t* pj, const double* quat, double* rot_io, int64_t fixed,
          const double* fixed_rot, const insfm_rotavg_options& o, int32_t* info_out, hipStream_t s) {
    StageTemps w(s);
    if (!w.ok()) return INSFM_BA_ENOMEM;
    Graph g;
    const int rc = prepare(w, n, P, pi, pj, fixed, g);
    if (rc != INSFM_BA_OK) return rc;
    const int64_t m3 = 3 * (P + 1), n3 = 3 * n;
    const int nb_rows = (int)blocks_for(P + 1, kT), nb_img = (int)blocks_for(n, kT);
    Dense D;
    D.alloc(w, n);
    double *rot = w.get<double>(n3), *res = w.get<double>(m3), *step = w.get<double>(n3), *t = w.get<double>(n3);
    double *z = w.get<double>(m3), *u = w.get<double>(m3), *dz = w.get<double>(m3), *tv = w.get<double>(m3);
    double *wt = w.get<double>(P), *part_rows = w.get<double>(4 * (size_t)nb_rows);
    double *part_img = w.get<double>(2 * (size_t)nb_img), *stats = w.get<double>(8);
    int* nan_w = w.get<int>(1);
    if (!w.ok()) return INSFM_BA_ENOMEM;
    double* host = reinterpret_cast<double*>(w.host());  // eight pinned words
    int32_t info[INSFM_ROTAVG_INFO_LEN] = {0};

    INSFM_HIP(hipMemcpyAsync(rot, rot_io, sizeof(double) * n3, hipMemcpyDeviceToDevice, s));
    const auto residuals = [&] { launch(k_residuals, P + 1, s, P, pi, pj, quat, rot, fixed, fixed_rot, res); };
    const auto finish = [&](int failed) {
        info[INSFM_ROTAVG_INFO_FAILED] = failed;
        for (int q = 0; q < INSFM_ROTAVG_INFO_LEN; ++q) info_out[q] = info[q];
        return INSFM_BA_OK;
    };
    residuals();

    if (o.max_num_l1_iterations > 0) {  // SolveL1Regression (:100-124)
        build_and_invert(g, D, nullptr, s);
        int host_ok = 0;
        INSFM_HIP(hipMemcpyAsync(&host_ok, D.ok, sizeof(int), hipMemcpyDeviceToHost, s));
        INSFM_HIP(settle(s));
        if (!host_ok) return INSFM_BA_ESOLVER;
        const double primal_abs = std::sqrt((double)m3) * o.absolute_tolerance;
        const double dual_abs = std::sqrt((double)n3) * o.absolute_tolerance;
        int cap = 10, iteration = 0;
        double curr_norm = 0.0;
        while (iteration < o.max_num_l1_iterations) {
            const double last_norm = curr_norm;
            launch(k_admm_init, m3, s, m3, res, z, u, tv);
            int inner = 0;
            while (inner < cap) {  // L1Solver.solve (l1_solver.py:20-38)
                ++inner;
                launch(k_gather, n, s, g, tv, nullptr, t);
                launch<kT / 64>(k_matvec, n, s, n, D.inv, t, step);
                launch(k_admm_rows, P + 1, s, g, o.alpha, 1.0 / o.rho, res, step, z, u, dz, tv, part_rows);
                launch(k_gather_norms, n, s, g, o.rho, dz, u, part_img);
                k_finish<<<1, kT, 0, s>>>(nb_rows, part_rows, nb_img, part_img, stats);
                INSFM_HIP(hipMemcpyAsync(host, stats, 6 * sizeof(double), hipMemcpyDeviceToHost, s));
                INSFM_HIP(settle(s));
                const double r_norm = std::sqrt(host[0]), ax_norm = std::sqrt(host[1]), z_norm = std::sqrt(host[2]);
                const double rhs_norm = std::sqrt(host[3]), s_norm = std::sqrt(host[4]), atu_norm = std::sqrt(host[5]);
                const double max_norm = std::fmax(std::fmax(ax_norm, z_norm), rhs_norm);
                const double primal_eps = primal_abs + o.relative_tolerance * max_norm;
                const double dual_eps = dual_abs + o.relative_tolerance * atu_norm;
                if (r_norm < primal_eps && s_norm < dual_eps) break;
            }
            if (iteration < 10) info[INSFM_ROTAVG_INFO_ADMM + iteration] = inner;
            info[INSFM_ROTAVG_INFO_L1_ITERS] = iteration + 1;
            k_step_stats<<<1, kT, 0, s>>>(n, step, nullptr, nullptr, stats);
            INSFM_HIP(hipMemcpyAsync(host, stats, 8 * sizeof(double), hipMemcpyDeviceToHost, s));
            INSFM_HIP(settle(s));
            if (host[2] != 0.0) return finish(INSFM_ROTAVG_FAILED_L1);
            curr_norm = std::sqrt(host[0]);
            launch(k_update, n, s, n, rot, step);
            residuals();
            ++iteration;
            if (host[1] / (double)n < o.l1_step_convergence_threshold || std::fabs(last_norm - curr_norm) < 1e-6) break;
            cap = cap * 2 < 100 ? cap * 2 : 100;
        }
    }

    const double sigma2 = o.irls_loss_parameter_sigma * o.irls_loss_parameter_sigma;
    for (int it = 0; it < o.max_num_irls_iterations; ++it) {  // SolveIRLS (:126-161)
        info[INSFM_ROTAVG_INFO_IRLS_ITERS] = it + 1;
        INSFM_HIP(hipMemsetAsync(nan_w, 0, sizeof(int), s));
        launch(k_weights, P, s, P, res, sigma2, wt, nan_w);
        build_and_invert(g, D, wt, s);
        launch(k_gather, n, s, g, res, wt, t);
        launch<kT / 64>(k_matvec, n, s, n, D.inv, t, step);
        k_step_stats<<<1, kT, 0, s>>>(n, step, nan_w, D.ok, stats);
        launch(k_update, n, s, n, rot, step);
        residuals();
        INSFM_HIP(hipMemcpyAsync(host, stats, 8 * sizeof(double), hipMemcpyDeviceToHost, s));
        INSFM_HIP(settle(s));
        if (host[3] != 0.0) return finish(INSFM_ROTAVG_FAILED_IRLS);  // (the reference tests the weights first)
        if (host[4] == 0.0) return INSFM_BA_ESOLVER;
        if (host[1] / (double)n < o.irls_step_convergence_threshold) break;
    }

    INSFM_HIP(hipMemcpyAsync(rot_io, rot, sizeof(double) * n3, hipMemcpyDeviceToDevice, s));
    INSFM_HIP(settle(s));
    return finish(0);
}

}  // namespace

extern "C" int insfm_rotavg_solve(int64_t n, int64_t n_pairs, const int32_t* pair_i, const int32_t* pair_j,
                                  const double* pair_quat, double* rot, int64_t fixed, const double* fixed_rot,
                                  const insfm_rotavg_options* opt, int32_t* info, void* stream) {
    if (!sizes_ok(n, n_pairs) || n == 0 || !rot || !fixed_rot || !opt || !info || fixed < 0 || fixed >= n)
        return INSFM_BA_EINVAL;
    if (n_pairs > 0 && (!pair_i || !pair_j || !pair_quat)) return INSFM_BA_EINVAL;
    if (!options_ok(opt)) return INSFM_BA_EINVAL;
    return solve(n, n_pairs, pair_i, pair_j, pair_quat, rot, fixed, fixed_rot, *opt, info,
                 reinterpret_cast<hipStream_t>(stream));
}

extern "C" int insfm_rotavg_residuals(int64_t n, int64_t n_pairs, const int32_t* pair_i, const int32_t* pair_j,
                                      const double* pair_quat, const double* rot, int64_t fixed,
                                      const double* fixed_rot, double* res, void* stream) {
    if (!sizes_ok(n, n_pairs) || n == 0 || !rot || !fixed_rot || !res || fixed < 0 || fixed >= n) return INSFM_BA_EINVAL;
    if (n_pairs > 0 && (!pair_i || !pair_j || !pair_quat)) return INSFM_BA_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    StageTemps w(s, /*pinned=*/false);
    Graph g;
    const int rc = prepare(w, n, n_pairs, pair_i, pair_j, fixed, g);
    if (rc != INSFM_BA_OK) return rc;
    launch(k_residuals, n_pairs + 1, s, n_pairs, pair_i, pair_j, pair_quat, rot, fixed, fixed_rot, res);
    INSFM_HIP(settle(s));
    return INSFM_BA_OK;
}

extern "C" int insfm_rotavg_update(int64_t n, double* rot, const double* step, void* stream) {
    if (n < 0 || n > INSFM_ROTAVG_MAX_IMAGES) return INSFM_BA_EINVAL;
    if (n == 0) return INSFM_BA_OK;
    if (!rot || !step) return INSFM_BA_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    launch(k_update, n, s, n, rot, step);
    INSFM_HIP(settle(s));
    return INSFM_BA_OK;
}

extern "C" int insfm_rotavg_system(int64_t n, int64_t n_pairs, const int32_t* pair_i, const int32_t* pair_j,
                                   const double* weights, int64_t fixed, double* M, double* inverse, void* stream) {
    if (!sizes_ok(n, n_pairs) || n == 0 || !M || fixed < 0 || fixed >= n) return INSFM_BA_EINVAL;
    if (n_pairs > 0 && (!pair_i || !pair_j)) return INSFM_BA_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    StageTemps w(s, /*pinned=*/false);
    Graph g;
    const int rc = prepare(w, n, n_pairs, pair_i, pair_j, fixed, g);
    if (rc != INSFM_BA_OK) return rc;
    Dense D;
    if (inverse) D.alloc(w, n);
    if (!w.ok()) return INSFM_BA_ENOMEM;
    k_system<<<(unsigned)n, kT, 0, s>>>(n, n, g.row_ptr, g.ent, pair_i, pair_j, weights, fixed, M, nullptr);
    int host_ok = 1;
    if (inverse) {
        build_and_invert(g, D, weights, s);
        INSFM_HIP(hipMemcpyAsync(inverse, D.inv, sizeof(double) * n * n, hipMemcpyDeviceToDevice, s));
        INSFM_HIP(hipMemcpyAsync(&host_ok, D.ok, sizeof(int), hipMemcpyDeviceToHost, s));
    }
    INSFM_HIP(settle(s));
    return host_ok ? INSFM_BA_OK : INSFM_BA_ESOLVER;
}

extern "C" int insfm_rotavg_pair_errors(int64_t n, int64_t n_pairs, const int32_t* pair_i, const int32_t* pair_j,
                                        const double* pair_quat, const double* world2cam, double* angle_deg,
                                        void* stream) {
    // (no n x n buffer here: n is only bounded by the 32-bit indices)
    if (n < 0 || n >= ((int64_t)1 << 31) || n_pairs < 0 || n_pairs >= ((int64_t)1 << 30) || (n == 0 && n_pairs > 0))
        return INSFM_BA_EINVAL;
    if (n_pairs == 0) return INSFM_BA_OK;
    if (!pair_i || !pair_j || !pair_quat || !world2cam || !angle_deg) return INSFM_BA_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    StageTemps w(s, /*pinned=*/false);
    Graph g;
    const int rc = prepare(w, n, n_pairs, pair_i, pair_j, 0, g);
    if (rc != INSFM_BA_OK) return rc;
    launch(k_pair_errors, n_pairs, s, n_pairs, pair_i, pair_j, pair_quat, world2cam, angle_deg);
    INSFM_HIP(settle(s));
    return INSFM_BA_OK;
}
