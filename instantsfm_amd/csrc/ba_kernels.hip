// MI355X (gfx950) sparse bundle-adjustment core: HIP kernels + host LM driver behind include/insfm_ba.h.
//
// One LM step (bae.optim.LM.step as reconstructed in SURVEY.md 3.3, options of bundle_adjustment.py:115-119):
//   linearize (per step)   k_lin_points  : per track, residual + analytic J + Huber/Triggs weight  -> W_o, V_p, g_p
//                          k_lin_cams    : per camera, J~c^T J~c and -J~c^T r~ (LDS-staged batch)  -> U_c, g_c
//   per trial (damping f)  k_point_prep  : V_p clamp/damp + 3x3 SPD inverse                          -> V^-1, y = V^-1 g_p
//                          k_schur       : per camera row, LDS-resident row of S (upper blocks), b
//                          k_cg_factor / k_cg_scale : S_ii = L L^T, S~ = L^-1 S L^-T, r0 = L^-1 b
//                          k_cg_iter x k : Chronopoulos-Gear CG on S~, ONE launch per iteration
//                          k_cg_finish   : dc = L^-T x~
//                          k_backsub_rc  : dp = V^-1 (g_p - W^T dc), trial points, gain terms; its last blocks the
//                                          SE3 left retraction of the cameras, intrinsics +=, gain terms
//                          k_cost        : Huber loss + sum ||r||^2 at the trial parameters
//                          k_final       : fixed-order reduction of all partials -> 64 B to the host
// Every cross-workgroup reduction is a fixed-order partial sum (no float atomics in global memory), so a step is
// bitwise reproducible when desc.deterministic = 1 (the Schur row accumulation then uses one wave per row).
#include <hip/hip_runtime.h>

#include <atomic>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <unordered_map>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/insfm_ba.h"
#include "../../include/insfm_gp.h"
#include "../../include/insfm_ba_debug.h"
#include "ba_device.h"
#include "ba_common.h"
#include "ba_twolevel.h"
#include "ba_cgp.h"
#include "ba_gp.h"
#include "cg_poll.h"
#include "create_plan.h"

using namespace insfm;

namespace {

constexpr int kLdsBudget = 96 * 1024;  // dynamic LDS cap for one k_schur workgroup
#ifndef SCHUR_LDS_KB
#define SCHUR_LDS_KB 96  // k_schur row-chunk LDS target (rows with more upper blocks are split into chunks)
#endif
constexpr int kLdsTarget = SCHUR_LDS_KB * 1024;
#ifndef SCHUR_LDS_KB_DET
#define SCHUR_LDS_KB_DET 52  // deterministic mode's k_schur row-chunk LDS target (3 four-wave workgroups per CU)
#endif
constexpr int kLdsTargetDet = SCHUR_LDS_KB_DET * 1024;
#ifndef INSFM_SCHUR_WAVES
#define INSFM_SCHUR_WAVES 8
#endif
constexpr int kSchurWaves = INSFM_SCHUR_WAVES;  // waves per k_schur workgroup (non-deterministic mode)
constexpr int kSchurChunk = 4;  // k_schur rounds per chunk of a camera's observation list (create)
#ifndef LIN_CAMS_NT
#define LIN_CAMS_NT 128  // k_lin_cams_reg threads per camera (measured 128 / 192 / 256 / 320: 0.156 / 0.161 / 0.167 / 0.194 ms linearize)
#endif
#ifndef COST_THREADS
#define COST_THREADS 256
#endif
constexpr int kCostThreads = COST_THREADS;  // k_cost workgroup size (64 / 128 / 512: same time, 25-26 us; 1024: trial cost 0.045 -> 0.055 ms)
#ifndef SCHUR_MINW
#define SCHUR_MINW 1  // k_schur launch bound: minimum waves per SIMD (caps VGPRs: 4 -> 128)
#endif
#ifndef SCHUR_SLOTPRE
#define SCHUR_SLOTPRE 1  // k_schur: a round's partner slots looked up before its LDS adds
#endif
// the persistent CG's solves form the factorization and the coarse basis in one launch (k_cg_factor_basis; 0: the
// separate k_cg_factor and k_tl_basis launches, for A/B builds)
#ifndef FACTOR_BASIS
#define FACTOR_BASIS 1
#endif
#ifndef SCHUR_UP
#define SCHUR_UP 10
#endif
#ifndef LIN_NT_STORE
// k_lin_points: the 384-MB Y-record stream stored with the nontemporal hint (global_store_dwordx4 ... nt).  Config 3
// (profiles/r6_v10/nt_ab.txt, same box): back-to-back launches 152-153 -> 85 us, LM step 1.046-1.050 -> 1.013-1.033
// ms; k_schur, which reads the records next, unchanged (440-448 us).
#define LIN_NT_STORE 1
#endif
#ifndef SCHUR_NT_STORE
#define SCHUR_NT_STORE 0  // k_schur: S blocks stored with the nontemporal hint (A/B builds)
#endif
// deterministic mode's k_schur: waves per workgroup; with more than one the waves take their LDS adds in turn.
// Measured on config 3 (profiles/r6_v7/det_ab*.txt, k_schur per trial): 1 wave (round 5) 1.15 ms; 2 / 3 / 4 / 6 / 8
// waves 1.06 / 0.97 / 0.90 / 1.68 / 1.36 ms (4 waves at 5 partners in flight: 148 VGPRs, three workgroups per CU;
// 3 / 4 / 10 partners in flight 0.98 / 0.93 / 1.10 ms; row chunks of 40 / 52 / 64 KB 1.33 / 0.90 / 1.03 ms)
#ifndef SCHUR_DET_WAVES
#define SCHUR_DET_WAVES 4
#endif
#ifndef SCHUR_UP_DET
#define SCHUR_UP_DET 5  // partners in flight per group in the turn-taking form
#endif
#define SCHUR_DET_ORD (SCHUR_DET_WAVES > 1)
constexpr int kDetWaves = SCHUR_DET_WAVES;

// ------------------------------------------------------------------------------------------------------------
// reductions
// ------------------------------------------------------------------------------------------------------------
// Fixed-order block reduction of NV values per thread, returned to every thread: a butterfly per wave, then the wave
// sums in wave order (one barrier instead of one per tree level).
template <int NV, int NT = kThreads>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* sh /* >= NV * NT / 64 doubles */) {
    constexpr int NW = NT / 64;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const double s = wave_sum(v[k]);
        if (lane == 0) sh[k * NW + wv] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        double s = sh[k * NW];
#pragma unroll
        for (int w = 1; w < NW; ++w) s += sh[k * NW + w];
        v[k] = s;
    }
    __syncthreads();
}

// Sum n partial records of NV doubles (record-major) in a fixed order; every thread gets the result.
template <int NV, int NT = kThreads>
__device__ __forceinline__ void sum_partials(const double* __restrict__ part, int n, double (&out)[NV], double* sh) {
    double v[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = 0.0;
#pragma unroll 8
    for (int i = threadIdx.x; i < n; i += NT)  // unrolled: 8 loads in flight, the adds in order
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] += part[(size_t)i * NV + k];
    block_sum<NV, NT>(v, sh);
#pragma unroll
    for (int k = 0; k < NV; ++k) out[k] = v[k];
}

__device__ __forceinline__ double huber_weight_sqrt(double s, double delta) {
    const double rs = sqrt(s);
    const double w = rs < delta ? 1.0 : delta / rs;
    return sqrt(w);
}

// ------------------------------------------------------------------------------------------------------------
// linearization
// ------------------------------------------------------------------------------------------------------------
// Every observation's weighted J gives W_o = J~c^T J~p (stored [o][3][D]: a group of D lanes reads each column of W_o
// as one contiguous segment in k_schur); each track reduces V_p = sum J~p^T J~p (packed sym) and g_p = -sum J~p^T r~.
constexpr int kLinThreads = 128;  // k_lin_points workgroup (LDS: W staging + V/g terms of its observations)

// Symmetric camera-point records (round 4).  With R_p the Cholesky factor of point p's damped block at the first
// trial's damping (V_p,d = R_p R_p^T; f = 1 + damping is known when the linearization is enqueued) and L_p = R_p^-T,
// L_p L_p^T = V_p,d^-1, so every observation's record is stored as Y_o = W_o L_p (D x 3, [o][3][D] like W) and
//   S_ij -= sum_p Y_ip Y_jp^T,   b_i -= sum Y_o z_p,  z_p = L_p^T g_p = R_p^-1 g_p:
// k_schur's first trial needs no per-observation V^-1 loads or W V^-1 products.  A retried trial at another damping
// factor f' uses M_p = L_p^-1 V'_p^-1 L_p^-T = R_p^T V'_p^-1 R_p (symmetric) between the records and z'_p = R_p^T y'_p
// (y'_p = V'_p^-1 g_p), formed per point by k_point_prep: the same k_schur with M_p where the GP build has V^-1.
// The first trial's point preparation itself is fused into k_lin_points: per track the damped V_p (diagonal clamped,
// times f), its 3x3 inverse (bitwise k_point_prep's: the same Cholesky steps), R_p and z_p, and the CG status words
// cleared.
struct PointPrep {
    double f = 1.0, cmin = 0.0, cmax = 0.0;
    double* Vinv = nullptr;
    double* y = nullptr;   // z_p = R_p^-1 g_p (with R), else y_p = V_p^-1 g_p
    double* R = nullptr;   // R_p packed (00, 10, 20, 11, 21, 22); null: no records (points-only solves)
    int* flags = nullptr;
    int* status = nullptr;
};
// Returns R_p^-1 (packed) in Ri; all zero when the damped block is not positive definite (flag raised).
__device__ __forceinline__ void point_prep_first(int p, const double V[6], const double g[3], const PointPrep& a,
                                                 double Ri[6]) {
    double s[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k] = V[k];
    s[0] = clampd(s[0], a.cmin, a.cmax) * a.f;
    s[3] = clampd(s[3], a.cmin, a.cmax) * a.f;
    s[5] = clampd(s[5], a.cmin, a.cmax) * a.f;
    double o[6], R[6];
    if (!spd3_factor(s, o, R, Ri)) {
        atomicOr(a.flags, 1);
#pragma unroll
        for (int k = 0; k < 6; ++k) o[k] = R[k] = Ri[k] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) a.Vinv[6 * (size_t)p + k] = o[k];
    if (a.R) {
#pragma unroll
        for (int k = 0; k < 6; ++k) a.R[6 * (size_t)p + k] = R[k];
        a.y[3 * (size_t)p + 0] = Ri[0] * g[0];
        a.y[3 * (size_t)p + 1] = Ri[1] * g[0] + Ri[3] * g[1];
        a.y[3 * (size_t)p + 2] = Ri[2] * g[0] + Ri[4] * g[1] + Ri[5] * g[2];
    } else {
        a.y[3 * (size_t)p + 0] = o[0] * g[0] + o[1] * g[1] + o[2] * g[2];
        a.y[3 * (size_t)p + 1] = o[1] * g[0] + o[3] * g[1] + o[4] * g[2];
        a.y[3 * (size_t)p + 2] = o[2] * g[0] + o[4] * g[1] + o[5] * g[2];
    }
}

// One observation's weighted linearization: the V / g_p terms (cv: V packed sym 6, J~p^T r~ 3) and W_o (w[k * D + a] =
// (J~c^T J~p)[a][k]).
template <int M>
__device__ __forceinline__ void lin_obs(int o, const int* __restrict__ cam, const int* __restrict__ ptl,
                                        const double* __restrict__ uv, const double* __restrict__ pp,
                                        const double* __restrict__ cams, const double* __restrict__ pts, double delta,
                                        double cv[9], double w[3 * kD<M>]) {
    constexpr int D = kD<M>, ST = kStride<M>;
    const int c = cam[o], p = ptl[o];
    const double X[3] = {pts[3 * (size_t)p], pts[3 * (size_t)p + 1], pts[3 * (size_t)p + 2]};
    const double2 z = reinterpret_cast<const double2*>(uv)[o];
    const double uvo[2] = {z.x, z.y};
    const double ppc[2] = {pp[2 * c], pp[2 * c + 1]};
    double r[2], Jc[2][D], Jp[2][3];
    eval_obs<M, true>(cams + (size_t)c * ST, X, ppc, uvo, r, Jc, Jp);
    const double sw = huber_weight_sqrt(r[0] * r[0] + r[1] * r[1], delta);
    r[0] *= sw; r[1] *= sw;
#pragma unroll
    for (int a = 0; a < D; ++a) { Jc[0][a] *= sw; Jc[1][a] *= sw; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { Jp[0][k] *= sw; Jp[1][k] *= sw; }
    cv[0] = Jp[0][0] * Jp[0][0] + Jp[1][0] * Jp[1][0];
    cv[1] = Jp[0][0] * Jp[0][1] + Jp[1][0] * Jp[1][1];
    cv[2] = Jp[0][0] * Jp[0][2] + Jp[1][0] * Jp[1][2];
    cv[3] = Jp[0][1] * Jp[0][1] + Jp[1][1] * Jp[1][1];
    cv[4] = Jp[0][1] * Jp[0][2] + Jp[1][1] * Jp[1][2];
    cv[5] = Jp[0][2] * Jp[0][2] + Jp[1][2] * Jp[1][2];
#pragma unroll
    for (int k = 0; k < 3; ++k) cv[6 + k] = Jp[0][k] * r[0] + Jp[1][k] * r[1];
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k * D + a] = Jc[0][a] * Jp[0][k] + Jc[1][a] * Jp[1][k];
}

// Y_o = W_o L_p in place (w[k * D + a] as lin_obs), L_p = R_p^-T: Y[a][j] = sum_{k <= j} W[a][k] (R_p^-1)[j][k].
template <int D>
__device__ __forceinline__ void y_from_w(double w[3 * D], const double Ri[6]) {
#pragma unroll
    for (int a = 0; a < D; ++a) {
        const double w0 = w[a], w1 = w[D + a], w2 = w[2 * D + a];
        w[a] = w0 * Ri[0];
        w[D + a] = w0 * Ri[1] + w1 * Ri[3];
        w[2 * D + a] = w0 * Ri[2] + w1 * Ri[4] + w2 * Ri[5];
    }
}

// Records of observations [base, base + n) from the LDS staging rows (odd stride WRP) to HBM, consecutive lanes storing
// consecutive 16-B pairs when the record length is even (a pair never crosses a record; every record starts 16-B
// aligned).
template <int WR, int WRP>
__device__ __forceinline__ void store_records(const double* wst, double* __restrict__ Y, int base, int n) {
    const int t = threadIdx.x;
    if constexpr ((WR & 1) == 0) {
        double2* dst = reinterpret_cast<double2*>(Y + (size_t)base * WR);
        for (int k2 = t; k2 < n * (WR / 2); k2 += kLinThreads) {
            const int k = 2 * k2, rec = k / WR, e = k - rec * WR;
            const double* src = wst + rec * WRP + e;
#if LIN_NT_STORE
            typedef double nt_d2 __attribute__((ext_vector_type(2)));
            nt_d2 v2 = {src[0], src[1]};
            __builtin_nontemporal_store(v2, reinterpret_cast<nt_d2*>(dst + k2));
#else
            dst[k2] = make_double2(src[0], src[1]);
#endif
        }
    } else {
        double* dst = Y + (size_t)base * WR;
        for (int k = t; k < n * WR; k += kLinThreads) dst[k] = wst[(k / WR) * WRP + k % WR];
    }
}

template <int M>
__global__ __launch_bounds__(kLinThreads) void k_lin_points(const int* __restrict__ blk, const int* __restrict__ pt_ptr,
                                                         const int* __restrict__ cam, const int* __restrict__ ptl,
                                                         const double* __restrict__ uv, const double* __restrict__ pp,
                                                         const double* __restrict__ cams, const double* __restrict__ pts,
                                                         double delta, double* __restrict__ Y, double* __restrict__ V,
                                                         double* __restrict__ gp, PointPrep pp1, long long* stp) {
    // One workgroup per run of whole tracks (blk, built at create: at most kLinThreads observations unless a single track
    // is longer), one thread per observation: coalesced uv / cam / point loads.  Each observation's V / g terms go to
    // LDS and one thread per track adds them in observation order -- the same sequence of additions as a thread walking
    // its track; that thread then prepares the point (damped V^-1, R_p, z_p) and puts R_p^-1 in LDS, and every
    // observation turns its W_o (kept in registers) into Y_o, staged in LDS (odd row stride) and stored coalesced in
    // 16-B pairs (192-B records for D = 8).  A run that is one track longer than the workgroup evaluates its
    // observations twice (once for the sums, once for the records).  One 25.6-KB LDS buffer serves the terms, the
    // R_p^-1 table and the record staging (6 workgroups per CU).  Y null (points-only solves): no records.
    constexpr int D = kD<M>, WR = 3 * D, WRP = WR | 1;  // odd LDS row stride
    static_assert(WRP >= 9, "the V / g terms reuse a record staging row");
    const StampScope stamp_(stp);
    __shared__ double wst[kLinThreads * WRP];
    const int t = threadIdx.x;
    const int tb = blk[blockIdx.x], te = blk[blockIdx.x + 1];
    const int ob = pt_ptr[tb], oe = pt_ptr[te];
    const bool one = oe - ob <= kLinThreads;  // (uniform) the run's observations fit one pass
    double Vs[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
    const int tr = tb + t;  // the track this thread sums (tracks of the run)
    const int tlo = tr < te ? pt_ptr[tr] : 0, thi = tr < te ? pt_ptr[tr + 1] : 0;
    double w[WR];
    for (int base = ob; base < oe; base += kLinThreads) {
        const int o = base + t;
        double cv[9];
        if (o < oe) {
            lin_obs<M>(o, cam, ptl, uv, pp, cams, pts, delta, cv, w);
#pragma unroll
            for (int k = 0; k < 9; ++k) wst[(size_t)t * 9 + k] = cv[k];
        }
        __syncthreads();
        if (tr < te) {
            const int lo = max(tlo, base), hi = min(thi, base + kLinThreads);
            for (int q = lo; q < hi; ++q) {
                const double* cq = wst + (size_t)(q - base) * 9;
#pragma unroll
                for (int k = 0; k < 6; ++k) Vs[k] += cq[k];
#pragma unroll
                for (int k = 0; k < 3; ++k) g[k] -= cq[6 + k];
            }
        }
        __syncthreads();
    }
    double Ri[6];
    if (tr < te) {
#pragma unroll
        for (int k = 0; k < 6; ++k) V[6 * (size_t)tr + k] = Vs[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) gp[3 * (size_t)tr + k] = g[k];
        point_prep_first(tr, Vs, g, pp1, Ri);
        if (Y) {
#pragma unroll
            for (int k = 0; k < 6; ++k) wst[(size_t)t * 6 + k] = Ri[k];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < 4) pp1.status[threadIdx.x] = 0;  // (k_point_prep's status clear)
    if (!Y) return;
    __syncthreads();
    if (one) {
        const int o = ob + t;
        if (o < oe) {
            const double* rq = wst + (size_t)(ptl[o] - tb) * 6;
            double r6[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) r6[k] = rq[k];
            y_from_w<D>(w, r6);
        }
        __syncthreads();  // (every R^-1 read before the staging overwrites the table)
        if (o < oe) {
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int k = 0; k < 3; ++k) wst[(size_t)t * WRP + k * D + a] = w[k * D + a];
        }
        __syncthreads();
        store_records<WR, WRP>(wst, Y, ob, oe - ob);
        return;
    }
    // one track longer than the workgroup: its R^-1 from the table, then the records chunk by chunk
    double r6[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) r6[k] = wst[k];
    __syncthreads();
    for (int base = ob; base < oe; base += kLinThreads) {
        const int o = base + t;
        if (o < oe) {
            double cv[9];
            lin_obs<M>(o, cam, ptl, uv, pp, cams, pts, delta, cv, w);
            y_from_w<D>(w, r6);
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int k = 0; k < 3; ++k) wst[(size_t)t * WRP + k * D + a] = w[k * D + a];
        }
        __syncthreads();
        store_records<WR, WRP>(wst, Y, base, min(kLinThreads, oe - base));
        __syncthreads();
    }
}

// One workgroup per camera: 256 observations at a time are evaluated (one per thread) into an LDS batch
// [obs][J~c row0 | J~c row1 | r~0 r~1]; then thread e owns entry e of [U (DxD) | g_c (D)] and sums the batch in
// observation order (the oracle's order).  The camera-major point index and uv of each observation (cm_pt, cm_uv,
// built at create) are read coalesced; the next batch's point is fetched while the current batch is reduced and
// the indices two batches ahead, so no batch waits on a dependent load chain.
template <int M>
__global__ __launch_bounds__(kThreads) void k_lin_cams(const int* __restrict__ cam_ptr, const int* __restrict__ cm_pt,
                                                       const double* __restrict__ cm_uv, const double* __restrict__ pp,
                                                       const double* __restrict__ cams, const double* __restrict__ pts,
                                                       double delta, double* __restrict__ U, double* __restrict__ gc) {
    constexpr int D = kD<M>, ST = kStride<M>;
    constexpr int RW = 2 * D + 2;
    constexpr int E = D * D + D;
    constexpr int EPT = (E + kThreads - 1) / kThreads;
    extern __shared__ __attribute__((aligned(16))) double sh[];
    const int c = blockIdx.x, t = threadIdx.x;
    const int eb = cam_ptr[c], ee = cam_ptr[c + 1];
    const double2* uv2 = reinterpret_cast<const double2*>(cm_uv);
    double camv[ST];
#pragma unroll
    for (int k = 0; k < ST; ++k) camv[k] = cams[(size_t)c * ST + k];
    const double ppc[2] = {pp[2 * c], pp[2 * c + 1]};
    double acc[EPT];
#pragma unroll
    for (int m = 0; m < EPT; ++m) acc[m] = 0.0;
    // pipeline registers: current batch (X, z), next batch (pn, zn), two ahead (pnn, znn)
    double X[3] = {0.0, 0.0, 0.0};
    double2 z = make_double2(0.0, 0.0), zn = z, znn = z;
    int pn = 0, pnn = 0;
    {
        const int e0 = eb + t, e1 = e0 + kThreads;
        if (e0 < ee) {
            const int p0 = cm_pt[e0];
            z = uv2[e0];
            X[0] = pts[3 * (size_t)p0]; X[1] = pts[3 * (size_t)p0 + 1]; X[2] = pts[3 * (size_t)p0 + 2];
        }
        if (e1 < ee) { pn = cm_pt[e1]; zn = uv2[e1]; }
    }
    for (int base = eb; base < ee; base += kThreads) {
        const int e = base + t;
        const bool has = e < ee, hn = e + kThreads < ee, hnn = e + 2 * kThreads < ee;
        double Xn[3] = {0.0, 0.0, 0.0};
        if (hn) { Xn[0] = pts[3 * (size_t)pn]; Xn[1] = pts[3 * (size_t)pn + 1]; Xn[2] = pts[3 * (size_t)pn + 2]; }
        if (hnn) { pnn = cm_pt[e + 2 * kThreads]; znn = uv2[e + 2 * kThreads]; }
        double* row = sh + (size_t)t * RW;
        if (has) {
            const double uvo[2] = {z.x, z.y};
            double r[2], Jc[2][D], Jp[2][3];
            eval_obs<M, true>(camv, X, ppc, uvo, r, Jc, Jp);
            const double sw = huber_weight_sqrt(r[0] * r[0] + r[1] * r[1], delta);
#pragma unroll
            for (int a = 0; a < D; ++a) { row[a] = Jc[0][a] * sw; row[D + a] = Jc[1][a] * sw; }
            row[2 * D] = r[0] * sw;
            row[2 * D + 1] = r[1] * sw;
        }
        __syncthreads();
        const int n = min(kThreads, ee - base);
#pragma unroll
        for (int m = 0; m < EPT; ++m) {
            const int ent = t + m * kThreads;
            if (ent < D * D) {
                const int a = ent / D, b = ent % D;
                double s = acc[m];
                for (int i = 0; i < n; ++i) {
                    const double* rw = sh + (size_t)i * RW;
                    s += rw[a] * rw[b] + rw[D + a] * rw[D + b];
                }
                acc[m] = s;
            } else if (ent < E) {
                const int a = ent - D * D;
                double s = acc[m];
                for (int i = 0; i < n; ++i) {
                    const double* rw = sh + (size_t)i * RW;
                    s -= rw[a] * rw[2 * D] + rw[D + a] * rw[2 * D + 1];
                }
                acc[m] = s;
            }
        }
        __syncthreads();
        X[0] = Xn[0]; X[1] = Xn[1]; X[2] = Xn[2];
        z = zn; pn = pnn; zn = znn;
    }
#pragma unroll
    for (int m = 0; m < EPT; ++m) {
        const int ent = t + m * kThreads;
        if (ent < D * D) U[(size_t)c * D * D + ent] = acc[m];
        else if (ent < E) gc[(size_t)c * D + (ent - D * D)] = acc[m];
    }
}

// Register form of k_lin_cams for D <= 9 (D(D+1)/2 + D accumulators per thread): one workgroup per camera, thread t
// evaluates observations t, t + 256, ... of the camera and keeps its own partial sums of the upper triangle of U and
// of g_c in registers (no per-batch LDS round trip, no 256-long dependent add chain per entry); the partials are then
// summed by a fixed butterfly per wave and the 4 wave sums in wave order, and U is written with both triangles from
// the upper one (a product commutes exactly, so U stays exactly symmetric).  Same point / uv pipeline as k_lin_cams.
template <int M, int NT = LIN_CAMS_NT>
__global__ __launch_bounds__(NT) void k_lin_cams_reg(const int* __restrict__ cam_ptr, const int* __restrict__ cm_pt,
                                                           const double* __restrict__ cm_uv, const double* __restrict__ pp,
                                                           const double* __restrict__ cams, const double* __restrict__ pts,
                                                           double delta, double* __restrict__ U, double* __restrict__ gc) {
    constexpr int D = kD<M>, ST = kStride<M>, NU = D * (D + 1) / 2, NE = NU + D;
    static_assert(D <= 9, "register accumulation is sized for D <= 9");
    constexpr int NW = NT / 64;
    __shared__ double red[NW][NE];
    const int c = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int eb = cam_ptr[c], ee = cam_ptr[c + 1];
    const double2* uv2 = reinterpret_cast<const double2*>(cm_uv);
    double camv[ST];
#pragma unroll
    for (int k = 0; k < ST; ++k) camv[k] = cams[(size_t)c * ST + k];
    const double ppc[2] = {pp[2 * c], pp[2 * c + 1]};
    double acc[NE];
#pragma unroll
    for (int m = 0; m < NE; ++m) acc[m] = 0.0;
    double X[3] = {0.0, 0.0, 0.0};
    double2 z = make_double2(0.0, 0.0), zn = z, znn = z;
    int pn = 0, pnn = 0;
    {
        const int e0 = eb + t, e1 = e0 + NT;
        if (e0 < ee) {
            const int p0 = cm_pt[e0];
            z = uv2[e0];
            X[0] = pts[3 * (size_t)p0]; X[1] = pts[3 * (size_t)p0 + 1]; X[2] = pts[3 * (size_t)p0 + 2];
        }
        if (e1 < ee) { pn = cm_pt[e1]; zn = uv2[e1]; }
    }
    for (int e = eb + t; e < ee; e += NT) {
        const bool hn = e + NT < ee, hnn = e + 2 * NT < ee;
        double Xn[3] = {0.0, 0.0, 0.0};
        if (hn) { Xn[0] = pts[3 * (size_t)pn]; Xn[1] = pts[3 * (size_t)pn + 1]; Xn[2] = pts[3 * (size_t)pn + 2]; }
        if (hnn) { pnn = cm_pt[e + 2 * NT]; znn = uv2[e + 2 * NT]; }
        const double uvo[2] = {z.x, z.y};
        double r[2], Jc[2][D], Jp[2][3];
        eval_obs<M, true>(camv, X, ppc, uvo, r, Jc, Jp);
        const double sw = huber_weight_sqrt(r[0] * r[0] + r[1] * r[1], delta);
#pragma unroll
        for (int a = 0; a < D; ++a) { Jc[0][a] *= sw; Jc[1][a] *= sw; }
        r[0] *= sw; r[1] *= sw;
        int m = 0;
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
            for (int b = a; b < D; ++b, ++m) acc[m] += Jc[0][a] * Jc[0][b] + Jc[1][a] * Jc[1][b];
#pragma unroll
        for (int a = 0; a < D; ++a) acc[NU + a] -= Jc[0][a] * r[0] + Jc[1][a] * r[1];
        X[0] = Xn[0]; X[1] = Xn[1]; X[2] = Xn[2];
        z = zn; pn = pnn; zn = znn;
    }
#pragma unroll
    for (int m = 0; m < NE; ++m) {
        const double v = wave_sum(acc[m]);
        if (lane == 0) red[wv][m] = v;
    }
    __syncthreads();
    for (int m = t; m < NE; m += NT) {
        double s = red[0][m];
#pragma unroll
        for (int w = 1; w < NW; ++w) s += red[w][m];
        if (m < NU) {
            int a = 0, rem = m;
            while (rem >= D - a) { rem -= D - a; ++a; }
            const int b = a + rem;
            U[(size_t)c * D * D + a * D + b] = s;
            U[(size_t)c * D * D + b * D + a] = s;
        } else {
            gc[(size_t)c * D + (m - NU)] = s;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------
// per-trial point preparation
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_point_prep(int Pl, const double* __restrict__ V, const double* __restrict__ gp,
                                                         double f, double cmin, double cmax, double* __restrict__ Vinv,
                                                         double* __restrict__ y, int* __restrict__ flags,
                                                         int* __restrict__ status, const double* __restrict__ R,
                                                         double* __restrict__ Mp) {
    // R non-null (a retried trial on the symmetric records, see PointPrep): M_p = R^T V'^-1 R (packed sym) and
    // z'_p = R^T y'_p into y; else y'_p = V'^-1 g_p (global positioning's re-prep, points-only solves)
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < 4) status[threadIdx.x] = 0;  // the CG status word of this solve
    if (p >= Pl) return;
    double s[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k] = V[6 * (size_t)p + k];
    s[0] = clampd(s[0], cmin, cmax) * f;
    s[3] = clampd(s[3], cmin, cmax) * f;
    s[5] = clampd(s[5], cmin, cmax) * f;
    double o[6];
    if (!spd3_inverse(s, o)) {
        atomicOr(flags, 1);
#pragma unroll
        for (int k = 0; k < 6; ++k) o[k] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) Vinv[6 * (size_t)p + k] = o[k];
    const double g0 = gp[3 * (size_t)p], g1 = gp[3 * (size_t)p + 1], g2 = gp[3 * (size_t)p + 2];
    const double y0 = o[0] * g0 + o[1] * g1 + o[2] * g2;
    const double y1 = o[1] * g0 + o[3] * g1 + o[4] * g2;
    const double y2 = o[2] * g0 + o[4] * g1 + o[5] * g2;
    if (!R) {
        y[3 * (size_t)p + 0] = y0;
        y[3 * (size_t)p + 1] = y1;
        y[3 * (size_t)p + 2] = y2;
        return;
    }
    const double* r = R + 6 * (size_t)p;
    const double r00 = r[0], r10 = r[1], r20 = r[2], r11 = r[3], r21 = r[4], r22 = r[5];
    // T = V'^-1 R (columns of R: (r00, r10, r20), (0, r11, r21), (0, 0, r22))
    const double Rm[3][3] = {{r00, 0.0, 0.0}, {r10, r11, 0.0}, {r20, r21, r22}};
    const double O[3][3] = {{o[0], o[1], o[2]}, {o[1], o[3], o[4]}, {o[2], o[4], o[5]}};
    double T[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) T[a][c] = O[a][0] * Rm[0][c] + O[a][1] * Rm[1][c] + O[a][2] * Rm[2][c];
    double Mq[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) Mq[a][c] = Rm[0][a] * T[0][c] + Rm[1][a] * T[1][c] + Rm[2][a] * T[2][c];
    double* mo = Mp + 6 * (size_t)p;
    mo[0] = Mq[0][0]; mo[1] = Mq[0][1]; mo[2] = Mq[0][2]; mo[3] = Mq[1][1]; mo[4] = Mq[1][2]; mo[5] = Mq[2][2];
    y[3 * (size_t)p + 0] = r00 * y0 + r10 * y1 + r20 * y2;
    y[3 * (size_t)p + 1] = r11 * y1 + r21 * y2;
    y[3 * (size_t)p + 2] = r22 * y2;
}

// ------------------------------------------------------------------------------------------------------------
// Schur complement: one workgroup per (camera row i, chunk of its upper blocks); the chunk of S's row lives in LDS.
// A group of D lanes owns one of camera i's observations o (64/D observations in flight per wave); lane b of the
// group owns column b.  The group stages the rows of its own record (row b per lane, shared through LDS) -- the BA's
// symmetric record Y_o as it is on the first trial, Y_o M_p on a retried one (PointPrep), global positioning's
// W^_o = W_o V_p^-1 -- then walks the upper partners q of track p -- tracks are sorted by camera at create, so they
// are exactly [ustart[o], end) -- and adds column b of -Y^_o Y_q^T into slot(cam[q]) with LDS f64 atomics
// (ds_add_f64).  b_i -= Y_o z_p (z_p, z'_p: PointPrep) alongside.  Each camera's
// observation list is in point order cut into chunks sorted by partner count (create: the groups of a wave stay
// balanced, and the rows walk the tracks in step).  The kernel is bound by the
// chain of dependent loads per round, not by bytes (cache-resident partner data: no faster): every own-observation
// index comes from one descriptor {o, p, partner range} prefetched a round ahead.  Measured and rejected: a
// precomputed per-pair block position (36 MB streamed per trial, slower than cam[] from cache + an LDS lookup).
// ------------------------------------------------------------------------------------------------------------
// LDS strides of k_schur.  The D groups of a wave add into D different blocks at the same (row, column): with a
// block stride that is a multiple of the 64-bank period (D*D = 64 doubles = 512 B for D = 8) every group lands on the
// same banks (8-way conflicts, SQ_LDS_BANK_CONFLICT ~1.6x the busy cycles); 8 extra doubles spread the groups over 4
// bank quarters.  The W^ staging of each group gets an odd stride for the same reason.
__host__ __device__ constexpr int schur_bs(int D) { return D * D + ((D * D) % 16 == 0 ? 8 : 0); }
__host__ __device__ constexpr int schur_ws(int D) { return D * 4 + 1; }

// Column cb of W_o: the BA stores W [o][3][D]; global positioning (GPW) stores the 32-byte record {u, beta^2} of
// W_o = -beta^2 (I - u u^T) (u = a / sqrt(h_ss), 0 for a fixed scale; symmetric, D = 3) written by k_gp_prep_points.
template <int D, bool GPW>
__device__ __forceinline__ void load_wcol(const double* __restrict__ W, int o, int cb, double& w0, double& w1, double& w2) {
    if constexpr (GPW) {
        const double4 r = reinterpret_cast<const double4*>(W)[o];
        const double uc = cb == 0 ? r.x : (cb == 1 ? r.y : r.z);
        w0 = -r.w * ((cb == 0 ? 1.0 : 0.0) - r.x * uc);
        w1 = -r.w * ((cb == 1 ? 1.0 : 0.0) - r.y * uc);
        w2 = -r.w * ((cb == 2 ? 1.0 : 0.0) - r.z * uc);
    } else {
        const double* wo = W + (size_t)o * D * 3 + cb;
        w0 = wo[0]; w1 = wo[D]; w2 = wo[2 * D];
    }
}

// SCHUR_PROBE (timing-only builds for the floor model of DESIGN.md section 8, tools/schur_variants.sh; wrong results):
//   1  the partner products summed in a register instead of the LDS atomics (gathers + FMAs, no ds_add_f64)
//   2  the partner walk's loads only (records + camera indices; no slot lookup, no FMA, no LDS add)
//   3  no partner-record gathers: the own record stands in for the partner's (camera index, slot lookup, FMAs and
//      LDS adds as usual)
#ifndef SCHUR_PROBE
#define SCHUR_PROBE 0
#endif
template <int D, int WAVES, bool GPW = false, bool RETRY = false, bool ORD = false>
__global__ __launch_bounds__(WAVES * 64, SCHUR_MINW) void k_schur(const int4* __restrict__ work, const int* __restrict__ row_ptr,
                                                      const int* __restrict__ col, int C, const int* __restrict__ cam_ptr,
                                                      const int* __restrict__ cam_obs, const int* __restrict__ ptl,
                                                      const int* __restrict__ pt_ptr, const int* __restrict__ ustart,
                                                      const int4* __restrict__ sdesc,
                                                      const int* __restrict__ cam, const double* __restrict__ W,
                                                      const double* __restrict__ Vinv, const double* __restrict__ y,
                                                      const double* __restrict__ U, const double* __restrict__ gc, double f,
                                                      double cmin, double cmax, int add_diag, double* __restrict__ S,
                                                      double* __restrict__ b, long long* stp) {
    const StampScope stamp_(stp);
    constexpr int DD = D * D;
    constexpr int BS = schur_bs(D);  // LDS stride of an accumulated block (padded off the 64-bank period)
    constexpr int WS = schur_ws(D);  // LDS stride of a group's W^ staging
    constexpr int NG = 64 / D;  // observation groups per wave
    constexpr int NT = WAVES * 64;
    extern __shared__ __attribute__((aligned(16))) double sh[];
    __shared__ int rnd_sh[ORD ? 2 * WAVES : 1];  // (ORD) partner-round counts of the waves, by own-round parity
    const int4 wk = work[blockIdx.x];
    const int i = wk.x, kb = wk.y, ke = wk.z, nb = ke - kb;
    double* acc = sh;
    double* wsh = acc + (size_t)nb * BS;           // [WAVES][NG][WS]  W^ rows ([D][4], padded group stride)
    double* bacc = wsh + (size_t)WAVES * NG * WS;  // [D]
    int* slot = reinterpret_cast<int*>(bacc + D + 12);  // [C]
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    for (int k = t; k < nb * BS; k += NT) acc[k] = 0.0;
    for (int k = t; k < C; k += NT) slot[k] = -1;
    if (t < D) bacc[t] = 0.0;
    __syncthreads();
    for (int e = kb + t; e < ke; e += NT) slot[col[e]] = e - kb;
    __syncthreads();
    const bool diag_chunk = (kb == row_ptr[i]);
    const int g = lane / D, cb = lane - g * D;
    const bool active = g < NG;
    double* my_wh = wsh + (size_t)(wv * NG + (active ? g : 0)) * WS;
    double breg = 0.0;
    double probe_sum = 0.0;  // (SCHUR_PROBE 1 / 2: keeps the probed work alive)
    const int ob = cam_ptr[i], oe = cam_ptr[i + 1];
    // per own observation one descriptor {o, p, partner begin, partner end}: one load gives every index, and the next
    // round's descriptor is loaded while the current round runs (the round chain is latency-bound, not byte-bound)
    int4 dnext = make_int4(0, 0, 0, 0);
    constexpr int UP = ORD ? SCHUR_UP_DET : SCHUR_UP;  // partners in flight per group
    {
        const int e0 = ob + wv * NG + g;
        if (active && e0 < oe) dnext = sdesc[e0];
        if constexpr (ORD) {  // the first own round's partner-round count of each wave
            const int n0 = (active && e0 < oe) ? dnext.w - dnext.z : 0;
            int nr0 = 0;
            while (__builtin_amdgcn_ballot_w64(nr0 * UP < n0) != 0) ++nr0;
            if (lane == 0) rnd_sh[wv] = nr0;
            __syncthreads();
        }
    }
    // ORD (deterministic mode): every wave runs the same number of rounds (own observations, and per own round the
    // workgroup's partner rounds), and in each partner round the waves make their LDS adds in turn (wave 0 first, a
    // barrier between turns), so each slot sees its additions in a fixed order
    // -- lanes of one wave adding into one address within one instruction are ordered by the hardware -- while the
    // waves' gathers stay in flight together
    const int nround = ORD ? (oe - ob + WAVES * NG - 1) / (WAVES * NG) : 0;
    for (int base = ob + wv * NG, rd = 0; ORD ? rd < nround : base < oe; base += WAVES * NG, ++rd) {
        const int e = base + g;
        const bool has = active && e < oe;
        const int4 dcur = dnext;
        {
            const int en = e + WAVES * NG;
            if (active && en < oe) dnext = sdesc[en];
        }
        const int qs = has ? dcur.z : 0, qe = has ? dcur.w : 0;
        const int n = qe - qs;
        // issue order = wait order (vmcnt retires in order): the own record first, then the first UP partner records,
        // so the W^ staging waits only for the own record while the partner loads stay in flight
        double w0 = 0.0, w1 = 0.0, w2 = 0.0, v00 = 0.0, v01 = 0.0, v02 = 0.0, v11 = 0.0, v12 = 0.0, v22 = 0.0;
        if (has) {
            if constexpr (GPW || RETRY) {  // V^-1 (global positioning) or M_p (a retried trial on the Y records)
                const double* vi = Vinv + 6 * (size_t)dcur.y;
                v00 = vi[0]; v01 = vi[1]; v02 = vi[2]; v11 = vi[3]; v12 = vi[4]; v22 = vi[5];
            }
            load_wcol<D, GPW>(W, dcur.x, cb, w0, w1, w2);
        }
        double x[UP][3];
        int cj[UP];
#pragma unroll
        for (int u = 0; u < UP; ++u) {
            cj[u] = -1;
            if (u < n) {
                if (SCHUR_PROBE == 3) { x[u][0] = w0; x[u][1] = w1; x[u][2] = w2; }
                else load_wcol<D, GPW>(W, qs + u, cb, x[u][0], x[u][1], x[u][2]);
                cj[u] = cam[qs + u];
            }
        }
        if (has) {
            // staged negated: the partner products below then come out with the sign S_ij needs (sign-symmetric
            // rounding: bitwise the negation of the positive products) and need no v_xor per row
            if constexpr (GPW || RETRY) {
                my_wh[cb * 4 + 0] = -(w0 * v00 + w1 * v01 + w2 * v02);
                my_wh[cb * 4 + 1] = -(w0 * v01 + w1 * v11 + w2 * v12);
                my_wh[cb * 4 + 2] = -(w0 * v02 + w1 * v12 + w2 * v22);
            } else {  // the first trial on the Y records: S_ij -= Y_o Y_q^T directly
                my_wh[cb * 4 + 0] = -w0;
                my_wh[cb * 4 + 1] = -w1;
                my_wh[cb * 4 + 2] = -w2;
            }
            if (diag_chunk) {
                const double* yp = y + 3 * (size_t)dcur.y;
                breg -= w0 * yp[0] + w1 * yp[1] + w2 * yp[2];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        double wh[D][3];
        if (has) {
#pragma unroll
            for (int a2 = 0; a2 < D; ++a2) {
                wh[a2][0] = my_wh[a2 * 4 + 0];
                wh[a2][1] = my_wh[a2 * 4 + 1];
                wh[a2][2] = my_wh[a2 * 4 + 2];
            }
        }
        // rounds while any lane of the wave has partners left: a ballot (scalar compare) instead of a shuffle max of n,
        // which cost six ds_bpermute per own-observation round on the LDS pipe the accumulation already saturates
        // ORD: the workgroup's partner-round count, the most any wave needs.  Each wave writes the next own round's
        // count (from the prefetched descriptor, by round parity) before this round's last barrier: the readers of
        // that buffer slot, two rounds back, have all passed the previous round's last barrier.
        int nrd = 0;
        if constexpr (ORD) {
#pragma unroll
            for (int w2 = 0; w2 < WAVES; ++w2) nrd = max(nrd, rnd_sh[(rd & 1) * WAVES + w2]);
            const int en = e + WAVES * NG;
            const int nn = (active && en < oe) ? dnext.w - dnext.z : 0;
            int nrn = 0;
            while (__builtin_amdgcn_ballot_w64(nrn * UP < nn) != 0) ++nrn;
            if (lane == 0) rnd_sh[((rd + 1) & 1) * WAVES + wv] = nrn;
        }
        for (int k0 = 0; ORD ? k0 < nrd * UP : __builtin_amdgcn_ballot_w64(k0 < n) != 0; k0 += UP) {
            if (k0 > 0) {
#pragma unroll
                for (int u = 0; u < UP; ++u) {
                    cj[u] = -1;
                    if (k0 + u < n) {
                        const int q = qs + k0 + u;
                        if (SCHUR_PROBE == 3) { x[u][0] = w0 + k0; x[u][1] = w1; x[u][2] = w2; }
                        else load_wcol<D, GPW>(W, q, cb, x[u][0], x[u][1], x[u][2]);
                        cj[u] = cam[q];
                    }
                }
            }
#if SCHUR_PROBE == 2
#pragma unroll
            for (int u = 0; u < UP; ++u)
                if (cj[u] >= 0) probe_sum += x[u][0] + x[u][1] + x[u][2] + (double)cj[u];
            continue;
#endif
#if SCHUR_SLOTPRE
            // every slot of the round looked up before the first ds_add_f64: one LDS wait per round instead of one
            // per partner (a slot read issued behind the previous partner's adds waits for them to retire)
            int slv[UP];
#pragma unroll
            for (int u = 0; u < UP; ++u) slv[u] = slot[cj[u] >= 0 ? cj[u] : 0];
            __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0) (vmcnt, expcnt unconstrained): all slots read
            __builtin_amdgcn_sched_barrier(0);
#endif
            // ORD: wave w adds between the w-th and the (w+1)-th of the round's WAVES barriers
            if constexpr (ORD)
                for (int k = 0; k < wv; ++k) __syncthreads();
#pragma unroll
            for (int u = 0; u < UP; ++u) {
                if (cj[u] >= 0) {
#if SCHUR_SLOTPRE
                    const int sl = slv[u];
#else
                    const int sl = slot[cj[u]];
#endif
                    if (sl >= 0) {
                        double* dst = acc + (size_t)sl * BS + cb;
                        const double y0 = x[u][0], y1 = x[u][1], y2 = x[u][2];
#pragma unroll
                        for (int a2 = 0; a2 < D; ++a2) {
                            if (SCHUR_PROBE == 1) probe_sum += wh[a2][0] * y0 + wh[a2][1] * y1 + wh[a2][2] * y2;
                            else atomicAdd(dst + a2 * D, wh[a2][0] * y0 + wh[a2][1] * y1 + wh[a2][2] * y2);
                        }
                    }
                }
            }
            if constexpr (ORD)
                for (int k = wv; k < WAVES; ++k) __syncthreads();
        }
        if (ORD && nrd == 0) __syncthreads();  // (a round without partners: its one barrier)
        __builtin_amdgcn_wave_barrier();
    }
    if constexpr (ORD)
        for (int k = 0; k < wv; ++k) __syncthreads();
    if (diag_chunk && active) atomicAdd(bacc + cb, breg);
    if constexpr (ORD)
        for (int k = wv; k < WAVES; ++k) __syncthreads();
    if (SCHUR_PROBE != 0 && probe_sum == 1.2345e-300) acc[0] = probe_sum;  // (never true: a use of the probed sums)
    __syncthreads();
    double* Sout = S + (size_t)kb * DD;
    const double* Ui = U + (size_t)i * DD;
    for (int k = t; k < nb * DD; k += NT) {
        double v = acc[(k / DD) * BS + k % DD];
        if (diag_chunk && add_diag && k < DD) {
            const int a2 = k / D, bb = k % D;
            double u = Ui[k];
            if (a2 == bb) u = clampd(u, cmin, cmax) * f;
            v += u;
        }
#if SCHUR_NT_STORE
        __builtin_nontemporal_store(v, Sout + k);
#else
        Sout[k] = v;
#endif
    }
    if (diag_chunk && t < D) b[(size_t)i * D + t] = (add_diag ? gc[(size_t)i * D + t] : 0.0) + bacc[t];
}

// ------------------------------------------------------------------------------------------------------------
// PCG on the reduced camera system
// ------------------------------------------------------------------------------------------------------------
// One wave per camera, in registers: lane r holds row r of S_ii and factors it right-looking (pivot and column
// entries broadcast with readlane), so S_ii = L L^T costs D short steps instead of a lane-0 loop over LDS; lane c
// then forms column c of L^-1 by forward substitution, and r0 = L^-1 b, zero p/x/s.  Same operations in the same
// order as the left-looking entry-wise loops (a[c] -= L[r][j] L[c][j] for j ascending, L[r][c] = s / L[c][c],
// I[r][c] = -sum_k L[r][k] I[k][c] / L[r][r]).
// U / g_c (`Ul` non-null): k_schur built S_ii and b_i without the camera terms (k_lin_cams ran beside it on another
// stream), so they are added here -- S_ii += U_i with the diagonal clamped and scaled by the damping factor, b_i =
// g_c + b_i, the same single additions k_schur makes -- and the completed block and right-hand side are written back.
// One camera's factorization on one wave (k_cg_factor's work for camera i).  On return lane r < D holds row r of L_i in
// a[] (zero above the diagonal) and column r of L_i^-1 in x[], and r0 = (L_i^-1 b_i)[lane] (0 when S_ii is not positive
// definite: *ok false, the CG status raised to 2).
template <int D>
__device__ __forceinline__ void factor_camera(int i, int lane, const int* __restrict__ row_ptr, double* __restrict__ S,
                                              double* __restrict__ b, double* __restrict__ Lf, double* __restrict__ Li,
                                              CgBufs& cg, const double* __restrict__ Ul, const double* __restrict__ gcl,
                                              double f, double cmin, double cmax, double (&a)[D], double (&x)[D],
                                              double& r0out, bool& okout) {
    constexpr int DD = D * D;
    const int rl = min(lane, D - 1);
    double* blk = S + (size_t)row_ptr[i] * DD;
#pragma unroll
    for (int c = 0; c < D; ++c) a[c] = blk[rl * D + c];
    double bl = b[(size_t)i * D + rl];
    if (Ul) {
        const double* Ui = Ul + (size_t)i * DD + rl * D;
#pragma unroll
        for (int c = 0; c < D; ++c) {
            double u = Ui[c];
            if (c == rl) u = clampd(u, cmin, cmax) * f;
            a[c] += u;
        }
        bl = gcl[(size_t)i * D + rl] + bl;
        if (lane < D) {
#pragma unroll
            for (int c = 0; c < D; ++c) blk[rl * D + c] = a[c];
            b[(size_t)i * D + rl] = bl;
        }
    }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        double piv = readlane_d(a[j], j);
        if (!(piv > 0.0)) { ok = false; piv = 1.0; }
        const double ljj = sqrt(piv);
        const double lrj = (lane == j) ? ljj : ((lane > j) ? a[j] / ljj : 0.0);
        a[j] = lrj;
#pragma unroll
        for (int c = j + 1; c < D; ++c) {
            const double lcj = readlane_d(lrj, c);
            if (lane >= c) a[c] -= lrj * lcj;
        }
    }
#pragma unroll
    for (int c = 0; c < D; ++c)
        if (c > lane) a[c] = 0.0;
    // column `lane` of L^-1: x[r] = (delta_rc - sum_{k<r} L[r][k] x[k]) / L[r][r]
#pragma unroll
    for (int r = 0; r < D; ++r) {
        double s = 0.0;  // (x[k] = 0 for k < lane: those terms leave s unchanged)
#pragma unroll
        for (int k = 0; k < r; ++k) s -= readlane_d(a[k], r) * x[k];
        x[r] = (r >= lane) ? ((r == lane) ? 1.0 / readlane_d(a[r], r) : s / readlane_d(a[r], r)) : 0.0;
    }
    if (!ok && lane == 0) atomicMax(cg.status, 2);
    if (lane < D) {
#pragma unroll
        for (int c = 0; c < D; ++c) {
            Lf[(size_t)i * DD + lane * D + c] = a[c];
            Li[(size_t)i * DD + c * D + lane] = ok ? x[c] : 0.0;
        }
    }
    // r0 = L^-1 b: row a of L^-1 is (x[a] of lanes 0..a)
    double r0 = 0.0;
#pragma unroll
    for (int aa = 0; aa < D; ++aa) {
        double sacc = 0.0;
#pragma unroll
        for (int k = 0; k <= aa; ++k) sacc += readlane_d(x[aa], k) * readlane_d(bl, k);
        if (lane == aa) r0 = sacc;
    }
    if (lane < D) {
        const size_t idx = (size_t)i * D + lane;
        cg.r[0][idx] = ok ? r0 : 0.0;
        cg.r[1][idx] = 0.0;
        cg.w[0][idx] = 0.0; cg.w[1][idx] = 0.0;
        cg.s[0][idx] = 0.0; cg.s[1][idx] = 0.0;
        cg.p[idx] = 0.0; cg.x[idx] = 0.0;
    }
    okout = ok;
    r0out = ok ? r0 : 0.0;
}

template <int D>
__global__ __launch_bounds__(kThreads) void k_cg_factor(int C, const int* __restrict__ row_ptr, double* __restrict__ S,
                                                        double* __restrict__ b, double* __restrict__ Lf,
                                                        double* __restrict__ Li, CgBufs cg, const double* __restrict__ Ul,
                                                        const double* __restrict__ gcl, double f, double cmin, double cmax,
                                                        long long* stp = nullptr) {
    const StampScope stamp_(stp);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i = blockIdx.x * kWaves + wv;
    if (i >= C) return;
    double a[D], x[D], r0;
    bool ok;
    factor_camera<D>(i, lane, row_ptr, S, b, Lf, Li, cg, Ul, gcl, f, cmin, cmax, a, x, r0, ok);
}

// k_cg_factor and k_tl_basis in one launch (round 6), for the persistent CG (k_tl_cgp): the waves take the cameras in
// cluster order -- workgroup g the four cameras k_tl_cgp's workgroup g holds -- and after its factorization each wave
// forms its camera's basis (k_tl_basis's tl_basis_entry: lane k < D + 1 the column k of G_i, Z~_i = L_i^T G_i, the
// restriction partial Z~_i[:,k]^T r0_i) from the factor still in its registers.  The restriction of r0 is summed per
// cluster run of the workgroup (rows in order) into slots 3..11 of the run records `runs` (k_tl_cgp's parity-1 records,
// which it sums per cluster in run order, det_cluster_sums) instead of k_tl_basis's per-cluster tl.Rc: one launch and
// its gap less per solve.
template <int D>
__global__ __launch_bounds__(kThreads) void k_cg_factor_basis(int C, const int* __restrict__ row_ptr, double* __restrict__ S,
                                                              double* __restrict__ b, double* __restrict__ Lf,
                                                              double* __restrict__ Li, CgBufs cg,
                                                              const double* __restrict__ Ul, const double* __restrict__ gcl,
                                                              double f, double cmin, double cmax,
                                                              const double* __restrict__ cams, TlBufs tl,
                                                              double* __restrict__ runs, long long* stp = nullptr) {
    static_assert(kWaves == kCgpRows, "k_cg_factor_basis's workgroups are k_tl_cgp's");
    const StampScope stamp_(stp);
    constexpr int MC = D + 1, ST = D + 1;  // (a BA camera row: pose [t, q] and D - 6 intrinsics)
    __shared__ double prt[kWaves][MC];
    __shared__ int pcl[kWaves];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int pos = blockIdx.x * kWaves + wv;
    const bool has = pos < C;
    const int i = has ? tl.cl_cams[pos] : 0;
    double rr = 0.0;
    if (has) {
        double a[D], x[D], r0;
        bool ok;
        factor_camera<D>(i, lane, row_ptr, S, b, Lf, Li, cg, Ul, gcl, f, cmin, cmax, a, x, r0, ok);
        const int k = min(lane, MC - 1);
        double col[D];
        basis_column<D>(k, cams + (size_t)i * ST, tl.alone[i] != 0, col);
        const bool st = lane < MC;
        const int cp = tl.cpos[i];
#pragma unroll
        for (int aa = 0; aa < D; ++aa) {
            double sz = 0.0;  // Z~[aa][k] = sum_{l >= aa} L[l][aa] G[l][k] (tl_basis_entry's order)
#pragma unroll
            for (int l = aa; l < D; ++l) sz += readlane_d(a[aa], l) * col[l];
            if (st) {
                tl.Zt[((size_t)i * D + aa) * MC + k] = sz;
                if (tl.Gb) tl.Gb[((size_t)i * D + aa) * MC + k] = col[aa];
                tl.Ztc[((size_t)cp * D + aa) * MC + k] = sz;
            }
            rr += sz * readlane_d(r0, aa);
        }
        if (st) tl.rowR[(size_t)cp * MC + k] = rr;
        if (lane < D) tl.vc[(size_t)cp * D + lane] = r0;
    }
    if (lane < MC) prt[wv][lane] = rr;
    if (lane == 0) pcl[wv] = has ? tl.clab[i] : -1;
    __syncthreads();
    if (has && (wv == 0 || pcl[wv - 1] != pcl[wv]) && lane < MC) {
        double v = prt[wv][lane];
        for (int r2 = wv + 1; r2 < kWaves && pcl[r2] == pcl[wv]; ++r2) v += prt[r2][lane];
        runs[(size_t)pos * 12 + 3 + lane] = v;
    }
}

// One wave per scale_nb(D) upper blocks: S~_ij = L_i^-1 S_ij L_j^-T (diagonal blocks -> I).  Off-diagonal blocks are also
// written, padded to DP = D + (D & 1) columns, into the row-contiguous neighbour copy Sn: S~_ij at slot pos_up[e]
// of row i and S~_ij^T at slot pos_lo[e] of row j, so the CG iteration reads every row's blocks as one
// contiguous, 16-byte-coalesced stream.
// Blocks per wave: their loads are issued together (one memory latency per NB blocks); fewer for large D so that the
// staging (3 NB D^2 doubles per wave) leaves several workgroups per CU.
__host__ __device__ constexpr int scale_nb(int D) { return D * D <= 64 ? 4 : (D * D <= 144 ? 2 : 1); }
template <int D>
__global__ __launch_bounds__(kThreads) void k_cg_scale(int nnzb, const int* __restrict__ blk_row, const int* __restrict__ col,
                                                       const int* __restrict__ row_ptr, const int* __restrict__ pos_up,
                                                       const int* __restrict__ pos_lo, const double* __restrict__ Li,
                                                       double* __restrict__ S, double* __restrict__ Sn, int keep_S) {
    constexpr int DD = D * D;
    constexpr int DP = D + (D & 1);
    constexpr int NB = scale_nb(D);
    constexpr int UL = (DD + 63) / 64;  // elements of a block per lane
    __shared__ double T[kWaves][DD];
    __shared__ double Sb[kWaves][NB][DD];
    __shared__ double La[kWaves][NB][DD];
    __shared__ double Lb[kWaves][NB][DD];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int e0 = (blockIdx.x * kWaves + wv) * NB;
    if (e0 >= nnzb) return;
    // every block of the wave and both factors' inverses staged together (all loads in flight at once; indices past
    // the end clamped to the last block, whose products are then not stored)
    int ei[NB], ii[NB], jj[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        ei[u] = min(e0 + u, nnzb - 1);
        ii[u] = blk_row[ei[u]];
        jj[u] = col[ei[u]];
    }
    double sv[NB][UL], av[NB][UL], bv[NB][UL];
#pragma unroll
    for (int u = 0; u < NB; ++u)
#pragma unroll
        for (int q = 0; q < UL; ++q) {
            const int k = min(lane + 64 * q, DD - 1);
            sv[u][q] = S[(size_t)ei[u] * DD + k];
            av[u][q] = Li[(size_t)ii[u] * DD + k];
            bv[u][q] = Li[(size_t)jj[u] * DD + k];
        }
#pragma unroll
    for (int u = 0; u < NB; ++u)
#pragma unroll
        for (int q = 0; q < UL; ++q) {
            const int k = lane + 64 * q;
            if (k < DD) { Sb[wv][u][k] = sv[u][q]; La[wv][u][k] = av[u][q]; Lb[wv][u][k] = bv[u][q]; }
        }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        const int e = e0 + u;
        if (e >= nnzb) break;
        const int i = ii[u];
        double* blk = S + (size_t)e * DD;
        if (e == row_ptr[i]) {
            if (keep_S)
                for (int k = lane; k < DD; k += 64) blk[k] = (k / D == k % D) ? 1.0 : 0.0;
            continue;
        }
        // same products in the same order as entry-wise loops over global memory
        for (int k = lane; k < DD; k += 64) {
            const int a = k / D, bb = k % D;
            double s = 0.0;
            for (int m = 0; m <= a; ++m) s += La[wv][u][a * D + m] * Sb[wv][u][m * D + bb];
            T[wv][k] = s;
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        double* up = Sn + (size_t)pos_up[e] * D * DP;
        double* lo = Sn + (size_t)pos_lo[e] * D * DP;
        for (int k = lane; k < D * DP; k += 64) {
            const int a = k / DP, bb = k % DP;
            double v = 0.0;
            if (bb < D) {
                for (int m = 0; m <= bb; ++m) v += T[wv][a * D + m] * Lb[wv][u][bb * D + m];
                if (keep_S) blk[a * D + bb] = v;  // the scaled upper S is only read by the debug getters
                Sb[wv][u][a * D + bb] = v;
            }
            up[k] = v;
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        // transpose: lo[a][bb] = S~_ij[bb][a]
        for (int k = lane; k < D * DP; k += 64) {
            const int a = k / DP, bb = k % DP;
            lo[k] = (bb < D) ? Sb[wv][u][bb * D + a] : 0.0;
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
}

// CG iteration kernel `it` (Chronopoulos-Gear on S~; diagonal blocks of S~ are I).  it = 0 computes w0 = S~ r0 and
// the first dots.  it >= 1 performs recurrence step i = it-1: reads dots_i (per-row partials of kernel it-1), decides
// convergence on the true residual rho_i = ||L r~_i||^2 <= tol^2 ||b||^2, then for its camera row
//   p = r + beta p; s = w + beta s; x += alpha p; r' = r - alpha s; w' = S~ r'
// where every neighbour's r'_j is recomputed from its previous-iteration (r, w, s), so one iteration = ONE launch.
// One 512-thread workgroup per camera row.  The row's neighbour blocks are contiguous in Sn (padded D x DP); lane l of
// a wave owns 16-byte piece (l mod PPB) of block (l / PPB): every load instruction is a contiguous 1 KiB stream.
// Loads that do not depend on alpha / beta (blocks, neighbour vectors, partials, history, own row) are issued first.
// Recurrence scalars for step i = it-1: ONE wave sums the per-row partial dots of launch it-1 in a fixed order
// (16 independent loads in flight per lane per quantity, butterfly across lanes; no barriers), tests convergence on the
// true residual and publishes {alpha, beta, flag} (+ history) for k_cg_iter.
__global__ __launch_bounds__(64) void k_cg_dots(int it, int C, int maxit, double tol2_rel, CgBufs cg) {
    const int lane = threadIdx.x;
    if (cg.status[0] != 0) return;
    const int i = it - 1;
    const double* P0 = cg.part[it & 1 ? 0 : 1];
    const double* P1 = P0 + C;
    const double* P2 = P1 + C;
    double g0 = 0.0, g1 = 0.0, g2 = 0.0;
    for (int base = lane; base < C; base += 64 * 16) {
        double a0[16], a1[16], a2[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int k = base + 64 * u;
            const bool ok = k < C;
            a0[u] = ok ? P0[k] : 0.0;
            a1[u] = ok ? P1[k] : 0.0;
            a2[u] = ok ? P2[k] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) { g0 += a0[u]; g1 += a1[u]; g2 += a2[u]; }
    }
    g0 = wave_sum(g0); g1 = wave_sum(g1); g2 = wave_sum(g2);
    const double h_alpha = (i >= 1) ? cg.hist[2 * (i - 1)] : 1.0;
    const double h_gam = (i >= 1) ? cg.hist[2 * (i - 1) + 1] : 1.0;
    const double h_bb = cg.hist[2 * (maxit + 1)];
    if (lane == 0) {
        const double gam = g0, del = g1, rho = g2;
        const double bb = (i == 0) ? rho : h_bb;
        double flag = 0.0, al = 0.0, be = 0.0;
        if (rho <= tol2_rel * bb || i >= maxit) {
            flag = 1.0;
            cg.status[0] = 1; cg.status[1] = i;
        } else {
            double den;
            if (i == 0) { be = 0.0; den = del; }
            else {
                be = gam / h_gam;
                den = del - be * gam / h_alpha;
            }
            if (!(den > 0.0)) {
                flag = 2.0;
                cg.status[0] = 2; cg.status[1] = i;
            } else {
                al = gam / den;
                cg.hist[2 * i] = al;
                cg.hist[2 * i + 1] = gam;
                if (i == 0) cg.hist[2 * (maxit + 1)] = bb;
            }
        }
        cg.scal[0] = al; cg.scal[1] = be; cg.scal[2] = flag;
    }
}

template <int D>
__global__ __launch_bounds__(kCgThreads) void k_cg_iter(int it, int C, int maxit, double tol2_rel,
                                                        const int* __restrict__ nbr_ptr, const int* __restrict__ nbr_j,
                                                        const double* __restrict__ Sn, const double* __restrict__ Lf,
                                                        CgBufs cg) {
    using G = CgGeom<D>;
    constexpr int DD = D * D;
    constexpr int DP = G::DP, HP = G::HP, PPB = G::PPB, BPW = G::BPW, PPL = G::PPL, BPR = G::BPR;
    __shared__ double red[kCgWaves][BPW][PPB];
    __shared__ double rsh[D];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int row = blockIdx.x;
    const int pin = (it + 1) & 1;
    const int pout = it & 1;
    const double* r_old = cg.r[it == 0 ? 0 : pin];
    const double* w_old = cg.w[pin];
    const double* s_old = cg.s[pout];
    const int bw = (PPB <= 64) ? lane / PPB : 0;     // block slot within the wave
    const int pc0 = (PPB <= 64) ? lane - bw * PPB : lane;
    const bool lane_on = (PPB <= 64) ? (bw < BPW) : true;
    const int slot = wv * BPW + bw;                  // block slot within the round
    // ======== phase 1: loads independent of alpha / beta ========
    const int status = cg.status[0];
    const int n0 = nbr_ptr[row], n1 = nbr_ptr[row + 1];
    double acc[PPL];
#pragma unroll
    for (int m = 0; m < PPL; ++m) acc[m] = 0.0;
    // first round prefetch
    double s0[PPL], s1[PPL], xr0[PPL], xr1[PPL], xw0[PPL], xw1[PPL], xs0[PPL], xs1[PPL];
    const int nfirst = n0 + slot;
    const bool have = lane_on && nfirst < n1;
    auto load_piece = [&](int nn, int m, double& a0, double& a1, double& r0, double& r1, double& w0, double& w1, double& q0,
                          double& q1) {
        const int pc = pc0 + 64 * m;
        a0 = a1 = r0 = r1 = w0 = w1 = q0 = q1 = 0.0;
        if (pc >= PPB) return;
        const int b = 2 * (pc % HP);
        const double2 sv = *reinterpret_cast<const double2*>(Sn + ((size_t)nn * D * DP + 2 * (size_t)pc));
        a0 = sv.x; a1 = sv.y;
        const int j = nbr_j[nn];
        const size_t jx = (size_t)j * D + b;
        if constexpr ((D & 1) == 0) {
            const double2 rv = *reinterpret_cast<const double2*>(r_old + jx);
            r0 = rv.x; r1 = rv.y;
            if (it > 0) {
                const double2 wv2 = *reinterpret_cast<const double2*>(w_old + jx);
                const double2 sv2 = *reinterpret_cast<const double2*>(s_old + jx);
                w0 = wv2.x; w1 = wv2.y; q0 = sv2.x; q1 = sv2.y;
            }
        } else {
            r0 = r_old[jx];
            if (b + 1 < D) r1 = r_old[jx + 1];
            if (it > 0) {
                w0 = w_old[jx]; q0 = s_old[jx];
                if (b + 1 < D) { w1 = w_old[jx + 1]; q1 = s_old[jx + 1]; }
            }
        }
    };
    if (have) {
#pragma unroll
        for (int m = 0; m < PPL; ++m) load_piece(nfirst, m, s0[m], s1[m], xr0[m], xr1[m], xw0[m], xw1[m], xs0[m], xs1[m]);
    }
    // wave 0: own row and the row of L (for the true-residual norm)
    double own_r = 0.0, own_w = 0.0, own_s = 0.0, own_p = 0.0;
    double lrow[D];
    const size_t own = (size_t)row * D + (lane < D ? lane : 0);
    if (wv == 0 && lane < D) {
        own_r = r_old[own];
        if (it > 0) { own_w = w_old[own]; own_s = s_old[own]; own_p = cg.p[own]; }
        const double* L = Lf + (size_t)row * DD + lane * D;
#pragma unroll
        for (int k = 0; k < D; ++k) lrow[k] = (k <= lane) ? L[k] : 0.0;
    }
    // recurrence scalars published by k_cg_dots (uniform loads)
    double alpha = 0.0, beta = 0.0;
    if (it > 0) {
        if (cg.scal[2] != 0.0) return;
        alpha = cg.scal[0];
        beta = cg.scal[1];
    }
    if (status != 0) return;
    // ======== phase 3: own row update (wave 0, lanes < D) ========
    double rn = 0.0;
    if (wv == 0 && lane < D) {
        if (it == 0) {
            rn = own_r;
        } else {
            const double sn = own_w + beta * own_s;
            const double pn = own_r + beta * own_p;
            cg.x[own] += alpha * pn;
            cg.p[own] = pn;
            cg.s[pin][own] = sn;
            rn = own_r - alpha * sn;
            cg.r[pout][own] = rn;
        }
        rsh[lane] = rn;
    }
    // ======== phase 4: neighbour blocks, streamed one round (BPR blocks) at a time ========
    auto consume = [&](int m, double a0, double a1, double r0, double r1, double w0, double w1, double q0, double q1) {
        const double v0 = (it == 0) ? r0 : r0 - alpha * (w0 + beta * q0);
        const double v1 = (it == 0) ? r1 : r1 - alpha * (w1 + beta * q1);
        acc[m] += a0 * v0 + a1 * v1;
    };
    if (have) {
#pragma unroll
        for (int m = 0; m < PPL; ++m) consume(m, s0[m], s1[m], xr0[m], xr1[m], xw0[m], xw1[m], xs0[m], xs1[m]);
    }
    for (int nn = nfirst + BPR; lane_on && nn < n1; nn += BPR) {
#pragma unroll
        for (int m = 0; m < PPL; ++m) {
            load_piece(nn, m, s0[m], s1[m], xr0[m], xr1[m], xw0[m], xw1[m], xs0[m], xs1[m]);
            consume(m, s0[m], s1[m], xr0[m], xr1[m], xw0[m], xw1[m], xs0[m], xs1[m]);
        }
    }
    if (lane_on) {
#pragma unroll
        for (int m = 0; m < PPL; ++m) {
            const int pc = pc0 + 64 * m;
            if (pc < PPB) red[wv][bw][pc] = acc[m];
        }
    }
    __syncthreads();
    // ======== phase 5: w' for the row and the partial dots (wave 0) ========
    if (wv == 0) {
        double g0 = 0.0, g1 = 0.0, g2 = 0.0;
        if (lane < D) {
            const int a = lane;
            double tot = 0.0;
            for (int w = 0; w < kCgWaves; ++w)
#pragma unroll
                for (int bb = 0; bb < BPW; ++bb)
#pragma unroll
                    for (int k = 0; k < HP; ++k) tot += red[w][bb][a * HP + k];
            const double wn = rn + tot;
            cg.w[pout][own] = wn;
            double lr = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) lr += lrow[k] * rsh[k];
            g0 = rn * rn;
            g1 = wn * rn;
            g2 = lr * lr;
        }
        g0 = wave_sum(g0); g1 = wave_sum(g1); g2 = wave_sum(g2);
        if (lane == 0) {
            double* pp = cg.part[pout];
            pp[row] = g0; pp[C + row] = g1; pp[2 * (size_t)C + row] = g2;
        }
    }
}

// dc = L^-T x~
template <int D>
__global__ __launch_bounds__(kThreads) void k_cg_finish(int C, const double* __restrict__ Li, const double* __restrict__ xt,
                                                        double* __restrict__ dc, long long* stp) {
    const StampScope stamp_(stp);
    const int k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= C * D) return;
    const int i = k / D, a = k % D;
    const double* L = Li + (size_t)i * D * D;
    double s = 0.0;
    for (int m = a; m < D; ++m) s += L[m * D + a] * xt[(size_t)i * D + m];
    dc[k] = s;
}

// ------------------------------------------------------------------------------------------------------------
// back-substitution, parameter update, cost
// ------------------------------------------------------------------------------------------------------------
// Cameras: X <- Exp(dc_pose) X, intrinsics += dc_intr; gain part 2 g_c.dc - dc^T U dc (rank 0 only).  One block of NT
// cameras per call; the block's gain partial goes to part[blk].
template <int M, int NT>
__device__ __forceinline__ void update_cams_block(int blk, int C, const double* __restrict__ cams,
                                                  const double* __restrict__ dc, const double* __restrict__ U,
                                                  const double* __restrict__ gc, int with_gain,
                                                  double* __restrict__ cams_new, double* __restrict__ part,
                                                  double* red /* >= NT / 64 doubles */) {
    constexpr int D = kD<M>, ST = kStride<M>, NI = Model<M>::NI;
    const int c = blk * NT + threadIdx.x;
    double gain[1] = {0.0};
    if (c < C) {
        const double* x = cams + (size_t)c * ST;
        double* o = cams_new + (size_t)c * ST;
        if (dc) {
            const double* d = dc + (size_t)c * D;
            retract_pose(x, d, o);
#pragma unroll
            for (int k = 0; k < NI; ++k) o[7 + k] = x[7 + k] + d[6 + k];
            if (with_gain) {
                const double* Uc = U + (size_t)c * D * D;
                double quad = 0.0, lin = 0.0;
                for (int a = 0; a < D; ++a) {
                    double s = 0.0;
                    for (int bb = 0; bb < D; ++bb) s += Uc[a * D + bb] * d[bb];
                    quad += d[a] * s;
                    lin += gc[(size_t)c * D + a] * d[a];
                }
                gain[0] = 2.0 * lin - quad;
            }
        } else {
#pragma unroll
            for (int k = 0; k < ST; ++k) o[k] = x[k];
        }
    }
    block_sum<1, NT>(gain, red);
    if (threadIdx.x == 0) part[blk] = gain[0];
}

// Back-substitution: dp = V^-1 (g_p - sum_o W_o^T dc_cam(o)) per track, trial points, gain part 2 g_p.dp - dp^T V dp
// (block partial).  Same runs of whole tracks as k_lin_points, one thread per observation; W_o^T dc is re-derived
// instead of read from W: J~ is evaluated again at the linearization point exactly as k_lin_points does (same inputs,
// same code: the same J~c, J~p) and q_o = J~p^T (J~c dc); one thread per track subtracts its q_o in observation order.
// It reads ~50 B per observation (uv, camera / point index, the run's points) instead of the 192-B W record, and the
// evaluation costs less than the record's HBM time (the W-reading form measured 107 vs 64 us on config 3).
template <int M>
__global__ __launch_bounds__(kLinThreads) void k_backsub_rc(const int* __restrict__ blk, const int* __restrict__ pt_ptr,
                                                            const int* __restrict__ cam, const int* __restrict__ ptl,
                                                            const double* __restrict__ uv, const double* __restrict__ pp,
                                                            const double* __restrict__ cams, double delta,
                                                            const double* __restrict__ dc, const double* __restrict__ V,
                                                            const double* __restrict__ Vinv, const double* __restrict__ gp,
                                                            const double* __restrict__ pts, double* __restrict__ dp,
                                                            double* __restrict__ pts_new, double* __restrict__ part,
                                                            int nrun, int C, const double* __restrict__ U,
                                                            const double* __restrict__ gc, int with_gain,
                                                            double* __restrict__ cams_new, double* __restrict__ part_gc,
                                                            long long* stp = nullptr) {
    const StampScope stamp_(stp);
    constexpr int D = kD<M>, ST = kStride<M>;
    __shared__ double red[kLinThreads];
    __shared__ double q[kLinThreads][3];
    if ((int)blockIdx.x >= nrun) {  // the camera update rides along as the launch's last blocks (no separate launch)
        update_cams_block<M, kLinThreads>(blockIdx.x - nrun, C, cams, dc, U, gc, with_gain, cams_new, part_gc, red);
        return;
    }
    const int t = threadIdx.x;
    const int tb = blk[blockIdx.x], te = blk[blockIdx.x + 1];
    const int p = tb + t;
    const bool own = p < te;
    double gain[1] = {0.0};
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
    if (own) { t0 = gp[3 * (size_t)p]; t1 = gp[3 * (size_t)p + 1]; t2 = gp[3 * (size_t)p + 2]; }
    if (dc) {
        const int ob = pt_ptr[tb], oe = pt_ptr[te];
        const int lo = own ? pt_ptr[p] : 0, hi = own ? pt_ptr[p + 1] : 0;
        for (int base = ob; base < oe; base += kLinThreads) {
            const int n = min(kLinThreads, oe - base);
            if (t < n) {
                const int o = base + t;
                const int c = cam[o], pl = ptl[o];
                const double X[3] = {pts[3 * (size_t)pl], pts[3 * (size_t)pl + 1], pts[3 * (size_t)pl + 2]};
                const double2 z = reinterpret_cast<const double2*>(uv)[o];
                const double uvo[2] = {z.x, z.y};
                const double ppc[2] = {pp[2 * c], pp[2 * c + 1]};
                double d[D];
                const double* dr = dc + (size_t)c * D;
#pragma unroll
                for (int a = 0; a < D; ++a) d[a] = dr[a];
                double r[2], Jc[2][D], Jp[2][3];
                eval_obs<M, true>(cams + (size_t)c * ST, X, ppc, uvo, r, Jc, Jp);
                const double sw = huber_weight_sqrt(r[0] * r[0] + r[1] * r[1], delta);
                double e0 = 0.0, e1 = 0.0;
#pragma unroll
                for (int a = 0; a < D; ++a) { e0 += (Jc[0][a] * sw) * d[a]; e1 += (Jc[1][a] * sw) * d[a]; }
#pragma unroll
                for (int k = 0; k < 3; ++k) q[t][k] = (Jp[0][k] * sw) * e0 + (Jp[1][k] * sw) * e1;
            }
            __syncthreads();
            for (int o = max(lo, base); o < min(hi, base + n); ++o) {
                t0 -= q[o - base][0]; t1 -= q[o - base][1]; t2 -= q[o - base][2];
            }
            __syncthreads();
        }
    }
    if (own) {
        const double* vi = Vinv + 6 * (size_t)p;
        const double d0 = vi[0] * t0 + vi[1] * t1 + vi[2] * t2;
        const double d1 = vi[1] * t0 + vi[3] * t1 + vi[4] * t2;
        const double d2 = vi[2] * t0 + vi[4] * t1 + vi[5] * t2;
        dp[3 * (size_t)p] = d0; dp[3 * (size_t)p + 1] = d1; dp[3 * (size_t)p + 2] = d2;
        pts_new[3 * (size_t)p] = pts[3 * (size_t)p] + d0;
        pts_new[3 * (size_t)p + 1] = pts[3 * (size_t)p + 1] + d1;
        pts_new[3 * (size_t)p + 2] = pts[3 * (size_t)p + 2] + d2;
        const double* v = V + 6 * (size_t)p;
        const double Vd0 = v[0] * d0 + v[1] * d1 + v[2] * d2;
        const double Vd1 = v[1] * d0 + v[3] * d1 + v[4] * d2;
        const double Vd2 = v[2] * d0 + v[4] * d1 + v[5] * d2;
        gain[0] = 2.0 * (t0 * d0 + t1 * d1 + t2 * d2) - (d0 * Vd0 + d1 * Vd1 + d2 * Vd2);
    }
    block_sum<1, kLinThreads>(gain, red);
    if (threadIdx.x == 0) part[blockIdx.x] = gain[0];
}

// Huber loss and sum ||r||^2 (block partials).  (Measured: 4 observations per thread, loads hoisted, ran 25 -> 33 us.)
template <int M>
__global__ __launch_bounds__(kCostThreads) void k_cost(int Nl, const int* __restrict__ cam, const int* __restrict__ ptl,
                                                       const double* __restrict__ uv, const double* __restrict__ pp,
                                                       const double* __restrict__ cams, const double* __restrict__ pts,
                                                       double delta, double* __restrict__ part,
                                                       long long* stp = nullptr) {
    const StampScope stamp_(stp);
    constexpr int ST = kStride<M>;
    __shared__ double red[2 * (kCostThreads / 64)];
    const int o = blockIdx.x * kCostThreads + threadIdx.x;
    double v[2] = {0.0, 0.0};
    if (o < Nl) {
        const int c = cam[o], p = ptl[o];
        const double X[3] = {pts[3 * (size_t)p], pts[3 * (size_t)p + 1], pts[3 * (size_t)p + 2]};
        const double2 z = reinterpret_cast<const double2*>(uv)[o];
        const double uvo[2] = {z.x, z.y};
        const double ppc[2] = {pp[2 * c], pp[2 * c + 1]};
        double r[2];
        eval_obs<M, false>(cams + (size_t)c * ST, X, ppc, uvo, r, nullptr, nullptr);
        const double s = r[0] * r[0] + r[1] * r[1];
        const double rs = sqrt(s);
        v[0] = rs < delta ? s : 2.0 * delta * rs - delta * delta;
        v[1] = s;
    }
    block_sum<2, kCostThreads>(v, red);
    if (threadIdx.x == 0) { part[2 * (size_t)blockIdx.x] = v[0]; part[2 * (size_t)blockIdx.x + 1] = v[1]; }
}

// result[0..4] = {loss, sum ||r||^2, gain_points, gain_cams, #non-PD point blocks}; fixed-order sums of the partials.
// All five are summed across ranks, so every rank takes the same accept / reject / fail branch.
// one 1024-thread workgroup (16 waves: four times the loads in flight of a 256-thread one; 11 -> 5 us on config 3's
// ~40k partials)
constexpr int kFinalThreads = 1024;
__global__ __launch_bounds__(kFinalThreads) void k_final(const double* __restrict__ cost_part, int ncost,
                                                    const double* __restrict__ gp_part, int ngp,
                                                    const double* __restrict__ gc_part, int ngc, int* __restrict__ flags,
                                                    double* __restrict__ result, const int* __restrict__ cgst,
                                                    long long* stp = nullptr) {
    const StampScope stamp_(stp);
    // the three partial arrays in one pass (every load of a round in flight together), each array still summed by
    // each thread in index order and then by the same butterfly and wave order: bitwise the sums of three separate
    // sum_partials passes, with one latency chain instead of three
    __shared__ double red[4 * kFinalThreads / 64];
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    const int ng1 = gp_part ? ngp : 0, ng2 = gc_part ? ngc : 0;
    const int nmax = max(ncost, max(ng1, ng2));
#pragma unroll 4
    for (int i = threadIdx.x; i < nmax; i += kFinalThreads) {
        if (i < ncost) { v[0] += cost_part[2 * (size_t)i]; v[1] += cost_part[2 * (size_t)i + 1]; }
        if (i < ng1) v[2] += gp_part[i];
        if (i < ng2) v[3] += gc_part[i];
    }
    block_sum<4, kFinalThreads>(v, red);
    const double c2[2] = {v[0], v[1]}, a[1] = {v[2]}, b[1] = {v[3]};
    if (threadIdx.x == 0) {
        result[0] = c2[0]; result[1] = c2[1]; result[2] = a[0]; result[3] = b[0];
        result[4] = (double)flags[0];
        // a k_tl_cgp solve whose status the host reads after the cost: 1 when it aborted at a grid barrier (status 4).
        // All-reduced with the other scalars, so every rank of a replicated CG sees whether any rank aborted.
        result[5] = (cgst != nullptr && cgst[0] == 4) ? 1.0 : 0.0;
        flags[0] = 0;  // consumed: the next solve's point preparation starts from a clear flag
    }
}

// flags[0..3] = 0, status[0..3] = 0
__global__ void k_zero_words(int* __restrict__ flags, int* __restrict__ status) {
    const int t = threadIdx.x;
    if (t < 4) flags[t] = 0;
    else if (t < 8) status[t - 4] = 0;
}

// After k_final (and the cross-rank sum): result[0..4] into host-mapped memory for the host's spin-wait, then
// sequence word `seq` (system-scope release), so the host reads the trial's cost without a stream synchronization or a
// copy launch.  With `cams_cur` set (insfm_ba_step: the caller's buffers hold the current parameters) the accepted
// trial is copied there in the same launch; the test is lm_step's accept rule on the same doubles (not SPD -> fail;
// last < loss with rejects left -> reject; otherwise accept), and the decision is published in pub[5] for the host to
// check against its own.
__global__ __launch_bounds__(kThreads) void k_publish(const double* __restrict__ result, const int* __restrict__ cgst,
                                                      double* pub, unsigned seq, double last,
                                                      int can_reject, const double* __restrict__ cams_new,
                                                      double* __restrict__ cams_cur, long long ncam,
                                                      const double* __restrict__ pts_new, double* __restrict__ pts_cur,
                                                      long long npts, long long* stp) {
    const StampScope stamp_(stp);
    const double loss = result[0];
    // cgst (a k_tl_cgp solve whose status the host reads afterwards): only a converged CG's trial can be accepted
    // (result[5]: a k_tl_cgp abort on any rank -- every rank then repeats the trial on the launch path)
    const bool acc = result[4] == 0.0 && !(last < loss && can_reject) && (cgst == nullptr || cgst[0] == 1) &&
                     result[5] == 0.0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (int k = 0; k < 5; ++k) pub[k] = result[k];
        pub[5] = acc ? 1.0 : 0.0;
        pub[6] = result[5];
        __threadfence_system();
        __hip_atomic_store(reinterpret_cast<unsigned*>(pub + 8), seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (!acc || cams_cur == nullptr) return;
    const long long g = (long long)blockIdx.x * kThreads + threadIdx.x, G = (long long)gridDim.x * kThreads;
    for (long long k = g; k < ncam; k += G) cams_cur[k] = cams_new[k];
    // points: 16-byte pieces (both buffers 16-B aligned: allocations and the shard offset are whole points of 24 B,
    // so the pair path is taken only when both pointers are)
    const bool al = ((reinterpret_cast<uintptr_t>(pts_new) | reinterpret_cast<uintptr_t>(pts_cur)) & 15) == 0;
    if (al) {
        const long long n2 = npts / 2;
        const double2* s2 = reinterpret_cast<const double2*>(pts_new);
        double2* d2 = reinterpret_cast<double2*>(pts_cur);
        for (long long k = g; k < n2; k += G) d2[k] = s2[k];
        if (g == 0 && (npts & 1)) pts_cur[npts - 1] = pts_new[npts - 1];
    } else {
        for (long long k = g; k < npts; k += G) pts_cur[k] = pts_new[k];
    }
}

inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

}  // namespace

// ============================================================================================================
// host side
// ============================================================================================================
#include "ba_handle.h"

#include "ba_solve.h"
#include "ba_step.h"

// ============================================================================================================
// C ABI
// ============================================================================================================
extern "C" {

void insfm_ba_default_desc(insfm_ba_desc* d) {
    std::memset(d, 0, sizeof(*d));
    d->cam_model = 2;
    d->optimize_poses = 1;
    d->deterministic = 0;
    d->huber_delta = 1.0;
    d->tr_radius = 1e4; d->tr_max = 1e10; d->tr_min = 1e-6; d->tr_up = 2.0; d->tr_down = 1.0 / 16.0;
    d->tr_factor = 0.25; d->tr_high = 0.5; d->tr_low = 1e-3;
    d->clamp_min = 1e-6; d->clamp_max = 1e32;
    d->max_rejects = 30;
    d->pcg_max_iter = 500;
    d->pcg_tol = 1e-5;
    d->world_size = 1; d->rank = 0;
    d->shard_point_begin = 0; d->shard_point_end = -1;
    d->precond = 2;
    d->cluster_size = 24;
    d->exchange_chunks = 4;
}

const char* insfm_ba_last_error(const insfm_ba* h) { return h ? h->err.c_str() : "null handle"; }

void insfm_ba_destroy(insfm_ba* h) {
    if (!h) return;
    if (h->side) (void)side_flush(h);
    // every stream that may still use the buffers, before they are parked for the next handle
    for (hipStream_t st : {h->stream, h->side, h->xstream, h->aux})
        if (st) (void)hipStreamSynchronize(st);
    if (!h->stream) (void)hipDeviceSynchronize();
    for (void* q : h->xopened) (void)hipIpcCloseMemHandle(q);  // (peers must be done writing: the caller's barrier)
    if (h->xwin) (void)hipFree(h->xwin);
    dfree_all(h);
    if (h->host_res) (void)hipHostFree(h->host_res);
    if (h->prog_host) (void)hipHostFree(h->prog_host);
    if (h->pub_host) (void)hipHostFree(h->pub_host);
    for (auto& e : h->ev)
        if (e) (void)hipEventDestroy(e);
    if (h->side) {
        (void)hipStreamSynchronize(h->side);
        release_helper_stream(h->side);
    }
    if (h->xstream) {
        (void)hipStreamSynchronize(h->xstream);
        (void)hipStreamDestroy(h->xstream);
    }
    if (h->aux) {
        (void)hipStreamSynchronize(h->aux);
        release_helper_stream(h->aux);
    }
    if (h->ev_lin0) (void)hipEventDestroy(h->ev_lin0);
    if (h->ev_lc) (void)hipEventDestroy(h->ev_lc);
    if (h->ev_x) (void)hipEventDestroy(h->ev_x);
    if (h->ev_xdone) (void)hipEventDestroy(h->ev_xdone);
    if (h->ev_pre) (void)hipEventDestroy(h->ev_pre);
    if (h->ev_E) (void)hipEventDestroy(h->ev_E);
    if (h->ev_built) (void)hipEventDestroy(h->ev_built);
    for (auto& e : h->ev_fact)
        if (e) (void)hipEventDestroy(e);
    delete h;
}

int64_t insfm_ba_nnzb(const insfm_ba* h) { return h ? h->nnzb : -1; }

int64_t insfm_ba_release_cache(void) { return (int64_t)release_cache(); }

}  // extern "C"

#include "ba_create.h"

extern "C" {

int insfm_ba_create(const insfm_ba_desc* desc, const double* obs_uv, const int32_t* cam_idx, const int32_t* pt_idx,
                    const double* pp, void* stream, insfm_ba** out) {
    return create_impl(desc, 0, obs_uv, cam_idx, pt_idx, pp, nullptr, stream, out);
}

int insfm_ba_set_timing(insfm_ba* h, int32_t on) {
    if (!h) return INSFM_BA_EINVAL;
    h->want_timing = on != 0;
    return INSFM_BA_OK;
}

int64_t insfm_ba_exchange_count(const insfm_ba* h) { return h ? h->xcount : -1; }

int insfm_ba_set_exchange(insfm_ba* h, double* buf, int64_t count) {
    if (!h || !buf || count < h->xcount) return INSFM_BA_EINVAL;
    const int C = h->C, D = h->D;
    h->xbuf = buf;
    h->S = h->xbuf;
    h->b = h->S + (size_t)h->nnzb * D * D;
    h->U = h->b + (size_t)C * D;
    h->gc = h->U + (size_t)C * D * D;
    h->scal = h->gc + (size_t)C * D;
    h->result = h->scal;
    return INSFM_BA_OK;
}

int insfm_ba_set_ranks_per_device(insfm_ba* h, int32_t ranks) {
    if (!h || ranks < 1) return INSFM_BA_EINVAL;
    if (h->cgp_nb && (long long)ranks * h->cgp_grid > (long long)h->cgp_slots) {
        if (diag("create"))
            std::fprintf(stderr, "[insfm create] %d ranks per GPU: k_tl_cgp would need %lld of %d workgroup slots; "
                         "launch path\n", ranks, (long long)ranks * h->cgp_grid, h->cgp_slots);
        h->cgp_nb = 0;
    }
    return INSFM_BA_OK;
}

int insfm_ba_cg_info(const insfm_ba* h, int32_t* out) {
    if (!h || !out) return INSFM_BA_EINVAL;
    out[0] = h->xpart ? 3 : h->cgp_nb ? (h->cgp_det ? (h->adef2 ? 5 : 2) : (h->adef2 ? 4 : 1)) : 0;
    out[1] = h->cgp_grid;
    out[2] = h->cgp_slots;
    out[3] = h->cgp_nb;
    return INSFM_BA_OK;
}

int32_t insfm_ba_cg_fallbacks(const insfm_ba* h) {
    if (!h) return INSFM_BA_EINVAL;
    return h->adef2_fallbacks;
}

int insfm_ba_set_persistent_cg(insfm_ba* h, int32_t on) {
    if (!h) return INSFM_BA_EINVAL;
    if (on) return h->cgp_nb ? INSFM_BA_OK : INSFM_BA_EINVAL;  // (cannot turn on what create found ineligible)
    cgp_drop_pending(h);
    h->cgp_nb = 0;
    return INSFM_BA_OK;
}

int insfm_ba_reset(insfm_ba* h) {
    if (!h) return INSFM_BA_EINVAL;
    h->damping = 1.0 / h->d.tr_radius;
    h->down = h->d.tr_down;
    h->have_loss = false;
    // a fresh LM: the first solve after the reset factorizes its own coarse matrix (no lagged E^-1 of an earlier solve
    // survives) and the CG's first batch is sized as for a new handle
    cgp_drop_pending(h);
    if (int rc = side_flush(h)) return rc;
    h->tl_solves = 0;
    h->tl_fresh = false;
    h->last_cg_iters = 16;
    h->chain_timed[0] = h->chain_timed[1] = false;
    return INSFM_BA_OK;
}

int insfm_ba_cost(insfm_ba* h, const double* cams, const double* pts, double* loss, double* rmse) {
    if (!h || !cams || !pts || h->kind != 0) return INSFM_BA_EINVAL;
    cgp_drop_pending(h);
    HIPCHK(hipMemsetAsync(h->flags, 0, sizeof(int) * 4, h->stream));
    int rc = run_cost(h, cams, pts + 3 * (size_t)h->p0, false);
    if (rc) return rc;
    if (loss) *loss = h->host_res[0];
    if (rmse) *rmse = h->N > 0 ? std::sqrt(h->host_res[1] / h->N) : 0.0;
    return INSFM_BA_OK;
}

int insfm_ba_step(insfm_ba* h, double* cams_user, double* pts_user, insfm_ba_stats* st) {
    if (!h || !cams_user || !pts_user || h->kind != 0) return INSFM_BA_EINVAL;
    // The caller's buffers are the linearization point of this step (read in place, no copy-in); trials go to the
    // internal cams_new / pts_new, and an accepted trial is copied back into the caller's buffers (stream-ordered, no
    // host wait: the step's loss is already on the host).
    double* const ic = h->cams_cur;
    double* const ip = h->pts_cur;
    h->cams_cur = cams_user;
    h->pts_cur = pts_user + 3 * (size_t)h->p0;
    h->ext_cur = true;
    const int rc = lm_step(h, st);
    h->cams_cur = ic;
    h->pts_cur = ip;
    h->ext_cur = false;
    return rc;
}

// ---- global positioning (include/insfm_gp.h) -------------------------------------------------------------------
void insfm_gp_default_desc(insfm_ba_desc* d) {
    insfm_ba_default_desc(d);
    d->cam_model = -1;
    d->huber_delta = 0.1;  // GLOBAL_POSITIONER_OPTIONS['thres_loss_function'] (config/colmap.py:41-46)
    d->tr_radius = 1e3;    // TrustRegion(radius=1e3, max=1e8, up=2.0, down=0.5**4) (global_positioning.py:158)
    d->tr_max = 1e8;
}

int insfm_gp_create(const insfm_ba_desc* desc, const double* trans, const int32_t* cam_idx, const int32_t* pt_idx,
                    const double* cam_factor, const int32_t* scale_free, void* stream, insfm_ba** out) {
    return create_impl(desc, 1, trans, cam_idx, pt_idx, cam_factor, scale_free, stream, out);
}

// Positions, the shard's points and the scales between the caller's buffers and the LM state (one k_gp_io launch).
static int gp_io(insfm_ba* h, int in, const double* pos, const double* pts, const double* scales) {
    const long long n3c = 3LL * h->C, n3p = 3LL * h->Pl, nl = h->Nl, tot = n3c + n3p + nl;
    if (tot == 0) return 0;
    const int grid = std::max(1, std::min(2048, cdiv(tot, kThreads)));
    k_gp_io<<<grid, kThreads, 0, h->stream>>>(in, n3c, const_cast<double*>(pos), h->cams_cur, n3p,
                                              const_cast<double*>(pts) + 3 * (size_t)h->p0, h->pts_cur, nl, h->osrc,
                                              const_cast<double*>(scales), h->scl_cur);
    return launch_err(h, "k_gp_io");
}

int insfm_gp_step(insfm_ba* h, double* pos, double* pts, double* scales, insfm_ba_stats* st) {
    if (!h || !pos || !pts || !scales || h->kind != 1) return INSFM_BA_EINVAL;
    int rc = gp_io(h, 1, pos, pts, scales);
    if (rc) return rc;
    if ((rc = lm_step(h, st))) return rc;
    // written back in stream order (no host wait: the step's loss is already on the host), like insfm_ba_step
    return gp_io(h, 0, pos, pts, scales);
}

int insfm_gp_cost(insfm_ba* h, const double* pos, const double* pts, const double* scales, double* loss, double* rmse) {
    if (!h || !pos || !pts || !scales || h->kind != 1) return INSFM_BA_EINVAL;
    HIPCHK(hipMemsetAsync(h->flags, 0, sizeof(int) * 4, h->stream));
    // scratch copies (the LM's current state is untouched: cams_new / pts_new / scl_new are trial buffers)
    HIPCHK(hipMemcpyAsync(h->cams_new, pos, sizeof(double) * 3 * (size_t)h->C, hipMemcpyDeviceToDevice, h->stream));
    if (h->Nl) k_gp_gather<<<cdiv(h->Nl, kThreads), kThreads, 0, h->stream>>>(h->Nl, h->osrc, scales, h->scl_new);
    int rc = launch_err(h, "k_gp_gather");
    if (rc) return rc;
    if ((rc = run_cost(h, h->cams_new, pts + 3 * (size_t)h->p0, false, h->scl_new))) return rc;
    if (loss) *loss = h->host_res[0];
    if (rmse) *rmse = h->N > 0 ? std::sqrt(h->host_res[1] / h->N) : 0.0;
    return INSFM_BA_OK;
}

}  // extern "C"

#include "ba_debug_api.h"
