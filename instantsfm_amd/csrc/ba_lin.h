// Linearization kernels of an LM step: k_lin_points (per track: residual, analytic J, Huber/Triggs weight -> the
// records Y_o, V_p, g_p, and the first trial's point preparation), k_lin_cams / k_lin_cams_reg (per camera: U_c, g_c)
// and k_point_prep (a retried trial's point preparation).  Part of the one translation unit ba_kernels.hip.
#pragma once
#include "ba_common.h"
#include "ba_device.h"

namespace {

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
            // the 384-MB Y-record stream stored with the nontemporal hint (global_store_dwordx4 ... nt).  Config 3
            // (profiles/r6_v10/nt_ab.txt, same box): back-to-back launches 152-153 -> 85 us, LM step 1.046-1.050 ->
            // 1.013-1.033 ms; k_schur, which reads the records next, unchanged (440-448 us).
            typedef double nt_d2 __attribute__((ext_vector_type(2)));
            nt_d2 v2 = {src[0], src[1]};
            __builtin_nontemporal_store(v2, reinterpret_cast<nt_d2*>(dst + k2));
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
#ifndef LIN_CAMS_NT
#define LIN_CAMS_NT 128  // threads per camera (measured 128 / 192 / 256 / 320: 0.156 / 0.161 / 0.167 / 0.194 ms linearize)
#endif
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

}  // namespace
