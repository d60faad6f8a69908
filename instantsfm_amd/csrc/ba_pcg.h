// Block-Jacobi side of the PCG on the reduced camera system: the per-camera factorization S_ii = L L^T (k_cg_factor,
// with the coarse basis k_cg_factor_basis), the scaling S~ = L^-1 S L^-T (k_cg_scale), the launch-per-iteration CG
// of precond 0 (k_cg_dots, k_cg_iter) and dc = L^-T x~ (k_cg_finish).  The two-level CG is in ba_twolevel.h and
// ba_cgp.h.  Part of the one translation unit ba_kernels.hip.
#pragma once
#include "ba_cgp.h"
#include "ba_common.h"
#include "ba_device.h"
#include "ba_twolevel.h"

namespace {

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

}  // namespace
