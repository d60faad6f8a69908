// E^-1 by blocked Gauss-Jordan inversion (multi-workgroup, f64 MFMA): the dense chain of the two-level preconditioner
// (included by ba_twolevel.h and tools/bench_dense.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

#include "ba_common.h"

namespace insfm {

// E (m x m, SPD) is held padded to ld = nB * kGB (pad: identity), symmetrically equilibrated on the fly
// (d = 1 / sqrt(diag E), from k_tl_ereduce; the pad's d is 1) and inverted by block Gauss-Jordan steps k = 0..nB-1
// with pivot block P = X_kk (no pivoting: every pivot block of an SPD matrix is SPD):
//   Y_kk = P^-1,  Y_kj = P^-1 X_kj,  Y_ik = -X_ik P^-1,  Y_ij = X_ij - X_ik (P^-1 X_kj)      (i, j != k)
// One launch per step (k_gj_step: nB x nB workgroups, one 32 x 32 tile each, v_mfma_f64_16x16x4f64), ping-ponging
// between two buffers so that no workgroup reads a tile another one writes in the same launch.  P^-1 is looked
// ahead: the workgroup that forms the next pivot block Y_{k+1,k+1} inverts it right away (k_gj_pinv0 does P_0) by
// scalar in-place Gauss-Jordan in one wave's registers (gj_invert_block), so the other workgroups only load it.
// The last step writes diag(d) Y diag(d) compactly (row stride m) for k_tl_pc.
// 2 m^3 flops in nB + 1 launches; the oracle (ba_oracle.c gj_inverse) runs the same steps, pivots and fused
// multiply-adds.
constexpr int kGB = 32;        // block size
constexpr int kGS = kGB + 1;   // LDS row stride (odd: the A-fragment column reads are conflict-free)
typedef double gj_acc_t __attribute__((ext_vector_type(4)));

// acc += sgn * As[R .. R+15][:] * Bs[:][Cc .. Cc+15] over K = 32 for wave w's subtile (R, Cc) = (16 (w >> 1),
// 16 (w & 1)) (v_mfma_f64_16x16x4f64: A fragment lane l = A[row l & 15][k l >> 4], B fragment = B[k l >> 4]
// [col l & 15], result reg q = D[row (l >> 4) + 4 q][col l & 15]; cdna_hip_programming.md, f64 MFMA layout).
__device__ __forceinline__ gj_acc_t gj_tile_mfma(const double (*As)[kGS], const double (*Bs)[kGS], gj_acc_t acc, double sgn,
                                                 int lane, int w) {
    const int R = (w >> 1) * 16, Cc = (w & 1) * 16, lr = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int s = 0; s < kGB / 4; ++s)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(sgn * As[R + lr][4 * s + lk], Bs[4 * s + lk][Cc + lr], acc, 0, 0, 0);
    return acc;
}

// tile (r0, c0) of X (row stride ld) -> LDS, optionally equilibrated ((x d_r) d_c, the oracle's order)
__device__ __forceinline__ void gj_stage(double (*dst)[kGS], const double* __restrict__ X, int ld, size_t r0, size_t c0,
                                         const double* __restrict__ d) {
    for (int e = threadIdx.x; e < kGB * kGB; e += 256) {
        const int r = e / kGB, c = e % kGB;
        double v = X[(r0 + r) * ld + c0 + c];
        if (d) v = v * d[r0 + r] * d[c0 + c];
        dst[r][c] = v;
    }
}

// gj_invert_block: in-place scalar Gauss-Jordan inversion of the SPD block in M (LDS) by wave 0, result back into M;
// every thread of the workgroup must call it.  Returns (in wave 0) whether a pivot was not positive.
// Lane l holds the 4 x 4 sub-block (rows 4 (l & 7) .., columns 4 (l >> 3) ..); per pivot P the lane fetches the 4
// pivot-column entries of its rows and the 4 pivot-row entries of its columns by ds_bpermute from the two lanes that
// hold them (16 dword permutes), forms 4 scaled row entries and does 16 fused multiply-adds: for every entry
// rpc = row * (1 / piv), fma(-aip, rpc, a), with the pivot row / column cases -- the oracle's values (ba_oracle.c
// gj_inverse).  The inversion of E (m = 639) takes 242 us standalone (tools/bench_dense.hip, profiles/r5_v2/).
// The readlane, LDS and ds_swizzle forms measured before it: DESIGN.md sections 4 and 8.
__device__ __forceinline__ double bperm_d(int src_lane, double v) {
    const int lo = __builtin_amdgcn_ds_bpermute(src_lane << 2, __double2loint(v));
    const int hi = __builtin_amdgcn_ds_bpermute(src_lane << 2, __double2hiint(v));
    return __hiloint2double(hi, lo);
}
template <int P>
__device__ __forceinline__ void gj_p6_round(double (&a)[4][4], int rb, int cb, bool& bad) {
    constexpr int PB = P >> 2, PI = P & 3;
    double colv[4], rowv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) colv[i] = bperm_d(PB * 8 + rb, a[i][PI]);  // row 4 rb + i, column P
#pragma unroll
    for (int c = 0; c < 4; ++c) rowv[c] = bperm_d(cb * 8 + PB, a[PI][c]);  // row P, column 4 cb + c
    double piv = readlane_d(a[PI][PI], PB * 8 + PB);
    if (!(piv > 0.0)) { bad = true; piv = 1.0; }
    const double inv = 1.0 / piv;
    double rpc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) rpc[c] = rowv[c] * inv;
    const bool prow = rb == PB, pcol = cb == PB;  // this lane holds part of row P / of column P
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double up = __builtin_fma(-colv[i], rpc[c], a[i][c]);
            if (c == PI && i == PI) {
                a[i][c] = pcol ? (prow ? inv : -colv[i] * inv) : (prow ? rpc[c] : up);
            } else if (c == PI) {
                a[i][c] = pcol ? -colv[i] * inv : up;
            } else if (i == PI) {
                a[i][c] = prow ? rpc[c] : up;
            } else {
                a[i][c] = up;
            }
        }
}
template <int... P>
__device__ __forceinline__ void gj_p6_all(double (&a)[4][4], int rb, int cb, bool& bad, std::integer_sequence<int, P...>) {
    (gj_p6_round<P>(a, rb, cb, bad), ...);
}

__device__ bool gj_invert_block(double (*M)[kGS]) {
    static_assert(kGB == 32, "64 lanes = 8 x 8 sub-blocks of 4 x 4");
    __syncthreads();
    bool bad = false;
    if (threadIdx.x < 64) {
        const int l = threadIdx.x, rb = l & 7, cb = l >> 3;
        double a[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) a[i][c] = M[4 * rb + i][4 * cb + c];
        gj_p6_all(a, rb, cb, bad, std::make_integer_sequence<int, kGB>{});
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) M[4 * rb + i][4 * cb + c] = a[i][c];
    }
    __syncthreads();
    return bad;
}

// P_0^-1 (one workgroup): the equilibrated first pivot block.
__global__ __launch_bounds__(256) void k_gj_pinv0(int ld, const double* __restrict__ X, const double* __restrict__ d,
                                                  double* __restrict__ Pout, int* __restrict__ ok) {
    __shared__ double M[kGB][kGS];
    gj_stage(M, X, ld, 0, 0, d);
    const bool bad = gj_invert_block(M);
    for (int e = threadIdx.x; e < kGB * kGB; e += 256) Pout[e] = M[e / kGB][e % kGB];
    if (threadIdx.x == 0) ok[0] = !bad;
}

__global__ __launch_bounds__(256) void k_gj_step(int k, int nB, int ld, int m, const double* __restrict__ X,
                                                 double* __restrict__ Y, const double* __restrict__ d, int first,
                                                 const double* __restrict__ Pin, double* __restrict__ Pnext,
                                                 double* __restrict__ Eout, int* __restrict__ ok) {
    __shared__ double Ps[kGB][kGS];   // P^-1
    __shared__ double Bk[kGB][kGS];   // X_kj, then P^-1 X_kj
    __shared__ double Ci[kGB][kGS];   // X_ik
    const int i = blockIdx.x / nB, j = blockIdx.x % nB, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const size_t k0 = (size_t)k * kGB, i0 = (size_t)i * kGB, j0 = (size_t)j * kGB;
    const int R = (w >> 1) * 16, Cc = (w & 1) * 16;
    const double* ds = first ? d : nullptr;   // equilibrate while reading E (step 0)
    // Every load of the step is issued before the first one is used (P^-1, X_kj, X_ik: 4 entries each per thread at
    // (row (t >> 5) + 8 q, column t & 31); X_ij: this lane's 4 accumulator entries), so the step waits for one global
    // latency instead of one per staged entry (a load-then-store loop retires its loads one at a time).
    const bool upd = i != k && j != k;
    const int sr = t >> 5, sc = t & 31;
    double pv[4], bv[4], cv[4], xv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        pv[q] = Pin[(sr + 8 * q) * kGB + sc];
        bv[q] = j != k ? X[(k0 + sr + 8 * q) * ld + j0 + sc] : 0.0;
        cv[q] = i != k ? X[(i0 + sr + 8 * q) * ld + k0 + sc] : 0.0;
        xv[q] = upd ? X[(i0 + R + (lane >> 4) + 4 * q) * ld + j0 + Cc + (lane & 15)] : 0.0;
    }
    if (ds) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const size_t rk = k0 + sr + 8 * q, ri = i0 + sr + 8 * q;
            bv[q] = bv[q] * ds[rk] * ds[j0 + sc];
            cv[q] = cv[q] * ds[ri] * ds[k0 + sc];
            xv[q] = xv[q] * ds[i0 + R + (lane >> 4) + 4 * q] * ds[j0 + Cc + (lane & 15)];
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        Ps[sr + 8 * q][sc] = pv[q];
        Bk[sr + 8 * q][sc] = bv[q];
        Ci[sr + 8 * q][sc] = cv[q];
    }
    __syncthreads();
    gj_acc_t acc = {0.0, 0.0, 0.0, 0.0};
    if (i == k && j == k) {
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = Ps[R + (lane >> 4) + 4 * q][Cc + (lane & 15)];
    } else if (i == k) {
        acc = gj_tile_mfma(Ps, Bk, acc, 1.0, lane, w);                // Y_kj = P^-1 X_kj
    } else if (j == k) {
        acc = gj_tile_mfma(Ci, Ps, acc, -1.0, lane, w);               // Y_ik = -X_ik P^-1
    } else {
        acc = gj_tile_mfma(Ps, Bk, acc, 1.0, lane, w);                // P^-1 X_kj ...
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) Bk[R + (lane >> 4) + 4 * q][Cc + (lane & 15)] = acc[q];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = xv[q];
        acc = gj_tile_mfma(Ci, Bk, acc, -1.0, lane, w);               // ... Y_ij = X_ij - X_ik (P^-1 X_kj)
    }
    const bool last = k == nB - 1;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const size_t r = i0 + R + (lane >> 4) + 4 * q, cc = j0 + Cc + (lane & 15);
        Y[r * ld + cc] = acc[q];
        if (last && r < (size_t)m && cc < (size_t)m) Eout[r * m + cc] = acc[q] * d[r] * d[cc];
    }
    if (i == k + 1 && j == k + 1) {
        // look-ahead: this tile is the next step's pivot block; invert it now
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) Ps[R + (lane >> 4) + 4 * q][Cc + (lane & 15)] = acc[q];
        const bool bad = gj_invert_block(Ps);
        for (int e = t; e < kGB * kGB; e += 256) Pnext[e] = Ps[e / kGB][e % kGB];
        if (t == 0 && bad) ok[0] = 0;
    }
}

inline int gj_steps(int m) { return (m + kGB - 1) / kGB; }

// Launch unit u of the inversion of E (padded [ld][ld], equilibration d [ld], pad entries 1), u = 0 .. gj_steps(m):
// 0 = P_0^-1, u >= 1 = step u - 1.  E and W are the ping-pong buffers, P [2][kGB][kGB] the pivot inverses; the last
// step writes the compact E^-1 into Eout [m][m]; ok[0] = 0 when E is not positive definite.  Units run in order on
// one stream.
inline void launch_gj_unit(int u, int m, double* E, double* W, double* P, const double* d, double* Eout, int* ok,
                           hipStream_t st) {
    const int nB = gj_steps(m), ld = nB * kGB;
    if (u == 0) {
        k_gj_pinv0<<<1, 256, 0, st>>>(ld, E, d, P, ok);
        return;
    }
    const int k = u - 1;
    const double* X = (k & 1) ? W : E;
    double* Y = (k & 1) ? E : W;
    k_gj_step<<<nB * nB, 256, 0, st>>>(k, nB, ld, m, X, Y, d, k == 0, P + (size_t)(k & 1) * kGB * kGB,
                                       P + (size_t)((k + 1) & 1) * kGB * kGB, Eout, ok);
}

}  // namespace insfm
