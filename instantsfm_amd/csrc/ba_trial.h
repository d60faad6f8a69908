// The rest of an LM trial: back-substitution and parameter update (k_backsub_rc), the trial's cost (k_cost), the
// fixed-order reduction of all partials (k_final) and its hand-off to the host (k_publish).  Part of the one
// translation unit ba_kernels.hip.
#pragma once
#include "ba_common.h"
#include "ba_device.h"
#include "ba_lin.h"  // kLinThreads: k_backsub_rc walks k_lin_points' track runs

namespace {

#ifndef COST_THREADS
#define COST_THREADS 256
#endif
constexpr int kCostThreads = COST_THREADS;  // k_cost workgroup size (64 / 128 / 512: same time, 25-26 us; 1024: trial cost 0.045 -> 0.055 ms)

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
    // passes, with one latency chain instead of three
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

}  // namespace
