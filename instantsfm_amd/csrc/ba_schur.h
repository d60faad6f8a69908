// Schur complement of an LM trial (k_schur) and its tuning knobs.  Part of the one translation unit ba_kernels.hip.
//
// One workgroup per (camera row i, chunk of its upper blocks); the chunk of S's row lives in LDS.
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
#pragma once
#include "ba_common.h"
#include "ba_device.h"

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
#ifndef SCHUR_MINW
#define SCHUR_MINW 1  // k_schur launch bound: minimum waves per SIMD (caps VGPRs: 4 -> 128)
#endif
#ifndef SCHUR_UP
#define SCHUR_UP 10  // partners in flight per group (non-deterministic mode)
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
                load_wcol<D, GPW>(W, qs + u, cb, x[u][0], x[u][1], x[u][2]);
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
                        load_wcol<D, GPW>(W, q, cb, x[u][0], x[u][1], x[u][2]);
                        cj[u] = cam[q];
                    }
                }
            }
            // every slot of the round looked up before the first ds_add_f64: one LDS wait per round instead of one
            // per partner (a slot read issued behind the previous partner's adds waits for them to retire)
            int slv[UP];
#pragma unroll
            for (int u = 0; u < UP; ++u) slv[u] = slot[cj[u] >= 0 ? cj[u] : 0];
            __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0) (vmcnt, expcnt unconstrained): all slots read
            __builtin_amdgcn_sched_barrier(0);
            // ORD: wave w adds between the w-th and the (w+1)-th of the round's WAVES barriers
            if constexpr (ORD)
                for (int k = 0; k < wv; ++k) __syncthreads();
#pragma unroll
            for (int u = 0; u < UP; ++u) {
                if (cj[u] >= 0) {
                    const int sl = slv[u];
                    if (sl >= 0) {
                        double* dst = acc + (size_t)sl * BS + cb;
                        const double y0 = x[u][0], y1 = x[u][1], y2 = x[u][2];
#pragma unroll
                        for (int a2 = 0; a2 < D; ++a2)
                            atomicAdd(dst + a2 * D, wh[a2][0] * y0 + wh[a2][1] * y1 + wh[a2][2] * y2);
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
        Sout[k] = v;
    }
    if (diag_chunk && t < D) b[(size_t)i * D + t] = (add_diag ? gc[(size_t)i * D + t] : 0.0) + bacc[t];
}

}  // namespace
