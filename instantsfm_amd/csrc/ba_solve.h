// One linear solve of the LM step driver, host side: linearization, the Schur build and its exchange, factorization,
// the two-level setup and its side chain, the CG (persistent k_tl_cgp, polled launches, block-Jacobi chunks), the
// back-substitution.  run_solve plans the solve once (solve_policy.h plan_solve, CPU-tested) and everything below it
// executes that plan.  Part of the one translation unit ba_kernels.hip (included after the kernels, before ba_step.h).
#pragma once
#include "ba_handle.h"
#include "cg_poll.h"
#include "solve_policy.h"

namespace {

// h->ev: phase markers on the main stream (each names where its phase begins), the debug timers' bracket
// (ba_debug_api.h), the side chain's span by slot (+ slot), the chunked exchange's span on the exchange stream.
enum Ev {
    kEvLinearize = 0, kEvTrial = 1, kEvBacksub = 3, kEvCost = 4, kEvTrialEnd = 5, kEvSchur = 6, kEvSchurEnd = 7,
    kEvCg = 8, kEvCgEnd = 9, kEvDebug = 10, kEvDebugEnd = 11, kEvChain = 12, kEvChainEnd = 14, kEvXchg = 16,
    kEvXchgEnd = 17
};
// h->tms: the slots of insfm_ba_stats.time_ms (include/insfm_ba.h)
enum Phase { kPhLinearize, kPhSchur, kPhSolve, kPhBacksub, kPhCost, kPhCgLaunches, kPhSideChain, kPhExchange };

int allreduce(insfm_ba* h, double* buf, int64_t n) {
    // a single rank skips the exchange unless a callback is installed (tests drive the RCCL path with one rank)
    if (h->d.world_size <= 1 && !h->d.allreduce) return 0;
    if (!h->d.allreduce) { h->err = "world_size > 1 needs an allreduce callback"; return INSFM_BA_ECOMM; }
    int rc = h->d.allreduce(h->d.allreduce_ctx, buf, n);
    if (rc) { h->err = "allreduce callback failed (" + std::to_string(rc) + ")"; return INSFM_BA_ECOMM; }
    return 0;
}

int allreduce_async(insfm_ba* h, double* buf, int64_t n) {
    int rc = h->d.allreduce_async(h->d.allreduce_ctx, buf, n, h->xstream);
    if (rc) { h->err = "allreduce_async callback failed (" + std::to_string(rc) + ")"; return INSFM_BA_ECOMM; }
    return 0;
}

long long* stamp_ptr(const insfm_ba* h, int kind) {
    if (!h->stamps) return nullptr;
    return h->stamps + ((size_t)(h->stamp_step % kStampSteps) * kStKinds + kind) * 2;
}

void rec(insfm_ba* h, Ev k) {
    if (h->timing) (void)hipEventRecord(h->ev[k], h->stream);
}

// INSFM_DIAG=trace2: host timestamps of one LM step's API calls (labels + microseconds since the step began),
// printed to stderr when the step ends -- where the host, not the GPU, sets the pace
bool host_trace2() {
    static const bool v = diag("trace2");
    return v;
}
void hmark(insfm_ba* h, const char* what) {
    if (host_trace2()) h->hmarks.emplace_back(what, wall_seconds());
}
void print_hmarks(insfm_ba* h) {  // (the end of a step)
    if (!host_trace2() || h->hmarks.empty()) return;
    hmark(h, "step end");
    std::string line = "[insfm host2]";
    for (auto& m : h->hmarks)
        line += " " + std::string(m.first) + "=" + std::to_string((int)(1e6 * (m.second - h->hmarks[0].second)));
    std::fprintf(stderr, "%s\n", line.c_str());
}

// after a stream sync: add the device time between events a and b to phase `slot`
void acc_time(insfm_ba* h, Ev a, Ev b, Phase slot) {
    if (!h->timing) return;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->ev[a], h->ev[b]) == hipSuccess) h->tms[slot] += ms;
}

// ---- phases --------------------------------------------------------------------------------------------------
// The main stream waits for the camera linearization on `aux` (before anything reads U / g_c).
int lin_join(insfm_ba* h) {
    if (!h->ss.lin_pending) return 0;
    HIPCHK(hipStreamWaitEvent(h->stream, h->ev_lc, 0));
    h->ss.lin_pending = false;
    return 0;
}

// The first trial's point preparation of a BA linearization (PointPrep): damping factor f = 1 + damping, records Y
// (and R_p) only when the poses are optimized (points-only solves have no Schur complement).
PointPrep first_trial_prep(insfm_ba* h) {
    PointPrep pp1;
    pp1.f = 1.0 + h->damping;
    pp1.cmin = h->d.clamp_min;
    pp1.cmax = h->d.clamp_max;
    pp1.Vinv = h->Vinv;
    pp1.y = h->y;
    pp1.R = h->d.optimize_poses ? h->Rf : nullptr;
    pp1.flags = h->flags;
    pp1.status = h->cg.status;
    return pp1;
}

template <int M>
void launch_lin_points_w(insfm_ba* h, const double* cams, const double* pts_local, const PointPrep& pp1) {
    k_lin_points<M><<<h->n_lin, kLinThreads, 0, h->stream>>>(h->lin_blk, h->pt_ptr, h->cam, h->ptl, h->uv, h->pp, cams,
                                                         pts_local, h->d.huber_delta, pp1.R ? h->W : nullptr, h->V, h->gp,
                                                         pp1, stamp_ptr(h, kStLinPoints));
}

// k_lin_cams on `stream`: the register form up to D = 9, else the LDS form.
template <int M>
void launch_lin_cams(insfm_ba* h, hipStream_t stream, const double* cams, const double* pts_local) {
    constexpr int D = kD<M>;
    if constexpr (D <= 9) {
        k_lin_cams_reg<M><<<h->C, LIN_CAMS_NT, 0, stream>>>(h->cam_ptr, h->cm_pt, h->cm_uv, h->pp, cams, pts_local,
                                                         h->d.huber_delta, h->U, h->gc);
    } else {
        const size_t lds = sizeof(double) * kThreads * (2 * D + 2);
        k_lin_cams<M><<<h->C, kThreads, lds, stream>>>(h->cam_ptr, h->cm_pt, h->cm_uv, h->pp, cams, pts_local,
                                                       h->d.huber_delta, h->U, h->gc);
    }
}

// The non-PD flag and the CG status word back to zero (where no k_final / k_point_prep in front does it).
int launch_zero_words(insfm_ba* h) {
    k_zero_words<<<1, 64, 0, h->stream>>>(h->flags, h->cg.status);
    return launch_err(h, "k_zero_words");
}

int run_linearize(insfm_ba* h, const double* cams, const double* pts_local) {
    h->ss.tl_fresh = true;
    if (h->kind == 1) {
        if (h->Nl > 0)
            k_gp_lin<<<cdiv(h->Nl, kThreads), kThreads, 0, h->stream>>>(h->Nl, h->cam, h->ptl, h->trans, h->fcam, h->sfree,
                                                                       cams, pts_local, h->scl_cur, h->d.huber_delta, h->gobs);
        k_gp_lin_cams<<<h->C, kThreads, 0, h->stream>>>(h->C, h->cam_ptr, h->cam_obs, h->gobs, h->U, h->gc);
        int rc = launch_err(h, "k_gp_lin");
        if (rc) return rc;
        return allreduce(h, h->U, (int64_t)h->C * h->D * h->D + (int64_t)h->C * h->D);
    }
    if (int rc0 = lin_join(h)) return rc0;  // (the previous linearization's U / g_c writes come first)
    // The first trial's point preparation rides along with k_lin_points (PointPrep): lm_step's first trial runs at
    // f = 1 + damping (config 3, same box, 3 runs each: 725 / 722 / 701 -> 733 / 725 / 734 LM it/s against a separate
    // k_point_prep launch; profiles/r3_v13/prep_fuse_ab.log).  The records Y_o depend on it (R_p).
    const PointPrep pp1 = first_trial_prep(h);
    h->ss.prep_valid = false;
    if (h->kind == 0 && h->Pl > 0) {
        if (h->ss.flags_dirty) {  // a solve without a cost left the flags / status set: clear them first (k_zero_words)
            if (int e = launch_zero_words(h)) return e;
            h->ss.flags_dirty = false;
        }
        h->ss.prep_valid = true;
        h->ss.prep_f = pp1.f;
    }
    int rc = with_model(h->model, [&](auto mc) -> int {
        constexpr int M = decltype(mc)::value;
        // k_lin_cams (compute-bound) forks after k_lin_points (HBM-bound) so that it overlaps k_schur (bound by
        // gather latency) instead of competing with k_lin_points for bandwidth
        if (h->Pl > 0) launch_lin_points_w<M>(h, cams, pts_local, pp1);
        if (!h->u_late) {
            launch_lin_cams<M>(h, h->stream, cams, pts_local);
            return launch_err(h, "linearize");
        }
        HIPCHK(hipEventRecord(h->ev_lin0, h->stream));
        HIPCHK(hipStreamWaitEvent(h->aux, h->ev_lin0, 0));
        launch_lin_cams<M>(h, h->aux, cams, pts_local);
        if (int e = launch_err(h, "k_lin_cams")) return e;
        HIPCHK(hipEventRecord(h->ev_lc, h->aux));
        h->ss.lin_pending = true;
        return launch_err(h, "k_lin_points");
    });
    if (rc) return rc;
    return allreduce(h, h->U, (int64_t)h->C * h->D * h->D + (int64_t)h->C * h->D);
}

// Two-level setup, part 1: coarse basis Z~ (on `basis_stream`, the CG needs it) and E into slot `slot` (on
// `build_stream`, which must already be ordered after the basis).
int run_tl_basis(insfm_ba* h, const double* cams, hipStream_t stream) {
    const int C = h->C;
    if (h->kind == 1) {
        if (h->ss.tl_solves == 0) {  // the first two-level solve since create / reset fixes the scale column's origin
            k_gp_tl_ref<<<cdiv(h->tl.nc, kThreads), kThreads, 0, stream>>>(cams, h->tl);
            if (int rc = launch_err(h, "k_gp_tl_ref")) return rc;
        }
        k_tl_basis<kGP><<<h->tl.nc, kThreads, 0, stream>>>(C, cams, h->Lf, h->tl, h->cg.r[0]);
        return launch_err(h, "k_tl_basis");
    }
    return with_model(h->model, [&](auto mc) -> int {
        constexpr int M = decltype(mc)::value;
        k_tl_basis<M><<<h->tl.nc, kThreads, 0, stream>>>(C, cams, h->Lf, h->tl, h->cg.r[0], stamp_ptr(h, kStBasis));
        return launch_err(h, "k_tl_basis");
    });
}

// The side stream's E build runs with at most kErowGrid workgroups (rows strided over the grid): with one workgroup
// per row it held CU / LDS slots the overlapping CG launches needed (config 3, round 1: grid 1000 / 512 / 384 / 256 /
// 192 / 128 -> 593 / 616 / 612-615 / 603 / 594 LM it/s).
constexpr int kErowGrid = 256;
int run_tl_build(insfm_ba* h, int slot, hipStream_t stream, bool have_oseg = false) {
    const int C = h->C, m = h->tl.m;
    TlBufs tl = h->tl;
    tl.E = h->Ebuf[slot];
    return with_D(h->D, [&](auto dc_) -> int {
        constexpr int DV = decltype(dc_)::value;
        const int grid = stream != h->stream ? std::min(C, kErowGrid) : C;
        if (!have_oseg)  // (k_tl_cgp wrote the segments of this solve)
            k_tl_erow<DV><<<grid, kThreads, 0, stream>>>(C, h->nbr_ptr, h->nbr_j, h->Sn, tl);
        k_tl_ereduce<DV><<<cdiv(m * m, kThreads), kThreads, 0, stream>>>(tl);
        return launch_err(h, "k_tl_erow/ereduce");
    });
}

// Two-level setup, part 2: unit u of E_slot's Gauss-Jordan inversion on `stream` (launch_gj_unit; the last writes
// Einvbuf[slot]).
int run_tl_gj_unit(insfm_ba* h, int slot, int u, hipStream_t stream) {
    launch_gj_unit(u, h->tl.m, h->Ebuf[slot], h->gjW, h->gjP, h->tl.Ed, h->Einvbuf[slot], h->okbuf + slot, stream);
    return launch_err(h, "k_gj_pinv0/k_gj_step");
}

// CG iterations the host keeps queued ahead of the device: 1 since late round 3 (config 3, same box, 3 runs each:
// 2 / 1 / 0 -> 714-721 / 722-726 / 720-727 LM it/s; every queued iteration a converged CG still runs costs ~9 us;
// profiles/r3_v12/cg_ahead_ab.log)
#ifndef CG_AHEAD
#define CG_AHEAD 1
#endif
#ifndef CG_INIT_BACK
#define CG_INIT_BACK 2
#endif
constexpr int kCgAhead = CG_AHEAD;

// The side-stream chain of solve `slot`: wait for the basis (ev_E), the E build (k_tl_erow, k_tl_ereduce), ev_built,
// then the Gauss-Jordan launches, the last followed by ev_fact[slot].  The whole chain (~20 launches) is issued at the
// solve's setup, while the GPU is still in k_lin_points / k_schur: the host is then ~0.6 ms ahead of the GPU, the
// launches cost the GPU nothing, and the chain overlaps the CG.  (Round 2 issued it piecemeal from the CG poll loop,
// and a chain deferred past the CG was measured too: both slower)
// set_timing: the device time of finished side chains (start after the wait on ev_E, end after the last Gauss-Jordan
// unit) into phase slot 6 of the current step.  A chain issued behind the CG usually finishes during the next step, so
// it is counted there; summed over the steps of a run every chain is counted once (but the last one).
void harvest_chain_time(insfm_ba* h) {
    for (int sl = 0; sl < 2; ++sl) {
        if (!h->chain_timed[sl] || hipEventQuery(h->ev[kEvChainEnd + sl]) != hipSuccess) continue;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, h->ev[kEvChain + sl], h->ev[kEvChainEnd + sl]) == hipSuccess) h->tms[kPhSideChain] += ms;
        h->chain_timed[sl] = false;
    }
}

int issue_side_chain(insfm_ba* h, int slot, bool have_oseg = false) {
    hipStream_t fs = h->side;
    HIPCHK(hipStreamWaitEvent(fs, h->ev_E, 0));
    const bool tm = h->timing && !h->chain_timed[slot];
    if (tm) HIPCHK(hipEventRecord(h->ev[kEvChain + slot], fs));
    if (int rc = run_tl_build(h, slot, fs, have_oseg)) return rc;
    h->ss.chain_oseg = have_oseg;
    HIPCHK(hipEventRecord(h->ev_built, fs));
    h->ss.built_pending = true;
    for (int u = 0; u <= gj_steps(h->tl.m); ++u)
        if (int rc = run_tl_gj_unit(h, slot, u, fs)) return rc;
    HIPCHK(hipEventRecord(h->ev_fact[slot], fs));
    if (tm) {
        HIPCHK(hipEventRecord(h->ev[kEvChainEnd + slot], fs));
        h->chain_timed[slot] = true;
    }
    return 0;
}

// Everything of the side chain finished (debug getters, kernel timing, destroy, reset).
int side_flush(insfm_ba* h) {
    if (h->side) HIPCHK(hipStreamSynchronize(h->side));
    return 0;
}

// Per-solve setup on the main stream (after k_cg_factor / k_cg_scale): the basis Z~, then this solve's side chain
// (E's build reads S~ and Z~: the next solve's k_cg_scale / k_tl_basis wait for ev_built, run_solve); the CG uses the
// previous solve's E^-1 under the lag rule, else its own and the main stream waits for the factorization (plan_solve).
int run_tl_setup(insfm_ba* h, const SolvePlan& p, const double* cams) {
    if (h->timing) harvest_chain_time(h);
    if (int rc = p.basis_by_factor ? 0 : run_tl_basis(h, cams, h->stream)) return rc;  // (k_cg_factor_basis formed it)
    h->ss.tl_fresh = false;
    // k_tl_cgp under the lag rule: this solve's chain runs after the CG (run_cgp records ev_E behind the CG; an
    // event record here as well would only cost the main queue a marker); else it runs now and the CG waits
    if (!p.defer_chain) {
        HIPCHK(hipEventRecord(h->ev_E, h->stream));
        if (int rc = issue_side_chain(h, p.slot)) return rc;
    }
    // a lagged solve's coarse inverse normally finished long ago: a completed event needs no wait marker in the main
    // queue (each one idles it a few us; always queueing it measured 659-665 vs 659-664 LM it/s, round 2)
    if (p.must_wait_fact || hipEventQuery(h->ev_fact[p.use]) != hipSuccess)
        HIPCHK(hipStreamWaitEvent(h->stream, h->ev_fact[p.use], 0));
    h->tl.Einv = h->Einvbuf[p.use];
    h->tl.ok = h->okbuf + p.use;
    ++h->ss.tl_solves;
    return 0;
}

// k_tl_pc / k_tl_pspmv of iteration `it` (-1: the setup) on the buffers `tl`; k_tl_pspmv for `rows` rows, which a
// row-partitioned handle writes into every rank's window (xp).
template <int D>
void launch_pc(insfm_ba* h, int it, int maxit, double tol2, const TlBufs& tl) {
    k_tl_pc<D><<<h->tl.nc, kPcThreads, h->pc_lds, h->stream>>>(it, h->C, maxit, tol2, h->pc_rows, h->cg, tl, h->tl.Einv);
}
template <int D>
void launch_pspmv(insfm_ba* h, int it, int rows, const TlBufs& tl, const XPart& xp = XPart{}) {
    k_tl_pspmv<D><<<rows, kPspmvThreads, 0, h->stream>>>(it, h->C, h->nbr_stride, h->nbr_ptr, h->nbr_j, h->Sn, h->Lf,
                                                          h->cg, tl, xp);
}

// Launch `it` of the two-level CG: update (recurrence step it-1 when it >= 1; restriction always), coarse
// correction, S~ u.
template <int D>
void launch_tl_iter(insfm_ba* h, int it, int maxit, double tol2) {
    if (it == 0) {  // setup: u0 = M~^-1 r0 (k_tl_basis formed r0's restriction), w0 = S~ u0, the partials of iteration 0
        launch_pc<D>(h, -1, maxit, tol2, h->tl);
        launch_pspmv<D>(h, -1, h->C, h->tl);
    }
    if (h->tl.Racc)  // per-cluster atomic sums of the row partials (single rank, non-deterministic)
        k_tl_pc_cl<D><<<h->tl.nc, kPcThreads, 0, h->stream>>>(it, h->C, maxit, tol2, h->cg, h->tl, h->tl.Einv);
    else
        launch_pc<D>(h, it, maxit, tol2, h->tl);
    launch_pspmv<D>(h, it, h->C, h->tl);
}

// TlBufs whose exchanged buffers (vc, gd, rowR) are window region q of a partitioned handle
TlBufs tl_region(const insfm_ba* h, int q) {
    TlBufs t = h->tl;
    const int C = h->C, D = h->D;
    double* base = h->xwin + h->xoff_region[q];
    t.vc = base;
    t.gd = base + (size_t)C * D;
    t.rowR = base + (size_t)C * D + 3 * (size_t)C;
    return t;
}

XPart xpart_region(const insfm_ba* h, int q) {
    XPart xp;
    xp.win = h->xbases;
    xp.world = h->d.world_size;
    xp.q0 = h->xq[h->d.rank];
    xp.off_vc = h->xoff_region[q];
    xp.off_gd = xp.off_vc + (long long)h->C * h->D;
    xp.off_rowR = xp.off_gd + 3LL * h->C;
    return xp;
}

// One exchange of the partitioned CG (slot 0: iterations, skipped once the CG status is set; 1: solution gather)
void launch_xchg(insfm_ba* h, int slot) {
    k_xsignal<<<1, 64, 0, h->stream>>>(h->cg.status, h->xcnt, h->xpflags, h->d.world_size, h->d.rank, slot);
    k_xwait<<<1, 64, 0, h->stream>>>(h->cg.status, h->cg.prog, h->xcnt,
                                     reinterpret_cast<unsigned*>(h->xwin + h->xoff_flags), h->d.world_size, slot);
}

// launch_tl_iter for a row-partitioned handle: k_tl_pc replicated on region it & 1, this rank's rows of k_tl_pspmv
// writing region (it + 1) & 1 of every window, then the exchange
template <int D>
void launch_tl_iter_x(insfm_ba* h, int it, int maxit, double tol2) {
    const int nrows = h->xq[h->d.rank + 1] - h->xq[h->d.rank];
    auto pspmv = [&](int i) {
        if (nrows > 0) launch_pspmv<D>(h, i, nrows, tl_region(h, i & 1), xpart_region(h, (i + 1) & 1));
        launch_xchg(h, 0);
    };
    if (it == 0) {  // setup (k_tl_basis wrote r0 and its restriction into region 1)
        launch_pc<D>(h, -1, maxit, tol2, tl_region(h, 1));
        pspmv(-1);
    }
    launch_pc<D>(h, it, maxit, tol2, tl_region(h, it & 1));
    pspmv(it);
}

// Iterations [from, to) of the two-level CG on the launch path (the row-partitioned form on a partitioned handle).
template <int D>
void launch_tl_iters(insfm_ba* h, int from, int to, int maxit, double tol2) {
    for (int k = from; k < to; ++k)
        if (h->xpart) launch_tl_iter_x<D>(h, k, maxit, tol2);
        else launch_tl_iter<D>(h, k, maxit, tol2);
}

// The k_tl_cgp instantiation for NB blocks per row (64 / 128), the fixed-order form (det) and A-DEF2 (adef).
using CgpKernel = decltype(&k_tl_cgp<64, false, false>);
CgpKernel cgp_kernel(int nb, bool det, bool adef) {
    if (nb == 64) {
        if (det) return adef ? k_tl_cgp<64, true, true> : k_tl_cgp<64, true, false>;
        return adef ? k_tl_cgp<64, false, true> : k_tl_cgp<64, false, false>;
    }
    if (det) return adef ? k_tl_cgp<128, true, true> : k_tl_cgp<128, true, false>;
    return adef ? k_tl_cgp<128, false, true> : k_tl_cgp<128, false, false>;
}

// k_tl_cgp's grid-barrier counters and the host's count of the barriers they have seen, both back to zero.
int cgp_reset_barriers(insfm_ba* h) {
    HIPCHK(hipMemsetAsync(h->cgp_sync, 0, sizeof(unsigned) * kCgpSyncWords, h->stream));
    h->ss.cgp_epochs = 0;
    return 0;
}

// The whole two-level CG of a solve on the persistent k_tl_cgp (D = 8, h->cgp_nb > 0): one launch for the coarse
// solve of r0 (u0 = M~^-1 r0, formerly k_tl_pc's setup launch), the setup's operator product and every iteration.
// adef2: the coarse correction as A-DEF2 (else additive); write_segments: the coarse segments for a side chain behind
// the CG.  The restriction of r0 is where the last planned solve (h->last) formed it.
int launch_tl_cgp(insfm_ba* h, bool adef2, bool write_segments) {
    const int maxit = h->d.pcg_max_iter;
    const double tol2 = h->d.pcg_tol * h->d.pcg_tol;
    if (h->ss.cgp_epochs > (1u << 24))  // (counter headroom: zero them now and then; an abort zeroes them too)
        if (int rc = cgp_reset_barriers(h)) return rc;
    // INSFM_DIAG=cgp_fault (tests): the first launch of the process aborts at iteration 2
    static std::atomic<int> faults{diag("cgp_fault") ? 1 : 0};
    const bool fault = faults.load() > 0 && faults.fetch_sub(1) > 0;
    // INSFM_DIAG=adef2_breakdown (tests): the first A-DEF2 launch of the process reports a breakdown at iteration 2
    static std::atomic<int> bkdn{diag("adef2_breakdown") ? 1 : 0};
    const bool breakdown = adef2 && bkdn.load() > 0 && bkdn.fetch_sub(1) > 0;
    hipLaunchKernelGGL(cgp_kernel(h->cgp_nb, h->cgp_det, adef2), dim3(h->cgp_grid), dim3(kCgpThreads), 0, h->stream,
                       h->C, h->nbr_ptr, h->nbr_j, (const double*)h->S, (const int*)h->cgp_src, (const double*)h->Li,
                       (const double*)h->Lf, h->cg, h->tl, (const double*)h->tl.Einv, maxit, tol2, h->cgp_wx, h->cgp_yg,
                       h->ss.cgp_tag, h->cgp_sync, h->ss.cgp_epochs,
                       cgp_flag_word(write_segments, fault, breakdown, !h->last.basis_by_factor), h->cgp_runs,
                       h->cgp_trace, h->dc, stamp_ptr(h, kStCgp));
    if (int rc = launch_err(h, "k_tl_cgp")) return rc;
    h->ss.cgp_tag += (unsigned)maxit + 3u;  // (the tags of this launch are never reused)
    return 0;
}

// The k_schur instantiation a handle launches (run_solve) and whose dynamic-LDS limit create raises.  BA: by D, the
// ordered-LDS-add form in deterministic mode, the M_p form for a retried trial.  Global positioning: D = 3 with the
// compact W record in deterministic mode; null otherwise (k_schur_gp, a kernel with its own argument list).
using SchurKernel = decltype(&k_schur<8, kSchurWaves>);
SchurKernel schur_kernel(int kind, int D, bool det, bool retry) {
    if (kind == 1) return det ? k_schur<3, kDetWaves, true, false, SCHUR_DET_ORD> : nullptr;
    SchurKernel k = nullptr;
    with_ba_D(D, [&](auto dc_) -> int {
        constexpr int DV = decltype(dc_)::value;
        if (det) k = retry ? k_schur<DV, kDetWaves, false, true, SCHUR_DET_ORD> : k_schur<DV, kDetWaves, false, false, SCHUR_DET_ORD>;
        else k = retry ? k_schur<DV, kSchurWaves, false, true> : k_schur<DV, kSchurWaves>;
        return 0;
    });
    return k;
}

// k_schur for the handle's kind on work items [w0, w1) (BA's chunked exchange; default: all).
int launch_schur(insfm_ba* h, double sf, double smin, double smax, int sdiag, bool retry, int w0 = 0, int w1 = -1) {
    const bool det = h->d.deterministic != 0, gpk = h->kind == 1;
    // global positioning: the scale-eliminated blocks are already damped, so k_schur takes U' / g'_c as they are
    const double *Uin = gpk ? h->Up : h->U, *gcin = gpk ? h->gpc : h->gc;
    if (w1 < 0) w1 = h->nwork;
    const int nt = det ? kDetWaves * 64 : kSchurWaves * 64;
    const SchurKernel kern = schur_kernel(h->kind, h->D, det, retry);
    if (gpk && !kern) {
        k_schur_gp<kSchurWaves, kGPSG><<<h->nwork, nt, h->schur_lds, h->stream>>>(
            h->work, h->row_ptr, h->col, h->C, h->cam_ptr, h->sdesc, h->cam, h->W, h->VY, Uin, gcin, h->S, h->b);
        return launch_err(h, "k_schur");
    }
    if (!kern) return INSFM_BA_EINVAL;
    if (!gpk && w1 <= w0) return 0;
    hipLaunchKernelGGL(kern, dim3(w1 - w0), dim3(nt), h->schur_lds, h->stream, h->work + w0, h->row_ptr, h->col, h->C,
                       h->cam_ptr, h->cam_obs, h->ptl, h->pt_ptr, h->ustart, h->sdesc, h->cam, h->W,
                       gpk ? h->Vinv : h->Mp, h->y, Uin, gcin, sf, smin, smax, sdiag, h->S, h->b,
                       gpk ? nullptr : stamp_ptr(h, kStSchur));
    return launch_err(h, "k_schur");
}

// INSFM_DIAG=cgp_trace: what the finished k_tl_cgp launch (status st) recorded, to stderr.
int print_cgp_trace(insfm_ba* h, const int* st) {
    double tr[kCgpTraceLen];
    HIPCHK(hipMemcpy(tr, h->cgp_trace, sizeof(tr), hipMemcpyDeviceToHost));
    const int n = std::min(st[1], 63);
    std::fprintf(stderr, "[insfm cgp] status %d iterations %d coarse %d: setup %.1f us (blocks + tables %.1f, A %.1f, "
                 "rest %.1f), iterations %.1f us (%.2f us each)\n",
                 st[0], st[1], st[2], 0.01 * (tr[257] - tr[256]), 0.01 * (tr[578] - tr[256]),
                 0.01 * (tr[579] - tr[578]), 0.01 * (tr[257] - tr[579]), 0.01 * (tr[258 + n] - tr[257]),
                 n > 0 ? 0.01 * (tr[258 + n] - tr[258]) / n : 0.0);
    for (int k = 0; k <= n; ++k) {
        std::fprintf(stderr, "[insfm cgp]   it %d gamma %.17g delta %.17g rho %.17g done %g t %.1f us | loads %.2f P1 %.2f y %.2f "
                     "P2 %.2f B2 %.2f\n", k, tr[4 * k], tr[4 * k + 1], tr[4 * k + 2], tr[4 * k + 3], 0.01 * (tr[258 + k] - tr[256]),
                     k > 0 ? 0.01 * (tr[258 + k] - tr[322 + 4 * (k - 1) + 3]) : 0.0,
                     0.01 * (tr[322 + 4 * k] - tr[258 + k]), 0.01 * (tr[323 + 4 * k] - tr[322 + 4 * k]),
                     0.01 * (tr[324 + 4 * k] - tr[323 + 4 * k]), 0.01 * (tr[325 + 4 * k] - tr[324 + 4 * k]));
        if (k < n)
            std::fprintf(stderr, "[insfm cgp]        P1 split: fills + workgroup barrier %.2f, y %.2f, S~w %.2f; "
                         "scalar partials in %.2f after the barrier\n",
                         0.01 * (tr[580 + 3 * k] - tr[258 + k]), 0.01 * (tr[581 + 3 * k] - tr[580 + 3 * k]),
                         0.01 * (tr[322 + 4 * k] - tr[581 + 3 * k]),
                         k > 0 ? 0.01 * (tr[582 + 3 * k] - tr[322 + 4 * (k - 1) + 3]) : 0.0);
    }
    const int G = std::min(h->cgp_grid, 256);
    if (st[1] > kCgpTraceIt + 1 && G > 0) {  // every workgroup's start and end of iteration kCgpTraceIt
        double s0 = tr[772], s1 = tr[772];
        for (int b = 0; b < G; ++b) { s0 = std::min(s0, tr[772 + b]); s1 = std::max(s1, tr[772 + b]); }
        std::vector<int> ord(G);
        for (int b = 0; b < G; ++b) ord[b] = b;
        std::sort(ord.begin(), ord.end(), [&](int a, int b) { return tr[1028 + a] > tr[1028 + b]; });
        std::fprintf(stderr, "[insfm cgp] it %d per workgroup: starts within %.2f us; arrival at the barrier "
                     "(us after the first start): median %.2f, last %.2f; latest:", kCgpTraceIt, 0.01 * (s1 - s0),
                     0.01 * (tr[1028 + ord[G / 2]] - s0), 0.01 * (tr[1028 + ord[0]] - s0));
        for (int q = 0; q < std::min(G, 8); ++q)
            std::fprintf(stderr, " wg %d (%.2f, start %.2f)", ord[q], 0.01 * (tr[1028 + ord[q]] - s0),
                         0.01 * (tr[772 + ord[q]] - s0));
        std::fprintf(stderr, "\n");
    }
    return 0;
}

// The k_tl_cgp launch of this solve has finished (the host saw its status word, or the trial's k_publish behind
// it): its status {status, iterations, coarse used} into st, the barrier bookkeeping, an abort's fallback, the trace.
// adef2: how the launch applied the coarse correction (launch_tl_cgp).
int cgp_complete(insfm_ba* h, bool adef2, int* st) {
    std::atomic_thread_fence(std::memory_order_seq_cst);
    volatile int* pg = h->prog_host;
    st[0] = pg[1]; st[1] = pg[2]; st[2] = pg[3];
    if (st[0] == 1 || st[0] == 2) {  // the barriers this launch counted; an abort restarts the counters
        h->ss.cgp_epochs += cgp_barriers(adef2, st[1]);
    } else {
        HIPCHK(hipStreamSynchronize(h->stream));
        if (int rc = cgp_reset_barriers(h)) return rc;
        // a barrier timed out: the grid was not resident at once (another process's kernels held CUs).  A single
        // rank drops the persistent CG for good and run_solve repeats this solve on the launch path; a rank of a
        // replicated multi-rank CG cannot (its peers would compute a dc that differs in rounding) and reports it.
        if (st[0] == 4 && h->d.world_size <= 1 && !h->xpart) {
            std::fprintf(stderr, "[insfm] k_tl_cgp: a grid barrier timed out (the GPU is shared with another "
                                 "process?); this handle continues on the launch-per-iteration CG\n");
            h->cgp_nb = 0;
            h->ss.cgp_lost = true;
        }
    }
    return h->cgp_trace ? print_cgp_trace(h, st) : 0;
}

// The two-level CGs the host polls (run_launch_cg, run_cgp): no stream sync inside the CG.  The lead workgroup
// publishes its progress into host-mapped memory and the host's loop ends when the status word turns non-zero.
// INSFM_DIAG=trace: per solve, host microseconds spent enqueueing CG iterations and the longest single call.
struct CgStart {
    // multi-rank: the CG's first launch waits for the exchange (the slowest peer); the stall deadline starts once
    // everything queued in front of the CG has completed (ev_pre), and that gate has its own longer deadline
    bool gated = false, htrace = false;
    double t_sol0 = 0.0, t_enq = 0.0, m_enq = 0.0;
    int n_enq = 0;
};

// In front of the CG's first launch: the progress word back to zero, the phase marker, the multi-rank gate.
int cg_begin(insfm_ba* h, CgStart& cs) {
    volatile int* pg = h->prog_host;
    pg[0] = pg[1] = pg[2] = pg[3] = 0;
    std::atomic_thread_fence(std::memory_order_seq_cst);
    static const bool htrace = diag("trace");
    cs.htrace = htrace;
    cs.t_sol0 = htrace ? wall_seconds() : 0.0;
    rec(h, kEvCg);
    cs.gated = h->d.world_size > 1 || h->d.allreduce;
    if (cs.gated) HIPCHK(hipEventRecord(h->ev_pre, h->stream));
    return 0;
}

// The host poll loop of a CG with *enq iterations queued: `enqueue(from, to)` tops them up while the GPU has fewer than
// kCgAhead pending; ends when the status word turns non-zero.  Then the CG's end marker and (set_timing) its time.
template <typename Enqueue>
int cg_wait(insfm_ba* h, CgStart& cs, int* enq, Enqueue&& enqueue) {
    volatile int* pg = h->prog_host;
    CgPoll poll;
    poll.enq = *enq;
    const double stall_s = cg_stall_limit();
    int erc = 0;
    const int pr = cg_poll(
        poll, h->d.pcg_max_iter + 2, kCgAhead, stall_s, cg_gate_limit_s(stall_s), [&] { return (int)pg[1]; },
        [&] { return (int)pg[0]; }, enqueue,
        [&] {
            const hipError_t q = hipStreamQuery(h->stream);
            if (q == hipSuccess) { std::atomic_thread_fence(std::memory_order_seq_cst); return 0; }
            return q == hipErrorNotReady ? 1 : -1;
        },
        wall_seconds, [] { cpu_relax(); },
        [&] { return !cs.gated || hipEventQuery(h->ev_pre) != hipErrorNotReady; }, &erc);
    hmark(h, "cg converged");
    if (cs.htrace)
        std::fprintf(stderr, "[insfm host] solve %.1f us: %d iterations enqueued in %.1f us (max %.1f per iteration)\n",
                     1e6 * (wall_seconds() - cs.t_sol0), cs.n_enq, 1e6 * cs.t_enq, 1e6 * cs.m_enq);
    *enq = poll.enq;
    if (pr == CgPoll::kEnqueueError) return erc;
    if (pr == CgPoll::kStreamError) {
        h->err = std::string("PCG: ") + hipGetErrorString(hipStreamQuery(h->stream));
        return INSFM_BA_EHIP;
    }
    if (pr == CgPoll::kStalled || pr == CgPoll::kGateStalled) {
        h->err = std::string(pr == CgPoll::kGateStalled ? "PCG: the cross-rank exchange in front of the CG did not "
                                                          "complete within "
                                                        : "PCG: no progress from the device for ") +
                 std::to_string(poll.stalled_s) + " s (iterations started " + std::to_string(pg[0]) + ", status " +
                 std::to_string(pg[1]) + ", enqueued " + std::to_string(*enq) +
                 "); set INSFM_CG_STALL_S to change the limit";
        return INSFM_BA_EHIP;
    }
    std::atomic_thread_fence(std::memory_order_seq_cst);
    rec(h, kEvCgEnd);
    if (h->timing) {
        HIPCHK(hipStreamSynchronize(h->stream));
        acc_time(h, kEvCg, kEvCgEnd, kPhCgLaunches);
    }
    return 0;
}

// The whole two-level CG of a solve as one k_tl_cgp launch (adef2: launch_tl_cgp).  defer_chain: this solve's side
// chain is issued behind the CG, from the segments the launch writes (SolvePlan).  async: return with the status unread
// (st = converged, 0 iterations; cgp_pending); else wait for the status word and complete the launch (cgp_complete).
int run_cgp(insfm_ba* h, bool adef2, bool defer_chain, bool async, int* st) {
    CgStart cs;
    if (int rc = cg_begin(h, cs)) return rc;
    if (int rc = launch_tl_cgp(h, adef2, defer_chain)) return rc;
    if (defer_chain) {
        // (INSFM_DIAG=chain_hold, timing only: no lagged chain at all -- later solves keep an older coarse inverse --
        // to measure what the chain's overlap costs the kernels it runs beside)
        static const bool hold = diag("chain_hold");
        if (!hold) HIPCHK(hipEventRecord(h->ev_E, h->stream));
        if (hold) h->ss.chain_oseg = false;
        else if (int rc = issue_side_chain(h, h->last.slot, true)) return rc;
    }
    if (async) {
        // one launch runs the whole CG and the kernels behind it need no host decision: the host queues them at once
        // and reads the CG status after the trial's k_publish (cgp_complete), which accepts the trial only for a
        // converged CG.  (Waiting here for the status word cost a host round trip and a launch from an idle queue
        // between the CG and k_cg_finish.)
        rec(h, kEvCgEnd);
        h->cg_launches += 1;
        h->ss.cgp_pending = true;
        st[0] = 1; st[1] = 0; st[2] = 1;
        return 0;
    }
    int enq = h->d.pcg_max_iter + 2;  // (one launch runs every iteration: the poll has nothing to top up)
    if (int rc = cg_wait(h, cs, &enq, [](int, int) { return 0; })) return rc;
    h->cg_launches += 1;
    return cgp_complete(h, adef2, st);
}

// The two-level CG on the launch path (k_tl_pc_cl / k_tl_pc + k_tl_pspmv per iteration; the row-partitioned form):
// a first batch sized by the last solve's count, then the poll tops up.  The few iterations enqueued past convergence
// exit at the device status flag.  Returns 0 with st[0..2] = {status, iterations, coarse used}.
int run_launch_cg(insfm_ba* h, int* st) {
    const int maxit = h->d.pcg_max_iter;
    const double tol2 = h->d.pcg_tol * h->d.pcg_tol;
    CgStart cs;
    if (int rc = cg_begin(h, cs)) return rc;
    auto enqueue = [&](int from, int to) -> int {
        const double t0 = cs.htrace ? wall_seconds() : 0.0;
        const int r = with_D(h->D, [&](auto dc_) -> int {
            launch_tl_iters<decltype(dc_)::value>(h, from, to, maxit, tol2);
            return launch_err(h, "k_tl_pc/k_tl_pspmv");
        });
        if (cs.htrace) {
            const double dt = wall_seconds() - t0;
            cs.t_enq += dt; cs.m_enq = std::max(cs.m_enq, dt / std::max(1, to - from)); cs.n_enq += to - from;
        }
        return r;
    };
    int enq = cg_first_batch(h->ss.last_cg_iters, maxit, kCgAhead, CG_INIT_BACK);
    if (int rc = enqueue(0, enq)) return rc;
    if (int rc = cg_wait(h, cs, &enq, enqueue)) return rc;
    h->cg_launches += enq;
    volatile int* pg = h->prog_host;
    st[0] = pg[1]; st[1] = pg[2]; st[2] = pg[3];
    return 0;
}

// The block-Jacobi CG (precond 0, or the two-level path without host-mapped memory): launches in chunks, a status
// copy and a stream sync per chunk.
int run_bj_cg(insfm_ba* h, int* st) {
    const int D = h->D, maxit = h->d.pcg_max_iter;
    const double tol2 = h->d.pcg_tol * h->d.pcg_tol;
    int it = 0;
    for (;;) {
        // the count grows by a few iterations per LM step as the damping drops: launch past the last count so most
        // solves need one host poll (a converged iteration costs ~1 us per launch: its kernels exit at the flag)
        const int chunk = (it == 0) ? std::max(8, h->ss.last_cg_iters + 6) : 8;
        const int stop = std::min(it + chunk, maxit + 2);
        rec(h, kEvCg);
        const int rc = with_D(D, [&](auto dc_) -> int {
            constexpr int DV = decltype(dc_)::value;
            if (h->tlon) launch_tl_iters<DV>(h, it, stop, maxit, tol2);
            else for (int k = it; k < stop; ++k) {
                if (k > 0) k_cg_dots<<<1, 64, 0, h->stream>>>(k, h->C, maxit, tol2, h->cg);
                k_cg_iter<DV><<<h->C, kCgThreads, 0, h->stream>>>(k, h->C, maxit, tol2, h->nbr_ptr, h->nbr_j, h->Sn,
                                                                h->Lf, h->cg);
            }
            return launch_err(h, "k_cg_iter");
        });
        if (rc) return rc;
        rec(h, kEvCgEnd);
        h->cg_launches += stop - it;
        it = stop;
        HIPCHK(hipMemcpyAsync(st, h->cg.status, sizeof(int) * 3, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        acc_time(h, kEvCg, kEvCgEnd, kPhCgLaunches);
        if (st[0] != 0 || it >= maxit + 2) break;
    }
    return 0;
}

// After the CG of a solve: its status (breakdown -> ESOLVER), the partitioned CG's solution gather, dc = L^-T x.
// dc_by_cgp: k_tl_cgp wrote dc itself (no k_cg_finish).  Returns the PCG iterations (0 while a k_tl_cgp status is
// still pending) or an error.
int cg_tail(insfm_ba* h, bool dc_by_cgp, int* st) {
    const int D = h->D;
    int rc = 0;
    if (st[0] != 1) {
        h->err = pcg_status_message(st[0], st[1], h->tlon ? st[2] : kCoarseOff);
        return st[0] == 4 ? INSFM_BA_EHIP : INSFM_BA_ESOLVER;
    }
    if (!h->ss.cgp_pending) {
        h->coarse_used = h->tlon ? st[2] : 0;
        h->ss.last_cg_iters = st[1];
    }
    if (h->xpart) {  // partitioned CG: every rank's solution rows into every window, then into cg.x
        const int n = h->xq[h->d.rank + 1] - h->xq[h->d.rank];
        if (n > 0)
            k_xput_x<<<cdiv((long long)n * D, 256), 256, 0, h->stream>>>(n, D, h->tl.cl_cams, h->cg.x,
                                                                        xpart_region(h, 0), h->xoff_xg);
        launch_xchg(h, 1);
        HIPCHK(hipMemcpyAsync(h->cg.x, h->xwin + h->xoff_xg, sizeof(double) * (size_t)h->C * D,
                              hipMemcpyDeviceToDevice, h->stream));
        if ((rc = launch_err(h, "partitioned CG gather"))) return rc;
        int sw[2] = {0, 0};  // (prototype path: one synchronization to see a gather that timed out)
        HIPCHK(hipMemcpyAsync(sw, h->cg.status, sizeof(sw), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (sw[0] == 4) {
            h->err = "partitioned CG: the solution gather across ranks timed out";
            return INSFM_BA_EHIP;
        }
    }
    if (dc_by_cgp) return h->ss.cgp_pending ? 0 : st[1];
    rc = with_D(D, [&](auto dc_) -> int {
        constexpr int DV = decltype(dc_)::value;
        k_cg_finish<DV><<<cdiv((long long)h->C * DV, kThreads), kThreads, 0, h->stream>>>(h->C, h->Li, h->cg.x,
                                                                                        h->dc, stamp_ptr(h, kStCgFinish));
        return launch_err(h, "k_cg_finish");
    });
    if (rc) return rc;
    hmark(h, "cg_finish");
    return h->ss.cgp_pending ? 0 : st[1];
}

// k_cg_scale: the scaled copy Sn of S~ (both triangles, row-contiguous) for the launch-path kernels.
template <int DV>
void launch_scale(insfm_ba* h) {
    k_cg_scale<DV><<<cdiv(h->nnzb, kWaves * scale_nb(DV)), kThreads, 0, h->stream>>>(
        h->nnzb, h->blk_row, h->col, h->row_ptr, h->pos_up, h->pos_lo, h->Li, h->S, h->Sn, 0);
}

// The scaled copy Sn of the current solve's S~ (k_cg_scale), for consumers that read it when the solve skipped it
// (k_tl_cgp's lagged solves): the launch-path CG after an abort, the debug timing of launch-path kernels.
int ensure_sn(insfm_ba* h) {
    if (h->ss.sn_valid || h->kind != 0 || !h->d.optimize_poses) return 0;
    const int rc = with_D(h->D, [&](auto dc_) -> int {
        launch_scale<decltype(dc_)::value>(h);
        return launch_err(h, "k_cg_scale");
    });
    if (!rc) h->ss.sn_valid = true;
    return rc;
}

// After a k_tl_cgp abort: the basis was formed again on the main stream; a side chain issued from the launch's coarse
// segments (incomplete when a workgroup never got past the A build) is issued once more from S~ / Z~ (k_tl_erow),
// behind the first on the side stream, so the next solve's coarse inverse is this solve's.
int reissue_chain(insfm_ba* h) {
    if (!h->ss.chain_oseg) return 0;
    h->ss.chain_oseg = false;
    HIPCHK(hipEventRecord(h->ev_E, h->stream));
    return issue_side_chain(h, h->last.slot);
}

// The block-Jacobi factorization L, L^-1 and r0 = L^-1 b: with the coarse basis at `basis_cams` in the same launch
// (k_cg_factor_basis) when they are given, else k_cg_factor.  add_U: U / g_c join S / b here (u_late).  first: the
// solve's own launch (the descriptor's clamps, stamped); a repeat on the completed S / b passes add_U = false, f = 1
// and gets the same L, L^-1 and r0.
template <int DV>
void launch_factor(insfm_ba* h, double f, bool add_U, const double* basis_cams, bool first = false) {
    const double *U = add_U ? h->U : nullptr, *gc = add_U ? h->gc : nullptr;
    const double cmin = first ? h->d.clamp_min : 0.0, cmax = first ? h->d.clamp_max : 0.0;
    long long* stamp = first ? stamp_ptr(h, kStFactor) : nullptr;
    if constexpr (DV != 3) {
        if (basis_cams) {
            k_cg_factor_basis<DV><<<cdiv(h->C, kWaves), kThreads, 0, h->stream>>>(
                h->C, h->row_ptr, h->S, h->b, h->Lf, h->Li, h->cg, U, gc, f, cmin, cmax, basis_cams, h->tl,
                h->cgp_runs + (size_t)h->cgp_grid * kCgpRows * 12, stamp);
            return;
        }
    }
    k_cg_factor<DV><<<cdiv(h->C, kWaves), kThreads, 0, h->stream>>>(h->C, h->row_ptr, h->S, h->b, h->Lf, h->Li, h->cg, U,
                                                                   gc, f, cmin, cmax, stamp);
}

// The back-substitution and the trial parameters of a solve (dcp: the camera step, null for a points-only solve).
int solve_tail(insfm_ba* h, double f, const double* cams, const double* pts_local, const double* dcp) {
    const bool gpk = h->kind == 1;
    rec(h, kEvBacksub);
    if (gpk) {
        if (h->Pl > 0)
            k_gp_backsub<kGPG><<<h->n_gp_grp, kThreads, 0, h->stream>>>(h->Pl, h->pt_ptr, h->cam, h->gobs, dcp, h->Vinv, h->gp,
                                                              pts_local, h->scl_cur, f, h->d.clamp_min, h->d.clamp_max, h->dp,
                                                              h->pts_new, h->scl_new, h->ds, h->part_gp);
        k_gp_update_cams<<<cdiv(3 * h->C, kThreads), kThreads, 0, h->stream>>>(3 * h->C, cams, dcp, h->cams_new);
        return launch_err(h, "k_gp_backsub/update");
    }
    if (int rc0 = lin_join(h)) return rc0;  // the camera update reads U / g_c (points-only solves skip the factor)
    const int rc = with_model(h->model, [&](auto mc) -> int {
        constexpr int M = decltype(mc)::value;
        const int nrun = h->Pl > 0 ? h->n_lin : 0;  // point runs, then the camera-update blocks
        k_backsub_rc<M><<<nrun + h->n_gc, kLinThreads, 0, h->stream>>>(
            h->lin_blk, h->pt_ptr, h->cam, h->ptl, h->uv, h->pp, cams, h->d.huber_delta, dcp, h->V, h->Vinv, h->gp,
            pts_local, h->dp, h->pts_new, h->part_gp, nrun, h->C, h->U, h->gc, h->d.rank == 0, h->cams_new, h->part_gc,
            stamp_ptr(h, kStBacksub));
        return launch_err(h, "k_backsub_rc");
    });
    if (rc) return rc;
    hmark(h, "backsub");
    return 0;
}

// The factorization again on the completed S / b (no U / g_c added: the same L, L^-1 and r0 = L^-1 b); with the
// coarse basis in the same launch when `basis_cams` is given.
int refactor(insfm_ba* h, const double* basis_cams) {
    return with_D(h->D, [&](auto dc_) -> int {
        launch_factor<decltype(dc_)::value>(h, 1.0, false, basis_cams);
        return launch_err(h, basis_cams ? "k_cg_factor_basis" : "k_cg_factor");
    });
}

// The CG of the last solve once more, after a k_tl_cgp launch that did not converge: the steps of `r`
// (solve_policy.h repeat_recipe) in their one order, around the current cameras.  st: the new CG's status.
int repeat_cg(insfm_ba* h, const RepeatRecipe& r, int* st) {
    const auto has = [&](RepeatStep s) { return (r.steps & s) != 0; };
    int rc = 0;
    h->ss.cgp_lost = false;
    if (has(kStepLeavePersistent)) {
        h->cgp_nb = 0;
        HIPCHK(hipStreamSynchronize(h->stream));
        if ((rc = cgp_reset_barriers(h))) return rc;
    }
    if (has(kStepZeroStatus)) HIPCHK(hipMemsetAsync(h->cg.status, 0, sizeof(int) * 4, h->stream));
    if (has(kStepFactorize) && (rc = refactor(h, r.factor_with_cams ? h->cams_cur : nullptr))) return rc;
    if (has(kStepEnsureSn) && (rc = ensure_sn(h))) return rc;
    if (has(kStepBasis) && (rc = run_tl_basis(h, h->cams_cur, h->stream))) return rc;
    if (has(kStepReissueChain) && (rc = reissue_chain(h))) return rc;
    if (!has(kStepRunCg)) return 0;
    return r.additive ? run_cgp(h, false, false, false, st) : run_launch_cg(h, st);
}

SolveFacts solve_facts(const insfm_ba* h, bool async_status) {
    SolveFacts s;
    s.kind = h->kind; s.optimize_poses = h->d.optimize_poses != 0; s.tlon = h->tlon;
    s.prog_host = h->prog_host != nullptr; s.cgp = h->cgp_nb != 0; s.u_late = h->u_late;
    s.rank0 = h->d.rank == 0; s.has_points = h->Pl > 0; s.keep_S = h->keep_S != 0;
    s.clamp_min = h->d.clamp_min; s.clamp_max = h->d.clamp_max;
    s.flags_dirty = h->ss.flags_dirty; s.prep_valid = h->ss.prep_valid; s.prep_f = h->ss.prep_f;
    s.tl_solves = h->ss.tl_solves; s.tl_fresh = h->ss.tl_fresh; s.async_status = async_status;
    return s;
}

// Build S/b for factor f, solve, back-substitute and form the trial parameters (cams / pts_local: the handle's current
// parameters).  async_status: a k_tl_cgp solve returns with its status unread (the caller reads it behind the trial's
// cost).  Returns PCG iterations (>= 0), INSFM_BA_ESOLVER on breakdown, or another negative code.
int run_solve(insfm_ba* h, double f, const double* cams, const double* pts_local, bool async_status) {
    const int D = h->D;
    const SolvePlan p = h->last = plan_solve(solve_facts(h, async_status), f);
    h->ss.prep_valid = false;
    if (int rc0 = p.zero_words ? launch_zero_words(h) : 0) return rc0;
    h->ss.flags_dirty = true;
    if (h->kind == 1) {
        if (h->Pl > 0)
            k_gp_prep_points<kGPG><<<cdiv((long long)h->Pl * kGPG, kThreads), kThreads, 0, h->stream>>>(h->Pl, h->pt_ptr, h->gobs, f, h->d.clamp_min,
                                                                               h->d.clamp_max, h->W, h->V, h->gp, h->Vinv,
                                                                               h->y, h->VY, h->flags);
        k_gp_prep_cams<<<h->C, kThreads, 0, h->stream>>>(h->C, h->cam_ptr, h->cam_obs, h->gobs, h->U, h->gc, f,
                                                                     h->d.clamp_min, h->d.clamp_max, h->d.rank == 0, h->Up,
                                                                     h->gpc);
    } else if (h->Pl > 0 && !p.prepared && (hmark(h, "point_prep"), true))
        k_point_prep<<<cdiv(h->Pl, kThreads), kThreads, 0, h->stream>>>(h->Pl, h->V, h->gp, f, h->d.clamp_min, h->d.clamp_max,
                                                                       h->Vinv, h->y, h->flags, h->cg.status,
                                                                       h->d.optimize_poses ? h->Rf : nullptr, h->Mp);
    int iters = 0;
    if (p.cg != kCgNone) {
        rec(h, kEvSchur);
        int rc = 0;
        if (h->xstream) {
            // chunked exchange: each row chunk's blocks of S are summed across ranks on the exchange stream while the
            // next chunk's Schur rows are built; b (filled by every row) after the last chunk
            const int K = (int)h->xw.size() - 1;
            for (int c = 0; c < K; ++c) {
                if ((rc = launch_schur(h, p.sf, p.smin, p.smax, p.sdiag, !p.prepared, h->xw[c], h->xw[c + 1]))) return rc;
                const int64_t b0 = h->rptr_host[h->xr[c]], b1 = h->rptr_host[h->xr[c + 1]];
                HIPCHK(hipEventRecord(h->ev_x, h->stream));
                HIPCHK(hipStreamWaitEvent(h->xstream, h->ev_x, 0));
                // set_timing: the exchange's span on its stream, from the first chunk's start to b's end (phase 7)
                if (h->timing && c == 0) HIPCHK(hipEventRecord(h->ev[kEvXchg], h->xstream));
                if (b1 > b0 && (rc = allreduce_async(h, h->S + b0 * D * D, (b1 - b0) * D * D))) return rc;
            }
            if ((rc = allreduce_async(h, h->b, (int64_t)h->C * D))) return rc;
            HIPCHK(hipEventRecord(h->ev_xdone, h->xstream));
            if (h->timing) HIPCHK(hipEventRecord(h->ev[kEvXchgEnd], h->xstream));
            HIPCHK(hipStreamWaitEvent(h->stream, h->ev_xdone, 0));
            rec(h, kEvSchurEnd);
        } else {
            if ((rc = launch_schur(h, p.sf, p.smin, p.smax, p.sdiag, !p.prepared))) return rc;
            hmark(h, "schur");
            rec(h, kEvSchurEnd);
            if ((rc = allreduce(h, h->S, (int64_t)h->nnzb * D * D + (int64_t)h->C * D))) return rc;
        }
        if (h->ss.built_pending) {  // the side stream's E build of the previous solve still reads S~ / Z~
            HIPCHK(hipStreamWaitEvent(h->stream, h->ev_built, 0));
            h->ss.built_pending = false;
        }
        if ((rc = lin_join(h))) return rc;
        rc = with_D(D, [&](auto dc_) -> int {
            constexpr int DV = decltype(dc_)::value;
            launch_factor<DV>(h, f, p.add_U_in_factor, p.basis_by_factor ? cams : nullptr, true);
            if (p.scale) launch_scale<DV>(h);
            return launch_err(h, "k_cg_factor/scale");
        });
        h->ss.sn_valid = p.scale;
        if (rc) return rc;
        hmark(h, "factor/scale");
        if (h->tlon && (rc = run_tl_setup(h, p, cams))) return rc;
        hmark(h, "tl setup");
        int* st = reinterpret_cast<int*>(h->host_res + 8);
        bool dc_by_cgp = p.dc_by_cgp;
        if (p.cg == kCgBlockJacobi) rc = run_bj_cg(h, st);
        else if (p.cg == kCgLaunchPath) rc = run_launch_cg(h, st);
        else rc = run_cgp(h, h->adef2, p.defer_chain, p.cg == kCgPersistentAsync, st);
        if (rc) return rc;
        if (h->ss.cgp_lost) {  // (a single rank's k_tl_cgp timed out: cgp_complete left the persistent CG)
            if ((rc = repeat_cg(h, repeat_recipe(kRepeatLaunchPath, p.basis_by_factor), st))) return rc;
            dc_by_cgp = false;
        }
        if ((iters = cg_tail(h, dc_by_cgp, st)) < 0) return iters;
    }
    if (int rb = solve_tail(h, f, cams, pts_local, p.cg != kCgNone ? h->dc : nullptr)) return rb;
    return iters;
}

}  // namespace
