// The LM step driver, host side: the trial cost and its published result, the repeats of a trial whose k_tl_cgp launch
// did not converge, and lm_step.  The decisions live in lm_policy.h, solve_policy.h and cg_poll.h (CPU-tested); this
// file issues the stream work.  Part of the translation unit ba_kernels.hip (after ba_solve.h, before ba_create.h).
#pragma once
#include "ba_solve.h"

namespace {

// A step that ended in an error with a k_tl_cgp status unread: wait for the launch and restart the barrier counters
// (the next launch's epochs would otherwise not match what this one counted).
void cgp_drop_pending(insfm_ba* h) {
    if (!h->ss.cgp_pending) return;
    h->ss.cgp_pending = false;
    (void)hipStreamSynchronize(h->stream);
    (void)cgp_reset_barriers(h);
}

// lm_step's accept rule for the trial being costed (k_publish copies an accepted trial into the caller's buffers)
struct TrialAccept {
    double last;     // the loss before the step
    int can_reject;  // rejects < max_rejects
};

// The cost result to the host: k_publish into host-mapped memory and a spin on its sequence word; without the mapped
// block, a copy and a stream synchronization.
// Sets h->trial_copied when k_publish also copied an accepted trial (h->pub_host[5] holds its decision).
int finish_cost(insfm_ba* h, const TrialAccept* ta) {
    h->trial_copied = false;
    if (!h->pub_host) {
        HIPCHK(hipMemcpyAsync(h->host_res, h->result, sizeof(double) * 6, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        return 0;
    }
    const unsigned seq = h->pub_seq = next_pub_seq(h->pub_seq);
    const bool copy = ta != nullptr && h->ext_cur && h->kind == 0;
    const long long ncam = copy ? (long long)h->C * h->stride : 0, npts = copy ? (long long)h->Pl * 3 : 0;
    const int grid = copy ? std::max(1, std::min(1024, cdiv(std::max(ncam, npts / 2 + 1), kThreads))) : 1;
    k_publish<<<grid, kThreads, 0, h->stream>>>(h->result, h->ss.cgp_pending ? h->cg.status : nullptr, h->pub_dev, seq,
                                               ta ? ta->last : 0.0, ta ? ta->can_reject : 0,
                                               h->cams_new, copy ? h->cams_cur : nullptr, ncam, h->pts_new, h->pts_cur, npts,
                                               stamp_ptr(h, kStPublish));
    if (int rc = launch_err(h, "k_publish")) return rc;
    hmark(h, "publish");
    const unsigned* w = reinterpret_cast<const unsigned*>(h->pub_host + 8);
    // bounded like the CG poll: a device that neither publishes nor reports an error ends the step with EHIP
    const double stall_s = 6.0 * cg_stall_limit();
    PublishWait pw;
    hipError_t q = hipSuccess;
    const int pr = publish_wait(
        pw, seq, stall_s, [&] { return __atomic_load_n(w, __ATOMIC_ACQUIRE); },
        [&] { return (q = hipStreamQuery(h->stream)) == hipSuccess ? 0 : q == hipErrorNotReady ? 1 : -1; },
        wall_seconds, [] { cpu_relax(); });
    if (pr != PublishWait::kPublished) {
        h->err = pr == PublishWait::kStreamError ? std::string("cost: ") + hipGetErrorString(q)
                 : pr == PublishWait::kDrainedUnpublished
                     ? std::string("cost: the stream drained without publishing the result")
                     : "cost: no result from the device for " + std::to_string(stall_s) +
                           " s (INSFM_CG_STALL_S scales the limit)";
        return INSFM_BA_EHIP;
    }
    hmark(h, "published");
    const volatile double* pv = h->pub_host;
    for (int k = 0; k < 5; ++k) h->host_res[k] = pv[k];
    h->host_res[5] = pv[6];  // k_tl_cgp aborts (summed over the ranks)
    h->trial_copied = copy;
    return 0;
}

// cost at (cams, pts_local) -> h->result[0..1]; with gain partials when `gains` (after a solve).
int run_cost(insfm_ba* h, const double* cams, const double* pts_local, bool gains, const double* scl = nullptr,
             const TrialAccept* ta = nullptr) {
    const bool gpk = h->kind == 1;  // (global positioning publishes without an accept rule)
    if (gpk) {
        if (h->Nl > 0)
            k_gp_cost<<<h->n_cost, kThreads, 0, h->stream>>>(h->Nl, h->cam, h->ptl, h->trans, h->fcam, cams, pts_local, scl,
                                                             h->d.huber_delta, h->part_cost);
        k_final<<<1, kFinalThreads, 0, h->stream>>>(h->part_cost, h->Nl > 0 ? h->n_cost : 0, gains && h->Pl > 0 ? h->part_gp : nullptr,
                                               h->n_gp, nullptr, 0, h->flags, h->result, nullptr);
    }
    int rc = gpk ? launch_err(h, "k_gp_cost/k_final") : with_model(h->model, [&](auto mc) -> int {
        constexpr int M = decltype(mc)::value;
        if (h->Nl > 0)
            k_cost<M><<<h->n_cost, kCostThreads, 0, h->stream>>>(h->Nl, h->cam, h->ptl, h->uv, h->pp, cams, pts_local,
                                                             h->d.huber_delta, h->part_cost,
                                                             gains ? stamp_ptr(h, kStCost) : nullptr);
        k_final<<<1, kFinalThreads, 0, h->stream>>>(h->part_cost, h->Nl > 0 ? h->n_cost : 0, gains && h->Pl > 0 ? h->part_gp : nullptr,
                                               h->n_gp, gains ? h->part_gc : nullptr, h->n_gc, h->flags, h->result,
                                               h->ss.cgp_pending ? h->cg.status : nullptr,
                                               gains ? stamp_ptr(h, kStFinal) : nullptr);
        return launch_err(h, "k_cost/k_final");
    });
    if (rc) return rc;
    h->ss.flags_dirty = false;
    rc = allreduce(h, h->result, 6);
    if (rc) return rc;
    return finish_cost(h, gpk ? nullptr : ta);
}

// A trial whose k_tl_cgp launch (status cst, read behind the trial's cost) did not converge, once more: the CG again
// by the recipe of `how` (solve_policy.h repeat_recipe, ba_solve.h repeat_cg), then cg_tail, the back-substitution and
// the cost (k_publish accepted the first nowhere: its CG did not converge).  Returns the PCG iterations,
// INSFM_BA_ESOLVER (from cg_tail alone) or an error.
int repeat_trial(insfm_ba* h, double f, const TrialAccept& ta, CgpNext how, const int* cst) {
    if (how == kRepeatCollective) {
        // a replicated multi-rank CG: some rank's k_tl_cgp timed out at a grid barrier (the all-reduced flag, the same
        // on every rank).  Every rank leaves the persistent CG for good and repeats the solve on the launch path from
        // r0 -- the same fixed-order arithmetic everywhere, so the ranks' dc stay bitwise equal.
        std::fprintf(stderr, "[insfm] rank %d: a k_tl_cgp grid barrier timed out on %s rank; every rank continues on the "
                             "launch-per-iteration CG\n", h->d.rank, cst[0] == 4 ? "this" : "another");
    } else if (how == kRepeatAdditive) {
        // An A-DEF2 solve that broke down (k_tl_cgp status 2): under the lag rule E^-1 is the previous solve's, Z~^T r
        // is not exactly zero and the single-reduction recurrence can break down.  The solve is
        // repeated with the additive coarse correction (precond 1, symmetric for any SPD E^-1) in one k_tl_cgp launch.
        // Every rank of a replicated multi-rank CG sees the same status (fixed-order arithmetic), so every rank does.
        std::fprintf(stderr, "[insfm] A-DEF2 PCG breakdown at iteration %d: the trial's solve is repeated with the additive "
                             "coarse correction\n", cst[1]);
        ++h->adef2_fallbacks;
    }  // (kRepeatLaunchPath, a single rank's time-out: cgp_complete reported it and left the persistent CG)
    const RepeatRecipe recipe = repeat_recipe(how, h->last.basis_by_factor);
    int* st = reinterpret_cast<int*>(h->host_res + 8);
    int rc;
    if ((rc = repeat_cg(h, recipe, st))) return rc;
    const int it = cg_tail(h, recipe.additive, st);
    if (it < 0) return it;
    if ((rc = solve_tail(h, f, h->cams_cur, h->pts_cur, h->dc))) return rc;
    if ((rc = run_cost(h, h->cams_new, h->pts_new, true, h->scl_new, &ta))) return rc;
    return it;
}

// set_timing: the phases of the trial that just ended (after its cost; the linearization with the step's first trial).
void end_trial_timing(insfm_ba* h, bool first) {
    rec(h, kEvTrialEnd);
    if (!h->timing) return;
    (void)hipEventSynchronize(h->ev[kEvTrialEnd]);
    if (first) acc_time(h, kEvLinearize, kEvTrial, kPhLinearize);
    if (h->d.optimize_poses) {
        acc_time(h, kEvSchur, kEvSchurEnd, kPhSchur);
        acc_time(h, kEvTrial, kEvBacksub, kPhSolve);
        if (h->xstream) acc_time(h, kEvXchg, kEvXchgEnd, kPhExchange);
    }
    acc_time(h, kEvBacksub, kEvCost, kPhBacksub);
    acc_time(h, kEvCost, kEvTrialEnd, kPhCost);
    rec(h, kEvTrial);  // the next trial starts here
}

// The accepted trial becomes the current parameters.
int adopt_trial(insfm_ba* h) {
    if (h->trial_copied) {  // k_publish already copied the accepted trial into the caller's buffers
        if (h->pub_host[5] != 1.0) {
            h->err = "accept decision of k_publish differs from the host's";
            return INSFM_BA_EHIP;
        }
    } else if (h->ext_cur) {  // the current parameters live in the caller's buffers: copy the accepted trial there
        HIPCHK(hipMemcpyAsync(h->cams_cur, h->cams_new, sizeof(double) * (size_t)h->C * h->stride,
                              hipMemcpyDeviceToDevice, h->stream));
        if (h->Pl)
            HIPCHK(hipMemcpyAsync(h->pts_cur, h->pts_new, sizeof(double) * (size_t)h->Pl * 3, hipMemcpyDeviceToDevice,
                                  h->stream));
    } else {
        std::swap(h->cams_cur, h->cams_new);
        std::swap(h->pts_cur, h->pts_new);
    }
    std::swap(h->scl_cur, h->scl_new);
    return 0;
}

// One LM step on the parameters loaded into cams_cur / pts_cur (/ scl_cur): bae.optim.LM.step semantics (SURVEY.md
// 3.3): cumulative damping, TrustRegion radius update, up to max_rejects rejected trials.
int lm_step(insfm_ba* h, insfm_ba_stats* st) {
    h->timing = st != nullptr && h->want_timing;
    for (auto& v : h->tms) v = 0.0;
    h->cg_launches = 0;
    int rc;
    if (!h->have_loss) {
        if ((rc = run_cost(h, h->cams_cur, h->pts_cur, false, h->scl_cur))) return rc;
        h->loss = h->host_res[0];
        h->have_loss = true;
    }
    const double last = h->loss;
    h->hmarks.clear();
    hmark(h, "step");
    if (h->stamps)  // (this step's slot of the ring: a kernel not launched in the step reads 0, not a stamp of 1024 ago)
        HIPCHK(hipMemsetAsync(stamp_ptr(h, 0), 0, sizeof(long long) * kStKinds * 2, h->stream));
    rec(h, kEvLinearize);
    if ((rc = run_linearize(h, h->cams_cur, h->pts_cur))) return rc;
    hmark(h, "linearize enqueued");
    if (h->timing && (rc = lin_join(h))) return rc;  // (the phase split times both linearization kernels)
    rec(h, kEvTrial);
    double f = 1.0;
    int rejects = 0, trials = 0, pcg_total = 0, pcg_last = 0, failed = 0;
    cgp_drop_pending(h);
    for (;;) {
        f *= (1.0 + h->damping);
        ++trials;
        int it = run_solve(h, f, h->cams_cur, h->pts_cur, true);  // (a k_tl_cgp status is read after the cost, below)
        if (it == INSFM_BA_ESOLVER) { failed = 1; h->loss = last; break; }
        if (it < 0) return it;
        rec(h, kEvCost);
        const TrialAccept ta{last, rejects < h->d.max_rejects ? 1 : 0};
        if ((rc = run_cost(h, h->cams_new, h->pts_new, true, h->scl_new, &ta))) return rc;  // waits for the result
        if (h->ss.cgp_pending) {  // the k_tl_cgp launch finished before the k_publish the host just saw
            h->ss.cgp_pending = false;
            int cst[3];
            if ((rc = cgp_complete(h, h->adef2, cst))) return rc;
            if (h->timing) acc_time(h, kEvCg, kEvCgEnd, kPhCgLaunches);
            const bool not_spd = h->host_res[4] != 0.0;  // a damped point block was not SPD
            const CgpNext next = cgp_next(cst[0], not_spd, h->d.world_size > 1 || h->d.allreduce, h->host_res[5] != 0.0,
                                          h->ss.cgp_lost, h->adef2);
            if (next == kConverged) {
                it = cst[1];
                h->coarse_used = cst[2];
                h->ss.last_cg_iters = it;
            } else if (next == kFailStep || next == kDeviceError) {
                if (!not_spd) h->err = pcg_status_message(cst[0], cst[1], kCgpLaunch);
                if (next == kDeviceError) return INSFM_BA_EHIP;
                it = INSFM_BA_ESOLVER;
            } else {
                it = repeat_trial(h, f, ta, next, cst);
            }
            if (it == INSFM_BA_ESOLVER) { failed = 1; h->loss = last; break; }
            if (it < 0) return it;
        }
        end_trial_timing(h, trials == 1);
        const double loss_new = h->host_res[0];
        const TrialVerdict verdict = trial_verdict(h->host_res[4] != 0.0, last, loss_new, rejects, h->d.max_rejects);
        if (h->trial_copied && verdict != kAccept && h->pub_host[5] != 0.0) {
            h->err = "k_publish accepted a trial the host rejects";  // (cannot happen: the same rule on the same doubles)
            return INSFM_BA_EHIP;
        }
        if (verdict == kFail) { failed = 1; h->loss = last; break; }
        pcg_last = it;
        pcg_total += it;
        const TrUpdate tr =
            tr_update(h->damping, h->down, gain_quality(last, loss_new, h->host_res[2], h->host_res[3]), h->d);
        h->damping = tr.damping;
        h->down = tr.down;
        if (verdict == kReject) {
            ++rejects;
            h->loss = last;
            continue;
        }
        if ((rc = adopt_trial(h))) return rc;
        h->loss = loss_new;
        break;
    }
    if (h->timing) harvest_chain_time(h);
    if (st) {
        st->loss = h->loss;
        st->loss_before = last;
        st->damping = h->damping;
        st->trials = trials;
        st->rejects = rejects;
        st->pcg_iters_last = pcg_last;
        st->pcg_iters_total = pcg_total;
        st->solver_failed = failed;
        for (int k = 0; k < 8; ++k) st->time_ms[k] = h->tms[k];
        st->cg_launches = h->cg_launches;
        st->coarse_used = h->coarse_used;
    }
    h->timing = false;
    if (h->stamps) ++h->stamp_step;
    print_hmarks(h);
    return 0;
}

}  // namespace
