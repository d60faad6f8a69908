// Host decisions of one linear solve (ba_solve.h run_solve and what it calls, ba_step.h repeat_trial): which kernels a
// solve runs and with which scalars, the lag rule of the coarse inverse, k_tl_cgp's flag word, the CG path code of
// insfm_ba_cg_info, and the steps of a repeated CG.  Plain C++ (no HIP types), unit-tested on the CPU
// (tests/test_solve_policy.py builds tests/cpp/solve_policy_test.cpp).
#pragma once
#include "lm_policy.h"

namespace insfm {

// ---- one solve ------------------------------------------------------------------------------------------------
// What the decisions of a solve read: constants of the handle, the state earlier solves left, the caller's wish.
struct SolveFacts {
    int kind = 0;                 // 0 bundle adjustment, 1 global positioning
    bool optimize_poses = true;   // (false: a points-only solve, no Schur complement)
    bool tlon = false;            // two-level preconditioner
    bool prog_host = false;       // the host-mapped progress word of the polled CG exists
    bool cgp = false;             // the persistent k_tl_cgp is eligible (cgp_nb != 0)
    bool u_late = false;          // k_lin_cams runs beside k_schur; U / g_c join S / b in the factorization
    bool rank0 = true;
    bool has_points = true;       // Pl > 0
    bool keep_S = false;          // debug entry points: every solve forms the scaled copy Sn
    double clamp_min = 0.0, clamp_max = 0.0;  // the descriptor's damping clamps
    bool flags_dirty = false;     // a solve's point preparation ran and no k_final has cleared its flag yet
    bool prep_valid = false;      // the linearization prepared the points for damping factor prep_f
    double prep_f = 0.0;
    long long tl_solves = 0;      // two-level solves since create / reset
    bool tl_fresh = false;        // no solve since the last linearization
    bool async_status = false;    // the caller reads a k_tl_cgp status behind the trial's cost (lm_step)
};

enum CgRun {
    kCgNone,             // a points-only solve
    kCgBlockJacobi,      // launches in chunks, a status copy and a stream sync per chunk (run_bj_cg)
    kCgLaunchPath,       // two launches per iteration from the host poll loop (run_launch_cg)
    kCgPersistent,       // one k_tl_cgp launch, the host waits for its status (run_cgp)
    kCgPersistentAsync   // one k_tl_cgp launch, its status is read behind the trial's cost
};

struct SolvePlan {
    bool prepared = false;    // the linearization's point preparation covers this solve (no k_point_prep, k_schur's
                              // first-trial form)
    bool zero_words = false;  // k_zero_words clears the non-PD flag and the CG status first
    // k_schur's scalars: damping factor, clamps, whether it adds U / g_c to the diagonal blocks / b
    double sf = 1.0, smin = 0.0, smax = 0.0;
    int sdiag = 0;
    bool add_U_in_factor = false;  // k_cg_factor adds U / g_c instead (u_late)
    bool scale = true;             // k_cg_scale forms the scaled copy Sn
    bool basis_by_factor = false;  // the factorization forms the coarse basis in the same launch (k_cg_factor_basis)
    CgRun cg = kCgNone;
    bool dc_by_cgp = false;        // k_tl_cgp writes dc itself (no k_cg_finish)
    // the coarse inverse (two-level solves): the slot this solve's side chain fills, the slot its CG reads (the other
    // one under the lag rule), whether the chain is issued behind the CG from k_tl_cgp's segments, and whether the wait
    // for ev_fact[use] is always queued (else only when the event has not completed yet)
    int slot = 0, use = 0;
    bool defer_chain = false, must_wait_fact = true;
};

inline SolvePlan plan_solve(const SolveFacts& s, double f) {
    SolvePlan p;
    const bool gpk = s.kind == 1;
    p.prepared = s.prep_valid && s.prep_f == f && s.kind == 0;
    // the non-PD flag is cleared by the k_final that consumed it and the CG status word by k_point_prep: one tiny launch
    // clears both only when that chain is broken (a solve not followed by a cost, or no local points)
    p.zero_words = s.flags_dirty || !s.has_points || gpk;
    // global positioning: the scale-eliminated blocks are already damped, so k_schur takes U' / g'_c as they are
    p.sf = gpk ? 1.0 : f;
    p.smin = gpk ? -1.0e308 : s.clamp_min;
    p.smax = gpk ? 1.0e308 : s.clamp_max;
    p.sdiag = gpk ? 1 : (s.u_late ? 0 : (s.rank0 ? 1 : 0));
    p.add_U_in_factor = s.u_late && !gpk;
    // k_tl_cgp holds S unscaled and scales the vectors (ba_cgp.h): a lagged solve on it (whose E build behind the CG
    // takes the coarse segments k_tl_cgp writes) needs no scaled copy Sn; the first solve after a linearization that
    // factorizes its own E (k_tl_erow reads Sn), the launch-path CG and the debug getters do
    p.scale = !(s.tlon && s.cgp && s.tl_solves > 0 && s.tl_fresh && !s.keep_S);
    p.basis_by_factor = s.tlon && s.cgp && !gpk;
    if (!s.optimize_poses) p.cg = kCgNone;
    else if (!(s.tlon && s.prog_host)) p.cg = kCgBlockJacobi;
    else if (!s.cgp) p.cg = kCgLaunchPath;
    else p.cg = s.async_status ? kCgPersistentAsync : kCgPersistent;
    p.dc_by_cgp = p.cg == kCgPersistent || p.cg == kCgPersistentAsync;
    // the oracle's lag rule (ora_pcg): the first solve after a linearization runs on the previous solve's coarse inverse
    p.slot = (int)(s.tl_solves & 1);
    p.use = (s.tl_solves > 0 && s.tl_fresh) ? (p.slot ^ 1) : p.slot;
    // k_tl_cgp under the lag rule: this solve's chain runs after the CG; else it runs now and the CG waits
    p.defer_chain = s.cgp && p.use != p.slot;
    p.must_wait_fact = p.use == p.slot;
    return p;
}

// ---- k_tl_cgp's flag word (its `oseg` argument) ---------------------------------------------------------------------
enum CgpFlag : int {
    kCgpWriteSegments = 1,         // also write this solve's coarse segments tl.Oseg (the chain behind the CG reads them)
    kCgpTestFault = 2,             // INSFM_DIAG=cgp_fault: abort at iteration 2
    kCgpTestBreakdown = 4,         // INSFM_DIAG=adef2_breakdown: report a breakdown at iteration 2
    kCgpRestrictionFromBasis = 8   // the restriction of r0 is k_tl_basis's (not k_cg_factor_basis's cluster runs)
};
inline int cgp_flag_word(bool write_segments, bool test_fault, bool test_breakdown, bool restriction_from_basis) {
    return (write_segments ? kCgpWriteSegments : 0) | (test_fault ? kCgpTestFault : 0) |
           (test_breakdown ? kCgpTestBreakdown : 0) | (restriction_from_basis ? kCgpRestrictionFromBasis : 0);
}

// insfm_ba_cg_info's out[0] (include/insfm_ba.h): 0 launch path / block-Jacobi, 1 persistent, 2 persistent in its
// fixed-order form, 3 row-partitioned, 4 / 5 = 1 / 2 with A-DEF2
inline int cg_path_code(bool xpart, int nb, bool det, bool adef2) {
    if (xpart) return 3;
    if (!nb) return 0;
    return det ? (adef2 ? 5 : 2) : (adef2 ? 4 : 1);
}

// ---- the CG of a trial once more ---------------------------------------------------------------------------------
// The steps of a repeat, in the one order they are ever taken (repeat_cg, ba_solve.h).
enum RepeatStep : unsigned {
    kStepLeavePersistent = 1u << 0,  // the handle drops k_tl_cgp for good: stream sync, barrier counters back to zero
    kStepZeroStatus = 1u << 1,       // the device CG status word
    kStepFactorize = 1u << 2,        // L, L^-1 and r0 = L^-1 b again from the completed S / b
    kStepEnsureSn = 1u << 3,         // the scaled copy Sn if the solve skipped it
    kStepBasis = 1u << 4,            // k_tl_basis: Z~ and the restriction of r0
    kStepReissueChain = 1u << 5,     // the side chain again if it was built from k_tl_cgp's segments
    kStepRunCg = 1u << 6
};
struct RepeatRecipe {
    bool valid = false;             // `how` names a repeat
    unsigned steps = 0;             // RepeatStep bits
    bool additive = false;          // the CG runs on k_tl_cgp with the additive coarse correction (else the launch path)
    bool factor_with_cams = false;  // kStepFactorize forms the basis in the same launch (k_cg_factor_basis)
};

// how: what cgp_next chose.  kRepeatCollective: some rank's k_tl_cgp timed out, every rank leaves it and repeats from
// r0 (a converged rank's launch left its final CG vectors in place of r0).  kRepeatLaunchPath: this single rank's
// launch timed out (cgp_complete already left the persistent CG; the aborted launch left r0 alone).  kRepeatAdditive:
// an A-DEF2 breakdown; r0, the basis and the restriction again, by one launch where the solve formed them so.
inline RepeatRecipe repeat_recipe(CgpNext how, bool basis_by_factor) {
    RepeatRecipe r;
    r.valid = true;
    if (how == kRepeatCollective) {
        r.steps = kStepLeavePersistent | kStepZeroStatus | kStepFactorize | kStepEnsureSn | kStepBasis |
                  kStepReissueChain | kStepRunCg;
    } else if (how == kRepeatLaunchPath) {
        r.steps = kStepZeroStatus | kStepEnsureSn | kStepBasis | kStepReissueChain | kStepRunCg;
    } else if (how == kRepeatAdditive) {
        r.steps = kStepZeroStatus | kStepFactorize | (basis_by_factor ? 0u : (unsigned)kStepBasis) | kStepRunCg;
        r.additive = true;
        r.factor_with_cams = basis_by_factor;
    } else {
        r.valid = false;
    }
    return r;
}

}  // namespace insfm
