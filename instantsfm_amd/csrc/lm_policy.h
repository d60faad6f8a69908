// Host decisions of the LM step driver (ba_step.h lm_step, ba_solve.h): the TrustRegion update, the accept rule, what
// follows a k_tl_cgp launch that did not converge, and the small integer rules of the CG launches.  Plain C++ (no HIP
// types), unit-tested on the CPU (tests/test_lm_policy.py builds tests/cpp/lm_policy_test.cpp).
#pragma once
#include <algorithm>
#include <string>

#include "../../include/insfm_ba.h"

namespace insfm {

// ---- TrustRegion (pypose TrustRegion.update; oracle/ba_oracle.c ora_step) --------------------------------------
struct TrUpdate {
    double damping, down;
};

inline double gain_quality(double last, double loss_new, double gp_gain, double gc_gain) {
    return (last - loss_new) / (gp_gain + gc_gain);
}

// A NaN quality fails both comparisons and shrinks the radius.
inline TrUpdate tr_update(double damping, double down, double quality, const insfm_ba_desc& d) {
    double radius = 1.0 / damping;
    if (quality > d.tr_high) { radius = d.tr_up * radius; down = d.tr_down; }
    else if (quality > d.tr_low) { down = d.tr_down; }
    else { radius = radius * down; down = down * d.tr_factor; }
    radius = std::min(std::max(radius, d.tr_min), d.tr_max);
    return {1.0 / radius, down};
}

// The fate of a costed trial (k_publish restates it on the device): a damped point block that was not SPD fails the
// step; a worse loss is rejected while rejects remain; everything else is accepted.
enum TrialVerdict { kFail, kReject, kAccept };
inline TrialVerdict trial_verdict(bool not_spd, double last, double loss_new, int rejects, int max_rejects) {
    if (not_spd) return kFail;
    return last < loss_new && rejects < max_rejects ? kReject : kAccept;
}

// ---- after a k_tl_cgp launch whose status was read behind the trial's cost -------------------------------------
// status: 1 converged, 2 breakdown, 4 a grid barrier timed out, else unfinished.  multi: a replicated multi-rank CG;
// any_rank_abort: its all-reduced abort flag; cgp_lost: cgp_complete switched this (single-rank) handle to the launch
// path; adef2: the launch applied the coarse correction as A-DEF2.  The order of the tests is the policy.
enum CgpNext { kConverged, kFailStep, kRepeatCollective, kRepeatLaunchPath, kRepeatAdditive, kDeviceError };
inline CgpNext cgp_next(int status, bool not_spd, bool multi, bool any_rank_abort, bool cgp_lost, bool adef2) {
    if (not_spd) return kFailStep;
    if (multi && any_rank_abort) return kRepeatCollective;
    if (status == 4 && cgp_lost) return kRepeatLaunchPath;
    if (status == 2 && adef2) return kRepeatAdditive;
    if (status != 1) return status == 2 ? kFailStep : kDeviceError;
    return kConverged;
}

// The launch-path CG's first batch: a little less than the last solve's count (counts drift by a few iterations per
// LM step; the poll tops up one iteration at a time), at least ahead + 2, at most every launch of the solve.
inline int cg_first_batch(int last_iters, int maxit, int ahead, int init_back) {
    return std::min(std::max(ahead + 2, last_iters - init_back), maxit + 2);
}

// Grid barriers a finished k_tl_cgp launch counted: the setup's two and one per completed iteration; A-DEF2: three
// and two.
inline unsigned cgp_barriers(bool adef2, int iterations) {
    return adef2 ? 2u * (unsigned)iterations + 3u : (unsigned)iterations + 2u;
}

// The error text of a CG that did not converge.  coarse >= 0: the coarse corrections used; kCoarseOff: no two-level
// preconditioner; kCgpLaunch: the status of a k_tl_cgp launch read behind its trial (no coarse field; anything but a
// breakdown is a grid barrier's time-out).
constexpr int kCoarseOff = -1, kCgpLaunch = -2;
inline std::string pcg_status_message(int status, int iteration, int coarse) {
    const char* what = status == 2 ? "breakdown"
                       : coarse == kCgpLaunch ? "timed out (a k_tl_cgp grid barrier)"
                       : status == 4 ? "timed out (a k_tl_cgp grid barrier or a cross-rank exchange of the partitioned CG)"
                                     : "did not finish";
    std::string s = std::string("PCG ") + what + " at iteration " + std::to_string(iteration) + " (status " +
                    std::to_string(status);
    if (coarse != kCgpLaunch) s += ", coarse " + (coarse == kCoarseOff ? std::string("off") : std::to_string(coarse));
    return s + ")";
}

}  // namespace insfm
