// CPU driver of the host decisions of one linear solve (instantsfm_amd/csrc/solve_policy.h): reads one query per line
// from stdin, prints one answer per line (doubles as %a, so tests/test_solve_policy.py compares them bitwise).
//   plan kind optimize_poses tlon prog_host cgp u_late rank0 has_points keep_S flags_dirty prep_valid prep_f tl_solves
//        tl_fresh async_status clamp_min clamp_max f
//     -> prepared zero_words sf smin smax sdiag add_U_in_factor scale basis_by_factor cg dc_by_cgp slot use defer_chain
//        must_wait_fact        (cg: none | block_jacobi | launch_path | persistent | persistent_async)
//   flags write_segments test_fault test_breakdown restriction_from_basis -> k_tl_cgp's flag word
//   bits                                                                   -> the four named bits, in that order
//   path xpart nb det adef2                                                -> insfm_ba_cg_info's path code
//   recipe how basis_by_factor  (how: a CgpNext name) -> invalid | the step names in order, then additive / with_cams
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../instantsfm_amd/csrc/solve_policy.h"

using namespace insfm;

int main() {
    static const char* const cgs[] = {"none", "block_jacobi", "launch_path", "persistent", "persistent_async"};
    static const char* const nexts[] = {"converged", "fail_step", "repeat_collective", "repeat_launch_path",
                                        "repeat_additive", "device_error"};
    static const char* const steps[] = {"leave_persistent", "zero_status", "factorize", "ensure_sn", "basis",
                                        "reissue_chain", "run_cg"};
    static const RepeatStep step_bits[] = {kStepLeavePersistent, kStepZeroStatus, kStepFactorize, kStepEnsureSn,
                                           kStepBasis, kStepReissueChain, kStepRunCg};
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, tok;
        in >> cmd;
        std::vector<std::string> t;
        while (in >> tok) t.push_back(tok);
        auto d = [&](size_t k) { return std::strtod(t.at(k).c_str(), nullptr); };
        auto b = [&](size_t k) { return d(k) != 0.0; };
        if (cmd == "plan" && t.size() == 18) {
            SolveFacts s;
            s.kind = (int)d(0); s.optimize_poses = b(1); s.tlon = b(2); s.prog_host = b(3); s.cgp = b(4);
            s.u_late = b(5); s.rank0 = b(6); s.has_points = b(7); s.keep_S = b(8); s.flags_dirty = b(9);
            s.prep_valid = b(10); s.prep_f = d(11); s.tl_solves = (long long)d(12); s.tl_fresh = b(13);
            s.async_status = b(14); s.clamp_min = d(15); s.clamp_max = d(16);
            const SolvePlan p = plan_solve(s, d(17));
            std::printf("%d %d %a %a %a %d %d %d %d %s %d %d %d %d %d\n", p.prepared, p.zero_words, p.sf, p.smin, p.smax,
                        p.sdiag, p.add_U_in_factor, p.scale, p.basis_by_factor, cgs[p.cg], p.dc_by_cgp, p.slot, p.use,
                        p.defer_chain, p.must_wait_fact);
        } else if (cmd == "flags" && t.size() == 4) {
            std::printf("%d\n", cgp_flag_word(b(0), b(1), b(2), b(3)));
        } else if (cmd == "bits" && t.empty()) {
            std::printf("%d %d %d %d\n", kCgpWriteSegments, kCgpTestFault, kCgpTestBreakdown, kCgpRestrictionFromBasis);
        } else if (cmd == "path" && t.size() == 4) {
            std::printf("%d\n", cg_path_code(b(0), (int)d(1), b(2), b(3)));
        } else if (cmd == "recipe" && t.size() == 2) {
            int how = -1;
            for (int k = 0; k < 6; ++k)
                if (t[0] == nexts[k]) how = k;
            if (how < 0) { std::fprintf(stderr, "bad query: %s\n", line.c_str()); return 2; }
            const RepeatRecipe r = repeat_recipe((CgpNext)how, b(1));
            if (!r.valid) { std::printf("invalid\n"); continue; }
            std::string out;
            unsigned left = r.steps;
            for (int k = 0; k < 7; ++k)
                if (r.steps & step_bits[k]) { out += std::string(out.empty() ? "" : " ") + steps[k]; left &= ~step_bits[k]; }
            if (left) out += " unknown_step";
            if (r.additive) out += " | additive";
            if (r.factor_with_cams) out += " | with_cams";
            std::printf("%s\n", out.c_str());
        } else {
            std::fprintf(stderr, "bad query: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
