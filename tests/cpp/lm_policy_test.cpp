// CPU driver of the LM step driver's host policy (instantsfm_amd/csrc/lm_policy.h): reads one query per line from
// stdin, prints one answer per line (doubles as %a, so tests/test_lm_policy.py compares them bitwise).
//   tr damping down quality tr_max tr_min tr_up tr_down tr_factor tr_high tr_low -> damping down
//   gq last loss_new gp_gain gc_gain                                             -> quality
//   verdict not_spd last loss_new rejects max_rejects                            -> fail | reject | accept
//   next status not_spd multi any_rank_abort cgp_lost adef2                      -> the CgpNext name
//   batch last_iters maxit ahead init_back | barriers adef2 iterations           -> integer
//   msg status iteration coarse                                                  -> the text
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../instantsfm_amd/csrc/lm_policy.h"

using namespace insfm;

int main() {
    static const char* const verdicts[] = {"fail", "reject", "accept"};
    static const char* const nexts[] = {"converged", "fail_step", "repeat_collective", "repeat_launch_path",
                                        "repeat_additive", "device_error"};
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, tok;
        in >> cmd;
        std::vector<double> a;
        while (in >> tok) a.push_back(std::strtod(tok.c_str(), nullptr));
        auto i = [&](size_t k) { return (int)a.at(k); };
        if (cmd == "tr" && a.size() == 10) {
            insfm_ba_desc d{};
            d.tr_max = a[3]; d.tr_min = a[4]; d.tr_up = a[5]; d.tr_down = a[6];
            d.tr_factor = a[7]; d.tr_high = a[8]; d.tr_low = a[9];
            const TrUpdate u = tr_update(a[0], a[1], a[2], d);
            std::printf("%a %a\n", u.damping, u.down);
        } else if (cmd == "gq" && a.size() == 4) {
            std::printf("%a\n", gain_quality(a[0], a[1], a[2], a[3]));
        } else if (cmd == "verdict" && a.size() == 5) {
            std::printf("%s\n", verdicts[trial_verdict(i(0) != 0, a[1], a[2], i(3), i(4))]);
        } else if (cmd == "next" && a.size() == 6) {
            std::printf("%s\n", nexts[cgp_next(i(0), i(1) != 0, i(2) != 0, i(3) != 0, i(4) != 0, i(5) != 0)]);
        } else if (cmd == "batch" && a.size() == 4) {
            std::printf("%d\n", cg_first_batch(i(0), i(1), i(2), i(3)));
        } else if (cmd == "barriers" && a.size() == 2) {
            std::printf("%u\n", cgp_barriers(i(0) != 0, i(1)));
        } else if (cmd == "msg" && a.size() == 3) {
            std::printf("%s\n", pcg_status_message(i(0), i(1), i(2)).c_str());
        } else {
            std::fprintf(stderr, "bad query: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
