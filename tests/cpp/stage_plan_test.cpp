// CPU driver of the stage passes' host arithmetic (instantsfm_amd/csrc/stage_plan.h): reads one query per line from
// stdin, prints one answer per line (integers, so tests/test_stage_plan.py compares them exactly).
//   bits n                 -> bits_for(n)
//   blocks n per           -> blocks_for(n, per)
//   temp b0 b1 ...         -> TempBytes::bytes() after one size query per argument
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../instantsfm_amd/csrc/stage_plan.h"

using namespace insfm;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        std::vector<long long> a;
        for (long long v; in >> v;) a.push_back(v);
        if (cmd == "bits" && a.size() == 1) {
            std::printf("%d\n", bits_for((int64_t)a[0]));
        } else if (cmd == "blocks" && a.size() == 2) {
            std::printf("%u\n", blocks_for((int64_t)a[0], (int)a[1]));
        } else if (cmd == "temp") {
            TempBytes need;
            for (long long v : a) need.next() = (size_t)v;  // what a hipcub size query does
            std::printf("%zu\n", need.bytes());
        } else {
            std::fprintf(stderr, "bad query: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
