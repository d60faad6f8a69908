// Host arithmetic shared by the stage passes (tracks.hip, covis.hip, pair_inliers.hip, passes.hip): radix-sort key
// bits, grid sizes and the size of hipcub's temporary storage.  Plain C++ (no HIP types) so it is unit-tested on the
// CPU (tests/test_stage_plan.py builds tests/cpp/stage_plan_test.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

namespace insfm {

// Key bits of a radix sort over keys in [0, n): the smallest b in [1, 62] with 2^b >= n.  One bit too few and the sort
// silently ignores the top bit, i.e. misorders.
inline int bits_for(int64_t n) {
    int b = 1;
    while (b < 62 && ((int64_t)1 << b) < n) ++b;
    return b;
}

// Blocks of `per` items that cover n items; 0 for n = 0 (such a launch is skipped, see stage_device.h launch()).
inline unsigned blocks_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// Running maximum over hipcub's size queries: each query writes into next(), bytes() is the largest answer, the size
// of the one buffer all of a call's sorts and scans then share.
class TempBytes {
public:
    size_t& next() {
        fold();
        return last_;
    }
    size_t bytes() {
        fold();
        return max_;
    }

private:
    void fold() {
        if (last_ > max_) max_ = last_;
        last_ = 0;
    }
    size_t last_ = 0, max_ = 0;
};

}  // namespace insfm
