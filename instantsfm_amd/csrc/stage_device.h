// Device-side toolkit of the stage passes (tracks.hip, covis.hip, pair_inliers.hip, passes.hip): the owner of one
// call's temporaries, the checked-call form, the launch helper, the run segmentation of a sorted key array and the
// float32 / float64 feature load.  The host arithmetic is in stage_plan.h.
//
// The rule the stage sources follow: before the host reads a device-produced count out of the pinned block it calls
// settle(), which collects the launch errors and synchronises the stream, and every HIP / hipcub call whose result the
// function depends on goes through INSFM_HIP.  A count that a failed sort or copy left behind is therefore never used
// as a grid size or a loop bound.
//
// No floating-point arithmetic in this header: the including files differ in their contraction setting, so a shared
// expression would be compiled two ways.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/insfm_ba.h"
#include "stage_plan.h"

// A failed HIP / hipcub call ends the enclosing function with INSFM_BA_EHIP (StageTemps' destructor cleans up).
#define INSFM_HIP(call)                                      \
    do {                                                     \
        if ((call) != hipSuccess) return INSFM_BA_EHIP;      \
    } while (0)

namespace insfm {
namespace {

constexpr int kT = 256;  // threads per block of every stage kernel

// One call's temporaries: stream-ordered device scratch and eight pinned host words the counts are read back through.
// pinned = false leaves the pinned block out: allocating and freeing it takes about 0.2 ms of host time, which a call
// that reads back a single word (pair_inliers.hip, 0.5 ms in all) does not have; it copies into a local instead, which
// the destructor's synchronise covers just the same.  segment_runs needs the block.
class StageTemps {
public:
    explicit StageTemps(hipStream_t s, bool pinned = true) : s_(s) {
        ok_ = !pinned || hipHostMalloc(reinterpret_cast<void**>(&host_), 8 * sizeof(int64_t)) == hipSuccess;
    }
    StageTemps(const StageTemps&) = delete;
    StageTemps& operator=(const StageTemps&) = delete;
    // The order is what makes an early return safe: the scratch is freed in stream order, the stream is synchronised
    // (nothing still reads the scratch or copies into the pinned words), and only then the pinned block is freed.
    ~StageTemps() {
        for (void* p : ptrs_) (void)hipFreeAsync(p, s_);
        (void)hipStreamSynchronize(s_);
        if (host_) (void)hipHostFree(host_);
    }
    // n items of scratch (at least one byte); nullptr after a failure, which ok() remembers.
    template <typename T>
    T* get(size_t n) {
        void* p = nullptr;
        if (!ok_ || hipMallocAsync(&p, (n ? n : 1) * sizeof(T), s_) != hipSuccess) {
            ok_ = false;
            return nullptr;
        }
        ptrs_.push_back(p);
        return static_cast<T*>(p);
    }
    bool ok() const { return ok_; }  // false: return INSFM_BA_ENOMEM
    hipStream_t stream() const { return s_; }
    int64_t* host() const { return host_; }                                // words 0-3 as int64
    int* hosti() const { return reinterpret_cast<int*>(host_ + 4); }      // words 4-7 as eight ints

private:
    hipStream_t s_;
    std::vector<void*> ptrs_;
    int64_t* host_ = nullptr;
    bool ok_;
};

// The launch errors since the last look, then the stream's completion: after hipSuccess the pinned words hold what the
// queued copies wrote.
inline hipError_t settle(hipStream_t s) {
    const hipError_t launched = hipGetLastError();
    const hipError_t ran = hipStreamSynchronize(s);
    return launched != hipSuccess ? launched : ran;
}

// kernel over n items, kPer per 256-thread block; a launch over zero items is skipped (a zero-block grid is an error).
template <int kPer = kT, typename... P, typename... A>
inline void launch(void (*kernel)(P...), int64_t n, hipStream_t s, A&&... args) {
    if (n > 0) kernel<<<blocks_for(n, kPer), kT, 0, s>>>(std::forward<A>(args)...);
}

template <typename K>
__global__ __launch_bounds__(kT) void k_heads(int64_t n, const K* __restrict__ key, int* __restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    head[i] = (i == 0 || key[i] != key[i - 1]) ? 1 : 0;
}

// start[run] = first element of the run (incl = inclusive scan of the heads); start[runs] = n.
// (maybe_unused: a source that segments nothing includes this header too, and gets no copy of the kernel.)
[[maybe_unused]] __global__ __launch_bounds__(kT) void k_starts(int64_t n, const int* __restrict__ head,
                                                                const int* __restrict__ incl, int* __restrict__ start) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    if (head[i]) start[incl[i] - 1] = (int)i;
    if (i == n - 1) start[incl[i]] = (int)n;
}

// Run segmentation of sorted key[0, n), n >= 1: head[i] = 1 where a run of equal keys starts, incl = inclusive scan of
// head (run of element i, plus one), start[r] = first element of run r with start[runs] = n (n + 1 ints).  Synchronises
// and returns the number of runs in *runs.  tmp / tmp_bytes: hipcub storage that covers an InclusiveSum over n ints.
template <typename K>
int segment_runs(StageTemps& w, void* tmp, size_t tmp_bytes, int n, const K* key, int* head, int* incl, int* start,
                 int* runs) {
    if (n < 1) return INSFM_BA_EINVAL;
    hipStream_t s = w.stream();
    launch(k_heads<K>, n, s, n, key, head);
    INSFM_HIP(hipcub::DeviceScan::InclusiveSum(tmp, tmp_bytes, head, incl, n, s));
    launch(k_starts, n, s, n, head, incl, start);
    INSFM_HIP(hipMemcpyAsync(w.hosti(), incl + n - 1, sizeof(int), hipMemcpyDeviceToHost, s));
    INSFM_HIP(settle(s));
    *runs = w.hosti()[0];
    return INSFM_BA_OK;
}

// Feature i of an [n, 2] float32 or float64 array, widened to double (a conversion, no arithmetic).
__device__ __forceinline__ void load_xy(const void* xy, int f32, int64_t i, double& u, double& v) {
    if (f32) {
        const float2 q = reinterpret_cast<const float2*>(xy)[i];
        u = q.x;
        v = q.y;
    } else {
        const double2 q = reinterpret_cast<const double2*>(xy)[i];
        u = q.x;
        v = q.y;
    }
}

}  // namespace
}  // namespace insfm
