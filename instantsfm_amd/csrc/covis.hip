// Co-visibility pair counts (include/insfm_covis.h): the visibility graph of PruneWeaklyConnectedImages on the GPU.
//
// Integer gather / sort work, no FLOPs and no atomics, so the result is bit-identical from run to run:
//   1. k_track_pairs + exclusive scan (int64) -- ordinals per track (L(L-1)/2 for L > 2) and each track's first ordinal;
//   2. k_expand     -- one thread per (track, i) row writes the keys (lo << 32) | hi of its j-loop at
//                      off[t] + i*L - i(i+1)/2 + (j-i-1) (integer only; no inversion of the triangular index), the
//                      all-ones sentinel for a pair of equal images, and the ordinal itself as the value;
//   3. radix sort (stable) of (key, ordinal) -- every run of equal keys starts with its smallest ordinal;
//   4. k_heads + scan + k_starts (stage_device.h segment_runs) -- run starts; k_keep + scan + k_emit -- the runs of
//      length >= min_count, the sentinel run dropped, compacted in key order.
// Image ids are only ever compared and packed, never used as an index, so no bound on them is needed.
// Scratch and the pinned words the counts come back through belong to one StageTemps (stage_device.h), released
// before the call returns (also an early one): 32 bytes per ordinal (two key and two value buffers, run starts, output
// positions; head flags and their scan reuse the unsorted key buffer, the keep flags the unsorted values), 16 bytes per
// track, and hipcub's temporary storage.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdint>

#include "../../include/insfm_ba.h"
#include "../../include/insfm_covis.h"
#include "../../include/insfm_tracks.h"
#include "stage_device.h"

namespace {

using namespace insfm;

constexpr int64_t kMaxItems = (int64_t)1 << 31;  // hipcub item counts are int
constexpr unsigned long long kSame = ~0ull;      // key of a pair whose two rows name one image

// A track longer than 65536 rows alone has 2^31 ordinals or more: its count saturates at 2^31 (the call is then
// refused) so that the int64 sum over fewer than 2^31 tracks cannot overflow.
__global__ __launch_bounds__(kT) void k_track_pairs(int64_t nt, const int64_t* __restrict__ ptr, int64_t* __restrict__ cnt,
                                                    int* __restrict__ bad) {
    const int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (t >= nt) return;
    const int64_t L = ptr[t + 1] - ptr[t];
    if (L < 0 || ptr[t] < 0) *bad = 1;
    cnt[t] = L <= 2 ? 0 : (L > 65536 ? kMaxItems : L * (L - 1) / 2);
}

__global__ __launch_bounds__(kT) void k_expand(int64_t nt, int64_t n_rows, const int64_t* __restrict__ ptr,
                                               const int64_t* __restrict__ off, const int32_t* __restrict__ obs_img,
                                               int64_t total, unsigned long long* __restrict__ key, int* __restrict__ val) {
    const int64_t r = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (r >= n_rows) return;
    const int64_t x = ptr[0] + r;
    // the track of row x: the last t with ptr[t] <= x (empty tracks share their start with the next one)
    int64_t lo = 0, hi = nt;  // ptr[lo] <= x < ptr[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (ptr[mid] <= x) lo = mid; else hi = mid;
    }
    const int64_t p = ptr[lo], L = ptr[lo + 1] - p;
    if (L <= 2) return;
    const int64_t i = x - p;
    const int64_t base = off[lo] + i * L - i * (i + 1) / 2;
    if (base + (L - i - 1) > total) return;  // (cannot happen for a monotone track_ptr; keeps every store in range)
    const int a = obs_img[x];
    for (int64_t j = i + 1; j < L; ++j) {
        const int b = obs_img[p + j];
        const int64_t o = base + (j - i - 1);
        const unsigned mn = (unsigned)(a < b ? a : b), mx = (unsigned)(a < b ? b : a);
        key[o] = a == b ? kSame : ((unsigned long long)mn << 32) | mx;
        val[o] = (int)o;
    }
}

__global__ __launch_bounds__(kT) void k_keep(int nr, const int* __restrict__ start, const unsigned long long* __restrict__ skey,
                                             int min_count, int* __restrict__ keep) {
    const int r = blockIdx.x * kT + threadIdx.x;
    if (r >= nr) return;
    const int s = start[r];
    keep[r] = (skey[s] != kSame && start[r + 1] - s >= min_count) ? 1 : 0;
}

__global__ __launch_bounds__(kT) void k_emit(int nr, const int* __restrict__ start, const int* __restrict__ keep,
                                             const int* __restrict__ pos, const unsigned long long* __restrict__ skey,
                                             const int* __restrict__ sval, int32_t* __restrict__ pair_lo,
                                             int32_t* __restrict__ pair_hi, int32_t* __restrict__ pair_count,
                                             int64_t* __restrict__ pair_first) {
    const int r = blockIdx.x * kT + threadIdx.x;
    if (r >= nr || !keep[r]) return;
    const int s = start[r], q = pos[r];
    const unsigned long long k = skey[s];
    pair_lo[q] = (int32_t)(unsigned)(k >> 32);
    pair_hi[q] = (int32_t)(unsigned)(k & 0xffffffffull);
    pair_count[q] = start[r + 1] - s;
    pair_first[q] = sval[s];
}

}  // namespace

extern "C" int insfm_covis_pairs(int64_t n_tracks, const int64_t* track_ptr, const int32_t* obs_img, int32_t min_count,
                                 int64_t capacity, int32_t* pair_lo, int32_t* pair_hi, int32_t* pair_count,
                                 int64_t* pair_first, int64_t* counts, void* stream) {
    if (!counts) return INSFM_BA_EINVAL;
    counts[0] = counts[1] = 0;
    if (n_tracks < 0 || n_tracks >= kMaxItems - 1 || capacity < 0 || min_count < 1) return INSFM_BA_EINVAL;
    if (n_tracks == 0) return INSFM_BA_OK;
    if (!track_ptr || !obs_img) return INSFM_BA_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int64_t nt = n_tracks;
    StageTemps w(s);
    int64_t* cnt = w.get<int64_t>(nt);
    int64_t* off = w.get<int64_t>(nt);
    int* bad = w.get<int>(1);
    if (!w.ok()) return INSFM_BA_ENOMEM;
    int64_t* host = w.host();
    int* hosti = w.hosti();

    size_t b = 0;
    INSFM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, b, cnt, off, (int)nt, s));
    void* tmp0 = w.get<unsigned char>(b);
    if (!w.ok()) return INSFM_BA_ENOMEM;
    INSFM_HIP(hipMemsetAsync(bad, 0, sizeof(int), s));
    launch(k_track_pairs, nt, s, nt, track_ptr, cnt, bad);
    INSFM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp0, b, cnt, off, (int)nt, s));
    INSFM_HIP(hipMemcpyAsync(host, off + nt - 1, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    INSFM_HIP(hipMemcpyAsync(host + 1, cnt + nt - 1, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    INSFM_HIP(hipMemcpyAsync(host + 2, track_ptr, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    INSFM_HIP(hipMemcpyAsync(host + 3, track_ptr + nt, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    INSFM_HIP(hipMemcpyAsync(hosti, bad, sizeof(int), hipMemcpyDeviceToHost, s));
    INSFM_HIP(settle(s));
    if (hosti[0]) return INSFM_BA_EINVAL;
    const int64_t total = host[0] + host[1], n_rows = host[3] - host[2];
    counts[1] = total;
    if (total >= kMaxItems) return INSFM_BA_EINVAL;
    if (total == 0) return INSFM_BA_OK;
    if (!pair_lo || !pair_hi || !pair_count || !pair_first) return INSFM_BA_EINVAL;

    unsigned long long* key = w.get<unsigned long long>(total);
    unsigned long long* skey = w.get<unsigned long long>(total);
    int* val = w.get<int>(total);
    int* sval = w.get<int>(total);
    int* start = w.get<int>(total + 1);
    int* pos = w.get<int>(total);
    int* head = reinterpret_cast<int*>(key);  // the unsorted keys are dead after the sort: 2 ints per key
    int* incl = head + total;
    int* keep = val;                          // and so are the unsorted values
    TempBytes need;
    INSFM_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, need.next(), key, skey, val, sval, (int)total, 0, 64, s));
    INSFM_HIP(hipcub::DeviceScan::InclusiveSum(nullptr, need.next(), head, incl, (int)total, s));
    INSFM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, need.next(), keep, pos, (int)total, s));
    const size_t tmp_bytes = need.bytes();
    void* tmp = w.get<unsigned char>(tmp_bytes);
    if (!w.ok()) return INSFM_BA_ENOMEM;

    launch(k_expand, n_rows, s, nt, n_rows, track_ptr, off, obs_img, total, key, val);
    INSFM_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, b = tmp_bytes, key, skey, val, sval, (int)total, 0, 64, s));
    int nr = 0;
    if (int rc = segment_runs(w, tmp, tmp_bytes, (int)total, skey, head, incl, start, &nr)) return rc;

    launch(k_keep, nr, s, nr, start, skey, min_count, keep);
    INSFM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, b = tmp_bytes, keep, pos, nr, s));
    INSFM_HIP(hipMemcpyAsync(hosti, pos + nr - 1, sizeof(int), hipMemcpyDeviceToHost, s));
    INSFM_HIP(hipMemcpyAsync(hosti + 1, keep + nr - 1, sizeof(int), hipMemcpyDeviceToHost, s));
    INSFM_HIP(settle(s));
    const int64_t n_out = (int64_t)hosti[0] + hosti[1];
    if (n_out > capacity) return INSFM_BA_EINVAL;  // before anything is written
    launch(k_emit, nr, s, nr, start, keep, pos, skey, sval, pair_lo, pair_hi, pair_count, pair_first);
    INSFM_HIP(settle(s));
    counts[0] = n_out;
    return INSFM_BA_OK;
}
