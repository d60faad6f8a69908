// The solver handle and the host helpers every part of the library uses: struct insfm_ba, HIPCHK, the INSFM_DIAG
// switches, the process-wide device-buffer cache behind dalloc / dfree_all / upload, the shared helper streams, and the
// camera-model / D dispatch.  Part of the one translation unit ba_kernels.hip (included after the kernels).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/insfm_ba.h"
#include "ba_common.h"
#include "ba_twolevel.h"
#include "solve_policy.h"

// What one solve leaves for the next (and for the cost, the repeats and the debug entry points behind it).
// insfm_ba_reset puts back tl_solves, tl_fresh and last_cg_iters alone.
struct SolveCarry {
    long long tl_solves = 0;     // two-level solves so far: its parity is the coarse-inverse slot of the next one
    bool tl_fresh = false;       // no solve since the last linearization (the lag rule applies to that solve only)
    bool sn_valid = false;       // Sn holds the scaled S~ of the current solve (k_cg_scale ran for it)
    bool built_pending = false;  // the side stream's E build may still read S~ / Z~ (the next solve waits for ev_built)
    bool lin_pending = false;    // k_lin_cams on `aux` has not been joined yet (lin_join waits for ev_lc)
    bool flags_dirty = false;    // a solve's point preparation ran and no k_final has consumed (cleared) its flag yet
    bool prep_valid = false;     // the last linearization prepared the points (Vinv, y, status) for damping factor prep_f
    double prep_f = 0.0;         // (PointPrep)
    bool chain_oseg = false;     // the side chain of the last solve builds E from k_tl_cgp's segments (reissue_chain)
    bool cgp_pending = false;    // a k_tl_cgp launch whose status the host has not read yet (cgp_complete)
    bool cgp_lost = false;       // the last k_tl_cgp timed out at a grid barrier (another process holds CUs)
    unsigned cgp_epochs = 0;     // grid barriers the counters in cgp_sync have counted (reset with them)
    unsigned cgp_tag = 1;        // tag of the next k_tl_cgp launch's first iteration
    int last_cg_iters = 16;      // the last converged CG's iterations (sizes the next CG's first batch)
};

struct insfm_ba {
    insfm_ba_desc d{};
    int model = 0, ni = 0, D = 0, stride = 0;
    int C = 0, P = 0, N = 0;
    int p0 = 0, p1 = 0, Pl = 0, o0 = 0, Nl = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // structure (device)
    double *uv = nullptr, *pp = nullptr;
    int *cam = nullptr, *ptl = nullptr, *pt_ptr = nullptr, *cam_ptr = nullptr, *cam_obs = nullptr;
    int *row_ptr = nullptr, *col = nullptr, *blk_row = nullptr, *ustart = nullptr;
    int *nbr_ptr = nullptr, *nbr_j = nullptr, *pos_up = nullptr, *pos_lo = nullptr;
    int4* sdesc = nullptr;  // k_schur: per camera-major own observation {o, p, partner begin, partner end}
    int* cm_pt = nullptr;    // k_lin_cams: per camera-major observation, its (local) point
    int* lin_blk = nullptr;  // k_lin_points: track runs of at most kThreads observations (or one longer track)
    int n_lin = 0;
    double* cm_uv = nullptr; // k_lin_cams: per camera-major observation, its uv
    double* Sn = nullptr;  // row-contiguous scaled neighbour blocks for the CG (both triangles, padded rows)
    int64_t n_nbr = 0;
    int nbr_stride = 0;  // > 0: every CG row has exactly nbr_stride neighbour slots (padded), row r starts at r * stride
    int keep_S = 0;      // debug entry points: every solve forms the scaled copy Sn (insfm_ba_debug_get(5) reads S~ from it;
                         // S itself stays unscaled -- k_tl_cgp reads it)
    std::vector<int> pos_up_host;  // [nnzb] Sn slot of each upper block (debug_get(5))
    int4* work = nullptr;
    int nwork = 0, nnzb = 0, max_chunk = 0;
    size_t schur_lds = 0;
    // numeric (device)
    // W: the BA's symmetric records Y_o = W_o L_p (PointPrep; global positioning: its {u, beta^2} records); y: z_p
    // (BA) / y_p (GP); Rf: R_p of the first trial's damped point blocks; Mp: M_p of a retried trial
    double *W = nullptr, *V = nullptr, *gp = nullptr, *Vinv = nullptr, *y = nullptr, *dp = nullptr;
    double *Rf = nullptr, *Mp = nullptr;
    double *xbuf = nullptr;  // [S | b | U | gc | scal]
    double *S = nullptr, *b = nullptr, *U = nullptr, *gc = nullptr, *scal = nullptr;
    int64_t xcount = 0;
    double *Lf = nullptr, *Li = nullptr, *dc = nullptr;
    double* cgmem = nullptr;
    CgBufs cg{};
    int cg_nwg = 0;
    double *cams_cur = nullptr, *cams_new = nullptr, *pts_cur = nullptr, *pts_new = nullptr;
    bool ext_cur = false;  // during insfm_ba_step: cams_cur / pts_cur are the caller's buffers
    bool trial_copied = false;  // the last trial cost's k_publish copied the accepted trial into cams_cur / pts_cur
    double *part_cost = nullptr, *part_gp = nullptr, *part_gc = nullptr;
    int n_cost = 0, n_gp = 0, n_gc = 0;
    int n_gp_grp = 0;  // global positioning: k_gp_backsub blocks (kGPG lanes per track)
    double* result = nullptr;
    int* flags = nullptr;
    double* host_res = nullptr;  // pinned 128 B: result[0..4] (doubles) | cg status (ints, from double slot 8)
    int* prog_host = nullptr;    // pinned, device-mapped: progress of the two-level CG (CgBufs::prog)
    double* pub_host = nullptr;  // pinned, device-mapped: k_publish's result[0..4], decision, sequence word (double 8)
    double* pub_dev = nullptr;
    unsigned pub_seq = 0;
    std::vector<void*> allocs;
    // LM state
    double damping = 0.0, down = 0.0, loss = 0.0;
    bool have_loss = false;
    SolveCarry ss;          // solve-to-solve state
    insfm::SolvePlan last;  // the plan of the last solve (solve_policy.h): the repeats and the debug timers read it
    hipEvent_t ev[18]{};  // 0-9 phase markers, 10-11 debug timing, 12-15 the side chain's start / end by slot,
                          // 16-17 the chunked exchange's span on the exchange stream
    bool chain_timed[2]{};  // set_timing: the side chain of that slot has timing events not yet harvested
    bool timing = false;
    // device time of the current step, accumulated per phase (ms): see insfm_ba_stats.time_ms
    double tms[8]{};
    int cg_launches = 0;
    bool want_timing = false;       // insfm_ba_set_timing: hipEvent phase timing inside insfm_ba_step
    // two-level preconditioner (desc.precond == 1)
    bool tlon = false;
    TlBufs tl{};
    std::vector<int> clab_host;
    size_t pc_lds = 0;
    int pc_rows = 0;  // k_tl_pc rows per restriction pass
    // the register-resident persistent CG (ba_cgp.h k_tl_cgp): blocks per row (0: not eligible), grid, the w exchange
    // [C][8], the coarse vector [kCoarseMax], the grid-barrier words
    int cgp_nb = 0, cgp_grid = 0;
    bool cgp_det = false;                // fixed-order partial sums (deterministic mode, multi-rank replicated CG)
    bool adef2 = false;                  // precond 2: k_tl_cgp applies the coarse correction as A-DEF2 (ba_cgp.h)
    int adef2_fallbacks = 0;             // A-DEF2 solves that broke down and were repeated additively (repeat_trial)
    double* cgp_runs = nullptr;               // [2][grid * 4][12] the cluster runs' partials by parity (cgp_det)
    int* cgp_src = nullptr;     // [n_nbr] S block of each CG slot: e (upper), ~e (lower, transposed), INT_MIN (pad)
    long long* stamps = nullptr;  // INSFM_DIAG=stamps: [kStampSteps][kStKinds][2] kernel entry / exit (wall_clock64)
    long long stamp_step = 0;     // LM steps stamped so far
    int cgp_slots = 0;            // workgroups of k_tl_cgp the device holds at once
    double* cgp_trace = nullptr;  // INSFM_DIAG=cgp_trace: [64][4] of the last solve, printed to stderr
    // row-partitioned multi-rank CG (ba_xpart.h; insfm_ba_cg_window / insfm_ba_cg_attach)
    bool xpart = false;
    double* xwin = nullptr;            // own window (uncached): 2 x [vc C*D | gd 3C | rowR C*MC + 2], xg C*D, flags
    size_t xwin_bytes = 0;
    long long xoff_region[2]{}, xoff_xg = 0, xoff_flags = 0;  // in doubles from the window base
    std::vector<void*> xopened;        // IPC-opened peer windows (closed at destroy)
    double** xbases = nullptr;         // device [world] window bases (own included)
    unsigned** xpflags = nullptr;      // device [world] flag blocks
    unsigned* xcnt = nullptr;          // device exchange counters [2]
    std::vector<int> xq;               // [world + 1] cluster-ordered row ranges of the ranks
    double* cgp_wx = nullptr;           // [2][C][8]
    unsigned long long* cgp_yg = nullptr;  // [kCoarseMax][2] tagged granules of y
    unsigned* cgp_sync = nullptr;
    // the coarse factorization of solve n runs on `side` while the CG of solve n uses slot (n-1)&1
    double *Ebuf[2]{}, *Einvbuf[2]{};
    double* gjW = nullptr;  // Gauss-Jordan ping-pong buffer [ldE][ldE]
    double* gjP = nullptr;  // Gauss-Jordan pivot-block inverses [2][64][64]
    int* okbuf = nullptr;  // [2]
    hipStream_t side = nullptr;
    hipEvent_t ev_E = nullptr, ev_built = nullptr, ev_fact[2]{};
    // chunked [S | b] exchange (desc.allreduce_async): work-item / row boundaries of the chunks, the exchange stream
    std::vector<int> xw, xr, rptr_host;
    hipStream_t xstream = nullptr;
    // u_late: k_lin_cams runs on `aux` beside k_lin_points / k_schur; k_schur builds S / b without U / g_c and
    // k_cg_factor adds them after waiting for ev_lc (lin_join).  Single-rank W-path only.
    bool u_late = false;
    hipStream_t aux = nullptr;
    hipEvent_t ev_lin0 = nullptr, ev_lc = nullptr;
    hipEvent_t ev_x = nullptr, ev_xdone = nullptr;
    hipEvent_t ev_pre = nullptr;  // multi-rank: recorded in front of the CG (its stall deadline starts after it)
    int coarse_used = 0;
    // global positioning (kind 1, insfm_gp_*): per local observation ray / scale-free flag / source index, camera
    // factors, the linearization records and the scale-eliminated camera blocks of the current trial
    int kind = 0;
    double *trans = nullptr, *fcam = nullptr, *gobs = nullptr, *Up = nullptr, *gpc = nullptr, *VY = nullptr;
    int *sfree = nullptr, *osrc = nullptr;
    double *scl_cur = nullptr, *scl_new = nullptr, *ds = nullptr;
    std::vector<int> osrc_host;
    std::vector<std::pair<const char*, double>> hmarks;  // INSFM_HOST_TRACE=2
};

namespace {

#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            h->err = std::string(#expr) + " failed: " + hipGetErrorString(e_);                    \
            return INSFM_BA_EHIP;                                                                 \
        }                                                                                         \
    } while (0)

// INSFM_DIAG: comma-separated diagnostics, read once per process (none is on by default):
//   poison        every buffer dalloc hands out is first filled with 0xff bytes (NaN doubles, -1 ints), so a read of
//                 something never written shows up instead of a fresh allocation's zero pages
//   pattern_host  create builds the block pattern by the host pass (the multi-rank path) on a single rank too
//   trace         per solve, host microseconds spent enqueueing CG iterations (stderr)
//   trace2        per LM step, host timestamps of the step's API calls (stderr)
//   create        host milliseconds of create's phases (stderr)
//   no_cgp        the two-level CG runs as two launches per iteration (k_tl_pc_cl + k_tl_pspmv) even where the
//                 persistent register-resident k_tl_cgp is eligible (A/B and parity of the two paths)
//   cgp_trace     k_tl_cgp records gamma, delta, rho and its stop flag per iteration; printed after each solve
//   cgp128        k_tl_cgp with 128 register blocks per row even for shorter rows (tests the wide variant)
//   own_streams   per-handle side / linearization streams instead of the process-wide ones (A/B)
//   chain_hold    timing only: the lagged coarse-inverse chain is never issued (later solves keep an older E^-1)
//   side_hi / side_normal   the coarse-inverse side stream at the high / normal stream priority (default: lowest)
bool diag(const char* name) {
    static const std::string v = [] { const char* e = std::getenv("INSFM_DIAG"); return std::string(e ? e : ""); }();
    const size_t n = std::strlen(name);
    for (size_t a = 0; a <= v.size();) {
        size_t b = v.find(',', a);
        if (b == std::string::npos) b = v.size();
        if (b - a == n && v.compare(a, n, name) == 0) return true;
        a = b + 1;
    }
    return false;
}

// Process-wide cache of the device buffers of destroyed handles.  TorchBA creates a handle per Solve (the mapper
// solves 4-5 times per reconstruction), and freeing config 3's ~1 GB of buffers took ~7 ms per destroy (hipFree
// synchronizes the device) plus the allocations of the next create.  insfm_ba_destroy waits for the handle's streams
// and parks its buffers here, keyed by their HIP device; dalloc takes the smallest parked buffer of the current device
// of at least the requested size and at most twice it.  Bounded by INSFM_DEVICE_CACHE_MB (default 4096; 0 disables
// it): beyond that, buffers are freed.  The parked memory is invisible to PyTorch's caching allocator, so
// insfm_ba_release_cache() frees it all (TorchBA calls it when torch reports an out-of-memory error, the mapper at the
// end of a reconstruction); a failing hipMalloc inside dalloc releases it too.
struct DeviceCache {
    struct Buf {
        size_t bytes;
        int dev;
        bool uc;  // uncached device memory (hipDeviceMallocUncached)
    };
    std::mutex m;
    std::map<std::pair<int, size_t>, std::vector<void*>> free;  // (2 * device + uncached, size) -> pointers
    size_t bytes = 0;
    std::unordered_map<void*, Buf> info;  // every pointer dalloc handed out (cached or fresh)
};
DeviceCache& device_cache() {
    static DeviceCache* c = new DeviceCache();  // (never destroyed: buffers may be parked until process exit)
    return *c;
}
size_t device_cache_cap() {
    static const size_t v = [] {
        const char* e = std::getenv("INSFM_DEVICE_CACHE_MB");
        return (size_t)(e ? std::max(0LL, std::atoll(e)) : 4096LL) << 20;
    }();
    return v;
}

// frees every parked buffer (any device); returns the bytes released
size_t release_cache() {
    DeviceCache& c = device_cache();
    std::vector<std::pair<void*, int>> drop;
    size_t n = 0;
    {
        std::lock_guard<std::mutex> lk(c.m);
        for (auto& kv : c.free)
            for (void* q : kv.second) {
                drop.emplace_back(q, kv.first.first / 2);
                c.info.erase(q);
            }
        c.free.clear();
        n = c.bytes;
        c.bytes = 0;
    }
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (auto& d : drop) {
        if (d.second != cur) (void)hipSetDevice(d.second);
        (void)hipFree(d.first);
        if (d.second != cur) (void)hipSetDevice(cur);
    }
    (void)hipGetLastError();
    return n;
}

// Process-wide helper streams, one per (HIP device, role): the side stream of the coarse-inverse chain (role 0, low
// priority) and the camera-linearization stream (role 1).  Every handle of a device shares them, so the number of
// hardware queues a process uses does not grow with the handles alive at once.  With per-handle streams, a TorchBA.Solve
// run while another config-3 handle was alive (bench.py's solve_end_to_end beside its main engine) took 1.9-2.0 ms per
// LM step instead of 1.17: its side chain landed on a queue that the dispatcher served behind k_schur, k_gj_step ran
// 2-4x longer, and the main stream waited ~330 us per step for the lagged coarse inverse (profiles/r5_v1/).  Handles
// on one device are driven one at a time (the reference builds a TorchBA per Solve, global_mapper.py:115), and all
// cross-stream ordering is by the handle's own events, so sharing only serializes what would compete anyway.
// INSFM_DIAG=own_streams restores per-handle streams (A/B).
std::mutex& stream_pool_mutex() {
    static std::mutex* m = new std::mutex();
    return *m;
}
std::map<std::pair<int, int>, hipStream_t>& stream_pool() {
    static auto* p = new std::map<std::pair<int, int>, hipStream_t>();  // (never destroyed, like the device cache)
    return *p;
}
hipError_t helper_stream(int role, int prio, hipStream_t* out) {
    if (diag("own_streams")) return hipStreamCreateWithPriority(out, hipStreamNonBlocking, prio);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    std::lock_guard<std::mutex> lk(stream_pool_mutex());
    auto& pool = stream_pool();
    auto it = pool.find(std::make_pair(dev, role));
    if (it != pool.end()) {
        *out = it->second;
        return hipSuccess;
    }
    const hipError_t e = hipStreamCreateWithPriority(out, hipStreamNonBlocking, prio);
    if (e == hipSuccess) pool[std::make_pair(dev, role)] = *out;
    return e;
}
void release_helper_stream(hipStream_t s) {
    if (!s) return;
    {
        std::lock_guard<std::mutex> lk(stream_pool_mutex());
        for (auto& kv : stream_pool())
            if (kv.second == s) return;  // pooled: stays for the next handle
    }
    (void)hipStreamDestroy(s);
}

// uc: uncached device memory (the CG's cross-workgroup hand-off buffers: their loads, stores and atomics skip the L2s,
// config 3: 10.4-11.0 -> 9.3-9.7 us per k_tl_cgp iteration; profiles/r4_v7/)
int dalloc(insfm_ba* h, void** p, size_t bytes, bool uc = false) {
    if (bytes == 0) bytes = 16;
    bytes = (bytes + 255) & ~(size_t)255;
    DeviceCache& c = device_cache();
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    const int key = 2 * dev + (uc ? 1 : 0);
    bool hit = false;
    {
        std::lock_guard<std::mutex> lk(c.m);
        auto it = c.free.lower_bound(std::make_pair(key, bytes));
        if (it != c.free.end() && it->first.first == key && it->first.second <= 2 * bytes && !it->second.empty()) {
            *p = it->second.back();
            it->second.pop_back();
            c.bytes -= it->first.second;
            if (it->second.empty()) c.free.erase(it);
            hit = true;
        }
    }
    if (hit) {
        h->allocs.push_back(*p);
        if (diag("poison")) (void)hipMemset(*p, 0xff, bytes);
        return 0;
    }
    auto alloc = [&] { return uc ? hipExtMallocWithFlags(p, bytes, hipDeviceMallocUncached) : hipMalloc(p, bytes); };
    hipError_t e = alloc();
    if (e == hipErrorOutOfMemory) {  // give the parked buffers back and try once more
        (void)hipGetLastError();
        release_cache();
        e = alloc();
    }
    if (e != hipSuccess) {
        h->err = std::string("hipMalloc(") + std::to_string(bytes) + ") failed: " + hipGetErrorString(e);
        return INSFM_BA_ENOMEM;
    }
    {
        std::lock_guard<std::mutex> lk(c.m);
        c.info[*p] = DeviceCache::Buf{bytes, dev, uc};
    }
    h->allocs.push_back(*p);
    if (diag("poison")) (void)hipMemset(*p, 0xff, bytes);
    return 0;
}

// the handle's buffers back to the cache (the caller has synchronized every stream that used them)
void dfree_all(insfm_ba* h) {
    DeviceCache& c = device_cache();
    const size_t cap = device_cache_cap();
    std::vector<void*> drop;
    {
        std::lock_guard<std::mutex> lk(c.m);
        for (void* q : h->allocs) {
            auto it = c.info.find(q);
            if (it == c.info.end()) { drop.push_back(q); continue; }
            const DeviceCache::Buf b = it->second;
            if (c.bytes + b.bytes > cap) {
                c.info.erase(it);
                drop.push_back(q);
            } else {
                c.free[std::make_pair(2 * b.dev + (b.uc ? 1 : 0), b.bytes)].push_back(q);
                c.bytes += b.bytes;
            }
        }
    }
    for (void* q : drop) (void)hipFree(q);  // (hipFree takes a pointer of any device)
    h->allocs.clear();
}

template <typename T>
int upload(insfm_ba* h, T** dst, const T* src, size_t n) {
    int rc = dalloc(h, (void**)dst, n * sizeof(T));
    if (rc) return rc;
    if (n) HIPCHK(hipMemcpyAsync(*dst, src, n * sizeof(T), hipMemcpyHostToDevice, h->stream));
    return 0;
}

int model_ni(int m) {
    switch (m) {
        case 0: return 1; case 1: return 2; case 2: return 2; case 3: return 3; case 4: return 6;
        case 5: return 6; case 6: return 10; case 8: return 2; case 9: return 3;
        default: return -1;
    }
}

// ---- model / D dispatch ----------------------------------------------------------------------------------------
template <typename F>
int with_model(int m, F&& f) {
    switch (m) {
        case 0: return f(std::integral_constant<int, 0>{});
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 5: return f(std::integral_constant<int, 5>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 8: return f(std::integral_constant<int, 8>{});
        case 9: return f(std::integral_constant<int, 9>{});
        default: return INSFM_BA_EINVAL;
    }
}
// the camera-block sizes of the bundle adjustment's models; with_D: those and global positioning's 3
template <typename F>
int with_ba_D(int D, F&& f) {
    switch (D) {
        case 7: return f(std::integral_constant<int, 7>{});
        case 8: return f(std::integral_constant<int, 8>{});
        case 9: return f(std::integral_constant<int, 9>{});
        case 12: return f(std::integral_constant<int, 12>{});
        case 16: return f(std::integral_constant<int, 16>{});
        default: return INSFM_BA_EINVAL;
    }
}
template <typename F>
int with_D(int D, F&& f) {
    if (D == 3) return f(std::integral_constant<int, 3>{});
    return with_ba_D(D, std::forward<F>(f));
}

int launch_err(insfm_ba* h, const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        h->err = std::string(what) + ": " + hipGetErrorString(e);
        return INSFM_BA_EHIP;
    }
    return 0;
}

}  // namespace
