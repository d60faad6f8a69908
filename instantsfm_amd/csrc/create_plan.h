// Host planning of insfm_ba_create (plain C++17, no HIP): every index array the kernels assume, as stage functions
// that take their inputs and return a result struct.  ba_create.h runs the stages in order and uploads the results;
// tests/cpp/create_plan_test.cpp runs them without a GPU.  Constants that live in device headers (LDS budgets, launch
// sizes, kCoarseMax, ...) come in as arguments.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "create_host.h"

namespace insfm {

// the host form of the device's int4 records (work items, segments, sort entries); uploaded as int4
struct Int4 {
    int x, y, z, w;
};
static_assert(sizeof(Int4) == 16, "Int4 is uploaded as int4");

// ---- input checks --------------------------------------------------------------------------------------------
// First failing index wins (the lowest slice with a failure holds it): 0 = fine, 1 = cam_idx out of range,
// 2 = pt_idx out of range, 3 = observations not track-major.
inline int plan_check_inputs(HostPool& pool, int C, int P, int N, const int32_t* cam_idx, const int32_t* pt_idx) {
    std::vector<int> bad(pool.size(), 0);
    pool.ranges(N, [&](int t, long long a, long long b) {
        for (long long i = a; i < b; ++i) {
            if (cam_idx[i] < 0 || cam_idx[i] >= C) { bad[t] = 1; return; }
            if (pt_idx[i] < 0 || pt_idx[i] >= P) { bad[t] = 2; return; }
            if (i && pt_idx[i] < pt_idx[i - 1]) { bad[t] = 3; return; }
        }
    });
    for (int e : bad)
        if (e) return e;
    return 0;
}

// ---- track order ---------------------------------------------------------------------------------------------
// Global track pointers gptr and the shard's [p0, p1) local arrays (observations [o0, o0 + Nl)).  Each track's
// observations are reordered by camera (stable insertion sort: tracks are short) so that the upper-triangle partners
// of an observation are the contiguous tail [lust[o], track end) of its track; key = that tail's length (the
// observation's upper-partner count).  lsrc: the global observation of each local one, lptl: its local track.
struct TrackOrder {
    std::vector<int> gptr, lptr;
    nivec<int> lptl, lcam, lsrc, lust, key;
    int o0 = 0, Nl = 0;
};
inline TrackOrder plan_track_order(HostPool& pool, int P, int N, int p0, int p1, const int32_t* cam_idx,
                                   const int32_t* pt_idx) {
    TrackOrder t;
    // (pt_idx is nondecreasing: one binary search per track)
    t.gptr.assign(P + 1, 0);
    pool.ranges(P + 1, [&](int, long long a, long long b) {
        for (long long p = a; p < b; ++p) t.gptr[p] = (int)(std::lower_bound(pt_idx, pt_idx + N, (int32_t)p) - pt_idx);
    });
    t.o0 = t.gptr[p0];
    t.Nl = t.gptr[p1] - t.o0;
    const int o0 = t.o0, Nl = t.Nl, Pl = p1 - p0;
    t.lptr.resize(Pl + 1);
    t.lptl.resize(Nl); t.lcam.resize(Nl); t.lsrc.resize(Nl); t.lust.resize(Nl); t.key.resize(Nl);
    for (int p = 0; p <= Pl; ++p) t.lptr[p] = t.gptr[p0 + p] - o0;
    pool.ranges(Pl, [&](int, long long pa, long long pb) {
        for (long long p = pa; p < pb; ++p) {
            const int b0 = t.lptr[p], b1 = t.lptr[p + 1];
            for (int o = b0; o < b1; ++o) {
                const int x = o0 + o, cx = cam_idx[x];
                int u = o;
                while (u > b0 && cam_idx[t.lsrc[u - 1]] > cx) { t.lsrc[u] = t.lsrc[u - 1]; --u; }
                t.lsrc[u] = x;
            }
            int u = b0;
            for (int o = b0; o < b1; ++o) {
                t.lcam[o] = cam_idx[t.lsrc[o]];
                t.lptl[o] = (int)p;
                if (o > b0 && t.lcam[o] != t.lcam[o - 1]) u = o;
                t.lust[o] = u;
                t.key[o] = b1 - u;
            }
        }
    });
    return t;
}

// ---- camera-major lists --------------------------------------------------------------------------------------
// Within a camera the observations in point order, cut into chunks of `chunk` entries (kSchurChunk k_schur rounds:
// 4 x 64 own observations for D = 8), each chunk sorted by descending upper-partner count (stable; balances the
// Schur groups of a wave: 2.8 % more wave partner slots than a global count sort, 10.8 % with one-round chunks).
// Every k_schur row then walks the points in the same global order at about the same pace, so rows running together
// read a shared track's partner W records close together in time.  Config 3, k_schur: 491 us (count sort over the
// whole camera) -> 467 us (chunks of 4 rounds; 1 / 2 / 8 / 16 rounds: 541 / 499 / 471 / 483 us -- the wave partner
// slots cost more than the locality buys below 4).  Measured and dropped in round 3: the
// chunk's slices dealt to the waves in snake order (480-484 vs 473-475 us) and runs of consecutive rows per XCD (L2
// hit 4 -> 54 %, yet 469-515 us).
struct CamMajor {
    std::vector<int> cptr;
    nivec<int> cobs;
};
inline CamMajor plan_cam_major(HostPool& pool, int C, const TrackOrder& t, int chunk) {
    CamMajor m;
    // observations are track-major (point order), so a stable counting sort by camera leaves each list in point
    // order; then a stable sort of each chunk by descending partner count
    pcount_sort(pool, t.Nl, C, nullptr, [&](int o) { return t.lcam[o]; }, m.cobs, m.cptr);
    pool.ranges(C, [&](int, long long i0, long long i1) {
        for (long long i = i0; i < i1; ++i)
            for (int a = m.cptr[i]; a < m.cptr[i + 1]; a += chunk) {
                const int e = std::min(a + chunk, m.cptr[i + 1]);
                std::stable_sort(m.cobs.data() + a, m.cobs.data() + e, [&](int x, int y) { return t.key[x] > t.key[y]; });
            }
    });
    return m;
}

// ---- block pattern and co-visibility graph -------------------------------------------------------------------
// The upper block pattern of S (row i: i, then the cameras j > i sharing a track; rptr / cols) and the co-visibility
// graph g (per camera every other camera sharing a track, ascending, weighted by the number of (obs of i, obs of j)
// pairs sharing one: the two-level clustering's weights).  gcptr: the global camera-major pointers.  upw (device
// form only): the pair count of every upper block, indexed like cols.
struct CovisGraph {
    std::vector<int> ptr, nb;
    std::vector<long long> w;
};
struct BlockPattern {
    std::vector<int> gcptr, rptr, cols, upw;
    CovisGraph g;
};

// host form: one pass over the global camera-major list
inline BlockPattern plan_pattern_host(HostPool& pool, int C, int N, const int32_t* cam_idx, const int32_t* pt_idx,
                                      const std::vector<int>& gptr) {
    BlockPattern b;
    CovisGraph& g = b.g;
    b.rptr.assign(C + 1, 0);
    nivec<int> gcpt;  // the point of every observation, camera-major (global)
    pcount_sort(pool, N, C, nullptr, [&](int i) { return cam_idx[i]; }, gcpt, b.gcptr, [&](int i) { return pt_idx[i]; });
    const int T = pool.size();
    std::vector<std::vector<int>> pnb(T);
    std::vector<std::vector<long long>> pw(T);
    std::vector<int> nlen(C, 0), ulen(C, 0);
    pool.ranges(C, [&](int t, long long i0, long long i1) {
        std::vector<int> mark(C, -1), buf;
        std::vector<long long> acc(C, 0);
        for (int i = (int)i0; i < (int)i1; ++i) {
            buf.clear();
            for (int e = b.gcptr[i]; e < b.gcptr[i + 1]; ++e) {
                const int p = gcpt[e];
                for (int q = gptr[p]; q < gptr[p + 1]; ++q) {
                    const int j = cam_idx[q];
                    if (j == i) continue;  // (the observation itself and same-camera duplicates)
                    if (mark[j] != i) { mark[j] = i; acc[j] = 0; buf.push_back(j); }
                    acc[j] += 1;
                }
            }
            std::sort(buf.begin(), buf.end());
            int up = 0;
            for (int j : buf) { pnb[t].push_back(j); pw[t].push_back(acc[j]); up += j > i; }
            nlen[i] = (int)buf.size();
            ulen[i] = up;
        }
    });
    g.ptr.assign(C + 1, 0);
    for (int i = 0; i < C; ++i) {
        g.ptr[i + 1] = g.ptr[i] + nlen[i];
        b.rptr[i + 1] = b.rptr[i] + 1 + ulen[i];
    }
    g.nb.reserve(g.ptr[C]);
    g.w.reserve(g.ptr[C]);
    for (int t = 0; t < T; ++t) {
        g.nb.insert(g.nb.end(), pnb[t].begin(), pnb[t].end());
        g.w.insert(g.w.end(), pw[t].begin(), pw[t].end());
    }
    b.cols.resize(b.rptr[C]);
    pool.ranges(C, [&](int, long long i0, long long i1) {
        for (int i = (int)i0; i < (int)i1; ++i) {
            int k = b.rptr[i];
            b.cols[k++] = i;
            for (int e = g.ptr[i]; e < g.ptr[i + 1]; ++e)
                if (g.nb[e] > i) b.cols[k++] = g.nb[e];
        }
    });
    return b;
}

// device form, first half: the upper lists k_pattern wrote (row i: ulen[i] neighbours unb / pair counts uwt from
// offset uoff[i]) give rptr, cols and upw; plan_graph_from_upper finishes g once the lower transpose exists
inline BlockPattern plan_pattern_from_upper(int C, const std::vector<int>& ulen, const std::vector<int>& uoff,
                                            const std::vector<int>& unb, const std::vector<int>& uwt) {
    BlockPattern b;
    b.rptr.assign(C + 1, 0);
    for (int i = 0; i < C; ++i) b.rptr[i + 1] = b.rptr[i] + 1 + ulen[i];
    b.cols.resize(b.rptr[C]);
    b.upw.assign(b.rptr[C], 0);
    for (int i = 0; i < C; ++i) {
        b.cols[b.rptr[i]] = i;
        for (int k = 0; k < ulen[i]; ++k) {
            b.cols[b.rptr[i] + 1 + k] = unb[uoff[i] + k];
            b.upw[b.rptr[i] + 1 + k] = uwt[uoff[i] + k];
        }
    }
    return b;
}

// ---- lower transpose -----------------------------------------------------------------------------------------
// brow: the row of every block; per camera c (lop) the upper blocks in column c: their rows locol (ascending) and
// block indices loblk
struct LowerLists {
    std::vector<int> brow, lop, locol, loblk;
};
inline LowerLists plan_lower(int C, const std::vector<int>& rptr, const std::vector<int>& cols) {
    LowerLists l;
    l.brow.resize(rptr[C]);
    for (int i = 0; i < C; ++i)
        for (int e = rptr[i]; e < rptr[i + 1]; ++e) l.brow[e] = i;
    l.lop.assign(C + 1, 0);
    for (int i = 0; i < C; ++i)
        for (int e = rptr[i] + 1; e < rptr[i + 1]; ++e) l.lop[cols[e] + 1]++;
    for (int c = 0; c < C; ++c) l.lop[c + 1] += l.lop[c];
    l.locol.resize(std::max(1, l.lop[C]));
    l.loblk.resize(std::max(1, l.lop[C]));
    std::vector<int> fill(l.lop.begin(), l.lop.end() - 1);
    for (int i = 0; i < C; ++i)
        for (int e = rptr[i] + 1; e < rptr[i + 1]; ++e) {
            const int k = fill[cols[e]]++;
            l.locol[k] = i;
            l.loblk[k] = e;
        }
    return l;
}

// device form, second half: the graph, per row the lower neighbours (transposed, ascending), then the upper ones
inline void plan_graph_from_upper(int C, const LowerLists& l, BlockPattern& b) {
    CovisGraph& g = b.g;
    const std::vector<int>&rptr = b.rptr, &cols = b.cols, &upw = b.upw;
    g.ptr.assign(C + 1, 0);
    for (int i = 0; i < C; ++i) g.ptr[i + 1] = g.ptr[i] + (l.lop[i + 1] - l.lop[i]) + (rptr[i + 1] - rptr[i] - 1);
    g.nb.resize(g.ptr[C]);
    g.w.resize(g.ptr[C]);
    for (int i = 0; i < C; ++i) {
        int k = g.ptr[i];
        for (int q = l.lop[i]; q < l.lop[i + 1]; ++q, ++k) { g.nb[k] = l.locol[q]; g.w[k] = upw[l.loblk[q]]; }
        for (int e2 = rptr[i] + 1; e2 < rptr[i + 1]; ++e2, ++k) { g.nb[k] = cols[e2]; g.w[k] = upw[e2]; }
    }
}

// ---- camera clusters of the two-level preconditioner (same rules as oracle/ba_oracle.c: ora_aggregate) ----------
// Co-visibility weight w(i,j) = number of (obs of i, obs of j) pairs sharing a track.  Greedy aggregation from seeds
// in increasing id, growing by the most-connected unassigned camera (ties: smallest id) up to K members; aggregates
// smaller than K/2 are dissolved into the most-connected aggregate of size >= K/2 (ties: smallest aggregate id);
// labels renumbered by first appearance.
inline int aggregate(const CovisGraph& g, int C, int K, std::vector<int>& lab) {
    lab.assign(C, -1);
    std::vector<long long> score(C, 0);
    std::vector<char> incand(C, 0);
    std::vector<int> cand, asize;
    int nagg = 0;
    for (int seed = 0; seed < C; ++seed) {
        if (lab[seed] >= 0) continue;
        cand.clear();
        int size = 0, cur = seed;
        for (;;) {
            lab[cur] = nagg;
            ++size;
            for (int e = g.ptr[cur]; e < g.ptr[cur + 1]; ++e) {
                const int j = g.nb[e];
                if (lab[j] >= 0) continue;
                if (!incand[j]) { incand[j] = 1; score[j] = 0; cand.push_back(j); }
                score[j] += g.w[e];
            }
            if (size >= K) break;
            int best = -1;
            long long bs = 0;
            for (int j : cand) {
                if (lab[j] >= 0) continue;
                if (score[j] > bs || (score[j] == bs && bs > 0 && j < best)) { bs = score[j]; best = j; }
            }
            if (best < 0) break;
            cur = best;
        }
        for (int j : cand) incand[j] = 0;
        asize.push_back(size);
        ++nagg;
    }
    const int minsz = K / 2 > 1 ? K / 2 : 1;
    std::vector<long long> to(nagg, 0);
    std::vector<int> nl(lab);
    for (int i = 0; i < C; ++i) {
        if (asize[lab[i]] >= minsz) continue;
        for (int e = g.ptr[i]; e < g.ptr[i + 1]; ++e) {
            const int a = lab[g.nb[e]];
            if (asize[a] >= minsz) to[a] += g.w[e];
        }
        int best = -1;
        long long bs = 0;
        for (int e = g.ptr[i]; e < g.ptr[i + 1]; ++e) {
            const int a = lab[g.nb[e]];
            if (asize[a] >= minsz && to[a] > 0 && (to[a] > bs || (to[a] == bs && a < best))) { bs = to[a]; best = a; }
        }
        for (int e = g.ptr[i]; e < g.ptr[i + 1]; ++e) to[lab[g.nb[e]]] = 0;
        if (best >= 0) nl[i] = best;
    }
    std::vector<int> ren(nagg, -1);
    int nc = 0;
    for (int i = 0; i < C; ++i) {
        if (ren[nl[i]] < 0) ren[nl[i]] = nc++;
        lab[i] = ren[nl[i]];
    }
    return nc;
}

// Cluster choice.  Target cluster size 14 by default (config 3, same box, 3 x 3 runs: K = 16 / 14 / 12 -> 703-711 /
// 716-720 / 713-720 LM it/s, CG iterations per 10 steps 225 / 213 / 208; profiles/r3_v10/cluster_size_probe_*.log).
// While the coarse dimension exceeds coarse_max (kCoarseMax) the target grows in proportion to the excess (at least
// by one), rounded up to even (aggregates below K / 2 are dissolved: an odd K would keep singletons):
// K' = max(K + 1, ceil(K nc MC / coarse_max)) rounded up to even, at most C -- the oracle's ora_cluster_cameras.
// With K = C the clusters are the co-visibility components: if even those do not fit (more components than
// coarse_max / MC), coarse_ok stays false and the solver runs the block-Jacobi PCG (precond 0) instead.
struct Clusters {
    int nc = 0;
    bool coarse_ok = false;
    std::vector<int> lab;
};
inline Clusters plan_clusters(const CovisGraph& g, int C, int cluster_size, int MC, int coarse_max) {
    Clusters c;
    int K = std::min(cluster_size > 0 ? cluster_size : 24, C);
    c.nc = aggregate(g, C, K, c.lab);
    while (c.nc * MC > coarse_max && K < C) {
        K = (int)std::min<long long>(C, std::max<long long>(K + 1, ((long long)K * c.nc * MC + coarse_max - 1) / coarse_max));
        K += K & 1;
        K = std::min(K, C);
        c.nc = aggregate(g, C, K, c.lab);
    }
    c.coarse_ok = c.nc * MC <= coarse_max;
    return c;
}

// ---- CG neighbour lists --------------------------------------------------------------------------------------
// Flattened CG neighbour list per row (nptr / nj): upper blocks then lower (transposed) ones -- with the two-level
// preconditioner (coarse_ok) each row's list is sorted by (cluster of the neighbour, neighbour), so that a row's
// neighbour-cluster segments are contiguous runs of its blocks (the register-resident CG kernel k_tl_cgp walks them
// in block order); pup / plo give each upper block's two slots in the row-contiguous copy Sn.
// Equal-length rows (every row padded to the longest with zero blocks of neighbour = the row itself; nbr_stride > 0)
// when that costs at most 10 % more slots: the CG's product kernel then derives a row's range from its index instead
// of loading nbr_ptr first (one dependent memory round trip less per iteration).  The padded blocks stay zero (Sn is
// cleared at create and k_cg_scale never writes them), so every consumer of the lists may walk them unchanged.
struct NbrLists {
    std::vector<int> nptr, nj, pup, plo;
    int nbr_stride = 0;
    int64_t n_nbr = 0;  // slots (nj holds one entry more when there are none)
};
inline NbrLists plan_nbr_lists(int C, const std::vector<int>& rptr, const std::vector<int>& cols, const LowerLists& l,
                               bool coarse_ok, const std::vector<int>& lab) {
    NbrLists n;
    const int nnzb = rptr[C];
    std::vector<int>&nptr = n.nptr, &nj = n.nj, &pup = n.pup, &plo = n.plo;
    nptr.assign(C + 1, 0);
    pup.assign(std::max(1, nnzb), -1);
    plo.assign(std::max(1, nnzb), -1);
    nj.reserve(2 * (size_t)nnzb);
    {
        // per row entries (neighbour j, block e, 0 = upper slot / 1 = lower slot), in cluster order when the coarse
        // space exists (stable: within a cluster the upper-then-lower order)
        std::vector<Int4> ent;
        for (int i = 0; i < C; ++i) {
            ent.clear();
            for (int e = rptr[i] + 1; e < rptr[i + 1]; ++e) ent.push_back(Int4{cols[e], e, 0, 0});
            for (int k = l.lop[i]; k < l.lop[i + 1]; ++k) ent.push_back(Int4{l.locol[k], l.loblk[k], 1, 0});
            if (coarse_ok)
                std::stable_sort(ent.begin(), ent.end(), [&](const Int4& x, const Int4& y) { return lab[x.x] < lab[y.x]; });
            for (const Int4& q : ent) {
                (q.z ? plo : pup)[q.y] = (int)nj.size();
                nj.push_back(q.x);
            }
            nptr[i + 1] = (int)nj.size();
        }
    }
    int stride = 0;
    for (int i = 0; i < C; ++i) stride = std::max(stride, nptr[i + 1] - nptr[i]);
    const int64_t nn = (int64_t)nj.size();
    if (stride > 0 && nn > 0 && (int64_t)C * stride * 10 <= nn * 11) {
        // the pad slots of a row (neighbour = the row itself) go behind the row's own-cluster entries when the
        // list is in cluster order, so that it stays in cluster order; else at the end
        std::vector<int> nj2((size_t)C * stride), nptr2(C + 1), ins(C);
        for (int i = 0; i < C; ++i) {
            const int len = nptr[i + 1] - nptr[i], pad = stride - len;
            int at = len;
            if (coarse_ok) {
                at = 0;
                while (at < len && lab[nj[nptr[i] + at]] <= lab[i]) ++at;
            }
            ins[i] = at;
            nptr2[i] = i * stride;
            int* dst = nj2.data() + (size_t)i * stride;
            for (int q = 0; q < len; ++q) dst[q < at ? q : q + pad] = nj[nptr[i] + q];
            for (int q = 0; q < pad; ++q) dst[at + q] = i;
        }
        nptr2[C] = C * stride;
        // remap the Sn slots of every upper block (row i = brow[e] for pos_up, row cols[e] for pos_lo)
        auto slot = [&](int r, int p) {
            const int q = p - nptr[r];
            return r * stride + (q < ins[r] ? q : q + stride - (nptr[r + 1] - nptr[r]));
        };
        for (int e = 0; e < nnzb; ++e) {
            if (e == rptr[l.brow[e]]) continue;  // diagonal block: no slot
            const int i = l.brow[e], j = cols[e];
            pup[e] = slot(i, pup[e]);
            plo[e] = slot(j, plo[e]);
        }
        nj.swap(nj2);
        nptr.swap(nptr2);
        n.nbr_stride = stride;
    }
    n.n_nbr = (int64_t)nj.size();
    for (int i = 0; i < C; ++i) { pup[rptr[i]] = 0; plo[rptr[i]] = 0; }  // diagonal blocks: unused slots
    if (nj.empty()) nj.push_back(0);
    return n;
}

// ---- Schur work items ----------------------------------------------------------------------------------------
// Long rows are split so that a chunk fits the LDS target.  Deterministic mode's k_schur runs kDetWaves waves per
// workgroup taking their LDS adds in turn (round 6; one wave in round 5): its workgroups stage kDetWaves waves' W^
// and take row chunks of <= kLdsTargetDet, so that three share a CU.  (With the 96-KB chunks of the 8-wave form one
// wave held a whole CU: k_schur 2.1 ms per trial on config 3 in deterministic mode.)
// Work order: natural (row order), so the 256 rows running at once are 256 consecutive cameras that share tracks in
// the Infinity Cache.
struct SchurLimits {
    size_t lds_budget, lds_target;  // kLdsBudget; kLdsTarget (deterministic mode: kLdsTargetDet)
    int waves;                      // kSchurWaves (deterministic mode: kDetWaves)
    int ws, bs;                     // schur_ws(D), schur_bs(D)
};
struct SchurWork {
    bool fits = false;  // false: too many cameras for the LDS budget (nothing else is set)
    int cap = 0;        // blocks per chunk
    std::vector<Int4> work;  // {row, block begin, block end, 0}
    int max_chunk = 1;
    size_t schur_lds = 0;
};
inline SchurWork plan_schur_work(int C, int D, const SchurLimits& lim, const std::vector<int>& gcptr,
                                 const std::vector<int>& rptr) {
    SchurWork s;
    const size_t wsh_lds = sizeof(double) * lim.waves * (64 / D) * lim.ws;  // W^ staging
    const size_t fixed_lds = sizeof(double) * (D + 12) + sizeof(int) * (size_t)C + wsh_lds + 64;
    if (fixed_lds + sizeof(double) * D * D > lim.lds_budget) return s;
    s.fits = true;
    // chunk target: lds_target when at least 8 blocks fit under it, else the hard budget
    const size_t tgt = lim.lds_target >= fixed_lds + 8 * sizeof(double) * lim.bs ? lim.lds_target : lim.lds_budget;
    s.cap = (int)((tgt - fixed_lds) / (sizeof(double) * lim.bs));
    for (int i = 0; i < C; ++i) {
        if (gcptr[i + 1] == gcptr[i] && rptr[i + 1] - rptr[i] == 1) {
            s.work.push_back(Int4{i, rptr[i], rptr[i + 1], 0});
            continue;
        }
        for (int kb = rptr[i]; kb < rptr[i + 1]; kb += s.cap) {
            const int ke = std::min(kb + s.cap, rptr[i + 1]);
            s.work.push_back(Int4{i, kb, ke, 0});
            s.max_chunk = std::max(s.max_chunk, ke - kb);
        }
    }
    s.schur_lds = sizeof(double) * ((size_t)s.max_chunk * lim.bs + D + 12) + wsh_lds + sizeof(int) * (size_t)C;
    s.schur_lds = (s.schur_lds + 15) & ~(size_t)15;
    return s;
}

// ---- exchange chunk boundaries -------------------------------------------------------------------------------
// Chunk boundaries at rows splitting the blocks into about equal counts (geometric series of chunk sizes were
// measured in round 3 and do not pay: the all-reduces run back to back on one stream), and the
// first work item of each boundary row.
struct ExchangeChunks {
    std::vector<int> xr, xw;
};
inline ExchangeChunks plan_exchange(int C, int chunks, const std::vector<int>& rptr, const std::vector<Int4>& work) {
    ExchangeChunks x;
    const int K = std::min(chunks, C);
    x.xr.assign(1, 0);
    x.xw.assign(1, 0);
    for (int c = 1; c < K; ++c) {
        const int64_t target = (int64_t)rptr[C] * c / K;
        const int r = (int)(std::upper_bound(rptr.begin(), rptr.end(), (int)target) - rptr.begin()) - 1;
        if (r <= x.xr.back() || r >= C) continue;
        int w = x.xw.back();
        while (w < (int)work.size() && work[w].x < r) ++w;
        x.xr.push_back(r);
        x.xw.push_back(w);
    }
    x.xr.push_back(C);
    x.xw.push_back((int)work.size());
    return x;
}

// ---- linearize runs ------------------------------------------------------------------------------------------
// k_lin_points: track runs of at most lin_threads (kLinThreads) tracks and observations (or one longer track)
inline std::vector<int> plan_lin_runs(int Pl, const std::vector<int>& lptr, int lin_threads) {
    std::vector<int> lb(1, 0);
    for (int p = 0; p < Pl; ++p)  // close the run before a track that would overflow it
        if (p > lb.back() && (lptr[p + 1] - lptr[lb.back()] > lin_threads || p - lb.back() >= lin_threads))
            lb.push_back(p);
    if (Pl > 0) lb.push_back(Pl);
    return lb;
}

// ---- coarse-space lists --------------------------------------------------------------------------------------
// Cluster membership (clp / clc, cpos the inverse of clc, alone = singleton cluster), per row the neighbour slots
// ordered by (cluster of the neighbour, slot) (sperm) and one segment per neighbour cluster (rsp / segs:
// {cluster, begin, end, own}; the row's own cluster always has one: it carries the diagonal term), and the E source
// lists per cluster pair (row cluster c', column cluster c): the segments of c's rows, rows ascending (eptr / eseg).
struct CoarseLists {
    std::vector<int> clp, clc, cpos, alone, sperm, rsp, eptr, eseg;
    std::vector<Int4> segs;
    int maxmem = 1, maxseg = 1;
};
inline CoarseLists plan_coarse(HostPool& pool, int C, int nc, const std::vector<int>& lab, const NbrLists& n) {
    CoarseLists c;
    const std::vector<int>&nptr = n.nptr, &nj = n.nj;
    c.clp.assign(nc + 1, 0);
    c.clc.resize(C);
    c.alone.resize(C);
    for (int i = 0; i < C; ++i) c.clp[lab[i] + 1]++;
    for (int k = 0; k < nc; ++k) c.clp[k + 1] += c.clp[k];
    {
        std::vector<int> fill(c.clp.begin(), c.clp.end() - 1);
        for (int i = 0; i < C; ++i) c.clc[fill[lab[i]]++] = i;
    }
    for (int k = 0; k < nc; ++k) c.maxmem = std::max(c.maxmem, c.clp[k + 1] - c.clp[k]);
    for (int i = 0; i < C; ++i) c.alone[i] = (c.clp[lab[i] + 1] - c.clp[lab[i]]) < 2;
    c.cpos.resize(C);
    for (int q = 0; q < C; ++q) c.cpos[c.clc[q]] = q;
    c.sperm.assign(std::max<int64_t>(n.n_nbr, 1), 0);
    c.rsp.assign(C + 1, 0);
    {
        // rows in parallel (each row's segments into its own list), then concatenated in row order
        std::vector<std::vector<Int4>> rsegs(C);
        pool.ranges(C, [&](int, long long i0, long long i1) {
            std::vector<int> ord;
            for (int i = (int)i0; i < (int)i1; ++i) {
                const int n0 = nptr[i], n1 = nptr[i + 1];
                ord.resize(n1 - n0);
                for (int q = 0; q < n1 - n0; ++q) ord[q] = n0 + q;
                std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return lab[nj[x]] < lab[nj[y]]; });
                for (int q = 0; q < n1 - n0; ++q) c.sperm[n0 + q] = ord[q];
                const int own = lab[i];
                bool own_done = false;
                int q = 0;
                std::vector<Int4>& out = rsegs[i];
                while (q < n1 - n0 || !own_done) {
                    const int cq = q < n1 - n0 ? lab[nj[ord[q]]] : nc;
                    if (!own_done && own < cq) {  // own cluster without neighbours in it
                        out.push_back(Int4{own, q, q, 1});
                        own_done = true;
                        continue;
                    }
                    int qe = q;
                    while (qe < n1 - n0 && lab[nj[ord[qe]]] == cq) ++qe;
                    out.push_back(Int4{cq, q, qe, cq == own ? 1 : 0});
                    if (cq == own) own_done = true;
                    q = qe;
                }
            }
        });
        for (int i = 0; i < C; ++i) {
            c.segs.insert(c.segs.end(), rsegs[i].begin(), rsegs[i].end());
            c.rsp[i + 1] = (int)c.segs.size();
            c.maxseg = std::max(c.maxseg, (int)rsegs[i].size());
        }
    }
    c.eptr.assign((size_t)nc * nc + 1, 0);
    c.eseg.reserve(c.segs.size());
    {
        std::vector<std::vector<int>> bucket(nc);
        for (int cr = 0; cr < nc; ++cr) {
            for (auto& v : bucket) v.clear();
            for (int e = c.clp[cr]; e < c.clp[cr + 1]; ++e) {
                const int i = c.clc[e];
                for (int sidx = c.rsp[i]; sidx < c.rsp[i + 1]; ++sidx) bucket[c.segs[sidx].x].push_back(sidx);
            }
            for (int k = 0; k < nc; ++k) {
                c.eseg.insert(c.eseg.end(), bucket[k].begin(), bucket[k].end());
                c.eptr[(size_t)cr * nc + k + 1] = (int)c.eseg.size();
            }
        }
    }
    if (c.eseg.empty()) c.eseg.push_back(0);
    return c;
}

// ---- k_tl_cgp facts ------------------------------------------------------------------------------------------
// What the persistent register-resident CG (ba_cgp.h) needs of the lists: rows of at most 128 blocks (nb = its
// register-block count: 64, 128, or 0 = too long; wide: 128 even for shorter rows), in cluster order (sperm the
// identity), at most seg_max (kCgpSegMax) neighbour clusters per row.
struct CgpFacts {
    int maxlen = 0, nb = 0;
    bool in_order = true;
    bool ok = false;  // nb && in_order && maxseg <= seg_max
};
inline CgpFacts plan_cgp_facts(int C, const NbrLists& n, const CoarseLists& c, int seg_max, bool wide) {
    CgpFacts f;
    for (int i = 0; i < C; ++i) f.maxlen = std::max(f.maxlen, n.nptr[i + 1] - n.nptr[i]);
    for (int64_t q = 0; q < n.n_nbr && f.in_order; ++q) f.in_order = c.sperm[q] == q;
    f.nb = (f.maxlen <= 64 && !wide) ? 64 : f.maxlen <= 128 ? 128 : 0;
    f.ok = f.nb && f.in_order && c.maxseg <= seg_max;
    return f;
}

// k_tl_cgp holds S unscaled: the S block (and orientation) of every slot -- e (upper), ~e (lower, transposed),
// pad_slot (kCgpPadSlot: a zero block)
inline std::vector<int> plan_cgp_src(const std::vector<int>& rptr, const LowerLists& l, const NbrLists& n, int pad_slot) {
    std::vector<int> src((size_t)std::max<int64_t>(n.n_nbr, 1), pad_slot);
    const int nnzb = (int)l.brow.size();
    for (int e = 0; e < nnzb; ++e) {
        if (e == rptr[l.brow[e]]) continue;  // diagonal block: no slot
        src[n.pup[e]] = e;
        src[n.plo[e]] = ~e;
    }
    return src;
}

}  // namespace insfm
