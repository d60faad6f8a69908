// CPU driver of the host planning of insfm_ba_create (instantsfm_amd/csrc/create_plan.h): reads one scene's index
// arrays, runs every stage the way create_impl does and dumps the resulting arrays; tests/test_create_plan.py checks
// them.  Usage: create_plan_test IN OUT POOL
//   IN   int32: a header of kHdr words (below), cam_idx[N], pt_idx[N], then the device-style upper lists of the block
//        pattern ulen[C], unb[U], uwt[U] (what k_pattern would write)
//   OUT  int32: the arrays in the order of the manifest printed to stdout ("array NAME COUNT" / "scalar NAME VALUE")
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../instantsfm_amd/csrc/create_plan.h"

using namespace insfm;

namespace {

enum {
    hC, hP, hN, hP0, hP1, hD, hCoarse, hClusterSize, hXChunks, hChunk, hLdsBudget, hLdsTarget, hWaves, hWs, hBs,
    hLinThreads, hCoarseMax, hSegMax, hPadSlot, hU, kHdr
};

FILE* g_out = nullptr;

template <class V>
void dump(const char* name, const V& v) {
    std::vector<int> buf(v.begin(), v.end());
    for (size_t i = 0; i < buf.size(); ++i)
        if ((long long)buf[i] != (long long)v[i]) { std::fprintf(stderr, "%s does not fit int32\n", name); std::exit(2); }
    if (!buf.empty() && std::fwrite(buf.data(), sizeof(int), buf.size(), g_out) != buf.size()) std::exit(3);
    std::printf("array %s %zu\n", name, buf.size());
}
void dump4(const char* name, const std::vector<Int4>& v) {
    std::vector<int> flat;
    for (const Int4& q : v) { flat.push_back(q.x); flat.push_back(q.y); flat.push_back(q.z); flat.push_back(q.w); }
    dump(name, flat);
}
void scalar(const char* name, long long v) { std::printf("scalar %s %lld\n", name, v); }

void dump_pattern(const std::string& pre, const BlockPattern& b) {
    dump((pre + "rptr").c_str(), b.rptr);
    dump((pre + "cols").c_str(), b.cols);
    dump((pre + "g_ptr").c_str(), b.g.ptr);
    dump((pre + "g_nb").c_str(), b.g.nb);
    dump((pre + "g_w").c_str(), b.g.w);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) return 1;
    std::vector<int> in;
    {
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) return 1;
        int buf[4096];
        size_t n;
        while ((n = std::fread(buf, sizeof(int), 4096, f)) > 0) in.insert(in.end(), buf, buf + n);
        std::fclose(f);
    }
    if (in.size() < (size_t)kHdr) return 1;
    const int C = in[hC], P = in[hP], N = in[hN], p0 = in[hP0], p1 = in[hP1], D = in[hD], U = in[hU];
    if (in.size() != (size_t)kHdr + 2 * (size_t)N + C + 2 * (size_t)U) return 1;
    const int32_t* cam_idx = in.data() + kHdr;
    const int32_t* pt_idx = cam_idx + N;
    const std::vector<int> ulen(pt_idx + N, pt_idx + N + C), unb(pt_idx + N + C, pt_idx + N + C + U),
        uwt(pt_idx + N + C + U, pt_idx + N + C + 2 * U);
    g_out = std::fopen(argv[2], "wb");
    if (!g_out) return 1;
    HostPool pool(std::atoi(argv[3]));

    const int bad = plan_check_inputs(pool, C, P, N, cam_idx, pt_idx);
    scalar("check", bad);
    if (bad) return std::fclose(g_out);

    const TrackOrder trk = plan_track_order(pool, P, N, p0, p1, cam_idx, pt_idx);
    scalar("o0", trk.o0);
    scalar("Nl", trk.Nl);
    dump("gptr", trk.gptr); dump("lptr", trk.lptr); dump("lsrc", trk.lsrc); dump("lcam", trk.lcam);
    dump("lptl", trk.lptl); dump("lust", trk.lust); dump("key", trk.key);
    const CamMajor cm = plan_cam_major(pool, C, trk, in[hChunk]);
    dump("cptr", cm.cptr); dump("cobs", cm.cobs);

    // the pattern in both forms: the host pass, and the assembly from the device-style upper lists
    const BlockPattern pat = plan_pattern_host(pool, C, N, cam_idx, pt_idx, trk.gptr);
    dump("gcptr", pat.gcptr);
    dump_pattern("", pat);
    const LowerLists low = plan_lower(C, pat.rptr, pat.cols);
    dump("brow", low.brow); dump("lop", low.lop); dump("locol", low.locol); dump("loblk", low.loblk);
    {
        std::vector<int> uoff(C + 1, 0);
        for (int i = 0; i < C; ++i) uoff[i + 1] = uoff[i] + ulen[i];
        BlockPattern dev = plan_pattern_from_upper(C, ulen, uoff, unb, uwt);
        plan_graph_from_upper(C, plan_lower(C, dev.rptr, dev.cols), dev);
        dump_pattern("dev_", dev);
        dump("dev_upw", dev.upw);
    }

    Clusters cl;
    if (in[hCoarse]) cl = plan_clusters(pat.g, C, in[hClusterSize], D + 1, in[hCoarseMax]);
    scalar("nc", cl.nc);
    scalar("coarse_ok", cl.coarse_ok);
    dump("lab", cl.lab);

    const NbrLists nbr = plan_nbr_lists(C, pat.rptr, pat.cols, low, cl.coarse_ok, cl.lab);
    scalar("nbr_stride", nbr.nbr_stride);
    scalar("n_nbr", nbr.n_nbr);
    dump("nptr", nbr.nptr); dump("nj", nbr.nj); dump("pup", nbr.pup); dump("plo", nbr.plo);

    const SchurLimits lim{(size_t)in[hLdsBudget], (size_t)in[hLdsTarget], in[hWaves], in[hWs], in[hBs]};
    const SchurWork sw = plan_schur_work(C, D, lim, pat.gcptr, pat.rptr);
    scalar("fits", sw.fits);
    scalar("cap", sw.cap);
    scalar("max_chunk", sw.max_chunk);
    scalar("schur_lds", (long long)sw.schur_lds);
    dump4("work", sw.work);
    const ExchangeChunks xc = plan_exchange(C, in[hXChunks], pat.rptr, sw.work);
    dump("xr", xc.xr); dump("xw", xc.xw);
    dump("lb", plan_lin_runs(p1 - p0, trk.lptr, in[hLinThreads]));

    if (cl.coarse_ok) {
        const CoarseLists co = plan_coarse(pool, C, cl.nc, cl.lab, nbr);
        scalar("maxmem", co.maxmem);
        scalar("maxseg", co.maxseg);
        dump("clp", co.clp); dump("clc", co.clc); dump("cpos", co.cpos); dump("alone", co.alone);
        dump("sperm", co.sperm); dump("rsp", co.rsp); dump4("segs", co.segs); dump("eptr", co.eptr);
        dump("eseg", co.eseg);
        const CgpFacts f = plan_cgp_facts(C, nbr, co, in[hSegMax], false);
        scalar("maxlen", f.maxlen);
        scalar("in_order", f.in_order);
        scalar("nb", f.nb);
        scalar("cgp_ok", f.ok);
        scalar("nb_wide", plan_cgp_facts(C, nbr, co, in[hSegMax], true).nb);
    }
    dump("src", plan_cgp_src(pat.rptr, low, nbr, in[hPadSlot]));
    return std::fclose(g_out);
}
