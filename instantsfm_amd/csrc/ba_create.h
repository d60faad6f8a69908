// Creation of a solver handle: validate, plan the index arrays (create_plan.h, plain C++), upload them, allocate the
// numeric buffers and set up streams, events and the two-level preconditioner.  Part of the one translation unit
// ba_kernels.hip (included after the kernels and the solve path: it names k_schur, k_tl_pc and cgp_kernel).
//
// The order of the device allocations and of the work enqueued on h->stream is part of the behaviour: the device
// cache (ba_handle.h) hands out parked buffers by request order, and the clears are stream-ordered.
#pragma once
#include "ba_handle.h"
#include "cg_poll.h"
#include "create_plan.h"

namespace {

// ---- create: structure derived on the device --------------------------------------------------------------------
// Per local track p (observations sorted by camera): each observation's track and the start of its camera run, i.e.
// of its upper partners (the tail of the track from there on).
__global__ __launch_bounds__(kThreads) void k_derive_tracks(int Pl, const int* __restrict__ pt_ptr, const int* __restrict__ cam,
                                                            int* __restrict__ ptl, int* __restrict__ ustart) {
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= Pl) return;
    const int b0 = pt_ptr[p], b1 = pt_ptr[p + 1];
    int u = b0, prev = -1;
    for (int o = b0; o < b1; ++o) {
        const int c = cam[o];
        if (c != prev) { u = o; prev = c; }
        ptl[o] = p;
        ustart[o] = u;
    }
}
// Per camera-major entry e (observation o = cam_obs[e]): the Schur descriptor {o, p, partner begin, partner end} and,
// for the BA, the point and uv the camera linearization reads.
__global__ __launch_bounds__(kThreads) void k_derive_cm(int Nl, const int* __restrict__ cam_obs, const int* __restrict__ ptl,
                                                        const int* __restrict__ ustart, const int* __restrict__ pt_ptr,
                                                        const double* __restrict__ uv, int4* __restrict__ sdesc,
                                                        int* __restrict__ cm_pt, double* __restrict__ cm_uv) {
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= Nl) return;
    const int o = cam_obs[e], p = ptl[o];
    sdesc[e] = make_int4(o, p, ustart[o], pt_ptr[p + 1]);
    if (uv) {
        cm_pt[e] = p;
        reinterpret_cast<double2*>(cm_uv)[e] = reinterpret_cast<const double2*>(uv)[o];
    }
}

// Upper block pattern of S and the co-visibility weights on the device (create, single rank; plan_pattern_host is the
// multi-rank / INSFM_DIAG=pattern_host path and gives the same lists): one workgroup per camera row i counts, in
// LDS, for every camera j the (observation of i, observation of j) pairs sharing a track, walking each own
// observation's upper partners [ustart, track end) exactly like k_schur.  `off` null: cnt[i] = #{j > i with pairs};
// else the j > i in increasing order and their pair counts go to nb / wt from off[i] (the second pass recounts).
constexpr int kPatternMaxC = 16384;  // the row's counters in <= 64 KB of LDS
__global__ __launch_bounds__(256) void k_pattern(int C, const int* __restrict__ cam_ptr, const int* __restrict__ cam_obs,
                                                 const int* __restrict__ ustart, const int* __restrict__ ptl,
                                                 const int* __restrict__ pt_ptr, const int* __restrict__ cam,
                                                 int* __restrict__ cnt, const int* __restrict__ off, int* __restrict__ nb,
                                                 int* __restrict__ wt) {
    extern __shared__ int acc[];  // [C]
    __shared__ int wsum[4];
    const int i = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    for (int j = t; j < C; j += 256) acc[j] = 0;
    __syncthreads();
    for (int e = cam_ptr[i] + t; e < cam_ptr[i + 1]; e += 256) {
        const int o = cam_obs[e];
        const int q1 = pt_ptr[ptl[o] + 1];
        for (int q = ustart[o]; q < q1; ++q) {
            const int j = cam[q];
            if (j != i) atomicAdd(&acc[j], 1);  // (the run of camera i itself: the observation and its duplicates)
        }
    }
    __syncthreads();
    if (!off) {
        int c = 0;
        for (int j = i + 1 + t; j < C; j += 256) c += acc[j] > 0;
        for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
        if (lane == 0) wsum[w] = c;
        __syncthreads();
        if (t == 0) cnt[i] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        return;
    }
    int base = off[i];
    for (int j0 = i + 1; j0 < C; j0 += 256) {  // ordered compaction, 256 columns at a time
        const int j = j0 + t;
        const int v = j < C ? acc[j] : 0;
        const unsigned long long bal = __ballot(v > 0);
        if (lane == 0) wsum[w] = __popcll(bal);
        __syncthreads();
        int wo = 0;
        for (int k = 0; k < w; ++k) wo += wsum[k];
        if (v > 0) {
            const int at = base + wo + __popcll(bal & ((1ull << lane) - 1));
            nb[at] = j;
            wt[at] = v;
        }
        base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
}

// ---- small helpers ----------------------------------------------------------------------------------------------
int create_err(insfm_ba* h, int rc, const std::string& msg) {
    h->err = msg;
    return rc;
}
int dd(insfm_ba* h, double** p, size_t n) { return dalloc(h, (void**)p, n * sizeof(double)); }
// the CG's cross-workgroup hand-off buffers (atomic partial sums, exchanged w, tagged granules, barrier words) in
// uncached device memory (INSFM_DIAG=cgp_cached: ordinary memory, for A/B runs)
int hand(insfm_ba* h, void** p, size_t bytes) { return dalloc(h, p, bytes, !diag("cgp_cached")); }
// the Int4 records of the plan go to the device as int4
int upload_int4(insfm_ba* h, int4** dst, const std::vector<Int4>& v) {
    return upload(h, dst, reinterpret_cast<const int4*>(v.data()), v.size());
}

// desc and the problem sizes into the handle
int create_validate(insfm_ba* h, const insfm_ba_desc* desc, int kind, const double* obs, const int32_t* cam_idx,
                    const int32_t* pt_idx, const double* cpar) {
    if (kind == 1) {
        h->model = kGP;
        h->ni = 0;
        h->D = 3;
        h->stride = 3;
        h->d.optimize_poses = 1;
    } else {
        h->model = desc->cam_model;
        h->ni = model_ni(h->model);
        if (h->ni < 0) return create_err(h, INSFM_BA_EINVAL, "unsupported camera model " + std::to_string(h->model));
        h->D = 6 + h->ni;
        h->stride = 7 + h->ni;
    }
    h->C = desc->n_cams; h->P = desc->n_points; h->N = desc->n_obs;
    if (h->C <= 0 || h->P <= 0 || h->N < 0) return create_err(h, INSFM_BA_EINVAL, "empty problem");
    if (!obs || !cam_idx || !pt_idx || !cpar) return create_err(h, INSFM_BA_EINVAL, "null input pointer");
    if (desc->world_size < 1 || desc->rank < 0 || desc->rank >= desc->world_size) return create_err(h, INSFM_BA_EINVAL, "bad rank");
    if (desc->world_size > 1 && !desc->allreduce) return create_err(h, INSFM_BA_EINVAL, "world_size > 1 needs allreduce");
    if (h->C > 30000) return create_err(h, INSFM_BA_EINVAL, "n_cams > 30000 not supported (LDS slot table)");
    // desc.schur_variant: only 0 (the W-reading k_schur) remains.  Variants 1 / 2 (camera-point blocks re-derived per
    // pair, LDS-atomic rows / MFMA register accumulation) and 3 (compact W records) were built, parity-tested and
    // measured slower or even in rounds 2-3; they live in the git history.
    if (desc->schur_variant != 0) return create_err(h, INSFM_BA_EINVAL, "schur_variant must be 0");
    return 0;
}

// The per-observation arrays go to the device, and what is derived there from them instead of uploaded (88 of 140 MB
// for config 3): per observation its track and the start of its upper partners; per camera-major entry the Schur
// descriptor and (BA) the linearization's point / uv gathers.
int upload_observations(insfm_ba* h, HostPool& pool, const double* obs, const double* cpar, const int32_t* sfree_in,
                        const TrackOrder& t, const CamMajor& cm) {
    const int C = h->C, Nl = h->Nl, Pl = h->Pl, kind = h->kind;
    const nivec<int>& lsrc = t.lsrc;
    int rc;
    if (kind == 1) {
        nivec<double> tl((size_t)3 * Nl);
        nivec<int> sl(Nl);
        pool.ranges(Nl, [&](int, long long a, long long b) {
            for (long long o = a; o < b; ++o) {
                for (int k = 0; k < 3; ++k) tl[3 * (size_t)o + k] = obs[3 * (size_t)lsrc[o] + k];
                sl[o] = sfree_in ? (sfree_in[lsrc[o]] != 0) : 1;
            }
        });
        if ((rc = upload(h, &h->trans, tl.data(), tl.size()))) return rc;
        if ((rc = upload(h, &h->sfree, sl.data(), sl.size()))) return rc;
        if ((rc = upload(h, &h->fcam, cpar, (size_t)C))) return rc;
        if ((rc = upload(h, &h->osrc, lsrc.data(), lsrc.size()))) return rc;
        h->osrc_host.assign(lsrc.begin(), lsrc.end());
        if ((rc = dd(h, &h->gobs, (size_t)Nl * kGO))) return rc;
        if ((rc = dd(h, &h->Up, (size_t)C * 9))) return rc;
        if ((rc = dd(h, &h->VY, (size_t)std::max(Pl, 1) * kVY))) return rc;
        if ((rc = dd(h, &h->gpc, (size_t)C * 3))) return rc;
        if ((rc = dd(h, &h->scl_cur, (size_t)std::max(Nl, 1)))) return rc;
        if ((rc = dd(h, &h->scl_new, (size_t)std::max(Nl, 1)))) return rc;
        if ((rc = dd(h, &h->ds, (size_t)std::max(Nl, 1)))) return rc;
    } else {
        nivec<double> uvl((size_t)2 * Nl);
        pool.ranges(Nl, [&](int, long long a, long long b) {
            for (long long o = a; o < b; ++o) {
                uvl[2 * (size_t)o] = obs[2 * (size_t)lsrc[o]];
                uvl[2 * (size_t)o + 1] = obs[2 * (size_t)lsrc[o] + 1];
            }
        });
        if ((rc = upload(h, &h->uv, uvl.data(), uvl.size()))) return rc;
        if ((rc = upload(h, &h->pp, cpar, (size_t)2 * C))) return rc;
    }
    if ((rc = upload(h, &h->cam, t.lcam.data(), t.lcam.size()))) return rc;
    if ((rc = upload(h, &h->pt_ptr, t.lptr.data(), t.lptr.size()))) return rc;
    if ((rc = upload(h, &h->cam_ptr, cm.cptr.data(), cm.cptr.size()))) return rc;
    if ((rc = upload(h, &h->cam_obs, cm.cobs.data(), cm.cobs.size()))) return rc;
    if ((rc = dalloc(h, (void**)&h->ptl, sizeof(int) * (size_t)std::max(Nl, 1)))) return rc;
    if ((rc = dalloc(h, (void**)&h->ustart, sizeof(int) * (size_t)std::max(Nl, 1)))) return rc;
    if ((rc = dalloc(h, (void**)&h->sdesc, sizeof(int4) * (size_t)std::max(Nl, 1)))) return rc;
    if (kind != 1) {
        if ((rc = dalloc(h, (void**)&h->cm_pt, sizeof(int) * (size_t)std::max(Nl, 1)))) return rc;
        if ((rc = dalloc(h, (void**)&h->cm_uv, sizeof(double) * 2 * (size_t)std::max(Nl, 1)))) return rc;
    }
    if (Pl > 0) k_derive_tracks<<<cdiv(Pl, kThreads), kThreads, 0, h->stream>>>(Pl, h->pt_ptr, h->cam, h->ptl, h->ustart);
    if (Nl > 0)
        k_derive_cm<<<cdiv(Nl, kThreads), kThreads, 0, h->stream>>>(Nl, h->cam_obs, h->ptl, h->ustart, h->pt_ptr,
                                                                    kind != 1 ? h->uv : nullptr, h->sdesc, h->cm_pt,
                                                                    h->cm_uv);
    return launch_err(h, "k_derive");
}

// The block pattern on the device (single rank): k_pattern in two passes (count, then fill from the offsets), the
// upper lists read back and assembled by plan_pattern_from_upper.
int device_pattern(insfm_ba* h, BlockPattern* out) {
    const int C = h->C;
    int rc;
    // (scratch from dalloc: a hipFree here would synchronize the device; it goes back with the handle's buffers)
    int *dcnt = nullptr, *doff = nullptr, *dnb = nullptr, *dwt = nullptr;
    const size_t lds = sizeof(int) * (size_t)C;
    std::vector<int> ulen(C), uoff(C + 1, 0);
    if ((rc = dalloc(h, (void**)&dcnt, sizeof(int) * (size_t)C))) return rc;
    if ((rc = dalloc(h, (void**)&doff, sizeof(int) * (size_t)(C + 1)))) return rc;
    hipError_t e = hipSuccess;
    {
        k_pattern<<<C, 256, lds, h->stream>>>(C, h->cam_ptr, h->cam_obs, h->ustart, h->ptl, h->pt_ptr, h->cam, dcnt,
                                              nullptr, nullptr, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(ulen.data(), dcnt, sizeof(int) * (size_t)C, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    for (int i = 0; i < C && e == hipSuccess; ++i) uoff[i + 1] = uoff[i] + ulen[i];
    const int U = uoff[C];
    std::vector<int> unb(std::max(U, 1)), uwt(std::max(U, 1));
    if (e == hipSuccess && ((rc = dalloc(h, (void**)&dnb, sizeof(int) * (size_t)std::max(U, 1))) ||
                            (rc = dalloc(h, (void**)&dwt, sizeof(int) * (size_t)std::max(U, 1)))))
        return rc;
    if (e == hipSuccess) e = hipMemcpyAsync(doff, uoff.data(), sizeof(int) * (size_t)(C + 1), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
        k_pattern<<<C, 256, lds, h->stream>>>(C, h->cam_ptr, h->cam_obs, h->ustart, h->ptl, h->pt_ptr, h->cam, nullptr,
                                              doff, dnb, dwt);
        e = hipGetLastError();
    }
    if (e == hipSuccess && U > 0) e = hipMemcpyAsync(unb.data(), dnb, sizeof(int) * (size_t)U, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && U > 0) e = hipMemcpyAsync(uwt.data(), dwt, sizeof(int) * (size_t)U, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return create_err(h, INSFM_BA_EHIP, std::string("k_pattern: ") + hipGetErrorString(e));
    *out = plan_pattern_from_upper(C, ulen, uoff, unb, uwt);
    return 0;
}

// the chunked [S | b] exchange (desc.allreduce_async): chunk boundaries, the exchange stream and its events
int setup_exchange(insfm_ba* h, const std::vector<int>& rptr, const std::vector<Int4>& work) {
    ExchangeChunks x = plan_exchange(h->C, h->d.exchange_chunks, rptr, work);
    h->rptr_host = rptr;
    h->xr = std::move(x.xr);
    h->xw = std::move(x.xw);
    hipError_t e = hipStreamCreateWithFlags(&h->xstream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_x, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_xdone, hipEventDisableTiming);
    if (e != hipSuccess) return create_err(h, INSFM_BA_EHIP, std::string("exchange stream: ") + hipGetErrorString(e));
    return 0;
}

// Camera linearization beside k_lin_points / k_schur (u_late), single rank (multi-rank, U / g_c are all-reduced
// before the Schur build adds them).
int setup_lin_stream(insfm_ba* h) {
    hipError_t e = helper_stream(1, 0, &h->aux);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_lin0, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_lc, hipEventDisableTiming);
    if (e != hipSuccess) return create_err(h, INSFM_BA_EHIP, std::string("linearization stream: ") + hipGetErrorString(e));
    h->u_late = true;
    return 0;
}

// the structure of S and of the CG's neighbour lists to the device; Sn allocated and cleared
int upload_structure(insfm_ba* h, const TrackOrder& t, const BlockPattern& pat, const LowerLists& low,
                     const NbrLists& nbr, const SchurWork& sw) {
    const int D = h->D;
    int rc;
    if (h->kind != 1) {
        const std::vector<int> lb = plan_lin_runs(h->Pl, t.lptr, kLinThreads);
        h->n_lin = (int)lb.size() - 1;
        if ((rc = upload(h, &h->lin_blk, lb.data(), lb.size()))) return rc;
    }
    if ((rc = upload(h, &h->row_ptr, pat.rptr.data(), pat.rptr.size()))) return rc;
    if ((rc = upload(h, &h->col, pat.cols.data(), pat.cols.size()))) return rc;
    if ((rc = upload(h, &h->blk_row, low.brow.data(), low.brow.size()))) return rc;
    if ((rc = upload(h, &h->nbr_ptr, nbr.nptr.data(), nbr.nptr.size()))) return rc;
    if ((rc = upload(h, &h->nbr_j, nbr.nj.data(), nbr.nj.size()))) return rc;
    if ((rc = upload(h, &h->pos_up, nbr.pup.data(), nbr.pup.size()))) return rc;
    h->pos_up_host = nbr.pup;
    if ((rc = upload(h, &h->pos_lo, nbr.plo.data(), nbr.plo.size()))) return rc;
    {
        const int DPd = D + (D & 1);
        const size_t snb = sizeof(double) * (size_t)std::max<int64_t>(h->n_nbr, 1) * D * DPd;
        if ((rc = dalloc(h, (void**)&h->Sn, snb))) return rc;
        if (hipMemsetAsync(h->Sn, 0, snb, h->stream) != hipSuccess) return create_err(h, INSFM_BA_EHIP, "Sn clear");
    }
    return upload_int4(h, &h->work, sw.work);
}

// the numeric buffers of the LM step and the CG
int alloc_numeric(insfm_ba* h) {
    const int C = h->C, D = h->D, Nl = h->Nl, Pl = h->Pl, kind = h->kind;
    const int maxit = h->d.pcg_max_iter;
    int rc;
    // W: [3][D] records per observation (global positioning: its 32-B {u, beta^2} records fit in the same buffer)
    if ((rc = dd(h, &h->W, (size_t)Nl * D * 3 + 2))) return rc;
    if ((rc = dd(h, &h->V, (size_t)Pl * 6))) return rc;
    if ((rc = dd(h, &h->gp, (size_t)Pl * 3))) return rc;
    if ((rc = dd(h, &h->Vinv, (size_t)Pl * 6))) return rc;
    if ((rc = dd(h, &h->y, (size_t)Pl * 3))) return rc;
    if (kind == 0) {
        if ((rc = dd(h, &h->Rf, (size_t)Pl * 6))) return rc;
        if ((rc = dd(h, &h->Mp, (size_t)Pl * 6))) return rc;
    }
    if ((rc = dd(h, &h->dp, (size_t)Pl * 3))) return rc;
    h->xcount = (int64_t)h->nnzb * D * D + (int64_t)C * D + (int64_t)C * D * D + (int64_t)C * D + 8;
    if ((rc = dd(h, &h->xbuf, (size_t)h->xcount))) return rc;
    h->S = h->xbuf;
    h->b = h->S + (size_t)h->nnzb * D * D;
    h->U = h->b + (size_t)C * D;
    h->gc = h->U + (size_t)C * D * D;
    h->scal = h->gc + (size_t)C * D;
    if ((rc = dd(h, &h->Lf, (size_t)C * D * D))) return rc;
    if ((rc = dd(h, &h->Li, (size_t)C * D * D))) return rc;
    if ((rc = dd(h, &h->dc, (size_t)C * D))) return rc;
    h->cg_nwg = C;  // one workgroup (and one partial record) per camera row
    const size_t cd = (size_t)C * D;
    const size_t cgn = 8 * cd + 2 * 3 * (size_t)h->cg_nwg + 2 * ((size_t)maxit + 2) + 16;
    if ((rc = dd(h, &h->cgmem, cgn))) return rc;
    {
        double* m = h->cgmem;
        h->cg.r[0] = m; m += cd; h->cg.r[1] = m; m += cd;
        h->cg.w[0] = m; m += cd; h->cg.w[1] = m; m += cd;
        h->cg.s[0] = m; m += cd; h->cg.s[1] = m; m += cd;
        h->cg.p = m; m += cd; h->cg.x = m; m += cd;
        h->cg.part[0] = m; m += 3 * (size_t)h->cg_nwg; h->cg.part[1] = m; m += 3 * (size_t)h->cg_nwg;
        h->cg.hist = m; m += 2 * ((size_t)maxit + 2);
        h->cg.scal = m; m += 4;
    }
    if ((rc = dalloc(h, (void**)&h->cg.status, sizeof(int) * 4))) return rc;
    const int ST = h->stride;
    if ((rc = dd(h, &h->cams_cur, (size_t)C * ST))) return rc;
    if ((rc = dd(h, &h->cams_new, (size_t)C * ST))) return rc;
    if ((rc = dd(h, &h->pts_cur, (size_t)std::max(Pl, 1) * 3))) return rc;
    if ((rc = dd(h, &h->pts_new, (size_t)std::max(Pl, 1) * 3))) return rc;
    h->n_cost = std::max(1, cdiv(Nl, kind == 1 ? kThreads : kCostThreads));
    h->n_gp = std::max(1, cdiv(Pl, kThreads));
    h->n_gp_grp = std::max(1, cdiv((long long)Pl * kGPG, kThreads));
    if (kind == 1) h->n_gp = h->n_gp_grp;  // the gain partials of k_gp_backsub
    else h->n_gp = std::max(1, h->n_lin);   // one per run of k_backsub
    h->n_gc = std::max(1, cdiv(C, kLinThreads));  // camera-update blocks (ride along with k_backsub_rc)
    if ((rc = dd(h, &h->part_cost, 2 * (size_t)h->n_cost))) return rc;
    if ((rc = dd(h, &h->part_gp, (size_t)h->n_gp))) return rc;
    if ((rc = dd(h, &h->part_gc, (size_t)h->n_gc))) return rc;
    h->result = h->scal;  // the 4 result scalars are all-reduced in place with the exchange buffer
    return dalloc(h, (void**)&h->flags, sizeof(int) * 4);
}

// pinned result memory, the phase events, the first clears (then the stream is idle), the Schur kernels' LDS limit
int setup_host_sync(insfm_ba* h) {
    {
        hipError_t e = hipHostMalloc((void**)&h->host_res, 128, hipHostMallocDefault);
        if (e != hipSuccess) return create_err(h, INSFM_BA_ENOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
        // the published cost block (without it, or with a cross-rank sum installed, costs come back by copy + sync)
        void* pm = nullptr;
        if (hipHostMalloc(&pm, 16 * sizeof(double), hipHostMallocMapped) == hipSuccess) {
            void* dp = nullptr;
            if (hipHostGetDevicePointer(&dp, pm, 0) == hipSuccess) {
                h->pub_host = static_cast<double*>(pm);
                h->pub_dev = static_cast<double*>(dp);
                std::memset(pm, 0, 16 * sizeof(double));
            } else {
                (void)hipHostFree(pm);
            }
        }
    }
    for (auto& e : h->ev) {
        hipError_t x = hipEventCreate(&e);
        if (x != hipSuccess) return create_err(h, INSFM_BA_EHIP, std::string("hipEventCreate: ") + hipGetErrorString(x));
    }
    if (h->d.world_size > 1 || h->d.allreduce) {
        const hipError_t x = hipEventCreateWithFlags(&h->ev_pre, hipEventDisableTiming);
        if (x != hipSuccess) return create_err(h, INSFM_BA_EHIP, std::string("hipEventCreate: ") + hipGetErrorString(x));
    }
    {
        hipError_t e = hipMemsetAsync(h->part_gp, 0, sizeof(double) * h->n_gp, h->stream);
        if (e == hipSuccess) e = hipMemsetAsync(h->part_gc, 0, sizeof(double) * h->n_gc, h->stream);
        if (e == hipSuccess) e = hipMemsetAsync(h->flags, 0, sizeof(int) * 4, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) return create_err(h, INSFM_BA_EHIP, std::string("init: ") + hipGetErrorString(e));
    }
    // the Schur kernels this handle launches (first trial, retried trial) may need more than the default dynamic-LDS limit
    const bool det = h->d.deterministic != 0;
    for (const bool retry : {false, true})
        if (const SchurKernel k = schur_kernel(h->kind, h->D, det, retry))
            (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->schur_lds);
    if (h->kind == 1 && !det)
        (void)hipFuncSetAttribute((const void*)k_schur_gp<kSchurWaves, kGPSG>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)h->schur_lds);
    return 0;
}

// two-level preconditioner: the cluster and segment lists to the device
int upload_coarse_lists(insfm_ba* h, const CoarseLists& co) {
    TlBufs& tl = h->tl;
    int rc;
    int* ip = nullptr;
    if ((rc = upload(h, &ip, co.clp.data(), co.clp.size()))) return rc;
    tl.cl_ptr = ip;
    if ((rc = upload(h, &ip, co.clc.data(), co.clc.size()))) return rc;
    tl.cl_cams = ip;
    if ((rc = upload(h, &ip, co.cpos.data(), co.cpos.size()))) return rc;
    tl.cpos = ip;
    if ((rc = upload(h, &ip, co.alone.data(), co.alone.size()))) return rc;
    tl.alone = ip;
    if ((rc = upload(h, &ip, co.sperm.data(), co.sperm.size()))) return rc;
    tl.sperm = ip;
    if ((rc = upload(h, &ip, co.rsp.data(), co.rsp.size()))) return rc;
    tl.rseg_ptr = ip;
    if ((rc = upload(h, &ip, co.eptr.data(), co.eptr.size()))) return rc;
    tl.ered_ptr = ip;
    if ((rc = upload(h, &ip, co.eseg.data(), co.eseg.size()))) return rc;
    tl.ered_seg = ip;
    int4* sp = nullptr;
    if ((rc = upload_int4(h, &sp, co.segs))) return rc;
    tl.seg = sp;
    return 0;
}

// two-level preconditioner: buffers, the side stream of the coarse-inverse chain, k_tl_pc's LDS
int setup_two_level(insfm_ba* h, const Clusters& cl, const CoarseLists& co) {
    const int C = h->C, D = h->D, MC = D + 1, nc = cl.nc, m = nc * MC;
    const size_t cd = (size_t)C * D;
    const insfm_ba_desc* desc = &h->d;
    TlBufs& tl = h->tl;
    int rc;
    tl.nc = nc;
    tl.m = m;
    tl.maxmem = co.maxmem;
    const int ldE = gj_steps(m) * kGB;
    tl.ldE = ldE;
    if ((rc = upload_coarse_lists(h, co))) return rc;
    if ((rc = dd(h, &tl.u, cd))) return rc;
    if ((rc = dd(h, &tl.Zt, cd * MC))) return rc;
    if ((rc = dd(h, &tl.Ztc, cd * MC))) return rc;
    if ((rc = dd(h, &tl.vc, cd))) return rc;
    if ((rc = dd(h, &tl.Rc, (size_t)m))) return rc;
    if ((rc = dd(h, &tl.gd, 3 * (size_t)C))) return rc;
    tl.gpref = nullptr;
    if (h->kind == 1 && (rc = dd(h, &tl.gpref, 3 * (size_t)nc))) return rc;
    {
        int* ip = nullptr;
        if ((rc = upload(h, &ip, cl.lab.data(), cl.lab.size()))) return rc;
        tl.clab = ip;
        // atomic cluster sums of the CG partials: single GPU, non-deterministic mode only -- the replicated
        // multi-rank CG needs bitwise-equal inputs on every rank (config 3: CG iteration 23.9 -> 22.3 us, round 3)
        tl.Racc = nullptr;
        tl.Gacc = nullptr;
        if (!desc->deterministic && desc->world_size <= 1 && !desc->allreduce) {
            if ((rc = hand(h, (void**)&tl.Racc, sizeof(double) * 3 * (size_t)m))) return rc;
            if ((rc = hand(h, (void**)&tl.Gacc, sizeof(double) * 3 * 3 * (size_t)nc))) return rc;
            if (hipMemsetAsync(tl.Racc, 0, sizeof(double) * 3 * (size_t)m, h->stream) != hipSuccess ||
                hipMemsetAsync(tl.Gacc, 0, sizeof(double) * 9 * (size_t)nc, h->stream) != hipSuccess)
                return create_err(h, INSFM_BA_EHIP, "Racc clear");
        }
    }
    if ((rc = dd(h, &tl.rowR, (size_t)C * MC + 2))) return rc;  // +2: k_tl_pc reads it in 16-B pairs
    if ((rc = dd(h, &tl.Oseg, co.segs.size() * MC * MC))) return rc;
    {
        // E is kept padded to whole blocks; the pad is the identity (k_tl_ereduce writes only the m x m part and
        // the Gauss-Jordan steps keep the pad an identity)
        std::vector<double> eye((size_t)ldE * ldE, 0.0);
        for (int q = m; q < ldE; ++q) eye[(size_t)q * ldE + q] = 1.0;
        for (int sl = 0; sl < 2; ++sl) {
            if ((rc = upload(h, &h->Ebuf[sl], eye.data(), eye.size()))) return rc;
            if ((rc = dd(h, &h->Einvbuf[sl], (size_t)m * m))) return rc;
        }
    }
    if ((rc = dd(h, &h->gjW, (size_t)ldE * ldE))) return rc;
    if ((rc = dd(h, &h->gjP, (size_t)2 * kGB * kGB))) return rc;
    {
        std::vector<double> ones(ldE, 1.0);   // equilibration of the pad (k_tl_ereduce writes the first m)
        if ((rc = upload(h, &tl.Ed, ones.data(), ones.size()))) return rc;
    }
    if ((rc = dalloc(h, (void**)&h->okbuf, sizeof(int) * 2))) return rc;
    tl.E = h->Ebuf[0];
    tl.Einv = h->Einvbuf[0];
    tl.ok = h->okbuf;
    hipError_t e = hipMemsetAsync(h->okbuf, 0, sizeof(int) * 2, h->stream);
    // The side stream (E build + factorization, off the critical path) at the lowest priority (ROCm exposes only
    // normal and high: no measured effect either way, round 1)
    int prio_lo = 0, prio_hi = 0;
    if (e == hipSuccess) e = hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    // (INSFM_DIAG=side_hi / side_normal: the side stream at the high / normal priority instead, for A/B runs)
    const int side_prio = diag("side_hi") ? prio_hi : diag("side_normal") ? 0 : prio_lo;
    if (e == hipSuccess) e = helper_stream(0, side_prio, &h->side);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_E, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_built, hipEventDisableTiming);
    for (int sl = 0; sl < 2 && e == hipSuccess; ++sl) e = hipEventCreateWithFlags(&h->ev_fact[sl], hipEventDisableTiming);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return create_err(h, INSFM_BA_EHIP, std::string("two-level init: ") + hipGetErrorString(e));
    {
        const size_t fixed = sizeof(double) * ((size_t)MC * m + (size_t)m), budget = 144 * 1024;
        h->pc_rows = (int)std::min<size_t>((size_t)C, (budget - fixed) / (sizeof(double) * MC));
        h->pc_lds = fixed + sizeof(double) * (size_t)h->pc_rows * MC;
    }
    if (h->pc_lds > 150 * 1024)
        return create_err(h, INSFM_BA_EINVAL,
                          "two-level preconditioner: scene too connected for the LDS budget (use precond 0)");
    with_D(D, [&](auto dc_) -> int {
        constexpr int DV = decltype(dc_)::value;
        (void)hipFuncSetAttribute((const void*)k_tl_pc<DV>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)h->pc_lds);
        return 0;
    });
    h->tlon = true;
    void* pm = nullptr;
    if (hipHostMalloc(&pm, sizeof(int) * 8, hipHostMallocMapped) == hipSuccess) {
        h->prog_host = static_cast<int*>(pm);
        void* dp = nullptr;
        if (hipHostGetDevicePointer(&dp, pm, 0) == hipSuccess) h->cg.prog = static_cast<int*>(dp);
        else { (void)hipHostFree(pm); h->prog_host = nullptr; }
    }
    return 0;
}

// The persistent register-resident CG (ba_cgp.h): D = 8, host-mapped progress, rows of at most NB = 128 blocks in
// cluster order, at most kCgpSegMax neighbour clusters per row (plan_cgp_facts), and the whole grid resident at once.
int setup_cgp(insfm_ba* h, const BlockPattern& pat, const LowerLists& low, const NbrLists& nbr, const CoarseLists& co) {
    const int C = h->C, D = h->D, MC = D + 1;
    const size_t cd = (size_t)C * D;
    TlBufs& tl = h->tl;
    int rc;
    const CgpFacts f = plan_cgp_facts(C, nbr, co, kCgpSegMax, diag("cgp128"));
    const int nb = f.nb, grid = (C + kCgpRows - 1) / kCgpRows;
    if (diag("create"))
        std::fprintf(stderr, "[insfm create] k_tl_cgp eligibility: D %d, atomic sums %d, progress %d, max row %d, "
                     "cluster order %d, max segments %d\n", D, tl.Racc != nullptr, h->prog_host != nullptr, f.maxlen,
                     (int)f.in_order, co.maxseg);
    // non-deterministic single rank: per-cluster atomic sums (tl.Racc); otherwise (deterministic mode, or every
    // rank of a replicated multi-rank CG) the fixed-order variant
    // (INSFM_DIAG=cgp_det: the fixed-order variant on a non-deterministic handle too, for A/B runs)
    const bool det = tl.Racc == nullptr || diag("cgp_det");
    // precond 2 (A-DEF2) in either form (round 6: the fixed-order DET form too); the launch path runs the additive
    // form of precond 1
    const bool adef = h->d.precond == 2;
    if (!(D == 8 && h->prog_host && f.ok && !diag("no_cgp"))) return 0;
    int dev = 0, ncu = 0, per_cu = 0;
    hipError_t ce = hipGetDevice(&dev);
    if (ce == hipSuccess) ce = hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    if (ce == hipSuccess)
        ce = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)cgp_kernel(nb, det, adef), kCgpThreads, 0);
    if (!(ce == hipSuccess && per_cu >= 1 && grid <= ncu)) return 0;
    if ((rc = hand(h, (void**)&h->cgp_wx, sizeof(double) * 2 * cd))) return rc;
    if ((rc = hand(h, (void**)&h->cgp_yg, sizeof(unsigned long long) * 2 * kCoarseMax))) return rc;
    if (hipMemsetAsync(h->cgp_yg, 0, sizeof(unsigned long long) * 2 * kCoarseMax, h->stream) != hipSuccess)
        return create_err(h, INSFM_BA_EHIP, "cgp granules");
    if ((rc = hand(h, (void**)&h->cgp_sync, sizeof(unsigned) * kCgpSyncWords))) return rc;
    if (hipMemsetAsync(h->cgp_sync, 0, sizeof(unsigned) * kCgpSyncWords, h->stream) != hipSuccess)
        return create_err(h, INSFM_BA_EHIP, "cgp barrier words");
    if (diag("cgp_trace") && (rc = dd(h, &h->cgp_trace, kCgpTraceLen))) return rc;
    // the run records: DET's partials by parity, and (every form) the restriction of r0 that
    // k_cg_factor_basis writes for the setup
    if ((rc = hand(h, (void**)&h->cgp_runs, sizeof(double) * 2 * 12 * (size_t)grid * kCgpRows))) return rc;
    // k_tl_cgp holds S unscaled: the S block (and orientation) of every slot, and the unscaled basis
    {
        const std::vector<int> src = plan_cgp_src(pat.rptr, low, nbr, kCgpPadSlot);
        if ((rc = upload(h, &h->cgp_src, src.data(), src.size()))) return rc;
        if ((rc = dd(h, &tl.Gb, cd * MC))) return rc;
    }
    h->cgp_det = det;
    h->adef2 = adef;
    h->cgp_nb = nb;
    h->cgp_grid = grid;
    h->cgp_slots = per_cu * ncu;
    if (diag("create"))
        std::fprintf(stderr, "[insfm create] k_tl_cgp<%d>: %d workgroups, %d CUs, %d per CU\n", nb, grid, ncu, per_cu);
    return 0;
}

// Shared creation of a BA (kind 0: obs = uv [N,2], cpar = pp [C,2]) or global-positioning (kind 1: obs = rays [N,3],
// cpar = camera factors [C], sfree = scale-free flags [N] or NULL) handle.
int create_impl(const insfm_ba_desc* desc, int kind, const double* obs, const int32_t* cam_idx, const int32_t* pt_idx,
                const double* cpar, const int32_t* sfree_in, void* stream, insfm_ba** out) {
    if (!desc || !out) return INSFM_BA_EINVAL;
    *out = nullptr;
    insfm_ba* h = new insfm_ba();
    h->d = *desc;
    h->kind = kind;
    h->stream = reinterpret_cast<hipStream_t>(stream);
    auto fail = [&](int rc, const std::string& msg) {
        if (!msg.empty()) h->err = msg;
        *out = h;  // handle returned so the caller can read the error; caller destroys it
        return rc;
    };
    int rc;
    if ((rc = create_validate(h, desc, kind, obs, cam_idx, pt_idx, cpar))) return fail(rc, "");
    const int C = h->C, P = h->P, N = h->N, D = h->D;
    // every pass over the observations below runs on this pool (create_host.h); joined when create returns
    HostPool pool(host_pool_size());
    switch (plan_check_inputs(pool, C, P, N, cam_idx, pt_idx)) {
        case 1: return fail(INSFM_BA_EINVAL, "cam_idx out of range");
        case 2: return fail(INSFM_BA_EINVAL, "pt_idx out of range");
        case 3: return fail(INSFM_BA_EINVAL, "observations must be track-major (pt_idx nondecreasing)");
        default: break;
    }
    h->p0 = std::max(0, desc->shard_point_begin);
    h->p1 = desc->shard_point_end < 0 ? P : std::min(P, desc->shard_point_end);
    if (h->p1 < h->p0) return fail(INSFM_BA_EINVAL, "bad shard range");
    h->Pl = h->p1 - h->p0;
    // INSFM_DIAG=create: host milliseconds of create's phases (stderr)
    static const bool ctrace = diag("create");
    const double ct0 = wall_seconds();
    auto tick = [&](const char* what) {
        if (ctrace) std::fprintf(stderr, "[insfm create] %-28s %8.1f ms\n", what, 1e3 * (wall_seconds() - ct0));
    };
    const TrackOrder trk = plan_track_order(pool, P, N, h->p0, h->p1, cam_idx, pt_idx);
    h->o0 = trk.o0;
    h->Nl = trk.Nl;
    const int o0 = h->o0, Nl = h->Nl, Pl = h->Pl;
    tick("local track order");
    const CamMajor cm = plan_cam_major(pool, C, trk, kSchurChunk * kSchurWaves * (64 / D));
    tick("camera-major lists");
    // the per-observation arrays go to the device now: the block pattern below is derived there (single rank)
    if ((rc = upload_observations(h, pool, obs, cpar, sfree_in, trk, cm))) return fail(rc, "");
    tick("uploads (observations)");
    // The block pattern and the co-visibility graph.  Single rank: on the device (k_pattern), the lower half of the
    // graph transposed from the upper on the host.  Multi-rank (every rank needs the global pattern, and holds only its
    // shard's observations on the device) or INSFM_DIAG=pattern_host: one host pass over the global camera-major list.
    static const bool pattern_host = diag("pattern_host");
    const bool gpu_pattern = !pattern_host && Pl == P && o0 == 0 && Nl == N && C <= kPatternMaxC && Nl > 0;
    BlockPattern pat;
    if (gpu_pattern) {
        if ((rc = device_pattern(h, &pat))) return fail(rc, "");
        pat.gcptr = cm.cptr;  // (single rank: the local camera-major list is the global one)
    } else {
        pat = plan_pattern_host(pool, C, N, cam_idx, pt_idx, trk.gptr);
    }
    h->nnzb = pat.rptr[C];
    const LowerLists low = plan_lower(C, pat.rptr, pat.cols);
    if (gpu_pattern) plan_graph_from_upper(C, low, pat);
    tick("block pattern + covisibility");
    if (desc->precond < 0 || desc->precond > 2) return fail(INSFM_BA_EINVAL, "precond must be 0, 1 or 2");
    Clusters cl;
    if (desc->precond >= 1 && h->d.optimize_poses) cl = plan_clusters(pat.g, C, desc->cluster_size, D + 1, kCoarseMax);
    h->clab_host = cl.lab;
    tick("clusters");
    const NbrLists nbr = plan_nbr_lists(C, pat.rptr, pat.cols, low, cl.coarse_ok, cl.lab);
    h->nbr_stride = nbr.nbr_stride;
    h->n_nbr = nbr.n_nbr;
    tick("CG neighbour lists");
    const bool det_schur = desc->deterministic != 0;
    const SchurLimits lim{(size_t)kLdsBudget, det_schur ? (size_t)kLdsTargetDet : (size_t)kLdsTarget,
                          det_schur ? kDetWaves : kSchurWaves, schur_ws(D), schur_bs(D)};
    const SchurWork sw = plan_schur_work(C, D, lim, pat.gcptr, pat.rptr);
    if (!sw.fits) return fail(INSFM_BA_EINVAL, "too many cameras for LDS");
    h->nwork = (int)sw.work.size();
    h->max_chunk = sw.max_chunk;
    if (kind == 0 && desc->allreduce_async && (desc->world_size > 1 || desc->allreduce) && desc->exchange_chunks > 1 &&
        desc->optimize_poses && (rc = setup_exchange(h, pat.rptr, sw.work)))
        return fail(rc, "");
    h->schur_lds = sw.schur_lds;
    if (kind == 0 && desc->world_size <= 1 && !desc->allreduce && (rc = setup_lin_stream(h))) return fail(rc, "");
    if ((rc = upload_structure(h, trk, pat, low, nbr, sw))) return fail(rc, "");
    if ((rc = alloc_numeric(h))) return fail(rc, "");
    if ((rc = setup_host_sync(h))) return fail(rc, "");
    tick("uploads + allocations");
    if (cl.coarse_ok) {
        // ---- two-level preconditioner: source lists of E, buffers, the persistent CG ----
        const CoarseLists co = plan_coarse(pool, C, cl.nc, cl.lab, nbr);
        tick("coarse segments");
        if ((rc = setup_two_level(h, cl, co))) return fail(rc, "");
        if ((rc = setup_cgp(h, pat, low, nbr, co))) return fail(rc, "");
    }
    tick("two-level setup (end)");
    if (kind == 0 && diag("stamps")) {
        const size_t n = (size_t)kStampSteps * kStKinds * 2;
        if ((rc = dalloc(h, (void**)&h->stamps, sizeof(long long) * n))) return fail(rc, "");
        if (hipMemsetAsync(h->stamps, 0, sizeof(long long) * n, h->stream) != hipSuccess) return fail(INSFM_BA_EHIP, "stamps");
    }
    h->damping = 1.0 / desc->tr_radius;
    h->down = desc->tr_down;
    *out = h;
    return INSFM_BA_OK;
}

}  // namespace
