// The debug / timing C ABI (include/insfm_ba_debug.h): insfm_ba_debug_*, the row-partitioned CG prototype's
// insfm_ba_cg_window / attach / partition, insfm_gp_debug_*.  Part of the one translation unit ba_kernels.hip (included
// last: it names the product ABI's gp_io).
#pragma once
#include "ba_step.h"

extern "C" {

int32_t insfm_ba_debug_stamps(insfm_ba* h, int64_t* host_out, int32_t max_steps) {
    if (!h || !host_out || max_steps < 0) return INSFM_BA_EINVAL;
    if (!h->stamps) return 0;
    HIPCHK(hipStreamSynchronize(h->stream));
    const long long n = std::min<long long>(std::min<long long>(h->stamp_step, kStampSteps), max_steps);
    std::vector<long long> ring((size_t)kStampSteps * kStKinds * 2);
    HIPCHK(hipMemcpy(ring.data(), h->stamps, sizeof(long long) * ring.size(), hipMemcpyDeviceToHost));
    const long long first = h->stamp_step - n;  // the oldest of the last n steps
    for (long long q = 0; q < n; ++q) {
        const size_t src = (size_t)((first + q) % kStampSteps) * kStKinds * 2;
        std::memcpy(host_out + (size_t)q * kStKinds * 2, ring.data() + src, sizeof(long long) * kStKinds * 2);
    }
    return (int32_t)n;
}

int insfm_ba_cg_window(insfm_ba* h, void* ipc_handle) {
    if (!h || !ipc_handle) return INSFM_BA_EINVAL;
    if (h->kind != 0 || h->d.world_size < 2 || !h->tlon || h->tl.Racc || h->xwin) {
        h->err = "cg_window: needs a multi-rank two-level handle (precond 1) that has no window yet";
        return INSFM_BA_EINVAL;
    }
    h->cgp_nb = 0;  // (the partitioned launch path replaces the replicated persistent CG)
    const int C = h->C, D = h->D, MC = D + 1, W = h->d.world_size;
    const long long region = (long long)C * D + 3LL * C + (long long)C * MC + 2;
    h->xoff_region[0] = 0;
    h->xoff_region[1] = region;
    h->xoff_xg = 2 * region;
    h->xoff_flags = h->xoff_xg + (long long)C * D;
    h->xwin_bytes = sizeof(double) * (size_t)h->xoff_flags + sizeof(unsigned) * kXFlagStride * 2 * (size_t)W;
    // uncached device memory: peers write into it over their mappings, and no cache of this device keeps a stale line
    hipError_t e = hipExtMallocWithFlags(reinterpret_cast<void**>(&h->xwin), h->xwin_bytes, hipDeviceMallocUncached);
    if (e == hipSuccess) e = hipMemsetAsync(h->xwin, 0, h->xwin_bytes, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) e = hipIpcGetMemHandle(reinterpret_cast<hipIpcMemHandle_t*>(ipc_handle), h->xwin);
    if (e != hipSuccess) {
        h->err = std::string("cg_window: ") + hipGetErrorString(e);
        return INSFM_BA_EHIP;
    }
    return INSFM_BA_OK;
}

int insfm_ba_cg_attach(insfm_ba* h, const void* handles) {
    if (!h || !handles || !h->xwin || h->xpart) return INSFM_BA_EINVAL;
    const int W = h->d.world_size, C = h->C;
    std::vector<double*> bases(W, nullptr);
    std::vector<unsigned*> flags(W, nullptr);
    for (int r = 0; r < W; ++r) {
        if (r == h->d.rank) {
            bases[r] = h->xwin;
        } else {
            void* q = nullptr;
            hipIpcMemHandle_t hd;
            std::memcpy(&hd, static_cast<const char*>(handles) + (size_t)r * sizeof(hipIpcMemHandle_t), sizeof(hd));
            const hipError_t e = hipIpcOpenMemHandle(&q, hd, hipIpcMemLazyEnablePeerAccess);
            if (e != hipSuccess) {
                h->err = std::string("cg_attach: rank ") + std::to_string(r) + ": " + hipGetErrorString(e);
                return INSFM_BA_EHIP;
            }
            h->xopened.push_back(q);
            bases[r] = static_cast<double*>(q);
        }
        flags[r] = reinterpret_cast<unsigned*>(bases[r] + h->xoff_flags);
    }
    int rc = 0;
    if ((rc = dalloc(h, reinterpret_cast<void**>(&h->xbases), sizeof(double*) * W))) return rc;
    if ((rc = dalloc(h, reinterpret_cast<void**>(&h->xpflags), sizeof(unsigned*) * W))) return rc;
    if ((rc = dalloc(h, reinterpret_cast<void**>(&h->xcnt), sizeof(unsigned) * 2))) return rc;
    HIPCHK(hipMemcpyAsync(h->xbases, bases.data(), sizeof(double*) * W, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->xpflags, flags.data(), sizeof(unsigned*) * W, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(h->xcnt, 0, sizeof(unsigned) * 2, h->stream));
    // rows: the cluster-ordered positions split at cluster boundaries, rank r from the boundary nearest r C / W
    const std::vector<int>& lab = h->clab_host;
    std::vector<int> bnd;  // cluster-ordered boundaries (positions where a cluster starts), incl. 0 and C
    {
        std::vector<int> size(h->tl.nc, 0);
        for (int i = 0; i < C; ++i) size[lab[i]]++;
        int q = 0;
        for (int c = 0; c < h->tl.nc; ++c) { bnd.push_back(q); q += size[c]; }
        bnd.push_back(q);
    }
    h->xq.assign(W + 1, C);
    h->xq[0] = 0;
    for (int r = 1; r < W; ++r) {
        const long long target = (long long)r * C / W;
        int best = bnd[0];
        for (int b : bnd)
            if (std::llabs(b - target) < std::llabs(best - target)) best = b;
        h->xq[r] = std::max(best, h->xq[r - 1]);
    }
    // the basis writes r0 and its restriction into region 1 (what the setup k_tl_pc reads)
    h->tl = tl_region(h, 1);
    HIPCHK(hipStreamSynchronize(h->stream));
    h->xpart = true;
    return INSFM_BA_OK;
}

int insfm_ba_debug_time_xchg(insfm_ba* h, int32_t reps, double* us) {
    if (!h || !us || !h->xpart || reps < 1) return INSFM_BA_EINVAL;
    HIPCHK(hipEventRecord(h->ev[kEvDebug], h->stream));
    for (int r = 0; r < reps; ++r) launch_xchg(h, 1);  // (slot 1: not gated by the CG status)
    HIPCHK(hipEventRecord(h->ev[kEvDebugEnd], h->stream));
    HIPCHK(hipEventSynchronize(h->ev[kEvDebugEnd]));
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, h->ev[kEvDebug], h->ev[kEvDebugEnd]));
    *us = 1e3 * ms / reps;
    return INSFM_BA_OK;
}

int insfm_ba_cg_partition(const insfm_ba* h, int32_t* rows_begin_end) {
    if (!h || !rows_begin_end || !h->xpart) return INSFM_BA_EINVAL;
    rows_begin_end[0] = h->xq[h->d.rank];
    rows_begin_end[1] = h->xq[h->d.rank + 1];
    return INSFM_BA_OK;
}

int insfm_ba_debug_linearize(insfm_ba* h, const double* cams, const double* pts) {
    if (!h || !cams || !pts || h->kind != 0) return INSFM_BA_EINVAL;
    cgp_drop_pending(h);
    h->keep_S = 1;
    HIPCHK(hipMemcpyAsync(h->cams_cur, cams, sizeof(double) * (size_t)h->C * h->stride, hipMemcpyDeviceToDevice, h->stream));
    if (h->Pl)
        HIPCHK(hipMemcpyAsync(h->pts_cur, pts + 3 * (size_t)h->p0, sizeof(double) * (size_t)h->Pl * 3, hipMemcpyDeviceToDevice,
                              h->stream));
    int rc = run_linearize(h, h->cams_cur, h->pts_cur);
    if (!rc) rc = lin_join(h);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int insfm_ba_debug_solve(insfm_ba* h, double f) {
    if (!h) return INSFM_BA_EINVAL;
    cgp_drop_pending(h);
    h->keep_S = 1;
    // solves around the parameters last passed to insfm_ba_debug_linearize
    int it = run_solve(h, f, h->cams_cur, h->pts_cur, false);
    HIPCHK(hipStreamSynchronize(h->stream));
    return it;
}

int insfm_ba_debug_spd_inverse(int32_t m, const double* E, double* Einv, void* stream, int32_t reps,
                               double* us_per_inverse) {
    if (m < 1 || m > 4096 || !E || !Einv) return INSFM_BA_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nB = gj_steps(m), ld = nB * kGB;
    const int n = reps > 0 && us_per_inverse ? reps : 1;
    // the padded, identity-extended copy and the equilibration d = 1 / sqrt(diag E) are built on the host
    std::vector<double> Eh((size_t)m * m), Ep((size_t)ld * ld, 0.0), dh(ld, 1.0);
    if (hipMemcpy(Eh.data(), E, sizeof(double) * Eh.size(), hipMemcpyDeviceToHost) != hipSuccess) return INSFM_BA_EHIP;
    for (int r = 0; r < ld; ++r)
        for (int c = 0; c < ld; ++c)
            Ep[(size_t)r * ld + c] = (r < m && c < m) ? Eh[(size_t)r * m + c] : (r == c ? 1.0 : 0.0);
    for (int r = 0; r < m; ++r) dh[r] = 1.0 / std::sqrt(Eh[(size_t)r * m + r]);
    double *Ew = nullptr, *Ww = nullptr, *dd = nullptr, *Pw = nullptr;
    int* ok = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int okh = 0;
    float ms = 0.f;
    hipError_t e = hipMalloc(&Ew, sizeof(double) * (size_t)ld * ld);
    if (e == hipSuccess) e = hipMalloc(&Ww, sizeof(double) * (size_t)ld * ld);
    if (e == hipSuccess) e = hipMalloc(&dd, sizeof(double) * ld);
    if (e == hipSuccess) e = hipMalloc(&Pw, sizeof(double) * 2 * kGB * kGB);
    if (e == hipSuccess) e = hipMalloc(&ok, sizeof(int));
    if (e == hipSuccess) e = hipMemcpy(dd, dh.data(), sizeof(double) * ld, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    for (int r = 0; r < n && e == hipSuccess; ++r) {
        e = hipMemcpyAsync(Ew, Ep.data(), sizeof(double) * Ep.size(), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipEventRecord(e0, st);
        for (int u = 0; u <= nB && e == hipSuccess; ++u) {
            launch_gj_unit(u, m, Ew, Ww, Pw, dd, Einv, ok, st);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(e1, st);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        float t = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
        ms += t;
    }
    if (e == hipSuccess) e = hipMemcpy(&okh, ok, sizeof(int), hipMemcpyDeviceToHost);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipFree(Ew); (void)hipFree(Ww); (void)hipFree(dd); (void)hipFree(Pw); (void)hipFree(ok);
    if (e != hipSuccess) return INSFM_BA_EHIP;
    if (us_per_inverse) *us_per_inverse = 1e3 * ms / n;
    return okh ? 1 : 0;
}

int insfm_ba_debug_time_kernel(insfm_ba* h, int32_t which, int32_t reps, double* us_per_launch) {
    if (!h || reps <= 0 || !us_per_launch || !h->d.optimize_poses) return INSFM_BA_EINVAL;
    // re-run one kernel `reps` times back to back on the data of the last solve; the CG state it overwrites is
    // scratch once the solve has finished (dc already extracted).  0: k_cg_iter  1: k_schur (damping factor 1)
    // 2: one two-level CG iteration  3: k_tl_pspmv  4: the two-level setup  5: k_lin_points (overwrites W / V / g_p)
    HIPCHK(hipMemsetAsync(h->cg.status, 0, sizeof(int) * 4, h->stream));
    HIPCHK(hipMemsetAsync(h->cg.scal, 0, sizeof(double) * 4, h->stream));
    if (((which >= 2 && which <= 4) || which == 6 || which == 7) && !h->tlon) return INSFM_BA_EINVAL;
    if (which == 5 && (h->kind != 0 || !h->W)) return INSFM_BA_EINVAL;
    if (which < 0 || which > 7) return INSFM_BA_EINVAL;
    if (int rc0 = side_flush(h)) return rc0;  // its pending E build / factorization must not interleave
    if (int rc0 = lin_join(h)) return rc0;
    if (which != 1 && which != 5 && which != 6)
        if (int rc0 = ensure_sn(h)) return rc0;  // (kernels that read the scaled copy Sn)
    if (which == 2 && h->tl.Racc) {
        // atomic cluster sums: iteration 1's k_tl_pc reads buffer 1 every repetition (its k_tl_pspmv adds into buffer
        // 0, which the next repetition clears), so fill buffer 1 once from a k_tl_pspmv of iteration 0
        HIPCHK(hipMemsetAsync(h->tl.Racc + h->tl.m, 0, sizeof(double) * h->tl.m, h->stream));
        HIPCHK(hipMemsetAsync(h->tl.Gacc + 3 * h->tl.nc, 0, sizeof(double) * 3 * h->tl.nc, h->stream));
        with_D(h->D, [&](auto dc_) -> int {
            launch_pspmv<decltype(dc_)::value>(h, 0, h->C, h->tl);
            return 0;
        });
    }
    HIPCHK(hipEventRecord(h->ev[kEvDebug], h->stream));
    int rc = with_D(h->D, [&](auto dc_) -> int {
        constexpr int DV = decltype(dc_)::value;
        for (int r = 0; r < reps; ++r) {
            if (which == 2) {
                launch_tl_iter<DV>(h, 1, h->d.pcg_max_iter, 0.0);
            } else if (which == 3) {
                launch_pspmv<DV>(h, 1, h->C, h->tl);
            } else if (which == 4) {
                int rc2 = run_tl_basis(h, h->cams_cur, h->stream);
                if (!rc2) rc2 = run_tl_build(h, 0, h->stream);
                for (int u = 0; u <= gj_steps(h->tl.m) && !rc2; ++u) rc2 = run_tl_gj_unit(h, 0, u, h->stream);
                if (rc2) return rc2;
            } else if (which == 6) {  // the coarse inverse alone: k_gj_pinv0 + nB x k_gj_step on slot 0's E
                for (int u = 1; u <= gj_steps(h->tl.m) + 1; ++u)
                    if (int rc2 = run_tl_gj_unit(h, 0, u - 1, h->stream)) return rc2;
            } else if (which == 7) {  // the E build alone: k_tl_erow + k_tl_ereduce
                if (int rc2 = run_tl_build(h, 0, h->stream)) return rc2;
            } else if (which == 5 && h->kind == 0 && h->W) {  // k_lin_points at the last trial's parameters
                with_model(h->model, [&](auto mc) -> int {
                    constexpr int M = decltype(mc)::value;
                    if (h->Pl > 0) launch_lin_points_w<M>(h, h->cams_new, h->pts_new, first_trial_prep(h));
                    return 0;
                });
            } else if (which == 0)
                k_cg_iter<DV><<<h->C, kCgThreads, 0, h->stream>>>(1, h->C, h->d.pcg_max_iter, 0.0, h->nbr_ptr, h->nbr_j, h->Sn,
                                                                h->Lf, h->cg);
            else {  // the k_schur form this handle runs (deterministic mode: one wave per workgroup, its LDS layout)
                const int rc2 = launch_schur(h, 1.0, h->kind ? -1e308 : h->d.clamp_min,
                                             h->kind ? 1e308 : h->d.clamp_max, h->kind ? 1 : h->d.rank == 0, false);
                if (rc2) return rc2;
            }
        }
        return launch_err(h, "debug_time_kernel");
    });
    if (rc) return rc;
    HIPCHK(hipEventRecord(h->ev[kEvDebugEnd], h->stream));
    HIPCHK(hipEventSynchronize(h->ev[kEvDebugEnd]));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, h->ev[kEvDebug], h->ev[kEvDebugEnd]));
    *us_per_launch = 1e3 * ms / reps;
    return INSFM_BA_OK;
}

int insfm_ba_debug_time_cgp(insfm_ba* h, int32_t reps, double* out) {
    // the persistent CG of the last solve again, `reps` times: k_cg_factor_basis on the completed S / b (no U / g_c
    // added: the same L, L^-1 and r0 = L^-1 b; Z~ and the restriction of r0), then the timed part -- the k_tl_cgp
    // launch, bracketed by events -- with the coarse segments written as in a lagged solve.  out[0] us per
    // k_tl_cgp launch, out[1] 0 (the setup launch k_tl_pc that preceded it until round 4 is folded in), out[2]
    // iterations (mean).
    if (!h || reps <= 0 || !out || !h->cgp_nb || h->kind != 0 || !h->prog_host) return INSFM_BA_EINVAL;
    cgp_drop_pending(h);
    if (int rc0 = side_flush(h)) return rc0;
    if (int rc0 = lin_join(h)) return rc0;
    double t_cg = 0.0, t_pc = 0.0, iters = 0.0;
    for (int r = 0; r < reps; ++r) {
        HIPCHK(hipMemsetAsync(h->cg.status, 0, sizeof(int) * 4, h->stream));
        // (the last trial's cameras; a handle whose solves did not form the basis with the factorization: k_tl_basis)
        if (int rc = refactor(h, h->last.basis_by_factor ? h->cams_new : nullptr)) return rc;
        if (!h->last.basis_by_factor)
            if (int rc = run_tl_basis(h, h->cams_new, h->stream)) return rc;
        volatile int* pg = h->prog_host;
        pg[0] = pg[1] = pg[2] = pg[3] = 0;
        std::atomic_thread_fence(std::memory_order_seq_cst);
        HIPCHK(hipEventRecord(h->ev[kEvDebug], h->stream));
        // (the segments are written, as in the lagged solves that are most of a run)
        if (int rc2 = launch_tl_cgp(h, h->adef2, true)) return rc2;
        HIPCHK(hipEventRecord(h->ev[kEvDebugEnd], h->stream));
        HIPCHK(hipEventSynchronize(h->ev[kEvDebugEnd]));
        int st[3];
        if (int rc2 = cgp_complete(h, h->adef2, st)) return rc2;
        if (st[0] != 1) {
            h->err = "debug_time_cgp: the CG ended with status " + std::to_string(st[0]);
            return st[0] == 2 ? INSFM_BA_ESOLVER : INSFM_BA_EHIP;
        }
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, h->ev[kEvDebug], h->ev[kEvDebugEnd]));
        t_cg += ms;
        iters += st[1];
    }
    // (round 5: the coarse solve of r0 runs inside k_tl_cgp; no setup launch in front of it)
    out[1] = t_pc;
    out[0] = 1e3 * t_cg / reps;
    out[2] = iters / reps;
    return INSFM_BA_OK;
}

int32_t insfm_ba_debug_clusters(const insfm_ba* h, int32_t* labels) {
    if (!h) return INSFM_BA_EINVAL;
    if (!h->tlon) return 0;
    if (labels) std::memcpy(labels, h->clab_host.data(), sizeof(int32_t) * h->C);
    return h->tl.nc;
}

int64_t insfm_ba_debug_get(insfm_ba* h, int32_t which, double* host) {
    if (!h || !host) return INSFM_BA_EINVAL;
    const size_t C = h->C, Pl = h->Pl, Nl = h->Nl, D = h->D;
    const double* src = nullptr;
    size_t n = 0;
    switch (which) {
        // (global positioning keeps its 32-byte {u, beta^2} records at the front of the same buffer: [N,4])
        case 0: src = h->W; n = h->kind == 1 ? Nl * 4 : Nl * D * 3; break;
        case 1: src = h->V; n = Pl * 6; break;
        case 2: src = h->gp; n = Pl * 3; break;
        case 3: src = h->U; n = C * D * D; break;
        case 4: src = h->gc; n = C * D; break;
        case 5: {  // the scaled upper blocks S~ (diagonal: I), assembled from the row-contiguous copy Sn
            if (h->kind != 0 && h->kind != 1) return INSFM_BA_EINVAL;
            if (int rc0 = side_flush(h)) return rc0;
            if (int rc0 = ensure_sn(h)) return rc0;
            const size_t DP = D + (D & 1), nb = (size_t)h->nnzb;
            std::vector<double> sn((size_t)std::max<int64_t>(h->n_nbr, 1) * D * DP);
            if (h->n_nbr) HIPCHK(hipMemcpyAsync(sn.data(), h->Sn, sizeof(double) * h->n_nbr * D * DP, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
            std::vector<int> rp(C + 1);
            HIPCHK(hipMemcpy(rp.data(), h->row_ptr, sizeof(int) * (C + 1), hipMemcpyDeviceToHost));
            std::vector<char> diag_blk(nb, 0);
            for (size_t i = 0; i < C; ++i) diag_blk[rp[i]] = 1;
            for (size_t e = 0; e < nb; ++e)
                for (size_t a = 0; a < D; ++a)
                    for (size_t c = 0; c < D; ++c)
                        host[(e * D + a) * D + c] = diag_blk[e] ? (a == c ? 1.0 : 0.0)
                                                                : sn[((size_t)h->pos_up_host[e] * D + a) * DP + c];
            return (int64_t)(nb * D * D);
        }
        case 6: src = h->b; n = C * D; break;
        case 7: src = h->dc; n = C * D; break;
        case 8: src = h->dp; n = Pl * 3; break;
        // two-level internals (debug): 9 u, 10 w, 11 rowR, 12/13 E^-1 slot 0/1, 14 row partials [r.u | w.u], 15 r
        case 9: src = h->tl.u; n = h->tlon ? C * D : 0; break;
        case 10: src = h->cg.w[0]; n = C * D; break;
        case 11: src = h->tl.rowR; n = h->tlon ? C * (D + 1) : 0; break;  // restriction row partials
        case 12: src = h->Einvbuf[0]; n = h->tlon ? (size_t)h->tl.m * h->tl.m : 0; break;
        case 13: src = h->Einvbuf[1]; n = h->tlon ? (size_t)h->tl.m * h->tl.m : 0; break;
        case 14: src = h->tl.gd; n = h->tlon ? 2 * C : 0; break;
        case 15: src = h->cg.r[0]; n = C * D; break;
        // 16/17 E slot 0/1 padded to whole blocks [ldE][ldE] (E^-1 once the slot's inversion has run)
        case 16: case 17: src = h->Ebuf[which - 16]; n = h->tlon ? (size_t)h->tl.ldE * h->tl.ldE : 0; break;
        // 18 the scaled coarse basis Z~ [C][D][MC] of the last two-level solve
        case 18: src = h->tl.Zt; n = h->tlon ? C * D * (D + 1) : 0; break;
        default: return INSFM_BA_EINVAL;
    }
    if (int rc0 = side_flush(h)) return rc0;
    if (int rc0 = lin_join(h)) return rc0;
    if (n) HIPCHK(hipMemcpyAsync(host, src, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return (int64_t)n;
}

int insfm_gp_debug_linearize(insfm_ba* h, const double* pos, const double* pts, const double* scales) {
    if (!h || !pos || !pts || !scales || h->kind != 1) return INSFM_BA_EINVAL;
    h->keep_S = 1;
    int rc = gp_io(h, 1, pos, pts, scales);
    if (rc) return rc;
    if ((rc = run_linearize(h, h->cams_cur, h->pts_cur))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int64_t insfm_gp_debug_get_ds(insfm_ba* h, double* host_out) {
    if (!h || !host_out || h->kind != 1) return INSFM_BA_EINVAL;
    std::vector<double> loc(h->Nl);
    if (h->Nl) HIPCHK(hipMemcpyAsync(loc.data(), h->ds, sizeof(double) * h->Nl, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    std::memset(host_out, 0, sizeof(double) * (size_t)h->N);
    for (int o = 0; o < h->Nl; ++o) host_out[h->osrc_host[o]] = loc[o];
    return h->N;
}

}  // extern "C"
