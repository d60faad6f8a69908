// MI355X (gfx950) sparse bundle-adjustment core behind include/insfm_ba.h: one translation unit.  This file holds the
// includes, in the order the headers need each other, and the C ABI; the kernels and the host driver are in headers.
//
// One LM step (bae.optim.LM.step as reconstructed in SURVEY.md 3.3, options of bundle_adjustment.py:115-119):
//   linearize (per step)   ba_lin.h      k_lin_points, k_lin_cams(_reg): the records Y_o, V_p, g_p, U_c, g_c and the
//                                        first trial's point preparation
//   per trial (damping f)  ba_lin.h      k_point_prep: a retried trial's V^-1, M_p, z'_p
//                          ba_schur.h    k_schur: per camera row, the LDS-resident row of S (upper blocks), b
//                          ba_pcg.h      k_cg_factor(_basis) / k_cg_scale: S_ii = L L^T, S~ = L^-1 S L^-T, r0 = L^-1 b
//                          ba_twolevel.h two-level setup (k_tl_basis, k_tl_erow, k_tl_ereduce) and, in ba_gj.h, the
//                                        dense inverse of the coarse matrix (k_gj_step)
//                          the CG        precond 1 / 2: the persistent k_tl_cgp (ba_cgp.h), one launch per solve, or
//                                        per iteration k_tl_pc_cl / k_tl_pc + k_tl_pspmv (ba_twolevel.h); precond 0:
//                                        k_cg_dots + k_cg_iter per iteration (ba_pcg.h)
//                          ba_pcg.h      k_cg_finish: dc = L^-T x~
//                          ba_trial.h    k_backsub_rc (dp, trial points and cameras, gain terms), k_cost, k_final (the
//                                        partials in a fixed order -> 64 B), k_publish (to the host's spin-wait)
//   global positioning     ba_gp.h       the same solve with D = 3 and its own linearization
//   host side              ba_handle.h; ba_solve.h executes what solve_policy.h plans (one solve), ba_step.h what
//                          lm_policy.h and cg_poll.h decide (the step); ba_create.h, create_plan.h, create_host.h
//                          (creation); ba_debug_api.h (the debug ABI)
// With desc.deterministic = 1 every cross-workgroup reduction is a fixed-order partial sum (no float atomics in global
// memory) and k_schur's workgroups run four waves that take their LDS adds in turn, so that each slot sees its
// additions in a fixed order: a step is then bitwise reproducible.
#include <hip/hip_runtime.h>

#include <atomic>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <unordered_map>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/insfm_ba.h"
#include "../../include/insfm_gp.h"
#include "../../include/insfm_ba_debug.h"
#include "ba_device.h"
#include "ba_common.h"
#include "ba_twolevel.h"
#include "ba_cgp.h"
#include "ba_gp.h"
#include "cg_poll.h"
#include "create_plan.h"

using namespace insfm;

#include "ba_lin.h"
#include "ba_schur.h"
#include "ba_pcg.h"
#include "ba_trial.h"

namespace {

inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

}  // namespace

// ============================================================================================================
// host side
// ============================================================================================================
#include "ba_handle.h"

#include "ba_solve.h"
#include "ba_step.h"

// ============================================================================================================
// C ABI
// ============================================================================================================
extern "C" {

void insfm_ba_default_desc(insfm_ba_desc* d) {
    std::memset(d, 0, sizeof(*d));
    d->cam_model = 2;
    d->optimize_poses = 1;
    d->deterministic = 0;
    d->huber_delta = 1.0;
    d->tr_radius = 1e4; d->tr_max = 1e10; d->tr_min = 1e-6; d->tr_up = 2.0; d->tr_down = 1.0 / 16.0;
    d->tr_factor = 0.25; d->tr_high = 0.5; d->tr_low = 1e-3;
    d->clamp_min = 1e-6; d->clamp_max = 1e32;
    d->max_rejects = 30;
    d->pcg_max_iter = 500;
    d->pcg_tol = 1e-5;
    d->world_size = 1; d->rank = 0;
    d->shard_point_begin = 0; d->shard_point_end = -1;
    d->precond = 2;
    d->cluster_size = 24;
    d->exchange_chunks = 4;
}

const char* insfm_ba_last_error(const insfm_ba* h) { return h ? h->err.c_str() : "null handle"; }

void insfm_ba_destroy(insfm_ba* h) {
    if (!h) return;
    if (h->side) (void)side_flush(h);
    // every stream that may still use the buffers, before they are parked for the next handle
    for (hipStream_t st : {h->stream, h->side, h->xstream, h->aux})
        if (st) (void)hipStreamSynchronize(st);
    if (!h->stream) (void)hipDeviceSynchronize();
    for (void* q : h->xopened) (void)hipIpcCloseMemHandle(q);  // (peers must be done writing: the caller's barrier)
    if (h->xwin) (void)hipFree(h->xwin);
    dfree_all(h);
    if (h->host_res) (void)hipHostFree(h->host_res);
    if (h->prog_host) (void)hipHostFree(h->prog_host);
    if (h->pub_host) (void)hipHostFree(h->pub_host);
    for (auto& e : h->ev)
        if (e) (void)hipEventDestroy(e);
    if (h->side) {
        (void)hipStreamSynchronize(h->side);
        release_helper_stream(h->side);
    }
    if (h->xstream) {
        (void)hipStreamSynchronize(h->xstream);
        (void)hipStreamDestroy(h->xstream);
    }
    if (h->aux) {
        (void)hipStreamSynchronize(h->aux);
        release_helper_stream(h->aux);
    }
    if (h->ev_lin0) (void)hipEventDestroy(h->ev_lin0);
    if (h->ev_lc) (void)hipEventDestroy(h->ev_lc);
    if (h->ev_x) (void)hipEventDestroy(h->ev_x);
    if (h->ev_xdone) (void)hipEventDestroy(h->ev_xdone);
    if (h->ev_pre) (void)hipEventDestroy(h->ev_pre);
    if (h->ev_E) (void)hipEventDestroy(h->ev_E);
    if (h->ev_built) (void)hipEventDestroy(h->ev_built);
    for (auto& e : h->ev_fact)
        if (e) (void)hipEventDestroy(e);
    delete h;
}

int64_t insfm_ba_nnzb(const insfm_ba* h) { return h ? h->nnzb : -1; }

int64_t insfm_ba_release_cache(void) { return (int64_t)release_cache(); }

}  // extern "C"

#include "ba_create.h"

extern "C" {

int insfm_ba_create(const insfm_ba_desc* desc, const double* obs_uv, const int32_t* cam_idx, const int32_t* pt_idx,
                    const double* pp, void* stream, insfm_ba** out) {
    return create_impl(desc, 0, obs_uv, cam_idx, pt_idx, pp, nullptr, stream, out);
}

int insfm_ba_set_timing(insfm_ba* h, int32_t on) {
    if (!h) return INSFM_BA_EINVAL;
    h->want_timing = on != 0;
    return INSFM_BA_OK;
}

int64_t insfm_ba_exchange_count(const insfm_ba* h) { return h ? h->xcount : -1; }

int insfm_ba_set_exchange(insfm_ba* h, double* buf, int64_t count) {
    if (!h || !buf || count < h->xcount) return INSFM_BA_EINVAL;
    const int C = h->C, D = h->D;
    h->xbuf = buf;
    h->S = h->xbuf;
    h->b = h->S + (size_t)h->nnzb * D * D;
    h->U = h->b + (size_t)C * D;
    h->gc = h->U + (size_t)C * D * D;
    h->scal = h->gc + (size_t)C * D;
    h->result = h->scal;
    return INSFM_BA_OK;
}

int insfm_ba_set_ranks_per_device(insfm_ba* h, int32_t ranks) {
    if (!h || ranks < 1) return INSFM_BA_EINVAL;
    if (h->cgp_nb && (long long)ranks * h->cgp_grid > (long long)h->cgp_slots) {
        if (diag("create"))
            std::fprintf(stderr, "[insfm create] %d ranks per GPU: k_tl_cgp would need %lld of %d workgroup slots; "
                         "launch path\n", ranks, (long long)ranks * h->cgp_grid, h->cgp_slots);
        h->cgp_nb = 0;
    }
    return INSFM_BA_OK;
}

int insfm_ba_cg_info(const insfm_ba* h, int32_t* out) {
    if (!h || !out) return INSFM_BA_EINVAL;
    out[0] = cg_path_code(h->xpart, h->cgp_nb, h->cgp_det, h->adef2);
    out[1] = h->cgp_grid;
    out[2] = h->cgp_slots;
    out[3] = h->cgp_nb;
    return INSFM_BA_OK;
}

int32_t insfm_ba_cg_fallbacks(const insfm_ba* h) {
    if (!h) return INSFM_BA_EINVAL;
    return h->adef2_fallbacks;
}

int insfm_ba_set_persistent_cg(insfm_ba* h, int32_t on) {
    if (!h) return INSFM_BA_EINVAL;
    if (on) return h->cgp_nb ? INSFM_BA_OK : INSFM_BA_EINVAL;  // (cannot turn on what create found ineligible)
    cgp_drop_pending(h);
    h->cgp_nb = 0;
    return INSFM_BA_OK;
}

int insfm_ba_reset(insfm_ba* h) {
    if (!h) return INSFM_BA_EINVAL;
    h->damping = 1.0 / h->d.tr_radius;
    h->down = h->d.tr_down;
    h->have_loss = false;
    // a fresh LM: the first solve after the reset factorizes its own coarse matrix (no lagged E^-1 of an earlier solve
    // survives) and the CG's first batch is sized as for a new handle
    cgp_drop_pending(h);
    if (int rc = side_flush(h)) return rc;
    h->ss.tl_solves = 0;
    h->ss.tl_fresh = false;
    h->ss.last_cg_iters = 16;
    h->chain_timed[0] = h->chain_timed[1] = false;
    return INSFM_BA_OK;
}

int insfm_ba_cost(insfm_ba* h, const double* cams, const double* pts, double* loss, double* rmse) {
    if (!h || !cams || !pts || h->kind != 0) return INSFM_BA_EINVAL;
    cgp_drop_pending(h);
    HIPCHK(hipMemsetAsync(h->flags, 0, sizeof(int) * 4, h->stream));
    int rc = run_cost(h, cams, pts + 3 * (size_t)h->p0, false);
    if (rc) return rc;
    if (loss) *loss = h->host_res[0];
    if (rmse) *rmse = h->N > 0 ? std::sqrt(h->host_res[1] / h->N) : 0.0;
    return INSFM_BA_OK;
}

int insfm_ba_step(insfm_ba* h, double* cams_user, double* pts_user, insfm_ba_stats* st) {
    if (!h || !cams_user || !pts_user || h->kind != 0) return INSFM_BA_EINVAL;
    // The caller's buffers are the linearization point of this step (read in place, no copy-in); trials go to the
    // internal cams_new / pts_new, and an accepted trial is copied back into the caller's buffers (stream-ordered, no
    // host wait: the step's loss is already on the host).
    double* const ic = h->cams_cur;
    double* const ip = h->pts_cur;
    h->cams_cur = cams_user;
    h->pts_cur = pts_user + 3 * (size_t)h->p0;
    h->ext_cur = true;
    const int rc = lm_step(h, st);
    h->cams_cur = ic;
    h->pts_cur = ip;
    h->ext_cur = false;
    return rc;
}

// ---- global positioning (include/insfm_gp.h) -------------------------------------------------------------------
void insfm_gp_default_desc(insfm_ba_desc* d) {
    insfm_ba_default_desc(d);
    d->cam_model = -1;
    d->huber_delta = 0.1;  // GLOBAL_POSITIONER_OPTIONS['thres_loss_function'] (config/colmap.py:41-46)
    d->tr_radius = 1e3;    // TrustRegion(radius=1e3, max=1e8, up=2.0, down=0.5**4) (global_positioning.py:158)
    d->tr_max = 1e8;
}

int insfm_gp_create(const insfm_ba_desc* desc, const double* trans, const int32_t* cam_idx, const int32_t* pt_idx,
                    const double* cam_factor, const int32_t* scale_free, void* stream, insfm_ba** out) {
    return create_impl(desc, 1, trans, cam_idx, pt_idx, cam_factor, scale_free, stream, out);
}

// Positions, the shard's points and the scales between the caller's buffers and the LM state (one k_gp_io launch).
static int gp_io(insfm_ba* h, int in, const double* pos, const double* pts, const double* scales) {
    const long long n3c = 3LL * h->C, n3p = 3LL * h->Pl, nl = h->Nl, tot = n3c + n3p + nl;
    if (tot == 0) return 0;
    const int grid = std::max(1, std::min(2048, cdiv(tot, kThreads)));
    k_gp_io<<<grid, kThreads, 0, h->stream>>>(in, n3c, const_cast<double*>(pos), h->cams_cur, n3p,
                                              const_cast<double*>(pts) + 3 * (size_t)h->p0, h->pts_cur, nl, h->osrc,
                                              const_cast<double*>(scales), h->scl_cur);
    return launch_err(h, "k_gp_io");
}

int insfm_gp_step(insfm_ba* h, double* pos, double* pts, double* scales, insfm_ba_stats* st) {
    if (!h || !pos || !pts || !scales || h->kind != 1) return INSFM_BA_EINVAL;
    int rc = gp_io(h, 1, pos, pts, scales);
    if (rc) return rc;
    if ((rc = lm_step(h, st))) return rc;
    // written back in stream order (no host wait: the step's loss is already on the host), like insfm_ba_step
    return gp_io(h, 0, pos, pts, scales);
}

int insfm_gp_cost(insfm_ba* h, const double* pos, const double* pts, const double* scales, double* loss, double* rmse) {
    if (!h || !pos || !pts || !scales || h->kind != 1) return INSFM_BA_EINVAL;
    HIPCHK(hipMemsetAsync(h->flags, 0, sizeof(int) * 4, h->stream));
    // scratch copies (the LM's current state is untouched: cams_new / pts_new / scl_new are trial buffers)
    HIPCHK(hipMemcpyAsync(h->cams_new, pos, sizeof(double) * 3 * (size_t)h->C, hipMemcpyDeviceToDevice, h->stream));
    if (h->Nl) k_gp_gather<<<cdiv(h->Nl, kThreads), kThreads, 0, h->stream>>>(h->Nl, h->osrc, scales, h->scl_new);
    int rc = launch_err(h, "k_gp_gather");
    if (rc) return rc;
    if ((rc = run_cost(h, h->cams_new, pts + 3 * (size_t)h->p0, false, h->scl_new))) return rc;
    if (loss) *loss = h->host_res[0];
    if (rmse) *rmse = h->N > 0 ? std::sqrt(h->host_res[1] / h->N) : 0.0;
    return INSFM_BA_OK;
}

}  // extern "C"

#include "ba_debug_api.h"
