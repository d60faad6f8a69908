/*
 * insfm_ba_debug.h -- introspection, timing probes and prototype entry points of libinsfm_ba.so that are not part of
 * the product ABI (insfm_ba.h, insfm_gp.h): what the parity tests, the profiling tools and the shelved row-partitioned
 * multi-rank CG use.  Same handle type, error codes and calling rules as insfm_ba.h; TorchBA / TorchGP need none of it.
 */
#ifndef INSFM_BA_DEBUG_H
#define INSFM_BA_DEBUG_H

#include "insfm_ba.h"
#include "insfm_gp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- bundle adjustment: introspection used by the parity tests ------------------------------------------- */
/* Linearize at DEVICE params (fills W, V, g_p, U, g_c). */
int insfm_ba_debug_linearize(insfm_ba* h, const double* cam_params, const double* points);
/* Build and solve the damped system for cumulative damping factor f; returns PCG iterations or a negative code. */
int insfm_ba_debug_solve(insfm_ba* h, double f);
/* Copy an internal buffer to HOST memory: 0 the camera-point records Y[N,3,D] (Y_o = W_o R_p^-T, R_p the Cholesky
 * factor of point p's block damped for the first trial: S = U - sum Y Y^T; column-major blocks) 1 V[P,6] 2 g_p[P,3] 3 U[C,D,D] 4 g_c[C,D] 5 S(scaled after a
 * solve)[nnzb,D,D] 6 b[C,D] 7 dc[C,D] 8 dp[P,3].  Two-level handles (0 doubles otherwise), m = clusters x (D + 1):
 * 9 u 10 w 11 the restriction's row partials [C,D+1] 12 / 13 E^-1 of coarse-inverse slot 0 / 1 [m,m] 14 the row
 * partials [r.u | w.u] 15 r 16 / 17 E of slot 0 / 1 padded to whole 32-blocks [ld,ld] (E^-1 once the slot's inversion
 * has run) 18 the scaled coarse basis Z~ [C,D,D+1] of the last solve.  Returns the number of doubles copied or a
 * negative code. */
int64_t insfm_ba_debug_get(insfm_ba* h, int32_t which, double* host_out);
/* Device time per launch (us, hipEvents on the library stream) of `reps` back-to-back launches of one kernel on the
 * data of the last solve: which = 0 k_cg_iter (one block-Jacobi CG iteration), 1 k_schur, 2 one two-level CG
 * iteration (k_tl_pc + k_tl_pspmv), 3 k_tl_pspmv alone, 4 the two-level setup (k_tl_basis, the E build k_tl_erow +
 * k_tl_ereduce, the Gauss-Jordan inversion k_gj_pinv0 + k_gj_step), 5 k_lin_points at the last trial's parameters
 * (BA with stored W records only), 6 the coarse inverse alone (k_gj_pinv0 + one k_gj_step per 32-wide block of E),
 * 7 the E build alone (k_tl_erow + k_tl_ereduce).  Overwrites CG scratch state. */
int insfm_ba_debug_time_kernel(insfm_ba* h, int32_t which, int32_t reps, double* us_per_launch);
/* The persistent two-level CG (k_tl_cgp, the default D = 8 solve) of the last solve, re-run `reps` times from its
 * right-hand side: out[0] device microseconds per k_tl_cgp launch (a whole solve: the coarse solve of r0, the in-kernel
 * setup and every iteration), out[1] 0 (reserved: the setup launch that preceded it until round 4), out[2] PCG
 * iterations per solve.  EINVAL when the handle does not
 * run k_tl_cgp.  Overwrites CG scratch state.  (Measurement of PCG(tol=1e-5), bundle_adjustment.py:117.) */
int insfm_ba_debug_time_cgp(insfm_ba* h, int32_t reps, double* out);
/* INSFM_DIAG=stamps only (else returns 0): the device-clock timestamps (wall_clock64, 100 MHz) of the last
 * min(steps taken, 1024, max_steps) LM steps, oldest first, [steps][10 kernels][entry, exit] as int64 into HOST
 * memory: kernels k_lin_points, k_schur, k_tl_cgp, k_cg_finish, k_publish, k_cg_factor, k_tl_basis, k_backsub_rc,
 * k_cost, k_final (the trial's: the last launch of each in the step; entry = workgroup 0's, exit = the latest
 * workgroup end; 0 = not launched).  Tracer-free main-queue busy time and gaps.  Returns the number of steps copied. */
int32_t insfm_ba_debug_stamps(insfm_ba* h, int64_t* host_out, int32_t max_steps);
/* Camera cluster labels [C] of the two-level preconditioner's coarse space (HOST out); returns the cluster count. */
int32_t insfm_ba_debug_clusters(const insfm_ba* h, int32_t* labels);
/* Number of upper-triangular camera blocks of the reduced system (incl. the diagonal). */
int64_t insfm_ba_nnzb(const insfm_ba* h);
/* E^-1 of a dense SPD matrix (DEVICE pointers, row-major m x m, 1 <= m <= 4096) by the two-level preconditioner's
 * blocked Gauss-Jordan kernels (k_gj_pinv0 / k_gj_step), on `stream` (NULL: the default stream); blocks until done.
 * Returns 1 when E is positive definite, 0 when a pivot was not positive (Einv is then meaningless), or a negative
 * code.  If us_per_inverse is non-NULL, the inversion is repeated `reps` times and the mean device time stored. */
int insfm_ba_debug_spd_inverse(int32_t m, const double* E, double* Einv, void* stream, int32_t reps,
                               double* us_per_inverse);

/* ---- global positioning: introspection used by the parity tests ------------------------------------------ */
/* Linearize at DEVICE parameters; then insfm_ba_debug_solve(h, f) solves the damped system and
 * insfm_ba_debug_get gives 0 W as [N,4] records {u, beta^2} (W_o = -beta^2 (I - u u^T), scale-eliminated) 1 V[P,6]
 * (damped) 2 g'_p 5 S 6 b 7 dc[C,3] 8 dp[P,3]. */
int insfm_gp_debug_linearize(insfm_ba* h, const double* positions, const double* points, const double* scales);
/* Scale steps of the last solve in the caller's observation order (HOST out, [N]); returns N. */
int64_t insfm_gp_debug_get_ds(insfm_ba* h, double* host_out);

/* ---- prototype: row-partitioned multi-rank CG (shelved: DESIGN.md section 5) ------------------------------ */
/* Row-partitioned two-level CG across ranks (multi-rank handles with precond 1): each rank applies
 * the reduced camera matrix to its own rows (whole camera clusters) and writes those rows' CG partials straight into
 * every rank's exchange window over peer-to-peer mappings; the recurrence scalars and the coarse correction stay
 * replicated, so the result is bitwise the replicated CG's.  After create (and set_exchange): insfm_ba_cg_window
 * allocates this rank's window and returns its IPC handle (hipIpcMemHandle_t, 64 bytes) in ipc_handle; every rank then
 * passes all ranks' handles (world_size x 64 bytes, in rank order) to insfm_ba_cg_attach before the first step.  Ranks
 * must not destroy their handle while a peer may still write into its window (barrier first).  Replaces the replicated
 * CG of the reference's PCG(tol=1e-5) solve (bundle_adjustment.py:117) on multi-rank runs.
 * insfm_ba_cg_partition: this rank's rows as [begin, end) cluster-ordered positions. */
int insfm_ba_cg_window(insfm_ba* h, void* ipc_handle);
int insfm_ba_cg_attach(insfm_ba* h, const void* handles);
int insfm_ba_cg_partition(const insfm_ba* h, int32_t* rows_begin_end);
/* Collective timing probe of the partitioned CG's exchange: `reps` back-to-back flag exchanges with every peer (the
 * k_xsignal / k_xwait pair each CG iteration pays), average microseconds per exchange into *us. */
int insfm_ba_debug_time_xchg(insfm_ba* h, int32_t reps, double* us);

#ifdef __cplusplus
}
#endif
#endif /* INSFM_BA_DEBUG_H */
