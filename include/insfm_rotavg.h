/*
 * insfm_rotavg.h -- C ABI of rotation averaging, same library and error codes as insfm_ba.h.
 *
 * Replaces the numeric core of RotationEstimator (processors/rotation_averaging.py:41-175 with utils/l1_solver.py:11-43)
 * and the per-pair loop of FilterRotations (processors/relpose_filter.py:5-23).  The spanning-tree initialisation
 * (:16-39) stays on the host (instantsfm_amd/processors/rotation_averaging.py).
 *
 * The reference's matrix A is B (x) I3: B is the signed incidence matrix of the pairs (row k: -1 at pair_i[k], +1 at
 * pair_j[k]) plus one gauge row with a single 1 at the fixed image.  So A^T W A = (B^T W B) (x) I3 and every linear
 * solve is an n x n SPD system with three right-hand sides,
 *     M_aa = sum of the weights of a's pairs + [a == fixed],   M_ab = -w_k for the pair k = {a, b}.
 * M is written densely, inverted explicitly by the blocked float64 Gauss-Jordan chain of the BA's coarse solver, and
 * every solve is a dense n x n by n x 3 product.
 *
 * Limit: n <= INSFM_ROTAVG_MAX_IMAGES (8192).  A call holds three n x n float64 buffers (the two ping-pong copies
 * of the padded M and the inverse): 1.5 GiB at the limit, and the inversion's 2 n^3 flops are repeated by every IRLS
 * iteration.  Above it the sparse factorisation the reference uses is the right tool, and the call returns
 * INSFM_BA_EINVAL.  insfm_rotavg_pair_errors holds no n x n buffer and takes any n below 2^31.
 *
 * Rotation maps (all float64).  Exp: rotation vector v of angle a = |v| -> unit quaternion (s v, cos(a / 2)) with
 * s = sin(a / 2) / a, for a <= 1e-3 the series 1/2 - a^2 / 48 + a^4 / 3840.  Log: the quaternion is negated when its
 * w < 0, a = 2 atan2(|xyz|, w) lies in [0, pi], the vector is (a / |xyz|) xyz, for a <= 1e-3 the series
 * (2 + a^2 / 12 + 7 a^4 / 2880) xyz.  Products are quaternion products.  These agree with scipy's from_rotvec /
 * as_rotvec to 1e-12 away from a = pi.  Within 1e-3 of a = pi the sign of the axis is decided by the rounding of w
 * around 0; it is just as arbitrary in scipy, and v and -v describe rotations that differ by 2 (pi - a).
 *
 * Sums over an image's pairs run in pair order, norms are reduced in a fixed order, there are no floating-point
 * atomics: two calls on the same inputs return the same bytes.
 *
 * Array arguments are DEVICE pointers unless marked host.  Every call waits for its work.  Returns 0, INSFM_BA_EHIP,
 * INSFM_BA_ENOMEM, INSFM_BA_ESOLVER or INSFM_BA_EINVAL.  INSFM_BA_EINVAL -- a negative size, n == 0 with pairs,
 * n > INSFM_ROTAVG_MAX_IMAGES, n_pairs >= 2^30, a missing pointer, an image index outside [0, n), pair_i[k] ==
 * pair_j[k], a pair {a, b} listed twice (in either direction), fixed outside [0, n), non-finite or negative options
 * -- is decided before any output is written.
 *
 * The same prototypes are repeated in insfm_tracks.h, the product header of the match-side entry points.
 */
#ifndef INSFM_ROTAVG_H
#define INSFM_ROTAVG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define INSFM_ROTAVG_MAX_IMAGES 8192

/* info (host, int32) of insfm_rotavg_solve */
#define INSFM_ROTAVG_INFO_LEN 16
#define INSFM_ROTAVG_INFO_L1_ITERS 0   /* L1 outer iterations run */
#define INSFM_ROTAVG_INFO_ADMM 1       /* 1..10: ADMM iterations of the first ten outer iterations */
#define INSFM_ROTAVG_INFO_IRLS_ITERS 11
#define INSFM_ROTAVG_INFO_FAILED 12    /* 0, INSFM_ROTAVG_FAILED_L1 (a NaN step) or INSFM_ROTAVG_FAILED_IRLS (a NaN weight) */
#define INSFM_ROTAVG_FAILED_L1 1
#define INSFM_ROTAVG_FAILED_IRLS 2

/* ROTATION_ESTIMATOR_OPTIONS and L1_SOLVER_OPTIONS.  The ADMM iteration cap is the reference's schedule (10, doubled
 * after every outer iteration, at most 100), not an option (rotation_averaging.py:106, :123). */
typedef struct insfm_rotavg_options {
    int32_t max_num_l1_iterations;   /* 0 skips the L1 phase */
    int32_t max_num_irls_iterations; /* 0 skips the IRLS phase */
    double l1_step_convergence_threshold;
    double irls_step_convergence_threshold;
    double irls_loss_parameter_sigma; /* radians (the reference's option is in degrees) */
    double rho, alpha, absolute_tolerance, relative_tolerance; /* rho > 0 */
} insfm_rotavg_options;

/* RotationEstimator.SolveL1Regression followed by SolveIRLS (rotation_averaging.py:100-161).
 *   n          registered images, dense indices 0 .. n-1
 *   pair_i, pair_j [n_pairs]  dense indices of image_id1 / image_id2 of the valid pairs, in view-graph order
 *   pair_quat  [n_pairs, 4]   the pairs' rotations R_rel (R_2 ~ R_rel R_1), xyzw, normalised here as scipy does
 *   rot        [n, 3]         in: the initial world-to-camera rotation vectors; out: the estimate
 *   fixed, fixed_rot [3]      the gauge: index of the fixed image and the rotation vector it is held at
 *   opt, info  (host)         see above; info has INSFM_ROTAVG_INFO_LEN entries
 * rot is written only when the call returns 0 with info[FAILED] == 0; after a NaN step or weight (return 0,
 * info[FAILED] set, the counts of the iterations begun) and after every error it is as it was.  A non-positive pivot
 * of the inversion (M singular: an image without a path to the fixed one) returns INSFM_BA_ESOLVER.  n_pairs == 0 is
 * legal: with n == 1 only the gauge row acts and the rotation stays where it is. */
int insfm_rotavg_solve(int64_t n, int64_t n_pairs, const int32_t* pair_i, const int32_t* pair_j,
                       const double* pair_quat, double* rot, int64_t fixed, const double* fixed_rot,
                       const insfm_rotavg_options* opt, int32_t* info, void* stream);

/* ComputeResiduals (:84-98): res [n_pairs + 1, 3]; row k = -Log(R_j^T R_rel R_i), the last row the gauge residual
 * Log(Exp(fixed_rot)^T Exp(rot[fixed])). */
int insfm_rotavg_residuals(int64_t n, int64_t n_pairs, const int32_t* pair_i, const int32_t* pair_j,
                           const double* pair_quat, const double* rot, int64_t fixed, const double* fixed_rot,
                           double* res, void* stream);

/* UpdateGlobalRotations (:163-168): rot[a] <- Log(Exp(rot[a]) Exp(-step[a])), rot and step [n, 3]. */
int insfm_rotavg_update(int64_t n, double* rot, const double* step, void* stream);

/* M = B^T W B [n, n] (row-major) for the pair weights `weights` [n_pairs] (NULL: all 1; the gauge row's weight is
 * always 1), and, when `inverse` [n, n] is not NULL, its inverse.  INSFM_BA_ESOLVER when a pivot of the inversion is
 * not positive (M is written, inverse is not meaningful). */
int insfm_rotavg_system(int64_t n, int64_t n_pairs, const int32_t* pair_i, const int32_t* pair_j,
                        const double* weights, int64_t fixed, double* M, double* inverse, void* stream);

/* FilterRotations' angle (relpose_filter.py:13-19): angle_deg[k] = degrees(acos(clip((trace((R_j R_i^T)^T R_rel) - 1)
 * / 2, -1, 1))), with world2cam [n, 9] the images' row-major world-to-camera rotation matrices. */
int insfm_rotavg_pair_errors(int64_t n, int64_t n_pairs, const int32_t* pair_i, const int32_t* pair_j,
                             const double* pair_quat, const double* world2cam, double* angle_deg, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* INSFM_ROTAVG_H */
