/*
 * cdhip.h -- C ABI of the MI355X-native coordinate-descent sweep.
 *
 * This is the drop-in boundary for ONE path of mlakolar/CoordinateDescent.jl
 * v0.3.0: coordinateDescent! -> _coordinateDescent! -> _cdPass! ->
 * descendCoordinate! for CDLeastSquaresLoss / CDSqrtLassoLoss (/ CDWeightedLSLoss)
 * with a ProxL1 penalty, plus the helpers that path calls (initialize!, gradient,
 * _findLambdaMax, _stdX!).  Each entry point names the reference interface it
 * replaces (paths relative to the reference's src/).  The Julia binding a
 * maintainer would add is in INTEGRATION.md and julia/CoordinateDescentHIP.jl.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; every function returns a cdh_status.
 *   - Coordinates cross the ABI 1-based int64 (Julia's Int64), rebased inside.
 *   - Host arrays are borrowed for the duration of the call only.
 *   - X is column-major n x p with leading dimension ld (elements), dtype T;
 *     y, r, w are length-n vectors of T; beta/omega and all scalars are double.
 *   - One process drives one GPU.  With several processes each handle owns the
 *     row shard [row_offset, row_offset + n_local) of an n_total-row problem and
 *     the per-coordinate gradient scalars are summed with an RCCL all-reduce
 *     (cdh_comm_init).  beta, omega and every scalar are replicated.
 *   - A handle is not thread-safe; calls block until results are host-visible.
 *   - Nothing here falls back to a CPU path: without a GPU cdh_create fails
 *     with CDH_HIP_ERROR.
 */
#ifndef CDHIP_H
#define CDHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cdh_handle_s *cdh_handle;

/* Julia exceptions the codes map to: DIM_MISMATCH -> DimensionMismatch
 * (coordinate_descent.jl:13,15; cd_differentiable_function.jl:53,129,212),
 * BAD_ARG -> ArgumentError (lasso.jl:128; the zero-step cold-start range),
 * DOMAIN -> DomainError (sqrt of a negative, cd_differentiable_function.jl:280,282). */
typedef enum cdh_status {
    CDH_OK = 0,
    CDH_DIM_MISMATCH = 1,
    CDH_BAD_ARG = 2,
    CDH_DOMAIN = 3,
    CDH_HIP_ERROR = 4,
    CDH_RCCL_ERROR = 5,
    CDH_OOM = 6
} cdh_status;

typedef enum cdh_dtype { CDH_F64 = 0, CDH_F32 = 1 } cdh_dtype;

/* CDLeastSquaresLoss (cd_differentiable_function.jl:43-111), CDSqrtLassoLoss
 * (:202-291), CDWeightedLSLoss (:118-194). */
typedef enum cdh_loss { CDH_LS = 0, CDH_SQRT = 1, CDH_WLS = 2 } cdh_loss;

/* SmoothingKernel subtypes (varying_coefficient_lasso.jl:3-21), evaluated as the reference writes them -- not the textbook
 * forms: Gaussian K(x, y) = exp(-(x - y)^2 / h) / h; Epanechnikov u = (x - y) / h, K = |u| >= 1 ? 0 : 0.75 (1 - u^2) / h. */
typedef enum cdh_vc_kernel { CDH_VC_GAUSSIAN = 0, CDH_VC_EPANECHNIKOV = 1 } cdh_vc_kernel;

/* How a pass is executed on the device (no reference counterpart).
 *  CDH_SWEEP_COORD : one fused kernel per coordinate visit (apply the previous
 *                    visit's residual update, then the dots of this column),
 *                    one gradient all-reduce per coordinate.
 *  CDH_SWEEP_BLOCK : visits are taken B at a time; one kernel reads the B
 *                    columns once and returns X_B'r and the B x B Gram block, the
 *                    B scalar updates run on those numbers (algebraically the
 *                    same iterates), then one rank-B residual update.  One
 *                    all-reduce per block.  B in {2, 4, 8, 16, 32, 64}; with
 *                    observation weights (CDH_WLS) B >= 16, narrower widths then
 *                    run the per-coordinate sweep.
 * A new handle sweeps in blocks of B = 32, the fastest width on one GPU for long columns (B = 64 for fp64 columns of
 * fewer than 262 144 rows, where a block of visits costs its three launches whatever it reads). */
typedef enum cdh_sweep_mode { CDH_SWEEP_COORD = 0, CDH_SWEEP_BLOCK = 1 } cdh_sweep_mode;

/* CDOptions (utils.jl:7-20), field for field, + the seed of the substitute RNG
 * (the reference's RandomIterator uses Julia's global RNG, atom_iterator.jl:60). */
typedef struct cdh_options {
    int64_t maxIter;   /* 2000 */
    double optTol;     /* 1e-7 */
    int32_t randomize; /* 1    */
    int32_t warmStart; /* 1    */
    int64_t numSteps;  /* 50   */
    uint64_t seed;
} cdh_options;

/* The reference reports nothing (maxIter exhaustion is silent,
 * coordinate_descent.jl:74-91); this is a strict superset. */
typedef struct cdh_stats {
    int64_t passes;
    int64_t full_passes;
    int64_t visits;
    int32_t converged;
    int32_t domain_error;
    double maxH;       /* of the last pass */
    double lambda_max; /* cold start only  */
} cdh_stats;

/* ---- lifetime -------------------------------------------------------------- */
/* Replaces the CDLeastSquaresLoss / CDSqrtLassoLoss / CDWeightedLSLoss outer
 * constructors (cd_differentiable_function.jl:52-55, 211-214, 128-131): allocates
 * X, y, r (and w) on `device`.  Single process: n_local == n_total, row_offset 0. */
int32_t cdh_create(cdh_handle *out, int32_t dtype, int32_t loss, int64_t n_local,
                   int64_t n_total, int64_t row_offset, int64_t p, int32_t device);
int32_t cdh_destroy(cdh_handle h);
const char *cdh_last_error(cdh_handle h); /* h may be NULL: last create error */
int32_t cdh_device_count(int32_t *out);
int32_t cdh_synchronize(cdh_handle h);

/* ---- data ------------------------------------------------------------------ */
/* Upload columns [j0, j0+ncols) (0-based here: a bulk-transfer helper, not a
 * coordinate) of the local row shard from a host column-major block. */
int32_t cdh_set_X_cols(cdh_handle h, int64_t j0, int64_t ncols, const void *host, int64_t ld);
int32_t cdh_get_X_cols(cdh_handle h, int64_t j0, int64_t ncols, void *host, int64_t ld);
/* out_m[k] = X[row0, idx1[k]] of the resident design as doubles, 1 <= m <= 4096 (row0 0-based and local, idx1 1-based as
 * coordinates are): the row wX[i, S] that the prediction of lvocv_locpolyl1 dots with the refit
 * (varying_coefficient_lasso.jl:132).  A row or a coordinate out of range: CDH_BAD_ARG. */
int32_t cdh_get_X_row(cdh_handle h, int64_t row0, int64_t m, const int64_t *idx1, double *out_m);
/* y (and r = copy(y), as the loss constructors do). */
int32_t cdh_set_y(cdh_handle h, const void *host_y);
int32_t cdh_get_y(cdh_handle h, void *host_y);
/* Observation weights of CDWeightedLSLoss. */
int32_t cdh_set_obs_weights(cdh_handle h, const void *host_w);
/* f.w (cd_differentiable_function.jl:118-126) as the handle holds it -- uploaded, or evaluated by cdh_vc_set_point;
 * CDH_BAD_ARG while none are set. */
int32_t cdh_get_obs_weights(cdh_handle h, void *host_w);
/* ---- varying-coefficient mode: locpolyl1 (varying_coefficient_lasso.jl:30-79) ------------------------------------
 * The reference rebuilds, on the host and for every grid point z0, the kernel weights (:63), the expanded design
 * X[i,:] (x) [1, (z_i - z0), ..., (z_i - z0)^degree] (_expand_X!, :550-569) and its weighted column scales (_stdX!,
 * utils.jl:140-151).  Here the base design and z stay in HBM and all three are regenerated on the device.
 *
 * cdh_vc_set_data replaces the allocation of expandX around X and z (:50-54): the handle must be CDH_WLS with
 * p == p_base * (degree + 1) (else CDH_DIM_MISMATCH); degree outside 0 .. 3 is CDH_BAD_ARG.  Base column j (host_X, column-major
 * n x p_base with leading dimension ld, dtype T) goes to column j (degree + 1) of the handle's X, host_z (n values of T) to a
 * buffer the handle owns.  The other columns hold nothing meaningful until the first cdh_vc_set_point.
 *
 * cdh_vc_set_point replaces :63-65 for one z0: w_i = K(z_i, z0) (evaluated in double, rounded once to T), the higher-order
 * columns by the reference's recurrence v = x; v *= (z_i - z0) in T, and out_std[j] = sqrt(sum_i w_i X_ij^2 / n_total) for
 * the p expanded columns (out_std may be NULL).  It leaves the handle as cdh_set_X_cols + cdh_set_obs_weights would:
 * residual, gradient cache and the one-launch solve's Gram matrix are void; the iterate is kept (the reference warm-starts
 * from the previous grid point on purpose, :39-42).  bandwidth <= 0, an unknown kernel, or a call before cdh_vc_set_data:
 * CDH_BAD_ARG.  Sums are taken in a fixed order (bit-identical run to run, and to cdh_col_wrms of the same state).
 *
 * Row-sharded handles (n_local != n_total, or any exchange installed) are refused with CDH_BAD_ARG by both calls: the
 * column sums would have to go through the all-reduce, and nothing tests that yet. */
int32_t cdh_vc_set_data(cdh_handle h, int64_t p_base, int32_t degree, const void *host_X, int64_t ld,
                        const void *host_z);
int32_t cdh_vc_set_point(cdh_handle h, int32_t kernel_kind, double bandwidth, double z0, double *out_std);
/* The leave-one-out point of lvocv_locpolyl1 (varying_coefficient_lasso.jl:82-137), replacing :109-113 and the scores of
 * _findLargestCorrelations(w, X, y, s) (utils.jl:108-124) for observation row0 (0-based: a bulk helper, like j0 above): z0 is
 * the stored z[row0], read on the device; weights, expansion and out_std exactly as cdh_vc_set_point(z0 = z[row0]) gives them,
 * except that w[row0] = 0 (:111) -- so out_std is _stdX! with the left-out weight already zero (:113) -- and
 * out_scores[j] = |sum_i X_ij w_i y_i| for the p expanded columns, accumulated in double in the pass that writes the
 * expansion (degree 0: in the pass that takes the scales).  Either output may be NULL.  Invalidates what cdh_vc_set_point
 * invalidates, keeps the iterate, and refuses the same things with CDH_BAD_ARG; so is row0 outside 0 .. n - 1, and a call
 * before cdh_set_y. */
int32_t cdh_vc_set_point_loo(cdh_handle h, int32_t kernel_kind, double bandwidth, int64_t row0, double *out_std,
                             double *out_scores);
/* The low-dimensional half of local-polynomial regression (locpoly, lvocv_locpoly, getStandardError, getStandardErrorHEW:
 * varying_coefficient_lasso.jl:197-235, 257-317, 348-380) rests on the weighted Gram matrix and right-hand side of the
 * expanded design, _expand_Xt_w_X! (varying_coefficient_lasso.jl:572-620) and _expand_Xt_w_Y! (:622-647).  cdh_vc_gram takes
 * both straight from the base design in one pass over the listed base columns, z and y -- nothing is expanded or written:
 *   out_G[(j,a),(k,b)] = sum_i om_i x_ij x_ik d_i^(a+b),   out_c[(j,a)] = sum_i om_i x_ij y_i d_i^a,   *out_sum_w = sum_i om_i,
 * d_i = z_i - z0 (formed in T, as cdh_vc_set_point forms it), om_i = K(z_i, z0)^wpow (K evaluated in double and rounded once to
 * T, as cdh_vc_set_point's weights) times host_e[i] when host_e is given (n values of T: eps^2 of getStandardErrorHEW, :306),
 * wpow 1 or 2 (:275).  With leave_out_row0 >= 0, z0 is the stored z[leave_out_row0] and that row's om is 0 (the commented-out
 * lvocv_locpoly's formulation, :432-436); -1 for none.  base_idx1 lists mb BASE columns (1-based, any order, repeats allowed),
 * 1 <= mb <= CDH_VC_GRAM_MAX_COLS; out_G is column-major ep x ep, ep = mb (degree + 1), both triangles filled, in the expanded
 * order (j, a) -> j (degree + 1) + a of the listed columns; out_c (ep values) and out_sum_w may be NULL.  Powers, products and
 * sums are taken in double, in a fixed order: results are bit-identical run to run.
 *
 * A read-only query: the handle's residual, gradient cache, weights, expanded columns and iterate are left as they were.
 * CDH_BAD_ARG: a call before cdh_vc_set_data; out_c given before cdh_set_y; mb outside 1 .. 64; a column outside 1 .. p_base;
 * bandwidth <= 0; an unknown kernel; wpow outside {1, 2}; a row outside 0 .. n - 1; a row-sharded handle; NULL out_G or
 * base_idx1. */
#define CDH_VC_GRAM_MAX_COLS 64
int32_t cdh_vc_gram(cdh_handle h, int32_t kernel_kind, double bandwidth, double z0,
                    int64_t leave_out_row0,      /* -1: none; else z0 := stored z[row], om[row] = 0 */
                    int32_t wpow,                /* 1 or 2 */
                    const void *host_e,          /* NULL, or n values of T multiplied into om */
                    int64_t mb, const int64_t *base_idx1,   /* 1-based BASE columns, any order */
                    double *out_G, double *out_c, double *out_sum_w);
/* Many points in one launch.  The reference's grid and leave-one-out loops call the two routines above once per point:
 * locpoly on a grid (varying_coefficient_lasso.jl:217-235), lvocv_locpoly (:348-380) and split_locpoly (:383-409), each over
 * _expand_Xt_w_X! / _expand_Xt_w_Y! (:572-647).  cdh_vc_gram_batch serves m such points with one launch per group of points
 * instead of m round trips.  Point t is exactly
 *   cdh_vc_gram(h, kernel_kind, bandwidth[t], z0[t], leave_out_row0[t], wpow, host_e, mb, base_idx1, ...)
 * -- d_i formed in T, K evaluated in double and rounded once to T, the left-out row moving z0 to the stored z[row], the
 * (j, a) -> j (degree + 1) + a order, both triangles filled, powers, products and sums in double -- and BIT-IDENTICAL to it:
 * every output entry goes through the same additions in the same order (the same deal of row chunks to workgroups, the
 * same slices, the same sums over slices and workgroups), so a point's result does not depend on what else is in the batch,
 * where it stands in it, or how the call is cut into launches.  No atomics; bit-identical run to run.
 * A batch may mix points with and without a left-out row, and bandwidths; the kernel kind, wpow, host_e and the column list
 * are shared.  z0 may be NULL when every point leaves a row out; leave_out_row0 may be NULL when none does, else it holds
 * -1 or a 0-based row per point.  out_G receives m blocks of ep x ep (column-major, point after point), out_c (NULL, or m
 * blocks of ep) and out_sum_w (NULL, or m values) likewise.
 *
 * Two regimes.  Where every workgroup of the single-point launch holds one chunk of 64 rows (n <= 32768, fewer for the
 * largest records) a workgroup stages its rows once and walks a share of the points: the design is read from memory once
 * per workgroup, not once per point.  Otherwise a (workgroup, point) does what cdh_vc_gram's workgroup does and the base
 * columns are re-read per point out of cache.  Scratch of its own (allocated by the first call, all or nothing): 128 MiB
 * of partial records and 32 MiB of summed records on the device, 32 MiB pinned; the call is cut into as many launch groups
 * as that allows.  host_e is uploaded once per call.
 *
 * A read-only query, like cdh_vc_gram.  CDH_BAD_ARG, before anything is launched: whatever cdh_vc_gram refuses, for any
 * point (the message names the point); m outside 1 .. CDH_VC_GRAM_MAX_POINTS; NULL bandwidth, out_G or base_idx1; NULL z0
 * while some point has no left-out row; a non-finite z0 at such a point; a row-sharded handle. */
#define CDH_VC_GRAM_MAX_POINTS 65536
int32_t cdh_vc_gram_batch(cdh_handle h, int32_t kernel_kind, int64_t m,
                          const double *bandwidth,        /* m values, each > 0 */
                          const double *z0,               /* m values; may be NULL when every point leaves a row out */
                          const int64_t *leave_out_row0,  /* NULL: none; else m entries, -1 or a 0-based row */
                          int32_t wpow, const void *host_e,
                          int64_t mb, const int64_t *base_idx1,
                          double *out_G,                  /* m blocks of ep x ep, column-major, point after point */
                          double *out_c,                  /* NULL, or m blocks of ep */
                          double *out_sum_w);             /* NULL, or m values */
/* ---- K-fold cross-validation of a lasso path (no reference counterpart) -----------------------------------------------
 * LassoPath (lasso.jl:229-260) on the training rows of a fold is the weighted loss on all rows with w_i = 1 on the training
 * rows and 0 on the others: with standardizeX the scales are _stdX!(w, X) (utils.jl:140-151; cdh_col_wrms) and lambda is
 * multiplied by sqrt(n_k / n), n_k the training rows; without, the scales are 1 and lambda is multiplied by n_k / n.  The
 * iterates are the same, so a resident X serves every fold, and nothing n-sized moves.
 *
 * cdh_set_folds keeps the fold of every row on the device, a byte each: fold_of_row holds n values in 0 .. K - 1,
 * 2 <= K <= 255 and K <= n, every fold non-empty (CDH_BAD_ARG otherwise; the message names the fold that is empty); out_count
 * (K values, may be NULL) receives the fold sizes.  fold_of_row == NULL with K == 0 drops the folds.  Nothing else on the
 * handle changes; a refused call leaves the folds it had.
 *
 * cdh_set_fold_weights writes the observation weights of fold k on the device: w_i = (fold_i == k ? 0 : 1) in the handle's
 * dtype, k == -1: all ones.  It leaves the handle exactly as cdh_set_obs_weights with those values would (the residual's
 * consistency, the gradient cache and the one-launch solve's Gram matrix are void; cdh_get_obs_weights returns the values).
 * CDH_BAD_ARG: not CDH_WLS; k >= 0 without folds, or k >= K; k < -1.
 *
 * cdh_path_sse evaluates the coefficients of a whole path against the rows in one pass over the listed columns: B is s x m,
 * column-major with leading dimension ldb >= s, row t belonging to coordinate idx1[t] (1-based; a coordinate may repeat, its
 * terms add), and
 *   out_held[j]  = sum over rows i with fold_i == k of (y_i - sum_t X[i, idx1[t]] B[t, j])^2,
 *   out_train[j] = the same sum over the other rows.
 * k == -1 counts every row as training (out_held is all zero; folds need not be set).  1 <= s <= 4096, 1 <= m <= 1024, y set;
 * either out pointer may be NULL, not both.  Storage values are converted to double and every product and sum is taken in
 * double, in a fixed order: bit-identical run to run.  A function of X, y and the fold ids only -- any loss kind, either
 * storage type -- and read-only: r does not catch up, and beta, the penalty, the weights, the residual's state, the gradient
 * cache and the one-launch solve's Gram matrix are left as they are.  Scratch of its own, allocated by the first call.
 *
 * All three refuse row-sharded handles (n_local != n_total, or any exchange installed) with CDH_BAD_ARG. */
int32_t cdh_set_folds(cdh_handle h, const int32_t *fold_of_row, int32_t K, int64_t *out_count);
int32_t cdh_set_fold_weights(cdh_handle h, int32_t k);
int32_t cdh_path_sse(cdh_handle h, int32_t k, int64_t s, const int64_t *idx1, int64_t m, const double *B, int64_t ldb,
                     double *out_held, double *out_train);
/* ---- l1-penalised logistic regression by IRLS (no reference counterpart) ----------------------------------------------
 * F(beta) = (1/n) sum_i [log(1 + e^eta_i) - y_i eta_i] + lambda0 sum_j omega_j |beta_j|, eta = X beta, labels y_i in [0, 1].
 * One round of IRLS solves the weighted lasso sum_i w_i (z_i - x_i'beta)^2 / (2n) + lambda0 sum_j omega_j |beta_j| -- the
 * loss of CDWeightedLSLoss (cd_differentiable_function.jl:118-194), so the solver and the resident X are unchanged -- and the
 * step between two rounds forms w, z and the residual z - X beta from the current linear predictor.  That step is
 * cdh_glm_irls: one elementwise pass on the device where the exports below would move three n-sized vectors across the host.
 * Per row, every quantity in double: eta = y_w - r (y_w the working response the handle holds, r the residual it stands
 * for), a = |eta|, e = exp(-a); p = 1/(1+e) if eta >= 0, else e/(1+e), and q = 1 - p taken from the other branch;
 * w = max(e/(1+e)^2, wmin); d = y q - (1-y) p; r_new = d / w; z = eta + r_new; nll = max(eta, 0) + log1p(e) - y eta.
 * Only w is clamped, so the fixed point's KKT conditions are those of F: X_j'W r = X_j'(y - p) whatever W is.
 *
 * cdh_glm_set_labels (stands in for cdh_set_y: the labels are kept beside y, which becomes the working response) stores n
 * doubles in a buffer the handle owns (allocated all-or-nothing) and zeroes the working response: the handle is left
 * exactly as cdh_set_y of n zeros would leave it.  family 0 = binomial.  CDH_BAD_ARG, the handle unchanged: another family;
 * not CDH_WLS; not CDH_F64 (eta = y_w - r in fp32 loses eta once |z| grows); row-sharded (n_local != n_total, or any
 * exchange installed); a label that is not finite or outside [0, 1] (the message names the row).  cdh_glm_get_labels copies
 * the labels back.
 *
 * cdh_glm_irls (stands in for cdh_get_residual, w and z formed on the host, cdh_set_y, cdh_set_obs_weights and
 * cdh_initialize) needs labels, CDH_WLS, fp64, apply in {0, 1} and 0 < wmin <= 0.25.  out3 = {sum_i nll_i, sum_i w_i,
 * number of rows whose weight was clamped} at the iterate the handle holds, summed in a fixed order: bit-identical run to
 * run.  Before the pass r catches up with what it owes, as for every reader of r (cdh_loadings); a residual that is not
 * the iterate's (after cdh_set_iterate, cdh_set_y, cdh_glm_set_labels, ...) is rebuilt as cdh_initialize would.
 *   apply = 0 reads only: beta, the penalty, the weights, y, r's state, the gradient cache and the one-launch solve's Gram
 *     data are left as they are.
 *   apply = 1 writes w to the observation weights, z to y and r_new to r, rows n .. ld - 1 as zeros, and leaves the handle
 *     as cdh_set_y(z), cdh_set_obs_weights(w) and cdh_initialize(beta) would: the gradient cache, the stashed dots, y'y
 *     and the one-launch solve's Gram matrix and X'Wy are void, cdh_get_obs_weights returns w; r is the iterate's residual
 *     (a warm start with cdh_set_reuse_residual may keep it) but not the bits cdh_initialize writes, so a later
 *     cdh_initialize is executed, not skipped. */
int32_t cdh_glm_set_labels(cdh_handle h, int32_t family, const void *host_labels);
int32_t cdh_glm_get_labels(cdh_handle h, void *host_labels);
int32_t cdh_glm_irls(cdh_handle h, int32_t apply, double wmin, double *out3);
/* cdh_glm_irls_fold: the step of cdh_glm_irls inside fold k of a cross-validated logistic path (no reference counterpart; it
 * joins the two sections above: a round's solve is the weighted lasso of CDWeightedLSLoss, cd_differentiable_function.jl:118-194,
 * and the path over the training rows is LassoPath's loop, lasso.jl:229-260, on 0/1 observation weights).  cdh_glm_irls
 * writes the weight of every row, so the first round of a fold would turn its held-out rows into training rows again; here
 * the fold ids of cdh_set_folds decide per row, in the same single pass:
 *   a training row (fold_i != k) is cdh_glm_irls' row: w (clamped below at wmin), z and r_new;
 *   a held-out row (fold_i == k) gets w = 0 exactly (never clamped), z = eta and r = 0, so that its row of X enters no
 *     gradient and eta = y_w - r stays what the next step reads after the solver's updates of r;
 *   rows n .. ld - 1 are written as zeros.
 * out5 = {sum of nll_i over the training rows, sum of w_i, training rows whose weight was clamped, sum of nll_i over the
 * held-out rows, sum over the held-out rows of y_i [eta_i <= 0] + (1 - y_i) [eta_i > 0]} at the iterate the handle holds --
 * the last is the number of misclassified held-out rows for 0/1 labels, eta = 0 predicting class 0 (glmnet's type.measure =
 * "class") -- each summed in a fixed order: bit-identical run to run.  With standardised penalty scales omega = _stdX!(w, X)
 * (utils.jl:140-151) of the 0/1 weights and lambda sqrt(n_k / n), the rounds are those of the logistic lasso on the n_k
 * training rows alone.
 * k == -1: no row is held out, folds need not be set, and w, z, r and out5[0..2] are cdh_glm_irls' bit for bit;
 * out5[3] = out5[4] = 0.  The catch-up of r before the pass, apply = 0 (read-only) and the state apply = 1 leaves are
 * cdh_glm_irls'; cdh_get_obs_weights returns the written weights, zeros included.  CDH_BAD_ARG, the handle unchanged:
 * everything cdh_glm_irls refuses; k < -1; k >= 0 without folds; k >= K. */
int32_t cdh_glm_irls_fold(cdh_handle h, int32_t k, int32_t apply, double wmin, double *out5);
/* ---- l1-penalised Poisson regression with an offset, by the same IRLS loop (no reference counterpart: a round's solve is
 * the weighted lasso of CDWeightedLSLoss, cd_differentiable_function.jl:118-194) ------------------------------------------
 * F(beta) = (1/n) sum_i [mu_i - y_i eta_i] + lambda0 sum_j omega_j |beta_j|, eta = X beta + o, mu = exp(eta), counts
 * y_i >= 0 and offsets o_i (log exposure).  The handle's working response y_w and residual r stand for eta_lin = y_w - r =
 * X beta WITHOUT the offset, so that every other reader of y_w and r sees the linear predictor of the columns.  Per row, in
 * double, each operation rounded on its own: eta = eta_lin + o; capped = eta > eta_max, ec = min(eta, eta_max); mu = exp(ec);
 * clamped = mu < wmin, w = max(mu, wmin); d = y - mu; r_new = d / w; z_lin = eta_lin + r_new; nll = mu - y ec;
 * dev = 2 ((y > 0 ? y log(y / mu) : 0) - (y - mu)).  Only w is clamped, so X'W r = X'(y - mu) and the fixed point keeps the
 * KKT conditions of F. */
/* cdh_glm_set_counts (no reference counterpart; the loss is that of cd_differentiable_function.jl:118-194 per round) stands
 * in for cdh_set_y: it stores n counts where cdh_glm_set_labels stores labels (cdh_glm_get_labels returns them) and, when
 * host_offset is not NULL, n offsets in a buffer of ld doubles the handle owns (pads zero; both buffers allocated
 * all-or-nothing before the handle changes), makes the handle a Poisson handle and leaves it exactly as cdh_set_y of n zeros
 * would.  CDH_BAD_ARG, the handle unchanged: what cdh_glm_set_labels refuses of the handle (not CDH_WLS, not CDH_F64,
 * row-sharded); a count that is negative or not finite, an offset that is not finite (the message names the row).  Counts
 * need not be integers.  cdh_glm_irls and cdh_glm_irls_fold refuse a Poisson handle; a later cdh_glm_set_labels(h, 0, ...)
 * makes it binomial again and drops the offset. */
int32_t cdh_glm_set_counts(cdh_handle h, const void *host_counts, const void *host_offset_or_null);
/* cdh_glm_get_offset (no reference counterpart; see cdh_glm_set_counts, cd_differentiable_function.jl:118-194): the n
 * offsets of a Poisson handle, or of a Cox handle (cdh_glm_set_survival), zeros when none was given.  CDH_BAD_ARG on a handle
 * that holds neither counts nor survival data -- a binomial handle included; the message names cdh_glm_set_counts either way. */
int32_t cdh_glm_get_offset(cdh_handle h, void *host_offset);
/* cdh_glm_poisson_irls (no reference counterpart; a round's solve is the weighted lasso of CDWeightedLSLoss,
 * cd_differentiable_function.jl:118-194): the step between two rounds at the iterate the handle holds, in one pass.
 *   a training row becomes (w, y_w, r) = (w, z_lin, r_new);
 *   a held-out row (fold id == k, after cdh_set_folds) becomes (0, eta_lin, 0): weight exactly 0, never clamped up;
 *   rows n .. ld - 1 are written as zeros.
 * k == -1: no row is held out and the fold ids are not read.  out6 = {sum of nll_i over the training rows, sum of w_i,
 * training rows clamped at wmin, live rows capped at eta_max, sum of dev_i over the held-out rows, sum of dev_i over the
 * training rows}, each summed in a fixed order: bit-identical run to run.  The catch-up of r before the pass, apply = 0
 * (read-only) and the state apply = 1 leaves are cdh_glm_irls'.  CDH_BAD_ARG, the handle unchanged: no counts set (a binomial
 * handle included); apply not in {0, 1}; wmin not finite or not > 0; eta_max outside (0, 700]; k < -1; k >= 0 without folds;
 * k >= K; out6 NULL. */
int32_t cdh_glm_poisson_irls(cdh_handle h, int32_t k, int32_t apply, double wmin, double eta_max, double *out6);
/* ---- observation weights of the binomial and the Poisson family (glmnet's weights =; no reference counterpart: a round's
 * solve is the weighted lasso of CDWeightedLSLoss, cd_differentiable_function.jl:118-194) ---------------------------------
 * F(beta) = (1/n) sum_i v_i nll_i + lambda0 sum_j omega_j |beta_j|, nll_i the family's own and v_i finite and > 0.  A
 * training row's step is the unweighted one -- r_new and z are its bits -- and the stored working weight is
 * w_i = v_i w_i^fam, w_i^fam the family's weight already clamped at wmin, one rounded multiplication: X'W r =
 * X'(v (y - mu)) whatever the clamp did.  Held-out rows stay (0, eta_lin, 0), rows n .. ld - 1 zeros.  The records keep
 * their layouts: the nll, sum w, the held-out nll and both deviances become sums weighted by v (sum v_i nll_i, sum w_i,
 * ...), the held-out misclassification sum v_i miss_i; the clamped and capped rows stay counts.  The three step exports
 * run the weighted instantiation while the handle holds weights; their signatures and what they refuse do not change, and
 * cdh_glm_irls returns the first three sums of the fold-aware weighted step at k = -1. */
/* cdh_glm_set_weights (no reference counterpart; see above, cd_differentiable_function.jl:118-194) stands in for the v in
 * cdh_set_obs_weights(v w), composed on the host every round: it stores n weights AS GIVEN (the library does not normalise
 * them; the front ends pass weights that sum to n) in a buffer of ld doubles the handle owns (pads zero, allocated
 * all-or-nothing before the handle changes).  NULL drops the weights: the steps are the unweighted ones again, bit for bit.
 * It voids what cdh_set_obs_weights voids and leaves y, r and beta alone.  CDH_BAD_ARG, the handle unchanged: what
 * cdh_glm_set_labels refuses of the handle; a handle without labels or counts; a Cox handle (its weights come through
 * cdh_glm_set_survival_strata); a weight that is not finite or not > 0 (the message names the row).  cdh_glm_set_labels,
 * cdh_glm_set_counts and the three cdh_glm_set_survival* drop the weights. */
int32_t cdh_glm_set_weights(cdh_handle h, const void *host_weights_or_null);
/* cdh_glm_get_weights (no reference counterpart; see cdh_glm_set_weights, cd_differentiable_function.jl:118-194): the n
 * weights the handle holds, ones when none are set.  CDH_BAD_ARG: host_weights NULL; a handle without labels or counts; a
 * Cox handle (cdh_glm_get_survival_strata returns its weights). */
int32_t cdh_glm_get_weights(cdh_handle h, void *host_weights);
/* ---- l1-penalised Cox regression (Breslow ties, as glmnet's family = "cox"), by the same IRLS loop (no reference
 * counterpart: a round's solve is the weighted lasso of CDWeightedLSLoss, cd_differentiable_function.jl:118-194) -----------
 * Rows have a time t_i, a status delta_i (1: event, 0: censored) and optionally an offset o_i.  With eta = X beta + o and
 * e_i = exp(min(eta_i, eta_max)):  S_i = sum of e_j over t_j >= t_i (the risk set; the same for every row of a tie group),
 * A_i = sum of delta_k / S_k and B_i = sum of delta_k / S_k^2 over t_k <= t_i.
 * F(beta) = -(1/n) sum_i delta_i (eta_i - log S_i) + lambda0 sum_j omega_j |beta_j|; there is no intercept (it cancels).
 * Per row, in double, each operation rounded on its own: eA = e A; w_raw = eA - e (e B); clamped = w_raw < wmin,
 * w = max(w_raw, wmin); d = delta - eA; r_new = d / w; z_lin = eta_lin + r_new (eta_lin = y_w - r = X beta WITHOUT the offset, as
 * for the Poisson family).  Only w is clamped, so X'W r = X'(delta - eA), the negative gradient of the partial likelihood.
 * S, A and B come from a segmented suffix scan and two segmented prefix scans in time order, a chain of launches on the
 * handle's stream in which every sum has a fixed order.
 * With strata and observation weights (cdh_glm_set_survival_strata): each row has a weight v_i > 0 and a stratum id g_i;
 * ev = v e and dv = v delta take the places of e and delta, S_i runs over the rows of g_i with t_j >= t_i, A_i and B_i over the
 * rows of g_i with t_k <= t_i: ev = v e; evA = ev A; w_raw = evA - ev (ev B); d = dv - evA; the nll term is dv (log S - eta).
 * The rows are ordered by (stratum, time) and the three scans restart at every stratum's boundary (segmented scans, the
 * rounding error of a sum relative to its own stratum's sum).  The diagonal is v e A - (v e)^2 B: an integer weight
 * reproduces a replicated row's gradient and nll, not its diagonal.
 * With start-stop times (cdh_glm_set_survival_interval; glmnet's Surv(start, stop, status)): row i is at risk at t iff
 * start_i < t <= stop_i, inside its stratum.  S(t) = sum of ev_j over stop_j >= t LESS the sum over start_j >= t -- a second
 * order by (stratum, start) with a second segmented suffix scan, read through a static lookup; A_i = P(stop_i) - P(start_i) with
 * P(u) the sum of dv / S(t) over the event times t <= u, B_i the same with dv / S^2 -- the prefix scans read at two positions.
 * The subtractions are inherent (glmnet and survival::coxph subtract too): the error of S is relative to the two sums of its
 * stratum, about n U (T + T2), not to S, and that of A and B to P(stop) + P(start); nothing crosses a stratum's boundary.  An
 * event whose computed S is not > 0 is skipped, a w_raw driven negative is clamped at wmin.  Efron ties are offered for right-censored data; not yet with
 * start-stop times (cdh_glm_set_cox_ties). */
/* cdh_glm_set_survival (no reference counterpart; the loss is that of cd_differentiable_function.jl:118-194 per round)
 * stands in for cdh_set_y: it stores n statuses where cdh_glm_set_labels stores labels, n offsets (when not NULL) where
 * cdh_glm_set_counts stores them, sorts the times on the host (stable, ascending) and keeps the order, the tie groups' bounds,
 * the scans' scratch and the times in one group of buffers, allocated all-or-nothing before the handle changes; the design
 * and the handle's vectors stay in the caller's row order.  Makes the handle a Cox handle and leaves it exactly as cdh_set_y
 * of n zeros would.  CDH_BAD_ARG, the handle unchanged: what cdh_glm_set_labels refuses of the handle; a NULL time or
 * status; a time or an offset that is not finite, a status other than 0 or 1 (the message names the row); no event at all.
 * cdh_glm_irls, cdh_glm_irls_fold and cdh_glm_poisson_irls refuse a Cox handle; a later cdh_glm_set_labels or
 * cdh_glm_set_counts makes it binomial or Poisson again.  cdh_glm_get_offset serves a Cox handle too. */
int32_t cdh_glm_set_survival(cdh_handle h, const void *host_time, const void *host_status, const void *host_offset_or_null);
/* cdh_glm_get_survival (no reference counterpart; see cdh_glm_set_survival, cd_differentiable_function.jl:118-194): the n
 * times and the n statuses of a Cox handle, in the caller's row order; a NULL output is skipped.  CDH_BAD_ARG: both NULL; no
 * survival data set. */
int32_t cdh_glm_get_survival(cdh_handle h, void *host_time, void *host_status);
/* cdh_glm_set_survival_strata (no reference counterpart; see cdh_glm_set_survival, cd_differentiable_function.jl:118-194):
 * cdh_glm_set_survival with n int32 stratum ids and n weights, either of which may be NULL (one stratum; unit weights).
 * With both NULL it IS cdh_glm_set_survival, call for call and bit for bit (on a handle set to Efron ties, cdh_glm_set_cox_ties,
 * either call stores one stratum and unit weights: the Efron chain is segmented and weighted).  Otherwise the order is a stable ascending sort
 * by (stratum id, time) -- every int32 is a valid id -- and the bounds of every position's stratum, the ids and the weights
 * live in a second group of buffers, allocated all-or-nothing with the rest before the handle changes.  The weights are stored
 * as given: the library does not normalise them.  CDH_BAD_ARG, the handle unchanged: what cdh_glm_set_survival refuses; a
 * weight that is not finite or not > 0 (the message names the row).  cdh_glm_set_survival, cdh_glm_set_labels and
 * cdh_glm_set_counts drop the strata and the weights. */
int32_t cdh_glm_set_survival_strata(cdh_handle h, const void *host_time, const void *host_status,
                                    const void *host_offset_or_null, const int32_t *host_strata_or_null,
                                    const void *host_weights_or_null);
/* cdh_glm_set_survival_interval (no reference counterpart; see cdh_glm_set_survival, cd_differentiable_function.jl:118-194):
 * cdh_glm_set_survival_strata with n start times: row i is at risk over (start_i, stop_i].  With host_start NULL it IS
 * cdh_glm_set_survival_strata, call for call and bit for bit.  Otherwise the handle always runs the segmented and weighted
 * arithmetic (absent strata and weights are stored as one stratum and unit weights), and the start order -- a stable ascending
 * sort by (stratum id, start) -- the two lookups, the second scan's scratch and the starts live in a third group of buffers,
 * allocated all-or-nothing with the rest before the handle changes.  A row whose start equals an event time is not at risk
 * at it; a row whose stop equals it is.  CDH_BAD_ARG, the handle unchanged: what cdh_glm_set_survival_strata refuses (of the
 * stop times what it refuses of the times); a start that is not finite; start >= stop (the message names the row).
 * cdh_glm_set_survival, cdh_glm_set_survival_strata, cdh_glm_set_labels and cdh_glm_set_counts drop the start times. */
int32_t cdh_glm_set_survival_interval(cdh_handle h, const void *host_start_or_null, const void *host_stop,
                                      const void *host_status, const void *host_offset_or_null,
                                      const int32_t *host_strata_or_null, const void *host_weights_or_null);
/* cdh_glm_get_survival_start (no reference counterpart; see cdh_glm_set_survival_interval,
 * cd_differentiable_function.jl:118-194): the n start times of a Cox handle, in the caller's row order; the stop times are
 * cdh_glm_get_survival's "time".  CDH_BAD_ARG: host_start NULL; the handle holds no start times. */
int32_t cdh_glm_get_survival_start(cdh_handle h, void *host_start);
/* cdh_glm_get_survival_strata (no reference counterpart; see cdh_glm_set_survival_strata,
 * cd_differentiable_function.jl:118-194): the n stratum ids and the n weights of a Cox handle, in the caller's row order --
 * zeros where it holds no strata, ones where it holds no weights; a NULL output is skipped.  CDH_BAD_ARG: both NULL; no
 * survival data set. */
int32_t cdh_glm_get_survival_strata(cdh_handle h, int32_t *host_strata, void *host_weights);
/* cdh_glm_cox_irls (no reference counterpart; a round's solve is the weighted lasso of CDWeightedLSLoss,
 * cd_differentiable_function.jl:118-194): the step between two rounds at the iterate the handle holds.
 *   a training row becomes (w, y_w, r) = (w, z_lin, r_new); a row before the first event has w = wmin and r_new = 0 exactly;
 *   a held-out row (fold id == k, after cdh_set_folds) leaves the risk sets and the event sums and becomes (0, eta_lin, 0);
 *   rows n .. ld - 1 are written as zeros.
 * k == -1: no row is held out and the fold ids are not read (the same bits whether or not folds are set).  out5 = {sum of
 * delta_i (log S_i - eta_i) over the training rows, sum of w_i, training rows clamped at wmin, live rows capped at eta_max,
 * sum of dv_i = v_i delta_i over the training rows: the events among them, bit for bit, on a handle without weights}, each
 * summed in a fixed order: bit-identical run to run; on a handle with strata and weights the first sum is that of
 * dv_i (log S_i - eta_i).  The catch-up of r before the
 * step, apply = 0 (read-only) and the state apply = 1 leaves are cdh_glm_irls'.  CDH_BAD_ARG, the handle unchanged: no
 * survival data set; apply not in {0, 1}; wmin not finite or not > 0; eta_max outside (0, 700]; k < -1; k >= 0 without
 * folds; k >= K; out5 NULL. */
int32_t cdh_glm_cox_irls(cdh_handle h, int32_t k, int32_t apply, double wmin, double eta_max, double *out5);
/* cdh_glm_set_cox_ties (no reference counterpart; the tie rule of the Cox steps' sums, a round's solve stays the weighted lasso
 * of cd_differentiable_function.jl:118-194): ties = 0 Breslow (the default of every fresh set of survival data), 1 Efron, the
 * default of survival::coxph.  Among the TRAINING rows of a tie group g (one stratum, one time) let d be the number of events,
 * D = sum of ev and m = (sum of dv) / d over them, S the risk-set sum; for l = 0 .. d - 1, den_l = S - (l / d) D.  Then
 * n nll = sum_g [m sum_l log den_l - sum over the events of g of dv eta], A_i = sum over the groups at or before i's of
 * m sum_l c / den_l and B_i the same with c^2 / den_l^2, where c = 1 - l / d if i is an event of g itself and 1 otherwise;
 * the rest of the step is cdh_glm_cox_irls' (d = dv - ev A, w_raw = ev A - ev^2 B, the clamp, z, r, the five-slot record).
 * The weights follow survival::coxph's convention: every event of a group enters with the group's MEAN event weight m.
 * d = 1 is Breslow; a group whose events are all held out adds nothing; an event whose den is not > 0 is skipped.  The sums
 * over a group are scans that restart at the group's bounds: constant work per row whatever the groups' sizes, no atomics,
 * bit-identical run to run.  An Efron handle always runs the segmented, weighted arithmetic (absent strata and weights are
 * stored as one stratum and unit weights) and holds a group of scratch buffers of its own, allocated all-or-nothing before
 * the handle changes; a handle that never asks for Efron allocates nothing.  With Breslow set, cdh_glm_cox_irls is what it
 * was, launch for launch and bit for bit.  cdh_glm_set_survival and cdh_glm_set_survival_strata keep the rule, and so does
 * cdh_glm_set_survival_interval without start times; WITH start times it puts the handle back to Breslow (Efron with
 * start-stop times is not offered yet); cdh_glm_set_labels and cdh_glm_set_counts drop it with the rest of the Cox state.  The
 * handle's y, w and r are not touched.  CDH_BAD_ARG, the handle unchanged: no survival data set; ties not 0 or 1; Efron on a
 * handle with start times (the message says so). */
int32_t cdh_glm_set_cox_ties(cdh_handle h, int32_t ties);
/* cdh_glm_get_cox_ties (no reference counterpart; see cdh_glm_set_cox_ties, cd_differentiable_function.jl:118-194): the
 * handle's rule, 0 Breslow or 1 Efron.  CDH_BAD_ARG: ties NULL; no survival data set. */
int32_t cdh_glm_get_cox_ties(cdh_handle h, int32_t *ties);
/* cdh_glm_cox_residuals (no reference counterpart; the model is the one whose rounds solve the weighted lasso of
 * cd_differentiable_function.jl:118-194): per row, in the caller's row order, at the iterate the handle holds and with no row
 * held out (fold ids are not read).  eta = X beta + offset capped at eta_max as in cdh_glm_cox_irls, e = exp(eta) WITHOUT
 * the weight, delta the status.
 *   cumhaz_i     = A_i, the baseline cumulative hazard accrued over the row's time at risk.  Breslow: the stratum's
 *                  cumulative hazard at the row's time, less that at its start on a handle with start times.  Efron: the
 *                  same for a row that is not an event; an event's own group enters with c = 1 - l / d.  It is the A the
 *                  handle's own step forms for the row, read from the step's scans at the positions where
 *                  cdh_glm_cox_baseline reads them.  So a row's cumhaz == the table's cumhaz at the last event time <= its
 *                  time (0 if there is none), and with start times == the one rounded difference of two such entries.
 *                  Where the row's own tie group holds an event, that position is the step's own and cumhaz is the step's
 *                  A bit for bit.  In an event-free group the step reads its scan further on, past zeros only, and may
 *                  differ from cumhaz in the last bits (the same sum along another association);
 *   martingale_i = delta_i - e_i A_i   (survival's residuals(coxph, "martingale"); v_i times it is the step's d_i);
 *   deviance_i   = sign(M_i) sqrt(-2 (M_i + delta_i log(e_i A_i))), the delta log term 0 where delta = 0; a radicand that rounds
 *                  below 0 (e A within rounding of 1) is taken as 0; an event with e A = 0 gives +inf.
 * A NULL output is skipped; each of the others receives n doubles.  The call runs the read-only step of cdh_glm_cox_irls
 * (k = -1, apply = 0, its catch-up of r included), then the table's launches of cdh_glm_cox_baseline, then one kernel over
 * the scratch.  y, w, r and beta are not touched; the results are bit-identical run to run.  The first call allocates a group of scratch buffers of its own, all-or-nothing
 * before anything else; a handle that never asks allocates nothing.  CDH_BAD_ARG, the handle unchanged: no survival data set;
 * eta_max outside (0, 700]; all three outputs NULL. */
int32_t cdh_glm_cox_residuals(cdh_handle h, double eta_max, void *host_cumhaz_or_null,
                              void *host_martingale_or_null, void *host_deviance_or_null);
/* cdh_glm_cox_baseline (no reference counterpart; R's basehaz and glmnet's survfit.coxnet at x = 0, offset 0 -- uncentred; the
 * model is the one whose rounds solve the weighted lasso of cd_differentiable_function.jl:118-194): one table row per tie
 * group (one stratum, one time) that holds at least one event, in (stratum id, time) ascending order, evaluated as
 * cdh_glm_cox_residuals evaluates.  Columns: stratum (int32 id; 0 without strata), time, n_event (sum of dv = v delta over
 * the group), risk_sum (S of the group: the sum of v e over the rows at risk), cumhaz (the stratum's cumulative baseline
 * hazard H0 at that time, the group included; under Efron with sum_l m / den_l) and cumvar (the same sum of h / S, B of the
 * step).  A group whose events were all skipped (S or den not > 0) still has a row.  *count is always written; the columns
 * are written, count entries each, only when count <= capacity (count never exceeds the number of events); a NULL column is
 * skipped.  The groups are compacted on the device by scans in a fixed order: the table is bit-identical run to run; y, w, r
 * and beta are not touched.  CDH_BAD_ARG, the handle unchanged: no survival data set; eta_max outside (0, 700]; count NULL;
 * capacity negative; count > capacity (the message names both numbers). */
int32_t cdh_glm_cox_baseline(cdh_handle h, double eta_max, int64_t capacity, int32_t *host_stratum,
                             void *host_time, void *host_n_event, void *host_risk_sum,
                             void *host_cumhaz, void *host_cumvar, int64_t *count);
/* cdh_glm_cox_concordance (no reference counterpart; R's survival::concordance and glmnet's Cindex -- Harrell's C; the model
 * is the one whose rounds solve the weighted lasso of cd_differentiable_function.jl:118-194): the weighted numbers of
 * concordant, discordant and tied pairs at the iterate the handle holds.  k == -1: all rows take part and the fold ids are
 * not read; k >= 0: the rows with fold id == k, the held-out rows, after cdh_set_folds.  Rows i != j that take part, in the
 * same stratum, are a comparable pair with i the earlier iff i is an event and t_j > t_i, or t_j == t_i and j is censored (a
 * row censored at an event's time outlived it; two events at one time are not comparable).  eta = X beta + offset, formed as
 * cdh_glm_cox_residuals forms it but NOT capped: only its order matters.  The pair is concordant if eta_i > eta_j, discordant
 * if eta_i < eta_j, tied if eta_i == eta_j (doubles: -0.0 == 0.0), and counts with weight v_i v_j (1 without weights).
 * out4 = {concordant, discordant, tied, number of rows taking part whose eta is NaN}; C = (concordant + tied / 2) /
 * (concordant + discordant + tied).  When out4[3] > 0 the first three are unspecified.  On a handle without weights the first
 * three are exact integers while their sum is below 2^53.  The tie rule does not enter.  Read-only: r first catches up as for
 * cdh_glm_cox_irls; y, w, r, beta and the step's scratch stay as they are; the results are bit-identical run to run.  The first
 * call after a setter of survival data allocates a group of scratch buffers of its own (9 doubles and 3 int32 per row,
 * rounded up to tiles of 1024 rows), all-or-nothing, and derives its order; the survival setters drop it.  CDH_BAD_ARG, the
 * handle unchanged: row shards and whatever else the GLM exports refuse of the handle; no survival data set; k < -1, k >= 0
 * without folds, k >= K; out4 NULL; a handle with start times ("concordance with start-stop times is not offered yet"). */
int32_t cdh_glm_cox_concordance(cdh_handle h, int32_t k, double *out4);
/* cdh_glm_cox_score (no reference counterpart; R's residuals(coxph, "score") and "schoenfeld" and the inverse of coxph's
 * var -- the model is the one whose rounds solve the weighted lasso of cd_differentiable_function.jl:118-194): what standard
 * errors, robust variances and a check of proportional hazards are made of, for m <= 64 columns idx1 (1-based like cdh_gram;
 * duplicates allowed: equal columns give equal bits) of the resident design, at the iterate the handle holds, Breslow ties, no
 * row held out.  With e, ev = v e, dv = v delta, S, h and A as cdh_glm_cox_residuals forms them, xt_c = x_c - centre_c,
 * N_c the stratum's suffix scan of ev xt_c, xbar_c = N_c / S at the tie group's first position (the risk-set mean) and Q_c
 * the stratum's prefix scan of h xbar_c read at the group's last position:
 *   schoenfeld[i, c] = xt_ic - xbar_c    at an event that counts (S > 0), exactly 0 on every other row
 *   score[i, c]      = delta_i schoenfeld[i, c] - e_i (xt_ic A_i - Q_ic)      R's unweighted score residual; v_i times it is
 *                      the weighted one, and its column sums over v are the gradient X_c'(dv - ev A)
 *   info[c, d]       = sum_i ev_i A_i xt_ic xt_id - sum over the events that count of dv xbar_c xbar_d
 *                      the Hessian of the un-normalised negative log partial likelihood in beta_idx; symmetric by construction
 * The centres are the columns' unweighted means over the rows, formed on the device in a fixed order, unless
 * host_centre_or_null gives m of them; host_centre_out_or_null receives the m used.  No output depends on the centres in exact
 * arithmetic, but info, a difference of two positive semidefinite sums, loses digits without centring.  Each residual output
 * is n x m doubles, column-major with leading dimension n, in the caller's row order; host_info is m x m.  A NULL output is
 * skipped.  The call runs the read-only step of cdh_glm_cox_irls (k = -1, apply = 0, its catch-up of r included), then a
 * fixed number of launches whatever m is: one gather of X per (row, column) through the time order, one segmented suffix scan
 * and one segmented prefix scan per column, the rows, and the matrix in pair tiles of columns with per-run partials added in
 * run order.  No atomics: every output is bit-identical run to run, and a column's residuals are the same bits whether it is
 * asked for alone or in any list.  y, w, r and beta are not touched.  The first call allocates a group of scratch buffers of its
 * own, all-or-nothing ((5 + 5 m) doubles per row and the partials of the matrix); a later call with a larger m regrows it,
 * all-or-nothing; a handle that never asks allocates nothing.  CDH_BAD_ARG, the handle unchanged: no survival data set;
 * eta_max outside (0, 700]; m < 1 or m > 64; idx1 NULL or an index outside 1 .. p; all three outputs NULL; a centre that is
 * not finite; a handle with start times ("cdh_glm_cox_score is not offered with start-stop times yet"); a handle set to Efron
 * ties ("cdh_glm_cox_score is not offered with Efron ties yet" -- a handle put back to Breslow is served). */
int32_t cdh_glm_cox_score(cdh_handle h, double eta_max, int64_t m, const int64_t *idx1,
                          const double *host_centre_or_null, double *host_centre_out_or_null,
                          void *host_schoenfeld_or_null, void *host_score_or_null,
                          double *host_info_or_null);
/* Which loss the resident X serves from now on.  The reference builds a new loss object around the
 * same matrix for every front-end call (lasso.jl:33,48,71,93,117,245: CDLeastSquaresLoss(y, X),
 * CDSqrtLassoLoss(y, X), CDWeightedLSLoss(y, X, w)); the binding keeps X in HBM across those objects
 * and switches the handle to the kind of the loss it is called with.  Invalidates the carried
 * residual; CDH_WLS needs cdh_set_obs_weights before the next sweep (weights are zero until then). */
int32_t cdh_set_loss(cdh_handle h, int32_t loss);
/* Synthetic Gaussian problem generated on the device from a counter-based
 * generator keyed (seed, global row, column), shapes of benchmark/cd_bench.jl:
 * 8-14: X_ij ~ N(0,1), beta*_j = z_j (1 + u_j) for j < s, y = X beta* + noise e.
 * out_beta_star (may be NULL) receives the s planted values.  0 <= s <= p, else
 * CDH_BAD_ARG and nothing is written.  On a handle that has solved before, the
 * handle starts over: the iterate is zero, and data and later solves are those
 * of a new handle generated the same way, bit for bit. */
int32_t cdh_generate(cdh_handle h, uint64_t seed, int64_t s, double noise, double *out_beta_star);

/* ---- penalty: ProxL1(lambda0) / ProxL1(lambda0, omega) (ProximalBase) -------- */
/* omega == NULL means unweighted; otherwise n_omega must equal p
 * (coordinate_descent.jl:14-16 -> CDH_DIM_MISMATCH). */
int32_t cdh_set_penalty(cdh_handle h, double lambda0, const double *omega, int64_t n_omega);

/* ---- the operator interface (cd_differentiable_function.jl:1-35) ------------- */
/* numCoordinates(f) */
int32_t cdh_num_coordinates(cdh_handle h, int64_t *out);
/* initialize!(f, x): load the iterate (support in SparseIterate order: idx1[i],
 * val[i]) and rebuild r = y - X beta (cd_differentiable_function.jl:59-72).
 * x_length is numCoordinates(x), checked against p (coordinate_descent.jl:13). */
int32_t cdh_initialize(cdh_handle h, int64_t x_length, int64_t nnz, const int64_t *idx1,
                       const double *val);
/* Load the iterate WITHOUT touching r: what the binding calls before gradient /
 * descendCoordinate! / _cdPass! when the caller's x changed since the last call
 * (the reference reads x[k] directly, cd_differentiable_function.jl:101,253). */
int32_t cdh_set_iterate(cdh_handle h, int64_t x_length, int64_t nnz, const int64_t *idx1,
                        const double *val);
/* gradient(f, x, k) (cd_differentiable_function.jl:75-76, 234-235, 149-158) */
int32_t cdh_gradient(cdh_handle h, int64_t k1, double *out);
/* descendCoordinate!(f, g, x, k) -> h (cd_differentiable_function.jl:83-111,
 * 242-291, 165-194); r is left consistent with beta on return. */
int32_t cdh_descend(cdh_handle h, int64_t k1, double *out_h);

/* ---- the driver (coordinate_descent.jl) -------------------------------------- */
/* _findLambdaMax (coordinate_descent.jl:118-149), at the current r. */
int32_t cdh_lambda_max(cdh_handle h, double *out);
/* _cdPass! over an explicit visit list (coordinate_descent.jl:94-110):
 * maxH = max |h|, then dropzeros!. */
int32_t cdh_pass(cdh_handle h, int64_t m, const int64_t *idx1, double *out_maxH);
/* _coordinateDescent! (coordinate_descent.jl:65-92): assumes r is initialised. */
int32_t cdh_solve(cdh_handle h, const cdh_options *opt, cdh_stats *out);
/* coordinateDescent!(x, f, g::ProxL1, options) (coordinate_descent.jl:7-39):
 * warm start = initialize! from the handle's current iterate + one solve; cold
 * start = zero, lambda_max, numSteps+1 solves down a log grid. */
int32_t cdh_coordinate_descent(cdh_handle h, const cdh_options *opt, cdh_stats *out);

/* ---- results ------------------------------------------------------------------ */
int32_t cdh_get_beta(cdh_handle h, double *out_p);                       /* Vector(x)   */
int32_t cdh_get_support(cdh_handle h, int64_t *out_idx1, int64_t *out_nnz); /* nzval2ind  */
int32_t cdh_get_residual(cdh_handle h, void *out_n_local);               /* f.r (dtype) */
/* _stdX!(out, X) (utils.jl:127-138): out_j = sqrt(sum_i X_ij^2 / n_total). */
int32_t cdh_col_rms(cdh_handle h, double *out_p);
/* _stdX!(out, w, X) (utils.jl:140-151): out_j = sqrt(sum_i w_i X_ij^2 / n_total); CDH_WLS with weights set, else CDH_BAD_ARG. */
int32_t cdh_col_wrms(cdh_handle h, double *out_p);
/* _getLoadings!(out, X, e) (utils.jl:153-164) at e = the current residual: out_j = sqrt(sum_i (X_ij r_i)^2 / n_total), the
 * penalty loadings of feasibleLasso! (lasso.jl:179,186).  One pass over X, summed in double in a fixed order (bit-identical
 * run to run) over all shards; a function of X and r only, so any loss.  Read-only: beta, the penalty, the weights and the
 * gradient cache are left as they are (r catches up with pending moves first, as for every reader of r). */
int32_t cdh_loadings(cdh_handle h, double *out_p);
/* out_j = X_j' r for every column at the current r (At_mul_B_row for all j: the
 * screening scores of _findLargestCorrelations, utils.jl:96-106; KKT checks). */
int32_t cdh_xt_r(cdh_handle h, double *out_p);
/* Gram block of up to 4096 columns against the current r:
 * out_G[i*m+j] = X_i'X_j, out_c[i] = X_i'r, *out_q = r'r (all shards).  With r = y this is
 * what the s-column OLS of _findInitResiduals! needs (utils.jl:65-77: Xs \ y), without moving
 * any n-sized array to the host.  Up to 64 columns in one pass over them; more (round 4: the
 * reference takes any s) in groups of 32, one launch per pair of groups. */
int32_t cdh_gram(cdh_handle h, int64_t m, const int64_t *idx1, double *out_G, double *out_c,
                 double *out_q);
/* The same block with the observation weights of a CDH_WLS handle: out_G[i*m+j] = X_i'WX_j, out_c[i] = X_i'Wr,
 * *out_q = r'Wr; same limits and grouping as cdh_gram, whose result does not depend on the weights.  The refit of locpolyl1
 * (varying_coefficient_lasso.jl:71-76: (Xs'W Xs) \ (Xs'W y)) reads its normal equations off this at the solve's own
 * residual: Xs'Wy = Xs'Wr + (Xs'WXs) beta_S when beta is supported inside S.  Without weights set: CDH_BAD_ARG. */
int32_t cdh_gram_weighted(cdh_handle h, int64_t m, const int64_t *idx1, double *out_G, double *out_c,
                          double *out_q);
/* out_m[i] = X_idx1[i]' r (X'Wr for the weighted loss) for a LIST of columns at the current r: one pass over those
 * columns only.  The refinement step of the screening init: Xs \ y (utils.jl:70, a QR in the reference) is solved from the
 * Gram block, and the normal equations' residual Xs'(y - Xs b) read off here corrects b -- so near-collinear screening
 * columns do not cost the squared condition number. */
int32_t cdh_xt_r_cols(cdh_handle h, int64_t m, const int64_t *idx1, double *out_m);
/* std(f.r) as Statistics.std computes it (lasso.jl:37,52,81,97,143): two passes -- the mean, then the centred sum of
 * squares, Bessel-corrected -- over all shards.  out_mean may be NULL. */
int32_t cdh_resid_std(cdh_handle h, double *out_std, double *out_mean);
/* sum r, sum r^2 over all shards (sigma of scaledLasso!, lasso.jl:134; std(f.r)). */
int32_t cdh_resid_moments(cdh_handle h, double *out_sum, double *out_sumsq);
/* The two sums of _getSigma(w, r) (utils.jl:167-175: sigma = sqrt(sum_i w_i r_i^2 / sum_i w_i)) at the current residual, in
 * double and in a fixed order; either out pointer may be NULL.  CDH_WLS with weights set, else CDH_BAD_ARG. */
int32_t cdh_resid_wmoments(cdh_handle h, double *out_sum_w, double *out_sum_wr2);
/* f(beta) + lambda0 sum omega|beta| at the current state (coordinate_descent.jl:1-3). */
int32_t cdh_objective(cdh_handle h, double *out);

/* ---- execution control (no reference counterpart) ------------------------------- */
/* default: CDH_SWEEP_BLOCK, block = 32; `block` is ignored for CDH_SWEEP_COORD */
int32_t cdh_set_sweep_mode(cdh_handle h, int32_t mode, int32_t block);
/* Warm starts normally rebuild r = y - X beta as the reference's initialize! does
 * (coordinate_descent.jl:21).  With reuse on, a warm start whose iterate is the one the
 * handle already holds keeps the carried residual (LassoPath, lasso.jl:250-252: 100 rebuilds
 * of n x nnz work saved); the difference is rounding only. */
int32_t cdh_set_reuse_residual(cdh_handle h, int32_t on);
/* Full passes of cdh_solve / cdh_coordinate_descent over a sparse iterate are screened by
 * default: runs of visits that provably leave beta and r unchanged (beta_k == 0 and |X_k'r|
 * below the threshold) are settled from one dots-only pass over their columns; the iterates
 * are the same as visiting one by one.  on: 0 = never, 1 = full passes of the solves (default; cdh_pass
 * visits every column it is given), 2 = cdh_pass as well. */
int32_t cdh_set_screening(cdh_handle h, int32_t on);
/* Gradient cache of the screened full passes (exact; every loss, fp64 and fp32 storage).  With the Gram
 * columns X'X_j of the coordinates that move, X_k'r is known for every k without reading X, so a full pass
 * over a sparse iterate costs its real visits only -- what a lambda path (lasso.jl:250-252), the sigma loop
 * of scaledLasso! (:132-141) or a cold start's 51 solves (coordinate_descent.jl:32-36) repeat hundreds of
 * times on one X.  mode: 0 off; 1 (default) engages once the handle has run as many screened full passes on
 * the same data as the Gram columns of its support cost to fetch (at least three; a cold start engages at
 * once); 2 from the first full pass (what a path driver that knows it has 100 lambdas to go asks for).
 * On columns of 1 MB and more, modes 1 and 2 engage only while n_total >= 32 * nnz(x) (round 3: the fold of a move into the
 * gradient and the re-check of skipped certificates run on the device; while they were p host flops per mover the bound was
 * 400): a support that large makes most visits real ones anyway; mode 3 is mode 2 without that guard (tests).  Shorter
 * columns keep the cache whatever n / nnz is (a streamed visit is launch-bound there and loses to the covariance form).
 * Same iterates, support order and pass counts as visiting every coordinate.
 * While the cache is engaged the visits themselves need no read of X either (least squares, sqrt-lasso): the block
 * record the scalar-update kernel consumes -- X_k'r, the Gram entries between the block's coordinates -- is
 * read off the cached gradient and Gram columns ("covariance form"), and r is brought up to date once, before
 * anything reads it (cdh_get_residual, the moments, a streamed visit, ...).
 * cdh_cache_stats: out10 = {passes served, visits settled from the cache, visits made in those passes,
 * dots-only re-reference passes over X, Gram batches (up to 32 columns, one pass over X each),
 * Gram columns held, visits made in covariance form, residual catch-ups, covariance chunks / passes rolled back
 * because a skipped coordinate's certificate did not survive their own moves, passes served entirely on the
 * device (scan, visits and certificate re-check without the gradient leaving HBM)}. */
int32_t cdh_set_gradient_cache(cdh_handle h, int32_t mode);
/* The mode the handle is in now (a path driver upgrades 1 -> 2 for its own duration and puts back what it found:
 * lasso.jl:250-252 runs on a caller's loss object, whose settings are the caller's). */
int32_t cdh_get_gradient_cache(cdh_handle h, int32_t *out_mode);
int32_t cdh_cache_stats(cdh_handle h, int64_t *out10);
/* While the cache serves the passes of a solve, the pass loop of _coordinateDescent! itself (coordinate_descent.jl:74-91:
 * reset!(it, full), _cdPass!, dropzeros!, the convergence test) runs on the device -- one workgroup, one host round trip per
 * solve instead of two per pass; it comes back early only for what the host alone can give (Gram columns of coordinates
 * about to enter, a re-reference, the careful walk after a certificate broke).  Same iterates, support order and pass
 * counts.  On by default (environment CDH_COV_SOLVE=0, or on = 0 here, keeps the pass loop on the host).
 * cdh_device_loop_stats: out12 = {launches of the loop, passes run inside it, in-kernel folds of pending moves into the
 * gradient, certificates re-checked with the exact gradient because the bound did not cover them, and the time the kernel
 * spent per phase in 10 ns ticks: building visit lists, the scan, exact gradients of the visited coordinates, the visits,
 * the re-check, accepting a pass, the SparseIterate bookkeeping, dropzeros! and the rest}. */
int32_t cdh_set_device_loop(cdh_handle h, int32_t on);   /* 0: off; 1: on; 2: on, without helper workgroups; n > 2: on, with n helpers (at most 64) */
int32_t cdh_device_loop_stats(cdh_handle h, int64_t *out12);
/* Visit lists beyond the loop's LDS-sized Gram block (~150 non-zeros) run from a Gram TABLE in device memory: X_j'X_k by
 * table id for every coordinate the loop has visited, filled from the cached columns as coordinates enter and kept from
 * solve to solve, with the exact gradient of every coordinate it holds carried through each block of visits (rows of the
 * table: contiguous).  out8 = {passes run in table mode, table rows filled, coordinates the table holds, its capacity,
 * and how often a full pass whose re-check found coordinates crossing their threshold through the pass's own moves was
 * run again with those coordinates visited (instead of being walked position by position): by the host's device pass, by
 * the loop itself}.
 * Launches that expect such lists bring HELPER workgroups (the crew; CDH_CS_CREW = their number, default 31, 0: none): they
 * keep the gradient current for all p coordinates while workgroup 0 visits, and re-check the skipped coordinates of full
 * passes on the way, so that full passes of large supports stay in the loop too; out8[6..7] = {passes run with the crew,
 * jobs it was given}. */
int32_t cdh_device_loop_table(cdh_handle h, int64_t *out8);
/* How far the carried gradient has been from X'r whenever it was taken afresh from X (after CDH_GC_REFRESH
 * covariance-form visits, or right now with rereference_now != 0: one dots-only pass over X):
 *   drift = max_k |g_carried[k] - X_k'r| / thr_k,   thr_k = lambda0 n omega_k (sqrt-lasso: lambda0 omega_k ||r||)
 * -- the quantity the certificates' relative margin (1e-9 for fp64 storage) has to cover.
 * out3 = {drift at the last re-reference, the largest seen on this handle, re-references measured}. */
int32_t cdh_cache_drift(cdh_handle h, int32_t rereference_now, double *out3);
/* Inspection: the Gram column X'X_k (X'WX_k) the cache holds for coordinate k1 (1-based; CDH_BAD_ARG if it holds none),
 * p doubles, and the relative error its entries are DECLARED to carry, in units of sqrt(a_i a_k): 0 for fp64 storage; for
 * fp32 storage 2^-24 * 512 / sqrt(n_total) -- the fp32 matrix pipe sums 256-row chunks in fp32 before folding them into
 * fp64 -- which the certificates of the skipped visits allow for (no reference counterpart: the reference reads X itself at
 * every visit, cd_differentiable_function.jl:94-99). */
int32_t cdh_cache_gram_column(cdh_handle h, int64_t k1, double *out_p, double *out_eps);
/* Problems whose Gram matrix fits on chip -- p <= 1024 columns, one process -- are solved in ONE launch.  With at most
 * 16 MB of X (the reference's own test and benchmark shapes: test/lasso.jl:76-101, benchmark/cd_bench.jl:8-14) from the
 * first solve; with more, once the solves the handle ran on the streamed kernels have cost what building the matrix
 * would (ceil(p / 32) passes over X; a cold start, being numSteps + 1 solves, buys a cheap build outright).  The handle keeps the
 * full Gram matrix X'X (X'WX) of the resident X, and one wave runs the whole of _coordinateDescent!
 * (coordinate_descent.jl:65-92; a cold start's numSteps + 1 solves, :32-36, in the same launch) in covariance form, with
 * the SparseIterate bookkeeping that fixes the visit order of active passes replayed on the device.  Same iterates as the
 * streamed sweeps up to rounding.  On by default (environment CDH_SMALL_PATH=0, or on = 0 here, keeps every solve on the
 * streamed kernels).  cdh_onchip_stats: out2 = {solves run this way, Gram matrices built}. */
int32_t cdh_set_onchip_solve(cdh_handle h, int32_t on);
int32_t cdh_onchip_stats(cdh_handle h, int64_t *out2);
/* Of the last one-launch solve: out3 = {visit steps taken (a step settles a run of positions and makes at most one
 * move), shader cycles the kernel ran for, the same span in 100 MHz ticks} -- cycles / ticks * 0.1 is the clock in GHz
 * the chip held for a one-wave kernel. */
int32_t cdh_onchip_last(cdh_handle h, int64_t *out3);
/* Replay each pass from a captured hipGraph instead of individual launches (the north_star's
 * "full sweep captured under hipGraph").  Works on row shards too: the direct exchange takes its epoch
 * from device memory, RCCL all-reduces are captured with the kernels around them; only the host-staged
 * exchange (cdh_set_host_exchange) is launched node by node. */
int32_t cdh_set_use_graph(cdh_handle h, int32_t on);
/* Multi-process row sharding: rank 0 calls cdh_comm_unique_id, broadcasts the
 * 128 bytes (any transport), every rank calls cdh_comm_init. */
int32_t cdh_comm_unique_id(void *out_128_bytes);
int32_t cdh_comm_init(cdh_handle h, const void *id_128_bytes, int32_t rank, int32_t nranks);
/* Give the communicator up (ncclCommAbort) so that another exchange can be installed on the handle -- for a
 * caller that found it unusable (wrong sums from cdh_exchange_probe).  The shard stays a shard: until
 * cdh_set_host_exchange / the direct exchange takes over, every exchange on it refuses rather than sum
 * local rows only.  A handle that never had a communicator: no-op. */
int32_t cdh_comm_drop(cdh_handle h);
/* Optional direct exchange for the short per-block records (<= 2688 doubles) of a row-sharded
 * sweep: every rank stores its record into an IPC-mapped inbox on every peer and sums the
 * sources in rank order (one hop over the xGMI mesh, no ring).  OFF unless connected AND
 * enabled; longer vectors keep going through RCCL when a communicator exists.
 *   1. every rank: cdh_p2p_local_handle -> 64 opaque bytes (a HIP IPC memory handle);
 *   2. all-gather the handles in rank order (any transport), every rank: cdh_p2p_connect;
 *   3. every rank: cdh_p2p_enable(h, 1)  (collectively: all ranks or none).
 * A peer that never arrives ends the wait after a bounded spin; that call and every later
 * exchange on the handle return CDH_RCCL_ERROR (the ranks no longer agree on what was exchanged).  cdh_exchange_probe all-reduces `count` (<= 4096) host
 * doubles in place through whatever exchange is active (self-test of the transport). */
int32_t cdh_p2p_local_handle(cdh_handle h, void *out_64_bytes);
int32_t cdh_p2p_connect(cdh_handle h, const void *handles_64_bytes_each, int32_t rank, int32_t nranks);
int32_t cdh_p2p_enable(cdh_handle h, int32_t on);
int32_t cdh_exchange_probe(cdh_handle h, double *inout, int64_t count);
/* Bring-your-own transport for the row-shard exchange (MPI.jl from the Julia side, gloo in this
 * repository's tests): `fn` must sum `count` doubles in place over all ranks and return 0.  The library
 * stages the record through pinned host memory and calls it on the caller's thread in the middle of
 * the sweep, between the reduce and the scalar-update kernels -- the same seam the RCCL all-reduce and
 * the direct exchange sit behind.  Slower than both (a stream round trip per exchange); fn == NULL
 * removes it. */
typedef int32_t (*cdh_host_allreduce_fn)(void *user, double *inout, int64_t count);
int32_t cdh_set_host_exchange(cdh_handle h, cdh_host_allreduce_fn fn, void *user, int32_t rank,
                              int32_t nranks);
/* How many all-reduces this handle has issued through each exchange since it was created, and the
 * rank count the active exchange reports (ncclCommCount for RCCL; 1 when the handle is not sharded).
 * Any out pointer may be NULL. */
int32_t cdh_exchange_stats(cdh_handle h, int64_t *out_rccl_calls, int64_t *out_p2p_calls,
                           int64_t *out_host_calls, int32_t *out_nranks);
/* Average time (microseconds, HIP events on the handle's stream) of `iters` back-to-back all-reduces
 * of `count` (<= 4096) doubles through the active exchange; 0-ish when the handle is not sharded.
 * Collective: every rank calls it with the same arguments. */
int32_t cdh_exchange_latency(cdh_handle h, int64_t count, int32_t iters, double *out_us);
/* HIP-event timing of the sweep kernels on the handle's stream: everything
 * launched by cdh_pass / cdh_solve (and the kernels of cdh_vc_set_point) between begin and end.  out_launches counts
 * the dominant (column-streaming) kernel launches, out_ms the event time they
 * span in total. */
int32_t cdh_profile_begin(cdh_handle h);
int32_t cdh_profile_end(cdh_handle h, double *out_ms, int64_t *out_launches,
                        double *out_algorithmic_bytes);

/* ---- CDQuadraticLoss: f(x) = x'Ax/2 + x'b (cd_differentiable_function.jl:299-348) ------------------------------------
 * A second handle in the same library, for a BATCH of up to max_batch problems that share one symmetric p x p matrix A and
 * differ in b, lambda0 and omega (neighbourhood selection of a graph: b_j = -A_j, omega_jj = +inf; CLIME columns; grids of
 * lambda; many right-hand sides).  cdh_quad_coordinate_descent solves all of them in ONE launch, one workgroup per problem
 * running the reference's whole pass loop with the problem's state in LDS; A stays in device memory, shared.
 *   - fp64 only: the reference's Ax is Float64 whatever T is (:301).
 *   - p <= CDH_QUAD_MAX_P, the largest p whose per-problem state fits the 160 KiB of LDS of a CU; more is CDH_BAD_ARG.
 *   - diag(A) must be positive (the reference's a = 1 / A_kk, :326, is not pinned for anything else): else CDH_BAD_ARG.
 *   - Problems are numbered j = 0 .. m - 1 (a bulk index, like j0 above); coordinates are 1-based as everywhere.
 *   - A quad handle keeps no error text of its own: whatever one of these calls refuses or fails on, NULL or live handle,
 *     is described by cdh_last_error(NULL).
 *   - Same iterates, support order and pass counts as visiting coordinate by coordinate; ordered and shuffled sweeps (the
 *     splitmix64 substitute, seeded per call: every problem of a batch starts from opt->seed, as m separate calls would). */
#define CDH_QUAD_MAX_P 2559
typedef struct cdh_quad_s *cdh_quad;
/* The CDQuadraticLoss constructor (cd_differentiable_function.jl:304-308) for problems of p coordinates. */
int32_t cdh_quad_create(cdh_quad *out, int64_t p, int64_t max_batch, int32_t device);
int32_t cdh_quad_destroy(cdh_quad q); /* NULL is CDH_BAD_ARG here */
/* f.A (cd_differentiable_function.jl:300, 306): column-major p x p with leading dimension lda; only symmetry makes "row k = column k" true, and it is the
 * caller's contract as it is the reference's. */
int32_t cdh_quad_set_A(cdh_quad q, const double *A, int64_t lda);
/* f.b (cd_differentiable_function.jl:300) of m <= max_batch problems, column j of B (leading dimension ldb); as the constructor leaves a new loss (:307):
 * every iterate zero, Ax = 0, so g = b.  The penalty has to be set again afterwards. */
int32_t cdh_quad_set_b(cdh_quad q, int64_t m, const double *B, int64_t ldb);
/* ProxL1(lambda0[j]) / ProxL1(lambda0[j], omega) per problem (coordinate_descent.jl:7-16): omega NULL: unweighted; ldo == 0:
 * one p-vector for all problems; else column j of a p x m matrix with leading dimension ldo >= p.  +inf entries are allowed
 * (that coordinate stays zero). */
int32_t cdh_quad_set_penalty(cdh_quad q, const double *lambda0, const double *omega, int64_t ldo);
/* Load the iterate of problem j (support in SparseIterate order) without touching g: what the binding does when the caller's
 * x changed (the reference reads x[k] directly, cd_differentiable_function.jl:328). */
int32_t cdh_quad_set_iterate(cdh_quad q, int64_t j, int64_t nnz, const int64_t *idx1, const double *val);
/* The iterate of problem j as coordinateDescent! leaves its x (coordinate_descent.jl:7-11): nzval2ind and nzval in slot order
 * (idx1 and val hold up to p entries). */
int32_t cdh_quad_get_iterate(cdh_quad q, int64_t j, int64_t *nnz, int64_t *idx1, double *val);
/* initialize!(f, x) (cd_differentiable_function.jl:311-320) for all m problems: g_j = A x_j + b_j, summed in slot order. */
int32_t cdh_quad_initialize(cdh_quad q);
/* gradient(f, x, k) for every k (cd_differentiable_function.jl:321-322): out[k] = (Ax)_k + b_k of problem j, p doubles. */
int32_t cdh_quad_get_gradient(cdh_quad q, int64_t j, double *out);
/* descendCoordinate!(f, g, x, k) -> h (cd_differentiable_function.jl:324-348) on problem j; no dropzeros!. */
int32_t cdh_quad_descend(cdh_quad q, int64_t j, int64_t k1, double *out_h);
/* _cdPass! over an explicit visit list on problem j (coordinate_descent.jl:94-110): maxH = max |h|, then dropzeros!. */
int32_t cdh_quad_pass(cdh_quad q, int64_t j, int64_t n, const int64_t *idx1, double *maxH);
/* coordinateDescent!(x, f, g::ProxL1, options) (coordinate_descent.jl:7-39) for all m problems in one launch and one host
 * round trip: warm start = initialize! from the iterates the handle holds + one solve each; cold start = zero iterates,
 * lambda_max_j = max_k |b_jk| / omega_jk, numSteps + 1 <= 64 solves down each problem's own log grid.  stats: m entries
 * (may be NULL). */
int32_t cdh_quad_coordinate_descent(cdh_quad q, const cdh_options *opt, cdh_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* CDHIP_H */
