/* libeks_hip.so - C ABI of the MI355X (gfx950) ensemble-Kalman-smoother hot path.
 *
 * Drop-in boundary for the reference operator
 *     run_kalman_smoother(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_frames, smooth_param,
 *                         blocks, lr, s_bounds_log, tol, safety_cap, h_fn) -> (s_finals, ms, Vs)
 * (/root/reference eks/core.py:159-302) and the stages it is built from.  Every entry point takes
 * plain DEVICE pointers + sizes + a hipStream_t, enqueues on that stream, never allocates, never
 * synchronises and returns an int status.  The caller owns all buffers; scratch comes from a
 * caller-provided workspace whose size the *_workspace_bytes functions report.
 *
 * Native data layout is FRAME-MAJOR (what the reference's drivers hold before they transpose for
 * JAX, eks/singlecam_smoother.py:166, eks/multicam_smoother.py:429-430):
 *     y, var   float32 [T][K][O]      observations / ensemble variances (R_t = diag(max(var,1e-12)),
 *                                     eks/utils.py:368-377 - never materialised as a matrix)
 *     ms       float32 [T][K][D]      smoothed means        (reference returns (K,T,D), core.py:296)
 *     Vs       float32 [T][K][D][D]   smoothed covariances  (reference returns (K,T,D,D), :297)
 * Model parameters are float64 device arrays with the reference's shapes:
 *     m0 [K][D], S0 [K][D][D], A [K][D][D], C [K][O][D], Q [K][D][D], s [K]  (eks/core.py:160-166)
 */
#ifndef EKS_HIP_H
#define EKS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* eks_stream_t; /* == hipStream_t */

/* status codes */
#define EKS_OK 0
#define EKS_ERR_NULL (-1)        /* a required pointer is NULL */
#define EKS_ERR_SHAPE (-2)       /* non-positive or inconsistent dimension */
#define EKS_ERR_UNSUPPORTED (-3) /* (D,O)/flag combination not built */
#define EKS_ERR_WORKSPACE (-4)   /* workspace missing or too small */
#define EKS_CSV_IO (-5)          /* eks_csv_read_numeric: the file cannot be opened / mapped */
#define EKS_CSV_FALLBACK 1       /* eks_csv_read_numeric: not an error - the file holds something other than numbers and
                                    missing values (quotes, text, ragged lines): let pandas read it */
#define EKS_ERR_HIP_BASE (-1000) /* -1000 - hipError_t */

/* flags */
#define EKS_FLAG_DIAG_MODEL 1u /* caller asserts A, C, Q, S0 are diagonal and D == O: the K*D
                                  coordinates are independent scalar chains (singlecam, reference
                                  eks/singlecam_smoother.py:246-284).  Off-diagonals are not read. */
#define EKS_FLAG_VS_DIAG 2u    /* Vs is written as [T][K][D] (diagonal of the covariance only,
                                  which is all the reference's drivers consume:
                                  singlecam_smoother.py:210-211, multicam_smoother.py:509-510,
                                  :540-542).  Default: full [T][K][D][D]. */
#define EKS_FLAG_UNIT_AC 4u    /* with DIAG_MODEL: caller asserts A = C = I (folds multiplies) */
#define EKS_FLAG_Q_PD 8u       /* caller asserts every Q[k] is positive definite.  eks_nll (one s per
                                  keypoint, with gradient) and eks_adam_run on the general (D, O) path may
                                  then take d nll / d log s from the smoothing distribution (Fisher's
                                  identity: exact, plain float64) instead of dual numbers through the scan.
                                  Without the flag the dual-number kernels run (any PSD Q). */

#define EKS_FLAG_ADAM_PREPARED 16u /* eks_adam_run: eks_adam_prepare has run on this (dims, y, A, workspace) and nothing
                                     has written the workspace since - the call skips its own pass over y */

typedef struct {
  int32_t n_keypoints; /* K */
  int32_t n_frames;    /* T */
  int32_t state_dim;   /* D */
  int32_t obs_dim;     /* O */
  uint32_t flags;
} eks_dims_t;

const char* eks_version(void);
const char* eks_status_string(int status);

/* ---- fixed-s smoothing: the final pass of run_kalman_smoother (eks/core.py:269-297), i.e.
 * dynamax extended_kalman_smoother with linear f,h vmapped over keypoints. ------------------ */
size_t eks_smooth_workspace_bytes(const eks_dims_t* dims);
int eks_smooth(const eks_dims_t* dims, const float* y, const float* var, const double* m0,
               const double* S0, const double* A, const double* C, const double* Q,
               const double* s, float* ms, float* Vs, void* workspace, size_t workspace_bytes,
               eks_stream_t stream);

/* ---- eks_smooth with one process-noise scale per frame, for sessions with uneven frame intervals (dropped frames,
 * concatenated sessions, moments of known larger motion).  No reference counterpart.  The model is
 *     x_0 ~ N(m0, S0),      x_t = A x_{t-1} + N(0, s w_t Q)      for t = 1 .. T-1.
 * dims, flags (EKS_FLAG_DIAG_MODEL, EKS_FLAG_UNIT_AC, EKS_FLAG_VS_DIAG), y, var, the parameters and the layouts of ms and
 * Vs are exactly those of eks_smooth.
 *   qscale               float32 device array; qscale[t] = w_t scales the noise of the step INTO frame t.
 *                        qscale_per_keypoint == 0: [T], shared by all keypoints; otherwise [T][K], frame-major like y:
 *                        all D chains of keypoint k read entry [t][k].  ENTRY 0 (row 0) IS NEVER READ.  There is no w_T:
 *                        where a lane predicts past frame T-1 it uses 1, and no output depends on that value.
 *   precondition         every w that is read is finite and 0 <= w <= 1e6.  The library does not check it (the Python
 *                        layer does): a value outside it gives wrong numbers for the keypoints that read it, never a
 *                        fault.  w = 0 (no motion over the step) and a singular Q are fine.
 *   scalar chains        float32 lanes, five launches: a summarize and a replay of their own around eks_em_stats'
 *                        three-launch scan; workspace as eks_em_stats.  Never the windowed replay of eks_smooth (its
 *                        forgetting bound assumes a constant process noise): the EKS_SMOOTH_WINDOW* knobs have no effect.
 *                        With w = 1 everywhere the result is eks_smooth's up to the rounding of a differently associated
 *                        scan.  Full Vs rows need D <= 8, as eks_smooth.
 *   general models       D <= 6 and O <= 64 (else EKS_ERR_UNSUPPORTED and a workspace size of 0); always the generic
 *                        float64 summarize / scan / replay kernels of eks_smooth.
 * Refusals are eks_smooth's plus EKS_ERR_NULL for a NULL qscale and EKS_ERR_SHAPE where a launch index would leave 32
 * bits (as eks_em_stats); all are returned before anything is enqueued and leave ms and Vs untouched. ------------------ */
size_t eks_smooth_tv_workspace_bytes(const eks_dims_t* dims);
int eks_smooth_tv(const eks_dims_t* dims, const float* y, const float* var, const float* qscale,
                  int32_t qscale_per_keypoint, const double* m0, const double* S0, const double* A, const double* C,
                  const double* Q, const double* s, float* ms, float* Vs, void* workspace, size_t workspace_bytes,
                  eks_stream_t stream);

/* ---- eks_smooth under Student-t observation noise, for frames where the whole ensemble agrees on a wrong place (paw
 * swaps, reflections, occlusions): small ensemble variance, wrong observation.  No reference counterpart.  For every
 * scalar observation (chain coordinate on scalar chains, row o on general models, whose R_t is diagonal)
 *     y_t | x_t, lam_t ~ N(C x_t, r_t / lam_t),    lam_t ~ Gamma(nu / 2, rate nu / 2),    r_t = clip(var_t),
 * with eks_smooth's dynamics; inference is the mean-field iteration of Agamennoni, Nieto and Nebot (2012).  A call runs
 * n_iters >= 1 smoothing passes, all enqueued back to back.  Every pass smooths under r_eff = clip(r_t / lam_t); every
 * pass but the last then sets lam_t = (nu + 1) / (nu + delta_t), delta_t = ((y_t - C ms_t)^2 + C Vs_t C') / r_t (the
 * full Vs on general models), in (0, (nu + 1) / nu].  The last pass writes ms, Vs and leaves the weights alone: the
 * weights returned are the ones ms, Vs were smoothed under.  n_iters = 1 without input weights is eks_smooth's model
 * (on scalar chains: eks_smooth_tv's bits at w = 1).  A frame with var = 1e30 stays effectively missing.
 * dims, flags, y, var, the parameters and the layouts of ms and Vs are exactly those of eks_smooth.
 *   nu          degrees of freedom, finite and > 0 (large nu: the Gaussian smoother).
 *   weights     float32 [T][K][O], frame-major like var; may be NULL (a plane of the workspace serves: the size query
 *               always includes one).  weights_in != 0: the first pass starts from the caller's values (each finite
 *               and > 0) instead of 1 - to continue a run, or for a single pass under weights the caller chose; needs
 *               a non-NULL weights (else EKS_ERR_NULL).  Without it the plane is not read before it is written.
 *   change      float32 [K], may be NULL: max over frames and coordinates of |lam_new - lam_old| in the call's last
 *               weight update (an atomic max on the bits of non-negative floats, as eks_ekf_smooth's resid).  The call
 *               zeroes it first; it stays zero when n_iters = 1.
 *   scalar chains   float32 lanes, five launches per pass: a summarize and a replay of their own around eks_em_stats'
 *               three-launch scan; workspace as eks_em_stats plus the plane and a [T] vector of ones (the frames run
 *               eks_smooth_tv's bodies at w = 1).  Never the windowed replay.
 *   general models  D <= 6 and O <= 64 (else EKS_ERR_UNSUPPORTED and a workspace size of 0); always the generic
 *               float64 summarize / scan / replay kernels.  Correct, not tuned.
 *   accuracy    y - C ms cancels in float32 on scalar chains, so delta carries an absolute error of about
 *               (2^-24 |y|)^2 / r: negligible for var >= 1e-2 at |y| <= 400 px, useless for var near the 1e-12 clip -
 *               there the weights stay finite and in range (floored at 1e-30) but mean nothing.
 * Refusals are eks_smooth_tv's plus EKS_ERR_SHAPE for a non-finite or non-positive nu and for n_iters < 1; all are
 * returned before anything is enqueued and leave every output untouched.  The size query returns 0 for refused
 * shapes. ------------------ */
size_t eks_smooth_robust_workspace_bytes(const eks_dims_t* dims);
int eks_smooth_robust(const eks_dims_t* dims, const float* y, const float* var, const double* m0, const double* S0,
                      const double* A, const double* C, const double* Q, const double* s, double nu, int32_t n_iters,
                      float* weights, int32_t weights_in, float* change, float* ms, float* Vs, void* workspace,
                      size_t workspace_bytes, eks_stream_t stream);

/* ---- eks_smooth_robust with ONE weight per group of `group` consecutive observed coordinates: the x and y of a
 * single-camera keypoint, the two coordinates of one view of a multi-camera keypoint - what a paw swap or an occlusion
 * spoils together.  The multivariate Student-t of Agamennoni, Nieto and Nebot: for group G of keypoint k at frame t
 *     y_{t,G} | x_t, lam_{t,G} ~ N(C_G x_t, diag(r_{t,o}) / lam_{t,G}),    lam_{t,G} ~ Gamma(nu / 2, rate nu / 2).
 * Passes, outputs, continuation and change are eks_smooth_robust's; a pass smooths under clip(r_{t,o} / lam_{t,G(o)}) and
 * every pass but the last sets lam_{t,G} = (nu + g) / (nu + sum_{o in G} delta_{t,o}), in (0, (nu + g) / nu].  A
 * coordinate whose clipped variance is 1e30 is missing: it is no evidence and leaves its group's Gamma factor (g counts
 * the observed coordinates), so a group with nothing observed keeps weight 1.
 *   group       >= 1 and a divisor of O (on scalar chains O = D), else EKS_ERR_SHAPE.  group = 1 IS eks_smooth_robust:
 *               the call is forwarded and returns its bits.
 *   weights     float32 [T][K][O / group]; NULL, weights_in as eks_smooth_robust.
 *   scalar chains   the coordinates of a group are separate chains: a middle pass is six launches - summarize, the
 *               three-launch scan, a replay that stores delta into a float32 [T][N] contribution plane, and a combine
 *               launch, the only one that changes the weights; the last pass is five.  Workspace: eks_smooth_robust's
 *               with the [T][N / group] plane, plus the contribution plane.
 *   general models  eks_smooth_robust's kernels with the group sum in the lane; no combine launch.
 * Every other refusal is eks_smooth_robust's, in its order, before anything is enqueued; the size query returns 0 for
 * refused shapes. ------------------ */
size_t eks_smooth_robust_group_workspace_bytes(const eks_dims_t* dims, int32_t group);
int eks_smooth_robust_group(const eks_dims_t* dims, const float* y, const float* var, const double* m0, const double* S0,
                            const double* A, const double* C, const double* Q, const double* s, double nu, int32_t group,
                            int32_t n_iters, float* weights, int32_t weights_in, float* change, float* ms, float* Vs,
                            void* workspace, size_t workspace_bytes, eks_stream_t stream);

/* ---- eks_smooth under Student-t PROCESS noise, for true fast movements (a paw reach, a saccade, a startle): a few
 * frames of motion far larger than the rest of the session, which one s per keypoint must either round off or follow
 * at the price of under-smoothing every still frame.  No reference counterpart.  One weight per keypoint and frame,
 * shared by its D state coordinates (they jump together):
 *     x_t = A x_{t-1} + eps_t,   eps_t | u_t ~ N(0, s Q / u_t),   u_t ~ Gamma(nu / 2, rate nu / 2),   t = 1 .. T-1,
 * with eks_smooth's prior and observations; inference is the mean-field iteration.  A call runs n_iters >= 1 smoothing
 * passes, all enqueued back to back.  Every pass smooths under the scales w_t = 1 / u_t - exactly eks_smooth_tv with
 * qscale_per_keypoint = 1; every pass but the last then sets w_t = (nu + delta_t) / (nu + D),
 * delta_t = E[eps_t' (s Q)^-1 eps_t | y] under the pass's own scales, formed from what the RTS step holds without
 * inverting Q (singular Q is fine on general models); u stays in [1e-30, (nu + D) / nu].  The last pass writes ms, Vs
 * and leaves the scales alone: the scales returned are the ones ms, Vs were smoothed under (bit for bit eks_smooth_tv
 * called with them).  n_iters = 1 without input scales is eks_smooth_tv at w = 1.
 * dims, flags, y, var, the parameters and the layouts of ms and Vs are exactly those of eks_smooth_tv.
 *   nu          degrees of freedom, finite and > 0 (large nu: the Gaussian smoother).
 *   scales      float32 [T][K], the layout of eks_smooth_tv's per-keypoint qscale: w of the step INTO frame t; may be
 *               NULL (a plane of the workspace serves: the size query always includes one).  Row 0 is never read and is
 *               returned as 1.  scales_in != 0: the first pass starts from the caller's values (each finite and > 0)
 *               instead of 1 - to continue a run, or for a single pass under scales the caller chose; needs a non-NULL
 *               scales (else EKS_ERR_NULL).
 *   change      float32 [K], may be NULL: max over frames of |u_new - u_old|, u = 1 / w, in the call's last scale
 *               update (an atomic max on the bits of non-negative floats).  The call zeroes it first; it stays zero
 *               when n_iters = 1.
 *   continuing  n1 passes continued (scales_in) by n2 passes are one call of n1 + n2 - 1 passes, bit for bit.
 *   scalar chains   float32 lanes.  A middle pass is six launches: eks_smooth_tv's summarize, eks_em_stats'
 *               three-launch scan, a replay without outputs that stores every chain's delta_{t,d} into a [T][K D]
 *               plane, and a combine launch - the only one that changes the scales, because the D chains of a keypoint
 *               sit in different lanes.  The last pass is eks_smooth_tv's five launches.  Workspace: eks_em_stats' plus
 *               the two planes.  Never the windowed replay.  A chain with s q = 0 contributes w_t, its prior value
 *               (never 0 / 0), so a keypoint whose chains all have s q = 0 keeps w = 1.
 *   general models  D <= 6 and O <= 64 (else EKS_ERR_UNSUPPORTED and a workspace size of 0); always the generic
 *               float64 summarize / scan / replay kernels, delta_t in a [T][K] float64 plane, the same combine launch.
 *   accuracy    dm = ms_t - a mf_{t-1} cancels in float32 on scalar chains as y - c ms does for eks_smooth_robust's
 *               weights: delta carries an absolute error of about (2^-24 |ms|)^2 / Pp - negligible for s q >= 1e-3 at
 *               |y| <= 400 px, growing as s q and var fall towards their floors, where the scales stay finite and in
 *               range but mean little.
 * Refusals are eks_smooth_tv's plus EKS_ERR_SHAPE for a non-finite or non-positive nu and for n_iters < 1; all are
 * returned before anything is enqueued and leave every output untouched.  The size query returns 0 for refused
 * shapes. ------------------ */
size_t eks_smooth_jumps_workspace_bytes(const eks_dims_t* dims);
int eks_smooth_jumps(const eks_dims_t* dims, const float* y, const float* var, const double* m0, const double* S0,
                     const double* A, const double* C, const double* Q, const double* s, double nu, int32_t n_iters,
                     float* scales, int32_t scales_in, float* change, float* ms, float* Vs, void* workspace,
                     size_t workspace_bytes, eks_stream_t stream);

/* ---- eks_smooth under Student-t noise on BOTH sides: eks_smooth_robust's weight per scalar observation AND
 * eks_smooth_jumps' scale per keypoint and frame, for sessions that hold wrong observations and true fast movements
 * at once (alone, the robust model reads a reach as a run of outliers and the jumps model follows a one-frame swap as
 * two jumps).  No reference counterpart.
 *     y_t | x_t, lam_t ~ N(C x_t, r_t / lam_t),   lam_t ~ Gamma(nu_obs / 2, rate nu_obs / 2),   r_t = clip_var(var_t),
 *     eps_t | u_t ~ N(0, s Q / u_t),              u_t ~ Gamma(nu_proc / 2, rate nu_proc / 2),   t = 1 .. T-1,
 * by mean field over q(x) q(lam) q(u).  A call runs n_iters >= 1 smoothing passes, all enqueued back to back.  Every
 * pass smooths under r_eff = clip_var(r / lam) and w = 1 / u; every pass but the last then sets, from that one
 * smoothed posterior, lam = (nu_obs + 1) / (nu_obs + delta_obs) and w = (nu_proc + delta_proc) / (nu_proc + D) with
 * eks_smooth_robust's and eks_smooth_jumps' delta, clamps and floors.  Given q(x) the two updates are independent, so
 * the variational bound cannot drop.  The last pass writes ms, Vs and updates nothing: the planes returned are the
 * ones the outputs were smoothed under.  n_iters = 1 without input planes is the Gaussian smoother.
 * dims, flags, y, var, the parameters and the layouts of ms and Vs are exactly those of eks_smooth_tv.
 *   nu_obs, nu_proc  degrees of freedom of the two sides, each finite and > 0.
 *   weights     float32 [T][K][O] as eks_smooth_robust's; may be NULL (a plane of the workspace serves).
 *   scales      float32 [T][K] as eks_smooth_jumps'; may be NULL (a plane of the workspace serves).  Row 0 is never
 *               read and is returned as 1.  The size query always includes both planes.
 *   planes_in   bit 0: the first pass starts from the caller's weights; bit 1: from the caller's scales (each value
 *               finite and > 0).  A bit set with a NULL plane gives EKS_ERR_NULL.
 *   change      float32 [2][K], may be NULL: row 0 max |lam_new - lam_old|, row 1 max |u_new - u_old| (u = 1 / w) of
 *               the call's last update.  The call zeroes it first; it stays zero when n_iters = 1.
 *   continuing  n1 passes continued through both planes (planes_in = 3) by n2 passes are one call of n1 + n2 - 1
 *               passes, bit for bit.
 *   scalar chains   float32 lanes.  A middle pass is six launches: a summarize under both planes, eks_em_stats'
 *               three-launch scan, a replay without outputs - one backward loop that stores every chain's
 *               delta_{t,d} into a [T][K D] plane and the new weights in place - and eks_smooth_jumps' combine launch,
 *               the only one that changes the scales.  The last pass is five launches.  Workspace: eks_em_stats' plus
 *               the three planes.  Never the windowed replay.
 *   general models  D <= 6 and O <= 64 (else EKS_ERR_UNSUPPORTED and a workspace size of 0); always the generic
 *               float64 summarize / scan / replay kernels, the same combine launch.  Correct, not tuned.
 *   accuracy    the limits of eks_smooth_robust's weights and eks_smooth_jumps' scales both apply.
 * Refusals are eks_smooth_jumps', in the same order, with EKS_ERR_SHAPE when either nu is non-finite or non-positive
 * or n_iters < 1; all are returned before anything is enqueued and leave every output untouched.  The size query
 * returns 0 for refused shapes. ------------------ */
size_t eks_smooth_heavy_workspace_bytes(const eks_dims_t* dims);
int eks_smooth_heavy(const eks_dims_t* dims, const float* y, const float* var, const double* m0, const double* S0,
                     const double* A, const double* C, const double* Q, const double* s, double nu_obs, double nu_proc,
                     int32_t n_iters, float* weights, float* scales, int32_t planes_in, float* change, float* ms,
                     float* Vs, void* workspace, size_t workspace_bytes, eks_stream_t stream);

/* ---- eks_smooth_heavy that also fits the smoothing parameter s, by EM inside the mean-field iteration.  The Gaussian
 * likelihood explains displaced observations as process noise, so an s found on the Gaussian model is too large in
 * exactly the sessions the Student-t smoothers exist for.  No reference counterpart.  A middle pass smooths under
 * (lam, w = 1 / u, s) and makes eks_smooth_heavy's updates of lam and u - same formulas, clamps and launches - and
 * then, with q(x) and the new q(u) held, maximises the bound over s:
 *     S_k = sum_{t=1}^{T-1} u_new[t,k] delta[t,k],   s_new = s S_k / n,   n = D (T - 1),
 * on log s clipped to [log_s_lo, log_s_hi]; delta[t,k] = E[eps_t' (s Q)^-1 eps_t | y] is what the pass stored for the
 * update of u.  Coordinate ascent: the bound cannot drop.  Everything not named here is eks_smooth_heavy's.
 *   nu_obs, nu_proc  each > 0; +inf makes that side Gaussian: its plane stays at ones and its update is skipped.  With
 *               both +inf the iteration is eks_em_scale_run's (tr(Q^-1 Sw) / n) with one keypoint per block.
 *   s           [K], the start; never written.
 *   s_out       [K], required; s_out == s is allowed.  The start is copied to it first, every pass reads it, and on
 *               return it holds the s under which ms and Vs were smoothed.
 *   log_s_lo, log_s_hi   finite, lo <= hi.  The first pass smooths under s as given; every update is clipped.
 *   planes_in   as eks_smooth_heavy's; a bit set for a Gaussian side is EKS_ERR_SHAPE.  A Gaussian side's plane, if
 *               passed, comes back as ones.
 *   change      float32 [3][K], may be NULL: rows 0 and 1 as eks_smooth_heavy's (0 for a Gaussian side), row 2
 *               |delta log s| of the call's last update.  The call zeroes all three rows first.
 *   n_iters     n_iters = 1 is eks_smooth_heavy with n_iters = 1, bit for bit, and s_out = s.  With both nu finite and
 *               n_iters = 2 the two planes are eks_smooth_heavy's 2-pass planes bit for bit: pass 1 and its updates
 *               precede the first step.
 *   continuing  n1 passes continued through both planes and s_out by n2 passes are one call of n1 + n2 - 1 passes,
 *               bit for bit.
 *   the sum     float64 in a fixed order that depends on the frame alone - 16 rows, 64 such runs, then the slabs of
 *               1 024 rows in order; no floating-point atomics - so two calls give the same bits and a call on a subset
 *               of the keypoints gives that subset's bits (eks_em_stats' contract).  One launch of its own behind the
 *               combine launch (the block that finishes a keypoint tile last - an integer ticket - adds the slabs and
 *               makes the step); workspace: eks_smooth_heavy's plus [ceil((T - 1) / 1024)][K] doubles and the tickets.
 *   s q = 0     such a chain keeps eks_smooth_jumps' convention (its contribution is w), so it counts 1 per frame
 *               towards S_k.
 *   NaN         a keypoint whose S_k is not finite (NaN-poisoned input) keeps its s, with 0 in row 2 of change; every
 *               other keypoint is untouched bit for bit.  An s[k] that is not finite and positive is never stepped.
 *   general models  nu_obs = +inf is EKS_ERR_UNSUPPORTED (eks_smooth_jumps' general path has no loop to step in); the
 *               size query takes no nu and cannot say so.
 *   limits      EM only: from an s 10 .. 100 times too large s does shrink, but the first Gaussian pass has already
 *               committed the displaced frames as jumps and the trajectory stays where it was.
 * Refusals: T < 2; a nu that is NaN or not positive; log_s_lo > log_s_hi or a non-finite bound; an input plane on a
 * Gaussian side (all EKS_ERR_SHAPE); otherwise eks_smooth_heavy's, in the same order, s_out among the outputs.  All
 * are returned before anything is enqueued and leave every output untouched.  The size query returns 0 for refused
 * shapes. ------------------ */
size_t eks_smooth_heavy_fit_workspace_bytes(const eks_dims_t* dims);
int eks_smooth_heavy_fit(const eks_dims_t* dims, const float* y, const float* var, const double* m0, const double* S0,
                         const double* A, const double* C, const double* Q, const double* s, double nu_obs,
                         double nu_proc, int32_t n_iters, double log_s_lo, double log_s_hi, float* weights,
                         float* scales, int32_t planes_in, float* change, double* s_out, float* ms, float* Vs,
                         void* workspace, size_t workspace_bytes, eks_stream_t stream);

/* ---- joint posterior trajectories: n_draws draws of x_1..x_T from the smoothing distribution p(x | y) of the model
 * eks_smooth smooths (same dims, flags, y, var and parameters; EKS_FLAG_VS_DIAG is ignored).  No reference counterpart:
 * the reference returns the per-frame marginals ms, Vs only (eks/core.py:296-297), which say nothing about how the
 * uncertainty of frame t is tied to that of frame t + 1.  A draw is ms + e with e a zero-mean draw of the joint
 * posterior covariance, an affine function of W standard normals per (draw, frame, keypoint):
 *   scalar chains (EKS_FLAG_DIAG_MODEL): W = D, backward sampling e_t = G_t e_{t+1} + sqrt(Pf_t s q / Pp_{t+1}) z_t in
 *     the smoother's chunked scan (eks_amd/csrc/eks_sample.hip): y is read twice and var three times per call whatever
 *     n_draws is, the filtered quantities are shared by all draws;
 *   general models: W = D + O, Durbin & Koopman's simulation smoother composed from eks_smooth
 *     (eks_amd/csrc/eks_sample_dense.hip): correct, not tuned - a draw costs a smoothing pass.
 * The normals come from Philox4x32-10 (key = (seed & 0xffffffff, seed >> 32)) and Box-Muller, with GLOBAL indices
 * k' = first_keypoint + k, d' = first_draw + d in the counter, so that a draw depends on no launch geometry and a call
 * on keypoints [k0, k1) / draws [d0, d1) of a larger problem (first_keypoint = k0, first_draw = d0) returns that
 * problem's normals bit for bit (and, on scalar chains, its draws bit for bit; on general models the draws agree to
 * the smoother's rounding, the stacked smoothing call being free to organise its kernels by size).  Exact layout (x0..x3 the block's output words):
 *   scalar chains: counter = (t / 4, k' * D + i, d', 0) for coordinate i; the block serves the four frames
 *     4 (t / 4) + {0, 1, 2, 3} of that chain: (z_+0, z_+1) = BM(x0, x1), (z_+2, z_+3) = BM(x2, x3);
 *   general models: counter = (t, k', d', b); the block gives normals w = 4 b .. 4 b + 3 of (draw, frame, keypoint):
 *     (z_4b, z_4b+1) = BM(x0, x1), (z_4b+2, z_4b+3) = BM(x2, x3); w < D: state noise (chol(S0) at t = 0, chol(s Q)
 *     after), w >= D: observation noise of output w - D;
 *   BM(a, b): u = ((a >> 8) + 0.5) 2^-24, v = (b >> 8) 2^-24, r = sqrt(-2 ln u), (r cos 2 pi v, r sin 2 pi v).
 *   draws float32 [n_draws][T][K][D]; ms float32 [T][K][D] optional (the smoothed mean of the same pass);
 *   noise float32 [n_draws][T][K][W] optional: used INSTEAD of the generator (all zeros give draws == ms).
 * eks_sample_noise writes exactly the normals eks_sample would generate.  n_draws < 1: EKS_ERR_SHAPE.  General
 * models: D > 6 or O > 64 is EKS_ERR_UNSUPPORTED, (n_draws + 1) K D > 2^24 (the stacked smoothing call's chains)
 * EKS_ERR_SHAPE, and eks_sample_workspace_bytes returns 0 for both; eks_sample_noise refuses W = D + O > 70, wider
 * than any supported model, with EKS_ERR_SHAPE.  Every refusal is returned before anything is enqueued. ------------ */
int32_t eks_sample_noise_width(const eks_dims_t* dims);
size_t eks_sample_workspace_bytes(const eks_dims_t* dims, int32_t n_draws);
int eks_sample(const eks_dims_t* dims, const float* y, const float* var, const double* m0, const double* S0,
               const double* A, const double* C, const double* Q, const double* s, int32_t n_draws, uint64_t seed,
               int32_t first_keypoint, int32_t first_draw, const float* noise, float* ms, float* draws,
               void* workspace, size_t workspace_bytes, eks_stream_t stream);
int eks_sample_noise(const eks_dims_t* dims, int32_t n_draws, uint64_t seed, int32_t first_keypoint,
                     int32_t first_draw, float* noise, eks_stream_t stream);

/* ---- eks_sample under a per-frame process-noise scale and observation weights: draws from the smoothing distribution of
 *   x_t = A x_{t-1} + N(0, s w_t Q),     y_t = C x_t + N(0, r_eff,t),     r_eff,t = clip(clip(var_t) / lam_t)
 * - eks_smooth_tv's model at lam = 1, and the Gaussian factor of the mean-field posteriors of eks_smooth_robust,
 * eks_smooth_robust_group, eks_smooth_jumps, eks_smooth_heavy and eks_smooth_heavy_fit at the planes they return (nu
 * does not enter).  No reference counterpart.
 *   qscale   float32 [T] (qscale_per_keypoint == 0) or [T][K], eks_smooth_tv's convention: the scale of the step INTO
 *            frame t; row 0 is never read (a NaN there changes nothing).  NULL: every scale is 1.  Precondition as
 *            there: 0 <= w <= 1e6, finite.
 *   weights  float32 [T][K][O] as eks_smooth_robust's; every value finite and > 0 (the caller's precondition; a
 *            grouped plane is expanded to one value per coordinate by the caller).  NULL: every weight is 1.
 * dims, flags, y, var, the parameters, n_draws, seed, first_keypoint, first_draw, noise, ms, draws, the generator, its
 * counter layout and the noise width are exactly eks_sample's; eks_sample_noise serves both entries.
 *   scalar chains   eks_sample's seven launches (eks_amd/csrc/eks_sample_tv.hip): frame t's filter step, gain G_t and
 *            innovation sd_t all read w[t + 1]; the session's last frame has G = 0, sd = sqrt(Pf).  The variances are
 *            reweighted in registers.  Workspace: eks_sample's.
 *   general models  Durbin & Koopman as eks_sample, the state noise of the step into frame t scaled by sqrt(w_t), the
 *            observation noise drawn at r_eff, and the stacked call eks_smooth_tv's (eks_amd/csrc/eks_sample_dense.hip).
 * Refusals: eks_sample's in eks_sample's order, then eks_smooth_tv's for the shape; all are returned before anything
 * is enqueued, and eks_sample_tv_workspace_bytes returns 0 for every refused shape.  Every workspace plane is written
 * by the call before the call reads it. ------------ */
size_t eks_sample_tv_workspace_bytes(const eks_dims_t* dims, int32_t n_draws);
int eks_sample_tv(const eks_dims_t* dims, const float* y, const float* var, const float* qscale,
                  int32_t qscale_per_keypoint, const float* weights, const double* m0, const double* S0,
                  const double* A, const double* C, const double* Q, const double* s, int32_t n_draws, uint64_t seed,
                  int32_t first_keypoint, int32_t first_draw, const float* noise, float* ms, float* draws,
                  void* workspace, size_t workspace_bytes, eks_stream_t stream);

/* ---- eks_smooth plus the posterior of frame-to-frame increments.  No reference counterpart: the variance of
 * x_{t+1} - x_t (velocity, speed, movement onsets) is not a function of the marginals ms, Vs; it needs
 * Cov(x_t, x_{t+1} | y), which the RTS step holds in closed form.  dims, flags, inputs and the ms / Vs layouts are
 * exactly those of eks_smooth (here ms and Vs may each be NULL).  For t = 0 .. T-2, with (mf, Pf) the filtered and
 * (m', P') the smoothed belief of frame t+1, Pp the predicted covariance and G the smoother gain of frame t:
 *   lag1[t]  = Cov(x_t, x_{t+1} | y) = G P'              row: coordinate of x_t, column: coordinate of x_{t+1}
 *   dmean[t] = E[x_{t+1} - x_t | y]                       formed in the lane, not as a difference of float32 means
 *   dV[t]    = Cov(x_{t+1} - x_t | y) = (I - G) P' (I - G)^T + (Pf - G Pp G^T)
 * (scalar chains: G = a Pf / Pp, g = 1 - G: lag1 = G P', dmean = g (m' - a mf) - (1 - a) mf, dV = g^2 P' + Pf s q / Pp;
 * a sum of non-negative products where Vs[t] + Vs[t+1] - 2 lag1[t] cancels).  Row T-1 of all three is zero.
 *   dmean float32 [T][K][D]; lag1, dV follow the layout rule of Vs: [T][K][D] (diagonals) with EKS_FLAG_VS_DIAG,
 *   [T][K][D][D] without.  Any of the three may be NULL, not all (EKS_ERR_NULL); a NULL output costs no stores.
 *   scalar chains (EKS_FLAG_DIAG_MODEL): off-diagonals are identically zero, so the call exists with EKS_FLAG_VS_DIAG
 *     only (EKS_ERR_UNSUPPORTED without); summarize, grouped Kalman scan, replay (eks_amd/csrc/eks_increments.hip):
 *     y and var are read twice, every output is written once;
 *   general models: D <= 6 and O <= 64 (else EKS_ERR_UNSUPPORTED); always the generic kernels of eks_smooth with a
 *     replay that works in float64 and rounds once (eks_amd/csrc/eks_dense.hip: dense_increments); only Pp is
 *     factored, so a singular Q or S0 is fine.
 * A shape whose launches would index threads beyond an int is EKS_ERR_SHAPE.  Every refusal is returned before
 * anything is enqueued, and the workspace query returns 0 for refused shapes. ------------------------------------ */
size_t eks_smooth_increments_workspace_bytes(const eks_dims_t* dims);
int eks_smooth_increments(const eks_dims_t* dims, const float* y, const float* var, const double* m0,
                          const double* S0, const double* A, const double* C, const double* Q, const double* s,
                          float* ms, float* Vs, float* lag1, float* dmean, float* dV, void* workspace,
                          size_t workspace_bytes, eks_stream_t stream);

/* ---- EM on the model eks_smooth runs (time-varying R = diag(max(var_t, 1e-12))).  No reference counterpart: the
 * reference fits s to a constant-R filter likelihood.  dims, flags and inputs are those of eks_smooth.
 * E-step statistic, per keypoint: the smoothed second moment of the process noise
 *   Sw = sum_{t=0}^{T-2} E[ w_t w_t^T | y ],   w_t = x_{t+1} - A x_t,
 * formed inside the RTS step as a sum of non-negative terms (eks_amd/csrc/eks_em_lane.hpp), summed in float64 in a
 * fixed order without floating-point atomics: two calls give the same bits, and on scalar chains a call on a subset
 * of the keypoints gives that subset's bits.  By Fisher's identity, with n = D (T - 1),
 *   d loglik / d log s = (tr(Q^-1 Sw) / s - n) / 2       (loglik: the filter's, with the time-varying R).
 *   Sw float64: scalar chains (EKS_FLAG_DIAG_MODEL) [K][D], the diagonal - all a diagonal Q's M-step reads; the
 *     off-diagonal sums of E w_a E w_b are not formed - and the call exists with EKS_FLAG_VS_DIAG only
 *     (EKS_ERR_UNSUPPORTED without); the filter and the RTS step are eks_smooth's float32 ones, nothing of length T
 *     is written.  General models: [K][D][D], or [K][D] diagonals with EKS_FLAG_VS_DIAG; D <= 6 and O <= 64 (else
 *     EKS_ERR_UNSUPPORTED), float64 throughout, only Pp is factored so a singular Q or S0 is fine.
 *   T == 1 gives zeros.  A shape whose launches would index threads beyond an int is EKS_ERR_SHAPE.  Every refusal
 *   is returned before anything is enqueued, and the workspace query returns 0 for refused shapes.
 * M-step for the scale s with Q fixed (eks_em_scale_step, one thread per block of keypoints sharing one s; blocks
 * in CSR form as for eks_adam_step):  s_new = sum_members tr(Q^-1 Sw) / sum_members n, on log s clipped to
 * [lo, hi]; done = |delta log s| < tol; each step cannot decrease the likelihood.
 *   state float64 [n_blocks][4] = {log s, last |delta log s|, iterations, done}: the caller sets {log s0, 0, 0, 0}
 *   and s_keypoint[k] = s0 of k's block.  Blocks that are done or at max_iters are left untouched.  The step writes
 *   s_keypoint [K] for the next E-step and *n_active = the number of blocks still running.
 *   Sw as eks_em_stats writes it: [K][D] on scalar chains (Q^-1 = 1 / q_i), [K][D][D] on general models (Q^-1 by
 *   Cholesky; EKS_FLAG_VS_DIAG there is EKS_ERR_UNSUPPORTED: the trace needs the off-diagonals).
 * eks_em_scale_run enqueues n_iters x { eks_em_stats at s_keypoint -> eks_em_scale_step } back to back, no host
 * round trip; workspace as eks_em_stats.  Both refuse T < 2 with EKS_ERR_SHAPE (n = 0); the run refuses general
 * models without EKS_FLAG_Q_PD with EKS_ERR_UNSUPPORTED.  EM is slow when the optimum is far from the start: these
 * calls REFINE an s that is already close (eks_adam_run's). -------------------------------------------------------- */
size_t eks_em_stats_workspace_bytes(const eks_dims_t* dims);
int eks_em_stats(const eks_dims_t* dims, const float* y, const float* var, const double* m0, const double* S0,
                 const double* A, const double* C, const double* Q, const double* s, double* Sw, void* workspace,
                 size_t workspace_bytes, eks_stream_t stream);
int eks_em_scale_step(const eks_dims_t* dims, const double* Q, const double* Sw, int32_t n_blocks,
                      const int32_t* block_offsets, const int32_t* block_members, double lo, double hi, double tol,
                      int32_t max_iters, double* state, double* s_keypoint, int32_t* n_active, eks_stream_t stream);
int eks_em_scale_run(const eks_dims_t* dims, const float* y, const float* var, const double* m0, const double* S0,
                     const double* A, const double* C, const double* Q, int32_t n_blocks,
                     const int32_t* block_offsets, const int32_t* block_members, double lo, double hi, double tol,
                     int32_t max_iters, int32_t n_iters, double* state, double* s_keypoint, double* Sw,
                     int32_t* n_active, void* workspace, size_t workspace_bytes, eks_stream_t stream);

/* ---- the forward filter's view of the model eks_smooth runs (time-varying R = diag(clip(var_t, 1e-12, 1e30))): the
 * prediction-error decomposition.  No reference counterpart: eks_nll has a constant R, eks_ar1_nll is the pupil
 * smoother's loss.  dims, flags, inputs and the variance clip are those of eks_smooth; EKS_FLAG_VS_DIAG is ignored.
 * Per frame t, from the PREDICTED belief (m_{t|t-1}, P_{t|t-1}) - the prior (m0, S0) at t = 0 - before any update
 * with frame t:
 *   innov     float32 [T][K][O]   v_t = y_t - C m_{t|t-1}
 *   innov_var float32 [T][K][O]   the diagonal of S_t = C P_{t|t-1} C' + R_t
 *   nis       float32 [T][K]      v' S^-1 v                                        (general models only)
 *   frame_ll  float32 [T][K]      -0.5 (O log 2 pi + log det S_t + nis)            (general models only)
 *   loglik    float64             the sum over frames: [K][D], per chain as Sw is, on scalar chains; [K] on general
 *                                 models.  By Fisher's identity its derivative in log s is eks_em_stats' statistic.
 * Every output may be NULL, not all of them (EKS_ERR_NULL); a NULL output costs no stores (and, for loglik, no
 * logarithms).  Standardised innovations v / sqrt(innov_var) are N(0, 1) and white when the model is right.
 *   scalar chains (EKS_FLAG_DIAG_MODEL): eks_em_stats' summarize and grouped Kalman scan as they are, then a forward
 *     replay (eks_amd/csrc/eks_innov.hip) that forms S and d with filter_step's own expressions - the belief carried
 *     forward is bit for bit the smoother's; the frame's term log 2 pi + log S + d^2 / S in float32, the sum in float64.
 *     nis and frame_ll are elementwise functions of innov and innov_var there: a non-NULL pointer is
 *     EKS_ERR_UNSUPPORTED.  y and var are read twice; with loglik alone nothing of length T is written.
 *   general models: D <= 6 and O <= 64 (else EKS_ERR_UNSUPPORTED); the generic summarize / scan kernels of eks_smooth,
 *     then a forward replay in float64 that rounds once (eks_amd/csrc/eks_dense.hip: dense_innovations): log det S_t
 *     and nis from the sequential scalar updates, exact for the diagonal R; nothing is factored, so a singular Q or
 *     S0 is fine while the innovation variances are positive.
 * loglik is summed in float64 from one partial per (chunk, chain or keypoint) in a fixed order without floating-point
 * atomics: two calls give the same bits, and on scalar chains a call on a subset of the keypoints gives that subset's
 * bits.  T == 1 is valid.  A shape whose launches would index threads beyond an int is EKS_ERR_SHAPE, a small
 * workspace EKS_ERR_WORKSPACE.  Every refusal is returned before anything is enqueued, the outputs stay untouched,
 * and the workspace query returns 0 for refused shapes. ---------------------------------------------------------- */
size_t eks_innovations_workspace_bytes(const eks_dims_t* dims);
int eks_innovations(const eks_dims_t* dims, const float* y, const float* var, const double* m0, const double* S0,
                    const double* A, const double* C, const double* Q, const double* s, float* innov,
                    float* innov_var, float* nis, float* frame_ll, double* loglik, void* workspace,
                    size_t workspace_bytes, eks_stream_t stream);

/* ---- constant observation noise for the loss: eks/core.py:702-709
 * rconst[k][o] = max(nanmedian_t max(var[t][k][o], 1e-12), min_var)  (float64 out) ----------- */
size_t eks_const_r_workspace_bytes(const eks_dims_t* dims);
int eks_const_r(const eks_dims_t* dims, const float* var, double min_var, double* rconst,
                void* workspace, size_t workspace_bytes, eks_stream_t stream);

/* ---- filter negative log-likelihood with constant R on a set of smoothing-parameter values:
 * the loss of eks/core.py:640-650 (nll = -marginal_loglik of extended_kalman_filter, non-finite
 * -> 1e12).  s_cand is [n_cand] when per_keypoint == 0 (one grid shared by all keypoints: the
 * 64-candidate search of BASELINE.json config 3) or [K][n_cand] when per_keypoint == 1 (used with
 * n_cand == 1 by the Adam loop).  nll is [K][n_cand] float64; dnll (optional, may be NULL) is
 * d nll / d log s of the same shape (forward sensitivity replacing jax.value_and_grad, :652). -- */
size_t eks_nll_workspace_bytes(const eks_dims_t* dims, int32_t n_cand);
int eks_nll(const eks_dims_t* dims, const float* y, const double* rconst, const double* m0,
            const double* S0, const double* A, const double* C, const double* Q,
            const double* s_cand, int32_t n_cand, int32_t per_keypoint, double* nll, double* dnll,
            void* workspace, size_t workspace_bytes, eks_stream_t stream);

/* ---- order statistics for numpy.percentile's linear interpolation: center_predictions' per-keypoint
 * threshold on the worst ensemble variance (eks/utils.py:318-322, np.percentile(..., axis=0)) and the
 * v_quantile_threshold of the variance-inflation loop (eks/stats.py:109-112).  x [n_rows][n_cols] float32;
 * out[c] = {x_sorted[rank_lo], x_sorted[rank_hi]} of column c with NaNs sorted last as numpy sorts them
 * (rank_hi = rank_lo or rank_lo + 1), nan_count[c] = number of NaNs in the column (numpy returns NaN for
 * such a slice).  The interpolation itself is three float32 operations per column and stays with the
 * caller, which forms it with numpy's own expressions (eks_amd/utils.py percentile_from_order_stats). ---- */
int eks_order_stats(int32_t n_rows, int32_t n_cols, const float* x, int32_t rank_lo, int32_t rank_hi,
                    float* out, int32_t* nan_count, eks_stream_t stream);

/* ---- numpy.nanstd(x, axis=1) of a [n_rows][n_cols] float32 matrix, BIT FOR BIT: the optimiser's initial guess
 * (reference eks/core.py:104-133, compute_initial_guesses: round(nanstd(differences of the ensemble variances), 5))
 * seeds the Adam trajectory through a float32, so it has to be numpy's value, and numpy's value is a function of
 * its summation order (pairwise, eks_amd/csrc/eks_np_sum.hpp).  leaves: n_leaves pairs (start, length <= 128) of
 * that recursion's leaves left to right; ops: n_leaves - 1 triples (dst, a, b) in evaluation order over slots
 * 0 .. n_leaves - 1 = leaf sums, n_leaves .. = internal nodes, the last one the root (both tables depend on n_cols
 * only; eks_amd/hip_ops.py: np_sum_program builds them).  out[r] float32; a row without a finite value gives NaN.
 * (n_cols + 2 n_leaves) * 4 bytes must fit 64 KB of LDS: EKS_ERR_UNSUPPORTED otherwise. ---------------------- */
int eks_np_nanstd_rows(int32_t n_rows, int32_t n_cols, const float* x, const int32_t* leaves, int32_t n_leaves,
                       const int32_t* ops, int32_t n_ops, float* out, eks_stream_t stream);

/* ---- the same for the rows compute_initial_guesses actually reduces (eks/core.py:128-130), formed on the fly: row k,
 * element t * obs_dim + o = x[t + 1][k][o] - x[t][k][o] of a frame-major [n_frames][n_keypoints][obs_dim] float32
 * tensor (the first n_frames <= 2 000 frames of the ensemble variances) - one launch instead of a subtraction, a
 * transposing copy and the reduction.  leaves / ops: the tables for n_cols = (n_frames - 1) * obs_dim. ------------- */
int eks_np_nanstd_diff_rows(int32_t n_frames, int32_t n_keypoints, int32_t obs_dim, const float* x, const int32_t* leaves,
                            int32_t n_leaves, const int32_t* ops, int32_t n_ops, float* out, eks_stream_t stream);

/* ---- argmin over candidates + gather: s_out[k] = s_cand[argmin_c nll[k][c]], numpy.argmin's rule: the first
 * minimum (ties, +0 / -0 included, go to the lower index), and a NaN counts as smaller than every number, so a row
 * with NaNs gives the index of its first NaN.  idx_out (optional) receives the int32 indices. ---------------------- */
int eks_argmin_s(int32_t n_keypoints, int32_t n_cand, const double* nll, const double* s_cand,
                 double* s_out, int32_t* idx_out, eks_stream_t stream);

/* ---- the grid search in one call: eks_nll (value only) followed by eks_argmin_s, as ONE entry point so that the
 * scalar-chain grid kernels can take the argmin inside the assembly of the table (the block that finishes a tile of
 * keypoints last does it: no separate launch).  This is the smoothing-parameter search of BASELINE.json config 3
 * (the reference's own search, eks/core.py:562-699, is the Adam loop below).  Arguments as eks_nll (per_keypoint = 0)
 * and eks_argmin_s; nll [K][n_cand] is still written in full.  Shapes the fused kernels do not cover run the two
 * steps one after the other - the results are the same either way.  workspace: eks_nll_workspace_bytes. ------------ */
int eks_nll_argmin(const eks_dims_t* dims, const float* y, const double* rconst, const double* m0,
                   const double* S0, const double* A, const double* C, const double* Q,
                   const double* s_cand, int32_t n_cand, double* nll, double* s_out, int32_t* idx_out,
                   void* workspace, size_t workspace_bytes, eks_stream_t stream);

/* ---- one Adam iteration on u = log s for every block of keypoints, with the reference's
 * control flow (eks/core.py:652-681 singletons, :509-549 blocks): L_b = sum of member nll,
 * g_b = lr * sum of member dnll (zero where u is outside [lo, hi], as jnp.clip differentiates),
 * optax.adam(1.0) update (b1 .9, b2 .999, eps 1e-8, bias-corrected), then
 * done = isfinite(prev) && |L - prev| < tol * |log(max(prev, 1e-12))| + 1e-6; prev = L; ++iters.
 * Blocks that are done or at safety_cap are left untouched.  Blocks are given in CSR form
 * (block_offsets [n_blocks+1], block_members [K]).  state is [n_blocks][6] float64:
 * {u, mom, vel, prev_loss, iters, done}.  Writes s_keypoint[k] = exp(clip(u_block(k), lo, hi)) for
 * the next evaluation and *n_active = number of blocks still running after this step. -------- */
int eks_adam_step(int32_t n_blocks, const int32_t* block_offsets, const int32_t* block_members,
                  const double* nll, const double* dnll, double lr, double lo, double hi,
                  double tol, int32_t safety_cap, double* state, double* s_keypoint,
                  int32_t* n_active, eks_stream_t stream);

/* ---- n_iters iterations of { eks_nll (one s per keypoint, with dnll) -> eks_adam_step } enqueued
 * back to back: the body of the lax.while_loop of eks/core.py:654-681 (:520-549 for blocks) without
 * a host round trip per iteration.  Arguments as in eks_nll / eks_adam_step; s_keypoint [K] is
 * both the evaluation point and the step's output; nll, dnll [K] hold the last evaluation.
 * Iterations enqueued after a block has stopped leave it untouched, so the caller may issue
 * n_iters at a time and read *n_active in between.  workspace: eks_nll_workspace_bytes(dims, 1).
 * Scalar chains with one keypoint per block (the reference's default, blocks = []): all n_iters iterations are ONE
 * launch with a workgroup per keypoint and no exchange between workgroups.  Sessions of 1 024 frames and more (at most
 * four chains per keypoint) do not read y per iteration at all: one streaming pass leaves 256 lag sums of the inputs
 * u_t = y_t - a y_{t-1} per chain - they do not depend on s - and every iteration evaluates loss and gradient from those
 * plus the first / last 257 rows (eks_amd/csrc/eks_lag_adam.hip); a chain whose pole leaves the range the sums cover
 * (|rho| > 0.906) is evaluated exactly from a private copy of its frames instead.  eks_adam_prepare runs that pass ahead
 * of time (see EKS_FLAG_ADAM_PREPARED). */
int eks_adam_run(const eks_dims_t* dims, const float* y, const double* rconst, const double* m0,
                 const double* S0, const double* A, const double* C, const double* Q,
                 int32_t n_blocks, const int32_t* block_offsets, const int32_t* block_members,
                 double lr, double lo, double hi, double tol, int32_t safety_cap, int32_t n_iters,
                 double* state, double* s_keypoint, double* nll, double* dnll, int32_t* n_active,
                 void* workspace, size_t workspace_bytes, eks_stream_t stream);

/* ---- the pass over y of eks_adam_run's scalar-chain search, ahead of the optimiser's starting point: the reference
 * computes its initial guesses from the ensemble variances on the host (eks/core.py:233-236), and this pass needs only
 * y and A - a caller enqueues it, fetches the guesses while it runs, uploads the state and calls eks_adam_run with
 * EKS_FLAG_ADAM_PREPARED set in dims->flags.  Returns EKS_ERR_UNSUPPORTED (nothing enqueued) where eks_adam_run would
 * not use the sums (other model classes, blocks of several keypoints, short sessions): call eks_adam_run without the
 * flag then.  workspace: the one eks_adam_run will be given. */
int eks_adam_prepare(const eks_dims_t* dims, const float* y, const double* A, int32_t n_blocks, void* workspace,
                     size_t workspace_bytes, eks_stream_t stream);

/* ---- how many iterations one eks_adam_run call should ask for on this problem, device and library build: the calls
 * are what the caller's host round trips (reading *n_active) are spaced by, and what they cost differs by the form the
 * loop takes - 4 096 (i.e. the whole search in one call) where the search runs from cached lag sums, 64 for short sessions
 * (one launch, a workgroup per keypoint), 16 where every iteration is its own launch on scalar chains (an over-issued
 * iteration is a launch that returns at once), 4 on the general (D, O) path (an over-issued iteration is a full
 * evaluation).  No reference counterpart (the reference's loop is one XLA while_loop, eks/core.py:654-681). */
int32_t eks_adam_run_stride(const eks_dims_t* dims, int32_t n_blocks);

/* ---- IBL pupil smoother, eks/ibl_pupil_smoother.py:363-607.
 * Independent chains k < n_keypoints (one per session), AR(1) dynamics A_k = diag(a[k][:]),
 * process noise diag(q[k][:]), observation matrix C [K][O][D], TIME-VARYING R_t = diag(max(var,
 * 1e-12)) also in the loss (:514-518).  eks_ar1_nll: nll[k] = -marginal_loglik of the filter
 * (_nll_from_u, :540-552); with n_tan > 0, dnll[i][k] = derivative of nll[k] along the tangent
 * (da[i][k][:], dq[i][k][:]) - forward sensitivities replacing jax.value_and_grad (:570); with
 * EKS_FLAG_Q_PD (q > 0 in every coordinate) on the pupil's shape D = 3, O = 8 the same derivatives
 * come from the smoothing distribution inside the smoother's kernels.  The
 * final smoothing pass is eks_smooth with A = diag(a), Q = diag(q), s = 1 (:427-445). -------- */
size_t eks_ar1_nll_workspace_bytes(const eks_dims_t* dims, int32_t n_tan);
int eks_ar1_nll(const eks_dims_t* dims, const float* y, const float* var, const double* m0,
                const double* S0, const double* C, const double* a, const double* q,
                const double* da, const double* dq, int32_t n_tan, double* nll, double* dnll,
                void* workspace, size_t workspace_bytes, eks_stream_t stream);

/* ---- one iteration of the pupil optimiser per chain (:560-594): optax.adam(lr) (b1 .9, b2 .999,
 * eps 1e-8, bias-corrected) on u = (u_diam, u_com) with the gradient dnll [2][n] w.r.t. u, then
 * done = isfinite(prev) && |L - prev| < tol * |log(max(prev, 1e-12))| + 1e-6; prev = L; ++iters.
 * Chains that are done or at safety_cap are left untouched.  state is [n][9] float64
 * {u_d, u_c, mom_d, mom_c, vel_d, vel_c, prev_loss, iters, done}.  Always (re)writes the inputs
 * of the next eks_ar1_nll call from u: s = sigmoid(u) * (1 - 2e-3) + 1e-3 (:506-508),
 * a [n][3] = (s_d, s_c, s_c), q [n][3] = latent_var * (1 - a^2), and the two tangents
 * da, dq [2][n][3] = d(a, q)/du_d, d(a, q)/du_c.  nll == NULL: only that (initialisation).
 * *n_active = number of chains still running after this step. ------------------------------- */
int eks_pupil_adam_step(int32_t n_chains, const double* latent_var, const double* nll,
                        const double* dnll, double lr, double tol, int32_t safety_cap,
                        double* state, double* a, double* q, double* da, double* dq,
                        int32_t* n_active, eks_stream_t stream);

/* ---- n_iters iterations of { eks_ar1_nll (2 tangents) -> eks_pupil_adam_step } enqueued back to
 * back (the while_loop of :571-594).  a, q, da, dq must have been initialised by
 * eks_pupil_adam_step(nll = NULL).  nll [n], dnll [2][n] hold the last evaluation.
 * workspace: eks_ar1_nll_workspace_bytes(dims, 2). ------------------------------------------ */
int eks_pupil_adam_run(const eks_dims_t* dims, const float* y, const float* var, const double* m0,
                       const double* S0, const double* C, const double* latent_var, double lr,
                       double tol, int32_t safety_cap, int32_t n_iters, double* state, double* a,
                       double* q, double* da, double* dq, double* nll, double* dnll,
                       int32_t* n_active, void* workspace, size_t workspace_bytes,
                       eks_stream_t stream);

/* ---- extended Kalman filter / smoother with calibrated pinhole cameras (SURVEY.md section 8(f)
 * rank 3): run_kalman_smoother(h_fn = multi-camera projection), eks/core.py:188-190, :274-295, as
 * called from eks/multicam_smoother.py:369-407; the projection is make_jax_projection_fn (:814-868)
 * with its analytic Jacobian in place of jax.jacfwd.  State dim 3, obs dim 2 * n_cams (u, v per
 * camera).
 *   dims.n_keypoints = number of CHAINS K; chain k reads the observations of keypoint
 *   k % n_data_keypoints (several chains per keypoint = several values of s over the same data,
 *   which is how the optimiser takes central differences in log s).
 *   y [T][Kd][O] float32; exactly one of var [T][Kd][O] float32 (time-varying R_t = diag(max(var,
 *   1e-12)), final pass) and rconst [Kd][O] float64 (constant R, the loss of :640-650) is non-NULL.
 *   m0 [K][3], S0, A, Q [K][3][3], s [K] per chain.  cams [n_cams][32] float64: R row-major (9),
 *   t (3), fx, fy, cx, cy, skew, then the 14 OpenCV-ordered distortion coefficients k1 k2 p1 p2 k3
 *   k4 k5 k6 s1 s2 s3 s4 tx ty (radial POLYNOMIAL in r^2 as in the reference; tx, ty ignored), pad.
 *   xlin [K][T][3] float64, in/out: the linearisation points (predicted means).  On entry any
 *   finite guess (the prior mean, a triangulation, the previous call's result); on return the
 *   extended filter's predicted means.  The filter is solved as a fixed point over xlin by at
 *   most max_sweeps (<= 64) gated scan sweeps, stopping once no point moves by more than tol
 *   (relative to max(1, |x|)); info[0] = sweeps executed, info[1] = last such change (the result
 *   equals the sequential extended filter's when info[1] <= tol).
 *   ms [T][K][3], Vs [T][K][3][3] (or [T][K][3] with EKS_FLAG_VS_DIAG) float32 smoothed outputs;
 *   ms == NULL: filter only.  nll [K] = -marginal log-likelihood (may be NULL). -------------- */
size_t eks_ekf_smooth_workspace_bytes(const eks_dims_t* dims, int32_t want_smoother);
int eks_ekf_smooth(const eks_dims_t* dims, int32_t n_data_keypoints, const float* y,
                   const float* var, const double* rconst, const double* m0, const double* S0,
                   const double* A, const double* Q, const double* s, const double* cams,
                   int32_t n_cams, double* xlin, int32_t max_sweeps, double tol, float* ms,
                   float* Vs, double* nll, double* info, void* workspace, size_t workspace_bytes,
                   eks_stream_t stream);

/* ---- ONE sweep of the extended Kalman filter / smoother for a user-supplied differentiable emission
 * function: run_kalman_smoother(h_fn = any y_t = h(x_t)), eks/core.py:159-177, :188-190.  The kernels
 * cannot call the user's function; the caller tabulates its linearisation at the current linearisation
 * points X (xlin) and this runs the linear time-varying filter y_t = J_t x_t + c_t + v_t of those tables:
 *   jac [T][K][O][D] float64: J_t = dh/dx at X_t, per chain, frame-major;
 *   off [T][K][O] float64: c_t = h(X_t) - J_t X_t.
 * Repeating (tabulate at xlin, sweep) until *change <= tol is the fixed point at which the result equals
 * the sequential extended filter's (eks_amd/core.py drives the loop).  1 <= D <= 6, 1 <= O <= 64.
 *   dims.n_keypoints = number of CHAINS K; chain k reads the observations of keypoint
 *   k % n_data_keypoints (as eks_ekf_smooth).  y [T][Kd][O] float32; exactly one of var [T][Kd][O]
 *   float32 (time-varying R_t = diag(max(var, 1e-12))) and rconst [Kd][O] float64 (constant R).
 *   m0 [K][D], S0, A, Q [K][D][D], s [K] per chain.
 *   xlin [K][T][D] float64, in/out: the points the tables were built at; on return the filter's
 *   predicted means (the next sweep's points; a non-finite prediction keeps the old point).
 *   ms [T][K][D], Vs [T][K][D][D] (or [T][K][D] with EKS_FLAG_VS_DIAG) float32 smoothed outputs;
 *   ms == NULL: filter only.  nll [K] = -marginal log-likelihood of the sweep's filter (may be NULL);
 *   change [1] = largest change of a point relative to max(1, |x|) (may be NULL).
 * Missing tables: EKS_ERR_SHAPE; D or O outside the limits: EKS_ERR_UNSUPPORTED.
 * workspace: eks_ekf_affine_workspace_bytes(dims, ms != NULL). --------------------------------- */
size_t eks_ekf_affine_workspace_bytes(const eks_dims_t* dims, int32_t want_smoother);
int eks_ekf_affine_sweep(const eks_dims_t* dims, int32_t n_data_keypoints, const float* y,
                         const float* var, const double* rconst, const double* m0, const double* S0,
                         const double* A, const double* Q, const double* s, const double* jac,
                         const double* off, double* xlin, float* ms, float* Vs, double* nll,
                         double* change, void* workspace, size_t workspace_bytes, eks_stream_t stream);

/* ---- ensemble statistics, eks/core.py:25-101: markers float32 [M][V][T][K][3] (x,y,likelihood)
 * -> stats float32 [V][T][K][5] (x, y, var_x, var_y, likelihood).  avg_mode 0 median / 1 mean,
 * var_mode 0 confidence_weighted_var / 1 var. ------------------------------------------------ */
int eks_ensemble(int32_t n_models, int32_t n_cameras, int32_t n_frames, int32_t n_keypoints,
                 const float* markers, int32_t avg_mode, int32_t var_mode, float nan_replacement,
                 float* stats, eks_stream_t stream);

/* ---- variance inflation, one pass of the loop of
 * eks/multicam_smoother.py:695-708 for every ACTIVE keypoint: the per-frame factor-analysis
 * reconstruction residual and per-view 2x2 Mahalanobis distance of compute_mahalanobis
 * (eks/stats.py:119-151) given the loading matrix W and mean mu, then inflate_variance
 * (eks/multicam_smoother.py:724-764): v *= scalar for every (frame, view) whose distance exceeds
 * threshold, the whole frame when n_views == 2.  The factor-analysis fit between passes stays on
 * the host.  x [K][N][2C] float64 (centred predictions, stacked views c0x c0y c1x ...),
 * v [K][N][2C] float32 in/out, W [K][2C][L], mu [K][2C] float64, active [K] (NULL = all),
 * maha [K][N][C] float64 out (may be NULL), n_inflated [K] out = number of frames with a hit
 * (0 = this keypoint's loop is finished).  2 <= C <= 8, 1 <= L <= 6. ------------------------- */
int eks_maha_inflate(int32_t n_keypoints, int32_t n_frames, int32_t n_views, int32_t n_latent,
                     const double* x, float* v, const double* W, const double* mu,
                     const int32_t* active, double epsilon, double threshold, double scalar,
                     double* maha, int32_t* n_inflated, eks_stream_t stream);

/* ---- output epilogue of the linear multi-camera driver (eks/multicam_smoother.py:481-544):
 * stats [V][T][K][5] float32 (eks_ensemble's x, y, var_x, var_y, likelihood), ev [T][K][2V]
 * float32 (the variances the filter used, possibly inflated), ms [T][K][D], Vs [T][K][D][D]
 * float32 (eks_smooth), C [K][2V][D], mean [V][K][2] float64 ->
 * tables [V][T][K][9] float64: x, y = C m + mean | likelihood | x, y ensemble average |
 * x, y ensemble variance (= ev, :505-508) | x, y posterior variance = diag(C V C') + ev (:509-510);
 * latent [T][K][2D] float64 = (m, diag V) (:529-544; may be NULL).  D <= 6. ------------------ */
int eks_multicam_tables(int32_t n_views, int32_t n_frames, int32_t n_keypoints, int32_t state_dim,
                        const float* stats, const float* ev, const float* ms, const float* Vs,
                        const double* C, const double* mean, double* tables, double* latent,
                        eks_stream_t stream);

/* ---- optional per-kernel timing (used by bench.py's roofline object).  on = 1: each kernel launch
 * (stage) is bracketed by hipEvents on the caller's stream; on = 2: only the roofline kernels - the
 * smoother's replay kernels (HBM-bound) and the NLL grid kernel (VALU-bound); 0: off. eks_profile_drain waits for the
 * recorded events, writes up to max_n NUL-terminated kernel names back to back into `names` and
 * their durations in milliseconds into `ms`, clears the record and returns the count. -------- */
int eks_profile_enable(int on);
int eks_profile_drain(char* names, size_t names_bytes, float* ms, int32_t max_n);

/* ---- first-call latency.  The HIP runtime loads a translation unit's code object (1-3 MB each here) the first
 * time one of its kernels is launched, so the FIRST call of a process into each part of the library pays tens of
 * milliseconds of loading on top of its kernels - for the reference's own 2 000-frame recordings that is the whole
 * run time.  eks_warmup loads the units named in `units` now (no kernel runs, no device memory is touched; needs a
 * current device) so that a caller - e.g. on a background thread while its CSV files parse - takes the cost off its
 * first smoothing call.  ms_per_unit (optional, 9 floats, bit order) receives each unit's load time.  No reference
 * counterpart (XLA compiles on first call instead: eks/core.py:585-588 mentions "28 separate XLA compilations"). */
#define EKS_WARM_MISC 1u        /* eks_const_r, eks_ensemble, eks_order_stats, eks_argmin_s, eks_adam_step */
#define EKS_WARM_DIAG 2u        /* eks_smooth on scalar chains (EKS_FLAG_DIAG_MODEL) */
#define EKS_WARM_DIAG_NLL 4u    /* eks_nll / eks_adam_run on scalar chains */
#define EKS_WARM_DENSE 8u       /* general (D, O): scan, generic summarize / replay, eks_ekf_smooth */
#define EKS_WARM_DENSE_WAVE 16u /* general (D, O), narrow sessions (and their smoothing-distribution gradient) */
#define EKS_WARM_DENSE_WIDE 32u /* general (D, O), wide sessions */
#define EKS_WARM_LOSS 64u       /* eks_nll on the general path (dual numbers) */
#define EKS_WARM_LOSS_AR1 128u  /* eks_ar1_nll (pupil) */
#define EKS_WARM_MULTICAM 256u  /* eks_maha_inflate, eks_multicam_tables */
#define EKS_WARM_ALL 511u
int eks_warmup(uint32_t units, float* ms_per_unit);

/* ---- measurement hook.  The EKS_* tuning variables (alternative kernel
 * organisations kept for A/B runs; none is needed in use) are read ONCE, on the first call into the
 * library, never per call.  eks_knobs_reload re-reads them (a test that flips a variable between two
 * calls of one process); not to be called while another thread is inside the library.  Returns the
 * number of EKS_* variables found set.  No reference counterpart. ------------------------------ */
int eks_knobs_reload(void);

/* ---- HOST-side helpers of the boundary (no device code, no stream: they return when done) ------------------------
 * eks_csv_read_numeric: the numeric body of a prediction CSV - what `pd.read_csv(path, header=[0, 1, 2], index_col=0)`
 * (reference eks/utils.py:188; the 3 header rows are skip_lines) parses field by field - into out[n_rows][n_cols]
 * float64, EVERY column including the index column, blank lines skipped, empty fields and pandas' default NA strings
 * -> NaN, [+-]inf / infinity accepted.  The decimal -> double conversion is pandas' own default (its tokenizer's
 * precise_xstrtod: <= 17 significant digits, one multiplication / division by a power of ten), so the values are the
 * ones pandas returns, bit for bit.  out == NULL: size query (n_rows_out, n_cols_out only).  col_is_int (optional,
 * n_cols bytes): 1 where every field of the column was written as an integer (pandas gives such a column dtype int64).
 * n_threads: blocks of lines parsed concurrently (std::thread).  Returns EKS_OK, EKS_CSV_FALLBACK (see above; also for
 * integers beyond 2^53), EKS_CSV_IO, EKS_ERR_NULL, EKS_ERR_WORKSPACE (capacity < n_rows * n_cols). ------------------- */
int eks_csv_read_numeric(const char* path, int32_t skip_lines, double* out, int64_t capacity, int64_t* n_rows_out,
                         int32_t* n_cols_out, uint8_t* col_is_int, int32_t col_capacity, int32_t n_threads);

/* eks_csv_write_table: `DataFrame.to_csv(path)` of a float64 table with an int64 index, byte for byte (the result
 * tables of fit_eks_*: reference eks/singlecam_smoother.py:98-99, eks/multicam_smoother.py:151-152, :270-275): `header`
 * (header_bytes of text, newline included: the caller takes it from pandas - the empty slice's to_csv) followed by one
 * line per row, "index,v0,v1,...": every number as Python's repr (the shortest decimal string that reads back as the
 * same double; fixed notation for decimal exponents -4 .. 15, d.ddde+XX otherwise), a NaN as the empty field, inf /
 * -inf as such.  values [n_rows][n_cols] row-major.  Row blocks are formatted on n_threads threads and written in
 * order.  eks_format_repr (test hook): the text of n doubles concatenated into out, offsets [n + 1]. --------------- */
int eks_csv_write_table(const char* path, const char* header, int64_t header_bytes, const int64_t* index,
                        const double* values, int64_t n_rows, int32_t n_cols, int32_t n_threads);
int eks_format_repr(const double* values, int64_t n, char* out, int64_t capacity, int64_t* offsets);

/* eks_host_thread_speedup: how many times faster n_threads threads of this process finish n_threads units of work than
 * one thread finishes one (a ~1 ms measurement; a sandbox may expose several CPUs and still run a process's threads
 * one at a time).  The Python wrapper asks once and takes the threaded writer only where threads run side by side. -- */
double eks_host_thread_speedup(int32_t n_threads);

/* eks_host_model_flags: the EKS_FLAG_DIAG_MODEL / EKS_FLAG_UNIT_AC / EKS_FLAG_Q_PD bits that HOST copies of the parameters
 * S0, A, Q [K][D][D] and C [K][O][D] allow (what run_kalman_smoother decides before its first launch; the reference has
 * no counterpart - eks/core.py:159-177 hands whatever it is given to dynamax): DIAG_MODEL when D == O and every matrix
 * is diagonal, UNIT_AC when also A = C = I, Q_PD when every Q[k] is finite with lambda_min > min_eig_ratio x lambda_max.
 * Returns the flags (>= 0); EKS_ERR_UNSUPPORTED when Q is finite but NOT diagonal (its eigenvalues decide Q_PD: the
 * caller asks LAPACK). ---------------------------------------------------------------------------------------------- */
int eks_host_model_flags(int32_t n_keypoints, int32_t state_dim, int32_t obs_dim, const double* S0, const double* A,
                         const double* C, const double* Q, double min_eig_ratio);

/* eks_host_gather_cols: dst[r][0 .. width) = src[r][col_offset .. col_offset + width) (bytes) for n_rows rows of a
 * row-major HOST matrix with rows of src_row_bytes, on n_threads threads: a keypoint tile of the frame-major ensemble
 * variances (T, K, O) (reference eks/core.py:159-177 takes them in that layout) made contiguous for its upload. ---- */
int eks_host_gather_cols(const void* src, int64_t n_rows, int64_t src_row_bytes, int64_t col_offset_bytes,
                         int64_t width_bytes, void* dst, int32_t n_threads);

#ifdef __cplusplus
}
#endif
#endif /* EKS_HIP_H */
