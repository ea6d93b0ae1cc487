/*
 * asr_hip.h -- C ABI of libasr_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * Augmented Super-Resolution hot path of nicoloalbergoni/DeepLabV3Plus-Augmented-SuperResolution.
 *
 * The reference is 100 % Python on TensorFlow 2.7 / tensorflow-addons 0.15 and has no FFI or
 * operator-plugin interface; each entry point below replaces one (group of) stock TF/TFA/Keras
 * op call site(s), cited as file:line relative to the reference checkout.  A Python
 * maintainer binds them with ctypes.
 *
 * Conventions
 *  - every function returns int: ASR_OK (0) or a negative ASR_ERR_*; asr_last_error() returns a
 *    thread-local message for the last failing call on this thread;
 *  - all array pointers are CALLER-OWNED DEVICE pointers (hipMalloc / torch ROCm tensors); the
 *    library allocates nothing and keeps no unsynchronised global state -- its only caches (a kernel's dynamic-LDS
 *    allowance, a device's CU count) are per-device atomics, and no environment variable changes which kernel runs --
 *    so it is callable from several host threads / streams / devices concurrently; scratch space is passed in explicitly;
 *  - every call takes an explicit stream (hipStream_t passed as void*) and is asynchronous
 *    with respect to the host;
 *  - layouts are dense row-major float32, images NHWC; "ld*" arguments are the element stride
 *    between consecutive pixels (>= channels) so outputs can land inside concat buffers;
 *  - projective transforms are 8 floats [a0,a1,a2,b0,b1,b2,c0,c1] exactly as
 *    ImageProjectiveTransformV3 takes them (output pixel (x,y) reads input at
 *    ((a0 x + a1 y + a2)/k, (b0 x + b1 y + b2)/k), k = c0 x + c1 y + 1), BILINEAR, out-of-range
 *    taps read 0.
 */
#ifndef ASR_HIP_H
#define ASR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASR_ABI_VERSION 3

#define ASR_OK 0
#define ASR_ERR_INVALID_ARG (-1)
#define ASR_ERR_UNSUPPORTED (-2)
#define ASR_ERR_HIP (-3)
#define ASR_ERR_WORKSPACE (-4)

typedef void* asr_stream_t; /* hipStream_t */

const char* asr_last_error(void);
int asr_abi_version(void);
const char* asr_target_arch(void);

/* ------------------------------------------------------------------------------------------
 * Augmentation / warps
 * ------------------------------------------------------------------------------------------ */

/* One ImageProjectiveTransformV3 pass.  Replaces tfa.image.rotate / tfa.image.translate
 * (superresolution_scripts/augmentation_utils.py:22-25, superresolution.py:61-64,142-147).
 * src [n or 1, h_in, w_in, c] (src_batched = 0: one shared source), transforms [n or 1, 8]
 * (tf_batched = 0: one shared transform), dst [n, h_out, w_out, c]. */
int asr_warp_affine_f32(const float* src, float* dst, const float* transforms, int n, int src_batched,
                        int tf_batched, int h_in, int w_in, int h_out, int w_out, int c, asr_stream_t stream);

/* The same pass with interpolation "NEAREST" (tfa.image.rotate / translate of the label maps,
 * check_robustness.py:45-50): dst = src(round(in_y), round(in_x)) with std::round, 0 outside. */
int asr_warp_affine_nearest_f32(const float* src, float* dst, const float* transforms, int n, int src_batched,
                        int tf_batched, int h_in, int w_in, int h_out, int w_out, int c, asr_stream_t stream);

/* copies[i] = translate(rotate(image, rot_tf[i]), trans_tf[i]) -- tile + two bilinear resamplings
 * fused (superresolution_scripts/augmentation_utils.py:12-25 create_augmented_copies; :46-54
 * chunked variant).  image [h,w,c] (c = 1 or 3), copies [n,h,w,c], rot_tf / trans_tf [n,8]. */
int asr_augment_copies_f32(const float* image, float* copies, const float* rot_tf, const float* trans_tf, int n,
                           int h, int w, int c, asr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Super-resolution solver (superresolution_scripts/superresolution.py, optimizer.py)
 * x [batch,H,W]; y / resid [batch,n,h,w]; transforms [batch,n,8]: any ImageProjectiveTransformV3 vector (the
 * reference builds rotations and pure translations, which take fast paths; affine-but-not-pure and projective
 * vectors take generic branches with the same arithmetic), the inv_* ones used as given.
 * Shapes: asr_sr_forward_residual_f32, asr_sr_backward_*, asr_sr_solve_* need H = f*h, W = f*w with ONE even
 * factor f >= 2 for both axes; anything else (odd f, f = 1, unequal factors, a non-multiple) returns
 * ASR_ERR_UNSUPPORTED before anything is launched or written.  asr_sr_init_target_f32 and asr_realign_* resize
 * with TF's half-pixel bilinear rule at any ratio: every positive H, W, h, w is accepted.
 * ------------------------------------------------------------------------------------------ */

/* x = tf.image.resize(y[:, 0], (H, W)) -- superresolution.py:112-113. */
int asr_sr_init_target_f32(const float* y, float* x, int batch, int n, int H, int W, int h, int w,
                           asr_stream_t stream);

/* resid[b,i] = resize(translate(rotate(tile(x_b), rot_tf), trans_tf), (h,w))[i] - y[b,i]
 * -- the forward model of loss_function, superresolution.py:58-72. */
int asr_sr_forward_residual_f32(const float* x, const float* y, const float* rot_tf, const float* trans_tf,
                                float* resid, int batch, int n, int H, int W, int h, int w, asr_stream_t stream);

/* One optimiser step: gradient of the loss (TensorFlow's registered gradients: SquaredDifference,
 * ResizeBilinearGrad, ImageProjectiveTransformV3 gradient = inverse warp with inv_*_tf, Tile
 * sum; TV / L2 / L1 priors, superresolution.py:71-98,133) followed by the Keras Adam / AMSGrad
 * update (optimizer.py:37-41, superresolution.py:134-135).  alphas [batch] =
 * lr_t * sqrt(1 - beta2^t) / (1 - beta1^t) per image.  x_new must not alias x.  grad_out
 * (optional) receives the raw gradient; with x_new == NULL only grad_out is produced. */
int asr_sr_backward_adam_f32(const float* x, float* x_new, const float* resid, const float* inv_rot_tf,
                             const float* inv_trans_tf, float* m, float* v, float* vhat, const float* alphas,
                             float* grad_out, int batch, int n, int H, int W, int h, int w, float lambda_df,
                             float lambda_tv, float lambda_l2, float lambda_l1, float one_minus_beta1,
                             float one_minus_beta2, float epsilon, int amsgrad, asr_stream_t stream);

/* terms[b] = {sum resid^2, TV(x), sum x^2, sum |x|} in float64 -- the pieces of the scalar loss
 * of superresolution.py:71-98 (reporting only). */
int asr_sr_loss_terms_f64(const float* x, const float* resid, double* terms, int batch, int n, int H, int W, int h,
                          int w, asr_stream_t stream);

/* Bytes of caller-owned workspace asr_sr_solve_f32 needs (residuals, the ping-pong x, the running data-term sum and the
 * zero-bordered gradient planes of one chunk of copies; library default chunking, see asr_sr_config.plane_chunk). */
size_t asr_sr_solve_workspace_bytes(int batch, int n, int H, int W, int h, int w);

/* The whole loop of augmented_superresolution (superresolution.py:120-135): num_iter x
 * {forward residual, backward + Adam}.  x holds the initial target on entry and the result on
 * exit; m / v / vhat [batch,H,W] are the optimiser slots (zero for a fresh variable); alphas
 * [num_iter, batch] (device); last_loss_terms [batch,4] float64 (optional) receives the loss
 * pieces of the last iteration, evaluated before its update like the reference's `loss`. */
int asr_sr_solve_f32(float* x, const float* y, const float* rot_tf, const float* trans_tf, const float* inv_rot_tf,
                     const float* inv_trans_tf, float* m, float* v, float* vhat, const float* alphas, int num_iter,
                     double* last_loss_terms, void* workspace, size_t workspace_bytes, int batch, int n, int H, int W,
                     int h, int w, float lambda_df, float lambda_tv, float lambda_l2, float lambda_l1,
                     float one_minus_beta1, float one_minus_beta2, float epsilon, int amsgrad, asr_stream_t stream);

/* --- the other optimisers and priors of the reference's sweeps -----------------------------------------------
 * optimizer.py:21-41 lets sweep_all.yaml pick Adadelta / Adagrad / Adamax / SGD besides Adam, and
 * superresolution.py:8-23,81-82 swaps the TV prior for bilateral TV (use_BTV).  asr_sr_config selects them for
 * the *_cfg entry points below; the *_adam_f32 / asr_sr_solve_f32 / asr_sr_loss_terms_f64 functions above are the
 * {ASR_OPT_ADAM, ASR_PRIOR_TV} case.  Update rules are the dense CPU kernels of tensorflow 2.7
 * (core/kernels/training_ops.cc) that the Keras optimisers dispatch to; `alphas` carries the per-step scalar:
 *
 *   optimizer          slots used (zero-initialised unless noted)      c0          c1          c2        alphas[it,b]
 *   ASR_OPT_ADAM       m, v, vhat (flag = amsgrad)                     1 - beta1   1 - beta2   epsilon   lr_t sqrt(1-beta2^t)/(1-beta1^t)
 *   ASR_OPT_SGD        m = momentum accumulator (flag = nesterov)      momentum    -           -         lr_t
 *   ASR_OPT_ADAGRAD    v = accumulator (init initial_accumulator_value) -          -           epsilon   lr_t
 *   ASR_OPT_ADADELTA   v = accum, m = accum_update                     rho         1 - rho     epsilon   lr_t
 *   ASR_OPT_ADAMAX     m, v                                            1 - beta1   beta2       epsilon   lr_t / (1 - beta1^t)
 *   ASR_OPT_PRIMAL_DUAL  m = p_y, v = p_x (the solves only; see "primal-dual" below)   dual ratio  -   -         tau
 */
#define ASR_OPT_ADAM 0
#define ASR_OPT_SGD 1
#define ASR_OPT_ADAGRAD 2
#define ASR_OPT_ADADELTA 3
#define ASR_OPT_ADAMAX 4
#define ASR_OPT_PRIMAL_DUAL 5
#define ASR_PRIOR_TV 0
#define ASR_PRIOR_BTV 1

typedef struct asr_sr_config {
    int optimizer;     /* ASR_OPT_* */
    int flag;          /* Adam: amsgrad; SGD: nesterov */
    float c0, c1, c2;  /* see the table above */
    int prior;         /* ASR_PRIOR_TV: tf.image.image_gradients TV; ASR_PRIOR_BTV: bilateral_tv */
    float btv_alpha;   /* bilateral_tv(alpha=0.6, ...) */
    int btv_shift;     /* bilateral_tv(shift_factor=2): pairs (h, v), h in [-s, s], v in [0, s]; 1 <= s <= 4 */
    int plane_chunk;   /* asr_sr_solve_*: copies whose per-copy gradient planes are alive at once (a K_gt + K_bwd launch pair
                        * per chunk, the data-term sum carried across in copy order: results do not depend on it).
                        * 0 = library default (all copies at once while the planes stay under 1 GiB per call -- the fastest
                        * form on every measured shape --, an even split beyond); >= n = all copies at once. */
} asr_sr_config;

/* asr_sr_backward_adam_f32 with the update rule and prior of `cfg` (host pointer, read during the call). */
int asr_sr_backward_cfg_f32(const float* x, float* x_new, const float* resid, const float* inv_rot_tf,
                            const float* inv_trans_tf, float* m, float* v, float* vhat, const float* alphas,
                            float* grad_out, int batch, int n, int H, int W, int h, int w, float lambda_df,
                            float lambda_tv, float lambda_l2, float lambda_l1, const asr_sr_config* cfg,
                            asr_stream_t stream);

/* asr_sr_loss_terms_f64 with terms[b][1] = the prior selected by cfg (TV or bilateral TV). */
int asr_sr_loss_terms_cfg_f64(const float* x, const float* resid, double* terms, int batch, int n, int H, int W,
                              int h, int w, const asr_sr_config* cfg, asr_stream_t stream);

/* asr_sr_solve_workspace_bytes for asr_sr_solve_cfg_f32 with this cfg (its plane_chunk decides the size). */
size_t asr_sr_solve_workspace_bytes_cfg(int batch, int n, int H, int W, int h, int w, const asr_sr_config* cfg);

/* asr_sr_solve_f32 with the update rule and prior of `cfg`. */
int asr_sr_solve_cfg_f32(float* x, const float* y, const float* rot_tf, const float* trans_tf, const float* inv_rot_tf,
                         const float* inv_trans_tf, float* m, float* v, float* vhat, const float* alphas, int num_iter,
                         double* last_loss_terms, void* workspace, size_t workspace_bytes, int batch, int n, int H, int W,
                         int h, int w, float lambda_df, float lambda_tv, float lambda_l2, float lambda_l1,
                         const asr_sr_config* cfg, asr_stream_t stream);

/* --- edge-weighted (image-guided) TV ---------------------------------------------------------------------------
 * The TV prior charges every unit of boundary the same; the weighted form makes a jump of the solution cheap across an
 * edge of the RGB image and full price elsewhere (the guided depth / label super-resolution prior).  The rule:
 *
 *   Edge weights.  guide I [batch, H, W, 3] float32 (the project's images, in [0, 1]; values are not checked), beta finite, >= 0.
 *     Y < H-1:  a_c = I[Y+1,X,c] - I[Y,X,c];  d = (a_0*a_0 + a_1*a_1) + a_2*a_2  in float32, in that order, no contraction;
 *               wy[Y,X] = 1.0f / (1.0f + beta*d), one IEEE division.      wy[H-1,X] = 1.0f.
 *     wx the same with X+1;  wx[Y,W-1] = 1.0f.  beta = 0 or a constant guide: every weight is exactly 1.
 *   Prior.  TV_w(x) = sum wy*|x[Y+1,X] - x[Y,X]| + wx*|x[Y,X+1] - x[Y,X]|; the gradient is the TV prior's statements with
 *     each lambda_tv replaced by (lambda_tv * w) of the edge it belongs to:
 *       sy   = (Y < H-1) ? sgn(x[Y+1,X] - xc) * (lambda_tv * wy[Y,X]) : 0
 *       sx   = (X < W-1) ? sgn(x[Y,X+1] - xc) * (lambda_tv * wx[Y,X]) : 0
 *       g_tv = -sy - sx
 *       if (Y > 0) g_tv += sgn(xc - x[Y-1,X]) * (lambda_tv * wy[Y-1,X])
 *       if (X > 0) g_tv += sgn(xc - x[Y,X-1]) * (lambda_tv * wx[Y,X-1])
 *     L2, L1 and every optimiser follow unchanged.  terms[b][1] accumulates (double)(wy*fabsf(dy) + wx*fabsf(dx)): product
 *     and sum in float32, the accumulation in float64 as for TV.
 *   The *_wtv entry points take ANY finite weights >= 0 (not only asr_tv_edge_weights_f32's): wy, wx [H, W] shared by the
 *   whole batch (w_shared != 0: the K classes of one image) or [batch, H, W].  Hence, bit for bit: weights of all ones are
 *   the TV prior (lambda_tv * 1.0f is lambda_tv), weights of all zeros are lambda_tv = 0, shared planes are the same planes
 *   broadcast.  Refusals, before any launch: every refusal of the *_cfg twin; null wy / wx -> ASR_ERR_INVALID_ARG;
 *   cfg->prior == ASR_PRIOR_BTV -> ASR_ERR_UNSUPPORTED (bilateral TV has no weighted form here). */
int asr_tv_edge_weights_f32(const float* guide, float* wy, float* wx, int batch, int H, int W, float beta,
                            asr_stream_t stream);

/* asr_sr_backward_cfg_f32 with the edge-weighted TV prior. */
int asr_sr_backward_wtv_f32(const float* x, float* x_new, const float* resid, const float* inv_rot_tf,
                            const float* inv_trans_tf, float* m, float* v, float* vhat, const float* alphas,
                            float* grad_out, int batch, int n, int H, int W, int h, int w, float lambda_df,
                            float lambda_tv, float lambda_l2, float lambda_l1, const asr_sr_config* cfg, const float* wy,
                            const float* wx, int w_shared, asr_stream_t stream);

/* asr_sr_loss_terms_cfg_f64 with terms[b][1] = TV_w(x). */
int asr_sr_loss_terms_wtv_f64(const float* x, const float* resid, double* terms, int batch, int n, int H, int W,
                              int h, int w, const asr_sr_config* cfg, const float* wy, const float* wx, int w_shared,
                              asr_stream_t stream);

/* asr_sr_solve_cfg_f32 with the edge-weighted TV prior; the workspace is that of asr_sr_solve_workspace_bytes_cfg. */
int asr_sr_solve_wtv_f32(float* x, const float* y, const float* rot_tf, const float* trans_tf, const float* inv_rot_tf,
                         const float* inv_trans_tf, float* m, float* v, float* vhat, const float* alphas, int num_iter,
                         double* last_loss_terms, void* workspace, size_t workspace_bytes, int batch, int n, int H, int W,
                         int h, int w, float lambda_df, float lambda_tv, float lambda_l2, float lambda_l1,
                         const asr_sr_config* cfg, const float* wy, const float* wx, int w_shared, asr_stream_t stream);

/* --- data term: L1, Huber and per-measurement weights -----------------------------------------------------------
 * The solver's data term above is sum (D(T(R(x))) - y)^2: every low-resolution pixel of every copy counts the same and a
 * copy on which the network failed pulls with the square of its error.  The *_dt entry points minimise sum w * rho(r)
 * instead (the reference carries the L1 form commented out, superresolution.py:73).  The rule, for the residual
 * r = D(T(R(x))) - y in float32, exactly what asr_sr_forward_residual_f32 writes:
 *
 *   loss                          rho(r)                                          psi(r) = rho'(r) / 2
 *   ASR_DF_L2                     r*r                                             r
 *   ASR_DF_L1                     |r|                                             r > 0 ? 0.5f : (r < 0 ? -0.5f : +0.0f)
 *   ASR_DF_HUBER, delta in (0,inf) |r| <= delta ? r*r : delta*(2|r| - delta)      r < -delta ? -delta : (r > delta ? delta : r)
 *
 *   q = w * psi(r), ONE float32 multiply, left out entirely without weights (w = 1 gives the same bits).  The forward kernel
 *   writes q where it wrote r, and every backward kernel reads that buffer as before, as (2*lambda_df * q) * 0.25f: no backward
 *   kernel knows about the data term, and one explicit step feeds q to asr_sr_backward_cfg_f32 / _wtv_f32 as `resid`.  Under L1
 *   the data gradient is that of lambda_df * |r| (2*lambda_df and 0.5 are exact in float32): TF's own gradient of the
 *   commented-out line.  Huber with delta >= max |r| is L2 bit for bit; so is a weight plane of all ones; a copy whose weights
 *   are all zero adds +-0 to every sum it enters.  A NaN residual stays NaN under L2 and Huber and gives psi = +0 under L1.
 *   Weights: any finite values >= 0 (not checked), [batch, n, h, w], or [n, h, w] shared by the batch (weights_shared != 0: the
 *   K classes of one image); NULL: unweighted.
 *   terms[b][0] = sum w * rho(r) over the RAW residual: each term in float32, one operation per statement as written above
 *   (then the weight), the accumulation in float64.  The other three terms do not change.
 *   wy, wx: both NULL for the plain TV or bilateral-TV prior of cfg, or the edge weights of the *_wtv calls (tv_shared as
 *   their w_shared).  Refusals, before any launch, outputs untouched: every refusal of the *_cfg / *_wtv twin; dt NULL, an
 *   unknown loss, Huber with delta not finite or <= 0, one of wy / wx NULL, weights with n, h or w <= 0 -> ASR_ERR_INVALID_ARG. */
#define ASR_DF_L2 0
#define ASR_DF_L1 1
#define ASR_DF_HUBER 2

typedef struct asr_sr_data_term {
    int loss;              /* ASR_DF_* */
    float delta;           /* Huber's threshold, in the units of y; read under ASR_DF_HUBER only */
    const float* weights;  /* device; NULL = unweighted */
    int weights_shared;    /* != 0: weights are [n, h, w], the same for every image of the batch */
    const float* wy;       /* edge-weighted TV planes (device), or both NULL */
    const float* wx;
    int tv_shared;         /* != 0: wy, wx are [H, W], shared by the batch */
} asr_sr_data_term;

/* asr_sr_forward_residual_f32 under a data term: q_out = w * psi(r) and, with r_out != NULL, the raw r as well. */
int asr_sr_forward_residual_dt_f32(const float* x, const float* y, const float* rot_tf, const float* trans_tf, float* q_out,
                                   float* r_out, int batch, int n, int H, int W, int h, int w, const asr_sr_data_term* dt,
                                   asr_stream_t stream);

/* asr_sr_loss_terms_cfg_f64 / _wtv_f64 with terms[b][0] = sum w * rho(r); r is the RAW residual (r_out above), not q. */
int asr_sr_loss_terms_dt_f64(const float* x, const float* r, double* terms, int batch, int n, int H, int W, int h, int w,
                             const asr_sr_config* cfg, const asr_sr_data_term* dt, asr_stream_t stream);

/* Workspace of asr_sr_solve_dt_f32: that of asr_sr_solve_workspace_bytes_cfg plus one more [batch, n, h, w] buffer (the raw
 * residual of the last iteration, for last_loss_terms). */
size_t asr_sr_solve_workspace_bytes_dt(int batch, int n, int H, int W, int h, int w, const asr_sr_config* cfg);

/* asr_sr_solve_cfg_f32 / _wtv_f32 under a data term.  The same launches per iteration: the forward kernel's data-term
 * instantiation in place of the plain one, the raw residual a second output of the last iteration's launch when
 * last_loss_terms is asked for.  {ASR_DF_L2, no weights} gives asr_sr_solve_cfg_f32's results bit for bit. */
int asr_sr_solve_dt_f32(float* x, const float* y, const float* rot_tf, const float* trans_tf, const float* inv_rot_tf,
                        const float* inv_trans_tf, float* m, float* v, float* vhat, const float* alphas, int num_iter,
                        double* last_loss_terms, void* workspace, size_t workspace_bytes, int batch, int n, int H, int W,
                        int h, int w, float lambda_df, float lambda_tv, float lambda_l2, float lambda_l1,
                        const asr_sr_config* cfg, const asr_sr_data_term* dt, asr_stream_t stream);

/* --- convergence monitor: a reproducible loss trace and a per-image stop rule --------------------------------------
 * asr_sr_solve_mon_f32 is asr_sr_solve_dt_f32 (dt may be {ASR_DF_L2, no weights}: every combination of the solver is
 * reachable) that evaluates the loss every `every` iterations, records it, and freezes each image of the batch by itself
 * once its loss has stalled.  The whole loop is enqueued as before: the rule runs on the device, the host never waits.
 *
 *   Loss terms.  The four terms of asr_sr_loss_terms_dt_f64 for the current x, before the iteration's update: the same
 *     float32 summands, statement for statement (bilateral TV: the float64 product of its two float32 factors, which is
 *     exact), accumulated in float64 -- but WITHOUT floating-point atomics and in one fixed order:
 *       image b's P elements (its n*h*w residuals for term 0, its H*W pixels for terms 1..3), p = 0 .. P-1, are dealt to
 *       256 workgroups of 256 threads; thread t of workgroup g adds the summands of p = g*256 + t + k*65536, k = 0, 1, ...,
 *       in rising p; a wave adds its 64 lanes by the tree s[l] += s[l + o] for o = 32, 16, 8, 4, 2, 1; a workgroup adds its
 *       four waves as ((w0 + w1) + w2) + w3: partial g, written to the workspace; one lane adds the 256 partials of a term
 *       in index order, from 0.
 *     The terms of image b depend on image b's data alone: the same bits from call to call, alone or inside any batch,
 *     for any plane_chunk.
 *   Scalar loss, in float64, each operation rounding by itself (no contraction), the lambdas the float32 arguments widened:
 *       L = ((lambda_df*t0 + lambda_tv*t1) + lambda_l2*t2),  then  L = L + lambda_l1*t3  only when lambda_l1 > 0.
 *   Stop rule, per image (Keras' EarlyStopping with a relative min_delta).  best = +inf, stall = 0 on entry.  Iteration
 *     it (0-based) is an evaluation when it % every == 0; its loss L is that of the x before update `it`.
 *       bar = (best == +inf) ? +inf : best - rel_tol*|best|          (float64; inf - tol*inf would be NaN)
 *       if (L < bar) { best = L; stall = 0; } else stall += 1;        (false for a NaN L, and for L = +inf)
 *       the image stops at the first evaluation with patience >= 1, stall >= patience and it >= min_iter:
 *       iters_done[b] = it, and no update from `it` on is applied to it.  An image that never stops: iters_done[b] = num_iter.
 *     A stopped image is frozen: its workgroups in the forward and gradient-plane kernels return at once, those of the
 *     update kernel carry x over and touch nothing else (not m, v, vhat).  Hence, bit for bit: x, m, v, vhat of image b equal
 *     image b of the same batch through asr_sr_solve_dt_f32 with num_iter = iters_done[b] and the first iters_done[b] rows of
 *     alphas; with patience = 0 that is the unmonitored solve itself.
 *   Outputs.  history (optional) [ceil(num_iter / every), batch, 4] float64: row e holds the terms of every image still
 *     running at evaluation e; the call first fills it with 0xFF bytes, so the rows after an image's stop read NaN.
 *     last_loss_terms (optional): the terms of the stopping evaluation for a stopped image -- the loss of the x that is
 *     returned --, the terms of the last iteration for the others, from the same reproducible sums.
 *   Optimiser counter.  alphas is prepared by the host before the solve, for all num_iter iterations; a stopped image leaves
 *     its remaining rows unused.  The caller's persistent step counter therefore advances by num_iter per solve, stop or no
 *     stop: it must not come to depend on a device result.
 *   Refusals, before any launch, outputs untouched: every refusal of asr_sr_solve_dt_f32; mon NULL, every < 1, rel_tol
 *     negative or not finite, patience < 0, min_iter < 0, iters_done NULL -> ASR_ERR_INVALID_ARG. */
typedef struct asr_sr_monitor {
    int every;            /* >= 1: iteration it (0-based) is an evaluation when it % every == 0 */
    double rel_tol;       /* >= 0, finite; 0 with patience 0 = trace only, never stop */
    int patience;         /* >= 1 to stop; 0 = never stop */
    int min_iter;         /* >= 0: no stop before this iteration */
    double* history;      /* device [ceil(num_iter/every), batch, 4] or NULL */
    int32_t* iters_done;  /* device [batch]: updates applied to each image */
} asr_sr_monitor;

/* Workspace of asr_sr_solve_mon_f32: that of asr_sr_solve_workspace_bytes_dt plus the partial sums and the rule's state. */
size_t asr_sr_solve_workspace_bytes_mon(int batch, int n, int H, int W, int h, int w, const asr_sr_config* cfg);

int asr_sr_solve_mon_f32(float* x, const float* y, const float* rot_tf, const float* trans_tf, const float* inv_rot_tf,
                         const float* inv_trans_tf, float* m, float* v, float* vhat, const float* alphas, int num_iter,
                         double* last_loss_terms, void* workspace, size_t workspace_bytes, int batch, int n, int H, int W,
                         int h, int w, float lambda_df, float lambda_tv, float lambda_l2, float lambda_l1,
                         const asr_sr_config* cfg, const asr_sr_data_term* dt, const asr_sr_monitor* mon,
                         asr_stream_t stream);

/* --- primal-dual: a solver for "smooth term + TV" that needs no learning rate ------------------------------------------
 * ASR_OPT_PRIMAL_DUAL is the iteration of Condat and Vu on the loss the other rules minimise by the sign subgradient: the TV
 * term is handled through its dual variable (one plane per difference direction, each value in a box) instead of a sign, and
 * the step comes from a bound on the data term's curvature (asr_sr_data_bound_f32) instead of a schedule.  It is accepted by
 * asr_sr_solve_cfg_f32, _wtv_f32, _dt_f32 and _mon_f32; the launches per iteration are those of the other rules.  The rule:
 *
 *   Slots.  m holds p_y and v holds p_x, the dual planes [batch, H, W], zero for a fresh solve; vhat is not touched (may be NULL).
 *   Scalars.  alphas[it,b] = tau;  c0 = the dual ratio, sigma = c0 / tau as ONE float32 division;  c1, c2 and flag are ignored.
 *   Per pixel (Y,X), every operation rounding by itself, everything read from the x and p BEFORE the iteration (a Jacobi
 *   step: the new duals of a pixel's neighbours are rebuilt from old values, never read from what the iteration writes):
 *       dY  = (Y < H-1) ? x[Y+1,X] - x[Y,X] : 0            dX = (X < W-1) ? x[Y,X+1] - x[Y,X] : 0
 *       by  = lambda_tv    (edge-weighted TV: lambda_tv * wy[Y,X], one multiply as in the weighted prior)     bx likewise
 *       py' = fminf(fmaxf(py + sigma*dY, -by), by)         px' likewise
 *       qy  = 2*py' - py                                   qx likewise
 *       div = -qy[Y,X] - qx[Y,X];  if (Y > 0) div += qy[Y-1,X];  if (X > 0) div += qx[Y,X-1];
 *       g   = g_df + div + two_lambda_l2 * x               (g_df: the data-term gradient every other rule receives)
 *       u   = x - g * tau
 *       x'  = lambda_l1 > 0 ? (u > t ? u - t : (u < -t ? u + t : 0)),  t = tau * lambda_l1   :   u
 *     The solves have no grad_out; g is not returned.  The result does not depend on plane_chunk.
 *   Workspace.  A second pair of dual planes: asr_sr_solve_workspace_bytes_cfg / _dt / _mon grow by 2 * batch * H * W floats
 *     when cfg->optimizer is ASR_OPT_PRIMAL_DUAL, and only then.
 *   Monitor.  A frozen image keeps x, p_y and p_x; the loss terms are those of x, as for every rule.
 *   Refusals, before any launch, outputs untouched: the bilateral-TV prior and ASR_DF_L1 (not smooth) as data loss ->
 *     ASR_ERR_UNSUPPORTED (Huber and weights are accepted); c0 not finite, <= 0 or > 1/16 -> ASR_ERR_INVALID_ARG.  The explicit
 *     one-step entry points asr_sr_backward_cfg_f32 / _wtv_f32 do not know the rule (they update slots in place; a solve with
 *     num_iter = 1 is the one-step form): optimizer 5 stays what it always was to them, "unknown optimizer 5",
 *     ASR_ERR_INVALID_ARG.
 *
 *   Step bound.  Let M be the linear map v -> the data-term gradient at x = v for measurements y = 0 under ASR_DF_L2 with the
 *     given weights (q = w * D(T(R(v))), then the gradient-plane and gather kernels with their 2*lambda_df and 0.25 factors).
 *     Every entry of M is >= 0, so for any v > 0 the largest (Mv)_i / v_i bounds M's spectral radius from above
 *     (Collatz-Wielandt), tighter with every application.  Per image, in float32:
 *       v = 1 everywhere;  repeat `iters` times (1..64):
 *           w = M v;   B = max over {i : v_i > 0} of w_i / v_i  (0 when the set is empty);   s = max_i w_i
 *           if (s > 0) v = w / s, else stop
 *       bound[b] = B of the last repetition done
 *     Maxima are order-free (taken on the bits of floats >= 0, as integers: no floating-point atomics): the same bits from call
 *     to call, alone or in any batch, for any plane_chunk.  A repetition costs one solver iteration; no y is needed.
 *     With tau = 1 / (bound + 2*lambda_l2) and c0 = 1/16:  1/tau - 8*sigma = (bound + 2*lambda_l2) / 2, the Condat-Vu
 *     condition for a smooth part with that Lipschitz constant and a difference operator of squared norm <= 8.  The
 *     theorem assumes the data gradient is a true gradient (M symmetric).  Under ASR_ADJ_REGISTERED the registered gradient of
 *     the projective transform is an inverse warp, not the adjoint: the step is a heuristic and the monitor is the guard.  Under
 *     ASR_ADJ_EXACT ("exact adjoint" below; asr_sr_data_bound_adj_f32) M = 2*lambda_df * A^T W A is symmetric and non-negative,
 *     the theorem's assumption holds and the bound is a bound.
 *     Refusals: null pointers (weights may be NULL), iters outside 1..64, lambda_df negative or not finite, plane_chunk < 0
 *     -> ASR_ERR_INVALID_ARG; the shape refusals of the solves; a short workspace -> ASR_ERR_WORKSPACE. */

/* Bytes of workspace asr_sr_data_bound_f32 needs (cfg: its plane_chunk, may be NULL); 0 for a size below 1. */
size_t asr_sr_data_bound_workspace_bytes(int batch, int n, int H, int W, int h, int w, const asr_sr_config* cfg);

/* bound [batch] (device): the step bound above.  weights: NULL, or [n, h, w] shared by the batch (weights_shared != 0) or
 * [batch, n, h, w], the data term's per-measurement weights.  cfg: its plane_chunk alone is read (may be NULL). */
int asr_sr_data_bound_f32(float* bound, const float* rot_tf, const float* trans_tf, const float* inv_rot_tf,
                          const float* inv_trans_tf, const float* weights, int weights_shared, int iters, void* workspace,
                          size_t workspace_bytes, int batch, int n, int H, int W, int h, int w, float lambda_df,
                          const asr_sr_config* cfg, asr_stream_t stream);

/* --- multi-label coupling: the classes of one image solved as one problem ------------------------------------------------
 * The K per-class solves of an image know nothing of each other; coupled, they minimise the sum of their losses subject to
 * x_k(p) >= 0 and sum_k x_k(p) <= 1 at every pixel (the convex multi-label relaxation; the slack 1 - sum_k x_k is "no class").
 * ASR_OPT_PRIMAL_DUAL ends every iteration in a prox step on x, and the prox of "lambda_l1 |.|_1 + the indicator of that set"
 * is the soft threshold followed by the Euclidean projection of the pixel's K values onto the set (the projection reads the
 * positive parts alone).  So the coupling is one per-pixel launch after the update launch; no other kernel changes.
 *
 *   Groups.  A group is G consecutive planes of the batch, 1 <= G <= ASR_MAX_CLASS_SET: batch indices g*G .. g*G + G-1.
 *   The projection rule, for one pixel with the group's values v_0 .. v_(G-1), all finite; every operation is float32 and
 *   rounds by itself:
 *       a_j = (v_j > 0) ? v_j : 0.0f                             (-0 and negatives become +0)
 *       s   = ((a_0 + a_1) + a_2) + ...                          in index order
 *       if (s <= 1.0f)  x_j = a_j  for all j                     (a feasible point is returned bit for bit, up to the sign of zero)
 *       else
 *          u_1 >= u_2 >= .. >= u_G : the a_j in descending order (equal values are interchangeable)
 *          c = 0;  theta = 0
 *          for k = 1 .. G:  c = c + u_k;  t = (c - 1.0f) / (float)k;  if (u_k > t) theta = t     (no break: the last k that holds)
 *          x_j = (a_j > theta) ? a_j - theta : 0.0f
 *     Against the exact projection the rule agrees to 1.6e-7 for G <= 32, with min x = 0 and sum x <= 1 + 8e-7.  It is
 *     idempotent only on feasible inputs: a second application moves a projected point by up to 1.8e-7, because the
 *     float32 sum of a projected point may still exceed 1 by a rounding.
 *   asr_simplex_project_f32: the rule in place on x [groups*group, pixels].  Refusals: null pointer, group outside
 *     1..ASR_MAX_CLASS_SET, groups < 1, pixels < 1 -> ASR_ERR_INVALID_ARG.
 *   asr_sr_solve_ml_f32: the arguments of asr_sr_solve_mon_f32 (mon may be NULL) and `group`.
 *     group == 0: asr_sr_solve_mon_f32 (mon given) or asr_sr_solve_dt_f32 (mon NULL), bit for bit, the same launches.
 *     group >= 1: after the update launch of the last copy chunk of every iteration, one projection launch over all groups
 *       rewrites the iteration's new x (and the bordered copy of it that the next forward launch reads).  The duals are not
 *       touched.  The result equals, bit for bit, num_iter rounds of {a solve of one iteration carrying its slots, then
 *       asr_simplex_project_f32}; it does not depend on plane_chunk.
 *     Monitor under coupling: the stop rule is applied per group.  At an evaluation every member's four terms and scalar loss
 *       L_b are computed exactly as above; history and last_loss_terms rows stay per member.  The group's loss is the members'
 *       L_b added in index order in float64, from 0; best, stall and the decision are the group's, kept at its first member.
 *       All members stop together: stopped and iters_done are set for each.  A stopped group's planes are skipped by the
 *       projection launch and carried by the update launch as above.  Hence, bit for bit: the members of a group stopped at
 *       `it` equal the same coupled solve with num_iter = it; with patience = 0 the monitored coupled solve is the unmonitored
 *       coupled solve with a trace.
 *     Refusals, before any launch, outputs untouched: group outside 0..ASR_MAX_CLASS_SET or batch % group != 0 ->
 *       ASR_ERR_INVALID_ARG; group >= 1 with an optimizer other than ASR_OPT_PRIMAL_DUAL -> ASR_ERR_UNSUPPORTED; every refusal
 *       of the entry point it wraps.
 *   Workspace: the coupling needs none.  asr_sr_solve_workspace_bytes_ml is asr_sr_solve_workspace_bytes_mon (monitored != 0)
 *     or asr_sr_solve_workspace_bytes_dt (monitored == 0). */
int asr_simplex_project_f32(float* x, int groups, int group, int64_t pixels, asr_stream_t stream);

size_t asr_sr_solve_workspace_bytes_ml(int batch, int n, int H, int W, int h, int w, const asr_sr_config* cfg, int monitored);

int asr_sr_solve_ml_f32(float* x, const float* y, const float* rot_tf, const float* trans_tf, const float* inv_rot_tf,
                        const float* inv_trans_tf, float* m, float* v, float* vhat, const float* alphas, int num_iter,
                        double* last_loss_terms, void* workspace, size_t workspace_bytes, int batch, int n, int H, int W,
                        int h, int w, float lambda_df, float lambda_tv, float lambda_l2, float lambda_l1,
                        const asr_sr_config* cfg, const asr_sr_data_term* dt, const asr_sr_monitor* mon /* may be NULL */,
                        int group, asr_stream_t stream);

/* --- copy reweighting: whole unreliable copies down-weighted inside the solve (IRLS over the copies) ------------------------
 * Huber caps the pull of each pixel; a copy on which the network failed outright still pulls with all of its h*w pixels.
 * Every few iterations the reweighted solve measures each copy's residual energy, compares it with the median over the copies
 * of its image and scales the whole copy by a robust weight c in [0, 1].  No existing kernel changes: the forward kernel already
 * multiplies by a weight buffer, and the launches below only rewrite that buffer (w_eff) and the buffer q the backward kernels
 * read, on the iterations that reweight.  No floating-point atomics anywhere.  The rule:
 *
 *   Inputs.  r [batch, n, h, w]: the RAW residual D(T(R(x))) - y, what asr_sr_forward_residual_dt_f32 writes to r_out.
 *     u: the data term's weights (weights / weights_shared as above), or none (u = 1).  rho, psi: the float32 statements of
 *     "data term" above.
 *   Per copy (b, i), over its P = h*w elements p = 0 .. P-1:
 *       energy e = sum_p (double)(u_p * rho(r_p))     each summand the float32 value asr_sr_loss_terms_dt_f64 adds (rho, then the
 *                                                     weight; no multiply without weights)
 *       mass   a = sum_p (double)u_p                  (double)P without weights, no sum
 *     both in float64 in one fixed order: one workgroup of 256 threads per copy; thread t adds p = t, t + 256, ... in rising p
 *     from 0.0; a wave adds its 64 lanes by the tree s[l] += s[l + o], o = 32, 16, 8, 4, 2, 1; the workgroup adds its four waves
 *     as ((w0 + w1) + w2) + w3 (the monitor's scheme at the scale of one copy).
 *       ebar = e / a, one float64 division.  The copy is ACTIVE when a > 0 and ebar is finite; an inactive copy (all-zero
 *       weights, e.g. one masked by the caller's copy dropout; a NaN residual) gets c = 0 and takes no part in the scale.
 *   Per image, with A = the number of active copies:
 *       s = the lower median of the active ebar: the value of rank (A-1)/2 (integer division), where
 *           rank(i) = #{j active : ebar_j < ebar_i  or  (ebar_j == ebar_i and j < i)}        (ranking by counting; n <= 640)
 *       if (A == 0 or s == 0)  c_i = 1 for every active copy (nothing to compare with: no reweighting); scale_out = s, or 0 for A = 0
 *       else  t_i = ebar_i / (kappa * s)  in float64: one multiply, one division, and
 *           ASR_RW_CAUCHY:  c_i = 1.0 / (1.0 + t_i*t_i)        (float64: a product, a sum, a division)
 *           ASR_RW_HARD:    c_i = (t_i <= 1.0) ? 1 : 0
 *         c_i is rounded ONCE to float32.  kappa is finite and > 0; a huge kappa (1e30) gives c = 1 exactly.
 *   Apply, per element:  w_eff = u * c_i, ONE float32 multiply (c_i itself without weights);  q = w_eff * psi(r): sr_dt_psi, then
 *     the multiply -- the statements of the forward kernel's data-term tail.  Hence q is bit for bit what a forward launch with
 *     weights = w_eff would have written.
 *   Nothing depends on plane_chunk, on the batch size or on what ran before.
 *
 *   asr_sr_solve_rw_f32: the arguments of asr_sr_solve_ml_f32 and rw.  rw == NULL: asr_sr_solve_ml_f32, bit for bit, the same
 *     launches.  Iteration `it` (0-based) reweights when it >= start and (it - start) % every == 0.  On such an iteration the
 *     forward launch also writes the raw residual (its existing second output); then energy + mass, copy weights and apply run
 *     (three launches) and the iteration proceeds as always.  The new weights are in force for that iteration's gradient and for
 *     every later forward launch until the next reweighting; before the first one w_eff = u (the caller's buffer is read as it
 *     is).  w_eff is a solver-owned [batch, n, h, w] buffer even when u is shared.  copy_weights starts at 1 for every copy and
 *     holds the last c at the end.  history (optional) [R, batch, n], R = the number of reweighting iterations below num_iter:
 *     row k holds the c of the k-th reweighting; the call first fills it with 0xFF bytes, so the rows of an image stopped by the
 *     monitor read NaN from its stop on.
 *     Hence, bit for bit: the solve equals the host-driven sequence {a solve of the iterations up to a reweighting point,
 *     carrying its slots; asr_sr_forward_residual_dt_f32 with r_out; the three stand-alone entry points below; the next segment
 *     with weights = w_eff}.  start >= num_iter is the unreweighted solve with every copy weight 1.
 *     Monitor.  Term 0 is evaluated under the weights in force at that iteration, after its reweighting if there was one.  The
 *       objective changes at a reweighting: on a reweighting iteration best goes back to +inf and stall to 0 for every image (or
 *       group) not yet stopped, before the decision (one small launch; the decision kernel is unchanged) -- so a reweighting
 *       iteration that is an evaluation always counts as an improvement.  A stopped image is frozen and never reweighted again:
 *       its w_eff, its copy_weights and, from then on, its history rows are not written.
 *     Coupling.  Weights stay per (plane, copy); nothing is shared across a group.
 *     Primal-dual.  The step bound (asr_sr_data_bound_f32) is still computed from the base weights u.  Every c <= 1 and every entry
 *       of the gradient map M is >= 0, so M under w_eff = u*c is entrywise <= M under u: reweighting only shrinks the map, its
 *       spectral radius can only fall (Perron-Frobenius), and the bound stays a bound.  The refusals of the wrapped entry points
 *       stay (ASR_DF_L1, bilateral TV, the dual ratio).
 *     Workspace: asr_sr_solve_workspace_bytes_rw = asr_sr_solve_workspace_bytes_ml + one [batch, n, h, w] float32 buffer (w_eff)
 *       + two float64 per copy (energy, mass), needed only when rw != NULL.
 *     Refusals, before any launch, outputs untouched: every refusal of asr_sr_solve_ml_f32; an unknown kind, kappa not finite or
 *       <= 0, every < 1, start < 0, copy_weights NULL -> ASR_ERR_INVALID_ARG.
 *   The stand-alone entry points (host-driven use; r, energy, mass, c, w_eff, q on the device):
 *     asr_sr_copy_energy_f64: energy, mass [batch, n] float64 from r; dt: loss, delta, weights, weights_shared are read.
 *     asr_sr_copy_weights_f32: c [batch, n] float32 and, optionally, scale_out [batch] float64 from energy and mass.
 *     asr_sr_apply_copy_weights_f32: w_eff and q [batch, n, h, w] from r, dt and c; four distinct buffers (w_eff must not
 *       alias the weights of dt).
 *     Refusals: null pointers (scale_out may be NULL), batch, n, h or w < 1, n > 640, batch * n > 2^31 - 1, h * w > 65535 * 256, the data term's
 *       own refusals, an unknown kind, kappa not finite or <= 0 -> ASR_ERR_INVALID_ARG. */
#define ASR_RW_CAUCHY 0
#define ASR_RW_HARD 1
#define ASR_RW_MAX_COPIES 640

typedef struct asr_sr_reweight {
    int kind;             /* ASR_RW_* */
    double kappa;         /* finite, > 0: a copy at kappa times the median energy gets weight 1/2 (Cauchy) or is the last kept (hard) */
    int every;            /* >= 1 */
    int start;            /* >= 0: iteration it reweights when it >= start and (it - start) % every == 0 */
    float* copy_weights;  /* device [batch, n]: 1 on entry to the loop, the last c at the end */
    float* history;       /* device [R, batch, n] or NULL */
} asr_sr_reweight;

int asr_sr_copy_energy_f64(const float* r, const asr_sr_data_term* dt, double* energy, double* mass, int batch, int n, int h,
                           int w, asr_stream_t stream);

int asr_sr_copy_weights_f32(const double* energy, const double* mass, int kind, double kappa, float* c, double* scale_out,
                            int batch, int n, asr_stream_t stream);

int asr_sr_apply_copy_weights_f32(const float* r, const asr_sr_data_term* dt, const float* c, float* w_eff, float* q, int batch,
                                  int n, int h, int w, asr_stream_t stream);

size_t asr_sr_solve_workspace_bytes_rw(int batch, int n, int H, int W, int h, int w, const asr_sr_config* cfg, int monitored);

int asr_sr_solve_rw_f32(float* x, const float* y, const float* rot_tf, const float* trans_tf, const float* inv_rot_tf,
                        const float* inv_trans_tf, float* m, float* v, float* vhat, const float* alphas, int num_iter,
                        double* last_loss_terms, void* workspace, size_t workspace_bytes, int batch, int n, int H, int W,
                        int h, int w, float lambda_df, float lambda_tv, float lambda_l2, float lambda_l1,
                        const asr_sr_config* cfg, const asr_sr_data_term* dt, const asr_sr_monitor* mon /* may be NULL */,
                        int group, const asr_sr_reweight* rw /* may be NULL */, asr_stream_t stream);

/* --- exact adjoint: the data-term gradient as the true transpose of the forward operator -----------------------------------
 * Every update rule receives the data-term gradient g_df = sum_n c_n.  Under ASR_ADJ_REGISTERED (what every other entry point
 * computes) c_n(p) is TensorFlow's registered gradient of the rotate: one bilinear tap of the per-copy plane G_R[n] at R_n^-1 p,
 * an inverse warp, not the transpose.  The resize gradient is the exact transpose and the translate stage's inverse warp is the
 * transpose up to the rounding of its tap weights; the defect sits in the rotate alone.  Under ASR_ADJ_EXACT only the gather
 * changes: the grad-translate kernel writes the same zero-bordered planes G_R, and the tap is replaced by the transpose of the
 * forward rotate, as a gather (no floating-point atomics).  The rule, for HR pixel p = (X, Y) and copy n with rot_tf[n] = R
 * (a0 a1 a2 b0 b1 b2) and inv_rot_tf[n] = I (i00 i01 i02 i10 i11 i12), every operation float32 and rounding by itself:
 *
 *   Window.  (qx, qy) = (i00*X + i01*Y + i02,  i10*X + i11*Y + i12)          the forward kernels' affine map, with I
 *       ex = (|i00| + |i01|) + 1/64        ey = (|i10| + |i11|) + 1/64       the margin 1/64: I is a rounded inverse, q is float32
 *       x positions  ceil(qx - ex) .. floor(qx + ex),   y positions  ceil(qy - ey) .. floor(qy + ey)
 *     A forward tap of position q touches p only if |R q - p| < 1 on both axes, i.e. |q - R^-1 p| < (|i00|+|i01|, |i10|+|i11|):
 *     the window holds every q with a non-zero weight.  For a rotation it is at most 3 x 3.  The first position is clamped to
 *     [-2, size - 1] and the last to [-3, size + 1]: positions outside the image contribute nothing (G_R is 0 there, the plane's
 *     border), and nothing outside the bordered plane is read, however far outside the image R^-1 p lies.
 *   Weights.  For a position q = (x, y) of the window:
 *       ix = a0*x + a1*y + a2      iy = b0*x + b1*y + b2                      the forward kernel's own statements at q
 *       xf = floor(ix)             wx = (xf == X) ? (xf + 1) - ix : ((xf + 1 == X) ? ix - xf : 0)        wy likewise with iy, Y
 *     A position too many (a margin, a clamp) has weight 0 and adds +-0: the result does not depend on the window's extent.
 *   Order.  c_n = 0;  for y rising, for x rising:  c_n = c_n + (wy * wx) * G_R[n][y, x].   g_df = the running sum over the
 *     copies n = 0 .. N-1 in order, from +0, each c_n added once: the result does not depend on plane_chunk or on the batch.
 *   Forms.  When ex <= 1.46875 and ey <= 1.46875 for every copy of the image (every rotation: |cos| + |sin| <= 1.4143) the three
 *     positions ceil(q - e) + {0, 1, 2} per axis cover the window and a branch-free 3 x 3 form runs; otherwise a counted loop.
 *   Where it applies, per image (one small flags launch per call): every rot_tf and inv_rot_tf of the image affine (c0 == c1 == 0),
 *     every trans_tf a pure translation (1 0 t 0 1 t 0 0), ex and ey <= 8 and |i02|, |i12| <= 16384 (float32 then keeps q within
 *     the margin).  An image that fails any of these -- a projective rotation, a non-pure translate, a transform that is not
 *     finite -- takes the REGISTERED statements for all its copies, bit for bit.  asr_sr_adjoint_flags_i32 reports the choice:
 *     flags[b] = 1 exact, 0 registered.  inv_rot_tf is used as given, to locate the window only; the weights never read it.
 *   With angle 0 every R q is an integer position (a shift), the transpose is the single tap the registered form takes, and both
 *     forms return the same bits.
 *
 *   asr_sr_solve_adj_f32: the arguments of asr_sr_solve_rw_f32 and `adjoint`.  ASR_ADJ_REGISTERED: asr_sr_solve_rw_f32, bit for
 *     bit, the same launches.  ASR_ADJ_EXACT: the flags launch and the gather launches are the exact ones, one for one; the forward
 *     and grad-translate launches, the monitor, the coupling and the reweighting are unchanged, and so is every workspace size
 *     (asr_sr_solve_workspace_bytes_rw / _ml / _mon / _dt).  Combines with every optimizer, data term and prior.
 *   asr_sr_data_bound_adj_f32: asr_sr_data_bound_f32 with the gather chosen by `adjoint`; the same workspace.
 *   asr_sr_backward_adj_f32: one step, the arguments of asr_sr_backward_wtv_f32 with rot_tf, trans_tf, `adjoint` and a workspace;
 *     wy == wx == NULL means the unweighted prior (asr_sr_backward_cfg_f32).  ASR_ADJ_REGISTERED: the one launch of the entry point
 *     it wraps; the workspace is not read (may be NULL).  ASR_ADJ_EXACT: the grad-translate and exact gather launches per chunk of
 *     cfg->plane_chunk copies, so grad_out is available with x_new == NULL.  asr_sr_backward_adj_workspace_bytes: the running sum
 *     [batch, H, W] + the planes of a chunk + one int per image; host arithmetic, 0 for a size below 1.
 *   Refusals, before any launch, outputs untouched: adjoint other than 0 or 1 -> ASR_ERR_INVALID_ARG; every refusal of the
 *     wrapped entry point; asr_sr_backward_adj_f32 under ASR_ADJ_EXACT also a NULL or short workspace, plane_chunk < 0 and
 *     batch * chunk > 65535. */
#define ASR_ADJ_REGISTERED 0
#define ASR_ADJ_EXACT 1

int asr_sr_adjoint_flags_i32(const float* rot_tf, const float* trans_tf, const float* inv_rot_tf, int* flags /* device [batch] */,
                             int batch, int n, asr_stream_t stream);

int asr_sr_solve_adj_f32(float* x, const float* y, const float* rot_tf, const float* trans_tf, const float* inv_rot_tf,
                         const float* inv_trans_tf, float* m, float* v, float* vhat, const float* alphas, int num_iter,
                         double* last_loss_terms, void* workspace, size_t workspace_bytes, int batch, int n, int H, int W,
                         int h, int w, float lambda_df, float lambda_tv, float lambda_l2, float lambda_l1,
                         const asr_sr_config* cfg, const asr_sr_data_term* dt, const asr_sr_monitor* mon /* may be NULL */,
                         int group, const asr_sr_reweight* rw /* may be NULL */, int adjoint, asr_stream_t stream);

int asr_sr_data_bound_adj_f32(float* bound, const float* rot_tf, const float* trans_tf, const float* inv_rot_tf,
                              const float* inv_trans_tf, const float* weights, int weights_shared, int iters, void* workspace,
                              size_t workspace_bytes, int batch, int n, int H, int W, int h, int w, float lambda_df,
                              const asr_sr_config* cfg, int adjoint, asr_stream_t stream);

size_t asr_sr_backward_adj_workspace_bytes(int batch, int n, int H, int W, const asr_sr_config* cfg /* may be NULL */);

int asr_sr_backward_adj_f32(const float* x, float* x_new, const float* resid, const float* rot_tf, const float* trans_tf,
                            const float* inv_rot_tf, const float* inv_trans_tf, float* m, float* v, float* vhat,
                            const float* alphas, float* grad_out, int batch, int n, int H, int W, int h, int w, float lambda_df,
                            float lambda_tv, float lambda_l2, float lambda_l1, const asr_sr_config* cfg, const float* wy,
                            const float* wx, int w_shared, int adjoint, void* workspace, size_t workspace_bytes,
                            asr_stream_t stream);

/* out[b] = max / mean over copies of rotate(translate(resize(y[b,i], (H,W)), trans_tf), rot_tf)
 * -- max_superresolution / mean_superresolution, superresolution.py:139-161 (trans_tf built
 * from -shifts, rot_tf from -angles).  out [batch,H,W]; (H, W) need not be a multiple of (h, w).  The maximum runs
 * over the warped copies as they are, zero fill included: where every copy is negative or out of frame it is 0. */
int asr_realign_max_f32(const float* y, float* out, const float* trans_tf, const float* rot_tf, int batch, int n,
                        int H, int W, int h, int w, asr_stream_t stream);
int asr_realign_mean_f32(const float* y, float* out, const float* trans_tf, const float* rot_tf, int batch, int n,
                         int H, int W, int h, int w, asr_stream_t stream);

/* Both of the above in one pass over the copies (the reference computes max- and mean-SR of the same
 * copies, SR_single_class.py:103-110): out_max / out_mean [batch,H,W], bit-identical to the two calls. */
int asr_realign_max_mean_f32(const float* y, float* out_max, float* out_mean, const float* trans_tf,
                             const float* rot_tf, int batch, int n, int H, int W, int h, int w, asr_stream_t stream);

/* Order statistics over the realigned copies: the pixel-wise median, other quantiles and the trimmed mean, the robust
 * fusions of multi-frame super-resolution, in ONE launch that never writes the N warped planes to memory.
 * y, trans_tf, rot_tf, batch, n, H, W, h, w are exactly those of asr_realign_max_f32: any positive sizes at any ratio,
 * any ImageProjectiveTransformV3 vector.  lo_rank, hi_rank, t are HOST arrays of num_q entries, read during the call
 * (like asr_sr_config).
 *
 * The rule.  For output pixel (b, Y, X) let v_0 .. v_(n-1) be the values sr_realign_kernel folds, that is
 * rotate(translate(resize(y[b,i]))) at that pixel, zero fill included: an out-of-frame copy contributes 0 to the order
 * statistics, as it does to max and mean.  Let s_0 <= .. <= s_(n-1) be the same values sorted.
 *  - out_q is [num_q, batch, H, W], 0 <= num_q <= 8.  Plane j is s[lo] when lo == hi, otherwise
 *    s[lo] + (s[hi] - s[lo]) * t[j], in f32 with two roundings and no contraction (lo = lo_rank[j], hi = hi_rank[j]).
 *    It needs 0 <= lo <= hi <= n - 1.
 *  - out_trim is [batch, H, W] and optional: pass NULL and trim_k = 0 to skip it.  It is the mean of s[k] .. s[n-1-k]
 *    with k = trim_k, 0 <= 2k < n.
 *  - The trimmed mean is computed as follows.  Let a = s[k] and c = s[n-1-k].  The sum is (the sum of the v_i with
 *    a < v_i < c, in copy order) + c_a * a + c_c * c, where c_a and c_c are how many copies of each boundary value lie
 *    inside the kept ranks.  When a == c the sum is (n - 2k) * a.  The result is that sum divided by (float)(n - 2k).
 *  - -0 and +0 compare equal, and either may be returned.  Results for NaN inputs are unspecified.
 * num_q == 0 with out_trim == NULL, a bad rank, null pointers and bad shapes return ASR_ERR_INVALID_ARG before any
 * launch; n above asr_realign_select_max_copies() returns ASR_ERR_UNSUPPORTED (the message names the cap) and nothing is
 * launched.  Each thread owns one output pixel and keeps its n values in LDS (256 bytes per copy and workgroup of 64
 * pixels), so the cap is what fits a workgroup's 160 KiB. */
int asr_realign_select_max_copies(void);      /* host arithmetic, no GPU: the largest n accepted below (>= 256) */
int asr_realign_select_f32(const float* y, float* out_q, float* out_trim, const int* lo_rank, const int* hi_rank,
                           const float* t, int num_q, int trim_k, const float* trans_tf, const float* rot_tf, int batch,
                           int n, int H, int W, int h, int w, asr_stream_t stream);

/* Coverage-normalised fusions over the realigned copies: the shift-and-add mean of multi-frame super-resolution (sum of
 * the realigned values over the sum of the realigned weights), the median over the copies that saw the pixel, and the
 * coverage map itself, in ONE launch.  y, trans_tf, rot_tf, batch, n, H, W, h, w are exactly those of
 * asr_realign_max_f32.  wgt holds the weight planes: [batch, n, h, w] when wgt_shared == 0, ONE [h, w] plane used for every
 * copy of every image when wgt_shared != 0.  out_mean, out_median, out_cov are [batch, H, W]; each is optional (NULL), at
 * least one must be given.
 *
 * The rule.  For output pixel (b, Y, X) and copy i, v_i is the value sr_realign_kernel folds for plane (b, i) of y, and
 * c_i is the value the SAME statements give for that copy's weight plane, same transforms, zero fill included: a copy that
 * left the frame has c_i = 0 instead of counting as a measurement of 0.  y is NOT multiplied by wgt: a caller who wants
 * sum R(w y) / sum R(w) passes y already weighted.
 *  - C = c_0 + .. + c_(n-1) and S = v_0 + .. + v_(n-1), each in copy order, in f32, no contraction (the sum of
 *    asr_realign_mean_f32).
 *  - out_cov is C.
 *  - out_mean is S / C (one IEEE f32 division) where C >= cov_min, otherwise 0.
 *  - Copy i is valid at the pixel when c_i >= valid_min.  Let nv be the number of valid copies and
 *    s_0 <= .. <= s_(nv-1) their v_i sorted.  out_median is 0 when nv == 0; otherwise, with lo = (nv - 1) / 2 and
 *    hi = nv / 2 (integer division), it is s[lo] when lo == hi, else s[lo] + (s[hi] - s[lo]) * 0.5f, in f32 with two
 *    roundings and no contraction (the rule of asr_realign_select_f32).
 *  - -0 and +0 compare equal, and either may be returned.  Results for NaN inputs are unspecified.
 * Null y / wgt / transforms, all three outputs NULL, a bad shape, and a cov_min or valid_min that is not finite and > 0
 * return ASR_ERR_INVALID_ARG before any launch.  With out_median, n above asr_realign_select_max_copies() returns
 * ASR_ERR_UNSUPPORTED (the message names the cap) and nothing is launched: the median keeps a pixel's n values in LDS like
 * asr_realign_select_f32.  Without out_median any n is accepted and no LDS is used. */
int asr_realign_covered_f32(const float* y, const float* wgt, int wgt_shared, float* out_mean, float* out_median,
                            float* out_cov, float cov_min, float valid_min, const float* trans_tf, const float* rot_tf,
                            int batch, int n, int H, int W, int h, int w, asr_stream_t stream);

/* Moments over the realigned copies: the mean, the population variance about it and the number of copies that saw the pixel,
 * in ONE launch -- how far the copies disagree at a pixel, the second product of test-time augmentation next to the fused
 * value.  y, trans_tf, rot_tf, batch, n, H, W, h, w are exactly those of asr_realign_max_f32.  wgt may be NULL; when given
 * it is as in asr_realign_covered_f32: [batch, n, h, w] when wgt_shared == 0, ONE [h, w] plane when wgt_shared != 0.
 * out_mean, out_var, out_nv are [batch, H, W]; each is optional (NULL), at least one must be given.
 *
 * The rule.  For output pixel (b, Y, X) and copy i, v_i is the value sr_realign_kernel folds for plane (b, i) of y, zero
 * fill included.
 *  - wgt == NULL: every copy is valid, nv = n, and valid_min is ignored.
 *  - wgt given: c_i is the value the SAME statements give for the copy's weight plane; copy i is valid when
 *    c_i >= valid_min, and nv is the number of valid copies.  valid_min must be finite and > 0.
 *  - out_nv is (float)nv.
 *  - out_mean is m = S / (float)nv, S the sum of the valid v_i in copy order, in f32, no contraction, then one IEEE f32
 *    division; 0 when nv == 0.  With wgt == NULL it is asr_realign_mean_f32 bit for bit.
 *  - out_var is the population variance about that ROUNDED m: s = s + d * d with d = v_i - m over the valid copies in copy
 *    order (the subtraction, the product and the add each round once, no contraction), then one IEEE f32 division by
 *    (float)nv.  It is 0 when nv == 0 and exactly 0 when nv == 1 (m is v_i itself there).
 *  - Results for NaN inputs are unspecified.
 * Null y / transforms, all three outputs NULL, a bad shape, and with wgt a valid_min that is not finite and > 0 return
 * ASR_ERR_INVALID_ARG before any launch.  Any n is accepted and no LDS is used: a thread owns one output pixel and walks
 * the copies twice, recomputing each v_i for the deviations instead of parking it. */
int asr_realign_moments_f32(const float* y, const float* wgt, int wgt_shared, float* out_mean, float* out_var, float* out_nv,
                            float valid_min, const float* trans_tf, const float* rot_tf, int batch, int n, int H, int W,
                            int h, int w, asr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Output processing, thresholding, IoU
 * ------------------------------------------------------------------------------------------ */

/* out_minmax[s] = {min, max} of segment s (tf.reduce_min / tf.reduce_max,
 * augmentation_utils.py:100-101, superres_utils.py:134). */
int asr_minmax_f32(const float* x, float* out_minmax, int64_t per_segment, int segments, asr_stream_t stream);

/* Activation(last_activation) over the class axis (model.py:124-125): kind 1 = softmax, 2 = sigmoid.
 * out may alias logits. */
int asr_class_activation_f32(const float* logits, float* out, int64_t pixels, int classes, int kind,
                             asr_stream_t stream);

/* The network's confidence per pixel from the logits rows [pixels, classes] -> out [pixels]: the weights of the SR solver's
 * data term (asr_sr_data_term).  With max = the row's largest logit and sum = the float32 sum, in class order, of
 * expf(z_c - max):
 *   ASR_CONF_MAXPROB  1.0f / sum: the largest entry of asr_class_activation_f32's softmax, bit for bit;
 *   ASR_CONF_MARGIN   that value minus expf(z_second - max) / sum, z_second the second largest logit counted with multiplicity:
 *                     the difference of the two largest softmax entries; a tie for the maximum gives 0, one class gives 1.
 * Refusals before any launch: null pointers, pixels or classes <= 0, an unknown kind -> ASR_ERR_INVALID_ARG. */
#define ASR_CONF_MAXPROB 1
#define ASR_CONF_MARGIN 2
int asr_opm_confidence_f32(const float* logits, float* out, int64_t pixels, int classes, int kind, asr_stream_t stream);

/* create_mask: argmax over the class axis, first maximum wins (utils.py:115-119). */
int asr_argmax_i32(const float* logits, int32_t* out, int64_t pixels, int classes, asr_stream_t stream);

/* argmax OPM: class_id where argmax == class_id else 0, as float32 (augmentation_utils.py:106-113). */
int asr_opm_argmax_f32(const float* logits, float* class_mask, int64_t pixels, int classes, int class_id,
                       asr_stream_t stream);

/* slice_max OPM: class logit and max over the other classes (augmentation_utils.py:82-93). */
int asr_opm_slice_max_f32(const float* logits, float* class_mask, float* max_mask, int64_t pixels, int classes,
                          int class_id, asr_stream_t stream);

/* slice OPM: class logit min-max normalised with the copy's global min / max over all classes
 * (augmentation_utils.py:95-104 + superres_utils.py:56-62).  minmax_ws: [copies,2] floats. */
int asr_opm_slice_f32(const float* logits, float* class_mask, float* minmax_ws, int copies, int64_t pixels_per_copy,
                      int classes, int class_id, float new_min, float new_max, asr_stream_t stream);

/* threshold_image (superres_utils.py:118-139): out = image >= th_mask ? th_value : 0, or
 * (th_mask == NULL) image > th_factor * max(image) ? th_value : 0 per segment.
 * minmax_ws: [segments,2] floats (needed when th_mask == NULL). */
int asr_threshold_f32(const float* image, const float* th_mask, float* minmax_ws, int32_t* out, int64_t per_segment,
                      int segments, float th_factor, int th_value, asr_stream_t stream);

/* single_class_IOU integer counts (utils.py:180-204): counts[s] = {inter_c, union_c, inter_bg,
 * union_bg}; with include_bg the truth is first remapped (truth != class_id -> 0).  Void (255)
 * pixels are not excluded, exactly like the reference. */
int asr_iou_counts_i32(const int32_t* truth, const int32_t* pred, int64_t* counts, int64_t per_segment, int segments,
                       int class_id, int include_bg, asr_stream_t stream);

/* The same counts for num_preds prediction masks [num_preds, pixels] against ONE label map [pixels] -- the four masks of an
 * image (standard, ASR, max-SR, mean-SR) against its ground truth, SR_single_class.py:109-120 -- without replicating it. */
int asr_iou_counts_shared_truth_i32(const int32_t* truth, const int32_t* preds, int64_t* counts, int64_t pixels, int num_preds,
                                    int class_id, int include_bg, asr_stream_t stream);

/* Threshold sweep (threshold_tests.py:113-121): for S images [segments, per_segment] and K = num_factors threshold factors
 * [K] (device floats, any order, repeats allowed), counts[s][k] = {inter_c, union_c, inter_bg, union_bg} equals, bit for bit,
 * asr_threshold_f32(image_s, NULL, factors[k], class_id) followed by asr_iou_counts_i32(truth_s, ., class_id, include_bg):
 * the threshold is the f32 product max(image_s) * factors[k] and the comparison is strict.  truth: [per_segment] shared by
 * every image (shared_truth != 0) or [segments, per_segment].  One pass over the images for all K factors; exact for
 * finite images.  1 <= K <= 256, segments <= 65535.  workspace: asr_threshold_sweep_workspace_bytes(segments, K) bytes
 * (histograms + per-image extrema), fully rewritten by each call. */
size_t asr_threshold_sweep_workspace_bytes(int segments, int num_factors);
int asr_threshold_sweep_iou_counts_f32(const float* images, const int32_t* truth, const float* factors, void* workspace,
                                       size_t workspace_bytes, int64_t* counts, int64_t per_segment, int segments,
                                       int num_factors, int shared_truth, int class_id, int include_bg,
                                       asr_stream_t stream);

/* min_max_normalization of whole stacks with their own global extrema, as load_SR_data applies it to the argmax / slice_max
 * masks of an image (superres_utils.py:56-62, 183-206): per segment out = new_min + ((x - min) * (new_max - new_min)) /
 * (max - min, or 1 when they are equal).  minmax_ws: [segments, 2] floats of scratch (receives the extrema). */
int asr_minmax_normalize_f32(const float* x, float* out, float* minmax_ws, int64_t per_segment, int segments, float new_min,
                             float new_max, asr_stream_t stream);

/* Standard-output mask of ONE image (generate_standard_output.py:52-65: the model built with final_upsample=True,
 * model.py:108-111, then create_mask and the class filter): bilinear half-pixel upsample of the logits [h_in, w_in, classes]
 * to h_out x w_out, argmax over the classes (first maximum), mask = class_id where it wins, else 0 -- in one pass. */
int asr_standard_mask_i32(const float* logits, int32_t* mask, int h_in, int w_in, int classes, int h_out, int w_out, int class_id,
                          asr_stream_t stream);

/* --- class sets: several classes of one image from one forward pass ----------------------------------------------
 * Each entry point below takes K distinct class ids `ids` (a HOST int array, read during the call; 1 <= K <=
 * ASR_MAX_CLASS_SET, every id in [0, classes)) and equals, bit for bit, K calls of its single-class counterpart, one per
 * id, while reading its input once.  For the OPM and the standard mask the single-class entry points (asr_opm_argmax_f32,
 * asr_opm_slice_f32, asr_opm_slice_max_f32, asr_standard_mask_i32) ARE the K = 1 case: they keep their own argument checks
 * and messages and then run the class-set kernels on a set of one, so a one-id class-set call and the single-class call
 * issue the same launches.  A bad set (K out of range, an id twice, an id out of range) returns
 * ASR_ERR_INVALID_ARG before any launch.  Each class keeps the reference's single-class meaning; the label-map entry
 * points further down fuse the classes into one label map. */
#define ASR_MAX_CLASS_SET 32
#define ASR_OPM_ARGMAX 0
#define ASR_OPM_SLICE 1
#define ASR_OPM_SLICE_MAX 2
/* OPM of mode ASR_OPM_* for K classes: plane k, at class_masks + k * class_stride (and max_masks + k * class_stride,
 * slice_max only), holds [copies * pixels_per_copy] floats equal to asr_opm_argmax_f32 / asr_opm_slice_f32 /
 * asr_opm_slice_max_f32 for ids[k] (class_stride >= copies * pixels_per_copy when K > 1: a forward batch can fill rows of
 * per-class [K, N, h, w] stacks).  minmax_ws: [copies, 2] floats, slice only (the per-copy extrema, computed once). */
int asr_opm_classes_f32(const float* logits, const int* ids, int K, int mode, float* class_masks, float* max_masks,
                        float* minmax_ws, int copies, int64_t pixels_per_copy, int classes, int64_t class_stride,
                        float new_min, float new_max, asr_stream_t stream);

/* asr_threshold_f32 on K segments [K, per_segment] with th_value = th_values[k] on segment k (th_values: K distinct
 * ids >= 0).  minmax_ws: [K, 2] floats, needed when th_mask == NULL. */
int asr_threshold_classes_f32(const float* image, const float* th_mask, float* minmax_ws, int32_t* out, int64_t per_segment,
                              int K, float th_factor, const int* th_values, asr_stream_t stream);

/* asr_iou_counts_shared_truth_i32 for K classes in one pass over the label map: preds [K, M, pixels] (the M masks of class
 * ids[k] in row k; 1 <= M <= 8), counts [K, M, 4] int64 (zeroed by the call).  Ids may be any value >= 0 here. */
int asr_iou_counts_classes_i32(const int32_t* truth, const int32_t* preds, int64_t* counts, int64_t pixels, int K, int M,
                               const int* ids, int include_bg, asr_stream_t stream);

/* asr_standard_mask_i32 for K classes: one bilinear upsample + argmax per output pixel, masks [K, h_out, w_out]. */
int asr_standard_mask_classes_i32(const float* logits0, int32_t* masks, int h_in, int w_in, int classes, int h_out,
                                  int w_out, const int* ids, int K, asr_stream_t stream);

/* --- label maps: the K single-class results of one image fused into one int32 label map ---------------------------
 * ids: K distinct class ids, a HOST int array as above, each in [1, classes) (classes <= 0: any id >= 1); 0 is the label
 * of "no class" and never a candidate.  A bad set returns ASR_ERR_INVALID_ARG before any launch.
 *
 * Label fusion of one SR type.  scores [K, pixels]: plane k is the float32 SR output S_k of class ids[k], the tensor
 * asr_threshold_classes_f32 would threshold; max_scores [K, pixels] or NULL: the SR outputs Smax_k of the classes' max maps
 * (slice_max).  Class k PASSES at pixel p exactly when its single-class mask is set there: S_k(p) > th_factor * max(S_k)
 * (f32 product, strict, as asr_threshold_f32), or with max_scores S_k(p) >= Smax_k(p).  Its rank value is r_k(p) = S_k(p),
 * or with max_scores the single f32 subtraction S_k(p) - Smax_k(p).  labels[p] = ids[k*], k* the passing class with the
 * greatest r_k(p), equal values (-0.0 == +0.0 among them) going to the lowest k; labels[p] = 0 when no class passes.
 * Inputs are finite.  Hence labels[p] = c != 0 implies that the single-class mask of c is set at p, labels[p] = 0 exactly
 * when no mask is set, and with K = 1 the label map is the single-class mask, bit for bit.
 * minmax_ws: [K, 2] floats of scratch, needed when max_scores == NULL (the per-plane extrema, asr_minmax_f32).
 * truth / counts: both NULL, or a label map [pixels] and int64 [3, 256]: the same pass then leaves in counts what
 * asr_class_counts_i32(truth, labels) would (zeroed by the call), so the label map is not read back for scoring. */
int asr_fuse_labels_f32(const float* scores, const float* max_scores, float* minmax_ws, const int32_t* truth, int32_t* labels,
                        int64_t* counts, int64_t pixels, int K, float th_factor, const int* ids, int classes,
                        asr_stream_t stream);

/* Label fusion swept over T = num_factors threshold factors, counts only (the label-map counterpart of
 * asr_threshold_sweep_iou_counts_f32): th_factor is read by the fusion alone, so the SR outputs of one run hold every factor's
 * label map.  scores [K, pixels], ids, classes: as asr_fuse_labels_f32 (a bad set is refused through the same check, before
 * any launch); truth [pixels]: required; factors: T device floats in any order, repeats, negative values and values above 1
 * allowed, 1 <= T <= 64.
 *  - Equivalence: counts is int64 [T, 3, 256], zeroed by the call, and counts[j] equals, bit for bit, the counts that
 *    asr_fuse_labels_f32(scores, NULL, ws, truth, labels, counts_j, pixels, K, factors[j], ids, classes) leaves.
 *  - Pass rule: class k passes at pixel p for factor j exactly when S_k(p) > max(S_k) * factors[j] (f32 product, strict).
 *  - Winner: the passing class with the greatest S_k(p) labels the pixel, equal values (-0.0 == +0.0 among them) going to the
 *    lowest k; the label is 0 when no class passes.  The winner is NOT monotone in the factor: the top-scoring class can fail
 *    its own, larger, threshold while a lower-scoring class of a smaller maximum still passes and takes the pixel.
 *  - Counted labels: labels outside 0..255 are not counted, as in asr_class_counts_i32; counts[j][0], the truth histogram, is
 *    therefore the same for every j.
 *  - No max-map form: with max maps (slice_max) the threshold plays no part, so there is nothing to sweep.
 *  - Exact for finite inputs.  No label map is written; only the counts leave the device.
 * One asr_minmax_f32 over the K planes, one pass in which every plane is read once for all T factors, one small finalize
 * launch.  workspace: asr_fuse_labels_sweep_workspace_bytes(K, T) = 8 * (T * 2 * (K + 1) + 256) + 8 * K bytes (per factor the
 * predicted and the agreeing pixels of label 0 and of the K ids, one truth histogram, then the per-plane extrema), 8-byte
 * aligned, fully rewritten by each call (0 for K <= 0 or T <= 0); a short workspace returns ASR_ERR_WORKSPACE. */
size_t asr_fuse_labels_sweep_workspace_bytes(int K, int num_factors);
int asr_fuse_labels_sweep_counts_f32(const float* scores, const int32_t* truth, const float* factors, void* workspace,
                                     size_t workspace_bytes, int64_t* counts, int64_t pixels, int K, int num_factors,
                                     const int* ids, int classes, asr_stream_t stream);

/* Label fusion of a coupled solve ("multi-label coupling" above): the planes are shares of one pixel, so no threshold is
 * needed.  scores [K, pixels], ids: as asr_fuse_labels_f32 (classes = 0: any id >= 1).  Per pixel, in float32, every operation
 * rounding by itself:  s = ((S_0 + S_1) + ...) in index order;  bg = 1.0f - s, the share of "no class";  k* = the first k of
 * greatest S_k;  labels[p] = (S_k* > bg) ? ids[k*] : 0.  Inputs are finite.  Counts come from asr_class_counts_i32. */
int asr_fuse_labels_simplex_f32(const float* scores, const int* ids, int K, int32_t* labels, int64_t pixels,
                                asr_stream_t stream);

/* The standard label map of the same class set: bilinear upsample + argmax of the un-augmented copy's logits (exactly
 * asr_standard_mask_classes_i32's), the winner kept when it is one of ids, else 0 -- bit for bit the sum over k of that
 * entry point's K masks, one int32 [h_out, w_out] written once. */
int asr_standard_labels_i32(const float* logits0, int32_t* labels, int h_in, int w_in, int classes, int h_out, int w_out,
                            const int* ids, int K, asr_stream_t stream);

/* Per-label pixel counts for the multi-class Mean_IOU (utils.py:151-177, compute_IoU(class_id=None)):
 * counts[seg][0][l] = |truth == l|, counts[seg][1][l] = |pred == l|, counts[seg][2][l] = |truth == l and pred == l|,
 * l = 0..255 (int64, zeroed by the call); IoU_l = c2 / (c0 + c1 - c2). */
int asr_class_counts_i32(const int32_t* truth, const int32_t* pred, int64_t* counts, int64_t per_segment, int segments,
                         asr_stream_t stream);

/* --- trimap: label maps scored inside bands round the ground truth's label boundaries -----------------------------------
 * Definitions (everything is integer; nothing is ever rounded):
 *  - a pixel p of a ground-truth label map T [h, w] (int32) is a BOUNDARY PIXEL when at least one of its 4-neighbours inside
 *    the image holds a different value.  Void (255) is a value like any other here, so the void ring VOC draws round objects
 *    makes boundaries; the image border itself makes none;
 *  - d2(p) is the squared Euclidean distance, in pixels, from p to the nearest boundary pixel (0 on a boundary pixel);
 *  - the BAND OF WIDTH w (integer, 1 <= w <= 64) is {p : d2(p) <= w * w}.  Bands are nested;
 *  - ignore_label (-1 = none): pixels whose truth equals it are counted in no bin, but still make boundaries;
 *  - the band counts of a prediction P against T at width w are counts[0][l], [1][l], [2][l] exactly as
 *    asr_class_counts_i32 defines them, over the pixels of the band that are not ignored.
 * Hence with ignore_label = -1 and a band that covers the image, the band counts are asr_class_counts_i32's bit for bit.
 *
 * asr_boundary_dist2_u16: truth [segments, h, w] int32 -> dist2 [segments, h, w] uint16 = d2(p) where d2(p) <= r_max^2, else
 * 0xFFFF (a map without a boundary is all 0xFFFF).  1 <= r_max <= 64, any h, w >= 1, segments <= 65535.  Not a
 * (2 r_max + 1)^2 window: boundary bits packed by wave ballots, the row distance from two 64-bit windows, then a min over the
 * rows above and below that stops as soon as the row offset alone exceeds the running minimum. */
int asr_boundary_dist2_u16(const int32_t* truth, uint16_t* dist2, int segments, int h, int w, int r_max, asr_stream_t stream);

/* Band counts of num_preds (1..8) predictions [num_preds, pixels] against ONE truth [pixels] and its dist2 [pixels] (the four
 * label maps of an image, shared as asr_iou_counts_shared_truth_i32 shares its truth), for num_widths = B (1..16) widths:
 * widths is a HOST int array read during the call, any order, repeats allowed, each in [1, 64] and <= r_max, the value the
 * distance map was built with (the kernel cannot tell it from its inputs).  counts [num_preds, B, 3, 256] int64, zeroed by the
 * call, in the caller's width order.  Labels outside 0..255 are not counted.  A bad argument returns ASR_ERR_INVALID_ARG
 * before any launch.  One launch reads the planes once for all widths: each pixel is added once, under the narrowest
 * requested width that holds it, and a small second launch turns those into the cumulative counts per width.  Cost: 3 KiB of
 * LDS per DISTINCT width in a workgroup (48 KiB at 16); each prediction is a grid row of its own that re-reads truth and
 * dist2 (6 bytes per pixel, cache-fed), so the time grows with num_preds and hardly with B. */
int asr_band_class_counts_i32(const int32_t* truth, const int32_t* preds, const uint16_t* dist2, const int* widths,
                              int64_t* counts, int64_t pixels, int num_preds, int num_widths, int r_max, int ignore_label,
                              asr_stream_t stream);

/* --- binned counts: label maps scored over the pixels whose value u lies at or below each of B edges ------------------------
 * (the risk-coverage curve: u an uncertainty map, the edges its quantiles, so that bin j keeps the most certain pixels)
 *  - bin j is {p : u[p] <= edges[j]}, one f32 compare: -0 <= +0 holds, a NaN (in u or as an edge) is in no bin, and an edge of
 *    +inf holds every pixel whose u is not NaN.  Bins are defined independently: the edges need not be sorted or distinct;
 *  - ignore_label (-1 = none): pixels whose truth equals it are in no bin;
 *  - the counts of a prediction P against T in bin j are counts[0][l], [1][l], [2][l] exactly as asr_class_counts_i32
 *    defines them, over the pixels of the bin.  Labels outside 0..255 are not counted (and index nothing).
 * Hence with every edge +inf, no NaN in u and ignore_label = -1, each bin is asr_class_counts_i32's counts bit for bit.
 *
 * asr_binned_class_counts_f32: num_preds (1..8) predictions [num_preds, pixels] against ONE truth [pixels] and ONE u [pixels]
 * f32 (shared as asr_band_class_counts_i32 shares truth and dist2), for num_bins = B (1..16) edges: edges is a DEVICE array of
 * B floats (they come from a selection on the device; nothing is read back).  counts [num_preds, B, 3, 256] int64, zeroed by
 * the call, in the caller's edge order.  A bad argument returns ASR_ERR_INVALID_ARG before any launch.  One launch: each
 * prediction is a grid row of at most 64 workgroups (or as many as keep a workgroup below 2^32 pixels) that re-reads truth and
 * u (cache-fed); a pixel is added once per bin that holds it.  3 KiB of LDS per bin in a workgroup (48 KiB at 16). */
int asr_binned_class_counts_f32(const int32_t* truth, const int32_t* preds, const float* u, const float* edges,
                                int64_t* counts, int64_t pixels, int num_preds, int num_bins, int ignore_label,
                                asr_stream_t stream);

/* --- confusion matrix: where the pixels of each ground-truth label go in a label map --------------------------------------
 * Definitions (everything is integer):
 *  - num_labels = L (1..64) labels 0..L-1 are told apart; bin(v) = v when 0 <= v < L, else L.  Bin L is OTHER: void (255),
 *    negative values and every id >= L;
 *  - the confusion matrix of a prediction P against a ground truth T is M [L+1, L+1] int64, truth in the rows:
 *    M[i][j] = |{x : bin(T[x]) == i and bin(P[x]) == j}|.
 * Hence M sums to pixels, and for l < L row sum l, column sum l and M[l][l] are asr_class_counts_i32's counts[0][l],
 * counts[1][l] and counts[2][l], bit for bit.
 *
 * asr_confusion_counts_i32: num_preds (1..8) predictions [num_preds, pixels] against ONE truth [pixels] (shared as
 * asr_band_class_counts_i32 shares its truth) -> counts [num_preds, L+1, L+1] int64, zeroed by the call.  A bad argument
 * returns ASR_ERR_INVALID_ARG before any launch.  One launch: each prediction is a grid row that re-reads the truth
 * (cache-fed); a workgroup of 256 threads takes ASR_CONFUSION_SPAN pixels per trip of its grid-stride loop, and a grid row
 * has at most ASR_CONFUSION_GRID workgroups, or as many as keep a workgroup below 2^32 pixels.  (L+1)^2 * 4 bytes of LDS
 * per workgroup: 1.9 KiB at L = 21, 16.5 KiB at L = 64. */
#define ASR_CONFUSION_MAX_LABELS 64
#define ASR_CONFUSION_MAX_PREDS 8
#define ASR_CONFUSION_SPAN 1024
#define ASR_CONFUSION_GRID 64
int asr_confusion_counts_i32(const int32_t* truth, const int32_t* preds, int64_t* counts, int64_t pixels, int num_preds,
                             int num_labels, asr_stream_t stream);

/* --- guided filter: score planes refined against the image before they are thresholded or fused ----------------------------
 * The guided filter of He, Sun and Tang ("Guided Image Filtering", ECCV 2010 / TPAMI 2013) with a colour guide: one
 * deterministic pass that moves the boundary of an upsampled score map onto the edges of the image it was computed from.
 *  - guide I [H, W, 3] f32 (the project's images are in [0, 1]); input p [P, H, W] f32; output q [P, H, W] f32;
 *  - radius r, an integer, 0 <= r <= 32; eps finite and > 0;
 *  - the window w_k is the (2r+1)^2 square centred at pixel k, CLIPPED to the image; N_k is the number of pixels it keeps.
 *    No padding, no reflection.
 * The rule, for every pixel k and every plane (U = 3x3 identity):
 *    mu_k = (1/N_k) sum_{j in w_k} I_j                          (3-vector)
 *    S_k  = (1/N_k) sum_{j in w_k} I_j I_j^T - mu_k mu_k^T      (3x3, symmetric)
 *    m_k  = (1/N_k) sum_{j in w_k} p_j
 *    c_k  = (1/N_k) sum_{j in w_k} I_j p_j - mu_k m_k           (3-vector)
 *    a_k  = (S_k + eps U)^-1 c_k
 *    b_k  = m_k - a_k^T mu_k
 *    q_i  = ((1/N_i) sum_{k in w_i} a_k)^T I_i + (1/N_i) sum_{k in w_i} b_k
 * Everything is f32.  The implementation centres the guide (tile by tile, on a guide value of the tile: covariances do not
 * change with a shift) and sums each window's terms directly in a fixed order -- never a running sum or a summed-area table,
 * whose cancellation (S + eps U)^-1 would amplify by up to 1/eps.  No atomics: the same input gives the same bits on every
 * call, and every plane of a P-plane call is bit for bit what a one-plane call gives for it.
 *
 * asr_guided_prepare_f32: the guide-only pass, once per image whatever the number of planes.  state receives
 * asr_guided_state_bytes(H, W) = 9 * 4 * H * W bytes: per pixel the window mean of the (centred) guide and the six numbers
 * of the factorisation S_k + eps U = L diag(d) L^T (l10, l20, l21, 1/d0, 1/d1, 1/d2), from which a_k is two triangular
 * solves; its layout is private to the library and belongs to this (H, W, r, eps) and this guide.
 * asr_guided_apply_f32: p -> q with the state and the guide it was prepared from, and the same H, W, r.  Two launches: window
 * sums of p and I p give a_k and b_k, 4 floats per pixel and plane, into workspace (asr_guided_workspace_bytes(planes, H, W)
 * = 16 * planes * H * W bytes, fully rewritten by each call); window means of those give q.  q may alias p.
 * Null pointers, H or W < 1, planes < 1, r < 0 and an eps that is not finite and > 0 return ASR_ERR_INVALID_ARG; r > 32
 * returns ASR_ERR_UNSUPPORTED (the message names the cap), as do more than 65535 planes in one call (a plane is a grid
 * layer).  Refusals happen before any launch and nothing is written.  The two size functions are host arithmetic (no GPU)
 * and return 0 for a size below 1.
 * A workgroup owns a 32 x 32 tile and stages it with its r-wide halo in LDS: with R = 32 + 2r, 4 * (4 * R * (R + 1) + 33 * R)
 * bytes in asr_guided_apply_f32, 43 KiB at r = 8, 158 KiB (one workgroup per CU) at r = 32. */
size_t asr_guided_state_bytes(int H, int W);
size_t asr_guided_workspace_bytes(int planes, int H, int W);
int asr_guided_prepare_f32(const float* guide, void* state, int H, int W, int r, float eps, asr_stream_t stream);
int asr_guided_apply_f32(const void* state, const float* guide, const float* p, float* q, void* workspace, int planes, int H,
                         int W, int r, asr_stream_t stream);

/* --- regions: connected components of a label map, and the label map cleaned of its small ones -----------------------------
 * (what is elsewhere called remove_small_objects / remove_small_holes, or an area opening, for every value at once)
 * Definitions (everything is integer; nothing is ever rounded):
 *  - a label map is int32 [h, w], linear index y * w + x; the connectivity c is 4 or 8;
 *  - a REGION is a maximal set of pixels of equal value that is connected by c-neighbour steps inside the image.  Every value
 *    makes regions: 0, 255, negative values and ids alike.  The image border connects nothing;
 *  - root[p] is the smallest linear index of p's region and area[p] that region's pixel count: functions of the input alone,
 *    independent of dispatch order and bit-identical from call to call;
 *  - for a threshold min_area >= 1 a region is SMALL when area < min_area;
 *  - the SURROUND V(R) of a small region R is the set of values of the pixels q outside R that are c-adjacent to a pixel of R,
 *    lie inside the image, and whose own region is not small: small regions never vote;
 *  - the CLEANED MAP: out[p] = labels[p] when p's region is not small; else the single element of V(R) when |V(R)| = 1; else
 *    0 ("no class").  One pass over the regions of the INPUT; it is not iterated.
 * Hence: min_area = 1 returns the input bit for bit; min_area > h * w returns all zeros; a small island inside one large
 * region takes that region's value (a pin-hole of 0 inside a class is filled, a speck of a class inside background goes to
 * 0); a small island that touches two large regions of different values goes to 0; two adjacent small regions inside a large
 * 0 region both go to 0; a small region nested in another small region goes to 0, not to the outer small region's value; a
 * small 0-region with a mixed surround stays 0.
 *  - stats [maps, 4] int64, zeroed by the call, per map: the number of regions, the number of small regions, the number of
 *    pixels in small regions, the number of pixels whose value changed.
 *
 * asr_label_regions_i32: labels [maps, h, w] -> root, area [maps, h, w] int32; root holds indices within the pixel's own map.
 * asr_clean_labels_i32: labels with the root and area of the same connectivity -> out [maps, h, w] (out may alias labels) and
 * stats (may be NULL).  Both need a workspace of at least their *_workspace_bytes(maps, h, w) bytes, 4-byte aligned, fully
 * rewritten by each call (host arithmetic, 0 for a size below 1); a short one returns ASR_ERR_WORKSPACE.  Null pointers, a
 * connectivity other than 4 or 8, min_area < 1, h or w < 1, h * w > 2^31 - 1 and maps outside 1..65535 (a map is a grid
 * layer) return ASR_ERR_INVALID_ARG.  Refusals happen before any launch and nothing is written.
 * How: a workgroup of 256 threads labels one ASR_REGIONS_TILE_W x ASR_REGIONS_TILE_H tile by union-find in LDS (links made
 * by atomic min, so parent[i] <= i always); a second launch joins the neighbour pairs that straddle a tile border with the
 * same routine on global memory; a third flattens and adds each tile-local pixel count once to its region's root; a fourth
 * spreads the areas.  The clean-up keeps, per small region, the minimum and maximum of the non-small neighbours' values
 * (|V| = 1 exactly when they are equal).  Phases are separate launches on the caller's stream: no workgroup ever waits for
 * another, and every walk is a counted loop (a root of -1 would report an overrun, which parent[i] <= i excludes).  An
 * address receives one atomic per tile, wave or workgroup, never one per pixel. */
#define ASR_REGIONS_TILE_W 32
#define ASR_REGIONS_TILE_H 32
size_t asr_label_regions_workspace_bytes(int maps, int h, int w);
int asr_label_regions_i32(const int32_t* labels, int32_t* root, int32_t* area, void* workspace, size_t workspace_bytes,
                          int maps, int h, int w, int connectivity, asr_stream_t stream);
size_t asr_clean_labels_workspace_bytes(int maps, int h, int w);
int asr_clean_labels_i32(const int32_t* labels, const int32_t* root, const int32_t* area, int32_t* out, int64_t* stats,
                         void* workspace, size_t workspace_bytes, int maps, int h, int w, int connectivity, int min_area,
                         asr_stream_t stream);

/* --- segments: a label map scored region by region against the ground truth (panoptic quality) -----------------------------
 * The rule takes a truth map, a prediction map, a label count, a connectivity and a background flag (everything is integer):
 *  - the truth T and a prediction P are int32 [h, w]; L = num_labels is the number of labels told apart, 1 <= L <= 64
 *    (ASR_SEGMENTS_MAX_LABELS); the connectivity c is 4 or 8; the flag include_zero is off by default;
 *  - the SEGMENT VALUES are v0 .. L-1, with v0 = 0 when include_zero is set, else 1: value 0 is "no class" and makes no segments
 *    by default;
 *  - a pixel is VOID when T there is outside 0 .. L-1 (255, negatives, ids >= L).  Void pixels belong to no truth segment; they
 *    are taken out of every predicted segment's area and out of every intersection;
 *  - a TRUTH SEGMENT g is a region of T (the regions section's definition, connectivity c) with a segment value; A_g is its
 *    pixel count;
 *  - a PREDICTED SEGMENT p is a region of P with a segment value.  It is labelled on the whole map, so void pixels do not cut a
 *    region; A_p is the number of its pixels where T is not void.  A predicted segment with A_p = 0 is DROPPED and counted
 *    nowhere;
 *  - the INTERSECTION I(g, p) = |g n p|;
 *  - g and p MATCH when their values are equal and 3 I > A_g + A_p, that is I / (A_g + A_p - I) > 1/2, strictly, in integers:
 *    an IoU of exactly 1/2 is no match.  A segment is in at most one match: 3 I > A_g + A_p with A_g >= I gives 2 I > A_p, so
 *    two matches (g, p) and (g', p) of one p would have I + I' > A_p, but truth segments are disjoint and hold no void pixel,
 *    so I + I' <= A_p: two matches would need more than all of p's pixels.  The same with the roles swapped (A_p >= I, the
 *    predicted segments disjoint) holds for one g and two predicted segments;
 *  - per segment value v: TP_v the matches, FN_v the unmatched truth segments of value v, FP_v the unmatched, non-dropped
 *    predicted segments of value v, and Q_v = sum over the matches of floor(I * 2^30 / (A_g + A_p - I))
 *    (ASR_SEGMENTS_IOU_ONE = 1 << 30; I < 2^31, so the product fits an int64; one 64-bit integer division per match).
 * Nothing is rounded except that one floor, and Q_v is a sum of integers: the result does not depend on arrival order, is
 * bit-identical from call to call and to a restatement in Python integers; the error per match is below 2^-30.
 *
 * asr_segment_match_i32: truth, truth_root, truth_area [h, w] and preds, pred_root [maps, h, w] int32, the roots and the area
 * those of asr_label_regions_i32 at the caller's connectivity (the match itself does not need c) -> counts [maps, L, 4] int64
 * (TP, FP, FN, Q), zeroed by the call, rows below v0 left zero: one entry for each prediction map against the one shared truth.
 * Two optional int32 planes [maps, h, w], either of which may be NULL:
 *    pred_match   pixels of P in a matched segment: the root of the matched truth segment; in an unmatched, non-dropped
 *                 segment: -1; of a non-segment value or in a dropped segment: -2
 *    truth_match  pixels of T in a matched segment: the matched predicted root; in an unmatched segment: -1; void or of a
 *                 non-segment value: -2
 * The workspace holds at least asr_segment_match_workspace_bytes(maps, h, w) bytes, 8-byte aligned (as counts is), and is fully
 * rewritten by each call (host arithmetic, 0 for a size below 1); a short one returns ASR_ERR_WORKSPACE.  Null pointers among
 * the required arguments, num_labels outside 1..64, h or w < 1, h * w > 2^31 - 1 and maps outside 1..65535 (a map is a grid
 * layer) return ASR_ERR_INVALID_ARG.  Refusals happen before any launch and nothing is written.
 * How: the pixels that count are those whose predicted value is a segment value and whose truth is not void.  A workgroup of
 * 256 threads owns an ASR_REGIONS_TILE_W x ASR_REGIONS_TILE_H tile and gathers the tile's distinct (truth root, predicted root)
 * pairs with their pixel counts in an open-addressed LDS table (a tile has at most 1024 of them, the table 2048 slots); it then
 * adds each distinct pair once to the map's table in the workspace, keyed by the 64-bit pair: the key is claimed with a 64-bit
 * compare-and-swap, the count added with an integer atomic add, so an address receives one atomic per pair and tile, never one
 * per pixel.  That table has the power of two at or above 2 h w slots and a map at most h w distinct pairs, so no input can
 * fill it: there is no overflow path.  Later launches walk the table: one accumulates A_p, the next decides the matches and
 * adds TP and Q (per workgroup in LDS first); a last pass over the pixels counts FN and FP from the pixels that are their own
 * root and writes the planes.  Phases are separate launches on the caller's stream: no workgroup ever waits for another, every
 * probe sequence and every walk is a counted loop, and the atomics are integer, device scope, relaxed -- a kernel boundary is
 * the only ordering relied on.  A root outside the map (the planes are the caller's) takes its pixel out of the count. */
#define ASR_SEGMENTS_MAX_LABELS 64
#define ASR_SEGMENTS_IOU_ONE (1 << 30)
size_t asr_segment_match_workspace_bytes(int maps, int h, int w);
int asr_segment_match_i32(const int32_t* truth, const int32_t* truth_root, const int32_t* truth_area, const int32_t* preds,
                          const int32_t* pred_root, int64_t* counts, int32_t* pred_match, int32_t* truth_match, void* workspace,
                          size_t workspace_bytes, int maps, int h, int w, int num_labels, int include_zero, asr_stream_t stream);

/* --- windowed CRF: label maps decided jointly over classes and image ------------------------------------------------------
 * Mean-field inference of a dense CRF with Potts compatibility whose pairwise terms reach a (dilated) window round each pixel
 * -- the locally connected form of ConvCRF (Teichmann and Cipolla, "Convolutional CRFs for Semantic Segmentation") of the
 * dense CRF of Kraehenbuehl and Koltun: exact message passing inside the window, no lattice, no atomics.
 *  - labels l = 0 .. L-1, 2 <= L <= 32: label 0 is "no class", label l >= 1 is class ids[l-1] (ids: K = L - 1 distinct ids >= 1,
 *    a HOST int array as in the label-map section);
 *  - unaries z [L, H, W] f32, finite; guide I [H, W, 3] f32 (the project's images are in [0, 1]);
 *  - asr_crf_config: radius r in 1..7; dilation d >= 1 with r d <= 16; iterations T in 0..32; w_app, w_smooth finite and >= 0;
 *    theta_pos, theta_rgb, theta_smooth finite and > 0.
 * Weights.  The neighbours of p are q = p + d (dy, dx), |dy|, |dx| <= r, (dy, dx) != (0, 0), q inside the image (a CLIPPED
 * window, as in the guided filter).  With delta^2 = d^2 (dy^2 + dx^2):
 *    a(p,q) = exp(max(-delta^2 / (2 theta_pos^2) - |I_p - I_q|^2 / (2 theta_rgb^2), -80))
 *    g(p,q) = exp(max(-delta^2 / (2 theta_smooth^2), -80))
 * The clamp keeps every weight a normal f32 number: no normaliser underflows to 0, and a pixel whose colour is far from all
 * its neighbours still averages them by distance.
 * Iteration.  Q^0 = softmax_l(z).  For t = 1 .. T, all pixels in parallel from Q^{t-1} (ping-pong buffers):
 *    s_l(p) = z_l(p) + w_app sum_q a Q_l^{t-1}(q) / sum_q a + w_smooth sum_q g Q_l^{t-1}(q) / sum_q g
 *    Q^t = softmax_l(s), the maximum subtracted first.
 * A pixel without neighbours (the 1 x 1 image) has both terms equal to 0.
 * Output.  labels[p] = the id of argmax_l over the FINAL LOGITS s (z when T = 0), equal values going to the lowest l; q_out,
 * when not NULL, receives Q^T [L, H, W].  Everything is f32; the sums run over the offsets in ascending (dy, dx) order; the same
 * input gives the same bits on every call.
 *
 * Unaries, both specified to the bit:
 * asr_crf_unaries_scores_f32: scores [K, pixels] (plane k: the SR output S_k of class ids[k], what asr_fuse_labels_f32 reads)
 *   -> z [K + 1, pixels]: z_0 = 0, z_{k+1} = (S_k - t_k) / tau with t_k = max(S_k) * th_factor, the f32 product of
 *   asr_fuse_labels_f32, then one f32 subtraction and one f32 division; tau finite and > 0.  minmax_ws: [K, 2] floats of scratch
 *   (asr_minmax_f32's extrema, as in the fusion).  S_k > t_k exactly when S_k - t_k > 0 (gradual underflow), and with tau <= 1
 *   the division cannot round a non-zero margin to zero; hence, for tau <= 1, with T = 0 the label map is asr_fuse_labels_f32's
 *   bit for bit at K = 1, and for K > 1 wherever at most one class passes.  (With tau > 1 a subnormal margin can round to 0 and
 *   the pixel then falls to label 0.)  Where several classes pass, the MARGIN S_k - t_k ranks them here, not S_k as
 *   in the fusion: a class of a small maximum can win over a class of a greater score.  There is no max-map (slice_max) form: the
 *   pass rule S >= Smax there is not a threshold.
 * asr_crf_unaries_labels_f32: an int32 label map [pixels] -> z [L, pixels], the unary_from_labels of common CRF practice:
 *   z_l = log(conf) where the map holds label l's id (0 for l = 0), log((1 - conf) / (L - 1)) for the other l; all z_l = 0 where
 *   the map holds a value outside {0} u ids.  conf in (1/L, 1); the two logarithms are taken on the host in double, of the f32
 *   conf, and rounded once to f32.
 * asr_crf_refine_f32: one launch for Q^0, one per iteration, the last of which writes the labels (T = 0: a single launch).
 *   workspace: asr_crf_workspace_bytes(L, H, W) = 2 * 4 * L * H * W bytes (the two Q buffers; host arithmetic, 0 for a bad size),
 *   4-byte aligned, required whatever T is.  q_out must not overlap z (the launches read z while they park logits in q_out):
 *   an overlap returns ASR_ERR_INVALID_ARG.
 * Null pointers and bad values return ASR_ERR_INVALID_ARG; a value beyond a cap (radius > 7, radius * dilation > 16,
 * iterations > 32, L > 32 or K > 31) returns ASR_ERR_UNSUPPORTED and the message names the cap.  Refusals happen before any
 * launch and nothing is written.
 * How: a workgroup of 1024 threads owns a 32 x 32 tile, one pixel per thread, and stages the guide tile with its r d halo in
 * LDS once, then the Q planes with halo in chunks of 8 labels (4 when L <= 4 or when r d > 14, so that the planes fit):
 * 4 * (452 + (3 + chunk) * R * (R + 1)) bytes with R = 32 + 2 r d (452 floats: two per-offset tables).  Within a chunk the offset loop is outermost, so a and g are formed
 * once per pixel, offset and chunk.  No workgroup ever waits for another. */
typedef struct asr_crf_config {
    int radius;          /* r: the window is (2r+1)^2 offsets */
    int dilation;        /* d: offsets are d * (dy, dx) */
    int iterations;      /* T mean-field iterations */
    float w_app;         /* weight of the appearance (bilateral) kernel a */
    float w_smooth;      /* weight of the smoothness kernel g */
    float theta_pos;     /* spatial width of a, pixels */
    float theta_rgb;     /* colour width of a, in the guide's units */
    float theta_smooth;  /* spatial width of g, pixels */
} asr_crf_config;
size_t asr_crf_workspace_bytes(int L, int H, int W);
int asr_crf_unaries_scores_f32(const float* scores, float* minmax_ws, float* z, int64_t pixels, int K, float th_factor,
                               float tau, asr_stream_t stream);
int asr_crf_unaries_labels_f32(const int32_t* labels, float* z, int64_t pixels, const int* ids, int L, float conf,
                               asr_stream_t stream);
int asr_crf_refine_f32(const float* guide, const float* z, const int* ids, int L, int H, int W, const asr_crf_config* cfg,
                       void* workspace, int32_t* labels, float* q_out, asr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * DeepLabV3+ (Xception-65, OS16) layers -- model.py.  BatchNorm is folded by the caller.
 * ------------------------------------------------------------------------------------------ */

/* Packed-weight size (floats) and packing for the MFMA GEMM: w_kn [k,n] row-major (a Keras
 * HWIO kernel reshaped to [kh*kw*cin, cout]) -> private layout [ceil32(k)/4][ceil128(n)][4]. */
size_t asr_pwconv_packed_floats(int k, int n);
int asr_pwconv_pack_weights_f32(const float* w_kn, float* w_packed, int k, int n, asr_stream_t stream);

/* Conv2D 1x1 (+ folded BN bias, optional ReLU, optional residual Add) on FP32 MFMA:
 * y[r, :n] = act(x[row(r), :k] @ W + bias) + residual[r, :n].  Replaces every pointwise
 * Conv2D + BatchNormalization (+ ReLU / Add) group of model.py (:195-231, :244-247, :303-304,
 * :403-417, :500-506).  sub_stride > 1: rows are gathered at (b, s*oy, s*ox) of an
 * h_in x w_in map -- the stride-2 1x1 shortcut of _conv2d_same (model.py:529-541).
 * relu: 0 = linear, 1 = ReLU, 2 = ReLU6 (the expand convs of _inverted_res_block, model.py:434-440; the same
 * encoding is used by every `relu` / `post_relu` argument below).  k % 4 == 0, ldx % 4 == 0. */
int asr_pwconv_mfma_f32(const float* x, const float* w_packed, const float* bias, const float* residual, float* y,
                        int64_t m, int k, int n, int ldx, int ldy, int ldres, int relu, int sub_stride, int h_in,
                        int w_in, asr_stream_t stream);

/* Split-f16 variant of asr_pwconv_mfma_f32 (same arguments, n > 64): every f32 operand is split into
 * f16 hi + lo on the way into LDS and x*w is evaluated as hi*hi + hi*lo + lo*hi on
 * v_mfma_f32_32x32x16_f16 with f32 accumulation -- f32-grade results (error ~1e-6 of sum |x||w|) at
 * 3/16 of the FP32-MFMA matrix time.  Weights are packed by asr_pwconv_pack_weights_f16x3
 * (asr_pwconv_packed_floats_f16x3 floats: two half planes [ceil32(k)/8][ceil128(n)][8]). */
size_t asr_pwconv_packed_floats_f16x3(int k, int n);
int asr_pwconv_pack_weights_f16x3(const float* w_kn, float* w_packed, int k, int n, asr_stream_t stream);
int asr_pwconv_mfma_f16x3(const float* x, const float* w_packed, const float* bias, const float* residual, float* y,
                          int64_t m, int k, int n, int ldx, int ldy, int ldres, int relu, int sub_stride, int h_in,
                          int w_in, asr_stream_t stream);

/* Conv2D 3x3 as implicit GEMM on FP32 MFMA (cin % 32 == 0): entry_flow_conv1_2, model.py:155-159. */
int asr_conv3x3_mfma_f32(const float* x, const float* w_packed, const float* bias, float* y, int batch, int h_in,
                         int w_in, int cin, int cout, int stride, int pad, int dil, int h_out, int w_out, int ldx,
                         int ldy, int relu, asr_stream_t stream);

/* The same 3x3 implicit GEMM on the split-f16 matrix path (asr_pwconv_mfma_f16x3): w_packed from
 * asr_pwconv_pack_weights_f16x3 on the [9 * cin, cout] matrix; cin % 32 == 0. */
int asr_conv3x3_mfma_f16x3(const float* x, const float* w_packed, const float* bias, float* y, int batch, int h_in,
                         int w_in, int cin, int cout, int stride, int pad, int dil, int h_out, int w_out, int ldx,
                         int ldy, int relu, asr_stream_t stream);

/* --- split-f16 activations between the two halves of a separable conv ------------------------------------------
 * The depthwise output of _SepConv_BN (model.py:478-495) is consumed only by its pointwise conv.  Written directly in
 * the A-operand format of the split-f16 GEMM -- per pixel and per chunk of 32 channels one 128-byte line
 * [hi(32 halfs) | lo(32 halfs)], hi = f16(v), lo = f16(v - hi): the very split asr_pwconv_mfma_f16x3 applies to the
 * f32 value on its way into LDS, and the same number of bytes -- it lets the GEMM take both operands by LDS-DMA
 * (no staging registers, no conversion work) on a 256 x 256 tile.  Same hi / lo halves, same three products; the 256 x 256
 * kernel sums each 32-deep K-step in one v_mfma_f32_16x16x32_f16, so it differs from asr_dwconv3x3_nhwc_f32 followed by
 * asr_pwconv_mfma_f16x3 by f32 summation-order noise only (both within 4e-6 * sum |x||w| of the exact product).
 *
 * asr_dwconv3x3_nhwc_split_f16: asr_dwconv3x3_nhwc_f32 with y in that format; ldy_chunks = ceil(c / 32) chunks per
 * pixel, channels c .. 32 * ldy_chunks - 1 are written as zeros; needs (stride 1, rate 1|2) or (stride 2, rate 1) and
 * h_out a multiple of 16 (32 above 32 rows); y_split 128-byte aligned.
 * asr_pwconv_mfma_f16x3_presplit: asr_pwconv_mfma_f16x3 on such an operand (m rows = pixels, ldx_chunks chunks per
 * row); ceil128(n) must be a multiple of 256; no sub_stride. */
int asr_dwconv3x3_nhwc_split_f16(const float* x, const float* w, const float* bias, void* y_split, int batch, int h_in,
                                 int w_in, int c, int stride, int rate, int pad_top, int pad_left, int h_out, int w_out,
                                 int ldx, int ldy_chunks, int pre_relu, int post_relu, asr_stream_t stream);
int asr_pwconv_mfma_f16x3_presplit(const void* x_split, const float* w_packed, const float* bias, const float* residual,
                                   float* y, int64_t m, int k, int n, int ldx_chunks, int ldy, int ldres, int relu,
                                   asr_stream_t stream);

/* 1 when asr_aspp_dwconv3_nhwc_{f32,split_f16} can run an h x w plane at these three rates (a residue class of the plane
 * modulo gcd(rates) must fit the CU's LDS in one of the kernel's column groupings), else 0: the caller then runs the three
 * branches (model.py:214-221) as separate asr_dwconv3x3_nhwc_f32 launches.  Host arithmetic only -- no device call, no
 * stream; the same function the launchers use, so a plan built on its answer never meets ASR_ERR_UNSUPPORTED for geometry. */
int asr_aspp_dwconv3_supported(int h, int w, int rate0, int rate1, int rate2);

/* asr_aspp_dwconv3_nhwc_f32 with its three outputs as split-f16 operands (ldy_chunks = c / 32; c % 32 == 0). */
int asr_aspp_dwconv3_nhwc_split_f16(const float* x, const float* w3, const float* bias3, void* y0, void* y1, void* y2,
                                    int batch, int h, int w, int c, int rate0, int rate1, int rate2, int ldx,
                                    int ldy_chunks, int pre_relu, int post_relu, asr_stream_t stream);

/* Conv2D 3x3 for tiny cin, weights HWIO [3,3,cin,cout]: entry_flow_conv1_1, model.py:150-153
 * ('same' with stride 2 on an even input pads bottom/right only: pad_top = pad_left = 0). */
int asr_conv3x3_direct_f32(const float* x, const float* w, const float* bias, float* y, int batch, int h_in, int w_in,
                           int cin, int cout, int stride, int pad_top, int pad_left, int h_out, int w_out, int ldx,
                           int ldy, int relu, asr_stream_t stream);

/* The same layer (cin = 3, cout = 32 only) as an implicit GEMM on split-f16 MFMA (K = 27 padded to 32; hi*hi + hi*lo +
 * lo*hi with f32 accumulation: f32-grade results, like asr_pwconv_mfma_f16x3).  Same arguments. */
int asr_conv3x3_stem_f16x3(const float* x, const float* w, const float* bias, float* y, int batch, int h_in, int w_in,
                           int cin, int cout, int stride, int pad_top, int pad_left, int h_out, int w_out, int ldx,
                           int ldy, int relu, asr_stream_t stream);

/* entry_flow_conv1_1 + BN + ReLU + entry_flow_conv1_2 + BN + ReLU (model.py:150-155) in one kernel on split-f16 MFMA:
 * x [batch,h_in,w_in,3] (even sizes) -> y [batch,h_in/2,w_in/2,64].  w1 [3,3,3,32] HWIO and b1 [32], b2 [64] with the BNs
 * folded; w2_packed = asr_pwconv_pack_weights_f16x3 of the [288, 64] matrix (rows (ky, kx, cin)).  The 32-channel
 * intermediate stays in LDS. */
int asr_entry_stem_f16x3(const float* x, const float* w1, const float* b1, const void* w2_packed, const float* b2, float* y,
                         int batch, int h_in, int w_in, int ldx, int ldy, asr_stream_t stream);

/* A whole _SepConv_BN (model.py:463-508) in one kernel for the high-resolution entry-flow layers: [ReLU ->] depthwise
 * 3x3 (stride 1, rate 1, 'same') + BN [-> ReLU] -> pointwise 1x1 + BN [-> ReLU]; cin in {64, 128}, cout = 128.  The
 * depthwise output goes to LDS as split-f16 lines and is consumed there by the MFMA GEMM (weights resident in LDS);
 * bit-identical to asr_dwconv3x3_nhwc_f32 followed by asr_pwconv_mfma_f16x3.  w_dw [3,3,cin], w_pw_packed from
 * asr_pwconv_pack_weights_f16x3 of the [cin, cout] matrix. */
int asr_sepconv_fused_f16x3(const float* x, const float* w_dw, const float* bias_dw, const void* w_pw_packed,
                            const float* bias_pw, float* y, int batch, int h, int w, int cin, int cout, int ldx, int ldy,
                            int pre_relu, int dw_relu, int out_relu, asr_stream_t stream);

/* DepthwiseConv2D 3x3 (+ ZeroPadding2D, folded BN, ReLU before and/or after): the depthwise half
 * of _SepConv_BN, model.py:478-495, and of _inverted_res_block, model.py:442-449 (post_relu = 2: ReLU6).
 * w [3,3,c] with the BN scale folded, bias [c].
 * mode: 0 = auto, 1 = direct (any stride / rate), 2 = register-window streaming ((stride 1, rate 1|2) or (stride 2, rate 1)).
 * Every output is acc = bias; for (ky, kx) row-major: acc = fma(x, w, acc), whichever kernel runs (a tap outside the image
 * leaves acc unchanged).  INPUTS MUST BE FINITE, for this entry, asr_dwconv3x3_nhwc_split_f16 and the two fused ASPP entries:
 * the full-strip kernels multiply a clamped edge value by a zeroed weight, so an infinity (or NaN) in an edge column yields
 * NaN in the neighbouring outputs where the other kernels, which skip the tap, yield a finite value. */
int asr_dwconv3x3_nhwc_f32(const float* x, const float* w, const float* bias, float* y, int batch, int h_in,
                           int w_in, int c, int stride, int rate, int pad_top, int pad_left, int h_out, int w_out,
                           int ldx, int ldy, int pre_relu, int post_relu, int mode, asr_stream_t stream);

/* The three dilated depthwise convs of the ASPP (aspp1/2/3_depthwise + BN + ReLU, model.py:212-221)
 * fused: each residue class of the plane modulo g = gcd(rates) -- on which the dilated taps close -- is staged in LDS
 * once and read by all three rates (input read from HBM once, any plane size).  w3 [3,3,3,c] (branch major),
 * bias3 [3,c]; stride 1, 'same' padding; ceil(h/g) * ceil(w/g) * 128 bytes must fit the 160 KB LDS (ASR_ERR_UNSUPPORTED
 * otherwise: run asr_dwconv3x3_nhwc_f32 per branch). */
int asr_aspp_dwconv3_nhwc_f32(const float* x, const float* w3, const float* bias3, float* y0, float* y1, float* y2,
                              int batch, int h, int w, int c, int rate0, int rate1, int rate2, int ldx, int ldy,
                              int pre_relu, int post_relu, asr_stream_t stream);

/* GlobalAveragePooling2D(keepdims=True): y[b, :c] = mean over hw pixels (model.py:196-197). */
int asr_gap_f32(const float* x, float* y, int batch, int hw, int c, int ldx, asr_stream_t stream);

/* Resizing(bilinear) / tf.image.resize, half-pixel centres (model.py:109-110, 204-205, 241-242). */
int asr_resize_bilinear_f32(const float* x, float* y, int batch, int h_in, int w_in, int c, int h_out, int w_out,
                            int ldx, int ldy, asr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ASR_HIP_H */
