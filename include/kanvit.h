/*
 * kanvit.h -- C ABI of the MI355X (gfx950) hot-path library for the ViKANformer
 * reference (akshathmangudi/KAN-ViT).
 *
 * The reference has no native / FFI layer at all: its boundary is the Python
 * nn.Module surface.  This header is the boundary the
 * replacement adds UNDERNEATH that surface; each entry point below cites the
 * reference function whose arithmetic it replaces (paths relative to the
 * reference repository root).
 *
 * Conventions (all entry points)
 *   - plain C types only; every pointer is a BORROWED device pointer to fp32
 *     data owned by the caller (a torch tensor, a hipMalloc block, ...), which
 *     must stay alive until the work queued on `stream` has completed;
 *   - asynchronous on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream); no internal synchronisation, no allocation, graph-capturable;
 *   - returns 0 on success, a negative KANVIT_E* code otherwise; never throws,
 *     never exits; kanvit_last_error() gives a thread-local message;
 *   - re-entrant and thread safe for distinct streams.
 */
#ifndef KANVIT_H
#define KANVIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: only what this header declares is exported. */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define KANVIT_ABI_VERSION 7

/* error codes */
#define KANVIT_OK 0
#define KANVIT_EINVAL (-22)      /* bad descriptor / unsupported shape          */
#define KANVIT_ENOMEM (-12)      /* workspace too small                         */
#define KANVIT_EDEVICE (-5)      /* HIP runtime error (no device, launch error) */

/* descriptor flags */
#define KANVIT_FLAG_BF16_MFMA 1  /* contract on the bf16 matrix cores (operands rounded to bf16, fp32 accumulate, fp32
                                    I/O); used for the bf16 configurations, never for the fp32 parity path.  Shapes
                                    the bf16 kernels do not cover silently use the exact fp32 kernels.               */

#define KANVIT_FLAG_UNIFORM_KNOTS 2 /* BSPLINE, spline_order 3: every knot row is g0 + j*h (the layout the reference builds
                                    at models/effkan.py:44-53 and never changes) -> closed-form cubic evaluation of
                                    the 4 non-zero bases instead of the Cox-de Boor recursion.  g0, h are read from
                                    the first two knots of each group.
                                    RBF with G = 8: the centres are c0 + j/rbf_inv_h (FastKAN's own grid, models/
                                    fastkan.py:22-27: linspace centres, denominator = their spacing) -> the eight
                                    Gaussians come from two exp anchors and a two-step recurrence instead of eight
                                    exps (relative error <= ~2e-6 where the anchor exp(-(t-2)^2) / exp(-(t-5)^2) is a
                                    normal number; beyond, values below 4e-24 are flushed to 0: absolute error
                                    <= 4e-24); the caller vouches for the layout.                                  */
#define KANVIT_FLAG_FUSED_LN 8   /* RBF (FastKAN): the LayerNorm in front of the spline path (models/fastkan.py:68) is formed IN the
                                    kernels: u = (x - mean) * rstd * gamma + beta over the I features of the group's x slice,
                                    eps = ln_eps.  bparams of a group = [centres(G) | gamma(I) | beta(I)].  The `u` argument
                                    of the three entry points then carries a statistics buffer float[M][x_group_mod][2]
                                    (mean, rstd per row and x slice): WRITTEN by kanvit_layer_fwd, read by the backward
                                    calls; `du` still receives d loss / d u (the caller applies the LayerNorm backward).
                                    Only shapes for which kanvit_layer_ln_fusable() returns 1.                          */
#define KANVIT_FLAG_SHARED_BPARAMS 4 /* groups that read the same x columns (q, k, v of a head) also have identical
                                    basis parameters, so one basis tile may serve all of them (as for the
                                    parameter-free families).  Honoured for BSPLINE.                                */

#define KANVIT_FLAG_SINE_DFREQ 16 /* SINE, kanvit_layer_bwd_weight only: the generated operand is x * cos(x f_g + p_ig) instead of
                                    sin(x f_g + p_ig), so the result is Q[(i,g)][o] = sum_m dy[m][o] x[m][i] cos(...) and
                                    d loss / d freq_g = sum_{i,o} w[(i,g)][o] Q[(i,g)][o] -- the frequency gradient of a layer
                                    whose INPUT gradient nobody needs (the patch embedding: its input is the image) at the
                                    cost of a second weight-gradient pass instead of the slower input-gradient contraction
                                    (models/sinekan.py:81-91; freq is trainable, sinekan.py:60).  Shapes the register
                                    weight-gradient kernels do not cover are refused (EINVAL).                          */

/* basis families: phi_g(x) generated on the fly, never stored in HBM */
#define KANVIT_LINEAR 0   /* phi = x                               nn.Linear in attention.py:136-142           */
#define KANVIT_CHEBY 1    /* T_g(tanh x), g = 0..degree            models/cheby.py:36-48                       */
#define KANVIT_BSPLINE 2  /* Cox-de Boor B-splines (+ base act)    models/effkan.py:99-132,174-187             */
#define KANVIT_RBF 3      /* exp(-((u-c_g)/h)^2) (+ base act)      models/fastkan.py:29-30,66-76               */
#define KANVIT_SINE 4     /* sin(x f_g + p_ig)                     models/sinekan.py:81-91                     */
#define KANVIT_FOURIER 5  /* cos(k x), sin(k x), k = 1..G          models/nfkan.py:36-52                       */

/*
 * One launch evaluates `groups` independent KAN layers that share M rows:
 *   y[m, g*O + o] = bias[g][o] + sum_i sum_j phi_j(x[m, (g % x_group_mod)*I + i]) * w[g][i*GP + j][o]
 * groups = 1 is a plain layer (patch embedding, model.py:146); groups = 3*H with
 * x_group_mod = H is the per-head q|k|v mapping of MSA (attention.py:191-197)
 * folded over the batch, group index = proj*H + head.
 *
 * GP (generated columns per input feature):
 *   LINEAR 1 | CHEBY G | BSPLINE G+has_base | RBF G+has_base | SINE G | FOURIER 2G
 * Packed weights w: [groups][I*GP][O] row-major, k = i*GP + j, with j ordered
 *   CHEBY   j = degree d                      (cheby_coeffs[i][o][d])
 *   BSPLINE j = basis 0..G-1, then base       (spline_weight*spline_scaler [o][i][j], base_weight[o][i])
 *   RBF     j = centre 0..G-1, then base      (spline_linear.weight[o][i*G+j], base_linear.weight[o][i])
 *   SINE    j = g                             (amplitudes[o][i][g])
 *   FOURIER j = c*G + (k-1), c = 0 cos, 1 sin (fouriercoeffs[c][o][i][k-1])
 * Basis parameters bparams: [groups][bparam_stride] floats per group
 *   BSPLINE knots[I][G+spline_order+1] | RBF centres[G] | SINE freq[G] then phase[I][G] | others: none (NULL)
 */
typedef struct kanvit_layer_desc {
    int32_t family;        /* KANVIT_*                                                      */
    int32_t groups;        /* independent layers in this launch (>= 1)                      */
    int32_t x_group_mod;   /* group g reads x columns [(g % x_group_mod)*I, +I)             */
    int32_t I;             /* input features per group                                      */
    int32_t O;             /* output features per group                                     */
    int32_t G;             /* cheby: degree+1; bspline: grid_size+spline_order; rbf: num_grids;
                              sine: grid_size; fourier: gridsize; linear: 1                 */
    int32_t spline_order;  /* BSPLINE only                                                  */
    int32_t has_base;      /* BSPLINE / RBF: extra base column act(x) per input feature     */
    float rbf_inv_h;       /* RBF: 1 / denominator                                          */
    int32_t flags;         /* KANVIT_FLAG_*                                                  */
    int64_t M;             /* rows                                                          */
    int64_t ldx;           /* row stride (floats) of x and dx                               */
    int64_t ldu;           /* row stride of u and du (RBF; group g uses columns [g*I, +I))  */
    int64_t ldy;           /* row stride of y and dy (group g uses columns [g*O, +O))       */
    int64_t bparam_stride; /* floats between consecutive groups in bparams                  */
    float ln_eps;          /* KANVIT_FLAG_FUSED_LN: epsilon of the fused LayerNorm          */
    int32_t base_act;      /* BSPLINE / RBF with has_base: KANVIT_BASE_* of the base column (0 = SiLU).  Nonzero for
                              another family, with has_base = 0, or outside 0..5 is KANVIT_EINVAL  */
} kanvit_layer_desc;

/*
 * Alignment and strides of kanvit_layer_fwd / kanvit_layer_bwd_input / kanvit_layer_bwd_weight (x, u, w, bparams, bias, y, dy, dx, du,
 * dparam, dw):
 *   - every operand pointer needs 4-byte alignment only;
 *   - ldx, ldu, ldy and bparam_stride need only be at least the documented minimum (x_group_mod*I, groups*I, groups*O, the family's
 *     basis-parameter count), any value; padding between rows is neither read nor written;
 *   - the workspace of kanvit_layer_fwd and kanvit_layer_bwd_input needs 16-byte alignment (KANVIT_ENOMEM otherwise, as for one
 *     that is too small); kanvit_layer_bwd_weight's holds partial sums accessed one float at a time: 4-byte alignment;
 *   - the KANVIT_FLAG_FUSED_LN statistics buffer (the `u` argument) needs 8-byte alignment (KANVIT_EINVAL otherwise);
 *   - an operand off the 16-byte grid, or an ld / bparam_stride that is not a multiple of 4 floats, selects slower kernel forms
 *     (narrower loads, the LDS-tile kernels, the exact fp32 kernels under KANVIT_FLAG_BF16_MFMA) with the same results up to the
 *     order of the fp32 sums.  KANVIT_FLAG_FUSED_LN has register kernels only: a call is served where one of them takes the
 *     operands as they are (the forward with x off the grid or ldx % 4 != 0, the weight gradient with any x, dy, ldx, ldy) and is
 *     refused with KANVIT_EINVAL otherwise (the forward with y, w, bias off the grid or ldy % 4 != 0; the input gradient with x,
 *     dx, dy, w off the grid or ldx, ldy % 4 != 0).
 * Packed operands from a 16-byte aligned allocation (what kanvit/ops.py passes) take the fastest form of their shape.
 */

/* base activations of the BSPLINE / RBF base column (kanvit_layer_desc.base_act): the reference's `base_activation`
 * (models/effkan.py:38, models/fastkan.py:61), whose value the base weights multiply.  Every kernel form of the two families
 * exists for each of them, so a descriptor takes the same kernels whatever its activation.                                */
#define KANVIT_BASE_SILU 0        /* x * sigmoid(x)                                    nn.SiLU (the default)             */
#define KANVIT_BASE_GELU 1        /* x/2 (1 + erf(x / sqrt 2))                         nn.GELU(), F.gelu                 */
#define KANVIT_BASE_GELU_TANH 2   /* x/2 (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3)))     nn.GELU(approximate='tanh')       */
#define KANVIT_BASE_RELU 3        /* max(x, 0), derivative 0 at x = 0                  nn.ReLU(), F.relu                 */
#define KANVIT_BASE_TANH 4        /* tanh x                                            nn.Tanh(), torch.tanh             */
#define KANVIT_BASE_IDENTITY 5    /* x                                                 nn.Identity()                     */

/* 1 if KANVIT_FLAG_FUSED_LN may be set for this layer (register kernels cover forward and both gradients), else 0 */
int kanvit_layer_ln_fusable(const kanvit_layer_desc* d);

/* Backward of the fused LayerNorm (what autograd does for models/fastkan.py:68's nn.LayerNorm), given du from
 * kanvit_layer_bwd_input and the statistics kanvit_layer_fwd wrote:  dx[M][ldx] += LN-backward (IN PLACE, may be NULL),
 * dgamma / dbeta [groups][I] = column sums.  Deterministic (fixed-order partial sums in the workspace).              */
size_t kanvit_layer_ln_bwd_workspace(const kanvit_layer_desc* d);
int kanvit_layer_ln_bwd(const kanvit_layer_desc* d, const float* x, const float* stats, const float* bparams, const float* du,
                        float* dx, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream);

/* ---- fused basis evaluation + coefficient contraction -------------------------------------
 * forward of models/cheby.py:36-48, models/effkan.py:174-187, models/fastkan.py:66-76 (the
 * LayerNorm of :68 is applied by the caller and passed as u; u = NULL means u = x),
 * models/nfkan.py:36-52, models/sinekan.py:81-91, and nn.Linear (attention.py:136-142).
 * With KANVIT_FLAG_FUSED_LN the LayerNorm is applied inside the kernel and `u` is the statistics buffer (see the flag). */
size_t kanvit_layer_fwd_workspace(const kanvit_layer_desc* d);   /* 0 unless KANVIT_FLAG_BF16_MFMA (repacked weights) */
int kanvit_layer_fwd(const kanvit_layer_desc* d, const float* x, const float* u, const float* w,
                     const float* bparams, const float* bias, float* y, void* workspace, size_t workspace_bytes,
                     void* stream);

/* ---- backward w.r.t. the layer input (what torch.autograd derives for the reference) ------
 * dx[m, c*I + i] = sum over the groups g with g % x_group_mod == c of
 *                  sum_j phi_j'(x) * sum_o dy[m, g*O+o] * w[g][i*GP+j][o]     (written, not accumulated)
 * RBF: du[m, g*I+i] gets the spline-path gradient, dx the base-path gradient.
 * SINE: dparam receives per-row-tile partial sums of d loss / d freq, shape
 *       [kanvit_layer_dparam_tiles(d)][groups][G]; the caller sums over dim 0.                */
size_t kanvit_layer_bwd_input_workspace(const kanvit_layer_desc* d);   /* 0 unless KANVIT_FLAG_BF16_MFMA */
int kanvit_layer_bwd_input(const kanvit_layer_desc* d, const float* x, const float* u, const float* w,
                           const float* bparams, const float* dy, float* dx, float* du, float* dparam,
                           void* workspace, size_t workspace_bytes, void* stream);
int64_t kanvit_layer_dparam_tiles(const kanvit_layer_desc* d);
/* 1 if KANVIT_FLAG_SINE_DFREQ may be set for kanvit_layer_bwd_weight on this layer (SINE, a shape the register weight-gradient
 * kernels cover), else 0.  The flag is refused by kanvit_layer_fwd and kanvit_layer_bwd_input.  (ABI >= 6) */
int kanvit_layer_sine_dfreq_ok(const kanvit_layer_desc* d);

/* ---- backward w.r.t. the packed weights ---------------------------------------------------
 * dw[g][i*GP+j][o] = sum_m phi_j(x[m, ...i]) * dy[m, g*O+o]; split over row ranges into
 * partial slabs in `workspace`, then reduced in a fixed order (deterministic, no atomics).   */
size_t kanvit_layer_bwd_weight_workspace(const kanvit_layer_desc* d);
int kanvit_layer_bwd_weight(const kanvit_layer_desc* d, const float* x, const float* u, const float* bparams,
                            const float* dy, float* dw, void* workspace, size_t workspace_bytes, void* stream);

/* ---- per-edge mean absolute activation: the KAN paper's regulariser without the (rows, in, out) tensor -------------
 * The reference cannot compute it (models/effkan.py:244-264 says so and regularises the spline WEIGHTS instead); a kernel
 * that generates the basis on the fly can, at the memory cost of its [O, I] result.  d, w, bparams as for kanvit_layer_fwd
 * (groups, x_group_mod, ldx, family, G, spline_order, has_base, base_act, KANVIT_FLAG_UNIFORM_KNOTS mean the same; ldy and
 * the bias are unused):
 *     phi[m, g, i, o] = sum_j Phi_j(x[m, (g % x_group_mod)*I + i]) * w[g][i*GP + j][o]
 *     A[g][i][o]      = (1/M) sum_m |phi[m, g, i, o]|                                   fwd: A [groups][I][O], written
 * bwd, given gA[groups][I][O] = d loss / d A, with s = sign(phi) * gA / M and sign(0) = 0 (as torch.abs differentiates):
 *     dw[g][i*GP + j][o] = sum_m Phi_j(x) * s[m, i, o]
 *     dx[m, c*I + i]     = sum over the groups g with g % x_group_mod == c of
 *                          sum_j Phi_j'(x) * sum_o s[m, i, o] * w[g][i*GP + j][o]       (written; dx may be NULL; row stride ldx)
 * Families: BSPLINE (closed-form uniform cubic under KANVIT_FLAG_UNIFORM_KNOTS, Cox-de Boor for every other order / knot
 * layout, has_base 0 or 1 with any KANVIT_BASE_*), CHEBY, RBF; at most 24 generated columns per feature.  RBF takes the
 * LayerNorm'ed spline input as x; with has_base = 1 the base column reads the layer's raw input from the SAME rows, ldu
 * columns further right (x[m*ldx + ldu + c*I + i]; ldu = 0: the same values, else ldu >= x_group_mod*I), and dx carries both
 * gradients in that layout.
 * LINEAR, SINE, FOURIER, KANVIT_FLAG_FUSED_LN and KANVIT_FLAG_BF16_MFMA (the statistic has no bf16 mode: callers clear the
 * flag and it runs exact fp32 under autocast) are KANVIT_EINVAL, named in kanvit_last_error.
 * The rows are cut into kanvit_edge_l1_row_bands(d) bands (a function of M alone); every band writes a partial result to the
 * workspace (bands x the result's size) and a second kernel adds the partials in band order: no atomics, bitwise
 * reproducible, and a group's result does not depend on the other groups of the launch.  M = 0 writes zeros.
 * kanvit_edge_l1_supported and kanvit_edge_l1_row_bands are pure host functions.  (ABI 7: no struct or version change) */
int kanvit_edge_l1_supported(const kanvit_layer_desc* d);
int64_t kanvit_edge_l1_row_bands(const kanvit_layer_desc* d);
size_t kanvit_edge_l1_fwd_workspace(const kanvit_layer_desc* d);
int kanvit_edge_l1_fwd(const kanvit_layer_desc* d, const float* x, const float* w, const float* bparams, float* A, void* workspace,
                       size_t workspace_bytes, void* stream);
size_t kanvit_edge_l1_bwd_workspace(const kanvit_layer_desc* d);
int kanvit_edge_l1_bwd(const kanvit_layer_desc* d, const float* x, const float* w, const float* bparams, const float* gA, float* dw,
                       float* dx, void* workspace, size_t workspace_bytes, void* stream);

/* ---- B-spline refit to a new knot table: the numerical half of KANLinear.update_grid (models/effkan.py:189-242) -------
 * The reference evaluates the per-edge spline output on the OLD knots into a (rows, in, out) tensor and fits new coefficients
 * to it with lstsq.  The target is a spline in the old basis, so per feature two nb x nb matrices carry the whole problem
 * (nb = d->G = grid_size + spline_order, c = g % x_group_mod):
 *     N[c][i][j][k] = sum_m Bnew_j(x[m, c*I + i]) Bnew_k(x[m, c*I + i])          [x_group_mod][I][nb][nb], float64, written
 *     C[g][i][j][k] = sum_m Bnew_j(x[m, c*I + i]) Bold_k(x[m, c*I + i])          [groups][I][nb][nb],      float64, written
 *     w_new[g][i*nb + :][o] = N[c][i]^-1 C[g][i] w_old[g][i*nb + :][o]           packed as kanvit_layer_fwd's w with has_base = 0
 * d as for kanvit_layer_fwd: family BSPLINE only (every other family is KANVIT_EINVAL, named in kanvit_last_error), has_base = 0
 * and base_act = 0 (the spline weights alone), any spline_order < G and any knots within 40 per feature, G <= 24 (more is
 * KANVIT_EINVAL), KANVIT_FLAG_UNIFORM_KNOTS vouches for the OLD knots only (closed-form cubic for Bold); KANVIT_FLAG_BF16_MFMA
 * is refused (callers clear it: exact fp32 / float64 also under autocast).  old_knots: [groups][bparam_stride] with knots[I][nk]
 * in front, as kanvit_layer_fwd's bparams; new_knots: [x_group_mod][I][nk] contiguous, one table per x slice; ldy and the bias
 * are unused.
 * kanvit_bspline_refit_gram: fp32 sums inside a row band, the bands of kanvit_edge_l1_row_bands (a function of M alone); band
 * partials go to the workspace (bands x 4 x (x_group_mod + groups) x I x nb x nb bytes) and are added in band order in
 * float64: no atomics, bitwise reproducible, and a group's result does not depend on the other groups of the launch.
 * kanvit_bspline_refit_solve: float64 Cholesky of N[c][i], right-hand side and both triangular solves on the device (no host
 * synchronisation, no solver library).  ok[x_group_mod][I] (bytes) is 1 where the fit exists; a feature whose N[c][i] has a
 * Cholesky pivot <= KANVIT_BSPLINE_REFIT_TAU * max_j N[c][i][j][j] or whose matrices hold a non-finite entry (a constant x
 * column, fewer distinct samples than nb, knot intervals of zero width) gets ok = 0 and NOTHING is written to its rows of
 * w_new: the caller keeps that feature's old knots and weights, i.e. its old function.  M = 0: ok = 0 everywhere, no launch.
 * kanvit_bspline_refit_supported and kanvit_bspline_refit_workspace are pure host functions.  (ABI 7: no struct or version change) */
#define KANVIT_BSPLINE_REFIT_TAU 1e-5
int kanvit_bspline_refit_supported(const kanvit_layer_desc* d);
size_t kanvit_bspline_refit_workspace(const kanvit_layer_desc* d);
int kanvit_bspline_refit_gram(const kanvit_layer_desc* d, const float* x, const float* old_knots, const float* new_knots, double* N,
                              double* C, void* workspace, size_t workspace_bytes, void* stream);
int kanvit_bspline_refit_solve(const kanvit_layer_desc* d, const double* N, const double* C, const float* w_old, float* w_new,
                               unsigned char* ok, void* stream);

/* ---- the same fit onto a basis of ANOTHER size: the numerical half of KANLinear.extend_grid ("grid extension") ---------
 * Train on a coarse grid, then carry every edge's function to a finer (or coarser) one.  The descriptor describes the NEW
 * layer, G = nb_new = new_grid_size + spline_order; old_G = nb_old describes the old one; the spline order is the same on both
 * sides, nk_old = old_G + order + 1, nk_new = G + order + 1, both nb <= 24 and both nk <= 40.  With c = g % x_group_mod:
 *     N[c][i][j][k] = sum_m Bnew_j(x) * Bnew_k(x)        [x_group_mod][I][nb_new][nb_new]  float64
 *     C[g][i][j][k] = sum_m Bnew_j(x) * Bold_k(x)        [groups][I][nb_new][nb_old]       float64  (rectangular)
 *     w_new[g][i*nb_new + :][o] = N[c][i]^-1 * C[g][i] * w_old[g][i*nb_old + :][o]
 * Everything else is kanvit_bspline_refit_*'s: the same kernels (old_G = G runs exactly the refit's arithmetic), families, flags
 * and has_base refused alike, KANVIT_FLAG_UNIFORM_KNOTS vouching for the OLD knots only, bparam_stride the stride of old_knots
 * (>= I * nk_old), new_knots [x_group_mod][I][nk_new], the same bands, float64 band-order reduction, Cholesky, pivot rule
 * (KANVIT_BSPLINE_REFIT_TAU) and non-finite check.  A size over the limit is KANVIT_EINVAL and the message names the side
 * ("old nb=25", "new nb=25").  Workspace: bands x 4 x (x_group_mod*I*nb_new^2 + groups*I*nb_new*nb_old) bytes.  ok[c][i] = 0:
 * nothing is written to that feature's rows of w_new (the shapes differ, so the caller cannot keep the old ones: see
 * KANLinear.extend_grid).  M = 0: ok = 0 everywhere, no launch.  (ABI 7: no struct or version change) */
int kanvit_bspline_regrid_supported(const kanvit_layer_desc* d, int old_G);
size_t kanvit_bspline_regrid_workspace(const kanvit_layer_desc* d, int old_G);
int kanvit_bspline_regrid_gram(const kanvit_layer_desc* d, int old_G, const float* x, const float* old_knots, const float* new_knots,
                               double* N, double* C, void* workspace, size_t workspace_bytes, void* stream);
int kanvit_bspline_regrid_solve(const kanvit_layer_desc* d, int old_G, const double* N, const double* C, const float* w_old,
                                float* w_new, unsigned char* ok, void* stream);

/* ---- fused patch embedding --------------------------------------
 * The patch-embedding layer of VisionTransformer.forward (model.py:144-152) with its prologue and epilogue inside the
 * kernel: the rows of x are gathered straight from the NCHW image batch -- row m = (image m / P, patch m % P),
 * feature i = (c, iy, ix) of the patch, i.e. model.py:111-126's patchify without the [B, P, I] staging tensor -- and the
 * output is written as the token sequence the first transformer block reads:
 *     y[b, prepend_rows + p, :] = layer(patch(b, p)) + pos[prepend_rows + p, :]
 *     y[b, 0, :]                = cls + pos[0, :]                    (prepend_rows = 1; model.py:150-152)
 * d describes the layer as for kanvit_layer_fwd with M = B*P rows, I = C*ph*pw, groups = 1; `ldy` is the row stride of y,
 * whose row count is B*(P + prepend_rows).  pos ([P + prepend_rows][O]) and cls ([O]) may be NULL (nothing added /
 * prepend_rows = 0).  Runs on the register-form kernels only: returns KANVIT_EINVAL for shapes they do not cover
 * (O % 32, a feature chunk that does not divide the patch width, FastKAN, which needs u = LayerNorm(x)) -- the caller
 * then uses patchify + kanvit_layer_fwd.  With KANVIT_FLAG_BF16_MFMA the bf16 register-form forward runs the same gather
 * (workspace as kanvit_layer_fwd_workspace(d) reports, ABI >= 7; without the flag no workspace is needed).
 *
 * kanvit_patch_embed_bwd_weight (ABI >= 7): the layer's weight gradient with the same gather on both operands --
 *     dw[i*GP + j][o] = sum_{b,p} phi_j(patch(b, p)[i]) * dy[b, prepend_rows + p, o]
 * x rows come from the NCHW images, dY rows from the token-sequence gradient [B][P + prepend_rows][ldy] as the first block's
 * backward leaves it (class-token rows are stepped over): no transient [B*P, I] patch matrix, no copy of dY.  d as above
 * (M = B*P, `ldy` = row stride of dy); KANVIT_FLAG_SINE_DFREQ as for kanvit_layer_bwd_weight.  Exact fp32: with
 * KANVIT_FLAG_BF16_MFMA (whose short MFMA phases cannot hide the row walker: measured slower than the copy it saves)
 * kanvit_patch_embed_bwd_weight_ok() answers 0.
 * kanvit_patch_embed_bwd_weight_ok() (pure host function) says whether the gathering kernels cover the layer: the patch
 * embeddings VisionTransformer builds (model.py:67-80) with ChebyKAN degree 4, SineKAN and FourierKAN at grid 28 (I, O
 * multiples of 32, M >= 256, 32-bit element offsets); otherwise (efficient-KAN: its weight-gradient kernels have no register
 * left for the row walker and measured slower with it; bf16 mode) the call returns KANVIT_EINVAL and the caller uses
 * patchify + kanvit_layer_bwd_weight. */
typedef struct kanvit_patch_desc {
    int32_t C, H, W;         /* image batch is [B][C][H][W], contiguous                                  */
    int32_t n_patches;       /* patches per side: patch = (H / n_patches) x (W / n_patches) pixels       */
    int32_t prepend_rows;    /* 0, or 1 = a class-token row in front of every image's patch tokens       */
    int32_t reserved;
} kanvit_patch_desc;
int kanvit_patch_embed_fwd(const kanvit_layer_desc* d, const kanvit_patch_desc* p, const float* images, const float* w,
                           const float* bparams, const float* bias, const float* cls, const float* pos, float* y,
                           void* stream);
int kanvit_patch_embed_fwd_ws(const kanvit_layer_desc* d, const kanvit_patch_desc* p, const float* images, const float* w,
                              const float* bparams, const float* bias, const float* cls, const float* pos, float* y,
                              void* workspace, size_t workspace_bytes, void* stream);
int kanvit_patch_embed_bwd_weight_ok(const kanvit_layer_desc* d, const kanvit_patch_desc* p);
size_t kanvit_patch_embed_bwd_weight_workspace(const kanvit_layer_desc* d, const kanvit_patch_desc* p);
int kanvit_patch_embed_bwd_weight(const kanvit_layer_desc* d, const kanvit_patch_desc* p, const float* images,
                                  const float* bparams, const float* dy, float* dw, void* workspace, size_t workspace_bytes,
                                  void* stream);

/* ---- multi-head attention core ------------------------------------------------------------
 * o = softmax(q k^T * scale) v per (batch, head); replaces attention.py:199-200 (MSA) and
 * utils.py:137-227 (FlashAttentionFunction.forward; lse is what it saves for backward).
 * Element (b, h, n, c) of q/k/v/o lives at base[b*stride_b + h*stride_h + n*stride_n + c];
 * lse is [B][H][N] contiguous.  D even, D <= KANVIT_ATTN_MAX_D; one head must fit the 160 KiB
 * LDS of a CU: N <= 256 for D <= 32, N <= 224 for D <= 64.                                   */
#define KANVIT_ATTN_MAX_N 256
#define KANVIT_ATTN_MAX_D 64
typedef struct kanvit_attn_desc {
    int32_t B, H, N, D;
    int32_t causal;         /* utils.py:177-180 with equal q/k lengths */
    float scale;            /* D^-1/2 in both callers */
    int32_t flags;          /* KANVIT_FLAG_BF16_MFMA: products on the bf16 matrix cores (needs D % 16 == 0) */
    int32_t reserved;
    int64_t q_stride_b, q_stride_h, q_stride_n;
    int64_t k_stride_b, k_stride_h, k_stride_n;
    int64_t v_stride_b, v_stride_h, v_stride_n;
    int64_t o_stride_b, o_stride_h, o_stride_n;   /* also the layout of do; dq/dk/dv use the q/k/v strides */
} kanvit_attn_desc;

int kanvit_attn_fwd(const kanvit_attn_desc* d, const float* q, const float* k, const float* v,
                    float* o, float* lse, void* stream);
/* backward of the above; replaces utils.py:229-295 (recompute p from q, k, lse).
 * workspace: kanvit_attn_bwd_workspace(d) bytes (holds rowsum(dO*O), "D" of utils.py:286). */
size_t kanvit_attn_bwd_workspace(const kanvit_attn_desc* d);
int kanvit_attn_bwd(const kanvit_attn_desc* d, const float* q, const float* k, const float* v,
                    const float* o, const float* lse, const float* d_o,
                    float* dq, float* dk, float* dv, void* workspace, size_t workspace_bytes, void* stream);

/* ---- general attention core: q_len != k_len and an attend-mask (ABI >= 7) -----------------------------------------
 * The rest of FlashAttentionFunction's domain (utils.py:134-295): independent query / key lengths (cross-attention through
 * FlashAttention(context=...), attention.py:59-109; utils.py:150-160), a boolean mask broadcastable to [b, h, q_len, k_len]
 * (a [b, k_len] key-padding mask is [b, 1, 1, k_len], utils.py:156-157; nonzero = attend).  `causal` (key j > query i dead)
 * needs k_len <= q_len: with k_len > q_len utils.py:169 shifts the diagonal so that the first k_len - q_len queries see no
 * key and the reference's answer depends on its bucket sizes -- KANVIT_EINVAL here.  d as for kanvit_attn_fwd with
 * d->N = q_len (q, o, do, dq: [B][H][q_len][D] through the q / o strides; k, v, dk, dv: [B][H][Nk][D] through the k / v
 * strides; lse [B][H][q_len]).  Exact fp32 by default.  With KANVIT_FLAG_BF16_MFMA in d->flags and D <= KANVIT_ATTN_MAX_D (64)
 * the products run on the bf16 matrix cores with the rounding points of kanvit_attn_fwd's bf16 mode (operands of S, dP, O, dV,
 * dK, dQ rounded to bf16; softmax, lse, delta, accumulation and all I/O fp32); for D > 64 the flag is refused (KANVIT_EINVAL):
 * there is no bf16 form of the wide heads, and the caller runs them exact.  kanvit_attn_x_bwd must get the flags its forward
 * got: the lse of one mode is not valid input to the other mode's backward.  A query whose keys are all dead gets o = 0,
 * lse = -FLT_MAX, zero gradients.  Any q_len / k_len: the swept operand is walked in LDS chunks of 128 rows (running max / sum in
 * the forward, utils.py:199-221), so these entry points also serve self-attention heads too long for kanvit_attn_fwd's
 * one-head-per-work-group form (N > 224 at D = 64).  Head size: D even and <= KANVIT_ATTN_X_MAX_D, wider than
 * kanvit_attn_fwd's KANVIT_ATTN_MAX_D, so they also serve every head wider than 64 (ViT-H/14: D = 80; D = 128).  The domain
 * grew from D <= 64 to D <= 128, and then by the bf16 mode for D <= 64, without a change of struct, signature or ABI version. */
#define KANVIT_ATTN_X_MAX_D 128
typedef struct kanvit_attn_ext {
    int32_t Nk;              /* key / value length */
    int32_t reserved;
    const void* mask;        /* NULL, or bytes (torch.bool): element (b, h, i, j) at mask[b*sb + h*sh + i*sq + j*sk] */
    int64_t mask_stride_b, mask_stride_h, mask_stride_q, mask_stride_k;      /* in bytes = elements; 0 broadcasts */
} kanvit_attn_ext;
int kanvit_attn_x_fwd(const kanvit_attn_desc* d, const kanvit_attn_ext* e, const float* q, const float* k, const float* v,
                      float* o, float* lse, void* stream);
size_t kanvit_attn_x_bwd_workspace(const kanvit_attn_desc* d, const kanvit_attn_ext* e);
int kanvit_attn_x_bwd(const kanvit_attn_desc* d, const kanvit_attn_ext* e, const float* q, const float* k, const float* v,
                      const float* o, const float* lse, const float* d_o, float* dq, float* dk, float* dv, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---- attention probabilities: the matrix the fused kernels never materialise (attention maps, attention rollout) -----------
 * The reference forms softmax(q k^T / sqrt(d_head)) per sample and head (attention.py:199), so a forward hook on MSA.softmax
 * sees every head's map; kanvit_attn_fwd / kanvit_attn_x_fwd keep only o and the row log-sum-exp.  This entry writes the map:
 *     p[b*p_stride_b + h*p_stride_h + i*p_stride_q + j] = softmax_j(scale * q[b,h,i,:] . k[b,h,j,:])      i < rows, j < e->Nk
 * Domain and semantics are kanvit_attn_x_fwd's, so that a map describes exactly the attention the library computes: d->N =
 * q_len, e->Nk = k_len, both >= 1 and of any size (the keys are walked in LDS chunks of 64 rows); D even and <=
 * KANVIT_ATTN_X_MAX_D; q and k through the q / k strides of d (the packed [B][N][3][H][D] views are read in place; the v and o
 * strides are ignored); the mask through e (required; e->mask may be NULL); `causal` needs k_len <= q_len.  A dead position gets
 * exactly 0.0 and a query with no live key an all-zero row (the counterpart of o = 0, lse = -FLT_MAX).
 * rows in [1, d->N]: only the first `rows` queries of every (b, h) are computed and written (rows = 1: the class-token row a ViT
 * saliency map reads).  p_stride_q >= Nk; the innermost dimension of p is contiguous.  B, H >= 1.
 * One mode, fp32 on the vector pipe (compensated dot products: a score carries the error of its inputs' rounding only; the row
 * maximum subtracted before exp): d->flags must be 0, and KANVIT_FLAG_BF16_MFMA is refused by name (callers clear it: the same
 * arithmetic under autocast).  KANVIT_EINVAL with a
 * kanvit_last_error() text for a null d / e / q / k / p, D odd or too large, scale <= 0, rows out of range, p_stride_q < Nk, a
 * size < 1, causal with k_len > q_len.
 * No workspace, no atomics; the stores of p are contiguous along j.  Bitwise reproducible: row (b, h, i) has the same bits run to
 * run, for every `rows`, whatever other samples and heads the launch holds, and whether q / k arrive packed or as separate
 * contiguous tensors.  (ABI 7: no struct or version change) */
int kanvit_attn_probs(const kanvit_attn_desc* d, const kanvit_attn_ext* e, const float* q, const float* k, float* p,
                      int64_t p_stride_b, int64_t p_stride_h, int64_t p_stride_q, int32_t rows, void* stream);

/* ---- single-query attention: one query per (batch, head) against all keys and values ------------------------------------------
 * The classification head reads only the class token (model.py:166-169), so the last block of a ViT needs one attention row per
 * head.  With q0 = q[b,h,:]:
 *     s_j = scale * q0 . k[b,h,j,:]        p = softmax_j(s), the maximum subtracted        o[b,h,:] = sum_j p_j v[b,h,j,:]
 * and from d_o[b,h,:], with dP_j = d_o . v_j and delta = sum_j p_j dP_j (= d_o . o, which is how it is formed):
 *     ds_j = p_j (dP_j - delta)      dq0 = scale sum_j ds_j k_j      dk_j = scale ds_j q0      dv_j = p_j d_o
 * d and e as for kanvit_attn_probs: d->N = q_len must be 1, e->Nk = k_len >= 1 of any size, D even and <= KANVIT_ATTN_X_MAX_D,
 * any finite scale; no causal form, e->mask must be NULL, d->flags must be 0 (one mode, exact fp32 on the vector pipe; there is
 * no matrix product left).  q, dq: [B][H][D] through q_stride_b / q_stride_h; o, d_o through o_stride_b / o_stride_h (the _n
 * strides are ignored); k, v, dk, dv: [B][H][Nk][D] through the k / v strides -- the halves of a packed [B][Nk][2][H][D] tensor
 * are read and written in place; p: [B][H][Nk] contiguous, written by the forward (it is scratch for the scores while the kernel
 * runs) and read by the backward.  Innermost dimensions are contiguous; rows on the 16-byte grid with D % 4 == 0 take 16-byte
 * loads, narrower ones otherwise, same results.  dk / dv must not alias k / v.
 * Two streaming passes forward (K, then V), one backward (K and V read, dK and dV written): no workspace, no atomics, one fixed
 * summation order -- bitwise reproducible.  B = 0 returns without a launch.  KANVIT_EINVAL with a kanvit_last_error() text for a
 * null argument, q_len != 1, D odd or too large, a size < 1, causal, a mask, a flag.  (ABI 7: no struct or version change) */
int kanvit_attn_q1_fwd(const kanvit_attn_desc* d, const kanvit_attn_ext* e, const float* q, const float* k, const float* v,
                       float* o, float* p, void* stream);
int kanvit_attn_q1_bwd(const kanvit_attn_desc* d, const kanvit_attn_ext* e, const float* q, const float* k, const float* v,
                       const float* o, const float* p, const float* d_o, float* dq, float* dk, float* dv, void* stream);

/* ---- fused feed-forward for the small geometries ---------------------------------------------
 * y = relu(x W1^T + b1) W2^T + b2, the TransformerBlock's nn.Sequential(Linear, ReLU(inplace), Linear) (model.py:25-29,36),
 * x[M][D], W1[F][D], b1[F], W2[D][F], b2[D] in nn.Linear's own layouts; fp32 products and sums.  Forward: one launch;
 * backward (recomputes the hidden activations): dx[M][D], dW1[F][D], db1[F], dW2[D][F], db2[D], deterministic.
 * Instantiated for the reference's default width only (D = 64, F = 256) and M <= kanvit_ff_small_max_rows().            */
int kanvit_ff_small_supported(int D, int F);
int64_t kanvit_ff_small_max_rows(void);
int kanvit_ff_small_fwd(int64_t M, int D, int F, const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                        float* y, void* stream);
size_t kanvit_ff_small_bwd_workspace(int64_t M, int D, int F);
int kanvit_ff_small_bwd(int64_t M, int D, int F, const float* x, const float* w1, const float* b1, const float* w2, const float* dy,
                        float* dx, float* dw1, float* db1, float* dw2, float* db2, void* workspace, size_t workspace_bytes, void* stream);
/* The same with the block's second LayerNorm fused in front (model.py:36  x = x + FF(LN2(x)),  x = x_in + delta):
 *   fwd: s = x + delta (delta may be NULL), y = FF(LayerNorm(s; gamma, beta, eps)); writes s[M][D], mean[M], rstd[M], y[M][D]
 *   bwd: ds = ds_in (may be NULL) + LayerNorm-backward(FF-backward(dy))  -- the gradient of x and of delta alike --
 *        dgamma[D], dbeta[D], dW1, db1, dW2, db2.  Workspace: kanvit_ff_small_bwd_workspace.                         */
int kanvit_lnff_small_fwd(int64_t M, int D, int F, float eps, const float* x, const float* delta, const float* gamma, const float* beta,
                          const float* w1, const float* b1, const float* w2, const float* b2, float* s, float* mean, float* rstd, float* y,
                          void* stream);
int kanvit_lnff_small_bwd(int64_t M, int D, int F, const float* s, const float* mean, const float* rstd, const float* gamma, const float* beta,
                          const float* w1, const float* b1, const float* w2, const float* dy, const float* ds_in, float* ds, float* dgamma,
                          float* dbeta, float* dw1, float* db1, float* dw2, float* db2, void* workspace, size_t workspace_bytes, void* stream);

/* ---- residual add + LayerNorm (the TransformerBlock assembly around the KAN / attention kernels) -------------------
 * Replaces the `x + ...` adds and the nn.LayerNorm calls of model.py:31-37 (TransformerBlock.forward) and their autograd
 * backward, two to four separate passes over [M, D] each in the reference, by one pass forward and one backward.
 *   forward : s = x + delta (delta may be NULL);  y = (s - mean) * rstd * gamma + beta  (biased variance, eps inside the
 *             square root: torch.nn.LayerNorm).  Writes y[M, D], mean[M], rstd[M] and, if xsum != NULL, s to xsum[M, D].
 *   backward: dx = LayerNorm backward of dy w.r.t. s, plus dres[M, D] if not NULL (the gradient that arrives on the
 *             residual stream); dgamma[D], dbeta[D] are fully written.  `xsum` is the s of the forward.
 * Rows are contiguous (row stride D), D % 4 == 0, 4 <= D <= 1024, pointers 16-byte aligned.                        */
int kanvit_addln_fwd(int64_t M, int D, float eps, const float* x, const float* delta, const float* gamma, const float* beta,
                     float* xsum, float* y, float* mean, float* rstd, void* stream);
size_t kanvit_addln_bwd_workspace(int64_t M, int D);
int kanvit_addln_bwd(int64_t M, int D, const float* xsum, const float* gamma, const float* mean, const float* rstd,
                     const float* dy, const float* dres, float* dx, float* dgamma, float* dbeta, void* workspace,
                     size_t workspace_bytes, void* stream);
/* The same two passes with bf16 tensors at the boundary (torch.autocast: the feed-forward's output `delta`, its input `y` and the
 * gradient `dy` arriving from it are bf16; the residual stream x / xsum / dres / dx stays fp32): *_bf16 != 0 says that the pointer
 * in front of it is bf16 [M][D]; dx_bf16, if not NULL, receives a second copy of dx rounded to bf16 (the gradient of a bf16
 * delta).  With all flags 0 and dx_bf16 NULL these ARE kanvit_addln_fwd / _bwd.  (ABI >= 6) */
int kanvit_addln_fwd_ex(int64_t M, int D, float eps, const float* x, const void* delta, int delta_bf16, const float* gamma, const float* beta,
                        float* xsum, void* y, int y_bf16, float* mean, float* rstd, void* stream);
int kanvit_addln_bwd_ex(int64_t M, int D, const float* xsum, const float* gamma, const float* mean, const float* rstd,
                        const void* dy, int dy_bf16, const float* dres, float* dx, void* dx_bf16, float* dgamma, float* dbeta, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---- stochastic depth (DropPath): a per-sample scale of the branch inside the residual add + LayerNorm pass -----------------
 * The reference model has no regulariser (model.py:31-37 adds every branch as it is); the DeiT recipe drops each residual branch per
 * sample with a rate that grows with the depth.  Stock PyTorch spends a bernoulli_, a divide, a broadcast multiply over [B, N, D] and
 * that multiply's backward per branch; here the scale rides in the pass that adds the branch anyway.
 *
 * kanvit_depth_scales: the keep decisions of all n_branch <= KANVIT_DEPTH_MAX_BRANCHES branches of one forward, ONE launch of ONE
 * work-group.  keep[n_branch] is a HOST array of fp32 keep probabilities in (0, 1]; they, their reciprocals inv_j = float32(1) /
 * float32(keep_j) (divided on the host) and the thresholds T_j = round(keep_j * 2^24) (to nearest, ties to even) travel by value in the
 * kernel argument, so a captured graph bakes them in and nothing is uploaded.  With mix() the splitmix64 step stated at
 * kanvit_augment_u8 and c the value of *counter when the kernel starts,
 *   h = mix(mix(mix(seed) + c) + ((uint64)j << 32) + b),      scales[j][b] = (h >> 40) < T_j ? inv_j : 0.0f,
 * scales being [n_branch][B] fp32 on the device.  keep = 1 gives T = 2^24: always kept, scale exactly 1.0.  Every thread reads
 * *counter, the work-group synchronises, then one thread stores c + 1: consecutive launches (and replays of a captured launch) walk
 * c, c + 1, ... with no RNG state and nothing from the host.  counter is a device uint64, 8-byte aligned.  KANVIT_EINVAL (named in
 * kanvit_last_error, before the device is touched) for n_branch outside 1..64, B < 0, a keep outside (0, 1] or a null pointer.
 *
 * kanvit_addln_sd_fwd / _bwd: kanvit_addln_fwd_ex / _bwd_ex with  s = x + row_scale[r / rows_per_sample] * delta  for row r -- the
 * product and the sum are two fp32 roundings, never contracted (bit for bit torch's x + scale * delta in fp32; a bf16 delta is widened
 * first); y, mean, rstd as before.  Backward: dx as before; the gradient of delta is its own tensor now, ddelta = row_scale[.] * dx,
 * written by the same pass -- fp32 [M][D], or bf16 rounded to nearest even when ddelta_bf16 != 0; it may not be dx.  dgamma / dbeta and
 * the workspace are those of kanvit_addln_bwd (kanvit_addln_bwd_workspace).  delta and row_scale (fp32 [M / rows_per_sample], on the
 * device) are required; KANVIT_EINVAL unless rows_per_sample >= 1 divides M, besides the width and alignment conditions above.
 * Additive: the ABI version stays 7. */
#define KANVIT_DEPTH_MAX_BRANCHES 64
int kanvit_depth_scales(int64_t B, int n_branch, const float* keep, uint64_t seed, uint64_t* counter, float* scales, void* stream);
int kanvit_addln_sd_fwd(int64_t M, int D, float eps, const float* x, const void* delta, int delta_bf16, const float* gamma, const float* beta,
                        float* xsum, void* y, int y_bf16, float* mean, float* rstd, const float* row_scale, int64_t rows_per_sample,
                        void* stream);
int kanvit_addln_sd_bwd(int64_t M, int D, const float* xsum, const float* gamma, const float* mean, const float* rstd,
                        const void* dy, int dy_bf16, const float* dres, float* dx, void* ddelta, int ddelta_bf16, float* dgamma, float* dbeta,
                        const float* row_scale, int64_t rows_per_sample, void* workspace, size_t workspace_bytes, void* stream);

/* ---- PatchDropout: train on a hashed subset of every sample's patch tokens (csrc/patch_drop.hip) ------------------------------
 * Liu et al. 2023, timm's patch_drop_rate, the masking of FLIP / MAE: in training every sample keeps K of its P patch tokens and the
 * class token; everything behind the embedding runs on N = K + 1 tokens.  The reference model has no such option (model.py:144-152
 * builds all P + 1 rows).  Stock PyTorch spends rand + argsort + gather on a full [B, P, I] patch matrix and needs a generator a
 * captured graph does not step; here the keep set is a hash, the gather reads only the kept patches out of the NCHW batch, and the
 * sequence is assembled with the position embedding of the ORIGINAL patch positions.
 *
 * kanvit_patch_keep: idx[B][K] (int32, device), the kept patch numbers of every sample in ascending order.  With mix() the splitmix64
 * step stated at kanvit_augment_u8 and c the value of *counter when the launch starts,
 *   base = mix(mix(seed ^ KANVIT_PATCH_KEEP_TAG) + c),          key(b, p) = mix(base + ((uint64)b << 32) + p),
 * patch p of sample b is kept iff fewer than K pairs (key(b, p'), p') are lexicographically below (key(b, p), p): the K smallest
 * keys, ties (which a 64-bit hash all but never has) going to the smaller p.  The tag keeps this stream apart from
 * kanvit_depth_scales' under the same seed; a sample's row does not depend on B.  counter is a device uint64, 8-byte aligned, with a
 * value below 2^48: every work-group reads it and the launch adds exactly 1 to it, with nothing from the host (one atomic per
 * work-group is its read and its ticket in the top 16 bits; the last ticket puts c + 1 back -- DESIGN.md section 4.26), so consecutive
 * launches and replays of a captured one draw new sets.  1 <= K <= P <= KANVIT_PATCH_KEEP_MAX_P (a sample's keys live in LDS), 0 <= B
 * < 2^31; B = 0 returns KANVIT_OK without touching the counter.  KANVIT_EINVAL (named in kanvit_last_error, before the device is
 * touched) outside that domain and for a null or misaligned pointer.
 *
 * kanvit_patch_gather: p as for kanvit_patch_embed_fwd (prepend_rows is ignored); ph = H / n_patches, pw = W / n_patches, I = C ph pw.
 *   rows[(b*K + j)*ldr + i] = images[b][c][py*ph + iy][px*pw + ix],   idx[b][j] = py*n_patches + px,   i = (c*ph + iy)*pw + ix
 * -- patchify restricted to the kept patches, a pure copy of B*K*I floats.  idx is any int32 [B][K] on the device with entries in
 * [0, P): unsorted and repeated entries are fine, an entry outside is the caller's error (not checked on the device).  Any pw, any
 * 4-byte aligned images / rows, ldr >= I; float4 moves where pw % 4 == 0, ldr % 4 == 0 and both addresses are 16-byte aligned.
 * B*K < 2^31.  No gradient: the images are data.
 *
 * kanvit_tokens_assemble_fwd: out[B][K + 1][O] (contiguous) from the embedded rows tokens[B*K][ldt], cls[O] and pos[P + 1][O]:
 *   out[b][0][:] = cls + pos[0],     out[b][1 + j][:] = tokens[(b*K + j)*ldt + :] + pos[1 + idx[b][j]]
 * one fp32 add per element (bit for bit torch's cat + indexed add).  cls / pos may not be NULL.
 * kanvit_tokens_assemble_bwd: dtokens[b*K + j][:] = dout[b][1 + j][:] (contiguous [B*K][O], a copy) and dcls[o] = sum_b dout[b][0][o];
 * either may be NULL (not wanted), not both.  The sum has a fixed order and no atomics: slice s of eight adds samples s, s + 8, ...
 * in that order, then the eight slices are added in order -- bitwise the same from run to run.
 * All four return KANVIT_EINVAL before the device is touched for sizes below 1, ld below the row length, row counts of 2^31 and
 * more, null and misaligned (4-byte) pointers.  Additive: the ABI version stays 7. */
#define KANVIT_PATCH_KEEP_MAX_P 1024
#define KANVIT_PATCH_KEEP_TAG 0x5061746368447270ull /* "PatchDrp" */
int kanvit_patch_keep(int64_t B, int P, int K, uint64_t seed, uint64_t* counter, int32_t* idx, void* stream);
int kanvit_patch_gather(const kanvit_patch_desc* p, int64_t B, int K, const int32_t* idx, const float* images, float* rows, int64_t ldr,
                        void* stream);
int kanvit_tokens_assemble_fwd(int64_t B, int K, int O, const float* tokens, int64_t ldt, const float* cls, const float* pos,
                               const int32_t* idx, float* out, void* stream);
int kanvit_tokens_assemble_bwd(int64_t B, int K, int O, const float* dout, float* dtokens, float* dcls, void* stream);

/* ---- ReLU backward + bias gradient of the feed-forward's first Linear in one pass ----------------
 * The TransformerBlock's nn.Sequential(Linear, ReLU(inplace), Linear) (model.py:25-29): what autograd runs for the ReLU and
 * for the first Linear's bias -- threshold_backward on the saved activation y, then a column sum of the result --
 *     dh[m][n] = y[m][n] > 0 ? dy[m][n] : 0,      dbias[n] = sum_m dh[m][n]
 * as one pass over [M, N] + an ordered reduce of per-row-band partial sums (deterministic).  dh may alias dy.
 * Row-major contiguous [M][N] fp32, N % 4 == 0, 16-byte aligned pointers; workspace: kanvit_relu_bwd_bias_workspace(M, N). */
size_t kanvit_relu_bwd_bias_workspace(int64_t M, int N);
int kanvit_relu_bwd_bias(int64_t M, int N, const float* dy, const float* y, float* dh, float* dbias, void* workspace,
                         size_t workspace_bytes, void* stream);
/* The same on bf16 tensors (torch.autocast): dy, y, dh are bf16 [M][N] (16-byte aligned, N % 4 == 0); dbias and the workspace stay
 * fp32 (sizes as above).  (ABI >= 6) */
int kanvit_relu_bwd_bias_bf16(int64_t M, int N, const void* dy_bf16, const void* y_bf16, void* dh_bf16, float* dbias, void* workspace,
                              size_t workspace_bytes, void* stream);

/* ---- three-term bf16 split image (opt-in "bf16x3" feed-forward mode, kanvit/dense.py) --------------------------------
 * v = hi + lo, hi = bf16(v), lo = bf16(v - hi).  Writes out[M][3K] (bf16) = [hi|hi|lo] (pattern 0) or [hi|lo|hi]
 * (pattern 1) of  v = x (+ bias[K]) (ReLU if relu) (zeroed where mask_hi[m][k] <= 0, a bf16 image with row stride
 * mask_ld elements): an fp32-accurate (~5e-6) product through ONE bf16 GEMM over a 3K-long axis, pattern-0 image times
 * pattern-1 image.  Replaces nothing in the reference (model.py:25-29 runs fp32 nn.Linear); K % 8 == 0.           */
int kanvit_split3_bf16(int64_t M, int K, const float* x, const float* bias, int relu, const void* mask_hi, int64_t mask_ld,
                       void* out, int pattern, void* stream);

/* ---- batches from a GPU-resident uint8 dataset (kanvit/data.py; csrc/batch_u8.hip) --------------------------------------
 * The reference's input pipeline (train.py:100-118: RandomHorizontalFlip, RandomCrop(size, padding) on the zero-padded uint8 image,
 * ToTensor, Normalize) as one gather over a dataset that stays in HBM:
 *   out[b][c][y][x] = lut[c][ images[idx[b]][sy][sx][c] ],  sy = y + dy - pad_y,  sx = x + dx - pad_x,  sx <- W - 1 - sx if flipped;
 *                     lut[c][0] where (sy, sx) is outside the image (the zero padding, normalised).
 * images [N][H][W][C] uint8 (NHWC, as the CIFAR / MNIST arrays come); labels [N] int64 or NULL; idx [B] int64 sample indices (any
 * order, repeats allowed; each in [0, N): the CALLER checks that, an entry outside is not dereferenced and gives padding and label
 * -1); lut [C][256] fp32, the normalised value of every byte, built by the host with the reference's fp32 operations (the kernel
 * does no floating-point arithmetic: the output equals the CPU transform bit for bit); out [B][C][H][W] fp32 contiguous; y_out [B]
 * = labels[idx[b]] or NULL; params_out [B][3] = the (dy, dx, flip) used, or NULL.
 * (dy, dx, flip) depend on (seed, epoch, idx[b]) only -- not on B, the position in the batch or the rank.  With mix() the
 * splitmix64 step (z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB;
 * z ^ z >> 31), all mod 2^64:
 *   h = mix(mix(mix(seed) + epoch) + idx),  dy = (h & 0xFFFFF) % (2 pad_y + 1),  dx = ((h >> 20) & 0xFFFFF) % (2 pad_x + 1),
 *   flip = flip_enabled ? (h >> 40) & 1 : 0.          pad = 0, flip = 0 is the evaluation transform (normalise only).
 * Stores are 16 bytes per lane where W % 4 == 0 and out is 16-byte aligned, 4 bytes otherwise (decided on the host).  One launch,
 * no atomics, no workspace, no synchronisation: capturable.  KANVIT_EINVAL (named in kanvit_last_error) unless N >= 1, 1 <= C <= 4,
 * 1 <= H, W <= 2^20, 0 <= pad_y <= H, 0 <= pad_x <= W, B >= 0, flip in {0, 1}; B = 0 launches nothing.
 * kanvit_augment_u8_supported is the same shape check as a pure host function (1 / 0).  Additive: the ABI version stays 7. */
int kanvit_augment_u8_supported(int64_t N, int H, int W, int C, int pad_y, int pad_x);
int kanvit_augment_u8(const uint8_t* images, const int64_t* labels, const int64_t* idx, const float* lut, float* out, int64_t* y_out,
                      int32_t* params_out, int64_t N, int64_t B, int H, int W, int C, int pad_y, int pad_x, int flip, uint64_t seed,
                      uint64_t epoch, void* stream);

/* ---- Mixup / CutMix on the same pass (kanvit/data.py: mix_table; csrc/batch_u8.hip) --------------------------------------
 * kanvit_augment_u8 with a second source.  Three tables indexed by the DATASET index s (not by the position in the batch):
 * partner [N] int64 (the sample mixed into s, or -1), weight [N] fp32 (the weight w of s's own label; 1 where partner is -1) and box
 * [N][4] int32 = (y0, y1, x0, x1), half open, in OUTPUT coordinates.  With s = idx[b], j = partner[s],
 *   a(b,c,y,x) = kanvit_augment_u8's value for s,   p(b,c,y,x) = kanvit_augment_u8's value for j -- with j's OWN (dy, dx, flip),
 *   out = a                                           j outside [0, N)  (-1: not mixed; anything else is never dereferenced)
 *   out = (y0 <= y < y1 && x0 <= x < x1) ? p : a      y0 < y1 and x0 < x1  (CutMix: look-ups only, bit-exact)
 *   out = fadd(fmul(w, a), fmul(1 - w, p))            otherwise  (Mixup: three fp32 roundings to nearest, 1 - w one more; never an
 *                                                     fma, so the same four operations on the host give the same bits)
 *   y_out[b] = labels[s],  y2_out[b] = labels[j] (labels[s] where not mixed),  w_out[b] = weight[s]   (each may be NULL).
 * A sample's pixels depend on (seed, epoch, s) and its table row only.  Stores, the staged table, the launch (one, no atomics, no
 * workspace, capturable) and the checks are kanvit_augment_u8's; the three tables are required; B = 0 launches nothing.  The
 * CALLER checks partner against [-1, N) when it uploads the table.  Additive: the ABI version stays 7. */
int kanvit_mix_u8(const uint8_t* images, const int64_t* labels, const int64_t* idx, const float* lut, const int64_t* partner,
                  const float* weight, const int32_t* box, float* out, int64_t* y_out, int64_t* y2_out, float* w_out, int64_t N, int64_t B,
                  int H, int W, int C, int pad_y, int pad_x, int flip, uint64_t seed, uint64_t epoch, void* stream);

/* ---- bilinear resize / RandomResizedCrop on the same pass (kanvit/data.py: crop_table; csrc/batch_u8.hip) -----------------
 * kanvit_augment_u8 / kanvit_mix_u8 at an output size of their own: out [B][C][OH][OW] fp32 contiguous; images, labels, idx and
 * lut as kanvit_augment_u8's.  crop [N][5] int32, indexed by the DATASET index s = idx[b] (as the mix tables are), or NULL.  A row
 * (y0, x0, bh, bw, flip) is a box of bh x bw source pixels with its top-left corner at (y0, x0), in the coordinates of the possibly
 * flipped image extended by zero padding on all sides; it may lie partly or wholly outside the image; NULL means (0, 0, H, W, 0)
 * for every sample (the evaluation transform).  The tap at box-local (r, u) reads row sy = y0 + r, column sx = x0 + u:
 *   t(r, u) = lut[c][0]                                      where (sy, sx) is outside [0, H) x [0, W)
 *           = lut[c][ images[s][sy][flip ? W-1-sx : sx][c] ]  otherwise
 * -- kanvit_augment_u8's rule: the row (dy - pad_y, dx - pad_x, H, W, flip) describes its crop.  The output is the bilinear resize
 * of the box with half-pixel centres and the taps clamped to the box (F.interpolate(crop, size, mode="bilinear",
 * align_corners=False, antialias=False): no antialiasing, so meant for upsampling and mild downsampling).  The fp32 operation
 * sequence is fixed, every operation rounded to nearest, none contracted into an fma, the division correctly rounded:
 *   scale_y = float(bh) / float(OH);   src = max(scale_y * (float(oy) + 0.5f) - 0.5f, 0.f)
 *   r0 = min(int(src), bh - 1);  r1 = min(r0 + 1, bh - 1);  wy1 = src - float(r0);  wy0 = 1.f - wy1
 *   (the same along x with bw, OW, ox  ->  u0, u1, wx0, wx1)
 *   top = wx0 * t(r0,u0) + wx1 * t(r0,u1);   bot = wx0 * t(r1,u0) + wx1 * t(r1,u1);   a = wy0 * top + wy1 * bot
 * so the same operations in float32 on the host give the same bits, and at bh == OH, bw == OW they give t(r0, u0) exactly: the
 * call reproduces kanvit_augment_u8 bit for bit at the identity size.  A row with bh < 1 or bw < 1 reads nothing and gives
 * lut[c][0] (no arithmetic).
 * partner / weight / box: kanvit_mix_u8's tables with its three rules (unmixed / CutMix look-up / Mixup fadd(fmul(w, a),
 * fmul(1 - w, p))), all three or all NULL (no mixing; y2_out and w_out must then be NULL).  box is in OUTPUT coordinates
 * (OH x OW); p is the resampled value of sample j = partner[s] under j's OWN crop row.  y_out, y2_out, w_out as there.  A
 * sample's pixels depend on its own and its partner's table rows only -- never on B, the position in the batch or the rank.
 * An idx or partner outside [0, N) is never dereferenced; no tap outside the image is loaded; the CALLER validates the tables on
 * the CPU before the upload.  Stores are 16 bytes per lane where OW % 4 == 0 and out is 16-byte aligned, 4 bytes otherwise
 * (decided on the host).  One launch, no atomics, no workspace, no synchronisation: capturable.  KANVIT_EINVAL (named in
 * kanvit_last_error, before any device call) unless N >= 1, 1 <= C <= 4, 1 <= H, W, OH, OW <= 2^20, B >= 0 (B = 0 returns 0 and
 * launches nothing); for a null images / idx / lut / out, mix tables not given together, y_out / y2_out without labels, a
 * misaligned pointer.  kanvit_resample_u8_supported is the shape check as a pure host function (1 / 0).  Additive: the ABI
 * version stays 7. */
int kanvit_resample_u8_supported(int64_t N, int H, int W, int C, int OH, int OW);
int kanvit_resample_u8(const uint8_t* images, const int64_t* labels, const int64_t* idx, const float* lut, const int32_t* crop,
                       const int64_t* partner, const float* weight, const int32_t* box, float* out, int64_t* y_out, int64_t* y2_out,
                       float* w_out, int64_t N, int64_t B, int H, int W, int C, int OH, int OW, void* stream);

/* ---- Random Erasing on the same pass (kanvit/data.py: erase_table, normal_table; csrc/batch_u8.hip) ----------------------
 * kanvit_resample_u8 with a per-sample erase box applied BEFORE mixing (torchvision's RandomErasing / timm's, per sample, at the
 * output resolution, after normalisation).  Every argument up to OW is kanvit_resample_u8's, with its meaning and its checks.
 * erase [N][4] int32 = (y0, y1, x0, x1), half open, in OUTPUT coordinates, indexed by the DATASET index like the other tables.  With
 * s = idx[b] and a(b,c,y,x) kanvit_resample_u8's value of s before mixing,
 *   a'(b,c,y,x) = fill(s,c,y,x)   where erase[s] has y0 <= y < y1 and x0 <= x < x1
 *               = a(b,c,y,x)      otherwise
 * and p' is the same for the partner j = partner[s]: j's resampled value under j's OWN erase row and j's own fill.  The three mixing
 * rules (unmixed / CutMix look-up / Mixup fadd(fmul(w, a'), fmul(1 - w, p'))) then run on a' and p'; labels and weights are not
 * touched.  The test is a comparison on output coordinates and forms no sum of table entries: any int32 row is safe, one with
 * y0 >= y1 or x0 >= x1 erases nothing, and one that reaches outside [0, OH) x [0, OW) is clipped by the comparison.  The erase row
 * of an idx or partner outside [0, N) is never read (such a sample stays padding with label -1, such a partner leaves the row
 * unmixed, but erased).
 * The fill does no floating-point arithmetic:
 *   noise == NULL (noise_len == 0):  fill = 0.0f  -- the dataset mean, normalised (torchvision's value=0, timm's "const");
 *   otherwise (timm's "pixel"):      fill = noise[ h >> (64 - log2 noise_len) ],
 *                                    h = mix( mix(noise_key + s) + ((c * OH + y) * OW + x) ),  all mod 2^64, mix() as above;
 * noise [noise_len] fp32, noise_len a power of two in 2..65536 (data.normal_table: standard-normal quantiles), noise_key any value
 * (data.erase_noise_key derives it from (seed, epoch)).  The fill depends on (noise_key, s, c, y, x) only -- not on B, the
 * position in the batch, the rank, or whether s appears as a sample or as a partner -- and the same uint64 operations on the host
 * give the same bits.  A row of a work item that lies wholly inside the box loads no source pixel.
 * erase == NULL: the call is kanvit_resample_u8 (the same kernels, the same arguments); noise must then be NULL.  Stores, the
 * launch (one, no atomics, no workspace, no synchronisation: capturable) and B = 0 as there.  KANVIT_EINVAL (named in
 * kanvit_last_error, before any device call) for kanvit_resample_u8's cases and for noise_len not 0 or a power of two in 2..65536,
 * noise without erase, noise without noise_len or noise_len without noise, a misaligned erase / noise.
 * kanvit_erase_u8_supported is the shape check as a pure host function (1 / 0).  Additive: the ABI version stays 7. */
int kanvit_erase_u8_supported(int64_t N, int H, int W, int C, int OH, int OW, int noise_len);
int kanvit_erase_u8(const uint8_t* images, const int64_t* labels, const int64_t* idx, const float* lut, const int32_t* crop,
                    const int64_t* partner, const float* weight, const int32_t* box, float* out, int64_t* y_out, int64_t* y2_out, float* w_out,
                    int64_t N, int64_t B, int H, int W, int C, int OH, int OW, const int32_t* erase, const float* noise, int noise_len,
                    uint64_t noise_key, void* stream);

/* ---- RandAugment: one uint8 -> uint8 pass over the dataset per epoch (kanvit/data.py: randaug_table; csrc/randaug.hip) --------
 * dst[s] = src[s] passed through its K table rows in order, s = 0 .. N-1.  src and dst are [N][H][W][C] uint8 and do not overlap
 * (several ops read more than the byte they write); table is [N][K][8] int32, row = (op, p0 .. p6), indexed by the DATASET index
 * like the batch kernels' tables -- the batch kernels then read dst in place of the stored images, so crop, flip, resize, erase and
 * mix work unchanged and a partner comes augmented under its own rows.  The ops run at the STORED resolution, before the crop
 * (timm runs them after RandomResizedCrop).
 * All arithmetic is integer; `>>` is an arithmetic shift, `/` divides non-negative integers, clamp is to [0, 255], Q16 means the
 * host rounded value * 65536 to int32, and
 *   blend(d, v, f) = clamp((d * 65536 + f * (v - d) + 32768) >> 16),   f in Q16, 0 <= f <= 2 * 65536,
 *   L(pixel)       = (19595 R + 38470 G + 7471 B + 32768) >> 16        (PIL's conversion to "L"; channels 0, 1, 2).
 * Per byte v of channel c of an H x W image:
 *   IDENTITY      v
 *   AUTOCONTRAST  lo, hi = min, max of channel c over the image; hi <= lo: v; else ((v - lo) * 255) / (hi - lo)
 *   EQUALIZE      PIL's ImageOps.equalize per channel: h the histogram, step = (H W - h[last non-empty bin]) / 255; step == 0 or
 *                 one non-empty bin: v; else min(255, (step / 2 + sum_{j < v} h[j]) / step)
 *   INVERT        255 - v
 *   POSTERIZE     p0 = bits kept, 0..8:                 v & ~(0xFF >> p0)
 *   SOLARIZE      p0 = threshold, 0..256:               v < p0 ? v : 255 - v
 *   SOLARIZE_ADD  p0 = add, 0..255, p1 = threshold, 0..256:   v < p1 ? min(v + p0, 255) : v
 *   BRIGHTNESS    blend(0, v, p0)
 *   COLOR         C >= 3: blend(L(pixel), v, p0) for c < 3, v for c = 3; C < 3: v
 *   CONTRAST      blend(m, v, p0) for every channel, m = (sum of g over the pixels + H W / 2) / (H W), g = L(pixel) for C >= 3 and
 *                 channel 0 for C < 3
 *   SHARPNESS     blend(sm, v, p0), sm = (the 8 neighbours of the same channel + 5 v + 6) / 13 (PIL's SMOOTH); sm = v on the
 *                 one-pixel border, so an image with H < 3 or W < 3 is unchanged
 *   AFFINE        the byte of channel c at source pixel (xs, ys), nearest neighbour under an inverse map with half-pixel centres:
 *                   xs = (p0 (2x + 1) + p1 (2y + 1) + 2 p2) >> 17,   ys = (p3 (2x + 1) + p4 (2y + 1) + 2 p5) >> 17   (64-bit)
 *                 p0, p1, p3, p4 Q16 matrix entries, p2, p5 Q16 offsets in pixels, any int32; a source outside the image gives the
 *                 fill byte (p6 >> 8 c) & 255.  Shear, translation and rotation are all AFFINE; the host builds the matrix.
 * An unknown op code, or a parameter outside the range stated above, makes the row IDENTITY; parameters an op does not name are
 * ignored.  Whatever a row holds, nothing outside image s of src and dst is read or written.
 * One launch: one work-group per image, striding beyond 2048 work-groups, the image in LDS (two buffers, a C x 256 int32
 * histogram / look-up area); integer sums and LDS integer atomics only, so the output does not depend on the launch shape and the
 * same integer operations on the host give the same bytes.  No workspace, no synchronisation; capturable.  N = 0 returns 0 and
 * touches nothing.  KANVIT_EINVAL (named in kanvit_last_error, before any device call) for N < 0, C outside 1..4, H or W < 1,
 * H W C > KANVIT_RA_MAX_BYTES, K outside 1..KANVIT_RA_MAX_OPS, a null pointer, src == dst or overlapping arrays, a misaligned
 * table.  `stream` is a hipStream_t.  Additive: the ABI version stays 7. */
#define KANVIT_RA_IDENTITY 0
#define KANVIT_RA_AUTOCONTRAST 1
#define KANVIT_RA_EQUALIZE 2
#define KANVIT_RA_INVERT 3
#define KANVIT_RA_POSTERIZE 4
#define KANVIT_RA_SOLARIZE 5
#define KANVIT_RA_SOLARIZE_ADD 6
#define KANVIT_RA_BRIGHTNESS 7
#define KANVIT_RA_COLOR 8
#define KANVIT_RA_CONTRAST 9
#define KANVIT_RA_SHARPNESS 10
#define KANVIT_RA_AFFINE 11
#define KANVIT_RA_MAX_OPS 4          /* rows per sample */
#define KANVIT_RA_MAX_BYTES 24576    /* H W C: two image buffers and the histograms stay under 64 KB of LDS */
int kanvit_randaug_u8(const uint8_t* src, uint8_t* dst, const int32_t* table, long long N, int H, int W, int C, int K, void* stream);

/* ---- soft-target cross-entropy, loss and gradient in one pass (ops.soft_cross_entropy; csrc/soft_ce.hip) -----------------
 * The training loss for Mixup / CutMix pairs and label smoothing.  logits [B][C] fp32, unit column stride, row stride ld >= C;
 * y1 [B] int64; y2 [B] int64 and w [B] fp32 together or both NULL (NULL: w = 1); eps in [0, 1).
 *   t_c    = (1 - eps) (w [c == y1] + (1 - w) [c == y2]) + eps / C
 *   loss_b = lse(z_b) - sum_c t_c z_bc,  computed as log(sum_c exp(z_c - m)) + sum_c t_c (m - z_c) with m = max_c z_c
 *   dz_bc  = (softmax(z_b)_c - t_c) / B,      loss = (1/B) sum_b loss_b
 * loss_rows [B], dlogits [B][C] contiguous, loss [1], all fp32.  One wave per row, fixed lane assignment and shuffle tree: a row's
 * loss_rows entry does not depend on B or on its position, and its gradient only through the factor 1/B (rounded once on the
 * host, one multiply per element).  The mean is an ordered sum in a second, one-work-group launch: no floating-point atomics, the
 * same bits on every run.  A row whose y1 or y2 is outside [0, C) gets loss 0 and a zero gradient row and is never used as an index;
 * the divisor stays B.  No host synchronisation; capturable.  KANVIT_EINVAL (named in kanvit_last_error, before any launch) for
 * C < 2, B < 1, ld < C, eps outside [0, 1), a null logits / y1 / output pointer, exactly one of y2 and w, a misaligned pointer.
 * Additive: the ABI version stays 7. */
int kanvit_soft_ce(const float* logits, int64_t ld, const int64_t* y1, const int64_t* y2, const float* w, int64_t B, int C, float eps,
                   float* loss_rows, float* dlogits, float* loss, void* stream);

/* ---- masked-autoencoder pretraining: token restore and the masked-patch loss (mae.py; csrc/mae.hip) ------------------------
 * He et al. 2022 on top of kanvit_patch_keep: the encoder runs on the K kept patches and the class token; a light decoder then
 * reconstructs the P - K dropped patches from the full sequence.  The reference has no such mode.  idx is int32 [B][K] exactly as
 * kanvit_patch_keep writes it -- every row strictly ascending with entries in [0, P): a precondition, not checked on the device.
 *
 * kanvit_tokens_restore_fwd: out[B][P + 1][O] (contiguous) from y[B][K + 1][O] (contiguous: the encoder output after the decoder's
 * input projection), mask_token[O] and pos[P + 1][O]:
 *   out[b][0][:] = y[b][0] + pos[0],    out[b][1 + p][:] = (y[b][1 + j] if p == idx[b][j] else mask_token) + pos[1 + p]
 * one fp32 add per element (bit for bit torch's repeat + cat + gather + add); the rank of p is a binary search of the sample's row.
 * kanvit_tokens_restore_bwd: dy[b][0] = dout[b][0], dy[b][1 + j] = dout[b][1 + idx[b][j]] (contiguous [B][K + 1][O], copies) and
 * dmask[o] = the sum of dout[b][1 + p][o] over every dropped (b, p); either may be NULL (not wanted), not both.  No atomics; the
 * addition tree depends on (B, P, K) alone: with the n = B (P - K) dropped rows numbered in (sample, ascending patch) order and L =
 * ceil(n / 128), slice s of 128 adds rows s L .. min(n, (s + 1) L) - 1 in that order, then slice s += slice s + h for h = 64, 32, ..,
 * 1 -- bitwise the same from run to run.  Both: 1 <= K < P <= KANVIT_PATCH_KEEP_MAX_P, O >= 1, 0 <= B, B (P + 1) < 2^31; any 4-byte
 * aligned pointers, float4 moves where O % 4 == 0 and every address is 16-byte aligned.
 *
 * kanvit_mae_loss: p as for kanvit_patch_gather (I = C ph pw, a patch flattened in patchify's (C, ph, pw) order); images fp32 NCHW
 * contiguous; pred and dpred [B][P + 1][I] fp32 contiguous -- the decoder head's output with its class row in place, which the kernel
 * skips.  For every dropped (b, p) with target t = the patch of the image:
 *   norm_pix != 0: mu = sum(t) / I, var = sum((t - mu)^2) / (I - 1) (unbiased, as Tensor.var), that = (t - mu) / sqrt(var + 1e-6);
 *   norm_pix == 0: that = t;
 *   rows[b][p] = sum_i (pred - that)^2 / I,      dpred[b][1 + p][i] = 2 (pred - that) / (I B (P - K)),
 * kept entries of rows, and the kept rows and the class row of dpred, are written as +0; loss[0] = (the ordered sum of the B P entries
 * of rows, kanvit_soft_ce's tree: thread t of 256 adds entries t, t + 256, ... in order, then a fixed tree) / float(B (P - K)).  One
 * wave per row holds the patch in registers: read once for mean, variance and error; a row's bits depend on the row alone; the factor
 * 2 / (I B (P - K)) is rounded once on the host.  Two launches, no host synchronisation, capturable.  1 <= K < P, 1 <= I <=
 * KANVIT_MAE_MAX_I (I = 1 only without norm_pix: one value has no variance), B >= 1, B (P + 1) < 2^31; any 4-byte aligned pointers,
 * float4 moves where pw % 4 == 0 and images, pred and dpred are 16-byte aligned.  No gradient reaches the images: they are data.
 * All three return KANVIT_EINVAL (named in kanvit_last_error, before the device is touched) outside their domain and for a null or
 * misaligned pointer.  Additive: the ABI version stays 7. */
#define KANVIT_MAE_MAX_I 4096
int kanvit_tokens_restore_fwd(int64_t B, int P, int K, int O, const float* y, const float* mask_token, const float* pos, const int32_t* idx,
                              float* out, void* stream);
int kanvit_tokens_restore_bwd(int64_t B, int P, int K, int O, const float* dout, const int32_t* idx, float* dy, float* dmask, void* stream);
int kanvit_mae_loss(const kanvit_patch_desc* p, int64_t B, int K, const int32_t* idx, const float* images, const float* pred, int norm_pix,
                    float* rows, float* loss, float* dpred, void* stream);

/* ---- epoch metrics on the device (kanvit/metrics.py; csrc/metrics.hip) ---------------------------------------------------
 * The reference appends labels, argmax and softmax of every step to host lists and runs scikit-learn on them per epoch
 * (train.py:42-44, utils.py:13-47).  Accuracy, balanced accuracy and weighted F1 are functions of the C x C confusion matrix; the
 * one-vs-rest ROC-AUC of class c is the Mann-Whitney statistic (2 gt_c + eq_c) / (2 P_c (N - P_c)) with
 *   gt_c = #{(i, j): label_i = c, label_j != c, p[i][c] > p[j][c]},  eq_c = the same pairs with p[i][c] == p[j][c]
 * (float32 compares of the stored values), P_c the samples of class c.  All of it is integer counting: exact, and the same whatever
 * the order of the atomic adds.
 *
 * kanvit_metrics_update: one launch per step.  logits [B][C], float32 (logits_bf16 = 0) or bfloat16 (1, widened exactly), unit
 * column stride, row stride ld elements; labels [B] int64.  Row b goes to slot n = n0 + b of the state buffers:
 *   probs_t[c][n]  (float32, CLASS-major [C][cap]) = exp(z_c - max z) / sum_c exp(z_c - max z), in fp32;
 *   preds_out[n]   (int32) = argmax_c z_c, the smallest index among equal maxima;
 *   labels_out[n]  (int32) = labels[b], or -1 where labels[b] is outside [0, C);
 *   confusion[labels[b]][preds_out[n]] += 1  (int64 [C][C], atomic; the caller zeroes it at the start of an epoch).
 * A row whose label is outside [0, C) is dropped: no confusion update, and the pair counts skip a slot with label -1 both as a
 * positive and as a negative.  A row's arithmetic does not depend on B or on its position: an epoch fed in other batch sizes gives
 * the same bits.  KANVIT_EINVAL (named in kanvit_last_error, checked before any launch) for a null pointer, logits_bf16 outside
 * {0, 1}, C < 2, B < 1, ld < C, n0 < 0 or n0 + B > cap, a pointer not aligned to its element.
 *
 * kanvit_metrics_auc_pairs: counts[c][0] = gt_c, counts[c][1] = eq_c (int64 [C][2], zeroed inside the call) over slots 0..n-1 of
 * probs_t ([C][cap]) and labels (int32 [n], as labels_out above).  A class without positives or without negatives counts 0.  The
 * cost is n^2 compares in total whatever C is: meant for CIFAR-sized epochs (n <= 2^28 is enforced; an ImageNet-sized epoch wants
 * a sort-based form, which this is not).  workspace: kanvit_metrics_auc_pairs_workspace(n, C) bytes (a pure host function; 0 for
 * arguments the call refuses), 16-byte aligned.  KANVIT_EINVAL for a null pointer, C < 2, n < 1, n > cap, n > 2^28, a short or
 * misaligned workspace.
 * Neither call synchronises with the host; both are capturable.  Additive: the ABI version stays 7. */
int kanvit_metrics_update(const void* logits, int logits_bf16, int64_t ld, const int64_t* labels, int64_t B, int C, int64_t n0, int64_t cap,
                          float* probs_t, int32_t* labels_out, int32_t* preds_out, int64_t* confusion, void* stream);
size_t kanvit_metrics_auc_pairs_workspace(int64_t n, int C);
int kanvit_metrics_auc_pairs(const float* probs_t, const int32_t* labels, int64_t n, int C, int64_t cap, int64_t* counts, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ---- fused AdamW step: global-norm clipping, schedule table, weight EMA (kanvit/optim.py; csrc/optim.hip) -----------------
 * Multi-tensor launches over fp32 tensors: up to KANVIT_OPTIM_MAX_TENSORS (the host query returns it) per call, passed BY VALUE in
 * the kernel arguments -- no device-side pointer table, and the pointers a HIP-graph capture records are the tensors' own.  A
 * work-group takes one chunk of KANVIT_OPTIM_CHUNK elements of one tensor.  The arrays params / grads / offsets / numel / decay are
 * HOST arrays of n entries; a tensor with numel = 0 may have null pointers and gets no work-group; n = 0 launches nothing.
 *
 * Sum of squares: the partials of tensor i's chunks follow those of tensor i - 1 in `workspace` (float64, one per chunk;
 * kanvit_optim_sumsq_workspace(n, numel) bytes, a pure host function, 0 for arguments the call refuses).  A chunk's partial is the
 * float64 sum of the float64 squares (exact products): thread t of 256 adds elements 4 (256 r + t) + k in the order r = 0..3,
 * k = 0..3, then part[t] += part[t + o] for o = 128, 64, .., 1.  No atomics: the same bits on every run, whatever the alignment.
 * Several calls fill one workspace side by side (the caller advances the pointer).
 *
 * Begin: one work-group.  S = the float64 sum of partials[0 .. n_partials) (thread t adds t, t + 256, .. in order, then the same
 * tree); norm_coef[0] = (float)sqrt(S); norm_coef[1] = (float)min(1, max_norm / (sqrt(S) + 1e-6)) evaluated in float64 and rounded
 * once -- torch's clip_grad_norm_ rule -- or 1 when max_norm <= 0 (no clipping); step[0] += 1 (int64).  partials = NULL with
 * n_partials = 0 and max_norm <= 0: the norm is not taken and norm_coef[0] = NaN.  A non-finite norm is not special-cased: a NaN
 * sum gives a NaN coefficient, as torch's clamp does.
 *
 * Update: with t = step[0] (already counted by the begin call) and row = table[min(t, table_rows) - 1] of the [table_rows][4]
 * float table (1 - lr_t wd, lr_t / (1 - b1^t), sqrt(1 - b2^t), 1 - d^t), every element runs this sequence, each operation one
 * fp32 rounding, none contracted into an fma, denormals kept, division and square root correctly rounded:
 *   g   = fmul(g, coef)                                  (norm_coef != NULL only; coef = norm_coef[1])
 *   p   = fmul(p, row[0])                                (has_wd != 0 and decay[i] != 0 only)
 *   m   = fadd(fmul(b1, m), fmul(ob1, g))
 *   v   = fadd(fmul(b2, v), fmul(fmul(ob2, g), g))
 *   den = fadd(fdiv(fsqrt(v), row[2]), eps)           (fsqrt: the correctly rounded square root, sqrtf -- not HIP's __fsqrt_rn)
 *   p   = fsub(p, fmul(row[1], fdiv(m, den)))
 *   e   = fadd(fmul(d, e), fmul(od, p))                  (ema != NULL only)
 * so a float32 restatement on the host gives the same bits.  m / v / e of tensor i are exp_avg / exp_avg_sq / ema + offsets[i]:
 * offsets are multiples of 4 elements and the three buffers 16-byte aligned, state_numel elements long.  p and g need 4-byte
 * alignment only; a tensor whose p and g are both 16-byte aligned moves as 16-byte accesses, any other as 4-byte ones, with
 * identical results.  row[3] debiases the EMA on read (weights = e / row[3]); the kernel does not use it.
 *
 * None of the calls synchronises with the host; all are capturable.  KANVIT_EINVAL (named in kanvit_last_error, checked before any
 * launch) for n outside 0..KANVIT_OPTIM_MAX_TENSORS, a null array or pointer, a negative numel, a pointer off its alignment, a
 * state slice outside the buffers or off a multiple of 4, a short workspace, table_rows < 1, a NaN max_norm, max_norm > 0 without
 * partials.  Additive: the ABI version stays 7. */
#define KANVIT_OPTIM_MAX_TENSORS 80
#define KANVIT_OPTIM_CHUNK 4096
int kanvit_optim_max_tensors(void);
size_t kanvit_optim_sumsq_workspace(int n, const int64_t* numel);
int kanvit_optim_sumsq(int n, const void* const* grads, const int64_t* numel, void* workspace, size_t workspace_bytes, void* stream);
int kanvit_optim_begin(const void* partials, int64_t n_partials, double max_norm, int64_t* step, float* norm_coef, void* stream);
int kanvit_optim_adamw(int n, void* const* params, const void* const* grads, const int64_t* offsets, const int64_t* numel,
                       const int32_t* decay, float* exp_avg, float* exp_avg_sq, float* ema, int64_t state_numel, const float* table,
                       int64_t table_rows, const int64_t* step, const float* norm_coef, int has_wd, float b1, float ob1, float b2, float ob2,
                       float eps, float d, float od, void* stream);

/* ---- KAN edge pruning: ranked edge masks, held at zero (csrc/edge_prune.hip) ----------------------------------
 * kanvit_edge_select: scores A[groups][E] (float32, device; the [out, in] activation table of kanvit_edge_l1_fwd, flat index
 * e = i O + o) -> mask[groups][E] (uint8, 1 = keep, any alignment) and kept[groups] (int64: the ones of the group's mask).
 * The order of the entries of a group is exact and total: key(a) = bits(a) & 0x7fffffff compared as uint32, ties broken by
 * ascending e.  A is finite and non-negative by construction; the key order defines the behaviour for every other input (a
 * negative entry ranks as its magnitude, a NaN above every number) and the kernel does not special-case them.
 *   KANVIT_PRUNE_COUNT  exactly the n_prune smallest entries of every group in that order get 0; 0 <= n_prune <= E - 1, so a
 *                       group always keeps its strongest edge.  Where the cut falls inside a run of equal keys the lower flat
 *                       indices are the pruned ones.  threshold is ignored.
 *   KANVIT_PRUNE_ABS    mask = key(a) >= key(threshold); threshold finite and >= 0.  n_prune is ignored.
 *   KANVIT_PRUNE_REL    mask = key(a) >= key(t_g), t_g = fmul(threshold, max_g): ONE fp32 rounding, denormals kept, max_g the
 *                       float whose bits are the group's largest key; 0 <= threshold <= 1, so the maximum always stays.
 * One work-group per group: a group's result does not depend on the other groups of the launch.  An exact radix select on the
 * keys (integer LDS histograms) and one index-ordered pass that walks laps of KANVIT_EDGE_SELECT_LAP entries; no atomics on
 * floats, no global atomics, no workspace, no host synchronisation: capturable, and the same bits on every run.  groups = 0
 * launches nothing.  KANVIT_EINVAL (named in kanvit_last_error, checked before any launch) for an unknown mode, groups outside
 * 0..2^31-1, E outside 1..2^31-1, n_prune outside 0..E-1 (COUNT), a NaN, negative or infinite threshold, or one above 1 in REL
 * mode, a null pointer, A off 4-byte or kept off 8-byte alignment.
 *
 * kanvit_mask_rows: a multi-tensor launch in the style of kanvit_optim_adamw -- up to KANVIT_MASK_MAX_TENSORS tensors (the host
 * query returns it) passed BY VALUE in the kernel arguments, so a captured graph keeps the tensors' own pointers; tensors / numel /
 * run / masks are HOST arrays of n entries.  Tensor k is fp32 with numel[k] elements seen as rows of run[k] contiguous ones:
 *   x[e] = masks[k][e / run[k]] ? x[e] : +0.0f
 * a select, not a multiply: a kept element keeps its bits (the kernel neither reads nor writes it), a masked NaN, infinity or
 * -0 becomes +0.  Tensors need 4-byte alignment only; a 16-byte-aligned one may take 16-byte stores, with identical results;
 * masks are uint8 (0 = masked) at any alignment, and one mask may serve several tensors.  A work-group takes one chunk of
 * KANVIT_MASK_CHUNK elements of one tensor; a tensor with numel = 0 may have null pointers and gets none; n = 0 launches nothing.
 * No host synchronisation; capturable.  KANVIT_EINVAL (named in kanvit_last_error, checked before any launch) for n outside
 * 0..KANVIT_MASK_MAX_TENSORS, a null array or pointer, a negative numel, run[k] < 1 or numel[k] % run[k] != 0, a tensor off
 * 4-byte alignment.  Additive: the ABI version stays 7. */
#define KANVIT_PRUNE_COUNT 0
#define KANVIT_PRUNE_ABS 1
#define KANVIT_PRUNE_REL 2
#define KANVIT_EDGE_SELECT_LAP 4096
#define KANVIT_MASK_MAX_TENSORS 80
#define KANVIT_MASK_CHUNK 4096
int kanvit_edge_select(const float* A, int64_t groups, int64_t E, int mode, float threshold, int64_t n_prune, uint8_t* mask, int64_t* kept,
                       void* stream);
int kanvit_mask_max_tensors(void);
int kanvit_mask_rows(int n, void* const* tensors, const int64_t* numel, const int64_t* run, const uint8_t* const* masks, void* stream);

/* ---- per-family named entry points (SURVEY.md section 8b naming) ----------------------------
 * kanvit_<family>_{fwd,bwd_input,bwd_weight} are kanvit_layer_* with d->family checked;
 * kanvit_<family>_qkv_* additionally require groups == 3 * x_group_mod (one launch for all
 * heads' q, k and v mappings).                                                                 */
#define KANVIT_DECLARE_FAMILY(name)                                                                           \
    int kanvit_##name##_fwd(const kanvit_layer_desc*, const float*, const float*, const float*, const float*, \
                            const float*, float*, void*, size_t, void*);                                      \
    int kanvit_##name##_bwd_input(const kanvit_layer_desc*, const float*, const float*, const float*,         \
                                  const float*, const float*, float*, float*, float*, void*, size_t, void*);  \
    int kanvit_##name##_bwd_weight(const kanvit_layer_desc*, const float*, const float*, const float*,        \
                                   const float*, float*, void*, size_t, void*);                               \
    int kanvit_##name##_qkv_fwd(const kanvit_layer_desc*, const float*, const float*, const float*,           \
                                const float*, const float*, float*, void*, size_t, void*);                    \
    int kanvit_##name##_qkv_bwd_input(const kanvit_layer_desc*, const float*, const float*, const float*,     \
                                      const float*, const float*, float*, float*, float*, void*, size_t,      \
                                      void*);                                                                 \
    int kanvit_##name##_qkv_bwd_weight(const kanvit_layer_desc*, const float*, const float*, const float*,    \
                                       const float*, float*, void*, size_t, void*);
KANVIT_DECLARE_FAMILY(linear)
KANVIT_DECLARE_FAMILY(cheby)
KANVIT_DECLARE_FAMILY(bspline)
KANVIT_DECLARE_FAMILY(rbf)
KANVIT_DECLARE_FAMILY(sine)
KANVIT_DECLARE_FAMILY(fourier)

/* ---- misc ---------------------------------------------------------------------------------- */
int kanvit_abi_version(void);
const char* kanvit_last_error(void);
/* Kernel-selection switches (KANVIT_NO_REG, KANVIT_NO_BF16, KANVIT_ATTN_V1, ...: fallback kernels for the parity tests and two
 * tuning knobs).  The environment is read ONCE, on first use of the library -- never on the launch path; kanvit_config()
 * returns the active set as "name=value ..." (all zero = the default kernels) so a measurement can say what it ran, and
 * kanvit_config_reload() re-reads the environment (test hook; not for use while launches are in flight).            */
const char* kanvit_config(void);
int kanvit_config_reload(void);
/* number of HIP devices visible, or a negative error code; does not initialise a context */
int kanvit_device_count(void);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif /* KANVIT_H */
