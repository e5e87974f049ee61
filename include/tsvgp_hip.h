/*
 * tsvgp_hip.h -- C ABI of the MI355X (gfx950) t-SVGP natural-gradient E-step kernels.
 *
 * The reference (AaltoML/t-SVGP) is pure Python on TensorFlow/GPflow and has NO FFI;
 * this header is the seam introduced *under* its Python API.
 * Every entry point replaces a group of TensorFlow ops on the hot path
 * `t_SVGP.natgrad_step` (reference src/models/tsvgp.py:234-304); the citation on each
 * declaration names the reference lines it stands in for.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch / C++ types.
 *   - All pointers are DEVICE pointers (caller-allocated, caller-owned) unless the parameter name ends in `_host`
 *     (small arrays of per-latent scalars, read during the call and passed on as kernel arguments); `stream` is a
 *     hipStream_t passed as void* (NULL = default stream).  No allocation and no
 *     synchronisation inside: safe to capture into a hipGraph.  The only process-wide
 *     state is one "dynamic-LDS opt-in done" flag per (kernel, device) for the two
 *     kernels that use more than 64 KB of LDS (set on first use, thread-safe; any
 *     device of the process may be current).
 *   - Input dimension policy (one for the fill and for the M-step gradient): the fused kernels pad D to a compile-time
 *     size -- D <= 32 for the fill (tsvgp_kernel_fill_*), D <= 16 for the gradient contraction (tsvgp_kernel_grad_*);
 *     larger D returns 1 from them.  Beyond that the scaled distance is a GEMM, r2 = |x~|^2 + |z~|^2 - 2 x~ z~^T,
 *     taken from the BLAS library by the host, and an elementwise kernel finishes it in place:
 *     tsvgp_gram_to_kernel_* (K(X, Z)) and tsvgp_gram_to_gradw_* (the gradient's weight matrix W); any D.
 *   - Suffix _f64 / _f32 selects the arithmetic type T of the N-sized arrays.
 *   - "Padded" dimensions: Np = N rounded up to 128, Mp = M rounded up to 128.  Work
 *     buffers (Kfu, B) are [Np x Mp] row-major with the padding ZERO-filled by the
 *     producing kernel, so the MFMA kernels need no bounds checks.
 *   - Return value: 0 ok; 1 invalid argument; 2 launch failure (hipGetLastError != 0).
 */
#ifndef TSVGP_HIP_H
#define TSVGP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSVGP_OK 0
#define TSVGP_EINVAL 1
#define TSVGP_ELAUNCH 2

#define TSVGP_TILE 128 /* padding granule of N and M */
#define TSVGP_MAX_BATCH 32 /* latent GPs per launch of the *_batched entry points (their per-latent scalars travel as
                              kernel arguments); callers with more latents issue several calls */

/* likelihood selectors for tsvgp_moments_* */
#define TSVGP_LIK_NONE 0      /* moments only (predict_f) */
#define TSVGP_LIK_GAUSSIAN 1  /* gpflow.likelihoods.Gaussian: closed form */
#define TSVGP_LIK_BERNOULLI 2 /* gpflow.likelihoods.Bernoulli, probit + 1e-3 jitter, 20-pt Gauss-Hermite */
#define TSVGP_LIK_HETERO 3    /* gpflow.likelihoods.HeteroskedasticTFPConditional (Normal, Exp scale) over TWO coupled latents:
                                 tsvgp_lik_map_hetero_* only (the moments kernels and tsvgp_lik_map_* reject it) */
#define TSVGP_LIK_SOFTMAX 4   /* gpflow.likelihoods.Softmax(C) (a MonteCarloLikelihood) over C coupled latents:
                                 tsvgp_lik_map_softmax_* only */
#define TSVGP_LIK_STUDENT_T 5 /* gpflow.likelihoods.StudentT(scale, df), 20-pt Gauss-Hermite: tsvgp_lik_map_scalar_* only */
#define TSVGP_LIK_POISSON 6   /* gpflow.likelihoods.Poisson(binsize), exp link, closed form: tsvgp_lik_map_scalar_* only */
#define TSVGP_LIK_MULTICLASS 7 /* gpflow.likelihoods.MultiClass(C) with the RobustMax link over C coupled latents, 20-pt
                                  Gauss-Hermite over the labelled latent: tsvgp_lik_map_robustmax_* only */
#define TSVGP_LIK_GAMMA 8     /* gpflow.likelihoods.Gamma(shape), exp link, closed form (shape = 1: gpflow.likelihoods.Exponential):
                                 tsvgp_lik_map_scalar_* only */
#define TSVGP_LIK_ORDINAL 9   /* gpflow.likelihoods.Ordinal(bin_edges), 20-pt Gauss-Hermite: tsvgp_lik_map_ordinal_* only */
#define TSVGP_LIK_NOCROP 0x100 /* OR-ed into the selector: leave g1 = d ve/d var uncropped (reference
                                  src/models/tsvgp_white.py:188-191 has no crop; src/models/tsvgp.py:262-263 has) */
#define TSVGP_LIK_MEANONLY 0x200 /* OR-ed into the selector (NONE or GAUSSIAN only): skip the variance product.  Under a
                                    Gaussian likelihood g0 = (y - mean)/s2 and g1 = -1/(2 s2) do not depend on the
                                    predictive variance, so the natural-gradient step (src/models/tsvgp.py:246-263)
                                    needs the mean alone: one HBM-bound sweep of A instead of the MFMA product.
                                    Tm and mode are ignored, var must be NULL, Mp*P*sizeof(T) <= 128 KB (gamma sits in LDS), ve_partial is written as NaN (the
                                    variational expectation itself does need the variance), nonpos_partial counts rows with a
                                    non-finite mean or gradient. */

/* k-range selectors of the panel product C[n,i] = sum_j A[n,j] * Tm[i,j] */
#define TSVGP_TRI_LOWER 0 /* j <= i  (forward substitution with the inverted factor)   */
#define TSVGP_TRI_UPPER 1 /* j >= i  (product with a transposed lower factor)         */
#define TSVGP_TRI_DENSE 2 /* all j                                                    */

/* Library / build identification: returns a static string "tsvgp_hip gfx950 <version>". */
const char *tsvgp_version(void);
/* Number of this header's calling conventions: bumped whenever an entry point's argument list changes without a new symbol
 * name.  A binding checks it against the TSVGP_ABI_VERSION it was written for before the first call (t-svgp_amd/_backend.py
 * refuses a library whose number differs: a shifted argument would otherwise hand a kernel a garbage stream or pointer). */
#define TSVGP_ABI_VERSION 5
int tsvgp_abi_version(void);

/* Upper bound on the number of workgroup slots the site-accumulation kernel can keep resident
 * (CUs x resident workgroups per CU for that kernel); used by the host to choose `nsplit`. */
int tsvgp_site_accum_slots_f64(void);
int tsvgp_site_accum_slots_f32(void);

/* (1) Kernel-matrix fill: squared-exponential K(X, Z) -> K[n, m] = variance * exp(-0.5 * sum_d ((x_nd - z_md) * inv_ls_d)^2)
 *     Replaces gpflow.covariances.Kuf / Kuu (reference src/models/tsvgp.py:209-211, 222-225, 268-269).
 *     X [N x D] row-major, Z [M x D] row-major, inv_ls [D] (1/lengthscale per dimension),
 *     K [rows_alloc x ldk] row-major with rows_alloc >= round_up(N,128) and ldk >= round_up(M,128); entries with n >= N or
 *     m >= M (up to the padded extents) are written as 0.  D <= 32 (padded to 1, 2, 4, 8, 16 or 32 inside).
 *     fp64: exp is the device library's algorithm restated for arguments <= 0 (bit-identical values).  An output of 512 MB or
 *     more is written with non-temporal stores (it cannot stay cached for its reader; work on other streams keeps its L2).
 *     ldk even and K on a boundary of two elements -- 16 bytes in fp64, 8 bytes in fp32 (a thread stores its adjacent columns as
 *     one vector; TSVGP_EINVAL otherwise, before any launch).  fp32 with D <= 16 stores four columns per thread (16 bytes) when
 *     K is on a 16-byte boundary and ldk (and strideK of (1c)) a multiple of 4, else two: the same values either way.  The same
 *     rule holds for (1b). */
int tsvgp_se_fill_f64(const double *X, const double *Z, const double *inv_ls, double variance, double *K, int64_t N,
                      int M, int D, int64_t ldk, void *stream);
int tsvgp_se_fill_f32(const float *X, const float *Z, const float *inv_ls, float variance, float *K, int64_t N, int M,
                      int D, int64_t ldk, void *stream);

/* (1b) The same fill for the other stationary kernels of the reference's experiments (experiments/uci_regression.py:42-44
 *     uses gpflow.kernels.Matern52): K = variance * k(r), r^2 = sum_d ((x_nd - z_md) * inv_ls_d)^2 (r = sqrt(max(r^2, 1e-36))
 *     as GPflow), kind one of TSVGP_KERNEL_*.  TSVGP_KERNEL_SE is tsvgp_se_fill_*. */
#define TSVGP_KERNEL_SE 0       /* exp(-r^2 / 2) */
/* (1 is reserved: Matern-1/2 = exp(-r) is not offered -- it is not differentiable at r = 0, so GPflow's own expanded-form
 * r^2 leaves 1e-8 relative rounding noise on K(Z, Z) and no 1e-8 parity statement can be made for it) */
#define TSVGP_KERNEL_MATERN32 2 /* (1 + sqrt(3) r) exp(-sqrt(3) r) */
#define TSVGP_KERNEL_MATERN52 3 /* (1 + sqrt(5) r + 5 r^2 / 3) exp(-sqrt(5) r) */
int tsvgp_kernel_fill_f64(int kind, const double *X, const double *Z, const double *inv_ls, double variance, double *K,
                          int64_t N, int M, int D, int64_t ldk, void *stream);
int tsvgp_kernel_fill_f32(int kind, const float *X, const float *Z, const float *inv_ls, float variance, float *K,
                          int64_t N, int M, int D, int64_t ldk, void *stream);

/* (1c) The fill for P latent GPs with one kernel each on shared inputs and shared inducing points
 *     (gpflow SeparateIndependent + SharedIndependentInducingVariables, reference docs/notebooks/heteroskedastic.py:62-76;
 *     Kuf [P, M, N] at src/models/tsvgp.py:269 for BASELINE configs[4]) in ONE launch:
 *        K[p][n, m] = variance[p] * k(r_p),   r_p^2 = sum_d ((x_nd - z_md) * inv_ls[p*D + d])^2,   latent p at K + p*strideK.
 *     inv_ls [P x D] is a device array; variance_host [P] is a HOST array (the scalars travel as kernel arguments, exactly
 *     as `variance` does above).  1 <= P <= TSVGP_MAX_BATCH; strideK >= round_up(N,128) * ldk, even; K on a boundary of two
 *     elements as in (1) -- with the even strideK every K + p*strideK is then on it too (TSVGP_EINVAL otherwise, before any launch). */
int tsvgp_kernel_fill_batched_f64(int kind, const double *X, const double *Z, const double *inv_ls,
                                  const double *variance_host, double *K, int64_t strideK, int64_t N, int M, int D,
                                  int64_t ldk, int P, void *stream);
int tsvgp_kernel_fill_batched_f32(int kind, const float *X, const float *Z, const float *inv_ls,
                                  const float *variance_host, float *K, int64_t strideK, int64_t N, int M, int D,
                                  int64_t ldk, int P, void *stream);

/* (1s) The fill of a SUM of C stationary kernels (gpflow.kernels.Sum / k1 + k2 [ext]) on shared inputs, in ONE launch and one
 *     write of K:
 *        K[n, m] = sum_c variance[c] * k_{kind[c]}(r_c),   r_c^2 = sum_d ((x_nd - z_md) * inv_ls[c*D + d])^2,
 *     the components added in index order, profiles and difference-form distance exactly as (1b) (same device functions).  A
 *     component that acts on some input columns only has zeros in its row of inv_ls.  inv_ls [C x D] is a device array;
 *     kinds_host [C] and variance_host [C] are HOST arrays (they travel as kernel arguments, as variance_host of (1c)).
 *     1 <= C <= TSVGP_MAX_COMPONENTS, every kind one of TSVGP_KERNEL_* (the reserved 1 is refused).  Everything else as (1):
 *     padding rows and columns up to the 128-multiples are written as exact zeros, D <= 32, ldk even and K on a boundary of
 *     two elements (fp32 stores four columns per thread where K is on a 16-byte boundary and ldk a multiple of 4, else two:
 *     the same values either way), non-temporal stores from 512 MB up; TSVGP_EINVAL before any launch otherwise.  With
 *     C * Dpad <= 32 (Dpad = D padded to 1, 2, 4, 8, 16, 32) a thread keeps the scaled Z columns of all components in registers;
 *     beyond it reloads them per component and chunk of 8 rows (csrc/tsvgp_sumfill.hip). */
#define TSVGP_MAX_COMPONENTS 4
int tsvgp_kernel_fill_sum_f64(const int *kinds_host, const double *X, const double *Z, const double *inv_ls,
                              const double *variance_host, double *K, int64_t N, int M, int D, int64_t ldk, int C,
                              void *stream);
int tsvgp_kernel_fill_sum_f32(const int *kinds_host, const float *X, const float *Z, const float *inv_ls,
                              const float *variance_host, float *K, int64_t N, int M, int D, int64_t ldk, int C, void *stream);

/* (1p) The fill of a PRODUCT of C stationary kernels (gpflow.kernels.Product / k1 * k2 [ext]) on shared inputs, in ONE launch and
 *     one write of K:
 *        K[n, m] = variance * prod_c k_{kind[c]}(r_c),   r_c^2 = sum_d ((x_nd - z_md) * inv_ls[c*D + d])^2,
 *     variance = prod_c variance_c formed by the caller.  The kernel of (1s) under a compile-time flag: the same device functions
 *     for the profiles and the difference-form distance, the components multiplied in index order starting from 1, the variance
 *     last.  inv_ls [C x D] is a device array (zeros on a component's inactive columns), kinds_host [C] a HOST array.  Everything
 *     else as (1s): 1 <= C <= TSVGP_MAX_COMPONENTS, the reserved kind 1 refused, padding rows and columns written as exact zeros,
 *     D <= 32, ldk even and K on a boundary of two elements (the fp32 four-column store where K is on a 16-byte boundary and ldk a
 *     multiple of 4), non-temporal stores from 512 MB up, both register forms; TSVGP_EINVAL before any launch otherwise. */
int tsvgp_kernel_fill_prod_f64(const int *kinds_host, const double *X, const double *Z, const double *inv_ls, double variance,
                               double *K, int64_t N, int M, int D, int64_t ldk, int C, void *stream);
int tsvgp_kernel_fill_prod_f32(const int *kinds_host, const float *X, const float *Z, const float *inv_ls, float variance,
                               float *K, int64_t N, int M, int D, int64_t ldk, int C, void *stream);

/* (1d) Input dimensions beyond 32 (the reference's MNIST notebook has D = 784): the scaled squared distance is then a
 *     GEMM, r2[n,m] = xx[n] + zz[m] - 2 G[n,m] with G = (X/l)(Z/l)^T (GPflow's square_distance form [ext]), which the caller
 *     takes from the BLAS library into K [rows_pad x ldk]; this call turns it into K = variance * k(r2) in place and
 *     zero-fills the padding (rows >= N, columns >= M).  xx [N], zz [M]: squared norms of the scaled rows.  ldk even and K on a
 *     boundary of two elements (16 bytes in fp64, 8 in fp32: a thread loads and stores its two columns as one vector;
 *     TSVGP_EINVAL otherwise, before any launch).  A slightly negative r2 (rounding of the expanded form) goes into the profile
 *     as it is: the squared exponential returns variance * exp(-r2 / 2) > variance, the Matern kernels clamp. */
int tsvgp_gram_to_kernel_f64(int kind, double *K, const double *xx, const double *zz, double variance, int64_t N, int M,
                             int64_t ldk, void *stream);
int tsvgp_gram_to_kernel_f32(int kind, float *K, const float *xx, const float *zz, float variance, int64_t N, int M,
                             int64_t ldk, void *stream);

/* (1e) Joint predictive covariance of one latent GP over N test points (GPflow conditional(..., full_cov=True) [ext], reference
 *     src/models/tsvgp.py:103-112, src/models/tsvgp_white.py:122, src/models/tsvgp_sites.py:179-187): a symmetric rank-Mp update
 *     with the kernel function in the epilogue,
 *        C[i, j] = C[j, i] = base(i, j) + sign * sum_{m < Mp} T[i, m] * T[j, m]            i, j < N
 *        base(i, j) = variance * k_kind(r(x_i, x_j))        r as tsvgp_kernel_fill_* (same device functions, D <= 32)
 *                   = C[i, j] as found on entry             with TSVGP_COV_ACCUMULATE in flags: only the LOWER triangle (j <= i) is
 *                                                           read; kind, X, inv_ls, variance and D are ignored (X, inv_ls may be NULL)
 *     T [Np x Mp] row-major is the tile tsvgp_trmm_* writes (row n = Tm a_n, rows >= N zero), X [N x D], inv_ls [D], sign -1.0 or
 *     +1.0, C [Np x ldc] with ldc >= Np.  Np = N rounded up to 128; rows and columns >= N of C are written as 0 off the diagonal
 *     and 1 ON it -- the identity block tsvgp_potrf_f64 asks for, so C can be factored in place.  T and C on 16-byte boundaries,
 *     ldc * sizeof(element) a multiple of 16, Np <= 128 * 32768.  One workgroup per 128 x 128 tile of the lower block triangle
 *     stores the tile and its transpose; the upper part of a diagonal tile is a copy of its lower part, so C == C^T bit for bit;
 *     no atomics, fixed summation order.  The variance forms of the models:
 *        kff - |Tm a|^2                                 one call, sign -1
 *        kff - |b|^2 + |T2 b|^2 (t_SVGP_white)          one call on the whitened tile b, sign -1; then ACCUMULATE on T2 b, sign +1
 *        D > 32                                         K(X, X) into C by BLAS + tsvgp_gram_to_kernel_*; then ACCUMULATE, sign -1 */
#define TSVGP_COV_ACCUMULATE 1
int tsvgp_cov_f64(int kind, const double *T, const double *X, const double *inv_ls, double variance, double sign, double *C,
                  int64_t N, int64_t Np, int Mp, int D, int64_t ldc, int flags, void *stream);
int tsvgp_cov_f32(int kind, const float *T, const float *X, const float *inv_ls, float variance, float sign, float *C, int64_t N,
                  int64_t Np, int Mp, int D, int64_t ldc, int flags, void *stream);

/* (1c) M-step gradient for D beyond tsvgp_kernel_grad_*'s sizes, GEMM form (replaces TensorFlow autodiff through Kuf [ext],
 *     reference experiments/uci_regression.py:159-160, docs/notebooks/mnist.py:117-192 with D = 784).  G [N x ldk] holds the
 *     Gram block x~ z~^T on entry; on return W = -2 variance V * k'(r2) with V = g0 beta^T - 2 g1 * U (padding zero), and
 *     vpart [tsvgp_gram_to_gradw_parts(N, M)] one partial sum of V k(r2) per workgroup (d ELBO / d variance = their sum).
 *     g0, g1: element stride gstride; beta: element stride bstride; U [N x ldu].  ldk and ldu even, G and U on a boundary of two
 *     elements (16 bytes in fp64, 8 in fp32; TSVGP_EINVAL otherwise, before any launch).  The caller finishes in M x D:
 *     dZ = (W^T x~ - z~ * colsum W) / l,  d l_d = (sum_n x~_nd^2 rowsum_n - 2 sum_m z~_md (W^T x~)_md + sum_m z~_md^2 colsum_m) / l_d. */
int64_t tsvgp_gram_to_gradw_parts(int64_t N, int M);
int tsvgp_gram_to_gradw_f64(int kind, double *G, const double *xx, const double *zz, double variance, const double *U,
                            int64_t ldu, const double *g0, const double *g1, int gstride, const double *beta, int bstride,
                            int64_t N, int M, int64_t ldk, double *vpart, void *stream);
int tsvgp_gram_to_gradw_f32(int kind, float *G, const float *xx, const float *zz, float variance, const float *U, int64_t ldu,
                            const float *g0, const float *g1, int gstride, const float *beta, int bstride, int64_t N, int M,
                            int64_t ldk, double *vpart, void *stream);

/* (2) Blocked triangular solve with an N-sized right-hand side, in inverted-factor form:
 *        C[n, i] = sum_{j in range(i)} A[n, j] * Tm[i, j],   range = j<=i | j>=i | all j   (mode)
 *     With Tm = inv(chol(Kuu + jitter I)) and mode LOWER this is B = Kfu * L^-T, i.e. the forward substitution
 *     L^-1 Kuf of tf.linalg.cholesky_solve / triangular_solve (reference src/models/tsvgp.py:270-271 and GPflow's
 *     conditional behind :103), done as MFMA tile products.
 *     A, C [Np x Mp] row-major (lda/ldc = Mp), Tm [Mp x Mp] row-major, zero outside its triangle/valid block. */
int tsvgp_trmm_f64(const double *A, const double *Tm, double *C, int64_t Np, int Mp, int mode, void *stream);
int tsvgp_trmm_f32(const float *A, const float *Tm, float *C, int64_t Np, int Mp, int mode, void *stream);

/* (2b) The same solve batched over the latent dimension (the rank-3 A = cholesky_solve(chol(Kuu [P,M,M]),
 *     Kuf [P,M,N]) of reference src/models/tsvgp.py:270-277 for one kernel per latent): latent b < batch reads
 *     A + b*strideA (strideA = 0: one operand shared by all latents) and Tm + b*strideT, writes C + b*strideC, one launch.
 *     In place (C == A with strideC == strideA) is allowed for TSVGP_TRI_UPPER only: a workgroup owns its 128-row panel,
 *     takes the output column tiles in increasing order, and tile `it` reads only columns >= 128*it before it overwrites
 *     columns [128*it, 128*it + 128).  batch <= 65535; strideC >= Np*Mp when batch > 1. */
int tsvgp_trmm_batched_f64(const double *A, int64_t strideA, const double *Tm, int64_t strideT, double *C,
                           int64_t strideC, int64_t Np, int Mp, int mode, int batch, void *stream);
int tsvgp_trmm_batched_f32(const float *A, int64_t strideA, const float *Tm, int64_t strideT, float *C, int64_t strideC,
                           int64_t Np, int Mp, int mode, int batch, void *stream);

/* (3)+(4) Fused predictive moments and likelihood-gradient map.
 *     For every row n < N and latent p < P:
 *        q    = sum_i ( sum_{j in range(i)} A[n,j] * Tm[p][i,j] )^2
 *        mean = sum_j A[n,j] * gamma[j*P + p]
 *        var  = kdiag - q
 *     then (lik != NONE)  g0 = d ve/d mean,  g1 = min(d ve/d var, -1e-8),  ve_sum += ve.
 *     Replaces base_SVGP.predict_f / GPflow conditional (reference src/models/tsvgp.py:97-114, :246), the site-form
 *     predictive (src/util.py:175-184), likelihood.variational_expectations + GradientTape (:256-259) and the crop (:262-263).
 *     A [Np x Mp]; Tm [P x Mp x Mp]; gamma [Mp x P]; Y [N x P]; outputs mean,var [N x P] (may be NULL),
 *     g0,g1 [Np x P] (rows >= N written as 0; may be NULL when lik == NONE);
 *     ve_partial [Np/128] doubles (per-workgroup sums of ve; may be NULL when lik == NONE);
 *     nonpos_partial [Np/128] int32 (count of var <= 0, the tf.debugging.assert_positive of :113).
 *     lik_param: Gaussian noise variance (ignored otherwise). */
int tsvgp_moments_f64(const double *A, const double *Tm, const double *gamma, const double *Y, double kdiag, int lik,
                      double lik_param, double *mean, double *var, double *g0, double *g1, double *ve_partial,
                      int32_t *nonpos_partial, int64_t N, int64_t Np, int Mp, int P, int mode, void *stream);
int tsvgp_moments_f32(const float *A, const float *Tm, const float *gamma, const float *Y, double kdiag, int lik,
                      double lik_param, float *mean, float *var, float *g0, float *g1, double *ve_partial,
                      int32_t *nonpos_partial, int64_t N, int64_t Np, int Mp, int P, int mode, void *stream);

/* (4) The likelihood-gradient map on its own (reference src/models/tsvgp.py:256-263: GPflow variational_expectations [ext] +
 *     tf.GradientTape): mean, var, Y [N x P] -> g0 = d ve / d mean, g1 = d ve / d var [Np x P] (rows >= N zero; g1 cropped at
 *     -1e-8 unless TSVGP_LIK_NOCROP), ve_partial / nonpos_partial [Np / 128] as tsvgp_moments_*.  lik = TSVGP_LIK_GAUSSIAN
 *     (lik_param = noise variance) or TSVGP_LIK_BERNOULLI.  The moments kernels run this map in their epilogue; this entry
 *     point serves a caller that assembled the moments itself (t_SVGP_white's two-product variance). */
int tsvgp_lik_map_f64(const double *mean, const double *var, const double *Y, int lik, double lik_param, double *g0, double *g1,
                      double *ve_partial, int32_t *nonpos_partial, int64_t N, int64_t Np, int P, void *stream);
int tsvgp_lik_map_f32(const float *mean, const float *var, const float *Y, int lik, double lik_param, float *g0, float *g1,
                      double *ve_partial, int32_t *nonpos_partial, int64_t N, int64_t Np, int P, void *stream);

/* (4b) The heteroskedastic Gaussian likelihood map (reference docs/notebooks/heteroskedastic.py:58-76: gpflow
 *     HeteroskedasticTFPConditional [ext] with a Normal distribution and an Exp scale; 20 x 20 Gauss-Hermite grid): the first
 *     likelihood whose row couples two latents, log p(y | f0, f1) = log N(y | f0, exp(f1)^2), so it cannot run in the per-latent
 *     epilogue of the moments kernels.  mean, var [N x 2] (latent 0: location, latent 1: log scale), Y [N x 1] ->
 *     g0 = d ve / d mean, g1 = d ve / d var [Np x 2] of the quadrature sum (rows >= N zero; g1 cropped at -1e-8 unless
 *     TSVGP_LIK_NOCROP), ve_partial [Np / 128] (fp64 per-128-row sums of ve), nonpos_partial [Np / 128] (count of var <= 0 over
 *     both latents).  flags = TSVGP_LIK_HETERO, optionally | TSVGP_LIK_NOCROP.  Arithmetic in fp64 for either array type. */
int tsvgp_lik_map_hetero_f64(const double *mean, const double *var, const double *Y, int flags, double *g0, double *g1,
                             double *ve_partial, int32_t *nonpos_partial, int64_t N, int64_t Np, void *stream);
int tsvgp_lik_map_hetero_f32(const float *mean, const float *var, const float *Y, int flags, float *g0, float *g1,
                             double *ve_partial, int32_t *nonpos_partial, int64_t N, int64_t Np, void *stream);

/* (4b'') The MultiClass likelihood map with the RobustMax inverse link (gpflow.likelihoods.MultiClass(C), GPflow 2.2.1 [ext]): C
 *     coupled latents, deterministic.  With y the row's label, s_c = sqrt(max(var_c, 1e-10)), (x_i, w_i) = hermgauss(20),
 *        X_i  = mean_y + x_i sqrt(max(2 var_y, 1e-10)),   d_ci = (X_i - mean_c) / s_c,
 *        F_ci = 1/2 (1 + erf(d_ci / sqrt 2)) (1 - 2e-4) + 1e-4,   P_i = prod_{c != y} F_ci,   p = sum_i w_i / sqrt(pi) P_i,
 *        ve   = p log(1 - epsilon) + (1 - p) log(epsilon / (C - 1))
 *     and g0 = d ve / d mean, g1 = d ve / d var of that quadrature sum (reference src/models/tsvgp.py:256-263); with
 *     kappa = log(1 - epsilon) - log(epsilon / (C - 1)), r_ci = (1 - 2e-4) N(d_ci) / F_ci, z_i = sqrt(2) x_i:
 *        c != y:  g0_c = -kappa sum_i w_i/sqrt(pi) P_i r_ci / s_c,   g1_c = -kappa sum_i w_i/sqrt(pi) P_i r_ci d_ci / (2 var_c)
 *        c == y:  g0_y = kappa sum_i w_i/sqrt(pi) P_i sum_{c != y} r_ci / s_c,   g1_y = the same sum with z_i / (2 s_y) inside.
 *     The derivative through an active clip (var_c < 1e-10, 2 var_y < 1e-10) is zero, as under tf.clip_by_value.
 *     mean, var [N x C]; Y [N x 1] class labels 0 .. C-1 in the array type (never used as an address; a label that is not an
 *     integer in [0, C) makes its row's ve, g0, g1 NaN); flags = TSVGP_LIK_MULTICLASS, optionally | TSVGP_LIK_NOCROP;
 *     2 <= C <= TSVGP_MAX_BATCH; 0 < epsilon < 1.  g0, g1 [Np x C] (rows >= N zero; g1 cropped at -1e-8 unless
 *     TSVGP_LIK_NOCROP, a NaN stays NaN), ve_partial [Np / 128] (fp64 per-128-row sums of ve), nonpos_partial [Np / 128]: rows
 *     with any var_c <= 0 or a non-finite mean.  Arithmetic in fp64 for either array type.  No atomics, a summation order fixed
 *     by the shape: two calls agree bit for bit. */
int tsvgp_lik_map_robustmax_f64(const double *mean, const double *var, const double *Y, int flags, int C, double epsilon,
                                double *g0, double *g1, double *ve_partial, int32_t *nonpos_partial, int64_t N, int64_t Np,
                                void *stream);
int tsvgp_lik_map_robustmax_f32(const float *mean, const float *var, const float *Y, int flags, int C, double epsilon, float *g0,
                                float *g1, double *ve_partial, int32_t *nonpos_partial, int64_t N, int64_t Np, void *stream);

/* (4b') The scalar likelihoods without an arm in the moments kernels (GPflow 2.2.1 [ext]), one latent column per call, behind the
 *     moments like (4b): lik = TSVGP_LIK_STUDENT_T (param0 = scale > 0, param1 = df > 0), TSVGP_LIK_POISSON (param0 = binsize > 0,
 *     exp link; param1 ignored) or TSVGP_LIK_GAMMA (param0 = shape a > 0, exp link: scale = exp(f); param1 ignored), optionally
 *     | TSVGP_LIK_NOCROP.
 *        StudentT  log p(y | f) = lgamma((df+1)/2) - lgamma(df/2) - 1/2 log(df pi) - log scale - (df+1)/2 log1p(((y-f)/scale)^2 / df);
 *                  ve by 20-point Gauss-Hermite, g0 = sum_i w_i l'(f_i), g1 = sum_i w_i l'(f_i) z_i / (2 sqrt(var)), f_i = mean + sqrt(var) z_i
 *                  (the derivative of the quadrature sum, what tf.GradientTape returns at reference src/models/tsvgp.py:256-259)
 *        Poisson   ve = y (mean + log b) - b exp(mean + var/2) - lgamma(y + 1),  g0 = y - b exp(mean + var/2),  g1 = -1/2 b exp(mean + var/2)
 *        Gamma     the closed form under the exp link, e = y exp(-mean + var/2):
 *                  ve = -a mean - lgamma(a) + (a - 1) log y - e,  g0 = -a + e,  g1 = -e / 2,  d ve / d a = -mean - digamma(a) + log y.
 *                  At a == 1 exactly (gpflow.likelihoods.Exponential) the term (a - 1) log y is skipped, not multiplied, so y = 0
 *                  is a legal target there.
 *     mean, var, Y: row n at element n * in_stride (a column of an [N x P] array: in_stride = P), read for n < N only;
 *     g0, g1: row n at element n * out_stride, written for every n < Np (rows >= N zero; g1 cropped at -1e-8 unless
 *     TSVGP_LIK_NOCROP, a NaN stays NaN); ve_partial [Np / 128] (fp64 per-128-row sums of ve); dparam_partial [Np / 128] or NULL
 *     (per-128-row sums of the parameter derivative for the M-step: StudentT d ve / d scale, Gamma d ve / d shape; must be NULL
 *     for Poisson); nonpos_partial [Np / 128]: rows with var <= 0 or a non-finite mean; under Gamma also rows with y < 0, or
 *     with y == 0 at a != 1, whose ve is NaN.  Arithmetic in fp64 for either array type; the log-gamma (and digamma) terms that
 *     no row changes are taken once on the host.  No atomics, a summation order fixed by the shape: two calls agree bit for bit. */
int tsvgp_lik_map_scalar_f64(const double *mean, const double *var, const double *Y, int64_t in_stride, int lik, double param0,
                             double param1, double *g0, double *g1, int64_t out_stride, double *ve_partial, double *dparam_partial,
                             int32_t *nonpos_partial, int64_t N, int64_t Np, void *stream);
int tsvgp_lik_map_scalar_f32(const float *mean, const float *var, const float *Y, int64_t in_stride, int lik, double param0,
                             double param1, float *g0, float *g1, int64_t out_stride, double *ve_partial, double *dparam_partial,
                             int32_t *nonpos_partial, int64_t N, int64_t Np, void *stream);

/* (4b''') The Ordinal likelihood map (gpflow.likelihoods.Ordinal(bin_edges), GPflow 2.2.1 [ext]): one latent, K = n_edges + 1 ordered
 *     bins, one latent column per call with the conventions of (4b').  With y the row's label in {0 .. K-1},
 *        up = edges[y] (+inf for y = K-1),   lo = edges[y-1] (-inf for y = 0),   a = (up - f) / sigma,   b = (lo - f) / sigma,
 *        Phi~(x) = Phi(x) (1 - 2e-3) + 1e-3,   phi = Phi~(a) - Phi~(b),   log p(y | f) = log(phi + 1e-6),
 *     ve is the 20-point Gauss-Hermite sum over f_i = mean + sqrt(var) z_i (the nodes and weights of StudentT) and g0, g1,
 *     dparam are the derivatives of that sum (reference src/models/tsvgp.py:256-263), N the standard normal density:
 *        l'(f)       = -(1 - 2e-3) (N(a) - N(b)) / (sigma (phi + 1e-6)),     g0 = sum_i w_i l'(f_i),
 *        d l/d sigma = -(1 - 2e-3) (a N(a) - b N(b)) / (sigma (phi + 1e-6)), g1 = sum_i w_i l'(f_i) z_i / (2 sqrt(var)),
 *     the terms of an infinite edge being 0.  phi is evaluated as (1 - 2e-3) (Phi(a) - Phi(b)) from erfc on the side where both
 *     tail masses are small, so a bin in the far upper tail keeps its digits.
 *     edges [n_edges] fp64 in device memory for either array type, 1 <= n_edges <= TSVGP_ORDINAL_MAX_EDGES (staged into LDS once
 *     per workgroup).  THE CALLER guarantees that they are finite and strictly increasing: the entry cannot read device memory
 *     and does not check them.  sigma > 0, finite.  flags = TSVGP_LIK_ORDINAL, optionally | TSVGP_LIK_NOCROP.  Y holds the labels
 *     in the array type; a label that is not an integer in [0, K) is never used as an address, makes its row's ve, g0, g1 NaN
 *     and counts the row in nonpos_partial (the MultiClass convention).  mean, var, Y, in_stride, g0, g1, out_stride (rows >= N
 *     zero; g1 cropped at -1e-8 unless TSVGP_LIK_NOCROP, a NaN stays NaN), ve_partial, nonpos_partial [Np / 128] as in (4b');
 *     dparam_partial [Np / 128] or NULL: per-128-row sums of d ve / d sigma.  Arithmetic in fp64 for either array type.  No
 *     atomics, a summation order fixed by the shape: two calls agree bit for bit. */
#define TSVGP_ORDINAL_MAX_EDGES 255
int tsvgp_lik_map_ordinal_f64(const double *mean, const double *var, const double *Y, int64_t in_stride, int flags,
                              const double *edges, int n_edges, double sigma, double *g0, double *g1, int64_t out_stride,
                              double *ve_partial, double *dparam_partial, int32_t *nonpos_partial, int64_t N, int64_t Np,
                              void *stream);
int tsvgp_lik_map_ordinal_f32(const float *mean, const float *var, const float *Y, int64_t in_stride, int flags,
                              const double *edges, int n_edges, double sigma, float *g0, float *g1, int64_t out_stride,
                              double *ve_partial, double *dparam_partial, int32_t *nonpos_partial, int64_t N, int64_t Np,
                              void *stream);

/* (4b'''') The linear model of coregionalization (gpflow.kernels.LinearCoregionalization, gpflow.conditionals.util.mix_latent_gp,
 *     GPflow 2.2.1 [ext]): P outputs f = W g mixed from L independent latent GPs, 1 <= L, P <= TSVGP_MAX_BATCH.  W [P x L] fp64
 *     row-major in DEVICE memory for either array type (read at execution: a replayed graph sees the current values), staged
 *     into LDS once per workgroup.  One thread per row, one workgroup per 128 rows, fp64 arithmetic for either array type, no
 *     atomics and a summation order fixed by the shape: two calls agree bit for bit.  N > 0, Np a multiple of 128 with
 *     0 <= Np - N < 128.
 *     tsvgp_lmc_mix_*: mean_g, var_g [N x L] -> Fmu, Fvar [N x P],
 *        Fmu[n, p] = sum_l W[p, l] mean_g[n, l],   Fvar[n, p] = sum_l W[p, l]^2 var_g[n, l];
 *     nonpos_partial [Np / 128] or NULL: per 128 rows, the rows with any var_g <= 0 (or NaN) or a non-finite mean_g.
 *     tsvgp_lmc_unmix_*: the chain rule of the variational expectations through the mix, g0_f, g1_f [Np x P] (d ve / d Fmu,
 *     d ve / d Fvar, never cropped) -> g0_g, g1_g [Np x L] (rows >= N written as zeros),
 *        g0_g[n, l] = sum_p W[p, l] g0_f[n, p],   g1_g[n, l] = sum_p W[p, l]^2 g1_f[n, p]
 *     with g1_g cropped at -1e-8 (reference src/models/tsvgp.py:262-263) unless flags = TSVGP_LIK_NOCROP (no other bit); a NaN
 *     stays NaN.  dW_partial [Np / 128 x P x L] or NULL (given: mean_g, var_g [N x L] are required, otherwise they are not
 *     read): the sums over each 128 rows of  g0_f[n, p] mean_g[n, l] + 2 W[p, l] g1_f[n, p] var_g[n, l] = d ve_n / d W[p, l]; the
 *     caller adds the blocks. */
int tsvgp_lmc_mix_f64(const double *mean_g, const double *var_g, const double *W, double *Fmu, double *Fvar,
                      int32_t *nonpos_partial, int64_t N, int64_t Np, int L, int P, void *stream);
int tsvgp_lmc_mix_f32(const float *mean_g, const float *var_g, const double *W, float *Fmu, float *Fvar, int32_t *nonpos_partial,
                      int64_t N, int64_t Np, int L, int P, void *stream);
int tsvgp_lmc_unmix_f64(const double *g0_f, const double *g1_f, const double *W, int flags, double *g0_g, double *g1_g,
                        const double *mean_g, const double *var_g, double *dW_partial, int64_t N, int64_t Np, int L, int P,
                        void *stream);
int tsvgp_lmc_unmix_f32(const float *g0_f, const float *g1_f, const double *W, int flags, float *g0_g, float *g1_g,
                        const float *mean_g, const float *var_g, double *dW_partial, int64_t N, int64_t Np, int L, int P,
                        void *stream);

/* (4c) The per-datum site step of t_SVGP_sites (reference src/models/tsvgp_sites.py:113-148) fused with the likelihood map of
 *     (4): mean, var, Y [N x P] -> g0, g1 as tsvgp_lik_map_* (never cropped: TSVGP_LIK_NOCROP semantics whatever lik says), then
 *     IN PLACE on the fp64 site state lambda_1, lambda_2 [Np x P]:
 *         lambda_1 <- (1 - lr) lambda_1 + lr (g0 - 2 g1 mean),
 *         lambda_2 <- -2 min((1 - lr)(-lambda_2 / 2) + lr g1, -1e-8)       (so lambda_2 >= 2e-8).
 *     Rows >= N are not touched.  ve_partial / nonpos_partial [Np / 128] as tsvgp_lik_map_*.  var may be NULL with
 *     lik = TSVGP_LIK_GAUSSIAN (neither update reads it): ve_partial is then NaN and nonpos_partial counts rows with a
 *     non-finite mean or gradient.  0 <= lr <= 1.  The fp32 entry reads fp32 mean / var / Y, keeps the state in fp64 and also
 *     writes fp32 copies of the new lambda_1, lambda_2 [Np x P] (the weights tsvgp_site_accum_f32 reads on the next step). */
int tsvgp_diag_site_step_f64(const double *mean, const double *var, const double *Y, int lik, double lik_param, double lr,
                             double *lambda_1, double *lambda_2, double *ve_partial, int32_t *nonpos_partial, int64_t N, int64_t Np,
                             int P, void *stream);
int tsvgp_diag_site_step_f32(const float *mean, const float *var, const float *Y, int lik, double lik_param, double lr,
                             double *lambda_1, double *lambda_2, float *lambda_1_f32, float *lambda_2_f32, double *ve_partial,
                             int32_t *nonpos_partial, int64_t N, int64_t Np, int P, void *stream);

/* The normal generator of the Monte Carlo likelihoods: Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11) and Box-Muller.
 * The draw for (seed, draw, global row n, sample s, class c) is a pure function of those five integers -- not of the launch
 * geometry, the array type or the rank that computes it:
 *   key     = (seed & 0xffffffff, seed >> 32)                       seed, n taken as unsigned 64-bit, draw modulo 2^32
 *   counter = (n & 0xffffffff, n >> 32, s * 8 + (c >> 2), draw)     (0 <= c < 32, 0 <= s < TSVGP_MC_MAX_SAMPLES)
 *   (x0, x1, x2, x3) = Philox4x32-10(counter, key): ten rounds of
 *        (c0, c1, c2, c3) <- (hi(0xCD9E8D57 * c2) ^ c1 ^ k0, lo(0xCD9E8D57 * c2), hi(0xD2511F53 * c0) ^ c3 ^ k1, lo(0xD2511F53 * c0)),
 *        the key stepping by (0x9E3779B9, 0xBB67AE85) after each round
 *   u(x) = (x + 0.5) * 2^-32   (exact in fp64, inside (0, 1))
 *   class 4 (c >> 2) + 0 = sqrt(-2 ln u(x0)) * cos(2 pi u(x1)),   + 1 = sqrt(-2 ln u(x0)) * sin(2 pi u(x1)),
 *   class 4 (c >> 2) + 2 = sqrt(-2 ln u(x2)) * cos(2 pi u(x3)),   + 3 = sqrt(-2 ln u(x2)) * sin(2 pi u(x3))
 * with 2 pi = 6.283185307179586 and every operation an fp64 operation in the order written (2 pi * u is one rounded product).
 * Both array types compute the draws in fp64; the _f32 entry points round the finished draw.
 *
 * (4c) tsvgp_mc_normals_*: out [S x N x C] (GPflow's epsilon layout), out[s, n, c] = the draw of (seed, draw, row_offset + n, s, c).
 *      1 <= C <= TSVGP_MAX_BATCH, 1 <= S <= TSVGP_MC_MAX_SAMPLES, row_offset >= 0, S * N * ceil(C / 4) <= (2^31 - 1) * 256. */
#define TSVGP_MC_MAX_SAMPLES (1 << 28)
int tsvgp_mc_normals_f64(double *out, int64_t seed, int64_t draw, int64_t row_offset, int64_t S, int64_t N, int C, void *stream);
int tsvgp_mc_normals_f32(float *out, int64_t seed, int64_t draw, int64_t row_offset, int64_t S, int64_t N, int C, void *stream);

/* (4d) The Softmax likelihood map (gpflow.likelihoods.Softmax(C), GPflow 2.2.1 [ext]; reference docs/notebooks/mnist.py): the
 *      Monte Carlo estimate over S draws eps^s [N x C] of log p(y | f) = f_y - logsumexp_c f_c at f^s = mean + sqrt(var) eps^s, and
 *      its derivative through the reparameterisation (reference src/models/tsvgp.py:256-263): with p^s = softmax(f^s),
 *      d_c^s = [c == y] - p_c^s:  ve = 1/S sum_s log p(y | f^s),  g0_c = 1/S sum_s d_c^s,
 *      g1_c = 1/S sum_s d_c^s eps_c^s / (2 sqrt(var_c)) (cropped at -1e-8 unless TSVGP_LIK_NOCROP; a NaN stays NaN
 *      under the crop, as under np.minimum: a row with a negative variance has NaN g0 and g1 and is counted in nonpos_partial).
 *      mean, var [N x C]; Y [N x 1] class labels 0 .. C-1 in the array type (never used as an address; a label that is not an
 *      integer in [0, C) makes its row's ve, g0, g1 NaN); flags = TSVGP_LIK_SOFTMAX, optionally | TSVGP_LIK_NOCROP;
 *      2 <= C <= TSVGP_MAX_BATCH; 1 <= S <= TSVGP_MC_MAX_SAMPLES; rng_state: DEVICE int64 [seed, draw], read by the kernel (a
 *      captured graph replays with whatever the words hold then; the caller advances draw with an in-stream add);
 *      row_offset: global number of row 0 (a row shard's first row); epsilon: NULL, or [S x N x C] draws that replace the
 *      generator (GPflow's epsilon= hook; rng_state may then be NULL).  Outputs as tsvgp_lik_map_hetero_*: g0, g1 [Np x C] (rows
 *      >= N zero), ve_partial, nonpos_partial [Np / 128].  Sums in fp64 for either array type, max-shifted logsumexp. */
int tsvgp_lik_map_softmax_f64(const double *mean, const double *var, const double *Y, int flags, int C, int S,
                              const int64_t *rng_state, int64_t row_offset, const double *epsilon, double *g0, double *g1,
                              double *ve_partial, int32_t *nonpos_partial, int64_t N, int64_t Np, void *stream);
int tsvgp_lik_map_softmax_f32(const float *mean, const float *var, const float *Y, int flags, int C, int S,
                              const int64_t *rng_state, int64_t row_offset, const float *epsilon, float *g0, float *g1,
                              double *ve_partial, int32_t *nonpos_partial, int64_t N, int64_t Np, void *stream);

/* (3b) The moments for P latents with one kernel each: latent p has its own operand A + p*strideA ([Np x Mp] each; strideA = 0
 *     is the shared operand of tsvgp_moments_*) and its own prior variance kdiag_host[p] (HOST array of P doubles, passed
 *     as kernel arguments).  1 <= P <= TSVGP_MAX_BATCH.  Everything else as tsvgp_moments_*; one launch, each workgroup
 *     takes its 128-row panel through the P latents in turn. */
int tsvgp_moments_batched_f64(const double *A, int64_t strideA, const double *Tm, const double *gamma, const double *Y,
                              const double *kdiag_host, int lik, double lik_param, double *mean, double *var, double *g0,
                              double *g1, double *ve_partial, int32_t *nonpos_partial, int64_t N, int64_t Np, int Mp,
                              int P, int mode, void *stream);
int tsvgp_moments_batched_f32(const float *A, int64_t strideA, const float *Tm, const float *gamma, const float *Y,
                              const double *kdiag_host, int lik, double lik_param, float *mean, float *var, float *g0,
                              float *g1, double *ve_partial, int32_t *nonpos_partial, int64_t N, int64_t Np, int Mp,
                              int P, int mode, void *stream);

/* (5) Site accumulation (the two einsums of reference src/models/tsvgp.py:278-281 in whitened coordinates):
 *        acc2[p][i][j] = sum_n g1[n,p] * B[n,i] * B[n,j]        (full symmetric [P x Mp x Mp], fp64)
 *        acc1[p][i]    = sum_n g0[n,p] * B[n,i]                 ([P x Mp], fp64)
 *     B [Np x Mp]; g0,g1 contiguous [Np x P] with rows >= N equal to 0.  B, g0, g1 and work on 16-byte boundaries (operand
 *     rows and the 16 P weights of a chunk travel as 16-byte LDS-DMA pieces; TSVGP_EINVAL otherwise).
 *     The N range is cut into `nsplit` slices; partial tiles go to `work` and are summed in a fixed order (bitwise
 *     reproducible; no atomics); on a diagonal tile the row-block operands are the column-block fragments already in registers
 *     (one LDS read per fragment and k-step).  work must hold tsvgp_site_accum_work_bytes_*(Mp, P, nsplit) bytes.  Any nsplit >= 1 is
 *     valid (a slice is a whole number of chunks -- 16 rows in fp64, 32 in fp32 with P <= 8 -- so a count above Np / chunk
 *     leaves workgroups with empty slices: correct, wasted); the launch runs in rounds of tsvgp_site_accum_slots_*() equal workgroups (per latent: n_off * nsplit off-diagonal
 *     + nt * ceil(20 nsplit / 32) diagonal ones, 22 / 32 in fp32), so a count that fills whole rounds is the fast one
 *     (N = 1e6, M = 1024, fp64: 62 slices = 2048 workgroups = 8 rounds of 256; the Python mirror's EStepEngine.choose_nsplit). */
int64_t tsvgp_site_accum_work_bytes_f64(int Mp, int P, int nsplit);
int64_t tsvgp_site_accum_work_bytes_f32(int Mp, int P, int nsplit);
int tsvgp_site_accum_f64(const double *B, const double *g0, const double *g1, double *acc2, double *acc1, void *work,
                         int64_t Np, int Mp, int P, int nsplit, void *stream);
int tsvgp_site_accum_f32(const float *B, const float *g0, const float *g1, double *acc2, double *acc1, void *work,
                         int64_t Np, int Mp, int P, int nsplit, void *stream);
/* (5b) The same sums with one operand per latent (the rank-3 A of reference src/models/tsvgp.py:271-281): latent p reads
 *     B + p*strideB ([Np x Mp] each; strideB = 0 is tsvgp_site_accum_*).  One launch over all P latents. */
int tsvgp_site_accum_batched_f64(const double *B, int64_t strideB, const double *g0, const double *g1, double *acc2,
                                 double *acc1, void *work, int64_t Np, int Mp, int P, int nsplit, void *stream);
int tsvgp_site_accum_batched_f32(const float *B, int64_t strideB, const float *g0, const float *g1, double *acc2,
                                 double *acc1, void *work, int64_t Np, int Mp, int P, int nsplit, void *stream);
/* (5c) The constant-weight form of (5) and (5b): g1[n, p] = g1_const[p] on every row n < N (a homoskedastic Gaussian
 *     likelihood: -1 / (2 s2)).  g1_const: P doubles in DEVICE memory (8-byte boundary), in both precisions.  The kernels sum
 *     B[n,i] * B[n,j] unweighted -- no weight is moved, read back or multiplied into the operand -- and the reduction multiplies
 *     each summed element of acc2 by g1_const[p] once, in fp64, before it writes it and its mirror image:
 *        acc2[p][i][j] = g1_const[p] * sum_n B[n,i] * B[n,j]
 *     so the rows >= N of B must be zero (they are: the producers zero-fill the padding) and no weight array marks them.
 *     acc1, g0, work, nsplit, the slices and the fixed summation order are those of (5): acc1 is bit-identical to (5)'s, acc2
 *     equals (5)'s with g1 = g1_const on every row up to the rounding of the products (bit for bit when they are exact).
 *     1 <= P <= 8 (the hand-laid kernels; TSVGP_EINVAL above: callers with more latents use the general form). */
int tsvgp_site_accum_cw_f64(const double *B, const double *g0, const double *g1_const, double *acc2, double *acc1, void *work,
                            int64_t Np, int Mp, int P, int nsplit, void *stream);
int tsvgp_site_accum_cw_f32(const float *B, const float *g0, const double *g1_const, double *acc2, double *acc1, void *work,
                            int64_t Np, int Mp, int P, int nsplit, void *stream);
int tsvgp_site_accum_cw_batched_f64(const double *B, int64_t strideB, const double *g0, const double *g1_const, double *acc2,
                                    double *acc1, void *work, int64_t Np, int Mp, int P, int nsplit, void *stream);
int tsvgp_site_accum_cw_batched_f32(const float *B, int64_t strideB, const float *g0, const double *g1_const, double *acc2,
                                    double *acc1, void *work, int64_t Np, int Mp, int P, int nsplit, void *stream);

/* (6) Batched lower Cholesky of the M x M site matrices, in place:  A[b] = L[b] L[b]^T, L written to the lower triangle
 *     of the 128x128 diagonal blocks and below (the strictly upper part of the diagonal blocks is zeroed; blocks above
 *     the diagonal are left untouched).  Replaces tf.linalg.cholesky of reference src/models/tsvgp.py:270,300 and
 *     src/util.py:377-388.  M must be a multiple of 128 (pad with an identity block), lda >= M and even, A on a 16-byte
 *     boundary (16-byte row accesses), matrix b starts at A + b*stride; with batch > 1 stride even and >= M * lda (the
 *     matrices are factored side by side and must not overlap; batch == 1 does not read stride).  Anything else is
 *     TSVGP_EINVAL before any launch.  info[b] = 0, or the 1-based index of the first non-positive pivot (LAPACK potrf
 *     convention; a NaN pivot counts as non-positive).  work: batch * 128 * 128 doubles, on a 16-byte boundary like A. */
#define TSVGP_POTRF_SUBST 1 /* flags: solve the panels below each diagonal block by substitution against L_kk (16-wide
                               sub-blocks by forward substitution, the rest by MFMA updates, as LAPACK's blocked trsm)
                               instead of multiplying by inv(L_kk): ~0.15 ms slower at M = 1024, but as robust as a
                               LAPACK factorisation on numerically barely definite matrices (cond ~ 1e14), where the
                               inverse-based panels lose cond(L_kk) digits of the trailing matrix.  The callers set it
                               when cond(K_uu + jitter I) is beyond 1e7. */
#define TSVGP_POTRF_DIAG_V1 4 /* flags: round 4's block step -- the diagonal block's inverse assembled by the 2 x 2 recursion and
                                 the panel rows multiplied by it -- instead of round 5's (inverted 16 x 16 diagonal tiles only,
                                 panel rows by substitution on MFMA tile registers, tsvgp_chol.hip); for A/B measurements */
#define TSVGP_POTRF_FUSE 16 /* flags: the diagonal block and the panel rows below it in ONE launch (every panel workgroup factors
                               the diagonal block for itself); experimental: measured slower than the two launches it replaces */
int tsvgp_potrf_f64(double *A, int M, int lda, int batch, int64_t stride, int32_t *info, double *work, int flags,
                    void *stream);

/* (6a) Factor AND solve in one pass: the buffer of matrix b holds, directly below its M rows, `rhs_rows` further rows B
 *     [rhs_rows x M] (same lda, even; A on a 16-byte boundary; stride >= (M + rhs_rows) * lda for every batch, and even with
 *     batch > 1; TSVGP_EINVAL otherwise, before any launch).  They ride through the factorisation as panel rows -- every
 *     block step solves them against the diagonal block and applies the trailing update to them with the same tile kernels --
 *     and come out as  B L^-T  (= (L^-1 B^T)^T: the triangular solve of reference src/util.py:173, D = chol(W)^-1 L^T, without
 *     the inverse factor of (6b), its recursion levels and the GEMM that applied it).  rhs_rows a multiple of 128.
 *     TSVGP_POTRF_RHS_UPPER: B is block upper triangular (row block i zero in the column blocks < i), as J L J of a lower
 *     triangular L is -- the zero blocks are skipped.  work, info, TSVGP_POTRF_SUBST as in (6). */
#define TSVGP_POTRF_RHS_UPPER 2
int tsvgp_potrf_solve_f64(double *A, int M, int lda, int batch, int64_t stride, int32_t *info, double *work, int rhs_rows,
                          int flags, void *stream);
/*     dst[b][i][j] = i <= j ? src[b][M-1-j][M-1-i] : 0  on the leading M x M block: transpose + index reversal + upper triangle
 *     in one pass -- what turns the solved rows (J L J) C^-T of (6a) into the upper triangular D = U_W^-1 L^T. */
int tsvgp_flip_transpose_f64(const double *src, int lds, int64_t sstride, double *dst, int ldd, int64_t dstride, int M, int batch,
                             void *stream);

/* (6v) t_VGP, the exact N x N model (reference src/models/tvgp.py:72-160), around (6a).  With s = sqrt|lambda_2| (s_n = 0 for
 *     n >= N), y~ = lambda_1 / lambda_2, K~ = variance * k_kind(X, X) + jitter I (r as tsvgp_kernel_fill_*, same device functions,
 *     D <= 32) the model factors B = I + s s^T * K~ = L L^T (eigenvalues >= 1: the plain factorisation) and needs
 *     C = (K~ s) L^-T and z = L^-1 (s y~).  tsvgp_vgp_system_f64 writes, in one launch, the stacked operand of (6a),
 *     S [(2 Np + 128) x lds] with Np = N rounded up to 128, lds >= Np and even, S on a 16-byte boundary:
 *        rows [0, Np)         B[i, j] = [i == j] + s_i s_j K~[i, j]: the lower block triangle of 128 x 128 tiles, diagonal tiles in
 *                             full (what (6) reads; the blocks above the diagonal are NOT written); the padding is the identity block
 *        rows [Np, 2 Np)      R[n, j] = K~[n, j] s_j, zero for n >= N or j >= N
 *        rows [2 Np, + 128)   row 0: s_j y~_j (0 for j >= N); the other 127 rows zero
 *     (columns >= Np of a wider buffer are not touched).  One workgroup per tile of the lower block triangle; the kernel function
 *     is evaluated once per pair.  TSVGP_VGP_NO_ROWS: rows [0, Np) only (S may then end there) -- for a caller that brings its
 *     own right-hand sides (predict_f: K(Xnew, X) s by tsvgp_kernel_fill_f64).  After
 *     tsvgp_potrf_solve_f64(S, Np, lds, 1, (2 Np + 128) lds, info, work, Np + 128, 0, stream) rows [Np, 2 Np) hold C and row 2 Np
 *     holds z.  lambda_1, lambda_2: [>= N] fp64 (DiagSites' padded state). */
#define TSVGP_VGP_NO_ROWS 1
int tsvgp_vgp_system_f64(int kind, const double *X, const double *inv_ls, double variance, double jitter, const double *lambda_1,
                         const double *lambda_2, double *S, int64_t N, int64_t Np, int D, int64_t lds, int flags, void *stream);
/*     The sweep over the solved rows (reference src/models/tvgp.py:90-96, :104-107, :146-157), HBM bound: for n < N
 *        q = sum_{i < K} C[n, i]^2,   mean = sum_{i < K} C[n, i] z[i]  (z == NULL: 0),   var = kdiag - q
 *     C [Np x ldc] (all Np rows are read), K even and <= ldc, ldc even, C and z on 16-byte boundaries.  lik = TSVGP_LIK_NONE: mean
 *     and / or var [N] are written, nothing else is read (predict_f's variance: C = K(Xnew, X) s L^-T, z NULL).  lik =
 *     TSVGP_LIK_GAUSSIAN (lik_param = noise variance) or TSVGP_LIK_BERNOULLI: g0, g1, ve of tsvgp_lik_map_* at (mean, var, Y[n]),
 *     never cropped (the reference has no crop here); ve and E_q log t = -1/2 lambda_2 ((y~ - mean)^2 + var) of the sites found on
 *     entry are summed into ve_partial / eqt_partial [Np / 128] (fp64, one per 128 rows); then, when beta != 0, in place
 *        lambda_1 <- (1 - beta) lambda_1 + beta (g0 - 2 g1 mean),     lambda_2 <- (1 - beta) lambda_2 - 2 beta g1
 *     (beta == 0 stores nothing: the sites stay bit for bit; 0 <= beta <= 1; z, Y, lambda_1, lambda_2 and both partials required;
 *     mean, var may be NULL).  nonpos_partial [Np / 128]: rows with var <= 0 or a non-finite mean, g0 or g1.  No atomics, a
 *     summation order fixed by the shape, 16-byte loads. */
int tsvgp_vgp_rows_f64(const double *C, int64_t ldc, const double *z, const double *Y, double *lambda_1, double *lambda_2,
                       double kdiag, int lik, double lik_param, double beta, double *mean, double *var, double *ve_partial,
                       double *eqt_partial, int32_t *nonpos_partial, int64_t N, int64_t Np, int K, void *stream);

/* (6w) The hyperparameter gradient of t_VGP: the contraction of a symmetric N x N weight matrix with d K(X, X) / d theta, formed
 *     pair by pair (no N x N x D array).  With G[i, j] = W[i, j] + 1/2 (a_i c_j + c_i a_j), x~ = X * inv_ls, s_ij = |x~_i - x~_j|^2
 *     and K = variance * f(s) (f, f' as tsvgp_kernel_fill_* / tsvgp_kernel_grad_*; kind, D <= 32 as (6v)):
 *        column 0       sum_ij G[i, j] f(s_ij)                                           = d / d variance  (dK / d variance = f)
 *        column 1 + d   sum_ij G[i, j] variance f'(s_ij) (-2) (x~_id - x~_jd)^2          = l_d * d / d lengthscale_d
 *     over all i, j < N -- so the caller divides column 1 + d by lengthscale_d (and adds the columns for one shared lengthscale).
 *     W [Np x ldw], ldw >= Np and even, on a 16-byte boundary, symmetric: only the lower block triangle of 128 x 128 tiles is read,
 *     diagonal tiles in full (the convention tsvgp_vgp_system_f64 writes); a tile below the diagonal counts twice.  Rows and
 *     columns >= N contribute nothing whatever W holds there (NaN included); X [N x D], a, c [>= N] are not read beyond N.
 *     part [tsvgp_vgp_kernel_grad_parts(Np, D)] doubles = (ntiles + 1) rows of 1 + Dp, ntiles = nt (nt + 1) / 2, nt = Np / 128,
 *     Dp = D rounded up to 1, 2, 4, 8, 16 or 32: row k < ntiles the weighted sums of tile k (row-major over the lower block
 *     triangle), row ntiles their totals, added by a second small kernel in an order fixed by ntiles.  No atomics: two calls
 *     agree bit for bit.  One workgroup per tile, 16-byte row-contiguous loads of W; bound by the one read of W. */
int64_t tsvgp_vgp_kernel_grad_parts(int64_t Np, int D);
int tsvgp_vgp_kernel_grad_f64(int kind, const double *X, const double *inv_ls, double variance, const double *W, int64_t ldw,
                              const double *a, const double *c, int64_t N, int64_t Np, int D, double *part, void *stream);

/* (6b) The same factorisation plus the inverse factor: X[b] = inv(L[b]) (lower triangular, exact zeros above) and
 *     Xt[b] = X[b]^T, both [batch x M x M] row-major (leading dimension M).  The inverted diagonal blocks the panel
 *     solve needs anyway are combined by the 2x2 block recursion inv([[A,0],[C,B]]) = [[A^-1,0],[-B^-1 C A^-1, B^-1]]
 *     as MFMA tile products.  Replaces tf.linalg.triangular_solve / cholesky_solve with M x M right-hand sides
 *     (reference src/util.py:168-175, src/models/tsvgp.py:270-271): the callers apply X by GEMM.
 *     T: scratch, batch * M * M doubles.  X, Xt and T on 16-byte boundaries.  Other arguments as tsvgp_potrf_f64: lda even, A on a
 *     16-byte boundary, with batch > 1 stride even and >= M * lda; TSVGP_EINVAL otherwise, before any launch. */
int tsvgp_potrf_inv_f64(double *A, int M, int lda, int batch, int64_t stride, int32_t *info, double *work, double *X,
                        double *Xt, double *T, int flags, void *stream);

/* (7) Triangle extraction for the factors above, fused with a scale and (optionally) the index reversal of the upper-form
 *     factorisation A = U U^T (U = J C J with C the lower factor of J A J, J the exchange matrix):
 *        dst[b][i][j] = keep ? scale * src[b][si][sj] : 0   on the leading M x M block,
 *        flip = 0: (si, sj) = (i, j), keep = i >= j;   flip = 1: (si, sj) = (M-1-i, M-1-j), keep = i <= j;
 *        flip = 2: (si, sj) = (M-1-i, M-1-j), keep everything (J A J, the input of the upper-form factorisation).
 *     Replaces tf.linalg.band_part / the triangular() transform of reference src/sites.py:63 and the leading minus of
 *     src/models/tsvgp.py:300 (scale = -1) in one pass.  src [batch x * x lds], dst [batch x * x ldd] (strides in elements). */
int tsvgp_tri_copy_f64(const double *src, int lds, int64_t sstride, double *dst, int ldd, int64_t dstride, int M, int batch,
                       double scale, int flip, void *stream);
/* (7') The same pass with a shift of the diagonal, dst[b][i][i] += diag_add (after the scale), and flip = 3: (si, sj) = (i, j), keep
 *     everything -- K_uu + jitter I (reference src/models/tsvgp.py:209-211, :270) and I + L^T K L (src/util.py:171-172) written where
 *     the factorisation reads them, instead of a copy, an addition on the diagonal and a triangle pass each. */
int tsvgp_tri_copy_shift_f64(const double *src, int lds, int64_t sstride, double *dst, int ldd, int64_t dstride, int M, int batch,
                             double scale, double diag_add, int flip, void *stream);

/* (7b) The matrix of the final factorisation of one E-step (reference src/models/tsvgp.py:286-300), in one pass:
 *        G1s    = (G1 + G1^T) / 2
 *        target = c_ll * LLt + c_g * s * G1s + jitter * I,     s = num_data / rows[0]  (1 when num_data <= 0)
 *     with LLt = L L^T of the old site factor, c_ll = 1 - lr, c_g = -2 lr:  -2 [(1-lr) lambda_2 + lr s G1] + jitter I.
 *     `rows` is a device scalar (the all-reduced row count of the step), so the minibatch scale of :286-291 needs no host
 *     read.  All matrices [P x M x M] contiguous. */
int tsvgp_site_target_f64(const double *G1, const double *LLt, double *target, double *G1s, int M, int P, double c_ll,
                          double c_g, double jitter, const double *rows, double num_data, void *stream);

/* (7b') The elementwise part of the site update in one call (reference src/util.py:429-438, src/models/tsvgp.py:284-300):
 *        Gs     = (G1 + G1^T) / 2
 *        target = (1 - lr) LLt - 2 lr s Gs + jitter I                      (what (7b) writes)
 *        l1_new = (1 - lr) l1_old + lr s (G0 - 2 Gs meanZ)                  (the chain rule of util.py:436 and the update of :296)
 *     G1, LLt, target [P x M x M]; G0, meanZ, l1_old, l1_new [M x P]; all contiguous; s and `rows` as in (7b);
 *     work: P * ceil(M / 32) * M doubles (per-tile partial row sums, added in a fixed order).  Replaces (7b), a matrix-vector
 *     product and about ten elementwise launches on the replicated critical path of a step (two launches). */
int tsvgp_site_update_f64(const double *G1, const double *G0, const double *LLt, const double *meanZ, const double *l1_old,
                          double *target, double *l1_new, double *work, int M, int P, double lr, double jitter, const double *rows,
                          double num_data, void *stream);

/* (7b'') beta = l1 - D^T (D v) per latent: D [P x M x M] upper triangular (only that triangle is read), v, l1, beta [M x P]
 *     contiguous; work: P * M * (1 + ceil(M / 64)) doubles.  With v = (K_uu + 1e-6 I) lambda_1 this is K^-1 m of reference
 *     src/util.py:176-179 -- the two triangular matrix-vector products between the factorisation and the moments kernel, three
 *     small launches, summation in a fixed order. */
int tsvgp_site_beta_f64(const double *D, const double *v, const double *l1, double *work, double *beta, int M, int P,
                        void *stream);

/* (7b''') y[:, p] = A_p v[:, p]: row-major A_p [M x M] at A + p * strideA (strideA = 0: one matrix for every latent), v and y
 *     [M x P] contiguous.  The matrix-vector products of the replicated chain -- (K_uu + 1e-6 I) lambda_1 and K_uu beta of
 *     reference src/util.py:176-179 / src/models/tsvgp.py:249-254, K9^-1 acc1 of :279 -- one wave per row. */
int tsvgp_gemv_f64(const double *A, int64_t strideA, const double *v, double *y, int M, int P, void *stream);

/* (7c) Status word of one step: flags[0] = sum |info_a| (prelude factorisations), flags[1] = nonpos[0] (count of
 *     non-positive predictive variances, the assert_positive of :113; NULL = 0), flags[2] = sum |info_b| (the final
 *     factorisation, :300).  One device->host read of these three doubles ends a step. */
int tsvgp_step_status_f64(const int32_t *info_a, int na, const int32_t *info_b, int nb, const double *nonpos, double *flags,
                          void *stream);

/* (7d) Lower triangle of P symmetric M x M accumulators <-> packed [P x M (M + 1) / 2] (row by row): the payload of the
 *     all-reduce of the dual accumulators (half of P M^2).  Unpack writes both triangles. */
int tsvgp_sym_pack_f64(const double *A, int lda, int64_t stride, int M, int P, double *packed, void *stream);
int tsvgp_sym_unpack_f64(const double *packed, double *A, int lda, int64_t stride, int M, int P, void *stream);

/* (8) Kernel-parameter gradient contraction for the M-step (d ELBO / d theta with the sites fixed: reference
 *     experiments/uci_regression.py:159-160, pinned by tests/models/test_tsvgp.py:168-188; TensorFlow autodiff there).
 *     For one latent GP, with V[n,m] = g0[n] beta[m] - 2 g1[n] U[n,m] (U = K_fu Q from tsvgp_trmm, Q = D^T D):
 *        sum_{n,m} V[n,m] * dK[n,m]/d variance,   /d lengthscale_d,   and per m  sum_n V[n,m] * dK[n,m]/d Z[m,d].
 *     X [N x D], Z [M x D], U [N x ldu]; g0, g1 with element stride gstride (so a column of an [N x P] array can be
 *     passed), beta with stride bstride.  Outputs are per-block partial sums to be added by the caller:
 *        zpart [nrb x Mp x Dp], lpart [nrb x ncb x Dp], vpart [nrb x ncb],   nrb = ceil(N / tsvgp_kernel_grad_rows()),
 *        ncb = ceil(Mp / 512), Mp = M rounded up to 128, Dp = tsvgp_kernel_grad_dpad(D)  (D <= 16). */
int tsvgp_kernel_grad_rows(void);
int tsvgp_kernel_grad_dpad(int D);
int tsvgp_kernel_grad_f64(int kind, const double *X, const double *Z, const double *inv_ls, double variance,
                          const double *U, int64_t ldu, const double *g0, const double *g1, int gstride,
                          const double *beta, int bstride, int64_t N, int M, int D, double *zpart, double *lpart,
                          double *vpart, void *stream);
int tsvgp_kernel_grad_f32(int kind, const float *X, const float *Z, const float *inv_ls, float variance, const float *U,
                          int64_t ldu, const float *g0, const float *g1, int gstride, const float *beta, int bstride,
                          int64_t N, int M, int D, double *zpart, double *lpart, double *vpart, void *stream);

/* (8p) The contraction of (8) for a PRODUCT of C stationary kernels (1p), all C parameter sets in ONE pass over U.  With
 *     K = variance * prod_c f_c(s_c), s_c = sum_d s_cd^2, s_cd = (x_nd - z_md) * inv_ls[c*D + d], V as in (8) and
 *     P_c = prod_{c' != c} f_c'(s_c') (running prefix and suffix products, never a division by f_c):
 *        vpart  sums V * prod_c f_c              (the caller: d / d variance_c = (variance / variance_c) * sum)
 *        w_c  = -2 * variance * V * P_c * f_c'(s_c)
 *        d lengthscale[c, d] = sum_{n,m} w_c s_cd^2 inv_ls[c, d],        dZ[m, d] = sum_n sum_c w_c s_cd inv_ls[c, d].
 *     kinds_host [C] is a HOST array, inv_ls [C x D] a device array, variance the product of the components' variances.  Operands,
 *     strides and the per-block partials as (8), with lpart [nrb x ncb x C x Dp] (component-major inside a block); fp64
 *     accumulation, no atomics, bitwise reproducible.  D <= 16, 1 <= C <= TSVGP_MAX_COMPONENTS, ldu even and >= Mp, U on a boundary
 *     of two elements; TSVGP_EINVAL before any launch otherwise (the reserved kind 1 included).  The kernel stages X and keeps its Z
 *     columns unscaled and scales the difference per component, so its registers do not grow with C beyond the C x Dp sums. */
int tsvgp_kernel_grad_prod_f64(const int *kinds_host, const double *X, const double *Z, const double *inv_ls, double variance,
                               const double *U, int64_t ldu, const double *g0, const double *g1, int gstride,
                               const double *beta, int bstride, int64_t N, int M, int D, int C, double *zpart, double *lpart,
                               double *vpart, void *stream);
int tsvgp_kernel_grad_prod_f32(const int *kinds_host, const float *X, const float *Z, const float *inv_ls, float variance,
                               const float *U, int64_t ldu, const float *g0, const float *g1, int gstride, const float *beta,
                               int bstride, int64_t N, int M, int D, int C, double *zpart, double *lpart, double *vpart,
                               void *stream);

/* (9) Greedy conditional-variance selection of inducing points (Burt, Rasmussen, van der Wilk 2020, "ConditionalVariance"; [ext]:
 *     nothing in the reference chooses Z): pivoted Cholesky of K(X, X) that always takes the row with the largest residual prior
 *     variance.  With k = variance * f_kind(r) exactly as tsvgp_kernel_fill_* (same device functions, D <= 32), d[n] = variance:
 *        for j in 0 .. M-1:
 *            p = the lowest n with d[n] == max(d);   stop unless d[p] > floor      (count = j)
 *            c = (k(X, x_p) - sum_{i<j} C[i, :] * C[i, p]) / sqrt(d[p])
 *            C[j, :] = c;   d = max(d - c * c, 0);   d[p] = 0;   indices[j] = p;   pivots[j] = d[p] as found
 *     X [N x D] row-major, inv_ls [D].  C [M x ldc]: the factor TRANSPOSED (row j = the j-th Cholesky column over n), ldc >= Np = N
 *     rounded up to 128 and even; columns n in [N, Np) are written as 0, columns >= Np are not touched, rows >= count neither.
 *     d [Np]: on return the residual conditional variance diag(K_ff - K_fS K_SS^-1 K_Sf) for n < N (exactly 0 at every picked
 *     row), 0 beyond.  indices, pivots [M]: entries [0, count) are written.  count: one device int.  C and d on 16-byte
 *     boundaries; work: tsvgp_greedy_select_work_bytes(N, M) bytes on an 8-byte boundary (-1: N < 1, M < 1 or N beyond 128 * (2^31 - 1)).
 *     N >= 1, M >= 1 (M > N is allowed: the selection stops at count <= N), variance > 0, floor finite and >= 0 -- the caller
 *     passes max(threshold, 1e-12 * variance): below that a residual is rounding noise of the subtraction, and a duplicate row
 *     must not be taken with a pivot of 1e-17.
 *     The call enqueues 2 M launches on `stream` (one grid over n that extends the factor, one workgroup that reduces the
 *     per-workgroup maxima and gathers the next pivot's factor entries) and reads nothing back: the steps behind the stop
 *     condition return at once on a device flag.  No workgroup waits for another.  HBM bound on the read of the rows of C
 *     built so far, 8 Np count^2 / 2 bytes in all.  The dot product's summation order depends on j alone: two calls agree bit for
 *     bit, and identical rows of X get identical columns of C. */
int64_t tsvgp_greedy_select_work_bytes(int64_t N, int M);
int tsvgp_greedy_select_f64(int kind, const double *X, const double *inv_ls, double variance, double floor, double *C, int64_t ldc,
                            double *d, int64_t *indices, double *pivots, int32_t *count, void *work, int64_t N, int M, int D,
                            void *stream);

/* (10) Pathwise function draws (Matheron's rule; Wilson, Borovitskiy, Terenin, Mostowsky, Deisenroth 2020 [ext]: nothing in the
 *     reference draws functions): S sample paths of one latent GP evaluated at N points without any N-sized matrix,
 *        out[s, n] = sum_{l < L} ( W[s, l] cos(Omega_l . x~_n) + W[s, L + l] sin(Omega_l . x~_n) )
 *                  + sum_{m < M} V[s, m] * variance * k_kind(r(x_n, z_m)),        x~ = x * inv_ls,
 *     the first sum a random-feature draw of the prior (the caller scales W by sqrt(variance / L)), the second the update that
 *     carries it through the inducing values (V = K6^-1 (u - g(Z))); r and k as tsvgp_kernel_fill_* (same device functions, the
 *     difference form on the scaled inputs).  X [N x D], Z [M x D], inv_ls [D], Omega [L x D] (unitless frequencies), W [S x 2 L],
 *     V [S x M], all row-major and contiguous; out [S x ldo], ldo >= N, columns >= N are not written.  M = 0 with V (and Z) NULL
 *     gives the prior part alone.  1 <= D <= 32, 1 <= S <= TSVGP_PATHWISE_MAX_S (the caller loops over chunks of samples: a row's
 *     S sums live in registers), N >= 1 and at most 256 * (2^31 - 1), L >= 1, M >= 0, variance finite and > 0; TSVGP_EINVAL
 *     otherwise, before any launch.  One thread per row; the sine / cosine pair and the kernel value are taken once per (n, l) and
 *     (n, m) and serve all S samples; Omega, W, Z~ and V go through LDS in chunks of 64.  A row's values depend on that row and the
 *     operands alone -- not on N, on the other rows or on the launch geometry: the same x gives the same bits in any call.
 *     No atomics, a summation order fixed by (L, M). */
#define TSVGP_PATHWISE_MAX_S 16
int tsvgp_pathwise_f64(int kind, const double *X, const double *Z, const double *inv_ls, double variance, const double *Omega,
                       const double *W, const double *V, double *out, int64_t N, int M, int L, int D, int S, int64_t ldo,
                       void *stream);

/* (10b) The vector-Jacobian product of (10) with respect to the rows of X: with cotangents C [S x ldc] on out,
 *        dX[n, d] = sum_s C[s, n] * d out[s, n] / d x_nd
 *                 = inv_ls_d * (  sum_{l < L} Omega[l, d] * ( cos(a_nl) * (sum_s C[s, n] W[s, L + l]) - sin(a_nl) * (sum_s C[s, n] W[s, l]) )
 *                               + sum_{m < M} 2 (x~_nd - z~_md) * variance * k'_kind(s2_nm) * (sum_s C[s, n] V[s, m]) ),
 *        a_nl = Omega_l . x~_n,   x~ = x * inv_ls,   z~ = z * inv_ls,   s2_nm = |x~_n - z~_m|^2,
 *     k' the derivative of the profile with respect to s2, the device function of tsvgp_kernel_grad_* (the Matern kernels take
 *     r = sqrt(max(s2, 1e-36)): on an inducing point the factor x~ - z~ makes the term an exact zero, no special case).  X, Z,
 *     inv_ls, Omega, W, V exactly as in (10); C [S x ldc], ldc >= N, columns >= N are not read; dX [N x D] row-major and contiguous
 *     like X, rows >= N of a larger buffer are not written.  M = 0 with V (and Z) NULL differentiates the prior part alone.  The
 *     limits of (10) on N, M, L, D, S and variance; TSVGP_EINVAL otherwise, before any launch.  A full Jacobian [S, N, D] would
 *     need S D sums per row; the product with C needs D and shares the sine / cosine pair and the profile among the samples as
 *     (10) does.  One thread per row: x~, the row's S cotangents and its D sums stay in registers, the LDS stages are those of
 *     (10).  A row's dX depends on that row, its column of C and the operands alone -- not on N, on the other rows or on the launch
 *     geometry: the same row gets the same bits in any call.  No atomics, a summation order fixed by (L, M). */
int tsvgp_pathwise_vjp_f64(int kind, const double *X, const double *Z, const double *inv_ls, double variance, const double *Omega,
                           const double *W, const double *V, const double *C, int64_t ldc, double *dX, int64_t N, int M, int L,
                           int D, int S, void *stream);

/* (11) Input gradient of the marginal moments of one latent GP (predict_f under torch autograd; GPflow users get it from
 *     tf.GradientTape over predict_f [ext]).  With mean[n] = k_n^T beta, var[n] = variance - k_n^T Q k_n, k_n = K(Z, x_n), Q
 *     symmetric, cotangents cm, cv of (mean, var) and U = K(X, Z) Q (the caller's GEMM):
 *        dX[n, d] (+)= sum_{m < M} (cm[n] beta[m] - 2 cv[n] U[n, m]) * variance * f'(s_nm) * 2 s_d * inv_ls_d,
 *        s_d = (x_nd - z_md) * inv_ls_d,   s_nm = sum_d s_d^2,   K = variance * f(s),
 *     f' the device function of tsvgp_kernel_grad_* (the Matern profiles take r = sqrt(max(s, 1e-36)): on an inducing point the
 *     factor s_d makes the term an exact zero) -- the dZ term of (8) summed over m per row instead of over n per column.
 *     One latent per call.  X [N x D], Z [M x D], inv_ls [D] row-major and contiguous; U [N x ldu]; cm, cv with element stride
 *     cstride (a column of an [N x P] array), beta with stride bstride; dX [N x D] fp64, row-major and contiguous: accumulate = 0
 *     writes it, accumulate != 0 adds to what is there; rows >= N of a larger buffer are not written.  Columns >= M of U are
 *     not read, whatever they hold; X, cm, cv are not read beyond N.
 *     TSVGP_EINVAL before any launch: a NULL pointer; N <= 0; M <= 0; D < 1 or D > 32; a kind other than SE, Matern-3/2,
 *     Matern-5/2; cstride <= 0 or bstride <= 0; ldu < M; and what the 16-byte row loads of U need: U off a 16-byte boundary
 *     or ldu no multiple of 16 / sizeof(T) (2 doubles, 4 floats).
 *     One launch.  Lanes run along m, 16 bytes of a row of U each (a wave sweeps 128 columns in fp64, 256 in fp32), a workgroup
 *     takes tsvgp_moments_vjp_rows(D) rows; z~ and beta sit in LDS, tsvgp_moments_vjp_stage_*(D) columns at a time (-1 from
 *     either: D out of range): a wider M is walked in stages of that many columns inside the kernel, in column order, and dX
 *     receives the whole sum at the end -- accumulate != 0 gives old + sum, bit for bit what a write followed by an addition
 *     gives.  Arithmetic in T, accumulation in fp64, no atomics, every sum's order fixed by (M, D): dX[n] has the same bits
 *     whatever N is, wherever row n stands and whatever the other rows hold.  HBM traffic is one read of U, but the launch is bound by instruction issue, not by HBM:
 *     measured 4 (fp64, D = 8) and 8 (fp32, D = 16) times the time of that read at N = 1e6, M = 1024. */
int tsvgp_moments_vjp_rows(int D);
int tsvgp_moments_vjp_stage_f64(int D);
int tsvgp_moments_vjp_stage_f32(int D);
int tsvgp_moments_vjp_f64(int kind, const double *X, const double *Z, const double *inv_ls, double variance, const double *U,
                          int64_t ldu, const double *cm, const double *cv, int cstride, const double *beta, int bstride, int64_t N,
                          int M, int D, double *dX, int accumulate, void *stream);
int tsvgp_moments_vjp_f32(int kind, const float *X, const float *Z, const float *inv_ls, float variance, const float *U, int64_t ldu,
                          const float *cm, const float *cv, int cstride, const float *beta, int bstride, int64_t N, int M, int D,
                          double *dX, int accumulate, void *stream);

/* (12) Lloyd's k-means for inducing points (the reference's drivers name KMeans(n_clusters=M).fit(X).cluster_centers_ as the
 *     alternative to Z = X[:M]; [ext]: nothing in the reference runs it): the two N-sized steps of one iteration.  The scaled
 *     squared distance is the difference form of (9) in its operation order, with no contraction:
 *        s(x, c) = sum_{q = 0 .. D-1} dd_q^2,   a = x_q * inv_ls_q,  b = c_q * inv_ls_q,  dd = a - b,  s = fma(dd, dd, s).
 *     tsvgp_kmeans_assign_f64: labels[n] = the lowest m with s(x_n, c_m) minimal, dist[n] = that s, for n < N.  X [N x D],
 *     C [M x D] row-major and contiguous, inv_ls [D]; labels [N] int32, dist [N]; part [tsvgp_kmeans_assign_parts(N, D)]: one
 *     partial sum of dist per workgroup of tsvgp_kmeans_assign_rows(D) rows (the sum of the last workgroup runs over its rows
 *     < N), which the caller adds up for the inertia.  Nothing of size N * M is written or read.  A row's label and distance
 *     are a function of that row, C and inv_ls alone: the same bits for any N, any position of the row in X and any launch
 *     geometry, so a call on X + a * D with N = b - a gives the slice [a, b) of the full call.  Lanes run along rows, 2 or 4 rows
 *     per lane, the centres pass through LDS scaled, tsvgp_kmeans_assign_chunk() at a time, walked in index order with a strict
 *     comparison.  Compute bound: 3 N M D fp64 operations.  A NaN distance never wins; a row whose distances are all NaN gets
 *     label 0 and dist +inf.
 *     tsvgp_kmeans_update_f64: C_new[m] = the mean of the rows X[order[i]], i in [offsets[m], offsets[m + 1]), summed in fp64 in
 *     an order fixed by the segment's length (256 / DP interleaved slots, DP = D rounded up to a power of two, each added in
 *     increasing i, then a pairwise tree over the slots) and divided by the count; an empty segment copies C_old[m] bit for bit.
 *     order [N] int64 (the caller's stable sort of the labels), offsets [M + 1] int64 non-decreasing from 0 to N, C_old and
 *     C_new [M x D] (distinct buffers).  One workgroup per cluster: the bits of C_new[m] depend on that segment's rows and their
 *     order alone, not on M, on the other segments or on the grid.  No atomics.  A row number outside [0, N) is not
 *     dereferenced and a segment is clipped to [0, N).
 *     Both: N >= 1, M >= 1, 1 <= D <= 32, no NULL pointer, every buffer on the boundary of its element type (8 bytes; labels
 *     4); TSVGP_EINVAL otherwise, before any launch.  tsvgp_kmeans_assign_parts is -1 for N < 1, D out of range or N beyond
 *     rows * (2^31 - 1); tsvgp_kmeans_assign_rows is -1 for D out of range.  One launch each. */
int tsvgp_kmeans_assign_rows(int D);
int tsvgp_kmeans_assign_chunk(void);
int64_t tsvgp_kmeans_assign_parts(int64_t N, int D);
int tsvgp_kmeans_assign_f64(const double *X, const double *C, const double *inv_ls, int32_t *labels, double *dist, double *part,
                            int64_t N, int M, int D, void *stream);
int tsvgp_kmeans_update_f64(const double *X, const int64_t *order, const int64_t *offsets, const double *C_old, double *C_new,
                            int64_t N, int M, int D, void *stream);

/* (13) k-means++ seeding for (12) (Arthur, Vassilvitskii 2007, with scikit-learn's greedy local trials [ext]: the seeding behind
 *     the KMeans(n_clusters=M, random_state=0) the reference's drivers name): M rows of X, each drawn with probability
 *     proportional to its scaled squared distance s (12) to the nearest row already taken, the best of L draws kept.
 *        u(r, j) = ((x0 >> 5) * 2^26 + (x1 >> 6)) * 2^-53 in [0, 1), exact in fp64, with
 *                  (x0, x1, ., .) = Philox4x32-10(counter = (r, j, 0x6B2B2B, 0), key = (seed & 0xffffffff, seed >> 32))  (see (4a))
 *        round 0:  i_0 = min(floor(u(0, 0) * N), N - 1);   mind[n] = s(x_n, x_{i_0});   pot_0 = sum_n mind[n]
 *        round r = 1 .. M-1, for j < L:  t_j = u(r, j) * pot_{r-1};   cand_j = the lowest n whose running sum of mind through n
 *                  exceeds t_j (rows in increasing n);   newpot_j = sum_n min(mind[n], s(x_n, x_{cand_j}))
 *                  j* = the lowest j with newpot_j minimal;  i_r = cand_{j*};  mind[n] = min(mind[n], s(x_n, x_{i_r}));  pot_r = newpot_{j*}
 *     A row of zero mass (mind[n] == 0: a taken row or a duplicate of one) is never a candidate while any row has mass; a
 *     t_j at or above the top of the running sum takes the last row of positive mass; with no mass left (fewer than M
 *     distinct rows) nothing is divided, every candidate is N - 1, the rounds complete and pot_hist shows the zeros.
 *     Summation order (fixed by N, D, L alone -- no floating-point atomics, two calls agree bit for bit): the sums over n are
 *     taken per workgroup of tsvgp_kmeanspp_rows(D) consecutive rows in the tree of (12)'s partial inertia, then over the
 *     workgroups b (16 slots, slot k adds b = k, k + 16, ... in that order, then a pairwise tree over the slots).  The running
 *     sum is hierarchical: the same per-workgroup sums, in 256 chunks of ceil(B / 256) consecutive workgroups (each chunk
 *     added in order, a Hillis-Steele scan over the chunks), the workgroups of one chunk in order, and inside one workgroup
 *     its rows in increasing n (rows / 256 consecutive rows per lane added in order, the same scan over the lanes).  Each
 *     level takes the highest position of positive mass whose running sum before it is <= t_j.
 *     X [N x D] row-major and contiguous, FINITE (not checked here), inv_ls [D]; indices [M] int64 in the order chosen;
 *     dist [N]: the final mind, bit for bit tsvgp_kmeans_assign_f64's dist against X[indices]; pot_hist [M]: pot_r;
 *     cand, cand_pot, unif [M x L] row-major: cand_j, newpot_j and u(r, j) of every round, row 0 holding i_0, pot_0 and
 *     u(0, 0) in column 0; entries no round uses are -1, +inf and 0.  work: tsvgp_kmeanspp_work(N, D, L) doubles (one partial
 *     sum per workgroup and candidate; -1 for N < 1, D or L out of range, or N beyond rows * (2^31 - 1)).
 *     N >= 1, 1 <= M <= N, 1 <= D <= 32, 1 <= L <= TSVGP_KMEANSPP_MAX_TRIALS, no NULL pointer, every buffer on an 8-byte
 *     boundary; TSVGP_EINVAL otherwise, before any launch.  The call enqueues 2 M + 2 launches on `stream` (one fill, per centre
 *     one grid over n and L workgroups that reduce, choose and draw the next round's candidates, one last grid over n) and
 *     reads nothing back; no workgroup waits for another.  X is read once per centre; nothing of size N x M or N x L exists. */
#define TSVGP_KMEANSPP_MAX_TRIALS 16
int tsvgp_kmeanspp_rows(int D);
int64_t tsvgp_kmeanspp_work(int64_t N, int D, int L);
int tsvgp_kmeanspp_f64(const double *X, const double *inv_ls, int64_t seed, int M, int L, int64_t *indices, double *dist,
                       double *pot_hist, int64_t *cand, double *cand_pot, double *unif, double *work, int64_t N, int D, void *stream);

/* Device self-test of the MFMA fragment maps used above (writes a 16x16 product C = A*B, k = 4, for host checking).
 * a [16 x 4], b [4 x 16], c [16 x 16] row-major. */
int tsvgp_selftest_mfma_f64(const double *a, const double *b, double *c, void *stream);
int tsvgp_selftest_mfma_f32(const float *a, const float *b, float *c, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TSVGP_HIP_H */
