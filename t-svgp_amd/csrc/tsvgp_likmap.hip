// tsvgp_likmap.hip -- the likelihood maps of the E-step that run as launches of their own (behind the moments, not in their
// epilogue) for CDNA4 (gfx950 / MI355X), with their launchers and C entry points.  O(N P) each: microseconds beside the N-pass.
// A translation unit of its own: it shares tsvgp_device.h (the Gauss-Hermite tables, lik_eval) with the E-step kernels of
// tsvgp_kernels.hip, and their object code does not depend on it.
//
// Kernel inventory
//   lik_map_kernel            (mean, var, Y) -> (g0, g1, ve) of the Gaussian and Bernoulli likelihoods, the moments' epilogue alone.
//   lik_map_hetero_kernel     the heteroskedastic Gaussian: two coupled latents per row.
//   lik_map_scalar_kernel     StudentT, Poisson, Gamma / Exponential: one latent per target column, 20-point Gauss-Hermite.
//   lik_map_ordinal_kernel    Ordinal(bin_edges).
//   lmc_mix_kernel, lmc_unmix_kernel   LinearCoregionalization: P outputs mixed from L latents, and the gradients' way back.
//   diag_site_step_kernel     t_SVGP_sites: the map and the per-datum site update in one launch.
//   mc_normals_kernel         Philox4x32-10 + Box-Muller standard normals (the Softmax map's draws, also on their own).
//   lik_map_softmax_kernel    Softmax over C coupled latents, Monte Carlo.
//   lik_map_robustmax_kernel  MultiClass (RobustMax link), 20-point Gauss-Hermite.

#include <hip/hip_runtime.h>

#include <cmath>
#include <stdint.h>

#include "tsvgp_hip.h"
#include "tsvgp_device.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// lik_map_kernel: the likelihood-gradient map on its own: (mean, var, Y) -> g0 = d ve / d mean,
// g1 = d ve / d var (cropped at -1e-8 unless TSVGP_LIK_NOCROP), per-128-row sums of ve and counts of non-positive variances --
// what the moments kernels do in their epilogue, for a caller that assembled the moments itself (t_SVGP_white's two-product
// variance).  Reference src/models/tsvgp.py:256-263.  One workgroup per 128 rows, two threads per row (the Bernoulli
// quadrature split as in panel_kernel).  O(N P): microseconds.
// ---------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(NTHREADS) void lik_map_kernel(const T* __restrict__ mean, const T* __restrict__ var,
                                                           const T* __restrict__ Y, int lik, double lik_param,
                                                           T* __restrict__ g0o, T* __restrict__ g1o, double* __restrict__ ve_partial,
                                                           int32_t* __restrict__ nonpos_partial, int64_t N, int P) {
    __shared__ double red[NTHREADS / 64];
    __shared__ int redi[NTHREADS / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int srow = t >> 1, skh = t & 1;
    const int64_t n = (int64_t)blockIdx.x * TILE + srow;
    const bool live = n < N;
    double ve_acc = 0.0;
    int nonpos = 0;
    for (int p = 0; p < P; ++p) {
        const double mu = live ? (double)mean[n * P + p] : 0.0;
        const double v = live ? (double)var[n * P + p] : 1.0;
        double g0 = 0.0, g1 = 0.0, ve = 0.0;
        if ((lik & 0xFF) == TSVGP_LIK_BERNOULLI) {
            double a0, a1, av;
            const double sd = sqrt(v);
            bern_sums_t<T>(mu, sd, live && (double)Y[n * P + p] == 1.0, skh * 5, skh * 5 + 5, a0, a1, av);
            a0 += __shfl_xor(a0, 1);
            a1 += __shfl_xor(a1, 1);
            av += __shfl_xor(av, 1);
            g0 = a0;
            g1 = a1 / (2.0 * sd);
            if (!(lik & TSVGP_LIK_NOCROP)) g1 = fmin(g1, -1e-8);
            ve = av;
        } else if (live) {
            lik_eval(lik, lik_param, mu, v, (double)Y[n * P + p], g0, g1, ve);
        }
        if (skh == 0) {
            if (live) {
                if (!(v > 0.0)) nonpos += 1;
                ve_acc += ve;
            }
            g0o[n * P + p] = (T)(live ? g0 : 0.0);  // rows >= N of the [Np x P] outputs: zeros
            g1o[n * P + p] = (T)(live ? g1 : 0.0);
        }
    }
    double s = ve_acc;
    int c = nonpos;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o);
        c += __shfl_xor(c, o);
    }
    if (lane == 0) {
        red[w] = s;
        redi[w] = c;
    }
    __syncthreads();
    if (t == 0) {
        ve_partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
        nonpos_partial[blockIdx.x] = redi[0] + redi[1] + redi[2] + redi[3];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// lik_map_hetero_kernel: the heteroskedastic Gaussian likelihood (gpflow HeteroskedasticTFPConditional with a Normal and an
// Exp scale [ext]; reference docs/notebooks/heteroskedastic.py:58-76), the first map that couples two latents:
//     log p(y | f0, f1) = -1/2 log 2 pi - f1 - 1/2 (y - f0)^2 exp(-2 f1),
// its variational expectation by the 20 x 20 product Gauss-Hermite grid and the derivative OF THAT SUM with respect to
// (mean, var) of each latent.  The grid sum separates (S0 = sum_i w_i (y - f0_i)^2, S1 = sum_j w_j exp(-2 f1_j),
// W0 = sum_i w_i, Q2 = sum_i w_i z_i^2; the odd sums vanish node pair by node pair):
//     ve = -1/2 log 2 pi W0^2 - W0^2 m1 - 1/2 S0 S1,   S0 = W0 r^2 + Q2 v0,   r = y - m0
//     d/dm0 = W0 r S1,   d/dv0 = -1/2 Q2 S1,   d/dm1 = S0 S1 - W0^2,   d/dv1 = S0 T1 / (2 s1),  T1 = sum_j w_j z_j e^(-2 f1_j)
// so a row needs 20 exponentials, not 400.  fp64 arithmetic for either array type: exp(-2 f1) at f1 = m1 - 7.6 s1 leaves the
// fp32 range at moderate variances, and the map is bandwidth-trivial.  One thread per row, one workgroup per 128 rows.
// ---------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(TILE) void lik_map_hetero_kernel(const T* __restrict__ mean, const T* __restrict__ var,
                                                              const T* __restrict__ Y, int flags, T* __restrict__ g0o,
                                                              T* __restrict__ g1o, double* __restrict__ ve_partial,
                                                              int32_t* __restrict__ nonpos_partial, int64_t N) {
    __shared__ double red[TILE / 64];
    __shared__ int redi[TILE / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t n = (int64_t)blockIdx.x * TILE + t;
    const bool live = n < N;
    double d0m = 0.0, d0v = 0.0, d1m = 0.0, d1v = 0.0, ve = 0.0;
    int nonpos = 0;
    if (live) {
        const double m0 = (double)mean[2 * n], m1 = (double)mean[2 * n + 1];
        const double v0 = (double)var[2 * n], v1 = (double)var[2 * n + 1];
        const double r = (double)Y[n] - m0;
        const double s1 = sqrt(v1);
        double W0 = 0.0, Q2 = 0.0, S1 = 0.0, T1 = 0.0;
#pragma unroll
        for (int i = 0; i < 10; ++i) {  // node pairs +-z
            const double z = GH_X[i], wi = GH_W[i];
            const double ep = exp(-2.0 * (m1 + s1 * z)), em = exp(-2.0 * (m1 - s1 * z));
            W0 += 2.0 * wi;
            Q2 += 2.0 * wi * z * z;
            S1 += wi * (ep + em);
            T1 += wi * z * (ep - em);
        }
        const double S0 = W0 * r * r + Q2 * v0;
        ve = -0.5 * 1.83787706640934548356 * W0 * W0 - W0 * W0 * m1 - 0.5 * S0 * S1;
        d0m = W0 * r * S1;
        d0v = -0.5 * Q2 * S1;
        d1m = S0 * S1 - W0 * W0;
        d1v = S0 * T1 / (2.0 * s1);
        if (!(flags & TSVGP_LIK_NOCROP)) {  // reference tsvgp.py:262-263
            d0v = fmin(d0v, -1e-8);
            d1v = fmin(d1v, -1e-8);
        }
        nonpos = (v0 > 0.0 ? 0 : 1) + (v1 > 0.0 ? 0 : 1);
    }
    g0o[2 * n] = (T)d0m;  // rows >= N of the [Np x 2] outputs: zeros
    g0o[2 * n + 1] = (T)d1m;
    g1o[2 * n] = (T)d0v;
    g1o[2 * n + 1] = (T)d1v;
    double s = ve;
    int c = nonpos;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o);
        c += __shfl_xor(c, o);
    }
    if (lane == 0) {
        red[w] = s;
        redi[w] = c;
    }
    __syncthreads();
    if (t == 0) {
        ve_partial[blockIdx.x] = red[0] + red[1];
        nonpos_partial[blockIdx.x] = redi[0] + redi[1];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// lik_map_scalar_kernel: the scalar likelihoods that have no arm in the moments kernels' epilogue -- gpflow.likelihoods.StudentT
// and gpflow.likelihoods.Poisson (exp link) [ext], GPflow 2.2.1 -- as a map of their own behind the moments, one latent column
// per launch: (mean, var, Y) with element stride istride -> g0 = d ve / d mean, g1 = d ve / d var with element stride ostride
// (rows >= N zero; g1 cropped at -1e-8 unless TSVGP_LIK_NOCROP, a NaN stays NaN as under np.minimum), per-128-row sums of ve and
// (StudentT: d ve / d scale, Gamma: d ve / d shape; dparam_partial != nullptr) of the parameter derivative, and the count of rows
// with var <= 0 or a non-finite mean (Gamma: or a target outside its support).
//   StudentT (p0 = scale s, p1 = df nu, c0 = lgamma((nu+1)/2) - lgamma(nu/2) - 1/2 log(nu pi) - log s from the host):
//     log p(y | f) = c0 - (nu+1)/2 log1p(r^2 / nu),  r = (y - f) / s;  ve and the derivative OF THE 20-point Gauss-Hermite sum:
//     g0 = sum_i w_i l'(f_i),  g1 = sum_i w_i l'(f_i) z_i / (2 sqrt v),  f_i = m + sqrt(v) z_i,  l' = (nu+1) r / (s nu (1 + r^2/nu)),
//     d l / d s = ((nu+1) u / (1 + u) - 1) / s with u = r^2 / nu.
//   Poisson (p0 = binsize b, c0 = log b): the closed form GPflow takes under the exp link,
//     ve = y (m + log b) - b exp(m + v/2) - lgamma(y + 1),  g0 = y - b exp(m + v/2),  g1 = -1/2 b exp(m + v/2).
//   Gamma (p0 = shape a, c0 = lgamma(a), c1 = digamma(a) from the host; gpflow.likelihoods.Gamma with its exp link, scale = exp(f);
//   a == 1 is gpflow.likelihoods.Exponential): closed like Poisson's, with e = y exp(-m + v/2),
//     ve = -a m - lgamma(a) + (a - 1) log y - e,  g0 = -a + e,  g1 = -e / 2,  d ve / d a = -m - digamma(a) + log y;
//     at a == 1 exactly the term (a - 1) log y is skipped, not multiplied: y = 0 is then a legal target.  A row with y < 0, or with
//     y == 0 at a != 1, is counted with the bad rows and its ve is NaN.
// fp64 arithmetic for either array type (the map moves 5 N elements and is bound by them).  One thread per row, one workgroup per
// 128 rows; the sums are wave-reduced and written once per workgroup, no atomics: two calls agree bit for bit.
// ---------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(TILE) void lik_map_scalar_kernel(const T* __restrict__ mean, const T* __restrict__ var,
                                                              const T* __restrict__ Y, int64_t istride, int lik, double p0,
                                                              double p1, double c0, double c1, T* __restrict__ g0o,
                                                              T* __restrict__ g1o, int64_t ostride,
                                                              double* __restrict__ ve_partial,
                                                              double* __restrict__ dparam_partial,
                                                              int32_t* __restrict__ nonpos_partial, int64_t N) {
    __shared__ double red[TILE / 64], redp[TILE / 64];
    __shared__ int redi[TILE / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t n = (int64_t)blockIdx.x * TILE + t;
    const bool live = n < N;
    double g0 = 0.0, g1 = 0.0, ve = 0.0, dp = 0.0;
    int bad = 0;
    if (live) {
        const double m = (double)mean[n * istride], v = (double)var[n * istride], y = (double)Y[n * istride];
        bool ybad = false;
        if ((lik & 0xFF) == TSVGP_LIK_STUDENT_T) {
            const double sd = sqrt(v), inv_s = 1.0 / p0, nu1 = p1 + 1.0, inv_nu = 1.0 / p1;
            double a0 = 0.0, a1 = 0.0;
#pragma unroll 2
            for (int i = 0; i < 10; ++i) {  // node pairs +-z
                const double z = GH_X[i], wi = GH_W[i];
                const double rp = (y - (m + sd * z)) * inv_s, rm = (y - (m - sd * z)) * inv_s;
                const double up = rp * rp * inv_nu, um = rm * rm * inv_nu;
                const double dlp = nu1 * rp * inv_nu * inv_s / (1.0 + up), dlm = nu1 * rm * inv_nu * inv_s / (1.0 + um);
                ve += wi * ((c0 - 0.5 * nu1 * log1p(up)) + (c0 - 0.5 * nu1 * log1p(um)));
                a0 += wi * (dlp + dlm);
                a1 += wi * z * (dlp - dlm);
                dp += wi * ((nu1 * up / (1.0 + up) - 1.0) + (nu1 * um / (1.0 + um) - 1.0));
            }
            g0 = a0;
            g1 = a1 / (2.0 * sd);
            dp *= inv_s;
        } else if ((lik & 0xFF) == TSVGP_LIK_GAMMA) {
            const double e = y * exp(-m + 0.5 * v);
            const bool unit = p0 == 1.0;  // Exponential: no power of y in the density
            const double ly = (!unit || dparam_partial) ? log(y) : 0.0;
            ve = -p0 * m - c0 - e;
            if (!unit) ve += (p0 - 1.0) * ly;
            g0 = -p0 + e;
            g1 = -0.5 * e;
            dp = -m - c1 + ly;
            if (!(y > 0.0 || (unit && y == 0.0))) {  // outside the support (a NaN target too)
                ve = __builtin_nan("");
                ybad = true;
            }
        } else {  // TSVGP_LIK_POISSON
            const double e = p0 * exp(m + 0.5 * v);
            ve = y * (m + c0) - e - lgamma(y + 1.0);
            g0 = y - e;
            g1 = -0.5 * e;
        }
        if (!(lik & TSVGP_LIK_NOCROP) && g1 > -1e-8) g1 = -1e-8;  // reference tsvgp.py:262-263
        bad = (v > 0.0 && isfinite(m) && !ybad) ? 0 : 1;
    }
    g0o[n * ostride] = (T)g0;  // rows >= N of the padded outputs: zeros
    g1o[n * ostride] = (T)g1;
    double s = ve, d = dp;
    int c = bad;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o);
        d += __shfl_xor(d, o);
        c += __shfl_xor(c, o);
    }
    if (lane == 0) {
        red[w] = s;
        redp[w] = d;
        redi[w] = c;
    }
    __syncthreads();
    if (t == 0) {
        ve_partial[blockIdx.x] = red[0] + red[1];
        if (dparam_partial) dparam_partial[blockIdx.x] = redp[0] + redp[1];
        nonpos_partial[blockIdx.x] = redi[0] + redi[1];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// lik_map_ordinal_kernel: gpflow.likelihoods.Ordinal(bin_edges) [ext], GPflow 2.2.1 -- one latent, K = n_edges + 1 ordered bins,
// label y in {0 .. K-1}; one latent column per launch with the strides, outputs and partials of lik_map_scalar_kernel.  With
// up = edges[y] (+inf for y = K-1), lo = edges[y-1] (-inf for y = 0), a = (up - f) / sigma, b = (lo - f) / sigma,
//     Phi~(x) = Phi(x) (1 - 2e-3) + 1e-3,   phi = Phi~(a) - Phi~(b),   log p(y | f) = log(phi + 1e-6),
// ve the 20-point Gauss-Hermite sum over f_i = m + sqrt(v) z_i and g0, g1, dparam the derivatives OF THAT SUM:
//     l'(f) = -(1 - 2e-3) (N(a) - N(b)) / (sigma (phi + 1e-6)),   d l / d sigma = -(1 - 2e-3) (a N(a) - b N(b)) / (sigma (phi + 1e-6)),
//     g0 = sum_i w_i l'(f_i),   g1 = sum_i w_i l'(f_i) z_i / (2 sqrt v),   dparam = sum_n sum_i w_i d l / d sigma
// (N the standard normal density; the terms of an infinite edge are 0).  The two jitters 1e-3 cancel in phi, and what is left,
// (1 - 2e-3) (Phi(a) - Phi(b)), is taken from erfc on the side where both arguments are small: Phi(a) - Phi(b) = Q(b) - Q(a) when
// b > 0 -- the difference of two values near 1 would lose every digit of a far-tail bin.  The edges are staged into LDS once per
// workgroup (at most 255 doubles); the label selects two of them and is checked first: one that is no integer in [0, K) reads
// edge 0, makes the row's ve, g0, g1 NaN and counts the row as bad (lik_map_robustmax_kernel's convention).  Per row 40 erfc,
// 40 exp, 20 log: the map is bound by fp64 VALU work, not by its 5 N elements.  fp64 arithmetic for either array type; one thread
// per row, one workgroup per 128 rows, wave-reduced sums written once per workgroup, no atomics.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ordinal_node(double a, double b, bool a_inf, bool b_inf, double& logp, double& dl, double& ds) {
    const bool flip = b > 0.0;  // both arguments in the upper tail: take the difference of the upper tail masses
    const double hi = flip ? -b : a, lw = flip ? -a : b;
    const double phi = (0.5 * (1.0 - 2e-3)) * (erfc(-0.70710678118654752440 * hi) - erfc(-0.70710678118654752440 * lw));
    const double q = phi + 1e-6;
    const double na = a_inf ? 0.0 : 0.39894228040143267794 * exp(-0.5 * a * a);
    const double nb = b_inf ? 0.0 : 0.39894228040143267794 * exp(-0.5 * b * b);
    const double r = (1.0 - 2e-3) / q;
    logp = log(q);
    dl = -(na - nb) * r;
    ds = -((a_inf ? 0.0 : a * na) - (b_inf ? 0.0 : b * nb)) * r;
}

template <typename T>
__global__ __launch_bounds__(TILE) void lik_map_ordinal_kernel(const T* __restrict__ mean, const T* __restrict__ var,
                                                               const T* __restrict__ Y, int64_t istride, int flags,
                                                               const double* __restrict__ edges, int n_edges, double sigma,
                                                               T* __restrict__ g0o, T* __restrict__ g1o, int64_t ostride,
                                                               double* __restrict__ ve_partial,
                                                               double* __restrict__ dparam_partial,
                                                               int32_t* __restrict__ nonpos_partial, int64_t N) {
    __shared__ double ed[TSVGP_ORDINAL_MAX_EDGES + 1];
    __shared__ double red[TILE / 64], redp[TILE / 64];
    __shared__ int redi[TILE / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t n = (int64_t)blockIdx.x * TILE + t;
    const bool live = n < N;
    for (int i = t; i < n_edges; i += TILE) ed[i] = edges[i];
    __syncthreads();
    double g0 = 0.0, g1 = 0.0, ve = 0.0, dp = 0.0;
    int bad = 0;
    if (live) {
        const double m = (double)mean[n * istride], v = (double)var[n * istride], y = (double)Y[n * istride];
        const bool ok = y >= 0.0 && y <= (double)n_edges && y == floor(y);
        const int k = ok ? (int)y : 0;  // 0 <= k <= n_edges: ed[k] is read for k < n_edges, ed[k - 1] for k > 0
        const bool top = k == n_edges, bottom = k == 0;
        const double inf = __builtin_inf();
        const double up = top ? inf : ed[k], lo = bottom ? -inf : ed[k - 1];
        const double sd = sqrt(v), inv_s = 1.0 / sigma;
        const double a0 = (up - m) * inv_s, b0 = (lo - m) * inv_s, dz = sd * inv_s;
        double s0 = 0.0, s1 = 0.0;
#pragma unroll 2
        for (int i = 0; i < 10; ++i) {  // node pairs +-z: f = m +- sd z, so a = a0 -+ dz z
            const double z = GH_X[i], wi = GH_W[i];
            double lp, dlp, dsp, lm, dlm, dsm;
            ordinal_node(a0 - dz * z, b0 - dz * z, top, bottom, lp, dlp, dsp);
            ordinal_node(a0 + dz * z, b0 + dz * z, top, bottom, lm, dlm, dsm);
            ve += wi * (lp + lm);
            s0 += wi * (dlp + dlm);
            s1 += wi * z * (dlp - dlm);
            dp += wi * (dsp + dsm);
        }
        g0 = s0 * inv_s;
        g1 = s1 * inv_s / (2.0 * sd);
        dp *= inv_s;
        if (!(flags & TSVGP_LIK_NOCROP) && g1 > -1e-8) g1 = -1e-8;  // reference tsvgp.py:262-263; a NaN stays NaN
        if (!ok) {
            const double poison = __builtin_nan("");
            ve = poison;
            g0 = poison;
            g1 = poison;
        }
        bad = (v > 0.0 && isfinite(m) && ok) ? 0 : 1;
    }
    g0o[n * ostride] = (T)g0;  // rows >= N of the padded outputs: zeros
    g1o[n * ostride] = (T)g1;
    double s = ve, d = dp;
    int c = bad;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o);
        d += __shfl_xor(d, o);
        c += __shfl_xor(c, o);
    }
    if (lane == 0) {
        red[w] = s;
        redp[w] = d;
        redi[w] = c;
    }
    __syncthreads();
    if (t == 0) {
        ve_partial[blockIdx.x] = red[0] + red[1];
        if (dparam_partial) dparam_partial[blockIdx.x] = redp[0] + redp[1];
        nonpos_partial[blockIdx.x] = redi[0] + redi[1];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// lmc_mix_kernel / lmc_unmix_kernel: the linear model of coregionalization (gpflow.kernels.LinearCoregionalization and
// gpflow.conditionals.util.mix_latent_gp [ext], GPflow 2.2.1): P outputs f = W g of L independent latent GPs, W [P x L] fp64
// row-major in device memory for either array type.  Per row n
//     mix:    Fmu[n, p] = sum_l W[p, l] mean_g[n, l],        Fvar[n, p] = sum_l W[p, l]^2 var_g[n, l]
//     unmix:  g0_g[n, l] = sum_p W[p, l] g0_f[n, p],          g1_g[n, l] = sum_p W[p, l]^2 g1_f[n, p]
// (the chain rule of the variational expectations through the mix; g1_g cropped at -1e-8 unless TSVGP_LIK_NOCROP, a NaN stays
// NaN), and with dW_partial the per-128-row sums of  d ve / d W[p, l] = g0_f[n, p] mean_g[n, l] + 2 W[p, l] g1_f[n, p] var_g[n, l].
// One thread per row, one workgroup per 128 rows; W and its elementwise square are staged into LDS once per workgroup (at most
// 2 x 32 x 32 doubles) and read as broadcasts; the sums run over l (p) in index order in registers -- B is the compile-time
// bound of the accumulator array (8 or 32).  The block sums of dW take the 128 rows in four chunks of 32 staged into LDS, one
// thread per (p, l) pair (up to 8 pairs per thread; with fewer than 128 pairs, 128 / (P L) threads per pair, each on every
// G-th row, their sums added in order through LDS) adding the rows of a chunk in order: no atomics, no shuffles, an order fixed
// by the shape.  fp64 arithmetic for either array type; O(N (L + P)) loads and stores, HBM bound.
// ---------------------------------------------------------------------------------------------------------------
template <typename T, int B>
__global__ __launch_bounds__(TILE) void lmc_mix_kernel(const T* __restrict__ mean_g, const T* __restrict__ var_g,
                                                       const double* __restrict__ W, T* __restrict__ Fmu, T* __restrict__ Fvar,
                                                       int32_t* __restrict__ nonpos_partial, int64_t N, int L, int P) {
    __shared__ double Ws[TSVGP_MAX_BATCH * TSVGP_MAX_BATCH], W2s[TSVGP_MAX_BATCH * TSVGP_MAX_BATCH];
    __shared__ int redi[TILE / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t n = (int64_t)blockIdx.x * TILE + t;
    for (int i = t; i < P * L; i += TILE) {
        const double x = W[i];
        Ws[i] = x;
        W2s[i] = x * x;
    }
    __syncthreads();
    int bad = 0;
    if (n < N) {
        double am[B], av[B];
#pragma unroll
        for (int p = 0; p < B; ++p) am[p] = av[p] = 0.0;
        for (int l = 0; l < L; ++l) {
            const double m = (double)mean_g[n * L + l], v = (double)var_g[n * L + l];
            if (!(v > 0.0) || !isfinite(m)) bad = 1;
#pragma unroll
            for (int p = 0; p < B; ++p)
                if (p < P) {
                    am[p] = fma(Ws[p * L + l], m, am[p]);
                    av[p] = fma(W2s[p * L + l], v, av[p]);
                }
        }
#pragma unroll
        for (int p = 0; p < B; ++p)
            if (p < P) {
                Fmu[n * P + p] = (T)am[p];
                Fvar[n * P + p] = (T)av[p];
            }
    }
    if (nonpos_partial) {  // (uniform over the grid)
        int c = bad;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
        if (lane == 0) redi[w] = c;
        __syncthreads();
        if (t == 0) nonpos_partial[blockIdx.x] = redi[0] + redi[1];
    }
}

#define LMC_CHUNK 32
template <typename T, int B>
__global__ __launch_bounds__(TILE) void lmc_unmix_kernel(const T* __restrict__ g0_f, const T* __restrict__ g1_f,
                                                         const double* __restrict__ W, int flags, T* __restrict__ g0_g,
                                                         T* __restrict__ g1_g, const T* __restrict__ mean_g,
                                                         const T* __restrict__ var_g, double* __restrict__ dW_partial, int64_t N,
                                                         int L, int P) {
    __shared__ double Ws[TSVGP_MAX_BATCH * TSVGP_MAX_BATCH], W2s[TSVGP_MAX_BATCH * TSVGP_MAX_BATCH];
    __shared__ double c0[LMC_CHUNK * TSVGP_MAX_BATCH], c1[LMC_CHUNK * TSVGP_MAX_BATCH];  // g0_f, g1_f of a chunk [32 x P]
    __shared__ double cm[LMC_CHUNK * TSVGP_MAX_BATCH], cv[LMC_CHUNK * TSVGP_MAX_BATCH];  // mean_g, var_g of a chunk [32 x L]
    const int t = threadIdx.x;
    const int64_t n0 = (int64_t)blockIdx.x * TILE, n = n0 + t;
    for (int i = t; i < P * L; i += TILE) {
        const double x = W[i];
        Ws[i] = x;
        W2s[i] = x * x;
    }
    __syncthreads();
    {
        double a0[B], a1[B];
#pragma unroll
        for (int l = 0; l < B; ++l) a0[l] = a1[l] = 0.0;
        if (n < N) {
            for (int p = 0; p < P; ++p) {
                const double d0 = (double)g0_f[n * P + p], d1 = (double)g1_f[n * P + p];
#pragma unroll
                for (int l = 0; l < B; ++l)
                    if (l < L) {
                        a0[l] = fma(Ws[p * L + l], d0, a0[l]);
                        a1[l] = fma(W2s[p * L + l], d1, a1[l]);
                    }
            }
            if (!(flags & TSVGP_LIK_NOCROP)) {
#pragma unroll
                for (int l = 0; l < B; ++l)
                    if (a1[l] > -1e-8) a1[l] = -1e-8;  // reference tsvgp.py:262-263; a NaN stays NaN
            }
        }
#pragma unroll
        for (int l = 0; l < B; ++l)
            if (l < L) {  // rows >= N of the padded outputs: zeros
                g0_g[n * L + l] = (T)a0[l];
                g1_g[n * L + l] = (T)a1[l];
            }
    }
    if (!dW_partial) return;  // (uniform over the grid)
    // P L <= 1024 pairs: thread t owns the pairs t, t + 128, ...; with fewer than 128 pairs the threads form G = 128 / (P L) row
    // groups instead, group g of a pair adding the rows g, g + G, ... of every chunk, and the groups are added in order at the end
    const int npair = P * L;
    const int G = npair >= TILE ? 1 : TILE / npair;
    const int grp = G > 1 ? t / npair : 0, t0 = G > 1 ? t - grp * npair : t;
    const bool active = grp < G;  // (G > 1: the last 128 - G P L threads only help to load)
    double s0[8], s1[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) s0[k] = s1[k] = 0.0;
    for (int c = 0; c < TILE / LMC_CHUNK; ++c) {
        const int64_t r0 = n0 + (int64_t)c * LMC_CHUNK;
        __syncthreads();  // the previous chunk has been read
        for (int i = t; i < LMC_CHUNK * P; i += TILE) {  // rows of g0_f, g1_f [Np x P]: all exist, those >= N count as zero
            const bool live = r0 + i / P < N;
            c0[i] = live ? (double)g0_f[r0 * P + i] : 0.0;
            c1[i] = live ? (double)g1_f[r0 * P + i] : 0.0;
        }
        for (int i = t; i < LMC_CHUNK * L; i += TILE) {  // mean_g, var_g [N x L]: rows >= N are not there
            const bool live = r0 + i / L < N;
            cm[i] = live ? (double)mean_g[r0 * L + i] : 0.0;
            cv[i] = live ? (double)var_g[r0 * L + i] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int idx = t0 + k * TILE;
            if (active && idx < npair) {
                const int p = idx / L, l = idx - p * L;
                double b0 = s0[k], b1 = s1[k];
                for (int r = grp; r < LMC_CHUNK; r += G) {
                    b0 = fma(c0[r * P + p], cm[r * L + l], b0);
                    b1 = fma(c1[r * P + p], cv[r * L + l], b1);
                }
                s0[k] = b0;
                s1[k] = b1;
            }
        }
    }
    if (G > 1) {  // (uniform over the block) one pair per thread: the groups' sums through LDS, added in group order
        __syncthreads();  // the last chunk has been read: c0, c1 are free
        if (active) {
            c0[grp * npair + t0] = s0[0];
            c1[grp * npair + t0] = s1[0];
        }
        __syncthreads();
        if (t < npair) {
            double b0 = 0.0, b1 = 0.0;
            for (int g = 0; g < G; ++g) {
                b0 += c0[g * npair + t];
                b1 += c1[g * npair + t];
            }
            dW_partial[(int64_t)blockIdx.x * npair + t] = b0 + 2.0 * Ws[t] * b1;
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int idx = t + k * TILE;
        if (idx < npair) dW_partial[(int64_t)blockIdx.x * npair + idx] = s0[k] + 2.0 * Ws[idx] * s1[k];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// diag_site_step_kernel: the per-datum site update of t_SVGP_sites (reference src/models/tsvgp_sites.py:113-145) fused with
// the likelihood-gradient map of lik_map_kernel (same device functions, same two-threads-per-row quadrature split, g1 never
// cropped).  Per row and latent, in place on the fp64 site state [Np x P]:
//     g0' = g0 - 2 g1 mean,   lambda_1 <- (1 - lr) lambda_1 + lr g0',
//     n2 = min((1 - lr)(-lambda_2 / 2) + lr g1, -1e-8),   lambda_2 <- -2 n2      (so lambda_2 >= 2e-8)
// plus, when l1c / l2c are given (the fp32 entry), copies of the new values in T: the weights tsvgp_site_accum_f32 reads on
// the next projection.  Rows >= N are not touched (the caller keeps them zero: the projection then adds nothing for them).
// ve_partial / nonpos_partial as lik_map_kernel; var == nullptr (Gaussian only: neither update reads the variance) gives
// NaN ve partials and counts rows with a non-finite mean or gradient instead, as mean_lik_kernel does.  One workgroup per
// 128 rows; O(N P) loads and stores, HBM bound.
// ---------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(NTHREADS) void diag_site_step_kernel(const T* __restrict__ mean, const T* __restrict__ var,
                                                                  const T* __restrict__ Y, int lik, double lik_param, double lr,
                                                                  double* __restrict__ l1, double* __restrict__ l2,
                                                                  T* __restrict__ l1c, T* __restrict__ l2c,
                                                                  double* __restrict__ ve_partial,
                                                                  int32_t* __restrict__ nonpos_partial, int64_t N, int P) {
    __shared__ double red[NTHREADS / 64];
    __shared__ int redi[NTHREADS / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int srow = t >> 1, skh = t & 1;
    const int64_t n = (int64_t)blockIdx.x * TILE + srow;
    const bool live = n < N;
    const int lk = (lik & 0xFF) | TSVGP_LIK_NOCROP;
    double ve_acc = 0.0;
    int nonpos = 0;
    for (int p = 0; p < P; ++p) {
        const int64_t i = n * P + p;
        const double mu = live ? (double)mean[i] : 0.0;
        const double v = (live && var) ? (double)var[i] : 1.0;
        double g0 = 0.0, g1 = 0.0, ve = 0.0;
        if ((lk & 0xFF) == TSVGP_LIK_BERNOULLI) {
            double a0, a1, av;
            const double sd = sqrt(v);
            bern_sums_t<T>(mu, sd, live && (double)Y[i] == 1.0, skh * 5, skh * 5 + 5, a0, a1, av);
            a0 += __shfl_xor(a0, 1);
            a1 += __shfl_xor(a1, 1);
            av += __shfl_xor(av, 1);
            g0 = a0;
            g1 = a1 / (2.0 * sd);
            ve = av;
        } else if (live) {
            lik_eval(lk, lik_param, mu, v, (double)Y[i], g0, g1, ve);
        }
        if (skh == 0 && live) {
            if (var) {
                if (!(v > 0.0)) nonpos += 1;
                ve_acc += ve;
            } else if (!(fabs(mu) <= 1.79769313486231570815e308) || !(fabs(g0) <= 1.79769313486231570815e308)) {
                nonpos += 1;
            }
            const double g0m = g0 - 2.0 * g1 * mu;  // tsvgp_sites.py:133
            const double a1 = (1.0 - lr) * l1[i] + lr * g0m;  // :139
            const double n2 = fmin((1.0 - lr) * (-0.5 * l2[i]) + lr * g1, -1e-8);  // :136, :140, :144
            const double a2 = -2.0 * n2;  // :148
            l1[i] = a1;
            l2[i] = a2;
            if (l1c) {
                l1c[i] = (T)a1;
                l2c[i] = (T)a2;
            }
        }
    }
    double s = ve_acc;
    int c = nonpos;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o);
        c += __shfl_xor(c, o);
    }
    if (lane == 0) {
        red[w] = s;
        redi[w] = c;
    }
    __syncthreads();
    if (t == 0) {
        ve_partial[blockIdx.x] = var ? red[0] + red[1] + red[2] + red[3] : __builtin_nan("");
        nonpos_partial[blockIdx.x] = redi[0] + redi[1] + redi[2] + redi[3];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The Monte Carlo normal generator (include/tsvgp_hip.h, "The normal generator"): Philox4x32-10 [Salmon et al. 2011] and
// Box-Muller.  The draw for (seed, draw, global row n, sample s, class c) is a pure function of those five integers:
// key = (seed lo, seed hi), counter = (n lo, n hi, s * 8 + (c >> 2), draw lo); one call gives the four normals of classes
// 4 (c >> 2) .. + 3: outputs (x0, x1) -> classes +0 (cos) and +1 (sin), (x2, x3) -> +2 and +3.  All of it in fp64 for either
// array type, so a draw does not depend on the dtype around it.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t& x0, uint32_t& x1, uint32_t& x2, uint32_t& x3) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    x0 = c0, x1 = c1, x2 = c2, x3 = c3;
}

__device__ __forceinline__ void box_muller(uint32_t xa, uint32_t xb, double& za, double& zb) {
    const double u1 = ((double)xa + 0.5) * 0x1p-32, u2 = ((double)xb + 0.5) * 0x1p-32;  // exact: in (0, 1)
    const double r = sqrt(-2.0 * log(u1));
    const double th = 6.283185307179586 * u2;
    za = r * cos(th);
    zb = r * sin(th);
}

__device__ __forceinline__ void mc_normals4(int64_t seed, int64_t draw, int64_t n, uint32_t s, uint32_t q, double z[4]) {
    uint32_t x0, x1, x2, x3;
    philox4x32_10((uint32_t)(uint64_t)n, (uint32_t)((uint64_t)n >> 32), s * 8u + q, (uint32_t)(uint64_t)draw,
                  (uint32_t)(uint64_t)seed, (uint32_t)((uint64_t)seed >> 32), x0, x1, x2, x3);
    box_muller(x0, x1, z[0], z[1]);
    box_muller(x2, x3, z[2], z[3]);
}

// mc_normals_kernel: out[s, n, c] (GPflow's epsilon layout [S x N x C]) = the draw of (seed, draw, row_offset + n, s, c).
// One thread per (s, n, class quad).
template <typename T>
__global__ __launch_bounds__(256) void mc_normals_kernel(T* __restrict__ out, int64_t seed, int64_t draw, int64_t row_offset,
                                                         int64_t S, int64_t N, int C) {
    const int Q4 = (C + 3) >> 2;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= S * N * Q4) return;
    const int q = (int)(i % Q4);
    const int64_t sn = i / Q4, n = sn % N, s = sn / N;
    double z[4];
    mc_normals4(seed, draw, row_offset + n, (uint32_t)s, (uint32_t)q, z);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (4 * q + k < C) out[sn * C + 4 * q + k] = (T)z[k];
}

// ---------------------------------------------------------------------------------------------------------------
// lik_map_softmax_kernel: gpflow.likelihoods.Softmax [ext] (a MonteCarloLikelihood; reference docs/notebooks/mnist.py), the
// map that couples C latents: with f^s = mean + sqrt(var) eps^s, p^s = softmax(f^s), d_c^s = [c == y] - p_c^s,
//     ve = 1/S sum_s (f_y^s - logsumexp_c f_c^s),  g0_c = 1/S sum_s d_c^s,  g1_c = 1/S sum_s d_c^s eps_c^s / (2 sqrt(var_c))
// (the derivative of the estimator through the reparameterisation, reference src/models/tsvgp.py:256-263).
// ONE WAVE PER ROW: lane = sg * Q + q holds the classes 4 q .. 4 q + 3 (one Philox call) of the samples s = sg, sg + 64 / Q, ...;
// Q = the class quads of the row rounded up to a power of two (template: 1, 2, 4, 8), so the per-row values are a fixed four per
// lane and nothing is indexed at run time.  The softmax of a sample is a max / sum butterfly over its Q lanes, the sample
// sums a butterfly over the 64 / Q sample groups; every sum has one fixed order.  A workgroup of four waves takes 128 rows
// (32 per wave, one after the other) and writes their fp64 block sum of ve.  eps comes from `epsilon` [S x N x C] if given,
// else from the generator with (seed, draw) READ FROM DEVICE MEMORY (a replayed graph sees the advanced draw).
// The label is never an address: lanes compare their class numbers with it; a label that is no integer in [0, C) makes the
// row's ve, g0, g1 NaN.
// ---------------------------------------------------------------------------------------------------------------
template <typename T, int Q>
__global__ __launch_bounds__(256) void lik_map_softmax_kernel(const T* __restrict__ mean, const T* __restrict__ var,
                                                              const T* __restrict__ Y, int flags, int C, int S,
                                                              const int64_t* __restrict__ rng_state, int64_t row_offset,
                                                              const T* __restrict__ epsilon, T* __restrict__ g0o,
                                                              T* __restrict__ g1o, double* __restrict__ ve_partial,
                                                              int32_t* __restrict__ nonpos_partial, int64_t N) {
    constexpr int NSG = 64 / Q;  // sample groups of a wave
    __shared__ double red[4];
    __shared__ int redi[4];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int q = lane % Q, sg = lane / Q;
    int64_t seed = 0, draw = 0;
    if (!epsilon) seed = rng_state[0], draw = rng_state[1];
    bool valid[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) valid[k] = 4 * q + k < C;
    const double inv_S = 1.0 / (double)S;
    double ve_wave = 0.0;
    int nonpos_wave = 0;
    for (int r = 0; r < 32; ++r) {
        const int64_t n = (int64_t)blockIdx.x * TILE + w * 32 + r;  // wave-uniform
        if (n >= N) {  // rows >= N of the [Np x C] outputs: zeros
            if (sg == 0) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (valid[k]) g0o[n * C + 4 * q + k] = (T)0.0, g1o[n * C + 4 * q + k] = (T)0.0;
            }
            continue;
        }
        double m[4], sd[4], a0[4], a1[4];
        bool isy[4];
        const double y = (double)Y[n];
        const bool bad = !(y >= 0.0 && y < (double)C && y == floor(y));
        int nonpos = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double v = valid[k] ? (double)var[n * C + 4 * q + k] : 1.0;
            m[k] = valid[k] ? (double)mean[n * C + 4 * q + k] : 0.0;
            sd[k] = sqrt(v);
            a0[k] = a1[k] = 0.0;
            isy[k] = valid[k] && (double)(4 * q + k) == y;
            nonpos += (sg == 0 && !(v > 0.0)) ? 1 : 0;
        }
        double vel = 0.0;
        for (int s0 = 0; s0 < S; s0 += NSG) {  // wave-uniform trip count; lanes beyond S are masked
            const int s = s0 + sg;
            const bool act = s < S;
            double eps[4] = {0.0, 0.0, 0.0, 0.0};
            if (act && valid[0]) {
                if (epsilon) {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (valid[k]) eps[k] = (double)epsilon[((int64_t)s * N + n) * C + 4 * q + k];
                } else {
                    mc_normals4(seed, draw, row_offset + n, (uint32_t)s, (uint32_t)q, eps);
                }
            }
            double f[4], mx = -INFINITY;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                f[k] = m[k] + sd[k] * eps[k];
                mx = valid[k] ? fmax(mx, f[k]) : mx;
            }
#pragma unroll
            for (int o = 1; o < Q; o <<= 1) mx = fmax(mx, __shfl_xor(mx, o));
            double e[4], sum = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                e[k] = valid[k] ? exp(f[k] - mx) : 0.0;
                sum += e[k];
            }
#pragma unroll
            for (int o = 1; o < Q; o <<= 1) sum += __shfl_xor(sum, o);
            const double inv = 1.0 / sum;
            if (act) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double d = (isy[k] ? 1.0 : 0.0) - e[k] * inv;
                    a0[k] += d;
                    a1[k] += d * eps[k];
                    vel += isy[k] ? f[k] - mx : 0.0;
                }
                if (q == 0) vel -= log(sum);
            }
        }
#pragma unroll
        for (int o = Q; o < 64; o <<= 1) {  // over the sample groups
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                a0[k] += __shfl_xor(a0[k], o);
                a1[k] += __shfl_xor(a1[k], o);
            }
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            vel += __shfl_xor(vel, o);
            nonpos += __shfl_xor(nonpos, o);
        }
        const double poison = bad ? NAN : 0.0;
        if (sg == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                double d0 = a0[k] * inv_S, d1 = a1[k] * inv_S / (2.0 * sd[k]);
                // reference tsvgp.py:262-263; a NaN (non-positive variance) stays NaN as under np.minimum: fmin would drop it
                if (!(flags & TSVGP_LIK_NOCROP)) d1 = d1 != d1 ? d1 : fmin(d1, -1e-8);
                if (valid[k]) g0o[n * C + 4 * q + k] = (T)(d0 + poison), g1o[n * C + 4 * q + k] = (T)(d1 + poison);
            }
        }
        ve_wave += vel * inv_S + poison;
        nonpos_wave += nonpos;
    }
    if (lane == 0) {
        red[w] = ve_wave;
        redi[w] = nonpos_wave;
    }
    __syncthreads();
    if (t == 0) {
        ve_partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
        nonpos_partial[blockIdx.x] = redi[0] + redi[1] + redi[2] + redi[3];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// lik_map_robustmax_kernel: gpflow.likelihoods.MultiClass(C) with the RobustMax inverse link [ext] (GPflow 2.2.1), the
// deterministic map over C coupled latents.  With y the row's label, s_c = sqrt(max(v_c, 1e-10)), the 20 Gauss-Hermite nodes
// X_i = m_y + x_i sqrt(max(2 v_y, 1e-10)) over the labelled latent and d_ci = (X_i - m_c) / s_c,
//     F_ci = 1/2 (1 + erf(d_ci / sqrt 2)) (1 - 2e-4) + 1e-4,   P_i = prod_{c != y} F_ci,   p = sum_i w_i P_i   (w_i: weights / sqrt pi)
//     ve = p log(1 - eps) + (1 - p) log(eps / (C - 1)),   kappa = log(1 - eps) - log(eps / (C - 1)),
// and the derivative OF THAT SUM (reference src/models/tsvgp.py:256-263), r_ci = (1 - 2e-4) N(d_ci) / F_ci:
//     c != y:  g0_c = -kappa sum_i w_i P_i r_ci / s_c,             g1_c = -kappa sum_i w_i P_i r_ci d_ci / (2 v_c)
//     c == y:  g0_y =  kappa sum_i w_i P_i sum_{c != y} r_ci / s_c,  g1_y = kappa sum_i w_i P_i (sum_{c != y} r_ci / s_c) z_i / (2 s_y)
// (z_i = sqrt 2 x_i); a clipped variance has derivative zero, as under tf.clip_by_value; a NaN variance stays NaN.
// One thread per row, one workgroup per 128 rows as lik_map_scalar_kernel.  The loops run class by class: the first pass
// multiplies the 20 products P_i up (one LDS column of 20 doubles per thread: indexed by the node, never by the class, so
// nothing of the row is indexed at run time in registers and nothing goes to scratch), the second evaluates F_ci again,
// weighs r_ci with the finished P_i and writes class c's g0, g1 at once, summing the labelled class's two values on the way.
// The label is never an address: the class loop compares its counter with it; a label that is no integer in [0, C) makes the
// row's ve, g0, g1 NaN.  fp64 arithmetic for either array type; no atomics, a summation order fixed by the shape.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double robustmax_cdf(double d) {
    return 0.5 * (1.0 + erf(d * 0.70710678118654752440)) * (1.0 - 2e-4) + 1e-4;
}

template <typename T>
__global__ __launch_bounds__(TILE) void lik_map_robustmax_kernel(const T* __restrict__ mean, const T* __restrict__ var,
                                                                 const T* __restrict__ Y, int flags, int C, double log_hit,
                                                                 double log_miss, T* __restrict__ g0o, T* __restrict__ g1o,
                                                                 double* __restrict__ ve_partial,
                                                                 int32_t* __restrict__ nonpos_partial, int64_t N) {
    __shared__ double prod[20][TILE];  // P_i of the thread's row: nodes +z_i in [i], -z_i in [10 + i]
    __shared__ double red[TILE / 64];
    __shared__ int redi[TILE / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t n = (int64_t)blockIdx.x * TILE + t;
    const bool crop = !(flags & TSVGP_LIK_NOCROP);
    T* __restrict__ g0r = g0o + n * C;
    T* __restrict__ g1r = g1o + n * C;
    double ve = 0.0;
    int bad = 0;
    if (n < N) {
        const T* __restrict__ mr = mean + n * C;
        const T* __restrict__ vr = var + n * C;
        const double y = (double)Y[n];
        const double poison = (y >= 0.0 && y < (double)C && y == floor(y)) ? 0.0 : __builtin_nan("");
        double my = 0.0, vy = 1.0;
        for (int c = 0; c < C; ++c) {
            const double m = (double)mr[c], v = (double)vr[c];
            bad |= (v > 0.0 && isfinite(m)) ? 0 : 1;
            if ((double)c == y) my = m, vy = v;
        }
        const bool clip_y = 2.0 * vy < 1e-10;
        const double sy = sqrt(clip_y ? 1e-10 : 2.0 * vy) * 0.70710678118654752440;  // s_y: X_i = m_y + z_i s_y
#pragma unroll
        for (int i = 0; i < 20; ++i) prod[i][t] = 1.0;
        for (int c = 0; c < C; ++c) {
            if ((double)c == y) continue;
            const double m = (double)mr[c], v = (double)vr[c];
            const double is = 1.0 / sqrt(v < 1e-10 ? 1e-10 : v);
            const double d0 = (my - m) * is, dz = sy * is;
#pragma unroll 2
            for (int i = 0; i < 10; ++i) {
                const double z = GH_X[i];
                prod[i][t] *= robustmax_cdf(d0 + dz * z);
                prod[10 + i][t] *= robustmax_cdf(d0 - dz * z);
            }
        }
        double p = 0.0;
#pragma unroll
        for (int i = 0; i < 10; ++i) p += GH_W[i] * (prod[i][t] + prod[10 + i][t]);
        ve = p * log_hit + (1.0 - p) * log_miss + poison;
        const double kappa = log_hit - log_miss;
        double gy0 = 0.0, gy1 = 0.0;
        for (int c = 0; c < C; ++c) {
            if ((double)c == y) continue;
            const double m = (double)mr[c], v = (double)vr[c];
            const bool clip_c = v < 1e-10;
            const double vc = clip_c ? 1e-10 : v;
            const double is = 1.0 / sqrt(vc);
            const double d0 = (my - m) * is, dz = sy * is;
            double a = 0.0, b = 0.0, az = 0.0;
#pragma unroll 2
            for (int i = 0; i < 10; ++i) {
                const double z = GH_X[i], wi = GH_W[i];
                const double dp = d0 + dz * z, dm = d0 - dz * z;
                // w_i P_i r_ci at +z_i and -z_i
                const double rp = wi * prod[i][t] * ((1.0 - 2e-4) * 0.39894228040143267794) * exp(-0.5 * dp * dp) / robustmax_cdf(dp);
                const double rm = wi * prod[10 + i][t] * ((1.0 - 2e-4) * 0.39894228040143267794) * exp(-0.5 * dm * dm) / robustmax_cdf(dm);
                a += rp + rm;
                b += rp * dp + rm * dm;
                az += (rp - rm) * z;
            }
            gy0 += a * is;
            gy1 += az * is;
            double g1 = clip_c ? 0.0 : -kappa * b / (2.0 * vc);
            if (crop && g1 > -1e-8) g1 = -1e-8;  // reference tsvgp.py:262-263; a NaN stays NaN
            g0r[c] = (T)(-kappa * a * is + poison);
            g1r[c] = (T)(g1 + poison);
        }
        double g1y = clip_y ? 0.0 : kappa * gy1 / (2.0 * sy);
        if (crop && g1y > -1e-8) g1y = -1e-8;
        for (int c = 0; c < C; ++c) {
            if ((double)c == y) {
                g0r[c] = (T)(kappa * gy0);
                g1r[c] = (T)g1y;
            }
        }
    } else {
        for (int c = 0; c < C; ++c) {  // rows >= N of the [Np x C] outputs: zeros
            g0r[c] = (T)0.0;
            g1r[c] = (T)0.0;
        }
    }
    double s = ve;
    int k = bad;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o);
        k += __shfl_xor(k, o);
    }
    if (lane == 0) {
        red[w] = s;
        redi[w] = k;
    }
    __syncthreads();
    if (t == 0) {
        ve_partial[blockIdx.x] = red[0] + red[1];
        nonpos_partial[blockIdx.x] = redi[0] + redi[1];
    }
}

template <typename T>
int lik_map(const T* mean, const T* var, const T* Y, int lik, double lik_param, T* g0, T* g1, double* ve_partial,
            int32_t* nonpos_partial, int64_t N, int64_t Np, int P, void* stream) {
    if (!mean || !var || !Y || !g0 || !g1 || !ve_partial || !nonpos_partial || N <= 0 || Np < N || (Np % TILE) || P <= 0)
        return TSVGP_EINVAL;
    if (lik & ~(0xFF | TSVGP_LIK_NOCROP)) return TSVGP_EINVAL;
    const int base = lik & 0xFF;
    if (base != TSVGP_LIK_GAUSSIAN && base != TSVGP_LIK_BERNOULLI) return TSVGP_EINVAL;
    if (base == TSVGP_LIK_GAUSSIAN && !(lik_param > 0.0)) return TSVGP_EINVAL;
    hipLaunchKernelGGL(lik_map_kernel<T>, dim3((unsigned)(Np / TILE)), dim3(NTHREADS), 0, (hipStream_t)stream, mean, var, Y, lik,
                       lik_param, g0, g1, ve_partial, nonpos_partial, N, P);
    return launch_status();
}

template <typename T>
int diag_site_step(const T* mean, const T* var, const T* Y, int lik, double lik_param, double lr, double* l1, double* l2, T* l1c,
                   T* l2c, double* ve_partial, int32_t* nonpos_partial, int64_t N, int64_t Np, int P, void* stream) {
    if (!mean || !Y || !l1 || !l2 || !ve_partial || !nonpos_partial || N <= 0 || Np < N || (Np % TILE) || P <= 0) return TSVGP_EINVAL;
    if (!l1c != !l2c) return TSVGP_EINVAL;
    if (lik & ~(0xFF | TSVGP_LIK_NOCROP)) return TSVGP_EINVAL;
    const int base = lik & 0xFF;
    if (base != TSVGP_LIK_GAUSSIAN && base != TSVGP_LIK_BERNOULLI) return TSVGP_EINVAL;
    if (base == TSVGP_LIK_GAUSSIAN && !(lik_param > 0.0)) return TSVGP_EINVAL;
    if (base == TSVGP_LIK_BERNOULLI && !var) return TSVGP_EINVAL;
    if (!(lr >= 0.0 && lr <= 1.0)) return TSVGP_EINVAL;
    hipLaunchKernelGGL(diag_site_step_kernel<T>, dim3((unsigned)(Np / TILE)), dim3(NTHREADS), 0, (hipStream_t)stream, mean, var, Y,
                       lik, lik_param, lr, l1, l2, l1c, l2c, ve_partial, nonpos_partial, N, P);
    return launch_status();
}

template <typename T>
int lik_map_hetero(const T* mean, const T* var, const T* Y, int flags, T* g0, T* g1, double* ve_partial, int32_t* nonpos_partial,
                   int64_t N, int64_t Np, void* stream) {
    if (!mean || !var || !Y || !g0 || !g1 || !ve_partial || !nonpos_partial || N <= 0 || Np < N || (Np % TILE)) return TSVGP_EINVAL;
    if ((flags & ~TSVGP_LIK_NOCROP) != TSVGP_LIK_HETERO) return TSVGP_EINVAL;
    hipLaunchKernelGGL(lik_map_hetero_kernel<T>, dim3((unsigned)(Np / TILE)), dim3(TILE), 0, (hipStream_t)stream, mean, var, Y, flags,
                       g0, g1, ve_partial, nonpos_partial, N);
    return launch_status();
}

// digamma(x), x > 0, on the host (the Gamma arm's d lgamma(a) / d a): the recurrence up to x >= 10, then the asymptotic series,
// whose first dropped term is 691 / (32760 x^12) < 3e-14 there.
static double digamma_host(double x) {
    double r = 0.0;
    while (x < 10.0) {
        r -= 1.0 / x;
        x += 1.0;
    }
    const double f = 1.0 / (x * x);
    return r + std::log(x) - 0.5 / x -
           f * (1.0 / 12.0 - f * (1.0 / 120.0 - f * (1.0 / 252.0 - f * (1.0 / 240.0 - f * (1.0 / 132.0)))));
}

template <typename T>
int lik_map_scalar(const T* mean, const T* var, const T* Y, int64_t in_stride, int lik, double param0, double param1, T* g0, T* g1,
                   int64_t out_stride, double* ve_partial, double* dparam_partial, int32_t* nonpos_partial, int64_t N, int64_t Np,
                   void* stream) {
    if (!mean || !var || !Y || !g0 || !g1 || !ve_partial || !nonpos_partial || N <= 0 || Np < N || (Np % TILE)) return TSVGP_EINVAL;
    if (in_stride < 1 || out_stride < 1) return TSVGP_EINVAL;
    if (lik & ~(0xFF | TSVGP_LIK_NOCROP)) return TSVGP_EINVAL;
    const int base = lik & 0xFF;
    double c0, c1 = 0.0;
    if (base == TSVGP_LIK_STUDENT_T) {
        if (!(param0 > 0.0) || !(param1 > 0.0) || !std::isfinite(param0) || !std::isfinite(param1)) return TSVGP_EINVAL;
        // the terms of log p that no row changes, once, on the host
        c0 = std::lgamma(0.5 * (param1 + 1.0)) - std::lgamma(0.5 * param1) - 0.5 * std::log(param1 * 3.14159265358979323846) -
             std::log(param0);
    } else if (base == TSVGP_LIK_POISSON) {
        if (!(param0 > 0.0) || !std::isfinite(param0) || dparam_partial) return TSVGP_EINVAL;
        c0 = std::log(param0);
    } else if (base == TSVGP_LIK_GAMMA) {
        if (!(param0 > 0.0) || !std::isfinite(param0)) return TSVGP_EINVAL;
        c0 = std::lgamma(param0);
        c1 = digamma_host(param0);
    } else {
        return TSVGP_EINVAL;
    }
    hipLaunchKernelGGL(lik_map_scalar_kernel<T>, dim3((unsigned)(Np / TILE)), dim3(TILE), 0, (hipStream_t)stream, mean, var, Y,
                       in_stride, lik, param0, param1, c0, c1, g0, g1, out_stride, ve_partial, dparam_partial, nonpos_partial, N);
    return launch_status();
}

template <typename T>
int lik_map_ordinal(const T* mean, const T* var, const T* Y, int64_t in_stride, int flags, const double* edges, int n_edges,
                    double sigma, T* g0, T* g1, int64_t out_stride, double* ve_partial, double* dparam_partial,
                    int32_t* nonpos_partial, int64_t N, int64_t Np, void* stream) {
    if (!mean || !var || !Y || !g0 || !g1 || !ve_partial || !nonpos_partial || N <= 0 || Np < N || (Np % TILE)) return TSVGP_EINVAL;
    if (in_stride < 1 || out_stride < 1) return TSVGP_EINVAL;
    if ((flags & ~TSVGP_LIK_NOCROP) != TSVGP_LIK_ORDINAL) return TSVGP_EINVAL;
    if (!edges || n_edges < 1 || n_edges > TSVGP_ORDINAL_MAX_EDGES) return TSVGP_EINVAL;
    if (!(sigma > 0.0) || !std::isfinite(sigma)) return TSVGP_EINVAL;
    if (Np / TILE > 0x7fffffff) return TSVGP_EINVAL;  // the grid's block count is 31 bits
    hipLaunchKernelGGL(lik_map_ordinal_kernel<T>, dim3((unsigned)(Np / TILE)), dim3(TILE), 0, (hipStream_t)stream, mean, var, Y,
                       in_stride, flags, edges, n_edges, sigma, g0, g1, out_stride, ve_partial, dparam_partial, nonpos_partial, N);
    return launch_status();
}

static bool lmc_shape_ok(int64_t N, int64_t Np, int L, int P) {
    if (N <= 0 || Np < N || Np - N >= TILE || (Np % TILE) || Np / TILE > 0x7fffffff) return false;
    return L >= 1 && L <= TSVGP_MAX_BATCH && P >= 1 && P <= TSVGP_MAX_BATCH;
}

template <typename T>
int lmc_mix(const T* mean_g, const T* var_g, const double* W, T* Fmu, T* Fvar, int32_t* nonpos_partial, int64_t N, int64_t Np, int L,
            int P, void* stream) {
    if (!mean_g || !var_g || !W || !Fmu || !Fvar || !lmc_shape_ok(N, Np, L, P)) return TSVGP_EINVAL;
    const dim3 grid((unsigned)(Np / TILE)), block(TILE);
    if (P <= 8)
        hipLaunchKernelGGL((lmc_mix_kernel<T, 8>), grid, block, 0, (hipStream_t)stream, mean_g, var_g, W, Fmu, Fvar, nonpos_partial, N,
                           L, P);
    else
        hipLaunchKernelGGL((lmc_mix_kernel<T, TSVGP_MAX_BATCH>), grid, block, 0, (hipStream_t)stream, mean_g, var_g, W, Fmu, Fvar,
                           nonpos_partial, N, L, P);
    return launch_status();
}

template <typename T>
int lmc_unmix(const T* g0_f, const T* g1_f, const double* W, int flags, T* g0_g, T* g1_g, const T* mean_g, const T* var_g,
              double* dW_partial, int64_t N, int64_t Np, int L, int P, void* stream) {
    if (!g0_f || !g1_f || !W || !g0_g || !g1_g || !lmc_shape_ok(N, Np, L, P)) return TSVGP_EINVAL;
    if (flags & ~TSVGP_LIK_NOCROP) return TSVGP_EINVAL;
    if (dW_partial && (!mean_g || !var_g)) return TSVGP_EINVAL;
    const dim3 grid((unsigned)(Np / TILE)), block(TILE);
    if (L <= 8)
        hipLaunchKernelGGL((lmc_unmix_kernel<T, 8>), grid, block, 0, (hipStream_t)stream, g0_f, g1_f, W, flags, g0_g, g1_g, mean_g,
                           var_g, dW_partial, N, L, P);
    else
        hipLaunchKernelGGL((lmc_unmix_kernel<T, TSVGP_MAX_BATCH>), grid, block, 0, (hipStream_t)stream, g0_f, g1_f, W, flags, g0_g,
                           g1_g, mean_g, var_g, dW_partial, N, L, P);
    return launch_status();
}

template <typename T>
int lik_map_softmax(const T* mean, const T* var, const T* Y, int flags, int C, int S, const int64_t* rng_state, int64_t row_offset,
                    const T* epsilon, T* g0, T* g1, double* ve_partial, int32_t* nonpos_partial, int64_t N, int64_t Np, void* stream) {
    if (!mean || !var || !Y || !g0 || !g1 || !ve_partial || !nonpos_partial || N <= 0 || Np < N || (Np % TILE)) return TSVGP_EINVAL;
    if ((flags & ~TSVGP_LIK_NOCROP) != TSVGP_LIK_SOFTMAX) return TSVGP_EINVAL;
    if (C < 2 || C > TSVGP_MAX_BATCH || S < 1 || S > TSVGP_MC_MAX_SAMPLES || row_offset < 0) return TSVGP_EINVAL;
    if (!epsilon && !rng_state) return TSVGP_EINVAL;
    const dim3 grid((unsigned)(Np / TILE)), block(256);
    const hipStream_t st = (hipStream_t)stream;
#define TSVGP_SOFTMAX_LAUNCH(QQ)                                                                                              \
    hipLaunchKernelGGL((lik_map_softmax_kernel<T, QQ>), grid, block, 0, st, mean, var, Y, flags, C, S, rng_state, row_offset, \
                       epsilon, g0, g1, ve_partial, nonpos_partial, N)
    if (C <= 4) TSVGP_SOFTMAX_LAUNCH(1);
    else if (C <= 8) TSVGP_SOFTMAX_LAUNCH(2);
    else if (C <= 16) TSVGP_SOFTMAX_LAUNCH(4);
    else TSVGP_SOFTMAX_LAUNCH(8);
#undef TSVGP_SOFTMAX_LAUNCH
    return launch_status();
}

template <typename T>
int lik_map_robustmax(const T* mean, const T* var, const T* Y, int flags, int C, double epsilon, T* g0, T* g1, double* ve_partial,
                      int32_t* nonpos_partial, int64_t N, int64_t Np, void* stream) {
    if (!mean || !var || !Y || !g0 || !g1 || !ve_partial || !nonpos_partial || N <= 0 || Np < N || (Np % TILE)) return TSVGP_EINVAL;
    if ((flags & ~TSVGP_LIK_NOCROP) != TSVGP_LIK_MULTICLASS) return TSVGP_EINVAL;
    if (C < 2 || C > TSVGP_MAX_BATCH || !(epsilon > 0.0 && epsilon < 1.0)) return TSVGP_EINVAL;
    if (Np / TILE > 0x7fffffff) return TSVGP_EINVAL;  // the grid's block count is 31 bits
    // the two values log p(y | f) takes, once, on the host: log(1 - eps) where the labelled latent is the largest, log(eps / (C - 1))
    const double log_hit = std::log(1.0 - epsilon), log_miss = std::log(epsilon / (double)(C - 1));
    hipLaunchKernelGGL(lik_map_robustmax_kernel<T>, dim3((unsigned)(Np / TILE)), dim3(TILE), 0, (hipStream_t)stream, mean, var, Y,
                       flags, C, log_hit, log_miss, g0, g1, ve_partial, nonpos_partial, N);
    return launch_status();
}

template <typename T>
int mc_normals(T* out, int64_t seed, int64_t draw, int64_t row_offset, int64_t S, int64_t N, int C, void* stream) {
    if (!out || S < 1 || S > TSVGP_MC_MAX_SAMPLES || N <= 0 || C < 1 || C > TSVGP_MAX_BATCH || row_offset < 0) return TSVGP_EINVAL;
    const int64_t per_row = S * ((C + 3) / 4);  // <= 2^28 * 8
    if (N > (int64_t)0x7fffffff * 256 / per_row) return TSVGP_EINVAL;  // the grid's block count is 31 bits (and the product cannot wrap)
    const int64_t total = per_row * N, blocks = (total + 255) / 256;
    if (blocks > 0x7fffffff) return TSVGP_EINVAL;
    hipLaunchKernelGGL(mc_normals_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, out, seed, draw, row_offset,
                       S, N, C);
    return launch_status();
}

}  // namespace

extern "C" {

int tsvgp_lik_map_f64(const double* mean, const double* var, const double* Y, int lik, double lik_param, double* g0, double* g1,
                      double* ve_partial, int32_t* nonpos_partial, int64_t N, int64_t Np, int P, void* stream) {
    return lik_map<double>(mean, var, Y, lik, lik_param, g0, g1, ve_partial, nonpos_partial, N, Np, P, stream);
}
int tsvgp_lik_map_f32(const float* mean, const float* var, const float* Y, int lik, double lik_param, float* g0, float* g1,
                      double* ve_partial, int32_t* nonpos_partial, int64_t N, int64_t Np, int P, void* stream) {
    return lik_map<float>(mean, var, Y, lik, lik_param, g0, g1, ve_partial, nonpos_partial, N, Np, P, stream);
}
int tsvgp_lik_map_hetero_f64(const double* mean, const double* var, const double* Y, int flags, double* g0, double* g1,
                             double* ve_partial, int32_t* nonpos_partial, int64_t N, int64_t Np, void* stream) {
    return lik_map_hetero<double>(mean, var, Y, flags, g0, g1, ve_partial, nonpos_partial, N, Np, stream);
}
int tsvgp_lik_map_hetero_f32(const float* mean, const float* var, const float* Y, int flags, float* g0, float* g1,
                             double* ve_partial, int32_t* nonpos_partial, int64_t N, int64_t Np, void* stream) {
    return lik_map_hetero<float>(mean, var, Y, flags, g0, g1, ve_partial, nonpos_partial, N, Np, stream);
}
int tsvgp_diag_site_step_f64(const double* mean, const double* var, const double* Y, int lik, double lik_param, double lr,
                             double* lambda_1, double* lambda_2, double* ve_partial, int32_t* nonpos_partial, int64_t N, int64_t Np,
                             int P, void* stream) {
    return diag_site_step<double>(mean, var, Y, lik, lik_param, lr, lambda_1, lambda_2, nullptr, nullptr, ve_partial, nonpos_partial,
                                  N, Np, P, stream);
}
int tsvgp_diag_site_step_f32(const float* mean, const float* var, const float* Y, int lik, double lik_param, double lr,
                             double* lambda_1, double* lambda_2, float* lambda_1_f32, float* lambda_2_f32, double* ve_partial,
                             int32_t* nonpos_partial, int64_t N, int64_t Np, int P, void* stream) {
    if (!lambda_1_f32 || !lambda_2_f32) return TSVGP_EINVAL;
    return diag_site_step<float>(mean, var, Y, lik, lik_param, lr, lambda_1, lambda_2, lambda_1_f32, lambda_2_f32, ve_partial,
                                 nonpos_partial, N, Np, P, stream);
}
int tsvgp_lik_map_scalar_f64(const double* mean, const double* var, const double* Y, int64_t in_stride, int lik, double param0,
                             double param1, double* g0, double* g1, int64_t out_stride, double* ve_partial, double* dparam_partial,
                             int32_t* nonpos_partial, int64_t N, int64_t Np, void* stream) {
    return lik_map_scalar<double>(mean, var, Y, in_stride, lik, param0, param1, g0, g1, out_stride, ve_partial, dparam_partial,
                                  nonpos_partial, N, Np, stream);
}
int tsvgp_lik_map_ordinal_f64(const double* mean, const double* var, const double* Y, int64_t in_stride, int flags,
                              const double* edges, int n_edges, double sigma, double* g0, double* g1, int64_t out_stride,
                              double* ve_partial, double* dparam_partial, int32_t* nonpos_partial, int64_t N, int64_t Np,
                              void* stream) {
    return lik_map_ordinal<double>(mean, var, Y, in_stride, flags, edges, n_edges, sigma, g0, g1, out_stride, ve_partial,
                                   dparam_partial, nonpos_partial, N, Np, stream);
}
int tsvgp_lik_map_ordinal_f32(const float* mean, const float* var, const float* Y, int64_t in_stride, int flags, const double* edges,
                              int n_edges, double sigma, float* g0, float* g1, int64_t out_stride, double* ve_partial,
                              double* dparam_partial, int32_t* nonpos_partial, int64_t N, int64_t Np, void* stream) {
    return lik_map_ordinal<float>(mean, var, Y, in_stride, flags, edges, n_edges, sigma, g0, g1, out_stride, ve_partial,
                                  dparam_partial, nonpos_partial, N, Np, stream);
}
int tsvgp_lmc_mix_f64(const double* mean_g, const double* var_g, const double* W, double* Fmu, double* Fvar, int32_t* nonpos_partial,
                      int64_t N, int64_t Np, int L, int P, void* stream) {
    return lmc_mix<double>(mean_g, var_g, W, Fmu, Fvar, nonpos_partial, N, Np, L, P, stream);
}
int tsvgp_lmc_mix_f32(const float* mean_g, const float* var_g, const double* W, float* Fmu, float* Fvar, int32_t* nonpos_partial,
                      int64_t N, int64_t Np, int L, int P, void* stream) {
    return lmc_mix<float>(mean_g, var_g, W, Fmu, Fvar, nonpos_partial, N, Np, L, P, stream);
}
int tsvgp_lmc_unmix_f64(const double* g0_f, const double* g1_f, const double* W, int flags, double* g0_g, double* g1_g,
                        const double* mean_g, const double* var_g, double* dW_partial, int64_t N, int64_t Np, int L, int P,
                        void* stream) {
    return lmc_unmix<double>(g0_f, g1_f, W, flags, g0_g, g1_g, mean_g, var_g, dW_partial, N, Np, L, P, stream);
}
int tsvgp_lmc_unmix_f32(const float* g0_f, const float* g1_f, const double* W, int flags, float* g0_g, float* g1_g,
                        const float* mean_g, const float* var_g, double* dW_partial, int64_t N, int64_t Np, int L, int P,
                        void* stream) {
    return lmc_unmix<float>(g0_f, g1_f, W, flags, g0_g, g1_g, mean_g, var_g, dW_partial, N, Np, L, P, stream);
}
int tsvgp_lik_map_scalar_f32(const float* mean, const float* var, const float* Y, int64_t in_stride, int lik, double param0,
                             double param1, float* g0, float* g1, int64_t out_stride, double* ve_partial, double* dparam_partial,
                             int32_t* nonpos_partial, int64_t N, int64_t Np, void* stream) {
    return lik_map_scalar<float>(mean, var, Y, in_stride, lik, param0, param1, g0, g1, out_stride, ve_partial, dparam_partial,
                                 nonpos_partial, N, Np, stream);
}
int tsvgp_lik_map_softmax_f64(const double* mean, const double* var, const double* Y, int flags, int C, int S,
                              const int64_t* rng_state, int64_t row_offset, const double* epsilon, double* g0, double* g1,
                              double* ve_partial, int32_t* nonpos_partial, int64_t N, int64_t Np, void* stream) {
    return lik_map_softmax<double>(mean, var, Y, flags, C, S, rng_state, row_offset, epsilon, g0, g1, ve_partial, nonpos_partial, N,
                                   Np, stream);
}
int tsvgp_lik_map_softmax_f32(const float* mean, const float* var, const float* Y, int flags, int C, int S,
                              const int64_t* rng_state, int64_t row_offset, const float* epsilon, float* g0, float* g1,
                              double* ve_partial, int32_t* nonpos_partial, int64_t N, int64_t Np, void* stream) {
    return lik_map_softmax<float>(mean, var, Y, flags, C, S, rng_state, row_offset, epsilon, g0, g1, ve_partial, nonpos_partial, N,
                                  Np, stream);
}
int tsvgp_lik_map_robustmax_f64(const double* mean, const double* var, const double* Y, int flags, int C, double epsilon, double* g0,
                                double* g1, double* ve_partial, int32_t* nonpos_partial, int64_t N, int64_t Np, void* stream) {
    return lik_map_robustmax<double>(mean, var, Y, flags, C, epsilon, g0, g1, ve_partial, nonpos_partial, N, Np, stream);
}
int tsvgp_lik_map_robustmax_f32(const float* mean, const float* var, const float* Y, int flags, int C, double epsilon, float* g0,
                                float* g1, double* ve_partial, int32_t* nonpos_partial, int64_t N, int64_t Np, void* stream) {
    return lik_map_robustmax<float>(mean, var, Y, flags, C, epsilon, g0, g1, ve_partial, nonpos_partial, N, Np, stream);
}
int tsvgp_mc_normals_f64(double* out, int64_t seed, int64_t draw, int64_t row_offset, int64_t S, int64_t N, int C, void* stream) {
    return mc_normals<double>(out, seed, draw, row_offset, S, N, C, stream);
}
int tsvgp_mc_normals_f32(float* out, int64_t seed, int64_t draw, int64_t row_offset, int64_t S, int64_t N, int C, void* stream) {
    return mc_normals<float>(out, seed, draw, row_offset, S, N, C, stream);
}

}  // extern "C"
