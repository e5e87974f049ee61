// tsvgp_vgp.hip -- the kernels of t_VGP, the exact (N x N) model, for CDNA4 (gfx950 / MI355X), with their launchers and C entry
// points (tsvgp_vgp_system_f64, tsvgp_vgp_rows_f64, tsvgp_vgp_kernel_grad_*).  A translation unit of its own: it shares
// tsvgp_device.h (the kernel profiles, the Gaussian / Bernoulli map, COV_XS) with the E-step kernels of tsvgp_kernels.hip, and
// their object code does not depend on it.  The factorisation between vgp_system_kernel and vgp_rows_kernel is
// tsvgp_potrf_solve_f64 (tsvgp_kernels.hip, tsvgp_chol.hip).
//
// Kernel inventory
//   vgp_system_kernel        B = I + s s^T * K~, the right-hand-side rows K~ s and s y~ in one launch: the stacked operand of the solve.
//   vgp_rows_kernel          moments of the solved rows, likelihood map, ELBO partials and the site update in one sweep.  HBM bound.
//   vgp_kgrad_kernel         the N x N contraction behind d ELBO / d (variance, lengthscales).  HBM bound on the one read of W.
//   vgp_kgrad_reduce_kernel  the totals of its per-tile partials, in a fixed order.

#include <hip/hip_runtime.h>

#include <cmath>
#include <stdint.h>

#include "tsvgp_hip.h"
#include "tsvgp_device.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// t_VGP, the exact N x N model (reference src/models/tvgp.py:72-160).  With s = sqrt|lambda_2|, y~ = lambda_1 / lambda_2 and
// K~ = K(X, X) + jitter I the model factors B = I + s s^T * K~ = L L^T and needs K~ s L^-T and L^-1 (s y~).
// vgp_system_kernel writes, in one launch, the stacked operand tsvgp_potrf_solve_f64 takes:
//     rows [0, Np)        B[i, j] = [i == j] + s_i s_j K~[i, j]     lower block triangle and full diagonal tiles -- what the
//                                                                   factorisation reads (potrf_diag_kernel drops the strict upper
//                                                                   triangle of a diagonal block, chol_tile_kernel<1> updates the
//                                                                   32 x 32 tiles on and below the diagonal); s_n = 0 for n >= N,
//                                                                   so the padding is the identity block
//     rows [Np, 2 Np)     R[n, j] = K~[n, j] s_j                    the right-hand-side rows (both triangles), zero in the padding
//     rows [2 Np, + 128)  row 0: s_j y~_j, the other 127 rows zero
// One workgroup per 128 x 128 tile (it, jt), jt <= it, as cov_kernel; the kernel function is evaluated once per pair, in the
// fill's difference form sum_d (x~_id - x~_jd)^2 in the order of d on inputs pre-scaled by inv_ls (so k(i, j) == k(j, i) bit for
// bit), and an off-diagonal tile also stores the mirror image of its R tile, 16 rows at a time through LDS.  Lane l of wave w
// owns the columns 2 l, 2 l + 1 (16-byte stores, a wave writes one 1 KB row segment) and the rows w, w + 4, .. of a chunk.
// ---------------------------------------------------------------------------------------------------------------
constexpr int VS_CH = 16;          // rows of the tile per pass
constexpr int VS_TS = VS_CH + 1;   // mirror image [128 columns][16 rows]: column stride (odd: 16 lanes of a row hit 16 banks)
struct VgpSysArgs {
    const double* X;       // [N x D]
    const double* inv_ls;  // [D]
    const double* l1;      // [>= N]
    const double* l2;      // [>= N]
    double* S;             // [(2 Np + 128) x lds]
    double variance, jitter;
    int64_t N, Np, lds;
    int D, rows;
};

template <int KIND>
__global__ __launch_bounds__(NTHREADS) void vgp_system_kernel(VgpSysArgs a) {
    __shared__ double xj[TILE * COV_XS];
    __shared__ double xi[VS_CH * COV_XS];
    __shared__ double img[TILE * VS_TS];
    __shared__ double sj[TILE], si[TILE];
    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int bid = blockIdx.x;
    int it = (int)((sqrtf(8.0f * (float)bid + 1.0f) - 1.0f) * 0.5f);
    while ((it + 1) * (it + 2) / 2 <= bid) ++it;
    while (it * (it + 1) / 2 > bid) --it;
    const int jt = bid - it * (it + 1) / 2;
    const bool diag = it == jt;
    const int64_t i0 = (int64_t)it * TILE, j0 = (int64_t)jt * TILE;
    const int D = a.D;

    for (int idx = t; idx < TILE * D; idx += NTHREADS) {
        const int rr = idx / D, d = idx - rr * D;
        const int64_t n = j0 + rr;
        xj[rr * COV_XS + d] = n < a.N ? a.X[n * D + d] * a.inv_ls[d] : 0.0;
    }
    {
        const int r = t & (TILE - 1);
        const int64_t n = (t < TILE ? j0 : i0) + r;
        (t < TILE ? sj : si)[r] = n < a.N ? sqrt(fabs(a.l2[n])) : 0.0;
    }
    __syncthreads();
    const int c = 2 * lane;
    const int64_t gj = j0 + c;
    const double sj0 = sj[c], sj1 = sj[c + 1];
    double* const Bm = a.S;
    double* const Rm = a.S + a.Np * a.lds;

    for (int ch = 0; ch < TILE / VS_CH; ++ch) {
        if (ch) __syncthreads();  // the previous pass has read its rows and its image
        for (int idx = t; idx < VS_CH * D; idx += NTHREADS) {
            const int rr = idx / D, d = idx - rr * D;
            const int64_t n = i0 + ch * VS_CH + rr;
            xi[rr * COV_XS + d] = n < a.N ? a.X[n * D + d] * a.inv_ls[d] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < VS_CH / 4; ++k) {
            const int lr = w + 4 * k, li = ch * VS_CH + lr;
            const int64_t gi = i0 + li;
            double s0 = 0.0, s1 = 0.0;
            for (int d = 0; d < D; ++d) {
                const double x = xi[lr * COV_XS + d];
                const double d0 = x - xj[c * COV_XS + d], d1 = x - xj[(c + 1) * COV_XS + d];
                s0 += d0 * d0;
                s1 += d1 * d1;
            }
            double k0 = a.variance * kernel_profile<KIND>(s0), k1 = a.variance * kernel_profile<KIND>(s1);
            if (gi == gj) k0 += a.jitter;
            if (gi == gj + 1) k1 += a.jitter;
            if (gi >= a.N || gj >= a.N) k0 = 0.0;
            if (gi >= a.N || gj + 1 >= a.N) k1 = 0.0;
            const double sr = si[li];
            v2d b;
            b[0] = (gi == gj ? 1.0 : 0.0) + sr * sj0 * k0;
            b[1] = (gi == gj + 1 ? 1.0 : 0.0) + sr * sj1 * k1;
            *reinterpret_cast<v2d*>(Bm + gi * a.lds + gj) = b;
            if (a.rows) {
                v2d r;
                r[0] = k0 * sj0;
                r[1] = k1 * sj1;
                *reinterpret_cast<v2d*>(Rm + gi * a.lds + gj) = r;
                if (!diag) {
                    img[c * VS_TS + lr] = k0;
                    img[(c + 1) * VS_TS + lr] = k1;
                }
            }
        }
        if (a.rows && !diag) {  // R[j0 + lj, i0 + 16 ch + e] = K~[i, j] s_i: 128 rows of 16 columns
            __syncthreads();
            for (int u = t; u < TILE * VS_CH / 2; u += NTHREADS) {
                const int lj = u >> 3, e = (u & 7) * 2;
                v2d v;
                v[0] = img[lj * VS_TS + e] * si[ch * VS_CH + e];
                v[1] = img[lj * VS_TS + e + 1] * si[ch * VS_CH + e + 1];
                *reinterpret_cast<v2d*>(Rm + (j0 + lj) * a.lds + i0 + ch * VS_CH + e) = v;
            }
        }
    }
    if (a.rows && diag) {  // the row s * y~ and the 127 zero rows below it, this tile's 128 columns
        double* const rrow = a.S + 2 * a.Np * a.lds + j0;
        for (int u = t; u < TILE * TILE / 2; u += NTHREADS) {
            const int r = u >> 6, e = (u & 63) * 2;
            v2d v{0.0, 0.0};
            if (r == 0) {
                if (j0 + e < a.N) v[0] = sj[e] * (a.l1[j0 + e] / a.l2[j0 + e]);
                if (j0 + e + 1 < a.N) v[1] = sj[e + 1] * (a.l1[j0 + e + 1] / a.l2[j0 + e + 1]);
            }
            *reinterpret_cast<v2d*>(rrow + (int64_t)r * a.lds + e) = v;
        }
    }
}

int vgp_system(int kind, const double* X, const double* inv_ls, double variance, double jitter, const double* l1, const double* l2,
               double* S, int64_t N, int64_t Np, int D, int64_t lds, int flags, void* stream) {
    if (flags & ~TSVGP_VGP_NO_ROWS) return TSVGP_EINVAL;
    if (kind != TSVGP_KERNEL_SE && kind != TSVGP_KERNEL_MATERN32 && kind != TSVGP_KERNEL_MATERN52) return TSVGP_EINVAL;
    if (!X || !inv_ls || !l1 || !l2 || !S || N <= 0 || D <= 0 || D > 32) return TSVGP_EINVAL;
    if (Np < N || Np - N >= TILE || (Np % TILE) || Np / TILE > 32768) return TSVGP_EINVAL;
    if (lds < Np || (lds % 2) != 0 || (reinterpret_cast<uintptr_t>(S) & 15) != 0) return TSVGP_EINVAL;
    if (!(jitter >= 0.0)) return TSVGP_EINVAL;
    VgpSysArgs a{};
    a.X = X;
    a.inv_ls = inv_ls;
    a.l1 = l1;
    a.l2 = l2;
    a.S = S;
    a.variance = variance;
    a.jitter = jitter;
    a.N = N;
    a.Np = Np;
    a.lds = lds;
    a.D = D;
    a.rows = (flags & TSVGP_VGP_NO_ROWS) ? 0 : 1;
    const int64_t nt = Np / TILE;
    const dim3 grid((unsigned)(nt * (nt + 1) / 2)), block(NTHREADS);
    if (kind == TSVGP_KERNEL_SE)
        hipLaunchKernelGGL((vgp_system_kernel<TSVGP_KERNEL_SE>), grid, block, 0, (hipStream_t)stream, a);
    else if (kind == TSVGP_KERNEL_MATERN32)
        hipLaunchKernelGGL((vgp_system_kernel<TSVGP_KERNEL_MATERN32>), grid, block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((vgp_system_kernel<TSVGP_KERNEL_MATERN52>), grid, block, 0, (hipStream_t)stream, a);
    return launch_status();
}

// ---------------------------------------------------------------------------------------------------------------
// vgp_rows_kernel: the sweep over the solved rows C = R L^-T [. x ldc] behind the factorisation (reference
// src/models/tvgp.py:135-157): per row n < N
//     q = sum_{i < K} C[n, i]^2,   mean = sum_i C[n, i] z[i],   var = kdiag - q,
// then the likelihood map (never cropped), ve and E_q log t = -1/2 lambda_2 ((y~ - mean)^2 + var) of the OLD sites into
// per-128-row partials, and the site update in place (beta = 0: no store at all).  HBM bound: C is read once.  One workgroup
// per 128 rows; a wave takes 32 of them, eight at a time, lane l the element pairs 2 l + 128 k (16-byte loads, a wave reads 1 KB
// of a row per instruction) with the pair of z loaded once for the eight rows; the lane sums are folded by a butterfly, so the
// order of every sum is fixed by the shape alone.  The epilogue is diag_site_step_kernel's: two threads per row share the
// Bernoulli quadrature.
// ---------------------------------------------------------------------------------------------------------------
constexpr int VR_ROWS = 8;  // rows a wave carries through one sweep of k
struct VgpRowsArgs {
    const double* C;
    const double* z;
    const double* Y;
    double* l1;
    double* l2;
    double* mean;
    double* var;
    double* ve_partial;
    double* eqt_partial;
    int32_t* nonpos_partial;
    double kdiag, lik_param, beta;
    int64_t ldc, N;
    int K, lik;
};

__global__ __launch_bounds__(NTHREADS) void vgp_rows_kernel(VgpRowsArgs a) {
    __shared__ double qs[TILE], ms[TILE];
    __shared__ double red[2][NTHREADS / 64];
    __shared__ int redi[NTHREADS / 64];
    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int64_t r0 = (int64_t)blockIdx.x * TILE;
    for (int g = 0; g < TILE / 4 / VR_ROWS; ++g) {
        const int lrow = w * (TILE / 4) + g * VR_ROWS;
        const double* Cr = a.C + (r0 + lrow) * a.ldc + 2 * lane;
        double q[VR_ROWS], m[VR_ROWS];
#pragma unroll
        for (int r = 0; r < VR_ROWS; ++r) q[r] = m[r] = 0.0;
        for (int k = 2 * lane; k < a.K; k += 128) {
            v2d zz{0.0, 0.0};
            if (a.z) zz = *reinterpret_cast<const v2d*>(a.z + k);
            v2d cv[VR_ROWS];
#pragma unroll
            for (int r = 0; r < VR_ROWS; ++r) cv[r] = *reinterpret_cast<const v2d*>(Cr + r * a.ldc);
#pragma unroll
            for (int r = 0; r < VR_ROWS; ++r) {
                q[r] = fma(cv[r][0], cv[r][0], q[r]);
                q[r] = fma(cv[r][1], cv[r][1], q[r]);
                m[r] = fma(cv[r][0], zz[0], m[r]);
                m[r] = fma(cv[r][1], zz[1], m[r]);
            }
            Cr += 128;
        }
#pragma unroll
        for (int r = 0; r < VR_ROWS; ++r) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                q[r] += __shfl_xor(q[r], o);
                m[r] += __shfl_xor(m[r], o);
            }
            if (lane == 0) {
                qs[lrow + r] = q[r];
                ms[lrow + r] = m[r];
            }
        }
    }
    __syncthreads();

    const int srow = t >> 1, skh = t & 1;
    const int64_t n = r0 + srow;
    const bool live = n < a.N;
    const double mu = (live && a.z) ? ms[srow] : 0.0;
    const double v = live ? a.kdiag - qs[srow] : 1.0;
    double ve_acc = 0.0, eqt_acc = 0.0;
    int nonpos = 0;
    if (a.lik == TSVGP_LIK_NONE) {
        if (live && skh == 0 && (!(v > 0.0) || !(fabs(mu) <= 1.79769313486231570815e308))) nonpos = 1;
    } else {
        double g0 = 0.0, g1 = 0.0, ve = 0.0;
        if (a.lik == TSVGP_LIK_BERNOULLI) {
            double a0, a1, av;
            const double sd = sqrt(v);
            bern_sums_t<double>(mu, sd, live && a.Y[live ? n : 0] == 1.0, skh * 5, skh * 5 + 5, a0, a1, av);
            a0 += __shfl_xor(a0, 1);
            a1 += __shfl_xor(a1, 1);
            av += __shfl_xor(av, 1);
            g0 = a0;
            g1 = a1 / (2.0 * sd);
            ve = av;
        } else if (live) {
            lik_eval(TSVGP_LIK_GAUSSIAN | TSVGP_LIK_NOCROP, a.lik_param, mu, v, a.Y[n], g0, g1, ve);
        }
        if (live && skh == 0) {
            const double o1 = a.l1[n], o2 = a.l2[n];
            const double dy = o1 / o2 - mu;
            ve_acc = ve;
            eqt_acc = -0.5 * o2 * (dy * dy + v);  // tvgp.py:107
            if (!(v > 0.0) || !(fabs(mu) <= 1.79769313486231570815e308) || !(fabs(g0) <= 1.79769313486231570815e308) ||
                !(fabs(g1) <= 1.79769313486231570815e308))
                nonpos = 1;
            if (a.beta != 0.0) {
                a.l1[n] = (1.0 - a.beta) * o1 + a.beta * (g0 - 2.0 * g1 * mu);  // tvgp.py:156
                a.l2[n] = (1.0 - a.beta) * o2 + a.beta * (-2.0 * g1);           // tvgp.py:157
            }
        }
    }
    if (live && skh == 0) {
        if (a.mean) a.mean[n] = mu;
        if (a.var) a.var[n] = v;
    }
    double s = ve_acc, e = eqt_acc;
    int c = nonpos;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o);
        e += __shfl_xor(e, o);
        c += __shfl_xor(c, o);
    }
    if (lane == 0) {
        red[0][w] = s;
        red[1][w] = e;
        redi[w] = c;
    }
    __syncthreads();
    if (t == 0) {
        if (a.ve_partial) a.ve_partial[blockIdx.x] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        if (a.eqt_partial) a.eqt_partial[blockIdx.x] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
        a.nonpos_partial[blockIdx.x] = redi[0] + redi[1] + redi[2] + redi[3];
    }
}

int vgp_rows(const double* C, int64_t ldc, const double* z, const double* Y, double* l1, double* l2, double kdiag, int lik,
             double lik_param, double beta, double* mean, double* var, double* ve_partial, double* eqt_partial,
             int32_t* nonpos_partial, int64_t N, int64_t Np, int K, void* stream) {
    if (!C || !nonpos_partial || N <= 0 || Np < N || Np - N >= TILE || (Np % TILE) || K <= 0 || (K % 2) != 0) return TSVGP_EINVAL;
    if (ldc < K || (ldc % 2) != 0 || (reinterpret_cast<uintptr_t>(C) & 15) != 0 || (reinterpret_cast<uintptr_t>(z) & 15) != 0)
        return TSVGP_EINVAL;
    if (lik != TSVGP_LIK_NONE && lik != TSVGP_LIK_GAUSSIAN && lik != TSVGP_LIK_BERNOULLI) return TSVGP_EINVAL;
    if (lik == TSVGP_LIK_NONE) {
        if (!mean && !var) return TSVGP_EINVAL;
    } else {
        if (!z || !Y || !l1 || !l2 || !ve_partial || !eqt_partial || !(beta >= 0.0 && beta <= 1.0)) return TSVGP_EINVAL;
        if (lik == TSVGP_LIK_GAUSSIAN && !(lik_param > 0.0)) return TSVGP_EINVAL;
    }
    VgpRowsArgs a{};
    a.C = C;
    a.z = z;
    a.Y = Y;
    a.l1 = l1;
    a.l2 = l2;
    a.mean = mean;
    a.var = var;
    a.ve_partial = ve_partial;
    a.eqt_partial = eqt_partial;
    a.nonpos_partial = nonpos_partial;
    a.kdiag = kdiag;
    a.lik_param = lik_param;
    a.beta = beta;
    a.ldc = ldc;
    a.N = N;
    a.K = K;
    a.lik = lik;
    hipLaunchKernelGGL(vgp_rows_kernel, dim3((unsigned)(Np / TILE)), dim3(NTHREADS), 0, (hipStream_t)stream, a);
    return launch_status();
}

// ---------------------------------------------------------------------------------------------------------------
// vgp_kgrad_kernel: the N x N contraction behind d ELBO / d (variance, lengthscales) of t_VGP (models/tvgp.py: elbo_and_grads).
// With G[i, j] = W[i, j] + 1/2 (a_i c_j + c_i a_j) symmetric, x~ = X / lengthscales, s = |x~_i - x~_j|^2 and K = variance f(s):
//     part[tile][0]     = weight * sum_{i, j in tile} G[i, j] f(s)                                      (dK / d variance = f)
//     part[tile][1 + d] = weight * sum_{i, j in tile} G[i, j] variance f'(s) (-2) (x~_id - x~_jd)^2     (= l_d dK / d l_d)
// over the tiles of the lower block triangle, weight = 2 off the diagonal (G and K are symmetric; only the tiles vgp_system_kernel
// writes are read), f and f' from kernel_profile_grad as kgrad_kernel.  G is formed in registers: no N x N x D array and no second
// N x N buffer.  HBM bound on the one read of W: lane l of wave w owns the columns 2 l, 2 l + 1 (16-byte loads, a wave reads one
// 1 KB row segment per instruction) and the rows w, w + 4, ..; the column panel of x~ sits in LDS, the row's x~ is a wave-uniform
// LDS read.  A pair with i >= N or j >= N is masked by a select (whatever W holds there, NaN included), a, c and X are not read
// beyond N.  Every sum has an order fixed by the shape: lane sums, a butterfly, the four waves in order; vgp_kgrad_reduce_kernel
// then adds the tiles' partials in a fixed order (256 strided chains, a tree over them).  No atomics.
// DT = D padded to a compile-time size (padded dimensions are zeros on both sides).
// ---------------------------------------------------------------------------------------------------------------
struct VgpKgradArgs {
    const double* X;       // [N x D]
    const double* inv_ls;  // [D]
    const double* W;       // [Np x ldw]
    const double* a;       // [>= N]
    const double* c;       // [>= N]
    double* part;          // [(ntiles + 1) x (1 + DT)]
    double variance;
    int64_t N, ldw;
    int D;
};

template <int KIND, int DT>
__global__ __launch_bounds__(NTHREADS) void vgp_kgrad_kernel(VgpKgradArgs a) {
    constexpr int XS = DT + 1;  // odd row stride (DT >= 2): a wave's 64 column reads spread over the banks
    constexpr int VG_CH = 64;   // rows of x~ staged per pass (with DT = 32 the two full panels would not fit 64 KB of LDS)
    __shared__ double xj[TILE * XS];
    __shared__ double xi[VG_CH * DT];  // wave-uniform reads: no padding needed
    __shared__ double aj[TILE], cj[TILE], ai[TILE], ci[TILE];
    __shared__ double red[NTHREADS / 64][DT + 1];
    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int bid = blockIdx.x;
    int it = (int)((sqrtf(8.0f * (float)bid + 1.0f) - 1.0f) * 0.5f);
    while ((it + 1) * (it + 2) / 2 <= bid) ++it;
    while (it * (it + 1) / 2 > bid) --it;
    const int jt = bid - it * (it + 1) / 2;
    const int64_t i0 = (int64_t)it * TILE, j0 = (int64_t)jt * TILE;
    const int D = a.D;

    for (int idx = t; idx < TILE * DT; idx += NTHREADS) {
        const int rr = idx / DT, d = idx - rr * DT;
        const int64_t nj = j0 + rr;
        xj[rr * XS + d] = (d < D && nj < a.N) ? a.X[nj * D + d] * a.inv_ls[d] : 0.0;
    }
    if (t < TILE) {
        const int64_t nj = j0 + t, ni = i0 + t;
        aj[t] = nj < a.N ? a.a[nj] : 0.0;
        cj[t] = nj < a.N ? a.c[nj] : 0.0;
        ai[t] = ni < a.N ? a.a[ni] : 0.0;
        ci[t] = ni < a.N ? a.c[ni] : 0.0;
    }
    __syncthreads();

    const int c = 2 * lane;
    const int64_t gj = j0 + c;
    const bool live0 = gj < a.N, live1 = gj + 1 < a.N;
    const double a0 = aj[c], a1 = aj[c + 1], c0 = cj[c], c1 = cj[c + 1];
    double acc[DT + 1];
#pragma unroll
    for (int d = 0; d <= DT; ++d) acc[d] = 0.0;
    const double m2v = -2.0 * a.variance;

    for (int ch = 0; ch < TILE / VG_CH; ++ch) {
        if (ch) __syncthreads();  // the previous pass has read its rows
        for (int idx = t; idx < VG_CH * DT; idx += NTHREADS) {
            const int rr = idx / DT, d = idx - rr * DT;
            const int64_t ni = i0 + ch * VG_CH + rr;
            xi[idx] = (d < D && ni < a.N) ? a.X[ni * D + d] * a.inv_ls[d] : 0.0;
        }
        __syncthreads();
        for (int lr = w; lr < VG_CH; lr += 4) {
            const int li = ch * VG_CH + lr;
            const int64_t gi = i0 + li;
            if (gi >= a.N) break;  // wave-uniform (the rows of a wave ascend); no barrier inside this loop
            const v2d wv = *reinterpret_cast<const v2d*>(a.W + gi * a.ldw + gj);
            const double ar = ai[li], cr = ci[li];
            const double g0 = live0 ? wv[0] + 0.5 * (ar * c0 + cr * a0) : 0.0;
            const double g1 = live1 ? wv[1] + 0.5 * (ar * c1 + cr * a1) : 0.0;
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int d = 0; d < DT; ++d) {
                const double x = xi[lr * DT + d];
                const double d0 = x - xj[c * XS + d], d1 = x - xj[(c + 1) * XS + d];
                s0 += d0 * d0;
                s1 += d1 * d1;
            }
            double f0, df0, f1, df1;
            kernel_profile_grad<KIND>(s0, f0, df0);
            kernel_profile_grad<KIND>(s1, f1, df1);
            acc[0] += g0 * f0 + g1 * f1;
            const double q0 = g0 * m2v * df0, q1 = g1 * m2v * df1;
#pragma unroll
            for (int d = 0; d < DT; ++d) {
                const double x = xi[lr * DT + d];
                const double d0 = x - xj[c * XS + d], d1 = x - xj[(c + 1) * XS + d];
                acc[1 + d] += q0 * (d0 * d0) + q1 * (d1 * d1);
            }
        }
    }
#pragma unroll
    for (int d = 0; d <= DT; ++d) {
        double v = acc[d];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) red[w][d] = v;
    }
    __syncthreads();
    if (t <= DT) {
        const double v = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
        a.part[(int64_t)bid * (DT + 1) + t] = (it == jt ? 1.0 : 2.0) * v;
    }
}

// the totals of the tiles' partials, row ntiles of part: one workgroup per column, thread t the tiles t, t + 256, .. in order
__global__ __launch_bounds__(NTHREADS) void vgp_kgrad_reduce_kernel(double* part, int64_t ntiles, int cols) {
    __shared__ double red[NTHREADS];
    const int t = threadIdx.x, col = blockIdx.x;
    double v = 0.0;
    for (int64_t k = t; k < ntiles; k += NTHREADS) v += part[k * cols + col];
    red[t] = v;
    __syncthreads();
    for (int o = NTHREADS / 2; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) part[ntiles * cols + col] = red[0];
}

inline int vgp_kgrad_dpad(int D) { return D <= 1 ? 1 : D <= 2 ? 2 : D <= 4 ? 4 : D <= 8 ? 8 : D <= 16 ? 16 : 32; }

template <int KIND>
void vgp_kgrad_launch(const VgpKgradArgs& a, int DT, dim3 grid, hipStream_t st) {
    const dim3 block(NTHREADS);
    switch (DT) {
        case 1: hipLaunchKernelGGL((vgp_kgrad_kernel<KIND, 1>), grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL((vgp_kgrad_kernel<KIND, 2>), grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL((vgp_kgrad_kernel<KIND, 4>), grid, block, 0, st, a); break;
        case 8: hipLaunchKernelGGL((vgp_kgrad_kernel<KIND, 8>), grid, block, 0, st, a); break;
        case 16: hipLaunchKernelGGL((vgp_kgrad_kernel<KIND, 16>), grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL((vgp_kgrad_kernel<KIND, 32>), grid, block, 0, st, a); break;
    }
}

int vgp_kernel_grad(int kind, const double* X, const double* inv_ls, double variance, const double* W, int64_t ldw, const double* av,
                    const double* cv, int64_t N, int64_t Np, int D, double* part, void* stream) {
    if (kind != TSVGP_KERNEL_SE && kind != TSVGP_KERNEL_MATERN32 && kind != TSVGP_KERNEL_MATERN52) return TSVGP_EINVAL;
    if (!X || !inv_ls || !W || !av || !cv || !part || N <= 0 || D <= 0 || D > 32) return TSVGP_EINVAL;
    if (Np < N || Np - N >= TILE || (Np % TILE) || Np / TILE > 32768) return TSVGP_EINVAL;
    if (ldw < Np || (ldw % 2) != 0 || (reinterpret_cast<uintptr_t>(W) & 15) != 0) return TSVGP_EINVAL;
    VgpKgradArgs a{};
    a.X = X;
    a.inv_ls = inv_ls;
    a.W = W;
    a.a = av;
    a.c = cv;
    a.part = part;
    a.variance = variance;
    a.N = N;
    a.ldw = ldw;
    a.D = D;
    const int DT = vgp_kgrad_dpad(D);
    const int64_t nt = Np / TILE, ntiles = nt * (nt + 1) / 2;
    const dim3 grid((unsigned)ntiles);
    hipStream_t st = (hipStream_t)stream;
    if (kind == TSVGP_KERNEL_SE)
        vgp_kgrad_launch<TSVGP_KERNEL_SE>(a, DT, grid, st);
    else if (kind == TSVGP_KERNEL_MATERN32)
        vgp_kgrad_launch<TSVGP_KERNEL_MATERN32>(a, DT, grid, st);
    else
        vgp_kgrad_launch<TSVGP_KERNEL_MATERN52>(a, DT, grid, st);
    if (hipGetLastError() != hipSuccess) return TSVGP_ELAUNCH;
    hipLaunchKernelGGL(vgp_kgrad_reduce_kernel, dim3((unsigned)(DT + 1)), dim3(NTHREADS), 0, st, part, ntiles, DT + 1);
    return launch_status();
}

}  // namespace

extern "C" {

int tsvgp_vgp_system_f64(int kind, const double* X, const double* inv_ls, double variance, double jitter, const double* lambda_1,
                         const double* lambda_2, double* S, int64_t N, int64_t Np, int D, int64_t lds, int flags, void* stream) {
    return vgp_system(kind, X, inv_ls, variance, jitter, lambda_1, lambda_2, S, N, Np, D, lds, flags, stream);
}
int tsvgp_vgp_rows_f64(const double* C, int64_t ldc, const double* z, const double* Y, double* lambda_1, double* lambda_2,
                       double kdiag, int lik, double lik_param, double beta, double* mean, double* var, double* ve_partial,
                       double* eqt_partial, int32_t* nonpos_partial, int64_t N, int64_t Np, int K, void* stream) {
    return vgp_rows(C, ldc, z, Y, lambda_1, lambda_2, kdiag, lik, lik_param, beta, mean, var, ve_partial, eqt_partial,
                    nonpos_partial, N, Np, K, stream);
}
// part: one row of 1 + Dp doubles per tile of the lower block triangle, and one more for the totals
int64_t tsvgp_vgp_kernel_grad_parts(int64_t Np, int D) {
    if (Np <= 0 || (Np % TILE) || Np / TILE > 32768 || D <= 0 || D > 32) return -1;
    const int64_t nt = Np / TILE;
    return (nt * (nt + 1) / 2 + 1) * (1 + vgp_kgrad_dpad(D));
}
int tsvgp_vgp_kernel_grad_f64(int kind, const double* X, const double* inv_ls, double variance, const double* W, int64_t ldw,
                              const double* a, const double* c, int64_t N, int64_t Np, int D, double* part, void* stream) {
    return vgp_kernel_grad(kind, X, inv_ls, variance, W, ldw, a, c, N, Np, D, part, stream);
}

}  // extern "C"
