// tsvgp_grad.hip -- the hyperparameter gradients of the sparse models (the M-step's N-sized contractions) for CDNA4 (gfx950 /
// MI355X), with their launchers and C entry points (tsvgp_kernel_grad_*, tsvgp_gram_to_gradw_*).  A translation unit of its own:
// it shares tsvgp_device.h (the kernel profiles, FILL_COLS) and tsvgp_mfma.h (Mfma<T>::pair_t) with the E-step kernels of
// tsvgp_kernels.hip, and their object code does not depend on it.
//
// Kernel inventory
//   kgrad_kernel          kernel-parameter gradient contraction of the M-step (D <= 16).  HBM bound.
//   gram_to_gradw_kernel  the same contraction in GEMM form for D > 16: turns the Gram block into W in place.

#include <hip/hip_runtime.h>

#include <cmath>
#include <stdint.h>

#include "tsvgp_hip.h"
#include "tsvgp_device.h"
#include "tsvgp_mfma.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// kgrad_kernel: the N-sized part of d ELBO / d (variance, lengthscales, Z) for one latent GP (M-step, reference
// experiments/uci_regression.py:159-160).  With s = sum_d s_d^2, s_d = (x_nd - z_md) / l_d and K = variance * f(s):
//   V[n, m]  = g0[n] * beta[m] - 2 * g1[n] * U[n, m]                       (U = K_fu Q, a tsvgp_trmm product)
//   dvar    += V * f(s)
//   dls[d]  += V * variance * f'(s) * (-2 s_d^2 / l_d)
//   dZ[m,d] += V * variance * f'(s) * (-2 s_d   / l_d)
// f'(s) in closed form: SE -f/2;  Matern-3/2 -(3/2) e^-a, a = sqrt(3 s);  Matern-5/2 -(5/6)(1 + a) e^-a, a = sqrt(5 s).
// HBM bound (one read of U).  Grid (row blocks of KG_ROWS, column tiles of FILL_COLS); thread = two columns, its dZ sums
// stay in registers over the block's rows; per-block partials are written out and summed by the caller in a fixed order
// (bitwise reproducible, no atomics).  DT = D padded to a compile-time size (padded dimensions contribute zeros).
// ---------------------------------------------------------------------------------------------------------------
constexpr int KG_ROWS = 1024;
constexpr int KG_CHUNK = 64;

template <typename T, int KIND, int DT>
__global__ __launch_bounds__(NTHREADS) void kgrad_kernel(const T* __restrict__ X, const T* __restrict__ Z,
                                                         const T* __restrict__ inv_ls, T variance,
                                                         const T* __restrict__ U, int64_t ldu, const T* __restrict__ g0,
                                                         const T* __restrict__ g1, int gstride,
                                                         const T* __restrict__ beta, int bstride, int64_t N, int M, int D,
                                                         double* __restrict__ zpart, double* __restrict__ lpart,
                                                         double* __restrict__ vpart, int Mp) {
    __shared__ T Xs[KG_CHUNK][DT];
    __shared__ T Gs[KG_CHUNK][2];
    __shared__ double red[NTHREADS / 64][DT + 1];
    typedef typename Mfma<T>::pair_t pair_t;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t n0 = (int64_t)blockIdx.x * KG_ROWS;
    const int m0 = blockIdx.y * FILL_COLS + 2 * t;
    const bool c0 = m0 < M, c1 = m0 + 1 < M;
    T z[2][DT], il[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) {
        il[d] = d < D ? inv_ls[d] : T(0);
        z[0][d] = (c0 && d < D) ? Z[(int64_t)m0 * D + d] * il[d] : T(0);
        z[1][d] = (c1 && d < D) ? Z[(int64_t)(m0 + 1) * D + d] * il[d] : T(0);
    }
    const T b0 = c0 ? beta[(int64_t)m0 * bstride] : T(0), b1 = c1 ? beta[(int64_t)(m0 + 1) * bstride] : T(0);
    double za[2][DT], la[DT], va = 0.0;
#pragma unroll
    for (int d = 0; d < DT; ++d) za[0][d] = za[1][d] = la[d] = 0.0;
    const int64_t nend = (n0 + KG_ROWS < N) ? n0 + KG_ROWS : N;
    for (int64_t nc = n0; nc < nend; nc += KG_CHUNK) {
        __syncthreads();
        for (int idx = t; idx < KG_CHUNK * DT; idx += NTHREADS) {
            const int rr = idx / DT, d = idx - rr * DT;
            const int64_t n = nc + rr;
            Xs[rr][d] = (n < nend && d < D) ? X[n * D + d] * inv_ls[d] : T(0);
        }
        if (t < KG_CHUNK) {
            const int64_t n = nc + t;
            Gs[t][0] = n < nend ? g0[n * gstride] : T(0);
            Gs[t][1] = n < nend ? g1[n * gstride] : T(0);
        }
        __syncthreads();
        const int nr = (int)((nend - nc < KG_CHUNK) ? nend - nc : KG_CHUNK);
        if (c0) {
#pragma unroll 2
            for (int rr = 0; rr < nr; ++rr) {
                const pair_t u = *reinterpret_cast<const pair_t*>(U + (nc + rr) * ldu + m0);
                const T gg0 = Gs[rr][0], gg1 = Gs[rr][1];
                T sd[2][DT], s0 = T(0), s1 = T(0);
#pragma unroll
                for (int d = 0; d < DT; ++d) {
                    const T x = Xs[rr][d];
                    sd[0][d] = x - z[0][d];
                    sd[1][d] = x - z[1][d];
                    s0 += sd[0][d] * sd[0][d];
                    s1 += sd[1][d] * sd[1][d];
                }
                T f0, df0, f1, df1;
                kernel_profile_grad<KIND>(s0, f0, df0);
                kernel_profile_grad<KIND>(s1, f1, df1);
                const T v0 = gg0 * b0 - T(2) * gg1 * u[0];
                const T v1 = c1 ? gg0 * b1 - T(2) * gg1 * u[1] : T(0);
                va += (double)(v0 * f0) + (double)(v1 * f1);
                const T w0 = T(-2) * variance * v0 * df0, w1 = T(-2) * variance * v1 * df1;
#pragma unroll
                for (int d = 0; d < DT; ++d) {
                    const T p0 = w0 * sd[0][d], p1 = w1 * sd[1][d];
                    za[0][d] += (double)p0;  // times 1 / l_d below
                    za[1][d] += (double)p1;
                    la[d] += (double)(p0 * sd[0][d]) + (double)(p1 * sd[1][d]);
                }
            }
        }
    }
    // dZ partials: this thread's two columns
    const int64_t zb = ((int64_t)blockIdx.x * Mp) * DT;
#pragma unroll
    for (int d = 0; d < DT; ++d) {
        if (c0) zpart[zb + (int64_t)m0 * DT + d] = za[0][d] * (double)il[d];
        if (c1) zpart[zb + (int64_t)(m0 + 1) * DT + d] = za[1][d] * (double)il[d];
    }
    // lengthscale / variance partials: sum over the workgroup's threads
#pragma unroll
    for (int d = 0; d <= DT; ++d) {
        double v = d < DT ? la[d < DT ? d : 0] * (double)il[d < DT ? d : 0] : va;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) red[w][d] = v;
    }
    __syncthreads();
    if (t <= DT) {
        double v = 0.0;
        for (int u = 0; u < NTHREADS / 64; ++u) v += red[u][t];
        const int64_t blk = (int64_t)blockIdx.x * gridDim.y + blockIdx.y;
        if (t < DT)
            lpart[blk * DT + t] = v;
        else
            vpart[blk] = v;
    }
}

// M-step gradient for input dimensions beyond kgrad_kernel's compile-time sizes (D > 16): the contraction with dK/d(theta, Z)
// in the same GEMM form as the fill (gram_to_kernel_kernel, tsvgp_kernels.hip).  With s = |x~|^2 + |z~|^2 - 2 G (G = x~ z~^T from
// the BLAS library), V = g0 beta^T - 2 g1 * U and W = -2 variance V * k'(s), everything N-sized that is left is
//     d variance = sum V k(s);    W^T x~ [M, D], the row and column sums of W     (BLAS GEMM + two reductions, on the host side)
// and dZ, d lengthscales follow in M x D (estep.kernel_grad).  This kernel turns G into W IN PLACE (padding zero) and writes
// one partial sum of V k(s) per workgroup.  One thread per two adjacent columns, one row per blockIdx.y.
template <typename T, int KIND>
__global__ __launch_bounds__(NTHREADS) void gram_to_gradw_kernel(T* __restrict__ G, const T* __restrict__ xx,
                                                                 const T* __restrict__ zz, T variance, const T* __restrict__ U,
                                                                 int64_t ldu, const T* __restrict__ g0, const T* __restrict__ g1,
                                                                 int gstride, const T* __restrict__ beta, int bstride, int64_t N,
                                                                 int M, int64_t ldk, int64_t rows_pad, int cols_pad,
                                                                 double* __restrict__ vpart) {
    typedef typename Mfma<T>::pair_t pair_t;
    __shared__ double red[NTHREADS / 64];
    const int64_t n = blockIdx.y;
    const int m = (blockIdx.x * NTHREADS + threadIdx.x) * 2;
    double va = 0.0;
    if (n < rows_pad && m < cols_pad) {
        pair_t* p = reinterpret_cast<pair_t*>(G + n * ldk + m);
        pair_t out;
        out[0] = out[1] = T(0);
        if (n < N) {
            const pair_t g = *p;
            const pair_t u = *reinterpret_cast<const pair_t*>(U + n * ldu + m);
            const T x = xx[n], gg0 = g0[n * gstride], gg1 = g1[n * gstride];
#pragma unroll
            for (int q = 0; q < 2; ++q)
                if (m + q < M) {
                    T f, df;
                    kernel_profile_grad<KIND>(x + zz[m + q] - T(2) * g[q], f, df);
                    const T v = gg0 * beta[(int64_t)(m + q) * bstride] - T(2) * gg1 * u[q];
                    va += (double)(v * f);
                    out[q] = T(-2) * variance * v * df;
                }
        }
        *p = out;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) va += __shfl_xor(va, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = va;
    __syncthreads();
    if (threadIdx.x == 0) vpart[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

template <typename T>
int gram_to_gradw(int kind, T* G, const T* xx, const T* zz, T variance, const T* U, int64_t ldu, const T* g0, const T* g1,
                  int gstride, const T* beta, int bstride, int64_t N, int M, int64_t ldk, double* vpart, void* stream) {
    if (!G || !xx || !zz || !U || !g0 || !g1 || !beta || !vpart || N <= 0 || M <= 0 || gstride <= 0 || bstride <= 0 ||
        (kind != TSVGP_KERNEL_SE && kind != TSVGP_KERNEL_MATERN32 && kind != TSVGP_KERNEL_MATERN52))
        return TSVGP_EINVAL;
    const int64_t rows_pad = (N + TILE - 1) / TILE * TILE;
    const int cols_pad = (M + TILE - 1) / TILE * TILE;
    if (ldk < cols_pad || (ldk % 2) != 0 || ldu < cols_pad || (ldu % 2) != 0 || rows_pad > 0x7fffffff) return TSVGP_EINVAL;
    // a thread moves its two columns of G and of U as one vector each (m, ldk, ldu even): 16 bytes in fp64, 8 in fp32
    if ((reinterpret_cast<uintptr_t>(G) & (2 * sizeof(T) - 1)) != 0 || (reinterpret_cast<uintptr_t>(U) & (2 * sizeof(T) - 1)) != 0)
        return TSVGP_EINVAL;
    const dim3 block(NTHREADS);
    const unsigned gx = (unsigned)((cols_pad / 2 + NTHREADS - 1) / NTHREADS);
    for (int64_t r0 = 0; r0 < rows_pad; r0 += 65535) {
        const unsigned gy = (unsigned)((rows_pad - r0 < 65535) ? rows_pad - r0 : 65535);
        const int64_t Nr = N - r0 > 0 ? N - r0 : 0;
        const int64_t ro = r0 < N ? r0 : 0;  // rows past N are only zero-filled: no per-row operand is read
#define TSVGP_G2W(KIND_)                                                                                                         \
    hipLaunchKernelGGL((gram_to_gradw_kernel<T, KIND_>), dim3(gx, gy), block, 0, (hipStream_t)stream, G + r0 * ldk, xx + ro, zz,  \
                       variance, U + ro * ldu, ldu, g0 + ro * gstride, g1 + ro * gstride, gstride, beta, bstride, Nr, M, ldk,      \
                       (int64_t)gy, cols_pad, vpart + r0 * gx)
        if (kind == TSVGP_KERNEL_SE) TSVGP_G2W(TSVGP_KERNEL_SE);
        else if (kind == TSVGP_KERNEL_MATERN32) TSVGP_G2W(TSVGP_KERNEL_MATERN32);
        else TSVGP_G2W(TSVGP_KERNEL_MATERN52);
#undef TSVGP_G2W
    }
    return launch_status();
}

template <typename T>
int kernel_grad(int kind, const T* X, const T* Z, const T* inv_ls, T variance, const T* U, int64_t ldu, const T* g0,
                const T* g1, int gstride, const T* beta, int bstride, int64_t N, int M, int D, double* zpart,
                double* lpart, double* vpart, void* stream) {
    if (!X || !Z || !inv_ls || !U || !g0 || !g1 || !beta || !zpart || !lpart || !vpart || N <= 0 || M <= 0 || D <= 0 ||
        D > 16 || gstride <= 0 || bstride <= 0 || (ldu % 2) != 0)
        return TSVGP_EINVAL;
    if (kind != TSVGP_KERNEL_SE && kind != TSVGP_KERNEL_MATERN32 && kind != TSVGP_KERNEL_MATERN52) return TSVGP_EINVAL;
    const int Mp = (M + TILE - 1) / TILE * TILE;
    if (ldu < Mp) return TSVGP_EINVAL;
    const dim3 grid((unsigned)((N + KG_ROWS - 1) / KG_ROWS), (unsigned)((Mp + FILL_COLS - 1) / FILL_COLS));
    hipStream_t st = (hipStream_t)stream;
    const int DT = D <= 1 ? 1 : D <= 2 ? 2 : D <= 4 ? 4 : D <= 8 ? 8 : 16;
    if (hipMemsetAsync(zpart, 0, sizeof(double) * (size_t)grid.x * Mp * DT, st) != hipSuccess) return TSVGP_ELAUNCH;
#define TSVGP_KG_LAUNCH(KIND_, DT_)                                                                                  \
    hipLaunchKernelGGL((kgrad_kernel<T, KIND_, DT_>), grid, dim3(NTHREADS), 0, st, X, Z, inv_ls, variance, U, ldu, g0, g1, \
                       gstride, beta, bstride, N, M, D, zpart, lpart, vpart, Mp)
#define TSVGP_KG_DT(KIND_)                          \
    switch (DT) {                                   \
        case 1: TSVGP_KG_LAUNCH(KIND_, 1); break;   \
        case 2: TSVGP_KG_LAUNCH(KIND_, 2); break;   \
        case 4: TSVGP_KG_LAUNCH(KIND_, 4); break;   \
        case 8: TSVGP_KG_LAUNCH(KIND_, 8); break;   \
        default: TSVGP_KG_LAUNCH(KIND_, 16); break; \
    }
    if (kind == TSVGP_KERNEL_SE) {
        TSVGP_KG_DT(TSVGP_KERNEL_SE)
    } else if (kind == TSVGP_KERNEL_MATERN32) {
        TSVGP_KG_DT(TSVGP_KERNEL_MATERN32)
    } else {
        TSVGP_KG_DT(TSVGP_KERNEL_MATERN52)
    }
#undef TSVGP_KG_DT
#undef TSVGP_KG_LAUNCH
    return launch_status();
}

// ---------------------------------------------------------------------------------------------------------------
// kgrad_prod_kernel: the same contraction for a PRODUCT of C stationary kernels, K = variance * prod_c f_c(s_c) with
// variance = prod_c variance_c and s_c = sum_d s_cd^2, s_cd = (x_nd - z_md) * inv_ls[c, d] -- all C parameter sets in ONE pass
// over U.  With V as above and P_c = prod_{c' != c} f_c'(s_c'):
//   vsum      += V * prod_c f_c                          (d / d variance_c = (variance / variance_c) * vsum: the caller's)
//   w_c        = -2 * variance * V * P_c * f_c'(s_c)
//   dls[c, d] += w_c * s_cd^2 * inv_ls[c, d]
//   dZ[m, d]  += sum_c w_c * s_cd * inv_ls[c, d]
// P_c comes from running prefix and suffix products, never from a division by f_c (a profile can flush to zero in fp32).
// Geometry of kgrad_kernel: KG_ROWS-row blocks, KG_CHUNK-row chunks staged in LDS, two columns per thread, one 16-byte read of U
// per row, per-block partials (lpart [nrb x ncb x C x DT]), fp64 accumulation, no atomics.
// What differs is how the C scalings are held.  C pre-scaled copies of the thread's Z columns would take 2 * C * DT registers
// (256 VGPRs at C = 4, DT = 16 in fp64) beside the C * DT lengthscale sums; instead X is staged and Z is kept UNSCALED, the
// difference x_d - z_d is formed once per row and column, and component c multiplies it by inv_ls[c, d] (read from LDS at a
// wave-uniform address) where the pre-scaled form subtracts: one multiply for one subtract, 2 * DT registers of Z for any C.
// The kind of a component is uniform over the launch: a scalar branch per component picks the profile.
// ---------------------------------------------------------------------------------------------------------------
struct ProdGradKinds {
    int kind[TSVGP_MAX_COMPONENTS];
};

template <typename T>
__device__ __forceinline__ void prod_profile_grad(int kind, T s, T& f, T& df) {
    if (kind == TSVGP_KERNEL_SE) kernel_profile_grad<TSVGP_KERNEL_SE>(s, f, df);
    else if (kind == TSVGP_KERNEL_MATERN32) kernel_profile_grad<TSVGP_KERNEL_MATERN32>(s, f, df);
    else kernel_profile_grad<TSVGP_KERNEL_MATERN52>(s, f, df);
}

template <typename T, int DT, int C, int QS>
__global__ __launch_bounds__(NTHREADS) void kgrad_prod_kernel(const T* __restrict__ X, const T* __restrict__ Z,
                                                              const T* __restrict__ inv_ls, ProdGradKinds kinds, T variance,
                                                              const T* __restrict__ U, int64_t ldu, const T* __restrict__ g0,
                                                              const T* __restrict__ g1, int gstride,
                                                              const T* __restrict__ beta, int bstride, int64_t N, int M, int D,
                                                              double* __restrict__ zpart, double* __restrict__ lpart,
                                                              double* __restrict__ vpart, int Mp) {
    static_assert(QS == 1 || QS == 2, "columns per pass");
    __shared__ T Xs[KG_CHUNK][DT];  // unscaled
    __shared__ T Gs[KG_CHUNK][2];
    __shared__ T Il[C][DT];         // inv_ls, zero in the padded dimensions
    __shared__ double red[NTHREADS / 64][C * DT + 1];
    typedef typename Mfma<T>::pair_t pair_t;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t n0 = (int64_t)blockIdx.x * KG_ROWS;
    const int m0 = blockIdx.y * FILL_COLS + 2 * t;
    if (t < C * DT) {
        const int c = t / DT, d = t - c * DT;
        Il[c][d] = d < D ? inv_ls[c * D + d] : T(0);
    }
    double la[C][DT], va = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int d = 0; d < DT; ++d) la[c][d] = 0.0;
    const int64_t nend = (n0 + KG_ROWS < N) ? n0 + KG_ROWS : N;
    const int64_t zb = ((int64_t)blockIdx.x * Mp) * DT;
    // QS = 2: one pass over the block's rows on both columns; QS = 1: two passes, one column each
#pragma unroll 1
    for (int mq = m0; mq < m0 + 2; mq += QS) {
        bool cv[QS];
        T z[QS][DT], b[QS];
        double za[QS][DT];
#pragma unroll
        for (int j = 0; j < QS; ++j) {
            cv[j] = mq + j < M;
            b[j] = cv[j] ? beta[(int64_t)(mq + j) * bstride] : T(0);
#pragma unroll
            for (int d = 0; d < DT; ++d) {
                z[j][d] = (cv[j] && d < D) ? Z[(int64_t)(mq + j) * D + d] : T(0);
                za[j][d] = 0.0;
            }
        }
        for (int64_t nc = n0; nc < nend; nc += KG_CHUNK) {
            __syncthreads();  // (the first: Il is written)
            for (int idx = t; idx < KG_CHUNK * DT; idx += NTHREADS) {
                const int rr = idx / DT, d = idx - rr * DT;
                const int64_t n = nc + rr;
                Xs[rr][d] = (n < nend && d < D) ? X[n * D + d] : T(0);
            }
            if (t < KG_CHUNK) {
                const int64_t n = nc + t;
                Gs[t][0] = n < nend ? g0[n * gstride] : T(0);
                Gs[t][1] = n < nend ? g1[n * gstride] : T(0);
            }
            __syncthreads();
            const int nr = (int)((nend - nc < KG_CHUNK) ? nend - nc : KG_CHUNK);
            if (cv[0]) {
                for (int rr = 0; rr < nr; ++rr) {
                    // Il is read from LDS where it is used, in both sweeps over the components: held in registers across the rows
                    // (C * DT values, which the compiler hoists when left to itself) it costs what keeping Z unscaled saves
                    asm volatile("" ::: "memory");
                    T u[QS];
                    if constexpr (QS == 2) {
                        const pair_t uu = *reinterpret_cast<const pair_t*>(U + (nc + rr) * ldu + mq);
                        u[0] = uu[0];
                        u[1] = uu[1];
                    } else {
                        u[0] = U[(nc + rr) * ldu + mq];
                    }
                    const T gg0 = Gs[rr][0], gg1 = Gs[rr][1];
                    T df[QS][DT];  // x_d - z_d
#pragma unroll
                    for (int d = 0; d < DT; ++d) {
                        const T x = Xs[rr][d];
#pragma unroll
                        for (int j = 0; j < QS; ++j) df[j][d] = x - z[j][d];
                    }
                    T f[C][QS], dfs[C][QS];
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        T s[QS];
#pragma unroll
                        for (int j = 0; j < QS; ++j) s[j] = T(0);
#pragma unroll
                        for (int d = 0; d < DT; ++d) {
                            const T il = Il[c][d];
#pragma unroll
                            for (int j = 0; j < QS; ++j) {
                                const T a = df[j][d] * il;
                                s[j] += a * a;
                            }
                        }
#pragma unroll
                        for (int j = 0; j < QS; ++j) prod_profile_grad(kinds.kind[c], s[j], f[c][j], dfs[c][j]);
                    }
                    // suf[c] = prod_{c' > c} f_c'; pre = prod_{c' < c} f_c' runs forward below: P_c = pre * suf[c]
                    T suf[C][QS], pre[QS], q[QS];
#pragma unroll
                    for (int j = 0; j < QS; ++j) {
                        suf[C - 1][j] = T(1);
#pragma unroll
                        for (int c = C - 2; c >= 0; --c) suf[c][j] = suf[c + 1][j] * f[c + 1][j];
                        const T v = cv[j] ? gg0 * b[j] - T(2) * gg1 * u[j] : T(0);
                        va += (double)(v * (f[0][j] * suf[0][j]));
                        q[j] = T(-2) * variance * v;
                        pre[j] = T(1);
                    }
                    asm volatile("" ::: "memory");
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        T wc[QS];
#pragma unroll
                        for (int j = 0; j < QS; ++j) {
                            wc[j] = q[j] * (pre[j] * suf[c][j]) * dfs[c][j];
                            pre[j] *= f[c][j];
                        }
#pragma unroll
                        for (int d = 0; d < DT; ++d) {
                            const T il = Il[c][d];
#pragma unroll
                            for (int j = 0; j < QS; ++j) {
                                const T a = df[j][d] * il;
                                const T p = wc[j] * a;
                                za[j][d] += (double)(p * il);
                                la[c][d] += (double)(p * a);  // times inv_ls[c, d] below
                            }
                        }
                    }
                }
            }
        }
        // dZ partials: this thread's columns
#pragma unroll
        for (int j = 0; j < QS; ++j)
#pragma unroll
            for (int d = 0; d < DT; ++d)
                if (cv[j]) zpart[zb + (int64_t)(mq + j) * DT + d] = za[j][d];
    }
    // lengthscale / variance partials: sum over the workgroup's threads
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int d = 0; d < DT; ++d) {
            double v = la[c][d] * (double)Il[c][d];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if (lane == 0) red[w][c * DT + d] = v;
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) va += __shfl_xor(va, o);
    if (lane == 0) red[w][C * DT] = va;
    __syncthreads();
    if (t <= C * DT) {
        double v = 0.0;
        for (int u = 0; u < NTHREADS / 64; ++u) v += red[u][t];
        const int64_t blk = (int64_t)blockIdx.x * gridDim.y + blockIdx.y;
        if (t < C * DT)
            lpart[blk * (C * DT) + t] = v;
        else
            vpart[blk] = v;
    }
}

template <typename T>
int kernel_grad_prod(const int* kinds, const T* X, const T* Z, const T* inv_ls, T variance, const T* U, int64_t ldu,
                     const T* g0, const T* g1, int gstride, const T* beta, int bstride, int64_t N, int M, int D, int C,
                     double* zpart, double* lpart, double* vpart, void* stream) {
    if (!kinds || !X || !Z || !inv_ls || !U || !g0 || !g1 || !beta || !zpart || !lpart || !vpart || N <= 0 || M <= 0 || D <= 0 ||
        D > 16 || C < 1 || C > TSVGP_MAX_COMPONENTS || gstride <= 0 || bstride <= 0 || (ldu % 2) != 0)
        return TSVGP_EINVAL;
    ProdGradKinds kk{};
    for (int c = 0; c < C; ++c) {
        if (kinds[c] != TSVGP_KERNEL_SE && kinds[c] != TSVGP_KERNEL_MATERN32 && kinds[c] != TSVGP_KERNEL_MATERN52)
            return TSVGP_EINVAL;
        kk.kind[c] = kinds[c];
    }
    const int Mp = (M + TILE - 1) / TILE * TILE;
    // a thread reads its two columns of U as one vector (m, ldu even): 16 bytes in fp64, 8 in fp32
    if (ldu < Mp || (reinterpret_cast<uintptr_t>(U) & (2 * sizeof(T) - 1)) != 0) return TSVGP_EINVAL;
    const int64_t nrb = (N + KG_ROWS - 1) / KG_ROWS;
    if (nrb > 0x7fffffff) return TSVGP_EINVAL;
    const dim3 grid((unsigned)nrb, (unsigned)((Mp + FILL_COLS - 1) / FILL_COLS));
    hipStream_t st = (hipStream_t)stream;
    const int DT = D <= 1 ? 1 : D <= 2 ? 2 : D <= 4 ? 4 : D <= 8 ? 8 : 16;
    if (hipMemsetAsync(zpart, 0, sizeof(double) * (size_t)grid.x * Mp * DT, st) != hipSuccess) return TSVGP_ELAUNCH;
#define TSVGP_PG_LAUNCH(DT_, C_)                                                                                                \
    hipLaunchKernelGGL((kgrad_prod_kernel<T, DT_, C_, (C_ * DT_ * sizeof(T) >= 256 ? 1 : 2)>), grid, dim3(NTHREADS), 0, st, X, Z, inv_ls, kk, variance, U, ldu, g0, g1, \
                       gstride, beta, bstride, N, M, D, zpart, lpart, vpart, Mp)
#define TSVGP_PG_C(DT_)                          \
    switch (C) {                                 \
        case 1: TSVGP_PG_LAUNCH(DT_, 1); break;  \
        case 2: TSVGP_PG_LAUNCH(DT_, 2); break;  \
        case 3: TSVGP_PG_LAUNCH(DT_, 3); break;  \
        default: TSVGP_PG_LAUNCH(DT_, 4); break; \
    }
    switch (DT) {
        case 1: TSVGP_PG_C(1) break;
        case 2: TSVGP_PG_C(2) break;
        case 4: TSVGP_PG_C(4) break;
        case 8: TSVGP_PG_C(8) break;
        default: TSVGP_PG_C(16) break;
    }
#undef TSVGP_PG_C
#undef TSVGP_PG_LAUNCH
    return launch_status();
}

}  // namespace

extern "C" {

int tsvgp_kernel_grad_prod_f64(const int* kinds_host, const double* X, const double* Z, const double* inv_ls, double variance,
                               const double* U, int64_t ldu, const double* g0, const double* g1, int gstride,
                               const double* beta, int bstride, int64_t N, int M, int D, int C, double* zpart, double* lpart,
                               double* vpart, void* stream) {
    return kernel_grad_prod<double>(kinds_host, X, Z, inv_ls, variance, U, ldu, g0, g1, gstride, beta, bstride, N, M, D, C, zpart,
                                    lpart, vpart, stream);
}
int tsvgp_kernel_grad_prod_f32(const int* kinds_host, const float* X, const float* Z, const float* inv_ls, float variance,
                               const float* U, int64_t ldu, const float* g0, const float* g1, int gstride, const float* beta,
                               int bstride, int64_t N, int M, int D, int C, double* zpart, double* lpart, double* vpart,
                               void* stream) {
    return kernel_grad_prod<float>(kinds_host, X, Z, inv_ls, variance, U, ldu, g0, g1, gstride, beta, bstride, N, M, D, C, zpart,
                                   lpart, vpart, stream);
}

// vpart: one double per workgroup = ceil(Mp / 512) * Np of them (tsvgp_gram_to_gradw_parts)
int64_t tsvgp_gram_to_gradw_parts(int64_t N, int M) {
    if (N <= 0 || M <= 0) return -1;
    const int64_t rows_pad = (N + TILE - 1) / TILE * TILE;
    const int64_t cols_pad = (M + TILE - 1) / TILE * TILE;
    return rows_pad * ((cols_pad / 2 + NTHREADS - 1) / NTHREADS);
}
int tsvgp_gram_to_gradw_f64(int kind, double* G, const double* xx, const double* zz, double variance, const double* U, int64_t ldu,
                            const double* g0, const double* g1, int gstride, const double* beta, int bstride, int64_t N, int M,
                            int64_t ldk, double* vpart, void* stream) {
    return gram_to_gradw<double>(kind, G, xx, zz, variance, U, ldu, g0, g1, gstride, beta, bstride, N, M, ldk, vpart, stream);
}
int tsvgp_gram_to_gradw_f32(int kind, float* G, const float* xx, const float* zz, float variance, const float* U, int64_t ldu,
                            const float* g0, const float* g1, int gstride, const float* beta, int bstride, int64_t N, int M,
                            int64_t ldk, double* vpart, void* stream) {
    return gram_to_gradw<float>(kind, G, xx, zz, variance, U, ldu, g0, g1, gstride, beta, bstride, N, M, ldk, vpart, stream);
}

int tsvgp_kernel_grad_rows(void) { return KG_ROWS; }
int tsvgp_kernel_grad_dpad(int D) { return D <= 1 ? 1 : D <= 2 ? 2 : D <= 4 ? 4 : D <= 8 ? 8 : 16; }
int tsvgp_kernel_grad_f64(int kind, const double* X, const double* Z, const double* inv_ls, double variance,
                          const double* U, int64_t ldu, const double* g0, const double* g1, int gstride,
                          const double* beta, int bstride, int64_t N, int M, int D, double* zpart, double* lpart,
                          double* vpart, void* stream) {
    return kernel_grad<double>(kind, X, Z, inv_ls, variance, U, ldu, g0, g1, gstride, beta, bstride, N, M, D, zpart, lpart,
                               vpart, stream);
}
int tsvgp_kernel_grad_f32(int kind, const float* X, const float* Z, const float* inv_ls, float variance, const float* U,
                          int64_t ldu, const float* g0, const float* g1, int gstride, const float* beta, int bstride,
                          int64_t N, int M, int D, double* zpart, double* lpart, double* vpart, void* stream) {
    return kernel_grad<float>(kind, X, Z, inv_ls, variance, U, ldu, g0, g1, gstride, beta, bstride, N, M, D, zpart, lpart,
                              vpart, stream);
}

}  // extern "C"
