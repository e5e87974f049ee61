// tsvgp_select.hip -- greedy conditional-variance selection of inducing points (tsvgp_greedy_select_f64) for CDNA4 (gfx950 /
// MI355X), with its launcher and C entry points.  A translation unit of its own: it shares tsvgp_device.h (the kernel profiles)
// with the E-step kernels of tsvgp_kernels.hip, and their object code does not depend on it.
//
// Kernel inventory
//   greedy_init_kernel   d = variance, the state's head.
//   greedy_step_kernel, greedy_pick_kernel   pivoted Cholesky of K(X, X), two launches per step.  HBM bound on the re-read of the
//                        transposed factor.

#include <hip/hip_runtime.h>

#include <cmath>
#include <stdint.h>

#include "tsvgp_hip.h"
#include "tsvgp_device.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// Greedy conditional-variance selection of inducing points (Burt, Rasmussen, van der Wilk 2020): pivoted Cholesky of
// K(X, X), one column per step, always taking the row with the largest residual prior variance
//     d[n] = variance - sum_{i < j} C[i, n]^2.
// The factor is stored TRANSPOSED, C [M x ldc]: row j (the j-th Cholesky column) is contiguous in n, so the lane that owns
// rows n, n + 1 reads C[i * ldc + n] with one 16-byte load per i, a wave 1 KB.  Step j is two launches:
//   greedy_step_kernel   one wave per 128 rows: c = (k(x_n, x_p) - sum_{i < j} C[i, n] C[i, p]) / sqrt(d[p]) into row j,
//                        d[n] <- max(d[n] - c^2, 0), d[p] <- 0, and one (max d, lowest n) candidate per workgroup.  HBM bound
//                        on the read of rows < j (8 Np j bytes); the pivot's entries C[i, p] come as scalars from `cvec`.
//   greedy_pick_kernel   one workgroup: the candidates' maximum (lowest index on equal values), the stop test against the
//                        floor, indices / pivots / count, and the strided gather C[0 .. j, p] -> cvec for the next step (once,
//                        not once per workgroup of the step kernel).
// The dot product runs over i in increasing order into four accumulators per row (i mod 4), added as (a0 + a1) + (a2 + a3):
// the order depends on j alone, not on the grid, so two calls agree bit for bit and identical rows of X get identical columns
// of C.  No workgroup waits for another one: the stop condition is a device flag that every later launch reads first.
// ---------------------------------------------------------------------------------------------------------------
constexpr int GS_ROWS = TILE;           // rows per workgroup of the step kernel: one wave, two rows per lane
constexpr int GS_PICK_THREADS = 1024;   // the one workgroup of the pick kernel

struct GreedyState {  // head of the workspace (32 bytes), then cvec [M], cand_val [nblk], cand_idx [nblk]
    int64_t p;     // pivot of the step about to run
    double dp;     // its residual variance as found
    int64_t stop;  // nonzero: the stop condition was met, every later launch returns at once
    int64_t reserved;
};

// (max, lowest index) of two candidates
__device__ __forceinline__ void greedy_take(double& bv, long long& bi, double v, long long i) {
    if (v > bv || (v == bv && i < bi)) {
        bv = v;
        bi = i;
    }
}
__device__ __forceinline__ void greedy_wave_max(double& bv, long long& bi) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(bv, off);
        const long long oi = __shfl_xor(bi, off);
        greedy_take(bv, bi, ov, oi);
    }
}

// The scaled squared distance in the fill's form: both rows scaled and rounded, then subtracted.  Contraction is off: fused
// into fma(x, il, -(z il)) the difference of two identical rows would be the rounding error of z il instead of exactly 0.
__device__ __forceinline__ double greedy_dist2(const double* __restrict__ x, const double* __restrict__ z,
                                               const double* __restrict__ inv_ls, int D) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int q = 0; q < D; ++q) {
        const double il = inv_ls[q];
        const double a = x[q] * il, b = z[q] * il;
        const double dd = a - b;
        s = fma(dd, dd, s);
    }
    return s;
}

__global__ __launch_bounds__(NTHREADS) void greedy_init_kernel(double* __restrict__ d, GreedyState* __restrict__ st,
                                                               int64_t* __restrict__ indices, double* __restrict__ pivots,
                                                               int32_t* __restrict__ count, double variance, double vfloor,
                                                               int64_t N, int64_t Np) {
    const int64_t n = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
    if (n < Np) d[n] = n < N ? variance : 0.0;
    if (n == 0) {
        // every d starts equal: the lowest index wins the first step
        const bool accept = variance > vfloor;
        st->p = 0;
        st->dp = variance;
        st->stop = accept ? 0 : 1;
        st->reserved = 0;
        indices[0] = 0;
        pivots[0] = variance;
        *count = accept ? 1 : 0;
    }
}

template <int KIND>
__global__ __launch_bounds__(64) void greedy_step_kernel(const double* __restrict__ X, const double* __restrict__ inv_ls,
                                                         double variance, double* __restrict__ C, int64_t ldc,
                                                         double* __restrict__ d, const GreedyState* __restrict__ st,
                                                         const double* __restrict__ cvec, double* __restrict__ cand_val,
                                                         int64_t* __restrict__ cand_idx, int64_t N, int D, int j) {
    if (st->stop) return;
    const int64_t p = st->p;
    const double dp = st->dp;
    const int64_t n0 = (int64_t)blockIdx.x * GS_ROWS + 2 * (int)threadIdx.x;  // < Np: the grid is Np / GS_ROWS workgroups
    const double* __restrict__ Cn = C + n0;
    double a0[4] = {0.0, 0.0, 0.0, 0.0}, a1[4] = {0.0, 0.0, 0.0, 0.0};
    int i = 0;
    for (; i + 8 <= j; i += 8) {
        v2d c[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) c[u] = *reinterpret_cast<const v2d*>(Cn + (int64_t)(i + u) * ldc);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const double w = cvec[i + u];
            a0[u & 3] = fma(c[u][0], w, a0[u & 3]);
            a1[u & 3] = fma(c[u][1], w, a1[u & 3]);
        }
    }
    {  // the last j mod 8 terms: i is a multiple of 8 here, so term i + u still goes to accumulator (i + u) mod 4
        const int left = j - i;
        v2d c[7];
#pragma unroll
        for (int u = 0; u < 7; ++u)
            c[u] = u < left ? *reinterpret_cast<const v2d*>(Cn + (int64_t)(i + u) * ldc) : v2d{0.0, 0.0};
#pragma unroll
        for (int u = 0; u < 7; ++u) {
            if (u < left) {
                const double w = cvec[i + u];
                a0[u & 3] = fma(c[u][0], w, a0[u & 3]);
                a1[u & 3] = fma(c[u][1], w, a1[u & 3]);
            }
        }
    }
    const double dot[2] = {(a0[0] + a0[1]) + (a0[2] + a0[3]), (a1[0] + a1[1]) + (a1[2] + a1[3])};
    const double rs = sqrt(dp);
    const v2d dold = *reinterpret_cast<const v2d*>(d + n0);
    v2d cnew, dnew;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int64_t n = n0 + r;
        double cn = 0.0, dn = 0.0;
        if (n < N) {
            cn = (variance * kernel_profile<KIND>(greedy_dist2(X + n * D, X + p * D, inv_ls, D)) - dot[r]) / rs;
            dn = n == p ? 0.0 : fmax(fma(-cn, cn, dold[r]), 0.0);
        }
        cnew[r] = cn;  // rows >= N of C are zeros
        dnew[r] = dn;
    }
    *reinterpret_cast<v2d*>(C + (int64_t)j * ldc + n0) = cnew;
    *reinterpret_cast<v2d*>(d + n0) = dnew;
    // this workgroup's candidate for the next pivot; rows >= N never win (every workgroup holds at least one row < N)
    double bv = n0 < N ? dnew[0] : -1.0;
    long long bi = n0;
    if (n0 + 1 < N) greedy_take(bv, bi, dnew[1], n0 + 1);
    greedy_wave_max(bv, bi);
    if (threadIdx.x == 0) {
        cand_val[blockIdx.x] = bv;
        cand_idx[blockIdx.x] = bi;
    }
}

__global__ __launch_bounds__(GS_PICK_THREADS) void greedy_pick_kernel(const double* __restrict__ C, int64_t ldc,
                                                                      GreedyState* __restrict__ st, double* __restrict__ cvec,
                                                                      const double* __restrict__ cand_val,
                                                                      const int64_t* __restrict__ cand_idx, int64_t nblk,
                                                                      double vfloor, int64_t* __restrict__ indices,
                                                                      double* __restrict__ pivots, int32_t* __restrict__ count,
                                                                      int j) {
    __shared__ double sv[GS_PICK_THREADS / 64];
    __shared__ long long si[GS_PICK_THREADS / 64];
    if (st->stop) return;  // (read by every thread in front of the barrier below; written behind it)
    const int t = threadIdx.x;
    double bv = -1.0;
    long long bi = INT64_MAX;
    for (int64_t b = t; b < nblk; b += GS_PICK_THREADS) greedy_take(bv, bi, cand_val[b], cand_idx[b]);
    greedy_wave_max(bv, bi);
    if ((t & 63) == 0) {
        sv[t >> 6] = bv;
        si[t >> 6] = bi;
    }
    __syncthreads();
    bv = sv[0];
    bi = si[0];
#pragma unroll
    for (int w = 1; w < GS_PICK_THREADS / 64; ++w) greedy_take(bv, bi, sv[w], si[w]);
    if (!(bv > vfloor)) {  // nothing left above the floor (NaN included): count stays at j + 1
        if (t == 0) st->stop = 1;
        return;
    }
    for (int i = t; i <= j; i += GS_PICK_THREADS) cvec[i] = C[(int64_t)i * ldc + bi];
    if (t == 0) {
        st->p = bi;
        st->dp = bv;
        indices[j + 1] = bi;
        pivots[j + 1] = bv;
        *count = j + 2;
    }
}

int64_t greedy_select_work_bytes(int64_t N, int M) {
    if (N <= 0 || M <= 0 || (N + GS_ROWS - 1) / GS_ROWS > 0x7fffffffLL) return -1;
    return (int64_t)sizeof(GreedyState) + 8 * ((int64_t)M + 2 * ((N + GS_ROWS - 1) / GS_ROWS));
}

int greedy_select(int kind, const double* X, const double* inv_ls, double variance, double vfloor, double* C, int64_t ldc,
                  double* d, int64_t* indices, double* pivots, int32_t* count, void* work, int64_t N, int M, int D,
                  void* stream) {
    if (!X || !inv_ls || !C || !d || !indices || !pivots || !count || !work || N < 1 || M < 1 || D < 1 || D > 32 ||
        !(variance > 0.0) || !std::isfinite(variance) || !(vfloor >= 0.0) || !std::isfinite(vfloor))
        return TSVGP_EINVAL;
    if (kind != TSVGP_KERNEL_SE && kind != TSVGP_KERNEL_MATERN32 && kind != TSVGP_KERNEL_MATERN52) return TSVGP_EINVAL;
    if (greedy_select_work_bytes(N, M) < 0) return TSVGP_EINVAL;
    const int64_t Np = (N + TILE - 1) / TILE * TILE;
    // 16-byte accesses: a lane's two rows of C and d travel together
    if (ldc < Np || (ldc % 2) != 0 || (reinterpret_cast<uintptr_t>(C) & 15) != 0 || (reinterpret_cast<uintptr_t>(d) & 15) != 0 ||
        (reinterpret_cast<uintptr_t>(work) & 7) != 0)
        return TSVGP_EINVAL;
    const int64_t nblk = Np / GS_ROWS;
    GreedyState* st = static_cast<GreedyState*>(work);
    double* cvec = reinterpret_cast<double*>(st + 1);
    double* cand_val = cvec + M;
    int64_t* cand_idx = reinterpret_cast<int64_t*>(cand_val + nblk);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(greedy_init_kernel, dim3((unsigned)((Np + NTHREADS - 1) / NTHREADS)), dim3(NTHREADS), 0, s, d, st, indices,
                       pivots, count, variance, vfloor, N, Np);
    for (int j = 0; j < M; ++j) {
#define TSVGP_GS_STEP(KIND_)                                                                                                   \
    hipLaunchKernelGGL(greedy_step_kernel<KIND_>, dim3((unsigned)nblk), dim3(64), 0, s, X, inv_ls, variance, C, ldc, d, st, cvec, \
                       cand_val, cand_idx, N, D, j)
        if (kind == TSVGP_KERNEL_SE) TSVGP_GS_STEP(TSVGP_KERNEL_SE);
        else if (kind == TSVGP_KERNEL_MATERN32) TSVGP_GS_STEP(TSVGP_KERNEL_MATERN32);
        else TSVGP_GS_STEP(TSVGP_KERNEL_MATERN52);
#undef TSVGP_GS_STEP
        if (j + 1 < M)  // the last step needs no successor
            hipLaunchKernelGGL(greedy_pick_kernel, dim3(1), dim3(GS_PICK_THREADS), 0, s, C, ldc, st, cvec, cand_val, cand_idx, nblk,
                               vfloor, indices, pivots, count, j);
    }
    return launch_status();
}

}  // namespace

extern "C" {

int64_t tsvgp_greedy_select_work_bytes(int64_t N, int M) { return greedy_select_work_bytes(N, M); }
int tsvgp_greedy_select_f64(int kind, const double* X, const double* inv_ls, double variance, double floor, double* C, int64_t ldc,
                            double* d, int64_t* indices, double* pivots, int32_t* count, void* work, int64_t N, int M, int D,
                            void* stream) {
    return greedy_select(kind, X, inv_ls, variance, floor, C, ldc, d, indices, pivots, count, work, N, M, D, stream);
}

}  // extern "C"
