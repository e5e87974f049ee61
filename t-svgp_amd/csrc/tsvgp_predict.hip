// tsvgp_predict.hip -- prediction-time kernels; so far the pathwise posterior function draws and their input gradient
// (tsvgp_pathwise_f64, tsvgp_pathwise_vjp_f64) for CDNA4 (gfx950 / MI355X), with their launchers and C entry points.  A translation unit of its own: it shares tsvgp_device.h
// (the kernel profiles) with the E-step kernels of tsvgp_kernels.hip, and their object code does not depend on it.  cov_kernel
// (tsvgp_cov_*, still in tsvgp_kernels.hip) belongs here too and follows with the MFMA wrappers it shares with panel_kernel.
//
// Kernel inventory
//   pathwise_kernel     S pathwise function draws at N points: random-feature prior draw + update through the inducing values,
//                       one thread per row, no N-sized operand.  fp64 VALU bound (one sincos per row and frequency).
//   pathwise_vjp_kernel its vector-Jacobian product with respect to the rows: the same layout, the same sincos and profile.

#include <hip/hip_runtime.h>

#include <cmath>
#include <stdint.h>

#include "tsvgp_hip.h"
#include "tsvgp_device.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// pathwise_kernel: S function draws of one latent GP at the rows of X (tsvgp_pathwise_f64),
//   out[s, n] = sum_l (W[s, l] cos(Omega_l . x~_n) + W[s, L + l] sin(Omega_l . x~_n)) + sum_m V[s, m] variance k(x_n, z_m).
// One thread per row: x~ (DT registers) and the S sums (SB registers) stay in registers through both sweeps; the frequencies with
// their 2 S weights, then the scaled inducing points with their S weights, pass through LDS in chunks of PW_CHUNK, every read a
// wave-uniform address (a broadcast: no bank conflicts).  DT = D and SB = S padded to compile-time sizes, the padding zeros on both
// sides (a padded sample's weights are zeros and its sums are not stored).  The sine / cosine pair (the device library's fp64
// sincos with its full argument reduction: |Omega . x~| reaches hundreds) and the kernel profile cost ~100 and ~30 fp64-rate
// instructions against D + 2 S and D + S fused multiply-adds, so up to S = 16 the work per row is that of one sample.
// ---------------------------------------------------------------------------------------------------------------
constexpr int PW_ROWS = 256;  // rows (threads) per workgroup
constexpr int PW_CHUNK = 64;  // frequencies / inducing points per LDS stage

struct PathwiseArgs {
    const double *X, *Z, *inv_ls, *Omega, *W, *V;
    double* out;
    double variance;
    int64_t N, ldo;
    int M, L, D, S;
};

template <int KIND, int DT, int SB>
__device__ __forceinline__ void pathwise_inducing_sweep(const PathwiseArgs& a, const double (&x)[DT], double (&acc)[SB],
                                                        double (*Fs)[DT], double (*Cs)[2 * SB], bool active) {
    const int t = threadIdx.x;
    for (int m0 = 0; m0 < a.M; m0 += PW_CHUNK) {
        const int nm = a.M - m0 < PW_CHUNK ? a.M - m0 : PW_CHUNK;
        __syncthreads();  // the previous chunk has been read
        for (int idx = t; idx < PW_CHUNK * DT; idx += PW_ROWS) {
            const int r = idx / DT, d = idx - r * DT;
            Fs[r][d] = (r < nm && d < a.D) ? a.Z[(int64_t)(m0 + r) * a.D + d] * a.inv_ls[d] : 0.0;
        }
        for (int idx = t; idx < PW_CHUNK * SB; idx += PW_ROWS) {
            const int r = idx / SB, s = idx - r * SB;
            Cs[r][s] = (r < nm && s < a.S) ? a.V[(int64_t)s * a.M + m0 + r] : 0.0;
        }
        __syncthreads();
        if (active) {
            for (int r = 0; r < nm; ++r) {
                double s2 = 0.0;
#pragma unroll
                for (int d = 0; d < DT; ++d) {
                    const double dd = x[d] - Fs[r][d];
                    s2 = fma(dd, dd, s2);
                }
                const double k = a.variance * kernel_profile<KIND>(s2);
#pragma unroll
                for (int s = 0; s < SB; ++s) acc[s] = fma(k, Cs[r][s], acc[s]);
            }
        }
    }
}

template <int DT, int SB>
__global__ __launch_bounds__(PW_ROWS) void pathwise_kernel(PathwiseArgs a, int kind) {
    __shared__ __attribute__((aligned(16))) double Fs[PW_CHUNK][DT];      // Omega rows, then scaled rows of Z
    __shared__ __attribute__((aligned(16))) double Cs[PW_CHUNK][2 * SB];  // [cos weights | sin weights] of a frequency, then V
    const int t = threadIdx.x;
    const int64_t n = (int64_t)blockIdx.x * PW_ROWS + t;
    const bool active = n < a.N;  // (no early return: every thread stages and meets the barriers)
    double x[DT], acc[SB];
#pragma unroll
    for (int d = 0; d < DT; ++d) x[d] = (active && d < a.D) ? a.X[n * a.D + d] * a.inv_ls[d] : 0.0;
#pragma unroll
    for (int s = 0; s < SB; ++s) acc[s] = 0.0;
    for (int l0 = 0; l0 < a.L; l0 += PW_CHUNK) {
        const int nl = a.L - l0 < PW_CHUNK ? a.L - l0 : PW_CHUNK;
        if (l0 > 0) __syncthreads();  // the previous chunk has been read
        for (int idx = t; idx < PW_CHUNK * DT; idx += PW_ROWS) {
            const int r = idx / DT, d = idx - r * DT;
            Fs[r][d] = (r < nl && d < a.D) ? a.Omega[(int64_t)(l0 + r) * a.D + d] : 0.0;
        }
        for (int idx = t; idx < PW_CHUNK * 2 * SB; idx += PW_ROWS) {
            const int r = idx / (2 * SB), j = idx - r * (2 * SB);
            const int half = j / SB, s = j - half * SB;
            Cs[r][j] = (r < nl && s < a.S) ? a.W[(int64_t)s * 2 * a.L + (int64_t)half * a.L + l0 + r] : 0.0;
        }
        __syncthreads();
        if (active) {
            for (int r = 0; r < nl; ++r) {
                double arg = 0.0;
#pragma unroll
                for (int d = 0; d < DT; ++d) arg = fma(Fs[r][d], x[d], arg);
                double sn, cs;
                sincos(arg, &sn, &cs);
#pragma unroll
                for (int s = 0; s < SB; ++s) acc[s] = fma(sn, Cs[r][SB + s], fma(cs, Cs[r][s], acc[s]));
            }
        }
    }
    if (kind == TSVGP_KERNEL_SE)
        pathwise_inducing_sweep<TSVGP_KERNEL_SE, DT, SB>(a, x, acc, Fs, Cs, active);
    else if (kind == TSVGP_KERNEL_MATERN32)
        pathwise_inducing_sweep<TSVGP_KERNEL_MATERN32, DT, SB>(a, x, acc, Fs, Cs, active);
    else
        pathwise_inducing_sweep<TSVGP_KERNEL_MATERN52, DT, SB>(a, x, acc, Fs, Cs, active);
    if (active) {
#pragma unroll
        for (int s = 0; s < SB; ++s)
            if (s < a.S) a.out[(int64_t)s * a.ldo + n] = acc[s];  // consecutive lanes, consecutive columns
    }
}

template <int DT>
void pathwise_launch(const PathwiseArgs& a, int kind, dim3 grid, hipStream_t st) {
    if (a.S == 1)
        hipLaunchKernelGGL((pathwise_kernel<DT, 1>), grid, dim3(PW_ROWS), 0, st, a, kind);
    else if (a.S <= 4)
        hipLaunchKernelGGL((pathwise_kernel<DT, 4>), grid, dim3(PW_ROWS), 0, st, a, kind);
    else
        hipLaunchKernelGGL((pathwise_kernel<DT, TSVGP_PATHWISE_MAX_S>), grid, dim3(PW_ROWS), 0, st, a, kind);
}

int pathwise(int kind, const double* X, const double* Z, const double* inv_ls, double variance, const double* Omega, const double* W,
             const double* V, double* out, int64_t N, int M, int L, int D, int S, int64_t ldo, void* stream) {
    if (!X || !inv_ls || !Omega || !W || !out || N <= 0 || L <= 0 || M < 0 || D <= 0 || D > 32 || S < 1 ||
        S > TSVGP_PATHWISE_MAX_S || ldo < N || !(variance > 0.0) || !std::isfinite(variance))
        return TSVGP_EINVAL;
    if (M > 0 && (!Z || !V)) return TSVGP_EINVAL;
    if (kind != TSVGP_KERNEL_SE && kind != TSVGP_KERNEL_MATERN32 && kind != TSVGP_KERNEL_MATERN52) return TSVGP_EINVAL;
    const int64_t blocks = (N + PW_ROWS - 1) / PW_ROWS;
    if (blocks > 0x7fffffff) return TSVGP_EINVAL;
    const PathwiseArgs a = {X, Z, inv_ls, Omega, W, V, out, variance, N, ldo, M, L, D, S};
    const dim3 grid((unsigned)blocks);
    hipStream_t st = (hipStream_t)stream;
    if (D <= 4)
        pathwise_launch<4>(a, kind, grid, st);
    else if (D <= 8)
        pathwise_launch<8>(a, kind, grid, st);
    else if (D <= 16)
        pathwise_launch<16>(a, kind, grid, st);
    else
        pathwise_launch<32>(a, kind, grid, st);
    return launch_status();
}

// ---------------------------------------------------------------------------------------------------------------
// pathwise_vjp_kernel: the vector-Jacobian product of pathwise_kernel with respect to the rows of X (tsvgp_pathwise_vjp_f64),
//   dX[n, d] = inv_ls_d ( sum_l Omega[l, d] (cos(a_nl) sum_s C[s, n] W[s, L + l] - sin(a_nl) sum_s C[s, n] W[s, l])
//                       + sum_m 2 (x~_nd - z~_md) variance f'(s2_nm) sum_s C[s, n] V[s, m] ),      a_nl = Omega_l . x~_n.
// The layout of pathwise_kernel: one thread per row, the same LDS stages, the same padding.  A thread keeps x~ (DT), its column of
// C (SB) and the D sums (DT) in registers; the sine / cosine pair and the profile are taken once per (n, l) and (n, m) as in the
// value kernel, and the S samples enter through two (one) dot products of length SB with the staged weights.  In the inducing
// sweep the differences x~ - z~ are formed again from LDS for the accumulation (a wave-uniform read) instead of being kept:
// DT fewer live doubles.  Every register array is indexed by unrolled compile-time indices; no atomics; a row's result depends
// on that row, its column of C and the operands alone, in a summation order fixed by (L, M).
// ---------------------------------------------------------------------------------------------------------------
struct PathwiseVjpArgs {
    const double *X, *Z, *inv_ls, *Omega, *W, *V, *C;
    double* dX;
    double variance;
    int64_t N, ldc;
    int M, L, D, S;
};

template <int KIND, int DT, int SB>
__device__ __forceinline__ void pathwise_vjp_inducing_sweep(const PathwiseVjpArgs& a, const double (&x)[DT], const double (&c)[SB],
                                                            double (&acc)[DT], double (*Fs)[DT], double (*Cs)[2 * SB], bool active) {
    const int t = threadIdx.x;
    const double v2 = 2.0 * a.variance;
    for (int m0 = 0; m0 < a.M; m0 += PW_CHUNK) {
        const int nm = a.M - m0 < PW_CHUNK ? a.M - m0 : PW_CHUNK;
        __syncthreads();  // the previous chunk has been read
        for (int idx = t; idx < PW_CHUNK * DT; idx += PW_ROWS) {
            const int r = idx / DT, d = idx - r * DT;
            Fs[r][d] = (r < nm && d < a.D) ? a.Z[(int64_t)(m0 + r) * a.D + d] * a.inv_ls[d] : 0.0;
        }
        for (int idx = t; idx < PW_CHUNK * SB; idx += PW_ROWS) {
            const int r = idx / SB, s = idx - r * SB;
            Cs[r][s] = (r < nm && s < a.S) ? a.V[(int64_t)s * a.M + m0 + r] : 0.0;
        }
        __syncthreads();
        if (active) {
            for (int r = 0; r < nm; ++r) {
                double s2 = 0.0;
#pragma unroll
                for (int d = 0; d < DT; ++d) {
                    const double dd = x[d] - Fs[r][d];
                    s2 = fma(dd, dd, s2);
                }
                double f, df;
                kernel_profile_grad<KIND>(s2, f, df);
                double cv = 0.0;
#pragma unroll
                for (int s = 0; s < SB; ++s) cv = fma(c[s], Cs[r][s], cv);
                const double g = v2 * df * cv;
#pragma unroll
                for (int d = 0; d < DT; ++d) acc[d] = fma(g, x[d] - Fs[r][d], acc[d]);
            }
        }
    }
}

template <int DT, int SB>
__global__ __launch_bounds__(PW_ROWS) void pathwise_vjp_kernel(PathwiseVjpArgs a, int kind) {
    __shared__ __attribute__((aligned(16))) double Fs[PW_CHUNK][DT];      // Omega rows, then scaled rows of Z
    __shared__ __attribute__((aligned(16))) double Cs[PW_CHUNK][2 * SB];  // [cos weights | sin weights] of a frequency, then V
    const int t = threadIdx.x;
    const int64_t n = (int64_t)blockIdx.x * PW_ROWS + t;
    const bool active = n < a.N;  // (no early return: every thread stages and meets the barriers)
    double x[DT], c[SB], acc[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) {
        x[d] = (active && d < a.D) ? a.X[n * a.D + d] * a.inv_ls[d] : 0.0;
        acc[d] = 0.0;
    }
#pragma unroll
    for (int s = 0; s < SB; ++s) c[s] = (active && s < a.S) ? a.C[(int64_t)s * a.ldc + n] : 0.0;  // consecutive lanes, consecutive columns
    for (int l0 = 0; l0 < a.L; l0 += PW_CHUNK) {
        const int nl = a.L - l0 < PW_CHUNK ? a.L - l0 : PW_CHUNK;
        if (l0 > 0) __syncthreads();  // the previous chunk has been read
        for (int idx = t; idx < PW_CHUNK * DT; idx += PW_ROWS) {
            const int r = idx / DT, d = idx - r * DT;
            Fs[r][d] = (r < nl && d < a.D) ? a.Omega[(int64_t)(l0 + r) * a.D + d] : 0.0;
        }
        for (int idx = t; idx < PW_CHUNK * 2 * SB; idx += PW_ROWS) {
            const int r = idx / (2 * SB), j = idx - r * (2 * SB);
            const int half = j / SB, s = j - half * SB;
            Cs[r][j] = (r < nl && s < a.S) ? a.W[(int64_t)s * 2 * a.L + (int64_t)half * a.L + l0 + r] : 0.0;
        }
        __syncthreads();
        if (active) {
            for (int r = 0; r < nl; ++r) {
                double arg = 0.0;
#pragma unroll
                for (int d = 0; d < DT; ++d) arg = fma(Fs[r][d], x[d], arg);
                double sn, cs;
                sincos(arg, &sn, &cs);
                double wc = 0.0, ws = 0.0;  // the cotangent's weight on the cosine and on the sine of this frequency
#pragma unroll
                for (int s = 0; s < SB; ++s) {
                    wc = fma(c[s], Cs[r][s], wc);
                    ws = fma(c[s], Cs[r][SB + s], ws);
                }
                const double g = fma(cs, ws, -(sn * wc));
#pragma unroll
                for (int d = 0; d < DT; ++d) acc[d] = fma(g, Fs[r][d], acc[d]);
            }
        }
    }
    if (kind == TSVGP_KERNEL_SE)
        pathwise_vjp_inducing_sweep<TSVGP_KERNEL_SE, DT, SB>(a, x, c, acc, Fs, Cs, active);
    else if (kind == TSVGP_KERNEL_MATERN32)
        pathwise_vjp_inducing_sweep<TSVGP_KERNEL_MATERN32, DT, SB>(a, x, c, acc, Fs, Cs, active);
    else
        pathwise_vjp_inducing_sweep<TSVGP_KERNEL_MATERN52, DT, SB>(a, x, c, acc, Fs, Cs, active);
    if (active) {
#pragma unroll
        for (int d = 0; d < DT; ++d)
            if (d < a.D) a.dX[n * a.D + d] = a.inv_ls[d] * acc[d];
    }
}

template <int DT>
void pathwise_vjp_launch(const PathwiseVjpArgs& a, int kind, dim3 grid, hipStream_t st) {
    if (a.S == 1)
        hipLaunchKernelGGL((pathwise_vjp_kernel<DT, 1>), grid, dim3(PW_ROWS), 0, st, a, kind);
    else if (a.S <= 4)
        hipLaunchKernelGGL((pathwise_vjp_kernel<DT, 4>), grid, dim3(PW_ROWS), 0, st, a, kind);
    else
        hipLaunchKernelGGL((pathwise_vjp_kernel<DT, TSVGP_PATHWISE_MAX_S>), grid, dim3(PW_ROWS), 0, st, a, kind);
}

int pathwise_vjp(int kind, const double* X, const double* Z, const double* inv_ls, double variance, const double* Omega,
                 const double* W, const double* V, const double* C, int64_t ldc, double* dX, int64_t N, int M, int L, int D, int S,
                 void* stream) {
    if (!X || !inv_ls || !Omega || !W || !C || !dX || N <= 0 || L <= 0 || M < 0 || D <= 0 || D > 32 || S < 1 ||
        S > TSVGP_PATHWISE_MAX_S || ldc < N || !(variance > 0.0) || !std::isfinite(variance))
        return TSVGP_EINVAL;
    if (M > 0 && (!Z || !V)) return TSVGP_EINVAL;
    if (kind != TSVGP_KERNEL_SE && kind != TSVGP_KERNEL_MATERN32 && kind != TSVGP_KERNEL_MATERN52) return TSVGP_EINVAL;
    const int64_t blocks = (N + PW_ROWS - 1) / PW_ROWS;
    if (blocks > 0x7fffffff) return TSVGP_EINVAL;
    const PathwiseVjpArgs a = {X, Z, inv_ls, Omega, W, V, C, dX, variance, N, ldc, M, L, D, S};
    const dim3 grid((unsigned)blocks);
    hipStream_t st = (hipStream_t)stream;
    if (D <= 4)
        pathwise_vjp_launch<4>(a, kind, grid, st);
    else if (D <= 8)
        pathwise_vjp_launch<8>(a, kind, grid, st);
    else if (D <= 16)
        pathwise_vjp_launch<16>(a, kind, grid, st);
    else
        pathwise_vjp_launch<32>(a, kind, grid, st);
    return launch_status();
}

}  // namespace

extern "C" {

int tsvgp_pathwise_f64(int kind, const double* X, const double* Z, const double* inv_ls, double variance, const double* Omega,
                       const double* W, const double* V, double* out, int64_t N, int M, int L, int D, int S, int64_t ldo,
                       void* stream) {
    return pathwise(kind, X, Z, inv_ls, variance, Omega, W, V, out, N, M, L, D, S, ldo, stream);
}
int tsvgp_pathwise_vjp_f64(int kind, const double* X, const double* Z, const double* inv_ls, double variance, const double* Omega,
                           const double* W, const double* V, const double* C, int64_t ldc, double* dX, int64_t N, int M, int L,
                           int D, int S, void* stream) {
    return pathwise_vjp(kind, X, Z, inv_ls, variance, Omega, W, V, C, ldc, dX, N, M, L, D, S, stream);
}

}  // extern "C"
