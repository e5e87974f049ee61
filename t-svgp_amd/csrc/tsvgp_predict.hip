// tsvgp_predict.hip -- the posterior at new inputs: the pathwise posterior function draws and their input gradient
// (tsvgp_pathwise_f64, tsvgp_pathwise_vjp_f64), the joint predictive covariance (tsvgp_cov_*) and the input gradient of the
// marginal moments (tsvgp_moments_vjp_*) for CDNA4 (gfx950 / MI355X), with their launchers and C entry points.  A translation
// unit of its own: it shares tsvgp_device.h (the kernel profiles) and tsvgp_mfma.h (the tile product of cov_kernel, which is
// panel_kernel's) with the E-step kernels of tsvgp_kernels.hip, and their object code does not depend on it.
//
// Kernel inventory
//   pathwise_kernel     S pathwise function draws at N points: random-feature prior draw + update through the inducing values,
//                       one thread per row, no N-sized operand.  fp64 VALU bound (one sincos per row and frequency).
//   pathwise_vjp_kernel its vector-Jacobian product with respect to the rows: the same layout, the same sincos and profile.
//   cov_kernel          predict_f(full_cov=True): symmetric rank-Mp update of the test covariance with the kernel function in
//                       the epilogue, lower block triangle and its mirror image.  MFMA bound.
//   mvjp_kernel         input gradient of the marginal moments (predict_f under autograd): kgrad_kernel's pair term summed over
//                       m per row, lanes along m.  One read of U = K_fu Q; VALU-issue bound as measured.

#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>
#include <stdint.h>

#include "tsvgp_hip.h"
#include "tsvgp_device.h"
#include "tsvgp_mfma.h"

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

// ---------------------------------------------------------------------------------------------------------------
// cov_kernel: the joint predictive covariance of one latent over N test points (GPflow conditional(full_cov=True) [ext],
// reference src/models/tsvgp.py:103-112) from the stored moments product T [Np x Mp] (row n = Tm a_n, tsvgp_trmm):
//     C[i, j] = C[j, i] = base(i, j) + sign * sum_m T[i, m] T[j, m],    base = variance * k(r(x_i, x_j))  or  C[i, j] on entry
// a symmetric rank-Mp update with the kernel function in the epilogue.  One workgroup per 128 x 128 tile of the LOWER block
// triangle (tile (it, jt), jt <= it, from the linear workgroup index); the k-loop is panel_kernel's dense one -- both
// 128-row panels of T as [row][k] images, two LDS buffers, one barrier per chunk, mma_chunk_rowk -- and the epilogue
//   * stages the two 128-row X panels (pre-scaled by inv_ls) over the operand buffers and evaluates kernel_profile on the
//     scaled squared distance in the fill's difference form, sum_d (x~_id - x~_jd)^2 in the order of d (runtime D <= 32);
//   * forces the padding (row or column >= N) to the identity block tsvgp_potrf_f64 asks for;
//   * stores the tile from the accumulator layout (16 consecutive elements per row and 16 lanes), then the TRANSPOSED tile
//     to (jt, it) through LDS in two halves of 64 columns, read back row-wise as 16-byte vectors.
// A diagonal tile computes all of its entries but stores only those with column <= row directly and those with column > row
// from the transposed image, so its upper part is a copy of its lower part: the matrix is symmetric bit for bit.  No atomics,
// one workgroup per output element pair, a fixed k order: run-to-run identical.
// ---------------------------------------------------------------------------------------------------------------
template <typename T>
struct CovArgs {
    const T* Tt;      // [Np x Mp]
    const T* X;       // [N x D]
    const T* inv_ls;  // [D]
    T* C;             // [Np x ldc]
    T variance, sign;
    int64_t N, ldc;
    int Mp, D, accumulate;
};

template <typename T, int KIND>
__global__ __launch_bounds__(NTHREADS, 2) void cov_kernel(CovArgs<T> a) {
    constexpr int RS = PanelK<T>::RS, KC = PanelK<T>::KC, H = PanelK<T>::H;  // KC shadows the site kernel's constant
    constexpr int VW = 16 / sizeof(T);                    // elements per 16-byte vector
    constexpr int TS = sizeof(T) == 8 ? 130 : 132;        // transposed half-tile image [64 columns][128 rows]: column stride
    static_assert(2 * TILE * COV_XS <= 4 * TILE * RS && 64 * TS <= 4 * TILE * RS, "the epilogue images reuse the operand buffers");
    __shared__ __attribute__((aligned(16))) T lds[2][2][TILE * RS];
    typedef typename Mfma<T>::acc_t acc_t;
    typedef typename std::conditional<sizeof(T) == 8, v2d, v4f>::type vec_t;

    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    // tile (it, jt), jt <= it, of the lower block triangle: workgroup b = it (it + 1) / 2 + jt
    const int bid = blockIdx.x;
    int it = (int)((sqrtf(8.0f * (float)bid + 1.0f) - 1.0f) * 0.5f);
    while ((it + 1) * (it + 2) / 2 <= bid) ++it;
    while (it * (it + 1) / 2 > bid) --it;
    const int jt = bid - it * (it + 1) / 2;
    const bool diag = it == jt;
    const int64_t i0 = (int64_t)it * TILE, j0 = (int64_t)jt * TILE;
    const int Mp = a.Mp, nchunk = Mp / KC;
    const int srow = t >> 1, skh = t & 1;  // staging role: row of the panel, which half of the k-chunk

    const T* Arow = a.Tt + (i0 + srow) * Mp + skh * H;
    const T* Brow = a.Tt + (j0 + srow) * Mp + skh * H;
    T* const lds_wr = &lds[0][0][srow * RS + skh * H];
    constexpr int BUF_STRIDE = 2 * TILE * RS, OP_STRIDE = TILE * RS;

    acc_t acc[2][8];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int n = 0; n < 8; ++n) acc[s][n] = acc_t{0, 0, 0, 0};

    T ra[H], rb[H];
    load_run<T, H>(ra, Arow);
    load_run<T, H>(rb, Brow);
    store_run<T, H>(lds_wr, ra);
    store_run<T, H>(lds_wr + OP_STRIDE, rb);
    __syncthreads();
    int buf = 0;
    for (int c = 0; c < nchunk; ++c) {
        const bool has_next = c + 1 < nchunk;
        if (has_next) {
            load_run<T, H>(ra, Arow + (c + 1) * KC);
            load_run<T, H>(rb, Brow + (c + 1) * KC);
        }
        mma_chunk_rowk<T, 0xFF, 0xFF>(acc, &lds[buf][0][0], &lds[buf][1][0], w, lane);
        if (has_next) {
            store_run<T, H>(lds_wr + (buf ^ 1) * BUF_STRIDE, ra);
            store_run<T, H>(lds_wr + (buf ^ 1) * BUF_STRIDE + OP_STRIDE, rb);
        }
        __syncthreads();
        buf ^= 1;
    }

    // ---- epilogue (every wave is past its last fragment read: the operand buffers are free)
    T* const img = &lds[0][0][0];
    const int D = a.D;
    if (!a.accumulate) {
        for (int idx = t; idx < 2 * TILE * D; idx += NTHREADS) {
            const int side = idx / (TILE * D), rem = idx - side * (TILE * D);
            const int rr = rem / D, d = rem - rr * D;
            const int64_t n = (side ? j0 : i0) + rr;
            img[(side * TILE + rr) * COV_XS + d] = n < a.N ? a.X[n * D + d] * a.inv_ls[d] : T(0);
        }
        __syncthreads();
    }
    const int lr = lane & 15;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int li = row_block(w, s) * 16 + Mfma<T>::row(lane, r);
            const int64_t gi = i0 + li;
            T* const Cr = a.C + gi * a.ldc + j0 + lr;
            T base[8];
            if (a.accumulate) {
#pragma unroll
                for (int n = 0; n < 8; ++n) base[n] = (!diag || n * 16 + lr <= li) ? Cr[n * 16] : T(0);
            } else {
                T sv[8];
#pragma unroll
                for (int n = 0; n < 8; ++n) sv[n] = T(0);
                const T* xi = img + li * COV_XS;
                const T* xj = img + (TILE + lr) * COV_XS;
                for (int d = 0; d < D; ++d) {
                    const T x = xi[d];
#pragma unroll
                    for (int n = 0; n < 8; ++n) {
                        const T dd = x - xj[n * 16 * COV_XS + d];
                        sv[n] += dd * dd;
                    }
                }
#pragma unroll
                for (int n = 0; n < 8; ++n) base[n] = a.variance * kernel_profile<KIND>(sv[n]);
            }
#pragma unroll
            for (int n = 0; n < 8; ++n) {
                const int lj = n * 16 + lr;
                const int64_t gj = j0 + lj;
                T v = base[n] + a.sign * acc[s][n][r];
                if (gi >= a.N || gj >= a.N) v = (gi == gj) ? T(1) : T(0);  // identity block in the padding
                acc[s][n][r] = v;
                if (!diag || lj <= li) Cr[n * 16] = v;
            }
        }

    // ---- the mirror image: C[j0 + c, i0 + row] = tile[row, c], 64 columns c at a time through LDS
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        __syncthreads();  // the X panels (h = 0) / the first half's image (h = 1) have been read
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int li = row_block(w, s) * 16 + Mfma<T>::row(lane, r);
#pragma unroll
                for (int n = 0; n < 4; ++n) img[(n * 16 + lr) * TS + li] = acc[s][4 * h + n][r];
            }
        __syncthreads();
        constexpr int UPR = TILE / VW;  // 16-byte units per image column (= output row)
        for (int u = t; u < 64 * UPR; u += NTHREADS) {
            const int c = u / UPR, q = u - c * UPR;
            const vec_t v = *reinterpret_cast<const vec_t*>(img + c * TS + q * VW);
            const int lj = 64 * h + c;  // output row within the mirrored tile
            T* const dst = a.C + (j0 + lj) * a.ldc + i0 + q * VW;
            if (!diag) {
                *reinterpret_cast<vec_t*>(dst) = v;
            } else {
#pragma unroll
                for (int e = 0; e < VW; ++e)
                    if (q * VW + e > lj) dst[e] = v[e];
            }
        }
    }
}

template <typename T>
int cov(int kind, const T* Tt, const T* X, const T* inv_ls, T variance, T sign, T* C, int64_t N, int64_t Np, int Mp, int D,
        int64_t ldc, int flags, void* stream) {
    if (flags & ~TSVGP_COV_ACCUMULATE) return TSVGP_EINVAL;
    const bool accumulate = (flags & TSVGP_COV_ACCUMULATE) != 0;
    if (!accumulate && ((kind != TSVGP_KERNEL_SE && kind != TSVGP_KERNEL_MATERN32 && kind != TSVGP_KERNEL_MATERN52) || D <= 0 ||
                        D > 32 || !X || !inv_ls))
        return TSVGP_EINVAL;
    if (!(sign == T(1) || sign == T(-1))) return TSVGP_EINVAL;
    if (!Tt || !C || N <= 0 || Np < N || Np - N >= TILE || (Np % TILE) || Mp <= 0 || (Mp % TILE)) return TSVGP_EINVAL;
    if (Np / TILE > 32768) return TSVGP_EINVAL;  // it (it + 1) / 2 in 32 bits
    if (ldc < Np || (ldc * sizeof(T)) % 16 != 0) return TSVGP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(Tt) & 15) != 0 || (reinterpret_cast<uintptr_t>(C) & 15) != 0) return TSVGP_EINVAL;
    CovArgs<T> a{};
    a.Tt = Tt;
    a.X = X;
    a.inv_ls = inv_ls;
    a.C = C;
    a.variance = variance;
    a.sign = sign;
    a.N = N;
    a.ldc = ldc;
    a.Mp = Mp;
    a.D = accumulate ? 0 : D;
    a.accumulate = accumulate ? 1 : 0;
    const int64_t nt = Np / TILE;
    const dim3 grid((unsigned)(nt * (nt + 1) / 2)), block(NTHREADS);
    if (accumulate || kind == TSVGP_KERNEL_SE)
        hipLaunchKernelGGL((cov_kernel<T, TSVGP_KERNEL_SE>), grid, block, 0, (hipStream_t)stream, a);
    else if (kind == TSVGP_KERNEL_MATERN32)
        hipLaunchKernelGGL((cov_kernel<T, TSVGP_KERNEL_MATERN32>), grid, block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((cov_kernel<T, TSVGP_KERNEL_MATERN52>), grid, block, 0, (hipStream_t)stream, a);
    return launch_status();
}

// ---------------------------------------------------------------------------------------------------------------
// mvjp_kernel: the vector-Jacobian product of the marginal moments of one latent GP with respect to the rows of X
// (tsvgp_moments_vjp_*; predict_f under torch autograd).  With mean[n] = k_n^T beta, var[n] = variance - k_n^T Q k_n,
// k_n = K(Z, x_n), cotangents cm, cv and U = K(X, Z) Q (Q symmetric), s = sum_d s_d^2, s_d = (x_nd - z_md) / l_d, K = variance * f(s):
//   V[n, m]   = cm[n] * beta[m] - 2 * cv[n] * U[n, m]
//   dX[n, d] (+)= sum_m V[n, m] * variance * f'(s_nm) * 2 s_d / l_d
// -- the dZ term of kgrad_kernel with the opposite sign, summed over m per row instead of over n per column; f' is
// kernel_profile_grad (the Matern profiles take r = sqrt(max(s, 1e-36)): on an inducing point s_d = 0 makes the term an exact
// zero).  HBM traffic is one read of U; measured, the launch is bound by instruction issue (4 to 8 times that read).  Lanes run along m: a lane owns 16 bytes of a row of U (two doubles, four floats), a wave
// sweeps 64 * CPL columns at a time and carries RW rows per pass (RW * DT fp64 sums in registers: 4 rows up to DT = 2, 2 up to
// 8, 1 beyond); at the end of a pass a halving exchange over the wave leaves each sum on one lane group (RW DT - 1 + 6 - log2(RW DT)
// exchanges instead of 6 RW DT), which owns it from there.  A workgroup takes mvjp_rows(DT) rows.  z~ [DT][columns] (m fastest: a
// lane's columns are one 16-byte LDS read per dimension, consecutive lanes consecutive slots) and beta are staged in LDS, x~, cm,
// cv per 64 rows (read wave-uniformly).  A stage holds mvjp_stage_cols columns (32 KiB of z~, 1024 at most); a wider M is walked
// stage by stage, the workgroup's rows inside each, and the rows' running sums wait in LDS (Acc) between stages -- so that what
// is added to dX at the end is the whole sum, whatever M is.  Arithmetic in T, accumulation in fp64; no atomics; every sum's order
// is fixed by (M, D): the lane a column falls on, the sweep order, the exchange tree, the stage order -- a row's result does not
// depend on N, on its position or on the other rows.  DT = D padded to a compile-time size (padded dimensions are zero on both
// sides).
// ---------------------------------------------------------------------------------------------------------------
constexpr int MV_SUB = 64;  // rows per stage of x~, cm, cv: 16 per wave
constexpr int MV_STAGE_BYTES = 32768;

constexpr int mvjp_rows(int DT) { return DT <= 8 ? 256 : DT == 16 ? 128 : 32; }  // rows per workgroup: 16 KiB of Acc at most
constexpr int mvjp_rows_per_pass(int DT) { return DT <= 2 ? 4 : DT <= 8 ? 2 : 1; }
template <typename T>
constexpr int mvjp_stage_cols(int DT) {
    return MV_STAGE_BYTES / (DT * (int)sizeof(T)) < 1024 ? MV_STAGE_BYTES / (DT * (int)sizeof(T)) : 1024;
}
constexpr int mvjp_dpad(int D) { return D <= 1 ? 1 : D <= 2 ? 2 : D <= 4 ? 4 : D <= 8 ? 8 : D <= 16 ? 16 : 32; }

// One halving step of the exchange: of CNT sums a lane keeps the half its bit `o` selects and adds the partner's copy of it.
template <int CNT>
__device__ __forceinline__ void mvjp_exchange(double* a, int lane, int o) {
    if constexpr (CNT > 1) {
        const bool up = (lane & o) != 0;
#pragma unroll
        for (int i = 0; i < CNT / 2; ++i) {
            const double send = up ? a[i] : a[i + CNT / 2];
            const double keep = up ? a[i + CNT / 2] : a[i];
            a[i] = keep + __shfl_xor(send, o);
        }
        mvjp_exchange<CNT / 2>(a, lane, o >> 1);
    }
}

template <typename T, int KIND, int DT>
__global__ __launch_bounds__(NTHREADS) void mvjp_kernel(const T* __restrict__ X, const T* __restrict__ Z,
                                                        const T* __restrict__ inv_ls, T variance, const T* __restrict__ U,
                                                        int64_t ldu, const T* __restrict__ cm, const T* __restrict__ cv,
                                                        int cstride, const T* __restrict__ beta, int bstride, int64_t N, int M,
                                                        int D, double* __restrict__ dX, int accumulate) {
    // Contraction is off and the fused operations are written out: left to the compiler, the unrolled copies of the pair term (one per
    // row of a pass and column of a lane) were fused differently, and a row's bits depended on its place in the pass.
#pragma clang fp contract(off)
    constexpr int CPL = 16 / (int)sizeof(T), SWEEP = 64 * CPL, RW = mvjp_rows_per_pass(DT), MC = mvjp_stage_cols<T>(DT);
    constexpr int ROWS = mvjp_rows(DT), SUB = ROWS < MV_SUB ? ROWS : MV_SUB, WROWS = SUB / (NTHREADS / 64), NV = RW * DT;
    constexpr int LV = NV == 32 ? 5 : NV == 16 ? 4 : NV == 8 ? 3 : 2;  // log2(NV): NV is 4, 8, 16 or 32
    static_assert(NV == (1 << LV) && MC % SWEEP == 0 && WROWS % RW == 0 && ROWS % SUB == 0, "tiling");
    typedef T vec_t __attribute__((ext_vector_type(CPL)));
    __shared__ __attribute__((aligned(16))) T Zs[DT][MC];  // pre-scaled by inv_ls, zero beyond (M, D)
    __shared__ __attribute__((aligned(16))) T Bs[MC];
    __shared__ __attribute__((aligned(16))) T Xs[SUB][DT];  // pre-scaled by inv_ls
    __shared__ T Cs[SUB][2];
    __shared__ double Acc[ROWS][DT];  // the rows' sums over the stages behind (M > MC only)
    const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int64_t n0 = (int64_t)blockIdx.x * ROWS;
    const int64_t nend = (n0 + ROWS < N) ? n0 + ROWS : N;
    const T v2 = T(2) * variance;
    for (int m0 = 0; m0 < M; m0 += MC) {
        const int mc = M - m0 < MC ? M - m0 : MC;  // columns of this stage
        const bool first = m0 == 0, last = m0 + MC >= M;
        if (!first) __syncthreads();  // the previous stage has been read
        for (int idx = t; idx < MC * DT; idx += NTHREADS) {
            const int m = idx / DT, d = idx - m * DT;
            Zs[d][m] = (m < mc && d < D) ? Z[(int64_t)(m0 + m) * D + d] * inv_ls[d] : T(0);
        }
        for (int m = t; m < MC; m += NTHREADS) Bs[m] = m < mc ? beta[(int64_t)(m0 + m) * bstride] : T(0);
        for (int64_t nb = n0; nb < nend; nb += SUB) {
            if (nb > n0) __syncthreads();  // the previous rows have been read
            for (int idx = t; idx < SUB * DT; idx += NTHREADS) {
                const int rr = idx / DT, d = idx - rr * DT;
                const int64_t n = nb + rr;
                Xs[rr][d] = (n < nend && d < D) ? X[n * D + d] * inv_ls[d] : T(0);
            }
            if (t < SUB) {
                const int64_t n = nb + t;
                Cs[t][0] = n < nend ? cm[n * cstride] : T(0);
                Cs[t][1] = n < nend ? cv[n * cstride] : T(0);
            }
            __syncthreads();
            for (int pr = 0; pr < WROWS; pr += RW) {
                const int rb = w * WROWS + pr;  // the pass's first row within the rows staged
                const int64_t nr0 = nb + rb;
                const int nr = (int)((nend - nr0 < RW) ? nend - nr0 : RW);  // wave-uniform
                if (nr <= 0) break;
                double acc[NV];
#pragma unroll
                for (int i = 0; i < NV; ++i) acc[i] = 0.0;
                for (int m = lane * CPL; m < mc; m += SWEEP) {
                    vec_t u[RW];
#pragma unroll
                    for (int r = 0; r < RW; ++r) {
#pragma unroll
                        for (int c = 0; c < CPL; ++c) u[r][c] = T(0);
                        if (r < nr) {
                            const T* up = U + (nr0 + r) * ldu + m0 + m;
                            if (m + CPL <= mc) {
                                u[r] = *reinterpret_cast<const vec_t*>(up);
                            } else {  // the last columns of an M that is no multiple of CPL: nothing beyond M is read
#pragma unroll
                                for (int c = 0; c < CPL; ++c)
                                    if (m + c < mc) u[r][c] = up[c];
                            }
                        }
                    }
                    vec_t z[DT];
#pragma unroll
                    for (int d = 0; d < DT; ++d) z[d] = *reinterpret_cast<const vec_t*>(&Zs[d][m]);
                    const vec_t b = *reinterpret_cast<const vec_t*>(&Bs[m]);
#pragma unroll
                    for (int r = 0; r < RW; ++r) {
                        if (r < nr) {
                            const T gm = Cs[rb + r][0], gv = Cs[rb + r][1];
#pragma unroll
                            for (int c = 0; c < CPL; ++c) {
                                T s = T(0);
#pragma unroll
                                for (int d = 0; d < DT; ++d) {
                                    const T dd = Xs[rb + r][d] - z[d][c];
                                    s = fma(dd, dd, s);
                                }
                                T f, df;
                                kernel_profile_grad<KIND>(s, f, df);
                                const T v = gm * b[c] - T(2) * gv * u[r][c];
                                const T wgt = (m + c < mc) ? v2 * v * df : T(0);
#pragma unroll
                                for (int d = 0; d < DT; ++d) {
                                    const T sd = Xs[rb + r][d] - z[d][c];  // times 1 / l_d below
                                    if constexpr (sizeof(T) == 8)
                                        acc[r * DT + d] = fma((double)wgt, (double)sd, acc[r * DT + d]);
                                    else
                                        acc[r * DT + d] += (double)(wgt * sd);
                                }
                            }
                        }
                    }
                }
                // sum idx = r * DT + d ends up on the lanes whose upper LV bits are idx
                mvjp_exchange<NV>(acc, lane, 32);
#pragma unroll
                for (int o = 32 >> LV; o > 0; o >>= 1) acc[0] += __shfl_xor(acc[0], o);
                if ((lane & ((64 >> LV) - 1)) == 0) {
                    const int idx = lane >> (6 - LV), r = idx / DT, d = idx - r * DT;
                    if (r < nr && d < D) {
                        const int row = (int)(nr0 + r - n0);  // this wave's in every stage: no other wave touches Acc[row]
                        double tot = acc[0];
                        if (!first) tot += Acc[row][d];
                        if (!last) {
                            Acc[row][d] = tot;
                        } else {
                            double* const out = dX + (nr0 + r) * D + d;
                            const double g = tot * (double)inv_ls[d];
                            *out = accumulate ? *out + g : g;
                        }
                    }
                }
            }
        }
    }
}

template <typename T>
int moments_vjp(int kind, const T* X, const T* Z, const T* inv_ls, T variance, const T* U, int64_t ldu, const T* cm, const T* cv,
                int cstride, const T* beta, int bstride, int64_t N, int M, int D, double* dX, int accumulate, void* stream) {
    constexpr int CPL = 16 / (int)sizeof(T);
    if (!X || !Z || !inv_ls || !U || !cm || !cv || !beta || !dX || N <= 0 || M <= 0 || D < 1 || D > 32 || cstride <= 0 ||
        bstride <= 0 || ldu < M || (ldu % CPL) != 0 || ((uintptr_t)U % 16) != 0 || ((uintptr_t)dX % 8) != 0)
        return TSVGP_EINVAL;
    if (kind != TSVGP_KERNEL_SE && kind != TSVGP_KERNEL_MATERN32 && kind != TSVGP_KERNEL_MATERN52) return TSVGP_EINVAL;
    const int DT = mvjp_dpad(D);
    const int64_t blocks = (N + mvjp_rows(DT) - 1) / mvjp_rows(DT);
    if (blocks > 0x7fffffff) return TSVGP_EINVAL;
    const dim3 grid((unsigned)blocks);
    hipStream_t st = (hipStream_t)stream;
#define TSVGP_MV_LAUNCH(KIND_, DT_)                                                                                              \
    hipLaunchKernelGGL((mvjp_kernel<T, KIND_, DT_>), grid, dim3(NTHREADS), 0, st, X, Z, inv_ls, variance, U, ldu, cm, cv, cstride, \
                       beta, bstride, N, M, D, dX, accumulate ? 1 : 0)
#define TSVGP_MV_DT(KIND_)                          \
    switch (DT) {                                   \
        case 1: TSVGP_MV_LAUNCH(KIND_, 1); break;   \
        case 2: TSVGP_MV_LAUNCH(KIND_, 2); break;   \
        case 4: TSVGP_MV_LAUNCH(KIND_, 4); break;   \
        case 8: TSVGP_MV_LAUNCH(KIND_, 8); break;   \
        case 16: TSVGP_MV_LAUNCH(KIND_, 16); break; \
        default: TSVGP_MV_LAUNCH(KIND_, 32); break; \
    }
    if (kind == TSVGP_KERNEL_SE) {
        TSVGP_MV_DT(TSVGP_KERNEL_SE)
    } else if (kind == TSVGP_KERNEL_MATERN32) {
        TSVGP_MV_DT(TSVGP_KERNEL_MATERN32)
    } else {
        TSVGP_MV_DT(TSVGP_KERNEL_MATERN52)
    }
#undef TSVGP_MV_DT
#undef TSVGP_MV_LAUNCH
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

int tsvgp_cov_f64(int kind, const double* T, const double* X, const double* inv_ls, double variance, double sign, double* C,
                  int64_t N, int64_t Np, int Mp, int D, int64_t ldc, int flags, void* stream) {
    return cov<double>(kind, T, X, inv_ls, variance, sign, C, N, Np, Mp, D, ldc, flags, stream);
}
int tsvgp_cov_f32(int kind, const float* T, const float* X, const float* inv_ls, float variance, float sign, float* C, int64_t N,
                  int64_t Np, int Mp, int D, int64_t ldc, int flags, void* stream) {
    return cov<float>(kind, T, X, inv_ls, variance, sign, C, N, Np, Mp, D, ldc, flags, stream);
}

int tsvgp_moments_vjp_rows(int D) { return D < 1 || D > 32 ? -1 : mvjp_rows(mvjp_dpad(D)); }
int tsvgp_moments_vjp_stage_f64(int D) { return D < 1 || D > 32 ? -1 : mvjp_stage_cols<double>(mvjp_dpad(D)); }
int tsvgp_moments_vjp_stage_f32(int D) { return D < 1 || D > 32 ? -1 : mvjp_stage_cols<float>(mvjp_dpad(D)); }
int tsvgp_moments_vjp_f64(int kind, const double* X, const double* Z, const double* inv_ls, double variance, const double* U,
                          int64_t ldu, const double* cm, const double* cv, int cstride, const double* beta, int bstride, int64_t N,
                          int M, int D, double* dX, int accumulate, void* stream) {
    return moments_vjp<double>(kind, X, Z, inv_ls, variance, U, ldu, cm, cv, cstride, beta, bstride, N, M, D, dX, accumulate, stream);
}
int tsvgp_moments_vjp_f32(int kind, const float* X, const float* Z, const float* inv_ls, float variance, const float* U, int64_t ldu,
                          const float* cm, const float* cv, int cstride, const float* beta, int bstride, int64_t N, int M, int D,
                          double* dX, int accumulate, void* stream) {
    return moments_vjp<float>(kind, X, Z, inv_ls, variance, U, ldu, cm, cv, cstride, beta, bstride, N, M, D, dX, accumulate, stream);
}

}  // extern "C"
