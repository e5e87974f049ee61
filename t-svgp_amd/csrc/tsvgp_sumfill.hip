// tsvgp_sumfill.hip -- the K(X, Z) fill of a SUM of stationary kernels (gpflow.kernels.Sum of SquaredExponential / Matern32 /
// Matern52 components, each with its own variance, lengthscales and active dimensions), gfx950 / MI355X:
//
//     K[n, m] = sum_c variance[c] * k_{kind[c]}(r_c),    r_c^2 = sum_d ((x_nd - z_md) * inv_ls[c * D + d])^2
//
// One pass: X and Z are read once per workgroup and K is written once, where C single-kernel fills would write it C times and
// read it C - 1 times.  A translation unit of its own, as the other kernel families that were split off tsvgp_kernels.hip: this
// file shares tsvgp_device.h with them (the profiles kernel_profile<KIND> and exp_nonpos) and nothing else, and the object
// code of every other unit is what it was without it.
//
// Geometry of se_fill_kernel (tsvgp_kernels.hip): grid = (row blocks, column tiles of CPT * 256 columns); the block's X rows are
// staged in LDS pre-scaled -- here once per component, Xs[c][row][d] -- and read back with wave-uniform addresses; a thread owns
// CPT adjacent columns (2, or 4 in fp32 where the layout allows it) and writes each row of them as one 16-byte store (8 bytes for
// the fp32 two-column form).  Row blocks are 64 rows, 8 for a small output (K(Z, Z), which opens the M x M chain of every step).
// The distance is the difference form, on column PAIRS (v_pk_add_f32 / v_pk_fma_f32 in fp32, two fp64 instructions each in fp64).
//
// Registers.  se_fill_kernel keeps its scaled Z columns in registers, z[CPT][DT]: 128 VGPRs at DT = 32 in fp64.  C components
// have C times as many.  Two forms, chosen at compile time:
//   CH = C (1..4), C * DT <= 32   all C scaled Z columns of the thread stay in registers over the whole row block (at most the
//                                 128 VGPRs of the single-kernel fill); rows go two at a time, the components innermost.
//   CH = 0, runtime C             the rows go in chunks of 8 with the chunk's sums in registers (acc[8][CPT]); per chunk and
//                                 component the thread reloads its scaled Z columns (z[CPT][DT], from L2: the Z tile of a column
//                                 tile is 128 KB at most) -- one reload per 8 rows of arithmetic on them.
// The kind of a component is uniform over the launch: a scalar branch per (row chunk, component) picks the profile.  The
// per-component scalars (kind, variance) travel as kernel arguments in a by-value struct, like FillBatch.
//
// The same kernel fills a PRODUCT of stationary kernels (gpflow.kernels.Product, tsvgp_kernel_fill_prod_*) under the compile-time
// flag PROD:
//
//     K[n, m] = variance * prod_c k_{kind[c]}(r_c)         variance = prod_c variance[c], formed on the host (args.variance[0])
//
// The accumulator starts at 1, "acc *= k" stands where the variance-weighted fma of the sum stands, and the variance multiplies
// last (a zero for a column >= M, as in the sum).  Geometry, staging and both register forms are shared; with PROD = false every
// `if constexpr (PROD)` below drops out and the instantiation is the sum's own.

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "tsvgp_hip.h"

// No floating-point contraction anywhere in this unit, the inlined profiles of tsvgp_device.h included: every fma below is
// written out.  Contraction is the compiler's choice per instruction, and the rows of a chunk are unrolled -- row slot r of the
// chunk is its own instruction sequence.  Left to itself the compiler fused a * b + c in some slots and not in others (fp32,
// reload form), so K(Z, Z)[i, j] (row slot i % 8) and K(Z, Z)[j, i] (slot j % 8) differed in the last bit.  With every operation
// rounded on its own a value depends on its operands alone: K(Z, Z) is exactly symmetric and a row has the same bits in any slot.
#pragma clang fp contract(off)
#include "tsvgp_device.h"

namespace {

constexpr int SF_ROWS = 64;       // rows per block of an N-sized output
constexpr int SF_ROWS_SMALL = 8;  // and of a small one (rows_pad <= 4096), as se_fill_kernel

template <typename T>
struct SumFillArgs {
    int kind[TSVGP_MAX_COMPONENTS];
    T variance[TSVGP_MAX_COMPONENTS];
};

template <typename T>
struct SfPair;
template <>
struct SfPair<double> {
    typedef v2d type;
};
template <>
struct SfPair<float> {
    typedef v2f type;
};
template <typename T, int CPT>
struct SfVec {
    typedef typename SfPair<T>::type type;
};
template <>
struct SfVec<float, 4> {
    typedef v4f type;
};

// acc[r][q] += variance * k_KIND(s[r][q]) on the pairs of R rows
// acc[r][q] *= k_KIND(s[r][q]) on the pairs of R rows (PROD)
template <int KIND, typename T, int R, int NP>
__device__ __forceinline__ void sf_profile_mul(typename SfPair<T>::type (&acc)[R][NP], const typename SfPair<T>::type (&s)[R][NP]) {
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            acc[r][q][0] = acc[r][q][0] * kernel_profile<KIND>(s[r][q][0]);
            acc[r][q][1] = acc[r][q][1] * kernel_profile<KIND>(s[r][q][1]);
        }
}

template <int KIND, typename T, int R, int NP>
__device__ __forceinline__ void sf_profile_add(typename SfPair<T>::type (&acc)[R][NP], const typename SfPair<T>::type (&s)[R][NP],
                                               const typename SfPair<T>::type (&varc)[NP]) {
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            acc[r][q][0] = __builtin_elementwise_fma(varc[q][0], kernel_profile<KIND>(s[r][q][0]), acc[r][q][0]);
            acc[r][q][1] = __builtin_elementwise_fma(varc[q][1], kernel_profile<KIND>(s[r][q][1]), acc[r][q][1]);
        }
}

template <typename T, int DT, int CPT, int CH, bool PROD>
__global__ __launch_bounds__(NTHREADS) void sum_fill_kernel(const T* __restrict__ X, const T* __restrict__ Z,
                                                            const T* __restrict__ inv_ls, SumFillArgs<T> args,
                                                            T* __restrict__ K, int64_t N, int M, int D, int64_t ldk,
                                                            int cols_pad, int stream_out, int rows_blk, int C) {
    constexpr bool HOIST = CH > 0;
    constexpr int NP = CPT / 2;        // column pairs per thread
    constexpr int R = HOIST ? 2 : 8;   // rows per chunk (divides both row-block sizes)
    constexpr int NZ = HOIST ? CH : 1;
    typedef typename SfPair<T>::type pair_t;
    typedef typename SfVec<T, CPT>::type vec_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char sf_lds[];
    T* const Xs = reinterpret_cast<T*>(sf_lds);  // [C][rows_blk][DT], pre-scaled by the component's inv_ls

    __builtin_amdgcn_s_setprio(1);  // behind the factorisation's waves, as se_fill_kernel
    const int nc = HOIST ? CH : C;
    const int t = threadIdx.x;
    const int m = blockIdx.y * (CPT * NTHREADS) + CPT * t;  // this thread's columns
    const bool active = (m < cols_pad);
    const int64_t n0 = (int64_t)blockIdx.x * rows_blk;

    for (int idx = t; idx < nc * rows_blk * DT; idx += NTHREADS) {
        const int d = idx % DT, rr = (idx / DT) % rows_blk, c = idx / (DT * rows_blk);
        const int64_t n = n0 + rr;
        Xs[idx] = (n < N && d < D) ? X[n * D + d] * inv_ls[c * D + d] : T(0);
    }

    pair_t z[NZ][NP][DT];
    // the thread's scaled Z columns of component c into slot k; columns >= M are zeros (their variance factor is zero as well)
    auto load_z = [&](int c, int k) {
#pragma unroll
        for (int q = 0; q < NP; ++q)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int col = m + 2 * q + e;
                const bool vc = col < M;
#pragma unroll
                for (int d = 0; d < DT; ++d)
                    z[k][q][d][e] = (vc && d < D) ? Z[(int64_t)col * D + d] * inv_ls[c * D + d] : T(0);
            }
    };
    if constexpr (HOIST) {
#pragma unroll
        for (int c = 0; c < CH; ++c) load_z(c, c);
    }
    __syncthreads();
    if (!active) return;

    // valid rows get kernel values, the padding rows of the block zeros (rows_pad is a multiple of 128, so of rows_blk: every row
    // of the block is written).  Invalid columns come out as exact zeros through their variance factor.
    const int64_t left = N - n0;
    const int nvalid = left >= rows_blk ? rows_blk : (left > 0 ? (int)left : 0);
    T* const Kp = K + n0 * ldk + m;

    for (int r0 = 0; r0 < rows_blk; r0 += R) {
        pair_t acc[R][NP];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int q = 0; q < NP; ++q) acc[r][q] = PROD ? pair_t{T(1), T(1)} : pair_t{T(0), T(0)};
        if (r0 < nvalid) {
            auto component = [&](int c, int k) {
                pair_t s[R][NP];
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int q = 0; q < NP; ++q) s[r][q] = pair_t{T(0), T(0)};
                const T* const xr = Xs + ((size_t)c * rows_blk + r0) * DT;
#pragma unroll
                for (int d = 0; d < DT; ++d) {
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const T x = xr[r * DT + d];
                        const pair_t xx = {x, x};
#pragma unroll
                        for (int q = 0; q < NP; ++q) {
                            const pair_t dd = xx - z[k][q][d];
                            s[r][q] = __builtin_elementwise_fma(dd, dd, s[r][q]);
                        }
                    }
                }
                const int kind = args.kind[c];  // uniform over the launch
                if constexpr (PROD) {
                    if (kind == TSVGP_KERNEL_SE) sf_profile_mul<TSVGP_KERNEL_SE, T, R, NP>(acc, s);
                    else if (kind == TSVGP_KERNEL_MATERN32) sf_profile_mul<TSVGP_KERNEL_MATERN32, T, R, NP>(acc, s);
                    else sf_profile_mul<TSVGP_KERNEL_MATERN52, T, R, NP>(acc, s);
                    return;
                }
                const T variance = args.variance[c];
                pair_t varc[NP];
#pragma unroll
                for (int q = 0; q < NP; ++q) {
                    varc[q][0] = (m + 2 * q < M) ? variance : T(0);
                    varc[q][1] = (m + 2 * q + 1 < M) ? variance : T(0);
                }
                if (kind == TSVGP_KERNEL_SE) sf_profile_add<TSVGP_KERNEL_SE, T, R, NP>(acc, s, varc);
                else if (kind == TSVGP_KERNEL_MATERN32) sf_profile_add<TSVGP_KERNEL_MATERN32, T, R, NP>(acc, s, varc);
                else sf_profile_add<TSVGP_KERNEL_MATERN52, T, R, NP>(acc, s, varc);
            };
            if constexpr (HOIST) {
#pragma unroll
                for (int c = 0; c < CH; ++c) component(c, c);
            } else {
#pragma unroll 1
                for (int c = 0; c < C; ++c) {
                    load_z(c, 0);
                    component(c, 0);
                }
            }
            if constexpr (PROD) {  // the variance last; a column >= M (computed on zero Z columns: finite) takes a zero
#pragma unroll
                for (int q = 0; q < NP; ++q) {
                    const pair_t varc = {(m + 2 * q < M) ? args.variance[0] : T(0), (m + 2 * q + 1 < M) ? args.variance[0] : T(0)};
#pragma unroll
                    for (int r = 0; r < R; ++r) acc[r][q] = acc[r][q] * varc;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            vec_t out;
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                const bool valid = r0 + r < nvalid;  // (a chunk that straddles N computed its rows past N on zero X rows)
                out[2 * q] = valid ? acc[r][q][0] : T(0);
                out[2 * q + 1] = valid ? acc[r][q][1] : T(0);
            }
            vec_t* const p = reinterpret_cast<vec_t*>(Kp + (int64_t)(r0 + r) * ldk);
            if (stream_out)
                __builtin_nontemporal_store(out, p);
            else
                *p = out;
        }
    }
}

// variance: [C] for the sum, the one product of the components' variances for PROD
template <typename T, bool PROD>
int sum_fill(const int* kinds, const T* X, const T* Z, const T* inv_ls, const T* variance, T* K, int64_t N, int M, int D,
             int64_t ldk, int C, void* stream) {
    if (!kinds || !X || !Z || !inv_ls || !variance || !K || N <= 0 || M <= 0 || D <= 0 || C < 1 || C > TSVGP_MAX_COMPONENTS)
        return TSVGP_EINVAL;
    SumFillArgs<T> args{};
    for (int c = 0; c < C; ++c) {
        if (kinds[c] != TSVGP_KERNEL_SE && kinds[c] != TSVGP_KERNEL_MATERN32 && kinds[c] != TSVGP_KERNEL_MATERN52)
            return TSVGP_EINVAL;
        args.kind[c] = kinds[c];
        args.variance[c] = PROD ? variance[0] : variance[c];
    }
    const int64_t rows_pad = (N + TILE - 1) / TILE * TILE;
    const int cols_pad = (M + TILE - 1) / TILE * TILE;
    if (ldk < cols_pad || (ldk % 2) != 0) return TSVGP_EINVAL;
    // a thread stores its columns as one vector at K + n * ldk + m (m, ldk even): 16 bytes in fp64; 8 in fp32, which takes the
    // 16-byte stores of four columns per thread only where the layout allows them
    if ((reinterpret_cast<uintptr_t>(K) & (2 * sizeof(T) - 1)) != 0) return TSVGP_EINVAL;
    if (D > 32) return TSVGP_EINVAL;  // input dimensions are padded to a compile-time size (1, 2, 4, 8, 16, 32)
    const int rows_blk = rows_pad <= 4096 ? SF_ROWS_SMALL : SF_ROWS;
    const int DT = D <= 1 ? 1 : D <= 2 ? 2 : D <= 4 ? 4 : D <= 8 ? 8 : D <= 16 ? 16 : 32;
    const bool cpt4 = sizeof(T) == 4 && (ldk % 4) == 0 && (reinterpret_cast<uintptr_t>(K) & 15) == 0;
    const int cols_wg = (cpt4 ? 4 : 2) * NTHREADS;
    const int64_t nrb = rows_pad / rows_blk;
    if (nrb > 0x7fffffff) return TSVGP_EINVAL;
    const dim3 grid((unsigned)nrb, (unsigned)((cols_pad + cols_wg - 1) / cols_wg));
    const size_t lds = (size_t)C * rows_blk * DT * sizeof(T);  // <= 4 * 64 * 32 * 8 = 64 KB
    const int stream_out = (double)rows_pad * (double)ldk * sizeof(T) >= 512.0 * 1024 * 1024 ? 1 : 0;
    const int CH = C * DT <= 32 ? C : 0;  // all components' Z columns in registers, or a reload per row chunk
#define TSVGP_SF_LAUNCH(DT_, CPT_, CH_)                                                                                      \
    hipLaunchKernelGGL((sum_fill_kernel<T, DT_, CPT_, CH_, PROD>), grid, dim3(NTHREADS), lds, (hipStream_t)stream, X, Z, inv_ls,    \
                       args, K, N, M, D, ldk, cols_pad, stream_out, rows_blk, C)
#define TSVGP_SF_CPT(DT_, CH_)                            \
    do {                                                  \
        if constexpr (sizeof(T) == 4) {                   \
            if (cpt4) {                                   \
                TSVGP_SF_LAUNCH(DT_, 4, CH_);             \
                break;                                    \
            }                                             \
        }                                                 \
        TSVGP_SF_LAUNCH(DT_, 2, CH_);                     \
    } while (0)
#define TSVGP_SF_CH4(DT_)                          \
    switch (CH) {                                  \
        case 1: TSVGP_SF_CPT(DT_, 1); break;       \
        case 2: TSVGP_SF_CPT(DT_, 2); break;       \
        case 3: TSVGP_SF_CPT(DT_, 3); break;       \
        default: TSVGP_SF_CPT(DT_, 4); break;      \
    }
    switch (DT) {
        case 1: TSVGP_SF_CH4(1) break;
        case 2: TSVGP_SF_CH4(2) break;
        case 4: TSVGP_SF_CH4(4) break;
        case 8: TSVGP_SF_CH4(8) break;
        case 16:
            if (CH == 1) TSVGP_SF_CPT(16, 1);
            else if (CH == 2) TSVGP_SF_CPT(16, 2);
            else TSVGP_SF_CPT(16, 0);
            break;
        default:
            if (CH == 1) TSVGP_SF_CPT(32, 1);
            else TSVGP_SF_CPT(32, 0);
            break;
    }
#undef TSVGP_SF_CH4
#undef TSVGP_SF_CPT
#undef TSVGP_SF_LAUNCH
    return launch_status();
}

}  // namespace

extern "C" {

int tsvgp_kernel_fill_sum_f64(const int* kinds_host, const double* X, const double* Z, const double* inv_ls,
                              const double* variance_host, double* K, int64_t N, int M, int D, int64_t ldk, int C,
                              void* stream) {
    return sum_fill<double, false>(kinds_host, X, Z, inv_ls, variance_host, K, N, M, D, ldk, C, stream);
}
int tsvgp_kernel_fill_sum_f32(const int* kinds_host, const float* X, const float* Z, const float* inv_ls,
                              const float* variance_host, float* K, int64_t N, int M, int D, int64_t ldk, int C,
                              void* stream) {
    return sum_fill<float, false>(kinds_host, X, Z, inv_ls, variance_host, K, N, M, D, ldk, C, stream);
}

int tsvgp_kernel_fill_prod_f64(const int* kinds_host, const double* X, const double* Z, const double* inv_ls, double variance,
                               double* K, int64_t N, int M, int D, int64_t ldk, int C, void* stream) {
    return sum_fill<double, true>(kinds_host, X, Z, inv_ls, &variance, K, N, M, D, ldk, C, stream);
}
int tsvgp_kernel_fill_prod_f32(const int* kinds_host, const float* X, const float* Z, const float* inv_ls, float variance,
                               float* K, int64_t N, int M, int D, int64_t ldk, int C, void* stream) {
    return sum_fill<float, true>(kinds_host, X, Z, inv_ls, &variance, K, N, M, D, ldk, C, stream);
}

}  // extern "C"
