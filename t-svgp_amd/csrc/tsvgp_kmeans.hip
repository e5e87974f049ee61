// tsvgp_kmeans.hip -- Lloyd's k-means for inducing points (tsvgp_kmeans_assign_f64, tsvgp_kmeans_update_f64; include/tsvgp_hip.h
// (12)) for CDNA4 (gfx950 / MI355X): 64-wide wavefronts, fp64 vector arithmetic, LDS broadcast reads.  A translation unit of its
// own: it shares nothing with the E-step kernels of tsvgp_kernels.hip but the C-ABI header, and their object code does not depend
// on it.
//
// Kernel inventory
//   kmeans_assign_kernel<DT>   nearest scaled centre per row: lanes along rows, centres broadcast from LDS; fp64 VALU bound, no
//                              N x M array.
//   kmeans_update_kernel       the fixed-order mean per cluster over the stably sorted rows; gather-latency bound.

#include <hip/hip_runtime.h>

#include <cmath>
#include <stdint.h>

#include "tsvgp_hip.h"

namespace {

inline int launch_status() { return hipGetLastError() == hipSuccess ? TSVGP_OK : TSVGP_ELAUNCH; }

// ---------------------------------------------------------------------------------------------------------------
// Lloyd's k-means for inducing points (tsvgp_kmeans_assign_f64, tsvgp_kmeans_update_f64): the two N-sized steps of an iteration.
//   kmeans_assign_kernel   lanes along rows: a lane keeps R rows' scaled coordinates a = x il in registers (R DT doubles) with
//                          their running (min, argmin); the centres pass through LDS scaled (b = c il), KM_CHUNK at a time, and
//                          every lane reads the same centre address (a broadcast, 16 bytes per read).  s = sum_q (a_q - b_q)^2 in
//                          greedy_dist2's operation order, contraction off.  The centres are walked in index order and only a
//                          strictly smaller s replaces the minimum: the lowest index wins a tie, across chunks as within one.
//                          Nothing of size N M is written.  3 N M D fp64 operations; per centre and wave DT / 2 LDS reads of 4
//                          cycles serve 2 R DT vector operations of 4 cycles, so the four SIMDs' reads fill 1 / R of the LDS.
//                          A padded dimension holds 0 on both sides and adds fma(0, 0, s) = s: the bits are those of D terms.
//                          A row's label and distance depend on that row and C alone.  The workgroup's partial inertia is a
//                          fixed tree (a lane's R rows in order, the wave's butterfly, the four waves in order).
//   kmeans_update_kernel   one workgroup per cluster over its segment of `order`: thread t owns dimension t mod DP of row slot
//                          t / DP (DP = D rounded up to a power of two, 256 / DP slots), adds its rows i = slot, slot + S, ... in
//                          that order, the slots are added pairwise in LDS (a fixed tree), the sum is divided by the count.  The
//                          bits of a centre depend on its segment's rows and their order alone.  No atomics.
// ---------------------------------------------------------------------------------------------------------------
constexpr int KM_THREADS = 256;  // lanes per workgroup of both kernels
constexpr int KM_CHUNK = 128;    // centres per LDS stage of the assignment

constexpr int km_dpad(int D) { return D <= 1 ? 1 : D <= 2 ? 2 : D <= 4 ? 4 : D <= 8 ? 8 : D <= 16 ? 16 : 32; }
constexpr int km_rows_per_lane(int DT) { return DT <= 16 ? 4 : 2;  }  // R DT <= 64 doubles of coordinates per lane
constexpr int km_rows(int DT) { return KM_THREADS * km_rows_per_lane(DT); }  // rows per workgroup

template <int DT>
__global__ __launch_bounds__(KM_THREADS) void kmeans_assign_kernel(const double* __restrict__ X, const double* __restrict__ C,
                                                                    const double* __restrict__ inv_ls, int32_t* __restrict__ labels,
                                                                    double* __restrict__ dist, double* __restrict__ part, int64_t N,
                                                                    int M, int D) {
#pragma clang fp contract(off)
    constexpr int R = km_rows_per_lane(DT);
    __shared__ __attribute__((aligned(16))) double Cs[KM_CHUNK][DT];
    __shared__ double wsum[KM_THREADS / 64];
    const int t = threadIdx.x;
    const int64_t n0 = (int64_t)blockIdx.x * (KM_THREADS * R) + t;  // this lane's rows: n0 + r * KM_THREADS
    double a[R][DT], best[R];
    int arg[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t n = n0 + (int64_t)r * KM_THREADS;
#pragma unroll
        for (int q = 0; q < DT; ++q) a[r][q] = (n < N && q < D) ? X[n * D + q] * inv_ls[q] : 0.0;
        best[r] = INFINITY;
        arg[r] = 0;
    }
    for (int m0 = 0; m0 < M; m0 += KM_CHUNK) {
        const int nm = M - m0 < KM_CHUNK ? M - m0 : KM_CHUNK;
        if (m0 > 0) __syncthreads();  // the previous chunk has been read
        for (int idx = t; idx < nm * DT; idx += KM_THREADS) {
            const int c = idx / DT, q = idx - c * DT;
            Cs[c][q] = q < D ? C[(int64_t)(m0 + c) * D + q] * inv_ls[q] : 0.0;
        }
        __syncthreads();
        for (int c = 0; c < nm; ++c) {
            double s[R];
#pragma unroll
            for (int r = 0; r < R; ++r) s[r] = 0.0;
#pragma unroll
            for (int q = 0; q < DT; ++q) {
                const double b = Cs[c][q];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const double dd = a[r][q] - b;
                    s[r] = fma(dd, dd, s[r]);
                }
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (s[r] < best[r]) {  // strictly: an equal later centre never replaces an earlier one
                    best[r] = s[r];
                    arg[r] = m0 + c;
                }
            }
        }
    }
    double sum = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t n = n0 + (int64_t)r * KM_THREADS;
        if (n < N) {
            labels[n] = arg[r];
            dist[n] = best[r];
            sum += best[r];
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    if ((t & 63) == 0) wsum[t >> 6] = sum;
    __syncthreads();
    if (t == 0) part[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

int64_t kmeans_assign_parts(int64_t N, int D) {
    if (N < 1 || D < 1 || D > 32) return -1;
    const int64_t rows = km_rows(km_dpad(D));
    const int64_t blocks = (N + rows - 1) / rows;
    return blocks > 0x7fffffffLL ? -1 : blocks;
}

int kmeans_assign(const double* X, const double* C, const double* inv_ls, int32_t* labels, double* dist, double* part, int64_t N,
                  int M, int D, void* stream) {
    if (!X || !C || !inv_ls || !labels || !dist || !part || N < 1 || M < 1 || D < 1 || D > 32) return TSVGP_EINVAL;
    const int64_t blocks = kmeans_assign_parts(N, D);
    if (blocks < 0) return TSVGP_EINVAL;
    // every buffer is addressed element by element: its own element's boundary is all that is required
    if ((reinterpret_cast<uintptr_t>(X) & 7) || (reinterpret_cast<uintptr_t>(C) & 7) || (reinterpret_cast<uintptr_t>(inv_ls) & 7) ||
        (reinterpret_cast<uintptr_t>(dist) & 7) || (reinterpret_cast<uintptr_t>(part) & 7) || (reinterpret_cast<uintptr_t>(labels) & 3))
        return TSVGP_EINVAL;
    const dim3 grid((unsigned)blocks);
    hipStream_t st = (hipStream_t)stream;
#define TSVGP_KM_ASSIGN(DT_)                                                                                                  \
    hipLaunchKernelGGL(kmeans_assign_kernel<DT_>, grid, dim3(KM_THREADS), 0, st, X, C, inv_ls, labels, dist, part, N, M, D)
    switch (km_dpad(D)) {
        case 1: TSVGP_KM_ASSIGN(1); break;
        case 2: TSVGP_KM_ASSIGN(2); break;
        case 4: TSVGP_KM_ASSIGN(4); break;
        case 8: TSVGP_KM_ASSIGN(8); break;
        case 16: TSVGP_KM_ASSIGN(16); break;
        default: TSVGP_KM_ASSIGN(32); break;
    }
#undef TSVGP_KM_ASSIGN
    return launch_status();
}

__global__ __launch_bounds__(KM_THREADS) void kmeans_update_kernel(const double* __restrict__ X, const int64_t* __restrict__ order,
                                                                    const int64_t* __restrict__ offsets,
                                                                    const double* __restrict__ C_old, double* __restrict__ C_new,
                                                                    int64_t N, int D, int DP) {
    __shared__ double acc[KM_THREADS];
    const int t = threadIdx.x;
    const int m = blockIdx.x;
    // a segment is clipped to [0, N) and a row number outside it is not dereferenced: wrong inputs give wrong means, not a fault
    int64_t lo = offsets[m], hi = offsets[m + 1];
    lo = lo < 0 ? 0 : (lo > N ? N : lo);
    hi = hi < lo ? lo : (hi > N ? N : hi);
    const int64_t cnt = hi - lo;
    if (cnt == 0) {  // an empty cluster keeps its centre, bit for bit
        if (t < D) C_new[(int64_t)m * D + t] = C_old[(int64_t)m * D + t];
        return;
    }
    const int q = t & (DP - 1), slot = t / DP, slots = KM_THREADS / DP;
    double s = 0.0;
    if (q < D) {
        int64_t i = lo + slot;
        for (; i + 3 * slots < hi; i += 4 * slots) {  // four gathers in flight; the additions keep the order of i
            double x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t n = order[i + u * slots];
                x[u] = (uint64_t)n < (uint64_t)N ? X[n * D + q] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) s += x[u];
        }
        for (; i < hi; i += slots) {
            const int64_t n = order[i];
            if ((uint64_t)n < (uint64_t)N) s += X[n * D + q];
        }
    }
    acc[t] = s;
    for (int half = slots >> 1; half >= 1; half >>= 1) {  // slot j += slot j + half: the same tree for every segment
        __syncthreads();
        if (slot < half) acc[t] += acc[t + half * DP];
    }
    if (t < D) C_new[(int64_t)m * D + t] = acc[t] / (double)cnt;  // (slot 0: t = q)
}

int kmeans_update(const double* X, const int64_t* order, const int64_t* offsets, const double* C_old, double* C_new, int64_t N, int M,
                  int D, void* stream) {
    if (!X || !order || !offsets || !C_old || !C_new || N < 1 || M < 1 || D < 1 || D > 32) return TSVGP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(X) & 7) || (reinterpret_cast<uintptr_t>(order) & 7) || (reinterpret_cast<uintptr_t>(offsets) & 7) ||
        (reinterpret_cast<uintptr_t>(C_old) & 7) || (reinterpret_cast<uintptr_t>(C_new) & 7))
        return TSVGP_EINVAL;
    hipLaunchKernelGGL(kmeans_update_kernel, dim3((unsigned)M), dim3(KM_THREADS), 0, (hipStream_t)stream, X, order, offsets, C_old,
                       C_new, N, D, km_dpad(D));
    return launch_status();
}

}  // namespace

extern "C" {

int tsvgp_kmeans_assign_rows(int D) { return D < 1 || D > 32 ? -1 : km_rows(km_dpad(D)); }
int tsvgp_kmeans_assign_chunk(void) { return KM_CHUNK; }
int64_t tsvgp_kmeans_assign_parts(int64_t N, int D) { return kmeans_assign_parts(N, D); }
int tsvgp_kmeans_assign_f64(const double* X, const double* C, const double* inv_ls, int32_t* labels, double* dist, double* part,
                            int64_t N, int M, int D, void* stream) {
    return kmeans_assign(X, C, inv_ls, labels, dist, part, N, M, D, stream);
}
int tsvgp_kmeans_update_f64(const double* X, const int64_t* order, const int64_t* offsets, const double* C_old, double* C_new,
                            int64_t N, int M, int D, void* stream) {
    return kmeans_update(X, order, offsets, C_old, C_new, N, M, D, stream);
}

}  // extern "C"
