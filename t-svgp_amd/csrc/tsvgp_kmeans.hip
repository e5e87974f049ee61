// tsvgp_kmeans.hip -- Lloyd's k-means for inducing points (tsvgp_kmeans_assign_f64, tsvgp_kmeans_update_f64; include/tsvgp_hip.h
// (12)) and its k-means++ seeding (tsvgp_kmeanspp_f64; (13)) for CDNA4 (gfx950 / MI355X): 64-wide wavefronts, fp64 vector arithmetic, LDS broadcast reads.  A translation unit of its
// own: of what it shares with the E-step kernels of tsvgp_kernels.hip it uses the C-ABI header and launch_status alone (the rest of
// tsvgp_device.h, which it includes for that one line, compiles to nothing here), and their object code does not depend on it.
//
// Kernel inventory
//   kmeans_assign_kernel<DT>   nearest scaled centre per row: lanes along rows, centres broadcast from LDS; fp64 VALU bound, no
//                              N x M array.
//   kmeans_update_kernel       the fixed-order mean per cluster over the stably sorted rows; gather-latency bound.
//   kmeanspp_*_kernel          k-means++ seeding (tsvgp_kmeanspp_f64; (13)): per centre one sweep over the rows in the assignment's
//                              layout and one small launch that reduces, chooses and draws the next candidates; latency bound.

#include <hip/hip_runtime.h>

#include <cmath>
#include <stdint.h>

#include "tsvgp_hip.h"
#include "tsvgp_device.h"

namespace {

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

// ---------------------------------------------------------------------------------------------------------------
// k-means++ seeding (tsvgp_kmeanspp_f64; include/tsvgp_hip.h (13)): D^2 sampling with L greedy local trials per centre.  Round r
// is two launches, and one more pass at the end writes the final distances: 2 M + 2 launches in all, X read once per centre,
// nothing of size N x M or N x L.
//   kmeanspp_init_kernel      fills cand / cand_pot / unif with -1 / +inf / 0 and draws the first centre into cand[0].
//   kmeanspp_sweep_kernel<DT> the N-sized pass of round r, kmeans_assign_kernel's layout (lanes along rows, R rows per lane in
//                             registers, the previous winner and this round's candidates scaled once into LDS and read as
//                             broadcasts).  It applies the previous winner, mind <- min(mind, s(x, x_{i_{r-1}})), stores it, and
//                             writes part[b, j] = the workgroup's sum of min(mind, s(x, cand_j)) in the fixed tree of the
//                             assignment's partial inertia (a lane's R rows in order, the wave's butterfly, the four waves in
//                             order).  Round 0 has the one candidate i_0 and no mind yet (+inf); the pass after the last round has
//                             no candidate and leaves the final mind in `dist`.
//   kmeanspp_pick_kernel      L workgroups (one when no round follows), each of which adds part[:, j] over the workgroups for
//                             every j (slot t / 16 takes b = slot, slot + 16, ... in that order, then a pairwise tree over the 16
//                             slots), takes j* = the lowest j of the minimum -- all L workgroups compute the same bits; workgroup 0
//                             records them -- and then draws ONE target of the next round, workgroup j target j:
//                             t = u(r + 1, j) * pot_r, searched in the running sum of the updated mind, whose per-workgroup masses
//                             are column j* of part already: an inclusive scan over 256 chunks of ceil(B / 256) consecutive
//                             workgroups (each chunk added in order, then a Hillis-Steele scan in lane order), the workgroups of the
//                             chunk found walked in order by one lane, and inside the workgroup found the values
//                             min(mind, s(x, x_{i_r})) recomputed for its rows in increasing n (R consecutive rows per lane added in
//                             order, the same scan across lanes).  Each level takes the HIGHEST position of positive mass
//                             whose running sum before it is <= t: with exact sums that is the lowest position whose running sum
//                             through it exceeds t; in floating point it never lands on a row of zero mass, it needs no second
//                             comparison that rounding could contradict, and a t at or above the top of the sum clips to the last
//                             row of positive mass by the same rule.  N - 1 when there is no mass at all.
// Every sum has an order fixed by (N, D, L); an integer LDS atomicMax picks the highest flagged position; no floating-point
// atomics: two calls agree bit for bit.  Row numbers read back from device memory are clamped before they address X.
// ---------------------------------------------------------------------------------------------------------------
constexpr int KPP_MAXL = TSVGP_KMEANSPP_MAX_TRIALS;
constexpr int KPP_SLOTS = KM_THREADS / KPP_MAXL;  // 16 slots of workgroups per candidate in the reduction of part
static_assert(KPP_MAXL == 16 && KPP_SLOTS == 16, "the reduction of part maps lane t to candidate t & 15 of slot t >> 4");

// u(r, j) in [0, 1): 53 bits of Philox4x32-10(counter = (r, j, 0x6B2B2B, 0), key = seed), exact in fp64
__device__ inline double kpp_uniform(int64_t seed, uint32_t r, uint32_t j) {
    uint32_t c0 = r, c1 = j, c2 = 0x6B2B2Bu, c3 = 0u;
    uint32_t k0 = (uint32_t)((uint64_t)seed & 0xffffffffu), k1 = (uint32_t)((uint64_t)seed >> 32);
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0, c1 = (uint32_t)p1, c2 = n2, c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return ((double)(c0 >> 5) * 67108864.0 + (double)(c1 >> 6)) * (1.0 / 9007199254740992.0);
}

__global__ __launch_bounds__(KM_THREADS) void kmeanspp_init_kernel(int64_t* __restrict__ cand, double* __restrict__ cand_pot,
                                                                    double* __restrict__ unif, int64_t seed, int64_t total,
                                                                    int64_t N) {
    const int64_t g = (int64_t)blockIdx.x * KM_THREADS + threadIdx.x;
    for (int64_t i = g; i < total; i += (int64_t)gridDim.x * KM_THREADS) {
        cand[i] = -1;
        cand_pot[i] = INFINITY;
        unif[i] = 0.0;
    }
    if (g == 0) {  // (the lane that filled entry 0)
        const double u = kpp_uniform(seed, 0u, 0u);
        int64_t i0 = (int64_t)(u * (double)N);
        unif[0] = u;
        cand[0] = i0 < N - 1 ? i0 : N - 1;
    }
}

template <int DT>
__global__ __launch_bounds__(KM_THREADS) void kmeanspp_sweep_kernel(const double* __restrict__ X, const double* __restrict__ inv_ls,
                                                                     double* __restrict__ mind, const int64_t* __restrict__ indices,
                                                                     const int64_t* __restrict__ cand, double* __restrict__ part,
                                                                     int r, int ncand, int L, int64_t N, int D) {
#pragma clang fp contract(off)
    constexpr int R = km_rows_per_lane(DT);
    __shared__ __attribute__((aligned(16))) double Cs[KPP_MAXL + 1][DT];  // [0]: the previous winner, [1 + j]: candidate j
    __shared__ double wsum[KPP_MAXL][KM_THREADS / 64];
    const int t = threadIdx.x;
    const int64_t n0 = (int64_t)blockIdx.x * (KM_THREADS * R) + t;  // this lane's rows: n0 + i * KM_THREADS
    for (int idx = t; idx < (ncand + 1) * DT; idx += KM_THREADS) {
        const int c = idx / DT, q = idx - c * DT;
        int64_t row = c == 0 ? (r >= 1 ? indices[r - 1] : 0) : cand[(int64_t)r * L + (c - 1)];
        row = (uint64_t)row < (uint64_t)N ? row : 0;
        Cs[c][q] = q < D ? X[row * D + q] * inv_ls[q] : 0.0;
    }
    double a[R][DT], m[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int64_t n = n0 + (int64_t)i * KM_THREADS;
#pragma unroll
        for (int q = 0; q < DT; ++q) a[i][q] = (n < N && q < D) ? X[n * D + q] * inv_ls[q] : 0.0;
        m[i] = (r >= 2 && n < N) ? mind[n] : INFINITY;
    }
    __syncthreads();
    if (r >= 1) {
        double s[R];
#pragma unroll
        for (int i = 0; i < R; ++i) s[i] = 0.0;
#pragma unroll
        for (int q = 0; q < DT; ++q) {
            const double b = Cs[0][q];
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const double dd = a[i][q] - b;
                s[i] = fma(dd, dd, s[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const int64_t n = n0 + (int64_t)i * KM_THREADS;
            m[i] = s[i] < m[i] ? s[i] : m[i];
            if (n < N) mind[n] = m[i];
        }
    }
    for (int j = 0; j < ncand; ++j) {
        double s[R];
#pragma unroll
        for (int i = 0; i < R; ++i) s[i] = 0.0;
#pragma unroll
        for (int q = 0; q < DT; ++q) {
            const double b = Cs[1 + j][q];
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const double dd = a[i][q] - b;
                s[i] = fma(dd, dd, s[i]);
            }
        }
        double sum = 0.0;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            if (n0 + (int64_t)i * KM_THREADS < N) sum += s[i] < m[i] ? s[i] : m[i];
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
        if ((t & 63) == 0) wsum[j][t >> 6] = sum;
    }
    __syncthreads();
    if (t < ncand) part[(int64_t)blockIdx.x * L + t] = ((wsum[t][0] + wsum[t][1]) + wsum[t][2]) + wsum[t][3];
}

// the exclusive prefix of the 256 lanes' v in lane order: a Hillis-Steele inclusive scan (a fixed tree), read one lane back
__device__ inline double kpp_scan_exclusive(double v, double* buf, int t) {
    buf[t] = v;
    __syncthreads();
    for (int off = 1; off < KM_THREADS; off <<= 1) {
        const double x = t >= off ? buf[t - off] : 0.0;
        __syncthreads();
        if (t >= off) buf[t] = buf[t] + x;
        __syncthreads();
    }
    const double exc = t > 0 ? buf[t - 1] : 0.0;
    __syncthreads();  // buf is free again
    return exc;
}

__global__ __launch_bounds__(KM_THREADS) void kmeanspp_pick_kernel(const double* __restrict__ X, const double* __restrict__ inv_ls,
                                                                    const double* __restrict__ mind, const double* __restrict__ part,
                                                                    int64_t* __restrict__ indices, double* __restrict__ pot_hist,
                                                                    int64_t* __restrict__ cand, double* __restrict__ cand_pot,
                                                                    double* __restrict__ unif, int64_t seed, int r, int M, int L,
                                                                    int64_t B, int rows, int64_t N, int D) {
#pragma clang fp contract(off)
    __shared__ double red[KPP_SLOTS][KPP_MAXL];
    __shared__ double buf[KM_THREADS];
    __shared__ double bw[32];
    __shared__ double s_pot, s_acc;
    __shared__ int64_t s_w, s_b;
    __shared__ int s_j, s_c, s_p;
    const int t = threadIdx.x;
    const int Lr = r == 0 ? 1 : L;  // candidates of this round
    // newpot_j = sum over the workgroups of part[b, j]
    const int j = t & (KPP_MAXL - 1), slot = t / KPP_MAXL;
    {
        double acc = 0.0;
        if (j < Lr) {
            int64_t b = slot;
            for (; b + 7 * KPP_SLOTS < B; b += 8 * KPP_SLOTS) {  // eight loads in flight; the additions keep the order of b
                double v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = part[(b + k * KPP_SLOTS) * L + j];
#pragma unroll
                for (int k = 0; k < 8; ++k) acc += v[k];
            }
            for (; b < B; b += KPP_SLOTS) acc += part[b * L + j];
        }
        red[slot][j] = acc;
    }
    for (int half = KPP_SLOTS >> 1; half >= 1; half >>= 1) {
        __syncthreads();
        if (slot < half) red[slot][j] += red[slot + half][j];
    }
    __syncthreads();
    if (t == 0) {
        int js = 0;
        for (int k = 1; k < Lr; ++k)
            if (red[0][k] < red[0][js]) js = k;  // strictly: the lowest j of the minimum
        int64_t w = cand[(int64_t)r * L + js];
        w = (uint64_t)w < (uint64_t)N ? w : 0;
        s_j = js, s_w = w, s_pot = red[0][js];
        s_c = -1, s_p = -1;
        if (blockIdx.x == 0) {
            indices[r] = w;
            pot_hist[r] = red[0][js];
            for (int k = 0; k < Lr; ++k) cand_pot[(int64_t)r * L + k] = red[0][k];
        }
    }
    __syncthreads();
    if (r + 1 >= M) return;  // no round follows (one workgroup was launched)
    const int js = s_j, jt = blockIdx.x;  // this workgroup draws target jt of round r + 1
    const int64_t w = s_w;
    const double u = kpp_uniform(seed, (uint32_t)(r + 1), (uint32_t)jt);
    const double tgt = u * s_pot;
    if (t < D) bw[t] = X[w * D + t] * inv_ls[t];
    // level 1: 256 chunks of Q consecutive workgroups
    const int64_t Q = (B + KM_THREADS - 1) / KM_THREADS;
    const int64_t b_lo = (int64_t)t * Q < B ? (int64_t)t * Q : B, b_hi = b_lo + Q < B ? b_lo + Q : B;
    double csum = 0.0;
    for (int64_t b = b_lo; b < b_hi; ++b) csum += part[b * L + js];
    const double cexc = kpp_scan_exclusive(csum, buf, t);
    if (csum > 0.0 && cexc <= tgt) atomicMax(&s_c, t);  // (a sum of zeros is 0 <= tgt: the first chunk with mass always qualifies)
    __syncthreads();
    const int chunk = s_c;
    if (chunk < 0) {  // no mass at all: the clip to N - 1
        if (t == 0) {
            unif[(int64_t)(r + 1) * L + jt] = u;
            cand[(int64_t)(r + 1) * L + jt] = N - 1;
        }
        return;
    }
    // level 2: the chunk's workgroups in order, one lane
    if (t == chunk) {
        int64_t found = b_lo;
        double acc = cexc, facc = cexc;
        for (int64_t b = b_lo; b < b_hi; ++b) {
            const double p = part[b * L + js];
            if (p > 0.0 && acc <= tgt) found = b, facc = acc;
            acc += p;
        }
        s_b = found, s_acc = facc;
    }
    __syncthreads();
    // level 3: the rows of that workgroup in increasing n, rows / 256 consecutive rows per lane
    const int R = rows / KM_THREADS;
    const int64_t k0 = s_b * rows + (int64_t)t * R;
    double v[4], lsum = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t n = k0 + i;
        v[i] = 0.0;
        if (i < R && n < N) {
            double s = 0.0;
            for (int q = 0; q < D; ++q) {
                const double dd = X[n * D + q] * inv_ls[q] - bw[q];
                s = fma(dd, dd, s);
            }
            const double old = r >= 1 ? mind[n] : INFINITY;
            v[i] = s < old ? s : old;
            lsum += v[i];
        }
    }
    double acc = s_acc + kpp_scan_exclusive(lsum, buf, t);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (v[i] > 0.0 && acc <= tgt) atomicMax(&s_p, t * 4 + i);
        acc += v[i];
    }
    __syncthreads();
    if (t == 0) {
        const int pos = s_p;  // lane pos / 4, its row pos % 4
        const int64_t n = pos >= 0 ? s_b * rows + (int64_t)(pos >> 2) * R + (pos & 3) : s_b * rows;
        unif[(int64_t)(r + 1) * L + jt] = u;
        cand[(int64_t)(r + 1) * L + jt] = n < N ? n : N - 1;
    }
}

int64_t kmeanspp_work(int64_t N, int D, int L) {
    if (L < 1 || L > KPP_MAXL) return -1;
    const int64_t blocks = kmeans_assign_parts(N, D);
    return blocks < 0 ? -1 : blocks * L;
}

int kmeanspp(const double* X, const double* inv_ls, int64_t seed, int M, int L, int64_t* indices, double* dist, double* pot_hist,
             int64_t* cand, double* cand_pot, double* unif, double* work, int64_t N, int D, void* stream) {
    if (!X || !inv_ls || !indices || !dist || !pot_hist || !cand || !cand_pot || !unif || !work) return TSVGP_EINVAL;
    if (N < 1 || M < 1 || M > N || D < 1 || D > 32 || L < 1 || L > KPP_MAXL) return TSVGP_EINVAL;
    const int64_t blocks = kmeans_assign_parts(N, D);
    if (blocks < 0) return TSVGP_EINVAL;
    for (const void* p : {(const void*)X, (const void*)inv_ls, (const void*)indices, (const void*)dist, (const void*)pot_hist,
                          (const void*)cand, (const void*)cand_pot, (const void*)unif, (const void*)work})
        if (reinterpret_cast<uintptr_t>(p) & 7) return TSVGP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)blocks), threads(KM_THREADS);
    const int DT = km_dpad(D), rows = km_rows(DT);
    const int64_t total = (int64_t)M * L;
    const int64_t fill = (total + KM_THREADS - 1) / KM_THREADS;
    hipLaunchKernelGGL(kmeanspp_init_kernel, dim3((unsigned)(fill < 1024 ? fill : 1024)), threads, 0, st, cand, cand_pot, unif, seed,
                       total, N);
#define TSVGP_KPP_SWEEP(DT_)                                                                                              \
    hipLaunchKernelGGL(kmeanspp_sweep_kernel<DT_>, grid, threads, 0, st, X, inv_ls, dist, indices, cand, work, r, ncand, L, N, D)
    for (int r = 0; r <= M; ++r) {  // the pass r = M has no candidate: it applies the last winner and leaves the final mind
        const int ncand = r == 0 ? 1 : r < M ? L : 0;
        switch (DT) {
            case 1: TSVGP_KPP_SWEEP(1); break;
            case 2: TSVGP_KPP_SWEEP(2); break;
            case 4: TSVGP_KPP_SWEEP(4); break;
            case 8: TSVGP_KPP_SWEEP(8); break;
            case 16: TSVGP_KPP_SWEEP(16); break;
            default: TSVGP_KPP_SWEEP(32); break;
        }
        if (r < M)
            hipLaunchKernelGGL(kmeanspp_pick_kernel, dim3((unsigned)(r + 1 < M ? L : 1)), threads, 0, st, X, inv_ls, dist, work, indices,
                               pot_hist, cand, cand_pot, unif, seed, r, M, L, blocks, rows, N, D);
    }
#undef TSVGP_KPP_SWEEP
    return launch_status();
}

}  // namespace

extern "C" {

int tsvgp_kmeanspp_rows(int D) { return D < 1 || D > 32 ? -1 : km_rows(km_dpad(D)); }
int64_t tsvgp_kmeanspp_work(int64_t N, int D, int L) { return kmeanspp_work(N, D, L); }
int tsvgp_kmeanspp_f64(const double* X, const double* inv_ls, int64_t seed, int M, int L, int64_t* indices, double* dist,
                       double* pot_hist, int64_t* cand, double* cand_pot, double* unif, double* work, int64_t N, int D, void* stream) {
    return kmeanspp(X, inv_ls, seed, M, L, indices, dist, pot_hist, cand, cand_pot, unif, work, N, D, stream);
}

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
