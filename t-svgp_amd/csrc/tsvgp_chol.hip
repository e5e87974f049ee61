// tsvgp_chol.hip -- the panel step of the blocked Cholesky factorisation (tsvgp_potrf*_f64), round 5.
//
// Replaces: the serial part of  tf.linalg.cholesky  in reference src/util.py:376-389 (posterior_from_dense_site: chol of
// W = I + L^T K L) and src/models/tsvgp.py:270, :300 (chol of K_uu + jitter I, chol of -2 lambda_2 + jitter I): two
// dependent M x M factorisations per E-step, each eight 128-wide block steps.
//
// The diagonal block is factored by potrf_diag_kernel (tsvgp_kernels.hip), which leaves the factor's 16 x 16 tiles in the
// ACCUMULATOR layout of v_mfma_f64_16x16x4_f64,
//     lane (n = l & 15, G = l >> 4), register r   <->   T[n][4 r + G]              (the f64 C/D layout: row = G + 4 r),
// and the inverted 16 x 16 diagonal tiles in `work` (tsvgp_chol.h).  chol_panel2_kernel (below) solves the panel rows from
// that image by substitution over the eight 16-wide column blocks -- MFMAs on tile registers.  On MI355X an fp64 MFMA takes
// 64 cycles of its SIMD's matrix pipe (profiles/r02_mfma_peak_microbench.txt), as many FMAs per clock as the vector ALU: the
// matrix instructions buy the data movement, not arithmetic.
// (A diagonal-block kernel in the same tile dataflow -- one wave on the 4 x 4 pivot chains, seven on tile rows -- was built and
// measured slower than potrf_diag_kernel: profiles/r05_potrf_diag_lab.txt; code in git history, its lane-level NumPy model in
// tools/emul_diag2.py.)

#include "tsvgp_chol.h"

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int NB = 128;         // block size of the factorisation (CH_NB)
constexpr int NTC = NB / 16;    // tile columns
constexpr int NTILES = NTC * (NTC + 1) / 2;  // lower tiles of the block

#define TSVGP_CHOL_PRIO 3

__device__ __forceinline__ v4d mfma(double a, double b, v4d c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// the `work` image: column j, slot u = tile (j + u, j), columns packed one after the other; a tile is [4 registers][64 lanes]
__device__ __forceinline__ int tile_index(int col, int slot) { return tsvgp_chol::work_tile_index(col, slot); }

// Panel rows below the diagonal block (and the right-hand-side rows that ride along, tsvgp_potrf_solve_f64):
//     P = A_panel inv(L_kk)^T     by substitution over the eight 16-wide column blocks, right-looking:
//     P_s = U_s inv(L_ss)^T,   U_s' -= P_s L_s's^T  (s' > s)
// One WAVE per 16-row strip, the strip's eight tiles in registers in the accumulator layout: the product with the inverted
// diagonal tile is four MFMAs whose B operands are the registers of U_s as they stand, and P_s's registers are in turn the
// B operands of the updates -- 144 MFMAs per strip against the 256 of the product with the assembled 128 x 128 inverse
// (round 4's chol_tile_kernel<0>), and no inverse to assemble.  The operands on the factor's side (the tiles L_s's and
// inv(L_ss), 36 KB) come from `work`, where potrf_diag_kernel left them in register layout: coalesced 512-byte loads.
// The factor-side operands of column block s + 1 are requested before the MFMAs of column block s (they do not depend on
// them): without that every stage sat out one L2 round trip per operand (40 us instead of 6).
constexpr int P2_THREADS = 256;
template <int S>
struct P2Ops {  // operands of column block S: inv(L_SS) and the tiles (s2, S), s2 > S
    double x[4];
    double l[NTC - 1 - S > 0 ? NTC - 1 - S : 1][4];
};
template <int S>
__device__ __forceinline__ void p2_load(P2Ops<S>& o, const double* __restrict__ Wb, int lane, int n, int G) {
    const double* Xb = Wb + (size_t)NTILES * 256 + S * 256 + n * 16 + G;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) o.x[kk] = Xb[4 * kk];
#pragma unroll
    for (int s2 = S + 1; s2 < NTC; ++s2) {
        const double* lt = Wb + (size_t)tile_index(S, s2 - S) * 256 + lane;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) o.l[s2 - S - 1][kk] = lt[kk * 64];
    }
}
// (The solved tiles stay in registers until the end: vmcnt counts loads and stores in one queue, so a store issued in stage s
// would make the wait for stage s + 1's operands sit out the store's round trip as well.)
template <int S>
__device__ __forceinline__ void p2_stage(v4d (&U)[NTC], const P2Ops<S>& o) {
    v4d ps = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) ps = mfma(o.x[kk], U[S][kk], ps);
#pragma unroll
    for (int s2 = S + 1; s2 < NTC; ++s2)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) U[s2] = mfma(-o.l[s2 - S - 1][kk], ps[kk], U[s2]);
    U[S] = ps;
}
// Strip I/O: a strip's 16 rows x 128 columns travel as whole 512-byte row halves (16 bytes per lane, two rows per
// instruction) and change layout in LDS -- read straight in the register layout (lane (n, G), tile s, register r <->
// [n][16 s + 4 r + G]: 16 x 32-byte pieces per 8-byte wave load) a strip took 6.2 us to load and 3.2 us to store, more than
// its 144 MFMAs (profiles/r05_potrf_diag_lab.txt).  One 64-column half at a time through a private [16][66] image per wave: row stride
// 66 doubles = 4 banks (mod 64 dwords), so the 8-byte register-layout accesses of a half wave hit 32 different bank pairs.
constexpr int P2_LD = 66;
typedef double v2d_ __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void strip_load(v4d (&U)[NTC], const double* __restrict__ Arow0, int lda, double* __restrict__ img, int lane,
                                           int n, int G) {
    v2d_ v[2][8];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 8; ++i)  // rows 2 i, 2 i + 1: lanes 0..31 / 32..63, 16 bytes each
            v[h][i] = *reinterpret_cast<const v2d_*>(Arow0 + (size_t)(2 * i + (lane >> 5)) * lda + 64 * h + 2 * (lane & 31));
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            double* d = img + (2 * i + (lane >> 5)) * P2_LD + 2 * (lane & 31);
            d[0] = v[h][i][0];
            d[1] = v[h][i][1];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int r = 0; r < 4; ++r) U[4 * h + s][r] = img[n * P2_LD + 16 * s + 4 * r + G];
    }
}
__device__ __forceinline__ void strip_store(const v4d (&U)[NTC], double* __restrict__ Arow0, int lda, double* __restrict__ img, int lane,
                                            int n, int G) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int r = 0; r < 4; ++r) img[n * P2_LD + 16 * s + 4 * r + G] = U[4 * h + s][r];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const double* d = img + (2 * i + (lane >> 5)) * P2_LD + 2 * (lane & 31);
            v2d_ v;
            v[0] = d[0];
            v[1] = d[1];
            *reinterpret_cast<v2d_*>(Arow0 + (size_t)(2 * i + (lane >> 5)) * lda + 64 * h + 2 * (lane & 31)) = v;
        }
    }
}

__global__ __launch_bounds__(P2_THREADS) __attribute__((amdgpu_waves_per_eu(1, 1))) void chol_panel2_kernel(
    double* __restrict__ A, int lda, int64_t stride, int k, const double* __restrict__ work, int nstrips) {
    __builtin_amdgcn_s_setprio(TSVGP_CHOL_PRIO);
    __shared__ double imgs[P2_THREADS / 64][16 * P2_LD];
    const int lane = threadIdx.x & 63, n = lane & 15, G = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int strip = blockIdx.x * (P2_THREADS / 64) + w;
    if (strip >= nstrips) return;
    double* Arow0 = A + (size_t)blockIdx.y * stride + (size_t)((k + 1) * NB + 16 * strip) * lda + (size_t)k * NB;
    const double* Wb = work + (size_t)blockIdx.y * NB * NB;
    P2Ops<0> o0;
    P2Ops<1> o1;
    P2Ops<2> o2;
    P2Ops<3> o3;
    P2Ops<4> o4;
    P2Ops<5> o5;
    P2Ops<6> o6;
    P2Ops<7> o7;
    v4d U[NTC];
    p2_load(o0, Wb, lane, n, G);
    strip_load(U, Arow0, lda, imgs[w], lane, n, G);
    p2_load(o1, Wb, lane, n, G);
    __builtin_amdgcn_sched_barrier(0);
    p2_stage(U, o0);
    p2_load(o2, Wb, lane, n, G);
    __builtin_amdgcn_sched_barrier(0);
    p2_stage(U, o1);
    p2_load(o3, Wb, lane, n, G);
    __builtin_amdgcn_sched_barrier(0);
    p2_stage(U, o2);
    p2_load(o4, Wb, lane, n, G);
    p2_load(o5, Wb, lane, n, G);
    __builtin_amdgcn_sched_barrier(0);
    p2_stage(U, o3);
    p2_load(o6, Wb, lane, n, G);
    p2_load(o7, Wb, lane, n, G);
    __builtin_amdgcn_sched_barrier(0);
    p2_stage(U, o4);
    p2_stage(U, o5);
    p2_stage(U, o6);
    p2_stage(U, o7);
    strip_store(U, Arow0, lda, imgs[w], lane, n, G);
}

}  // namespace

namespace tsvgp_chol {
hipError_t launch_panel2(double* A, int lda, int64_t stride, int k, const double* work, int nstrips, int batch,
                         hipStream_t stream) {
    if (nstrips <= 0) return hipSuccess;
    hipLaunchKernelGGL(chol_panel2_kernel, dim3((nstrips + P2_THREADS / 64 - 1) / (P2_THREADS / 64), batch), dim3(P2_THREADS), 0,
                       stream, A, lda, stride, k, work, nstrips);
    return hipGetLastError();
}

}  // namespace tsvgp_chol
