// tsvgp_mfma.h -- the MFMA wrappers and the 128 x 128 tile product of the N-sized kernels: Mfma, PanelK, load_run / store_run,
// row_block and the two mma_chunk_* (panel_kernel, the syrk family and selftest_kernel in tsvgp_kernels.hip, cov_kernel in
// tsvgp_predict.hip; tsvgp_grad.hip takes Mfma<T>::pair_t).  Only the units with tile products include it.  Not part of the C-ABI:
// include/tsvgp_hip.h is.  Everything sits in an anonymous namespace, as in tsvgp_device.h, and no __global__ function belongs
// here.  The cache caveat of tsvgp_device.h holds for this header too.
#pragma once

#include <hip/hip_runtime.h>

#include "tsvgp_device.h"

namespace {

constexpr int KC = 16;            // k-chunk of the site-accumulation kernel ([k][row] images)
constexpr int LDS_KS = 144;       // [k][row] image: k stride (elements)

// ---------------------------------------------------------------------------------------------------------------
// MFMA wrappers.  A operand: lane l holds A[i = l&15][k = l>>4]; B operand: lane l holds B[k = l>>4][j = l&15].
// C/D: column = l&15 for both types; row = (l>>4) + 4*r for f64, (l>>4)*4 + r for f32 (r = register index 0..3).
// ---------------------------------------------------------------------------------------------------------------
template <typename T>
struct Mfma;
template <>
struct Mfma<double> {
    typedef v4d acc_t;
    typedef v2d pair_t;
    static __device__ __forceinline__ acc_t run(double a, double b, acc_t c) {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ int row(int lane, int r) { return (lane >> 4) + 4 * r; }
};
template <>
struct Mfma<float> {
    typedef v4f acc_t;
    typedef v2f pair_t;
    static __device__ __forceinline__ acc_t run(float a, float b, acc_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ int row(int lane, int r) { return (lane >> 4) * 4 + r; }
};

// k-chunk of the panel kernels ([row][k] images): 16 doubles or 32 floats -- the same 128 bytes per row, the same 64
// bytes staged per thread and operand, and the same MFMA time between two barriers for both types (an fp32 MFMA takes
// half the cycles of an fp64 one; with 16-float chunks the barrier and the staging latency weigh twice as much).
// Row stride in elements: 17 doubles / 34 floats (18 for 16-float chunks) make the fragment reads (banked modulo 32
// dwords per group of 32 lanes) and the 8-byte staging writes conflict free.
template <typename T>
struct PanelK {
    static constexpr int KC = sizeof(T) == 8 ? 16 : 32;
    static constexpr int H = KC / 2;  // elements one thread stages per operand and chunk
    static constexpr int RS = KC + (sizeof(T) == 8 ? 1 : 2);
};

// H consecutive elements of one row: global -> registers (16-byte loads) and registers -> LDS (8-byte stores: the rows
// of the double image are only 8-byte aligned).
template <typename T, int H>
__device__ __forceinline__ void load_run(T (&r)[H], const T* __restrict__ p) {
    if constexpr (sizeof(T) == 8) {
#pragma unroll
        for (int q = 0; q < H / 2; ++q) {
            v2d v = *reinterpret_cast<const v2d*>(p + 2 * q);
            r[2 * q] = v[0];
            r[2 * q + 1] = v[1];
        }
    } else {
#pragma unroll
        for (int q = 0; q < H / 4; ++q) {
            v4f v = *reinterpret_cast<const v4f*>(p + 4 * q);
            r[4 * q] = v[0];
            r[4 * q + 1] = v[1];
            r[4 * q + 2] = v[2];
            r[4 * q + 3] = v[3];
        }
    }
}
template <typename T, int H>
__device__ __forceinline__ void store_run(T* p, const T (&r)[H]) {
    if constexpr (sizeof(T) == 8) {
#pragma unroll
        for (int q = 0; q < H; ++q) p[q] = r[q];
    } else {
#pragma unroll
        for (int q = 0; q < H / 2; ++q) {
            v2f v;
            v[0] = r[2 * q];
            v[1] = r[2 * q + 1];
            *reinterpret_cast<v2f*>(p + 2 * q) = v;
        }
    }
}

// Wave w (0..3) of a workgroup owns the 16-row blocks {w, 7 - w} and ALL eight 16-column blocks of the 128x128 tile
// (32 x 128 per wave, acc[2][8]).  Every wave therefore sees the same column structure -- the k-tile on the diagonal
// of a triangular product skips the same (chunk, column block) pairs in all waves, with compile-time masks -- and the
// row pairing {w, 7 - w} gives every wave 9 of its 16 accumulators on a diagonal tile of the symmetric product.
__device__ __forceinline__ int row_block(int w, int slot) { return slot == 0 ? w : 7 - w; }

// One k-chunk of MFMAs on [row][k] images: acc[s][n] += A(row block s) * B(column block n)^T.
// MLO / MHI (compile time): bit n set = column block n takes part in the first / second half of the chunk's k-steps
// (a 32-wide chunk spans two 16-wide k-blocks of a triangular operand; for 16-wide chunks both masks are equal).
template <typename T, int MLO, int MHI>
__device__ __forceinline__ void mma_chunk_rowk(typename Mfma<T>::acc_t (&acc)[2][8], const T* __restrict__ As,
                                               const T* __restrict__ Bs, int w, int lane) {
    constexpr int RS = PanelK<T>::RS, PKC = PanelK<T>::KC, NKS = PKC / 4;
    const int lr = lane & 15, lk = lane >> 4;
    const T* ap0 = As + (w * 16 + lr) * RS + lk;
    const T* ap1 = As + ((7 - w) * 16 + lr) * RS + lk;
    const T* bp = Bs + lr * RS + lk;
#pragma unroll
    for (int ks = 0; ks < PKC / 4; ++ks) {
        const int NMASK = (ks < PKC / 8) ? MLO : MHI;
        T a[2], b[8];
        a[0] = ap0[ks * 4];
        a[1] = ap1[ks * 4];
#pragma unroll
        for (int n = 0; n < 8; ++n)
            if (NMASK & (1 << n)) b[n] = bp[n * 16 * RS + ks * 4];
#pragma unroll
        for (int n = 0; n < 8; ++n)
            if (NMASK & (1 << n)) {
                acc[0][n] = Mfma<T>::run(a[0], b[n], acc[0][n]);
                acc[1][n] = Mfma<T>::run(a[1], b[n], acc[1][n]);
            }
    }
}

// One k-chunk (16) of MFMAs on [k][row] images.  DIAG: only accumulators with column block <= row block
// (W = the wave index, compile time, selects the row blocks {W, 7 - W}).
template <typename T, bool DIAG, int W>
__device__ __forceinline__ void mma_chunk_krow(typename Mfma<T>::acc_t (&acc)[2][8], const T* __restrict__ As,
                                               const T* __restrict__ Bs, int w, int lane) {
    const int lr = lane & 15, lk = lane >> 4;
    const T* ap0 = As + lk * LDS_KS + w * 16 + lr;
    const T* ap1 = As + lk * LDS_KS + (7 - w) * 16 + lr;
    const T* bp = Bs + lk * LDS_KS + lr;
#pragma unroll
    for (int ks = 0; ks < KC / 4; ++ks) {
        T a[2], b[8];
        a[0] = ap0[ks * 4 * LDS_KS];
        a[1] = ap1[ks * 4 * LDS_KS];
#pragma unroll
        for (int n = 0; n < 8; ++n)
            if (!DIAG || n <= 7 - W || n <= W) b[n] = bp[ks * 4 * LDS_KS + n * 16];
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            if (!DIAG || n <= W) acc[0][n] = Mfma<T>::run(a[0], b[n], acc[0][n]);
            if (!DIAG || n <= 7 - W) acc[1][n] = Mfma<T>::run(a[1], b[n], acc[1][n]);
        }
    }
}

}  // namespace
