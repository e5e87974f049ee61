// tsvgp_device.h -- what more than one translation unit of libtsvgp_hip.so uses, and nothing else: the tile constants and vector
// types, the Gauss-Hermite tables with the Gaussian / Bernoulli map lik_eval (the moments epilogues of tsvgp_kernels.hip,
// vgp_rows_kernel of tsvgp_vgp.hip, lik_map_kernel and diag_site_step_kernel of tsvgp_likmap.hip), the kernel profiles k(s) and
// k'(s) with exp_nonpos, and launch_status.  The MFMA wrappers and the tile product, which only the units with tile products
// need, are in tsvgp_mfma.h.  Not part of the C-ABI: include/tsvgp_hip.h is.  Everything sits in an anonymous namespace: every unit
// compiles its own copy and exports none of it.  No __global__ function belongs here (each unit that includes the header would
// emit it again).
//
// The cached assembly of the `product_asm` fixture (tests/conftest.py) is keyed by the hash of tsvgp_kernels.hip and
// include/tsvgp_hip.h ONLY: after an edit to this header alone (as to tsvgp_mfma.h or tsvgp_chol.h) remove tsvgp_kernels_*.s from
// the temporary directory by hand, or the ISA lint and the register-budget test read the assembly of the previous build.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "tsvgp_hip.h"

namespace {

constexpr int TILE = TSVGP_TILE;  // 128
constexpr int NTHREADS = 256;
constexpr int FILL_COLS = 512;  // columns per workgroup of se_fill_kernel and kgrad_kernel: two adjacent columns per thread
constexpr int COV_XS = 33;  // X panel image: row stride in elements (D <= 32; odd: the 16 rows of a fragment column hit 16 banks)

typedef double v4d __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));
typedef float v2f __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------------------------------------------
// Likelihood maps (fp64; round 5: the Bernoulli quadrature of fp32 N-arrays in fp32, bern_sums_f below).  Restates gpflow.likelihoods.{Gaussian,Bernoulli}.variational_expectations
// and its tf.GradientTape derivative (reference src/models/tsvgp.py:256-263).
// ---------------------------------------------------------------------------------------------------------------
__device__ const double GH_X[10] = {  // positive nodes of 20-pt Gauss-Hermite, times sqrt(2)
    3.46964157081355917e-01, 1.04294534880275114e+00, 1.74524732081412703e+00, 2.45866361117236787e+00,
    3.18901481655339003e+00, 3.94396735065731630e+00, 4.73458133404605519e+00, 5.57873880589320148e+00,
    6.51059015701365507e+00, 7.61904854167975909e+00};
__device__ const double GH_W[10] = {  // matching weights / sqrt(pi)
    2.60793063449554885e-01, 1.61739333983999978e-01, 6.15063720639768968e-02, 1.39978374471010220e-02,
    1.83010313108049002e-03, 1.28826279961929280e-04, 4.40212109023085101e-06, 6.12749025998292797e-08,
    2.48206236231517553e-10, 1.25780067243792340e-13};

__device__ __forceinline__ void bern_point(double f, bool y1, double& lp, double& dl) {
    const double jit = 1e-3;
    const double p = 0.5 * (1.0 + erf(f * 0.70710678118654752440)) * (1.0 - 2.0 * jit) + jit;
    const double dp = (1.0 - 2.0 * jit) * 0.39894228040143267794 * exp(-0.5 * f * f);
    if (y1) {
        lp = log(p);
        dl = dp / p;
    } else {
        const double q = 1.0 - p;
        lp = log(q);
        dl = -dp / q;
    }
}

// Gauss-Hermite partial sums over the node pairs [i0, i1) of the Bernoulli map (two threads share a row in the panel kernel)
__device__ __forceinline__ void bern_sums(double m, double sd, bool y1, int i0, int i1, double& a0, double& a1, double& av) {
    a0 = a1 = av = 0.0;
#pragma unroll 1
    for (int i = i0; i < i1; ++i) {
        const double z = GH_X[i], w = GH_W[i];
        double lp, dl;
        bern_point(m + sd * z, y1, lp, dl);
        av += w * lp;
        a0 += w * dl;
        a1 += w * dl * z;
        bern_point(m - sd * z, y1, lp, dl);
        av += w * lp;
        a0 += w * dl;
        a1 -= w * dl * z;
    }
}

// The same sums in fp32, for the fp32 N-arrays (round 5): mean and variance arrive with 1e-6 of relative error from the fp32 MFMA
// sums, and the fp64 quadrature -- 20 x (erf, exp, log, a division) per row on four waves per CU -- was 0.30 ms of the 8.0 ms fp32
// moments kernel at N = 1e6 (profiles/r05_lik_split_lab.txt).  The class probability is formed from erfc of the signed argument,
// never as 1 - p: p saturates at 1 - 1e-3, where 1 - p in fp32 would keep four digits.
__device__ const float GH_XF[10] = {3.46964157e-01f, 1.04294535e+00f, 1.74524732e+00f, 2.45866361e+00f, 3.18901482e+00f,
                                    3.94396735e+00f, 4.73458133e+00f, 5.57873881e+00f, 6.51059016e+00f, 7.61904854e+00f};
__device__ const float GH_WF[10] = {2.60793063e-01f, 1.61739334e-01f, 6.15063721e-02f, 1.39978374e-02f, 1.83010313e-03f,
                                    1.28826280e-04f, 4.40212109e-06f, 6.12749026e-08f, 2.48206236e-10f, 1.25780067e-13f};
__device__ __forceinline__ void bern_point_f(float f, bool y1, float& lp, float& dl) {
    const float jit = 1e-3f;
    const float pp = 0.5f * erfcf((y1 ? -f : f) * 0.70710678f) * (1.0f - 2.0f * jit) + jit;  // p(y | f), >= 1e-3
    const float dp = (1.0f - 2.0f * jit) * 0.39894228f * expf(-0.5f * f * f);
    lp = logf(pp);
    dl = (y1 ? dp : -dp) / pp;
}
__device__ __forceinline__ void bern_sums_f(float m, float sd, bool y1, int i0, int i1, float& a0, float& a1, float& av) {
    a0 = a1 = av = 0.0f;
#pragma unroll 1
    for (int i = i0; i < i1; ++i) {
        const float z = GH_XF[i], w = GH_WF[i];
        float lp, dl;
        bern_point_f(m + sd * z, y1, lp, dl);
        av += w * lp;
        a0 += w * dl;
        a1 += w * dl * z;
        bern_point_f(m - sd * z, y1, lp, dl);
        av += w * lp;
        a0 += w * dl;
        a1 -= w * dl * z;
    }
}
// The quadrature in the arithmetic of the N-arrays' type T (fp64 for both up to round 5 -- profiles/r05_lik_split_lab.txt)
template <typename T>
__device__ __forceinline__ void bern_sums_t(double m, double sd, bool y1, int i0, int i1, double& a0, double& a1, double& av) {
    if constexpr (sizeof(T) == 4) {
        float b0, b1, bv;
        bern_sums_f((float)m, (float)sd, y1, i0, i1, b0, b1, bv);
        a0 = (double)b0;
        a1 = (double)b1;
        av = (double)bv;
    } else {
        bern_sums(m, sd, y1, i0, i1, a0, a1, av);
    }
}

__device__ __forceinline__ void lik_eval(int lik_flags, double s2, double m, double v, double y, double& g0, double& g1,
                                         double& ve) {
    const int lik = lik_flags & 0xFF;
    if (lik == TSVGP_LIK_GAUSSIAN) {
        const double r = y - m;
        g0 = r / s2;
        g1 = -0.5 / s2;
        ve = -0.5 * 1.83787706640934548356 - 0.5 * log(s2) - 0.5 * (r * r + v) / s2;
    } else {  // Bernoulli, probit, 20-pt Gauss-Hermite; derivative OF the quadrature sum
        const double sd = sqrt(v);
        double a0, a1, av;
        bern_sums(m, sd, y == 1.0, 0, 10, a0, a1, av);
        g0 = a0;
        g1 = a1 / (2.0 * sd);
        ve = av;
    }
    if (!(lik_flags & TSVGP_LIK_NOCROP)) g1 = fmin(g1, -1e-8);  // reference tsvgp.py:262-263 (tsvgp_white.py does not crop)
}

// exp(a) for a <= 0 (every kernel profile below).  fp64: the device library's algorithm restated -- k = rint(a log2 e),
// r = a - k ln2 (two-term), degree-11 polynomial, ldexp; same constants, same operation order, bit-identical values
// -- minus what a <= 0 does not need and with the coefficients as FMA addends: 22 VALU instructions instead of the 33
// the library call compiles to (9 of them register copies in front of v_fmac, 5 for the overflow / underflow selects).
// The K(X, Z) fill is VALU-issue bound (108 fp64-rate instructions per row pair, 1.66 ms of arithmetic against 1.35 ms
// of stores at N = 1e6, M = 1024), so this is 24 % of its arithmetic.  Below -1080 the result is 0 as in the library
// (ldexp underflows); NaN stays NaN.
template <typename T>
__device__ __forceinline__ T exp_nonpos(T a) {
    return exp(a);
}
// fp32: the hardware exponential, v_exp_f32(a log2 e) -- two instructions where the library's range-reduced expf takes thirteen
// (a quarter-rate v_exp_f32 among them either way): with the packed distance loop the exponentials were half of the fp32 fill's
// issue time.  Relative error ~|a| 2^-24 (the product a log2 e is rounded once), i.e. <= 1e-5 for kernel values down to 1e-30 and
// far inside the fp32 path's stated tolerance against the fp64 reference values (atol 1e-4 + rtol 1e-3); results below the
// normal range flush to zero.
template <>
__device__ __forceinline__ float exp_nonpos<float>(float a) {
    return __expf(a);
}
template <>
__device__ __forceinline__ double exp_nonpos<double>(double a) {
    constexpr auto C = [](unsigned long long bits) { return __builtin_bit_cast(double, bits); };
    a = (a < -1080.0) ? -1080.0 : a;
    const double k = __builtin_rint(a * C(0x3ff71547652b82feULL));
    double r = fma(C(0xbfe62e42fefa39efULL), k, a);
    r = fma(C(0xbc7abc9e3b39803fULL), k, r);
    // q <- r q + c with c in a scalar register pair (VOP3 takes one scalar operand): left to itself the compiler keeps the
    // coefficients in VGPRs and copies each one in front of a destructive v_fmac
    auto horner = [](double r_, double q_, double c) {
        double d;
        asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(r_), "v"(q_), "s"(c));
        return d;
    };
    double q = horner(r, C(0x3e5ade156a5dcb37ULL), C(0x3e928af3fca7ab0cULL));
    q = horner(r, q, C(0x3ec71dee623fde64ULL));
    q = horner(r, q, C(0x3efa01997c89e6b0ULL));
    q = horner(r, q, C(0x3f2a01a014761f6eULL));
    q = horner(r, q, C(0x3f56c16c1852b7b0ULL));
    q = horner(r, q, C(0x3f81111111122322ULL));
    q = horner(r, q, C(0x3fa55555555502a1ULL));
    q = horner(r, q, C(0x3fc5555555555511ULL));
    q = horner(r, q, C(0x3fe000000000000bULL));
    q = fma(r, q, 1.0);
    q = fma(r, q, 1.0);
    return ldexp(q, (int)k);
}

// stationary kernel profile k(s) as a function of the scaled squared distance s = sum_d ((x_d - z_d) / l_d)^2
// (GPflow [ext]: Matern kernels take r = sqrt(max(s, 1e-36)))
template <int KIND, typename T>
__device__ __forceinline__ T kernel_profile(T s) {
    if constexpr (KIND == TSVGP_KERNEL_SE) {
        return exp_nonpos(T(-0.5) * s);
    } else {
        const T r = sqrt(s > T(1e-36) ? s : T(1e-36));
        if constexpr (KIND == TSVGP_KERNEL_MATERN32) {
            const T a = T(1.7320508075688772935) * r;
            return (T(1) + a) * exp_nonpos(-a);
        } else {
            const T a = T(2.2360679774997896964) * r;
            return (T(1) + a + T(5.0 / 3.0) * r * r) * exp_nonpos(-a);
        }
    }
}

// k(s) and k'(s) together, in closed form (the comment block above kgrad_kernel, tsvgp_grad.hip)
template <int KIND, typename T>
__device__ __forceinline__ void kernel_profile_grad(T s, T& f, T& df) {
    if constexpr (KIND == TSVGP_KERNEL_SE) {
        f = exp(T(-0.5) * s);
        df = T(-0.5) * f;
    } else {
        const T r = sqrt(s > T(1e-36) ? s : T(1e-36));
        if constexpr (KIND == TSVGP_KERNEL_MATERN32) {
            const T a = T(1.7320508075688772935) * r, e = exp(-a);
            f = (T(1) + a) * e;
            df = T(-1.5) * e;
        } else {
            const T a = T(2.2360679774997896964) * r, e = exp(-a);
            f = (T(1) + a + T(5.0 / 3.0) * r * r) * e;
            df = T(-5.0 / 6.0) * (T(1) + a) * e;
        }
    }
}

inline int launch_status() { return hipGetLastError() == hipSuccess ? TSVGP_OK : TSVGP_ELAUNCH; }

}  // namespace
