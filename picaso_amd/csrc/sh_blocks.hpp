// Building blocks of the spherical-harmonics kernels (sh_sweep.hip, sh_thermal.hip, sh_clear.hip): clipped
// exponentials, division by a constant, the NB x NB block algebra in its two forms and the written-out modes.
#pragma once

#include "common.hpp"
#include "device_math.hpp"

namespace pz {

__device__ __forceinline__ double clip35(double x) { return fmin(fmax(x, -35.0), 35.0); }   // slice_rav
constexpr double LOG2E = LOG2E_D;
constexpr double EXP_M35 = 6.305116760146989e-16;        // exp(-35)
// exp(-clip35(y/u)) for y >= 0 given t = y * (-log2(e)/u): only the lower clip can bind
__device__ __forceinline__ double fexp2_clip(double t, const Exp2Coef &K) { return fexp2(fmax(t, -35.0 * LOG2E), K); }

// x / d for a compile-time divisor, correctly rounded like the division it replaces, in 3 instructions
// instead of the 11 of v_div_scale / v_rcp / v_div_fmas / v_div_fixup: q = x RN(1/d), r = x - d q (exact in
// the fma), q' = q + r RN(1/d) (Markstein's quotient refinement; checked against x/d on 2e5 values each for
// d = 9 and d = 4 pi).  Four such divisions per layer (three /9 in the SH4 quartic, one /(4 pi) in the
// single-scattering term, fluxes.py:3388-3391, :2959) were 7 % of the SH4 kernel.
__device__ __forceinline__ double div_const(double x, double d, double rd)
{
#pragma clang fp contract(off)
    const double q = x * rd;
    const double r = fma(-d, q, x);
    return fma(r, rd, q);
}
constexpr double R9 = 1.0 / 9.0, FOURPI = 4 * PI, R4PI = 1.0 / (4 * PI);

__device__ __forceinline__ void legP4(double mu, double (&P)[4])   // fluxes.py:3639-3646, l = 0..3
{
    P[0] = 1;
    P[1] = mu;
    P[2] = (3 * mu * mu - 1) / 2;
    P[3] = (5 * mu * mu * mu - 3 * mu) / 2;
}

template <int NB>
struct Blk {
    double m[NB][NB];
};

template <int NB>
__device__ __forceinline__ Blk<NB> scale_cols(const Blk<NB> &A, const double (&e)[NB])   // A diag(e)
{
    Blk<NB> R;
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) R.m[i][j] = A.m[i][j] * e[j];
    return R;
}

// The block algebra exists twice, and the two families give different bits.
//   mm mv mtv inv dot            sums of products as written: whether a product and the sum after it become one fma
//                                is the compiler's choice (no pragma: the build's contraction mode).  Used by
//                                sh_body (sh_sweep.hip), whose results the tests pin as they are.
//   mmx mvx mtvx invx dotx subx  every fma written out and contraction off inside each function: the value does not
//                                depend on what the compiler finds around the call, so an angle's result stays the
//                                same however many angles share its lane.  Used by k_sh_thermal (sh_thermal.hip)
//                                and k_sh4_clear (sh_clear.hip).
// Tried once: sh_body on the ...x forms changes the instruction stream of all ten k_sh / k_sh_refl kernels, and with
// it their results.  The families stay apart until sh_body itself is written without contraction.
template <int NB>
__device__ __forceinline__ Blk<NB> mm(const Blk<NB> &A, const Blk<NB> &B)
{
    Blk<NB> C;
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < NB; ++k) s += A.m[i][k] * B.m[k][j];
            C.m[i][j] = s;
        }
    return C;
}
template <int NB>
__device__ __forceinline__ Blk<NB> mmx(const Blk<NB> &A, const Blk<NB> &B)
{
#pragma clang fp contract(off)
    Blk<NB> C;
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            double s = A.m[i][0] * B.m[0][j];
#pragma unroll
            for (int k = 1; k < NB; ++k) s = fma(A.m[i][k], B.m[k][j], s);
            C.m[i][j] = s;
        }
    return C;
}

template <int NB>
__device__ __forceinline__ void mv(const Blk<NB> &A, const double (&x)[NB], double (&y)[NB])
{
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < NB; ++k) s += A.m[i][k] * x[k];
        y[i] = s;
    }
}
template <int NB>
__device__ __forceinline__ void mvx(const Blk<NB> &A, const double (&x)[NB], double (&y)[NB])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        double s = A.m[i][0] * x[0];
#pragma unroll
        for (int k = 1; k < NB; ++k) s = fma(A.m[i][k], x[k], s);
        y[i] = s;
    }
}

template <int NB>
__device__ __forceinline__ void mtv(const Blk<NB> &A, const double (&x)[NB], double (&y)[NB])   // A^T x
{
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < NB; ++k) s += A.m[k][i] * x[k];
        y[i] = s;
    }
}
template <int NB>
__device__ __forceinline__ void mtvx(const Blk<NB> &A, const double (&x)[NB], double (&y)[NB])   // A^T x
{
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        double s = A.m[0][i] * x[0];
#pragma unroll
        for (int k = 1; k < NB; ++k) s = fma(A.m[k][i], x[k], s);
        y[i] = s;
    }
}

template <int NB>
__device__ __forceinline__ double dot(const double (&a)[NB], const double (&b)[NB])
{
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < NB; ++i) s += a[i] * b[i];
    return s;
}
template <int NB>
__device__ __forceinline__ double dotx(const double (&a)[NB], const double (&b)[NB])
{
#pragma clang fp contract(off)
    double s = a[0] * b[0];
#pragma unroll
    for (int i = 1; i < NB; ++i) s = fma(a[i], b[i], s);
    return s;
}

template <int NB>
__device__ __forceinline__ Blk<NB> inv(const Blk<NB> &A)
{
    Blk<NB> R;
    if (NB == 1) {
        R.m[0][0] = frcp(A.m[0][0]);
    } else {
        const double idet = frcp(A.m[0][0] * A.m[NB - 1][NB - 1] - A.m[0][NB - 1] * A.m[NB - 1][0]);
        R.m[0][0] = A.m[NB - 1][NB - 1] * idet;
        R.m[NB - 1][NB - 1] = A.m[0][0] * idet;
        R.m[0][NB - 1] = -A.m[0][NB - 1] * idet;
        R.m[NB - 1][0] = -A.m[NB - 1][0] * idet;
    }
    return R;
}
template <int NB>
__device__ __forceinline__ Blk<NB> invx(const Blk<NB> &A)
{
#pragma clang fp contract(off)
    Blk<NB> R;
    if (NB == 1) {
        R.m[0][0] = frcp(A.m[0][0]);
    } else {
        const double idet = frcp(fma(A.m[0][0], A.m[NB - 1][NB - 1], -(A.m[0][NB - 1] * A.m[NB - 1][0])));
        R.m[0][0] = A.m[NB - 1][NB - 1] * idet;
        R.m[NB - 1][NB - 1] = A.m[0][0] * idet;
        R.m[0][NB - 1] = -(A.m[0][NB - 1] * idet);
        R.m[NB - 1][0] = -(A.m[NB - 1][0] * idet);
    }
    return R;
}

template <int NB>
__device__ __forceinline__ Blk<NB> subx(const Blk<NB> &A, const Blk<NB> &B)
{
#pragma clang fp contract(off)
    Blk<NB> C;
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) C.m[i][j] = A.m[i][j] - B.m[i][j];
    return C;
}

// The modes of a layer with the arithmetic written out like the ...x family (fluxes.py:3388-3434, 3245-3251), for
// the two kernels that use it.  sh_body has its own (sh_sweep.hip).
struct ModesT4 { double lam[2], E[2], iE[2], R[2], Q[2], S[2], beta, gama; Blk<2> Mn, Pl; };
__device__ __forceinline__ void modes_sh4x(const double (&a)[4], double dt, ModesT4 &M, const Exp2Coef &K)
{
#pragma clang fp contract(off)
    const double a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];
    const double a01 = a0 * a1;
    const double beta = (a01 + div_const(4 * (a0 * a3), 9.0, R9)) + div_const(a2 * a3, 9.0, R9);
    const double gama = div_const((a01 * a2) * a3, 9.0, R9);
    M.beta = beta;
    M.gama = gama;
    const double disc = fsqrt(fma(beta, beta, -(4 * gama)));
    const double x1 = 0.5 * (beta + disc), x2 = 0.5 * (beta - disc);
    const double il1 = frsq(x1), il2 = frsq(x2);
    const double l1 = x1 * il1, l2 = x2 * il2;
    M.lam[0] = l1;
    M.lam[1] = l2;
    const double s3 = -1.5 * frcp(a3);
    const double R1 = -(a0 * il1), R2 = -(a0 * il2);
    const double Q1 = 0.5 * fma(a01 * il1, il1, -1.0), Q2 = 0.5 * fma(a01 * il2, il2, -1.0);
    const double S1 = s3 * fma(a01, il1, -l1), S2 = s3 * fma(a01, il2, -l2);
    M.R[0] = R1; M.R[1] = R2; M.Q[0] = Q1; M.Q[1] = Q2; M.S[0] = S1; M.S[1] = S2;
    const double tp = 2 * PI, q1 = 0.625 * Q1, q2 = 0.625 * Q2;
    M.Pl.m[0][0] = ((0.5 + R1) + q1) * tp;
    M.Pl.m[0][1] = ((0.5 + R2) + q2) * tp;
    M.Pl.m[1][0] = ((-0.125 + q1) + S1) * tp;
    M.Pl.m[1][1] = ((-0.125 + q2) + S2) * tp;
    M.Mn.m[0][0] = ((0.5 - R1) + q1) * tp;
    M.Mn.m[0][1] = ((0.5 - R2) + q2) * tp;
    M.Mn.m[1][0] = ((-0.125 + q1) - S1) * tp;
    M.Mn.m[1][1] = ((-0.125 + q2) - S2) * tp;
    M.E[0] = fexpk(-clip35(l1 * dt), K);
    M.E[1] = fexpk(-clip35(l2 * dt), K);
    M.iE[0] = frcp(M.E[0]);
    M.iE[1] = frcp(M.E[1]);
}
struct ModesT2 { double lam[1], E[1], iE[1], q; Blk<1> Mn, Pl; };
__device__ __forceinline__ void modes_sh2x(const double (&a)[2], double dt, ModesT2 &M, const Exp2Coef &K)
{
#pragma clang fp contract(off)
    const double lam = fsqrt(a[0] * a[1]);
    M.lam[0] = lam;
    M.q = lam * frcp(a[1]);
    M.Mn.m[0][0] = (0.5 + M.q) * (2 * PI);
    M.Pl.m[0][0] = (0.5 - M.q) * (2 * PI);
    M.E[0] = fexpk(-clip35(lam * dt), K);
    M.iE[0] = frcp(M.E[0]);
}

}  // namespace pz
