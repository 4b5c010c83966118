// Spherical-harmonics (SH2 / SH4) reflected light and thermal emission, the general sweep -- gfx950.
//
// Replaces fluxes.get_reflected_SH / get_thermal_SH with setup_2_stream_fluxes,
// setup_4_stream_fluxes and solve_4_stream_banded (reference picaso/fluxes.py:2675-3628).  The
// reference assembles a banded matrix (5 diagonals for SH2, 11 for SH4: 3.2 GB at 1e5 x 90) per
// angle and calls LAPACK dgbsv per wavelength.  Here nothing is assembled: per layer the stream
// coefficients split into NB = stream/2 decaying-mode unknowns d and NB growing-mode unknowns
// u = E v (E = diag exp(-lambda_m dtau), so v is the bounded value at the layer bottom); with the
// NB x NB blocks Mn, Pl of the reference's boundary rows the moment fluxes are
//     top :  Fmn = Mn d + Pl E v + zmn_dn      Fpl = Pl d + Mn E v + zpl_dn
//     bot :  Fmn = Mn E d + Pl v + zmn_up      Fpl = Pl E d + Mn v + zpl_up
// (SH4: Mn = [[p1mn,p2mn],[q1mn,q2mn]], Pl = [[p1pl,p2pl],[q1pl,q2pl]], fluxes.py:3427-3543;
//  SH2: Mn = Q1, Pl = Q2, fluxes.py:3251-3301).  One top-down sweep carries the relation
// d_i = delta_i - R_i v_i that everything above imposes on layer i and the TOA functional
// J = kappa + zeta.v_i of the source-function integrals (fluxes.py:2898-2970, 3105-3182); the
// surface rows fix v_{n-1}.  Only decaying exponentials appear, the blocks are the physical
// reflection operators, and no pivoting across layers is needed: tools/sh_sweep_numpy.py agrees
// with the reference's pivoted LAPACK solve to 2e-13 on thin, thick (35-clipped) and conservative
// columns (tests/test_single_sweep_numpy.py).  One lane per wavelength, every plane read once per
// angle, coalesced in the reference's (nlayer, nwno) layout.
//
// Reference quirk kept: in the TTHG branch f_deltaM is multiplied in place once per angle
// (fluxes.py:2823-2824), so angle k (in (g,t) order) sees f_deltaM * fac^(k+1).
#include "sh.hpp"
#include "sh_blocks.hpp"

#pragma clang fp contract(fast)   // sh_body leaves contraction to the compiler; the tests pin its results as they are

namespace pz {

// Per-layer mode structure from the a_l coefficients.
template <int NB>
struct Modes {
    double lam[NB], E[NB];
    Blk<NB> Mn, Pl;
    double cA[2 * NB][2 * NB];   // A[j][m] of fluxes.py:3601-3605 (SH4); unused for SH2
    double q;                    // SH2: lam/a1
    double beta, gama;           // SH4 quartic coefficients (particular solution)
};

// SH4: the quartic's coefficients, its two roots lam_r with 1/lam_r = il[r], and E
__device__ __forceinline__ void sh4_roots(const double (&a)[4], double dt, Modes<2> &M, double (&il)[2],
                                          const Exp2Coef &K)
{
    const double a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];
    M.beta = a0 * a1 + div_const(4 * a0 * a3, 9.0, R9) + div_const(a2 * a3, 9.0, R9);   // fluxes.py:3388-3391
    M.gama = div_const(a0 * a1 * a2 * a3, 9.0, R9);
    const double disc = fsqrt(M.beta * M.beta - 4 * M.gama);
    // lam = x rsqrt(x) and 1/lam = rsqrt(x) from one v_rsq_f64 + Newton (frsq, ~1 ulp) instead of a
    // correctly rounded sqrt followed by a reciprocal (fluxes.py:3393-3394, 3423-3425)
    const double x1 = (M.beta + disc) / 2, x2 = (M.beta - disc) / 2;
    il[0] = frsq(x1);
    il[1] = frsq(x2);
    M.lam[0] = x1 * il[0];
    M.lam[1] = x2 * il[1];
    M.E[0] = fexpk(-clip35(M.lam[0] * dt), K);                        // :3418-3421
    M.E[1] = fexpk(-clip35(M.lam[1] * dt), K);
}

// SH4: the blocks Pl, Mn and the coefficients A[j][m] from the roots and ia3 = 1/a3
__device__ __forceinline__ void sh4_blocks(const double (&a)[4], const double (&il)[2], double ia3, Modes<2> &M)
{
    const double a0 = a[0], a1 = a[1];
    const double il1 = il[0], il2 = il[1], l1 = M.lam[0], l2 = M.lam[1];
    const double a01 = a0 * a1, s3 = -1.5 * ia3;
    const double R1 = -a0 * il1, R2 = -a0 * il2;                      // :3423-3425
    const double Q1 = 0.5 * (a01 * il1 * il1 - 1), Q2 = 0.5 * (a01 * il2 * il2 - 1);
    const double S1 = s3 * (a01 * il1 - l1), S2 = s3 * (a01 * il2 - l2);
    const double tp = 2 * PI;
    M.Pl.m[0][0] = (0.5 + R1 + 5 * Q1 / 8) * tp;                      // p1pl  :3427-3434
    M.Pl.m[0][1] = (0.5 + R2 + 5 * Q2 / 8) * tp;                      // p2pl
    M.Pl.m[1][0] = (-0.125 + 5 * Q1 / 8 + S1) * tp;                   // q1pl
    M.Pl.m[1][1] = (-0.125 + 5 * Q2 / 8 + S2) * tp;                   // q2pl
    M.Mn.m[0][0] = (0.5 - R1 + 5 * Q1 / 8) * tp;                      // p1mn
    M.Mn.m[0][1] = (0.5 - R2 + 5 * Q2 / 8) * tp;                      // p2mn
    M.Mn.m[1][0] = (-0.125 + 5 * Q1 / 8 - S1) * tp;                   // q1mn
    M.Mn.m[1][1] = (-0.125 + 5 * Q2 / 8 - S2) * tp;                   // q2mn
    // A[j][m], m = (d0, u0, d1, u1)
    const double Aj[4][4] = {{1, 1, 1, 1}, {R1, -R1, R2, -R2}, {Q1, Q1, Q2, Q2}, {S1, -S1, S2, -S2}};
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int m = 0; m < 4; ++m) M.cA[j][m] = Aj[j][m];
}

__device__ __forceinline__ void modes_sh4(const double (&a)[4], double dt, Modes<2> &M, const Exp2Coef &K)
{
    double il[2];
    sh4_roots(a, dt, M, il, K);
    sh4_blocks(a, il, frcp(a[3]), M);
}

// modes_sh4 for reflected light with the layer's six independent reciprocals -- 1/a3, 1/Delta(1/u0) of the particular
// solution (:3397), 1/((1/u1)^2 - lam_r^2) and 1/E_r of the source-function weights (:2929-2937) -- taken from ONE
// v_rcp_f64 + Newton core (Montgomery's trick: prefix products, one reciprocal, 2 multiplies per value on the way back;
// 23 instructions instead of 6 x 5, and five fewer quarter-rate v_rcp_f64).  The six values of a layer span
// 1e-31 (E at the 35 clip, twice) .. 1e9 (Delta at grazing incidence): their product stays far inside the fp64 range.
struct ShRcp { double iDel, rab[2], iE[2]; };
__device__ __forceinline__ void modes_sh4_batched(const double (&a)[4], double dt, double iu0, double iu1, Modes<2> &M,
                                                  ShRcp &Q, const Exp2Coef &K)
{
    double il[2];
    sh4_roots(a, dt, M, il, K);
    const double l1 = M.lam[0], l2 = M.lam[1];
    const double xx = iu0 * iu0;
    const double v0 = a[3], v1 = 9 * (xx * xx - M.beta * xx + M.gama), v2 = (iu1 + l1) * (iu1 - l1),
                 v3 = (iu1 + l2) * (iu1 - l2), v4 = M.E[0], v5 = M.E[1];
    const double p1 = v0 * v1, p2 = p1 * v2, p3 = p2 * v3, p4 = p3 * v4, p5 = p4 * v5;
    double r = frcp(p5);
    Q.iE[1] = r * p4;
    r *= v5;
    Q.iE[0] = r * p3;
    r *= v4;
    Q.rab[1] = r * p2;
    r *= v3;
    Q.rab[0] = r * p1;
    r *= v2;
    Q.iDel = r * v0;
    r *= v1;                                                          // 1/a3
    sh4_blocks(a, il, r, M);
}

__device__ __forceinline__ void modes_sh2(const double (&a)[2], double dt, Modes<1> &M, const Exp2Coef &K)
{
    const double lam = sqrt(a[0] * a[1]);                             // fluxes.py:3245
    M.lam[0] = lam;
    M.q = lam * frcp(a[1]);                                           // :3251
    M.Mn.m[0][0] = (0.5 + M.q) * 2 * PI;                              // Q1
    M.Pl.m[0][0] = (0.5 - M.q) * 2 * PI;                              // Q2
    M.E[0] = fexpk(-clip35(lam * dt), K);                             // :3246-3248
}

// One kernel for stream 2 / 4 (NB = 1 / 2), reflected / thermal.
// FAST: the reference's default SH options (config.json: TTHG weights for single and multiple
// scattering, TTHG single-scattering phase function, Rayleigh in all three, explicit single form,
// frac_c = 2) fixed at compile time: the nine option words are branches inside the layer loop otherwise.
#ifndef PZ_SH_MINWAVES
#define PZ_SH_MINWAVES 2
#endif
// DRVT (FAST reflected kernels): the level planes tau and tau_og are not in HBM (NULL).  compute_opacity forms them as
// running sums of dtau / dtau_og from 0 at the top (optics.py:353-354, 418-420), so the beam exponentials of a level,
// exp(-tau/u0) and exp(-tau_og/u0), are running PRODUCTS of the layers' exp(-dtau/u0): carried unclipped down the column,
// one multiply per layer -- in the symmetric geometry (u0 == u1) by exp(-dtau/u1), which the layer needs anyway, so
// two of its five exponentials (15 instructions each) and three of its eleven loads go; other geometries pay one
// exponential for the two.  The reference's clipped form exp(-clip35(tau/u0)) (:3418-3421) is max(., e^-35) of the
// unclipped one.  A column's value differs from the plane-reading kernel's by the rounding of the product (<= n ulp).
template <int NB, bool THERMAL, bool FLX, bool FAST, bool DRVT, typename AnglePtr>
__device__ __forceinline__ void sh_body(const SHArgs &a, AnglePtr angp)
{
    static_assert(!DRVT || (FAST && !THERMAL && !FLX), "derived level planes: the default-options reflected kernels");
    constexpr int NS = 2 * NB;      // stream
    // 1-D grid, XCD-aware order.  Consecutive workgroups go to consecutive XCDs (8 of them, each with
    // its own L2), and every angle re-reads the same 13 planes: block b = (chunk of 8 column groups,
    // angle, column group within the chunk), so the nang blocks of one column group are dispatched
    // within 8*nang blocks of each other, all on XCD (column group % 8): the first one's plane rows are
    // L2 hits for the others (HBM fetch 3.6 GB -> ~1.2 GB per 1e5 x 90 x 5 spectrum, PMC).
    // Small launches (about one block per CU or less) keep the plain angle-major order: there the XCD
    // grouping would put five blocks of a column group on one XCD while others stay short of work.
    const int nang = a.nang;
    const unsigned b = blockIdx.x;
    int ang;
    long w;
    if (a.xcd_order) {
        const unsigned chunk = b / (8u * nang), rem = b - chunk * (8u * nang);
        ang = (int)(rem >> 3);
        w = ((long)chunk * 8 + (rem & 7u)) * blockDim.x + threadIdx.x;
    } else {
        ang = (int)(b / a.ncg);
        w = (long)(b - (unsigned)ang * a.ncg) * blockDim.x + threadIdx.x;
    }
    if (w >= a.nwno) return;
    const int n = a.nlayer;
    const long pitch = a.pitch;
    // Plane element of a layer (`LD` in the layer body).  FAST kernels address the planes as SGPR base + 32-bit lane
    // offset (launch_sh takes them only for planes smaller than 4 GB): one v_add_u32 per layer for all planes instead of a
    // 64-bit v_lshl_add_u64 per load (eleven per layer; profiles/r05_isa_k_sh4_fast_before.json).
    const unsigned voff0 = (unsigned)(w * 8), pitch8 = (unsigned)(pitch * 8);
    const int w_single_form = FAST ? 0 : a.w_single_form, w_multi_form = FAST ? 0 : a.w_multi_form;
    const int psingle_form = FAST ? 0 : a.psingle_form, single_form = FAST ? 0 : a.single_form;
    const int w_single_rayleigh = FAST ? 1 : a.w_single_rayleigh, w_multi_rayleigh = FAST ? 1 : a.w_multi_rayleigh;
    const int psingle_rayleigh = FAST ? 1 : a.psingle_rayleigh;
    const double frac_c = FAST ? 2.0 : a.frac_c;
    const auto &g = angp[ang];
    const double u0 = g.u0, u1 = g.u1, ct = a.cos_theta;
    const int fd_power = a.compound ? a.first_angle + ang + 1 : 1;   // compounded f_deltaM
    double *const xint = a.xint + (long)ang * a.nwno;
    const double F = THERMAL ? 0.0 : a.F0PI[w], rs = a.surf_reflect[w];
    double Pu0[4], Pu1[4];
    legP4(-u0, Pu0);
    legP4(u1, Pu1);
    const double mus = g.mus, iu1 = g.iu1, iu0 = g.iu0, imus = g.imus;
    const bool sym = (u0 == u1);                                     // mus = 2/u1
    Exp2Coef K;
    K.load();

    // thermal: Planck at the levels (fluxes.py:3058-3060)
    const double wn = THERMAL ? a.wno[w] : 0.0;
    double Bn = THERMAL ? planck_lambda(a.tlevel[0], wn, K) : 0.0;
    const double B_top = Bn;
    double b1_last = 0.0;

    double T = 1.0, kappa = 0.0;
    double e_top = 0.0;              // exp(-tau/u0) at the top of the current layer (carried)
    double p_og = 1.0;               // DRVT: exp(-tau_og/u0) at the top of the current layer, unclipped (e_top: exp(-tau/u0))
    if (DRVT) e_top = 1.0;           // tau[0] = 0
    double zeta[NB], delta[NB];
    Blk<NB> R;
    // previous layer
    Blk<NB> pMn, pPl, pME, pPE;
    double p_zmn_up[NB], p_zpl_up[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) { zeta[i] = delta[i] = p_zmn_up[i] = p_zpl_up[i] = 0.0; }

    // flx = 1: sweep-1 state of every layer for the back-substitution ([slot][layer][wavelength])
    constexpr int NSLOT = 4 * NB * NB + 5 * NB;
    double *const scr = FLX ? a.scratch + (long)ang * NSLOT * n * a.nwno + w : nullptr;
    auto slot = [&](int sl, int i) -> double & { return scr[((long)sl * n + i) * a.nwno]; };
    double top_zmn[NB], top_zpl[NB];
#pragma unroll
    for (int r = 0; r < NB; ++r) top_zmn[r] = top_zpl[r] = 0.0;

    if (!THERMAL && !FLX && a.start_layer > 0) {
        // the layers above start_layer were swept by k_sh4_clear (no cloud there): take its state over
        const double *sp = a.state + w;
        auto ld = [&](int sl) { return sp[(long)sl * a.nwno]; };
        int sl = 0;
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int c2 = 0; c2 < NB; ++c2) R.m[r][c2] = ld(sl++);
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int c2 = 0; c2 < NB; ++c2) pMn.m[r][c2] = ld(sl++);
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int c2 = 0; c2 < NB; ++c2) pPl.m[r][c2] = ld(sl++);
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int c2 = 0; c2 < NB; ++c2) pME.m[r][c2] = ld(sl++);
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int c2 = 0; c2 < NB; ++c2) pPE.m[r][c2] = ld(sl++);
        sl = SHC_SHARED + SHC_STATE * (a.first_angle + ang);
        T = ld(sl++);
        kappa = ld(sl++);
        e_top = ld(sl++);            // unclipped exp(-tau/u0) at the top of start_layer (k_sh4_clear)
        p_og = e_top;                // no cloud above: tau_og = tau
        if (!DRVT && NB == 2) e_top = fmax(e_top, EXP_M35);
#pragma unroll
        for (int r = 0; r < NB; ++r) zeta[r] = ld(sl++);
#pragma unroll
        for (int r = 0; r < NB; ++r) delta[r] = ld(sl++);
#pragma unroll
        for (int r = 0; r < NB; ++r) p_zmn_up[r] = ld(sl++);
#pragma unroll
        for (int r = 0; r < NB; ++r) p_zpl_up[r] = ld(sl++);
    }
    // One layer of the sweep.  Called twice per trip of the loop below: the sweep state of a layer (R, the previous layer's
    // four blocks and particular solutions: 18 doubles) then alternates between two register sets instead of being copied
    // back at the end of every layer (18 v_mov_b64 per layer in the single-body loop; the compiler does not unroll a loop
    // around wave-uniform votes by itself).
    auto layer = [&](const int i) {
        const long o = (long)i * pitch + w;
        const unsigned vo = voff0 + (unsigned)i * pitch8;
        auto LD = [&](const double *base, int below = 0) -> double {      // below = 1: the level under the layer
            if constexpr (FAST) return *(const double *)((const char *)base + (vo + (below ? pitch8 : 0u)));
            else return base[o + (below ? pitch : 0)];
        };
        const double dt = LD(a.dtau), w0 = LD(a.w0), cbo = LD(a.cosb_og);
        // ---- Legendre weights of the phase function ----
        double wsg[NS], wmu[NS];
#pragma unroll
        for (int l = 0; l < NS; ++l) { wsg[l] = 1.0; wmu[l] = 1.0; }
        double psing = 0.0;
        if (!THERMAL) {
            const double fc = LD(a.ftau_cld), fr = LD(a.ftau_ray);
            // f_deltaM as angle k of the reference sees it: its TTHG branch multiplies the array in
            // place by `fac` once per angle (:2823-2824), so the OTHG branch of angle k reads
            // f_deltaM fac^k (the aliasing is live when one form is OTHG and the other TTHG) and
            // the TTHG branch f_deltaM fac^(k+1).
            double fd_prev = LD(a.f_deltaM), fd = fd_prev, f = 0.0, gf = 0.0, gb = 0.0;
            // No cloud in this layer anywhere in the wave and Rayleigh-weighted moments (w_*_rayleigh = 1):
            // every l >= 1 moment is multiplied by ftau_cld = 0, so the weights are (1, 0, ftau_ray/2, 0)
            // whatever the phase-function form and f_deltaM -- the TTHG / OTHG blocks (a pow, two
            // reciprocals, the compounding loop) are skipped.  Same values as the general path gives on
            // such a layer (there the moments come out as +-0).
            const bool nocld = (w_single_rayleigh == 1) && (w_multi_rayleigh == 1) && __all(fc == 0.0);
            const bool tthg = !nocld && (w_single_form == 0 || w_multi_form == 0);
            if (nocld) {
#pragma unroll
                for (int l = 1; l < NS; ++l) { wsg[l] = 0.0; wmu[l] = 0.0; }
                if (NS == 4) { wsg[2] = 0.5 * fr; wmu[2] = 0.5 * fr; }
            }
            if (tthg) {
                gf = a.constant_forward * cbo;
                gb = a.constant_back * cbo;
                f = a.frac_a + a.frac_b * pow_frac(gb, frac_c);
                double cfs = 1.0, cbs = 1.0;
#pragma unroll
                for (int l = 0; l < NS; ++l) { cfs *= a.constant_forward; cbs *= a.constant_back; }
                const double fac = (f * cfs + (1 - f) * cbs);
                for (int p = 1; p < fd_power; ++p) fd_prev *= fac;
                fd = fd_prev * fac;
            }
            if (!nocld && (w_single_form == 1 || w_multi_form == 1)) {   // OTHG :2811-2817
                double cl = 1.0;
                const double ifp = frcp(1 - fd_prev);
#pragma unroll
                for (int l = 1; l < NS; ++l) {
                    cl *= cbo;
                    const double ww = ((2 * l + 1) * cl - (2 * l + 1) * fd_prev) * ifp;
                    if (w_single_form == 1) wsg[l] = ww;
                    if (w_multi_form == 1) wmu[l] = ww;
                }
            }
            if (tthg) {                                                      // TTHG :2819-2831
                double gfl = 1.0, gbl = 1.0;
                const double ifd = frcp(1 - fd);
#pragma unroll
                for (int l = 1; l < NS; ++l) {
                    gfl *= gf;
                    gbl *= gb;
                    const double ww = ((2 * l + 1) * (f * gfl + (1 - f) * gbl) - (2 * l + 1) * fd) * ifd;
                    if (w_single_form == 0) wsg[l] = ww;
                    if (w_multi_form == 0) wmu[l] = ww;
                }
            }
            if (!nocld && w_single_rayleigh == 1) {                        // :2833-2836
#pragma unroll
                for (int l = 1; l < NS; ++l) wsg[l] *= fc;
                if (NS == 4) wsg[2] += 0.5 * fr;
            }
            if (!nocld && w_multi_rayleigh == 1) {                         // :2837-2840
#pragma unroll
                for (int l = 1; l < NS; ++l) wmu[l] *= fc;
                if (NS == 4) wmu[2] += 0.5 * fr;
            }
            if (single_form == 0 && nocld && psingle_rayleigh == 1) {       // ftau_cld (..) + Rayleigh = Rayleigh
                psing = fr * (0.75 * (1 + ct * ct));
            } else if (single_form == 0) {                                 // :2843-2855
                if (psingle_form == 1) psing = hg_term(cbo, ct);
                else if (psingle_form == 0) {
                    const double gf = a.constant_forward * cbo, gb = a.constant_back * cbo;
                    const double f = a.frac_a + a.frac_b * pow_frac(gb, frac_c);
                    psing = f * hg_term(gf, ct) + (1 - f) * hg_term(gb, ct);
                }
                if (psingle_rayleigh == 1) psing = fc * psing + fr * (0.75 * (1 + ct * ct));
            } else {                                                         // legendre form :2954-2957
#pragma unroll
                for (int l = 0; l < NS; ++l) psing += wsg[l] * Pu0[l] * Pu1[l];
            }
        } else {                                                             // thermal :3072-3083
            const double ff = a.use_ff ? ((NS == 4) ? cbo * cbo * cbo * cbo : cbo * cbo) : 0.0;
            double cl = 1.0;
            const double iff = frcp(1 - ff);
#pragma unroll
            for (int l = 0; l < NS; ++l) {
                wmu[l] = (2 * l + 1) * (cl - ff) * iff;
                cl *= cbo;
            }
        }
        double al[NS], bl[NS];
#pragma unroll
        for (int l = 0; l < NS; ++l) {                                       // :2858-2860, :3083
            al[l] = (2 * l + 1) - w0 * wmu[l];
            bl[l] = THERMAL ? 0.0 : (F * (w0 * wsg[l])) * Pu0[l] * (0.25 / PI);
        }
        const double edt_layer = fexp2(dt * g.nl1, K);                   // exp(-dtau/u1)
        // ---- modes ----
        Modes<NB> M;
        constexpr bool BATCH = NB == 2 && !THERMAL;
        ShRcp rq;
        if constexpr (BATCH) modes_sh4_batched(al, dt, g.iu0, g.iu1, M, rq, K);
        else if constexpr (NB == 2) modes_sh4(al, dt, M, K);
        else modes_sh2(al, dt, M, K);
        // ---- particular solution at the layer top / bottom ----
        double eta[NS];
        double zmn_dn[NB], zpl_dn[NB], zmn_up[NB], zpl_up[NB];
        double B0 = 0.0, b1 = 0.0, ed_layer = 0.0, exp_dt_u0 = 0.0;
        if (!THERMAL) {
            double zpl[NB], zmn[NB];
            double tau_t = 0.0, tau_b = 0.0;
            if constexpr (!DRVT) { tau_t = LD(a.tau); tau_b = LD(a.tau, 1); }
            // DRVT: exp(-dtau/u0), the factor of the running products
            const double fac0 = !DRVT ? 0.0 : (sym ? edt_layer : fexp2(dt * g.nl0, K));
            exp_dt_u0 = fac0;
            double ed, eu;
            if constexpr (NB == 2) {                                         // :3397-3416, :3441-3450
                const double x = iu0, x2 = x * x;
                const double iDel = BATCH ? rq.iDel : frcp(9 * (x2 * x2 - M.beta * x2 + M.gama));
                const double a0 = al[0], a1 = al[1], a2 = al[2], a3 = al[3];
                const double b0 = bl[0], b1_ = bl[1], b2 = bl[2], b3 = bl[3];
                {
                    // eta_l = Delta_l / Delta (:3398-3411), operations written out (no contraction).  k_sh4_clear
                    // has the same expressions without the terms that carry b1 = b3 = 0 on a cloud-free layer
                    // (odd moments times ftau_cld = 0), each of them an exact zero here
#pragma clang fp contract(off)
                    const double P = fma(a2, a3, -(9 * x2)), Q = fma(a0, a1, -x2);
                    const double a3b2 = a3 * b2, b0x = b0 * x;
                    const double a0b1 = a0 * b1_, b3x3 = 3 * (b3 * x);
                    const double A = a1 * b0 - b1_ * x;
                    const double B = (a3b2 - 2 * (a3 * b0)) - b3x3;
                    const double C = a0b1 - b0x;
                    const double D = a3b2 - b3x3;
                    const double E_ = a2 * b3 - 3 * (b2 * x);
                    const double F_ = (3 * a0b1 - 2 * (a0 * b3)) - 3 * b0x;
                    eta[0] = fma(A, P, 2 * (B * x2)) * iDel;
                    eta[1] = fma(C, P, -((2 * a0) * (D * x))) * iDel;
                    eta[2] = fma(D, Q, -((2 * a3) * (C * x))) * iDel;
                    eta[3] = fma(E_, Q, 2 * (F_ * x2)) * iDel;
                    const double h0 = 0.5 * eta[0], e58 = 0.625 * eta[2], m0 = -0.125 * eta[0];
                    zpl[0] = ((h0 + eta[1]) + e58) * (2 * PI);
                    zmn[0] = ((h0 - eta[1]) + e58) * (2 * PI);
                    zpl[1] = ((m0 + e58) + eta[3]) * (2 * PI);
                    zmn[1] = ((m0 + e58) - eta[3]) * (2 * PI);
                }
                if constexpr (DRVT) {
                    ed = fmax(e_top, EXP_M35);
                    e_top = e_top * fac0;                                    // unclipped, carried
                    eu = fmax(e_top, EXP_M35);
                } else {
                    ed = (i == 0) ? fexp2_clip(tau_t * g.nl0, K) : e_top;    // = last layer's eu (same element)
                    eu = fexp2_clip(tau_b * g.nl0, K);
                }
            } else {                                                         // :3240-3265
                const double x = iu0;
                const double iDel = frcp(x * x - al[0] * al[1]);
                eta[0] = (bl[1] * x - al[1] * bl[0]) * iDel;
                eta[1] = (bl[0] * x - al[0] * bl[1]) * iDel;
                zmn[0] = (0.5 * eta[0] - eta[1]) * 2 * PI;
                zpl[0] = (0.5 * eta[0] + eta[1]) * 2 * PI;
                if constexpr (DRVT) {
                    ed = e_top;
                    e_top = e_top * fac0;
                    eu = e_top;
                } else {
                    ed = (i == 0) ? fexp2(tau_t * g.nl0, K) : e_top;
                    eu = fexp2(tau_b * g.nl0, K);
                }
            }
            if constexpr (!DRVT) e_top = eu;
            ed_layer = ed;
#pragma unroll
            for (int r = 0; r < NB; ++r) {
                zmn_dn[r] = zmn[r] * ed; zpl_dn[r] = zpl[r] * ed;
                zmn_up[r] = zmn[r] * eu; zpl_up[r] = zpl[r] * eu;
            }
        } else {                                                             // :3451-3459 / :3266-3270
            B0 = Bn;
            Bn = planck_lambda(a.tlevel[i + 1], wn, K);
            b1 = (Bn - B0) * frcp(dt);
            b1_last = b1;
            const double oma = (1 - w0) * frcp(al[0]), b1a = b1 * frcp(al[1]);
            zmn_dn[0] = oma * (B0 / 2 - b1a) * 2 * PI;
            zpl_dn[0] = oma * (B0 / 2 + b1a) * 2 * PI;
            zmn_up[0] = oma * (B0 / 2 - b1a + b1 * dt / 2) * 2 * PI;
            zpl_up[0] = oma * (B0 / 2 + b1a + b1 * dt / 2) * 2 * PI;
            if constexpr (NB == 2) {
                zmn_dn[1] = zpl_dn[1] = -0.125 * oma * (B0) * 2 * PI;
                zmn_up[1] = zpl_up[1] = -0.125 * oma * (B0 + b1 * dt) * 2 * PI;
            }
#pragma unroll
            for (int l = 0; l < NS; ++l) eta[l] = 0.0;
        }
        const Blk<NB> ME = scale_cols(M.Mn, M.E), PE = scale_cols(M.Pl, M.E);

        // ---- functional weights (source-function integrals) ----
        double gd[NB], gv[NB], c, Tn;
        {
            double cm[NS];
            if constexpr (NB == 2) {
                // sum_j w_multi_j P_j(u1) A[j][m] (:3601-3605): A's columns come in +- pairs (rows 1 and 3
                // change sign between the decaying and the growing mode), so the four sums are two even and
                // two odd parts; the odd parts vanish exactly on a cloud-free layer (w_multi_1 = w_multi_3 = 0)
#pragma clang fp contract(off)
                const double wP0 = wmu[0] * Pu1[0], wP2 = wmu[2] * Pu1[2];
                const double e01 = fma(wP2, M.cA[2][0], wP0), e23 = fma(wP2, M.cA[2][2], wP0);
                const double wP1 = wmu[1] * Pu1[1], wP3 = wmu[3] * Pu1[3];
                const double o01 = fma(wP3, M.cA[3][0], wP1 * M.cA[1][0]);
                const double o23 = fma(wP3, M.cA[3][2], wP1 * M.cA[1][2]);
                cm[0] = e01 + o01;
                cm[1] = e01 - o01;
                cm[2] = e23 + o23;
                cm[3] = e23 - o23;
            } else {                                                         // :2916-2917, :3124-3125
                cm[0] = (wmu[0] - wmu[1] * Pu1[1] * M.q);
                cm[1] = (wmu[0] + wmu[1] * Pu1[1] * M.q);
            }
            const double scale = THERMAL ? 2 * PI : 1.0;                     // :3167 vs :2961
            const double tw = T * iu1 * w0 * scale;
            const double edt = edt_layer;                                    // exp(-dtau/u1)
            // exp(-(1/u1 +- lam) dtau) = exp(-dtau/u1) E^{+-1} when no 35-clip binds anywhere in the
            // wave ((1/u1 + lam_max) dtau <= 35 covers all four arguments); otherwise the reference's
            // clipped exponentials are formed directly (:2929-2937).
            // The choice is made per LANE (a wavelength's bits must not depend on which other wavelengths share
            // its wave: blocks of a sharded spectrum cut the waves differently); only the work is wave-uniform --
            // the direct exponentials are formed when some lane of the wave needs them.
            const bool noclip_lane = (iu1 + M.lam[0]) * dt <= 35.0;
            const bool noclip = __all(noclip_lane);
#pragma unroll
            for (int r = 0; r < NB; ++r) {
                const double alpha = iu1 + M.lam[r], beta = iu1 - M.lam[r];
                const double rab = BATCH ? rq.rab[r] : frcp(alpha * beta);    // one reciprocal for both
                double ea = edt * M.E[r], eb = edt * (BATCH ? rq.iE[r] : frcp(M.E[r]));
                if (!noclip) {
                    const double ead = fexpk(-clip35(alpha * dt), K), ebd = fexpk(-clip35(beta * dt), K);
                    ea = noclip_lane ? ea : ead;
                    eb = noclip_lane ? eb : ebd;
                }
                const double ha = (1 - ea) * (rab * beta);
                const double hb = (1 - eb) * (rab * alpha);
                gd[r] = tw * cm[2 * r] * ha;
                gv[r] = tw * cm[2 * r + 1] * hb * M.E[r];
            }
            if (!THERMAL) {
                // (1 - exp(-clip35(mus dtau)))/mus (:2901-2905); mus = 2/u1 in the symmetric geometry
                const bool sq_lane = sym && (mus * dt <= 35.0);                 // per lane, as above
                double e_mus = edt * edt;
                if (!__all(sq_lane)) {
                    const double d = fexp2_clip(dt * g.nlm, K);
                    e_mus = sq_lane ? e_mus : d;
                }
                const double exptrm_mus = (1 - e_mus) * imus;
                // exp(-clip35(tau/u0)): the layer-top exponential above (SH4 clips it too; SH2 does not)
                const double expon1 = exptrm_mus * ((NB == 2) ? ed_layer : fmax(ed_layer, EXP_M35));
                double Nsum;
                {                                                            // :2919-2920, 2945-2948
#pragma clang fp contract(off)
                    double sN = (wmu[0] * Pu1[0]) * eta[0];
                    if (NS == 4) sN = fma(wmu[2] * Pu1[2], eta[2], sN);
                    sN = fma(wmu[1] * Pu1[1], eta[1], sN);
                    if (NS == 4) sN = fma(wmu[3] * Pu1[3], eta[3], sN);
                    Nsum = sN * expon1;
                }
                const double dto = LD(a.dtau_og);
                double e_muso = e_mus;
                double faco = 0.0;                                           // DRVT: exp(-dtau_og/u0)
                if constexpr (DRVT) faco = exp_dt_u0;
                if (!__all(dto == dt)) {
                    const double d = fexp2_clip(dto * g.nlm, K);
                    e_muso = (dto == dt) ? e_mus : d;
                    if constexpr (DRVT) {
                        const double d0 = fexp2(dto * g.nl0, K);
                        faco = (dto == dt) ? faco : d0;
                    }
                }
                // exp(-tau_og/u0) at the layer top, unclipped (:2962)
                double e_tauo;
                if constexpr (DRVT) {
                    e_tauo = p_og;
                    p_og = p_og * faco;
                } else {
                    e_tauo = fexp2(LD(a.tau_og) * g.nl0, K);
                }
                const double single = div_const(LD(a.w0_og) * F, FOURPI, R4PI) * psing *
                                      (1 - e_muso) * e_tauo * imus;          // :2959-2965
                c = T * iu1 * (w0 * Nsum + single);
            } else {
                const double edc = (NB == 2) ? fmax(edt, EXP_M35) : edt;   // exp(-clip35(dtau/u1)) :3154 vs :3127
                const double core = (1 - w0) * u1 * frcp(al[0]);
                const double N0 = wmu[0] * (core * (B0 * (1 - edc) + b1 * (u1 - (dt + u1) * edc)));     // :3128, :3155
                const double N1 = wmu[1] * Pu1[1] * (core * (b1 * (1 - edc) * frcp(al[1])));            // :3129, :3156
                c = T * iu1 * (w0 * (N0 + N1) * 2 * PI +
                               2 * PI * (1 - w0) * u1 * (B0 * (1 - edt) + b1 * (u1 - (dt + u1) * edt)));    // :3163-3165
            }
            Tn = T * edt;
        }
        if (i == n - 1) {
            if (!THERMAL) {       // xint[n] = flux_bot/pi = (Pl E d + Mn v + zpl_up)[0]/pi  (:2891, :2967)
#pragma unroll
                for (int r = 0; r < NB; ++r) {
                    gd[r] += Tn * (1.0 / PI) * PE.m[0][r];
                    gv[r] += Tn * (1.0 / PI) * M.Mn.m[0][r];
                }
                c += Tn * (1.0 / PI) * zpl_up[0];
            } else {              // :3173-3176
                c += Tn * (a.hard_surface ? Bn * 2 * PI : (Bn + b1 * u1) * 2 * PI);
            }
        }
        // ---- elimination ----
        if (i == 0) {
            double bt[NB];
            double b_top;
            if (!THERMAL) b_top = a.b_top;
            else {
                const double tau_top = dt * a.plevel[0] / (a.plevel[1] - a.plevel[0]);   // :3062-3063
                b_top = PI * (1.0 - fexpk(-tau_top / 0.5, K)) * B_top;
            }
            bt[0] = b_top - zmn_dn[0];                                       // :3479-3480 / :3283
            if constexpr (NB == 2) bt[1] = -b_top / 4 - zmn_dn[1];
            const Blk<NB> Mni = inv(M.Mn);
            R = mm(Mni, PE);
            mv(Mni, bt, delta);
            double tmp[NB];
            mtv(R, gd, tmp);
            kappa = c + dot(gd, delta);
#pragma unroll
            for (int r = 0; r < NB; ++r) zeta[r] = gv[r] - tmp[r];
        } else {
            Blk<NB> A1 = mm(pME, R), A2 = mm(pPE, R);
#pragma unroll
            for (int r = 0; r < NB; ++r)
#pragma unroll
                for (int s = 0; s < NB; ++s) {
                    A1.m[r][s] = pPl.m[r][s] - A1.m[r][s];
                    A2.m[r][s] = pMn.m[r][s] - A2.m[r][s];
                }
            const Blk<NB> A2i = inv(A2);
            const Blk<NB> G = mm(A1, A2i);
            double cP[NB], cM[NB], t1[NB], t2[NB];
            mv(pPE, delta, t1);
            mv(pME, delta, t2);
#pragma unroll
            for (int r = 0; r < NB; ++r) {
                cP[r] = zpl_dn[r] - p_zpl_up[r] - t1[r];
                cM[r] = t2[r] + p_zmn_up[r] - zmn_dn[r];
            }
            Blk<NB> K = mm(G, M.Pl), GM = mm(G, ME);
#pragma unroll
            for (int r = 0; r < NB; ++r)
#pragma unroll
                for (int s = 0; s < NB; ++s) {
                    K.m[r][s] = M.Mn.m[r][s] - K.m[r][s];
                    GM.m[r][s] = PE.m[r][s] - GM.m[r][s];        // -(G Mn E - Pl E)
                }
            K = inv(K);
            const Blk<NB> Rn = mm(K, GM);
            double deltan[NB], rhs[NB];
            mv(G, cP, rhs);
#pragma unroll
            for (int r = 0; r < NB; ++r) rhs[r] += cM[r];
            mv(K, rhs, deltan);
            double tv[NB];
            mv(M.Pl, deltan, tv);
#pragma unroll
            for (int r = 0; r < NB; ++r) tv[r] += cP[r];
            double z1[NB], z2[NB];                               // zeta = z1 + gv - z2
            if constexpr (!FLX) {
                // v_{i-1} = Sm v_i + t with Sm = A2i (ME - Pl Rn), t = A2i tv enters the TOA functional only through
                // zeta.t and Sm^T zeta: with z = A2i^T zeta these are z.tv and ME^T z - Rn^T (Pl^T z), and the two
                // NB x NB products that form Sm (and the matrix-vector product for t) are not needed -- 34 instead of
                // 49 fp64 instructions per layer at NB = 2 (the flx = 1 kernels keep Sm and t: their second sweep reads them)
                double z[NB], y[NB];
                mtv(A2i, zeta, z);
                kappa = kappa + dot(z, tv) + dot(gd, deltan) + c;
                mtv(M.Pl, z, y);
#pragma unroll
                for (int r = 0; r < NB; ++r) y[r] += gd[r];
                mtv(ME, z, z1);
                mtv(Rn, y, z2);
            } else {
                Blk<NB> Sm = mm(M.Pl, Rn);
#pragma unroll
                for (int r = 0; r < NB; ++r)
#pragma unroll
                    for (int s = 0; s < NB; ++s) Sm.m[r][s] = ME.m[r][s] - Sm.m[r][s];
                Sm = mm(A2i, Sm);
                double t[NB];
                mv(A2i, tv, t);
                // v_{i-1} = Sm v_i + t
                int sl = 3 * NB * NB + 4 * NB;
#pragma unroll
                for (int r = 0; r < NB; ++r)
#pragma unroll
                    for (int c2 = 0; c2 < NB; ++c2) slot(sl++, i) = Sm.m[r][c2];
#pragma unroll
                for (int r = 0; r < NB; ++r) slot(sl++, i) = t[r];
                kappa = kappa + dot(zeta, t) + dot(gd, deltan) + c;
                mtv(Sm, zeta, z1);
                mtv(Rn, gd, z2);
            }
#pragma unroll
            for (int r = 0; r < NB; ++r) {
                zeta[r] = z1[r] + gv[r] - z2[r];
                delta[r] = deltan[r];
            }
            R = Rn;
        }
        if constexpr (FLX) {
            int sl = 0;
#pragma unroll
            for (int r = 0; r < NB; ++r) slot(sl++, i) = delta[r];
#pragma unroll
            for (int r = 0; r < NB; ++r)
#pragma unroll
                for (int c = 0; c < NB; ++c) slot(sl++, i) = R.m[r][c];
#pragma unroll
            for (int r = 0; r < NB; ++r)
#pragma unroll
                for (int c = 0; c < NB; ++c) slot(sl++, i) = M.Mn.m[r][c];
#pragma unroll
            for (int r = 0; r < NB; ++r)
#pragma unroll
                for (int c = 0; c < NB; ++c) slot(sl++, i) = M.Pl.m[r][c];
#pragma unroll
            for (int r = 0; r < NB; ++r) slot(sl++, i) = M.E[r];
#pragma unroll
            for (int r = 0; r < NB; ++r) slot(sl++, i) = zmn_up[r];
#pragma unroll
            for (int r = 0; r < NB; ++r) slot(sl++, i) = zpl_up[r];
            if (i == 0) {
#pragma unroll
                for (int r = 0; r < NB; ++r) { top_zmn[r] = zmn_dn[r]; top_zpl[r] = zpl_dn[r]; }
            }
        }
        pMn = M.Mn; pPl = M.Pl; pME = ME; pPE = PE;
#pragma unroll
        for (int r = 0; r < NB; ++r) { p_zmn_up[r] = zmn_up[r]; p_zpl_up[r] = zpl_up[r]; }
        T = Tn;
    };
    if constexpr (FAST && !THERMAL && !FLX) {      // (the generic and flx = 1 bodies are larger: two copies would spill)
        int i = a.start_layer;
        for (; i + 1 < n; i += 2) {
            layer(i);
            layer(i + 1);
        }
        if (i < n) layer(i);
    } else {
        for (int i = (!THERMAL && !FLX) ? a.start_layer : 0; i < n; ++i) layer(i);
    }
    // ---- surface rows (:3484-3494 / :3287-3289) ----
    double bs[NB];
    if (!THERMAL) {
        double e_bot;                                                        // exp(-tau[n]/u0), unclipped
        if constexpr (DRVT) e_bot = e_top;
        else e_bot = fexpk(-a.tau[(long)n * pitch + w] / u0, K);
        const double bsf = (0. + rs * u0 * F * e_bot);                                          // :2863-2864
        bs[0] = bsf;
        if constexpr (NB == 2) bs[1] = -bsf / 4;
    } else {
        bs[0] = a.hard_surface ? PI * Bn : PI * (Bn + b1_last * 0.5);                       // :3065-3068
        if constexpr (NB == 2) bs[1] = (-PI * Bn / 4);                                       // :3070
    }
    Blk<NB> L, W;
#pragma unroll
    for (int r = 0; r < NB; ++r)
#pragma unroll
        for (int s = 0; s < NB; ++s) {
            W.m[r][s] = pPE.m[r][s] - rs * pME.m[r][s];
            L.m[r][s] = pMn.m[r][s] - rs * pPl.m[r][s];
        }
    const Blk<NB> WR = mm(W, R);
#pragma unroll
    for (int r = 0; r < NB; ++r)
#pragma unroll
        for (int s = 0; s < NB; ++s) L.m[r][s] -= WR.m[r][s];
    double wd[NB], rhs[NB], v[NB];
    mv(W, delta, wd);
#pragma unroll
    for (int r = 0; r < NB; ++r) rhs[r] = bs[r] - p_zpl_up[r] + rs * p_zmn_up[r] - wd[r];
    mv(inv(L), rhs, v);
    xint[w] = kappa + dot(zeta, v);
    if constexpr (FLX) {
        // ---- sweep 2: back-substitute v_i, d_i = delta_i - R_i v_i and write the moment fluxes at the
        // bottom of every layer (and the top of layer 0) in the row order of the reference's F.X + G:
        // (Fmn[0..NB), Fpl[0..NB)) per level (fluxes.py:3311-3331, 3552-3599)
        double *fl = a.flux + (long)ang * NS * (n + 1) * a.nwno + w;
        double vv[NB];
#pragma unroll
        for (int r = 0; r < NB; ++r) vv[r] = v[r];
        for (int i = n - 1; i >= 0; --i) {
            int sl = 0;
            double dl[NB], E[NB], zmu[NB], zpu[NB], d[NB], Rv[NB];
            Blk<NB> Ri, Mn, Pl;
#pragma unroll
            for (int r = 0; r < NB; ++r) dl[r] = slot(sl++, i);
#pragma unroll
            for (int r = 0; r < NB; ++r)
#pragma unroll
                for (int c2 = 0; c2 < NB; ++c2) Ri.m[r][c2] = slot(sl++, i);
#pragma unroll
            for (int r = 0; r < NB; ++r)
#pragma unroll
                for (int c2 = 0; c2 < NB; ++c2) Mn.m[r][c2] = slot(sl++, i);
#pragma unroll
            for (int r = 0; r < NB; ++r)
#pragma unroll
                for (int c2 = 0; c2 < NB; ++c2) Pl.m[r][c2] = slot(sl++, i);
#pragma unroll
            for (int r = 0; r < NB; ++r) E[r] = slot(sl++, i);
#pragma unroll
            for (int r = 0; r < NB; ++r) zmu[r] = slot(sl++, i);
#pragma unroll
            for (int r = 0; r < NB; ++r) zpu[r] = slot(sl++, i);
            mv(Ri, vv, Rv);
#pragma unroll
            for (int r = 0; r < NB; ++r) d[r] = dl[r] - Rv[r];
            const Blk<NB> MEi = scale_cols(Mn, E), PEi = scale_cols(Pl, E);
            double x1[NB], x2[NB];
            mv(MEi, d, x1);
            mv(Pl, vv, x2);
#pragma unroll
            for (int r = 0; r < NB; ++r) fl[(long)(NS * (i + 1) + r) * a.nwno] = x1[r] + x2[r] + zmu[r];
            mv(PEi, d, x1);
            mv(Mn, vv, x2);
#pragma unroll
            for (int r = 0; r < NB; ++r) fl[(long)(NS * (i + 1) + NB + r) * a.nwno] = x1[r] + x2[r] + zpu[r];
            if (i == 0) {
                mv(Mn, d, x1);
                mv(PEi, vv, x2);
#pragma unroll
                for (int r = 0; r < NB; ++r) fl[(long)r * a.nwno] = x1[r] + x2[r] + top_zmn[r];
                mv(Pl, d, x1);
                mv(MEi, vv, x2);
#pragma unroll
                for (int r = 0; r < NB; ++r) fl[(long)(NB + r) * a.nwno] = x1[r] + x2[r] + top_zpl[r];
            } else {
                Blk<NB> Smi;
                double ti[NB], nv[NB];
#pragma unroll
                for (int r = 0; r < NB; ++r)
#pragma unroll
                    for (int c2 = 0; c2 < NB; ++c2) Smi.m[r][c2] = slot(sl++, i);
#pragma unroll
                for (int r = 0; r < NB; ++r) ti[r] = slot(sl++, i);
                mv(Smi, vv, nv);
#pragma unroll
                for (int r = 0; r < NB; ++r) vv[r] = nv[r] + ti[r];
            }
        }
    }
}

template <int NB, bool THERMAL, bool FLX, bool FAST = false, bool DRVT = false>
__global__ __launch_bounds__(256, PZ_SH_MINWAVES) void k_sh(const SHArgs a)
{
    sh_body<NB, THERMAL, FLX, FAST, DRVT>(a, a.ang);
}

// Reflected light without layer fluxes: ONE kernel for a single spectrum and for `nspec` spectra of one shape and option
// set in one grid (picaso_get_reflected_SH_batch_dev: blockIdx.y = spectrum, whose planes, output and angle table come
// from the device table a.batch, read through the constant address space like kernel arguments).  A single launch is the
// same machine code with a.batch = NULL -- its angle table is the kernel-argument segment itself -- so "spectrum s of a
// batch is bit-identical to its own launch" does not rest on the compiler contracting two instantiations of the body
// alike (round 5: it did not, once the layer body was inlined twice).
template <int NB, bool FAST, bool DRVT = false>
__global__ __launch_bounds__(256, PZ_SH_MINWAVES) void k_sh_refl(const SHArgs a)
{
    typedef const __attribute__((address_space(4))) SHBatchItem *ItemPtr;
    typedef const __attribute__((address_space(4))) SHArgs::Angle *AngPtr;
    typedef const __attribute__((address_space(4))) char *ArgBytes;
    SHArgs b = a;
    AngPtr angp = (AngPtr)((ArgBytes)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(SHArgs, ang));
    if (a.batch) {
        const ItemPtr it = (ItemPtr)(unsigned long)a.batch + blockIdx.y;
        b.dtau = it->dtau; b.tau = it->tau; b.w0 = it->w0; b.ftau_cld = it->ftau_cld; b.ftau_ray = it->ftau_ray;
        b.f_deltaM = it->f_deltaM; b.dtau_og = it->dtau_og; b.tau_og = it->tau_og; b.w0_og = it->w0_og;
        b.cosb_og = it->cosb_og; b.surf_reflect = it->surf_reflect; b.F0PI = it->F0PI; b.xint = it->xint;
        b.cos_theta = it->cos_theta;
        angp = it->ang;
    }
    sh_body<NB, false, false, FAST, DRVT>(b, angp);
}

// PICASO_AMD_SH_CHECK_TOP=1: count the elements of the first `top` layers that contradict the caller's statement
// (picaso_get_reflected_SH_top_dev) -- a synchronising debug aid, the tests run with it.
__global__ void k_sh_check_top(const SHArgs a, int top, unsigned long long *bad)
{
#pragma clang fp contract(off)
    const long w = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= a.nwno) return;
    unsigned n = 0;
    for (int i = 0; i < top; ++i) {
        const long o = (long)i * a.pitch + w;
        const double dt = a.dtau[o];
        n += (a.ftau_cld[o] != 0.0) + (a.cosb_og[o] != 0.0) + (a.f_deltaM[o] != 0.0) + (a.ftau_ray[o] != 1.0) +
             (a.dtau_og[o] != dt) + (a.w0_og[o] != a.w0[o]);
        if (a.tau && a.tau_og)                  // (left out: re-derived as running sums in the kernels)
            n += (a.tau[o + a.pitch] != a.tau[o] + dt) + (a.tau_og[o] != a.tau[o]) + (i == 0 && a.tau[o] != 0.0);
    }
    if (n) atomicAdd(bad, (unsigned long long)n);
}

int sh_check_top(picaso_ctx *ctx, const SHArgs &a, int top)
{
    PZ_TRY(ck_scratch_reserve(ctx, 256));
    unsigned long long *d = (unsigned long long *)ctx->ck_scratch, h = 0;
    PZ_HIP(ctx, hipMemsetAsync(d, 0, sizeof(h), ctx->stream));
    hipLaunchKernelGGL(k_sh_check_top, dim3((unsigned)((a.nwno + 255) / 256)), dim3(256), 0, ctx->stream, a, top, d);
    PZ_HIP(ctx, hipGetLastError());
    PZ_HIP(ctx, hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    PZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h)
        return fail(ctx, "get_reflected_SH: cloud_free_above = %d, but %llu plane elements of those layers are not what a "
                         "cloud-free layer holds (ftau_cld = cosb_og = f_deltaM = 0, ftau_ray = 1, dtau_og = dtau, w0_og = w0, "
                         "tau = tau_og = the running sum of dtau)", top, h);
    return 0;
}

int launch_sh(picaso_ctx *ctx, SHArgs &a, int nang, bool thermal)
{
    const int block = 256;
    const unsigned ncg = (unsigned)((a.nwno + block - 1) / block);          // column groups
    a.ncg = ncg;
    const unsigned nspec = a.batch ? (unsigned)a.nspec_ : 1u;
    a.xcd_order = (ncg * (unsigned)nang * nspec >= 4u * (unsigned)ctx->ncu) && !getenv("PICASO_AMD_SH_ANGLE_MAJOR");
    const dim3 grid(a.xcd_order ? ((ncg + 7u) / 8u) * 8u * (unsigned)nang : ncg * (unsigned)nang, a.batch ? nspec : 1u);
    const bool flx = a.flux != nullptr;
    const bool fast = !thermal && !flx && !getenv("PICASO_AMD_SH_GENERIC") && a.w_single_form == 0 &&
                      a.w_multi_form == 0 && a.psingle_form == 0 && a.single_form == 0 && a.w_single_rayleigh == 1 &&
                      a.w_multi_rayleigh == 1 && a.psingle_rayleigh == 1 && a.frac_c == 2.0 &&   // config.json defaults
                      (double)a.pitch * (a.nlayer + 1) * 8.0 < 4294967296.0;                   // 32-bit plane offsets
    if (a.batch && (thermal || flx)) return fail(ctx, "SH batch: reflected light without layer fluxes only");
    const bool drvt = !thermal && (!a.tau || !a.tau_og);   // level planes left out: picaso_reflected_SH_can_derive_levels
    if (drvt && (!fast || a.tau || a.tau_og))
        return fail(ctx, "get_reflected_SH: tau and tau_og may be left out (both) only with the reference's default "
                         "options, flx = 0 and planes below 4 GB (picaso_reflected_SH_can_derive_levels)");
#define SH_GO(KERNEL) hipLaunchKernelGGL(KERNEL, grid, dim3(block), 0, ctx->stream, a)
    if (!thermal && !flx) {                         // single spectrum (a.batch = NULL) or a batch: the same kernel
        if (a.stream == 4) {
            if (drvt) SH_GO((k_sh_refl<2, true, true>));
            else if (fast) SH_GO((k_sh_refl<2, true>));
            else SH_GO((k_sh_refl<2, false>));
        } else {
            if (drvt) SH_GO((k_sh_refl<1, true, true>));
            else if (fast) SH_GO((k_sh_refl<1, true>));
            else SH_GO((k_sh_refl<1, false>));
        }
    } else if (a.stream == 4) {
        if (thermal) SH_GO((k_sh<2, true, false>));
        else SH_GO((k_sh<2, false, true>));
    } else {
        if (thermal) SH_GO((k_sh<1, true, false>));
        else SH_GO((k_sh<1, false, true>));
    }
#undef SH_GO
    PZ_HIP(ctx, hipGetLastError());
    return 0;
}

// All angles of a call go into one launch (grid.y = angle, SH_MAX_ANG per launch): a 1e5-column
// spectrum is only 1.5 waves per SIMD per angle, five angles together fill the chip evenly.
int launch_sh_angles(picaso_ctx *ctx, SHArgs &a, int nang, const double *ubar0, const double *ubar1,
                     double *xint_at_top, double *flux, bool thermal)
{
    const int nb = a.stream / 2, nslot = 4 * nb * nb + 5 * nb;
    const size_t per_angle = (size_t)nslot * a.nlayer * a.nwno;
    // flx = 1 keeps the sweep state of every layer: limit the angles per launch to ~8 GB of scratch
    int max_ang = SH_MAX_ANG;
    if (flux) {
        const size_t cap = (size_t)8 << 30;
        max_ang = (int)(cap / (per_angle * sizeof(double)));
        if (max_ang < 1) max_ang = 1;
        if (max_ang > SH_MAX_ANG) max_ang = SH_MAX_ANG;
        PZ_TRY(ck_scratch_reserve(ctx, sizeof(double) * per_angle * (size_t)(nang < max_ang ? nang : max_ang)));
    }
    for (int done = 0; done < nang; done += max_ang) {
        const int m = (nang - done < max_ang) ? nang - done : max_ang;
        a.flux = flux ? flux + (size_t)done * a.stream * (a.nlayer + 1) * a.nwno : nullptr;
        a.scratch = flux ? ctx->ck_scratch : nullptr;
        for (int k = 0; k < m; ++k) a.ang[k] = make_sh_angle(thermal ? 0.0 : ubar0[done + k], ubar1[done + k], thermal);
        a.first_angle = done;
        a.nang = m;
        a.xint = xint_at_top + (size_t)done * a.nwno;
        PZ_TRY(launch_sh(ctx, a, m, thermal));
    }
    return 0;
}

}  // namespace pz
