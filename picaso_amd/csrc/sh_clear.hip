// Spherical-harmonics reflected light, SH4, cloud-free layers, the reference's default options: the angle-independent
// half of a layer shared between the disk angles of a lane -- gfx950.
//
// Without cloud every l >= 1 moment of the phase function is multiplied by ftau_cld = 0 (w_*_rayleigh = 1), so the
// Legendre weights are (1, 0, ftau_ray / 2, 0) with ftau_ray = 1, cosb = 0 makes the delta-scaling the identity
// (f_deltaM = 0: dtau_og = dtau, w0_og = w0, tau_og = tau -- and the reference's in-place compounding of f_deltaM,
// which gives every angle of a cloudy column its own matrices, multiplies a zero), and the level depths are the
// running sums of dtau.  The stream coefficients a_l = (1 - w0, 3, 5 - w0 / 2, 7), the two modes, the blocks Mn / Pl
// and the matrix half of the sweep (R, S, the two inverses) are then the same for every angle; what is left per
// angle is the particular solution along 1/u0, the right-hand sides of the elimination, the source-function weights
// along u1 and the update of its TOA functional: ~190 fp64 instructions per layer shared, ~275 per angle (from the
// timings below) -- k_sh<2,false,false,true> spends ~590 per angle.  The launch reads dtau and w0 only (and F0PI,
// surf_reflect): picaso_get_reflected_SH_dev with the nine other plane arguments NULL.
//
// Same formulas in the same order as sh_body (sh_sweep.hip; fluxes.py:2675-2976, 3336-3607) with the exact zeros
// dropped, written out like k_sh_thermal (explicit fma): a column's result depends neither on the launch shape nor on
// how many angles share its lane.  It is NOT bit-identical to k_sh on the full plane set of the same column -- k_sh
// takes six reciprocals of a layer, two of them along the angle, from one Newton core (modes_sh4_batched), so even
// its angle-independent blocks carry the angle in their last bits; the two agree to <= 1e-9 like each does with the
// oracle (observed 5e-10 over 1e5 columns; tests/test_sh_clear_gpu.py).
#include "sh.hpp"
#include "sh_blocks.hpp"

#pragma clang fp contract(off)   // every fma is written out: an angle's bits do not depend on how many share its lane

namespace pz {

// Angles per lane: two (SHC_MAX_PER_LANE).  Measured at 1e5 x 90 x 5 (tools/sh_clear_time.py; the full-plane kernel on the
// same cloud-free scene: 1.009 ms): one angle per lane 0.804 ms (what dropping the cloud arithmetic and nine planes gives by
// itself), two 0.667 (198 -> 256 VGPRs, 6 spilled, still two waves per SIMD), three 0.80 (100 VGPRs spilled to scratch),
// five 1.52 -- or 0.80 in 352 registers with one wave per SIMD (1 563 waves on 1 024 SIMDs: two rounds).  The per-angle
// sweep state in LDS instead (11 doubles per angle, a plain loop over the angles in 232 VGPRs): 0.884 / 0.735 / 0.737 for
// one / two / three angles per lane -- the LDS round trips cost more than the third angle's share of the common half saves.
// From the two register timings: ~190 instructions per layer shared, ~275 per angle.
// The angle's three reciprocals from one Newton core (prefix products, as modes_sh4_batched): 0.629 ms at 1e5 columns but
// 0.148 instead of 0.135 at 12 500, where one wave per SIMD waits out the longer dependency chain; not kept.
// The beam exponential exp(-tau[i+1]/u0) as the product of the two at hand (symmetric geometry, no clip): 0.641 ms against
// 0.629 with its own polynomial -- the wave-uniform test costs more than the exponential (as in k_sh: DESIGN.md
// section 8, "Measured out").
template <int NA>
__global__ __launch_bounds__(256, 2) void k_sh4_clear(const SHCArgs a)
{
    constexpr int NB = 2;
    const long w = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= a.nwno) return;
    const int n = a.nlayer;
    const long pitch = a.pitch;
    const int k0 = blockIdx.y * NA;
    const int na = min(NA, a.na - k0);
    const SHCArgs::Angle *const ang = a.ang + k0;
    Exp2Coef K;
    K.load();
    const double F = a.F0PI[w], rs = a.surf_reflect[w];
    // per angle: transmission to the top T, TOA functional J = kappa + zeta . v, sweep right-hand side delta, the
    // beam exponential at the layer top and the previous layer's particular solution at its bottom
    double T[NA], kappa[NA], zeta[NA][NB], delta[NA][NB], e_top[NA], p_zmn_up[NA][NB], p_zpl_up[NA][NB];
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        T[k] = 1.0;
        kappa[k] = 0.0;
        e_top[k] = 1.0;                                                      // tau[0] = 0 (optics.py cumsum)
#pragma unroll
        for (int r = 0; r < NB; ++r) zeta[k][r] = delta[k][r] = p_zmn_up[k][r] = p_zpl_up[k][r] = 0.0;
    }
    Blk<NB> R, pMn, pPl, pME, pPE;
    double tau_t = 0.0;

    const int nsweep = a.state ? a.nstop : n;
    for (int i = 0; i < nsweep; ++i) {
        const long o = (long)i * pitch + w;
        const double dt = a.dtau[o], w0 = a.w0[o];
        const double tau_b = tau_t + dt;
        // ---- stream coefficients and modes (:2858-2860, 3388-3434) ----
        const double al[4] = {1.0 - w0, 3.0, fma(-w0, 0.5, 5.0), 7.0};
        ModesT4 M;
        modes_sh4x(al, dt, M, K);
        const Blk<NB> ME = scale_cols(M.Mn, M.E), PE = scale_cols(M.Pl, M.E);
        // beam source moments b_l = F w0 w_single_l P_l(-u0) / 4 pi: b_0 for all angles, b_2 = fw2 P_2(-u0) / 4 pi
        const double b0 = (F * w0) * (0.25 / PI), fw2 = F * (w0 * 0.5);
        const double sgl = div_const(w0 * F, FOURPI, R4PI) * a.psing;         // :2959-2965
        const double a0 = al[0], a2 = al[2];
        const double A_ = 3.0 * b0, a3b0 = 7.0 * b0;

        // ---- elimination, matrix half (angle independent) ----
        Blk<NB> Rn, Sm, A2i, G, Ki, Mni;
        if (i == 0) {
            Mni = invx(M.Mn);
            Rn = mmx(Mni, PE);
            Sm = Rn; A2i = Rn; G = Rn; Ki = Rn;                              // not used for i == 0
        } else {
            const Blk<NB> A1 = subx(pPl, mmx(pME, R)), A2 = subx(pMn, mmx(pPE, R));
            A2i = invx(A2);
            G = mmx(A1, A2i);
            Ki = invx(subx(M.Mn, mmx(G, M.Pl)));
            const Blk<NB> GM = subx(PE, mmx(G, ME));
            Rn = mmx(Ki, GM);
            Sm = mmx(A2i, subx(ME, mmx(M.Pl, Rn)));
            Mni = Rn;                                                        // not used for i > 0
        }

        // ---- per angle ----
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            if (k >= na) break;
            const SHCArgs::Angle &g = ang[k];
            const double iu1 = g.iu1, x = g.iu0, x2 = g.x2;
            const double edt = fexp2(dt * g.nl1, K);                         // exp(-dtau/u1)
            // particular solution eta_l = Delta_l / Delta (:3397-3416) with b_1 = b_3 = 0
            const double b2 = (fw2 * g.p2u0) * (0.25 / PI);
            const double iDel = frcp(9 * ((g.x4 - M.beta * x2) + M.gama));
            const double P = fma(a2, 7.0, -(9 * x2)), Q = fma(a0, 3.0, -x2);
            const double a3b2 = 7.0 * b2, b0x = b0 * x;
            const double B_ = a3b2 - 2 * a3b0, C_ = -b0x, E_ = -(3 * (b2 * x)), F_ = -(3 * b0x);
            double eta[4];
            eta[0] = fma(A_, P, 2 * (B_ * x2)) * iDel;
            eta[1] = fma(C_, P, -((2 * a0) * (a3b2 * x))) * iDel;
            eta[2] = fma(a3b2, Q, -(14.0 * (C_ * x))) * iDel;
            eta[3] = fma(E_, Q, 2 * (F_ * x2)) * iDel;
            const double h0 = 0.5 * eta[0], e58 = 0.625 * eta[2], m0 = -0.125 * eta[0];
            const double zpl0 = ((h0 + eta[1]) + e58) * (2 * PI), zmn0 = ((h0 - eta[1]) + e58) * (2 * PI);
            const double zpl1 = ((m0 + e58) + eta[3]) * (2 * PI), zmn1 = ((m0 + e58) - eta[3]) * (2 * PI);
            // exp(-tau/u0) at the layer top and bottom.  e_top carries the UNCLIPPED value: in the symmetric geometry
            // (u0 == u1) the bottom one is the top one times exp(-dtau/u1), already at hand -- one multiply instead of a
            // 15-instruction polynomial -- and the reference's exp(-clip35(tau/u0)) (:3418-3421) is max(., e^-35) of it
            // (exp is monotonic).  Other geometries form the exponential of the running sum tau directly.
            const double pt = e_top[k];
            const double pb = g.sym ? pt * edt : fexp2(tau_b * g.nl0, K);
            e_top[k] = pb;
            const double ed = fmax(pt, EXP_M35), eu = fmax(pb, EXP_M35);
            const double zmn_dn[NB] = {zmn0 * ed, zmn1 * ed}, zpl_dn[NB] = {zpl0 * ed, zpl1 * ed};
            const double zmn_up[NB] = {zmn0 * eu, zmn1 * eu}, zpl_up[NB] = {zpl0 * eu, zpl1 * eu};

            // source-function weights along u1 (:2898-2970, 3601-3605): the odd moments vanish
            const double e01 = fma(g.hp2u1, M.Q[0], 1.0), e23 = fma(g.hp2u1, M.Q[1], 1.0);
            const double cm[4] = {e01, e01, e23, e23};
            const double Tk = T[k];
            const double Ti = Tk * iu1, tw = Ti * w0;
            const bool noclip_lane = (iu1 + M.lam[0]) * dt <= 35.0;          // per lane; the work is wave-uniform (sh_body)
            const bool noclip = __all(noclip_lane);
            double gd[NB], gv[NB];
#pragma unroll
            for (int r = 0; r < NB; ++r) {
                const double alpha = iu1 + M.lam[r], beta = iu1 - M.lam[r];
                const double rab = frcp(alpha * beta);
                double ea = edt * M.E[r], eb = edt * M.iE[r];
                if (!noclip) {
                    const double ead = fexpk(-clip35(alpha * dt), K), ebd = fexpk(-clip35(beta * dt), K);
                    ea = noclip_lane ? ea : ead;
                    eb = noclip_lane ? eb : ebd;
                }
                const double ha = (1 - ea) * (rab * beta), hb = (1 - eb) * (rab * alpha);
                gd[r] = (tw * cm[2 * r]) * ha;
                gv[r] = ((tw * cm[2 * r + 1]) * hb) * M.E[r];
            }
            // (1 - exp(-clip35(mus dtau)))/mus (:2901-2905); mus = 2/u1 in the symmetric geometry
            const bool sq_lane = g.sym && (g.mus * dt <= 35.0);
            double e_mus = edt * edt;
            if (!__all(sq_lane)) {
                const double d = fexp2_clip(dt * g.nlm, K);
                e_mus = sq_lane ? e_mus : d;
            }
            const double om = 1 - e_mus;
            const double expon1 = (om * g.imus) * ed;
            const double Nsum = fma(g.hp2u1, eta[2], eta[0]) * expon1;      // :2919-2920, 2945-2948
            // exp(-tau_og/u0) at the layer top, unclipped (:2962): tau_og = tau without cloud
            const double e_tauo = pt;
            const double single = ((sgl * om) * e_tauo) * g.imus;
            double c = Ti * fma(w0, Nsum, single);
            const double Tn = Tk * edt;
            T[k] = Tn;
            if (i == n - 1) {             // xint[n] = flux_bot/pi = (Pl E d + Mn v + zpl_up)[0]/pi  (:2891, :2967)
                const double tp = Tn * (1.0 / PI);
#pragma unroll
                for (int r = 0; r < NB; ++r) {
                    gd[r] = fma(tp, PE.m[0][r], gd[r]);
                    gv[r] = fma(tp, M.Mn.m[0][r], gv[r]);
                }
                c = fma(tp, zpl_up[0], c);
            }
            // elimination, right-hand sides
            double z2[NB], deltan[NB];
            mtvx(Rn, gd, z2);
            if (i == 0) {
                const double bt[NB] = {a.b_top - zmn_dn[0], -a.b_top / 4 - zmn_dn[1]};    // :3479-3480
                mvx(Mni, bt, deltan);
                kappa[k] = c + dotx(gd, deltan);
#pragma unroll
                for (int r = 0; r < NB; ++r) zeta[k][r] = gv[r] - z2[r];
            } else {
                double cP[NB], cM[NB], t1[NB], t2[NB], rhs[NB], tv[NB], t[NB], z1[NB];
                mvx(pPE, delta[k], t1);
                mvx(pME, delta[k], t2);
#pragma unroll
                for (int r = 0; r < NB; ++r) {
                    cP[r] = (zpl_dn[r] - p_zpl_up[k][r]) - t1[r];
                    cM[r] = (t2[r] + p_zmn_up[k][r]) - zmn_dn[r];
                }
                mvx(G, cP, rhs);
#pragma unroll
                for (int r = 0; r < NB; ++r) rhs[r] += cM[r];
                mvx(Ki, rhs, deltan);
                mvx(M.Pl, deltan, tv);
#pragma unroll
                for (int r = 0; r < NB; ++r) tv[r] += cP[r];
                mvx(A2i, tv, t);
                kappa[k] = ((kappa[k] + dotx(zeta[k], t)) + dotx(gd, deltan)) + c;
                mtvx(Sm, zeta[k], z1);
#pragma unroll
                for (int r = 0; r < NB; ++r) zeta[k][r] = (z1[r] + gv[r]) - z2[r];
            }
#pragma unroll
            for (int r = 0; r < NB; ++r) {
                delta[k][r] = deltan[r];
                p_zmn_up[k][r] = zmn_up[r];
                p_zpl_up[k][r] = zpl_up[r];
            }
        }
        R = Rn;
        pMn = M.Mn; pPl = M.Pl; pME = ME; pPE = PE;
        tau_t = tau_b;
    }
    if (a.state) {
        // hand the sweep over at the top of layer nstop: shared blocks (every angle chunk holds the same values; the
        // first one writes them), then this lane's angles
        double *sp = a.state + w;
        auto st = [&](int sl, double v) { sp[(long)sl * a.nwno] = v; };
        if (blockIdx.y == 0) {
            int sl = 0;
            const Blk<NB> *const blks[5] = {&R, &pMn, &pPl, &pME, &pPE};
#pragma unroll
            for (int b = 0; b < 5; ++b)
#pragma unroll
                for (int r = 0; r < NB; ++r)
#pragma unroll
                    for (int c2 = 0; c2 < NB; ++c2) st(sl++, blks[b]->m[r][c2]);
        }
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            if (k >= na) break;
            int sl = SHC_SHARED + SHC_STATE * (a.first_angle + k0 + k);
            st(sl++, T[k]);
            st(sl++, kappa[k]);
            st(sl++, e_top[k]);
#pragma unroll
            for (int r = 0; r < NB; ++r) st(sl++, zeta[k][r]);
#pragma unroll
            for (int r = 0; r < NB; ++r) st(sl++, delta[k][r]);
#pragma unroll
            for (int r = 0; r < NB; ++r) st(sl++, p_zmn_up[k][r]);
#pragma unroll
            for (int r = 0; r < NB; ++r) st(sl++, p_zpl_up[k][r]);
        }
        return;
    }
    // ---- surface rows (:3484-3494) ----
    Blk<NB> W, L;
#pragma unroll
    for (int r = 0; r < NB; ++r)
#pragma unroll
        for (int s_ = 0; s_ < NB; ++s_) {
            W.m[r][s_] = fma(-rs, pME.m[r][s_], pPE.m[r][s_]);
            L.m[r][s_] = fma(-rs, pPl.m[r][s_], pMn.m[r][s_]);
        }
    const Blk<NB> Li = invx(subx(L, mmx(W, R)));
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        if (k >= na) break;
        const SHCArgs::Angle &g = ang[k];
        const double bsf = (rs * g.u0) * F * fexpk(-(tau_t * g.iu0), K);     // :2863-2864
        const double bs[NB] = {bsf, -bsf / 4};
        double wd[NB], rhs[NB], v[NB];
        mvx(W, delta[k], wd);
#pragma unroll
        for (int r = 0; r < NB; ++r) rhs[r] = ((bs[r] - p_zpl_up[k][r]) + rs * p_zmn_up[k][r]) - wd[r];
        mvx(Li, rhs, v);
        a.xint[(long)(k0 + k) * a.nwno + w] = kappa[k] + dotx(zeta[k], v);
    }
}

int launch_sh4_clear(picaso_ctx *ctx, SHCArgs &a, int nang, const double *ubar0, const double *ubar1, double *xint)
{
    return sh_launch_chunks(ctx, a.nwno, nang, 190.0, 275.0, "PICASO_AMD_SHC_ANGLES", SHC_MAX_PER_LANE,
                            [&](int done, int na, int per_lane, int chunks) {
        for (int k = 0; k < na; ++k) {
#pragma clang fp contract(off)
            const SHArgs::Angle s = make_sh_angle(ubar0[done + k], ubar1[done + k], false);
            SHCArgs::Angle &g = a.ang[k];
            g.u0 = s.u0; g.iu0 = s.iu0; g.iu1 = s.iu1; g.mus = s.mus; g.imus = s.imus;
            g.nl0 = s.nl0; g.nl1 = s.nl1; g.nlm = s.nlm;
            g.x2 = g.iu0 * g.iu0;
            g.x4 = g.x2 * g.x2;
            const double m0 = -s.u0, m1 = s.u1;                                  // legP (fluxes.py:3639-3646)
            g.p2u0 = (3 * m0 * m0 - 1) / 2;
            g.hp2u1 = 0.5 * ((3 * m1 * m1 - 1) / 2);
            g.sym = (s.u0 == s.u1) ? 1 : 0;
        }
        a.na = na;
        a.first_angle = done;
        a.xint = xint + (size_t)done * a.nwno;
        const dim3 grid((unsigned)((a.nwno + 255) / 256), (unsigned)chunks);
        if (per_lane == 1) hipLaunchKernelGGL(k_sh4_clear<1>, grid, dim3(256), 0, ctx->stream, a);
        else hipLaunchKernelGGL(k_sh4_clear<2>, grid, dim3(256), 0, ctx->stream, a);
    });
}

}  // namespace pz
