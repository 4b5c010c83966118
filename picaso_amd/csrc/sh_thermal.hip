// Spherical-harmonics thermal emission: the angle-independent block algebra shared between the disk angles of a
// lane -- gfx950.
//
// In get_thermal_SH (fluxes.py:2979-3182) the angle enters only through the source-function integration along ubar1
// (:3105-3182): the Legendre weights, the stream matrices, the particular solution and therefore the whole sweep
// relation d_i = delta_i - R_i v_i are the same for every (g, t).  k_sh<NB, true> (sh_sweep.hip) nevertheless redoes
// them per angle (one wave per angle: 5 x 560 fp64 instructions per wavelength-layer at five angles).  Here one lane
// carries NA angles: per layer the modes, the Planck terms and the elimination once (~400 instructions), and per angle
// only exp(-dtau/ubar1), the integration weights (gd, gv, c) and the update of its TOA functional (kappa, zeta, T):
// ~110 instructions each.  Small launches keep fewer angles per lane (down to one) so that every SIMD has a wave.
#include <type_traits>

#include "sh.hpp"
#include "sh_blocks.hpp"

#pragma clang fp contract(off)   // every fma is written out: an angle's bits do not depend on how many share its lane

namespace pz {

template <int NB, int NA>
__global__ __launch_bounds__(256, 2) void k_sh_thermal(const SHTArgs a)
{
    constexpr int NS = 2 * NB;
    using ModesT = typename std::conditional<NB == 2, ModesT4, ModesT2>::type;
    const long w = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= a.nwno) return;
    const int n = a.nlayer;
    const long pitch = a.pitch;
    const int k0 = blockIdx.y * NA;                 // this lane's angles: k0 .. k0 + na - 1 (the last chunk may be short)
    const int na = min(NA, a.na - k0);
    const SHTArgs::Angle *const ang = a.ang + k0;
    Exp2Coef K;
    K.load();
    const double rs = a.surf_reflect[w], wn = a.wno[w];
    // Planck function at the levels (fluxes.py:3058-3060): planck_lambda with its level-independent factors hoisted
    const double hP = 6.62607004e-27, cP_ = 2.99792458e+10, kP = 1.38064852e-16;
    const double wcm = 1.0 / wn, w2 = wcm * wcm;
    const double pf = (2.0 * hP * (cP_ * cP_)) / (w2 * w2 * wcm), wk = wcm * kP, hc = hP * cP_;
    auto planck = [&](double t) { return pf * planck_rcp(fexpk(fdiv(hc, t * wk), K)); };
    double Bn = planck(a.tlevel[0]);
    const double B_top = Bn;
    double b1 = 0.0;
    // per angle: transmission to the top, TOA functional J = kappa + zeta . v
    double T[NA], kappa[NA], zeta[NA][NB];
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        T[k] = 1.0;
        kappa[k] = 0.0;
#pragma unroll
        for (int r = 0; r < NB; ++r) zeta[k][r] = 0.0;
    }
    double delta[NB];
    Blk<NB> R, pMn, pPl, pME, pPE;
    double p_zmn_up[NB], p_zpl_up[NB];
#pragma unroll
    for (int r = 0; r < NB; ++r) delta[r] = p_zmn_up[r] = p_zpl_up[r] = 0.0;

    for (int i = 0; i < n; ++i) {
        const long o = (long)i * pitch + w;
        const double dt = a.dtau[o], w0 = a.w0[o], cbo = a.cosb_og[o];
        // ---- Legendre weights and stream coefficients (:3072-3083) ----
        double wmu[NS], al[NS];
        {
            const double c2 = cbo * cbo;
            const double ff = a.use_ff ? ((NS == 4) ? c2 * c2 : c2) : 0.0;
            const double iff = frcp(1 - ff);
            double cl = 1.0;
#pragma unroll
            for (int l = 0; l < NS; ++l) {
                wmu[l] = ((2 * l + 1) * (cl - ff)) * iff;
                al[l] = fma(-w0, wmu[l], (double)(2 * l + 1));
                cl *= cbo;
            }
        }
        ModesT M;
        if constexpr (NB == 2) modes_sh4x(al, dt, M, K);
        else modes_sh2x(al, dt, M, K);
        // ---- particular solution (:3451-3459 / :3266-3270) ----
        const double B0 = Bn;
        Bn = planck(a.tlevel[i + 1]);
        b1 = (Bn - B0) * frcp(dt);
        const double omw = 1 - w0;
        const double ia0 = frcp(al[0]), ia1 = frcp(al[1]);
        const double oma = omw * ia0, b1a = b1 * ia1, hB = 0.5 * B0, hbd = 0.5 * (b1 * dt);
        double zmn_dn[NB], zpl_dn[NB], zmn_up[NB], zpl_up[NB];
        zmn_dn[0] = (oma * (hB - b1a)) * (2 * PI);
        zpl_dn[0] = (oma * (hB + b1a)) * (2 * PI);
        zmn_up[0] = (oma * ((hB - b1a) + hbd)) * (2 * PI);
        zpl_up[0] = (oma * ((hB + b1a) + hbd)) * (2 * PI);
        if constexpr (NB == 2) {
            zmn_dn[1] = zpl_dn[1] = ((-0.125 * oma) * B0) * (2 * PI);
            zmn_up[1] = zpl_up[1] = ((-0.125 * oma) * fma(b1, dt, B0)) * (2 * PI);
        }
        const Blk<NB> ME = scale_cols(M.Mn, M.E), PE = scale_cols(M.Pl, M.E);

        // ---- elimination (angle independent) ----
        Blk<NB> Rn, Sm;
        double deltan[NB], t[NB];
        if (i == 0) {
            const double tau_top = dt * a.plevel[0] / (a.plevel[1] - a.plevel[0]);   // :3062-3063
            const double b_top = PI * (1.0 - fexpk(-tau_top / 0.5, K)) * B_top;
            double bt[NB];
            bt[0] = b_top - zmn_dn[0];                                               // :3479-3480 / :3283
            if constexpr (NB == 2) bt[1] = -b_top / 4 - zmn_dn[1];
            const Blk<NB> Mni = invx(M.Mn);
            Rn = mmx(Mni, PE);
            mvx(Mni, bt, deltan);
#pragma unroll
            for (int r = 0; r < NB; ++r) t[r] = 0.0;
            Sm = Rn;                                       // not used for i == 0
        } else {
            const Blk<NB> A1 = subx(pPl, mmx(pME, R)), A2 = subx(pMn, mmx(pPE, R));
            const Blk<NB> A2i = invx(A2);
            const Blk<NB> G = mmx(A1, A2i);
            double cP[NB], cM[NB], t1[NB], t2[NB];
            mvx(pPE, delta, t1);
            mvx(pME, delta, t2);
#pragma unroll
            for (int r = 0; r < NB; ++r) {
                cP[r] = (zpl_dn[r] - p_zpl_up[r]) - t1[r];
                cM[r] = (t2[r] + p_zmn_up[r]) - zmn_dn[r];
            }
            const Blk<NB> Ki = invx(subx(M.Mn, mmx(G, M.Pl)));
            const Blk<NB> GM = subx(PE, mmx(G, ME));
            Rn = mmx(Ki, GM);
            double rhs[NB];
            mvx(G, cP, rhs);
#pragma unroll
            for (int r = 0; r < NB; ++r) rhs[r] += cM[r];
            mvx(Ki, rhs, deltan);
            Sm = mmx(A2i, subx(ME, mmx(M.Pl, Rn)));
            double tv[NB];
            mvx(M.Pl, deltan, tv);
#pragma unroll
            for (int r = 0; r < NB; ++r) tv[r] += cP[r];
            mvx(A2i, tv, t);
        }

        // ---- per angle: source-function integrals of this layer and the update of the TOA functional ----
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            if (k >= na) break;
            const double u1 = ang[k].u1, iu1 = ang[k].iu1;
            const double edt = fexp2(dt * ang[k].nl1, K);                         // exp(-dtau/u1)
            double cm[NS];
            if constexpr (NB == 2) {                                                 // :3601-3605
                const double wP2 = wmu[2] * ang[k].p2, wP1 = wmu[1] * ang[k].p1, wP3 = wmu[3] * ang[k].p3;
                const double e01 = fma(wP2, M.Q[0], wmu[0]), e23 = fma(wP2, M.Q[1], wmu[0]);
                const double o01 = fma(wP3, M.S[0], wP1 * M.R[0]), o23 = fma(wP3, M.S[1], wP1 * M.R[1]);
                cm[0] = e01 + o01;
                cm[1] = e01 - o01;
                cm[2] = e23 + o23;
                cm[3] = e23 - o23;
            } else {                                                                 // :3124-3125
                const double wq = (wmu[1] * ang[k].p1) * M.q;
                cm[0] = wmu[0] - wq;
                cm[1] = wmu[0] + wq;
            }
            const double Tk = T[k];
            const double tw = ((Tk * iu1) * w0) * (2 * PI);                          // :3167
            const bool noclip_lane = (iu1 + M.lam[0]) * dt <= 35.0;      // per lane; the work is wave-uniform (see sh_body)
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
            const double edc = (NB == 2) ? fmax(edt, EXP_M35) : edt;               // exp(-clip35(dtau/u1)) :3154 vs :3127
            const double core = oma * u1;
            const double dtu = dt + u1;
            const double N0 = wmu[0] * (core * fma(B0, 1 - edc, b1 * fma(-dtu, edc, u1)));     // :3128, :3155
            const double N1 = (wmu[1] * ang[k].p1) * (core * ((b1 * (1 - edc)) * ia1));      // :3129, :3156
            const double direct = ((2 * PI) * omw) * (u1 * fma(B0, 1 - edt, b1 * fma(-dtu, edt, u1)));   // :3163-3165
            double c = (Tk * iu1) * fma(w0 * (N0 + N1), 2 * PI, direct);
            const double Tn = Tk * edt;
            if (i == n - 1)                                                          // :3173-3176
                c = fma(Tn, a.hard_surface ? Bn * (2 * PI) : fma(b1, u1, Bn) * (2 * PI), c);
            double z2[NB];
            mtvx(Rn, gd, z2);
            if (i == 0) {
                kappa[k] = c + dotx(gd, deltan);
#pragma unroll
                for (int r = 0; r < NB; ++r) zeta[k][r] = gv[r] - z2[r];
            } else {
                kappa[k] = ((kappa[k] + dotx(zeta[k], t)) + dotx(gd, deltan)) + c;
                double z1[NB];
                mtvx(Sm, zeta[k], z1);
#pragma unroll
                for (int r = 0; r < NB; ++r) zeta[k][r] = (z1[r] + gv[r]) - z2[r];
            }
            T[k] = Tn;
        }
        R = Rn;
#pragma unroll
        for (int r = 0; r < NB; ++r) {
            delta[r] = deltan[r];
            p_zmn_up[r] = zmn_up[r];
            p_zpl_up[r] = zpl_up[r];
        }
        pMn = M.Mn; pPl = M.Pl; pME = ME; pPE = PE;
    }
    // ---- surface rows (:3484-3494 / :3287-3289) ----
    double bs[NB];
    bs[0] = a.hard_surface ? PI * Bn : PI * fma(b1, 0.5, Bn);                        // :3065-3068
    if constexpr (NB == 2) bs[1] = -(PI * Bn) / 4;                                   // :3070
    Blk<NB> W, L;
#pragma unroll
    for (int r = 0; r < NB; ++r)
#pragma unroll
        for (int s_ = 0; s_ < NB; ++s_) {
            W.m[r][s_] = fma(-rs, pME.m[r][s_], pPE.m[r][s_]);
            L.m[r][s_] = fma(-rs, pPl.m[r][s_], pMn.m[r][s_]);
        }
    L = subx(L, mmx(W, R));
    double wd[NB], rhs[NB], v[NB];
    mvx(W, delta, wd);
#pragma unroll
    for (int r = 0; r < NB; ++r) rhs[r] = ((bs[r] - p_zpl_up[r]) + rs * p_zmn_up[r]) - wd[r];
    mvx(invx(L), rhs, v);
#pragma unroll
    for (int k = 0; k < NA; ++k)
        if (k < na) a.xint[(long)(k0 + k) * a.nwno + w] = kappa[k] + dotx(zeta[k], v);
}

int launch_sh_thermal(picaso_ctx *ctx, SHTArgs &a, int stream, int nang, const double *ubar1, double *xint)
{
    constexpr int MAX_NA = 5;                                   // [NB - 1][angles per lane - 1]
    static void (*const kernel[2][MAX_NA])(const SHTArgs) = {
        {k_sh_thermal<1, 1>, k_sh_thermal<1, 2>, k_sh_thermal<1, 3>, k_sh_thermal<1, 4>, k_sh_thermal<1, 5>},
        {k_sh_thermal<2, 1>, k_sh_thermal<2, 2>, k_sh_thermal<2, 3>, k_sh_thermal<2, 4>, k_sh_thermal<2, 5>}};
    return sh_launch_chunks(ctx, a.nwno, nang, 400.0, 110.0, "PICASO_AMD_SHT_ANGLES", MAX_NA,
                            [&](int done, int na, int per_lane, int chunks) {
        for (int k = 0; k < na; ++k) {
#pragma clang fp contract(off)
            SHTArgs::Angle &g = a.ang[k];
            const double mu = ubar1[done + k];
            g.u1 = mu;
            g.iu1 = 1.0 / mu;
            g.nl1 = -LOG2E * g.iu1;
            g.p1 = mu;                                                             // legP (fluxes.py:3639-3646)
            g.p2 = (3 * mu * mu - 1) / 2;
            g.p3 = (5 * mu * mu * mu - 3 * mu) / 2;
        }
        a.na = na;
        a.xint = xint + (size_t)done * a.nwno;
        const dim3 grid((unsigned)((a.nwno + 255) / 256), (unsigned)chunks);
        hipLaunchKernelGGL(kernel[stream == 4][per_lane - 1], grid, dim3(256), 0, ctx->stream, a);
    });
}

}  // namespace pz
