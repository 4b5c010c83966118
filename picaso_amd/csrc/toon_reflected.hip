// Toon89 two-stream reflected light, top-of-atmosphere intensity -- gfx950.
//
// Replaces fluxes.get_reflected_1d / get_reflected_3d (reference picaso/fluxes.py:1009-1413,
// :354-660) for the spectrum path (get_toa_intensity=1, get_lvl_flux=0).
//
// Mapping: one LANE per wavelength column (3-D: per (wavelength, facet) column, facet index
// fastest exactly as the reference stores it), so every plane read is a coalesced 512-B row
// segment of the reference's own (nlayer, nwno[, ng, nt]) layout -- no transpose anywhere.
// All `NA` disk angles that share the planes are carried in registers of the same lane: the
// angle-independent work (g1, g2, lambda, Gamma, exp(lambda dtau), p_single, the elimination
// factors) is done once per layer instead of once per angle.
//
// Algorithm: the reference builds a 2n x 2n tridiagonal system per (wavelength, angle), solves it
// (Thomas, two sweeps) and then runs a bottom-up source-function recursion.  The matrix does not
// depend on the angle (only the right-hand side does) and the TOA intensity is a LINEAR functional
// of the solution, so the whole thing collapses into ONE top-down sweep with O(1) state:
//   * unknowns per layer are Toon's own (pos_i, neg_i) = (Y1+Y2, Y1-Y2); the flux-continuity
//     equations at interface i|i+1 are (reference fluxes.py:1227-1231 expressions)
//         EP_i pos_i + G_i EM_i neg_i + c+dn_i = pos_{i+1} + G_{i+1} neg_{i+1} + c+up_{i+1}
//         G_i EP_i pos_i + EM_i neg_i + c-dn_i = G_{i+1} pos_{i+1} + neg_{i+1} + c-up_{i+1}
//     (the reference's rows 2i+1, 2i+2, fluxes.py:161-175, are invertible combinations of these);
//   * sweeping down we keep the one relation everything above imposes on layer i,
//         neg_i = delta_i - rho_i pos_i            (rho shared by all angles, delta per angle)
//     and the TOA functional of layers 0..i as an affine function of the only free unknown,
//         J_{<=i} = kappa_i + zeta_i pos_i        (per angle),
//     using pos_{i-1} = s_i pos_i + t_i (contracting: s ~ exp(-lambda dtau));
//   * the surface row (fluxes.py:178-181) fixes pos_{n-1}; xint_at_top = kappa + zeta pos.
// Each input element is read exactly once; nothing but the result is written.  Against the
// reference the result differs only by rounding (<= 1e-10 relative on the golden scenes, at the
// level of the reference's own fp64 conditioning); see tests/test_parity_gpu.py.
//
// The kernel is FP64-VALU bound (~20 fp64 instructions per algorithmic byte at 5 angles), so the
// code below is organised around instruction count: lean exp / reciprocal / rsqrt helpers
// (device_math.hpp), first and last layer peeled out of the loop, host-precomputed per-angle
// constants (SGPR resident), and -- for the symmetric geometry -- exponentials carried as running
// products when the cumulative optical depth really is the running sum of the layer depths.
#include "common.hpp"
#include "device_math.hpp"

namespace pz {

// The three numeric tuning parameters of the file (-D overridable: PICASO_HIPCC_EXTRA with tools/ab.sh).  None selects a
// code path.
// Two waves per SIMD: one fp64 wave alone issues at most every ~5.1 cycles (tools/ubench/
// f64_rates.hip) while the pipe accepts one per ~3.5-4, and a 1e5-column spectrum is only 1.5 waves
// per SIMD, so co-residency beats the extra scratch spills (measured 0.405 ms vs 0.481 ms).
#ifndef PZ_REFL_MINWAVES
#define PZ_REFL_MINWAVES 2
#endif
// threads per block (the LDS state tile is [var][angle][PZ_REFL_BLOCK])
#ifndef PZ_REFL_BLOCK
#define PZ_REFL_BLOCK 256
#endif

// Per-angle sweep state (7 doubles per angle).  D1 = c+dn + Gamma EM delta, D2 = c-dn + EM delta of
// the layer above: the only combinations of (c+dn, c-dn, delta) the next interface and the surface
// row need.  For NA >= LDS_MIN_ANGLES part of the state lives in LDS ([var][angle][lane], so a wave's
// ds_read_b64 / ds_write_b64 hit 64 consecutive 8-byte words: conflict free): all in registers the
// 5-angle kernel needs ~300 VGPRs, i.e. either one wave per SIMD or ~50 registers spilled to
// scratch, whose reloads share the vmcnt queue with the plane prefetch.
constexpr int NSTATE = 7;
enum { S_T = 0, S_XU, S_EO, S_KAPPA, S_ZETA, S_D1, S_D2 };   // late-use variables last
constexpr int LDS_MIN_ANGLES = 4;

// NLDS = how many of the state variables (counted from the END of the enum order above) live in
// LDS when LDS is on; the rest stay in registers.
// Measured on the 5-angle headline case: 0 -> 50 VGPRs spilled to scratch (0.416 ms), 4 -> no
// spills, 41 KB LDS per block (0.410 ms), 7 -> 72 KB (0.421 ms): the kernel is VALU-issue bound,
// so 4 is chosen for being spill-free with the smaller LDS footprint.
#ifndef PZ_REFL_NLDS
#define PZ_REFL_NLDS 4
#endif

template <int NA, bool LDS>
struct ReflState {
    static constexpr int NL = LDS ? PZ_REFL_NLDS : 0;      // variables [NSTATE-NL, NSTATE) in LDS
    static constexpr int NR = NSTATE - NL;
    double reg[NR > 0 ? NR : 1][NA];
    double *lds;                                   // this lane's column of the block's LDS tile
    double rho, pgam, pEM;
    __device__ __forceinline__ double get(int var, int k) const
    {
        return (var >= NR) ? lds[((var - NR) * NA + k) * PZ_REFL_BLOCK] : reg[var < NR ? var : 0][k];
    }
    __device__ __forceinline__ void set(int var, int k, double v)
    {
        if (var >= NR) lds[((var - NR) * NA + k) * PZ_REFL_BLOCK] = v;
        else reg[var < NR ? var : 0][k] = v;
    }
};

struct LayerIn {
    double dt, tau_n, w0, g, gcos2, fc, fr, dto, tauo, w0o, cbo;
    // wave-uniform flags, set when the layer is consumed:
    bool cum_tau;    // tau[i+1] == tau[i] + dtau[i] bit-exactly: exp(-tau[i+1]/u) = exp(-tau[i]/u) exp(-dtau/u)
    bool eo_ok;      // tau_og[i] == tau_og[i-1] + dtau_og[i-1]: the carried product is exp(-tau_og[i]/u)
    bool same_dt;    // dtau_og == dtau (no delta-scaling in this layer)
    bool nocld;      // ftau_cld == 0 (no cloud in this layer)
    bool allf;       // cum_tau && eo_ok && same_dt
    bool af_cloud;   // cum_tau && eo_ok && !same_dt on a layer with cloud
};

// The copies of the layer body.  All perform the general body's operations on the same numbers, so which copy runs a
// layer never changes a bit; the later ones leave out what their layer is known not to need.
//   BODY_GENERAL          any layer: the wave-uniform flags of LayerIn are tested per angle.
//   BODY_CLOUD            cum_tau and eo_ok hold, same_dt does not (the usual cloud layer: delta-scaled, so dtau_og != dtau
//                         and the two extra exponentials are always formed), straight-line.
//   BODY_CLEAR            cum_tau, eo_ok and same_dt hold and no lane has cloud (ftau_cld == 0, checked per wave by the
//                         caller or known from a seal): every term that carries ftau_cld*cosb drops out.  The remaining
//                         operations are the general ones with fcg = +0 folded by hand (x + 0, x * 1 and fma(0, y, z)
//                         are exact).
//   BODY_CLEAR_TOP        BODY_CLEAR where no layer above was delta-scaled: exp(-tau_og/u0) is S_XU (it starts at
//                         fexp2_cold(-0) = 1.0 and e0o == e0 in a layer with dtau_og == dtau), so S_EO is neither read nor
//                         kept.
//   BODY_CLEAR_TOP_SMALL  BODY_CLEAR_TOP where every lane's |dtau| is at most a.dt_small, so dtau * nl1 lies within +-1/2
//                         for every angle of the launch and et is formed by fexp2_small -- fexp2 without its four range-
//                         reduction instructions, the same bits (device_math.hpp).  e0 is et there; EP takes another
//                         argument and keeps the general form.
//   BODY_CLEAR_TOP_SMALL_EP  BODY_CLEAR_TOP_SMALL in a launch with a.ep_small: every w0 lies in [0, 1], so lam <= sqrt(3),
//                         and the angle table is small enough that lam * dtau * log2(e) lies within +-1/2 as well (the
//                         launcher's proof, api.hip refl_ep_small): EP by fexp2_small too, the same bits.
// Assuming the flags (every copy but the general one) removes the 3-4 wave-uniform branches per angle they feed and the
// fall-back exponentials behind them; DESIGN.md section 6 has what each copy measured.
enum Body { BODY_GENERAL, BODY_CLOUD, BODY_CLEAR, BODY_CLEAR_TOP, BODY_CLEAR_TOP_SMALL, BODY_CLEAR_TOP_SMALL_EP };

// One layer of the sweep.  FIRST / LAST are compile-time so the top row and the bottom-boundary
// terms cost nothing inside the loop.  ZP: every angle has ubar0 == ubar1 (symmetric 1-D geometry,
// reference justdoit.py:1513-1532): exp(-dtau (u0+u1)/(u0 u1)) = exp(-dtau/u1)^2, and when the
// level optical depths are the exact running sums of the layer depths (how compute_opacity builds
// them, optics.py:353-354, 418-420) exp(-tau[i+1]/u0) = exp(-tau[i]/u0) exp(-dtau[i]/u1) needs no
// exponential of its own.  The check is bit-exact and per wave, so arbitrary caller-supplied tau
// planes still take the direct exp(-tau/u0).
// FAST: the reference's default options (config.json: quadrature coefficients, TTHG_ray single
// scattering with frac_c = 2, N=2 multiple scattering) fixed at compile time -- with ZP also cos_theta = 1: no option
// branches in the layer loop and the option values leave the SGPR file (the generic 5-angle kernel spills 49 SGPRs to
// VGPR lanes, this one 23).
// KIND: the copy of the body (above).
// XT: S_T (the running exp(-tau/u1)) and S_XU (exp(-tau/u0)) are one number -- u0 == u1, both start at 1.0 (fexp2 of
// 0 * nl1 = -0: rint -0, f = +0, fma(0, p, 1) = 1, ldexp(1, 0)), cum_tau holds by construction and every layer multiplies
// both by et -- so S_XU alone is carried: five multiplies and ten VGPRs per layer in every copy of the body.  The
// zero-phase default-options kernels that form the level sums themselves (reflected_toa_body's ZDRV).
template <int NA, bool IS3D, bool ZP, bool FIRST, bool LAST, bool LDS, bool FAST = false, Body KIND = BODY_GENERAL,
          bool XT = false>
__device__ __forceinline__ void reflected_layer(const ReflectedArgs &a, const LayerIn &L,
                                                ReflState<NA, LDS> &S,
                                                const ReflectedArgs::Angle (&g)[NA],
                                                const Exp2Coef &K, double F, double clip, int tc_,
                                                double b_top)
{
    // Every floating-point operation below is written out: contraction is off and each fused
    // multiply-add is an explicit fma().  With the compiler free to contract (hipcc's default) the
    // template instantiations (angles per lane, FAST, the body copy, first/last layer) each got their own choice
    // of fused operations and disagreed in the last bits (5e-12 relative between the one-angle and the
    // five-angle kernel): a column's result depended on how the launch was shaped.  Now it does not.
#pragma clang fp contract(off)
    // what the copy knows: NC no cloud in the layer; AF cum_tau and eo_ok hold, and same_dt is as SDT says (1: holds,
    // 2: does not); EOX eo is S_XU; SX small exponent arguments
    constexpr bool NC = KIND >= BODY_CLEAR, AF = KIND != BODY_GENERAL, EOX = KIND >= BODY_CLEAR_TOP;
    constexpr bool SX = KIND >= BODY_CLEAR_TOP_SMALL, SEP = KIND == BODY_CLEAR_TOP_SMALL_EP;
    constexpr int SDT = KIND == BODY_CLOUD ? 2 : 1;
    static_assert(!(XT || EOX) || (FAST && ZP), "XT, BODY_CLEAR_TOP*: the zero-phase default-options kernels only");
    const int tc = FAST ? 0 : tc_;
    const int single_phase = FAST ? 3 : a.single_phase;
    const int multi_phase = FAST ? 0 : a.multi_phase;
    const double cos_theta = (FAST && ZP) ? 1.0 : a.cos_theta;   // zero phase: cos_theta = 1 (what ZP geometry means)
    const double frac_c = FAST ? 2.0 : a.frac_c;
    const double dt = L.dt, w0 = L.w0;
    // ---- angle-independent layer quantities (fluxes.py:1132-1141, 1172-1177) ----
    const double fcg = NC ? 0.0 : L.fc * L.g;
    double g1, g2, lam, lam2;
    if (NC) toon_gammas_nocld(tc, w0, g1, g2, lam, lam2);
    else toon_gammas(tc, w0, fcg, g1, g2, lam, lam2);
    const double E = fmin(lam * dt, clip);
    // SEP: the launcher's proof and the caller's vote say |E log2(e)| <= 1/2 in every lane: same bits
    const double EP = SEP ? fexp2_small(E * -NEG_LOG2E, K) : fexp2(E * -NEG_LOG2E, K);
    // 1/g2 and 1/EP from one reciprocal (g2 of order w0 <= 1, EP <= e^35: the product stays in range; g2 = 0 -- a layer
    // that does not scatter -- is NaN in Gamma here as in the reference's (g1 - lamda)/g2, fluxes.py:1141)
    const double r_ge = frcp(g2 * EP);
    const double ig2 = r_ge * EP, EM = r_ge * g2;
    const double gam = (g1 - lam) * ig2;
    // No cloud anywhere in this layer of the wave (ftau_cld == 0 in every lane, checked per wave):
    // TTHG_ray's p_single = ftau_cld tthg + ftau_ray 3/4 (1 + cos^2) is its Rayleigh part alone
    // (bit-identical: 0 * tthg + x = x), without the two Henyey-Greenstein terms.
    double ps;
    if ((NC || L.nocld) && single_phase == 3)
        ps = L.fr * (0.75 * fma(cos_theta, cos_theta, 1.0));
    else
        ps = p_single<IS3D>(single_phase, L.cbo, L.gcos2, L.fc, L.fr, cos_theta, a.frac_a, a.frac_b,
                            frac_c, a.constant_back, a.constant_forward);
    const double ssa_h = (L.w0o * F * (0.125 / PI)) * ps;  // (w0_og F0PI/4pi) p_single / 2, fluxes.py:1397-1398
    const double w2pi = w0 * (0.5 / PI);                   // fluxes.py:1290-1296
    const double Fw0h = (0.5 * F) * w0;
    const double gcq = (multi_phase == 0) ? L.gcos2 : 0.0;   // N=2 vs N=1 (fluxes.py:1275-1287)
    // The direct-beam coefficients (fluxes.py:1146-1169) with g3 = 1/2 - c u0, g4 = 1/2 + c u0
    // (c = sqrt(3) fcg/2 quadrature, 3 fcg/4 Eddington) and u0 (1/u0) = 1 collapse to
    //   2 (g4 (g1 + 1/u0) + g2 g3) = A0 + hz,   2 (g3 (g1 - 1/u0) + g2 g4) = A0 - hz,
    //   A0 = g1 + g2 + 2c,  hz = 1/u0 + 2c (g1 - g2) u0,
    // and the multiple-scattering brackets (fluxes.py:1275-1296) with B0 = 1 + gcos2 q2 to
    //   (1 + 1.5 fcg u1 + q) + Gamma (1 - 1.5 fcg u1 + q) = (1 + Gamma) B0 + (1 - Gamma) 1.5 fcg u1  etc.
    const double c2 = NC ? 0.0 : ((tc == 1) ? 1.5 * fcg : SQ3 * fcg);
    const double A0 = NC ? (g1 + g2) : (g1 + g2) + c2;
    const double A1 = NC ? 0.0 : c2 * (g1 - g2);
    const double c15 = NC ? 0.0 : 1.5 * fcg;
    const double gp = 1.0 + gam;
    const double gmc = NC ? 0.0 : (1.0 - gam) * c15;
    const double w2gp = w2pi * gp, w2gmc = NC ? 0.0 : w2pi * gmc;      // common factors of the two mode integrals
    const double w2A0 = w2pi * A0;                                    // ... and of the undelta-scaled layer source

    // ---- elimination factors shared by all angles ----
    double a1i = 0.0, a2i = 0.0, ia = 0.0, rho_n = gam, sfac = 0.0;
    if (!FIRST) {
        const double em2 = S.pEM * S.pEM;
        const double a1 = fma(-(S.pgam * em2), S.rho, 1.0);
        const double a2 = fma(-em2, S.rho, S.pgam);
        const double d1 = fma(-gam, a2, a1);
        const double r12 = frcp(d1 * a1);                  // one reciprocal for 1/d1 and 1/a1
        const double inv = r12 * a1;
        a1i = a1 * inv;
        a2i = a2 * inv;
        rho_n = fma(gam, a1i, -a2i);
        ia = S.pEM * (r12 * d1);
        sfac = fma(-gam, rho_n, 1.0) * ia;
    }
    const double gEM = gam * EM;

    // One v_rcp_f64 (quarter rate) per angle for 1/den, 1/(lu-1) and 1/(lu+1): q_k = den_k (lu_k - 1)
    // (lu_k + 1).  Every factor is itself good to 1 ulp (lm1 is exact by Sterbenz near the lambda u1 = 1
    // singularity), so the results stay within a few ulp -- which matters: at lambda u1 -> 1 the
    // particular and homogeneous parts cancel with an amplification ~1/|lambda u1 - 1|.
    // The reciprocal takes ONE Newton step (frcp1, 2^-46): it is a common factor of every beam term of the layer and of
    // the mode integrals, so its error scales the layer's particular solution and the homogeneous response to it alike
    // (device_math.hpp; bounded by tools/headline_error_x87.py and tests/test_refl_coop_gpu.py).
    // One per angle, not one for all angles of the layer by batch inversion of their running product (-1.3 % time at five
    // angles): an angle's result would then depend, in its last bits, on which angles share its lane -- on the angle
    // chunking and on whether a small wavelength shard takes the one-angle-per-wave path.  As it is, a column's result
    // is bit-identical however the grid is sharded and the angles are grouped; the multi-GPU path and its tests rely on it.
    double den_[NA], lm1_[NA], lp1_[NA], lml_[NA], r3_[NA];
    {
        double q[NA], P[NA];
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            den_[k] = sub_unfused(lam2, g[k].iu0sq);   // lambda^2 - 1/u0^2, reference rounding
            const double lu = lam * g[k].u1;
            lm1_[k] = lu - 1.0;
            lp1_[k] = lu + 1.0;
            lml_[k] = lm1_[k] * lp1_[k];
            q[k] = den_[k] * lml_[k];
            // The running product that batch inversion would invert.  Nothing reads it and no instruction comes of it, but
            // without this line hipcc allocates registers differently in the 58 FAST kernels of three and more angles;
            // it stays until a change that may move the ISA takes it out.
            P[k] = (k == 0) ? q[0] : P[k - 1] * q[k];
        }
#pragma unroll
        for (int k = 0; k < NA; ++k) r3_[k] = frcp1(q[k]);
    }

#pragma unroll
    for (int k = 0; k < NA; ++k) {
        const double u1_k = g[k].u1, u0_k = ZP ? g[k].u1 : g[k].u0, iu0_k = g[k].iu0;
        const double nl1_k = g[k].nl1, nl0_k = ZP ? g[k].nl1 : g[k].nl0, q2_k = g[k].q2;
        const double wq2_k = ZP ? 1.0 : g[k].wq2;
        const double den = den_[k], lm1 = lm1_[k], lp1 = lp1_[k], lml = lml_[k];
        const double r3 = r3_[k];
        const double rden = r3 * lml;                      // 1/den
        const double rd = r3 * den;                        // 1/((lu-1)(lu+1))
        const double hz = NC ? iu0_k : fma(A1, u0_k, iu0_k);
        const double am2 = A0 + hz, ap2 = A0 - hz;
        // exp(-dtau/u1).  SX: the caller's vote says |dt * nl1_k| <= 1/2 in every lane and for every angle: same bits
        const double et = SX ? fexp2_small(dt * nl1_k, K) : fexp2(dt * nl1_k, K);
        const double e0 = ZP ? et : fexp2(dt * nl0_k, K);    // exp(-dtau/u0)
        const double xu = S.get(S_XU, k), Tk = XT ? xu : S.get(S_T, k);
        const double xd = (AF || XT || L.cum_tau) ? xu * e0 : fexp2_cold(L.tau_n * nl0_k, K);
        const double fw = Fw0h * rden;
        const double fx = fw * xu;
        const double cmu = am2 * fx, cpu = ap2 * fx;       // c-/c+ at the top of the layer
        double cmd, cpd;                                   // ... and at the bottom
        if (AF || L.cum_tau) {                             // xd = xu e0: the bottom terms are the top ones times e0
            cmd = cmu * e0;
            cpd = cpu * e0;
        } else {
            const double fxd = fw * xd;
            cmd = am2 * fxd;
            cpd = ap2 * fxd;
        }
        S.set(S_XU, k, xd);
        // source-function coefficients (fluxes.py:1275-1296, 1395-1406)
        const double B0 = fma(gcq, q2_k, 1.0);
        const double h15 = NC ? 0.0 : c15 * u1_k;
        const double Aqq = NC ? B0 * A0 : fma(B0, A0, -(h15 * hz));       // (mpl c+ + mmi c-) / (2 fx)
        const double ee = fma(EP, et, -1.0), ff = fma(-EM, et, 1.0);
        // the two mode integrals, their common factors T/(lu^2 - 1) w0/2pi (1 + Gamma) B0 multiplied once
        // (x + 0 = x - 0 = x exactly: the cloud-free copies and the general body agree bit for bit on a layer without cloud)
        const double Trd = Tk * rd, wX = w2gp * B0;
        const double wY = NC ? 0.0 : w2gmc * u1_k;
        double vp = ((Trd * (NC ? wX : wX + wY)) * lp1) * ee;
        double vn = ((Trd * (NC ? wX : wX - wY)) * lm1) * ff;
        // exp(-tau_og[i]/u0): the running product of the layers above when tau_og really is the
        // running sum of dtau_og, else formed directly
        const double eo = EOX ? xu : (!FIRST && (AF || L.eo_ok)) ? S.get(S_EO, k) : fexp2_cold(L.tauo * nl0_k, K);
        // 1 - exp(-dtau (1/u0 + 1/u1)) and the same for dtau_og (fluxes.py:1395-1406) from the two
        // single-angle exponentials; a layer that is not delta-scaled (dtau_og == dtau) shares them
        const double t2 = fma(-e0, et, 1.0);
        double t1 = t2, e0o = e0;
        if (AF ? (SDT == 2) : !L.same_dt) {
            const double e1o = fexp2_cold(L.dto * nl1_k, K);
            e0o = ZP ? e1o : fexp2_cold(L.dto * nl0_k, K);
            t1 = fma(-e0o, e1o, 1.0);
        }
        if (!LAST && !EOX) S.set(S_EO, k, eo * e0o);
        // S0 = (ssa eo t1 + Aq t2) u0/(u0+u1) with Aq = 2 w2pi fx Aqq; wq2 = 2 u0/(u0+u1) (1 if ZP)
        double S0;
        if (ZP && (NC || L.nocld) && (AF ? (SDT != 2) : L.same_dt)) {
            // t1 == t2 and Aqq = B0 A0 (no cloud: the general body's h15 hz is +0): S0 = t2 (ssa eo + (w0/2pi A0) (B0 fx))
            S0 = fma(w2A0, B0 * fx, ssa_h * eo) * t2;
        } else {
            const double s1 = (ssa_h * wq2_k) * (eo * t1);
            S0 = fma((w2pi * wq2_k) * fx, Aqq * t2, s1);
        }
        double kap = fma(Tk, S0, S.get(S_KAPPA, k));
        const double Tn = XT ? xd : Tk * et;               // XT: xd = xu e0 is Tk et
        if (LAST) {                                        // xint[n] = flux_zero/pi (fluxes.py:1266-1270)
            vp = fma(Tn * EP, 1.0 / PI, vp);
            vn = fma((Tn * gam) * EM, 1.0 / PI, vn);
            kap = fma(Tn * cpd, 1.0 / PI, kap);
        }
        double delta_n;
        if (FIRST) {                                       // top row (fluxes.py:155-158)
            delta_n = b_top - cmu;
            S.set(S_ZETA, k, fma(-vn, gam, vp));
            kap = fma(vn, delta_n, kap);
        } else {
            const double rP = cpu - S.get(S_D1, k);
            const double rM = cmu - S.get(S_D2, k);
            const double zeta = S.get(S_ZETA, k);
            delta_n = fma(a2i, rP, -(a1i * rM));
            const double t = fma(gam, delta_n, rP) * ia;
            kap = fma(zeta, t, fma(vn, delta_n, kap));
            S.set(S_ZETA, k, fma(-vn, rho_n, fma(zeta, sfac, vp)));
        }
        S.set(S_KAPPA, k, kap);
        if (!XT) S.set(S_T, k, Tn);
        S.set(S_D1, k, fma(gEM, delta_n, cpd));
        S.set(S_D2, k, fma(EM, delta_n, cmd));
    }
    S.rho = rho_n;
    S.pgam = gam;
    S.pEM = EM;
}

// albedo + xint*gweight*tweight in the reference's operation order, unfused (disco.py:145-146), so the
// fused disk sum, k_compress and numpy agree bit for bit
__device__ __forceinline__ double disk_accumulate(double acc, double x, double gw, double tw)
{
#pragma clang fp contract(off)
    return acc + x * gw * tw;
}

// sym_fac*0.5*albedo/F0PI*(cos_theta+1) (disco.py:148), the same operations as k_compress
__device__ __forceinline__ double disk_finish(double c1, double acc, double F, double cos_theta)
{
#pragma clang fp contract(off)
    return c1 * acc / F * (cos_theta + 1.0);
}

// The kernel body.  `bx_in` = this workgroup's column group within its spectrum, `by_in` = its angle group,
// `angp` = the angle table (the kernel argument's, or the batch entry's).
// BIG: one wave per SIMD (grids of up to 1 024 column-waves, five angles): the whole 512-entry register file
// belongs to the wave, so the sweep state stays in registers instead of LDS -- 50 000 columns 0.1365 ms against
// 0.1636 (round-2 sweep), same bits.  Of no use to the 1e5-column launch: its 1 563 waves need
// two per SIMD.
// DRV: which planes exist.  Planes that compute_opacity derives exactly from others may be left out (NULL) and are
// re-derived here with the same operations instead of being written to and read from HBM --
//   tau / tau_og   : running sums of dtau / dtau_og from 0 at the top (optics.py:353-354, 418-420)
//   gcos2          : 0.5 ftau_ray (optics.py:342)
//   ftau_cld (with cosb, cosb_og, ftau_ray, gcos2): column without cloud: 0, 0, 0, 1, 0.5 (optics.py:335-342
//                    with TAUCLD = 0)
//   dtau_og / w0_og: no delta-scaling (cosb = 0: f = 0, optics.py:412-420 reduce to x*1): dtau / w0
// all wave-uniform (kernel arguments).  The 3-D entry point and the 1-D default-options launches take these patterns (the
// product leaves tau / tau_og / gcos2 -- and for a cloud-free atmosphere everything but dtau and w0 -- out of HBM; a 1-D
// caller asks picaso_reflected_1d_can_derive first); every other 1-D launch is handed all eleven planes.
//   0  all eleven planes, the branch-free load sequence (the conditional loads cost the HBM-bound facet kernel 7 %).
//   1  any pattern of the above, looked up per plane at run time.
//   2  ("CLEAR") ONLY dtau and w0 exist -- the pattern of an atmosphere without cloud -- known at compile time: no flag, no
//      test and no copy of the body but the cloud-free ones survive.
//   3  ("LEVELS") the other pattern of the product (a cloudy atmosphere): tau, tau_og and gcos2 left out, the cloud planes
//      present -- known at compile time, so the two tests of "the level depths are the running sums" (they are: they are
//      formed here), the exec-mask tests and the branches behind them disappear from every layer.
//   4  ("LAYERS") 3 plus what a seal knows about the layers (planeseal.hip): bit i of a.lmask says that layer i carries no
//      cloud in ANY column of the set -- ftau_cld = 0, ftau_ray = 1, dtau_og = dtau, w0_og = w0, bit for bit.  Such a layer
//      is read and prepared as 2 does it (dtau and w0 alone, the constants put in, no vote, straight to a cloud-free copy
//      of the body); every other layer is 3 unchanged.  The values put in ARE the stored ones and the votes would have
//      passed, so the same copy of the body runs on the same numbers.
//
// The sweep.  The first and the last layer are peeled out.  Kernels with one, two or (FAST, ZP) five angles per lane
// prefetch into two register sets used alternately and sweep the interior two layers per trip, in up to four loops:
//   * the masked loop -- every kernel: per layer the mask test (DRV = 4), prep's votes and the choice between
//     BODY_CLEAR, BODY_CLOUD and BODY_GENERAL (FAST; the generic kernels have the general body alone);
//   * the top-run loop -- TOPRUN kernels: the run of known cloud-free layers from the top (DRV = 2: the whole column,
//     DRV = 4: by the mask) loads two planes per layer without looking at the mask, waits for them by count and runs
//     BODY_CLEAR_TOP.  It starts in its small-argument form (BODY_CLEAR_TOP_SMALL, a trip of two layers is 758 VALU
//     instructions against 793) and leaves that for good at the first trip with a layer that fails the vote.  Where the
//     run ends S_EO is set from S_XU once;
//   * the deck-run loop -- DECKRUN kernels: every maximal run of known cloud-free interior layers BELOW the top run
//     (under a cloud deck) is swept like the top run, by BODY_CLEAR, which keeps S_EO; the masked loop's mask test,
//     vmcnt(0) and dispatch block around each such layer (15-22 VALU) go;
//   * the cloud-run loop -- DECKRUN kernels: every run of layers the seal found cloudy and delta-scaled in EVERY column
//     (a.cmask) is swept by BODY_CLOUD with eight loads per layer under counted waits: prep's two votes are known to
//     fail, so they, the mask test, the vmcnt(0) and the dispatch go here too.
// The top run's small-argument form has a second copy for launches with a.ep_small (BODY_CLEAR_TOP_SMALL_EP).
// The other angle counts keep one prefetch set, a copy per layer and the masked loop's dispatch.
template <int NA, bool IS3D, bool ZP, bool FAST, bool BIG, int DRV, typename AnglePtr>
__device__ __forceinline__ void reflected_toa_body(const ReflectedArgs &a, const unsigned bx_in, const unsigned by_in,
                                                   AnglePtr angp)
{
#pragma clang fp contract(off)      // operations as written, see reflected_layer
    const unsigned bx = bx_in, by = by_in;
    const long col = bx * (long)blockDim.x + threadIdx.x;
    if (col >= a.ncol) return;
    const int nfac = IS3D ? a.nfac : 1;
    const long w = IS3D ? col / nfac : (a.ncolper > 1 ? col / a.ncolper : col);
    const int fac = IS3D ? (int)(col - w * nfac) : 0;
    const int n = a.nlayer;
    const long pitch = a.pitch;
    const double clip = IS3D ? 40.0 : 35.0;            // fluxes.py:516 vs :1174
    const int tc = IS3D ? 0 : a.toon_coefficients;     // 3-D is quadrature only (fluxes.py:489)
    const double b_top = IS3D ? 0.0 : a.b_top;         // fluxes.py:522

    Exp2Coef K;
    K.load();
    ReflectedArgs::Angle g[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        if (IS3D) {
            const double v0 = fabs(a.u0_tab[fac]), v1 = fabs(a.u1_tab[fac]);   // fluxes.py:467-468
            g[k].u0 = v0;
            g[k].u1 = v1;
            g[k].iu0 = 1.0 / v0;
            g[k].iu0sq = 1.0 / (v0 * v0);              // as the reference forms it (fluxes.py:1155)
            g[k].nl0 = NEG_LOG2E / v0;
            g[k].nl1 = NEG_LOG2E / v1;
            g[k].nlm = NEG_LOG2E * (1.0 / v0 + 1.0 / v1);
            g[k].wq2 = 2.0 * (v0 / (v0 + v1));
            const double ubar2 = 0.767;                 // fluxes.py:1280
            g[k].q2 = (3.0 * ubar2 * ubar2 * v1 * v1 - 1.0) / 2.0;
            g[k].wgt = g[k].wgt2 = 0.0;
        } else {                                        // host-precomputed, wave-uniform
            const auto &src = angp[by * NA + k];        // by: angle group (0 unless ny > 1)
            g[k].u1 = src.u1; g[k].iu0 = src.iu0; g[k].iu0sq = src.iu0sq; g[k].nl1 = src.nl1; g[k].q2 = src.q2;
            g[k].u0 = src.u0; g[k].nl0 = src.nl0; g[k].nlm = src.nlm; g[k].wq2 = src.wq2; g[k].wgt = src.wgt;
            g[k].wgt2 = src.wgt2;
        }
    }
    const double F = a.F0PI[w], rs = a.surf_reflect[w];

    const double *p_dtau = a.dtau + col, *p_tau = a.tau + col, *p_w0 = a.w0 + col,
                 *p_cosb = a.cosb + col, *p_gcos2 = a.gcos2 + col, *p_fc = a.ftau_cld + col,
                 *p_fr = a.ftau_ray + col, *p_dto = a.dtau_og + col, *p_tauo = a.tau_og + col,
                 *p_w0o = a.w0_og + col, *p_cbo = a.cosb_og + col;

    constexpr bool LDS = (NA >= LDS_MIN_ANGLES) && !IS3D && !BIG;
    __shared__ double lds_state[LDS ? (PZ_REFL_NLDS > 0 ? PZ_REFL_NLDS : 1) * NA * PZ_REFL_BLOCK : 1];
    ReflState<NA, LDS> S;
    S.lds = lds_state + threadIdx.x;
    S.rho = S.pgam = S.pEM = 0.0;
    constexpr bool CLEAR = (DRV == 2), LAYERS = (DRV == 4), LEVELS = (DRV == 3) || LAYERS;
    // the zero-phase default-options kernels that form the level sums themselves: cum_tau holds by construction and
    // u0 == u1, so S_XU stands for S_T in every copy of the body (reflected_layer's XT)
    constexpr bool ZDRV = FAST && ZP && !IS3D && (CLEAR || LEVELS);
    constexpr bool TOPRUN = ZDRV && (CLEAR || LAYERS);     // cloud-free layers are known before they are loaded: run loops
    constexpr bool DECKRUN = ZDRV && LAYERS;               // ... below the top run as well
    // a first / last layer known to be cloud-free takes a straight-line cloud-free copy of the body.  The last layer of the
    // DRV = 4 kernels does not: a third and fourth copy of it beside the general ones gave them a private segment
    constexpr bool CLEAR_FIRST = TOPRUN, CLEAR_LAST = ZDRV && CLEAR;
    const double dt_small = a.dt_small;
    // wave-uniform; a NaN fails it
    auto small_dt = [&](double dt) -> bool { return __all(__builtin_fabs(dt) <= dt_small); };
    // the mask, read once
    unsigned long long m0 = 0, m1 = 0;
    if constexpr (LAYERS) {
        m0 = a.lmask[0];
        m1 = a.lmask[1];
    }
    // the deck mask (layers cloudy and delta-scaled in every column), read once; 0 without cloud runs
    unsigned long long c0 = 0, c1 = 0;
    if constexpr (LAYERS) {
        c0 = a.cmask[0];
        c1 = a.cmask[1];
    }
    auto layer_clear = [&](int i) -> bool {          // wave-uniform: the mask is a kernel argument / a table entry
        if constexpr (LAYERS) return (((i & 64) ? m1 : m0) >> (i & 63)) & 1ull;
        return false;
    };
    const bool derive_tau = CLEAR || LEVELS || (DRV && a.tau == nullptr);
    const bool derive_tauo = CLEAR || LEVELS || (DRV && a.tau_og == nullptr);
    const bool derive_g2 = CLEAR || LEVELS || (DRV && a.gcos2 == nullptr);
    const bool clear = CLEAR || (!LEVELS && DRV && a.ftau_cld == nullptr);
    const bool alias_og = CLEAR || (!LEVELS && DRV && a.dtau_og == nullptr);
    double tau_i = derive_tau ? 0.0 : p_tau[0];
    double tauo_pred = 0.0;          // tau_og[i-1] + dtau_og[i-1] of the layer above
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        S.set(S_T, k, 1.0);
        S.set(S_KAPPA, k, 0.0);
        S.set(S_ZETA, k, 0.0);
        S.set(S_D1, k, 0.0);
        S.set(S_D2, k, 0.0);
        S.set(S_EO, k, 0.0);
        // ZDRV: tau_i is +0.0, the product -0.0 and fexp2 of it exactly 1.0 (see reflected_layer's XT)
        S.set(S_XU, k, ZDRV ? 1.0 : fexp2(mul_unfused(tau_i, ZP ? g[k].nl1 : g[k].nl0), K));
    }

    // Software prefetch with two register sets used alternately (loop unrolled by two): the eleven
    // plane loads of layer i+1 are issued before layer i is computed and nothing has to be copied
    // between the sets, so they stay in flight for a whole layer (a copy would force the wave to
    // drain vmcnt at the end of every layer, which costs the HBM-bound facet kernel ~25 %).
    // FAST: planes addressed as (uniform base) + (32-bit lane offset): one v_add_u32 per layer for all
    // eleven loads (global_load ... saddr) instead of eleven 64-bit lane address adds (-2.5 % time); the launcher
    // checks that a plane is smaller than 4 GB
    const unsigned voff0 = (unsigned)(col * 8);
    const unsigned pitch8 = (unsigned)(pitch * 8);
    auto ld = [&](const double *base, unsigned off) {
        return *(const double *)((const char *)base + off);
    };
    auto load = [&](LayerIn &L, int i, bool in_loop = false) {
        if constexpr (FAST && DRV) {               // planes left out: only what exists is loaded
            const unsigned o = voff0 + (unsigned)i * pitch8;
            if constexpr (LAYERS) {
                // The number of loads now differs from layer to layer, and a wait for the OTHER register set counted in
                // instructions issued since would have to assume the smaller number: it would wait for part of this
                // prefetch.  So the other set (issued a whole layer ago) is waited for here, by name, before this one
                // is issued: s_waitcnt vmcnt(0), the other counters left alone.
                if (in_loop) __builtin_amdgcn_s_waitcnt(0x0F70);
            }
            L.dt = ld(a.dtau, o);
            L.w0 = ld(a.w0, o);
            if constexpr (CLEAR) return;
            if constexpr (LAYERS) {
                if (layer_clear(i)) return;
            }
            if constexpr (LEVELS) {
                L.g = ld(a.cosb, o);
                L.fc = ld(a.ftau_cld, o);
                L.fr = ld(a.ftau_ray, o);
                L.cbo = ld(a.cosb_og, o);
                L.dto = ld(a.dtau_og, o);
                L.w0o = ld(a.w0_og, o);
                return;
            }
            if (!derive_tau) L.tau_n = ld(a.tau + pitch, o);
            if (!clear) {
                L.g = ld(a.cosb, o);
                L.fc = ld(a.ftau_cld, o);
                L.fr = ld(a.ftau_ray, o);
                L.cbo = ld(a.cosb_og, o);
                if (!derive_g2) L.gcos2 = ld(a.gcos2, o);
            }
            if (!alias_og) {
                L.dto = ld(a.dtau_og, o);
                L.w0o = ld(a.w0_og, o);
            }
            if (!derive_tauo) L.tauo = ld(a.tau_og, o);
            return;
        }
        if constexpr (FAST) {
            const unsigned o = voff0 + (unsigned)i * pitch8;
            L.dt = ld(a.dtau, o);
            L.tau_n = ld(a.tau + pitch, o);
            L.w0 = ld(a.w0, o);
            L.g = ld(a.cosb, o);
            L.gcos2 = ld(a.gcos2, o);
            L.fc = ld(a.ftau_cld, o);
            L.fr = ld(a.ftau_ray, o);
            L.dto = ld(a.dtau_og, o);
            L.tauo = ld(a.tau_og, o);
            L.w0o = ld(a.w0_og, o);
            L.cbo = ld(a.cosb_og, o);
            return;
        }
        const long o = (long)i * pitch;
        L.dt = p_dtau[o];
        L.w0 = p_w0[o];
        if constexpr (DRV) {                       // only the loads are issued here; derived values in prep
            if (!derive_tau) L.tau_n = p_tau[o + pitch];
            if (!clear) {
                L.g = p_cosb[o];
                L.fc = p_fc[o];
                L.fr = p_fr[o];
                L.cbo = p_cbo[o];
                if (!derive_g2) L.gcos2 = p_gcos2[o];
            }
            if (!alias_og) {
                L.dto = p_dto[o];
                L.w0o = p_w0o[o];
            }
            if (!derive_tauo) L.tauo = p_tauo[o];
            return;
        }
        L.tau_n = p_tau[o + pitch];
        L.g = p_cosb[o];
        L.gcos2 = p_gcos2[o];
        L.fc = p_fc[o];
        L.fr = p_fr[o];
        L.dto = p_dto[o];
        L.tauo = p_tauo[o];
        L.w0o = p_w0o[o];
        L.cbo = p_cbo[o];
    };
    auto prep = [&](LayerIn &L, bool lclear) {
        if (CLEAR || (LAYERS && lclear)) {
            L.g = 0.0; L.fc = 0.0; L.fr = 1.0; L.gcos2 = 0.5; L.cbo = 0.0;
            L.dto = L.dt; L.w0o = L.w0;
            L.tau_n = tau_i + L.dt;
            L.tauo = tauo_pred;
            L.cum_tau = L.eo_ok = L.same_dt = L.nocld = L.allf = true;
            L.af_cloud = false;
            tau_i = L.tau_n;
            tauo_pred = L.tauo + L.dto;
            return;
        }
        if constexpr (LEVELS) {
            L.gcos2 = 0.5 * L.fr;
            L.tau_n = tau_i + L.dt;
            L.tauo = tauo_pred;
            L.cum_tau = L.eo_ok = true;
            L.same_dt = __all(L.dto == L.dt);
            L.nocld = __all(L.fc == 0.0);
            L.allf = L.same_dt;
            L.af_cloud = !L.same_dt && !L.nocld;
            tau_i = L.tau_n;
            tauo_pred = L.tauo + L.dto;
            return;
        }
        if constexpr (DRV) {
            if (clear) { L.g = 0.0; L.fc = 0.0; L.fr = 1.0; L.gcos2 = 0.5; L.cbo = 0.0; }
            else if (derive_g2) L.gcos2 = 0.5 * L.fr;
            if (alias_og) { L.dto = L.dt; L.w0o = L.w0; }
            if (derive_tau) L.tau_n = tau_i + L.dt;
            if (derive_tauo) L.tauo = tauo_pred;
        }
        L.cum_tau = __all(L.tau_n == tau_i + L.dt);
        L.eo_ok = __all(L.tauo == tauo_pred);
        L.same_dt = __all(L.dto == L.dt);
        L.nocld = __all(L.fc == 0.0);
        L.allf = L.cum_tau && L.eo_ok && L.same_dt;
        L.af_cloud = L.cum_tau && L.eo_ok && !L.same_dt && !L.nocld;
        tau_i = L.tau_n;
        tauo_pred = L.tauo + L.dto;
    };
    // one layer by one copy of the body
#define PZ_BODY(FIRST_, LAST_, KIND_, L_) \
    reflected_layer<NA, IS3D, ZP, FIRST_, LAST_, LDS, FAST, KIND_, ZDRV>(a, L_, S, g, K, F, clip, tc, b_top)
    // a layer of the masked loop, and the first and the last layer: whichever copy the mask and prep's votes allow
#define PZ_LAYER(FIRST_, LAST_, L_, I_)                                                                  \
    do {                                                                                                 \
        const bool lclear_ = layer_clear(I_);                                                            \
        prep(L_, lclear_);                                                                               \
        constexpr bool interior_ = !(FIRST_) && !(LAST_);                                                \
        /* a first / last layer known to be cloud-free (the seal's mask, DRV = 2): the straight-line copy; nothing */ \
        /* above the first layer is delta-scaled */                                                      \
        constexpr bool kend_ = !interior_ && (!(FIRST_) || CLEAR_FIRST) && (!(LAST_) || CLEAR_LAST);      \
        constexpr Body kcopy_ = !kend_ ? BODY_GENERAL : (FIRST_) ? BODY_CLEAR_TOP : BODY_CLEAR;          \
        if (kend_ && (CLEAR || lclear_))                                                                 \
            PZ_BODY(FIRST_, LAST_, kcopy_, L_);                                                          \
        else if (FAST && interior_ && L_.nocld && L_.allf)                                               \
            PZ_BODY(FIRST_, LAST_, BODY_CLEAR, L_);                                                      \
        else if (FAST && interior_ && L_.af_cloud)                                                       \
            PZ_BODY(FIRST_, LAST_, BODY_CLOUD, L_);                                                      \
        else                                                                                             \
            PZ_BODY(FIRST_, LAST_, BODY_GENERAL, L_);                                                    \
        if constexpr (CLEAR) __builtin_amdgcn_sched_barrier(0);   /* straight-line code: keep the layers apart */ \
    } while (0)
    // a layer of a run (TOPRUN / DECKRUN kernels): known cloud-free, KIND_ as the loop says
#define PZ_RUN_LAYER(KIND_, L_)                                                                          \
    do {                                                                                                 \
        prep(L_, true);                                                                                  \
        PZ_BODY(false, false, KIND_, L_);                                                                \
        __builtin_amdgcn_sched_barrier(0);                                                               \
    } while (0)

    // a layer of a cloud run (DECKRUN kernels): the seal knows that prep's two votes fail in every wave -- every column has
    // !(ftau_cld == 0) and !(dtau_og == dtau) -- so prep's LEVELS branch is taken without them, straight to BODY_CLOUD
#define PZ_CLOUD_LAYER(L_)                                                                               \
    do {                                                                                                 \
        L_.gcos2 = 0.5 * L_.fr;                                                                          \
        L_.tau_n = tau_i + L_.dt;                                                                        \
        L_.tauo = tauo_pred;                                                                             \
        L_.cum_tau = L_.eo_ok = L_.af_cloud = true;                                                      \
        L_.same_dt = L_.nocld = L_.allf = false;                                                         \
        tau_i = L_.tau_n;                                                                                \
        tauo_pred = L_.tauo + L_.dto;                                                                    \
        PZ_BODY(false, false, BODY_CLOUD, L_);                                                           \
        __builtin_amdgcn_sched_barrier(0);                                                               \
    } while (0)
    // ... its loads: the eight planes of a LEVELS layer, no mask looked at, no wait by name
    auto load_cloud = [&](LayerIn &L, int l) {
        const unsigned o = voff0 + (unsigned)l * pitch8;
        L.dt = ld(a.dtau, o);
        L.w0 = ld(a.w0, o);
        L.g = ld(a.cosb, o);
        L.fc = ld(a.ftau_cld, o);
        L.fr = ld(a.ftau_ray, o);
        L.cbo = ld(a.cosb_og, o);
        L.dto = ld(a.dtau_og, o);
        L.w0o = ld(a.w0_og, o);
    };
    // a layer of a run: dtau and w0 alone
    auto load_clear = [&](LayerIn &L, int l) {
        const unsigned o = voff0 + (unsigned)l * pitch8;
        L.dt = ld(a.dtau, o);
        L.w0 = ld(a.w0, o);
    };
    // Two register sets used alternately (no copy) for one or two angles per lane -- the HBM-bound 3-D facet
    // kernel -- and for five in the zero-phase default-options kernels: there the eleven v_mov_b64 of the copy are
    // 2.3 % of the launch (0.2357 -> 0.2302 ms, same box, no spills at 254 VGPRs).  Three angles spill with a second
    // set (14 VGPRs), the generic five-angle kernel spills 30; four and six to eight (chunked launches, rarely used)
    // are left on the copying form.
    constexpr bool TWO_SETS = (NA <= 2) || (NA == 5 && FAST && ZP);
    LayerIn A, B;
    load(A, 0);
    if (n == 1) {
        PZ_LAYER(true, true, A, 0);
    } else if constexpr (TWO_SETS) {
        load(B, 1);
        PZ_LAYER(true, false, A, 0);
        int i = 1;                               // B holds layer i
        if constexpr (TOPRUN) {
            // r: the number of cloud-free layers from the top (scalar bit operations on the mask; DRV = 2: all of them)
            int r = n;
            if constexpr (LAYERS) {
                r = (~m0) ? __builtin_ctzll(~m0) : 64 + ((~m1) ? __builtin_ctzll(~m1) : 64);
                r = r < n ? r : n;
            }
            if (r >= 1) {
                // The top-run loop.  Layers i, i+1 and the two prefetched ones (i+1, i+2) all belong to the run: two loads
                // each, so the compiler's own counted vmcnt waits do, and no mask is looked at.
                // Its small-argument form first: a trip runs while both of its layers pass the vote, then the sweep
                // moves to the general form below for the rest of the run and never comes back.  Both votes are
                // taken before the trip on values loaded a trip ago -- B, and dtau of layer i + 1 read one layer
                // further ahead than the rest of A (two more VGPRs) -- so the loop has one exit and each trip is
                // one straight-line block of two layers; the row index is clamped to the last layer of the planes.
                if (i + 2 < r) {
                    double dt_a = ld(a.dtau, voff0 + (unsigned)(i + 1) * pitch8);
                    bool go = small_dt(B.dt) && small_dt(dt_a);
#define PZ_SMALL_LOOP(KIND_)                                                                             \
                    while (go) {                                                                         \
                        A.dt = dt_a;                                                                     \
                        A.w0 = ld(a.w0, voff0 + (unsigned)(i + 1) * pitch8);                             \
                        PZ_RUN_LAYER(KIND_, B);                                                          \
                        load_clear(B, i + 2);                                                            \
                        dt_a = ld(a.dtau, voff0 + (unsigned)(i + 3 < n ? i + 3 : n - 1) * pitch8);       \
                        PZ_RUN_LAYER(KIND_, A);                                                          \
                        i += 2;                                                                          \
                        go = i + 2 < r && small_dt(B.dt) && small_dt(dt_a);                              \
                    }
                    // a.ep_small (DRV = 4, a kernel argument, looked at once): a second copy of the loop whose EP takes
                    // fexp2_small as well
                    if constexpr (LAYERS) {
                        if (a.ep_small) PZ_SMALL_LOOP(BODY_CLEAR_TOP_SMALL_EP)
                    }
                    PZ_SMALL_LOOP(BODY_CLEAR_TOP_SMALL)
#undef PZ_SMALL_LOOP
                }
                for (; i + 2 < r; i += 2) {
                    load_clear(A, i + 1);
                    PZ_RUN_LAYER(BODY_CLEAR_TOP, B);
                    load_clear(B, i + 2);
                    PZ_RUN_LAYER(BODY_CLEAR_TOP, A);
                }
                // the run ends here (the layers left of it, at most two, take the masked loop): from now on S_EO is kept.
                // Layer 0 was cloud-free, so whichever copy of the body ran it, S_EO is S_XU at this point, bit for bit.
#pragma unroll
                for (int k = 0; k < NA; ++k) S.set(S_EO, k, S.get(S_XU, k));
            }
        }
        for (; i + 2 <= n - 1; i += 2) {         // the masked loop: layers i and i+1 are interior, layer i+2 exists
            if constexpr (DECKRUN) {
                // The cloud-run loop: a run of sealed deck layers (a.cmask) is swept two per trip by BODY_CLOUD straight-line:
                // eight loads per layer under the compiler's counted waits, no vote, no mask test, no wait by name, no
                // dispatch.  ec: one past the run that starts at layer i, the last layer left out.  A trip needs layers i
                // and i + 1 in the run; layer i + 2, which it prefetches, need not be: the eight planes are whatever the
                // masked loop or a deck run would have loaded for it and more (a clear layer's six extra values are
                // overwritten by prep), and i + 2 <= ec <= n - 1 is a row of the planes.  So a run is swept to its end
                // when its length is even and to its last layer but one when odd.  Ahead of the deck-run loop, so that the clear
                // layers under a deck go straight on to that.
                const unsigned long long wc = i < 64 ? (c0 >> i) | (i ? c1 << (64 - i) : 0ull) : c1 >> (i - 64);
                int ec = i + ((~wc) ? __builtin_ctzll(~wc) : 64);
                ec = ec < n - 1 ? ec : n - 1;
                if (i + 2 <= ec) {
                    for (; i + 2 <= ec; i += 2) {
                        load_cloud(A, i + 1);
                        PZ_CLOUD_LAYER(B);
                        load_cloud(B, i + 2);
                        PZ_CLOUD_LAYER(A);
                    }
                    if (!(i + 2 <= n - 1)) break;
                }
                // The deck-run loop: a run of sealed cloud-free interior layers below the top run (under a cloud deck, between
                // two) is swept like the top run -- two loads per layer under the compiler's counted waits, no mask test, no
                // dispatch -- by BODY_CLEAR, which keeps S_EO (a layer above was delta-scaled, so S_EO is not S_XU).
                // e: one past the run that starts at layer i (scalar bit operations on the mask), the last layer left out.
                const unsigned long long w = i < 64 ? (m0 >> i) | (i ? m1 << (64 - i) : 0ull) : m1 >> (i - 64);
                int e = i + ((~w) ? __builtin_ctzll(~w) : 64);
                e = e < n - 1 ? e : n - 1;
                if (i + 2 < e) {
                    // as in the top run: layers i .. i + 2 belong to the run, B holds layer i on the way in and out
                    for (; i + 2 < e; i += 2) {
                        load_clear(A, i + 1);
                        PZ_RUN_LAYER(BODY_CLEAR, B);
                        load_clear(B, i + 2);
                        PZ_RUN_LAYER(BODY_CLEAR, A);
                    }
                    if (!(i + 2 <= n - 1)) break;
                }
            }
            load(A, i + 1, true);
            PZ_LAYER(false, false, B, i);
            load(B, i + 2, true);
            PZ_LAYER(false, false, A, i + 1);
        }
        if (i == n - 1) {
            PZ_LAYER(false, true, B, i);
        } else {                                 // i == n - 2
            load(A, i + 1, true);
            PZ_LAYER(false, false, B, i);
            PZ_LAYER(false, true, A, i + 1);
        }
    } else {
        load(B, 1);                              // B: prefetch set, A: the layer being computed
        PZ_LAYER(true, false, A, 0);
        for (int i = 1; i < n - 1; ++i) {
            A = B;
            load(B, i + 1);
            PZ_LAYER(false, false, A, i);
        }
        A = B;
        PZ_LAYER(false, true, A, n - 1);
    }
#undef PZ_LAYER
#undef PZ_RUN_LAYER
#undef PZ_CLOUD_LAYER
#undef PZ_BODY

    // ---- surface row (fluxes.py:178-183) and output ----
    // EP(1 - rs G) pos + EM(G - rs) neg = b_surface - c+dn + rs c-dn with neg = delta - rho pos,
    // divided through by EP:  pos = EM (b_surface - D1 + rs D2) / ((1 - rs G) - EM^2 (G - rs) rho)
    // disk sum in the reference's order (one running sum over all angles): a later chunk of a launch
    // split over angles continues from the stored partial sum
    double alb = (!IS3D && a.albedo && !a.albedo_first) ? a.albedo[w] : 0.0;
    double xout[NA];
    {
#pragma clang fp contract(off)
        const double em2 = S.pEM * S.pEM;
        const double bden = 1.0 / fma(-(em2 * (S.pgam - rs)), S.rho, fma(-rs, S.pgam, 1.0));
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            const double b_surface = ((rs * (ZP ? g[k].u1 : g[k].u0)) * F) * S.get(S_XU, k);
            const double pos = (S.pEM * fma(rs, S.get(S_D2, k), b_surface - S.get(S_D1, k))) * bden;
            xout[k] = fma(S.get(S_ZETA, k), pos, S.get(S_KAPPA, k));
        }
    }
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        const double x = xout[k];
        if (IS3D) a.xint[(long)fac * a.nwno + w] = x;
        else if (NA == 1 || (int)by * NA + k < a.nvalid) a.xint[(long)(by * NA + k) * a.ncol + col] = x;
        alb = disk_accumulate(alb, x, g[k].wgt, g[k].wgt2);
    }
    if (!IS3D && a.albedo) {                              // fused disco.compress_disco (disco.py:145-148)
        double acc = alb;
        if (a.albedo_last) acc = disk_finish(a.albedo_scale, acc, F, a.cos_theta);
        a.albedo[w] = acc;
    }
}

// Workgroup b of a 1-D grid of `nrep` replicas (angle groups, or spectra that share their planes) of `ncg` column
// groups -> (replica, column group) in XCD-aware order, see the comment in k_reflected_toa.
__device__ __forceinline__ void xcd_decode(unsigned b, unsigned nrep, unsigned ncg, unsigned &rep, unsigned &cg)
{
    const unsigned nfull = ncg & ~7u;
    if (b < nfull * nrep) {
        const unsigned per = 8u * nrep, chunk = b / per, rem = b - chunk * per;
        rep = rem >> 3;
        cg = chunk * 8u + (rem & 7u);
    } else {
        const unsigned idx = b - nfull * nrep, left = ncg - nfull;
        rep = idx / left;
        cg = nfull + (idx - rep * left);
    }
}

template <int NA, bool IS3D, bool ZP, bool FAST = false, bool BIG = false, int DRV = 0>
__global__ __launch_bounds__(PZ_REFL_BLOCK, (BIG ? 1 : PZ_REFL_MINWAVES)) void k_reflected_toa(const ReflectedArgs a)
{
    // Angle groups as separate workgroups (ny > 1): every group re-reads the eleven planes of its columns.
    // Consecutive workgroups go to consecutive XCDs (8, each with its own L2), so the launch is 1-D and, for
    // the column groups that fill whole chunks of 8, block b = (chunk, angle group, column group within the
    // chunk): the ny workgroups of one column group are dispatched 8 apart, all to XCD (column group % 8),
    // and all but the first find the planes in that L2.  The last ncg % 8 column groups go out in plain
    // (angle group, column group) order, which spreads their workgroups over the XCDs -- sending them after
    // their chunk would put up to 8 x ny more workgroups on the first XCDs than on the others (12 500
    // columns, one angle per wave: 35 on XCD 0 of 32 CUs, 0.078 ms instead of 0.050).  A 2-D (x, y) grid
    // shares L2 only when the column-group count happens to be a multiple of 8 (12 250 columns 0.050 ms,
    // 12 000 0.069, 12 500 0.072: round-2 sweep).
    unsigned bx = blockIdx.x, by = 0;
    if (!IS3D && a.ny > 1) xcd_decode(blockIdx.x, (unsigned)a.ny, (unsigned)a.ncg, by, bx);
    reflected_toa_body<NA, IS3D, ZP, FAST, BIG, DRV>(a, bx, by, a.ang);
}

// The same body for `nspec` spectra in one grid (picaso_get_reflected_1d_batch_dev): the workgroup finds its
// spectrum's planes, outputs and angle table in the device table a.batch.  A separate instantiation so that the
// single-spectrum kernels keep their register allocation; same operations, same bits.
template <int NA, bool IS3D, bool ZP, bool FAST = false, bool BIG = false, int DRV = 0>
__global__ __launch_bounds__(PZ_REFL_BLOCK, (BIG ? 1 : PZ_REFL_MINWAVES)) void k_reflected_toa_batch(const ReflectedArgs a)
{
    unsigned spec, bx, by = 0;
    const unsigned ny = a.ny > 1 ? (unsigned)a.ny : 1u;
    if (!IS3D && a.batch_interleave) {          // shared planes: (spectrum, angle group) replicas of a column group on one XCD
        unsigned rep;
        xcd_decode(blockIdx.x, ny * (unsigned)a.nspec, (unsigned)a.ncg, rep, bx);
        spec = rep / ny;
        by = rep - spec * ny;
    } else {
        spec = blockIdx.x / a.bps;
        bx = blockIdx.x - spec * a.bps;
        if (!IS3D && ny > 1) xcd_decode(bx, ny, (unsigned)a.ncg, by, bx);
    }
    // The table is read through the constant address space (it is written before the launch and never by it):
    // its entries then behave like kernel arguments -- scalar loads the compiler may repeat instead of keeping
    // ~60 angle constants alive through the layer loop (as plain global loads they ended up in VGPRs: 98 spilled).
    typedef const __attribute__((address_space(4))) ReflBatchItem *ItemPtr;
    const auto &it = *((ItemPtr)(unsigned long)a.batch + spec);
    ReflectedArgs b = a;
    b.dtau = it.dtau; b.tau = it.tau; b.w0 = it.w0; b.cosb = it.cosb; b.gcos2 = it.gcos2; b.ftau_cld = it.ftau_cld;
    b.ftau_ray = it.ftau_ray; b.dtau_og = it.dtau_og; b.tau_og = it.tau_og; b.w0_og = it.w0_og; b.cosb_og = it.cosb_og;
    b.surf_reflect = it.surf_reflect; b.F0PI = it.F0PI; b.xint = it.xint; b.albedo = it.albedo;
    b.cos_theta = it.cos_theta;
    b.u0_tab = it.u0_tab; b.u1_tab = it.u1_tab;
    if constexpr (DRV == 4) {
        b.lmask[0] = it.lmask[0]; b.lmask[1] = it.lmask[1];
        b.cmask[0] = it.cmask[0]; b.cmask[1] = it.cmask[1];
    }
    reflected_toa_body<NA, IS3D, ZP, FAST, BIG, DRV>(b, bx, by, it.ang);
}

// the reference's default options (see reflected_layer); zp: the symmetric zero-phase geometry, where the
// compile-time variant also fixes cos_theta = 1 -- at other phase angles (ubar0 != ubar1) cos_theta stays an argument
static bool fast_options(const ReflectedArgs &a, bool zp)
{
    if (getenv("PICASO_AMD_REFL_GENERIC")) return false;      // A/B switch for tools/
    if ((double)a.pitch * (a.nlayer + 1) * 8.0 >= 4294967296.0) return false;   // 32-bit plane offsets
    // (a batched launch: a.cos_theta = 1 only if every spectrum's is)
    return a.toon_coefficients == 0 && a.single_phase == 3 && a.multi_phase == 0 && (!zp || a.cos_theta == 1.0) &&
           a.frac_c == 2.0;
}

// Launches one kernel of the family: its batched form when the arguments carry a batch table, else the single-spectrum one.
template <int NA, bool IS3D, bool ZP, bool FAST = false, bool BIG = false, int DRV = 0>
static void launch_kernel(picaso_ctx *ctx, const dim3 grid, const ReflectedArgs &a)
{
    if (a.batch)
        hipLaunchKernelGGL((k_reflected_toa_batch<NA, IS3D, ZP, FAST, BIG, DRV>), grid, dim3(PZ_REFL_BLOCK), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL((k_reflected_toa<NA, IS3D, ZP, FAST, BIG, DRV>), grid, dim3(PZ_REFL_BLOCK), 0, ctx->stream, a);
}

template <int NA>
static int launch1d(picaso_ctx *ctx, const ReflectedArgs &a_in)
{
    ReflectedArgs a = a_in;
    if (a.nvalid <= 0) a.nvalid = NA * (a.ny > 1 ? a.ny : 1);     // no padded angle slots
    const int block = PZ_REFL_BLOCK;
    const unsigned ncg = (unsigned)((a.ncol + block - 1) / block), ny = (unsigned)(a.ny > 1 ? a.ny : 1);
    const unsigned nspec = a.batch ? (unsigned)a.nspec : 1u;
    a.ncg = (int)ncg;
    a.bps = ncg * ny;
    const dim3 grid(ncg * ny * nspec);              // ny > 1: 1-D, in the XCD-aware order of the kernel
    bool zp = a.batch ? a.batch_zp != 0 : true;     // batch: the angle tables are on the device; the caller looked
    if (!a.batch)
        for (int k = 0; k < a.na * (int)ny; ++k) zp = zp && (a.ang[k].u0 == a.ang[k].u1);
    bool big = false;
    if constexpr (NA == 5)
        big = a.ny <= 1 && (long)nspec * ncg * (block / 64) <= 1024 && getenv("PICASO_AMD_REFL_NO_BIG") == nullptr;
    bool fast = fast_options(a, zp);
    // planes left out (re-derived in the kernel): the default-options kernels only -- reflected_1d_can_derive() is the
    // caller's way to know
    const bool drv = !(a.tau && a.tau_og && a.gcos2 && a.ftau_cld && a.dtau_og);
    if (drv) {
        // reflected_1d_can_derive() looked at ALL angles of the call; this launch may be a chunk of them whose angles
        // all happen to have ubar0 == ubar1 at a phase angle other than zero: not the zero-phase variant's geometry
        // (it fixes cos_theta = 1), but the general default-options kernel takes it -- same bits
        if (!fast && zp && a.cos_theta != 1.0) {
            zp = false;
            fast = fast_options(a, zp);
        }
        if (!fast) return fail(ctx, "reflected: planes may be left out only with the reference's default options");
        // only dtau and w0: the compile-time form (five angles, symmetric geometry: the shape of a spectrum() call)
        const bool only2 = !a.tau && !a.tau_og && !a.gcos2 && !a.ftau_cld && !a.dtau_og;
        const bool levels3 = !a.tau && !a.tau_og && !a.gcos2 && a.ftau_cld && a.dtau_og;
        // the seal's clear-layer mask (api.hip asks for it): the fused five-angle shape only, never the BIG form
        const bool layers4 = levels3 && a.use_lmask;
        if (zp && big) { if constexpr (NA == 5) launch_kernel<NA, false, true, true, true, 1>(ctx, grid, a); }
        else if (zp && layers4 && NA == 5) { if constexpr (NA == 5) launch_kernel<NA, false, true, true, false, 4>(ctx, grid, a); }
        else if (zp && only2 && NA == 5) { if constexpr (NA == 5) launch_kernel<NA, false, true, true, false, 2>(ctx, grid, a); }
        else if (zp && levels3 && NA == 5) { if constexpr (NA == 5) launch_kernel<NA, false, true, true, false, 3>(ctx, grid, a); }
        else if (zp) launch_kernel<NA, false, true, true, false, 1>(ctx, grid, a);
        else launch_kernel<NA, false, false, true, false, 1>(ctx, grid, a);
        PZ_HIP(ctx, hipGetLastError());
        return 0;
    }
    if (zp && fast && big) { if constexpr (NA == 5) launch_kernel<NA, false, true, true, true>(ctx, grid, a); }
    else if (zp && fast) launch_kernel<NA, false, true, true>(ctx, grid, a);
    else if (fast) launch_kernel<NA, false, false, true>(ctx, grid, a);        // default options at a non-zero phase angle
    else if (zp) launch_kernel<NA, false, true>(ctx, grid, a);
    else launch_kernel<NA, false, false>(ctx, grid, a);
    PZ_HIP(ctx, hipGetLastError());
    return 0;
}

int launch_reflected_toa(picaso_ctx *ctx, const ReflectedArgs &a, bool is3d)
{
    if (a.ncol <= 0 || a.nlayer < 1) return fail(ctx, "reflected: empty problem");
    if (is3d) {
        // 3-D: the reference's default options (TTHG_ray, N = 2, frac_c = 2; 3-D is quadrature-only anyway) fixed at compile
        // time like the 1-D launches, and with them the two plane patterns of the product known at compile time as well --
        // only dtau and w0 (a map without cloud), or everything but tau / tau_og / gcos2 (cloud tables): same bits as the
        // generic instantiations (PICASO_AMD_REFL3D_GENERIC=1), which every other option set and plane pattern keeps.
        // A batch: a.tau etc. are the presence pattern of EVERY spectrum's planes.
        const bool all3 = a.tau && a.tau_og && a.gcos2 && a.ftau_cld && a.dtau_og;
        const bool fast3 = a.single_phase == 3 && a.multi_phase == 0 && a.frac_c == 2.0 &&
                           (double)a.pitch * (a.nlayer + 1) * 8.0 < 4294967296.0 && !getenv("PICASO_AMD_REFL3D_GENERIC");
        const bool only2_3 = !a.tau && !a.tau_og && !a.gcos2 && !a.ftau_cld && !a.dtau_og;
        const bool levels3_3 = !a.tau && !a.tau_og && !a.gcos2 && a.ftau_cld && a.dtau_og;
        ReflectedArgs b = a;                        // (the single-spectrum kernels read neither of the two)
        b.bps = (unsigned)((a.ncol + PZ_REFL_BLOCK - 1) / PZ_REFL_BLOCK);
        b.batch_interleave = 0;
        const dim3 grid(b.bps * (a.batch ? (unsigned)a.nspec : 1u));
        if (fast3 && all3) launch_kernel<1, true, false, true, false, 0>(ctx, grid, b);
        else if (fast3 && only2_3) launch_kernel<1, true, false, true, false, 2>(ctx, grid, b);
        else if (fast3 && levels3_3) launch_kernel<1, true, false, true, false, 3>(ctx, grid, b);
        else if (fast3) launch_kernel<1, true, false, true, false, 1>(ctx, grid, b);
        else if (all3) launch_kernel<1, true, false>(ctx, grid, b);
        else launch_kernel<1, true, false, false, false, 1>(ctx, grid, b);
        PZ_HIP(ctx, hipGetLastError());
        return 0;
    }
    switch (a.na) {
        case 1: return launch1d<1>(ctx, a);
        case 2: return launch1d<2>(ctx, a);
        case 3: return launch1d<3>(ctx, a);
        case 4: return launch1d<4>(ctx, a);
        case 5: return launch1d<5>(ctx, a);
        case 6: return launch1d<6>(ctx, a);
        case 7: return launch1d<7>(ctx, a);
        case 8: return launch1d<8>(ctx, a);
    }
    return fail(ctx, "reflected: unsupported angle chunk %d", a.na);
}

}  // namespace pz
