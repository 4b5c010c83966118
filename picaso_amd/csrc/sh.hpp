// Spherical-harmonics (SH2 / SH4) reflected light and thermal emission: what the kernel families and the C entry
// points share -- the kernel-argument structs, the launchers and the host's angle tables.
//   sh_sweep.hip    sh_body / k_sh / k_sh_refl: the general sweep, one wave per angle
//   sh_thermal.hip  k_sh_thermal: thermal emission, the angle-independent algebra shared between the angles of a lane
//   sh_clear.hip    k_sh4_clear: SH4 reflected light on cloud-free layers, shared likewise
//   sh.hip          the extern "C" entries
#pragma once

#include "common.hpp"
#include "device_math.hpp"

namespace pz {

constexpr int SH_MAX_ANG = 16;                    // angles per launch (the angle table is a kernel argument)

struct SHArgs {
    int nlayer, nwno, stream;
    long pitch;
    const double *dtau, *tau, *w0, *ftau_cld, *ftau_ray, *f_deltaM, *dtau_og, *tau_og, *w0_og, *cosb_og;
    const double *surf_reflect, *F0PI;
    // angles of this launch chunk; constants derived on the host (wave-uniform -> SGPR)
    struct Angle {
        double u0, u1, iu0, iu1, mus, imus, nl0, nl1, nlm;   // nl* = -log2(e) {1/u0, 1/u1, mus}
    } ang[SH_MAX_ANG];
    int first_angle, compound, nang;                         // reference angle index of ang[0]; angles of this launch
    int xcd_order;                                           // block order, see k_sh
    unsigned ncg;                                            // column groups (blocks per angle)
    double cos_theta;
    int w_single_form, w_multi_form, psingle_form, w_single_rayleigh, w_multi_rayleigh,
        psingle_rayleigh, single_form;
    double frac_a, frac_b, frac_c, constant_back, constant_forward, b_top;
    // thermal
    const double *wno, *tlevel, *plevel;     // device (nwno) / (nlevel) / (nlevel)
    int hard_surface, use_ff;                // use_ff: cosb != cosb_og somewhere (fluxes.py:3072-3075)
    double *xint;                            // (angles of this launch, nwno)
    // flx = 1 (reflected): layer moment fluxes F.X + G (calculate_flux, fluxes.py:3631-3635)
    double *flux;                            // (angles of this launch, stream*nlevel, nwno)
    double *scratch;                         // (angles, 4 NB^2 + 5 NB, nlayer, nwno) sweep-1 state
    // batched launch (picaso_get_reflected_SH_batch_dev): blockIdx.y = spectrum, see ReflectedArgs::batch
    const struct SHBatchItem *batch;
    int nspec_;
    // resume below a cloud-free top (picaso_get_reflected_SH_top_dev): the sweep state k_sh4_clear left at the top of
    // layer `start_layer`, [slot][nwno] (SHC_SHARED shared slots, then SHC_STATE per angle of the call)
    int start_layer;
    const double *state;
};
constexpr int SHC_SHARED = 20, SHC_STATE = 11;
struct SHBatchItem {
    const double *dtau, *tau, *w0, *ftau_cld, *ftau_ray, *f_deltaM, *dtau_og, *tau_og, *w0_og, *cosb_og;
    const double *surf_reflect, *F0PI;
    double *xint;
    double cos_theta;
    SHArgs::Angle ang[SH_MAX_ANG];
};

struct SHTArgs {                                    // k_sh_thermal
    int nlayer, nwno;
    long pitch;
    const double *dtau, *w0, *cosb_og, *surf_reflect, *wno, *tlevel, *plevel;
    int hard_surface, use_ff;
    int na;                                         // angles of this launch: blockIdx.y = chunk of NA of them
    struct Angle { double u1, iu1, nl1, p1, p2, p3; } ang[SH_MAX_ANG];
    double *xint;                                   // first angle of this launch, (na, nwno)
};

struct SHCArgs {                                    // k_sh4_clear
    int nlayer, nwno;
    long pitch;
    const double *dtau, *w0, *surf_reflect, *F0PI;
    int na;                                         // angles of this launch: blockIdx.y = chunk of NA of them
    struct Angle {
        double u0, iu0, iu1, mus, imus, nl0, nl1, nlm;   // as SHArgs::Angle
        double x2, x4;                              // (1/u0)^2, (1/u0)^4
        double p2u0, hp2u1;                         // P_2(-u0); P_2(u1) / 2
        int sym;                                    // u0 == u1
    } ang[SH_MAX_ANG];
    double psing;                                   // Rayleigh single scattering 0.75 (1 + cos_theta^2), :2846
    double b_top;
    double *xint;                                   // first angle of this launch, (na, nwno)
    // a cloud-free TOP only (picaso_get_reflected_SH_top_dev): sweep the first `nstop` layers and leave the state for
    // k_sh (SHArgs::state) instead of closing the column with the surface rows
    int nstop, first_angle;
    double *state;
};
constexpr int SHC_MAX_PER_LANE = 2;               // angles per lane of k_sh4_clear, measured (sh_clear.hip)
constexpr int SH_TOP_MIN = 4;     // cloud-free layers from which the split (two launches, a state hand-over) is taken

// sh_sweep.hip: every angle of the call through k_sh / k_sh_refl, SH_MAX_ANG per launch; one launch of a filled SHArgs
// (the batch entry); the PICASO_AMD_SH_CHECK_TOP check of the first `top` layers
int launch_sh_angles(picaso_ctx *ctx, SHArgs &a, int nang, const double *ubar0, const double *ubar1,
                     double *xint_at_top, double *flux, bool thermal);
int launch_sh(picaso_ctx *ctx, SHArgs &a, int nang, bool thermal);
int sh_check_top(picaso_ctx *ctx, const SHArgs &a, int top);
// sh_thermal.hip, sh_clear.hip: every angle of the call, several per lane
int launch_sh_thermal(picaso_ctx *ctx, SHTArgs &a, int stream, int nang, const double *ubar1, double *xint);
int launch_sh4_clear(picaso_ctx *ctx, SHCArgs &a, int nang, const double *ubar0, const double *ubar1, double *xint);

inline SHArgs::Angle make_sh_angle(double u0, double u1, bool thermal)
{
    SHArgs::Angle g;
    g.u1 = u1;
    g.iu1 = 1.0 / g.u1;
    g.nl1 = -LOG2E_D * g.iu1;
    if (thermal) {
        g.u0 = g.iu0 = g.mus = g.imus = g.nl0 = g.nlm = 0.0;
    } else {
        g.u0 = u0;
        g.iu0 = 1.0 / g.u0;
        g.mus = (g.u1 + g.u0) / (g.u1 * g.u0);                       // fluxes.py:2899
        g.imus = 1.0 / g.mus;
        g.nl0 = -LOG2E_D * g.iu0;
        g.nlm = -LOG2E_D * g.mus;
    }
    return g;
}

// Angles per lane for a launch of `ncol` columns and `nang` angles: the split into ceil(nang / m) nearly equal
// chunks with the smallest modelled time.  Per wave and layer: S shared + m A per-angle instructions (400 / 110,
// counted from the source for SH4); one wave alone on its SIMD issues an fp64 instruction every ~5.5 cycles, two
// or more share the 4 cycles of the pipe, and a launch whose waves are not a multiple of the 2 x SIMD slots pays
// for the partly filled last round.
inline int sh_angles_per_lane(const picaso_ctx *ctx, long ncol, int nang, double S, double A, const char *env,
                              int max_per_lane)
{
    if (const char *e = getenv(env)) {
        const int m = atoi(e);
        if (m >= 1 && m <= max_per_lane) return m;
    }
    const long simds = 4L * ctx->ncu, groups = (ncol + 63) / 64;
    int best = 1;
    double best_t = 1e300;
    for (int m = 1; m <= max_per_lane; ++m) {
        const int nchunk = (nang + m - 1) / m;
        const long waves = groups * nchunk;
        const double per_wave = S + A * ((double)nang / nchunk);      // mean chunk
        const double longest = S + A * ((nang + nchunk - 1) / nchunk);
        const long full = waves / (2 * simds), rem = waves - full * 2 * simds;
        const double t = full * 8.0 * per_wave + (rem == 0 ? 0.0 : rem <= simds ? 5.5 * (full ? per_wave : longest)
                                                                                    : 8.0 * per_wave);
        if (t < best_t) { best_t = t; best = m; }
    }
    return best;
}

// The launches of an angle-sharing kernel: sh_angles_per_lane angles per lane in nearly equal chunks (the last one
// short), whole chunks per launch, at most SH_MAX_ANG angles per launch.  launch(done, na, per_lane, chunks) fills the
// angle table for the call's angles done .. done + na - 1 and launches them as `chunks` chunks (grid.y) of per_lane.
template <typename Launch>
int sh_launch_chunks(picaso_ctx *ctx, long ncol, int nang, double S, double A, const char *env, int max_per_lane,
                     Launch launch)
{
    const int m = sh_angles_per_lane(ctx, ncol, nang, S, A, env, max_per_lane);
    const int nchunk = (nang + m - 1) / m;
    const int per_lane = (nang + nchunk - 1) / nchunk;
    const int per_launch = (SH_MAX_ANG / per_lane) * per_lane;
    for (int done = 0; done < nang; done += per_launch) {
        const int na = (nang - done < per_launch) ? nang - done : per_launch;
        launch(done, na, per_lane, (na + per_lane - 1) / per_lane);
        PZ_HIP(ctx, hipGetLastError());
    }
    return 0;
}

}  // namespace pz
