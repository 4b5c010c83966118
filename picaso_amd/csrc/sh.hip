// Spherical-harmonics (SH2 / SH4) reflected light and thermal emission: the extern "C" entries.  The kernels and their
// launchers are in sh_sweep.hip, sh_thermal.hip and sh_clear.hip (see sh.hpp).
#include "sh.hpp"

#pragma clang fp contract(fast)   // host code only; the one sum of a product whose rounding matters (psing) says so itself

using namespace pz;

// The plane and option fields of SHArgs, as every reflected launch sets them.
static SHArgs reflected_sh_args(int nlevel, int nwno, long plane_pitch, int stream, const double *dtau,
                                const double *tau, const double *w0, const double *ftau_cld, const double *ftau_ray,
                                const double *f_deltaM, const double *dtau_og, const double *tau_og,
                                const double *w0_og, const double *cosb_og, const double *surf_reflect,
                                const double *F0PI, double cos_theta, int w_single_form, int w_multi_form,
                                int psingle_form, int w_single_rayleigh, int w_multi_rayleigh, int psingle_rayleigh,
                                double frac_a, double frac_b, double frac_c, double constant_back,
                                double constant_forward, double b_top, int single_form, int compound_f_deltaM)
{
    SHArgs a{};
    a.nlayer = nlevel - 1; a.nwno = nwno; a.stream = stream; a.pitch = plane_pitch;
    a.dtau = dtau; a.tau = tau; a.w0 = w0; a.ftau_cld = ftau_cld; a.ftau_ray = ftau_ray;
    a.f_deltaM = f_deltaM; a.dtau_og = dtau_og; a.tau_og = tau_og; a.w0_og = w0_og; a.cosb_og = cosb_og;
    a.surf_reflect = surf_reflect; a.F0PI = F0PI; a.cos_theta = cos_theta;
    a.w_single_form = w_single_form; a.w_multi_form = w_multi_form; a.psingle_form = psingle_form;
    a.w_single_rayleigh = w_single_rayleigh; a.w_multi_rayleigh = w_multi_rayleigh;
    a.psingle_rayleigh = psingle_rayleigh; a.single_form = single_form;
    a.frac_a = frac_a; a.frac_b = frac_b; a.frac_c = frac_c; a.constant_back = constant_back;
    a.constant_forward = constant_forward; a.b_top = b_top;
    a.compound = compound_f_deltaM ? 1 : 0;
    return a;
}

// The arguments of k_sh4_clear that do not depend on the launch.
static SHCArgs clear_sh_args(int nlevel, int nwno, long plane_pitch, const double *dtau, const double *w0,
                             const double *surf_reflect, const double *F0PI, double cos_theta, double b_top)
{
    SHCArgs c{};
    c.nlayer = nlevel - 1; c.nwno = nwno; c.pitch = plane_pitch;
    c.dtau = dtau; c.w0 = w0; c.surf_reflect = surf_reflect; c.F0PI = F0PI;
    {
#pragma clang fp contract(off)
        c.psing = 0.75 * (1 + cos_theta * cos_theta);
    }
    c.b_top = b_top;
    return c;
}

extern "C" {

int picaso_reflected_SH_can_derive(int stream, int w_single_form, int w_multi_form, int psingle_form,
                                   int w_single_rayleigh, int w_multi_rayleigh, int psingle_rayleigh, double frac_c,
                                   int single_form, int flx)
{
    if (getenv("PICASO_AMD_SH_NO_CLEAR")) return 0;
    return stream == 4 && !flx && w_single_form == 0 && w_multi_form == 0 && psingle_form == 0 && single_form == 0 &&
           w_single_rayleigh == 1 && w_multi_rayleigh == 1 && psingle_rayleigh == 1 && frac_c == 2.0;
}

int picaso_reflected_SH_can_derive_levels(int nlevel, long plane_pitch, int stream, int w_single_form, int w_multi_form,
                                          int psingle_form, int w_single_rayleigh, int w_multi_rayleigh,
                                          int psingle_rayleigh, double frac_c, int single_form, int flx)
{
    if (getenv("PICASO_AMD_SH_GENERIC") || getenv("PICASO_AMD_SH_ALL_PLANES")) return 0;
    return (stream == 2 || stream == 4) && !flx && w_single_form == 0 && w_multi_form == 0 && psingle_form == 0 &&
           single_form == 0 && w_single_rayleigh == 1 && w_multi_rayleigh == 1 && psingle_rayleigh == 1 && frac_c == 2.0 &&
           nlevel >= 2 && (double)plane_pitch * nlevel * 8.0 < 4294967296.0;
}

int picaso_get_reflected_SH_dev(picaso_ctx *ctx, int nlevel, int nwno, long plane_pitch, int numg, int numt,
                                const double *dtau, const double *tau, const double *w0,
                                const double *cosb, const double *ftau_cld, const double *ftau_ray,
                                const double *f_deltaM, const double *dtau_og, const double *tau_og,
                                const double *w0_og, const double *cosb_og, const double *surf_reflect,
                                const double *ubar0, const double *ubar1, double cos_theta,
                                const double *F0PI, int w_single_form, int w_multi_form,
                                int psingle_form, int w_single_rayleigh, int w_multi_rayleigh,
                                int psingle_rayleigh, double frac_a, double frac_b, double frac_c,
                                double constant_back, double constant_forward, int stream,
                                double b_top, int flx, int single_form, int compound_f_deltaM,
                                double *xint_at_top, double *flux, const double *gweight,
                                const double *tweight, double *albedo)
{
    return picaso_get_reflected_SH_top_dev(ctx, nlevel, nwno, plane_pitch, numg, numt, dtau, tau, w0, cosb, ftau_cld,
                                           ftau_ray, f_deltaM, dtau_og, tau_og, w0_og, cosb_og, surf_reflect, ubar0, ubar1,
                                           cos_theta, F0PI, w_single_form, w_multi_form, psingle_form, w_single_rayleigh,
                                           w_multi_rayleigh, psingle_rayleigh, frac_a, frac_b, frac_c, constant_back,
                                           constant_forward, stream, b_top, flx, single_form, compound_f_deltaM, 0,
                                           xint_at_top, flux, gweight, tweight, albedo);
}

int picaso_get_reflected_SH_top_dev(picaso_ctx *ctx, int nlevel, int nwno, long plane_pitch, int numg, int numt,
                                    const double *dtau, const double *tau, const double *w0,
                                    const double *cosb, const double *ftau_cld, const double *ftau_ray,
                                    const double *f_deltaM, const double *dtau_og, const double *tau_og,
                                    const double *w0_og, const double *cosb_og, const double *surf_reflect,
                                    const double *ubar0, const double *ubar1, double cos_theta,
                                    const double *F0PI, int w_single_form, int w_multi_form,
                                    int psingle_form, int w_single_rayleigh, int w_multi_rayleigh,
                                    int psingle_rayleigh, double frac_a, double frac_b, double frac_c,
                                    double constant_back, double constant_forward, int stream,
                                    double b_top, int flx, int single_form, int compound_f_deltaM,
                                    int cloud_free_above, double *xint_at_top, double *flux, const double *gweight,
                                    const double *tweight, double *albedo)
{
    if (!ctx) return fail(nullptr, "null context");
    if (nlevel < 2 || nwno < 1 || numg < 1 || numt < 1) return fail(ctx, "get_reflected_SH: bad sizes");
    if (stream != 2 && stream != 4) return fail(ctx, "get_reflected_SH: stream must be 2 or 4, got %d", stream);
    if (flx && !flux) return fail(ctx, "get_reflected_SH: flx=1 needs the flux output (numg,numt,stream*nlevel,nwno)");
    PZ_NEED(ctx, "get_reflected_SH", surf_reflect, ubar0, ubar1, F0PI, xint_at_top);
    if (flx && plane_pitch != nwno) return fail(ctx, "get_reflected_SH: flx=1 needs contiguous planes");
    if (plane_pitch < nwno) return fail(ctx, "get_reflected_SH: plane_pitch < nwno");
    if (!dtau || !w0) return fail(ctx, "get_reflected_SH: dtau and w0 are required");
    PZ_HIP(ctx, hipSetDevice(ctx->device));
    (void)cosb;                                                           // never read (fluxes.py:2675-2976)
    const double *const derivable[8] = {tau, ftau_cld, ftau_ray, f_deltaM, dtau_og, tau_og, w0_og, cosb_og};
    int nnull = 0;
    for (int j = 0; j < 8; ++j) nnull += derivable[j] ? 0 : 1;
    // only the two level planes left out: the running-product form of the beam exponentials (k_sh<.., DRVT>)
    const bool levels_only = (nnull == 2 && !tau && !tau_og);
    if (levels_only &&
        !picaso_reflected_SH_can_derive_levels(nlevel, plane_pitch, stream, w_single_form, w_multi_form, psingle_form,
                                               w_single_rayleigh, w_multi_rayleigh, psingle_rayleigh, frac_c, single_form, flx))
        return fail(ctx, "get_reflected_SH: tau and tau_og may be left out only with the reference's default phase-function "
                         "options, flx = 0 and planes below 4 GB (picaso_reflected_SH_can_derive_levels); pass them");
    const int nang = numg * numt;
    SHCArgs c = clear_sh_args(nlevel, nwno, plane_pitch, dtau, w0, surf_reflect, F0PI, cos_theta, b_top);
    if (nnull && !levels_only) {
        // cloud-free form: dtau and w0 only, everything else known (k_sh4_clear)
        if (nnull != 8)
            return fail(ctx, "get_reflected_SH: leave out all of tau, cosb, ftau_cld, ftau_ray, f_deltaM, dtau_og, tau_og, "
                             "w0_og, cosb_og (a cloud-free column: they are constants, copies and running sums) or none");
        if (!picaso_reflected_SH_can_derive(stream, w_single_form, w_multi_form, psingle_form, w_single_rayleigh,
                                            w_multi_rayleigh, psingle_rayleigh, frac_c, single_form, flx))
            return fail(ctx, "get_reflected_SH: the cloud-free form (dtau and w0 only) is built for stream 4, the default "
                             "phase-function options and flx = 0; pass all eleven planes");
        PZ_TRY(launch_sh4_clear(ctx, c, nang, ubar0, ubar1, xint_at_top));
        if (albedo && gweight && tweight)
            PZ_TRY(picaso_compress_disco_dev(ctx, nwno, cos_theta, xint_at_top, gweight, numg, tweight, numt, F0PI, albedo));
        return 0;
    }
    if (cloud_free_above < 0) return fail(ctx, "get_reflected_SH: cloud_free_above must be >= 0, got %d", cloud_free_above);
    SHArgs a = reflected_sh_args(nlevel, nwno, plane_pitch, stream, dtau, tau, w0, ftau_cld, ftau_ray, f_deltaM, dtau_og,
                                 tau_og, w0_og, cosb_og, surf_reflect, F0PI, cos_theta, w_single_form, w_multi_form,
                                 psingle_form, w_single_rayleigh, w_multi_rayleigh, psingle_rayleigh, frac_a, frac_b,
                                 frac_c, constant_back, constant_forward, b_top, single_form, compound_f_deltaM);
    // A cloud-free top (the caller's statement: no cloud in layers 0 .. cloud_free_above - 1 of any column): those
    // layers go through k_sh4_clear, two angles per lane sharing the angle-independent half, which leaves the sweep
    // state at the top of the first cloudy layer for k_sh to continue from.  Worth a second launch from a few layers on.
    const int nlayer = nlevel - 1;
    const int top = cloud_free_above > nlayer ? nlayer : cloud_free_above;
    if (top >= SH_TOP_MIN && !getenv("PICASO_AMD_SH_NO_TOP") &&
        picaso_reflected_SH_can_derive(stream, w_single_form, w_multi_form, psingle_form, w_single_rayleigh,
                                       w_multi_rayleigh, psingle_rayleigh, frac_c, single_form, flx)) {
        if (getenv("PICASO_AMD_SH_CHECK_TOP")) PZ_TRY(sh_check_top(ctx, a, top));
        if (top < nlayer) {
            PZ_TRY(ck_scratch_reserve(ctx, sizeof(double) * (size_t)(SHC_SHARED + SHC_STATE * nang) * nwno));
            c.nstop = top;
            c.state = ctx->ck_scratch;
            a.start_layer = top;
            a.state = ctx->ck_scratch;
        }
        PZ_TRY(launch_sh4_clear(ctx, c, nang, ubar0, ubar1, xint_at_top));
        if (top < nlayer) PZ_TRY(launch_sh_angles(ctx, a, nang, ubar0, ubar1, xint_at_top, nullptr, false));
    } else {
        PZ_TRY(launch_sh_angles(ctx, a, nang, ubar0, ubar1, xint_at_top, flx ? flux : nullptr, false));
    }
    if (albedo && gweight && tweight)
        PZ_TRY(picaso_compress_disco_dev(ctx, nwno, cos_theta, xint_at_top, gweight, numg, tweight, numt, F0PI, albedo));
    return 0;
}

int picaso_get_reflected_SH_batch_dev(picaso_ctx *ctx, int nspec, int nlevel, int nwno, long plane_pitch, int numg,
                                      int numt, const double *const *dtau, const double *const *tau,
                                      const double *const *w0, const double *const *cosb,
                                      const double *const *ftau_cld, const double *const *ftau_ray,
                                      const double *const *f_deltaM, const double *const *dtau_og,
                                      const double *const *tau_og, const double *const *w0_og,
                                      const double *const *cosb_og, const double *const *surf_reflect, int ngeom,
                                      const double *ubar0, const double *ubar1, const double *cos_theta,
                                      const double *const *F0PI, int w_single_form, int w_multi_form,
                                      int psingle_form, int w_single_rayleigh, int w_multi_rayleigh,
                                      int psingle_rayleigh, double frac_a, double frac_b, double frac_c,
                                      double constant_back, double constant_forward, int stream, double b_top,
                                      int single_form, int compound_f_deltaM, double *const *xint_at_top,
                                      const double *gweight, const double *tweight, double *const *albedo)
{
    (void)cosb;
    if (!ctx) return fail(nullptr, "null context");
    if (nspec < 1) return fail(ctx, "get_reflected_SH_batch: nspec must be >= 1, got %d", nspec);
    if (nlevel < 2 || nwno < 1 || numg < 1 || numt < 1) return fail(ctx, "get_reflected_SH_batch: bad sizes");
    if (stream != 2 && stream != 4) return fail(ctx, "get_reflected_SH_batch: stream must be 2 or 4, got %d", stream);
    if (plane_pitch < nwno) return fail(ctx, "get_reflected_SH_batch: plane_pitch < nwno");
    if (ngeom != 1 && ngeom != nspec)
        return fail(ctx, "get_reflected_SH_batch: ngeom must be 1 (one geometry for all) or nspec, got %d", ngeom);
    const int nang = numg * numt;
    if (nang > SH_MAX_ANG) return fail(ctx, "get_reflected_SH_batch: at most %d disk angles", SH_MAX_ANG);
    const double *const *pl[10] = {dtau, tau, w0, ftau_cld, ftau_ray, f_deltaM, dtau_og, tau_og, w0_og, cosb_og};
    for (int j = 0; j < 10; ++j) {
        if (!pl[j]) return fail(ctx, "get_reflected_SH_batch: null plane pointer array");
        for (int s = 0; s < nspec; ++s)
            if (!pl[j][s]) return fail(ctx, "get_reflected_SH_batch: plane %d of spectrum %d is NULL", j, s);
    }
    if (!surf_reflect || !F0PI || !xint_at_top || !ubar0 || !ubar1 || !cos_theta)
        return fail(ctx, "get_reflected_SH_batch: null argument");
    const bool fuse = albedo && gweight && tweight;
    for (int s = 0; s < nspec; ++s)
        if (!surf_reflect[s] || !F0PI[s] || !xint_at_top[s] || (fuse && !albedo[s]))
            return fail(ctx, "get_reflected_SH_batch: null per-spectrum pointer (spectrum %d)", s);
    if (sizeof(SHBatchItem) * (size_t)nspec > picaso_ctx::SLOT_BYTES)
        return fail(ctx, "get_reflected_SH_batch: at most %zu spectra per call", picaso_ctx::SLOT_BYTES / sizeof(SHBatchItem));
    PZ_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<SHBatchItem> items((size_t)nspec);
    for (int s = 0; s < nspec; ++s) {
        SHBatchItem &it = items[(size_t)s];
        it.dtau = dtau[s]; it.tau = tau[s]; it.w0 = w0[s]; it.ftau_cld = ftau_cld[s]; it.ftau_ray = ftau_ray[s];
        it.f_deltaM = f_deltaM[s]; it.dtau_og = dtau_og[s]; it.tau_og = tau_og[s]; it.w0_og = w0_og[s];
        it.cosb_og = cosb_og[s]; it.surf_reflect = surf_reflect[s]; it.F0PI = F0PI[s]; it.xint = xint_at_top[s];
        it.cos_theta = cos_theta[ngeom > 1 ? s : 0];
        const double *u0 = ubar0 + (ngeom > 1 ? (size_t)s * nang : 0), *u1 = ubar1 + (ngeom > 1 ? (size_t)s * nang : 0);
        for (int k = 0; k < nang; ++k) it.ang[k] = make_sh_angle(u0[k], u1[k], false);
    }
    const void *d = nullptr;
    PZ_TRY(table_upload(ctx, items.data(), sizeof(SHBatchItem) * items.size(), &d));
    SHArgs a = reflected_sh_args(nlevel, nwno, plane_pitch, stream, dtau[0], tau[0], w0[0], ftau_cld[0], ftau_ray[0],
                                 f_deltaM[0], dtau_og[0], tau_og[0], w0_og[0], cosb_og[0], surf_reflect[0], F0PI[0],
                                 cos_theta[0], w_single_form, w_multi_form, psingle_form, w_single_rayleigh,
                                 w_multi_rayleigh, psingle_rayleigh, frac_a, frac_b, frac_c, constant_back,
                                 constant_forward, b_top, single_form, compound_f_deltaM);
    a.batch = (const SHBatchItem *)d;
    a.nspec_ = nspec;
    a.nang = nang;
    a.xint = xint_at_top[0];
    PZ_TRY(launch_sh(ctx, a, nang, false));
    if (fuse)
        for (int s = 0; s < nspec; ++s)
            PZ_TRY(picaso_compress_disco_dev(ctx, nwno, cos_theta[ngeom > 1 ? s : 0], xint_at_top[s], gweight, numg,
                                             tweight, numt, F0PI[s], albedo[s]));
    return 0;
}

int picaso_get_reflected_SH(picaso_ctx *ctx, int nlevel, int nwno, int numg, int numt, const double *dtau,
                            const double *tau, const double *w0, const double *cosb,
                            const double *ftau_cld, const double *ftau_ray, const double *f_deltaM,
                            const double *dtau_og, const double *tau_og, const double *w0_og,
                            const double *cosb_og, const double *surf_reflect, const double *ubar0,
                            const double *ubar1, double cos_theta, const double *F0PI,
                            int w_single_form, int w_multi_form, int psingle_form,
                            int w_single_rayleigh, int w_multi_rayleigh, int psingle_rayleigh,
                            double frac_a, double frac_b, double frac_c, double constant_back,
                            double constant_forward, int stream, double b_top, int flx,
                            int single_form, int compound_f_deltaM, double *xint_at_top, double *flux)
{
    if (!ctx) return fail(nullptr, "null context");
    if (nlevel < 2 || nwno < 1 || numg < 1 || numt < 1) return fail(ctx, "get_reflected_SH: bad sizes");
    if (stream != 2 && stream != 4) return fail(ctx, "get_reflected_SH: stream must be 2 or 4, got %d", stream);
    if (flx && !flux) return fail(ctx, "get_reflected_SH: flx=1 needs the flux output (numg,numt,stream*nlevel,nwno)");
    PZ_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nl = (size_t)(nlevel - 1) * nwno, nv = (size_t)nlevel * nwno, nang = (size_t)numg * numt;
    const size_t nflux = flx ? nang * stream * nlevel * nwno : 0;
    PZ_TRY(arena_reset(ctx, sizeof(double) * (9 * nl + 2 * nv + 2 * (size_t)nwno + nang * nwno + nflux) + 64 * 256));
    const double *d[10], *d_rs, *d_f0;
    const double *h[10] = {dtau, tau, w0, ftau_cld, ftau_ray, f_deltaM, dtau_og, tau_og, w0_og, cosb_og};
    for (int j = 0; j < 10; ++j) {                    // planes left out (cloud-free form) stay NULL for the _dev entry
        d[j] = nullptr;
        if (h[j]) PZ_TRY(arena_upload(ctx, h[j], (j == 1 || j == 7) ? nv : nl, &d[j]));
    }
    PZ_TRY(arena_upload(ctx, surf_reflect, (size_t)nwno, &d_rs));
    PZ_TRY(arena_upload(ctx, F0PI, (size_t)nwno, &d_f0));
    double *d_x = (double *)arena_take(ctx, sizeof(double) * nang * nwno);
    double *d_fl = nflux ? (double *)arena_take(ctx, sizeof(double) * nflux) : nullptr;
    if (!d_x || (nflux && !d_fl)) return fail(ctx, "arena exhausted");
    PZ_TRY(picaso_get_reflected_SH_dev(ctx, nlevel, nwno, nwno, numg, numt, d[0], d[1], d[2], cosb, d[3], d[4], d[5],
                                       d[6], d[7], d[8], d[9], d_rs, ubar0, ubar1, cos_theta, d_f0, w_single_form,
                                       w_multi_form, psingle_form, w_single_rayleigh, w_multi_rayleigh,
                                       psingle_rayleigh, frac_a, frac_b, frac_c, constant_back, constant_forward,
                                       stream, b_top, flx, single_form, compound_f_deltaM, d_x, d_fl, nullptr,
                                       nullptr, nullptr));
    PZ_HIP(ctx, hipMemcpyAsync(xint_at_top, d_x, sizeof(double) * nang * nwno, hipMemcpyDeviceToHost, ctx->stream));
    if (nflux) PZ_HIP(ctx, hipMemcpyAsync(flux, d_fl, sizeof(double) * nflux, hipMemcpyDeviceToHost, ctx->stream));
    PZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int picaso_get_thermal_SH_dev(picaso_ctx *ctx, int nlevel, const double *wno, int nwno, long plane_pitch,
                              int numg, int numt, const double *tlevel, const double *dtau,
                              const double *tau, const double *w0, const double *cosb_og,
                              const double *plevel, const double *ubar1, const double *surf_reflect,
                              int stream, int hard_surface, int cosb_differs_from_cosb_og, int flx,
                              double *xint_at_top, const double *gweight, const double *tweight,
                              double *flux_disk)
{
    (void)tau;
    if (!ctx) return fail(nullptr, "null context");
    if (nlevel < 2 || nwno < 1 || numg < 1 || numt < 1) return fail(ctx, "get_thermal_SH: bad sizes");
    PZ_NEED(ctx, "get_thermal_SH", wno, tlevel, dtau, w0, cosb_og, plevel, ubar1, surf_reflect, xint_at_top);
    if (stream != 2 && stream != 4) return fail(ctx, "get_thermal_SH: stream must be 2 or 4, got %d", stream);
    if (flx) return fail(ctx, "get_thermal_SH: flx=1 is broken in the reference (fluxes.py:3102) and not built");
    PZ_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<double> tab(2 * (size_t)nlevel);
    for (int i = 0; i < nlevel; ++i) { tab[i] = tlevel[i]; tab[nlevel + i] = plevel[i]; }
    const void *d_tab = nullptr;
    PZ_TRY(table_upload(ctx, tab.data(), sizeof(double) * tab.size(), &d_tab));
    SHArgs a{};
    a.nlayer = nlevel - 1; a.nwno = nwno; a.stream = stream; a.pitch = plane_pitch;
    a.dtau = dtau; a.w0 = w0; a.cosb_og = cosb_og; a.surf_reflect = surf_reflect;
    a.wno = wno; a.tlevel = (const double *)d_tab; a.plevel = a.tlevel + nlevel;
    a.hard_surface = hard_surface; a.use_ff = cosb_differs_from_cosb_og;
    if (getenv("PICASO_AMD_SH_THERMAL_PER_ANGLE")) {            // the round-2 kernel: one wave per angle, nothing shared
        PZ_TRY(launch_sh_angles(ctx, a, numg * numt, nullptr, ubar1, xint_at_top, nullptr, true));
    } else {
        SHTArgs t{};
        t.nlayer = nlevel - 1; t.nwno = nwno; t.pitch = plane_pitch;
        t.dtau = dtau; t.w0 = w0; t.cosb_og = cosb_og; t.surf_reflect = surf_reflect; t.wno = wno;
        t.tlevel = a.tlevel; t.plevel = a.plevel; t.hard_surface = hard_surface; t.use_ff = cosb_differs_from_cosb_og;
        PZ_TRY(launch_sh_thermal(ctx, t, stream, numg * numt, ubar1, xint_at_top));
    }
    if (flux_disk && gweight && tweight)
        PZ_TRY(picaso_compress_thermal_dev(ctx, (size_t)nwno, xint_at_top, gweight, numg, tweight, numt, flux_disk));
    return 0;
}

int picaso_get_thermal_SH(picaso_ctx *ctx, int nlevel, const double *wno, int nwno, int numg, int numt,
                          const double *tlevel, const double *dtau, const double *tau, const double *w0,
                          const double *cosb_og, const double *plevel, const double *ubar1,
                          const double *surf_reflect, int stream, int hard_surface,
                          int cosb_differs_from_cosb_og, int flx, double *xint_at_top)
{
    if (!ctx) return fail(nullptr, "null context");
    if (nlevel < 2 || nwno < 1 || numg < 1 || numt < 1) return fail(ctx, "get_thermal_SH: bad sizes");
    PZ_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nl = (size_t)(nlevel - 1) * nwno, nang = (size_t)numg * numt;
    PZ_TRY(arena_reset(ctx, sizeof(double) * (3 * nl + 2 * (size_t)nwno + nang * nwno) + 32 * 256));
    const double *d_dtau, *d_w0, *d_cbo, *d_rs, *d_wno;
    PZ_TRY(arena_upload(ctx, dtau, nl, &d_dtau));
    PZ_TRY(arena_upload(ctx, w0, nl, &d_w0));
    PZ_TRY(arena_upload(ctx, cosb_og, nl, &d_cbo));
    PZ_TRY(arena_upload(ctx, surf_reflect, (size_t)nwno, &d_rs));
    PZ_TRY(arena_upload(ctx, wno, (size_t)nwno, &d_wno));
    double *d_x = (double *)arena_take(ctx, sizeof(double) * nang * nwno);
    if (!d_x) return fail(ctx, "arena exhausted");
    PZ_TRY(picaso_get_thermal_SH_dev(ctx, nlevel, d_wno, nwno, nwno, numg, numt, tlevel, d_dtau, tau, d_w0, d_cbo,
                                     plevel, ubar1, d_rs, stream, hard_surface, cosb_differs_from_cosb_og, flx, d_x,
                                     nullptr, nullptr, nullptr));
    PZ_HIP(ctx, hipMemcpyAsync(xint_at_top, d_x, sizeof(double) * nang * nwno, hipMemcpyDeviceToHost, ctx->stream));
    PZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

}  // extern "C"
