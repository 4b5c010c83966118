// Contribution functions of a spectrum -- gfx950.  "Which pressures does this emission feature come from?" and "which layers
// set this transit depth?": the reference's justplotit.thermal_contribution (justplotit.py:1584-1643) and
// justplotit.transmission_contribution (:1697-1779), on the three optical-depth planes the opacity stage leaves in HBM.
//
// Thermal (Lothringer+2018 eq. 4): t = (taugas + taucld) + tauray clipped at tau_max, s = cumsum(t) down the column,
//     CF[l] = bb(T_l, 1/wno) exp(-s_l) t_l / dlnp_l,   l = 0 .. nlayer-2,
// one lane per wavelength walking down its column, every product and quotient rounded where numpy rounds it.
//
// Transmission: CF[k] = (norm - F_k) / sum_k (norm - F_k), F_k the transit depth with layer k removed.  The reference forms
// norm - F_k from nlayer + 1 calls of get_transit_1d and a subtraction of two numbers ~ z^2; here it is the identity
//     norm - F_k = (2/rs^2) sum_{i>k} z_i dz_i exp(-(TAUALL_i - c_ik)) (1 - exp(-c_ik)),   c_ik = 2 TAU[k] delta_length[i][i-k-1],
// whose terms are all non-negative.  TAUALL_i - c_ik is the slant depth of chord i through every layer but k.
// Where layer k carries most of a large TAUALL_i the plain difference would keep ~ 2^-53 TAUALL_i of absolute error in
// an argument of exp; the chord sums are therefore kept with their rounding error (two-sum: s_i + e_i is the sum of the
// rounded terms to ~ 2^-100), and (s_i - c_ik) + e_i is exact where c dominates (Sterbenz) and one rounding of the
// result elsewhere.  transit.hip's layout: a 64-wavelength tile of TAU in LDS, [layer][lane], chord geometry from the
// host table through scalar loads, several waves per tile; behind it the chord sums (s: fp64, e: fp32 -- 2^-24 of an
// error term) in a second tile.  2/rs^2 cancels in the ratio and is not applied.  The chord table is formed without the
// cancellation of the reference's sqrt(z_o^2 - z^2) - sqrt(z_i^2 - z^2) (transit_tables, `conditioned`): that form leaves
// 2^-53 z / (2 dz) ~ 4e-15 in every segment, which a share behind 300 e-foldings shows as 1e-12.
#include "common.hpp"
#include "device_math.hpp"
#include "planck_cm.hpp"
#include "regrid_elem.hpp"
#include "transit_tab.hpp"

namespace pz {

// ---------------------------------------------------------------------------------------------- thermal
struct ThermalCfArgs {
    int nlayer, nwno;
    long pitch;
    const double *taugas, *taucld, *tauray;     // (nlayer, nwno), row pitch `pitch`; taucld may be NULL (zeros)
    const double *wno;                          // (nwno)
    const double *tab;                          // device table: tlayer[nlayer], dlnp[nlayer - 1]
    double tau_max;
    double *out;                                // (nlayer - 1, nwno)
};

__global__ __launch_bounds__(256) void k_thermal_cf(const ThermalCfArgs a)
{
#pragma clang fp contract(off)
    const long w = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (w >= a.nwno) return;
    const double *tlayer = a.tab, *dlnp = a.tab + a.nlayer;
    const double wcm = 1.0 / a.wno[w];          // the reference hands blackbody() 1 / wavenumber
    double s = 0.0;                             // np.cumsum: sequential adds, top down
    for (int l = 0; l < a.nlayer - 1; ++l) {
        const long o = (long)l * a.pitch + w;
        double t = (a.taugas[o] + (a.taucld ? a.taucld[o] : 0.0)) + a.tauray[o];
        t = t > a.tau_max ? a.tau_max : t;      // all_taus[all_taus > tau_max] = tau_max: a NaN stays
        s = s + t;
        // exp(-800) is 0 like every np.exp below -745.2; past it fexp's range reduction has nothing left to stand on
        const double ex = fexp(-(s > 800.0 ? 800.0 : s));
        a.out[(long)l * a.nwno + w] = ((planck_lambda_cm(tlayer[l], wcm) * ex) * t) / dlnp[l];
    }
}

// ---------------------------------------------------------------------------------------------- transmission
#ifndef PZ_TRANSIT_CF_WAVES
#define PZ_TRANSIT_CF_WAVES 8
#endif
constexpr int CF_WAVES = PZ_TRANSIT_CF_WAVES;
// the TAU tile (fp64), the chord sums (fp64) and their error terms (fp32), each [nlevel][64]
constexpr size_t CF_ROW_BYTES = TRANSIT_BLOCK * (2 * sizeof(double) + sizeof(float));

struct TransitCfArgs {
    int nlevel, nwno;
    long pitch;
    const double *dtau;        // (nlayer, nwno) device
    const double *tab;         // transit_tables()
    double *out;               // (nlayer, nwno)
};

__global__ __launch_bounds__(TRANSIT_BLOCK * CF_WAVES) void k_transit_cf(const TransitCfArgs a)
{
#pragma clang fp contract(off)
    extern __shared__ double cf_lds[];
    const int lane = threadIdx.x % TRANSIT_BLOCK, wave = threadIdx.x / TRANSIT_BLOCK;
    const long w = blockIdx.x * (long)TRANSIT_BLOCK + lane;
    const int n = a.nlevel, nl = n - 1;
    const double *dl = a.tab, *zdz = dl + (long)n * n, *colden = zdz + n, *mmw = colden + nl;
    double *const tl = cf_lds + lane;                                   // TAU[l] at tl[l * 64]; later the layer sums
    double *const sl = cf_lds + (long)n * TRANSIT_BLOCK + lane;          // chord sums
    float *const el = (float *)(cf_lds + 2L * n * TRANSIT_BLOCK) + lane; // their rounding errors
    const bool live = w < a.nwno;
    for (int l = wave; l < nl; l += CF_WAVES) {         // TAU = DTAU / colden * mmw   (fluxes.py:2648-2650)
        const double d = live ? a.dtau[(long)l * a.pitch + w] : 0.0;
        tl[l * TRANSIT_BLOCK] = d / colden[l] * mmw[l];
    }
    __syncthreads();
    // chord i: TAUALL_i in the reference's order (j ascending) with the rounding error of every add kept aside
    for (int i = wave; i < n; i += CF_WAVES) {
        double s = 0.0, e = 0.0;
        for (int j = 0; j < i; ++j) {
            const double t = (2.0 * tl[(i - j - 1) * TRANSIT_BLOCK]) * dl[(long)i * n + j];
            const double r = s + t, b = r - s;
            e = e + ((s - (r - b)) + (t - b));
            s = r;
        }
        sl[i * TRANSIT_BLOCK] = s;
        el[i * TRANSIT_BLOCK] = (float)e;
    }
    __syncthreads();
    // layer k: its share of every deeper chord, summed in chord order from +0.0; row k of the TAU tile is this wave's alone
    for (int k = wave; k < nl; k += CF_WAVES) {
        const double tk2 = 2.0 * tl[k * TRANSIT_BLOCK];
        double d = 0.0;
        for (int i = k + 1; i < n; ++i) {
            const double c = tk2 * dl[(long)i * n + (i - k - 1)];      // the bits of chord i's term for layer k
            double rest = (sl[i * TRANSIT_BLOCK] - c) + (double)el[i * TRANSIT_BLOCK];
            rest = rest < 0.0 ? 0.0 : rest;                             // comparisons are false for a NaN: it stays
            rest = rest > 800.0 ? 800.0 : rest;                         // exp(-800) = 0: an opaque chord gives 0, never 0 * inf
            d = d + (zdz[i] * fexp(-rest)) * -expm1(-c);                // 1 - exp(-c) with a small c's digits
        }
        tl[k * TRANSIT_BLOCK] = d;
    }
    __syncthreads();
    if (!live) return;
    double sum = 0.0;
    for (int k = 0; k < nl; ++k) sum = sum + tl[k * TRANSIT_BLOCK];     // every wave the same chain: layer order from +0.0
    for (int k = wave; k < nl; k += CF_WAVES)
        a.out[(long)k * a.nwno + w] = tl[k * TRANSIT_BLOCK] / sum;      // a column that absorbs nothing: 0 / 0 = NaN
}

// ---------------------------------------------------------------------------------------------- binning a plane
__global__ __launch_bounds__(64) void k_mean_regrid_plane(long nwno, long pitch, int nbins, const int *start,
                                                          const double *in, double *out)
{
#pragma clang fp contract(off)
    const int j = blockIdx.x, lane = threadIdx.x;
    const double *row = in + (long)blockIdx.y * pitch;
    long lo = start[j], hi = start[j + 1];              // clamped as in k_mean_regrid
    lo = lo < 0 ? 0 : lo;
    hi = hi > nwno ? nwno : hi;
    const double s = bin_sum(lo, hi, lane, [&](long i) { return row[i]; });
    const long count = hi > lo ? hi - lo : 0;
    if (lane == 0) out[(long)blockIdx.y * nbins + j] = s / (double)count;      // an empty bin: 0 / 0 = NaN
}

}  // namespace pz

using namespace pz;

extern "C" {

int picaso_thermal_cf_dev(picaso_ctx *ctx, int nlayer, int nwno, long pitch, const double *taugas, const double *taucld,
                          const double *tauray, const double *tlayer, const double *wno, const double *dlnp,
                          double tau_max, double *out)
{
    if (!ctx) return fail(nullptr, "null context");
    if (nlayer < 1 || nwno < 1) return fail(ctx, "thermal_cf: bad sizes nlayer=%d nwno=%d", nlayer, nwno);
    if (nlayer == 1) return 0;                          // (0, nwno): nothing to write
    PZ_NEED(ctx, "thermal_cf", taugas, tauray, tlayer, wno, dlnp, out);
    if (pitch < nwno) return fail(ctx, "thermal_cf: pitch %ld < nwno %d", pitch, nwno);
    PZ_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<double> tab((size_t)2 * nlayer - 1);
    for (int l = 0; l < nlayer; ++l) tab[l] = tlayer[l];
    for (int l = 0; l < nlayer - 1; ++l) tab[nlayer + l] = dlnp[l];
    const void *d_tab = nullptr;
    PZ_TRY(table_upload(ctx, tab.data(), sizeof(double) * tab.size(), &d_tab));
    ThermalCfArgs a{};
    a.nlayer = nlayer; a.nwno = nwno; a.pitch = pitch;
    a.taugas = taugas; a.taucld = taucld; a.tauray = tauray; a.wno = wno; a.tab = (const double *)d_tab;
    a.tau_max = tau_max; a.out = out;
    hipLaunchKernelGGL(k_thermal_cf, dim3((unsigned)((nwno + 255) / 256)), dim3(256), 0, ctx->stream, a);
    PZ_HIP(ctx, hipGetLastError());
    return 0;
}

int picaso_transit_cf_dev(picaso_ctx *ctx, const double *z, const double *dz, int nlevel, int nwno, long plane_pitch,
                          double rstar, const double *mmw, double k_b, double amu, const double *player,
                          const double *tlayer, const double *colden, const double *dtau, double *out)
{
    if (!ctx) return fail(nullptr, "null context");
    if (nlevel < 2 || nwno < 1) return fail(ctx, "transit_cf: bad sizes nlevel=%d nwno=%d", nlevel, nwno);
    PZ_NEED(ctx, "transit_cf", z, dz, mmw, player, tlayer, colden, dtau, out);
    if (plane_pitch < nwno) return fail(ctx, "transit_cf: plane_pitch %ld < nwno %d", plane_pitch, nwno);
    const size_t lds = CF_ROW_BYTES * (size_t)nlevel;
    if (lds > TRANSIT_LDS_MAX) return fail(ctx, "transit_cf: %d levels exceed the LDS tile", nlevel);
    PZ_HIP(ctx, hipSetDevice(ctx->device));
    TransitCfArgs a{};
    const void *d_tab = nullptr;
    double zmin_term, two_over_rs2;                     // the ratio needs neither
    PZ_TRY(transit_tables(ctx, z, dz, nlevel, rstar, mmw, k_b, amu, player, tlayer, colden, &d_tab, &zmin_term,
                          &two_over_rs2, true));
    a.nlevel = nlevel; a.nwno = nwno; a.pitch = plane_pitch; a.dtau = dtau; a.tab = (const double *)d_tab; a.out = out;
    if (lds > 64 * 1024)
        PZ_HIP(ctx, hipFuncSetAttribute((const void *)k_transit_cf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_transit_cf, dim3((unsigned)((nwno + TRANSIT_BLOCK - 1) / TRANSIT_BLOCK)),
                       dim3(TRANSIT_BLOCK * CF_WAVES), lds, ctx->stream, a);
    PZ_HIP(ctx, hipGetLastError());
    return 0;
}

int picaso_mean_regrid_plane_dev(picaso_ctx *ctx, int nrows, long nwno, long pitch, int nbins, const int *start,
                                 const double *in, double *out)
{
    if (!ctx || !start || !in || !out) return fail(ctx, "picaso_mean_regrid_plane_dev: null argument");
    if (nwno < 1 || nwno > 0x7fffffffL)
        return fail(ctx, "picaso_mean_regrid_plane_dev: nwno must be in [1, 2^31 - 1] (32-bit bin offsets), got %ld", nwno);
    if (nbins <= 0) return fail(ctx, "picaso_mean_regrid_plane_dev: nbins must be positive, got %d", nbins);
    if (nrows < 0 || nrows > 65535) return fail(ctx, "picaso_mean_regrid_plane_dev: nrows must be in [0, 65535], got %d", nrows);
    if (pitch < nwno) return fail(ctx, "picaso_mean_regrid_plane_dev: pitch %ld < nwno %ld", pitch, nwno);
    if (nrows == 0) return 0;
    PZ_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_mean_regrid_plane, dim3((unsigned)nbins, (unsigned)nrows), dim3(64), 0, ctx->stream, nwno, pitch,
                       nbins, start, in, out);
    PZ_HIP(ctx, hipGetLastError());
    return 0;
}

}  // extern "C"
