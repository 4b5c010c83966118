// Where the photons stop -- gfx950.  The reference's justplotit.photon_attenuation (justplotit.py:426-536) and
// justplotit.taumap (:1019-1131) without their figures, and the band means of justplotit.all_optics_1d (:1197-1282), on
// the optical-depth planes the opacity stage leaves in HBM.
//
// k_tau_level: three components (gas, cloud, Rayleigh), each a layer plane d[l] and an optional multiplier plane m[l]
// (the cloud's single-scattering albedo).  A lane owns one column and walks down it:
//     c[0] = 0,  c[i + 1] = c[i] + d[i] m[i]          (np.cumsum's sequential sum; the product rounded, then added)
// and keeps the level the reference's find_nearest_2d / find_nearest_1d (:848-869) picks for at_tau.  That rule sorts the
// column's values with np.unique, takes the first minimum of |value - at_tau| and returns the LAST level that holds the
// value.  On a non-decreasing column the values are already sorted, so one walk gives the same level: level i replaces
// the best one so far when it is strictly nearer, or when it repeats the best value.  (On a tie in distance the smaller,
// shallower value stays, as argmin keeps the first; of equal values the deepest wins, as iar + ic - 1.)  A column with a
// NaN gets level -1 and pressure NaN (the reference's answer depends on where np.unique puts the NaNs).
//
// Element (l, c) of a plane lies at l * pitch + c * stride + offset, so that one kernel reads monochromatic planes
// (stride 1), one Gauss point of a correlated-k plane (nlayer, nwno, ngauss) (stride ngauss, offset igauss) and the facet
// columns of a 3-D run.  With stride 1 the lanes of a wave read 512 contiguous bytes per plane and layer.
//
// k_band_mean_rows: the mean of the columns [lo, hi) of every row of up to three planes, one wave per row and plane:
// lane-strided partial sums, then a butterfly over the wave -- an order that depends on the window alone.
#include "common.hpp"

namespace pz {

constexpr int ATT_NCOMP = 3;
constexpr int ATT_BLOCK = 64;           // one wave per workgroup: 1e5 columns are 1 563 of them, six per CU

struct TauPlane {
    const double *d, *m;                // layer plane (NULL: zeros) and multiplier plane (NULL: none)
    long pitch, stride, offset, mpitch, mstride, moffset;
};

struct TauLevelArgs {
    int nlayer;
    long ncol;
    TauPlane comp[ATT_NCOMP];
    const double *plevel;               // device table: (nsets, nlayer + 1); nsets = 1, or one set per column
    int per_column;                     // 1: column c reads set c
    int one_zero_is_bottom;             // taumap's line :1082-1083 for the cloud component
    double at_tau;
    int *level;                         // (4, ncol): the three level indices, then the dominance code
    double *pressure;                   // (3, ncol)
};

__global__ __launch_bounds__(ATT_BLOCK) void k_tau_level(const TauLevelArgs a)
{
#pragma clang fp contract(off)
    const long w = blockIdx.x * (long)ATT_BLOCK + threadIdx.x;
    if (w >= a.ncol) return;            // the partial last tile
    const int n = a.nlayer;
    const double *plev = a.plevel + (a.per_column ? w * (long)(n + 1) : 0L);
    double p[ATT_NCOMP];
#pragma unroll
    for (int k = 0; k < ATT_NCOMP; ++k) {
        const TauPlane &t = a.comp[k];
        const double *d = t.d ? t.d + w * t.stride + t.offset : nullptr;
        const double *m = t.m ? t.m + w * t.mstride + t.moffset : nullptr;
        double c = 0.0, cb = 0.0;       // c[0] = 0 is the best level so far
        double gap = fabs(0.0 - a.at_tau);
        int best = 0, zeros = 1;
        if (d) {
#pragma unroll 4
            for (int l = 0; l < n; ++l) {
                double v = d[(long)l * t.pitch];
                if (m) v = v * m[(long)l * t.mpitch];       // rounded here, added below: never one fma
                c = c + v;
                const double g = fabs(c - a.at_tau);
                const bool take = g < gap || c == cb;       // both false for a NaN
                best = take ? l + 1 : best;
                gap = take ? g : gap;
                cb = take ? c : cb;
                zeros += c == 0.0 ? 1 : 0;
            }
        } else {                        // a plane of zeros: every level repeats c[0], the deepest one wins
            best = n;
            zeros = n + 1;
        }
        if (k == 1 && a.one_zero_is_bottom && zeros == 1) best = n;
        const bool nan = c != c;        // a NaN anywhere in the column has reached the last sum
        a.level[(long)k * a.ncol + w] = nan ? -1 : best;
        p[k] = nan ? __builtin_nan("") : plev[best];
        a.pressure[(long)k * a.ncol + w] = p[k];
    }
    // the three masks of :509-511: the component whose pressure is strictly the smallest; comparisons with a NaN are false
    int dom = -1;
    if (p[0] < p[1] && p[0] < p[2]) dom = 0;
    else if (p[1] < p[0] && p[1] < p[2]) dom = 1;
    else if (p[2] < p[1] && p[2] < p[0]) dom = 2;
    a.level[(long)ATT_NCOMP * a.ncol + w] = dom;
}

struct BandMeanArgs {
    int nrows, nplanes;
    long pitch, lo, hi;
    const double *plane[ATT_NCOMP];
    double *out;                        // (3, nrows); rows of planes not given are left alone
};

__global__ __launch_bounds__(64) void k_band_mean_rows(const BandMeanArgs a)
{
#pragma clang fp contract(off)
    const int r = blockIdx.x, k = blockIdx.y, lane = threadIdx.x;
    if (r >= a.nrows || k >= a.nplanes) return;
    const double *row = a.plane[k] + (long)r * a.pitch;
    double s = 0.0;
    for (long i = a.lo + lane; i < a.hi; i += 64) s = s + row[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s = s + __shfl_xor(s, off, 64);
    const long count = a.hi > a.lo ? a.hi - a.lo : 0;
    if (lane == 0) a.out[(long)k * a.nrows + r] = s / (double)count;        // an empty window: 0 / 0 = NaN
}

}  // namespace pz

using namespace pz;

extern "C" {

int picaso_tau_level_dev(picaso_ctx *ctx, int nlayer, long ncol, const double *const *planes, const long *layout,
                         const double *plevel, int per_column, double at_tau, int one_zero_is_bottom, int *level,
                         double *pressure)
{
    if (!ctx) return fail(nullptr, "null context");
    if (nlayer < 1 || ncol < 1) return fail(ctx, "tau_level: bad sizes nlayer=%d ncol=%ld", nlayer, ncol);
    PZ_NEED(ctx, "tau_level", planes, layout, plevel, level, pressure);
    if (!planes[0] || !planes[2]) return fail(ctx, "tau_level: the gas and the Rayleigh plane are required");
    TauLevelArgs a{};
    for (int k = 0; k < ATT_NCOMP; ++k) {
        TauPlane &t = a.comp[k];
        const long *d = layout + 3 * k, *m = layout + 3 * (ATT_NCOMP + k);
        t.d = planes[k];
        t.m = t.d ? planes[ATT_NCOMP + k] : nullptr;
        t.pitch = d[0]; t.stride = d[1]; t.offset = d[2];
        t.mpitch = m[0]; t.mstride = m[1]; t.moffset = m[2];
        if ((t.d && (t.pitch < 0 || t.stride < 1 || t.offset < 0)) || (t.m && (t.mpitch < 0 || t.mstride < 1 || t.moffset < 0)))
            return fail(ctx, "tau_level: component %d: pitch and offset must not be negative, stride at least 1", k);
    }
    const size_t nsets = per_column ? (size_t)ncol : 1;
    const size_t bytes = sizeof(double) * nsets * (size_t)(nlayer + 1);
    if (bytes > picaso_ctx::SLOT_BYTES)
        return fail(ctx, "tau_level: %zu sets of %d level pressures exceed the table slot", nsets, nlayer + 1);
    PZ_HIP(ctx, hipSetDevice(ctx->device));
    const void *d_plev = nullptr;
    PZ_TRY(table_upload(ctx, plevel, bytes, &d_plev));
    a.nlayer = nlayer; a.ncol = ncol; a.plevel = (const double *)d_plev; a.per_column = per_column ? 1 : 0;
    a.one_zero_is_bottom = one_zero_is_bottom ? 1 : 0; a.at_tau = at_tau; a.level = level; a.pressure = pressure;
    hipLaunchKernelGGL(k_tau_level, dim3((unsigned)((ncol + ATT_BLOCK - 1) / ATT_BLOCK)), dim3(ATT_BLOCK), 0, ctx->stream, a);
    PZ_HIP(ctx, hipGetLastError());
    return 0;
}

int picaso_band_mean_rows_dev(picaso_ctx *ctx, int nrows, long ncols, long pitch, long lo, long hi, int nplanes,
                              const double *plane0, const double *plane1, const double *plane2, double *out)
{
    if (!ctx) return fail(nullptr, "null context");
    if (nrows < 1 || nrows > 0x7fffffff / 2 || ncols < 1 || pitch < ncols)
        return fail(ctx, "band_mean_rows: bad sizes nrows=%d ncols=%ld pitch=%ld", nrows, ncols, pitch);
    if (nplanes < 1 || nplanes > ATT_NCOMP) return fail(ctx, "band_mean_rows: nplanes must be 1 to 3, got %d", nplanes);
    if (lo < 0 || hi > ncols) return fail(ctx, "band_mean_rows: the window [%ld, %ld) leaves the %ld columns", lo, hi, ncols);
    PZ_NEED(ctx, "band_mean_rows", plane0, out);
    if ((nplanes > 1 && !plane1) || (nplanes > 2 && !plane2)) return fail(ctx, "band_mean_rows: a plane is NULL");
    PZ_HIP(ctx, hipSetDevice(ctx->device));
    BandMeanArgs a{};
    a.nrows = nrows; a.nplanes = nplanes; a.pitch = pitch; a.lo = lo; a.hi = hi;
    a.plane[0] = plane0; a.plane[1] = plane1; a.plane[2] = plane2; a.out = out;
    hipLaunchKernelGGL(k_band_mean_rows, dim3((unsigned)nrows, (unsigned)nplanes), dim3(64), 0, ctx->stream, a);
    PZ_HIP(ctx, hipGetLastError());
    return 0;
}

}  // extern "C"
