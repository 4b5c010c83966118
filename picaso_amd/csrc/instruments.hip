// Several instruments from one resident spectrum: the bin means of regrid.hip and the line-spread windows of convolve.hip
// over ONE table of points, so that a spectrum compared with two data sets is neither solved twice nor copied back at full
// resolution (reference driver.py:232-236: `for obs_key in observation_data: mean_regrid(...)`, on the host).
//
// A point p has a column range [lo[p], hi[p]) and a place col[p] in the output row.  Points [0, nmean) are bin means, points
// [nmean, nmean + ngauss) Gaussian windows; the caller sorts them so (picaso_amd/regrid.py, InstrumentsPlan) and col puts
// every value back where its instrument stands.  Ranges may overlap, repeat and be empty: no point reads another's result.
//
// The two bodies are restated from their kernels, not changed, and keep their order of sums:
//   mean   k_mean_regrid: one wave per (point, row), np.bincount's chain from +0.0 through bin_sum (regrid_elem.hpp), divided
//          by the count; an empty range is 0 / 0 = NaN.
//   gauss  k_lsf_convolve: one workgroup of 1 024 threads per point, the weight exp(-(wl[k] - c)^2 / den) formed once per
//          column (no contraction: numpy's argument) and shared by all rows; lane t adds the columns lo + t, lo + t + 1024,
//          ... in increasing order, the 64 lanes of a wave are added in a butterfly, the 16 wave sums in wave order from LDS.
// So with scale == 1 a point has the bits of picaso_mean_regrid_dev / picaso_lsf_convolve_dev for the same range.
//
// scale: the reference scales the flux before it bins it (driver.py:230, 1e-8 (R / d)^2 thermal), so the element is
// regrid_elem(row, i) * scale, ONE rounded product per column formed before the value meets the sum or the weight; a mean
// point is then mean_regrid(wno, scale * v, newx) bit for bit.  scale == 1.0: no product.
#include "common.hpp"
#include "regrid_elem.hpp"

namespace pz {

constexpr int INS_THREADS = 1024;                   // CONV_THREADS of convolve.hip: a point's bits depend on it
constexpr int INS_WAVES = INS_THREADS / 64;

struct InstrumentsArgs {
    long nwno;
    int nmean, ngauss, nrows, scaled;
    double scale;
    const int *lo, *hi, *col;                       // (nmean + ngauss)
    const double *wl, *centre, *den;                // (nwno), (nmean + ngauss) x 2: read for the Gaussian points only
    picaso_regrid_row rows[PICASO_REGRID_MAX_ROWS];
    double *out;                                    // (nrows, nmean + ngauss)
};

__device__ __forceinline__ double ins_elem(const InstrumentsArgs &a, const picaso_regrid_row &row, long i)
{
#pragma clang fp contract(off)
    const double v = regrid_elem(row, i);
    return a.scaled ? v * a.scale : v;
}

// the caller's table is trusted; the clamps keep a broken one from reading or writing outside the arrays
__device__ __forceinline__ void ins_range(const InstrumentsArgs &a, int p, long &lo, long &hi, long &col)
{
    lo = a.lo[p];
    hi = a.hi[p];
    col = a.col[p];
    lo = lo < 0 ? 0 : lo;
    hi = hi > a.nwno ? a.nwno : hi;
    if (col < 0 || col >= (long)a.nmean + a.ngauss) col = -1;
}

__global__ __launch_bounds__(64) void k_instruments_mean(const InstrumentsArgs a)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x, lane = threadIdx.x;
    const picaso_regrid_row &row = a.rows[blockIdx.y];
    long lo, hi, col;
    ins_range(a, p, lo, hi, col);
    const double s = bin_sum(lo, hi, lane, [&](long i) { return ins_elem(a, row, i); });
    const long count = hi > lo ? hi - lo : 0;
    if (lane == 0 && col >= 0)
        a.out[(long)blockIdx.y * ((long)a.nmean + a.ngauss) + col] = s / (double)count;     // empty: 0 / 0 = NaN
}

__device__ __forceinline__ double ins_wave_sum(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

__global__ __launch_bounds__(INS_THREADS) void k_instruments_gauss(const InstrumentsArgs a)
{
    __shared__ double part[INS_WAVES][PICASO_REGRID_MAX_ROWS + 1];
    const int p = a.nmean + blockIdx.x, t = threadIdx.x, wave = t >> 6;
    long lo, hi, col;
    ins_range(a, p, lo, hi, col);
    const double c = a.centre[p], den = a.den[p];
    double s = 0.0, n[PICASO_REGRID_MAX_ROWS];
#pragma unroll
    for (int r = 0; r < PICASO_REGRID_MAX_ROWS; ++r) n[r] = 0.0;
    for (long k = lo + t; k < hi; k += INS_THREADS) {
        double g;
        {
#pragma clang fp contract(off)
            const double d = a.wl[k] - c;
            const double q = d * d;
            g = exp(-q / den);
        }
        s = s + g;
#pragma unroll
        for (int r = 0; r < PICASO_REGRID_MAX_ROWS; ++r)
            if (r < a.nrows) n[r] = fma(ins_elem(a, a.rows[r], k), g, n[r]);
    }
    s = ins_wave_sum(s);
#pragma unroll
    for (int r = 0; r < PICASO_REGRID_MAX_ROWS; ++r)
        if (r < a.nrows) n[r] = ins_wave_sum(n[r]);
    if ((t & 63) == 0) {
        part[wave][PICASO_REGRID_MAX_ROWS] = s;
#pragma unroll
        for (int r = 0; r < PICASO_REGRID_MAX_ROWS; ++r)
            if (r < a.nrows) part[wave][r] = n[r];
    }
    __syncthreads();
    if (t < a.nrows && col >= 0) {
        double st = 0.0, nt = 0.0;
        for (int w = 0; w < INS_WAVES; ++w) {
            st = st + part[w][PICASO_REGRID_MAX_ROWS];
            nt = nt + part[w][t];
        }
        a.out[(long)t * ((long)a.nmean + a.ngauss) + col] = nt / st;      // no weight in the window: 0 / 0 = NaN
    }
}

}  // namespace pz

using namespace pz;

extern "C" int picaso_instruments_reduce_dev(picaso_ctx *ctx, long nwno, const double *wl, int nmean, int ngauss,
                                             const int *lo, const int *hi, const int *col, const double *centre,
                                             const double *den, double scale, int nrows, const picaso_regrid_row *rows,
                                             double *out)
{
    const char *who = "picaso_instruments_reduce_dev";
    if (!ctx || !lo || !hi || !col || !centre || !den || !rows || !out) return fail(ctx, "%s: null argument", who);
    if (nwno < 1 || nwno > 0x7fffffffL)
        return fail(ctx, "%s: nwno must be in [1, 2^31 - 1] (32-bit window offsets), got %ld", who, nwno);
    if (nmean < 0 || ngauss < 0) return fail(ctx, "%s: negative count (nmean %d, ngauss %d)", who, nmean, ngauss);
    if ((long)nmean + ngauss < 1 || (long)nmean + ngauss > 0x7fffffffL)
        return fail(ctx, "%s: nmean + ngauss must be in [1, 2^31 - 1], got %d + %d", who, nmean, ngauss);
    if (ngauss > 0 && !wl) return fail(ctx, "%s: %d Gaussian points need wl", who, ngauss);
    if (scale != scale) return fail(ctx, "%s: scale is NaN", who);
    InstrumentsArgs a{};
    PZ_TRY(regrid_rows_check(ctx, who, nrows, rows, a.rows));
    a.nwno = nwno;
    a.nmean = nmean;
    a.ngauss = ngauss;
    a.nrows = nrows;
    a.scaled = scale != 1.0;
    a.scale = scale;
    a.lo = lo;
    a.hi = hi;
    a.col = col;
    a.wl = wl;
    a.centre = centre;
    a.den = den;
    a.out = out;
    PZ_HIP(ctx, hipSetDevice(ctx->device));
    if (nmean > 0) {
        hipLaunchKernelGGL(k_instruments_mean, dim3((unsigned)nmean, (unsigned)nrows), dim3(64), 0, ctx->stream, a);
        PZ_HIP(ctx, hipGetLastError());
    }
    if (ngauss > 0) {
        hipLaunchKernelGGL(k_instruments_gauss, dim3((unsigned)ngauss), dim3(INS_THREADS), 0, ctx->stream, a);
        PZ_HIP(ctx, hipGetLastError());
    }
    return 0;
}
