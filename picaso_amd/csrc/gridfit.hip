// Fit model grids to data: weighted sums of rows of a resident (nrows, nwave) matrix of spectra, binned to a data set's
// grid in the same launch, and the reductions that compare the binned models with the data (reference analyze.py:305-388
// fit_grid, :923-1000 custom_interp; driver.py:253-332 log_likelihood).
//
// A sample is a short table of (row, weight) pairs and a divisor: the 2^d corners of a d-parameter grid cell with the
// products of their linear weights (custom_interp's hypercube loop), three neighbours with 1/distance^2 (its fallback where
// a corner is missing), or ONE row with weight 1 and divisor 1 (a model of the grid as it is: 0.0 + 1.0 x and x / 1.0 are
// exact).  Column i of a sample is (((0.0 + w0 g[r0][i]) + w1 g[r1][i]) + ...) / div: the products and the additions in
// table order, each rounded, as the reference's `interp += np.prod(weights) * spectrum` forms it.  The binned form hands
// that column to bin_sum (regrid_elem.hpp) as it is formed, one wave per (bin, sample), so a bin's mean has the bits of
// mean_regrid of the interpolated spectrum without that spectrum ever reaching HBM.
//
// The table of a sample is read once per workgroup: thread c puts weight c and the offset of row c into LDS, and every
// column reads them from there at a wave-uniform address (a broadcast).  Row indices and the count are clamped there, so
// that a broken table cannot read outside the matrix; the Python wrapper refuses such a table before it is uploaded.
#include "common.hpp"
#include "regrid_elem.hpp"

namespace pz {

constexpr int GRID_KMAX = PICASO_GRID_MAX_K;

struct GridRowsArgs {
    long nwave;
    int nrows, kmax, nbins, s0;                     // s0: the first sample of this launch (grid.y holds 65 535 at most)
    const double *grid;                             // (nrows, nwave)
    const int *rows;                                // (S, kmax)
    const double *wts;                              // (S, kmax)
    const int *kcount;                              // (S)
    const double *div;                              // (S)
    const int *start;                               // (nbins + 1)
    double *out_full;                               // (S, nwave)
    double *out_binned;                             // (S, nbins)
};

// thread t < K of the workgroup stores entry t; returns K (clamped into [0, kmax])
__device__ __forceinline__ int sample_table(const GridRowsArgs &a, long s, int t, double *sw, long *soff)
{
    int k = a.kcount[s];
    k = k < 0 ? 0 : (k > a.kmax ? a.kmax : k);
    if (t < k) {
        int r = a.rows[s * a.kmax + t];
        r = r < 0 ? 0 : (r >= a.nrows ? a.nrows - 1 : r);
        sw[t] = a.wts[s * a.kmax + t];
        soff[t] = (long)r * a.nwave;
    }
    __syncthreads();
    return k;
}

__device__ __forceinline__ double sample_elem(const double *grid, const double *sw, const long *soff, int k, double div,
                                              long i)
{
#pragma clang fp contract(off)
    double v = 0.0;
    for (int c = 0; c < k; ++c) v = v + sw[c] * grid[soff[c] + i];
    return v / div;
}

__global__ __launch_bounds__(256) void k_grid_rows_full(const GridRowsArgs a)
{
    __shared__ double sw[GRID_KMAX];
    __shared__ long soff[GRID_KMAX];
    const long s = (long)a.s0 + blockIdx.y;
    const int k = sample_table(a, s, threadIdx.x, sw, soff);
    const double div = a.div[s];
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < a.nwave) a.out_full[s * a.nwave + i] = sample_elem(a.grid, sw, soff, k, div, i);
}

__global__ __launch_bounds__(64) void k_grid_rows_binned(const GridRowsArgs a)
{
    __shared__ double sw[GRID_KMAX];
    __shared__ long soff[GRID_KMAX];
    const int j = blockIdx.x, lane = threadIdx.x;
    const long s = (long)a.s0 + blockIdx.y;
    const int k = sample_table(a, s, lane, sw, soff);
    const double div = a.div[s];
    long lo = a.start[j], hi = a.start[j + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > a.nwave ? a.nwave : hi;
    const double *grid = a.grid;
    const double sum = bin_sum(lo, hi, lane, [&](long i) { return sample_elem(grid, sw, soff, k, div, i); });
    const long count = hi > lo ? hi - lo : 0;
    if (lane == 0) a.out_binned[s * a.nbins + j] = sum / (double)count;            // an empty bin: 0 / 0 = NaN
}

// ---- the reductions over a sample's ndata binned points ------------------------------------------------------------------
// One workgroup of 256 threads per sample.  Thread t adds its points t, t + 256, ... in that order to +0.0, the 256
// partial sums go through one fixed binary tree in LDS: a sample's bits depend on ndata alone.
constexpr int LL_THREADS = 256;

__device__ __forceinline__ double block_sum(double v, double *red, int t)
{
    __syncthreads();                                 // the previous sum's readers are done with `red`
    red[t] = v;
    __syncthreads();
#pragma unroll
    for (int stride = LL_THREADS / 2; stride > 0; stride >>= 1) {
        if (t < stride) red[t] = red[t] + red[t + stride];
        __syncthreads();
    }
    return red[0];
}

struct GridLoglikeArgs {
    int ndata, mode, fit_offset, numparams, s0;
    const double *binned;                            // (S, ndata)
    const double *y, *e;                             // (ndata)
    const double *offset, *scaling, *err_inf;        // (S), mode 0
    double *out;                                     // (S), mode 0
    double *shift, *chi2, *best;                     // (S), (S), (S, ndata), mode 1
};

__global__ __launch_bounds__(LL_THREADS) void k_grid_loglike(const GridLoglikeArgs a)
{
#pragma clang fp contract(off)
    __shared__ double red[LL_THREADS];
    const int t = threadIdx.x, n = a.ndata;
    const long s = (long)a.s0 + blockIdx.x;
    const double *m = a.binned + s * n;
    if (a.mode == 0) {
        // driver.py:296-326: -0.5 sum(((y + offset) scaling - m)^2 / (e^2 + err_inf) + ln(2 pi (e^2 + err_inf)))
        const double off = a.offset[s], sc = a.scaling[s], inf = a.err_inf[s];
        const double two_pi = 2.0 * 3.141592653589793;
        double p = 0.0;
        for (int i = t; i < n; i += LL_THREADS) {
            const double yd = (a.y[i] + off) * sc;
            const double sigma = a.e[i] * a.e[i] + inf;
            const double r = yd - m[i];
            p = p + (r * r / sigma + log(two_pi * sigma));
        }
        const double tot = block_sum(p, red, t);
        if (t == 0) a.out[s] = -0.5 * tot;
        return;
    }
    // analyze.py:369-381: the constant that an unweighted least-squares fit of y = m + shift finds is mean(y - m)
    double shift = 0.0;
    if (a.fit_offset) {
        double p = 0.0;
        for (int i = t; i < n; i += LL_THREADS) p = p + (a.y[i] - m[i]);
        shift = block_sum(p, red, t) / (double)n;
    }
    double p = 0.0;
    for (int i = t; i < n; i += LL_THREADS) {
        const double b = m[i] + shift;
        a.best[s * n + i] = b;
        const double q = (a.y[i] - b) / a.e[i];
        p = p + q * q;
    }
    const double tot = block_sum(p, red, t);
    if (t == 0) {
        a.shift[s] = shift;
        a.chi2[s] = tot / (double)(n - a.numparams);
    }
}

}  // namespace pz

using namespace pz;

extern "C" int picaso_grid_rows_dev(picaso_ctx *ctx, int nrows, long nwave, const double *grid, int nsamp, int kmax,
                                    const int *rows, const double *wts, const int *kcount, const double *div,
                                    double *out_full, int nbins, const int *start, double *out_binned)
{
    const char *who = "picaso_grid_rows_dev";
    if (!ctx) return fail(ctx, "%s: null context", who);
    PZ_NEED(ctx, who, grid, rows, wts, kcount, div);
    if (!out_full && !out_binned) return fail(ctx, "%s: neither out_full nor out_binned is given", who);
    if (out_binned && !start) return fail(ctx, "%s: out_binned needs the bin table start", who);
    if (kmax < 1 || kmax > GRID_KMAX) return fail(ctx, "%s: K must be in [1, %d], got %d", who, GRID_KMAX, kmax);
    if (nrows < 1) return fail(ctx, "%s: nrows must be positive, got %d", who, nrows);
    if (nwave < 1 || nwave > 0x7fffffffL)
        return fail(ctx, "%s: nwave must be in [1, 2^31 - 1] (32-bit bin offsets), got %ld", who, nwave);
    if (nsamp < 1) return fail(ctx, "%s: the number of samples must be positive, got %d", who, nsamp);
    if (out_binned && nbins < 1) return fail(ctx, "%s: nbins must be positive, got %d", who, nbins);
    GridRowsArgs a{};
    a.nwave = nwave;
    a.nrows = nrows;
    a.kmax = kmax;
    a.nbins = nbins;
    a.grid = grid;
    a.rows = rows;
    a.wts = wts;
    a.kcount = kcount;
    a.div = div;
    a.start = start;
    a.out_full = out_full;
    a.out_binned = out_binned;
    PZ_HIP(ctx, hipSetDevice(ctx->device));
    for (long s0 = 0; s0 < nsamp; s0 += 65535) {
        const unsigned ns = (unsigned)(nsamp - s0 < 65535 ? nsamp - s0 : 65535);
        a.s0 = (int)s0;
        if (out_full)
            hipLaunchKernelGGL(k_grid_rows_full, dim3((unsigned)((nwave + 255) / 256), ns), dim3(256), 0, ctx->stream, a);
        if (out_binned)
            hipLaunchKernelGGL(k_grid_rows_binned, dim3((unsigned)nbins, ns), dim3(64), 0, ctx->stream, a);
    }
    PZ_HIP(ctx, hipGetLastError());
    return 0;
}

extern "C" int picaso_grid_loglike_dev(picaso_ctx *ctx, int nsamp, int ndata, const double *binned, const double *y,
                                       const double *e, int mode, const double *offset, const double *scaling,
                                       const double *err_inf, double *out, int fit_offset, int numparams, double *shift,
                                       double *chi2, double *best)
{
    const char *who = "picaso_grid_loglike_dev";
    if (!ctx) return fail(ctx, "%s: null context", who);
    PZ_NEED(ctx, who, binned, y, e);
    if (mode != 0 && mode != 1) return fail(ctx, "%s: mode must be 0 (log likelihood) or 1 (chi squared), got %d", who, mode);
    if (nsamp < 1) return fail(ctx, "%s: the number of samples must be positive, got %d", who, nsamp);
    if (ndata < 1) return fail(ctx, "%s: ndata must be positive, got %d", who, ndata);
    if (mode == 0) {
        PZ_NEED(ctx, who, offset, scaling, err_inf, out);
    } else {
        PZ_NEED(ctx, who, shift, chi2, best);
        if (numparams < 0 || ndata - numparams <= 0)
            return fail(ctx, "%s: ndata - numparams must be positive, got %d - %d", who, ndata, numparams);
    }
    GridLoglikeArgs a{};
    a.ndata = ndata;
    a.mode = mode;
    a.fit_offset = fit_offset;
    a.numparams = numparams;
    a.binned = binned;
    a.y = y;
    a.e = e;
    a.offset = offset;
    a.scaling = scaling;
    a.err_inf = err_inf;
    a.out = out;
    a.shift = shift;
    a.chi2 = chi2;
    a.best = best;
    PZ_HIP(ctx, hipSetDevice(ctx->device));
    const long chunk = 1L << 30;
    for (long s0 = 0; s0 < nsamp; s0 += chunk) {
        a.s0 = (int)s0;
        const unsigned ns = (unsigned)(nsamp - s0 < chunk ? nsamp - s0 : chunk);
        hipLaunchKernelGGL(k_grid_loglike, dim3(ns), dim3(LL_THREADS), 0, ctx->stream, a);
    }
    PZ_HIP(ctx, hipGetLastError());
    return 0;
}
