// Bin resident spectra to an instrument grid: the mean of the points of every bin (reference justplotit.py:31-63,
// mean_regrid -> scipy.stats.binned_statistic(statistic='mean'), which is np.bincount(idx, weights) / counts), fused with
// the elementwise post-processing of the output dictionary (justdoit.py:552-599: fpfs_reflected = albedo k,
// fpfs_thermal = thermal / stellar k, fpfs_total = fpfs_thermal + fpfs_reflected).
//
// np.bincount adds a bin's weights in increasing index order to a sum that starts at +0.0, so a bin's value is ONE chain
// of dependent fp64 additions -- there is nothing to reorder if the bits are to be numpy's.  The parallelism is bins x rows:
// one wave per (bin, row).  The wave reads its bin in coalesced chunks of 64 columns (lane l forms v[base + l]) and every
// lane carries the same running sum, to which the chunk's 64 values are added in lane order; a value reaches the adder
// through v_readlane (two scalar registers, no LDS round trip and no barrier), and the next chunk's loads are issued before
// the chain of the current one, so that a long bin (1 000 columns at R = 100 on a 1e5-point grid) pays the memory latency
// once.  Contraction is off: op 3 as written is a product, a quotient, a product and a sum, each rounded, as numpy does it.
#include "common.hpp"
#include "regrid_elem.hpp"

namespace pz {

struct MeanRegridArgs {
    long nwno;
    int nbins, nrows;
    const int *start;                               // (nbins + 1)
    picaso_regrid_row rows[PICASO_REGRID_MAX_ROWS];
    double *out;                                    // (nrows, nbins)
};

__global__ __launch_bounds__(64) void k_mean_regrid(const MeanRegridArgs a)
{
#pragma clang fp contract(off)
    const int j = blockIdx.x, lane = threadIdx.x;
    const picaso_regrid_row &row = a.rows[blockIdx.y];
    // the caller's table is trusted to be non-decreasing; the clamps keep a broken one from reading outside the arrays
    long lo = a.start[j], hi = a.start[j + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > a.nwno ? a.nwno : hi;
    const double s = bin_sum(lo, hi, lane, [&](long i) { return regrid_elem(row, i); });
    const long count = hi > lo ? hi - lo : 0;
    if (lane == 0) a.out[(long)blockIdx.y * a.nbins + j] = s / (double)count;      // an empty bin: 0 / 0 = NaN
}

}  // namespace pz

using namespace pz;

extern "C" int picaso_mean_regrid_dev(picaso_ctx *ctx, long nwno, int nbins, const int *start, int nrows,
                                      const picaso_regrid_row *rows, double *out)
{
    if (!ctx || !start || !rows || !out) return fail(ctx, "picaso_mean_regrid_dev: null argument");
    if (nwno < 1 || nwno > 0x7fffffffL)
        return fail(ctx, "picaso_mean_regrid_dev: nwno must be in [1, 2^31 - 1] (32-bit bin offsets), got %ld", nwno);
    if (nbins <= 0) return fail(ctx, "picaso_mean_regrid_dev: nbins must be positive, got %d", nbins);
    MeanRegridArgs a{};
    PZ_TRY(regrid_rows_check(ctx, "picaso_mean_regrid_dev", nrows, rows, a.rows));
    a.nwno = nwno;
    a.nbins = nbins;
    a.nrows = nrows;
    a.start = start;
    a.out = out;
    PZ_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_mean_regrid, dim3((unsigned)nbins, (unsigned)nrows), dim3(64), 0, ctx->stream, a);
    PZ_HIP(ctx, hipGetLastError());
    return 0;
}
