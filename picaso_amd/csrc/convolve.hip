// Convolve resident spectra with an instrument's line-spread function and evaluate them at the observed wavelengths: a
// Gaussian whose resolving power varies along the spectrum (reference driver.py:338-381, conv_non_uniform_R), fused with
// the elementwise flux ratios of the output dictionary (regrid_elem.hpp).  For the observed point i, over the model columns
// k of its window [lo[i], hi[i]):
//
//     g = exp(-(wl[k] - c[i])^2 / den[i])        S += g        N_r += elem_r(k) g        out[r][i] = N_r / S
//
// The host cuts the window at 39 sigma, beyond which the reference's weight is exp(-760.5) = 0.0 exactly, so the sums run
// over the reference's non-zero terms (picaso_amd/convolve.py).  The argument of exp is formed without contraction and has
// numpy's bits; exp itself and the order of the sums are what differ from the reference.
//
// The fp64 exp (and the quotient in front of it) is the cost, some 60 fp64 instructions per column, so ONE workgroup per
// point forms the weight once per column and every row of the call takes it from a register: at most nine running sums per
// lane.  Lanes stride the window (coalesced loads of wl and of the row inputs).
//
// Workgroup: 1 024 threads, 16 waves.  What sets the time is the longest window, not the total: on the 1e5-point grid 400
// points at R = 100 have windows of 1 400 (4.9 um) to 30 000 columns (0.32 um), 2.5e6 columns in all -- a few microseconds of
// the chip if they were spread evenly -- while the longest window alone is 30 000 / nthreads trips of ~60 dependent fp64
// instructions per lane.  With one wave per point that is 464 trips on 400 of the chip's 1 024 SIMDs; with 16 waves it is 30
// trips, all 400 workgroups are resident at once (two per CU at <= 128 VGPRs), and the eight waves a SIMD then holds
// cover each other's load latency.  A window shorter than the workgroup leaves the waves past its end with empty sums: they
// cost one barrier.
//
// Order of the sums (no atomics; a point's bits depend on its window and on CONV_THREADS only): lane t adds the columns
// lo + t, lo + t + 1024, ... in increasing order; the 64 lanes of a wave are added in a butterfly (partners 32, 16, 8, 4, 2, 1
// lanes apart: an addition is commutative, so both partners hold the same bits after every step); the 16 wave sums are
// added in wave order from LDS.  S is formed the same way by every thread that divides by it.
#include "common.hpp"
#include "regrid_elem.hpp"

namespace pz {

constexpr int CONV_THREADS = 1024;
constexpr int CONV_WAVES = CONV_THREADS / 64;

struct LsfConvolveArgs {
    long nwno;
    int nobs, nrows;
    const double *wl, *centre, *den;                // (nwno), (nobs), (nobs)
    const int *lo, *hi;                             // (nobs)
    picaso_regrid_row rows[PICASO_REGRID_MAX_ROWS];
    double *out;                                    // (nrows, nobs)
};

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

__global__ __launch_bounds__(CONV_THREADS) void k_lsf_convolve(const LsfConvolveArgs a)
{
    __shared__ double part[CONV_WAVES][PICASO_REGRID_MAX_ROWS + 1];
    const int i = blockIdx.x, t = threadIdx.x, wave = t >> 6;
    // the caller's windows are trusted to lie inside the grid; the clamps keep broken ones from reading outside the arrays
    long lo = a.lo[i], hi = a.hi[i];
    lo = lo < 0 ? 0 : lo;
    hi = hi > a.nwno ? a.nwno : hi;
    const double c = a.centre[i], den = a.den[i];
    double s = 0.0, n[PICASO_REGRID_MAX_ROWS];
#pragma unroll
    for (int r = 0; r < PICASO_REGRID_MAX_ROWS; ++r) n[r] = 0.0;
    for (long k = lo + t; k < hi; k += CONV_THREADS) {
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
            if (r < a.nrows) n[r] = fma(regrid_elem(a.rows[r], k), g, n[r]);
    }
    s = wave_sum(s);
#pragma unroll
    for (int r = 0; r < PICASO_REGRID_MAX_ROWS; ++r)
        if (r < a.nrows) n[r] = wave_sum(n[r]);
    if ((t & 63) == 0) {
        part[wave][PICASO_REGRID_MAX_ROWS] = s;
#pragma unroll
        for (int r = 0; r < PICASO_REGRID_MAX_ROWS; ++r)
            if (r < a.nrows) part[wave][r] = n[r];
    }
    __syncthreads();
    if (t < a.nrows) {
        double st = 0.0, nt = 0.0;
        for (int w = 0; w < CONV_WAVES; ++w) {
            st = st + part[w][PICASO_REGRID_MAX_ROWS];
            nt = nt + part[w][t];
        }
        a.out[(long)t * a.nobs + i] = nt / st;      // no weight in the window: 0 / 0 = NaN, as the reference
    }
}

}  // namespace pz

using namespace pz;

extern "C" int picaso_lsf_convolve_dev(picaso_ctx *ctx, long nwno, const double *wl, int nobs, const double *centre,
                                       const double *den, const int *lo, const int *hi, int nrows,
                                       const picaso_regrid_row *rows, double *out)
{
    if (!ctx || !wl || !centre || !den || !lo || !hi || !rows || !out)
        return fail(ctx, "picaso_lsf_convolve_dev: null argument");
    if (nwno < 1 || nwno > 0x7fffffffL)
        return fail(ctx, "picaso_lsf_convolve_dev: nwno must be in [1, 2^31 - 1] (32-bit window offsets), got %ld", nwno);
    if (nobs <= 0) return fail(ctx, "picaso_lsf_convolve_dev: nobs must be positive, got %d", nobs);
    LsfConvolveArgs a{};
    PZ_TRY(regrid_rows_check(ctx, "picaso_lsf_convolve_dev", nrows, rows, a.rows));
    a.nwno = nwno;
    a.nobs = nobs;
    a.nrows = nrows;
    a.wl = wl;
    a.centre = centre;
    a.den = den;
    a.lo = lo;
    a.hi = hi;
    a.out = out;
    PZ_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_lsf_convolve, dim3((unsigned)nobs), dim3(CONV_THREADS), 0, ctx->stream, a);
    PZ_HIP(ctx, hipGetLastError());
    return 0;
}
