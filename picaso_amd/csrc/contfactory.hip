// The rows of an opacity database (reference opacity_factory.py:280-362 restructure_opacity, :850-1055 insert_molecular_1460).
//
// CONTINUUM.  For every temperature of the CIA file the reference interpolates each pair's log10 opacity onto the new grid,
// patches H2H2 (the 0.8 micron overtone table, the Linsky / Lenzuni fill of the -33 placeholders above 1000 cm-1, a median
// filter over 9950-11200 cm-1 where the fill met the data) and appends three rows that are functions of the wavenumber and
// the temperature alone: H2- (Bell 1980), H- bound-free (John 1988), H- free-free (Bell & Berrington 1987).  Here:
//
//   k_cont_rows            one thread per (temperature, wavenumber): all nmol + 3 species of the point.  np.interp's bracket,
//                          knot rule and fills (interp.hpp), then 10**x; the arithmetic of every source in numpy's operation
//                          order with contraction off.  Everything that depends on the temperature alone (the nearest overtone
//                          column and Bell row, Linsky's d, a, b, aa, t_coeff**((i+1)/2), the constant rows) is formed on the
//                          host in numpy and read from a table of CONT_NPAR doubles per temperature: the arguments of exp are
//                          the reference's bits, only the transcendental differs.  A temperature whose H2H2 row takes a Linsky
//                          point below 12000 cm-1 raises flags[t]: that row is smoothed.
//   k_cont_medfilt_lds     scipy.signal.medfilt of the region [lo, lo + n) of a flagged H2H2 row, window W (odd), zeros beyond
//   k_cont_medfilt_select  the region's ends.  The region is first copied aside (the filter is out of place); one workgroup
//                          per output point takes the order statistic W / 2 of its window: a bitonic sort of the keys in LDS
//                          while W <= lds_cap, a radix select (eight 8-bit digits, the window read from the copy once per
//                          digit) beyond.  The keys are the bit patterns made monotone (sign bit flipped for values >= 0, all
//                          bits for negative ones), so the median is one of the window's values, bit for bit, on both paths.
//
// MOLECULAR.  k_xsec_resample is np.interp(out_grid, src_grid, src, left, right) followed by the reference's floor
// (dset[dset < 1e-100] = 1e-100), for the every-BINS-th points of the reference's hi-res grid.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

#include "common.hpp"
#include "device_math.hpp"
#include "interp.hpp"

namespace pz {

constexpr int CONT_THREADS = 256;
constexpr int CONT_NPAR = 24;                   // doubles per temperature: picaso_amd/opacity_factory.py: _continuum_params
constexpr long CONT_LDS_CAP = 8192;             // keys in LDS: 64 KiB

enum ContPar {
    CP_OV_ADD = 0, CP_LIN_D, CP_LIN_A, CP_LIN_B, CP_LIN_AA, CP_LIN_W, CP_LIN_LIM, CP_T, CP_H2M_ON, CP_H2M_CONST, CP_HBF_ON,
    CP_HBF_CONST, CP_HFF_ON, CP_HFF_CONST, CP_TC0, CP_P33 = CP_TC0 + 6, CP_HBF_EDGE, CP_INV_L0, CP_LINSKY_ON
};
static_assert(CP_LINSKY_ON < CONT_NPAR, "the parameter table is too short");

struct ContRowsArgs {
    int ntemp, nmol, h2h2, nov, nbell;
    long nold, nwno;
    const double *old_wno, *log_opa, *new_wno, *ov_wno, *ov_log, *bell_wno, *bell_kappa, *par;
    double *out;
    int *flags;
};

struct ContMedArgs {
    int nsp, h2h2;
    long nwno, lo, n, window;
    const double *copy;                         // (ntemp, n): the region of every H2H2 row before the filter
    const int *flags;
    double *out;
};

// 10**x as csrc/cheminterp.hip's chem_exp10 forms it (the same operations: within 4 ulp of numpy's 10.0**x for |x| <= 300)
__device__ __forceinline__ double cont_exp10(double x)
{
#pragma clang fp contract(off)
    constexpr double L2_10_HI = 0x1.a934f0979a371p+1;
    constexpr double L2_10_LO = 0x1.7f2495fb7fa6dp-53;
    constexpr double LN2 = 0.6931471805599453;
    const double inf = __builtin_inf();
    if (x == inf) return inf;
    if (x == -inf) return 0.0;
    const double y = x * L2_10_HI;
    double e = fma(x, L2_10_HI, -y);
    e = fma(x, L2_10_LO, e);
    const double p = fexp2(y);
    return (p == inf) ? p : fma(p, e * LN2, p);
}

// 10**x of a log10 opacity; the placeholder -33 becomes the host's own 10**-33.0, so that the reference's test
// `new_bundle == 1e-33` is decided by numpy's pow, not by the device's
__device__ __forceinline__ double cont_pow10(double x, double p33) { return x == -33.0 ? p33 : cont_exp10(x); }

// Linsky (1969) / Lenzuni et al. (1991), the reference's fit_linsky at va = 3.  Its middle branch (wno < w) is always
// overwritten by the last one (wno < w + 1.5 d), so two branches are live: a rational one without a transcendental, and
// aa wno exp(-(wno - w) / b).
__device__ __forceinline__ double cont_linsky(const double *p, double wno)
{
#pragma clang fp contract(off)
    const double d = p[CP_LIN_D], a = p[CP_LIN_A], w = p[CP_LIN_W];
    if (wno < p[CP_LIN_LIM]) return a * d * wno / ((wno - w) * (wno - w) + d * d);
    return p[CP_LIN_AA] * wno * fexp(-(wno - w) / p[CP_LIN_B]);
}

// John (1988), the reference's get_hminusbf: Horner in x = sqrt(1 / wave - 1 / lambda_0) with separate products and sums
__device__ __forceinline__ double cont_hminus_bf(const double *p, double wno)
{
#pragma clang fp contract(off)
    if (!(wno > p[CP_HBF_EDGE])) return 1e-33;
    const double wave = 1e4 / wno;
    const double x = sqrt(1.0 / wave - p[CP_INV_L0]);
    const double coeff[6] = {4.982, -34.194, 92.536, -118.858, 49.534, 152.519};
    double f = 0.0;
    for (int i = 0; i < 6; ++i) f = f * x + coeff[i];
    const double y = wave * x;
    return y * y * y * f * 1e-18;               // numpy's (wave x)**3 goes through pow: DESIGN section 5q
}

// Bell & Berrington (1987), the reference's get_hminusff for t >= 800
__device__ __forceinline__ double cont_hminus_ff(const double *p, double wno)
{
#pragma clang fp contract(off)
    const double AJ1[6] = {0.e0, 2483.346, -3449.889, 2200.040, -696.271, 88.283};
    const double BJ1[6] = {0.e0, 285.827, -1158.382, 2427.719, -1841.400, 444.517};
    const double CJ1[6] = {0.e0, -2054.291, 8746.523, -13651.105, 8624.970, -1863.864};
    const double DJ1[6] = {0.e0, 2827.776, -11485.632, 16755.524, -10051.530, 2095.288};
    const double EJ1[6] = {0.e0, -1341.537, 5303.609, -7510.494, 4400.067, -901.788};
    const double FJ1[6] = {0.e0, 208.952, -812.939, 1132.738, -655.020, 132.985};
    const double AJ2[6] = {518.1021, 473.2636, -482.2089, 115.5291, 0.0, 0.0};
    const double BJ2[6] = {-734.8666, 1443.4137, -737.1616, 169.6374, 0.0, 0.0};
    const double CJ2[6] = {1021.1775, -1977.3395, 1096.8827, -245.649, 0.0, 0.0};
    const double DJ2[6] = {-479.0721, 922.3575, -521.1341, 114.243, 0.0, 0.0};
    const double EJ2[6] = {93.1373, -178.9275, 101.7963, -21.9972, 0.0, 0.0};
    const double FJ2[6] = {-6.4285, 12.3600, -7.0571, 1.5097, 0.0, 0.0};
    double wave = 1e4 / wno;
    const bool longw = wave > 0.3645, midw = wave <= 0.3645;
    if (wave < 0.1823) wave = 0.1823;
    double hm = 0.0;
    for (int i = 0; i < 6; ++i) {
        double hj = 0.0;
        if (longw)
            hj = 1e-29 * (wave * wave * AJ1[i] + BJ1[i] + (CJ1[i] + (DJ1[i] + (EJ1[i] + FJ1[i] / wave) / wave) / wave) / wave);
        else if (midw)
            hj = 1e-29 * (wave * wave * AJ2[i] + BJ2[i] + (CJ2[i] + (DJ2[i] + (EJ2[i] + FJ2[i] / wave) / wave) / wave) / wave);
        hm = hm + p[CP_TC0 + i] * hj;
    }
    if (wave > 20.0) hm = 0.0;
    return hm * 1.380658e-16 * p[CP_T];
}

__global__ __launch_bounds__(CONT_THREADS) void k_cont_rows(const ContRowsArgs a)
{
#pragma clang fp contract(off)
    const int t = blockIdx.y;
    const long j = (long)blockIdx.x * CONT_THREADS + threadIdx.x;
    const double *p = a.par + (long)t * CONT_NPAR;
    const int nsp = a.nmol + 3;
    bool linsky_low = false;
    if (j < a.nwno) {
        const double w = a.new_wno[j];
        const double p33 = p[CP_P33];
        double *out = a.out + (long)t * nsp * a.nwno + j;
        const RegridBracket b = regrid_bracket(a.old_wno, (int)a.nold, w);
        for (int m = 0; m < a.nmol; ++m) {
            const double *row = a.log_opa + ((long)t * a.nmol + m) * a.nold;
            double v = cont_pow10(regrid_value(row, b, (int)a.nold, -33.0, -33.0), p33);
            if (m == a.h2h2) {
                if (p[CP_OV_ADD] != 0.0 && w >= a.ov_wno[0] && w <= a.ov_wno[a.nov - 1]) {
                    const RegridBracket bo = regrid_bracket(a.ov_wno, a.nov, w);
                    v = cont_pow10(regrid_value(a.ov_log + (long)t * a.nov, bo), p33);
                }
                if (p[CP_LINSKY_ON] != 0.0 && v == 1e-33 && w >= 1000.0) {
                    v = cont_linsky(p, w);
                    linsky_low = linsky_low || (w < 12000.0);
                }
            }
            out[(long)m * a.nwno] = v;
        }
        double h2m = p[CP_H2M_CONST];
        if (p[CP_H2M_ON] != 0.0) {
            const RegridBracket bb = regrid_bracket(a.bell_wno, a.nbell, w);
            h2m = regrid_value(a.bell_kappa + (long)t * a.nbell, bb, a.nbell, 1e-33, 1e-33);
        }
        out[(long)a.nmol * a.nwno] = h2m;
        out[(long)(a.nmol + 1) * a.nwno] = p[CP_HBF_ON] != 0.0 ? cont_hminus_bf(p, w) : p[CP_HBF_CONST];
        out[(long)(a.nmol + 2) * a.nwno] = p[CP_HFF_ON] != 0.0 ? cont_hminus_ff(p, w) : p[CP_HFF_CONST];
    }
    if (__syncthreads_or(linsky_low ? 1 : 0) && threadIdx.x == 0) atomicOr(&a.flags[t], 1);
}

// a double's bit pattern made monotone: keys compare as unsigned integers the way the values compare (-0.0 below +0.0, a
// NaN with a clear sign bit above +inf)
__device__ __forceinline__ unsigned long long cont_key(double v)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ double cont_unkey(unsigned long long k)
{
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

// element i of the window of output point k: zeros beyond the region's ends, as medfilt pads
__device__ __forceinline__ unsigned long long cont_window_key(const double *r, long n, long k, long h, long i)
{
    const long idx = k - h + i;
    return cont_key(idx >= 0 && idx < n ? r[idx] : 0.0);
}

__global__ __launch_bounds__(CONT_THREADS) void k_cont_medfilt_lds(const ContMedArgs a)
{
    extern __shared__ unsigned long long cont_s[];
    const int t = blockIdx.y, tid = threadIdx.x;
    const long k = blockIdx.x;
    if (!a.flags[t]) return;
    const double *r = a.copy + (long)t * a.n;
    const long W = a.window, h = W >> 1;
    int P = 2;
    while (P < W) P <<= 1;                              // W <= lds_cap <= CONT_LDS_CAP, a power of two
    for (int i = tid; i < P; i += CONT_THREADS) cont_s[i] = i < W ? cont_window_key(r, a.n, k, h, i) : ~0ull;
    __syncthreads();
    for (int kk = 2; kk <= P; kk <<= 1)
        for (int jj = kk >> 1; jj > 0; jj >>= 1) {
            for (int i = tid; i < P; i += CONT_THREADS) {
                const int l = i ^ jj;
                if (l > i) {
                    const unsigned long long u = cont_s[i], v = cont_s[l];
                    if ((u > v) == ((i & kk) == 0)) {
                        cont_s[i] = v;
                        cont_s[l] = u;
                    }
                }
            }
            __syncthreads();
        }
    if (tid == 0) a.out[((long)t * a.nsp + a.h2h2) * a.nwno + a.lo + k] = cont_unkey(cont_s[h]);
}

__global__ __launch_bounds__(CONT_THREADS) void k_cont_medfilt_select(const ContMedArgs a)
{
    __shared__ unsigned int hist[256];
    __shared__ unsigned long long prefix;
    __shared__ unsigned int rank;
    const int t = blockIdx.y, tid = threadIdx.x;
    const long k = blockIdx.x;
    if (!a.flags[t]) return;
    const double *r = a.copy + (long)t * a.n;
    const long W = a.window, h = W >> 1;               // W <= INT_MAX: the counts fit 32 bits
    if (tid == 0) {
        prefix = 0;
        rank = (unsigned int)h;
    }
    for (int shift = 56; shift >= 0; shift -= 8) {
        hist[tid] = 0;                                  // CONT_THREADS == 256
        __syncthreads();
        const unsigned long long pre = prefix;
        const int hs = shift + 8;                       // the decided digits: bits hs and above (none in the first pass)
        for (long i = tid; i < W; i += CONT_THREADS) {
            const unsigned long long u = cont_window_key(r, a.n, k, h, i);
            if (hs >= 64 || ((u ^ pre) >> hs) == 0) atomicAdd(&hist[(u >> shift) & 255], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned int kk = rank, cum = 0;
            int d = 0;
            for (; d < 255; ++d) {
                const unsigned int c = hist[d];
                if (kk < cum + c) break;
                cum += c;
            }
            rank = kk - cum;
            prefix = pre | ((unsigned long long)d << shift);
        }
        __syncthreads();
    }
    if (tid == 0) a.out[((long)t * a.nsp + a.h2h2) * a.nwno + a.lo + k] = cont_unkey(prefix);
}

struct XsecResampleArgs {
    long n_out, n_src;
    double *out;
    const double *src, *src_grid, *out_grid;
    double guess_start, guess_step, left, right, floor;
};

__global__ __launch_bounds__(CONT_THREADS) void k_xsec_resample(const XsecResampleArgs a)
{
    const long stride = (long)gridDim.x * CONT_THREADS;
    for (long j = (long)blockIdx.x * CONT_THREADS + threadIdx.x; j < a.n_out; j += stride) {
        const RegridBracket b = regrid_bracket_guess(a.src_grid, (int)a.n_src, a.out_grid[j], a.guess_start, a.guess_step);
        double v = regrid_value(a.src, b, (int)a.n_src, a.left, a.right);
        if (v < a.floor) v = a.floor;                   // a NaN stays, as in dset[dset < 1e-100] = 1e-100
        a.out[j] = v;
    }
}

}  // namespace pz

using namespace pz;

extern "C" int picaso_continuum_npar(void) { return CONT_NPAR; }

extern "C" int picaso_continuum_rows_dev(picaso_ctx *ctx, int ntemp, int nmol, int h2h2, long nold, const double *old_wno,
                                         const double *log_opa, long nwno, const double *new_wno, int nov,
                                         const double *ov_wno, const double *ov_log, int nbell, const double *bell_wno,
                                         const double *bell_kappa, const double *par, long smooth_lo, long smooth_n,
                                         long window, long lds_cap, int smooth, double *work, double *out)
{
    const char *who = "picaso_continuum_rows_dev";
    if (!ctx) return fail(nullptr, "%s: null context", who);
    PZ_NEED(ctx, who, old_wno, log_opa, new_wno, ov_wno, ov_log, bell_wno, bell_kappa, par, work, out);
    if (ntemp < 1 || ntemp > 65535) return fail(ctx, "%s: ntemp must be in [1, 65535] per call, got %d", who, ntemp);
    if (nmol < 1) return fail(ctx, "%s: nmol must be positive, got %d", who, nmol);
    if (h2h2 < -1 || h2h2 >= nmol)
        return fail(ctx, "%s: h2h2 must be the index of the H2H2 row in [0, %d), or -1 for none, got %d", who, nmol, h2h2);
    if (nold < 1 || nold > (long)INT_MAX || nwno < 1 || nwno > (long)INT_MAX)
        return fail(ctx, "%s: nold (%ld) and nwno (%ld) must be in [1, %d]", who, nold, nwno, INT_MAX);
    if (nov < 1 || nbell < 1) return fail(ctx, "%s: the overtone (%d) and Bell (%d) tables need at least one knot", who, nov, nbell);
    if (window < 1 || !(window & 1) || window > (long)INT_MAX)
        return fail(ctx, "%s: the window must be odd and in [1, %d], got %ld", who, INT_MAX, window);
    if (smooth_lo < 0 || smooth_n < 0 || smooth_lo > nwno || smooth_n > nwno - smooth_lo)
        return fail(ctx, "%s: the smoothing region [%ld, %ld + %ld) lies outside the row of %ld points", who, smooth_lo,
                    smooth_lo, smooth_n, nwno);
    if (lds_cap < 0 || lds_cap > CONT_LDS_CAP)
        return fail(ctx, "%s: lds_cap must be in [0, %ld] (0: the default, %ld), got %ld", who, CONT_LDS_CAP, CONT_LDS_CAP,
                    lds_cap);
    PZ_HIP(ctx, hipSetDevice(ctx->device));
    const int nsp = nmol + 3;
    int *flags = reinterpret_cast<int *>(work + (size_t)ntemp * (size_t)smooth_n);
    PZ_HIP(ctx, hipMemsetAsync(flags, 0, sizeof(double) * (size_t)ntemp, ctx->stream));
    ContRowsArgs a{};
    a.ntemp = ntemp;
    a.nmol = nmol;
    a.h2h2 = h2h2;
    a.nov = nov;
    a.nbell = nbell;
    a.nold = nold;
    a.nwno = nwno;
    a.old_wno = old_wno;
    a.log_opa = log_opa;
    a.new_wno = new_wno;
    a.ov_wno = ov_wno;
    a.ov_log = ov_log;
    a.bell_wno = bell_wno;
    a.bell_kappa = bell_kappa;
    a.par = par;
    a.out = out;
    a.flags = flags;
    const dim3 grid((unsigned)((nwno + CONT_THREADS - 1) / CONT_THREADS), (unsigned)ntemp);
    hipLaunchKernelGGL(k_cont_rows, grid, dim3(CONT_THREADS), 0, ctx->stream, a);
    PZ_HIP(ctx, hipGetLastError());
    if (!smooth || h2h2 < 0 || smooth_n == 0) return 0;
    PZ_HIP(ctx, hipMemcpy2DAsync(work, sizeof(double) * (size_t)smooth_n, out + (size_t)h2h2 * nwno + smooth_lo,
                                 sizeof(double) * (size_t)nsp * nwno, sizeof(double) * (size_t)smooth_n, (size_t)ntemp,
                                 hipMemcpyDeviceToDevice, ctx->stream));
    ContMedArgs m{};
    m.nsp = nsp;
    m.h2h2 = h2h2;
    m.nwno = nwno;
    m.lo = smooth_lo;
    m.n = smooth_n;
    m.window = window;
    m.copy = work;
    m.flags = flags;
    m.out = out;
    const long cap = lds_cap ? lds_cap : CONT_LDS_CAP;
    const dim3 mgrid((unsigned)smooth_n, (unsigned)ntemp);
    if (window <= cap) {
        size_t P = 2;
        while ((long)P < window) P <<= 1;
        hipLaunchKernelGGL(k_cont_medfilt_lds, mgrid, dim3(CONT_THREADS), P * sizeof(unsigned long long), ctx->stream, m);
    } else {
        hipLaunchKernelGGL(k_cont_medfilt_select, mgrid, dim3(CONT_THREADS), 0, ctx->stream, m);
    }
    PZ_HIP(ctx, hipGetLastError());
    return 0;
}

extern "C" int picaso_xsec_resample_dev(picaso_ctx *ctx, long n_out, double *out, const double *src, long n_src,
                                        const double *src_grid, const double *out_grid, double guess_start,
                                        double guess_step, double left, double right, double floor)
{
    const char *who = "picaso_xsec_resample_dev";
    if (!ctx) return fail(nullptr, "%s: null context", who);
    PZ_NEED(ctx, who, out, src, src_grid, out_grid);
    PZ_TRY(xsec_row_args(ctx, who, n_out, n_src, true, guess_start, &guess_step));
    PZ_HIP(ctx, hipSetDevice(ctx->device));
    XsecResampleArgs a{};
    a.n_out = n_out;
    a.n_src = n_src;
    a.out = out;
    a.src = src;
    a.src_grid = src_grid;
    a.out_grid = out_grid;
    a.guess_start = guess_start;
    a.guess_step = guess_step;
    a.left = left;
    a.right = right;
    a.floor = floor;
    const long blocks = std::min(2048l, (n_out + CONT_THREADS - 1) / CONT_THREADS);
    hipLaunchKernelGGL(k_xsec_resample, dim3((unsigned)blocks), dim3(CONT_THREADS), 0, ctx->stream, a);
    PZ_HIP(ctx, hipGetLastError());
    return 0;
}
