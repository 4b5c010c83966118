// Correlated-k coefficients of one P-T point from its line-by-line cross sections (reference opacity_factory.py:1927-1955,
// the bin loop of compute_ck_molecular).  For every output bin the reference takes the points of the row that fall in it,
// clamps values <= 0 to 1e-200, sorts their logarithms and reads the sorted curve at the Gauss abscissae g with np.interp on
// x[j] = j / (n - 1.):
//
//     k[bin][i] = ((d[j+1] - d[j]) / (x[j+1] - x[j])) * (g[i] - x[j]) + d[j],   x[j] <= g[i] < x[j+1],   d = ln(sorted values)
//
// ln is monotone, so the values are ordered RAW and only the two order statistics at j and j + 1 of every Gauss point meet
// the logarithm: 2 ngauss logs per bin, not n.  After the clamp every value is positive, so the 64-bit patterns order as
// unsigned integers and both paths work on the patterns (+inf, 0x7ff0..., is the largest and pads the sorting network).
//
// A bin is a segment [lo, lo + n) of the row, found on the host (picaso_amd/opacity_factory.py: ck_segments); segments may
// overlap, be empty and come in any order.  One workgroup of 1 024 threads per bin, two kernels, chosen per segment:
//
//   n <= lds_cap   k_ck_sort_lds: the segment is loaded into LDS (clamped, padded with +inf to a power of two P >= n), sorted
//                  there by a bitonic network of P elements (log2 P (log2 P + 1) / 2 barrier-separated stages), and the order
//                  statistics are read off.  The LDS array holds 16 384 patterns = 128 KiB of the CU's 160 KiB: the default
//                  and largest lds_cap.
//   n >  lds_cap   k_ck_select_hbm: radix multi-select.  The segment stays in HBM and is read eight times, once per 8-bit
//                  digit from the most significant down.  All 2 ngauss ranks are narrowed together: the ranks are grouped by
//                  the prefix decided so far (ranks j and j + 1, and neighbouring Gauss points of a smooth curve, share it for
//                  most passes), every group has a 256-bin histogram in LDS (plain LDS atomic adds, 64-bit counts), an element
//                  is counted in the one group whose prefix it matches, and after the pass every rank walks its group's
//                  histogram to its digit.  After eight passes a rank's prefix IS its order statistic, bit for bit, at any
//                  n: there is no scratch copy and no limit on n but the row's.
//
// Both kernels hand the same two patterns per Gauss point to the same finish (ckf_finish): results do not depend on the path.
// A NaN in a used segment is reported, not sorted around: the thread that loads it lowers a flag word to its bin index with a
// plain atomicMin; the entry point reads the word back and fails, naming the bin.
#include "common.hpp"
#include "device_math.hpp"

namespace pz {

constexpr int CKF_THREADS = 1024;
constexpr int CKF_LDS_CAP = 16384;              // patterns in LDS: 128 KiB of 160 KiB per CU
constexpr int CKF_MAXR = 2 * MAX_CK_GAUSS;      // ranks per bin
constexpr unsigned long long CKF_INF = 0x7ff0000000000000ull;
constexpr int CKF_NO_NAN = 0x7f7f7f7f;          // the flag word after hipMemset(0x7f)
constexpr size_t CKF_MAX_BINS = picaso_ctx::SLOT_BYTES / (2 * sizeof(long long));      // lo and n share one table slot

struct CkFactoryArgs {
    const double *xsec;                         // (n_lbl)
    const long long *lo, *n;                    // (nbins), checked on the host: 0 <= lo, 0 <= n, lo + n <= n_lbl
    const double *g;                            // (ngauss), each inside (0, 1)
    int nbins, ngauss;
    long long cap;                              // 1 <= cap <= CKF_LDS_CAP
    double *k, *stats;                          // (nbins, ngauss), (nbins, ngauss, 2) or nullptr
    int *nanbin;
};

// the reference's clamp (linelist[linelist <= 0.0] = 1e-200; -0.0 <= 0.0 holds) and the pattern of the result
__device__ __forceinline__ unsigned long long ckf_key(double v, bool &nan)
{
    nan = nan || (v != v);
    if (v <= 0.0) v = 1e-200;
    return (unsigned long long)__double_as_longlong(v);
}

// np.interp's bracket on x[j] = j / (n - 1.): the j in [0, n - 2] with x[j] <= g < x[j+1] (n >= 2, 0 < g < 1), the
// quotients formed as numpy forms them (int64 -> double, a correctly rounded division).  floor(g (n - 1)) is off by at most
// one step either way.
__device__ __forceinline__ long long ckf_bracket(long long n, double g, double &x0, double &x1)
{
    const double nm1 = (double)n - 1.;
    long long j = (long long)(g * nm1);
    j = j > n - 2 ? n - 2 : (j < 0 ? 0 : j);
    while (j > 0 && (double)j / nm1 > g) --j;
    while (j < n - 2 && (double)(j + 1) / nm1 <= g) ++j;
    x0 = (double)j / nm1;
    x1 = (double)(j + 1) / nm1;
    return j;
}

// numpy's arr_interp between the two knots, operation for operation: a knot hit returns the knot; otherwise the slope, a
// separate multiply and add, and the NaN retry from the other side (+inf order statistics).
__device__ __forceinline__ double ckf_finish(double g, double x0, double x1, unsigned long long a, unsigned long long b)
{
#pragma clang fp contract(off)
    const double y0 = log(__longlong_as_double((long long)a)), y1 = log(__longlong_as_double((long long)b));
    if (x0 == g) return y0;
    const double slope = sub_unfused(y1, y0) / sub_unfused(x1, x0);
    double v = mul_unfused(slope, sub_unfused(g, x0)) + y0;
    if (v != v) {
        v = mul_unfused(slope, sub_unfused(g, x1)) + y1;
        if (v != v && y0 == y1) v = y0;
    }
    return v;
}

__device__ __forceinline__ void ckf_store(const CkFactoryArgs &a, int bin, int i, double k, unsigned long long s0,
                                          unsigned long long s1)
{
    const long o = (long)bin * a.ngauss + i;
    a.k[o] = k;
    if (a.stats) {
        a.stats[2 * o] = __longlong_as_double((long long)s0);
        a.stats[2 * o + 1] = __longlong_as_double((long long)s1);
    }
}

// n == 0: the reference sorts ten -200s; n == 1: it adds -200 to the zero it started from
__device__ __forceinline__ void ckf_store_empty(const CkFactoryArgs &a, int bin, int i)
{
    const unsigned long long floor_bits = (unsigned long long)__double_as_longlong(1e-200);
    ckf_store(a, bin, i, -200.0, floor_bits, floor_bits);
}

__global__ __launch_bounds__(CKF_THREADS) void k_ck_sort_lds(const CkFactoryArgs a)
{
    __shared__ unsigned long long s[CKF_LDS_CAP];
    const int bin = blockIdx.x, t = threadIdx.x;
    const long long lo = a.lo[bin], n = a.n[bin];
    if (n > a.cap) return;                              // k_ck_select_hbm's
    bool nan = false;
    if (n < 2) {
        if (n == 1 && t == 0) (void)ckf_key(a.xsec[lo], nan);
        if (nan) atomicMin(a.nanbin, bin);
        if (t < a.ngauss) ckf_store_empty(a, bin, t);
        return;
    }
    int P = 2;
    while (P < n) P <<= 1;                              // n <= cap <= CKF_LDS_CAP, a power of two
    for (int i = t; i < P; i += CKF_THREADS) s[i] = i < n ? ckf_key(a.xsec[lo + i], nan) : CKF_INF;
    if (nan) atomicMin(a.nanbin, bin);
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < P; i += CKF_THREADS) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long u = s[i], v = s[l];
                    if ((u > v) == ((i & k) == 0)) {
                        s[i] = v;
                        s[l] = u;
                    }
                }
            }
            __syncthreads();
        }
    if (t < a.ngauss) {
        const double g = a.g[t];
        double x0, x1;
        const long long j = ckf_bracket(n, g, x0, x1);
        const unsigned long long s0 = s[j], s1 = s[j + 1];
        ckf_store(a, bin, t, ckf_finish(g, x0, x1, s0, s1), s0, s1);
    }
}

__global__ __launch_bounds__(CKF_THREADS) void k_ck_select_hbm(const CkFactoryArgs a)
{
    __shared__ unsigned long long hist[CKF_MAXR][256];
    __shared__ unsigned long long gp[CKF_MAXR];         // the groups' prefixes (digits above the current one)
    __shared__ unsigned long long pre[CKF_MAXR];        // the ranks' prefixes
    __shared__ unsigned long long kk[CKF_MAXR];         // a rank's index among the elements that match its prefix
    __shared__ int grp[CKF_MAXR];
    __shared__ int ngroups;
    const int bin = blockIdx.x, t = threadIdx.x;
    const long long lo = a.lo[bin], n = a.n[bin];
    if (n <= a.cap) return;                             // k_ck_sort_lds's; here n > cap >= 1, so n >= 2
    const int R = 2 * a.ngauss;
    double g = 0.0, x0 = 0.0, x1 = 0.0;
    if (t < a.ngauss) {
        g = a.g[t];
        const long long j = ckf_bracket(n, g, x0, x1);
        kk[2 * t] = (unsigned long long)j;
        kk[2 * t + 1] = (unsigned long long)(j + 1);
    }
    if (t < R) {
        pre[t] = 0;
        grp[t] = 0;
    }
    if (t == 0) {
        gp[0] = 0;
        ngroups = 1;
    }
    __syncthreads();
    bool nan = false;
    for (int shift = 56; shift >= 0; shift -= 8) {
        const int G = ngroups;
        for (int i = t; i < G * 256; i += CKF_THREADS) hist[i >> 8][i & 255] = 0;
        __syncthreads();
        const int hs = shift + 8;                       // the decided digits: bits hs and above (none in the first pass)
        for (long long i = t; i < n; i += CKF_THREADS) {
            const unsigned long long u = ckf_key(a.xsec[lo + i], nan);
            for (int q = 0; q < G; ++q)
                if (hs >= 64 || ((u ^ gp[q]) >> hs) == 0) {
                    atomicAdd(&hist[q][(u >> shift) & 255], 1ull);
                    break;                              // the groups' prefixes are distinct
                }
        }
        __syncthreads();
        if (t < R) {
            const int q = grp[t];
            unsigned long long k = kk[t], cum = 0;
            int d = 0;
            for (; d < 255; ++d) {
                const unsigned long long h = hist[q][d];
                if (k < cum + h) break;
                cum += h;
            }
            kk[t] = k - cum;
            pre[t] = gp[q] | ((unsigned long long)d << shift);
        }
        __syncthreads();
        if (t == 0) {
            int G2 = 0;
            for (int r = 0; r < R; ++r) {
                int q = 0;
                while (q < G2 && gp[q] != pre[r]) ++q;
                if (q == G2) gp[G2++] = pre[r];
                grp[r] = q;
            }
            ngroups = G2;
        }
        __syncthreads();
    }
    if (nan) atomicMin(a.nanbin, bin);
    if (t < a.ngauss) {
        const unsigned long long s0 = pre[2 * t], s1 = pre[2 * t + 1];
        ckf_store(a, bin, t, ckf_finish(g, x0, x1, s0, s1), s0, s1);
    }
}

}  // namespace pz

using namespace pz;

extern "C" int picaso_ck_from_xsec_dev(picaso_ctx *ctx, long n_lbl, const double *xsec, int nbins, const long long *lo,
                                       const long long *n, int ngauss, const double *g, long lds_cap, double *k,
                                       double *stats)
{
    if (!ctx) return fail(nullptr, "picaso_ck_from_xsec_dev: null context");
    PZ_NEED(ctx, "picaso_ck_from_xsec_dev", xsec, lo, n, g, k);
    if (n_lbl < 1) return fail(ctx, "picaso_ck_from_xsec_dev: n_lbl must be positive, got %ld", n_lbl);
    if (nbins < 0) return fail(ctx, "picaso_ck_from_xsec_dev: nbins must not be negative, got %d", nbins);
    if ((size_t)nbins > CKF_MAX_BINS)
        return fail(ctx, "picaso_ck_from_xsec_dev: %d bins; one call takes at most %zu (their offsets and counts travel in one "
                         "%zu-byte table slot): split the grid", nbins, CKF_MAX_BINS, (size_t)picaso_ctx::SLOT_BYTES);
    if (ngauss < 1 || ngauss > MAX_CK_GAUSS)
        return fail(ctx, "picaso_ck_from_xsec_dev: ngauss must be in [1, %d], got %d", MAX_CK_GAUSS, ngauss);
    if (lds_cap < 0 || lds_cap > CKF_LDS_CAP)
        return fail(ctx, "picaso_ck_from_xsec_dev: lds_cap must be in [0, %d] (0: the default, %d), got %ld", CKF_LDS_CAP,
                    CKF_LDS_CAP, lds_cap);
    for (int i = 0; i < ngauss; ++i)
        if (!(g[i] > 0.0 && g[i] < 1.0))
            return fail(ctx, "picaso_ck_from_xsec_dev: g[%d] = %g lies outside (0, 1)", i, g[i]);
    bool any_short = false, any_long = false;
    const long long cap = lds_cap ? lds_cap : CKF_LDS_CAP;
    for (int b = 0; b < nbins; ++b) {
        if (n[b] < 0) return fail(ctx, "picaso_ck_from_xsec_dev: bin %d has a negative count (%lld)", b, n[b]);
        if (lo[b] < 0 || lo[b] > n_lbl || n[b] > n_lbl - lo[b])
            return fail(ctx, "picaso_ck_from_xsec_dev: bin %d, [%lld, %lld + %lld), lies outside the row of %ld points", b,
                        lo[b], lo[b], n[b], n_lbl);
        (n[b] > cap ? any_long : any_short) = true;
    }
    if (nbins == 0) return 0;
    PZ_HIP(ctx, hipSetDevice(ctx->device));
    CkFactoryArgs a{};
    std::vector<long long> seg(2 * (size_t)nbins);
    memcpy(seg.data(), lo, sizeof(long long) * nbins);
    memcpy(seg.data() + nbins, n, sizeof(long long) * nbins);
    const void *d_seg = nullptr, *d_g = nullptr;
    PZ_TRY(table_upload(ctx, seg.data(), seg.size() * sizeof(long long), &d_seg));
    PZ_TRY(table_upload(ctx, g, sizeof(double) * ngauss, &d_g));
    void *d_flag = nullptr;
    PZ_TRY(picaso_dev_malloc(ctx, sizeof(int), &d_flag));
    a.xsec = xsec;
    a.lo = static_cast<const long long *>(d_seg);
    a.n = a.lo + nbins;
    a.g = static_cast<const double *>(d_g);
    a.nbins = nbins;
    a.ngauss = ngauss;
    a.cap = cap;
    a.k = k;
    a.stats = stats;
    a.nanbin = static_cast<int *>(d_flag);
    int found = CKF_NO_NAN;
    auto run = [&]() -> int {
        PZ_HIP(ctx, hipMemsetAsync(d_flag, 0x7f, sizeof(int), ctx->stream));
        if (any_short) {
            hipLaunchKernelGGL(k_ck_sort_lds, dim3((unsigned)nbins), dim3(CKF_THREADS), 0, ctx->stream, a);
            PZ_HIP(ctx, hipGetLastError());
        }
        if (any_long) {
            hipLaunchKernelGGL(k_ck_select_hbm, dim3((unsigned)nbins), dim3(CKF_THREADS), 0, ctx->stream, a);
            PZ_HIP(ctx, hipGetLastError());
        }
        PZ_HIP(ctx, hipMemcpyAsync(&found, d_flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        PZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return 0;
    };
    const int rc = run();
    (void)picaso_dev_free(ctx, d_flag);
    if (rc != 0) return rc;
    if (found != CKF_NO_NAN)
        return fail(ctx, "picaso_ck_from_xsec_dev: NaN in the cross sections of bin %d (points [%lld, %lld) of the row)",
                    found, lo[found], lo[found] + n[found]);
    return 0;
}
