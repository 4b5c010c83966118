// Order statistics of every column of a resident (nsamp, ncol) matrix: the reduction behind a retrieval's prediction
// bands (reference retrieval.py:199-310, get_evaluations).  The reference reduces the stack of posterior draws through
// ultranest's PredictionBand.get_line(q) = scipy.stats.mstats.mquantiles(ys, q, axis=0)[0]: per column, with x the column
// in np.sort order and (k, gamma) the level's table entry (picaso_amd/retrieval.py: quantile_table, on the host),
//
//     out[i][c] = (1. - gamma[i]) * x[k[i] - 1] + gamma[i] * x[k[i]]        (nsamp == 1: x[0])
//
// two rounded products and one rounded addition, both products always formed (0 * inf is NaN, as in numpy).
//
// Keys.  np.sort orders -inf < finite < +inf < NaN, every NaN last whatever its sign.  A double maps to a 64-bit key that
// orders the same way as an unsigned integer: a non-negative value has its sign bit set, a negative one is inverted, and a
// NaN becomes the largest key, ~0.  The map is undone on the way out; ~0 reads back as 0x7fff..., a quiet NaN.  The same
// key pads a column to the sorting network's power of two P >= nsamp, so pads sort behind (or among) the NaNs of the data
// and no rank below nsamp ever reads one.  (-0.0 sorts before +0.0; they compare equal and numpy may leave them either
// way round, so results agree with numpy by value.)
//
// Tile.  A workgroup owns C adjacent columns and all nsamp rows.  The tile lives in LDS row-major, s[r * C + c]: a row
// segment is C * 8 contiguous bytes in HBM and in LDS.  C is the largest power of two <= 16 with P * C <= 16 384 keys
// (128 KiB of the CU's 160 KiB): 16 columns up to 1 024 draws, 8 up to 2 048, ... 1 column at 16 384.  The C columns are
// sorted concurrently by one bitonic network over the row index: a thread takes (pair of rows, column), the column
// fastest, so a wave's accesses are runs of C * 8 contiguous bytes.  Small tiles use a kernel with a smaller LDS array and
// fewer threads, so that several workgroups share a CU; the network and therefore the bits are the same.
//
// A column's result is a function of its own sorted keys: it depends neither on ncol, ld, its place in the tile, C nor
// the launch geometry.  y is read once and never written.
#include "common.hpp"
#include "device_math.hpp"

namespace pz {

constexpr int QT_LDS_KEYS = 16384;              // 128 KiB of 160 KiB per CU
constexpr int QT_MAX_C = 16;
constexpr unsigned long long QT_SIGN = 0x8000000000000000ull;
constexpr unsigned long long QT_NAN = ~0ull;    // every NaN, and the padding

struct QuantileArgs {
    const double *y;                            // (nsamp, ncol), row stride ld
    double *out;                                // (nq, ncol)
    long ncol, ld;
    int nsamp, nq;
    int P, logc;                                // padded rows (a power of two >= 2), log2 of the tile width
    int k[PICASO_BANDS_MAX_Q];
    double gamma[PICASO_BANDS_MAX_Q];
};

__device__ __forceinline__ unsigned long long qt_key(double v)
{
    if (v != v) return QT_NAN;
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u & QT_SIGN) ? ~u : (u | QT_SIGN);
}

__device__ __forceinline__ double qt_value(unsigned long long key)
{
    return __longlong_as_double((long long)((key & QT_SIGN) ? (key ^ QT_SIGN) : ~key));
}

// mquantiles' line, operation for operation
__device__ __forceinline__ double qt_finish(double gamma, double lo, double hi)
{
#pragma clang fp contract(off)
    const double a = mul_unfused(sub_unfused(1., gamma), lo), b = mul_unfused(gamma, hi);
    return a + b;
}

template <int KEYS, int THREADS>
__global__ __launch_bounds__(THREADS) void k_column_quantiles(const QuantileArgs a)
{
    __shared__ unsigned long long s[KEYS];
    const int t = threadIdx.x, logc = a.logc, C = 1 << logc, P = a.P;
    const long c0 = (long)blockIdx.x << logc;
    const int n = P << logc;                    // <= KEYS, chosen by the launcher
    for (int e = t; e < n; e += THREADS) {
        const int r = e >> logc, c = e & (C - 1);
        s[e] = (r < a.nsamp && c0 + c < a.ncol) ? qt_key(a.y[(long)r * a.ld + c0 + c]) : QT_NAN;
    }
    __syncthreads();
    const int half = n >> 1;
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int e = t; e < half; e += THREADS) {
                const int p = e >> logc, c = e & (C - 1);
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));      // the pair's row with bit j clear
                const int lo = (i << logc) + c, hi = ((i | j) << logc) + c;
                const unsigned long long u = s[lo], v = s[hi];
                if ((u > v) == ((i & k) == 0)) {
                    s[lo] = v;
                    s[hi] = u;
                }
            }
            __syncthreads();
        }
    for (int e = t; e < (a.nq << logc); e += THREADS) {
        const int i = e >> logc, c = e & (C - 1);
        if (c0 + c >= a.ncol) continue;
        double v;
        if (a.nsamp == 1) {
            v = qt_value(s[c]);
        } else {
            const int k = a.k[i];               // in [1, nsamp - 1], checked on the host
            v = qt_finish(a.gamma[i], qt_value(s[((k - 1) << logc) + c]), qt_value(s[(k << logc) + c]));
        }
        a.out[(long)i * a.ncol + c0 + c] = v;
    }
}

}  // namespace pz

using namespace pz;

extern "C" int picaso_column_quantiles_dev(picaso_ctx *ctx, int nsamp, long ncol, const double *y, long ld, int nq,
                                           const int *k, const double *gamma, double *out)
{
    const char *who = "picaso_column_quantiles_dev";
    if (!ctx) return fail(ctx, "%s: null context", who);
    PZ_NEED(ctx, who, y, k, gamma, out);
    if (nsamp < 1) return fail(ctx, "%s: the number of draws must be positive, got %d", who, nsamp);
    if (nsamp > PICASO_BANDS_MAX_DRAWS)
        return fail(ctx, "%s: %d draws; a column is sorted in LDS and takes at most PICASO_BANDS_MAX_DRAWS = %d", who, nsamp,
                    PICASO_BANDS_MAX_DRAWS);
    if (ncol < 1 || ncol > 0x7fffffffL) return fail(ctx, "%s: ncol must be in [1, 2^31 - 1], got %ld", who, ncol);
    if (ld < ncol) return fail(ctx, "%s: the row stride ld = %ld is shorter than a row of %ld columns", who, ld, ncol);
    if (nq < 1 || nq > PICASO_BANDS_MAX_Q)
        return fail(ctx, "%s: nq must be in [1, PICASO_BANDS_MAX_Q = %d], got %d", who, PICASO_BANDS_MAX_Q, nq);
    QuantileArgs a{};
    for (int i = 0; i < nq; ++i) {
        if (nsamp >= 2 && (k[i] < 1 || k[i] > nsamp - 1))
            return fail(ctx, "%s: k[%d] = %d lies outside [1, %d]", who, i, k[i], nsamp - 1);
        if (!(gamma[i] >= 0.0 && gamma[i] <= 1.0))
            return fail(ctx, "%s: gamma[%d] = %g lies outside [0, 1]", who, i, gamma[i]);
        a.k[i] = k[i];
        a.gamma[i] = gamma[i];
    }
    int P = 2;
    while (P < nsamp) P <<= 1;
    int logc = 0;
    while ((1 << (logc + 1)) <= QT_MAX_C && ((long)P << (logc + 1)) <= QT_LDS_KEYS) ++logc;
    a.y = y;
    a.out = out;
    a.ncol = ncol;
    a.ld = ld;
    a.nsamp = nsamp;
    a.nq = nq;
    a.P = P;
    a.logc = logc;
    const unsigned tiles = (unsigned)((ncol + (1L << logc) - 1) >> logc);
    const long keys = (long)P << logc;
    PZ_HIP(ctx, hipSetDevice(ctx->device));
    if (keys <= 2048)
        hipLaunchKernelGGL((k_column_quantiles<2048, 256>), dim3(tiles), dim3(256), 0, ctx->stream, a);
    else if (keys <= 8192)
        hipLaunchKernelGGL((k_column_quantiles<8192, 512>), dim3(tiles), dim3(512), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL((k_column_quantiles<QT_LDS_KEYS, 1024>), dim3(tiles), dim3(1024), 0, ctx->stream, a);
    PZ_HIP(ctx, hipGetLastError());
    return 0;
}
