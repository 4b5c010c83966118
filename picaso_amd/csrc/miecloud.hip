// Cloud tables of a batch of Mie clouds, written where the fused opacity launch reads them: the device form of
// mie.cloud_brewster_mie / mie.cloud_flex_fsed (reference parameterizations.py:94-198: the sum of a Mie table over a particle
// size distribution, then picaso_format) followed by cloud_averaging (:753-792).
//
// A sample is K decks.  A deck is a Mie table (qext, qscat, cos_qscat, each (nradii, nwave) with the wavelength index fastest
// and the wavenumber increasing), nradii weights wgt[r] = (ndz * (PI * radius[r]**2)) * distribution[r], a layer factor and a
// layer mask, all formed on the host, which takes every discrete decision.  Two launches:
//
//   k_mie_cloud_sums   one workgroup per deck.  Per wavelength the three left-to-right sums over r from 0 of q[r][w] * wgt[r]
//                      (opd, opd_scat, opd_cos), w0 = opd_scat / opd where opd > 0 else 0, g0 = opd_cos / opd_scat where
//                      opd_scat > 0 else 0, and the deck's max over all wavelengths of opd as np.max forms it (exact; a NaN
//                      anywhere gives NaN).  (nwave x 3 + 1) doubles per deck in `work`.
//   k_mie_cloud_rows   the shape of k_param_cloud_tables (paramcloud.hip): a workgroup owns one sample, a tile of wavelengths
//                      and a chunk of layers, keeps the decks' per-wavelength values and per-layer values in LDS and walks
//                      the chunk in memory order.  v = opd / max for a Brewster deck, opd for a flex_fsed deck; per element
//                      inside the mask (factor[l] * v, w0, g0), outside (opd * 0, w0 * 0, g0 * 0) as picaso_format forms
//                      them: +0 for every finite value that is not negative.  Then cloud_averaging as in paramcloud.hip.
//
// Rounded products, ordered sums, a max and IEEE quotients only, nothing contracted: the rows are the host route's bits.
#include "common.hpp"
#include "device_math.hpp"

#include <climits>

namespace pz {

constexpr int MC_THREADS = 256;
constexpr int MC_TILE = 256;                        // wavelengths per workgroup: 4 values x K decks x tile, 32 KB of LDS
constexpr int MC_CHUNK = 32;                        // most layers per workgroup
constexpr int MC_MAXK = 4;
constexpr long MC_TARGET = 1024;                    // workgroups wanted before chunks grow (4 per CU)

struct MieDeck {
    const double *table;                            // (3, nradii, nwave); nullptr: an empty deck
    int nradii, kind;                               // kind 0: brewster_mie, 1: flex_fsed
};

struct MieCloudArgs {
    const MieDeck *decks;                           // (S, K)
    const double *wgt;                              // (S, K, rmax)
    const double *factor, *inside;                  // (S, K, nlayer)
    double *work;                                   // (S, K, 3 * nwave + 1): opd, w0, g0 per wavelength, then max(opd)
    double *out;                                    // (S, 3, nlayer, nwave)
    int S, K, nlayer, nwave, rmax, average, chunk, nchunk, ntile;
};

__global__ __launch_bounds__(MC_THREADS) void k_mie_cloud_sums(const MieCloudArgs a)
{
#pragma clang fp contract(off)
    __shared__ double smax[MC_THREADS];
    __shared__ int snan[MC_THREADS];
    const long d = blockIdx.x;
    const MieDeck deck = a.decks[d];
    if (!deck.table) return;
    const int R = deck.nradii, nw = a.nwave;
    const double *const wgt = a.wgt + d * a.rmax;
    const double *const qe = deck.table, *const qs = qe + (long)R * nw, *const qc = qs + (long)R * nw;
    double *const wk = a.work + d * (3L * nw + 1);
    double mx = -__builtin_inf();
    int isnan_ = 0;
    for (int w = threadIdx.x; w < nw; w += MC_THREADS) {
        double opd = 0.0, sca = 0.0, cq = 0.0;
        for (int r = 0; r < R; ++r) {
            const double g = wgt[r];
            const long at = (long)r * nw + w;
            opd = opd + mul_unfused(qe[at], g);
            sca = sca + mul_unfused(qs[at], g);
            cq = cq + mul_unfused(qc[at], g);
        }
        wk[w] = opd;
        wk[nw + w] = (opd > 0.0) ? sca / opd : 0.0;
        wk[2 * nw + w] = (sca > 0.0) ? cq / sca : 0.0;
        if (opd != opd) isnan_ = 1;
        else if (opd > mx) mx = opd;
    }
    smax[threadIdx.x] = mx;
    snan[threadIdx.x] = isnan_;
    __syncthreads();
    for (int half = MC_THREADS / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) {
            if (smax[threadIdx.x + half] > smax[threadIdx.x]) smax[threadIdx.x] = smax[threadIdx.x + half];
            snan[threadIdx.x] |= snan[threadIdx.x + half];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) wk[3L * nw] = snan[0] ? __builtin_nan("") : smax[0];
}

__global__ __launch_bounds__(MC_THREADS) void k_mie_cloud_rows(const MieCloudArgs a)
{
#pragma clang fp contract(off)
    __shared__ double val[MC_MAXK * 4 * MC_TILE];          // per deck: v, w0, g0, opd * 0
    __shared__ double lay[MC_MAXK * 2 * MC_CHUNK];         // per deck: factor, inside
    __shared__ int live[MC_MAXK];
    const long b = blockIdx.x;
    const int tile = (int)(b % a.ntile);
    const int ch = (int)((b / a.ntile) % a.nchunk);
    const long s = b / ((long)a.ntile * a.nchunk);
    const int w0i = tile * MC_TILE;
    const int tw = min(MC_TILE, a.nwave - w0i);
    const int l0 = ch * a.chunk;
    const int nl = min(a.chunk, a.nlayer - l0);
    const int K = a.K, nw = a.nwave;

    if ((int)threadIdx.x < K) live[threadIdx.x] = a.decks[s * K + threadIdx.x].table != nullptr;
    for (int i = threadIdx.x; i < K * tw; i += MC_THREADS) {
        const int k = i / tw, w = i - k * tw;
        const MieDeck deck = a.decks[s * K + k];
        if (!deck.table) continue;
        const double *const wk = a.work + (s * K + k) * (3L * nw + 1);
        const double opd = wk[w0i + w];
        double *const v = val + (k * 4) * MC_TILE + w;
        v[0] = (deck.kind == 0) ? opd / wk[3L * nw] : opd;
        v[MC_TILE] = wk[nw + w0i + w];
        v[2 * MC_TILE] = wk[2 * nw + w0i + w];
        v[3 * MC_TILE] = mul_unfused(opd, 0.0);
    }
    for (int i = threadIdx.x; i < K * 2 * nl; i += MC_THREADS) {
        const int kv = i / nl, l = i - kv * nl;
        const int k = kv >> 1;
        const double *const src = (kv & 1) ? a.inside : a.factor;
        lay[kv * MC_CHUNK + l] = src[(s * K + k) * a.nlayer + l0 + l];
    }
    __syncthreads();

    const long plane = (long)a.nlayer * nw;
    double *const out = a.out + s * 3 * plane + (long)l0 * nw + w0i;
    // the chunk in memory order: element j is (layer j / tw, wavelength j % tw), carried without a division per element
    int l = threadIdx.x / tw, w = threadIdx.x - l * tw;
    const int dl = MC_THREADS / tw, dw = MC_THREADS - dl * tw;
    for (; l < nl; l += dl, w += dw) {
        if (w >= tw) {
            w -= tw;
            if (++l >= nl) break;
        }
        const long at = (long)l * nw + w;
        double opd = 0.0, g0 = 0.0, w0 = 0.0;
        for (int k = 0; k < K; ++k) {
            if (!live[k]) continue;
            const double *const v = val + (k * 4) * MC_TILE + w;
            const bool in = lay[(2 * k + 1) * MC_CHUNK + l] != 0.0;
            const double ok = in ? mul_unfused(lay[(2 * k) * MC_CHUNK + l], v[0]) : v[3 * MC_TILE];
            const double wk = in ? v[MC_TILE] : mul_unfused(v[MC_TILE], 0.0);
            const double gk = in ? v[2 * MC_TILE] : mul_unfused(v[2 * MC_TILE], 0.0);
            if (!a.average) {
                opd = ok;
                w0 = wk;
                g0 = gk;
                break;
            }
            opd = opd + ok;
            g0 = g0 + mul_unfused(ok, gk);
            w0 = w0 + mul_unfused(ok, wk);
        }
        if (a.average) {
            if (opd == 0.0) opd = 1e-33;
            w0 = w0 / opd;
            g0 = g0 / opd;
        }
        out[at] = opd;
        out[plane + at] = w0;
        out[2 * plane + at] = g0;
    }
}

}  // namespace pz

using namespace pz;

extern "C" int picaso_mie_cloud_tables_dev(picaso_ctx *ctx, int S, int K, int nlayer, int nwave, int average, int ntable,
                                           const double *const *tables, const int *nradii, const int *deck_table,
                                           const int *deck_kind, int rmax, const double *wgt, const double *factor,
                                           const double *inside, double *work, double *out)
{
    const char *who = "picaso_mie_cloud_tables_dev";
    if (!ctx) return fail(ctx, "%s: null context", who);
    if (S < 1) return fail(ctx, "%s: S must be at least 1, got %d", who, S);
    if (K < 1 || K > MC_MAXK) return fail(ctx, "%s: K must be in [1, %d], got %d", who, MC_MAXK, K);
    if (nlayer < 1) return fail(ctx, "%s: nlayer must be at least 1, got %d", who, nlayer);
    if (nwave < 2) return fail(ctx, "%s: the cloud grid needs at least 2 wavenumbers, got %d", who, nwave);
    if (average != 0 && average != 1) return fail(ctx, "%s: average must be 0 or 1, got %d", who, average);
    if (average == 0 && K != 1) return fail(ctx, "%s: average = 0 takes one deck per sample, got K = %d", who, K);
    if (ntable < 1) return fail(ctx, "%s: ntable must be at least 1, got %d", who, ntable);
    if (rmax < 1) return fail(ctx, "%s: rmax must be at least 1, got %d", who, rmax);
    PZ_NEED(ctx, who, tables, nradii, deck_table, deck_kind, wgt, factor, inside, work, out);
    for (int t = 0; t < ntable; ++t) {
        if (!tables[t]) return fail(ctx, "%s: table %d is NULL", who, t);
        if (nradii[t] < 1 || nradii[t] > rmax)
            return fail(ctx, "%s: table %d has %d radii; 1 to rmax = %d", who, t, nradii[t], rmax);
    }
    const long ndeck = (long)S * K;
    if (ndeck > INT_MAX) return fail(ctx, "%s: %ld decks are more than one launch takes", who, ndeck);
    std::vector<MieDeck> decks((size_t)ndeck);
    for (long d = 0; d < ndeck; ++d) {
        const int t = deck_table[d];
        if (t < -1 || t >= ntable) return fail(ctx, "%s: deck %ld names table %d of %d", who, d, t, ntable);
        if (t >= 0 && deck_kind[d] != 0 && deck_kind[d] != 1)
            return fail(ctx, "%s: deck %ld has kind %d; 0 (brewster_mie) or 1 (flex_fsed)", who, d, deck_kind[d]);
        if (t < 0 && !average) return fail(ctx, "%s: deck %ld is empty, and average = 0 stores the deck as it is", who, d);
        decks[(size_t)d] = MieDeck{t < 0 ? nullptr : tables[t], t < 0 ? 0 : nradii[t], deck_kind[d]};
    }
    MieCloudArgs a{};
    a.wgt = wgt;
    a.factor = factor;
    a.inside = inside;
    a.work = work;
    a.out = out;
    a.S = S;
    a.K = K;
    a.nlayer = nlayer;
    a.nwave = nwave;
    a.rmax = rmax;
    a.average = average;
    a.ntile = (nwave + MC_TILE - 1) / MC_TILE;
    const long small = (long)S * a.ntile * nlayer;              // workgroups at one layer each
    a.chunk = (int)std::min<long>(MC_CHUNK, std::max<long>(1, small / MC_TARGET));
    a.nchunk = (nlayer + a.chunk - 1) / a.chunk;
    const long blocks = (long)S * a.ntile * a.nchunk;
    if (blocks > 2147483647L) return fail(ctx, "%s: %ld workgroups are more than one launch takes", who, blocks);
    PZ_HIP(ctx, hipSetDevice(ctx->device));
    PZ_TRY(arena_reset(ctx, decks.size() * sizeof(MieDeck) + 256));
    PZ_TRY(arena_upload(ctx, decks.data(), decks.size(), &a.decks));
    hipLaunchKernelGGL(k_mie_cloud_sums, dim3((unsigned)ndeck), dim3(MC_THREADS), 0, ctx->stream, a);
    PZ_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_mie_cloud_rows, dim3((unsigned)blocks), dim3(MC_THREADS), 0, ctx->stream, a);
    PZ_HIP(ctx, hipGetLastError());
    PZ_HIP(ctx, hipStreamSynchronize(ctx->stream));             // the deck records are a host vector of this call
    return 0;
}
