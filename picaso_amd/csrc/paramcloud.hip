// Cloud tables of a batch of parametrized grey clouds, written where the fused opacity launch reads them: the device form of
// Parameterize.cloud_brewster_grey / cloud_hard_grey followed by cloud_averaging (reference parameterizations.py:200-253,
// :753-792) and of the stack onecall._cloud_inputs builds from their DataFrames.
//
// A sample is K decks.  A deck is three layer vectors (opd_l, w0_l, g0_l: what deck_decay / slab_decay / the box test of
// inputs.clouds give, formed on the host -- their argmin, caps and comparisons decide WHICH cloud it is and stay where the
// reference takes them) and two numbers, alpha and reference_wave.  Per element
//
//     opd_k = opd_l[k][l] * (wavelength[w] / reference_wave_k) ** (-alpha_k)
//
// with an IEEE division, the library's pow (alpha == 0: exactly 1) and one rounded product.  average == 0 (K = 1) stores
// opd_0, w0_l[0][l], g0_l[0][l].  average == 1 is cloud_averaging in deck order: opd the left-to-right sum of opd_k from 0,
// w0 and g0 the left-to-right sums of opd_k * w0_k and opd_k * g0_k from 0, opd replaced by 1e-33 where the sum is 0, then
// the two IEEE quotients; nothing contracted.  With every alpha = 0 these are the reference's bits.
//
// Shape.  The kernel is store-bound: 24 bytes per element against K powers per (sample, deck, wavelength) that no layer
// changes.  A workgroup owns one sample, one tile of at most PC_TILE wavelengths and a chunk of layers: its threads form
// the K x tile powers once into LDS (each power by one thread) and the chunk's 3 K layer values beside them, then walk the
// chunk's elements in memory order -- for nin <= PC_TILE the chunk is one contiguous run of (layers x nin) doubles per
// variable, so every wave stores 512 consecutive bytes whatever nin is (196 is no multiple of 64).  The host sizes the
// chunk: one layer per workgroup while the batch is small (S = 1, 90 layers: 90 workgroups), up to PC_CHUNK layers once
// there are PC_TARGET workgroups without that (S = 1000: 3 000 workgroups of 32 layers, each power formed 3 times, not 90).
// The chunk size moves no bit: every element is formed from its own inputs alone.
#include "common.hpp"
#include "device_math.hpp"

namespace pz {

constexpr int PC_THREADS = 256;
constexpr int PC_TILE = 512;                        // wavelengths per workgroup: K x tile powers, 16 KB of LDS at K = 4
constexpr int PC_CHUNK = 32;                        // most layers per workgroup
constexpr int PC_MAXK = 4;
constexpr long PC_TARGET = 1024;                    // workgroups wanted before chunks grow (4 per CU)

struct ParamCloudArgs {
    const double *layers;                           // (S, K, 3, nlayer): opd_l, w0_l, g0_l of every deck
    const double *params;                           // (S, K, 2): alpha, reference_wave
    const double *wavelength;                       // (nin): 1e4 / wavenumber, wavenumber increasing
    double *out;                                    // (S, 3, nlayer, nin): opd, w0, g0
    int S, K, nlayer, nin, average, chunk, nchunk, ntile;
};

__global__ __launch_bounds__(PC_THREADS) void k_param_cloud_tables(const ParamCloudArgs a)
{
#pragma clang fp contract(off)
    __shared__ double pw[PC_MAXK * PC_TILE];
    __shared__ double lay[PC_MAXK * 3 * PC_CHUNK];
    const long b = blockIdx.x;
    const int tile = (int)(b % a.ntile);
    const int ch = (int)((b / a.ntile) % a.nchunk);
    const long s = b / ((long)a.ntile * a.nchunk);
    const int w0i = tile * PC_TILE;
    const int tw = min(PC_TILE, a.nin - w0i);
    const int l0 = ch * a.chunk;
    const int nl = min(a.chunk, a.nlayer - l0);
    const int K = a.K;

    for (int i = threadIdx.x; i < K * tw; i += PC_THREADS) {
        const int k = i / tw, w = i - k * tw;
        const double alpha = a.params[(s * K + k) * 2], ref = a.params[(s * K + k) * 2 + 1];
        const double ratio = a.wavelength[w0i + w] / ref;
        pw[k * PC_TILE + w] = (alpha == 0.0) ? 1.0 : pow(ratio, -alpha);
    }
    for (int i = threadIdx.x; i < K * 3 * nl; i += PC_THREADS) {
        const int kv = i / nl, l = i - kv * nl;
        lay[kv * PC_CHUNK + l] = a.layers[(s * K * 3 + kv) * a.nlayer + l0 + l];
    }
    __syncthreads();

    const long plane = (long)a.nlayer * a.nin;
    double *const out = a.out + s * 3 * plane + (long)l0 * a.nin + w0i;
    // the chunk in memory order: element j is (layer j / tw, wavelength j % tw), carried without a division per element
    int l = threadIdx.x / tw, w = threadIdx.x - l * tw;
    const int dl = PC_THREADS / tw, dw = PC_THREADS - dl * tw;
    for (; l < nl; l += dl, w += dw) {
        if (w >= tw) {
            w -= tw;
            if (++l >= nl) break;
        }
        const long at = (long)l * a.nin + w;
        if (!a.average) {
            out[at] = mul_unfused(lay[l], pw[w]);
            out[plane + at] = lay[PC_CHUNK + l];
            out[2 * plane + at] = lay[2 * PC_CHUNK + l];
            continue;
        }
        double opd = 0.0, g0 = 0.0, w0 = 0.0;
        for (int k = 0; k < K; ++k) {
            const double ok = mul_unfused(lay[(3 * k) * PC_CHUNK + l], pw[k * PC_TILE + w]);
            opd = opd + ok;
            g0 = g0 + mul_unfused(ok, lay[(3 * k + 2) * PC_CHUNK + l]);
            w0 = w0 + mul_unfused(ok, lay[(3 * k + 1) * PC_CHUNK + l]);
        }
        if (opd == 0.0) opd = 1e-33;
        out[at] = opd;
        out[plane + at] = w0 / opd;
        out[2 * plane + at] = g0 / opd;
    }
}

}  // namespace pz

using namespace pz;

extern "C" int picaso_param_cloud_tables_dev(picaso_ctx *ctx, int S, int K, int nlayer, int nin, int average,
                                             const double *layers, const double *params, const double *wavelength,
                                             double *out)
{
    const char *who = "picaso_param_cloud_tables_dev";
    if (!ctx) return fail(ctx, "%s: null context", who);
    if (S < 1) return fail(ctx, "%s: S must be at least 1, got %d", who, S);
    if (K < 1 || K > PC_MAXK) return fail(ctx, "%s: K must be in [1, %d], got %d", who, PC_MAXK, K);
    if (nlayer < 1) return fail(ctx, "%s: nlayer must be at least 1, got %d", who, nlayer);
    if (nin < 2) return fail(ctx, "%s: the cloud grid needs at least 2 wavenumbers, got %d", who, nin);
    if (average != 0 && average != 1) return fail(ctx, "%s: average must be 0 or 1, got %d", who, average);
    if (average == 0 && K != 1) return fail(ctx, "%s: average = 0 takes one deck per sample, got K = %d", who, K);
    PZ_NEED(ctx, who, layers, params, wavelength, out);
    ParamCloudArgs a{};
    a.layers = layers;
    a.params = params;
    a.wavelength = wavelength;
    a.out = out;
    a.S = S;
    a.K = K;
    a.nlayer = nlayer;
    a.nin = nin;
    a.average = average;
    a.ntile = (nin + PC_TILE - 1) / PC_TILE;
    const long small = (long)S * a.ntile * nlayer;              // workgroups at one layer each
    a.chunk = (int)std::min<long>(PC_CHUNK, std::max<long>(1, small / PC_TARGET));
    a.nchunk = (nlayer + a.chunk - 1) / a.chunk;
    const long blocks = (long)S * a.ntile * a.nchunk;
    if (blocks > 2147483647L) return fail(ctx, "%s: %ld workgroups are more than one launch takes", who, blocks);
    PZ_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_param_cloud_tables, dim3((unsigned)blocks), dim3(PC_THREADS), 0, ctx->stream, a);
    PZ_HIP(ctx, hipGetLastError());
    return 0;
}
