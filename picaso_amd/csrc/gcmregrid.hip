// Facet-major cloud tables of every phase of a phase curve from ONE resident GCM cloud map: the device form of the host
// regrid of inputs.clouds_3d / clouds_by_phase (justdoit._regrid_lonlat: spectrum._interp_axis along longitude, then along
// latitude) followed by the re-stack of optics._facet_major_cloud_tables.
//
// The map is the caller's: three variables (opd, w0, g0) laid out (nlon, nlat, npres, nin), the wavenumber index fastest,
// in whatever order the caller's longitudes, latitudes, pressures and wavenumbers come.  The host does every search
// (picaso_amd/gcm.py: the index form of _interp_axis) and hands over, per phase, the two source columns and the weight of
// every Gauss angle along longitude and of every Chebyshev angle along latitude, as indices into the ORIGINAL axes, plus
// the source pressure index of every output layer and the source index of every output wavenumber.  Per element
//
//     a   = m[j0, i0] * (1.0 - t) + m[j1, i0] * t
//     b   = m[j0, i1] * (1.0 - t) + m[j1, i1] * t
//     out = a * (1.0 - u) + b * u
//
// with (1.0 - t) and (1.0 - u) one rounded subtraction each, every product and sum rounded in this order and nothing
// contracted: the bits numpy gives for longitude first and latitude second.
//
// Lanes.  A wave owns one (phase, facet, layer) row and walks its wavenumbers, lane l at l, l + 64, ...: the indices and
// weights of the row are wave-uniform, the four reads of a variable are runs of nin doubles (196 x 8 B for a native map)
// and the store is one such run.  The three variables of a row share the indices.  The kernel reads four times and writes
// once what it produces and does nothing else; no LDS.  Every index is clamped into the map, so a broken table cannot read
// outside it; the Python wrapper refuses such a table before it is uploaded.
#include "common.hpp"

namespace pz {

constexpr int GR_THREADS = 256;
constexpr int GR_ROWS = GR_THREADS / 64;            // rows per workgroup: one per wave

struct GcmFacetArgs {
    const double *map[3];                           // opd, w0, g0: (nlon, nlat, npres, nin)
    const int *lon_idx;                             // (nphase, ng, 2): j0, j1
    const double *lon_t;                            // (nphase, ng)
    const int *lat_idx;                             // (nphase, nt, 2): i0, i1
    const double *lat_u;                            // (nphase, nt)
    const int *layer_src;                           // (nlayer)
    const int *wno_src;                             // (nin)
    double *out;                                    // (nphase, 3, ng * nt * nlayer, nin)
    long nrows;                                     // ng * nt * nlayer
    int nlon, nlat, npres, nin, ng, nt, nlayer;
};

__device__ __forceinline__ int gr_clamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

__global__ __launch_bounds__(GR_THREADS) void k_gcm_facet_tables(const GcmFacetArgs a)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * GR_ROWS + (threadIdx.x >> 6);
    if (r >= a.nrows) return;
    const long phase = blockIdx.y;
    const int layer = (int)(r % a.nlayer);
    const int facet = (int)(r / a.nlayer);
    const int g = facet / a.nt, tt = facet % a.nt;
    const long lg = phase * a.ng + g, lt = phase * a.nt + tt;
    const int j0 = gr_clamp(a.lon_idx[2 * lg], a.nlon), j1 = gr_clamp(a.lon_idx[2 * lg + 1], a.nlon);
    const int i0 = gr_clamp(a.lat_idx[2 * lt], a.nlat), i1 = gr_clamp(a.lat_idx[2 * lt + 1], a.nlat);
    const int lp = gr_clamp(a.layer_src[layer], a.npres);
    const double t = a.lon_t[lg], u = a.lat_u[lt];
    const double ot = 1.0 - t, ou = 1.0 - u;
    const long col = (long)a.npres * a.nin;
    const long o00 = ((long)j0 * a.nlat + i0) * col + (long)lp * a.nin;
    const long o10 = ((long)j1 * a.nlat + i0) * col + (long)lp * a.nin;
    const long o01 = ((long)j0 * a.nlat + i1) * col + (long)lp * a.nin;
    const long o11 = ((long)j1 * a.nlat + i1) * col + (long)lp * a.nin;
    for (int w = lane; w < a.nin; w += 64) {
        const int ws = gr_clamp(a.wno_src[w], a.nin);
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const double *m = a.map[v];
            const double va = m[o00 + ws] * ot + m[o10 + ws] * t;
            const double vb = m[o01 + ws] * ot + m[o11 + ws] * t;
            a.out[((phase * 3 + v) * a.nrows + r) * a.nin + w] = va * ou + vb * u;
        }
    }
}

}  // namespace pz

using namespace pz;

extern "C" int picaso_gcm_facet_tables_dev(picaso_ctx *ctx, int nlon, int nlat, int npres, int nin, const double *opd,
                                           const double *w0, const double *g0, int nphase, int ng, int nt, int nlayer,
                                           const int *lon_idx, const double *lon_t, const int *lat_idx, const double *lat_u,
                                           const int *layer_src, const int *wno_src, double *out)
{
    const char *who = "picaso_gcm_facet_tables_dev";
    if (!ctx) return fail(ctx, "%s: null context", who);
    if (nlon < 1 || nlat < 1 || npres < 1 || nin < 1)
        return fail(ctx, "%s: the map must have longitudes, latitudes, pressures and wavenumbers, got (%d, %d, %d, %d)", who,
                    nlon, nlat, npres, nin);
    if (nphase < 0 || nphase > 65535) return fail(ctx, "%s: nphase must be in [0, 65535], got %d", who, nphase);
    if (ng < 1 || nt < 1 || nlayer < 1)
        return fail(ctx, "%s: ng, nt and nlayer must be positive, got %d, %d, %d", who, ng, nt, nlayer);
    const long nrows = (long)ng * nt * nlayer;
    const long blocks = (nrows + GR_ROWS - 1) / GR_ROWS;
    if (blocks > 2147483647L) return fail(ctx, "%s: %ld rows per phase are more than one launch takes", who, nrows);
    if (nphase == 0) return 0;
    PZ_NEED(ctx, who, opd, w0, g0, lon_idx, lon_t, lat_idx, lat_u, layer_src, wno_src, out);
    GcmFacetArgs a{};
    a.map[0] = opd;
    a.map[1] = w0;
    a.map[2] = g0;
    a.lon_idx = lon_idx;
    a.lon_t = lon_t;
    a.lat_idx = lat_idx;
    a.lat_u = lat_u;
    a.layer_src = layer_src;
    a.wno_src = wno_src;
    a.out = out;
    a.nrows = nrows;
    a.nlon = nlon;
    a.nlat = nlat;
    a.npres = npres;
    a.nin = nin;
    a.ng = ng;
    a.nt = nt;
    a.nlayer = nlayer;
    PZ_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_gcm_facet_tables, dim3((unsigned)blocks, (unsigned)nphase), dim3(GR_THREADS), 0, ctx->stream, a);
    PZ_HIP(ctx, hipGetLastError());
    return 0;
}
