// Abundances of every species at every point (T, P) from a resident chemistry table: the batched form of the reference's
// chem_interp (justdoit.py:3106-3199) and of the per-column joblib pool of chemeq_3d / premix_3d (:3517-3664).
//
// The table (picaso_amd/chemistry.py: ChemTable) is log10 of the abundances, row-major (nrow, nspecies), rows
// temperature-major: temperature it owns the rows row_start[it] .. row_start[it] + nc_p[it] - 1, the first nc_p[it] pressures
// of one ascending grid.  Per point, with the comparisons of chemistry.interp_numpy (a NaN makes every one false: index 0):
//
//     t_inv = 1 / T                                            p_log = log10 P, taken by the caller on the host
//     t_low = last i with t_inv_grid[i] > t_inv, else 0; ntemp - 1 becomes ntemp - 2;   t_hi = t_low + 1
//     p_low = min(last i with p_log_grid[i] <= p_log, else 0;  nc_p[t_hi] - 3);         p_hi = p_low + 1
//     t_i = (t_inv - t_inv_grid[t_low]) / (t_inv_grid[t_hi] - t_inv_grid[t_low])
//     p_i = (p_log - p_log_grid[p_low]) / (p_log_grid[p_hi] - p_log_grid[p_low])
//
// and per (point, species), with the rows a = [t_low, p_low], b = [t_hi, p_low], c = [t_hi, p_hi], d = [t_low, p_hi]:
//
//     x = ((((1 - t_i) (1 - p_i)) a + (t_i (1 - p_i)) b) + (t_i p_i) c) + ((1 - t_i) p_i) d
//
// every quotient an IEEE division, every product and sum rounded in this order, nothing contracted: x has numpy's bits.
// The abundance is 10**x (chem_exp10 below), within 4 ulp of numpy's.
//
// Lanes.  A lane owns a point and walks the species: the (nsel, npoints) result is point-fastest, so at every species the
// 64 lanes of a wave store 512 contiguous bytes.  The two searches and the four weights of a point are formed once and
// shared by its species.  The grids (a few hundred doubles) sit in LDS, every lane scanning the same address (a broadcast
// read); the four table rows of a point are gathers from a matrix of under 1 MB that L2 serves, and a row's cache lines
// are reused across the species walk.  The only HBM traffic that grows with the problem is the result.
#include "common.hpp"
#include "device_math.hpp"

namespace pz {

constexpr int CI_THREADS = 256;
constexpr long CI_MAX_BLOCKS = 1L << 20;
constexpr size_t CI_MAX_LDS = 64 * 1024;

struct ChemInterpArgs {
    const double *log_abunds;       // (nrow, nspecies)
    const double *t_inv_grid;       // (ntemp)
    const double *p_log_grid;       // (npres)
    const int *nc_p;                // (ntemp)
    const int *row_start;           // (ntemp)
    const double *temperature;      // (npoints)
    const double *p_log;            // (npoints)
    const int *sel;                 // (nsel) or NULL
    double *out;                    // (nsel, npoints)
    long npoints;
    int nrow, nspecies, ntemp, npres, nsel, log10_out;
};

// 10**x = 2**(x log2(10)).  The product y = x * hi is rounded; its error and the low part of log2(10) are recovered in
// e = fma(x, hi, -y) + x lo (|e| <= 2^-52 |y|), and 2**(y + e) = 2**y (1 + e ln 2 + O(e^2)): fexp2(y) (<= 1 ulp) and one
// fma.  Without e the error grows with |x| (141 ulp at x = -55).  x = -inf gives 0, +inf gives inf, NaN gives NaN, as
// numpy's 10.0**x; an overflowing fexp2 stays inf (inf * e would be NaN for e < 0).
__device__ __forceinline__ double chem_exp10(double x)
{
#pragma clang fp contract(off)
    constexpr double L2_10_HI = 0x1.a934f0979a371p+1;       // log2(10) rounded to double
    constexpr double L2_10_LO = 0x1.7f2495fb7fa6dp-53;      // log2(10) - L2_10_HI
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

__global__ __launch_bounds__(CI_THREADS) void k_chem_interp(const ChemInterpArgs a)
{
#pragma clang fp contract(off)
    extern __shared__ double ci_lds[];
    double *tg = ci_lds;
    double *pg = tg + a.ntemp;
    int *ncp = reinterpret_cast<int *>(pg + a.npres);
    int *rs = ncp + a.ntemp;
    for (int i = threadIdx.x; i < a.ntemp; i += CI_THREADS) {
        tg[i] = a.t_inv_grid[i];
        ncp[i] = a.nc_p[i];
        rs[i] = a.row_start[i];
    }
    for (int i = threadIdx.x; i < a.npres; i += CI_THREADS) pg[i] = a.p_log_grid[i];
    __syncthreads();

    const long stride = (long)gridDim.x * CI_THREADS;
    for (long i = (long)blockIdx.x * CI_THREADS + threadIdx.x; i < a.npoints; i += stride) {
        const double t_inv = 1.0 / a.temperature[i];
        const double p_log = a.p_log[i];
        int t_low = 0;
        for (int k = 0; k < a.ntemp; ++k)
            if (tg[k] > t_inv) t_low = k;
        if (t_low > a.ntemp - 2) t_low = a.ntemp - 2;
        const int t_hi = t_low + 1;
        int p_low = 0;
        for (int k = 0; k < a.npres; ++k)
            if (pg[k] <= p_log) p_low = k;
        p_low = min(p_low, ncp[t_hi] - 3);
        // the host refuses tables for which these two could bite (ChemTable); they keep a broken table inside the arrays
        p_low = max(0, min(p_low, a.npres - 2));
        const int p_hi = p_low + 1;
        const double t_i = (t_inv - tg[t_low]) / (tg[t_hi] - tg[t_low]);
        const double p_i = (p_log - pg[p_low]) / (pg[p_hi] - pg[p_low]);
        const double ot = 1.0 - t_i, op = 1.0 - p_i;
        const double wa = ot * op, wb = t_i * op, wc = t_i * p_i, wd = ot * p_i;
        const long last = a.nrow - 1;
        const long ra = max(0L, min((long)rs[t_low] + p_low, last)) * a.nspecies;
        const long rb = max(0L, min((long)rs[t_hi] + p_low, last)) * a.nspecies;
        const long rc = max(0L, min((long)rs[t_hi] + p_hi, last)) * a.nspecies;
        const long rd = max(0L, min((long)rs[t_low] + p_hi, last)) * a.nspecies;
        for (int s = 0; s < a.nsel; ++s) {
            int col = a.sel ? a.sel[s] : s;
            col = max(0, min(col, a.nspecies - 1));
            const double va = a.log_abunds[ra + col], vb = a.log_abunds[rb + col];
            const double vc = a.log_abunds[rc + col], vd = a.log_abunds[rd + col];
            const double x = ((wa * va + wb * vb) + wc * vc) + wd * vd;
            a.out[(long)s * a.npoints + i] = a.log10_out ? x : chem_exp10(x);
        }
    }
}

}  // namespace pz

using namespace pz;

extern "C" int picaso_chem_interp_dev(picaso_ctx *ctx, int nrow, int nspecies, const double *log_abunds, int ntemp, int npres,
                                      const double *t_inv_grid, const double *p_log_grid, const int *nc_p,
                                      const int *row_start, long npoints, const double *temperature, const double *p_log,
                                      int nsel, const int *sel, int log10_out, double *out)
{
    const char *who = "picaso_chem_interp_dev";
    if (!ctx) return fail(ctx, "%s: null context", who);
    if (npoints < 0) return fail(ctx, "%s: npoints must not be negative, got %ld", who, npoints);
    if (nrow < 1 || nspecies < 1) return fail(ctx, "%s: the table must have rows and species, got (%d, %d)", who, nrow, nspecies);
    if (ntemp < 2 || npres < 2)
        return fail(ctx, "%s: the interpolation needs two temperatures and two pressures, got %d and %d", who, ntemp, npres);
    if (nsel < 1) return fail(ctx, "%s: nsel must be positive, got %d", who, nsel);
    if (!sel && nsel != nspecies)
        return fail(ctx, "%s: without a selection nsel must be nspecies = %d, got %d", who, nspecies, nsel);
    const size_t lds = (size_t)ntemp * (sizeof(double) + 2 * sizeof(int)) + (size_t)npres * sizeof(double);
    if (lds > CI_MAX_LDS)
        return fail(ctx, "%s: grids of %d temperatures and %d pressures take %zu bytes of LDS, more than %zu", who, ntemp, npres,
                    lds, CI_MAX_LDS);
    if (npoints == 0) return 0;
    PZ_NEED(ctx, who, log_abunds, t_inv_grid, p_log_grid, nc_p, row_start, temperature, p_log, out);
    ChemInterpArgs a{};
    a.log_abunds = log_abunds;
    a.t_inv_grid = t_inv_grid;
    a.p_log_grid = p_log_grid;
    a.nc_p = nc_p;
    a.row_start = row_start;
    a.temperature = temperature;
    a.p_log = p_log;
    a.sel = sel;
    a.out = out;
    a.npoints = npoints;
    a.nrow = nrow;
    a.nspecies = nspecies;
    a.ntemp = ntemp;
    a.npres = npres;
    a.nsel = nsel;
    a.log10_out = log10_out;
    const long blocks = (npoints + CI_THREADS - 1) / CI_THREADS;
    PZ_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_chem_interp, dim3((unsigned)(blocks < CI_MAX_BLOCKS ? blocks : CI_MAX_BLOCKS)), dim3(CI_THREADS), lds,
                       ctx->stream, a);
    PZ_HIP(ctx, hipGetLastError());
    return 0;
}
