// One step of the abundance-weighted sum of line-by-line cross sections behind a premixed correlated-k table (reference
// opacity_factory.py:1617, 1707-1713, compute_sum_molecular):
//
//     total_sum = 0
//     for gas:  dset = np.interp(uniform_wno_grid_all, og_wvno_grid, dset)   when the two grids differ
//               total_sum += weight * dset
//
// acc[j] = (first ? 0.0 : acc[j]) + weight * v[j]: the product and the sum are two IEEE operations, nothing is contracted,
// so the device sum IS numpy's, bit for bit, subnormal products included (fp64 denormals are never flushed on gfx950).  With
// `first` the sum starts as 0.0 + weight * v as the reference's does: a product of -0.0 becomes +0.0.
//
// Two kernels:
//
//   k_xsec_axpy          v = src.  Streaming: two reads and one write of 8 bytes per element, 16 bytes per lane and access
//                        when acc and src are 16-byte aligned (every block of picaso_dev_malloc is), at most 2 048 workgroups
//                        of 256 threads that stride over the row.
//   k_xsec_axpy_interp   v = np.interp(out_grid, src_grid, src): numpy's bracket (the last knot <= x), its knot-hit rule, its
//                        clamps and its NaN retry (interp.hpp).  Cross-section grids are uniform, so the bracket is guessed
//                        from (x - start) / step and corrected against the grid ARRAY, a few steps either way; when the guess
//                        is further off than that (a grid that is not uniform after all) the binary search of interp.hpp finds
//                        it.  Either way the index is the one numpy finds: the guess decides nothing.
#include <algorithm>
#include <cstdint>

#include "common.hpp"
#include "interp.hpp"

namespace pz {

constexpr int XSUM_THREADS = 256;
constexpr long XSUM_MAX_BLOCKS = 2048;

struct XsecAxpyArgs {
    long n_out, n_src;
    double *acc;
    const double *src, *src_grid, *out_grid;
    double weight;
    int first;
    double guess_start, guess_step;             // guess_step > 0: knot j lies near guess_start + j guess_step
};

__device__ __forceinline__ double xsum_step(double acc, bool first, double weight, double v)
{
#pragma clang fp contract(off)
    const double p = weight * v;
    return (first ? 0.0 : acc) + p;
}

template <bool VEC>
__global__ __launch_bounds__(XSUM_THREADS) void k_xsec_axpy(const XsecAxpyArgs a)
{
    const long stride = (long)gridDim.x * XSUM_THREADS;
    const long t = (long)blockIdx.x * XSUM_THREADS + threadIdx.x;
    const bool first = a.first != 0;
    if (VEC) {
        const long npair = a.n_out >> 1;
        double2 *acc2 = reinterpret_cast<double2 *>(a.acc);
        const double2 *src2 = reinterpret_cast<const double2 *>(a.src);
        for (long i = t; i < npair; i += stride) {
            const double2 s = src2[i];
            double2 r = first ? make_double2(0.0, 0.0) : acc2[i];
            r.x = xsum_step(r.x, first, a.weight, s.x);
            r.y = xsum_step(r.y, first, a.weight, s.y);
            acc2[i] = r;
        }
        if ((a.n_out & 1) && t == 0) {
            const long j = a.n_out - 1;
            a.acc[j] = xsum_step(first ? 0.0 : a.acc[j], first, a.weight, a.src[j]);
        }
    } else {
        for (long j = t; j < a.n_out; j += stride)
            a.acc[j] = xsum_step(first ? 0.0 : a.acc[j], first, a.weight, a.src[j]);
    }
}

__global__ __launch_bounds__(XSUM_THREADS) void k_xsec_axpy_interp(const XsecAxpyArgs a)
{
    const long stride = (long)gridDim.x * XSUM_THREADS;
    const bool first = a.first != 0;
    for (long j = (long)blockIdx.x * XSUM_THREADS + threadIdx.x; j < a.n_out; j += stride) {
        const double v = regrid_value(a.src, regrid_bracket_guess(a.src_grid, (int)a.n_src, a.out_grid[j], a.guess_start,
                                                                  a.guess_step));
        a.acc[j] = xsum_step(first ? 0.0 : a.acc[j], first, a.weight, v);
    }
}

}  // namespace pz

using namespace pz;

extern "C" int picaso_xsec_axpy_dev(picaso_ctx *ctx, long n_out, double *acc, int first, double weight, const double *src,
                                    long n_src, const double *src_grid, const double *out_grid, double guess_start,
                                    double guess_step)
{
    if (!ctx) return fail(nullptr, "picaso_xsec_axpy_dev: null context");
    PZ_NEED(ctx, "picaso_xsec_axpy_dev", acc, src);
    if ((src_grid == nullptr) != (out_grid == nullptr))
        return fail(ctx, "picaso_xsec_axpy_dev: src_grid and out_grid go together: give both, or neither");
    PZ_TRY(xsec_row_args(ctx, "picaso_xsec_axpy_dev", n_out, n_src, src_grid != nullptr, guess_start, &guess_step));
    if (!src_grid && n_src != n_out)
        return fail(ctx, "picaso_xsec_axpy_dev: the source row has %ld points, the sum %ld, and no grids were given to "
                         "interpolate on", n_src, n_out);
    if (weight != weight) return fail(ctx, "picaso_xsec_axpy_dev: the weight is NaN");
    PZ_HIP(ctx, hipSetDevice(ctx->device));
    XsecAxpyArgs a{};
    a.n_out = n_out;
    a.n_src = n_src;
    a.acc = acc;
    a.src = src;
    a.src_grid = src_grid;
    a.out_grid = out_grid;
    a.weight = weight;
    a.first = first != 0;
    a.guess_start = guess_start;
    a.guess_step = guess_step;
    const bool vec = !src_grid && (((uintptr_t)acc | (uintptr_t)src) & 15) == 0;
    const long work = vec ? (n_out + 1) / 2 : n_out;
    const long blocks = std::min(XSUM_MAX_BLOCKS, (work + XSUM_THREADS - 1) / XSUM_THREADS);
    const dim3 grid((unsigned)blocks), block(XSUM_THREADS);
    if (src_grid) hipLaunchKernelGGL(k_xsec_axpy_interp, grid, block, 0, ctx->stream, a);
    else if (vec) hipLaunchKernelGGL(k_xsec_axpy<true>, grid, block, 0, ctx->stream, a);
    else hipLaunchKernelGGL(k_xsec_axpy<false>, grid, block, 0, ctx->stream, a);
    PZ_HIP(ctx, hipGetLastError());
    return 0;
}
