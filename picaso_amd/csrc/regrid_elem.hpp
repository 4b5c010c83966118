// One column of a `picaso_regrid_row` (include/picaso_hip.h), shared by the reductions that fuse the flux ratios of the
// output dictionary into their sums (regrid.hip: bin means; convolve.hip: line-spread convolution).  Contraction is off:
// op 3 as written is a quotient, two products and a sum, each rounded, as numpy forms fpfs_total (justdoit.py:552-599).
#pragma once
#include "common.hpp"

namespace pz {

__device__ __forceinline__ double regrid_elem(const picaso_regrid_row &r, long i)
{
#pragma clang fp contract(off)
    const double a = r.a[i];
    if (r.op == 0) return a;
    if (r.op == 1) return a * r.k1;
    const double q = a / r.b[i] * r.k1;
    if (r.op == 2) return q;
    const double p = r.c[i] * r.k2;
    return q + p;
}

// lane `i`'s value in every lane (`i` is the same in all of them)
__device__ __forceinline__ double lane_value(double v, int i)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), i);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), i);
    return __hiloint2double(hi, lo);
}

// np.bincount's sum of one bin by one wave: elem(i) for i in [lo, hi), added in increasing i to +0.0 -- one chain of
// dependent fp64 additions that every lane carries.  The wave reads the bin in coalesced chunks of 64 columns (lane l
// forms elem(base + l)), a value reaches the adder through v_readlane (no LDS round trip, no barrier), and the next
// chunk's loads are issued before the chain of the current one.
template <typename Elem>
__device__ __forceinline__ double bin_sum(long lo, long hi, int lane, Elem elem)
{
#pragma clang fp contract(off)
    double s = 0.0;                                  // np.bincount's accumulator starts at +0.0
    double v = lo + lane < hi ? elem(lo + lane) : 0.0;
    for (long base = lo; base < hi; base += 64) {
        const long next = base + 64 + lane;
        const double vn = next < hi ? elem(next) : 0.0;                  // in flight while this chunk is added
        const long left = hi - base;
        if (left >= 64) {
#pragma unroll
            for (int i = 0; i < 64; ++i) s = s + lane_value(v, i);
        } else {
            const int n = (int)left;
            for (int i = 0; i < n; ++i) s = s + lane_value(v, i);
        }
        v = vn;
    }
    return s;
}

// the argument checks the entry points share: `who` names the caller in the message
inline int regrid_rows_check(picaso_ctx *ctx, const char *who, int nrows, const picaso_regrid_row *rows,
                             picaso_regrid_row *dst)
{
    if (nrows < 1 || nrows > PICASO_REGRID_MAX_ROWS)
        return fail(ctx, "%s: nrows must be in [1, %d], got %d", who, PICASO_REGRID_MAX_ROWS, nrows);
    for (int r = 0; r < nrows; ++r) {
        const picaso_regrid_row &w = rows[r];
        if (w.op < 0 || w.op > 3) return fail(ctx, "%s: row %d: unknown op %d", who, r, w.op);
        if (!w.a || (w.op >= 2 && !w.b) || (w.op == 3 && !w.c))
            return fail(ctx, "%s: row %d: op %d needs %s", who, r, w.op,
                        w.op == 3 ? "a, b and c" : (w.op == 2 ? "a and b" : "a"));
        dst[r] = w;
    }
    return 0;
}

}  // namespace pz
