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
