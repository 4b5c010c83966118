// numpy.interp's arithmetic for one x against a nondecreasing grid (numpy/_core/src/multiarray/compiled_base.c:arr_interp),
// shared by the kernels that restate it: the cloud-table regrid (k_regrid_rows, k_regrid_facets, the fused gas + mixing
// launch: reference wavelength.regrid, wavelength.py:46-70), the tau-pressure of a contribution run (k_contribution_columns:
// find_press, justdoit.py:1281-1292), the continuum rows (k_cont_rows) and the two cross-section kernels, which guess the
// bracket of a uniform grid before they search (k_xsec_axpy_interp, csrc/xsecsum.hip; k_xsec_resample, csrc/contfactory.hip).
//
// The bracket: j = -2 for a NaN x, -1 left of the grid, nin right of it, else the LAST index with xp[j] <= x (what numpy's
// binary_search_with_guess returns; on a grid with ties, e.g. the zero cumulative optical depth above a cloud deck, the last
// of the tied knots).  Then numpy's rules: NaN x -> x; left -> fp[0]; right or j the last knot -> fp[last]; a knot hit ->
// fp[j]; otherwise slope = (fp[j+1]-fp[j])/(xp[j+1]-xp[j]) (a correctly rounded division), slope*(x-xp[j]) + fp[j] as a
// separate multiply and add, and the NaN retry from the other side.
#pragma once

#include <climits>
#include <cmath>

#include "common.hpp"

namespace pz {

constexpr int REGRID_GUESS_STEPS = 4;           // corrections of a guessed bracket before the binary search takes over

struct RegridBracket {
    int j, j0, j1;
    bool knot;
    double xv, x0, x1;
};

// The bracket of xv from numpy's index j (above); xp[i] is knot i (a pointer, or an accessor with operator[]).
template <class XP>
__device__ __forceinline__ RegridBracket regrid_bracket_at(int j, int nin, double xv, const XP &xp)
{
    RegridBracket b;
    const int last = nin - 1;
    const bool edge = (j < 0) || (j >= last);
    b.j = j;
    b.j0 = j < 0 ? 0 : (j >= last ? last : j);
    b.j1 = edge ? b.j0 : b.j0 + 1;
    b.xv = xv;
    b.x0 = xp[b.j0];
    b.x1 = xp[b.j1];
    b.knot = edge || (b.x0 == xv);
    return b;
}

// The bracket of xv in the contiguous grid xp[0..nin) by binary search.
__device__ __forceinline__ RegridBracket regrid_bracket(const double *xp, int nin, double xv)
{
    const int last = nin - 1;
    int j;
    if (xv != xv) j = -2;
    else if (xv > xp[last]) j = nin;
    else if (xv < xp[0]) j = -1;
    else {
        int lo = 0, hi = last;   // xp[lo] <= x <= xp[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (xv >= xp[mid]) lo = mid;
            else hi = mid;
        }
        j = (xv >= xp[hi]) ? hi : lo;
    }
    return regrid_bracket_at(j, nin, xv, xp);
}

// numpy's index for xv in xp[0..nin): the classes above (-2: NaN, -1: left, nin: right), else the last j with xp[j] <= xv.
// Cross-section grids are uniform, so with guess_step > 0 (knot j lies near guess_start + j guess_step) the bracket is guessed
// from (xv - guess_start) / guess_step and corrected against the grid ARRAY, at most REGRID_GUESS_STEPS knots either way;
// when the guess is further off than that (a grid that is not uniform after all) the binary search finds it.  Either way the
// index is the one numpy finds: the guess decides nothing.
__device__ __forceinline__ RegridBracket regrid_bracket_guess(const double *xp, int nin, double xv, double guess_start,
                                                              double guess_step)
{
    const int last = nin - 1;
    if (!(guess_step > 0.0) || xv != xv || xv > xp[last] || xv < xp[0]) return regrid_bracket(xp, nin, xv);
    double q = (xv - guess_start) / guess_step;
    q = q < 0.0 ? 0.0 : (q > (double)last ? (double)last : q);      // a NaN quotient (an infinite knot) becomes `last`
    int j = q == q ? (int)q : last;
    int steps = 0;
    while (j > 0 && xp[j] > xv && steps < REGRID_GUESS_STEPS) {
        --j;
        ++steps;
    }
    while (j < last && xp[j + 1] <= xv && steps < REGRID_GUESS_STEPS) {
        ++j;
        ++steps;
    }
    const bool found = xp[j] <= xv && (j == last || xv < xp[j + 1]);
    return found ? regrid_bracket_at(j, nin, xv, xp) : regrid_bracket(xp, nin, xv);
}

__device__ __forceinline__ double regrid_value(const double *row, const RegridBracket &b)
{
#pragma clang fp contract(off)
    const double y0 = row[b.j0], y1 = row[b.j1];
    if (b.j == -2) return b.xv;
    if (b.knot) return y0;
    const double slope = (y1 - y0) / (b.x1 - b.x0);
    double v = slope * (b.xv - b.x0) + y0;
    if (v != v) {
        v = slope * (b.xv - b.x1) + y1;
        if (v != v && y0 == y1) v = y0;
    }
    return v;
}

// np.interp(x, xp, fp, left, right) for the bracket b of x in the nin knots
__device__ __forceinline__ double regrid_value(const double *fp, const RegridBracket &b, int nin, double left, double right)
{
    if (b.j == -1) return left;
    if (b.j == nin) return right;
    return regrid_value(fp, b);
}

// Host side of regrid_bracket_guess, for the entry points of the two cross-section kernels: the row lengths they check alike
// (a source grid, when there is one, has at least 2 knots), and the guess_step the kernel gets: 0, "no guess", unless the
// step is positive and both numbers are finite.
inline int xsec_row_args(picaso_ctx *ctx, const char *who, long n_out, long n_src, bool has_grid, double guess_start,
                         double *guess_step)
{
    if (n_out < 1) return fail(ctx, "%s: n_out must be positive, got %ld", who, n_out);
    if (n_out > (long)INT_MAX || n_src > (long)INT_MAX)
        return fail(ctx, "%s: a row of %ld points (source %ld); rows hold at most %d", who, n_out, n_src, INT_MAX);
    if (has_grid && n_src < 2) return fail(ctx, "%s: a source grid needs at least 2 knots, got n_src = %ld", who, n_src);
    if (!(*guess_step > 0.0 && std::isfinite(*guess_step) && std::isfinite(guess_start))) *guess_step = 0.0;
    return 0;
}

}  // namespace pz
