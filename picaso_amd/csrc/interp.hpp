// numpy.interp's arithmetic for one x against a nondecreasing grid (numpy/_core/src/multiarray/compiled_base.c:arr_interp),
// shared by the kernels that restate it: the cloud-table regrid (k_regrid_rows, k_regrid_facets, the fused gas + mixing
// launch: reference wavelength.regrid, wavelength.py:46-70) and the tau-pressure of a contribution run (k_contribution_columns:
// find_press, justdoit.py:1281-1292).
//
// The bracket: j = -2 for a NaN x, -1 left of the grid, nin right of it, else the LAST index with xp[j] <= x (what numpy's
// binary_search_with_guess returns; on a grid with ties, e.g. the zero cumulative optical depth above a cloud deck, the last
// of the tied knots).  Then numpy's rules: NaN x -> x; left -> fp[0]; right or j the last knot -> fp[last]; a knot hit ->
// fp[j]; otherwise slope = (fp[j+1]-fp[j])/(xp[j+1]-xp[j]) (a correctly rounded division), slope*(x-xp[j]) + fp[j] as a
// separate multiply and add, and the NaN retry from the other side.
#pragma once

namespace pz {

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

}  // namespace pz
