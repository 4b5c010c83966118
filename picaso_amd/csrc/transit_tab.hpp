// What the transmission kernels share (transit.hip: the spectrum; contribfn.hip: its contribution function).
#pragma once
#include "common.hpp"

namespace pz {

constexpr int TRANSIT_BLOCK = 64;                   // wavelengths of one LDS tile, [layer][lane]
constexpr size_t TRANSIT_LDS_MAX = 160 * 1024;

// delta_length[nlevel*nlevel], zdz[nlevel], colden[nlayer], mmw_g[nlayer] of get_transit_1d's host arguments in a
// device table (fluxes.py:2623-2644), and the two scalars of its last line (:2660-2661).  `conditioned`: the chord
// segments without the cancellation of the reference's z^2 differences (the contribution function divides shares that
// span hundreds of e-foldings; the spectrum keeps the reference's bits)
int transit_tables(picaso_ctx *ctx, const double *z, const double *dz, int nlevel, double rstar, const double *mmw,
                   double k_b, double amu, const double *player, const double *tlayer, const double *colden,
                   const void **d_tab, double *zmin_term, double *two_over_rs2, bool conditioned);

}  // namespace pz
