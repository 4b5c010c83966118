// fluxes.blackbody's device function (reference picaso/fluxes.py:1660-1680), shared by planck.hip and contribfn.hip.
#pragma once
#include "device_math.hpp"

namespace pz {

// planck_lambda of device_math.hpp takes a wavenumber and forms wcm = 1/wno; the public function is handed the
// wavelength itself (the reference's thermal call passes 1/wno, so both see the same wcm bits)
__device__ __forceinline__ double planck_lambda_cm(double t, double wcm)
{
#pragma clang fp contract(off)
    const double h = 6.62607004e-27, c = 2.99792458e+10, k = 1.38064852e-16;
    const double w2 = wcm * wcm;
    return ((2.0 * h * (c * c)) / (w2 * w2 * wcm)) * planck_rcp(fexp(fdiv(h * c, t * (wcm * k))));
}

}  // namespace pz
