// Mie efficiencies of a list of spheres: Qext, Qsca and g Qsca per (size parameter x, refractive index m = n + ik), the
// producer of a Mie table (picaso_amd/mie.py: compute_mieff).  The arithmetic is the one stated in picaso_amd/mie.py and
// restated there in numpy (mie_efficiencies_numpy), operation by operation: complex products as (ac - bd, ad + bc),
// complex quotients by Smith's algorithm as numpy forms them, IEEE divisions, nothing contracted.  What is left between the
// two is the library's sin and cos of x (a common factor of psi and chi) -- tests/test_mie_gpu.py holds both to mpmath.
//
// Shape.  Both recurrences are sequential in n, so one lane carries one sphere, and the trip counts of a list span 1 to
// ~4e4.  The caller sorts the list by nmx (largest first: the long waves start first and the short ones fill in behind
// them) and a wave takes 64 neighbours of the sorted list; its loops run on the wave's largest count with the lanes that
// have not begun or are done masked off, so the lanes of a wave are at the same n at the same time.  The downward pass
// leaves D_n(y) and D_n(x), n = 1 .. nstop, for the upward pass in a scratch buffer: 24 bytes per term and lane (the terms
// above nstop are never read again and never stored), term-major within the wave -- row n holds the wave's 64 values of
// Re D_n(y), then of Im D_n(y), then of D_n(x) -- so that every access of a wave is three runs of 512 consecutive bytes.
// A wave's rows: the largest nstop of its lanes.  The host lays the waves' blocks end to end and checks the total against
// the buffer; every index the kernel forms follows from the two order arrays the entry point has checked.  A lane's
// bits depend on its own x and m alone.
#include "common.hpp"

#include <climits>

#pragma clang fp contract(off)

namespace pz {

constexpr int MIE_WAVE = 64;

struct MieArgs {
    const double *x, *m_re, *m_im;          // (n)
    const int *nstop, *nmx;                 // (n): 0, 0 marks an element that is not evaluated (NaN)
    const long *wave_base;                  // (nwave): first double of the wave's scratch block
    const int *wave_rows, *wave_top;        // (nwave): largest nstop, largest nmx of the wave's lanes
    double *scratch;
    double *out;                            // (3, n): qext, qsca, g qsca
    long n;
};

struct Cplx {
    double re, im;
};

// 1 / b as Smith's algorithm leaves it for the quotients by b that follow: a / b = quot(a, inv)
struct SmithInv {
    double rat, scl;
    bool real_major;                        // |Re b| >= |Im b|
};

__device__ __forceinline__ SmithInv smith(const Cplx b)
{
#pragma clang fp contract(off)
    SmithInv s;
    s.real_major = fabs(b.re) >= fabs(b.im);
    if (s.real_major) {
        s.rat = b.im / b.re;
        s.scl = 1.0 / (b.re + b.im * s.rat);
    } else {
        s.rat = b.re / b.im;
        s.scl = 1.0 / (b.im + b.re * s.rat);
    }
    return s;
}

__device__ __forceinline__ Cplx quot(const Cplx a, const SmithInv s)
{
#pragma clang fp contract(off)
    if (s.real_major) return {(a.re + a.im * s.rat) * s.scl, (a.im - a.re * s.rat) * s.scl};
    return {(a.re * s.rat + a.im) * s.scl, (a.im * s.rat - a.re) * s.scl};
}

__device__ __forceinline__ Cplx mul(const Cplx a, const Cplx b)
{
#pragma clang fp contract(off)
    return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}

__global__ __launch_bounds__(MIE_WAVE) void k_mie_q(const MieArgs a)
{
#pragma clang fp contract(off)
    const long w = blockIdx.x;
    const int lane = threadIdx.x;
    const long i = w * MIE_WAVE + lane;
    const bool have = i < a.n;
    double x = 1.0;
    Cplx m = {1.0, 0.0};
    int nstop = 0, nmx = 0;
    if (have) {
        x = a.x[i];
        m = {a.m_re[i], a.m_im[i]};
        nstop = a.nstop[i];
        nmx = a.nmx[i];
    }
    const bool ok = have && nstop >= 1 && x > 0.0 && m.im >= 0.0 && m.re == m.re;
    if (!ok) {
        nstop = nmx = 0;
        x = 1.0;
        m = {1.0, 0.0};
    }
    const int top = a.wave_top[w], rows = a.wave_rows[w];
    double *const rows_at = a.scratch + a.wave_base[w] + lane;          // row n: rows_at + (n - 1) * 3 * MIE_WAVE

    const Cplx y = mul(m, {x, 0.0});
    const SmithInv iy = smith(y), im_ = smith(m);
    Cplx cy = {0.0, 0.0};
    double cx = 0.0;
    for (int n = top; n >= 1; --n) {                    // D_{n-1} from D_n, for the lanes that have begun
        if (n > nmx) continue;
        const double dn = (double)n;
        const Cplx ny = quot({dn, 0.0}, iy);
        const Cplx t = {cy.re + ny.re, cy.im + ny.im};
        const Cplx r = quot({1.0, 0.0}, smith(t));
        cy = {ny.re - r.re, ny.im - r.im};
        const double nx = dn / x;
        cx = nx - 1.0 / (cx + nx);
        if (n >= 2 && n - 1 <= nstop) {
            double *const row = rows_at + (long)(n - 2) * 3 * MIE_WAVE;
            row[0] = cy.re;
            row[MIE_WAVE] = cy.im;
            row[2 * MIE_WAVE] = cx;
        }
    }

    double psi1 = sin(x), chi1 = cos(x), chi2 = -psi1;  // psi_{n-1}, chi_{n-1}, chi_{n-2}
    Cplx a1 = {0.0, 0.0}, b1 = {0.0, 0.0};
    double qext = 0.0, qsca = 0.0, gqsc = 0.0;
    for (int n = 1; n <= rows; ++n) {
        if (n > nstop) continue;
        const double *const row = rows_at + (long)(n - 1) * 3 * MIE_WAVE;
        const Cplx dy = {row[0], row[MIE_WAVE]};
        const double dx = row[2 * MIE_WAVE];
        const double dn = (double)n;
        const double nx = dn / x;
        const double psi = psi1 / (dx + nx);
        const double chi = (double)(2 * n - 1) / x * chi1 - chi2;
        const Cplx xi = {psi, -chi}, xi1 = {psi1, -chi1};
        Cplx ca = quot(dy, im_), cb = mul(m, dy);
        ca.re = ca.re + nx;
        cb.re = cb.re + nx;
        const Cplx pa = mul(ca, xi), pb = mul(cb, xi);
        const Cplx an = quot({ca.re * psi - psi1, ca.im * psi}, smith({pa.re - xi1.re, pa.im - xi1.im}));
        const Cplx bn = quot({cb.re * psi - psi1, cb.im * psi}, smith({pb.re - xi1.re, pb.im - xi1.im}));
        const double t1 = (double)(2 * n + 1);
        qext = qext + t1 * (an.re + bn.re);
        qsca = qsca + t1 * ((an.re * an.re + an.im * an.im) + (bn.re * bn.re + bn.im * bn.im));
        const double c1 = t1 / (dn * (dn + 1.0)), c2 = (dn - 1.0) * (dn + 1.0) / dn;
        gqsc = gqsc + (c1 * (an.re * bn.re + an.im * bn.im)
                       + c2 * ((a1.re * an.re + a1.im * an.im) + (b1.re * bn.re + b1.im * bn.im)));
        psi1 = psi;
        chi2 = chi1;
        chi1 = chi;
        a1 = an;
        b1 = bn;
    }
    if (!have) return;
    const double nan = __builtin_nan("");
    const double x2 = x * x;
    a.out[i] = ok ? 2.0 / x2 * qext : nan;
    a.out[a.n + i] = ok ? 2.0 / x2 * qsca : nan;
    a.out[2 * a.n + i] = ok ? 4.0 / x2 * gqsc : nan;
}

}  // namespace pz

using namespace pz;

extern "C" int picaso_mie_q_dev(picaso_ctx *ctx, long n, const double *x, const double *m_re, const double *m_im,
                                const int *nstop, const int *nmx, double *scratch, size_t scratch_bytes, double *out)
{
    const char *who = "picaso_mie_q_dev";
    if (!ctx) return fail(ctx, "%s: null context", who);
    if (n < 1) return fail(ctx, "%s: n must be at least 1, got %ld", who, n);
    PZ_NEED(ctx, who, x, m_re, m_im, nstop, nmx, out);
    const long nwave = (n + MIE_WAVE - 1) / MIE_WAVE;
    if (nwave > INT_MAX) return fail(ctx, "%s: %ld evaluations are more than one launch takes", who, n);
    std::vector<long> base(nwave);
    std::vector<int> rows(nwave), top(nwave);
    size_t need = 0;                                    // doubles of scratch
    for (long w = 0; w < nwave; ++w) {
        int r = 0, t = 0;
        for (long i = w * MIE_WAVE; i < std::min(n, (w + 1) * MIE_WAVE); ++i) {
            if (nmx[i] > PICASO_MIE_NMX_CAP)
                return fail(ctx, "%s: element %ld needs a series of %d terms; at most %d are taken (x of about 1e6)", who, i,
                            nmx[i], PICASO_MIE_NMX_CAP);
            if (nstop[i] < 0 || nmx[i] < 0 || (nmx[i] == 0 ? nstop[i] != 0 : nstop[i] >= nmx[i]))
                return fail(ctx, "%s: element %ld has nstop = %d and nmx = %d; 0 <= nstop < nmx, or both 0", who, i, nstop[i],
                            nmx[i]);
            r = std::max(r, nstop[i]);
            t = std::max(t, nmx[i]);
        }
        base[w] = (long)need;
        rows[w] = r;
        top[w] = t;
        need += (size_t)r * 3 * MIE_WAVE;
    }
    if (need * sizeof(double) > scratch_bytes)
        return fail(ctx, "%s: the list needs %zu bytes of scratch, the buffer holds %zu", who, need * sizeof(double),
                    scratch_bytes);
    if (need && !scratch) return fail(ctx, "%s: a required array argument is NULL (scratch)", who);
    PZ_HIP(ctx, hipSetDevice(ctx->device));
    PZ_TRY(arena_reset(ctx, (size_t)n * 32 + (size_t)nwave * 16 + 8 * 256));
    MieArgs a{};
    PZ_TRY(arena_upload(ctx, x, (size_t)n, &a.x));
    PZ_TRY(arena_upload(ctx, m_re, (size_t)n, &a.m_re));
    PZ_TRY(arena_upload(ctx, m_im, (size_t)n, &a.m_im));
    PZ_TRY(arena_upload(ctx, nstop, (size_t)n, &a.nstop));
    PZ_TRY(arena_upload(ctx, nmx, (size_t)n, &a.nmx));
    PZ_TRY(arena_upload(ctx, base.data(), (size_t)nwave, &a.wave_base));
    PZ_TRY(arena_upload(ctx, rows.data(), (size_t)nwave, &a.wave_rows));
    PZ_TRY(arena_upload(ctx, top.data(), (size_t)nwave, &a.wave_top));
    a.scratch = scratch;
    a.out = out;
    a.n = n;
    hipLaunchKernelGGL(k_mie_q, dim3((unsigned)nwave), dim3(MIE_WAVE), 0, ctx->stream, a);
    PZ_HIP(ctx, hipGetLastError());
    // the order tables and the wave records are host vectors of this call: the copies above have read them by now
    PZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}
