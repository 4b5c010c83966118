// Seals of resident reflected plane sets: the test "tau / tau_og are the running sums of dtau / dtau_og from +0 and gcos2
// is 0.5 ftau_ray" made ONCE, where the planes enter the device, instead of in every wave of every layer of every launch.
//
// k_reflected_toa and k_reflected_coop handed all eleven planes compare, per layer and per wave, the caller's level
// planes with the sums they carry anyway (prep() / layer_flags(): bit-exact comparisons) and read tau, tau_og and gcos2
// -- 272 of 992 plane rows at 90 layers -- to do so.  The variants that are told at compile time that the three planes
// are absent (DRV = 3, "LEVELS") form the same numbers with the same operations and skip loads, tests and branches:
// 0.2085 ms against 0.223 ms at 1e5 columns x 90 layers x 5 angles.  A seal lets a caller that keeps all eleven planes
// resident (picaso_amd/resident.py: many geometries on one atmosphere, wavelength shards, the benchmark loop) have
// that variant: picaso_reflected_planes_seal_dev verifies the set with one pass over the six planes involved and
// records it; reflected_1d_core (api.hip) looks the eleven addresses up and, where the launch would take a compile-time
// variant, treats the three planes as absent.  Same bits: when the flags hold, tau[i+1] IS tau[i] + dtau[i].
//
// The registry is process-wide (every context of a device sees a seal), keyed by device, guarded by one mutex.  A seal
// dies when the library sees its bytes change or go away: picaso_dev_free, the picaso_memcpy_h2d* / _d2d / picaso_memset
// calls whose destination overlaps a plane, picaso_pool_trim, picaso_ctx_destroy.  Writes the library cannot see
// (a kernel's output, another process) are the caller's to announce with picaso_reflected_planes_unseal.
#include "common.hpp"
#include "planeseal.hpp"

#include <atomic>
#include <cstdint>
#include <map>
#include <mutex>

namespace pz {

namespace {

struct Seal {
    const double *plane[11];
    int nlevel, nwno;
    long pitch;
    int flags;

    // bytes of plane j the solver may read: rows of `pitch` elements, the last one `nwno` long
    size_t extent(int j) const
    {
        const long rows = (j == 1 || j == 8) ? nlevel : nlevel - 1;      // tau and tau_og are level planes
        return sizeof(double) * (size_t)((rows - 1) * pitch + nwno);
    }
    bool overlaps(const void *p, size_t bytes) const
    {
        const uintptr_t lo = (uintptr_t)p, hi = lo + bytes;
        for (int j = 0; j < 11; ++j) {
            const uintptr_t q = (uintptr_t)plane[j];
            if (lo < q + extent(j) && q < hi) return true;
        }
        return false;
    }
    bool same_set(const double *const p[11]) const
    {
        for (int j = 0; j < 11; ++j)
            if (plane[j] != p[j]) return false;
        return true;
    }
};

struct DeviceSeals {
    std::vector<Seal> seals;
    long hits = 0;
};

struct Registry {
    std::mutex mu;
    std::map<int, DeviceSeals> dev;
};

// never destroyed: a buffer may be freed while the process shuts down, after the static destructors have run
Registry &registry()
{
    static Registry *r = new Registry();
    return *r;
}
std::atomic<long> g_records{0};      // seals of all devices: the copies and frees of a process without seals skip the mutex

long drop_where(DeviceSeals &d, bool (*pred)(const Seal &, const void *, size_t), const void *p, size_t bytes)
{
    long n = 0;
    for (size_t k = d.seals.size(); k-- > 0;)
        if (pred(d.seals[k], p, bytes)) {
            d.seals.erase(d.seals.begin() + (long)k);
            ++n;
        }
    g_records -= n;
    return n;
}

}  // namespace

bool seal_derivable(int device, const double *const planes[11], int nlevel, int nwno, long pitch)
{
    if (g_records.load(std::memory_order_relaxed) == 0) return false;
    Registry &r = registry();
    std::lock_guard<std::mutex> lock(r.mu);
    auto it = r.dev.find(device);
    if (it == r.dev.end()) return false;
    for (const Seal &s : it->second.seals)
        if (s.same_set(planes))
            return s.nlevel == nlevel && s.nwno == nwno && s.pitch == pitch &&
                   (s.flags & PICASO_SEAL_LEVELS) == PICASO_SEAL_LEVELS;
    return false;
}

void seal_count_hit(int device)
{
    Registry &r = registry();
    std::lock_guard<std::mutex> lock(r.mu);
    ++r.dev[device].hits;
}

void seal_invalidate(int device, const void *p, size_t bytes)
{
    if (!p || !bytes || g_records.load(std::memory_order_relaxed) == 0) return;
    Registry &r = registry();
    std::lock_guard<std::mutex> lock(r.mu);
    auto it = r.dev.find(device);
    if (it == r.dev.end()) return;
    drop_where(it->second, [](const Seal &s, const void *q, size_t n) { return s.overlaps(q, n); }, p, bytes);
}

void seal_drop_device(int device)
{
    if (g_records.load(std::memory_order_relaxed) == 0) return;
    Registry &r = registry();
    std::lock_guard<std::mutex> lock(r.mu);
    auto it = r.dev.find(device);
    if (it == r.dev.end()) return;
    drop_where(it->second, [](const Seal &, const void *, size_t) { return true; }, nullptr, 0);
}

// One lane per column, blockIdx.y = a run of SEAL_ROWS layers; every comparison needs only values of the planes
// themselves (tau[i + 1] against tau[i] + dtau[i] with the STORED tau[i]), so the runs are independent.  The rows read are
// the rows the solver reads: dtau, dtau_og, ftau_ray, gcos2 [0, nlayer), tau [0, nlayer], tau_og [0, nlayer) -- the
// solver never looks at tau_og[nlayer].  A NaN fails its comparison.  Lanes that found something OR their bits into
// one word (a vector atomic; none is issued for a set that passes).
constexpr int SEAL_BLOCK = 256, SEAL_ROWS = 8;

__global__ __launch_bounds__(SEAL_BLOCK) void k_planes_seal(int nlayer, int nwno, long pitch, const double *dtau,
                                                             const double *tau, const double *gcos2,
                                                             const double *ftau_ray, const double *dtau_og,
                                                             const double *tau_og, int *bad_out)
{
#pragma clang fp contract(off)      // the solver's own unfused operations
    const long col = (long)blockIdx.x * SEAL_BLOCK + threadIdx.x;
    if (col >= nwno) return;
    const int i0 = (int)blockIdx.y * SEAL_ROWS, i1 = (i0 + SEAL_ROWS < nlayer) ? i0 + SEAL_ROWS : nlayer;
    int bad = 0;
    double t = tau[(long)i0 * pitch + col], to = tau_og[(long)i0 * pitch + col];
    if (i0 == 0) {                                   // the sums start from +0.0 (the bit pattern: -0.0 is another start)
        if (__double_as_longlong(t) != 0) bad |= PICASO_SEAL_TAU;
        if (__double_as_longlong(to) != 0) bad |= PICASO_SEAL_TAU_OG;
    }
#pragma unroll 4
    for (int i = i0; i < i1; ++i) {
        const long o = (long)i * pitch + col;
        const double tn = tau[o + pitch];
        if (!(tn == t + dtau[o])) bad |= PICASO_SEAL_TAU;
        t = tn;
        if (i + 1 < nlayer) {
            const double ton = tau_og[o + pitch];
            if (!(ton == to + dtau_og[o])) bad |= PICASO_SEAL_TAU_OG;
            to = ton;
        }
        if (!(gcos2[o] == 0.5 * ftau_ray[o])) bad |= PICASO_SEAL_GCOS2;
    }
    if (bad) atomicOr(bad_out, bad);
}

}  // namespace pz

using namespace pz;

extern "C" {

int picaso_reflected_planes_seal_dev(picaso_ctx *ctx, int nlevel, int nwno, long plane_pitch, const double *dtau,
                                     const double *tau, const double *w0, const double *cosb, const double *gcos2,
                                     const double *ftau_cld, const double *ftau_ray, const double *dtau_og,
                                     const double *tau_og, const double *w0_og, const double *cosb_og, int *flags_out)
{
    if (!ctx) return fail(nullptr, "null context");
    if (flags_out) *flags_out = 0;
    if (nlevel < 2 || nwno < 1) return fail(ctx, "reflected_planes_seal: bad sizes nlevel=%d nwno=%d", nlevel, nwno);
    if (plane_pitch < nwno) return fail(ctx, "reflected_planes_seal: plane_pitch %ld < %d columns", plane_pitch, nwno);
    PZ_NEED(ctx, "reflected_planes_seal", dtau, tau, w0, cosb, gcos2, ftau_cld, ftau_ray, dtau_og, tau_og, w0_og, cosb_og);
    PZ_HIP(ctx, hipSetDevice(ctx->device));
    void *word = nullptr;
    PZ_TRY(picaso_dev_malloc(ctx, sizeof(int), &word));
    int bad = 0;
    auto run = [&]() -> int {
        const int nlayer = nlevel - 1;
        PZ_HIP(ctx, hipMemsetAsync(word, 0, sizeof(int), ctx->stream));
        const dim3 grid((unsigned)((nwno + SEAL_BLOCK - 1) / SEAL_BLOCK), (unsigned)((nlayer + SEAL_ROWS - 1) / SEAL_ROWS));
        hipLaunchKernelGGL(k_planes_seal, grid, dim3(SEAL_BLOCK), 0, ctx->stream, nlayer, nwno, plane_pitch, dtau, tau,
                           gcos2, ftau_ray, dtau_og, tau_og, (int *)word);
        PZ_HIP(ctx, hipGetLastError());
        PZ_HIP(ctx, hipMemcpyAsync(&bad, word, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        PZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return 0;
    };
    const int rc = run();
    PZ_TRY(picaso_dev_free(ctx, word));
    if (rc) return rc;
    Seal s{};
    const double *pl[11] = {dtau, tau, w0, cosb, gcos2, ftau_cld, ftau_ray, dtau_og, tau_og, w0_og, cosb_og};
    for (int j = 0; j < 11; ++j) s.plane[j] = pl[j];
    s.nlevel = nlevel;
    s.nwno = nwno;
    s.pitch = plane_pitch;
    s.flags = PICASO_SEAL_LEVELS & ~bad;
    {
        Registry &r = registry();
        std::lock_guard<std::mutex> lock(r.mu);
        DeviceSeals &d = r.dev[ctx->device];
        // a second seal of the same eleven addresses replaces the first
        drop_where(d, [](const Seal &x, const void *q, size_t) { return x.same_set((const double *const *)q); }, pl, 0);
        d.seals.push_back(s);
        ++g_records;
    }
    if (flags_out) *flags_out = s.flags;
    return 0;
}

int picaso_reflected_planes_unseal(picaso_ctx *ctx, const void *any_plane_ptr)
{
    if (!ctx) return fail(nullptr, "null context");
    seal_invalidate(ctx->device, any_plane_ptr, 1);
    return 0;
}

int picaso_reflected_seal_stat(picaso_ctx *ctx, long *seals, long *hits)
{
    if (!ctx) return fail(nullptr, "null context");
    Registry &r = registry();
    std::lock_guard<std::mutex> lock(r.mu);
    auto it = r.dev.find(ctx->device);
    long n = 0;
    if (it != r.dev.end())
        for (const Seal &s : it->second.seals) n += (s.flags & PICASO_SEAL_LEVELS) == PICASO_SEAL_LEVELS;
    if (seals) *seals = n;
    if (hits) *hits = it != r.dev.end() ? it->second.hits : 0;
    return 0;
}

}  // extern "C"
