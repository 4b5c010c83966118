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
//
// The same pass records WHICH LAYERS are cloud-free in every column (sets of up to 128 layers): ftau_cld == 0, dtau_og ==
// dtau, and ftau_ray / w0_og carrying the bit patterns of 1.0 / w0.  A cloud deck in a few of the layers is the usual
// atmosphere; in all the others six of the eight rows the LEVELS kernel reads hold constants and copies.  The fused five-
// angle launch takes the mask (DRV = 4, "LAYERS", toon_reflected.hip) and reads dtau and w0 alone there: 240 plane rows
// instead of 720 at 90 layers with a ten-layer cloud.  The mask lives and dies with its seal.  The bookkeeping itself is
// host-only code in planeseal_registry.hpp.
#include "common.hpp"
#include "planeseal.hpp"
#include "planeseal_registry.hpp"

namespace pz {

namespace {

using sealreg::Seal;
static_assert(sealreg::LEVELS_FLAGS == PICASO_SEAL_LEVELS, "planeseal_registry.hpp restates PICASO_SEAL_LEVELS");

// never destroyed: a buffer may be freed while the process shuts down, after the static destructors have run
sealreg::Registry &registry()
{
    static sealreg::Registry *r = new sealreg::Registry();
    return *r;
}

}  // namespace

bool seal_derivable(int device, const double *const planes[11], int nlevel, int nwno, long pitch,
                    unsigned long long *layer_mask, bool *mask_valid, unsigned long long *deck_mask, bool *w0_unit)
{
    uint64_t m[2], c[2];
    const bool ok = registry().derivable(device, planes, nlevel, nwno, pitch, m, mask_valid, c, w0_unit);
    if (layer_mask) {
        layer_mask[0] = m[0];
        layer_mask[1] = m[1];
    }
    if (deck_mask) {
        deck_mask[0] = c[0];
        deck_mask[1] = c[1];
    }
    return ok;
}

void seal_count_hit(int device, bool with_layer_mask) { registry().count_hit(device, with_layer_mask); }

void seal_invalidate(int device, const void *p, size_t bytes) { registry().invalidate(device, p, bytes); }

void seal_drop_device(int device) { registry().drop_device(device); }

// One lane per column, blockIdx.y = a run of SEAL_ROWS layers; every comparison needs only values of the planes
// themselves (tau[i + 1] against tau[i] + dtau[i] with the STORED tau[i]), so the runs are independent.  The rows read are
// the rows the solver reads: dtau, dtau_og, ftau_ray, gcos2 [0, nlayer), tau [0, nlayer], tau_og [0, nlayer) -- the
// solver never looks at tau_og[nlayer].  A NaN fails its comparison.  Lanes that found something OR their bits into
// one word (a vector atomic; none is issued for a set that passes).
//
// The clear-layer mask (notclear_out != nullptr: nlayer <= 128): a layer is NOT clear when some column has ftau_cld != 0
// or dtau_og != dtau (the solver's own two tests; a NaN fails them), or carries another bit pattern than 1.0 in ftau_ray
// or than w0's in w0_og -- those two values the LAYERS kernel puts in without loading them.  The lanes of a wave vote
// per layer; a wave that found a layer not clear ORs its eight bits (a run of SEAL_ROWS layers lies inside one 32-bit
// word) into the array with one vector atomic from its first lane.  A cloud-free set issues none.
//
// Two more facts from the same loads, kept with the mask and never handed to a caller (the LAYERS kernel's cloud-run loop
// and its small-argument EP, toon_reflected.hip):
//   * the deck mask: a layer is NOT a deck layer when some column has ftau_cld == 0 or dtau_og == dtau -- the two
//     comparisons prep() votes on, so a column with a NaN in either plane counts as cloudy and delta-scaled there as it
//     does here.  Voted and ORed like the clear mask into a second set of words; most layers of most sets are no deck
//     layers and most waves would send the same bits, so a wave looks at the word first and sends only bits it misses (a
//     stale look costs an atomic, never a bit);
//   * one word that stays 0 while every w0 read lies in [0, 1] (a NaN fails that).
constexpr int SEAL_BLOCK = 256, SEAL_ROWS = 8;
static_assert(32 % SEAL_ROWS == 0, "the layers of one block lie inside one word of the mask");
constexpr int SEAL_MASK_WORDS = sealreg::MASK_LAYERS / 32;
// the device buffer: flags found bad, the clear-mask words, the deck-mask words, w0 found outside [0, 1]
constexpr int SEAL_WORDS = 1 + 2 * SEAL_MASK_WORDS + 1;

__global__ __launch_bounds__(SEAL_BLOCK) void k_planes_seal(int nlayer, int nwno, long pitch, const double *dtau,
                                                             const double *tau, const double *gcos2,
                                                             const double *ftau_ray, const double *dtau_og,
                                                             const double *tau_og, const double *w0,
                                                             const double *ftau_cld, const double *w0_og, int *bad_out,
                                                             unsigned *notclear_out)
{
#pragma clang fp contract(off)      // the solver's own unfused operations
    const long col = (long)blockIdx.x * SEAL_BLOCK + threadIdx.x;
    if (col >= nwno) return;
    const int i0 = (int)blockIdx.y * SEAL_ROWS, i1 = (i0 + SEAL_ROWS < nlayer) ? i0 + SEAL_ROWS : nlayer;
    int bad = 0;
    unsigned notclear = 0;                           // wave-uniform: bit (i & 31) = some lane of this wave saw cloud in layer i
    unsigned lane_cloudy = 0;                        // this lane's own findings, bit (i - i0)
    unsigned notdeck = 0, lane_notdeck = 0;          // the same for "not cloudy and delta-scaled"
    bool w0_out = false;
    double t = tau[(long)i0 * pitch + col], to = tau_og[(long)i0 * pitch + col];
    if (i0 == 0) {                                   // the sums start from +0.0 (the bit pattern: -0.0 is another start)
        if (__double_as_longlong(t) != 0) bad |= PICASO_SEAL_TAU;
        if (__double_as_longlong(to) != 0) bad |= PICASO_SEAL_TAU_OG;
    }
#pragma unroll 4
    for (int i = i0; i < i1; ++i) {
        const long o = (long)i * pitch + col;
        const double tn = tau[o + pitch];
        const double dt = dtau[o], dto = dtau_og[o], fr = ftau_ray[o];
        if (!(tn == t + dt)) bad |= PICASO_SEAL_TAU;
        t = tn;
        if (i + 1 < nlayer) {
            const double ton = tau_og[o + pitch];
            if (!(ton == to + dto)) bad |= PICASO_SEAL_TAU_OG;
            to = ton;
        }
        if (!(gcos2[o] == 0.5 * fr)) bad |= PICASO_SEAL_GCOS2;
        if (notclear_out) {
            const double fc = ftau_cld[o], w = w0[o];
            const bool cloudy = !(fc == 0.0) || !(dto == dt) ||
                                __double_as_longlong(fr) != __double_as_longlong(1.0) ||
                                __double_as_longlong(w0_og[o]) != __double_as_longlong(w);
            if (cloudy) lane_cloudy |= 1u << (i - i0);
            if (fc == 0.0 || dto == dt) lane_notdeck |= 1u << (i - i0);
            if (!(w >= 0.0 && w <= 1.0)) w0_out = true;
        }
    }
    // (the votes after the loop: a vote inside it would keep the loop from being unrolled)
#pragma unroll
    for (int b = 0; b < SEAL_ROWS; ++b)
        if (__any((lane_cloudy >> b) & 1u)) notclear |= 1u << ((i0 & 31) + b);
#pragma unroll
    for (int b = 0; b < SEAL_ROWS; ++b)
        if (__any((lane_notdeck >> b) & 1u)) notdeck |= 1u << ((i0 & 31) + b);
    const bool any_w0_out = __any(w0_out);
    if (bad) atomicOr(bad_out, bad);
    if (notclear && (threadIdx.x & 63) == 0) atomicOr(notclear_out + (i0 >> 5), notclear);   // lane 0 is active if any is
    if (notclear_out && (threadIdx.x & 63) == 0) {
        unsigned *deck_word = notclear_out + SEAL_MASK_WORDS + (i0 >> 5), *w0_word = notclear_out + 2 * SEAL_MASK_WORDS;
        if (notdeck & ~__hip_atomic_load(deck_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(deck_word, notdeck);
        if (any_w0_out && !__hip_atomic_load(w0_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(w0_word, 1u);
    }
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
    PZ_TRY(picaso_dev_malloc(ctx, sizeof(int) * SEAL_WORDS, &word));
    int found[SEAL_WORDS] = {0};
    const int nlayer = nlevel - 1;
    const bool with_mask = nlayer <= sealreg::MASK_LAYERS;
    auto run = [&]() -> int {
        PZ_HIP(ctx, hipMemsetAsync(word, 0, sizeof(int) * SEAL_WORDS, ctx->stream));
        const dim3 grid((unsigned)((nwno + SEAL_BLOCK - 1) / SEAL_BLOCK), (unsigned)((nlayer + SEAL_ROWS - 1) / SEAL_ROWS));
        hipLaunchKernelGGL(k_planes_seal, grid, dim3(SEAL_BLOCK), 0, ctx->stream, nlayer, nwno, plane_pitch, dtau, tau,
                           gcos2, ftau_ray, dtau_og, tau_og, w0, ftau_cld, w0_og, (int *)word,
                           with_mask ? (unsigned *)word + 1 : nullptr);
        PZ_HIP(ctx, hipGetLastError());
        PZ_HIP(ctx, hipMemcpyAsync(found, word, sizeof(int) * SEAL_WORDS, hipMemcpyDeviceToHost, ctx->stream));
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
    s.flags = PICASO_SEAL_LEVELS & ~found[0];
    sealreg::mask_from_device_words(s, with_mask ? (const unsigned *)found + 1 : nullptr,
                                    with_mask ? (const unsigned *)found + 1 + SEAL_MASK_WORDS : nullptr,
                                    with_mask && found[1 + 2 * SEAL_MASK_WORDS] == 0);
    registry().record(ctx->device, s);
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
    registry().stat(ctx->device, seals, hits, nullptr);
    return 0;
}

int picaso_reflected_seal_layers(picaso_ctx *ctx, const void *any_plane_ptr, int cap, int *clear_out, int *nlayer_out)
{
    if (!ctx) return fail(nullptr, "null context");
    if (!nlayer_out || cap < 0 || (cap > 0 && !clear_out)) return fail(ctx, "reflected_seal_layers: bad arguments");
    *nlayer_out = registry().layers(ctx->device, any_plane_ptr, cap, clear_out);
    return 0;
}

int picaso_reflected_seal_layers_stat(picaso_ctx *ctx, long *mask_launches)
{
    if (!ctx) return fail(nullptr, "null context");
    registry().stat(ctx->device, nullptr, nullptr, mask_launches);
    return 0;
}

}  // extern "C"
