// The registry of sealed plane sets (planeseal.hip): host-only bookkeeping, no device call and no HIP header, so that a
// stand-alone program can drive it under a sanitizer (tools/seal_registry_check.cpp).  Included by planeseal.hip alone.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <map>
#include <mutex>
#include <vector>

namespace pz {
namespace sealreg {

constexpr int LEVELS_FLAGS = 7;          // PICASO_SEAL_LEVELS (picaso_hip.h; planeseal.hip asserts the two agree)
constexpr int MASK_LAYERS = 128;         // layers a clear-layer mask covers: sets with more record none

struct Seal {
    const double *plane[11];
    int nlevel, nwno;
    long pitch;
    int flags;
    // bit i: layer i is cloud-free in every column (k_planes_seal); meaningful only with mask_valid
    uint64_t clear[2];
    bool mask_valid;
    // bit i: layer i is cloudy AND delta-scaled in every column -- !(ftau_cld == 0) and !(dtau_og == dtau), the solver's
    // own two comparisons negated per column, so a NaN counts as cloudy as it does in the solver's votes; meaningful only
    // with mask_valid.  Disjoint from clear[].
    uint64_t deck[2];
    // every w0 of the set lies in [0, 1] (a NaN fails it); false without a mask
    bool w0_unit;

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
    bool sealed() const { return (flags & LEVELS_FLAGS) == LEVELS_FLAGS; }
    bool layer_clear(int i) const { return mask_valid && i >= 0 && i < MASK_LAYERS && ((clear[i >> 6] >> (i & 63)) & 1u); }
};

// The mask of a seal from what k_planes_seal left behind: `notclear` holds one bit per layer (32 per word, MASK_LAYERS / 32
// words) set by the waves that found a column with cloud.  Bits at and above nlayer stay 0 in the result.
// `notdeck`, in the same layout, holds the bits set by the waves that found a column that is not both cloudy and delta-
// scaled; `w0_unit` is what the pass found for w0.  Without them (or without a mask) the seal records no deck layer.
inline void mask_from_device_words(Seal &s, const unsigned *notclear, const unsigned *notdeck = nullptr,
                                   bool w0_unit = false)
{
    const int nlayer = s.nlevel - 1;
    s.clear[0] = s.clear[1] = 0;
    s.deck[0] = s.deck[1] = 0;
    s.w0_unit = false;
    s.mask_valid = notclear != nullptr && nlayer <= MASK_LAYERS;
    if (!s.mask_valid) return;
    s.w0_unit = w0_unit;
    for (int i = 0; i < nlayer; ++i) {
        const bool clear = !((notclear[i >> 5] >> (i & 31)) & 1u);
        if (clear) s.clear[i >> 6] |= (uint64_t)1 << (i & 63);
        // (a layer no wave found cloudy is no deck layer, whatever the second set of words says)
        if (!clear && notdeck && !((notdeck[i >> 5] >> (i & 31)) & 1u)) s.deck[i >> 6] |= (uint64_t)1 << (i & 63);
    }
}

struct DeviceSeals {
    std::vector<Seal> seals;
    long hits = 0;
    long mask_launches = 0;
};

struct Registry {
    std::mutex mu;
    std::map<int, DeviceSeals> dev;
    std::atomic<long> records{0};      // seals of all devices: the copies and frees of a process without seals skip the mutex

    long drop_where(DeviceSeals &d, bool (*pred)(const Seal &, const void *, size_t), const void *p, size_t bytes)
    {
        long n = 0;
        for (size_t k = d.seals.size(); k-- > 0;)
            if (pred(d.seals[k], p, bytes)) {
                d.seals.erase(d.seals.begin() + (long)k);
                ++n;
            }
        records -= n;
        return n;
    }

    // a second seal of the same eleven addresses replaces the first
    void record(int device, const Seal &s)
    {
        std::lock_guard<std::mutex> lock(mu);
        DeviceSeals &d = dev[device];
        drop_where(d, [](const Seal &x, const void *q, size_t) { return x.same_set((const double *const *)q); }, s.plane, 0);
        d.seals.push_back(s);
        ++records;
    }

    // mask, mask_valid (may be null): the seal's clear-layer mask and whether it recorded one (both words 0 when not);
    // deck, w0_unit (may be null): its deck-layer mask and its finding about w0, handed out with the mask only
    bool derivable(int device, const double *const planes[11], int nlevel, int nwno, long pitch, uint64_t *mask,
                   bool *mask_valid, uint64_t *deck = nullptr, bool *w0_unit = nullptr)
    {
        if (mask) mask[0] = mask[1] = 0;
        if (mask_valid) *mask_valid = false;
        if (deck) deck[0] = deck[1] = 0;
        if (w0_unit) *w0_unit = false;
        if (records.load(std::memory_order_relaxed) == 0) return false;
        std::lock_guard<std::mutex> lock(mu);
        auto it = dev.find(device);
        if (it == dev.end()) return false;
        for (const Seal &s : it->second.seals)
            if (s.same_set(planes)) {
                const bool ok = s.nlevel == nlevel && s.nwno == nwno && s.pitch == pitch && s.sealed();
                if (ok && s.mask_valid) {
                    if (mask) {
                        mask[0] = s.clear[0];
                        mask[1] = s.clear[1];
                    }
                    if (mask_valid) *mask_valid = true;
                    if (deck) {
                        deck[0] = s.deck[0];
                        deck[1] = s.deck[1];
                    }
                    if (w0_unit) *w0_unit = s.w0_unit;
                }
                return ok;
            }
        return false;
    }

    void count_hit(int device, bool with_mask)
    {
        std::lock_guard<std::mutex> lock(mu);
        DeviceSeals &d = dev[device];
        ++d.hits;
        if (with_mask) ++d.mask_launches;
    }

    void invalidate(int device, const void *p, size_t bytes)
    {
        if (!p || !bytes || records.load(std::memory_order_relaxed) == 0) return;
        std::lock_guard<std::mutex> lock(mu);
        auto it = dev.find(device);
        if (it == dev.end()) return;
        drop_where(it->second, [](const Seal &s, const void *q, size_t n) { return s.overlaps(q, n); }, p, bytes);
    }

    void drop_device(int device)
    {
        if (records.load(std::memory_order_relaxed) == 0) return;
        std::lock_guard<std::mutex> lock(mu);
        auto it = dev.find(device);
        if (it == dev.end()) return;
        drop_where(it->second, [](const Seal &, const void *, size_t) { return true; }, nullptr, 0);
    }

    void stat(int device, long *seals, long *hits, long *mask_launches)
    {
        std::lock_guard<std::mutex> lock(mu);
        auto it = dev.find(device);
        long n = 0;
        if (it != dev.end())
            for (const Seal &s : it->second.seals) n += s.sealed();
        if (seals) *seals = n;
        if (hits) *hits = it != dev.end() ? it->second.hits : 0;
        if (mask_launches) *mask_launches = it != dev.end() ? it->second.mask_launches : 0;
    }

    // one int (0 / 1) per layer of the sealed set that owns the byte at p; the layer count, 0 without such a set or mask
    int layers(int device, const void *p, int cap, int *clear_out)
    {
        if (!p || records.load(std::memory_order_relaxed) == 0) return 0;
        std::lock_guard<std::mutex> lock(mu);
        auto it = dev.find(device);
        if (it == dev.end()) return 0;
        for (const Seal &s : it->second.seals)
            if (s.sealed() && s.mask_valid && s.overlaps(p, 1)) {
                const int nlayer = s.nlevel - 1;
                for (int i = 0; i < nlayer && i < cap; ++i)
                    if (clear_out) clear_out[i] = s.layer_clear(i) ? 1 : 0;
                return nlayer;
            }
        return 0;
    }
};

}  // namespace sealreg
}  // namespace pz
