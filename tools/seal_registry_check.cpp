// The seal registry (picaso_amd/csrc/planeseal_registry.hpp) driven without a device: record, look up, replace,
// invalidate and drop seals, their clear-layer and deck-layer masks and their w0 fact over made-up plane addresses.  Meant for a sanitizer build on the
// CPU -- the registry is the host code behind picaso_reflected_planes_seal_dev / _seal_layers / _seal_stat:
//
//     c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//         -I picaso_amd/csrc tools/seal_registry_check.cpp -o /tmp/seal_registry_check -lpthread && /tmp/seal_registry_check
//
// Exit status 0 and "seal_registry_check: ok" when every expectation holds.
#include "planeseal_registry.hpp"

#include <cstdio>
#include <cstdlib>
#include <thread>

using namespace pz::sealreg;

#define EXPECT(cond)                                                                 \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "%s:%d: expectation failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

// eleven planes of (nlevel | nlevel - 1) rows of `pitch` doubles inside one host block: only the addresses are used
struct FakeSet {
    std::vector<double> block;
    const double *pl[11];
    int nlevel, nwno;
    long pitch;
    FakeSet(int nlevel_, int nwno_, long pitch_) : block((size_t)11 * nlevel_ * pitch_), nlevel(nlevel_), nwno(nwno_), pitch(pitch_)
    {
        for (int j = 0; j < 11; ++j) pl[j] = block.data() + (size_t)j * nlevel * pitch;
    }
    Seal seal(int flags, const unsigned *notclear, const unsigned *notdeck = nullptr, bool w0_unit = false) const
    {
        Seal s{};
        for (int j = 0; j < 11; ++j) s.plane[j] = pl[j];
        s.nlevel = nlevel;
        s.nwno = nwno;
        s.pitch = pitch;
        s.flags = flags;
        mask_from_device_words(s, notclear, notdeck, w0_unit);
        return s;
    }
};

int main()
{
    Registry r;
    uint64_t m[2];
    bool valid = true;
    long seals = -1, hits = -1, masks = -1;
    int clear[200], n;

    // nothing recorded
    FakeSet a(91, 600, 600);
    EXPECT(!r.derivable(0, a.pl, 91, 600, 600, m, &valid) && !valid && m[0] == 0 && m[1] == 0);
    EXPECT(r.layers(0, a.pl[0], 200, clear) == 0);
    r.invalidate(0, a.pl[0], 8);
    r.drop_device(0);
    r.stat(0, &seals, &hits, &masks);
    EXPECT(seals == 0 && hits == 0 && masks == 0);

    // 90 layers, cloud in 49..58: words of 32 layers, bits set = NOT clear
    unsigned nc[4] = {0, 0, 0, 0};
    for (int i = 49; i < 59; ++i) nc[i >> 5] |= 1u << (i & 31);
    nc[3] = 0xffffffffu;                       // rubbish above nlayer must not reach the mask
    r.record(0, a.seal(7, nc));
    EXPECT(r.derivable(0, a.pl, 91, 600, 600, m, &valid) && valid);
    for (int i = 0; i < 128; ++i) EXPECT((((m[i >> 6] >> (i & 63)) & 1) != 0) == (i < 90 && (i < 49 || i > 58)));
    EXPECT(!r.derivable(0, a.pl, 91, 599, 600, m, &valid) && !valid && m[0] == 0);      // another shape
    EXPECT(!r.derivable(1, a.pl, 91, 600, 600, nullptr, nullptr));                      // another device
    n = r.layers(0, (const char *)a.pl[9] + 8 * 12345 + 3, 200, clear);                 // any byte of any plane
    EXPECT(n == 90);
    for (int i = 0; i < 90; ++i) EXPECT(clear[i] == (i < 49 || i > 58));
    clear[5] = 7;
    EXPECT(r.layers(0, a.pl[2], 5, clear) == 90 && clear[5] == 7);                      // cap is honoured
    EXPECT(r.layers(0, a.pl[2], 0, nullptr) == 90);
    EXPECT(r.layers(0, a.block.data() + a.block.size(), 200, clear) == 0);             // one past the set

    // the deck mask and the w0 fact: handed out with a valid mask only, the deck mask disjoint from the clear mask and
    // empty above nlayer; words of 32 layers, bits set = NOT a deck layer
    {
        uint64_t c[2] = {1, 1};
        bool unit = true;
        EXPECT(r.derivable(0, a.pl, 91, 600, 600, m, &valid, c, &unit) && valid && c[0] == 0 && c[1] == 0 && !unit);   // recorded without
        unsigned nk[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0};
        for (int i = 50; i < 58; ++i) nk[i >> 5] &= ~(1u << (i & 31));      // 49 and 58: cloudy, but not in every column
        nk[0] &= ~(1u << 3);                                                // says "deck", but layer 3 is clear: not a deck layer
        r.record(0, a.seal(7, nc, nk, true));
        EXPECT(r.derivable(0, a.pl, 91, 600, 600, m, &valid, c, &unit) && valid && unit);
        for (int i = 0; i < 128; ++i) EXPECT((((c[i >> 6] >> (i & 63)) & 1) != 0) == (i >= 50 && i < 58));
        EXPECT((c[0] & m[0]) == 0 && (c[1] & m[1]) == 0);
        EXPECT(r.derivable(0, a.pl, 91, 600, 600, m, &valid, c, nullptr) && r.derivable(0, a.pl, 91, 600, 600, m, &valid, nullptr, &unit));
        EXPECT(!r.derivable(0, a.pl, 91, 599, 600, m, &valid, c, &unit) && c[0] == 0 && c[1] == 0 && !unit);          // another shape
        r.record(0, a.seal(7, nc, nk, false));                              // a w0 outside [0, 1]: the masks stay
        EXPECT(r.derivable(0, a.pl, 91, 600, 600, m, &valid, c, &unit) && valid && !unit && c[0] != 0);
        r.record(0, a.seal(7 & ~1, nc, nk, true));                          // not sealed: nothing is handed out
        EXPECT(!r.derivable(0, a.pl, 91, 600, 600, m, &valid, c, &unit) && c[0] == 0 && c[1] == 0 && !unit);
        r.record(0, a.seal(7, nc));
    }

    // counters
    r.count_hit(0, false);
    r.count_hit(0, true);
    r.stat(0, &seals, &hits, &masks);
    EXPECT(seals == 1 && hits == 2 && masks == 1);

    // re-seal replaces: now not derivable (a flag missing), the mask is not handed out
    r.record(0, a.seal(7 & ~2, nc));
    r.stat(0, &seals, nullptr, nullptr);
    EXPECT(seals == 0 && r.records.load() == 1);
    EXPECT(!r.derivable(0, a.pl, 91, 600, 600, m, &valid) && !valid && m[0] == 0);
    EXPECT(r.layers(0, a.pl[0], 200, clear) == 0);
    r.record(0, a.seal(7, nc));
    EXPECT(r.records.load() == 1 && r.derivable(0, a.pl, 91, 600, 600, m, &valid) && valid);

    // 128 layers: both words; 129 layers: sealed, no mask
    FakeSet b(129, 64, 70), c(130, 64, 64);
    unsigned nb[4] = {1u, 0, 0, 0x80000000u};
    r.record(0, b.seal(7, nb));
    EXPECT(r.derivable(0, b.pl, 129, 64, 70, m, &valid) && valid && m[0] == ~(uint64_t)1 && m[1] == (~(uint64_t)0 >> 1));
    r.record(0, c.seal(7, nullptr));
    EXPECT(r.derivable(0, c.pl, 130, 64, 64, m, &valid) && !valid && m[0] == 0 && m[1] == 0);
    {
        // 128 layers, every one a deck layer but the first; more than 128 layers: no mask, so no deck mask and no w0 fact
        unsigned all[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, nk[4] = {1u, 0, 0, 0};
        uint64_t k[2];
        bool unit;
        r.record(0, b.seal(7, all, nk, true));
        EXPECT(r.derivable(0, b.pl, 129, 64, 70, m, &valid, k, &unit) && valid && unit && m[0] == 0 && m[1] == 0);
        EXPECT(k[0] == ~(uint64_t)1 && k[1] == ~(uint64_t)0);
        r.record(0, b.seal(7, nb));
        r.record(0, c.seal(7, nullptr, nk, true));
        EXPECT(r.derivable(0, c.pl, 130, 64, 64, m, &valid, k, &unit) && !valid && !unit && k[0] == 0 && k[1] == 0);
    }
    EXPECT(r.layers(0, c.pl[0], 200, clear) == 0);
    r.stat(0, &seals, nullptr, nullptr);
    EXPECT(seals == 3);

    // one layer
    FakeSet d(2, 24, 24);
    unsigned nd[4] = {0, 0, 0, 0};
    r.record(1, d.seal(7, nd));
    EXPECT(r.derivable(1, d.pl, 2, 24, 24, m, &valid) && valid && m[0] == 1 && m[1] == 0);

    // invalidation: the pad of the last row of a pitched plane is not the solver's, the byte before it is
    const char *last = (const char *)(b.pl[0] + (size_t)127 * 70);       // dtau: 128 rows
    r.invalidate(0, last + 8 * 64, 8 * 6);
    EXPECT(r.derivable(0, b.pl, 129, 64, 70, m, &valid));
    r.invalidate(0, last + 8 * 63 + 7, 1);
    EXPECT(!r.derivable(0, b.pl, 129, 64, 70, m, &valid) && !valid && m[1] == 0);
    EXPECT(r.layers(0, b.pl[0], 200, clear) == 0);
    EXPECT(r.records.load() == 3);
    r.drop_device(0);
    EXPECT(r.records.load() == 1 && !r.derivable(0, a.pl, 91, 600, 600, m, &valid));
    EXPECT(r.derivable(1, d.pl, 2, 24, 24, m, &valid));
    r.stat(0, &seals, &hits, &masks);
    EXPECT(seals == 0 && hits == 2 && masks == 1);              // the counters outlive the seals

    // two threads sealing, looking up and invalidating their own sets
    auto worker = [&r](int device) {
        FakeSet s(7, 200, 200);
        unsigned w[4] = {8u, 0, 0, 0};
        uint64_t mm[2];
        bool v;
        for (int k = 0; k < 2000; ++k) {
            r.record(device, s.seal(7, w));
            if (!r.derivable(device, s.pl, 7, 200, 200, mm, &v) || !v || mm[0] != 0x37u) std::abort();
            r.count_hit(device, true);
            r.invalidate(device, s.pl[k % 11], 1);
        }
    };
    std::thread t0(worker, 2), t1(worker, 2), t2(worker, 3);
    t0.join();
    t1.join();
    t2.join();
    r.stat(2, &seals, &hits, &masks);
    EXPECT(seals == 0 && hits == 4000 && masks == 4000);
    r.drop_device(1);
    EXPECT(r.records.load() == 0);
    std::puts("seal_registry_check: ok");
    return 0;
}
