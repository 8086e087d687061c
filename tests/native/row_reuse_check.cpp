// row_reuse_check.cpp — the policy of row_reuse.hpp (keys, seen-ring, promotion, LRU, byte budget) on a CPU, with
// "device memory" that is a table of capacities.  Built with -fsanitize=address,undefined by tests/test_row_reuse.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "row_reuse.hpp"

using namespace maray;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static RowKey key_of(uint32_t w, uint32_t rows, uint32_t y0, const std::vector<double> &vals = {}, uint64_t mask = ~0ull,
                     uint32_t blk_rows = 0, uint32_t blk_stride = 0, uint32_t yrows = 32)
{
    RowKey k;
    k.geometry(w, rows, y0, blk_rows ? blk_rows : rows, blk_stride, yrows);
    k.params(vals.data(), (uint32_t)vals.size(), mask);
    return k;
}

// What jit_backend.cpp does around the policy (row_set() and the order step of launch()), without a device: the three tables
// of a set -- y values, guard words, launch order -- have capacities of their own, as they have there.  A launch's `need` is
// split among them (the order's share is a quarter).  Returns true when the launch ran a "ROW pass".  frees counts what waits
// for the device: a release by the policy and a table grown over an old one (the scratch's, as ever).  lazy_order: the order table of a kept set is
// left to the launch that computes an order (a set whose keys rotate away before that then never fits a take-over).
struct Model {
    RowReuse R;
    struct Caps { size_t yv = 0, gb = 0, od = 0; } cap[RowReuse::N_SETS];
    int releases = 0, grown = 0, passes = 0, orders = 0, last = -1;       // releases: by the policy; grown: a table over an old one
    int frees() const { return releases + grown; }
    bool lazy_order = false;
    void ensure(size_t &c, size_t n) { if (n <= c) return; if (c) grown++; c = n; }
    void order_step(int s, size_t od) {                 // launch(): the first launch that finds the set filled computes the order
        if (R.sets[s].order || R.sets[s].launches < 2) return;
        ensure(cap[s].od, od);
        R.sets[s].order = true;
        orders++;
    }
    bool launch(const RowKey &k, size_t need) {
        const size_t od = need / 4, yv = need / 2, gb = need - yv - od;
        int s = R.find(k);
        if (s >= 0) { R.touch(s); last = s; order_step(s, od); return false; }
        s = R.place(k, need, [&](int v) { return cap[v].yv >= yv && cap[v].gb >= gb && cap[v].od >= od; },
                    [&](int v) { CHECK(v >= 1 && cap[v].yv); cap[v] = Caps{}; releases++; });
        CHECK(!R.sets[s].keyed && !R.sets[s].order);
        ensure(cap[s].yv, yv);
        ensure(cap[s].gb, gb);
        if (s && !lazy_order) ensure(cap[s].od, od);
        R.filled(s);
        passes++;
        last = s;
        order_step(s, od);
        return true;
    }
    size_t kept_caps() const { size_t n = 0; for (int s = 1; s < RowReuse::N_SETS; s++) n += cap[s].yv + cap[s].gb + cap[s].od; return n; }
};

int main()
{
    {   // a key seen once is not promoted; the most recent launch's tables always carry their key
        Model m;
        const RowKey a = key_of(4096, 4096, 0);
        CHECK(m.launch(a, 1000) && m.last == 0 && m.R.kept_sets == 0 && m.R.sets[0].launches == 1);
        CHECK(!m.launch(a, 1000) && m.last == 0 && m.R.sets[0].launches == 2 && m.R.kept_sets == 0);
        for (int i = 0; i < 5; i++) CHECK(!m.launch(a, 1000));
        CHECK(m.passes == 1 && m.releases == 0);
    }
    {   // the tiles of a one-shot render share the scratch; the second frame fills kept sets; the third runs no pass
        Model m;
        std::vector<RowKey> tiles;
        for (uint32_t t = 0; t < 6; t++) tiles.push_back(key_of(1024, 128, 128 * t));
        for (const RowKey &k : tiles) CHECK(m.launch(k, 500) && m.last == 0);
        CHECK(m.R.kept_sets == 0 && m.kept_caps() == 0 && m.passes == 6);
        for (size_t t = 0; t < tiles.size(); t++) {
            const bool ran = m.launch(tiles[t], 500);
            if (t + 1 < tiles.size()) CHECK(ran && m.last >= 1 && m.R.sets[m.last].launches == 1);       // filled: the order waits for the first launch that finds it so
            else CHECK(!ran && m.last == 0);             // the last tile of the first frame is still in the scratch
        }
        CHECK(m.R.kept_sets == 5 && m.R.kept_bytes == 2500);
        const int before = m.passes;
        for (int f = 0; f < 3; f++) for (const RowKey &k : tiles) CHECK(!m.launch(k, 500));
        CHECK(m.passes == before && m.frees() == 0);
    }
    {   // A, B, A, B, A, B: a key seen twice is promoted; nothing runs after the second round
        Model m;
        const RowKey a = key_of(1024, 64, 0), b = key_of(1024, 128, 512);
        CHECK(m.launch(a, 100) && m.last == 0);
        CHECK(m.launch(b, 200) && m.last == 0);
        CHECK(m.launch(a, 100) && m.last >= 1);
        CHECK(!m.launch(b, 200) && m.last == 0);        // still in the scratch: a went to a set of its own
        CHECK(!m.launch(a, 100) && !m.launch(b, 200));
        CHECK(m.passes == 3 && m.R.kept_sets == 1 && m.R.kept_bytes == 100);
        CHECK(m.launch(key_of(8, 8, 0), 8) && m.last == 0);       // the scratch goes to another launch: b comes back into a kept set
        CHECK(m.launch(b, 200) && m.last >= 1 && !m.launch(a, 100) && !m.launch(b, 200));
        CHECK(m.passes == 5 && m.R.kept_sets == 2 && m.R.kept_bytes == 300);
    }
    {   // LRU eviction at the count limit: nine keys in rotation fit eight kept sets and the scratch, ten do not -- every
        // round then evicts what the next launch wants; sets of equal size are taken over, not freed
        std::vector<RowKey> k;
        for (uint32_t i = 0; i < 10; i++) k.push_back(key_of(256, 96, 96 * i));
        Model nine;
        for (int round = 0; round < 4; round++) for (uint32_t i = 0; i < 9; i++) nine.launch(k[i], 64);
        CHECK(nine.passes == 9 + 8 && nine.R.kept_sets == RowReuse::MAX_KEPT && nine.frees() == 0);
        Model m;
        for (int round = 0; round < 4; round++) for (const RowKey &x : k) m.launch(x, 64);
        CHECK(m.R.kept_sets == RowReuse::MAX_KEPT && m.R.kept_bytes == 64u * RowReuse::MAX_KEPT && m.frees() == 0);
        CHECK(m.passes == 10 + 3 * 9);                  // (the last key of a round stays in the scratch, which no kept key takes)
        CHECK(m.orders == 1);                           // only the scratch's key is ever found filled: no order kernel per launch in a rotation that does not fit
        for (int round = 0; round < 20; round++) for (const RowKey &x : k) m.launch(x, 64);
        CHECK(m.frees() == 0 && m.passes == 10 + 23 * 9);         // a steady loop: nothing waits for the device, however long it runs
        Model lazy;                                     // (the model sees the fault it is there for: order tables left for later never fit)
        lazy.lazy_order = true;
        for (int round = 0; round < 4; round++) for (const RowKey &x : k) lazy.launch(x, 64);
        CHECK(lazy.releases >= 9);
        // the least recently used goes: touch all but the set of k[j], then bring a new, larger key -- k[j]'s set is released
        Model n;
        for (int round = 0; round < 2; round++) for (uint32_t i = 0; i < 8; i++) n.launch(k[i], 64);
        n.launch(key_of(8, 8, 0), 8);                   // (something else into the scratch, which held k[7])
        n.launch(k[7], 64);
        CHECK(n.R.kept_sets == 8);
        const int victim = n.R.find(k[3]);
        for (uint32_t i = 0; i < 8; i++) if (i != 3) CHECK(!n.launch(k[i], 64));
        const RowKey big = key_of(512, 96, 0);
        CHECK(n.launch(big, 100) && n.last == 0);       // first sight: the scratch
        n.launch(key_of(8, 8, 8), 8);
        CHECK(n.launch(big, 100) && n.last == victim);  // second: a kept set, the least recently used one's place
        CHECK(n.R.find(big) == victim && n.R.find(k[3]) < 0 && n.releases == 1 && n.R.kept_sets == 8);
        CHECK(n.R.kept_bytes == 7 * 64 + 100 && n.kept_caps() == 7 * 64 + 100);
        for (uint32_t i = 0; i < 8; i++) if (i != 3) CHECK(n.R.find(k[i]) >= 1);
    }
    {   // LRU eviction at the byte limit, and an oversized set is never kept
        Model m;
        m.R.max_bytes = 1000;
        const RowKey a = key_of(100, 10, 0), b = key_of(100, 10, 10), c = key_of(100, 10, 20), huge = key_of(100, 1000, 0);
        uint32_t filler = 0;                        // one-off keys that push the scratch's key out
        auto promote = [&](const RowKey &k, size_t need) {
            m.launch(key_of(1, 1, filler++), 1);
            m.launch(k, need);
            if (m.R.find(k) < 1) { m.launch(key_of(1, 1, filler++), 1); m.launch(k, need); }
        };
        promote(a, 400); promote(b, 400);
        CHECK(m.R.find(a) >= 1 && m.R.find(b) >= 1 && m.R.kept_bytes == 800 && m.releases == 0);
        CHECK(!m.launch(a, 400));                   // b is now the least recently used
        promote(c, 500);                            // does not fit b's tables: they are freed, not taken over
        CHECK(m.R.find(c) >= 1 && m.R.find(a) >= 1 && m.R.find(b) < 0 && m.R.kept_bytes == 900 && m.releases == 1);
        for (int i = 0; i < 4; i++) { m.launch(key_of(1, 1, filler++), 1); CHECK(m.launch(huge, 1001) && m.last == 0); }
        CHECK(m.R.find(c) >= 1 && m.R.find(a) >= 1 && m.R.kept_bytes == 900 && m.releases == 1 && m.kept_caps() == 900);
        // a set as large as the whole budget is kept, alone
        const RowKey full = key_of(100, 999, 0);
        promote(full, 1000);
        CHECK(m.R.find(full) >= 1 && m.R.kept_sets == 1 && m.R.kept_bytes == 1000 && m.kept_caps() == 1000);
    }
    {   // a key that differs in one parameter's bits or one geometry field is a miss
        const std::vector<double> v{1.5, -2.0, 3.25};
        const RowKey base = key_of(1024, 64, 32, v, 0b101);
        RowReuse R;
        const int s = R.place(base, 10, [](int) { return false; }, [](int) {});
        CHECK(R.find(base) < 0);                    // placed, not yet filled: no key over tables that nothing filled
        R.filled(s);
        CHECK(R.find(base) == s);
        CHECK(R.find(key_of(1025, 64, 32, v, 0b101)) < 0);
        CHECK(R.find(key_of(1024, 65, 32, v, 0b101)) < 0);
        CHECK(R.find(key_of(1024, 64, 33, v, 0b101)) < 0);
        CHECK(R.find(key_of(1024, 64, 32, v, 0b101, 32)) < 0);
        CHECK(R.find(key_of(1024, 64, 32, v, 0b101, 0, 64)) < 0);
        CHECK(R.find(key_of(1024, 64, 32, v, 0b101, 0, 0, 1)) < 0);
        CHECK(R.find(key_of(1024, 64, 32, {1.5, 7.0, 3.25}, 0b101)) == s);          // parameter 1 is not in the mask
        CHECK(R.find(key_of(1024, 64, 32, {std::nextafter(1.5, 2.0), -2.0, 3.25}, 0b101)) < 0);
        CHECK(R.find(key_of(1024, 64, 32, {1.5, -2.0, std::nextafter(3.25, 0.0)}, 0b101)) < 0);
        CHECK(R.find(key_of(1024, 64, 32, v, 0b111)) < 0);
        CHECK(R.find(key_of(1024, 64, 32, v, 0b001)) < 0);
    }
    {   // -0.0 against +0.0 and two NaN payloads are distinct keys; the same NaN is the same key
        double nan1, nan2;
        const uint64_t b1 = 0x7FF8000000000000ull, b2 = 0x7FF8000000000001ull;
        memcpy(&nan1, &b1, 8); memcpy(&nan2, &b2, 8);
        const RowKey pz = key_of(64, 64, 0, {0.0}), nz = key_of(64, 64, 0, {-0.0}), n1 = key_of(64, 64, 0, {nan1}), n2 = key_of(64, 64, 0, {nan2});
        CHECK(!pz.same(nz) && !n1.same(n2) && n1.same(key_of(64, 64, 0, {nan1})) && pz.same(key_of(64, 64, 0, {0.0})));
        CHECK(pz.hash() != nz.hash() && n1.hash() != n2.hash());
        Model m;
        CHECK(m.launch(pz, 8) && m.launch(nz, 8) && m.launch(n1, 8) && m.launch(n2, 8) && !m.launch(n2, 8));
    }
    {   // reuse off: one scratch set, never a kept one
        Model m;
        m.R.enabled = false;
        const RowKey a = key_of(64, 64, 0), b = key_of(64, 64, 64);
        for (int i = 0; i < 3; i++) { m.launch(a, 8); CHECK(m.last == 0); m.launch(b, 8); CHECK(m.last == 0); }
        CHECK(m.R.kept_sets == 0 && m.passes == 6 && m.R.sets[0].launches == 1);
    }
    printf("row reuse ok\n");
    return 0;
}
