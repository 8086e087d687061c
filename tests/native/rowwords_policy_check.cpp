// rowwords_policy_check.cpp -- the life of a set's `rowwords` flag and the accounting of its tables (maray_amd/csrc/row_reuse.hpp)
// and the apply kernel's per-rectangle function (maray_amd/csrc/rowwords.hpp), as a stand-alone program for AddressSanitizer and
// UBSan (tests/test_rowwords_policy.py builds and runs it; nothing is preloaded).
//   rowwords_policy_check            the policy; prints "rowwords policy ok"
//   rowwords_policy_check apply      reads "nw yrows threshold flag n_rects", then per rectangle nw words and yrows bytes (all as
//                                    decimal numbers) from stdin; prints per rectangle its nw words and whether it was flagged
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "row_reuse.hpp"
#include "rowwords.hpp"

using namespace maray;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static RowKey key_of(uint32_t w, double v)
{
    RowKey k;
    k.geometry(w, 72, 0, 72, 0, 32);
    k.params(&v, 1, 1);
    return k;
}

static int policy()
{
    auto fits = [](int) { return true; };
    auto release = [](int) {};
    // a key's first launch fills the scratch; nothing is due before a second launch finds it
    RowReuse R;
    const RowKey a = key_of(320, 1.0);
    CHECK(R.find(a) < 0);
    int s = R.place(a, 1000, fits, release);
    CHECK(s == 0);
    R.filled(s);
    CHECK(!R.census_due(s, true) && !R.rowwords_due(s, true, true));
    R.touch(R.find(a));
    CHECK(R.census_due(s, true) && !R.cover_due(s, true) && !R.rowwords_due(s, true, true) && !R.rowwords_due(s, true, false));
    R.sets[s].census = true;
    // behind the cover for a program with cover bits, behind the census for one without
    CHECK(R.cover_due(s, true) && !R.rowwords_due(s, true, true) && R.rowwords_due(s, true, false));
    R.sets[s].cover = true;
    CHECK(R.rowwords_due(s, true, true) && !R.rowwords_due(s, false, true));
    R.sets[s].rowwords = true;
    CHECK(!R.rowwords_due(s, true, true) && !R.rowwords_due(s, true, false));
    // the scratch's tables are held to the budget but not accounted
    CHECK(R.rowwords_admit(0, 5000) && R.kept_bytes == 0 && R.sets[0].rw_bytes == 5000);
    CHECK(!R.rowwords_admit(0, RowReuse::MAX_BYTES + 1) && R.sets[0].rw_bytes == 5000);
    // a re-key by a ROW-read parameter: the key came before?  no: another key; the flag goes wherever the census's does
    const RowKey b = key_of(320, 2.0);
    CHECK(R.find(b) < 0);
    s = R.place(b, 1000, fits, release);
    CHECK(s == 0 && !R.sets[0].census && !R.sets[0].cover && !R.sets[0].rowwords && R.sets[0].rw_bytes == 5000);      // (the tables stay with the set)
    R.filled(s);
    // the first key comes back: seen before, so it is kept now -- in a fresh set, flags down
    s = R.place(a, 1000, fits, release);
    CHECK(s == 1 && R.kept_bytes == 1000 && !R.sets[1].rowwords && R.sets[1].rw_bytes == 0);
    R.filled(s);
    R.touch(s);
    R.sets[s].census = R.sets[s].cover = true;
    CHECK(R.rowwords_due(s, true, true));
    // kept sets: the tables are accounted, growth only, and refused where they do not fit
    R.max_bytes = 10000;
    CHECK(R.rowwords_admit(s, 6000) && R.kept_bytes == 7000 && R.sets[s].bytes == 7000);
    CHECK(R.rowwords_admit(s, 6000) && R.kept_bytes == 7000);                       // a second scan of the same size adds nothing
    CHECK(R.rowwords_admit(s, 8000) && R.kept_bytes == 9000 && R.sets[s].rw_bytes == 8000);
    CHECK(!R.rowwords_admit(s, 9500) && R.kept_bytes == 9000 && R.sets[s].rw_bytes == 8000);       // nothing is evicted for row words
    // eviction gives the bytes back, the row words' with the set's
    R.drop(s);
    CHECK(R.kept_bytes == 0 && R.kept_sets == 0 && R.sets[s].rw_bytes == 0 && !R.sets[s].rowwords);
    // reuse off: nothing is ever due
    RowReuse Off;
    Off.enabled = false;
    s = Off.place(a, 1000, fits, release);
    Off.filled(s);
    Off.touch(s);
    Off.sets[s].census = Off.sets[s].cover = true;
    CHECK(!Off.rowwords_due(s, true, true) && !Off.rowwords_due(s, true, false));
    // the flag's bit: one more free bit behind the cover's, never a word more
    int32_t bits[3];
    CHECK(cover_free_bits(129, 3, 2, bits) == 2 && bits[0] == 129 && bits[1] == 130);
    CHECK(cover_free_bits(191, 3, 2, bits) == 1 && bits[0] == 191);                 // a cover bit and no flag: no row words
    CHECK(cover_free_bits(192, 3, 1, bits) == 0);
    // the per-rectangle function: counts, thresholds, a threshold of 0 reads as 1
    unsigned char ch[32] = {0};
    unsigned long long in[3] = {1, 2, 4}, out[3] = {0, 0, 0};
    CHECK(rowwords_changed_rows(ch, 32) == 0 && !rowwords_rect(in, ch, out, 3, 32, 0, 8ull) && out[0] == 1 && out[1] == 2 && out[2] == 4);
    ch[31] = 1; ch[0] = 255;
    CHECK(rowwords_changed_rows(ch, 32) == 2 && rowwords_changed_rows(ch, 31) == 1);
    CHECK(!rowwords_rect(in, ch, out, 3, 32, 3, 8ull) && out[2] == 4);
    CHECK(rowwords_rect(in, ch, out, 3, 32, 2, 8ull) && out[0] == 1 && out[1] == 2 && out[2] == 12);
    CHECK(rowwords_rect(in, ch, out, 1, 32, 1, 8ull) && out[0] == 9);
    printf("rowwords policy ok\n");
    return 0;
}

static int apply()
{
    unsigned nw = 0, yrows = 0, threshold = 0, n = 0;
    unsigned long long flag = 0;
    if (scanf("%u %u %u %llu %u", &nw, &yrows, &threshold, &flag, &n) != 5 || !nw || !yrows) return 2;
    std::vector<unsigned long long> in(nw), out(nw);
    std::vector<unsigned char> ch(yrows);
    for (unsigned i = 0; i < n; i++) {
        for (unsigned j = 0; j < nw; j++) if (scanf("%llu", &in[j]) != 1) return 2;
        for (unsigned j = 0; j < yrows; j++) { unsigned v; if (scanf("%u", &v) != 1) return 2; ch[j] = (unsigned char)v; }
        const bool took = rowwords_rect(in.data(), ch.data(), out.data(), nw, yrows, threshold, flag);
        for (unsigned j = 0; j < nw; j++) printf("%llu ", out[j]);
        printf("%d\n", took ? 1 : 0);
    }
    return 0;
}

int main(int argc, char **argv)
{
    return argc > 1 && !strcmp(argv[1], "apply") ? apply() : policy();
}
