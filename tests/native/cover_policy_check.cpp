// cover_policy_check.cpp — the parts of the cover of guarded ORs that are policy (maray_amd/csrc/row_reuse.hpp), as a
// stand-alone program: which bits of the last guard word cover_free_bits hands out, and the life of a set's `cover` flag --
// due once the census is through, withdrawn with the census's flag by place(), by another key and by an eviction.
// tests/test_cover_policy.py builds it with AddressSanitizer and UBSan and runs it.
#include <cstdio>
#include <cstdlib>

#include "row_reuse.hpp"

using namespace maray;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static RowKey key(uint32_t w, double t)
{
    RowKey k;
    k.geometry(w, 72, 0, 72, 0, 32);
    k.params(&t, 1, 1);
    return k;
}

int main()
{
    // the free bits of the last word, never a word more
    int32_t b[8];
    for (int32_t &v : b) v = -7;
    CHECK(cover_free_bits(63, 1, 2, b) == 1 && b[0] == 63 && b[1] == -7);
    CHECK(cover_free_bits(64, 1, 2, b) == 0);
    CHECK(cover_free_bits(65, 2, 3, b) == 3 && b[0] == 65 && b[1] == 66 && b[2] == 67);
    CHECK(cover_free_bits(128, 2, 1, b) == 0);
    CHECK(cover_free_bits(129, 3, 1, b) == 1 && b[0] == 129);
    CHECK(cover_free_bits(10, 1, 0, b) == 0);
    CHECK(cover_free_bits(0, 0, 1, b) == 0);
    CHECK(cover_free_bits(1, 2, 2, b) == 2 && b[0] == 64 && b[1] == 65);        // only the LAST word's bits
    CHECK(cover_free_bits(200, 2, 1, b) == 0);

    RowReuse R;
    auto fits = [](int) { return true; };
    auto release = [](int) {};
    const RowKey a = key(320, 1.0), c = key(320, 2.0);
    // first launch: the scratch set, filled; second launch: found there, census due, then the cover
    int s = R.place(a, 1000, fits, release);
    CHECK(s == 0);
    R.filled(s);
    CHECK(!R.census_due(s, true) && !R.cover_due(s, true));           // one launch: neither
    CHECK(R.find(a) == s);
    R.touch(s);
    CHECK(R.census_due(s, true) && !R.cover_due(s, true));            // the cover reads the census'd words
    R.sets[s].census = true;
    CHECK(R.cover_due(s, true) && !R.cover_due(s, false));
    R.sets[s].cover = true;
    CHECK(!R.cover_due(s, true) && !R.census_due(s, true));
    // another value of a ROW-read parameter is another key: place() over the scratch withdraws both flags
    CHECK(R.find(c) < 0);
    int s2 = R.place(c, 1000, fits, release);
    CHECK(s2 == 0 && !R.sets[s2].cover && !R.sets[s2].census && !R.sets[s2].keyed);
    R.filled(s2);
    CHECK(R.find(a) < 0);
    // the first key comes back: a kept set of its own, which starts without either flag and gets them again
    s = R.place(a, 1000, fits, release);
    CHECK(s > 0 && !R.sets[s].cover && !R.sets[s].census);
    R.filled(s); R.touch(s);
    CHECK(R.census_due(s, true));
    R.sets[s].census = true;
    CHECK(R.cover_due(s, true));
    R.sets[s].cover = true;
    // ... and is taken over as it is by the next key that comes back once no more sets may be kept: withdrawn again
    R.max_kept = 1;
    const int s3 = R.place(c, 1000, fits, release);
    CHECK(s3 == s && !R.sets[s3].cover && !R.sets[s3].census && !R.sets[s3].keyed);
    // an eviction
    RowReuse E;
    E.max_kept = 1;
    int evicted = -1;
    auto never = [](int) { return false; };
    auto note = [&](int v) { evicted = v; };
    (void)E.place(a, 1000, never, note); E.filled(0);
    (void)E.place(c, 1000, never, note); E.filled(0);
    const int e1 = E.place(a, 1000, never, note);                      // a came back: kept
    CHECK(e1 > 0);
    E.filled(e1); E.touch(e1);
    E.sets[e1].census = E.sets[e1].cover = true;
    const int e2 = E.place(c, 1000, never, note);                      // c came back: a's set does not fit, evicted
    CHECK(evicted == e1 && e2 > 0 && !E.sets[e2].cover && !E.sets[e2].census);
    CHECK(E.find(a) < 0);
    // reuse off: never due
    RowReuse O;
    O.enabled = false;
    O.sets[0].keyed = true; O.sets[0].census = true; O.sets[0].launches = 5;
    CHECK(!O.cover_due(0, true));
    printf("cover policy ok\n");
    return 0;
}
