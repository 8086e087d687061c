// row_reuse_walk.cpp — a walk of launches through the policy of row_reuse.hpp on a CPU, the way row_set() and launch() of
// jit_backend.cpp drive it: find, touch, place, filled, the *_due tests and rowwords_admit, with "device memory" that is a table
// of capacities (as row_reuse_check.cpp).  Built with -fsanitize=address,undefined by tests/test_walks.py, which compares its
// lines with tests/walk_scenes.py's PolicyModel.
//
// stdin: a first line `budget enabled`, then a line per launch:
//   key-id rows_pass need  yvals gbits order hits cbits vbits cflags  want_order yrows has_census has_cover has_rw rw_bytes words row_ops
// (need = bytes asked of place(); the seven numbers are the elements the launch needs of the tables that fits() asks for; words =
// guard words of the launch).  stdout, per launch: set pass census cover scan order kept_sets kept_bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "row_reuse.hpp"

using namespace maray;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

struct Caps { size_t t[7] = {}; };

int main()
{
    RowReuse R;
    Caps cap[RowReuse::N_SETS];
    size_t words_of[RowReuse::N_SETS] = {};
    unsigned long long budget = 0;
    int enabled = 1;
    CHECK(scanf("%llu %d", &budget, &enabled) == 2);
    R.max_bytes = (size_t)budget;
    R.enabled = enabled != 0;
    for (;;) {
        unsigned long long kid, need, n[7], rw_bytes, words;
        int rows_pass, want_order, yrows, has_census, has_cover, has_rw, row_ops;
        const int got = scanf("%llu %d %llu %llu %llu %llu %llu %llu %llu %llu %d %d %d %d %d %llu %llu %d", &kid, &rows_pass, &need, &n[0], &n[1], &n[2], &n[3], &n[4],
                              &n[5], &n[6], &want_order, &yrows, &has_census, &has_cover, &has_rw, &rw_bytes, &words, &row_ops);
        if (got == EOF) break;
        CHECK(got == 18);
        RowKey key;
        key.geometry((uint32_t)kid, (uint32_t)(kid >> 32), 0, 1, 0, (uint32_t)yrows);
        int pass = 0, census = 0, cover = 0, scan = 0, order = 0;
        auto ensure = [](size_t &c, size_t v) { if (v > c) c = v; };
        // row_set()
        int s = R.find(key);
        if (s >= 0 && (R.enabled || !rows_pass)) R.touch(s);
        else {
            CHECK(rows_pass);
            const bool refill = s >= 0;
            if (!refill)
                s = R.place(key, (size_t)need,
                            [&](int v) { for (int k = 0; k < 7; k++) if (cap[v].t[k] < n[k]) return false; return true; },
                            [&](int v) { CHECK(v >= 1 && R.sets[v].bytes); cap[v] = Caps{}; });
            CHECK(s >= 0 && s < RowReuse::N_SETS && (refill || !R.sets[s].keyed));
            for (int k = 0; k < (s ? 7 : 2); k++) ensure(cap[s].t[k], (size_t)n[k]);
            if (row_ops) pass = 1;
            if (refill) R.touch(s); else R.filled(s);
            words_of[s] = (size_t)words;
        }
        // launch()
        if (has_census && R.census_due(s, true) && words_of[s]) {
            ensure(cap[s].t[3], (size_t)n[3]); ensure(cap[s].t[4], (size_t)n[4]);
            census = 1;
            R.sets[s].census = true;
        }
        if (has_census && has_cover && R.cover_due(s, true) && words_of[s]) {
            ensure(cap[s].t[5], (size_t)n[5]); ensure(cap[s].t[6], (size_t)n[6]);
            cover = 1;
            R.sets[s].cover = true;
        }
        if (has_rw && has_census && yrows > 1 && R.rowwords_due(s, true, has_cover != 0)) {
            if (words_of[s] && R.rowwords_admit(s, (size_t)rw_bytes)) scan = 1;
            R.sets[s].rowwords = true;
        }
        if (want_order && !R.sets[s].order && R.sets[s].launches >= 2) {
            ensure(cap[s].t[2], (size_t)n[2]);
            order = 1;
            R.sets[s].order = true;
        }
        CHECK(R.kept_bytes <= R.max_bytes && R.kept_sets <= RowReuse::MAX_KEPT);
        printf("%d %d %d %d %d %d %d %zu\n", s, pass, census, cover, scan, order, R.kept_sets, R.kept_bytes);
    }
    return 0;
}
