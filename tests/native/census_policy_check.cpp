// census_policy_check.cpp — when the census of a set's guard bits is due (row_reuse.hpp: Set::census, census_due) on a CPU, the
// way jit_backend.cpp's launch() asks: census first, then the order.  Built with -fsanitize=address,undefined by
// tests/test_census_policy.py.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "row_reuse.hpp"

using namespace maray;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static RowKey key_of(uint32_t w, uint32_t rows, const std::vector<double> &vals = {}, uint64_t mask = ~0ull)
{
    RowKey k;
    k.geometry(w, rows, 0, rows, 0, 32);
    k.params(vals.data(), (uint32_t)vals.size(), mask);
    return k;
}

// A launch as launch() issues it: the set, then the census where one is due, then the order.  `log` gets a letter per kernel:
// R (ROW pass), C (census), O (order), P (pixels).
struct Model {
    RowReuse R;
    std::string log;
    int censuses = 0;
    void launch(const RowKey &k, size_t need = 1000, bool rows_pass = true) {
        int s = R.find(k);
        bool matched = true;
        if (s >= 0 && (R.enabled || !rows_pass)) R.touch(s);
        else if (!rows_pass) { matched = false; s = 0; }
        else {
            const bool refill = s >= 0;
            if (!refill) s = R.place(k, need, [](int) { return true; }, [](int) {});
            CHECK(refill || (!R.sets[s].keyed && !R.sets[s].order && !R.sets[s].census));
            log += 'R';
            if (refill) R.touch(s); else R.filled(s);
        }
        if (R.census_due(s, matched)) { log += 'C'; censuses++; R.sets[s].census = true; }
        if (matched && !R.sets[s].order && R.sets[s].launches >= 2) { log += 'O'; R.sets[s].order = true; }
        log += 'P';
    }
};

int main()
{
    {   // a benchmark loop: the second launch takes the census, in front of the order; nothing after that
        Model m;
        const RowKey a = key_of(4096, 4096);
        for (int i = 0; i < 5; i++) m.launch(a);
        CHECK(m.log == "RPCOPPPP" && m.censuses == 1);
    }
    {   // a one-shot render: the tiles are keys of their own and share the scratch -- never
        Model m;
        for (uint32_t i = 0; i < 40; i++) m.launch(key_of(4096, 64 + i));
        CHECK(m.censuses == 0 && m.log.find('C') == std::string::npos);
    }
    {   // two keys in turn: the first comes back into a kept set and takes its census on the launch after that; the second is
        // still in the scratch when it comes back, and takes it there
        Model m;
        const RowKey a = key_of(1024, 512, {1.0}), b = key_of(1024, 512, {2.0});
        m.launch(a); m.launch(b);               // both through the scratch
        CHECK(m.log == "RPRP");
        m.launch(a);                            // seen before, and the scratch holds b: a kept set, filled anew
        CHECK(m.log == "RPRPRP" && m.censuses == 0 && m.R.sets[1].keyed && !m.R.sets[1].census);
        m.launch(b);                            // found filled, in the scratch
        CHECK(m.log == "RPRPRPCOP" && m.censuses == 1 && m.R.sets[0].census);
        m.launch(a); m.launch(b);
        CHECK(m.log == "RPRPRPCOPCOPP" && m.censuses == 2 && m.R.sets[1].census);
        m.launch(a); m.launch(b);
        CHECK(m.censuses == 2);
        m.launch(key_of(1024, 256));            // a one-off launch takes the scratch: its flags go with its key
        CHECK(!m.R.sets[0].census && !m.R.sets[0].order && m.R.sets[1].census);
    }
    {   // a set taken over for another key loses the flag with its order: place() withdraws both
        Model m;
        m.R.max_kept = 1;
        const RowKey a = key_of(512, 256, {1.0}), b = key_of(512, 256, {2.0}), c = key_of(512, 256, {3.0});
        m.launch(a); m.launch(b); m.launch(a); m.launch(a);         // a: scratch, (b: scratch,) kept set 1, census
        CHECK(m.censuses == 1 && m.R.sets[1].census && m.R.sets[1].order);
        m.launch(c);                                                // the scratch is c's now
        m.launch(b);                                                // b came before and no set holds it: it takes set 1 over
        CHECK(m.R.sets[1].key.same(b) && !m.R.sets[1].census && !m.R.sets[1].order && m.censuses == 1);
        m.launch(b);
        CHECK(m.censuses == 2 && m.R.sets[1].census);
    }
    {   // reuse off: every launch that asks for a ROW pass writes the words again -- no census, whatever the counters say
        Model m;
        m.R.enabled = false;
        const RowKey a = key_of(512, 256);
        for (int i = 0; i < 4; i++) m.launch(a);
        CHECK(m.censuses == 0 && m.log.find('C') == std::string::npos && m.R.sets[0].launches >= 2);
        m.launch(a, 1000, false);               // not even for a launch without a ROW pass of its own (time_rows)
        CHECK(m.censuses == 0);
    }
    {   // a launch that finds no set and runs no ROW pass (time_rows on another geometry) uses the previous set as it is: not matched
        Model m;
        const RowKey a = key_of(512, 256), b = key_of(512, 128);
        m.launch(a);
        m.launch(b, 1000, false);
        CHECK(m.censuses == 0);
        CHECK(!m.R.census_due(0, false));
        m.launch(a);
        CHECK(m.censuses == 1);
    }
    printf("census policy ok\n");
    return 0;
}
