// row_reuse.hpp — which ROW-stage tables a launch of the specialised backend uses, and whether they already hold what it
// needs (product code; the policy only: includes no HIP, so that it can be compiled and exercised on a CPU).
//
// A context's ROW outputs (y values per row, guard words per rectangle, and the launch order derived from them) depend on
// the program, the geometry of the launch and the values of the parameters that the ROW section reads -- nothing else.
// A set of tables therefore carries a key made of exactly that, and a launch whose key a set already holds runs no ROW
// kernel.  Set 0 is the context's scratch: whatever the most recent one-off launch filled.  Sets 1 .. are kept: a key
// gets one only when it comes a second time (the seen-ring remembers recent keys as 64-bit hashes; a collision costs
// memory, never a wrong pixel, because a hit compares whole keys), so the tiles of a one-shot render keep sharing the
// scratch and allocate nothing.  Kept sets are bounded by count and by bytes and evicted least recently used; a set that
// could not fit the byte budget is simply not kept.  jit_backend.cpp owns the device memory behind the set numbers.
// Two things are derived from a set's guard words once it is found filled, and kept with it: the launch order, and before it the
// census that clears the bits of shapes that are zero on every pixel of a rectangle (census_due).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "maray_tape.h"

namespace maray {

// Geometry words + the bit patterns of the ROW-read parameters' values (NaN payloads and the sign of zero count: the
// ROW kernel sees bits).  Compared like set_params compares values: memcmp.
struct RowKey {
    uint64_t words[3 + MARAY_MAX_PARAMS];
    uint32_t n = 0;

    void geometry(uint32_t w, uint32_t rows_total, uint32_t y0, uint32_t blk_rows, uint32_t blk_stride, uint32_t yrows) {
        words[0] = ((uint64_t)w << 32) | rows_total;
        words[1] = ((uint64_t)y0 << 32) | blk_rows;
        words[2] = ((uint64_t)blk_stride << 32) | yrows;
        n = 3;
    }
    // the values of the parameters in `mask` (bit p = parameter p), in order of p
    void params(const double *values, uint32_t n_params, uint64_t mask) {
        for (uint32_t p = 0; p < n_params && p < MARAY_MAX_PARAMS; p++)
            if ((mask >> p) & 1) memcpy(&words[n++], &values[p], sizeof(uint64_t));
    }
    bool same(const RowKey &o) const { return n == o.n && memcmp(words, o.words, (size_t)n * sizeof(uint64_t)) == 0; }
    uint64_t hash() const {                     // FNV-1a over the words; never 0 (0 = an empty place in the seen-ring)
        uint64_t h = 1469598103934665603ull;
        for (uint32_t i = 0; i < n; i++)
            for (int b = 0; b < 8; b++) { h ^= (words[i] >> (8 * b)) & 0xFF; h *= 1099511628211ull; }
        return h ? h : 1;
    }
};

// The cover bits of a program: `want` bits from those of the last of `n_words` guard words that no guard uses (bits n_used ..
// 64 n_words - 1).  Never a word more: returns how many were granted, lowest free bit first, into bits[0 .. granted).
inline uint32_t cover_free_bits(uint32_t n_used, uint32_t n_words, uint32_t want, int32_t *bits)
{
    if (!n_words || n_used > 64u * n_words) return 0;
    const uint32_t first = n_used > 64u * (n_words - 1) ? n_used : 64u * (n_words - 1);
    const uint32_t n_free = 64u * n_words - first, granted = want < n_free ? want : n_free;
    for (uint32_t k = 0; k < granted; k++) bits[k] = (int32_t)(first + k);
    return granted;
}

struct RowReuse {
    static constexpr int MAX_KEPT = 8;                      // design limits, not measurements
    static constexpr size_t MAX_BYTES = (size_t)256 << 20;
    static constexpr int N_SETS = 1 + MAX_KEPT;             // set 0 = scratch
    static constexpr int SEEN = 32;

    struct Set {
        RowKey key;
        bool keyed = false;         // the tables hold the ROW outputs of `key` (set only once the ROW kernel is enqueued)
        bool order = false;         // ... and the launch order computed from its guard bits
        bool cover = false;         // ... and the third table, in which a cover bit stands for the leaves of an OR that is 1 on every pixel of a rectangle (maray_jit_cover); set with or after `census`, withdrawn wherever it is
        bool census = false;        // ... and the second table of guard words the census made of them (maray_jit_census): without the bits of leaves that are zero on every pixel of a rectangle
        bool rowwords = false;      // ... and the fourth table and the row words (maray_jit_rowscan, rowwords.hpp): set behind the cover (or the census, for a program without cover bits), withdrawn wherever `census` is
        size_t rw_bytes = 0;        // device bytes of the row-word tables admitted for the set (rowwords_admit); they stay with its tables
        uint32_t launches = 0;      // launches that used the set under this key: the second one (the first that found it filled) computes the order
        uint64_t stamp = 0;         // last use (kept sets: least recently used goes first)
        size_t bytes = 0;           // kept sets: device bytes accounted to the set (0 = not in use)
    };

    bool enabled = true;            // MARAY_JIT_ROW_REUSE=0: one scratch set, a ROW pass per launch that asks for one
    int max_kept = MAX_KEPT;
    size_t max_bytes = MAX_BYTES;
    Set sets[N_SETS];
    uint64_t seen[SEEN] = {};
    int seen_next = 0;
    uint64_t clock = 0;
    size_t kept_bytes = 0;
    int kept_sets = 0;

    // The set that holds valid outputs for `key`, or -1.
    int find(const RowKey &key) const {
        for (int s = 0; s < N_SETS; s++)
            if (sets[s].keyed && sets[s].key.same(key)) return s;
        return -1;
    }

    // A launch uses set s, found by find().
    void touch(int s) { sets[s].stamp = ++clock; sets[s].launches++; }

    // Is the census of set s due on this launch?  Like the launch order it costs about a launch and is paid by the first launch
    // that finds the set holding its key (launches >= 2: a one-shot render never pays), once per filling -- place() and a
    // refill withdraw the flag with the order's -- and only while sets are reused at all: with reuse off every launch that asks
    // for a ROW pass writes the words again.  matched: the set holds this launch's key.  The caller sets Set::census once the
    // kernels are enqueued, and enqueues them in front of the order kernel, which counts the bits that are left.
    bool census_due(int s, bool matched) const { return enabled && matched && sets[s].keyed && !sets[s].census && sets[s].launches >= 2; }

    // The cover (maray_jit_cover) reads the census'd words: due on the launch that takes the census or any later one that finds
    // the set through its census and not yet covered.  The caller sets Set::cover once the kernels are enqueued.
    bool cover_due(int s, bool matched) const { return enabled && matched && sets[s].keyed && sets[s].census && !sets[s].cover; }

    // The row scan (maray_jit_rowscan) reads the cover's words: due on the launch that takes the cover or any later one that
    // finds the set covered and not yet scanned; for a program without cover bits (has_cover == false) behind the census
    // instead.  The caller sets Set::rowwords once the kernels are enqueued.
    bool rowwords_due(int s, bool matched, bool has_cover) const {
        return enabled && matched && sets[s].keyed && sets[s].census && (sets[s].cover || !has_cover) && !sets[s].rowwords;
    }

    // The row-word tables of set s, `bytes` of device memory, count against the budget of the kept sets: false when they do
    // not fit -- the set then takes no row words; nothing is evicted for them.  Bytes admitted once stay admitted (the tables
    // stay allocated with the set and go with it: drop(), or a take-over in place(), which keeps tables and accounting);
    // only growth is added.  The scratch's tables are held to the same bound but, like its other tables, not accounted.
    bool rowwords_admit(int s, size_t bytes) {
        const size_t more = bytes > sets[s].rw_bytes ? bytes - sets[s].rw_bytes : 0;
        const bool kept = s > 0 && sets[s].bytes;
        const size_t add = kept ? more : bytes;             // (the scratch's tables are not in kept_bytes: all of them count here)
        if (add > max_bytes || kept_bytes + add > max_bytes) return false;
        if (kept) { sets[s].bytes += more; kept_bytes += more; }
        sets[s].rw_bytes += more;
        return true;
    }

    bool was_seen(uint64_t h) const {
        for (uint64_t v : seen) if (v == h) return true;
        return false;
    }
    void remember(uint64_t h) {
        if (was_seen(h)) return;
        seen[seen_next] = h;
        seen_next = (seen_next + 1) % SEEN;
    }

    int lru() const {
        int v = -1;
        for (int s = 1; s <= max_kept; s++)
            if (sets[s].bytes && (v < 0 || sets[s].stamp < sets[v].stamp)) v = s;
        return v;
    }
    void drop(int s) {              // the caller frees the device memory of s
        kept_bytes -= sets[s].bytes;
        kept_sets--;
        sets[s] = Set{};
    }

    // No set holds `key`: the set its ROW pass will fill.  `need` = device bytes of its tables; fits(s) = the tables kept
    // set s has now are large enough for them (then s can be taken over without touching device memory); release(s) =
    // free the device memory of kept set s.  The chosen set's key is withdrawn until filled() -- an exception in between
    // leaves no key over tables that nothing filled.  Returns 0 (scratch) unless the key has come before.
    template <typename Fits, typename Release>
    int place(const RowKey &key, size_t need, Fits fits, Release release) {
        const uint64_t h = key.hash();
        const bool again = was_seen(h);
        remember(h);
        int s = 0;
        if (enabled && again && max_kept > 0 && need <= max_bytes) {
            int v = (kept_sets >= max_kept || kept_bytes + need > max_bytes) ? lru() : -1;
            if (v >= 0 && fits(v)) {
                // taken over as it is, new key: the set stays accounted with the bytes of its tables, which are what
                // the device holds -- at least `need`, so the budget errs on the safe side
                s = v;
            } else {
                if (kept_sets >= max_kept) { release(v); drop(v); }
                while (kept_bytes + need > max_bytes) { v = lru(); release(v); drop(v); }
                for (s = 1; sets[s].bytes; s++) {}
                sets[s].bytes = need;
                kept_bytes += need;
                kept_sets++;
            }
        }
        sets[s].keyed = false;
        sets[s].order = false;
        sets[s].census = false;
        sets[s].cover = false;
        sets[s].rowwords = false;
        sets[s].launches = 0;                          // (touch() by filled() counts this launch)
        sets[s].key = key;
        return s;
    }

    // The ROW kernel that fills set s for the key given to place() has been enqueued.
    void filled(int s) { sets[s].keyed = true; touch(s); }
};

}   // namespace maray
