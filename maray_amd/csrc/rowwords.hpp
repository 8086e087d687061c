// rowwords.hpp — which rectangles take their guard words per row (product code).  maray_jit_rowscan (jit_source.cpp) leaves,
// per rectangle and row of its band, one byte `changed` = (the row's words differ from the band's); maray_jit_rowscan_apply
// (rowwords.hip) writes a set's fourth table of words, xbits: the third table's words, with the ROW FLAG set in the last word of
// every rectangle where at least `threshold` rows changed.  A rectangle crossed only by a slanted edge changes on no row and stays
// unflagged: its wavefronts pay nothing.  The per-rectangle function is plain C++, so that it can be exercised on a CPU.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define MR_RW_HD __host__ __device__
#else
#define MR_RW_HD
#endif

namespace maray {

// rows of a band on which a rectangle's words changed: changed[0 .. yrows)
MR_RW_HD inline unsigned rowwords_changed_rows(const unsigned char *changed, unsigned yrows)
{
    unsigned n = 0;
    for (unsigned i = 0; i < yrows; i++) n += changed[i] ? 1u : 0u;
    return n;
}

// One rectangle: out[0 .. nw) = in[0 .. nw), the flag (a bit of the last word) set where rows pay.  Returns whether it was set.
// threshold >= 1: a rectangle that changes on no row is never flagged.
MR_RW_HD inline bool rowwords_rect(const unsigned long long *in, const unsigned char *changed, unsigned long long *out, unsigned nw, unsigned yrows,
                                   unsigned threshold, unsigned long long flag)
{
    const bool take = rowwords_changed_rows(changed, yrows) >= (threshold ? threshold : 1u);
    for (unsigned j = 0; j < nw; j++) out[j] = in[j];
    if (take) out[nw - 1] |= flag;
    return take;
}

// maray_jit_rowscan_apply over n_rects rectangles on `stream` (a hipStream_t); *n_set (device) is incremented per flag set.
// Returns a HIP error code (0 = success).
int rowwords_apply_launch(const unsigned long long *in, const unsigned char *changed, unsigned long long *out, unsigned n_rects, unsigned nw, unsigned yrows,
                          unsigned threshold, unsigned long long flag, unsigned *n_set, void *stream);

}   // namespace maray
