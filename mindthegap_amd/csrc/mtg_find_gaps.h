/*
 * mtg_find_gaps.h -- the gaps of the reference's `find` scan (FindBreakpoints::notify, src/FindBreakpoints.hpp:560-622) from the two bit
 * planes of a sequence (valid, present; layout of mtg_profile_runs.h).  The word-level logic of k_profile_count<true> / k_profile_write<true>
 * (mtg_gpu_misc.hip); the same source is compiled by g++ into tests/emu/find_gaps.cpp, which checks it against the literal loop of notify().
 *
 * The scan's gap is not the profile's run.  One present position with no present neighbour does not end a gap, it is counted into it
 * (:609-612); the gap observers are called at the SECOND position of a solid stretch (:579), and kmer_begin is taken only when the gap starts
 * behind a solid stretch of at least two (:613-617).  An invalid position resets both counters and both k-mers (:426-431), and so does the
 * start of a sequence (:393-400), so no kmer_begin of an earlier gap survives to a gap that is reported: behind a reported gap the solid
 * stretch has reached two, and the next absent position takes a fresh kmer_begin.
 *
 * In words: a position is an ANCHOR when it is present and its left or its right neighbour in the sequence is present.  A gap is a maximal
 * stretch of valid positions that are no anchors.  It is reported (the observers are called, at the position behind its first anchor) when
 * the position right behind it is an anchor -- flags bit 1 -- and its kmer_begin is valid, the k-mer right before the gap, when the position
 * right before it is an anchor -- flags bit 0.  A gap next to an invalid position or to an end of the sequence lacks that flag.  One bit of
 * look-around on either side: the anchors of a word need the present plane of the two neighbouring words only, and the counted two-pass
 * extraction of mtg_profile_runs.h (the j-th first and the j-th last position of a sequence belong to the same gap) applies as it stands.
 */
#ifndef MTG_FIND_GAPS_H
#define MTG_FIND_GAPS_H
#include "mtg_profile_runs.h"

namespace mtg {

/* the gaps of word w as a RunWord: first / last positions of gaps, lflag / rflag = an anchor right before / right behind */
MTG_DEV RunWord gap_word(const uint64_t* vplane, const uint64_t* pplane, uint32_t w, uint32_t npos)
{
    const uint32_t nw = run_words(npos);
    uint64_t v[3], p[3]; /* the word before, the word, the word behind */
MTG_UNROLL
    for (int i = 0; i < 3; i++) {
        const bool in = !(i == 0 && w == 0);
        v[i] = in ? run_plane_word(vplane, w + (uint32_t)i - 1u, nw, npos) : 0ull;
        p[i] = in ? run_plane_word(pplane, w + (uint32_t)i - 1u, nw, npos) & v[i] : 0ull;
    }
    /* anchors of the word, of the last position of the word before and of the first position of the word behind */
    const uint64_t anchor = p[1] & ((p[1] << 1) | (p[0] >> 63) | (p[1] >> 1) | ((p[2] & 1ull) << 63));
    const uint64_t anchor_before = (p[0] >> 63) & (((p[0] >> 62) | p[1]) & 1ull);
    const uint64_t anchor_behind = (p[2] & 1ull) & ((p[1] >> 63) | ((p[2] >> 1) & 1ull));
    const uint64_t g = v[1] & ~anchor, g_before = (v[0] >> 63) & ~anchor_before & 1ull, g_behind = (v[2] & 1ull) & ~anchor_behind;
    RunWord r;
    r.first = g & ~((g << 1) | g_before);
    r.last = g & ~((g >> 1) | (g_behind << 63));
    r.lflag = r.first & ((anchor << 1) | anchor_before);
    r.rflag = r.last & ((anchor >> 1) | (anchor_behind << 63));
    r.open = (uint32_t)(g_before & g & 1ull);
    return r;
}

/* What the observers in scope ask of a gap before anything is looked up: it is reported with a valid kmer_begin (both flags) and its length L
 * gives a repeat r = k - 1 - L with 0 <= r <= max_repeat (FindInsertion.hpp:53,107). */
MTG_HD bool gap_is_candidate(uint32_t length, uint32_t flags, int k, int max_repeat)
{
    return flags == 3u && length <= (uint32_t)(k - 1) && (uint32_t)(k - 1) - length <= (uint32_t)max_repeat;
}

} // namespace mtg
#endif
