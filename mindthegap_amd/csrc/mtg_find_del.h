/*
 * mtg_find_del.h -- the logic of `find` for homozygous deletions (FindDeletion::update, src/FindDeletion.hpp:58-188) on one gap of the scan
 * (mtg_find_gaps.h) and its two k-mers.  Shared by DelObserver (k_gap_mark / k_gap_emit) and k_del_judge (mtg_gpu_misc.hip); the same source is compiled by
 * g++ into tests/emu/find_del.cpp, which checks it against literal string loops.
 *
 * The observer is a pure function of the gap: kmer_begin (the anchor right before the gap, at left = start - 1), kmer_end (the first anchor
 * behind it, at right = start + L), the gap's length L and the graph.  It reads no history and leaves the gap state alone.  With r the
 * junction repeat of the two k-mers (del_fuzzy_site) the joined text is J_r = begin[0 : k - r] + end: 2k - r nucleotides, k - r + 1 k-mers.
 * Every k-mer of J_r in the graph: a deletion of del_size = L - k + r + 1 nucleotides.  Else, with r > 0, J_0 = begin + end is tried: a
 * deletion of L - k + 1 with repeat 0 (the fallback).  del_size <= 0 is no deletion.  The record's pos is that of the nucleotide before the
 * deleted text: position() - 2 - del_size with position() = start + L + 1, which is left + k - 1 - r.
 *
 * k-mers are little-endian images (mtg_post.h: le_kmer): nucleotide i in bits 2i, 2i + 1; k <= 32.
 */
#ifndef MTG_FIND_DEL_H
#define MTG_FIND_DEL_H
#include "mtg_find_gaps.h"

namespace mtg {

/* result word of k_del_judge for one candidate: DEL_CALLED | DEL_FALLBACK | r << 8 (the final r); 0: no deletion */
enum : uint32_t { DEL_CALLED = 1u, DEL_FALLBACK = 2u, DEL_REPEAT_SHIFT = 8u };

/* What FindDeletion asks of a gap before anything is looked up (:64-71): both k-mers valid -- the gap is reported and has an anchor before it
 * (both flags) -- and a length of at least k - max_repeat.  There is no upper bound. */
MTG_HD bool gap_is_del_candidate(uint32_t length, uint32_t flags, int k, int max_repeat)
{
    return flags == 3u && (int64_t)length >= (int64_t)k - (int64_t)max_repeat;
}

/* the n lowest nucleotides of an image, 0 <= n <= 32 */
MTG_HD uint64_t del_low_mask(int n) { return n <= 0 ? 0ull : n >= 32 ? ~0ull : (1ull << (2 * n)) - 1ull; }

/* the image of the k nucleotides at position p of a packed sequence (32 to a word; the word behind the last one read exists: the layout of
 * mtg_index_profile_packed_device).  It is le_kmer of mtg_post.h, restated so that this header stands without the fill path's */
MTG_HD uint64_t del_packed_kmer(const uint64_t* w, uint32_t p, int k)
{
    const uint32_t s = 2u * (p & 31u);
    const uint64_t lo = w[p >> 5] >> s, hi = s ? w[(p >> 5) + 1u] << (64u - s) : 0ull;
    return (lo | hi) & del_low_mask(k);
}

/* fuzzy_site (:179-188): the largest i in max_repeat .. 1 with the last i nucleotides of begin equal to the first i of end, else 0.
 * 0 <= max_repeat <= k - 2 */
MTG_HD int del_fuzzy_site(uint64_t begin, uint64_t end, int k, int max_repeat)
{
    for (int i = max_repeat; i > 0; i--)
        if (((begin >> (2 * (k - i))) & del_low_mask(i)) == (end & del_low_mask(i))) return i;
    return 0;
}

/* k-mer j of J_r = begin[0 : k - r] + end, 0 <= j <= k - r: the nucleotides j .. k - r - 1 of begin, then the first j + r of end */
MTG_HD uint64_t del_joined_kmer(uint64_t begin, uint64_t end, int r, int j, int k)
{
    const int n = k - r - j; /* nucleotides taken from begin */
    if (n >= k) return begin & del_low_mask(k);
    if (n <= 0) return end & del_low_mask(k);
    return (((begin >> (2 * j)) & del_low_mask(n)) | (end << (2 * n))) & del_low_mask(k);
}

/* del_size for the final r (:90,136) and the record's pos */
MTG_HD int64_t del_size_of(uint32_t length, int r, int k) { return (int64_t)length - (int64_t)k + (int64_t)r + 1; }
MTG_HD uint32_t del_pos_of(uint32_t start, int r, int k) { return start - 1u + (uint32_t)(k - 1 - r); }

} // namespace mtg
#endif
