/*
 * mtg_find_msnp.h -- the logic of `find` for close homozygous SNPs (FindMultiSNP::update with FindSNP::snp_at_end and correct_history,
 * src/FindSNP.hpp:435-564, :139-208) on one gap of the scan (mtg_find_gaps.h).  Shared by k_gap_mark<MultiObserver>, k_msnp_bound, k_msnp_judge
 * and k_msnp_emit (mtg_gpu_misc.hip); the same source is compiled by g++ into tests/emu/find_msnp.cpp, which checks it against literal string
 * loops.  Windows, alternatives and characters are those of mtg_find_snp.h.  The reverse pass (FindMultiSNPrev::update with snp_at_begin,
 * :593-709, :219-293), shared by k_msnp_rev_judge and k_msnp_rev_emit and compiled into tests/emu/find_msnp_rev.cpp, stands at the end.
 *
 * The observer takes a gap of L > k + m positions from `start` with both k-mers valid (m = snp_min_val) and walks it from the left, a
 * cursor c = 0 .. L: snp_at_end at the k-mer at start + c mutates the position g = start + c + k - 1, and a call puts the winner into the
 * k-mer history (correct_history), so the next step reads the corrected text.  Reduced to a pure function of the gap, with T a private copy
 * of the text, while c != L:
 *   1. ref = T[g]; cap = min(k, L - c + 1).
 *   2. f(a), for each of the three other nucleotides, = the number of leading windows j = 0, 1, .. < cap in the graph; window j is the k-mer
 *      of T at start + c + j with g (its nucleotide k - 1 - j) replaced by a.  The reference goes on to j < k: from j = L - c + 1 on it reads
 *      history slots at or beyond the scan position, partly stale ones.  A count that reaches cap < k gives c + M > L, the stop of step 4, so
 *      what lies behind cap decides nothing.  All text read lies in [start, start + L + k), inside the sequence: start + L and start + L + 1
 *      are anchors.
 *   3. M = max f.  M == k: the winner is the FIRST alternative in A, C, T, G order with f == k.  M < k: the LAST one in that order with
 *      f == M (the map erases a failing alternative unless it is the only one left: of those that fail in the same round the last one
 *      visited survives with its count).
 *   4. M < m: stop.  c + M > L: stop, no call, c unchanged (the reference's "did not go beyond the gap").
 *   5. a SNP at g, REF ref, ALT the winner; T[g] = winner; c += M.
 * The outcome is the list of calls and consumed = c: L = the gap is taken, 0 < c < L = partial (the reference shrinks the gap for the later
 * observers: not built), 0 = untouched.  A call advances c by M >= m and keeps c <= L: at most L / m calls.
 *
 * DEVIATION: the reference's history is a ring of 256 slots addressed by unsigned char.  From L = 255 on the ring has been overwritten and
 * its index arithmetic wraps (at L = 256 its loop does not even start); it reports positions it did not look at.  GAPS OF 255 POSITIONS AND
 * MORE ARE NOT JUDGED: counted, no call.
 *
 * k-mers are little-endian images (mtg_post.h: le_kmer): nucleotide i in bits 2i, 2i + 1; k <= 32.  Codes: A 0, C 1, T 2, G 3.
 */
#ifndef MTG_FIND_MSNP_H
#define MTG_FIND_MSNP_H
#include "mtg_find_snp.h"

namespace mtg {

/* the longest gap that is judged, and the packed words its text [start, start + L + k) can span: (31 + 254 + 32 - 1) / 32 + 1
 * (the text of both passes, [start - 1, start + L + k), spans no more: (31 + 254 + 32) / 32 + 1) */
enum : uint32_t { MSNP_MAX_GAP = 254u, MSNP_TEXT_WORDS = 10u };
/* one SNP of a gap, an entry of the gap's slab: MSNP_ENTRY | c (the cursor at the call, < 254) | alt << SNP_ALT_SHIFT | ref << SNP_REF_SHIFT.
 * Never 0: an unused slab entry is.  A call of the reverse pass (below) has MSNP_REV set and its cursor d in place of c */
enum : uint32_t { MSNP_ENTRY = 1u << 31 };

/* What FindMultiSNP asks of a gap before anything is looked up (:461-467): both k-mers valid and L > k + m.  max_repeat plays no part */
MTG_HD bool gap_is_msnp_candidate(uint32_t length, uint32_t flags, int k, int m) { return flags == 3u && length > (uint32_t)(k + m); }
/* of the candidates, the ones that are judged; the room for their calls */
MTG_HD bool msnp_is_judged(uint32_t length) { return length <= MSNP_MAX_GAP; }
MTG_HD uint32_t msnp_max_calls(uint32_t length, int m) { return msnp_is_judged(length) ? length / (uint32_t)m : 0u; }

/* how many words from W0 = start / 32 on hold a nucleotide of the gap's text [start, start + L + k): the others are not read */
MTG_HD uint32_t msnp_text_words(uint32_t start, uint32_t length, int k) { return ((start & 31u) + length + (uint32_t)k - 1u) / 32u + 1u; }

/* the k-mer at nucleotide rel of the private text t[0 .. nw) (rel counted from the first nucleotide of t[0]); the word behind is read only
 * when the k-mer reaches into it */
MTG_HD uint64_t msnp_text_kmer(const uint64_t* t, uint32_t rel, int k)
{
    const uint32_t w = rel >> 5, r = rel & 31u;
    return snp_text_kmer(t[w], r + (uint32_t)k > 32u ? t[w + 1u] : 0ull, 0ull, r, k);
}
MTG_HD uint32_t msnp_text_nuc(const uint64_t* t, uint32_t rel) { return (uint32_t)(t[rel >> 5] >> (2u * (rel & 31u))) & 3u; }
MTG_HD uint64_t msnp_substituted(uint64_t word, uint32_t rel, uint32_t a) /* the word of nucleotide rel with that nucleotide replaced */
{
    const uint32_t sh = 2u * (rel & 31u);
    return (word & ~(3ull << sh)) | ((uint64_t)a << sh);
}

MTG_HD uint32_t msnp_cap(uint32_t length, uint32_t c, int k) { return length - c + 1u < (uint32_t)k ? length - c + 1u : (uint32_t)k; }

/* step 3 on the three counts f[i] of the alternatives snp_alt(ref, i): the index of the winner, *best = M */
MTG_HD uint32_t msnp_winner(uint32_t f0, uint32_t f1, uint32_t f2, int k, uint32_t* best)
{
    const uint32_t m01 = f0 > f1 ? f0 : f1, M = m01 > f2 ? m01 : f2;
    *best = M;
    if (M == (uint32_t)k) return f0 == M ? 0u : f1 == M ? 1u : 2u;
    return f2 == M ? 2u : f1 == M ? 1u : 0u;
}
/* step 4: 0 = call, 1 = the best count is below snp_min_val, 2 = the call would go beyond the gap */
MTG_HD uint32_t msnp_stop(uint32_t c, uint32_t best, uint32_t length, int m) { return best < (uint32_t)m ? 1u : c + best > length ? 2u : 0u; }

MTG_HD uint32_t msnp_entry(uint32_t c, uint32_t alt, uint32_t ref) { return MSNP_ENTRY | c | (alt << SNP_ALT_SHIFT) | (ref << SNP_REF_SHIFT); }

/* The chain on a private text: t[0 .. msnp_text_words) = the words from start / 32 on, CHANGED by the calls; rel0 = start % 32.
 * in_graph(image of a k-mer); entries[0 .. msnp_max_calls) receives the calls.  Returns consumed; *n_snps = the calls */
template <typename InGraph>
MTG_HD uint32_t msnp_chain(uint64_t* t, uint32_t rel0, uint32_t length, int k, int m, InGraph in_graph, uint32_t* entries, uint32_t* n_snps)
{
    uint32_t c = 0, n = 0;
    while (c != length) {
        const uint32_t g = rel0 + c + (uint32_t)k - 1u, ref = msnp_text_nuc(t, g), cap = msnp_cap(length, c, k);
        uint32_t f[3], best;
        for (uint32_t i = 0; i < 3u; i++) {
            const uint32_t a = snp_alt(ref, i);
            uint32_t j = 0;
            while (j < cap && in_graph(snp_window(msnp_text_kmer(t, rel0 + c + j, k), (int)j, k, a))) j++;
            f[i] = j;
        }
        const uint32_t alt = snp_alt(ref, msnp_winner(f[0], f[1], f[2], k, &best));
        if (msnp_stop(c, best, length, m)) break;
        entries[n++] = msnp_entry(c, alt, ref);
        t[g >> 5] = msnp_substituted(t[g >> 5], g, alt);
        c += best;
    }
    *n_snps = n;
    return c;
}

/* the record of an entry: pos, and ins as for kind 5 (snp_ins_of reads alt and ref at the same shifts) */
MTG_HD uint32_t msnp_pos_of(uint32_t start, uint32_t entry, int k) { return start + (entry & 0xFFu) + (uint32_t)k - 1u; }

/* ---- The reverse pass: FindMultiSNPrev::update with FindSNP::snp_at_begin (src/FindSNP.hpp:593-709, :219-293), asked right behind the forward
 * observer, on what that one left: the residual gap start' = start + c, L' = L - c (c = the forward chain's consumed, 0 when it is not run),
 * on the SAME private text T with the forward substitutions in place.  It is asked only if c != L and L' > k + m, the reference's own entry
 * test on the shrunken gap, and walks from the right, a cursor d = 0 .. L'; while d != L':
 *   1. q = start + L - 1 - d, ref = T[q], the FIRST nucleotide of the k-mer at q (`>> 2(k-1) & 3` on a gatb k-mer; the "bug" comment at :234
 *      is stale, mutate_kmer(.., j + 1) substitutes at the same place); cap = min(k, L' - d + 1).
 *   2. f(a) = the number of leading windows j = 0, 1, .. < cap in the graph; window j is the k-mer of T at q - j with its nucleotide j (the
 *      position q) replaced by a.  Windows at and beyond cap decide nothing, as in the forward pass.  WINDOW j = L' - d IS THE K-MER AT
 *      start' - 1, THE LEFT ANCHOR, AND IT DOES DECIDE: if it holds, M = L' - d + 1 and step 4 stops the chain without a call; if it fails,
 *      M = L' - d and the gap is taken whole.
 *   3. winner and M: msnp_winner (snp_at_begin has the map, the erasure and the ties of snp_at_end).
 *   4. msnp_stop(d, M, L', m).
 *   5. a SNP at q, REF ref, ALT the winner; T[q] = winner; d += M.
 * consumed_rev = d.  The calls of one gap stand in the order they are made: the forward ones ascending, then the reverse ones DESCENDING in
 * position.  The gap is full if c + d = L, partial if 0 < c + d < L.  Each call consumes >= m of the L positions: L / m bounds both passes
 * together.
 *
 * THE TEXT: the reverse pass reads the nucleotides [start - 1, start + L + k - 1), one to the left of the forward text (start - 1 >= 0: the
 * left k-mer is an anchor).  Both passes together need [start - 1, start + L + k): the words from (start - 1) / 32 on, at most
 * (31 + 254 + 32) / 32 + 1 = 10 = MSNP_TEXT_WORDS.  With start % 32 == 0 the nucleotide start - 1 lies in a word the forward text never holds.
 *
 * DEVIATION (besides the gaps of 255 positions and more, which neither pass judges): THE RING INDICES COUNT AS RESTORED AFTER A GAP.  After
 * a partial take the reference subtracts the consumed length from m_position, m_het_kmer_end_index and m_het_kmer_begin_index (:672-674) and
 * restores m_position alone (src/FindBreakpoints.hpp:441-446); from then on its ring is addressed shifted.  The only text this misaddresses
 * for later gaps is the pair of slots of the two solid positions that closed the gap: a gap that starts exactly two positions behind a gap
 * the reverse pass took in part reads a stale left anchor.  The rule here is the pure function of the gap. */
enum : uint32_t { MSNP_REV = 1u << 12 }; /* in an entry: a call of the reverse pass, its low eight bits = d (< 254) */
enum : int { MSNP_PASS_FWD = 1, MSNP_PASS_REV = 2 }; /* `passes`: 1 forward, 2 reverse, 3 forward then reverse */
MTG_HD bool msnp_passes_valid(int passes) { return passes >= 1 && passes <= 3; }

/* the private text of both passes begins at start - 1: rel0 = the place of that nucleotide in its word (`start` itself is at rel0 + 1), and
 * the words from (start - 1) / 32 on that hold a nucleotide of [start - 1, start + L + k) */
MTG_HD uint32_t msnp_rev_rel0(uint32_t start) { return (start - 1u) & 31u; }
MTG_HD uint32_t msnp_rev_text_words(uint32_t start, uint32_t length, int k) { return (msnp_rev_rel0(start) + length + (uint32_t)k) / 32u + 1u; }

/* the reference's entry test on the gap the forward pass left */
MTG_HD bool msnp_rev_is_asked(uint32_t length, uint32_t c, int k, int m) { return c != length && length - c > (uint32_t)(k + m); }

/* window j of alternative a in the reverse pass: the k-mer at q - j, its nucleotide j replaced (mutate_kmer(.., j + 1)) */
MTG_HD uint64_t msnp_rev_window(uint64_t kmer, uint32_t j, uint32_t a) { return (kmer & ~(3ull << (2u * j))) | ((uint64_t)a << (2u * j)); }

MTG_HD uint32_t msnp_rev_entry(uint32_t d, uint32_t alt, uint32_t ref) { return msnp_entry(d, alt, ref) | MSNP_REV; }
MTG_HD bool msnp_entry_is_rev(uint32_t entry) { return (entry & MSNP_REV) != 0; }
/* the position of a reverse entry: q = start + L - 1 - d */
MTG_HD uint32_t msnp_rev_pos_of(uint32_t start, uint32_t length, uint32_t entry) { return start + length - 1u - (entry & 0xFFu); }

/* The reverse chain on the private text t[0 .. msnp_rev_text_words) = the words from (start - 1) / 32 on, CHANGED by the calls;
 * rel0 = msnp_rev_rel0(start); c = what the forward chain consumed.  The caller has asked msnp_rev_is_asked.  entries receives the calls in
 * the order they are made.  Returns consumed_rev; *n_snps = the calls */
template <typename InGraph>
MTG_HD uint32_t msnp_rev_chain(uint64_t* t, uint32_t rel0, uint32_t length, uint32_t c, int k, int m, InGraph in_graph, uint32_t* entries, uint32_t* n_snps)
{
    const uint32_t left = length - c;
    uint32_t d = 0, n = 0;
    while (d != left) {
        const uint32_t q = rel0 + length - d, ref = msnp_text_nuc(t, q), cap = msnp_cap(left, d, k); /* (start + L - 1 - d) - (start - 1) + rel0 */
        uint32_t f[3], best;
        for (uint32_t i = 0; i < 3u; i++) {
            const uint32_t a = snp_alt(ref, i);
            uint32_t j = 0;
            while (j < cap && in_graph(msnp_rev_window(msnp_text_kmer(t, q - j, k), j, a))) j++;
            f[i] = j;
        }
        const uint32_t alt = snp_alt(ref, msnp_winner(f[0], f[1], f[2], k, &best));
        if (msnp_stop(d, best, left, m)) break;
        entries[n++] = msnp_rev_entry(d, alt, ref);
        t[q >> 5] = msnp_substituted(t[q >> 5], q, alt);
        d += best;
    }
    *n_snps = n;
    return d;
}

/* Forward (if asked), then reverse (if asked, and the entry test holds) on what is left, on one private text that begins at start - 1.
 * entries[0 .. msnp_max_calls): the forward calls, then the reverse ones.  Returns the forward consumed; *consumed_rev, *n_fwd, *n_rev */
template <typename InGraph>
MTG_HD uint32_t msnp_passes_chain(uint64_t* t, uint32_t rel0, uint32_t length, int k, int m, int passes, InGraph in_graph, uint32_t* entries, uint32_t* n_fwd, uint32_t* consumed_rev,
                                  uint32_t* n_rev)
{
    uint32_t c = 0;
    *n_fwd = 0; *consumed_rev = 0; *n_rev = 0;
    if (passes & MSNP_PASS_FWD) c = msnp_chain(t, rel0 + 1u, length, k, m, in_graph, entries, n_fwd);
    if ((passes & MSNP_PASS_REV) && msnp_rev_is_asked(length, c, k, m)) *consumed_rev = msnp_rev_chain(t, rel0, length, c, k, m, in_graph, entries + *n_fwd, n_rev);
    return c;
}

} // namespace mtg
#endif
