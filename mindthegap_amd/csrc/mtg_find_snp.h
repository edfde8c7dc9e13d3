/*
 * mtg_find_snp.h -- the logic of `find` for isolated homozygous SNPs (FindSoloSNP::update with FindSNP::snp_at_end, src/FindSNP.hpp:297-355,
 * :139-208) on one gap of the scan (mtg_find_gaps.h).  Shared by SoloObserver (k_gap_mark / k_gap_emit) and k_snp_judge (mtg_gpu_misc.hip); the
 * same source is compiled by g++ into tests/emu/find_snp.cpp, which checks it against literal string loops.
 *
 * The observer is a pure function of the gap: it looks at gaps of exactly k positions with both k-mers valid, and at the k k-mers of the gap
 * itself, those at start .. start + k - 1, which are the k k-mers that cover the position g = start + k - 1.  With ref the nucleotide at g,
 * window j of an alternative a is the k-mer at start + j with position g -- its nucleotide k - 1 - j -- replaced by a.  snp_at_end keeps a map
 * of the three alternatives in the order of their codes (A, C, T, G: T before G), erases one at its first window that is not in the graph
 * unless it is the last one left, and with limit = k asks the best count to be k.  A count of k is an alternative whose k windows are all in
 * the graph, every such alternative survives with the same count, and the first of the map wins: THE CALL IS THE FIRST ALTERNATIVE IN A, C,
 * T, G ORDER, ref LEFT OUT, WHOSE k WINDOWS ARE ALL IN THE GRAPH; with none there is no call.  The record's pos is g (position() - 2 with
 * position() = start + k + 1).  The call corrects the reference's k-mer history, which only the heterozygous observer reads: not done here.
 *
 * k-mers are little-endian images (mtg_post.h: le_kmer): nucleotide i in bits 2i, 2i + 1; k <= 32.  Codes: A 0, C 1, T 2, G 3.
 */
#ifndef MTG_FIND_SNP_H
#define MTG_FIND_SNP_H
#include "mtg_find_gaps.h"

namespace mtg {

/* result word of k_snp_judge for one candidate: SNP_CALLED | alt << SNP_ALT_SHIFT | ref << SNP_REF_SHIFT (codes); 0: no call */
enum : uint32_t { SNP_CALLED = 1u, SNP_ALT_SHIFT = 8u, SNP_REF_SHIFT = 10u };

/* What FindSoloSNP asks of a gap before anything is looked up (:321-326): both k-mers valid (both flags) and a length of exactly k.
 * max_repeat plays no part */
MTG_HD bool gap_is_snp_candidate(uint32_t length, uint32_t flags, int k, int /*max_repeat*/) { return flags == 3u && length == (uint32_t)k; }

MTG_HD uint64_t snp_low_mask(int n) { return n <= 0 ? 0ull : n >= 32 ? ~0ull : (1ull << (2 * n)) - 1ull; }

/* The packed text that the k windows of a gap at `start` span, [start, start + 2k - 1), lies in the words W0 = start / 32 .. W0 + 2 at the
 * most: how many of the three hold a nucleotide of it (the others are not read, they need not exist) */
MTG_HD uint32_t snp_text_words(uint32_t start, int k) { return ((start & 31u) + 2u * (uint32_t)k - 2u) / 32u + 1u; }

/* the image of the k nucleotides at position rel of the text held by three words t[0 .. 2], 0 <= rel <= 62 */
MTG_HD uint64_t snp_text_kmer(uint64_t t0, uint64_t t1, uint64_t t2, uint32_t rel, int k)
{
    const uint32_t s = 2u * (rel & 31u);
    const uint64_t a = rel < 32u ? t0 : t1, b = rel < 32u ? t1 : t2;
    return ((a >> s) | (s ? b << (64u - s) : 0ull)) & snp_low_mask(k);
}

/* window j (0 <= j < k) of alternative a: the k-mer at start + j, its nucleotide k - 1 - j replaced (mutate_kmer, :88-96) */
MTG_HD uint64_t snp_window(uint64_t kmer, int j, int k, uint32_t a)
{
    const int sh = 2 * (k - 1 - j);
    return (kmer & ~(3ull << sh)) | ((uint64_t)a << sh);
}

/* the i-th (0 .. 2) of the three alternatives to ref in the order of the codes */
MTG_HD uint32_t snp_alt(uint32_t ref, uint32_t i) { return i < ref ? i : i + 1u; }

/* the rule on packed words: the code of the called alternative, -1 for none; *ref_out = the code at g.  in_graph(image of a k-mer) */
template <typename InGraph>
MTG_HD int snp_solo_call(const uint64_t* w, uint32_t start, int k, InGraph in_graph, uint32_t* ref_out)
{
    const uint32_t w0 = start >> 5, nw = snp_text_words(start, k), rel0 = start & 31u;
    const uint64_t t0 = w[w0], t1 = nw > 1u ? w[w0 + 1u] : 0ull, t2 = nw > 2u ? w[w0 + 2u] : 0ull;
    const uint32_t ref = (uint32_t)(snp_text_kmer(t0, t1, t2, rel0, k) >> (2 * (k - 1))) & 3u;
    *ref_out = ref;
    for (uint32_t i = 0; i < 3u; i++) {
        const uint32_t a = snp_alt(ref, i);
        bool all = true;
        for (int j = 0; j < k && all; j++) all = in_graph(snp_window(snp_text_kmer(t0, t1, t2, rel0 + (uint32_t)j, k), j, k, a));
        if (all) return (int)a;
    }
    return -1;
}

/* the record: pos, and ins = ALT's upper-case ASCII | REF's << 8 (nuc_to_char, :99-117) */
MTG_HD uint32_t snp_pos_of(uint32_t start, int k) { return start + (uint32_t)k - 1u; }
MTG_HD uint32_t snp_char(uint32_t code) { return (0x47544341u >> (8u * (code & 3u))) & 0xFFu; } /* "ACTG" */
MTG_HD uint32_t snp_ins_of(uint32_t res) { return snp_char(res >> SNP_ALT_SHIFT) | (snp_char(res >> SNP_REF_SHIFT) << 8); }

} // namespace mtg
#endif
