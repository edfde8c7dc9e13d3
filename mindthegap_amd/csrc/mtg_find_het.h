/*
 * mtg_find_het.h -- the word-level logic of `find` for heterozygous insertions (FindHeteroInsertion::update, src/FindHeteroInsertion.hpp:46-174)
 * on the bit planes of a sequence (layout of mtg_profile_runs.h): the candidate positions of a plane word, the history rule H(q), the count of
 * valid positions between two positions, and the resolution of the `recent` counter on the ordered list of judged candidates.  Shared by
 * k_het_count / k_het_list / k_het_judge / k_het_chain / k_het_final (mtg_gpu_misc.hip); the same source is compiled by g++ into
 * tests/emu/find_het.cpp, which checks it against literal loops.
 *
 * Planes of a sequence with npos k-mer positions: V valid, IN2 present with in-degree 2, OUT2 present with out-degree 2, BR present with a
 * degree above 1; REP has npos + 1 positions, bit q = the (k-1)-mer at q is repeated (so rep_prefix(p) = REP[p], rep_suffix(q) = REP[q + 1]);
 * a null REP means nothing is repeated.
 *
 * The observer at a valid position p reads the history slots of the positions q = p - k + i, 0 <= i <= max_repeat.  The history is a ring of
 * 256 slots written at valid positions only, so the slot of an invalid q still holds the record of q - 256, q - 512, ... (the first of them
 * that is valid; all zero when there is none): het_history_pos.  The candidate word does not chase that chain: an invalid position in the
 * window makes p a candidate, and the judge, which resolves H(q) exactly, says whether it is one.  Without invalid positions the candidates
 * are exact.
 *
 * `recent`: only an accepted site arms the counter, with max_repeat, and every valid position behind it takes one off.  So the observer is
 * silent at p exactly when an accepted site lies before p in the sequence with 1 .. max_repeat valid positions from the site (exclusive) to p
 * (inclusive).  On the list of judged candidates in scan order: a raw site (judged as if recent were 0) with no raw site within max_repeat
 * valid positions before it heads a chain and is accepted; walking on from it, a raw site within max_repeat valid positions of the last
 * ACCEPTED one is dropped (and arms nothing), any other is accepted; the chain ends at the first raw site more than max_repeat valid
 * positions behind the raw site before it -- that one heads the next chain.  Every other outcome (an insertion of 1-2 nt, a site the
 * branching filter refuses) then looks back for an accepted site within max_repeat valid positions.  Candidates are valid positions, so no
 * look goes further than max_repeat entries of the list.
 */
#ifndef MTG_FIND_HET_H
#define MTG_FIND_HET_H
#include "mtg_profile_runs.h"

namespace mtg {

enum : uint32_t { HET_NONE = 0, HET_INS = 1, HET_SITE = 2, HET_FILTERED = 3 }; /* HetEntry::out, judged as if recent were 0 */
enum : uint32_t { HET_ACCEPTED = 1, HET_DROPPED = 2 };                         /* HetEntry::state of a raw site */
struct HetEntry {
    uint32_t seq, p;   /* the candidate */
    uint32_t out;      /* HET_* */
    uint32_t rep;      /* the first qualifying i */
    uint32_t left;     /* position whose text the history slot holds */
    uint32_t ins;      /* HET_INS: index of the inserted string */
    uint32_t state;    /* HET_SITE: accepted / dropped */
    uint32_t pad;
};

MTG_DEV uint64_t het_bit(const uint64_t* plane, uint32_t q) { return (plane[q >> 6] >> (q & 63u)) & 1ull; }

/* the position whose record the history slot of q holds when the observer reads it (q below the current position, within 255 of it): q itself
 * when valid, else the first valid one of q - 256, q - 512, ...; -1: the slot is still zero */
MTG_DEV int64_t het_history_pos(const uint64_t* vplane, int64_t q)
{
    while (q >= 0 && !het_bit(vplane, (uint32_t)q)) q -= 256;
    return q < 0 ? -1 : q;
}

/* word w of the candidates of a sequence: bit p = V[p] & IN2[p] & !REP[p] & any over i of T[p - k + i], T[q] = (OUT2[q] & !REP[q + 1]) | !V[q]
 * for 0 <= q < npos and 0 before the sequence.  0 <= max_repeat <= k - 2, k <= 32: the window lies 2 .. 32 positions back, in this word and
 * the one before */
MTG_DEV uint64_t het_cand_word(const uint64_t* v, const uint64_t* in2, const uint64_t* out2, const uint64_t* rep, uint32_t w, uint32_t npos, int k, int max_repeat)
{
    const uint32_t nw = run_words(npos), nwr = run_words(npos + 1u);
    uint64_t t[2]; /* T of the word before, of the word */
MTG_UNROLL
    for (int i = 0; i < 2; i++) {
        t[i] = 0ull;
        if (i == 0 && w == 0) continue;
        const uint32_t ww = w + (uint32_t)i - 1u;
        if (ww >= nw) continue;
        const uint64_t in_seq = (ww + 1u == nw && (npos & 63u)) ? ((1ull << (npos & 63u)) - 1ull) : ~0ull;
        const uint64_t vv = run_plane_word(v, ww, nw, npos), oo = run_plane_word(out2, ww, nw, npos);
        const uint64_t r1 = rep ? (run_plane_word(rep, ww, nwr, npos + 1u) >> 1) | (run_plane_word(rep, ww + 1u, nwr, npos + 1u) << 63) : 0ull;
        t[i] = (oo & vv & ~r1) | (~vv & in_seq);
    }
    uint64_t any = 0ull;
    for (int i = 0; i <= max_repeat; i++) {
        const uint32_t d = (uint32_t)(k - i); /* 2 .. 32 */
        any |= (t[1] << d) | (t[0] >> (64u - d));
    }
    const uint64_t rr = rep ? run_plane_word(rep, w, nwr, npos + 1u) : 0ull;
    return run_plane_word(v, w, nw, npos) & run_plane_word(in2, w, nw, npos) & ~rr & any;
}

/* valid positions in (a, b], a < b < npos; the count stops once it is above limit */
MTG_DEV uint32_t het_vdist(const uint64_t* vplane, uint32_t a, uint32_t b, uint32_t limit)
{
    const uint32_t lo = a + 1u;
    uint32_t n = 0;
    for (uint32_t w = lo >> 6; w <= (b >> 6) && n <= limit; w++) {
        uint64_t x = vplane[w];
        if (w == (lo >> 6)) x &= ~0ull << (lo & 63u);
        if (w == (b >> 6) && (b & 63u) != 63u) x &= (2ull << (b & 63u)) - 1ull;
        n += run_popc(x);
    }
    return n;
}

/* entry c is a raw site: no raw site lies within max_repeat valid positions before it */
MTG_DEV bool het_is_head(const HetEntry* e, const uint64_t* vbits, const uint64_t* word_off, uint64_t c, uint32_t max_repeat)
{
    const uint64_t* vp = vbits + word_off[e[c].seq];
    for (uint64_t j = c; j-- > 0;) {
        if (e[j].seq != e[c].seq || het_vdist(vp, e[j].p, e[c].p, max_repeat) > max_repeat) break;
        if (e[j].out == HET_SITE) return false;
    }
    return true;
}
/* the chain headed by entry c: every raw site of it is accepted or dropped */
MTG_DEV void het_walk_chain(HetEntry* e, uint64_t n, const uint64_t* vbits, const uint64_t* word_off, uint64_t c, uint32_t max_repeat)
{
    const uint64_t* vp = vbits + word_off[e[c].seq];
    e[c].state = HET_ACCEPTED;
    uint32_t last_accepted = e[c].p, last_raw = e[c].p;
    for (uint64_t j = c + 1; j < n; j++) {
        if (e[j].seq != e[c].seq || het_vdist(vp, last_raw, e[j].p, max_repeat) > max_repeat) break;
        if (e[j].out != HET_SITE) continue;
        if (het_vdist(vp, last_accepted, e[j].p, max_repeat) > max_repeat) { e[j].state = HET_ACCEPTED; last_accepted = e[j].p; }
        else e[j].state = HET_DROPPED;
        last_raw = e[j].p;
    }
}
/* an accepted site lies within max_repeat valid positions before entry c (once the chains are resolved) */
MTG_DEV bool het_suppressed(const HetEntry* e, const uint64_t* vbits, const uint64_t* word_off, uint64_t c, uint32_t max_repeat)
{
    const uint64_t* vp = vbits + word_off[e[c].seq];
    for (uint64_t j = c; j-- > 0;) {
        if (e[j].seq != e[c].seq || het_vdist(vp, e[j].p, e[c].p, max_repeat) > max_repeat) break;
        if (e[j].out == HET_SITE && e[j].state == HET_ACCEPTED) return true;
    }
    return false;
}

} // namespace mtg
#endif
