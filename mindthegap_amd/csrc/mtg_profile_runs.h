/*
 * mtg_profile_runs.h -- the maximal runs of valid-and-absent positions of a sequence, from its two bit planes (valid, present; bit p % 64 of
 * word p / 64 = position p, bits at and past the number of positions ignored).  The word-level logic of k_profile_count / k_profile_write
 * (mtg_gpu_misc.hip); the same source is compiled by g++ into tests/emu/profile_runs.cpp, which checks it against a literal loop.
 *
 * A run is a maximal stretch of positions that are valid and not present.  An invalid position is in no run: it ends one, and it does not
 * count as a bound (flags bit 0 / bit 1 ask for a PRESENT position right before / right behind the run).  Every run has one first and one
 * last position and runs do not nest, so the j-th first position of a sequence and its j-th last position belong to the same run: whoever
 * holds a word numbers its firsts from the firsts before the word, its lasts from the same count less one when a run is open across the
 * word's lower seam, and writes its half of each record -- no thread ever looks further than the two neighbouring words, whatever the length
 * of the run.
 *
 * Also here, as word logic on a plane of the same layout: covers_bad, the test of k_profile, k_find_assemble and k_het_judge for a k-mer that
 * covers a character that is no nucleotide.
 */
#ifndef MTG_PROFILE_RUNS_H
#define MTG_PROFILE_RUNS_H
#include "../../include/mtg_fill.h"
#include "mtg_dev.h"

namespace mtg {

struct RunWord {
    uint64_t first;  /* positions of the word where a run begins */
    uint64_t last;   /* positions where one ends */
    uint64_t lflag;  /* subset of first: the position before it exists and is present */
    uint64_t rflag;  /* subset of last: the position behind it exists and is present */
    uint32_t open;   /* 1: the run of the word's position 0 began in an earlier word */
};

/* number of plane words of a sequence with npos positions */
MTG_HD uint32_t run_words(uint32_t npos) { return (npos >> 6) + ((npos & 63u) ? 1u : 0u); }
/* word w of a plane, positions at and past npos cleared; 0 outside the sequence */
MTG_DEV uint64_t run_plane_word(const uint64_t* plane, uint32_t w, uint32_t nw, uint32_t npos)
{
    if (w >= nw) return 0ull;
    const uint64_t x = plane[w];
    return (w + 1u == nw && (npos & 63u)) ? (x & ((1ull << (npos & 63u)) - 1ull)) : x;
}

/* do the k characters from position p (k <= 32) hold one that is no nucleotide: any of the k bits from p of the bad plane (one bit per
 * CHARACTER, same layout).  At most two words; the second is read only when the bits reach into it */
MTG_DEV bool covers_bad(const uint64_t* bw, uint32_t p, int k)
{
    const uint32_t sh = p & 63u;
    uint64_t m = bw[p >> 6] >> sh;
    if (sh + (uint32_t)k > 64u) m |= bw[(p >> 6) + 1] << (64u - sh);
    return (m & ((1ull << k) - 1ull)) != 0;
}

MTG_DEV RunWord run_word(const uint64_t* vplane, const uint64_t* pplane, uint32_t w, uint32_t npos)
{
    const uint32_t nw = run_words(npos);
    uint64_t v[3], p[3]; /* the word before, the word, the word behind */
MTG_UNROLL
    for (int i = 0; i < 3; i++) {
        const bool in = !(i == 0 && w == 0);
        v[i] = in ? run_plane_word(vplane, w + (uint32_t)i - 1u, nw, npos) : 0ull;
        p[i] = in ? run_plane_word(pplane, w + (uint32_t)i - 1u, nw, npos) & v[i] : 0ull;
    }
    const uint64_t a = v[1] & ~p[1], a_before = (v[0] & ~p[0]) >> 63, a_behind = (v[2] & ~p[2]) & 1ull;
    RunWord r;
    r.first = a & ~((a << 1) | a_before);
    r.last = a & ~((a >> 1) | (a_behind << 63));
    r.lflag = r.first & ((p[1] << 1) | (p[0] >> 63));
    r.rflag = r.last & ((p[1] >> 1) | ((p[2] & 1ull) << 63));
    r.open = (uint32_t)(a_before & a & 1ull);
    return r;
}

MTG_DEV uint32_t run_popc(uint64_t x)
{
#ifdef MTG_EMU
    return (uint32_t)__builtin_popcountll(x);
#else
    return (uint32_t)__popcll(x);
#endif
}
MTG_DEV uint32_t run_ctz(uint64_t x)
{
#ifdef MTG_EMU
    return (uint32_t)__builtin_ctzll(x);
#else
    return (uint32_t)__ffsll((unsigned long long)x) - 1u;
#endif
}

/* The halves of the records that word w of sequence seq holds.  `before` = runs of the whole input that begin before this word (those of the
 * sequences before seq and of the words before w); records at and past cap are not written.  The records must have been zeroed: the first
 * position writes seq and start, the last one leaves its END (start + length) in `length` -- run_finish turns it into the length once both
 * halves are there -- and each ORs its flag in. */
MTG_DEV void run_emit_word(const RunWord& r, uint32_t seq, uint32_t w, uint64_t before, mtg_run* runs, uint64_t cap)
{
    uint64_t i = before;
    for (uint64_t m = r.first; m; m &= m - 1ull, i++) {
        if (i >= cap) break;
        const uint32_t b = run_ctz(m);
        runs[i].seq = seq;
        runs[i].start = w * 64u + b;
        if ((r.lflag >> b) & 1ull) atomic_or32(&runs[i].flags, 1u);
    }
    i = before - r.open;
    for (uint64_t m = r.last; m; m &= m - 1ull, i++) {
        if (i >= cap) break;
        const uint32_t b = run_ctz(m);
        runs[i].length = w * 64u + b + 1u;
        if ((r.rflag >> b) & 1ull) atomic_or32(&runs[i].flags, 2u);
    }
}
MTG_DEV uint32_t run_finish(mtg_run& r) { r.length -= r.start; return r.length; }

} // namespace mtg
#endif
