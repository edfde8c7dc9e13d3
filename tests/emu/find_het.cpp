/*
 * TEST-ONLY: the word-level logic of `find` for heterozygous insertions (mindthegap_amd/csrc/mtg_find_het.h, shared with k_het_count / k_het_list /
 * k_het_judge / k_het_chain / k_het_final) compiled by g++ and checked against literal loops.
 *
 * Three literal loops.  cand_loop() is the candidate rule position by position.  ring_loop() keeps the reference's ring of 256 history slots
 * (two unsigned bytes as indices, written at valid positions only) and asks, at every valid position, which position each slot the observer
 * may read holds: het_history_pos must say the same.  recent_loop() is the counter m_recent_hetero over the positions of a sequence, given
 * what the observer would do at each (nothing / insertion of 1-2 nt / site / site refused by the branching filter): the chain resolution on
 * the ordered list of entries must accept, drop and silence the same ones, whatever the order in which the heads are visited.
 *   1. one site (an IN2 position p, an OUT2 position p - k + i) at every alignment against the 64-bit seams, for k = 5, 13, 31, 32 and every
 *      i in 0 .. max_repeat and one past it, with a repeat flag on the prefix of p, on the suffix of q, on both, and with q invalid;
 *   2. windows clipped at both ends of the sequence: p below k, q = 0, p the last position, the repeat flag of the last (k-1)-mer;
 *   3. chains of 1 to 4 raw sites at spacings max_repeat and max_repeat + 1, slid over the seams, with insertions and refused sites between
 *      and behind them and with invalid positions that stretch the distances;
 *   4. random planes and random outcomes, several sequences at arbitrary word offsets, junk past the last position.
 * Prints "OK <cases> cases <candidates> candidates <entries> entries".
 */
#include "../../mindthegap_amd/csrc/mtg_find_het.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace mtg;

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd()
{
    rng_state += 0x9E3779B97F4A7C15ull;
    uint64_t z = rng_state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct Seq {
    std::vector<uint8_t> valid, in2, out2; /* per position */
    std::vector<uint8_t> rep;              /* per (k-1)-mer position: one more */
    std::vector<uint8_t> outcome;          /* per position: what the observer would do there (HET_*), read where the position has an entry */
    uint64_t word_off;
};
static Seq make(uint32_t npos)
{
    Seq q;
    q.word_off = 0;
    q.valid.assign(npos, 1); q.in2.assign(npos, 0); q.out2.assign(npos, 0); q.rep.assign(npos + 1, 0); q.outcome.assign(npos, 0);
    return q;
}

struct Planes {
    std::vector<uint64_t> v, in2, out2, rep, word_off;
};
static Planes planes_of(const std::vector<Seq>& seqs, bool junk)
{
    Planes P;
    size_t nwords = 0;
    for (const Seq& q : seqs) nwords = std::max(nwords, (size_t)q.word_off + q.valid.size() / 64 + 2);
    P.v.resize(nwords + 1); P.in2.resize(nwords + 1); P.out2.resize(nwords + 1); P.rep.resize(nwords + 1);
    for (size_t i = 0; i <= nwords; i++) { P.v[i] = junk ? rnd() : 0; P.in2[i] = junk ? rnd() : 0; P.out2[i] = junk ? rnd() : 0; P.rep[i] = junk ? rnd() : 0; }
    for (const Seq& q : seqs) {
        P.word_off.push_back(q.word_off);
        const uint32_t npos = (uint32_t)q.valid.size();
        for (uint32_t w = 0; w < run_words(npos + 1); w++) {
            uint64_t v = 0, a = 0, o = 0, r = 0;
            for (uint32_t b = 0; b < 64; b++) {
                const uint32_t i = w * 64 + b;
                const uint64_t j = junk ? rnd() : 0;
                /* the present planes are subsets of the valid one, as k_profile writes them */
                if (i < npos) { v |= (uint64_t)(q.valid[i] != 0) << b; a |= (uint64_t)(q.valid[i] && q.in2[i]) << b; o |= (uint64_t)(q.valid[i] && q.out2[i]) << b; }
                else { v |= (j & 1) << b; a |= ((j >> 1) & 1) << b; o |= ((j >> 2) & 1) << b; }
                if (i < npos + 1) r |= (uint64_t)(q.rep[i] != 0) << b;
                else r |= ((j >> 3) & 1) << b;
            }
            if (w < run_words(npos)) { P.v[q.word_off + w] = v; P.in2[q.word_off + w] = a; P.out2[q.word_off + w] = o; }
            P.rep[q.word_off + w] = r;
        }
    }
    return P;
}

/* the candidate rule, position by position */
static void cand_loop(const Seq& q, int k, int max_repeat, std::vector<uint32_t>& out)
{
    out.clear();
    const int64_t npos = (int64_t)q.valid.size();
    for (int64_t p = 0; p < npos; p++) {
        if (!q.valid[p] || !q.in2[p] || q.rep[p]) continue;
        bool any = false;
        for (int i = 0; i <= max_repeat; i++) {
            const int64_t h = p - k + i;
            if (h < 0) continue;
            any = any || !q.valid[h] || (q.out2[h] && !q.rep[h + 1]);
        }
        if (any) out.push_back((uint32_t)p);
    }
}

static unsigned long long n_cases = 0, n_cand = 0, n_entries = 0;
static void fail(const char* what) { printf("FAIL (%s)\n", what); exit(1); }

static void check_candidates(const std::vector<Seq>& seqs, int k, int max_repeat, bool junk, bool with_rep, const char* what)
{
    std::vector<Seq> local = seqs;
    if (!with_rep) for (Seq& q : local) std::fill(q.rep.begin(), q.rep.end(), 0);
    const Planes P = planes_of(local, junk);
    for (size_t s = 0; s < local.size(); s++) {
        std::vector<uint32_t> want, got;
        cand_loop(local[s], k, max_repeat, want);
        const uint32_t npos = (uint32_t)local[s].valid.size();
        const uint64_t o = local[s].word_off;
        for (uint32_t w = 0; w < run_words(npos); w++)
            for (uint64_t m = het_cand_word(P.v.data() + o, P.in2.data() + o, P.out2.data() + o, with_rep ? P.rep.data() + o : nullptr, w, npos, k, max_repeat); m; m &= m - 1)
                got.push_back(w * 64 + run_ctz(m));
        if (got != want) {
            printf("FAIL (%s): sequence %zu of %u positions, k %d, max_repeat %d: %zu candidates, %zu expected\n", what, s, npos, k, max_repeat, got.size(), want.size());
            for (size_t i = 0; i < std::max(got.size(), want.size()) && i < 20; i++) printf("  got %d want %d\n", i < got.size() ? (int)got[i] : -1, i < want.size() ? (int)want[i] : -1);
            exit(1);
        }
        n_cand += want.size();
    }
    n_cases++;
}

/* the ring of 256 slots (src/FindBreakpoints.hpp:403-407,423,1037): which position each slot the observer reads holds, at every valid position */
static void check_history(const Seq& q, int k, int max_repeat)
{
    const std::vector<Seq> one(1, q);
    const Planes P = planes_of(one, false);
    int64_t slot[256];
    for (int i = 0; i < 256; i++) slot[i] = -1;
    uint8_t end_index = (uint8_t)(k + 1), begin_index = 1;
    for (int64_t p = 0; p < (int64_t)q.valid.size(); p++, end_index++, begin_index++) {
        if (!q.valid[p]) continue;
        slot[end_index] = p;
        for (int i = 0; i <= max_repeat; i++)
            if (slot[(uint8_t)(begin_index + i)] != het_history_pos(P.v.data() + q.word_off, p - k + i)) fail("history slot of the window");
        for (int j = 1; j <= 100; j++)
            if (slot[(uint8_t)(begin_index - j)] != het_history_pos(P.v.data() + q.word_off, p - k - j)) fail("history slot of the branching window");
    }
    n_cases++;
}

/* m_recent_hetero over the positions with an entry; state per entry: 1 = call (accepted site, insertion), 2 = silenced site or insertion,
 * 3 = refused site counted, 0 = nothing */
static void recent_loop(const std::vector<Seq>& seqs, const std::vector<HetEntry>& e, int max_repeat, std::vector<uint8_t>& state)
{
    state.assign(e.size(), 0);
    size_t c = 0;
    for (size_t s = 0; s < seqs.size(); s++) {
        int recent = 0;
        for (uint32_t p = 0; p < seqs[s].valid.size(); p++) {
            if (!seqs[s].valid[p]) continue;
            bool armed = false;
            if (c < e.size() && e[c].seq == s && e[c].p == p) {
                const uint32_t out = e[c].out;
                if (recent != 0) state[c] = (out == HET_SITE || out == HET_INS) ? 2 : 0;
                else if (out == HET_SITE) { state[c] = 1; recent = max_repeat; armed = true; }
                else if (out == HET_INS) state[c] = 1;
                else if (out == HET_FILTERED) state[c] = 3;
                c++;
            }
            if (!armed) recent = std::max(0, recent - 1);
        }
    }
    if (c != e.size()) fail("the entries are not positions of the sequences in order");
}

/* entries = the positions with a non-zero mark, outcomes from Seq::outcome */
static void check_chains(const std::vector<Seq>& seqs, const std::vector<std::vector<uint8_t>>& is_entry, int max_repeat, bool junk, const char* what)
{
    const Planes P = planes_of(seqs, junk);
    std::vector<HetEntry> e;
    for (size_t s = 0; s < seqs.size(); s++)
        for (uint32_t p = 0; p < seqs[s].valid.size(); p++)
            if (seqs[s].valid[p] && is_entry[s][p]) { HetEntry h; memset(&h, 0, sizeof h); h.seq = (uint32_t)s; h.p = p; h.out = seqs[s].outcome[p]; e.push_back(h); }
    std::vector<uint8_t> want;
    recent_loop(seqs, e, max_repeat, want);
    /* the heads in an arbitrary order: no chain depends on another */
    std::vector<size_t> order(e.size());
    for (size_t i = 0; i < e.size(); i++) order[i] = i;
    for (size_t i = e.size(); i > 1; i--) std::swap(order[i - 1], order[rnd() % i]);
    for (size_t c : order)
        if (e[c].out == HET_SITE && het_is_head(e.data(), P.v.data(), P.word_off.data(), c, (uint32_t)max_repeat)) het_walk_chain(e.data(), e.size(), P.v.data(), P.word_off.data(), c, (uint32_t)max_repeat);
    for (size_t c = 0; c < e.size(); c++) {
        uint8_t got = 0;
        if (e[c].out == HET_SITE) {
            if (e[c].state != HET_ACCEPTED && e[c].state != HET_DROPPED) fail("a raw site is in no chain");
            got = e[c].state == HET_ACCEPTED ? 1 : 2;
        } else if (e[c].out != HET_NONE) {
            const bool quiet = het_suppressed(e.data(), P.v.data(), P.word_off.data(), c, (uint32_t)max_repeat);
            got = e[c].out == HET_INS ? (quiet ? 2 : 1) : (quiet ? 0 : 3);
        }
        if (got != want[c]) {
            printf("FAIL (%s): max_repeat %d, entry %zu (sequence %u, position %u, outcome %u): %u, expected %u\n", what, max_repeat, c, e[c].seq, e[c].p, e[c].out, got, want[c]);
            for (size_t i = 0; i < e.size() && i < 30; i++) printf("  %u %u out %u state %u want %u\n", e[i].seq, e[i].p, e[i].out, e[i].state, want[i]);
            exit(1);
        }
    }
    n_entries += e.size();
    n_cases++;
}

int main()
{
    /* 1. one site at every alignment */
    for (int k : {5, 13, 31, 32})
        for (int max_repeat : {0, 3, k - 2}) {
            if (max_repeat > k - 2) continue;
            for (uint32_t p = 0; p < 200; p++)
                for (int i = 0; i <= max_repeat + 1; i++) {
                    if ((int64_t)p - k + i < 0 || (int64_t)p - k + i >= (int64_t)p) continue;
                    if (k > 5 && max_repeat == k - 2 && (p * 3 + (uint32_t)i) % 4 != 0) continue; /* a quarter of the alignments for the widest window */
                    for (int variant = 0; variant < 5; variant++) {
                        std::vector<Seq> seqs(1, make(270));
                        Seq& q = seqs[0];
                        q.word_off = 1;
                        const uint32_t h = p - (uint32_t)k + (uint32_t)i;
                        q.in2[p] = 1; q.out2[h] = 1;
                        if (variant == 1 || variant == 3) q.rep[p] = 1;
                        if (variant == 2 || variant == 3) q.rep[h + 1] = 1;
                        if (variant == 4) q.valid[h] = 0;
                        check_candidates(seqs, k, max_repeat, (p + (uint32_t)i) & 1, true, "one site");
                        if (variant == 0) check_candidates(seqs, k, max_repeat, false, false, "one site, no repeat plane");
                    }
                }
        }
    /* 2. windows clipped at both ends; every position a would-be site */
    for (int k : {5, 31})
        for (uint32_t npos : {1u, 2u, 4u, 5u, 6u, 30u, 31u, 32u, 63u, 64u, 65u, 128u, 129u})
            for (int variant = 0; variant < 4; variant++) {
                std::vector<Seq> seqs(1, make(npos));
                Seq& q = seqs[0];
                std::fill(q.in2.begin(), q.in2.end(), 1);
                std::fill(q.out2.begin(), q.out2.end(), 1);
                if (variant == 1) q.rep[npos] = 1;                          /* the suffix of the last k-mer */
                if (variant == 2) { q.rep[0] = 1; q.rep[1] = 1; }            /* the prefix and the suffix of the first */
                if (variant == 3) { q.valid[0] = 0; q.valid[npos - 1] = 0; }
                for (int max_repeat : {0, 2, k - 2}) check_candidates(seqs, k, max_repeat, true, true, "clipped windows");
                check_history(q, k, k - 2);
            }
    { std::vector<Seq> none; check_candidates(none, 31, 5, false, true, "no sequence"); }
    /* 3. chains of 1 to 4 raw sites at spacings max_repeat and max_repeat + 1, with other outcomes between and behind them */
    for (int max_repeat : {0, 1, 5, 29})
        for (uint32_t n = 1; n <= 4; n++)
            for (uint32_t spacing = 0; spacing < (1u << (n - 1)); spacing++)
                for (uint32_t start = 0; start < 140; start += (max_repeat == 29 ? 7 : 1))
                    for (int variant = 0; variant < 4; variant++) {
                        std::vector<Seq> seqs(2, make(400));
                        std::vector<std::vector<uint8_t>> mark(2, std::vector<uint8_t>(400, 0));
                        seqs[0].word_off = 0; seqs[1].word_off = 9;
                        Seq& q = seqs[1];
                        uint32_t p = start + 2;
                        for (uint32_t j = 0; j < n; j++) {
                            q.outcome[p] = HET_SITE; mark[1][p] = 1;
                            if (variant == 1) { /* an insertion right behind the site and one just outside its window, a refused site at the window's end */
                                if (max_repeat >= 2) { q.outcome[p + 1] = HET_INS; mark[1][p + 1] = 1; }
                            }
                            uint32_t step = (uint32_t)max_repeat + ((spacing >> j) & 1u);
                            if (step == 0) step = 1;
                            if (variant == 2 && step > 1) { q.valid[p + 1] = 0; step++; } /* an invalid position stretches the distance in positions, not in valid ones */
                            p += step;
                        }
                        if (variant == 1 || variant == 3) {
                            const uint32_t last = p; /* where a further site would be */
                            for (uint32_t d = 0; d < 3 && last + d < 400; d++) if (!mark[1][last + d]) { q.outcome[last + d] = d == 1 ? HET_FILTERED : HET_INS; mark[1][last + d] = 1; }
                        }
                        if (variant == 3) { seqs[0].outcome[399] = HET_SITE; mark[0][399] = 1; } /* a site at the end of the sequence before arms nothing here */
                        check_chains(seqs, mark, max_repeat, start & 1, "chains");
                    }
    /* 4. random planes, random outcomes */
    for (uint32_t npos = 0; npos <= 600; npos++)
        for (int t = 0; t < 6; t++) {
            const uint32_t nseq = 1 + (uint32_t)(rnd() % 3);
            const int k = (int[]){5, 13, 21, 31}[rnd() % 4], max_repeat = (int)(rnd() % (uint32_t)(k - 1));
            std::vector<Seq> seqs;
            std::vector<std::vector<uint8_t>> mark;
            uint64_t off = rnd() % 3;
            for (uint32_t s = 0; s < nseq; s++) {
                const uint32_t n = s == 0 ? npos : (uint32_t)(rnd() % 601);
                Seq q = make(n);
                q.word_off = off;
                off += n / 64 + 2 + rnd() % 3;
                const uint32_t p_deg = (uint32_t[]){2, 10, 50}[(t + s) % 3], p_invalid = (uint32_t[]){0, 1, 10}[rnd() % 3], p_rep = (uint32_t[]){0, 5, 50}[rnd() % 3];
                std::vector<uint8_t> m(n, 0);
                for (uint32_t i = 0; i < n; i++) {
                    q.valid[i] = rnd() % 100 >= p_invalid; q.in2[i] = rnd() % 100 < p_deg; q.out2[i] = rnd() % 100 < p_deg;
                    q.outcome[i] = (uint8_t)(rnd() % 4);
                    m[i] = rnd() % 100 < (uint32_t[]){3, 30, 90}[t % 3];
                }
                for (uint32_t i = 0; i <= n; i++) q.rep[i] = rnd() % 100 < p_rep;
                seqs.push_back(q);
                mark.push_back(m);
            }
            check_candidates(seqs, k, max_repeat, t & 1, t % 3 != 0, "random planes");
            check_chains(seqs, mark, (int)(rnd() % 8), t & 1, "random outcomes");
            if (t == 0) check_history(seqs[0], k, max_repeat);
        }
    printf("OK %llu cases %llu candidates %llu entries\n", n_cases, n_cand, n_entries);
    return 0;
}
