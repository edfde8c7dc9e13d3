/*
 * TEST-ONLY: the gap extraction of `find` (mindthegap_amd/csrc/mtg_find_gaps.h, the word-level logic of k_profile_count<true> /
 * k_profile_write<true>) compiled by g++ and checked against the literal loop of the reference's scan.
 *
 * Two literal loops.  notify() is FindBreakpoints::notify with its members (solid stretch, gap stretch, kmer_begin valid or not) over the
 * positions of a sequence, recording every call of the gap observers: (first position, length, kmer_begin valid).  anchors() is the
 * statement of mtg_find_gaps.h taken position by position: every gap, reported or not, with its two flags.  The word-level extraction must
 * equal anchors() record by record, and its gaps with flag bit 1 must equal notify() -- which also shows the two statements to agree.
 * The words are visited odd ones first, since no word may depend on what another one wrote.
 *   1. every single gap [a, b] with 0 <= a <= b < 200 in a sequence of 270 positions, with two present positions / an invalid one / nothing
 *      on either side, and with one isolated present position or two adjacent ones somewhere inside (every alignment against the 64-bit seams);
 *   2. isolated present bits at the word edges 0, 63, 64, 127, 128 in an otherwise absent sequence, a gap as long as the whole input;
 *   3. 0 and 1 sequences, sequences of 0, 1, 2 positions;
 *   4. random planes of 0 .. 700 positions, several sequences per case at arbitrary word offsets, junk past the last position.
 * Prints "OK <cases> cases <gaps> gaps".
 */
#include "../../mindthegap_amd/csrc/mtg_find_gaps.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace mtg;

static uint64_t rng_state = 0x13198A2E03707344ull;
static uint64_t rnd()
{
    rng_state += 0x9E3779B97F4A7C15ull;
    uint64_t z = rng_state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct Seq {
    std::vector<uint8_t> valid, present; /* per position */
    uint64_t word_off;
};

/* FindBreakpoints::notify (src/FindBreakpoints.hpp:560-622) and the reset on an invalid k-mer (:426-431), per sequence (:393-400) */
static void notify_loop(const std::vector<Seq>& seqs, std::vector<mtg_run>& out)
{
    out.clear();
    for (size_t s = 0; s < seqs.size(); s++) {
        const Seq& q = seqs[s];
        size_t solid_stretch = 0, gap_stretch = 0;
        bool kmer_begin_valid = false;
        for (size_t pos = 0; pos < q.valid.size(); pos++) {
            if (!q.valid[pos]) { solid_stretch = 0; gap_stretch = 0; kmer_begin_valid = false; continue; }
            const bool in_graph = q.present[pos];
            if (in_graph) {
                solid_stretch++;
                if (solid_stretch > 1 && gap_stretch > 0) {
                    mtg_run r;
                    r.seq = (uint32_t)s; r.start = (uint32_t)(pos - 1 - gap_stretch); r.length = (uint32_t)gap_stretch; r.flags = 2u | (kmer_begin_valid ? 1u : 0u);
                    out.push_back(r);
                    gap_stretch = 0;
                }
            } else {
                if (solid_stretch == 1) gap_stretch += solid_stretch;
                if (solid_stretch > 1) kmer_begin_valid = true; /* m_previous_kmer is the k-mer right before: valid, the stretch was not reset */
                gap_stretch++;
                solid_stretch = 0;
            }
        }
    }
}

static void anchors_loop(const std::vector<Seq>& seqs, std::vector<mtg_run>& out)
{
    out.clear();
    for (size_t s = 0; s < seqs.size(); s++) {
        const Seq& q = seqs[s];
        const size_t n = q.valid.size();
        std::vector<uint8_t> pres(n), anchor(n);
        for (size_t i = 0; i < n; i++) pres[i] = q.valid[i] && q.present[i];
        for (size_t i = 0; i < n; i++) anchor[i] = pres[i] && ((i > 0 && pres[i - 1]) || (i + 1 < n && pres[i + 1]));
        size_t p = 0;
        while (p < n) {
            if (!q.valid[p] || anchor[p]) { p++; continue; }
            size_t e = p;
            while (e < n && q.valid[e] && !anchor[e]) e++;
            mtg_run r;
            r.seq = (uint32_t)s; r.start = (uint32_t)p; r.length = (uint32_t)(e - p);
            r.flags = ((p > 0 && anchor[p - 1]) ? 1u : 0u) | ((e < n && anchor[e]) ? 2u : 0u);
            out.push_back(r);
            p = e;
        }
    }
}

/* the device's passes; writes min(total, cap_limit) records */
static uint64_t extract(const std::vector<Seq>& seqs, bool junk, std::vector<mtg_run>& out, uint64_t cap_limit)
{
    size_t nwords = 0;
    for (const Seq& q : seqs) nwords = std::max(nwords, (size_t)q.word_off + q.valid.size() / 64 + 1);
    std::vector<uint64_t> vp(nwords + 1), pp(nwords + 1);
    for (size_t i = 0; i < vp.size(); i++) { vp[i] = junk ? rnd() : 0; pp[i] = junk ? rnd() : 0; }
    for (const Seq& q : seqs) {
        const uint32_t npos = (uint32_t)q.valid.size();
        for (uint32_t w = 0; w < run_words(npos); w++) {
            uint64_t v = 0, p = 0;
            for (uint32_t b = 0; b < 64; b++) {
                const uint32_t i = w * 64 + b;
                if (i < npos) { v |= (uint64_t)(q.valid[i] != 0) << b; p |= (uint64_t)(q.valid[i] && q.present[i]) << b; }
                else if (junk) { v |= (rnd() & 1) << b; p |= (rnd() & 1) << b; }
            }
            vp[q.word_off + w] = v; pp[q.word_off + w] = p;
        }
    }
    std::vector<uint64_t> before(seqs.size());
    uint64_t total = 0;
    for (size_t s = 0; s < seqs.size(); s++) {
        const uint32_t npos = (uint32_t)seqs[s].valid.size();
        before[s] = total;
        for (uint32_t w = 0; w < run_words(npos); w++) total += run_popc(gap_word(vp.data() + seqs[s].word_off, pp.data() + seqs[s].word_off, w, npos).first);
    }
    const uint64_t cap = std::min(total, cap_limit);
    std::vector<mtg_run> all(cap + 1);
    memset(all.data(), 0, all.size() * sizeof(mtg_run));
    all[cap].seq = 0xDEADBEEFu; /* the record at the capacity stays as it is */
    for (int parity = 1; parity >= 0; parity--)
        for (size_t s = 0; s < seqs.size(); s++) {
            const uint32_t npos = (uint32_t)seqs[s].valid.size();
            uint64_t b = before[s];
            for (uint32_t w = 0; w < run_words(npos); w++) {
                const RunWord r = gap_word(vp.data() + seqs[s].word_off, pp.data() + seqs[s].word_off, w, npos);
                if ((int)(w & 1u) == parity) run_emit_word(r, (uint32_t)s, w, b, all.data(), cap);
                b += run_popc(r.first);
            }
        }
    if (all[cap].seq != 0xDEADBEEFu || all[cap].start || all[cap].length || all[cap].flags) { printf("FAIL: a record at the capacity was written\n"); exit(1); }
    for (uint64_t i = 0; i < cap; i++) run_finish(all[i]);
    out.assign(all.begin(), all.begin() + cap);
    return total;
}

static unsigned long long n_cases = 0, n_gaps = 0;
static void check(const std::vector<Seq>& seqs, bool junk, uint64_t cap_limit, const char* what)
{
    std::vector<mtg_run> want, reported, got;
    anchors_loop(seqs, want);
    notify_loop(seqs, reported);
    const uint64_t total = extract(seqs, junk, got, cap_limit);
    bool ok = total == want.size() && got.size() == std::min<uint64_t>(total, cap_limit);
    for (size_t i = 0; ok && i < got.size(); i++) ok = memcmp(&got[i], &want[i], sizeof(mtg_run)) == 0;
    size_t j = 0; /* the reported gaps, in order, are the calls of the gap observers */
    for (size_t i = 0; ok && i < want.size(); i++)
        if (want[i].flags & 2u) { ok = j < reported.size() && memcmp(&want[i], &reported[j], sizeof(mtg_run)) == 0; j++; }
    ok = ok && j == reported.size();
    if (!ok) {
        printf("FAIL (%s): %zu sequences, total %llu, by anchors %zu, by notify() %zu\n", what, seqs.size(), (unsigned long long)total, want.size(), reported.size());
        for (size_t i = 0; i < std::max(got.size(), want.size()) && i < 20; i++) {
            if (i < got.size()) printf("  got  %u %u %u %u", got[i].seq, got[i].start, got[i].length, got[i].flags);
            if (i < want.size()) printf("  want %u %u %u %u", want[i].seq, want[i].start, want[i].length, want[i].flags);
            printf("\n");
        }
        for (size_t i = 0; i < reported.size() && i < 20; i++) printf("  notify %u %u %u %u\n", reported[i].seq, reported[i].start, reported[i].length, reported[i].flags);
        exit(1);
    }
    n_cases++;
    n_gaps += total;
}

static Seq make(uint32_t npos, uint8_t present) { Seq q; q.word_off = 0; q.valid.assign(npos, 1); q.present.assign(npos, present); return q; }

int main()
{
    /* 1. every alignment of one gap */
    for (uint32_t a = 0; a < 200; a++)
        for (uint32_t b = a; b < 200; b++)
            for (int side = 0; side < 3; side++)
                for (int inside = 0; inside < 3; inside++) { /* nothing / one isolated present position / two adjacent ones inside */
                    const uint32_t npos = side == 2 ? b + 1 : 270;
                    if (side == 2 && a != 0) continue;
                    if ((a * 7 + b) % 5 != 0 && inside) continue; /* a fifth of the alignments for the inner variants */
                    std::vector<Seq> seqs(1, make(npos, 1));
                    seqs[0].word_off = 2;
                    for (uint32_t i = a; i <= b; i++) seqs[0].present[i] = 0;
                    if (inside && b - a >= 4) { const uint32_t m = a + 1 + (uint32_t)(rnd() % (b - a - 2)); seqs[0].present[m] = 1; if (inside == 2) seqs[0].present[m + 1] = 1; }
                    if (side == 1) { if (a) seqs[0].valid[a - 1] = 0; if (b + 1 < npos) seqs[0].valid[b + 1] = 0; }
                    check(seqs, (a + b) & 1, ~0ull, "one gap");
                }
    /* 2. isolated present bits at the word edges; a gap as long as the input */
    for (uint32_t npos : {1u, 63u, 64u, 65u, 127u, 128u, 129u, 192u, 300u})
        for (uint32_t mask = 0; mask < 64; mask++) {
            std::vector<Seq> seqs(1, make(npos, 0));
            const uint32_t edges[6] = {0, 63, 64, 127, 128, npos - 1};
            for (int i = 0; i < 6; i++) if (((mask >> i) & 1u) && edges[i] < npos) seqs[0].present[edges[i]] = 1;
            check(seqs, mask & 1, ~0ull, "word edges");
        }
    /* 3. 0 and 1 sequences, tiny ones */
    { std::vector<Seq> none; check(none, false, ~0ull, "no sequence"); }
    for (uint32_t npos = 0; npos <= 3; npos++)
        for (uint32_t bits = 0; bits < (1u << npos); bits++) {
            std::vector<Seq> seqs(1, make(npos, 0));
            for (uint32_t i = 0; i < npos; i++) seqs[0].present[i] = (bits >> i) & 1u;
            check(seqs, true, ~0ull, "tiny");
        }
    /* 4. random planes */
    for (uint32_t npos = 0; npos <= 700; npos++)
        for (int t = 0; t < 8; t++) {
            const uint32_t nseq = 1 + (uint32_t)(rnd() % 4);
            std::vector<Seq> seqs(nseq);
            uint64_t off = rnd() % 3;
            for (uint32_t s = 0; s < nseq; s++) {
                const uint32_t n = s == 0 ? npos : (uint32_t)(rnd() % 701);
                const uint32_t p_present = (uint32_t[]){2, 10, 50, 90, 98, 100}[(t + s) % 6], p_invalid = (uint32_t[]){0, 1, 5, 30}[rnd() % 4];
                seqs[s].word_off = off;
                off += n / 64 + 1 + rnd() % 3;
                seqs[s].valid.resize(n);
                seqs[s].present.resize(n);
                uint32_t i = 0;
                while (i < n) { /* stretches of many lengths, single positions among them: isolated present k-mers are the point */
                    const uint32_t longest = rnd() % 4 == 0 ? 300 : rnd() % 2 ? 3 : 40;
                    const uint32_t stretch = 1 + (uint32_t)(rnd() % longest);
                    const bool pres = rnd() % 100 < p_present;
                    for (uint32_t j = 0; j < stretch && i < n; j++, i++) { seqs[s].present[i] = pres; seqs[s].valid[i] = !(rnd() % 100 < p_invalid && rnd() % 4 == 0); }
                }
            }
            std::vector<mtg_run> want;
            anchors_loop(seqs, want);
            const uint64_t caps[4] = {~0ull, 0, 1, want.size() ? want.size() - 1 : 0};
            check(seqs, t & 1, caps[t % 4], "random planes");
        }
    printf("OK %llu cases %llu gaps\n", n_cases, n_gaps);
    return 0;
}
