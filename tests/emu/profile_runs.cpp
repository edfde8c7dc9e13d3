/*
 * TEST-ONLY: the run extraction of the sequence profile (mindthegap_amd/csrc/mtg_profile_runs.h, the word-level logic of k_profile_count /
 * k_profile_write / k_profile_finish) compiled by g++ and checked against a literal loop over positions.
 *
 * The device numbers the runs by counted passes: runs that begin in each sequence, an exclusive prefix sum over the sequences, then every
 * word on its own numbers the runs that begin and end in it.  Here the words are visited one after the other with the same counts, in an
 * order that is NOT ascending (odd words first), since no word may depend on what another one wrote.
 *   1. every single run [a, b] with 0 <= a <= b < 330 in a sequence of 400 positions -- every alignment of a run's first and last position
 *      against the seams of the 64-bit words and of the 256-position tiles -- with a present, an invalid or no position on either side;
 *   2. random planes of 0 .. 1100 positions, several sequences per case at arbitrary word offsets, densities from "almost all present" to
 *      "almost all absent", invalid positions sprinkled in, junk in the bits past the last position, capacities below the number of runs.
 *   3. covers_bad (the bad-bit test of k_profile, k_find_assemble and k_het_judge) against a loop over the k bits: every k in 11 .. 32 from
 *      every p in 0 .. 130, on planes that are random, all zero, and zero but for one bit at p - 1, p, p + k - 1 or p + k, in an array that
 *      ends with the last word the function may read (under AddressSanitizer a read behind it is an error).
 * Prints "OK <cases> cases <runs> runs <windows> windows".
 */
#include "../../mindthegap_amd/csrc/mtg_profile_runs.h"
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
    std::vector<uint8_t> valid, present; /* per position */
    uint64_t word_off;
};

/* the expected runs: the literal loop */
static void literal(const std::vector<Seq>& seqs, std::vector<mtg_run>& out)
{
    out.clear();
    for (size_t s = 0; s < seqs.size(); s++) {
        const Seq& q = seqs[s];
        const size_t n = q.valid.size();
        size_t p = 0;
        while (p < n) {
            if (!(q.valid[p] && !q.present[p])) { p++; continue; }
            size_t e = p;
            while (e < n && q.valid[e] && !q.present[e]) e++;
            mtg_run r;
            r.seq = (uint32_t)s; r.start = (uint32_t)p; r.length = (uint32_t)(e - p);
            r.flags = ((p > 0 && q.valid[p - 1] && q.present[p - 1]) ? 1u : 0u) | ((e < n && q.valid[e] && q.present[e]) ? 2u : 0u);
            out.push_back(r);
            p = e;
        }
    }
}

/* the device's passes.  Returns the total; writes min(total, cap) records and the longest run */
static uint64_t extract(const std::vector<Seq>& seqs, bool junk, std::vector<mtg_run>& out, uint64_t cap_limit, uint32_t& longest)
{
    size_t nwords = 0;
    for (const Seq& q : seqs) nwords = std::max(nwords, (size_t)q.word_off + q.valid.size() / 64 + 1);
    std::vector<uint64_t> vp(nwords + 1), pp(nwords + 1);
    for (size_t i = 0; i < vp.size(); i++) { vp[i] = junk ? rnd() : 0; pp[i] = junk ? rnd() : 0; } /* whatever lies outside a sequence's positions is not read as one */
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
    /* pass 1: runs that begin in each sequence; exclusive prefix sums */
    std::vector<uint64_t> before(seqs.size());
    uint64_t total = 0;
    for (size_t s = 0; s < seqs.size(); s++) {
        const uint32_t npos = (uint32_t)seqs[s].valid.size();
        before[s] = total;
        for (uint32_t w = 0; w < run_words(npos); w++) total += run_popc(run_word(vp.data() + seqs[s].word_off, pp.data() + seqs[s].word_off, w, npos).first);
    }
    /* pass 2: every word writes its halves; odd words first */
    const uint64_t cap = std::min(total, cap_limit);
    std::vector<mtg_run> all(total + 1);
    memset(all.data(), 0, all.size() * sizeof(mtg_run));
    all[total].seq = 0xDEADBEEFu; /* the record behind the last one stays as it is */
    for (int parity = 1; parity >= 0; parity--)
        for (size_t s = 0; s < seqs.size(); s++) {
            const uint32_t npos = (uint32_t)seqs[s].valid.size();
            uint64_t b = before[s];
            for (uint32_t w = 0; w < run_words(npos); w++) {
                const RunWord r = run_word(vp.data() + seqs[s].word_off, pp.data() + seqs[s].word_off, w, npos);
                if ((int)(w & 1u) == parity) run_emit_word(r, (uint32_t)s, w, b, all.data(), total);
                b += run_popc(r.first);
            }
        }
    if (all[total].seq != 0xDEADBEEFu || all[total].start || all[total].length || all[total].flags) { printf("FAIL: a record past the total was written\n"); exit(1); }
    longest = 0;
    for (uint64_t i = 0; i < total; i++) { const uint32_t l = run_finish(all[i]); longest = l > longest ? l : longest; }
    /* the device writes every run (the longest may lie past the caller's capacity) and hands the leading ones over; the capacity of
     * run_emit_word itself is exercised too: nothing at or past it may be touched */
    if (cap < total) {
        std::vector<mtg_run> part(total);
        memset(part.data(), 0, part.size() * sizeof(mtg_run));
        for (size_t s = 0; s < seqs.size(); s++) {
            const uint32_t npos = (uint32_t)seqs[s].valid.size();
            uint64_t b = before[s];
            for (uint32_t w = 0; w < run_words(npos); w++) {
                const RunWord r = run_word(vp.data() + seqs[s].word_off, pp.data() + seqs[s].word_off, w, npos);
                run_emit_word(r, (uint32_t)s, w, b, part.data(), cap);
                b += run_popc(r.first);
            }
        }
        for (uint64_t i = cap; i < total; i++)
            if (part[i].seq || part[i].start || part[i].length || part[i].flags) { printf("FAIL: record %llu at or past the capacity %llu was written\n", (unsigned long long)i, (unsigned long long)cap); exit(1); }
        for (uint64_t i = 0; i < cap; i++) {
            /* a run that begins below the capacity is complete: its end is numbered like its beginning */
            run_finish(part[i]);
            if (memcmp(&part[i], &all[i], sizeof(mtg_run))) { printf("FAIL: record %llu differs under capacity %llu\n", (unsigned long long)i, (unsigned long long)cap); exit(1); }
        }
    }
    out.assign(all.begin(), all.begin() + cap);
    return total;
}

static unsigned long long n_cases = 0, n_runs = 0;
static void check(const std::vector<Seq>& seqs, bool junk, uint64_t cap_limit, const char* what)
{
    std::vector<mtg_run> want, got;
    literal(seqs, want);
    uint32_t longest = 0, want_longest = 0;
    const uint64_t total = extract(seqs, junk, got, cap_limit, longest);
    for (const mtg_run& r : want) want_longest = r.length > want_longest ? r.length : want_longest;
    bool ok = total == want.size() && got.size() == std::min<uint64_t>(total, cap_limit) && longest == want_longest;
    for (size_t i = 0; ok && i < got.size(); i++) ok = memcmp(&got[i], &want[i], sizeof(mtg_run)) == 0;
    if (!ok) {
        printf("FAIL (%s): %zu sequences, total %llu (expected %zu), longest %u (expected %u)\n", what, seqs.size(), (unsigned long long)total, want.size(), longest, want_longest);
        for (size_t i = 0; i < std::max(got.size(), want.size()) && i < 20; i++) {
            if (i < got.size()) printf("  got  %u %u %u %u", got[i].seq, got[i].start, got[i].length, got[i].flags);
            if (i < want.size()) printf("  want %u %u %u %u", want[i].seq, want[i].start, want[i].length, want[i].flags);
            printf("\n");
        }
        exit(1);
    }
    n_cases++;
    n_runs += total;
}

/* 3. one window of k bits from p.  The plane is a heap array of exactly the words the window touches */
static unsigned long long n_windows = 0;
static void check_covers_bad(const std::vector<uint64_t>& plane, uint32_t p, int k, const char* what)
{
    bool want = false;
    for (uint32_t i = p; i < p + (uint32_t)k; i++) want = want || ((plane[i >> 6] >> (i & 63u)) & 1ull);
    if (covers_bad(plane.data(), p, k) != want) { printf("FAIL (covers_bad, %s): k %d p %u expected %d\n", what, k, p, (int)want); exit(1); }
    n_windows++;
}
static void covers_bad_cases()
{
    for (int k = 11; k <= 32; k++)
        for (uint32_t p = 0; p <= 130; p++) {
            const size_t nw = (size_t)((p + (uint32_t)k - 1u) >> 6) + 1; /* the word of the window's last bit is the last one */
            std::vector<uint64_t> plane(nw);
            for (int t = 0; t < 4; t++) {
                for (uint64_t& x : plane) x = t < 2 ? rnd() : rnd() & rnd() & rnd() & rnd() & rnd(); /* dense, and sparse enough for clean windows */
                check_covers_bad(plane, p, k, "random");
            }
            plane.assign(nw, 0ull);
            check_covers_bad(plane, p, k, "all zero");
            const int64_t at[4] = {(int64_t)p - 1, (int64_t)p, (int64_t)p + k - 1, (int64_t)p + k};
            for (int64_t b : at) {
                if (b < 0 || (size_t)(b >> 6) >= nw) continue; /* that bit lies outside the array */
                plane.assign(nw, 0ull);
                plane[(size_t)(b >> 6)] = 1ull << (b & 63);
                check_covers_bad(plane, p, k, "one bit");
            }
        }
}

int main()
{
    /* 1. every alignment of one run */
    for (uint32_t a = 0; a < 330; a++)
        for (uint32_t b = a; b < 330; b++)
            for (int side = 0; side < 3; side++) { /* around the run: present / invalid / (for a = 0) nothing */
                const uint32_t npos = side == 2 ? b + 1 : 400;
                if (side == 2 && a != 0) continue;
                std::vector<Seq> seqs(1);
                seqs[0].word_off = 3;
                seqs[0].valid.assign(npos, 1);
                seqs[0].present.assign(npos, 1);
                for (uint32_t i = a; i <= b; i++) seqs[0].present[i] = 0;
                if (side == 1) { if (a) seqs[0].valid[a - 1] = 0; if (b + 1 < npos) seqs[0].valid[b + 1] = 0; }
                check(seqs, (a + b) & 1, ~0ull, "one run");
            }
    /* 2. random planes */
    for (uint32_t npos = 0; npos <= 1100; npos++)
        for (int t = 0; t < 6; t++) {
            const uint32_t nseq = 1 + (uint32_t)(rnd() % 4);
            std::vector<Seq> seqs(nseq);
            uint64_t off = rnd() % 3;
            for (uint32_t s = 0; s < nseq; s++) {
                const uint32_t n = s == 0 ? npos : (uint32_t)(rnd() % 1101);
                const uint32_t p_present = (uint32_t[]){2, 10, 50, 90, 98, 100}[(t + s) % 6], p_invalid = (uint32_t[]){0, 1, 5, 30}[rnd() % 4];
                seqs[s].word_off = off;
                off += n / 64 + 1 + rnd() % 3; /* sometimes the next sequence's words follow at once */
                seqs[s].valid.resize(n);
                seqs[s].present.resize(n);
                /* stretches, not single positions: runs of many lengths */
                uint32_t i = 0;
                while (i < n) {
                    const uint32_t longest = rnd() % 4 == 0 ? 700 : 40;
                    const uint32_t stretch = 1 + (uint32_t)(rnd() % longest);
                    const bool pres = rnd() % 100 < p_present;
                    for (uint32_t j = 0; j < stretch && i < n; j++, i++) { seqs[s].present[i] = pres; seqs[s].valid[i] = !(rnd() % 100 < p_invalid && rnd() % 4 == 0); }
                }
            }
            std::vector<mtg_run> want;
            literal(seqs, want);
            const uint64_t caps[4] = {~0ull, 0, 1, want.size() ? want.size() - 1 : 0};
            check(seqs, t & 1, caps[t % 4], "random planes");
        }
    covers_bad_cases();
    printf("OK %llu cases %llu runs %llu windows\n", n_cases, n_runs, n_windows);
    return 0;
}
