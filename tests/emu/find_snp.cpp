/*
 * TEST-ONLY: the logic of `find` for isolated homozygous SNPs (mindthegap_amd/csrc/mtg_find_snp.h, shared with k_gap_mark / k_snp_judge /
 * k_gap_emit) compiled by g++ and checked against literal loops over strings.
 *   1. the windows: for k = 5 .. 32 and every gap start 0 .. 100 (every alignment against the 32-nucleotide word, the seams at 32, 64 and
 *      96), the k k-mers of the gap read by snp_text_kmer from the at most three words that snp_text_words names, each with every nucleotide
 *      put in by snp_window, against the substrings of the text with position start + k - 1 replaced; the packed array ends with the word
 *      of the text's last nucleotide, so a read behind it is an error under AddressSanitizer;
 *   2. snp_solo_call, the closed form, against snp_at_end as written (src/FindSNP.hpp:139-208: the map, its erasure, limit = k, the best
 *      count) on sets of k-mers at k = 5, 7 and 31 where no, one, two or three alternatives hold all windows and where one lacks exactly
 *      window 0, window k - 1 or a middle one;
 *   3. gap_is_snp_candidate against the two tests of update() (:321-326) for every flags value, k, max_repeat and length around k, and the
 *      record: snp_pos_of against position() - 2 with position() = start + k + 1, snp_ins_of against nuc_to_char for the twelve pairs.
 * Prints "OK <windows> windows <calls> calls <candidates> candidates".
 */
#include "../../mindthegap_amd/csrc/mtg_find_snp.h"
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
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

static const char NT[5] = "ACTG"; /* code = (ASCII >> 1) & 3 */
static std::string random_text(size_t n)
{
    std::string s(n, 'A');
    for (size_t i = 0; i < n; i++) s[i] = NT[rnd() % 4];
    return s;
}
static uint64_t image(const std::string& s) /* nucleotide i in bits 2i, 2i + 1 */
{
    uint64_t x = 0;
    for (size_t i = 0; i < s.size(); i++) x |= (uint64_t)(((unsigned char)s[i] >> 1) & 3u) << (2 * i);
    return x;
}
static std::vector<uint64_t> pack_tight(const std::string& s) /* no word behind the one of the last nucleotide */
{
    std::vector<uint64_t> w((s.size() + 31) / 32, 0);
    for (size_t i = 0; i < s.size(); i++) w[i >> 5] |= (uint64_t)(((unsigned char)s[i] >> 1) & 3u) << (2 * (i & 31));
    return w;
}

/* FindSNP::snp_at_end as written, on the text: history slot `beginpos` is the k-mer at that position.  Returns the called code or -1 */
static int literal_snp_at_end(const std::string& text, size_t beginpos, int k, size_t limit, const std::set<uint64_t>& graph, int* ref_nuc)
{
    std::map<int, unsigned> nuc;
    nuc[0] = 0; nuc[1] = 0; nuc[2] = 0; nuc[3] = 0;
    *ref_nuc = ((unsigned char)text.substr(beginpos, (size_t)k)[(size_t)k - 1] >> 1) & 3;
    nuc.erase(*ref_nuc);
    bool end = false;
    for (int j = 0; !end && j != k; beginpos++, j++)
        for (std::map<int, unsigned>::iterator it = nuc.begin(); it != nuc.end();) {
            std::string kmer = text.substr(beginpos, (size_t)k);
            kmer[(size_t)(k - j) - 1] = NT[it->first]; /* mutate_kmer(kmer, nuc, k - j): position 1-based from the start */
            if (graph.count(image(kmer))) {
                nuc[it->first]++;
                ++it;
            } else {
                if (nuc.size() == 1) {
                    end = true;
                    beginpos -= 1;
                    break;
                }
                nuc.erase(it++);
            }
        }
    int max = nuc.begin()->first;
    for (std::map<int, unsigned>::iterator it = nuc.begin(); it != nuc.end(); it++)
        if (it->second > nuc[max]) max = it->first;
    return nuc[max] >= limit ? max : -1;
}

static unsigned long long n_windows = 0, n_calls = 0, n_cand = 0;
static void fail(const char* what, long a, long b, long c, long d)
{
    printf("FAIL (%s): %ld %ld %ld %ld\n", what, a, b, c, d);
    exit(1);
}

int main()
{
    /* 1. the windows across the word seams */
    for (int k = 5; k <= 32; k++)
        for (uint32_t start = 0; start <= 100; start++) {
            const std::string text = random_text((size_t)start + 2 * (size_t)k - 1);
            const std::vector<uint64_t> w = pack_tight(text);
            const uint32_t g = start + (uint32_t)k - 1u, w0 = start >> 5, nw = snp_text_words(start, k);
            if (nw != ((start + 2u * (uint32_t)k - 2u) >> 5) - w0 + 1u || w0 + nw != w.size()) fail("text words", k, start, nw, (long)w.size());
            const uint64_t t0 = w[w0], t1 = nw > 1u ? w[w0 + 1u] : 0ull, t2 = nw > 2u ? w[w0 + 2u] : 0ull;
            for (int j = 0; j < k; j++) {
                const uint64_t km = snp_text_kmer(t0, t1, t2, (start & 31u) + (uint32_t)j, k);
                if (km != image(text.substr(start + (size_t)j, (size_t)k))) fail("text k-mer", k, start, j, 0);
                for (uint32_t a = 0; a < 4; a++, n_windows++) {
                    std::string changed = text;
                    changed[g] = NT[a];
                    if (snp_window(km, j, k, a) != image(changed.substr(start + (size_t)j, (size_t)k))) fail("window", k, start, j, a);
                }
            }
            uint32_t ref = 9;
            (void)snp_solo_call(w.data(), start, k, [](uint64_t) { return false; }, &ref); /* reads what the rule reads, from the tight array */
            if (ref != (uint32_t)(((unsigned char)text[g] >> 1) & 3u)) fail("ref", k, start, ref, 0);
        }
    /* 2. the closed form against the map */
    unsigned long long by_count[4] = {0, 0, 0, 0}, first_not_lowest = 0, holed = 0;
    for (int k : {5, 7, 31})
        for (int t = 0; t < 6000; t++) {
            const uint32_t start = (uint32_t)(rnd() % 70);
            const std::string text = random_text((size_t)start + 2 * (size_t)k - 1 + (size_t)(rnd() % 3));
            const std::vector<uint64_t> w = pack_tight(text);
            const size_t g = (size_t)start + (size_t)k - 1;
            std::set<uint64_t> graph;
            /* every alternative takes part with probability 1/2 with all its windows; then, half the time, one window of one alternative goes:
             * window 0, window k - 1 or a middle one */
            int full = 0;
            for (int a = 0; a < 4; a++) {
                if (NT[a] == text[g] || (rnd() & 1u)) continue;
                std::string changed = text;
                changed[g] = NT[a];
                for (int j = 0; j < k; j++) graph.insert(image(changed.substr(start + (size_t)j, (size_t)k)));
                full++;
            }
            if (full && (rnd() & 1u)) {
                int a = (int)(rnd() % 4);
                while (NT[a] == text[g]) a = (a + 1) % 4;
                std::string changed = text;
                changed[g] = NT[a];
                const int which = (int)(rnd() % 3), j = which == 0 ? 0 : which == 1 ? k - 1 : 1 + (int)(rnd() % (uint64_t)(k - 2));
                holed += graph.erase(image(changed.substr(start + (size_t)j, (size_t)k)));
            }
            int want_ref = -1;
            const int want = literal_snp_at_end(text, start, k, (size_t)k, graph, &want_ref);
            uint32_t ref = 9;
            const int got = snp_solo_call(w.data(), start, k, [&](uint64_t x) { return graph.count(x) != 0; }, &ref);
            if (got != want || (int)ref != want_ref) fail("closed form", k, t, got, want);
            /* how many alternatives hold all windows, and whether the winner is not the lowest code left (T before G needs no such case) */
            int holds = 0, first = -1;
            for (int a = 0; a < 4; a++) {
                if (NT[a] == text[g]) continue;
                std::string changed = text;
                changed[g] = NT[a];
                bool all = true;
                for (int j = 0; j < k; j++) all = all && graph.count(image(changed.substr(start + (size_t)j, (size_t)k)));
                if (all) { holds++; if (first < 0) first = a; }
            }
            if (first != want) fail("first alternative that holds", k, t, first, want);
            by_count[holds]++;
            if (holds >= 2 && first == 2) first_not_lowest++; /* T and G both hold: T wins */
            n_calls++;
        }
    if (!by_count[0] || !by_count[1] || !by_count[2] || !by_count[3] || !first_not_lowest || holed < 1000) fail("the cases do not cover", (long)by_count[0], (long)by_count[2], (long)by_count[3], (long)holed);
    /* 3. the candidate test and the record */
    for (int k = 5; k <= 32; k++)
        for (int mr = 0; mr <= k - 2; mr++)
            for (uint32_t flags = 0; flags < 4; flags++)
                for (uint32_t L = 1; L <= (uint32_t)k + 40u; L++, n_cand++) {
                    const bool both_valid = (flags & 1u) && (flags & 2u);
                    if (gap_is_snp_candidate(L, flags, k, mr) != (both_valid && L == (uint32_t)k)) fail("candidate", k, mr, flags, L);
                }
    for (int k = 5; k <= 32; k++)
        for (int t = 0; t < 50; t++) {
            const uint32_t start = 1u + (uint32_t)(rnd() % 100000);
            const long position = (long)start + (long)k + 1;
            if ((long)snp_pos_of(start, k) != position - 2) fail("pos", k, start, 0, 0);
        }
    for (uint32_t ref = 0; ref < 4; ref++)
        for (uint32_t i = 0; i < 3; i++) {
            const uint32_t alt = snp_alt(ref, i);
            if (alt == ref || alt > 3u || (i && alt <= snp_alt(ref, i - 1u))) fail("alternatives", ref, i, alt, 0);
            const uint32_t res = SNP_CALLED | (alt << SNP_ALT_SHIFT) | (ref << SNP_REF_SHIFT);
            if (snp_ins_of(res) != ((uint32_t)(unsigned char)NT[alt] | ((uint32_t)(unsigned char)NT[ref] << 8))) fail("ins", ref, alt, snp_ins_of(res), 0);
        }
    printf("OK %llu windows %llu calls %llu candidates\n", n_windows, n_calls, n_cand);
    return 0;
}
