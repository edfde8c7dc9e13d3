/*
 * TEST-ONLY: the logic of `find` for homozygous deletions (mindthegap_amd/csrc/mtg_find_del.h, shared with k_del_mark / k_del_judge / k_del_emit)
 * compiled by g++ and checked against literal loops over strings.
 *   1. del_fuzzy_site against the nested loop of FindDeletion::fuzzy_site (src/FindDeletion.hpp:179-188, on std::string), for k = 5 .. 32, every
 *      max_repeat 0 .. k - 2 and every planted agreement 0 .. max_repeat + 1 of the suffix of begin with the prefix of end, plus random pairs
 *      over a two-letter alphabet, where several lengths agree at once;
 *   2. del_joined_kmer: for k = 11 .. 31, every r = 0 .. k - 2 and every j = 0 .. k - r, the k-mer against the substring of the literal text
 *      begin.substr(0, k - r) + end, with begin and end read by del_packed_kmer from a packed sequence at every left position 20 .. 75 and gap
 *      lengths that put either k-mer across the 64-bit word seams at nucleotides 32 and 64; k = 32 with j = k;
 *   3. gap_is_del_candidate against the two tests of update() (:64-71) for every flags value, k, max_repeat and length around the threshold, and
 *      del_size_of / del_pos_of against the arithmetic of :90 and :148 with position() = start + L + 1.
 * Prints "OK <sites> sites <kmers> kmers <candidates> candidates".
 */
#include "../../mindthegap_amd/csrc/mtg_find_del.h"
#include <cstdio>
#include <cstdlib>
#include <string>
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

static const char NT[5] = "ACTG"; /* code = (ASCII >> 1) & 3 */
static std::string random_text(size_t n, unsigned letters = 4)
{
    std::string s(n, 'A');
    for (size_t i = 0; i < n; i++) s[i] = NT[rnd() % letters];
    return s;
}
static uint64_t image(const std::string& s) /* nucleotide i in bits 2i, 2i + 1 */
{
    uint64_t x = 0;
    for (size_t i = 0; i < s.size(); i++) x |= (uint64_t)(((unsigned char)s[i] >> 1) & 3u) << (2 * i);
    return x;
}
static std::vector<uint64_t> pack(const std::string& s)
{
    std::vector<uint64_t> w((s.size() + 31) / 32 + 2, 0);
    for (size_t i = 0; i < s.size(); i++) w[i >> 5] |= (uint64_t)(((unsigned char)s[i] >> 1) & 3u) << (2 * (i & 31));
    return w;
}

/* FindDeletion::fuzzy_site as written */
static unsigned literal_fuzzy_site(const std::string& begin, const std::string& end, unsigned max_repeat)
{
    for (unsigned i = max_repeat; i != 0; i--)
        for (unsigned j = 1; begin.substr(begin.length() - i, j) == end.substr(0, j); j++)
            if (i == j) return j;
    return 0;
}

static unsigned long long n_sites = 0, n_kmers = 0, n_cand = 0;
static void fail(const char* what, long a, long b, long c, long d)
{
    printf("FAIL (%s): %ld %ld %ld %ld\n", what, a, b, c, d);
    exit(1);
}

int main()
{
    /* 1. the junction repeat */
    for (int k = 5; k <= 32; k++)
        for (int mr = 0; mr <= k - 2; mr++) {
            for (int agree = 0; agree <= mr + 1 && agree <= k; agree++)
                for (int t = 0; t < 4; t++) {
                    std::string begin = random_text((size_t)k), end = random_text((size_t)k);
                    for (int i = 0; i < agree; i++) end[(size_t)i] = begin[(size_t)(k - agree + i)];
                    const int want = (int)literal_fuzzy_site(begin, end, (unsigned)mr), got = del_fuzzy_site(image(begin), image(end), k, mr);
                    if (got != want) fail("fuzzy_site, planted", k, mr, agree, got);
                    if (agree <= mr && want < agree) fail("fuzzy_site: the planted agreement was not found", k, mr, agree, want);
                    n_sites++;
                }
            for (int t = 0; t < 40; t++) {
                const std::string begin = random_text((size_t)k, 2), end = random_text((size_t)k, 2);
                if (del_fuzzy_site(image(begin), image(end), k, mr) != (int)literal_fuzzy_site(begin, end, (unsigned)mr)) fail("fuzzy_site, two letters", k, mr, t, 0);
                n_sites++;
            }
        }
    /* 2. the k-mers of the joined text, the two k-mers read from packed words */
    for (int k = 11; k <= 31; k++)
        for (uint32_t left = 20; left <= 75; left++)
            for (uint32_t L : {1u, 2u, (uint32_t)k - 5u, (uint32_t)k, 33u, 40u, 64u}) {
                const uint32_t right = left + 1u + L;
                const std::string text = random_text((size_t)right + (size_t)k + (size_t)(rnd() % 3));
                const std::vector<uint64_t> w = pack(text);
                const std::string begin = text.substr(left, (size_t)k), end = text.substr(right, (size_t)k);
                const uint64_t b = del_packed_kmer(w.data(), left, k), e = del_packed_kmer(w.data(), right, k);
                if (b != image(begin) || e != image(end)) fail("packed k-mer", k, left, right, 0);
                for (int r = 0; r <= k - 2; r++) {
                    const std::string joined = begin.substr(0, (size_t)(k - r)) + end;
                    if ((int)joined.size() != 2 * k - r) fail("joined length", k, r, 0, 0);
                    for (int j = 0; j + k <= (int)joined.size(); j++) {
                        if (del_joined_kmer(b, e, r, j, k) != image(joined.substr((size_t)j, (size_t)k))) fail("joined k-mer", k, r, j, left);
                        n_kmers++;
                    }
                }
            }
    { /* k = 32: the shifts by a whole word */
        const std::string begin = random_text(32), end = random_text(32);
        for (int r = 0; r <= 30; r++) {
            const std::string joined = begin.substr(0, (size_t)(32 - r)) + end;
            for (int j = 0; j <= 32 - r; j++, n_kmers++)
                if (del_joined_kmer(image(begin), image(end), r, j, 32) != image(joined.substr((size_t)j, 32))) fail("joined k-mer, k = 32", r, j, 0, 0);
        }
    }
    /* 3. the candidate test, del_size and pos */
    for (int k = 5; k <= 32; k++)
        for (int mr = 0; mr <= k - 2; mr++)
            for (uint32_t flags = 0; flags < 4; flags++)
                for (uint32_t L = 1; L <= (uint32_t)k + 70u; L += (L > (uint32_t)k + 3u ? 13u : 1u)) {
                    const bool both_valid = (flags & 1u) && (flags & 2u); /* kmer_begin valid, the observers are called (kmer_end valid) */
                    const bool want = both_valid && !((int)L < k - mr);
                    if (gap_is_del_candidate(L, flags, k, mr) != want) fail("candidate", k, mr, flags, L);
                    n_cand++;
                    for (int r = 0; r <= mr; r++) {
                        const uint32_t start = 1u + (uint32_t)(rnd() % 1000);
                        const long del_size = (long)L - (long)k + (long)r + 1, position = (long)start + (long)L + 1;
                        if (del_size_of(L, r, k) != del_size) fail("del_size", k, r, L, 0);
                        if (del_size > 0 && (long)del_pos_of(start, r, k) != position - 2 - del_size) fail("pos", k, r, L, start);
                    }
                }
    if (gap_is_del_candidate(0xFFFFFFF0u, 3u, 31, 5) != true) fail("candidate, a very long gap", 0, 0, 0, 0);
    printf("OK %llu sites %llu kmers %llu candidates\n", n_sites, n_kmers, n_cand);
    return 0;
}
