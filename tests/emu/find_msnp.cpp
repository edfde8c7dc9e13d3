/*
 * TEST-ONLY: the logic of `find` for close homozygous SNPs (mindthegap_amd/csrc/mtg_find_msnp.h, shared with k_gap_mark / k_msnp_bound /
 * k_msnp_judge / k_msnp_emit) compiled by g++ and checked against literal loops over strings.
 *   1. the chain: msnp_chain on the packed, private words of a gap against FindMultiSNP::update as written (src/FindSNP.hpp:459-545) with
 *      snp_at_end as written (:139-208: the map, its erasure, limit = snp_min_val, the best count and nb_kmer_val) and correct_history as a
 *      substitution in a string.  The string is long enough for every window the literal loop reads; the packed array ends with the word of
 *      nucleotide start + L + k - 1, the last one the rule may read, so a read behind it is an error under AddressSanitizer.  Cases: k = 5,
 *      7, 9 with a graph that holds a k-mer by a hash (dense: alternatives compete by chance), k = 31 and 32 with the k-mers of a donor that
 *      carries substitutions 1 .. k + 1 apart; snp_min_val 1, 2, 3, 5; every alignment of the start against the 32-nucleotide word; gap
 *      lengths k + m + 1 .. 254;
 *   2. gap_is_msnp_candidate against the tests of update() (:461-467), msnp_is_judged / msnp_max_calls / msnp_text_words at their limits,
 *      msnp_winner against the map's outcome for every triple of counts at k = 5, and the record (msnp_pos_of, snp_ins_of on an entry).
 * Prints "OK <gaps> gaps <calls> calls <several> several <partial> partial <full> full <ties> ties".
 */
#include "../../mindthegap_amd/csrc/mtg_find_msnp.h"
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
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
static uint64_t mix(uint64_t x)
{
    x = (x ^ (x >> 33)) * 0xFF51AFD7ED558CCDull;
    x = (x ^ (x >> 33)) * 0xC4CEB9FE1A85EC53ull;
    return x ^ (x >> 33);
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

struct Graph {
    bool hashed;
    uint64_t seed;
    unsigned percent;
    std::set<uint64_t> set;
    bool has(uint64_t x) const { return hashed ? mix(x ^ seed) % 100 < percent : set.count(x) != 0; }
};

static unsigned long long n_ties = 0;
/* FindSNP::snp_at_end as written, on the text: history slot `beginpos` is the k-mer at that position.  Returns the called code or -1 */
static int literal_snp_at_end(const std::string& text, size_t* beginpos, int k, size_t limit, const Graph& graph, int* ref_nuc, unsigned* nb_kmer_val)
{
    std::map<int, unsigned> nuc;
    nuc[0] = 0; nuc[1] = 0; nuc[2] = 0; nuc[3] = 0;
    const size_t beginpos_init = *beginpos;
    *ref_nuc = ((unsigned char)text.substr(*beginpos, (size_t)k)[(size_t)k - 1] >> 1) & 3;
    nuc.erase(*ref_nuc);
    bool end = false;
    unsigned last_erased = ~0u;
    for (int j = 0; !end && j != k; (*beginpos)++, j++)
        for (std::map<int, unsigned>::iterator it = nuc.begin(); it != nuc.end();) {
            std::string kmer = text.substr(*beginpos, (size_t)k);
            kmer[(size_t)(k - j) - 1] = NT[it->first]; /* mutate_kmer(kmer, nuc, k - j): position 1-based from the start */
            if (graph.has(image(kmer))) {
                nuc[it->first]++;
                ++it;
            } else {
                if (nuc.size() == 1) {
                    end = true;
                    *beginpos -= 1;
                    break;
                }
                last_erased = it->second;
                nuc.erase(it++);
            }
        }
    int max = nuc.begin()->first;
    for (std::map<int, unsigned>::iterator it = nuc.begin(); it != nuc.end(); it++)
        if (it->second > nuc[max]) max = it->first;
    if (nuc[max] >= limit) {
        if (end && last_erased == nuc[max]) n_ties++;
        *nb_kmer_val = nuc[max];
        return max;
    }
    *beginpos = beginpos_init;
    return -1;
}

struct Snp { uint32_t pos, ref, alt; };
/* FindMultiSNP::update as written, for a gap that passed its first tests: positions in place of ring indices.  Returns nb_kmer_correct */
static uint32_t literal_update(std::string text, uint32_t start, uint32_t L, int k, int m, const Graph& graph, std::vector<Snp>& out)
{
    size_t begin_pos = (size_t)start + (size_t)k - 1;
    const size_t begin_pos_init = begin_pos;
    size_t index_pos = start;
    const size_t index_end = (size_t)start + L;
    while (index_pos != index_end) {
        const size_t save_index = index_pos;
        unsigned nb_kmer_val = 0;
        int ref_nuc = -1;
        const int nuc = literal_snp_at_end(text, &index_pos, k, (size_t)m, graph, &ref_nuc, &nb_kmer_val);
        if (nuc < 0) break;
        if (begin_pos + nb_kmer_val - begin_pos_init > L) break;
        text[save_index + (size_t)k - 1] = NT[nuc]; /* correct_history: the k k-mers from save_index on, nucleotide k - i of the i-th */
        out.push_back(Snp{(uint32_t)begin_pos, (uint32_t)ref_nuc, (uint32_t)nuc});
        begin_pos += nb_kmer_val;
    }
    return (uint32_t)(begin_pos - begin_pos_init);
}

static void fail(const char* what, long a, long b, long c, long d)
{
    printf("FAIL (%s): %ld %ld %ld %ld\n", what, a, b, c, d);
    exit(1);
}

int main()
{
    unsigned long long n_gaps = 0, n_calls = 0, n_several = 0, n_partial = 0, n_full = 0, n_ten_words = 0;
    /* 1. the chain */
    for (int k : {5, 7, 9, 31, 32})
        for (int t = 0; t < (k < 31 ? 4000 : 600); t++) {
            static const int MIN_VALS[4] = {1, 2, 3, 5};
            const int m = MIN_VALS[rnd() % 4];
            const uint32_t start = t < 64 ? (uint32_t)t : (uint32_t)(rnd() % 200);
            const uint32_t lo = (uint32_t)(k + m + 1);
            const uint32_t L = t % 7 == 0 ? MSNP_MAX_GAP - (uint32_t)(rnd() % 3) : lo + (uint32_t)(rnd() % (t % 3 ? 40 : MSNP_MAX_GAP - lo + 1));
            const std::string text = random_text((size_t)start + L + 3 * (size_t)k + 2); /* the literal loop reads up to 2k - 2 behind start + L */
            Graph graph;
            graph.hashed = k < 31;
            graph.seed = rnd();
            graph.percent = 35 + (unsigned)(rnd() % 50);
            if (!graph.hashed) {
                /* a donor with substitutions 1 .. k + 1 apart from g = start + k - 1 on, sometimes a second donor that competes at the same places,
                 * sometimes k-mers taken out again */
                for (int donor = 0; donor < 2; donor++) {
                    std::string d = text;
                    size_t p = (size_t)start + (size_t)k - 1;
                    while (p < (size_t)start + L) {
                        d[p] = NT[((((unsigned char)text[p] >> 1) & 3u) + 1u + (unsigned)donor + (unsigned)(rnd() % 2)) % 4];
                        p += 1 + (size_t)(rnd() % (uint64_t)(k + 1));
                    }
                    for (size_t q = start; q + (size_t)k <= d.size(); q++)
                        if (donor == 0 || rnd() % 3) graph.set.insert(image(d.substr(q, (size_t)k)));
                    if (rnd() & 1u) break;
                }
                if (rnd() % 3 == 0)
                    for (int h = 0; h < 3 && !graph.set.empty(); h++) {
                        std::set<uint64_t>::iterator it = graph.set.begin();
                        std::advance(it, (long)(rnd() % graph.set.size()));
                        graph.set.erase(it);
                    }
            }
            std::vector<Snp> want;
            const uint32_t want_consumed = literal_update(text, start, L, k, m, graph, want);
            /* the header, on the tight private words of the gap */
            const std::vector<uint64_t> w = pack_tight(text.substr(0, (size_t)start + L + (size_t)k));
            const uint32_t w0 = start >> 5, nw = msnp_text_words(start, L, k);
            if (w0 + nw != w.size() || nw > MSNP_TEXT_WORDS) fail("text words", k, start, L, nw);
            n_ten_words += nw == MSNP_TEXT_WORDS;
            std::vector<uint64_t> priv(w.begin() + w0, w.end());
            std::vector<uint32_t> entries(msnp_max_calls(L, m) + 1u, 0xDEADBEEFu);
            uint32_t n = 0;
            const uint32_t consumed = msnp_chain(priv.data(), start & 31u, L, k, m, [&](uint64_t x) { return graph.has(x); }, entries.data(), &n);
            if (consumed != want_consumed || n != want.size()) fail("chain", k, t, consumed, want_consumed);
            if (n > msnp_max_calls(L, m) || entries[msnp_max_calls(L, m)] != 0xDEADBEEFu) fail("room", k, t, n, msnp_max_calls(L, m));
            for (uint32_t i = 0; i < n; i++) {
                const uint32_t e = entries[i];
                if (!(e & MSNP_ENTRY) || msnp_pos_of(start, e, k) != want[i].pos || ((e >> SNP_ALT_SHIFT) & 3u) != want[i].alt || ((e >> SNP_REF_SHIFT) & 3u) != want[i].ref)
                    fail("entry", k, t, i, e);
                if (snp_ins_of(e) != ((uint32_t)(unsigned char)NT[want[i].alt] | ((uint32_t)(unsigned char)NT[want[i].ref] << 8))) fail("ins", k, t, i, e);
            }
            /* the private words carry the substitutions and nothing else */
            std::string corrected = text.substr(0, (size_t)start + L + (size_t)k);
            for (const Snp& s : want) corrected[s.pos] = NT[s.alt];
            const std::vector<uint64_t> cw = pack_tight(corrected);
            for (uint32_t i = 0; i < nw; i++)
                if (priv[i] != cw[w0 + i]) fail("corrected text", k, t, i, 0);
            n_gaps++;
            n_calls += n;
            n_several += n > 1;
            n_partial += consumed && consumed != L;
            n_full += consumed == L;
        }
    if (n_several < 1000 || n_partial < 1000 || n_full < 200 || n_ties < 200 || n_ten_words < 20)
        fail("the cases do not cover", (long)n_several, (long)n_partial, (long)n_full, (long)n_ties);
    /* 2. the candidate test, the limits, the winner, the record */
    for (int k = 5; k <= 32; k++)
        for (int m = 1; m <= k; m++)
            for (uint32_t flags = 0; flags < 4; flags++)
                for (uint32_t L = 1; L <= 300u; L++) {
                    const bool both_valid = (flags & 1u) && (flags & 2u);
                    if (gap_is_msnp_candidate(L, flags, k, m) != (both_valid && L > (uint32_t)(k + m))) fail("candidate", k, m, flags, L);
                    if (msnp_is_judged(L) != (L <= 254u) || msnp_max_calls(L, m) != (L <= 254u ? L / (uint32_t)m : 0u)) fail("judged", k, m, flags, L);
                }
    if (msnp_text_words(31, 254, 32) != 10u || msnp_text_words(0, 254, 32) != 9u || msnp_text_words(0, 7, 5) != 1u) fail("text words at the limits", 0, 0, 0, 0);
    for (uint32_t f0 = 0; f0 <= 5; f0++)
        for (uint32_t f1 = 0; f1 <= 5; f1++)
            for (uint32_t f2 = 0; f2 <= 5; f2++) {
                /* the map: an alternative leaves at round f (its first missing window) unless it is the only one left; the rounds go in order */
                const uint32_t f[3] = {f0, f1, f2};
                bool in[3] = {true, true, true};
                int left = 3;
                for (uint32_t round = 0; round < 5 && left > 0; round++)
                    for (int i = 0; i < 3; i++)
                        if (in[i] && f[i] == round) {
                            if (left == 1) { round = 5; break; }
                            in[i] = false;
                            left--;
                        }
                int first = -1;
                for (int i = 2; i >= 0; i--) if (in[i]) first = i; /* every survivor has the same count: the first wins */
                uint32_t best = 99;
                const uint32_t got = msnp_winner(f0, f1, f2, 5, &best);
                if ((int)got != first || best != f[first]) fail("winner", f0, f1, f2, got);
            }
    printf("OK %llu gaps %llu calls %llu several %llu partial %llu full %llu ties\n", n_gaps, n_calls, n_several, n_partial, n_full, n_ties);
    return 0;
}
