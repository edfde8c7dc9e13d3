/*
 * TEST-ONLY: the reverse pass of `find` for close homozygous SNPs (mindthegap_amd/csrc/mtg_find_msnp.h: msnp_rev_chain, msnp_passes_chain,
 * shared with k_msnp_rev_judge / k_msnp_rev_emit) compiled by g++ and checked against literal loops over strings.
 *   1. the chains: msnp_passes_chain with passes 1, 2 and 3 on the packed, private words of a gap against FindMultiSNP::update (forward, as in
 *      find_msnp.cpp) followed by FindMultiSNPrev::update as written (src/FindSNP.hpp:593-689) with snp_at_begin as written (:219-293: the
 *      map, its erasure, limit = snp_min_val, the best count and nb_kmer_val) and correct_history as a substitution in a string, with the
 *      entry test on the shrunken gap in between.  The packed array BEGINS with the word of nucleotide start - 1 and ENDS with the word of
 *      nucleotide start + L + k - 1: a read on either side is an error under AddressSanitizer.  Cases as in find_msnp.cpp: k = 5, 7, 9 on a
 *      hashed graph, k = 31 and 32 on the k-mers of donors; snp_min_val 1, 2, 3, 5; every alignment of the start (from 1 on: the left k-mer is
 *      an anchor); gap lengths k + m + 1 .. 254;
 *   2. passes = 1 gives what msnp_chain gives on the forward text; the entry form (direction, offset, non-zero), the position of a reverse
 *      entry, msnp_rev_text_words / msnp_rev_rel0 at their limits, msnp_rev_is_asked, msnp_passes_valid.
 * Prints "OK <gaps> gaps <fwd> forward <rev> reverse <anchor> anchor <whole> whole <after> after <meet> meet <ten> ten".
 */
#include "../../mindthegap_amd/csrc/mtg_find_msnp.h"
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

/* FindSNP::snp_at_end / snp_at_begin as written, on the text: history slot `beginpos` is the k-mer at that position; dir = +1 / -1.
 * Returns the called code or -1 */
static int literal_snp_at(int dir, const std::string& text, long* beginpos, int k, size_t limit, const Graph& graph, int* ref_nuc, unsigned* nb_kmer_val)
{
    std::map<int, unsigned> nuc;
    nuc[0] = 0; nuc[1] = 0; nuc[2] = 0; nuc[3] = 0;
    const long beginpos_init = *beginpos;
    const std::string first = text.substr((size_t)*beginpos, (size_t)k);
    *ref_nuc = ((unsigned char)(dir > 0 ? first[(size_t)k - 1] : first[0]) >> 1) & 3; /* at begin: kmer >> 2(k - 1) & 3 on a gatb k-mer, its first nucleotide */
    nuc.erase(*ref_nuc);
    bool end = false;
    for (int j = 0; !end && j != k; (*beginpos) += dir, j++)
        for (std::map<int, unsigned>::iterator it = nuc.begin(); it != nuc.end();) {
            /* slots before the text's first k-mer are never reached where the anchor window decides; the literal loop goes on to j < k and
             * may read them: an absent k-mer there is as good as any other, what lies behind the cap decides nothing */
            bool in = false;
            if (*beginpos >= 0 && (size_t)*beginpos + (size_t)k <= text.size()) {
                std::string kmer = text.substr((size_t)*beginpos, (size_t)k);
                kmer[dir > 0 ? (size_t)(k - j) - 1 : (size_t)j] = NT[it->first]; /* mutate_kmer(kmer, nuc, k - j) / (kmer, nuc, j + 1): 1-based from the start */
                in = graph.has(image(kmer));
            }
            if (in) {
                nuc[it->first]++;
                ++it;
            } else {
                if (nuc.size() == 1) {
                    end = true;
                    *beginpos -= dir;
                    break;
                }
                nuc.erase(it++);
            }
        }
    int max = nuc.begin()->first;
    for (std::map<int, unsigned>::iterator it = nuc.begin(); it != nuc.end(); it++)
        if (it->second > nuc[max]) max = it->first;
    if (nuc[max] >= limit) {
        *nb_kmer_val = nuc[max];
        return max;
    }
    *beginpos = beginpos_init;
    return -1;
}

struct Snp { uint32_t pos, ref, alt; bool rev; };
/* FindMultiSNP::update as written on `text` (changed), for a gap that passed its first tests.  Returns nb_kmer_correct */
static uint32_t literal_forward(std::string& text, uint32_t start, uint32_t L, int k, int m, const Graph& graph, std::vector<Snp>& out)
{
    size_t begin_pos = (size_t)start + (size_t)k - 1;
    const size_t begin_pos_init = begin_pos;
    long index_pos = (long)start;
    const long index_end = (long)start + (long)L;
    while (index_pos != index_end) {
        const long save_index = index_pos;
        unsigned nb_kmer_val = 0;
        int ref_nuc = -1;
        const int nuc = literal_snp_at(+1, text, &index_pos, k, (size_t)m, graph, &ref_nuc, &nb_kmer_val);
        if (nuc < 0) break;
        if (begin_pos + nb_kmer_val - begin_pos_init > L) break;
        text[(size_t)save_index + (size_t)k - 1] = NT[nuc];
        out.push_back(Snp{(uint32_t)begin_pos, (uint32_t)ref_nuc, (uint32_t)nuc, false});
        begin_pos += nb_kmer_val;
    }
    return (uint32_t)(begin_pos - begin_pos_init);
}
static unsigned long long n_anchor = 0;
/* FindMultiSNPrev::update as written on `text` (changed), on the gap of `left` positions that ends at position start + L - 1 */
static uint32_t literal_reverse(std::string& text, uint32_t start, uint32_t L, uint32_t gap_stretch, int k, int m, const Graph& graph, std::vector<Snp>& out)
{
    long begin_pos = (long)start + (long)L - 1; /* position() - 2 */
    const long begin_pos_init = begin_pos;
    const long index_limit = begin_pos - (long)gap_stretch;
    long index_pos = begin_pos;
    while (index_pos != index_limit) {
        const long save_index = index_pos;
        unsigned nb_kmer_val = 0;
        int ref_nuc = -1;
        const int nuc = literal_snp_at(-1, text, &index_pos, k, (size_t)m, graph, &ref_nuc, &nb_kmer_val);
        if (nuc < 0) break;
        if (begin_pos_init - (begin_pos - (long)nb_kmer_val) > (long)gap_stretch) { n_anchor++; break; }
        text[(size_t)save_index] = NT[nuc]; /* correct_history(save_index - (k - 1), nuc): nucleotide k - i of the i-th k-mer from there */
        out.push_back(Snp{(uint32_t)begin_pos, (uint32_t)ref_nuc, (uint32_t)nuc, true});
        begin_pos -= (long)nb_kmer_val;
    }
    return (uint32_t)(begin_pos_init - begin_pos);
}

static void fail(const char* what, long a, long b, long c, long d)
{
    printf("FAIL (%s): %ld %ld %ld %ld\n", what, a, b, c, d);
    exit(1);
}

int main()
{
    unsigned long long n_gaps = 0, n_fwd_calls = 0, n_rev_calls = 0, n_whole = 0, n_after = 0, n_meet = 0, n_ten_words = 0, n_first_word_alone = 0;
    for (int k : {5, 7, 9, 31, 32})
        for (int t = 0; t < (k < 31 ? 3000 : 600); t++) {
            static const int MIN_VALS[4] = {1, 2, 3, 5};
            const int m = MIN_VALS[rnd() % 4];
            const uint32_t start = t < 64 ? (uint32_t)t + 1u : 1u + (uint32_t)(rnd() % 200);
            const uint32_t lo = (uint32_t)(k + m + 1);
            const uint32_t L = t % 7 == 0 ? MSNP_MAX_GAP - (uint32_t)(rnd() % 3) : lo + (uint32_t)(rnd() % (t % 3 ? 40 : MSNP_MAX_GAP - lo + 1));
            const std::string text = random_text((size_t)start + L + 3 * (size_t)k + 2);
            Graph graph;
            graph.hashed = k < 31;
            graph.seed = rnd();
            graph.percent = 35 + (unsigned)(rnd() % 50);
            if (!graph.hashed) {
                /* donors with substitutions 1 .. k + 1 apart across the gap, now and then k + 2 .. k + 6 apart, so that a chain ends in part
                 * and the other pass has the rest; sometimes a second donor, sometimes k-mers taken out again */
                for (int donor = 0; donor < 2; donor++) {
                    std::string d = text;
                    size_t p = (size_t)start + (size_t)k - 1 + (rnd() % 3 ? 0 : (size_t)(rnd() % 4));
                    while (p < (size_t)start + L) {
                        d[p] = NT[((((unsigned char)text[p] >> 1) & 3u) + 1u + (unsigned)donor + (unsigned)(rnd() % 2)) % 4];
                        p += rnd() % 6 ? 1 + (size_t)(rnd() % (uint64_t)(k + 1)) : (size_t)k + 2 + (size_t)(rnd() % 5);
                    }
                    for (size_t q = start - 1; q + (size_t)k <= d.size(); q++)
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
            /* the packed words of [start - 1, start + L + k) and nothing on either side */
            const uint32_t w0 = (start - 1u) >> 5, nw = msnp_rev_text_words(start, L, k), rel0 = msnp_rev_rel0(start);
            const std::vector<uint64_t> w = pack_tight(text.substr(0, (size_t)start + L + (size_t)k));
            if (w0 + nw != w.size() || nw > MSNP_TEXT_WORDS || ((w0 << 5) + rel0) != start - 1u) fail("text words", k, start, L, nw);
            n_ten_words += nw == MSNP_TEXT_WORDS;
            n_first_word_alone += (start & 31u) == 0;
            for (int passes = 1; passes <= 3; passes++) {
                std::string lit = text;
                std::vector<Snp> want;
                uint32_t want_c = 0, want_d = 0;
                if (passes & 1) want_c = literal_forward(lit, start, L, k, m, graph, want);
                const size_t want_fwd = want.size();
                /* the scan: a gap taken whole ends the observers; one taken in part goes on shrunken; FindMultiSNPrev's own test */
                if ((passes & 2) && want_c != L && L - want_c > (uint32_t)(k + m)) want_d = literal_reverse(lit, start, L, L - want_c, k, m, graph, want);
                std::vector<uint64_t> priv(w.begin() + w0, w.end()); /* exactly nw words */
                std::vector<uint32_t> entries(msnp_max_calls(L, m) + 1u, 0xDEADBEEFu);
                uint32_t n_fwd = 0, n_rev = 0, d = 0;
                const uint32_t c = msnp_passes_chain(priv.data(), rel0, L, k, m, passes, [&](uint64_t x) { return graph.has(x); }, entries.data(), &n_fwd, &d, &n_rev);
                if (c != want_c || d != want_d || n_fwd != want_fwd || n_fwd + n_rev != want.size()) fail("chain", k, t, passes, (long)c * 1000 + d);
                if (n_fwd + n_rev > msnp_max_calls(L, m) || entries[msnp_max_calls(L, m)] != 0xDEADBEEFu || c + d > L) fail("room", k, t, n_fwd + n_rev, msnp_max_calls(L, m));
                for (uint32_t i = 0; i < n_fwd + n_rev; i++) {
                    const uint32_t e = entries[i];
                    const uint32_t pos = msnp_entry_is_rev(e) ? msnp_rev_pos_of(start, L, e) : msnp_pos_of(start, e, k);
                    if (!(e & MSNP_ENTRY) || msnp_entry_is_rev(e) != want[i].rev || pos != want[i].pos || ((e >> SNP_ALT_SHIFT) & 3u) != want[i].alt || ((e >> SNP_REF_SHIFT) & 3u) != want[i].ref)
                        fail("entry", k, t, i, e);
                    if (snp_ins_of(e) != ((uint32_t)(unsigned char)NT[want[i].alt] | ((uint32_t)(unsigned char)NT[want[i].ref] << 8))) fail("ins", k, t, i, e);
                    if (i > n_fwd && want[i].pos >= want[i - 1].pos) fail("reverse calls descend", k, t, i, e);
                }
                /* the private words carry the substitutions of both passes and nothing else */
                const std::vector<uint64_t> cw = pack_tight(lit.substr(0, (size_t)start + L + (size_t)k));
                for (uint32_t i = 0; i < nw; i++)
                    if (priv[i] != cw[w0 + i]) fail("corrected text", k, t, i, passes);
                if (passes == 1) { /* the forward functions on the forward text give the same */
                    const uint32_t f0 = start >> 5;
                    std::vector<uint64_t> fpriv(w.begin() + f0, w.end());
                    std::vector<uint32_t> fentries(msnp_max_calls(L, m) + 1u, 0u);
                    uint32_t fn = 0;
                    const uint32_t fc = msnp_chain(fpriv.data(), start & 31u, L, k, m, [&](uint64_t x) { return graph.has(x); }, fentries.data(), &fn);
                    if (fc != c || fn != n_fwd) fail("passes 1 against msnp_chain", k, t, fc, c);
                    for (uint32_t i = 0; i < fn; i++) if (fentries[i] != entries[i]) fail("passes 1 entries", k, t, i, 0);
                }
                if (passes == 2) { n_rev_calls += n_rev; n_whole += d == L; }
                if (passes == 3) { n_fwd_calls += n_fwd; n_after += c && c != L && n_rev; n_meet += n_fwd && n_rev && c + d == L; }
            }
            n_gaps++;
        }
    if (n_rev_calls < 10000 || n_anchor < 200 || n_whole < 200 || n_after < 200 || n_meet < 20 || n_ten_words < 20 || n_first_word_alone < 20)
        fail("the cases do not cover", (long)n_anchor, (long)n_whole, (long)n_after, (long)n_meet);
    /* 2. the limits and the entry form */
    if (msnp_rev_text_words(32, 254, 32) != 10u || msnp_rev_rel0(32) != 31u || msnp_rev_text_words(1, 254, 32) != 9u || msnp_rev_rel0(1) != 0u || msnp_rev_text_words(33, 254, 31) != 9u ||
        msnp_rev_text_words(1, 7, 5) != 1u)
        fail("text words at the limits", 0, 0, 0, 0);
    for (uint32_t start = 1; start < 200; start++)
        for (uint32_t L = 7; L <= MSNP_MAX_GAP; L++)
            for (int k : {5, 11, 31, 32}) {
                const uint32_t first = (start - 1u) >> 5, last = (start + L + (uint32_t)k - 1u) >> 5;
                if (msnp_rev_text_words(start, L, k) != last - first + 1u || msnp_rev_text_words(start, L, k) > MSNP_TEXT_WORDS) fail("text words", start, L, k, 0);
            }
    for (uint32_t d = 0; d < MSNP_MAX_GAP; d++)
        for (uint32_t alt = 0; alt < 4; alt++)
            for (uint32_t ref = 0; ref < 4; ref++) {
                const uint32_t e = msnp_rev_entry(d, alt, ref), f = msnp_entry(d, alt, ref);
                if (!e || !msnp_entry_is_rev(e) || msnp_entry_is_rev(f) || (e & 0xFFu) != d || (e & ~MSNP_REV) != f || snp_ins_of(e) != snp_ins_of(f) || msnp_rev_pos_of(100, 254, e) != 353u - d)
                    fail("entry form", d, alt, ref, e);
            }
    for (int k : {5, 31})
        for (int m = 1; m <= 5; m++)
            for (uint32_t L = 1; L <= 300; L++)
                for (uint32_t c = 0; c <= L; c++)
                    if (msnp_rev_is_asked(L, c, k, m) != (c != L && L - c > (uint32_t)(k + m))) fail("entry test", k, m, L, c);
    for (int p = -2; p <= 6; p++)
        if (msnp_passes_valid(p) != (p == 1 || p == 2 || p == 3)) fail("passes", p, 0, 0, 0);
    printf("OK %llu gaps %llu forward %llu reverse %llu anchor %llu whole %llu after %llu meet %llu ten\n", n_gaps, n_fwd_calls, n_rev_calls, n_anchor, n_whole, n_after, n_meet, n_ten_words);
    return 0;
}
