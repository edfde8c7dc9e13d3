/* TEST-ONLY: the pieces of the terminal search's index (mtg_post.h: post_piece_begin, post_index_add, post_search_indexed) for every k and
 * nb_mis the product accepts.
 * 1. The layout: the nb_mis + 1 pieces tile the k nucleotides -- the first begins at 0, the last ends at k, each is k / np or k / np + 1 long.  The
 *    answers of the search do not depend on that (any nb_mis + 1 disjoint pieces leave one without a difference); the number of candidates a
 *    look-up returns does: a nucleotide outside every piece is one the index cannot tell targets apart by.
 * 2. The search: a dictionary of 40 targets, one of them a place of the contig with m <= nb_mis substitutions at EVERY set of m positions (all
 *    C(k, m) of them: each seam of the pieces, both ends, two in one piece); the indexed search must find that place with k - m matches.
 * Prints OK and the counts. */
#include "../../mindthegap_amd/csrc/mtg_hostutil.h"
#include "../../mindthegap_amd/csrc/mtg_post.h"
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

using namespace mtg;

int main()
{
    std::mt19937_64 rng(5);
    const char* NT = "ACGT";
    long layouts = 0, searches = 0;
    for (int k = 11; k <= 31; k++)
        for (uint32_t nb_mis = 0; nb_mis < (uint32_t)POST_PIECES_MAX; nb_mis++) {
            const uint32_t np = nb_mis + 1u;
            if (post_piece_begin(0, np, k) != 0u || post_piece_begin(np, np, k) != (uint32_t)k) { printf("k %d, %u pieces: they span %u .. %u\n", k, np, post_piece_begin(0, np, k), post_piece_begin(np, np, k)); return 1; }
            for (uint32_t p = 0; p < np; p++) {
                const uint32_t len = post_piece_begin(p + 1u, np, k) - post_piece_begin(p, np, k);
                if (len != (uint32_t)k / np && len != (uint32_t)k / np + 1u) { printf("k %d, %u pieces: piece %u has %u nucleotides\n", k, np, p, len); return 1; }
            }
            layouts++;
            if (!post_index_usable(k, nb_mis)) continue;
            /* a contig, 39 random targets and the target under test (number 17) */
            const size_t L = 300;
            std::string node(L, 'A');
            for (auto& c : node) c = NT[rng() & 3];
            const uint32_t n = 40, me = 17;
            std::vector<std::string> keys(n, std::string((size_t)k, 'A'));
            for (auto& key : keys) for (auto& c : key) c = NT[rng() & 3];
            const size_t place = 100 + (size_t)(rng() % 64);
            std::vector<uint64_t> words(L / 32 + 2, 0);
            for (size_t i = 0; i < L; i++) words[i >> 5] |= (uint64_t)nt_code((unsigned char)node[i]) << (2 * (i & 31));
            /* every set of m <= nb_mis positions (as a bit mask over k positions) */
            std::vector<uint32_t> sets = {0u};
            for (uint32_t m = 1; m <= nb_mis; m++) {
                std::vector<uint32_t> grown;
                for (uint32_t s : sets) {
                    if ((uint32_t)__builtin_popcount(s) != m - 1u) continue;
                    for (int i = s ? 32 - __builtin_clz(s) : 0; i < k; i++) grown.push_back(s | (1u << i));
                }
                sets.insert(sets.end(), grown.begin(), grown.end());
            }
            for (uint32_t s : sets) {
                std::string key = node.substr(place, (size_t)k);
                for (int i = 0; i < k; i++) if (s & (1u << i)) key[(size_t)i] = NT[(strchr(NT, key[(size_t)i]) - NT + 1 + (int)(rng() % 3)) & 3];
                keys[me] = key;
                std::vector<uint64_t> le(n), bad(n);
                for (uint32_t e = 0; e < n; e++) {
                    uint8_t slot[TARGET_SLOT] = {0};
                    memcpy(slot, keys[e].data(), (size_t)k);
                    slot[TARGET_SLOT - 1] = 1;
                    encode_target(slot, k, le[e], bad[e]);
                }
                std::vector<uint32_t> head(1024, POST_INDEX_NIL), next(4 * (size_t)n, POST_INDEX_NIL);
                for (uint32_t e = 0; e < n; e++) post_index_add(head.data(), next.data(), 1023u, 0u, e, le[e], bad[e], nb_mis, k);
                PostTargets T;
                T.le = le.data(); T.bad = bad.data(); T.n = n; T.nb_mis = nb_mis; T.fast_ok = 1;
                T.pi_head = head.data(); T.pi_next = next.data(); T.pi_mask = 1023u; T.gbase = 0; T.gid = 0;
                bool tie = false;
                const uint64_t best = post_search_indexed(T, words.data(), (uint32_t)L, k, tie);
                const uint64_t ORD = (1ull << 40) - 1, order = ORD - (best & ORD);
                const uint32_t m = (uint32_t)__builtin_popcount(s);
                /* (40 random targets of 11 or more nucleotides within two differences of a place of a random contig: not in this seed's draws) */
                if (best == 0 || (uint32_t)(best >> 40) != (uint32_t)k - m || order / n != place || order % n != me) {
                    printf("k %d nb_mis %u, substitutions at mask %#x: found count %u at %llu (target %llu), expected %u at %zu (target %u)\n", k, nb_mis, s, (uint32_t)(best >> 40),
                           (unsigned long long)(order / n), (unsigned long long)(order % n), (uint32_t)k - m, place, me);
                    return 1;
                }
                searches++;
            }
        }
    printf("OK %ld layouts, %ld searches\n", layouts, searches);
    return 0;
}
