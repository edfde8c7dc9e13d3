/* TEST-ONLY: the terminal search of a seed of a shared target table (mtg_post.h: post_search_indexed with the table's piece index under gid 0 and
 * the seed's excluded entries) against a literal restatement of Filler::find_nodes_containing_multiple_R (src/Filler.cpp:1294-1378) over the seed's
 * own dictionary -- a fresh std::unordered_map<std::string, std::pair<std::string, bool>> into which the table's entries but the excluded ones were
 * inserted in table order (:522-533).  Random tables of 2 .. 2 000 entries (keys with up to two differences from a place of the contig, N, lower
 * case, keys shorter than k, keys built to tie), 0 .. 2 exclusions.  The device's answer must equal the reference's, except that where several
 * entries of the seed's dictionary reach the winning count at the winning position the device answers the first in TABLE order and raises its tie
 * flag: the flag must be up exactly there.  Also the early-stop pattern with the excluded keys cut out of the key text (mtg_traverse.h:
 * swf_pattern, contig_contains) against std::string::find on the concatenated keys.  Prints OK and the counts. */
#include "../../mindthegap_amd/csrc/mtg_hostutil.h"
#include "../../mindthegap_amd/csrc/mtg_post.h"
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <unordered_map>
#include <vector>

using namespace mtg;

typedef std::unordered_map<std::string, std::pair<std::string, bool>> dict_t; /* bkpt_dict_t, src/Utils.hpp:43-44 */

static int identNT(char a, char b) { return ((a == b || a - b == 32 || a - b == -32) && a != 'N'); } /* src/Utils.cpp:81-84 */

struct Ref {
    bool found = false;
    int pos = 0, errors = 0;
    uint32_t entry = 0;
    int winners = 0; /* entries of the seed's dictionary with the best count at the best position */
};

/* find_nodes_containing_multiple_R for one contig, literally (a key shorter than k never matches: the project's rule for short anchors) */
static Ref reference(const std::string& node, const dict_t& d, const std::unordered_map<std::string, uint32_t>& entry_of, int k, int nb_mis)
{
    Ref r;
    int best_match = 0;
    std::string best_name;
    int position = 0;
    bool arret = false;
    for (size_t j = 0; j + (size_t)k <= node.size() && !arret; j++)
        for (auto it = d.begin(); it != d.end() && !arret; ++it) {
            if ((int)it->first.size() < k) continue;
            int nbmatch = 0;
            for (int i = 0; i < k; i++) nbmatch += identNT(node[j + i], it->first[i]);
            if (nbmatch > best_match && nbmatch >= k - nb_mis) {
                best_name = it->second.first;
                position = (int)j;
                best_match = nbmatch;
                if (nbmatch == k) { arret = true; break; }
            }
        }
    if (best_match == 0) return r;
    r.found = true;
    r.pos = position;
    r.errors = k - best_match;
    r.entry = entry_of.at(best_name);
    for (auto it = d.begin(); it != d.end(); ++it) {
        if ((int)it->first.size() < k) continue;
        int nbmatch = 0;
        for (int i = 0; i < k; i++) nbmatch += identNT(node[(size_t)position + i], it->first[i]);
        if (nbmatch == best_match) r.winners++;
    }
    return r;
}

int main()
{
    std::mt19937_64 rng(11);
    const char* NT = "ACGT";
    long trials = 0, found = 0, ties = 0, excl_hits = 0, r_checks = 0, r_found = 0;
    for (int round = 0; round < 3000; round++) {
        const int k = 11 + (int)(rng() % 21);
        uint32_t nb_mis = (uint32_t)(rng() % 3);
        if (!post_index_usable(k, nb_mis)) nb_mis = 0;
        const uint32_t n = round < 50 ? 2 + (uint32_t)round : 2 + (uint32_t)(rng() % (round % 10 == 0 ? 1999 : 200));
        const size_t L = (size_t)k + (size_t)(rng() % 600);
        std::string node(L, 'A');
        for (auto& c : node) c = NT[rng() & 3];
        /* the keys: random ones, and copies of places of the contig with up to two changes of every kind */
        std::vector<std::string> keys;
        dict_t all_check;
        while (keys.size() < n) {
            std::string key((size_t)k, 'A');
            const uint32_t kind = (uint32_t)(rng() % 8);
            if (kind < 2) for (auto& c : key) c = NT[rng() & 3];
            else {
                key = node.substr((size_t)(rng() % (L - (size_t)k + 1)), (size_t)k);
                const int changes = (int)(rng() % 4);
                for (int c = 0; c < changes; c++) key[rng() % (size_t)k] = NT[rng() & 3];
                if (kind == 5) key[rng() % (size_t)k] = 'N';
                if (kind == 6) for (auto& c : key) if (rng() & 1) c = (char)(c | 0x20);
                if (kind == 7 && rng() % 3 == 0) key.resize((size_t)(rng() % (size_t)k));
            }
            if (!all_check.insert({key, {"", false}}).second) continue; /* keys of a dictionary are distinct */
            keys.push_back(key);
            if (rng() % 6 == 0 && keys.size() < n && (int)key.size() == k) { /* a key that ties with this one: the other place of one difference */
                std::string twin = key;
                const size_t at = rng() % (size_t)k;
                twin[at] = NT[((twin[at] >> 1) + 1 + rng() % 3) & 3];
                if (all_check.insert({twin, {"", false}}).second) keys.push_back(twin);
            }
        }
        /* the table: entry numbers are the positions in `keys`; the seed leaves out 0 .. 2 of them */
        std::vector<uint8_t> excluded(n, 0);
        std::vector<uint32_t> excl;
        const int ne = (int)(rng() % 3);
        for (int e = 0; e < ne; e++) excluded[rng() % n] = 1;
        for (uint32_t e = 0; e < n; e++) if (excluded[e]) excl.push_back(e);
        dict_t d;
        std::unordered_map<std::string, uint32_t> entry_of;
        for (uint32_t e = 0; e < n; e++) {
            entry_of["t" + std::to_string(e)] = e;
            if (!excluded[e]) d.insert({keys[e], {"t" + std::to_string(e), false}});
        }
        /* the device's side: the table encoded (mtg_targets_create: TARGET_SLOT slots, encode_target), its piece index under gid 0 */
        std::vector<uint64_t> le(n), bad(n);
        for (uint32_t e = 0; e < n; e++) {
            uint8_t slot[TARGET_SLOT] = {0};
            const bool usable = keys[e].size() >= (size_t)k;
            if (usable) memcpy(slot, keys[e].data(), (size_t)k);
            slot[TARGET_SLOT - 1] = usable ? 1 : 0;
            encode_target(slot, k, le[e], bad[e]);
        }
        uint32_t cap = 1024;
        while (cap < 4 * n) cap <<= 1;
        std::vector<uint32_t> head(cap, POST_INDEX_NIL), next(4 * (size_t)n, POST_INDEX_NIL);
        for (uint32_t e = 0; e < n; e++) post_index_add(head.data(), next.data(), cap - 1, 0u, e, le[e], bad[e], nb_mis, k);
        std::vector<uint64_t> cut; /* (first nucleotide, length, entry) of every excluded key, as the pattern descriptor holds them */
        std::vector<uint64_t> key_off(n + 1, 0);
        for (uint32_t e = 0; e < n; e++) key_off[e + 1] = key_off[e] + keys[e].size();
        for (uint32_t e : excl) { cut.push_back(key_off[e]); cut.push_back(key_off[e + 1] - key_off[e]); cut.push_back(e); }
        PostTargets T;
        T.le = le.data(); T.bad = bad.data(); T.n = n; T.nb_mis = nb_mis; T.fast_ok = 1;
        T.pi_head = head.data(); T.pi_next = next.data(); T.pi_mask = cap - 1; T.gbase = 0; T.gid = 0;
        T.excl = cut.data(); T.n_excl = (uint32_t)excl.size();
        std::vector<uint64_t> words(L / 32 + 2, 0);
        for (size_t i = 0; i < L; i++) words[i >> 5] |= (uint64_t)nt_code((unsigned char)node[i]) << (2 * (i & 31));
        bool tie = false;
        const uint64_t best = post_search_indexed(T, words.data(), (uint32_t)L, k, tie);
        const Ref want = reference(node, d, entry_of, k, (int)nb_mis);
        trials++;
        const uint64_t ORD = (1ull << 40) - 1;
        if (!want.found) {
            if (best != 0) { printf("round %d: the device finds a target, the reference none\n", round); return 1; }
        } else {
            found++;
            const uint64_t order = ORD - (best & ORD);
            const int pos = (int)(order / n), errors = k - (int)(best >> 40);
            const uint32_t entry = (uint32_t)(order % n);
            if (best == 0 || pos != want.pos || errors != want.errors) {
                printf("round %d: device pos %d errors %d, reference pos %d errors %d\n", round, pos, errors, want.pos, want.errors);
                return 1;
            }
            if (excluded[entry]) { printf("round %d: the device answers an excluded entry\n", round); return 1; }
            if (tie != (want.winners >= 2)) { printf("round %d: tie flag %d, %d entries reach the best count at the best position\n", round, (int)tie, want.winners); return 1; }
            if (!tie && entry != want.entry) { printf("round %d: no tie flagged, device entry %u, reference entry %u\n", round, entry, want.entry); return 1; }
            ties += tie;
        }
        for (uint32_t e : excl) excl_hits += (keys[e].size() >= (size_t)k); /* (how often an exclusion could have mattered) */
        /* the early-stop pattern: R = the kept keys in table order; the device reads the key text with the excluded spans cut out */
        std::string R;
        for (uint32_t e = 0; e < n; e++) if (!excluded[e]) R += keys[e];
        std::vector<uint64_t> text(key_off[n] / 32 + 2, 0);
        for (uint32_t e = 0; e < n; e++)
            for (size_t c = 0; c < keys[e].size(); c++) { const uint64_t j = key_off[e] + c; text[j >> 5] |= (uint64_t)nt_code((unsigned char)keys[e][c]) << (2 * (j & 31)); }
        std::vector<uint64_t> desc = {(uint64_t)(uintptr_t)text.data(), (uint64_t)excl.size()};
        desc.insert(desc.end(), cut.begin(), cut.end());
        const uint32_t roff = SEED_PATTERN, rlen = (uint32_t)R.size();
        const uint64_t r0 = 0;
        const SwfPattern P = swf_pattern(desc.data(), &roff, &rlen, &r0, 0);
        for (uint32_t j = 0; j < rlen; j++)
            if (pattern_nt(P, j) != nt_code((unsigned char)R[j])) { printf("round %d: nucleotide %u of the cut pattern\n", round, j); return 1; }
        /* a contig that holds R (when R is short enough to be worth it) and one that may not */
        if (R.size() <= 4000) {
            std::string hay(rng() % 50, 'A');
            for (auto& c : hay) c = NT[rng() & 3];
            std::string R_up = R;
            for (auto& c : R_up) c = "ACTG"[nt_code((unsigned char)c)]; /* (the codes: A 0, C 1, T 2, G 3) */
            hay += R_up;
            for (int i = 0; i < 20; i++) hay += NT[rng() & 3];
            if (rng() & 1) hay[rng() % hay.size()] = NT[rng() & 3];
            std::vector<uint64_t> hw(hay.size() / 32 + 2, 0);
            for (size_t i = 0; i < hay.size(); i++) hw[i >> 5] |= (uint64_t)nt_code((unsigned char)hay[i]) << (2 * (i & 31));
            const bool got = contig_contains(hw.data(), (uint32_t)hay.size(), P), exp = hay.find(R_up) != std::string::npos;
            if (got != exp) { printf("round %d: contig_contains %d, find %d (|R| %zu)\n", round, (int)got, (int)exp, R.size()); return 1; }
            r_checks++;
            r_found += got;
        }
    }
    printf("OK %ld contigs, %ld with a target, %ld ties, %ld usable exclusions, %ld patterns (%ld found)\n", trials, found, ties, excl_hits, r_checks, r_found);
    return 0;
}
