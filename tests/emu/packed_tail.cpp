/* TEST-ONLY: the packed link path of a batch's sequence arena on the host.  expand_codes (AVX2 unless MTG_NO_VEC) against expand_codes_scalar for
 * every start offset modulo 32 and every length up to 300; expand_packed_tail (expansion over the pool + the NULs put back from the records)
 * against the arena it came from; and the device's writer (mtg_emit.h: emit_ascii_g with a PackedTail, one lane here) followed by the host's
 * expansion against the all-ASCII arena, for forward and reverse fills at every alignment.  Links with emu_backend.cpp.  Prints OK. */
#include "../../mindthegap_amd/csrc/mtg_host.cpp"
#include <random>

static const char NT[4] = {'A', 'C', 'T', 'G'};

int main()
{
    std::mt19937_64 rng(7);
    /* 1. the expander itself: nothing outside [b, e) is written */
    {
        std::vector<uint64_t> w(24);
        std::vector<char> a(24 * 32 + 64), s(24 * 32 + 64);
        for (int round = 0; round < 8; round++) {
            for (auto& x : w) x = rng();
            for (size_t b = 0; b < 64; b++)
                for (size_t len = 0; len <= 300; len++) {
                    std::fill(a.begin(), a.end(), '#');
                    std::fill(s.begin(), s.end(), '#');
                    mtgi::expand_codes(w.data(), b, b + len, a.data());
                    mtgi::expand_codes_scalar(w.data(), b, b + len, s.data());
                    if (a != s) { fprintf(stderr, "expand_codes b %zu len %zu differs from the scalar form\n", b, len); return 1; }
                    for (size_t i = b; i < b + len; i++)
                        if (s[i] != NT[(w[i >> 5] >> (2 * (i & 31))) & 3]) { fprintf(stderr, "expand_codes_scalar b %zu len %zu: byte %zu\n", b, len, i); return 1; }
                }
        }
    }
    /* 2. a batch's arena: fills of 0 .. 700 letters in gap order, gaps without a fill in between (their filled record is stale), every share */
    for (int round = 0; round < 60; round++) {
        const size_t n = 1 + rng() % (round < 10 ? 8 : 3000);
        std::vector<std::string> fills(n);
        std::vector<bool> has(n);
        size_t total = 0;
        for (size_t g = 0; g < n; g++) {
            has[g] = rng() % 4 != 0;
            if (!has[g]) continue;
            const size_t L = rng() % 8 == 0 ? rng() % 3 : rng() % 701;
            fills[g].resize(L);
            for (auto& c : fills[g]) c = NT[rng() & 3];
            total += L + 1;
        }
        char* want = (char*)aligned_alloc(64, total + 64);
        char* got = (char*)aligned_alloc(64, total + 64);
        std::vector<mtg_gap_result> res(n);
        std::vector<mtg_filled> fil(n);
        memset(res.data(), 0, n * sizeof(mtg_gap_result));
        size_t o = 0;
        for (size_t g = 0; g < n; g++) {
            fil[g].seq = (const char*)(uintptr_t)(rng() | 1); /* a stale pointer where the gap has no fill */
            if (!has[g]) continue;
            res[g].n_filled = 1;
            fil[g].seq = got + o;
            memcpy(want + o, fills[g].data(), fills[g].size());
            want[o + fills[g].size()] = 0;
            o += fills[g].size() + 1;
        }
        const uint64_t end = total;
        std::vector<uint64_t> shadow((end + 31) / 32 + 2);
        for (uint32_t q : {0u, 1u, 9000u, 32768u, 49152u, 65535u, 65536u, (uint32_t)(rng() % 65537)}) {
            const uint64_t x = packed_split(end, q);
            if (x % 32 || x > end) { fprintf(stderr, "packed_split(%llu, %u) = %llu\n", (unsigned long long)end, q, (unsigned long long)x); return 1; }
            std::fill(shadow.begin(), shadow.end(), 0);
            for (uint64_t i = x; i < end; i++) shadow[(i - x) >> 5] |= (uint64_t)(want[i] ? mtg::nt_code((unsigned char)want[i]) : 0u) << (2 * ((i - x) & 31));
            for (int nt : {1, 4}) {
                memcpy(got, want, x);
                memset(got + x, '#', end - x + 64);
                mtgi::expand_packed_tail(shadow.data(), got, x, end, res.data(), fil.data(), n, nt);
                if (memcmp(got, want, end) != 0 || got[end] != '#') {
                    size_t i = 0;
                    while (i < end && got[i] == want[i]) i++;
                    fprintf(stderr, "expand_packed_tail n %zu end %llu q %u threads %d: byte %zu is %d, not %d\n", n, (unsigned long long)end, q, nt, i, got[i], want[i]);
                    return 1;
                }
            }
        }
        free(want);
        free(got);
    }
    /* 3. the device's writer in packed form, then the host's expansion, against the ASCII it writes otherwise (fills read forward or backward from
     * random words, at every offset of the arena's 64-byte aligned base; ragged ends of neighbouring fills share the halves they are OR-ed into) */
    for (int round = 0; round < 200; round++) {
        std::vector<uint64_t> words(80);
        for (auto& x : words) x = rng();
        const size_t n = 1 + rng() % 40;
        struct F { uint32_t from, L; bool rc; uint64_t at; };
        std::vector<F> fs(n);
        uint64_t end = 0;
        for (auto& f : fs) {
            f.L = rng() % 5 == 0 ? rng() % 20 : rng() % 400;
            f.from = rng() % (75 * 32 - f.L);
            f.rc = rng() & 1;
            f.at = end;
            end += f.L + 1;
        }
        char* ascii = (char*)aligned_alloc(64, end + 128);
        char* got = (char*)aligned_alloc(64, end + 128);
        std::vector<mtg_gap_result> res(n);
        std::vector<mtg_filled> fil(n);
        memset(res.data(), 0, n * sizeof(mtg_gap_result));
        for (size_t g = 0; g < n; g++) { res[g].n_filled = 1; fil[g].seq = got + fs[g].at; }
        for (const F& f : fs) mtg::emit_ascii(words.data(), f.from, f.L, f.rc, ascii + f.at);
        const uint32_t q = round % 4 == 0 ? 65536u : (uint32_t)(rng() % 65537);
        const uint64_t x = packed_split(end, q);
        std::vector<uint32_t> half(2 * ((end - x + 31) / 32 + 1), 0);
        const PackedTail pk{half.data(), x, half.size()};
        memset(got, '#', end + 128);
        for (const F& f : fs) mtg::emit_ascii_g<1>(words.data(), f.from, f.L, f.rc, got + f.at, 0, pk, f.at);
        for (uint64_t i = x; i < end; i++)
            if (got[i] != '#') { fprintf(stderr, "the packed writer wrote arena byte %llu at or above the split %llu\n", (unsigned long long)i, (unsigned long long)x); return 1; }
        mtgi::expand_packed_tail(reinterpret_cast<const uint64_t*>(half.data()), got, x, end, res.data(), fil.data(), n, 3);
        if (memcmp(got, ascii, end) != 0 || got[end] != '#') {
            size_t i = 0;
            while (i < end && got[i] == ascii[i]) i++;
            fprintf(stderr, "packed writer + expansion, round %d end %llu x %llu: byte %zu is %d, not %d\n", round, (unsigned long long)end, (unsigned long long)x, i, got[i], ascii[i]);
            return 1;
        }
        free(ascii);
        free(got);
    }
    printf("OK\n");
    return 0;
}
