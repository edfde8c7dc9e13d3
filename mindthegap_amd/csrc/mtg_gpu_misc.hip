/*
 * mtg_gpu_misc.hip -- the smaller device entries of libmtgfill.so (gfx950 only) and the device side of the C ABI.
 *
 *   k_query                          : batched contains / queryAbundance / successors / predecessors
 *   k_scan                           : rolling 2-bit k-mer + minimizer-blocked Bloom probe along packed sequences, blocks staged in LDS
 *   k_profile, k_profile_*           : the scan's sibling (the same tile stage, scan_tile_stage) that also answers abundance and degrees per
 *                                      position, and the runs of absent k-mers
 *   k_find_*, k_mark_*               : `find` for homozygous insertions: the scan's gaps, their candidates compacted in order, one wave per
 *                                      candidate for the degree tests and the micro-assembly of 1-2 nt, the calls compacted in order
 *   k_nw                             : Needleman-Wunsch match counts for the de-duplication of multi-path solutions, one wave per pair
 *                                      (remove_almost_identical_solutions, /root/reference/src/Utils.cpp:87-189,208-238)
 *   k_fmt_*                          : the tool's text (FASTA / info / VCF) of the sites with one solution (mtg_format.h)
 *   k_chase                          : dependent random 64-byte reads (measured roofline ceiling)
 */
#include "mtg_gpu_common.h"
#include "mtg_profile_runs.h"
#include "mtg_find_gaps.h"
#include "mtg_find_het.h"
#include "mtg_find_del.h"
#include "mtg_find_snp.h"
#include "mtg_find_msnp.h"

namespace mtgi {

static thread_local char g_err[512] = "";
static thread_local mtg_batch_stats g_stats{};
void set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
void stats_store(const mtg_batch_stats& s) { g_stats = s; }

__global__ void k_query(Index ix, const uint64_t* __restrict__ kmers, size_t n, uint32_t* abund, uint8_t* succ, uint8_t* pred)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const uint64_t mk1 = kmask(ix.k - 1);
    uint32_t lines = 0;
    for (; i < n; i += stride) {
        Kmer x = make_kmer(kmers[i] & kmask(ix.k), ix.k);
        if (abund) abund[i] = abundance(ix, x, lines);
        if (succ) succ[i] = (uint8_t)adj_right_t(ix.adj, x, mk1, lines).out;
        if (pred) pred[i] = (uint8_t)adj_left(ix, x, mk1, lines).in;
    }
}

/* ---- the tool's text on the device (mtg_format.h): one wave per site.  pass 0: is the site simple, and how many bytes does it add to the
 * three files; pass 1 (after the scan): the bytes, at the site's offsets.  The records are the batch's C-ABI records (their seq pointers
 * are addresses of the HOST arena: the same offsets in the workspace's arena d_seq). */
struct FmtArgs {
    const mtg_gap_result* res;
    const mtg_filled* fil;
    const char* text;            /* the batch's text block on the device */
    const uint64_t* source_off;
    const uint32_t* source_len;
    const uint64_t* name_off;
    const uint32_t* name_len;
    const char* d_seq;           /* the sequence arena on the device */
    uint64_t host_seq;           /* address the arena has (would have) on the host */
    uint64_t seq_used;
    uint64_t host_fil;           /* address of the host's fil array: res[i].filled == host_fil + i * sizeof(mtg_filled) on the common path */
    FmtRec* rec;
    char* out[FMT_STREAMS];
    uint32_t n;
};
__device__ __forceinline__ bool fmt_load_site(const FmtArgs& A, uint32_t i, FmtSite& t)
{
    const mtg_gap_result r = A.res[i];
    /* the common path leaves a gap's one solution in slot i of the fil array; anything else (no solution, a record the host wrote) is not ours */
    if (r.n_filled != 1 || (uint64_t)(uintptr_t)r.filled != A.host_fil + (uint64_t)i * sizeof(mtg_filled)) return false;
    const mtg_filled f = A.fil[i];
    const uint64_t q = (uint64_t)(uintptr_t)f.seq;
    if (q < A.host_seq || q >= A.host_seq + A.seq_used) return false;
    t.name = A.text + A.name_off[i]; t.name_len = A.name_len[i];
    t.source = A.text + A.source_off[i]; t.source_len = A.source_len[i];
    t.seq = A.d_seq + (q - A.host_seq);
    t.seq_len = fmt_strlen(t.seq);
    t.nb_nodes = r.nb_nodes; t.total_nt = r.total_nt; t.nb_terminal = r.nb_terminal; t.has_counts = r.has_solution_counts;
    t.nb_total_filled = r.nb_total_filled; t.nb_reported = r.nb_reported;
    t.qual = f.qual; t.solution_count = f.solution_count; t.avg = f.avg_coverage; t.median = f.median_coverage;
    return fmt_site_simple(t);
}
__global__ void __launch_bounds__(64) k_fmt_size(FmtArgs A)
{
    const uint32_t i = blockIdx.x;
    if (i >= A.n) return;
    FmtSite t;
    FmtCount c;
    c.n[0] = c.n[1] = c.n[2] = 0;
    const bool simple = fmt_load_site(A, i, t);
    if (simple) format_site(c, t);
    if (threadIdx.x == 0) { FmtRec r; r.size[0] = c.n[0]; r.size[1] = c.n[1]; r.size[2] = c.n[2]; r.simple = simple ? 1u : 0u; r.off[0] = r.off[1] = r.off[2] = 0; A.rec[i] = r; }
}
/* exclusive prefix sums of the three sizes in site order, the list of the sites left to the host with the offsets where their text belongs;
 * tot[0..2] = bytes, tot[3] = simple sites, tot[4] = sites for the host.  One workgroup. */
__global__ void __launch_bounds__(1024) k_fmt_scan(FmtRec* rec, uint32_t n, uint32_t* cplx, uint64_t* cplx_off, unsigned long long* tot)
{
    __shared__ unsigned long long wsum[16][4];
    __shared__ unsigned long long carry[4];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    if (t < 4) carry[t] = 0;
    __syncthreads();
    for (uint32_t b0 = 0; b0 < n; b0 += 1024) {
        const uint32_t i = b0 + t;
        unsigned long long v[4] = {0, 0, 0, 0};
        if (i < n) { v[0] = rec[i].size[0]; v[1] = rec[i].size[1]; v[2] = rec[i].size[2]; v[3] = rec[i].simple ? 0 : 1; }
        unsigned long long incl[4];
        for (int j = 0; j < 4; j++) {
            unsigned long long x = v[j];
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)x, d, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(x >> 32), d, 64);
                if ((int)lane >= d) x += ((unsigned long long)hi << 32) | lo;
            }
            incl[j] = x;
            if (lane == 63) wsum[wv][j] = x;
        }
        __syncthreads();
        unsigned long long before[4];
        for (int j = 0; j < 4; j++) {
            unsigned long long x = carry[j];
            for (uint32_t w2 = 0; w2 < wv; w2++) x += wsum[w2][j];
            before[j] = x;
        }
        if (i < n) {
            const unsigned long long o0 = before[0] + incl[0] - v[0], o1 = before[1] + incl[1] - v[1], o2 = before[2] + incl[2] - v[2];
            rec[i].off[0] = o0; rec[i].off[1] = o1; rec[i].off[2] = o2;
            if (v[3]) { const unsigned long long c = before[3] + incl[3] - 1; cplx[c] = i; cplx_off[3 * c] = o0; cplx_off[3 * c + 1] = o1; cplx_off[3 * c + 2] = o2; }
        }
        __syncthreads();
        if (t < 4) { unsigned long long x = carry[t]; for (int w2 = 0; w2 < 16; w2++) x += wsum[w2][t]; carry[t] = x; }
        __syncthreads();
    }
    if (t < 3) tot[t] = carry[t];
    if (t == 3) { tot[4] = carry[3]; tot[3] = (unsigned long long)n - carry[3]; }
}
__global__ void __launch_bounds__(64) k_fmt_write(FmtArgs A)
{
    const uint32_t i = blockIdx.x;
    if (i >= A.n) return;
    const FmtRec r = A.rec[i];
    if (!r.simple) return;
    FmtSite t;
    if (!fmt_load_site(A, i, t)) return;
    FmtWrite w;
    w.p[0] = A.out[0] + r.off[0]; w.p[1] = A.out[1] + r.off[1]; w.p[2] = A.out[2] + r.off[2];
    format_site(w, t);
}

/* Needleman-Wunsch match count of src/Utils.cpp:87-189, one wave per sequence pair (a = rows, b = columns), exact for any length.
 * The matrix is swept in strips of 64 columns; inside a strip lane l owns column j0+l+1 and works on row t-l at step t, so that the
 * cell to its left (lane l-1, previous step) and the diagonal one (lane l-1, two steps ago) arrive by a one-lane shift and the cell
 * above is its own previous value.  The column left of a strip is kept in `bnd` (score, matches per row), read 64 rows at a time and
 * overwritten by lane 63 as the strip advances (row i is read at step i and rewritten at step i+63).  Scores are the reference's
 * floats times one (all multiples of 5: exact in int); ties are broken diagonal, up, left like the traceback of :150-180. */
__global__ void __launch_bounds__(64) k_nw(const uint8_t* __restrict__ text, const uint64_t* __restrict__ off_a, const uint32_t* __restrict__ len_a,
                                           const uint64_t* __restrict__ off_b, const uint32_t* __restrict__ len_b, int2* bnd_base,
                                           const uint64_t* __restrict__ bnd_off, uint32_t* out, uint32_t npairs)
{
    const uint32_t pair = blockIdx.x, lane = threadIdx.x;
    if (pair >= npairs) return;
    const uint8_t* a = text + off_a[pair];
    const uint8_t* b = text + off_b[pair];
    const uint32_t na = len_a[pair], nb = len_b[pair];
    int2* bnd = bnd_base + bnd_off[pair];
    if (na == 0 || nb == 0) { if (lane == 0) out[pair] = 0; return; }
    for (uint32_t i = lane; i <= na; i += 64) bnd[i] = make_int2(-5 * (int)i, 0); /* column 0 */
    __syncthreads();
    int result = 0;
    for (uint32_t j0 = 0; j0 < nb; j0 += 64) {
        const uint32_t j = j0 + lane + 1; /* 1-based column of this lane */
        const bool col_ok = j <= nb;
        const uint32_t bj = col_ok ? b[j - 1] : 256u;
        int s_up = -5 * (int)j, m_up = 0;  /* cell above: row 0 to start with */
        int s_cur = 0, m_cur = 0;          /* this lane's latest cell, handed to the right-hand neighbour at the next step */
        int s_diag = 0, m_diag = 0;
        uint32_t a_cur = 0;                /* the row character travels with the wavefront */
        int2 bchunk = make_int2(0, 0);
        uint32_t achunk = 0;
        const uint32_t nsteps = na + 63;
        for (uint32_t t = 1; t <= nsteps; t++) {
            if (((t - 1) & 63u) == 0) { /* next 64 rows of the left boundary column and of a */
                const uint32_t r = t + lane;
                bchunk = r <= na ? bnd[r] : make_int2(0, 0);
                achunk = r <= na ? a[r - 1] : 257u;
            }
            int s_left = __shfl_up(s_cur, 1, 64), m_left = __shfl_up(m_cur, 1, 64);
            uint32_t a_in = (uint32_t)__shfl_up((int)a_cur, 1, 64);
            const int src = (int)((t - 1) & 63u);
            const int bs = __shfl(bchunk.x, src, 64), bm = __shfl(bchunk.y, src, 64);
            const uint32_t ba = (uint32_t)__shfl((int)achunk, src, 64);
            if (lane == 0) { s_left = bs; m_left = bm; a_in = ba; }
            a_cur = a_in;
            const int i = (int)t - (int)lane; /* row of this lane */
            if (i == 1) { s_diag = -5 * ((int)j - 1); m_diag = 0; } /* row 0 */
            if (col_ok && i >= 1 && i <= (int)na) {
                const bool eq = a_cur == bj;
                const int diag = s_diag + (eq ? 10 : -5), del = s_up - 5, ins = s_left - 5;
                const int best = max(max(diag, del), ins);
                const int m = best == diag ? m_diag + (eq ? 1 : 0) : (best == del ? m_up : m_left);
                s_cur = best; m_cur = m;
                s_up = best; m_up = m;
                if (lane == 63) bnd[i] = make_int2(best, m);
                if (i == (int)na && j == nb) result = m;
            }
            s_diag = s_left; m_diag = m_left;
        }
        __syncthreads(); /* lane 63's column is the next strip's boundary */
    }
    /* the final cell was computed by lane (nb - 1) % 64 */
    result = __shfl(result, (int)((nb - 1) & 63u), 64);
    if (lane == 0) out[pair] = (uint32_t)result;
}

/* membership scan along packed sequences: rolling k-mer per position, minimizer-blocked Bloom with the blocks of a 256-position tile
 * staged in LDS by coalesced 64-byte reads, optional exact confirmation in the ABND table */
enum { SCAN_TILE = 256 };
struct ScanTile { /* a tile's LDS */
    uint32_t blk[SCAN_TILE][16];     /* the staged Bloom blocks, one per run of positions with the same block */
    uint64_t bid[SCAN_TILE];         /* the block of each position */
    uint64_t slot_bid[SCAN_TILE];    /* the block of each slot of blk */
    uint32_t wave_cnt[SCAN_TILE / 64];
    uint64_t mh[SCAN_TILE + 32];     /* hashes of the tile's m-mers */
};
/* The front end of a tile of k_scan and k_profile, called once per tile by every thread of the workgroup (all its barriers are in here):
 * positions base .. base + 255 of a sequence of npos positions with the packed words w.  x = the thread's k-mer at base + tid (zero when
 * that position is outside the sequence), T.blk[slot] = the Bloom block of that k-mer (inside the sequence), total = blocks staged.
 * The caller puts a barrier between its last read of T.blk and the next tile */
__device__ __forceinline__ void scan_tile_stage(const Index& ix, ScanTile& T, const uint64_t* __restrict__ w, uint32_t base, uint32_t npos, Kmer& x, uint32_t& slot, uint32_t& total)
{
    const int k = ix.k, mm = ix.bloom.mm;
    const uint32_t span = (uint32_t)(k - mm);
    const uint64_t mk = kmask(k), mmask = kmask(mm);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, p = base + tid;
    const bool in_seq = p < npos;
    /* the minimizer of a k-mer is the smallest hash among its k - m + 1 m-mers and neighbouring k-mers share all but one of them: the
     * tile's m-mers are hashed once (256 + k - m of them, one or two per thread) and a k-mer takes the minimum over its window in LDS
     * (rounds 1-4: bloom_block hashed fifteen m-mers per k-mer -- the kernel was bound by those multiplications, not by its reads) */
    const uint32_t tile_k = npos - base < (uint32_t)SCAN_TILE ? npos - base : (uint32_t)SCAN_TILE, tile_m = tile_k + span;
    for (uint32_t t = tid; t < tile_m; t += SCAN_TILE) {
        const uint32_t j = base + t, sh = 2u * (j & 31u);
        uint64_t v = w[j >> 5] >> sh;
        if ((j & 31u) + (uint32_t)mm > 32u) v |= w[(j >> 5) + 1] << (64u - sh);
        T.mh[t] = bloom_mmer_hash(v & mmask, mm);
    }
    __syncthreads();
    x.f = x.r = 0;
    uint64_t b = ~0ull;
    if (in_seq) {
        x.r = le_kmer(w, p, mk) ^ (0xAAAAAAAAAAAAAAAAULL & mk);
        x.f = revcomp(x.r, k);
        uint64_t best = ~0ull;
        for (uint32_t t = 0; t <= span; t++) { const uint64_t h = T.mh[tid + t]; best = h < best ? h : best; }
        b = bloom_block_of_min(ix.bloom, best);
    }
    T.bid[tid] = b;
    __syncthreads();
    const bool leader = in_seq && (tid == 0 || T.bid[tid - 1] != b);
    const unsigned long long bal = __ballot(leader);
    const uint32_t prefix = (uint32_t)__popcll(bal & ((lane == 63u) ? ~0ull : ((2ull << lane) - 1ull)));
    if (lane == 0) T.wave_cnt[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t woff = 0;
    total = 0;
    for (uint32_t i = 0; i < SCAN_TILE / 64; i++) { if (i < wave) woff += T.wave_cnt[i]; total += T.wave_cnt[i]; }
    slot = woff + prefix - 1u; /* a follower at the start of a wave continues the last block of the previous wave */
    if (leader) T.slot_bid[slot] = b;
    __syncthreads();
    for (uint32_t i = tid; i < total * 16u; i += SCAN_TILE) T.blk[i >> 4][i & 15u] = ix.bloom.bits[T.slot_bid[i >> 4] * 16u + (i & 15u)];
    __syncthreads();
}

enum { SCAN_KMERS, SCAN_BLOOM_POSITIVE, SCAN_CONFIRMED, SCAN_BLOCKS_STAGED, SCAN_COUNTERS }; /* k_scan's counters */
__global__ void __launch_bounds__(SCAN_TILE) k_scan(Index ix, const uint64_t* __restrict__ words, const uint64_t* __restrict__ word_off,
                                                    const uint32_t* __restrict__ len, size_t nseq, int mode, uint64_t* out_bits, unsigned long long* counters)
{
    __shared__ ScanTile T;
    const int k = ix.k;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    unsigned long long n_k = 0, n_pos = 0, n_conf = 0, n_staged = 0;
    for (size_t s = blockIdx.x; s < nseq; s += gridDim.x) {
        const uint32_t L = len[s];
        if (L < (uint32_t)k) continue;
        const uint64_t* w = words + word_off[s];
        uint64_t* ob = out_bits + word_off[s];
        const uint32_t npos = L - (uint32_t)k + 1;
        for (uint32_t base = 0; base < npos; base += SCAN_TILE) {
            const bool valid = base + tid < npos;
            Kmer x;
            uint32_t slot, total;
            scan_tile_stage(ix, T, w, base, npos, x, slot, total);
            bool res = false;
            if (valid) {
                const uint64_t c = canon(x);
                res = bloom_test_block(T.blk[slot], bloom_bits(c));
                n_k++;
                n_pos += res;
                if (res && mode == 1) {
                    uint32_t lines = 0;
                    res = abundance(ix, x, lines) != 0;
                    n_conf += res;
                }
            }
            const unsigned long long rb = __ballot(res);
            if (lane == 0 && base + wave * 64u < npos) ob[(base >> 6) + wave] = rb;
            if (tid == 0) n_staged += total;
            __syncthreads();
        }
    }
    /* per-workgroup totals */
    __shared__ unsigned long long s_tot[SCAN_COUNTERS];
    if (tid < SCAN_COUNTERS) s_tot[tid] = 0;
    __syncthreads();
    atomicAdd(&s_tot[SCAN_KMERS], n_k); atomicAdd(&s_tot[SCAN_BLOOM_POSITIVE], n_pos); atomicAdd(&s_tot[SCAN_CONFIRMED], n_conf); atomicAdd(&s_tot[SCAN_BLOCKS_STAGED], n_staged);
    __syncthreads();
    if (tid < SCAN_COUNTERS && s_tot[tid]) atomicAdd(&counters[tid], s_tot[tid]);
}

/* The counter block of profile_run and of the find runs (FindStage): 64-bit slots zeroed by the run, named here for its kernels and for the
 * host's read-back alike.  Every block begins with k_profile's three; a total and a longest run are neighbours (k_profile_seq_scan writes
 * tot[0], k_profile_finish tot[1]).  The gap observers (homozygous insertions, deletions, SNPs) share slots 4-8 and name their own from 10 up;
 * the heterozygous run names its slots where they differ */
enum { CNT_POSITIONS, CNT_VALID, CNT_PRESENT, CNT_PROFILE };
enum { CNT_RUNS = 4, CNT_RUNS_LONGEST, CNT_PROFILE_SLOTS = 8 };
enum { CNT_GAPS = 4, CNT_GAPS_LONGEST, CNT_GAP_CANDIDATES, CNT_GAP_CALLS, CNT_GAPS_SEEN, CNT_FIND_SLOTS = 16 }; /* (CNT_GAPS: gaps of any kind) */
enum { CNT_HOMO_CLEAN = 10, CNT_HOMO_FUZZY, CNT_SMALL_CLEAN, CNT_SMALL_FUZZY };
enum { CNT_DEL_CLEAN = 10, CNT_DEL_FUZZY, CNT_DEL_FALLBACK };
enum { CNT_SNP_SOLO = 10 };
enum { CNT_MSNP_FULL = 11, CNT_MSNP_PARTIAL, CNT_MSNP_LONG };
enum { CNT_HET_LISTED = 4, CNT_HET_CALLS = 6, CNT_HET_CANDIDATES = 8, CNT_HET_RAW_SITES, CNT_HET_FILTERED, CNT_HET_SUPPRESSED, CNT_HET_CLEAN, CNT_HET_FUZZY, CNT_HET_SMALL };

/* profile along packed sequences: the tile of k_scan (scan_tile_stage: the tile's m-mers hashed once in LDS, Bloom blocks staged by coalesced
 * reads; then pre-filter, exact confirmation), and for the confirmed positions the abundance and the neighbour masks of k_query, packed into one
 * word per position (include/mtg_fill.h).  bad = one bit per NUCLEOTIDE that is no nucleotide (bit i % 64 of bad[word_off[s] + i / 64];
 * nullptr: none): a k-mer that covers one is invalid.  The valid and the present plane (bit layout of k_scan's output) go to vbits / pbits for
 * k_profile_count / k_profile_write.  HET: three more planes for `find` for heterozygous insertions (mtg_find_het.h): in2 / out2 = present
 * with in- / out-degree 2, br = present with a degree above 1; nothing else differs */
template <bool HET>
__global__ void __launch_bounds__(SCAN_TILE) k_profile(Index ix, const uint64_t* __restrict__ words, const uint64_t* __restrict__ word_off,
                                                       const uint32_t* __restrict__ len, size_t nseq, const uint64_t* __restrict__ bad,
                                                       const uint64_t* __restrict__ pos_off, uint32_t* out, uint64_t* vbits, uint64_t* pbits,
                                                       unsigned long long* counters, uint64_t* in2, uint64_t* out2, uint64_t* br)
{
    __shared__ ScanTile T;
    const int k = ix.k;
    const uint64_t mk1 = kmask(k - 1);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    unsigned long long n_k = 0, n_valid = 0, n_present = 0;
    for (size_t s = blockIdx.x; s < nseq; s += gridDim.x) {
        const uint32_t L = len[s];
        if (L < (uint32_t)k) continue;
        const uint64_t* w = words + word_off[s];
        const uint64_t* bw = bad ? bad + word_off[s] : nullptr;
        uint64_t* vb = vbits + word_off[s];
        uint64_t* pb = pbits + word_off[s];
        uint32_t* ow = out ? out + pos_off[s] : nullptr;
        const uint32_t npos = L - (uint32_t)k + 1;
        for (uint32_t base = 0; base < npos; base += SCAN_TILE) {
            const uint32_t p = base + tid;
            const bool in_seq = p < npos;
            Kmer x;
            uint32_t slot, total;
            scan_tile_stage(ix, T, w, base, npos, x, slot, total);
            uint32_t word = 0;
            if (in_seq) {
                const bool ok = !(bw && covers_bad(bw, p, k));
                n_k++;
                n_valid += ok;
                if (ok) {
                    word = 1u << 16;
                    if (bloom_test_block(T.blk[slot], bloom_bits(canon(x)))) {
                        uint32_t lines = 0;
                        const uint32_t a = abundance(ix, x, lines);
                        if (a) {
                            const uint32_t succ = adj_right_t(ix.adj, x, mk1, lines).out, pred = adj_left(ix, x, mk1, lines).in;
                            word |= (1u << 17) | (a > 255u ? 255u : a) | ((succ & 15u) << 8) | ((pred & 15u) << 12);
                            n_present++;
                        }
                    }
                }
                if (ow) ow[p] = word;
            }
            const unsigned long long vbal = __ballot((word >> 16) & 1u), pbal = __ballot((word >> 17) & 1u);
            if (lane == 0 && base + wave * 64u < npos) { vb[(base >> 6) + wave] = vbal; pb[(base >> 6) + wave] = pbal; }
            if (HET) { /* an absent position has empty masks */
                const int nin = popc4((word >> 12) & 15u), nout = popc4((word >> 8) & 15u);
                const unsigned long long ibal = __ballot(nin == 2), obal = __ballot(nout == 2), bbal = __ballot(nin > 1 || nout > 1);
                if (lane == 0 && base + wave * 64u < npos) {
                    const size_t at = word_off[s] + (base >> 6) + wave;
                    in2[at] = ibal; out2[at] = obal; br[at] = bbal;
                }
            }
            __syncthreads();
        }
    }
    __shared__ unsigned long long s_tot[CNT_PROFILE];
    if (tid < CNT_PROFILE) s_tot[tid] = 0;
    __syncthreads();
    atomicAdd(&s_tot[CNT_POSITIONS], n_k); atomicAdd(&s_tot[CNT_VALID], n_valid); atomicAdd(&s_tot[CNT_PRESENT], n_present);
    __syncthreads();
    if (tid < CNT_PROFILE && s_tot[tid]) atomicAdd(&counters[tid], s_tot[tid]);
}

/* the runs of absent k-mers from the two planes (mtg_profile_runs.h), in ascending (seq, start) order by two counted passes:
 * k_profile_count: runs that begin in each sequence; k_profile_seq_scan: their exclusive prefix sums (one workgroup), tot[0] = all runs;
 * k_profile_write: every word numbers the runs that begin / end in it and writes its halves of their records; k_profile_finish: end ->
 * length, tot[1] = the longest. */
enum { RUNS_BLOCK = 256 };
__device__ __forceinline__ uint32_t runs_block_sum(uint32_t v, uint32_t* s_w, uint32_t& excl)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    uint32_t x = v;
    for (int d = 1; d < 64; d <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)x, d, 64); if ((int)lane >= d) x += y; }
    __syncthreads(); /* s_w of the previous call has been read */
    if (lane == 63u) s_w[wv] = x;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t i = 0; i < RUNS_BLOCK / 64; i++) { if (i < wv) before += s_w[i]; total += s_w[i]; }
    excl = before + x - v;
    return total;
}
/* GAPS = false: the profile's runs (run_word); true: the gaps of the `find` scan (gap_word, mtg_find_gaps.h) -- the predicate is the only difference */
template <bool GAPS> MTG_DEV RunWord runs_or_gaps_word(const uint64_t* vplane, const uint64_t* pplane, uint32_t w, uint32_t npos)
{
    return GAPS ? gap_word(vplane, pplane, w, npos) : run_word(vplane, pplane, w, npos);
}
template <bool GAPS>
__global__ void __launch_bounds__(RUNS_BLOCK) k_profile_count(const uint64_t* __restrict__ vbits, const uint64_t* __restrict__ pbits, const uint64_t* __restrict__ word_off,
                                                              const uint32_t* __restrict__ len, size_t nseq, int k, uint32_t* seq_cnt)
{
    __shared__ uint32_t s_w[RUNS_BLOCK / 64];
    for (size_t s = blockIdx.x; s < nseq; s += gridDim.x) {
        const uint32_t L = len[s], npos = L < (uint32_t)k ? 0u : L - (uint32_t)k + 1u, nw = run_words(npos);
        uint32_t mine = 0;
        for (uint32_t w = threadIdx.x; w < nw; w += RUNS_BLOCK) mine += run_popc(runs_or_gaps_word<GAPS>(vbits + word_off[s], pbits + word_off[s], w, npos).first);
        uint32_t excl;
        const uint32_t total = runs_block_sum(mine, s_w, excl);
        if (threadIdx.x == 0) seq_cnt[s] = total;
    }
}
__global__ void __launch_bounds__(1024) k_profile_seq_scan(const uint32_t* __restrict__ seq_cnt, size_t nseq, uint64_t* seq_before, unsigned long long* tot)
{
    __shared__ unsigned long long wsum[16];
    __shared__ unsigned long long carry;
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    if (t == 0) carry = 0;
    __syncthreads();
    for (size_t b0 = 0; b0 < nseq; b0 += 1024) {
        const size_t i = b0 + t;
        const unsigned long long v = i < nseq ? seq_cnt[i] : 0;
        unsigned long long x = v;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)x, d, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(x >> 32), d, 64);
            if ((int)lane >= d) x += ((unsigned long long)hi << 32) | lo;
        }
        if (lane == 63) wsum[wv] = x;
        __syncthreads();
        unsigned long long before = carry;
        for (uint32_t w2 = 0; w2 < wv; w2++) before += wsum[w2];
        if (i < nseq) seq_before[i] = before + x - v;
        __syncthreads();
        if (t == 0) { unsigned long long c = carry; for (int w2 = 0; w2 < 16; w2++) c += wsum[w2]; carry = c; }
        __syncthreads();
    }
    if (t == 0) tot[0] = carry;
}
template <bool GAPS>
__global__ void __launch_bounds__(RUNS_BLOCK) k_profile_write(const uint64_t* __restrict__ vbits, const uint64_t* __restrict__ pbits, const uint64_t* __restrict__ word_off,
                                                              const uint32_t* __restrict__ len, size_t nseq, int k, const uint64_t* __restrict__ seq_before, mtg_run* runs,
                                                              uint64_t cap)
{
    __shared__ uint32_t s_w[RUNS_BLOCK / 64];
    for (size_t s = blockIdx.x; s < nseq; s += gridDim.x) {
        const uint32_t L = len[s], npos = L < (uint32_t)k ? 0u : L - (uint32_t)k + 1u, nw = run_words(npos);
        uint64_t before = seq_before[s];
        if (before >= cap) continue; /* (uniform in the workgroup) */
        for (uint32_t w0 = 0; w0 < nw; w0 += RUNS_BLOCK) {
            const uint32_t w = w0 + threadIdx.x;
            RunWord r;
            r.first = r.last = r.lflag = r.rflag = 0; r.open = 0;
            if (w < nw) r = runs_or_gaps_word<GAPS>(vbits + word_off[s], pbits + word_off[s], w, npos);
            uint32_t excl;
            const uint32_t total = runs_block_sum(run_popc(r.first), s_w, excl);
            if (w < nw) run_emit_word(r, (uint32_t)s, w, before + excl, runs, cap);
            before += total;
        }
    }
}
__global__ void __launch_bounds__(RUNS_BLOCK) k_profile_finish(mtg_run* runs, uint64_t n, unsigned long long* tot)
{
    uint32_t longest = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * RUNS_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * RUNS_BLOCK) {
        const uint32_t l = run_finish(runs[i]);
        longest = l > longest ? l : longest;
    }
    if (longest) atomicMax(&tot[1], (unsigned long long)longest);
}

/* ---- `find` over the gaps of the scan (include/mtg_fill.h: mtg_index_find_homo_sequences, mtg_index_find_del_sequences).  The gaps come from
 * k_profile_count<true> / k_profile_write<true> as mtg_run records (flags: mtg_find_gaps.h).  An Observer (HomoObserver, DelObserver, SoloObserver,
 * MultiObserver below) is one kind of call on a gap: its candidate test and which argument of the run that test takes (candidate_param), the
 * calls on the candidates (calls, run by find_gap_run) and its statistics.  An observer with at most one call per gap has a judge kernel and the
 * record of a call, and takes the rest from OneCallPerGap.
 * k_gap_mark: one thread per gap, the observer's candidate test alone -- mark[i] = the gap is a candidate; CNT_GAPS_SEEN += gaps the observers see.
 * k_mark_count / k_profile_seq_scan / k_mark_index: the indices of the non-zero marks in ascending order (counts per workgroup, their
 * exclusive prefix sums, then every workgroup numbers its own); used for the candidates and, after the judge kernel, for the calls.
 * k_gap_emit: the records of the calls: call j is candidate sel[j] */
template <typename Observer>
__global__ void __launch_bounds__(RUNS_BLOCK) k_gap_mark(const mtg_run* __restrict__ gaps, uint64_t n, int k, int cand_param, uint32_t* mark, unsigned long long* counters)
{
    const uint64_t i = (uint64_t)blockIdx.x * RUNS_BLOCK + threadIdx.x;
    bool seen = false;
    if (i < n) {
        const mtg_run g = gaps[i];
        seen = (g.flags & 2u) != 0;
        mark[i] = Observer::is_candidate(g, k, cand_param) ? 1u : 0u;
    }
    const unsigned long long bal = __ballot(seen);
    if ((threadIdx.x & 63u) == 0 && bal) atomicAdd(&counters[CNT_GAPS_SEEN], (unsigned long long)__popcll(bal));
}
template <typename Observer>
__global__ void __launch_bounds__(RUNS_BLOCK) k_gap_emit(const mtg_run* __restrict__ gaps, const uint32_t* __restrict__ cand, const uint32_t* __restrict__ res,
                                                        const uint32_t* __restrict__ sel, uint64_t n, int k, mtg_find_call* calls)
{
    const uint64_t j = (uint64_t)blockIdx.x * RUNS_BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint32_t c = sel[j];
    calls[j] = Observer::call_of(gaps[cand[c]], res[c], k);
}
__global__ void __launch_bounds__(RUNS_BLOCK) k_mark_count(const uint32_t* __restrict__ mark, uint64_t n, uint32_t* blk_cnt)
{
    __shared__ uint32_t s_w[RUNS_BLOCK / 64];
    const uint64_t i = (uint64_t)blockIdx.x * RUNS_BLOCK + threadIdx.x;
    uint32_t excl;
    const uint32_t total = runs_block_sum((i < n && mark[i]) ? 1u : 0u, s_w, excl);
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = total;
}
__global__ void __launch_bounds__(RUNS_BLOCK) k_mark_index(const uint32_t* __restrict__ mark, uint64_t n, const uint64_t* __restrict__ blk_before, uint32_t* index, uint64_t cap)
{
    __shared__ uint32_t s_w[RUNS_BLOCK / 64];
    const uint64_t i = (uint64_t)blockIdx.x * RUNS_BLOCK + threadIdx.x;
    const bool on = i < n && mark[i];
    uint32_t excl;
    runs_block_sum(on ? 1u : 0u, s_w, excl);
    const uint64_t at = blk_before[blockIdx.x] + excl;
    if (on && at < cap) index[at] = (uint32_t)i;
}

/* The micro-assembly of the insertion observers (FindSmallInsertion.hpp:57-125, FindHeteroInsertion.hpp:80-116), by one wave: the first of the 20
 * strings A, C, G, T, AA .. TT for which the first k windows of left + string + right are all solid, -1 when there is none.  lk / rk: the
 * little-endian images of the two k-mers.  Two strings at a time: lanes 0-31 the windows 0 .. k-1 for string 2 * it, lanes 32-63 those of
 * string 2 * it + 1 (k <= 32); a window is cut from the 128-bit image of the text and looked up by the path of k_query (abundance != 0).  The
 * windows behind the k-th are not looked at, as in the reference, where nothing depends on them any more; the loop leaves at the first pair
 * with a hit, the lower half before the upper.  The result is uniform in the wave */
__device__ __forceinline__ int find_micro_assembly(const Index& ix, uint64_t lk, uint64_t rk, uint32_t lane, uint32_t& lines)
{
    const int k = ix.k;
    const uint64_t mk = kmask(k), cmpl = 0xAAAAAAAAAAAAAAAAULL & mk;
    const uint32_t half = lane >> 5, j = lane & 31u;
    int found = -1;
    for (uint32_t it = 0; it < 10u && found < 0; it++) {
        const uint32_t si = 2u * it + half, n = si < 4u ? 1u : 2u;
        /* codes of A, C, G, T in that order: 0, 1, 3, 2; the first inserted nucleotide lowest */
        const uint32_t ins = si < 4u ? (0xB4u >> (2u * si)) & 3u : ((0xB4u >> (2u * ((si - 4u) >> 2))) & 3u) | (((0xB4u >> (2u * ((si - 4u) & 3u))) & 3u) << 2);
        const unsigned __int128 text = (unsigned __int128)lk | ((unsigned __int128)ins << (2 * k)) | ((unsigned __int128)rk << (2 * (k + (int)n)));
        bool solid = true;
        if (j < (uint32_t)k) {
            Kmer x;
            x.r = ((uint64_t)(text >> (2u * j)) & mk) ^ cmpl;
            x.f = revcomp(x.r, k);
            solid = abundance(ix, x, lines) != 0;
        }
        const unsigned long long bal = __ballot(solid);
        if ((uint32_t)bal == 0xFFFFFFFFu) found = (int)(2u * it);
        else if ((uint32_t)(bal >> 32) == 0xFFFFFFFFu) found = (int)(2u * it + 1u);
    }
    return found;
}

/* The observers on one candidate gap, one wave each (four to a workgroup).  Gap of L positions from `start`, first solid position behind it
 * e = start + L, r = k - 1 - L: left k-mer at start - 1 (present: an anchor), right k-mer as written at e + r, which for r > 0 must lie in
 * the sequence and hold nucleotides only.  Lane 0 / lane 1 look up outdegree(left) / indegree(k-mer at e); every observer but the small
 * clean one wants both >= 1 (FindSmallInsertion.hpp:64 has no such test: kept).  The micro-assembly is find_micro_assembly's.
 * res[c] = 0: no call; else 1 | kind << 1 | ins << 8.  One of CNT_HOMO_CLEAN .. CNT_SMALL_FUZZY += 1 per call */
enum { FIND_WAVES = 4 };
__global__ void __launch_bounds__(FIND_WAVES * 64) k_find_assemble(Index ix, const uint64_t* __restrict__ words, const uint64_t* __restrict__ word_off, const uint32_t* __restrict__ len,
                                                                   const uint64_t* __restrict__ bad, const mtg_run* __restrict__ gaps, const uint32_t* __restrict__ cand, uint64_t ncand,
                                                                   uint32_t* res, unsigned long long* counters)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t c = (uint64_t)blockIdx.x * FIND_WAVES + (threadIdx.x >> 6);
    if (c >= ncand) return; /* (uniform in the wave; the kernel has no workgroup barrier) */
    const mtg_run g = gaps[cand[c]];
    const int k = ix.k;
    const uint64_t mk = kmask(k), mk1 = kmask(k - 1), cmpl = 0xAAAAAAAAAAAAAAAAULL & mk;
    const uint64_t* w = words + word_off[g.seq];
    const uint32_t L = len[g.seq], e = g.start + g.length, r = (uint32_t)(k - 1) - g.length, rp = e + r;
    bool right_ok = true; /* r = 0: the k-mer at e, present */
    if (r) {
        right_ok = (uint64_t)rp + (uint32_t)k <= L;
        if (right_ok && bad) right_ok = !covers_bad(bad + word_off[g.seq], rp, k);
    }
    uint32_t out = 0;
    if (right_ok) {
        const uint64_t lk = le_kmer(w, g.start - 1u, mk), ek = le_kmer(w, e, mk), rk = r ? le_kmer(w, rp, mk) : ek;
        uint32_t lines = 0;
        bool mine = true;
        if (lane < 2u) {
            Kmer x;
            x.r = (lane ? ek : lk) ^ cmpl;
            x.f = revcomp(x.r, k);
            mine = lane ? adj_left(ix, x, mk1, lines).in != 0 : adj_right_t(ix.adj, x, mk1, lines).out != 0;
        }
        const bool degrees = __ballot(!mine) == 0ull;
        if (r == 0 || degrees) {
            const int found = find_micro_assembly(ix, lk, rk, lane, lines);
            if (found >= 0) out = 1u | (1u << 1) | ((uint32_t)found << 8);
            else if (degrees) out = 1u;
        }
    }
    if (lane == 0) {
        res[c] = out;
        if (out) atomicAdd(&counters[((out >> 1) & 1u) ? (r ? CNT_SMALL_FUZZY : CNT_SMALL_CLEAN) : (r ? CNT_HOMO_FUZZY : CNT_HOMO_CLEAN)], 1ull);
    }
}
/* What the observers with at most one call per gap share: their candidate test takes max_repeat, and their calls are Observer::judge, one wave
 * per candidate, then k_gap_emit<Observer> (the body stands with the stage of the find runs, further down) */
namespace { struct FindStage; }
template <typename Observer> struct OneCallPerGap {
    static int candidate_param(int max_repeat, int) { return max_repeat; }
    static int calls(FindStage& S, const FindArgs& a, const mtg_run* gaps, const uint32_t* cand, uint64_t n_cand, uint64_t* total);
};

/* the gap observer of the homozygous insertions: gap_is_candidate (mtg_find_gaps.h), k_find_assemble, kinds 0 (site) and 1 (1-2 nt) */
struct HomoObserver : OneCallPerGap<HomoObserver> {
    using Stats = mtg_find_stats;
    static MTG_DEV bool is_candidate(const mtg_run& g, int k, int max_repeat) { return gap_is_candidate(g.length, g.flags, k, max_repeat); }
    static void judge(const Index& ix, const uint64_t* words, const uint64_t* word_off, const uint32_t* len, const uint64_t* bad, const mtg_run* gaps, const uint32_t* cand, uint64_t n_cand,
                      int, uint32_t* res, unsigned long long* cnt)
    {
        hipLaunchKernelGGL(k_find_assemble, dim3((unsigned)((n_cand + FIND_WAVES - 1) / FIND_WAVES)), dim3(FIND_WAVES * 64), 0, 0, ix, words, word_off, len, bad, gaps, cand, n_cand, res, cnt);
    }
    static MTG_DEV mtg_find_call call_of(const mtg_run& g, uint32_t o, int k)
    {
        const uint32_t e = g.start + g.length, r = (uint32_t)(k - 1) - g.length, kind = (o >> 1) & 1u;
        mtg_find_call q;
        q.seq = g.seq; q.pos = kind ? e - 1u : e - 1u + r; q.kind = kind; q.repeat = r; q.left = g.start - 1u; q.right = e + r; q.ins = o >> 8;
        return q;
    }
    static void fill(Stats& st, const unsigned long long* c, uint64_t n_cand, uint64_t)
    {
        st.n_positions = c[CNT_POSITIONS]; st.n_gaps = c[CNT_GAPS_SEEN]; st.n_candidates = n_cand;
        st.n_homo_clean = c[CNT_HOMO_CLEAN]; st.n_homo_fuzzy = c[CNT_HOMO_FUZZY]; st.n_small_clean = c[CNT_SMALL_CLEAN]; st.n_small_fuzzy = c[CNT_SMALL_FUZZY];
    }
};

/* ---- `find` for homozygous deletions (include/mtg_fill.h: mtg_index_find_del_sequences; the rule: mtg_find_del.h).  The gaps are those of the
 * insertion observers, marked, listed and emitted by the same kernels (k_gap_mark, k_mark_*, k_gap_emit) for DelObserver. */
/* every k-mer of J_r = begin[0 : k - r] + end is in the graph: lane j <= k - r looks up k-mer j (Bloom filter, then the table); uniform in the wave */
__device__ __forceinline__ bool del_joined_is_solid(const Index& ix, uint64_t begin, uint64_t end, int r, uint32_t lane, uint32_t& lines)
{
    const int k = ix.k;
    bool solid = true;
    if (lane <= (uint32_t)(k - r)) {
        Kmer x;
        x.r = del_joined_kmer(begin, end, r, (int)lane, k) ^ (0xAAAAAAAAAAAAAAAAULL & kmask(k));
        x.f = revcomp(x.r, k);
        solid = bloom_test(ix.bloom, x, k) && abundance(ix, x, lines) != 0;
    }
    return __ballot(!solid) == 0ull;
}
/* The observer on one candidate gap, one wave each (four to a workgroup): both k-mers are anchors, hence in the sequence and valid.
 * res[c] = 0: no deletion; else DEL_CALLED | DEL_FALLBACK | r << 8 with the final r.  CNT_DEL_FALLBACK += 1 when J_0 held after J_r failed,
 * CNT_DEL_CLEAN / CNT_DEL_FUZZY += 1 per call */
__global__ void __launch_bounds__(FIND_WAVES * 64) k_del_judge(Index ix, const uint64_t* __restrict__ words, const uint64_t* __restrict__ word_off, const mtg_run* __restrict__ gaps,
                                                               const uint32_t* __restrict__ cand, uint64_t ncand, int max_repeat, uint32_t* res, unsigned long long* counters)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t c = (uint64_t)blockIdx.x * FIND_WAVES + (threadIdx.x >> 6);
    if (c >= ncand) return; /* (uniform in the wave; the kernel has no workgroup barrier) */
    const mtg_run g = gaps[cand[c]];
    const int k = ix.k;
    const uint64_t* w = words + word_off[g.seq];
    const uint64_t begin = del_packed_kmer(w, g.start - 1u, k), end = del_packed_kmer(w, g.start + g.length, k);
    int r = del_fuzzy_site(begin, end, k, max_repeat);
    uint32_t lines = 0;
    bool called = del_joined_is_solid(ix, begin, end, r, lane, lines), fallback = false;
    if (!called && r > 0) {
        called = fallback = del_joined_is_solid(ix, begin, end, 0, lane, lines);
        r = 0;
    }
    if (called && del_size_of(g.length, r, k) <= 0) called = false;
    if (lane == 0) {
        res[c] = called ? DEL_CALLED | (fallback ? DEL_FALLBACK : 0u) | ((uint32_t)r << DEL_REPEAT_SHIFT) : 0u;
        if (fallback) atomicAdd(&counters[CNT_DEL_FALLBACK], 1ull);
        if (called) atomicAdd(&counters[r ? CNT_DEL_FUZZY : CNT_DEL_CLEAN], 1ull);
    }
}
/* the gap observer of the homozygous deletions: gap_is_del_candidate (mtg_find_del.h), k_del_judge, kind 4 */
struct DelObserver : OneCallPerGap<DelObserver> {
    using Stats = mtg_find_del_stats;
    static MTG_DEV bool is_candidate(const mtg_run& g, int k, int max_repeat) { return gap_is_del_candidate(g.length, g.flags, k, max_repeat); }
    static void judge(const Index& ix, const uint64_t* words, const uint64_t* word_off, const uint32_t*, const uint64_t*, const mtg_run* gaps, const uint32_t* cand, uint64_t n_cand,
                      int max_repeat, uint32_t* res, unsigned long long* cnt)
    {
        hipLaunchKernelGGL(k_del_judge, dim3((unsigned)((n_cand + FIND_WAVES - 1) / FIND_WAVES)), dim3(FIND_WAVES * 64), 0, 0, ix, words, word_off, gaps, cand, n_cand, max_repeat, res, cnt);
    }
    static MTG_DEV mtg_find_call call_of(const mtg_run& g, uint32_t o, int k)
    {
        const int r = (int)(o >> DEL_REPEAT_SHIFT);
        mtg_find_call q;
        q.seq = g.seq; q.pos = del_pos_of(g.start, r, k); q.kind = 4u; q.repeat = (uint32_t)r; q.left = g.start - 1u; q.right = g.start + g.length; q.ins = (uint32_t)del_size_of(g.length, r, k);
        return q;
    }
    static void fill(Stats& st, const unsigned long long* c, uint64_t n_cand, uint64_t total)
    {
        st.n_positions = c[CNT_POSITIONS]; st.n_gaps = c[CNT_GAPS_SEEN]; st.n_candidates = n_cand;
        st.n_del_clean = c[CNT_DEL_CLEAN]; st.n_del_fuzzy = c[CNT_DEL_FUZZY]; st.n_fallback = c[CNT_DEL_FALLBACK]; st.n_calls = total;
    }
};

/* ---- `find` for isolated homozygous SNPs (include/mtg_fill.h: mtg_index_find_snp_sequences; the rule: mtg_find_snp.h).  The gaps are those of
 * the other gap observers, marked, listed and emitted by the same kernels for SoloObserver. */
/* The observer on one candidate gap, one wave each (four to a workgroup): a gap of k positions from `start`, both k-mers anchors, so the text
 * [start - 1, start + 2k) lies in the sequence and holds nucleotides only.  The at most three packed words of [start, start + 2k - 1) are
 * loaded uniformly; lane l takes window j = l % 32 (< k) of the k-mer at start + j (Bloom filter, then the table).  Two alternatives side by
 * side -- lanes 0-31 the first in A, C, T, G order, lanes 32-63 the second -- then the third in lanes 0-31, not looked at when one of the
 * first two holds: the order is fixed.  res[c] = 0: no call; else SNP_CALLED | alt << SNP_ALT_SHIFT | ref << SNP_REF_SHIFT.
 * CNT_SNP_SOLO += 1 per call */
__global__ void __launch_bounds__(FIND_WAVES * 64) k_snp_judge(Index ix, const uint64_t* __restrict__ words, const uint64_t* __restrict__ word_off, const mtg_run* __restrict__ gaps,
                                                               const uint32_t* __restrict__ cand, uint64_t ncand, uint32_t* res, unsigned long long* counters)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t c = (uint64_t)blockIdx.x * FIND_WAVES + (threadIdx.x >> 6);
    if (c >= ncand) return; /* (uniform in the wave; the kernel has no workgroup barrier) */
    const mtg_run g = gaps[cand[c]];
    const int k = ix.k;
    const uint64_t* w = words + word_off[g.seq] + (g.start >> 5);
    const uint32_t nw = snp_text_words(g.start, k), rel0 = g.start & 31u;
    const uint64_t t0 = w[0], t1 = nw > 1u ? w[1] : 0ull, t2 = nw > 2u ? w[2] : 0ull;
    const uint32_t ref = (uint32_t)(snp_text_kmer(t0, t1, t2, rel0, k) >> (2 * (k - 1))) & 3u;
    const uint32_t half = lane >> 5, j = lane & 31u;
    const bool mine = j < (uint32_t)k;
    const uint64_t km = mine ? snp_text_kmer(t0, t1, t2, rel0 + j, k) : 0ull, cmpl = 0xAAAAAAAAAAAAAAAAULL & kmask(k);
    uint32_t lines = 0;
    int alt = -1;
    for (uint32_t it = 0; it < 2u && alt < 0; it++) {
        bool solid = true;
        if (mine && 2u * it + half < 3u) {
            Kmer x;
            x.r = snp_window(km, (int)j, k, snp_alt(ref, 2u * it + half)) ^ cmpl;
            x.f = revcomp(x.r, k);
            solid = bloom_test(ix.bloom, x, k) && abundance(ix, x, lines) != 0;
        }
        const unsigned long long bal = __ballot(solid);
        if ((uint32_t)bal == 0xFFFFFFFFu) alt = (int)snp_alt(ref, 2u * it);
        else if (it == 0 && (uint32_t)(bal >> 32) == 0xFFFFFFFFu) alt = (int)snp_alt(ref, 1u);
    }
    if (lane == 0) {
        res[c] = alt >= 0 ? SNP_CALLED | ((uint32_t)alt << SNP_ALT_SHIFT) | (ref << SNP_REF_SHIFT) : 0u;
        if (alt >= 0) atomicAdd(&counters[CNT_SNP_SOLO], 1ull);
    }
}
/* the gap observer of the isolated homozygous SNPs: gap_is_snp_candidate (mtg_find_snp.h), k_snp_judge, kind 5 */
struct SoloObserver : OneCallPerGap<SoloObserver> {
    using Stats = mtg_find_snp_stats;
    static MTG_DEV bool is_candidate(const mtg_run& g, int k, int max_repeat) { return gap_is_snp_candidate(g.length, g.flags, k, max_repeat); }
    static void judge(const Index& ix, const uint64_t* words, const uint64_t* word_off, const uint32_t*, const uint64_t*, const mtg_run* gaps, const uint32_t* cand, uint64_t n_cand,
                      int, uint32_t* res, unsigned long long* cnt)
    {
        hipLaunchKernelGGL(k_snp_judge, dim3((unsigned)((n_cand + FIND_WAVES - 1) / FIND_WAVES)), dim3(FIND_WAVES * 64), 0, 0, ix, words, word_off, gaps, cand, n_cand, res, cnt);
    }
    static MTG_DEV mtg_find_call call_of(const mtg_run& g, uint32_t o, int k)
    {
        mtg_find_call q;
        q.seq = g.seq; q.pos = snp_pos_of(g.start, k); q.kind = 5u; q.repeat = 0u; q.left = g.start - 1u; q.right = g.start + g.length; q.ins = snp_ins_of(o);
        return q;
    }
    static void fill(Stats& st, const unsigned long long* c, uint64_t n_cand, uint64_t)
    {
        st.n_positions = c[CNT_POSITIONS]; st.n_gaps = c[CNT_GAPS_SEEN]; st.n_candidates = n_cand; st.n_calls = c[CNT_SNP_SOLO];
    }
};

/* ---- `find` for close homozygous SNPs (include/mtg_fill.h: mtg_index_find_msnp_sequences; the rule: mtg_find_msnp.h).  The gaps are those of
 * the other gap observers, marked and listed by the same kernels for MultiObserver; a gap makes several calls, so the middle is its own:
 * k_msnp_bound: per candidate the room for its calls, L / m (0 for a gap that is not judged); k_profile_seq_scan turns it into the slab offsets.
 * k_msnp_judge: one wave per candidate, the chain; its calls go to the gap's slab as non-zero entries, the rest of the slab stays 0.
 * FindStage::calls_tail lists the non-zero entries of all slabs in order -- ascending gap, then pos -- and k_msnp_emit writes their records.
 * k_msnp_gaps: the per-candidate records. */
__global__ void __launch_bounds__(RUNS_BLOCK) k_msnp_bound(const mtg_run* __restrict__ gaps, const uint32_t* __restrict__ cand, uint64_t ncand, int m, uint32_t* bound)
{
    const uint64_t c = (uint64_t)blockIdx.x * RUNS_BLOCK + threadIdx.x;
    if (c < ncand) bound[c] = msnp_max_calls(gaps[cand[c]].length, m);
}
/* a word of the wave's text: lane `from` (uniform) holds it; a lane beyond the text holds 0 */
__device__ __forceinline__ uint64_t msnp_lane_word(uint64_t tw, uint32_t from)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)tw, (int)from, 64), hi = (uint32_t)__shfl((int)(uint32_t)(tw >> 32), (int)from, 64);
    return ((uint64_t)hi << 32) | lo;
}
/* the leading ones of one half of a ballot (windows 0 .. 31 of an alternative; a lane at or beyond cap votes 0) */
__device__ __forceinline__ uint32_t msnp_leading(uint32_t half) { return (uint32_t)__builtin_ctzll((unsigned long long)(uint32_t)~half | (1ull << 32)); }
/* The observer on one candidate gap, one wave each (four to a workgroup): a gap of L <= 254 positions from `start`, both k-mers anchors, so
 * the text [start, start + L + k) lies in the sequence and holds nucleotides only.  Its at most MSNP_TEXT_WORDS packed words are the wave's
 * private copy, word i in a register of lane i; no other word is read, and a call changes the copy, never the input.  A step at cursor c
 * fetches the three words from (start % 32 + c) / 32 on by uniform lane reads; lane l takes window j = l % 32 (< cap) of the k-mer at
 * start + c + j (Bloom filter, then the table): lanes 0-31 the first alternative in A, C, T, G order, lanes 32-63 the second, then lanes
 * 0-31 the third -- all three counts are needed.  A count is the leading ones of its half of the ballot; winner and stop tests are
 * msnp_winner / msnp_stop, uniform in the wave.  slab[slab_off[c] ..] receives the entries (msnp_entry), out[2c] = consumed,
 * out[2c + 1] = calls.  CNT_MSNP_FULL / _PARTIAL / _LONG += 1 per gap taken whole / in part / not judged (L >= 255) */
__global__ void __launch_bounds__(FIND_WAVES * 64) k_msnp_judge(Index ix, const uint64_t* __restrict__ words, const uint64_t* __restrict__ word_off, const mtg_run* __restrict__ gaps,
                                                                const uint32_t* __restrict__ cand, uint64_t ncand, int m, const uint64_t* __restrict__ slab_off, uint32_t* slab,
                                                                uint32_t* out, unsigned long long* counters)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t c = (uint64_t)blockIdx.x * FIND_WAVES + (threadIdx.x >> 6);
    if (c >= ncand) return; /* (uniform in the wave; the kernel has no workgroup barrier) */
    const mtg_run g = gaps[cand[c]];
    const uint32_t L = g.length;
    if (!msnp_is_judged(L)) {
        if (lane == 0) { out[2 * c] = 0u; out[2 * c + 1] = 0u; atomicAdd(&counters[CNT_MSNP_LONG], 1ull); }
        return;
    }
    const int k = ix.k;
    const uint32_t nw = msnp_text_words(g.start, L, k), rel0 = g.start & 31u;
    uint64_t tw = lane < nw ? words[word_off[g.seq] + (g.start >> 5) + lane] : 0ull;
    uint32_t* entries = slab + slab_off[c];
    const uint32_t half = lane >> 5, j = lane & 31u;
    const uint64_t cmpl = 0xAAAAAAAAAAAAAAAAULL & kmask(k);
    uint32_t lines = 0, at = 0, n = 0;
    while (at != L) {
        const uint32_t rel = rel0 + at, w0 = rel >> 5, r = rel & 31u, cap = msnp_cap(L, at, k);
        const uint64_t t0 = msnp_lane_word(tw, w0), t1 = msnp_lane_word(tw, w0 + 1u), t2 = msnp_lane_word(tw, w0 + 2u);
        const uint32_t ref = (uint32_t)(snp_text_kmer(t0, t1, t2, r, k) >> (2 * (k - 1))) & 3u;
        const bool mine = j < cap;
        const uint64_t km = mine ? snp_text_kmer(t0, t1, t2, r + j, k) : 0ull;
        uint32_t f0 = 0, f1 = 0, f2 = 0;
        for (uint32_t it = 0; it < 2u; it++) {
            bool solid = false;
            if (mine && 2u * it + half < 3u) {
                Kmer x;
                x.r = snp_window(km, (int)j, k, snp_alt(ref, 2u * it + half)) ^ cmpl;
                x.f = revcomp(x.r, k);
                solid = bloom_test(ix.bloom, x, k) && abundance(ix, x, lines) != 0;
            }
            const unsigned long long bal = __ballot(solid);
            if (it == 0) { f0 = msnp_leading((uint32_t)bal); f1 = msnp_leading((uint32_t)(bal >> 32)); }
            else f2 = msnp_leading((uint32_t)bal);
        }
        uint32_t best;
        const uint32_t alt = snp_alt(ref, msnp_winner(f0, f1, f2, k, &best));
        if (msnp_stop(at, best, L, m)) break;
        if (lane == 0) entries[n] = msnp_entry(at, alt, ref);
        n++;
        const uint32_t gp = rel + (uint32_t)k - 1u;
        if (lane == (gp >> 5)) tw = msnp_substituted(tw, gp, alt);
        at += best;
    }
    if (lane == 0) {
        out[2 * c] = at; out[2 * c + 1] = n;
        if (at) atomicAdd(&counters[at == L ? CNT_MSNP_FULL : CNT_MSNP_PARTIAL], 1ull);
    }
}
/* The three counts of one step of either pass (the kernel below): lane l holds km, the k-mer of its window j = l % 32 (mine: j < cap).  Lanes
 * 0-31 the first alternative in A, C, T, G order, lanes 32-63 the second, then lanes 0-31 the third; a count is the leading ones of its
 * half of the ballot.  REV: the window replaces the k-mer's nucleotide j (msnp_rev_window), else its nucleotide k - 1 - j (snp_window) */
template <bool REV>
__device__ __forceinline__ void msnp_step_counts(const Index& ix, uint64_t km, bool mine, uint32_t j, uint32_t half, uint32_t ref, uint32_t& lines, uint32_t& f0, uint32_t& f1, uint32_t& f2)
{
    const int k = ix.k;
    const uint64_t cmpl = 0xAAAAAAAAAAAAAAAAULL & kmask(k);
    for (uint32_t it = 0; it < 2u; it++) {
        bool solid = false;
        if (mine && 2u * it + half < 3u) {
            const uint32_t a = snp_alt(ref, 2u * it + half);
            Kmer x;
            x.r = (REV ? msnp_rev_window(km, j, a) : snp_window(km, (int)j, k, a)) ^ cmpl;
            x.f = revcomp(x.r, k);
            solid = bloom_test(ix.bloom, x, k) && abundance(ix, x, lines) != 0;
        }
        const unsigned long long bal = __ballot(solid);
        if (it == 0) { f0 = msnp_leading((uint32_t)bal); f1 = msnp_leading((uint32_t)(bal >> 32)); }
        else f2 = msnp_leading((uint32_t)bal);
    }
}
/* The observer with the reverse pass (mtg_find_msnp.h: msnp_passes_chain), one wave per candidate as k_msnp_judge, which stays as it is for
 * the forward-only entries.  The private copy is the text [start - 1, start + L + k): the at most MSNP_TEXT_WORDS words from (start - 1) / 32
 * on, word i in a register of lane i; start - 1 >= 0 and start + L + k - 1 lie in the sequence (both k-mers are anchors), no other word is
 * read.  passes & 1: the forward chain as in k_msnp_judge, `start` now at rel0 + 1.  passes & 2, if msnp_rev_is_asked on what is left: the
 * reverse chain on the SAME register copy.  A step at cursor d fetches the three words that hold [q - (cap - 1), q + k) by uniform lane
 * reads; lane l takes window j = l % 32 (< cap) of the k-mer at q - j, window cap - 1 = L' - d being the left anchor's k-mer at
 * start' - 1.  Winner and stop tests are msnp_winner / msnp_stop, uniform in the wave; lane 0 appends the entry behind the forward ones, the
 * lane that holds q substitutes.  out[4c ..] = consumed, calls, consumed_rev, calls of the reverse pass.  CNT_MSNP_FULL / _PARTIAL by
 * consumed + consumed_rev, CNT_MSNP_LONG as in k_msnp_judge */
__global__ void __launch_bounds__(FIND_WAVES * 64) k_msnp_rev_judge(Index ix, const uint64_t* __restrict__ words, const uint64_t* __restrict__ word_off, const mtg_run* __restrict__ gaps,
                                                                    const uint32_t* __restrict__ cand, uint64_t ncand, int m, int passes, const uint64_t* __restrict__ slab_off, uint32_t* slab,
                                                                    uint32_t* out, unsigned long long* counters)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t c = (uint64_t)blockIdx.x * FIND_WAVES + (threadIdx.x >> 6);
    if (c >= ncand) return; /* (uniform in the wave; the kernel has no workgroup barrier) */
    const mtg_run g = gaps[cand[c]];
    const uint32_t L = g.length;
    if (!msnp_is_judged(L)) {
        if (lane == 0) { out[4 * c] = 0u; out[4 * c + 1] = 0u; out[4 * c + 2] = 0u; out[4 * c + 3] = 0u; atomicAdd(&counters[CNT_MSNP_LONG], 1ull); }
        return;
    }
    const int k = ix.k;
    const uint32_t nw = msnp_rev_text_words(g.start, L, k), rel0 = msnp_rev_rel0(g.start);
    uint64_t tw = lane < nw ? words[word_off[g.seq] + ((g.start - 1u) >> 5) + lane] : 0ull;
    uint32_t* entries = slab + slab_off[c];
    const uint32_t half = lane >> 5, j = lane & 31u;
    uint32_t lines = 0, at = 0, n = 0, d = 0, nr = 0;
    while ((passes & MSNP_PASS_FWD) && at != L) {
        const uint32_t rel = rel0 + 1u + at, w0 = rel >> 5, r = rel & 31u, cap = msnp_cap(L, at, k);
        const uint64_t t0 = msnp_lane_word(tw, w0), t1 = msnp_lane_word(tw, w0 + 1u), t2 = msnp_lane_word(tw, w0 + 2u);
        const uint32_t ref = (uint32_t)(snp_text_kmer(t0, t1, t2, r, k) >> (2 * (k - 1))) & 3u;
        const bool mine = j < cap;
        const uint64_t km = mine ? snp_text_kmer(t0, t1, t2, r + j, k) : 0ull;
        uint32_t f0 = 0, f1 = 0, f2 = 0, best;
        msnp_step_counts<false>(ix, km, mine, j, half, ref, lines, f0, f1, f2);
        const uint32_t alt = snp_alt(ref, msnp_winner(f0, f1, f2, k, &best));
        if (msnp_stop(at, best, L, m)) break;
        if (lane == 0) entries[n] = msnp_entry(at, alt, ref);
        n++;
        const uint32_t gp = rel + (uint32_t)k - 1u;
        if (lane == (gp >> 5)) tw = msnp_substituted(tw, gp, alt);
        at += best;
    }
    if ((passes & MSNP_PASS_REV) && msnp_rev_is_asked(L, at, k, m)) {
        const uint32_t left = L - at;
        while (d != left) {
            const uint32_t q = rel0 + L - d, cap = msnp_cap(left, d, k), w0 = (q - (cap - 1u)) >> 5, base = w0 << 5; /* q - base <= cap - 1 + 31 <= 62 */
            const uint64_t t0 = msnp_lane_word(tw, w0), t1 = msnp_lane_word(tw, w0 + 1u), t2 = msnp_lane_word(tw, w0 + 2u);
            const uint32_t ref = (uint32_t)snp_text_kmer(t0, t1, t2, q - base, k) & 3u;
            const bool mine = j < cap;
            const uint64_t km = mine ? snp_text_kmer(t0, t1, t2, q - j - base, k) : 0ull;
            uint32_t f0 = 0, f1 = 0, f2 = 0, best;
            msnp_step_counts<true>(ix, km, mine, j, half, ref, lines, f0, f1, f2);
            const uint32_t alt = snp_alt(ref, msnp_winner(f0, f1, f2, k, &best));
            if (msnp_stop(d, best, left, m)) break;
            if (lane == 0) entries[n + nr] = msnp_rev_entry(d, alt, ref);
            nr++;
            if (lane == (q >> 5)) tw = msnp_substituted(tw, q, alt);
            d += best;
        }
    }
    if (lane == 0) {
        out[4 * c] = at; out[4 * c + 1] = n; out[4 * c + 2] = d; out[4 * c + 3] = nr;
        if (at + d) atomicAdd(&counters[at + d == L ? CNT_MSNP_FULL : CNT_MSNP_PARTIAL], 1ull);
    }
}
/* the gap of slab entry e: the last candidate whose slab begins at or before e (a candidate without room shares its offset with the next) */
__device__ __forceinline__ uint64_t msnp_owner(const uint64_t* __restrict__ slab_off, uint64_t ncand, uint64_t e)
{
    uint64_t lo = 0, hi = ncand; /* slab_off[lo] <= e < slab_off[hi] */
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (slab_off[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}
/* the records of the calls: call j is slab entry sel[j]; kind 6, left / right the gap's two k-mers for every SNP of the gap */
__global__ void __launch_bounds__(RUNS_BLOCK) k_msnp_emit(const mtg_run* __restrict__ gaps, const uint32_t* __restrict__ cand, uint64_t ncand, const uint64_t* __restrict__ slab_off,
                                                          const uint32_t* __restrict__ slab, const uint32_t* __restrict__ sel, uint64_t n, int k, mtg_find_call* calls)
{
    const uint64_t j = (uint64_t)blockIdx.x * RUNS_BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint32_t e = sel[j], o = slab[e];
    const mtg_run g = gaps[cand[msnp_owner(slab_off, ncand, e)]];
    mtg_find_call q;
    q.seq = g.seq; q.pos = msnp_pos_of(g.start, o, k); q.kind = 6u; q.repeat = 0u; q.left = g.start - 1u; q.right = g.start + g.length; q.ins = snp_ins_of(o);
    calls[j] = q;
}
__global__ void __launch_bounds__(RUNS_BLOCK) k_msnp_gaps(const mtg_run* __restrict__ gaps, const uint32_t* __restrict__ cand, const uint32_t* __restrict__ out, uint64_t n,
                                                          mtg_find_msnp_gap* recs)
{
    const uint64_t c = (uint64_t)blockIdx.x * RUNS_BLOCK + threadIdx.x;
    if (c >= n) return;
    const mtg_run g = gaps[cand[c]];
    mtg_find_msnp_gap q;
    q.seq = g.seq; q.start = g.start; q.length = g.length; q.consumed = out[2 * c]; q.n_snps = out[2 * c + 1];
    recs[c] = q;
}
/* the same two for the entries with the reverse pass (out: four words per candidate, k_msnp_rev_judge).  A reverse entry is kind 7:
 * pos = q, left = the k-mer before the residual gap, start + consumed - 1 */
__global__ void __launch_bounds__(RUNS_BLOCK) k_msnp_rev_emit(const mtg_run* __restrict__ gaps, const uint32_t* __restrict__ cand, uint64_t ncand, const uint64_t* __restrict__ slab_off,
                                                              const uint32_t* __restrict__ slab, const uint32_t* __restrict__ out, const uint32_t* __restrict__ sel, uint64_t n, int k,
                                                              mtg_find_call* calls)
{
    const uint64_t j = (uint64_t)blockIdx.x * RUNS_BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint32_t e = sel[j], o = slab[e];
    const uint64_t c = msnp_owner(slab_off, ncand, e);
    const mtg_run g = gaps[cand[c]];
    const bool rev = msnp_entry_is_rev(o);
    mtg_find_call q;
    q.seq = g.seq; q.pos = rev ? msnp_rev_pos_of(g.start, g.length, o) : msnp_pos_of(g.start, o, k); q.kind = rev ? 7u : 6u; q.repeat = 0u;
    q.left = g.start - 1u + (rev ? out[4 * c] : 0u); q.right = g.start + g.length; q.ins = snp_ins_of(o);
    calls[j] = q;
}
__global__ void __launch_bounds__(RUNS_BLOCK) k_msnp_rev_gaps(const mtg_run* __restrict__ gaps, const uint32_t* __restrict__ cand, const uint32_t* __restrict__ out, uint64_t n,
                                                              mtg_find_msnp_rev_gap* recs)
{
    const uint64_t c = (uint64_t)blockIdx.x * RUNS_BLOCK + threadIdx.x;
    if (c >= n) return;
    const mtg_run g = gaps[cand[c]];
    mtg_find_msnp_rev_gap q;
    q.seq = g.seq; q.start = g.start; q.length = g.length; q.consumed = out[4 * c]; q.n_snps = out[4 * c + 1]; q.consumed_rev = out[4 * c + 2]; q.n_snps_rev = out[4 * c + 3];
    recs[c] = q;
}
/* the gap observer of the close homozygous SNPs: gap_is_msnp_candidate (mtg_find_msnp.h) on snp_min_val, the slab middle (calls, with the
 * stage of the find runs further down), kind 6; MultiRevObserver: the same with the passes of FindArgs, kinds 6 and 7 */
struct MultiObserver {
    using Stats = mtg_find_msnp_stats;
    static int candidate_param(int, int snp_min_val) { return snp_min_val; }
    static MTG_DEV bool is_candidate(const mtg_run& g, int k, int snp_min_val) { return gap_is_msnp_candidate(g.length, g.flags, k, snp_min_val); }
    static int calls(FindStage& S, const FindArgs& a, const mtg_run* gaps, const uint32_t* cand, uint64_t n_cand, uint64_t* total);
    static void fill(Stats& st, const unsigned long long* c, uint64_t n_cand, uint64_t total)
    {
        st.n_positions = c[CNT_POSITIONS]; st.n_gaps = c[CNT_GAPS_SEEN]; st.n_candidates = n_cand; st.n_calls = total;
        st.n_full = c[CNT_MSNP_FULL]; st.n_partial = c[CNT_MSNP_PARTIAL]; st.n_long = c[CNT_MSNP_LONG];
    }
};
struct MultiRevObserver : MultiObserver {
    static int calls(FindStage& S, const FindArgs& a, const mtg_run* gaps, const uint32_t* cand, uint64_t n_cand, uint64_t* total);
};

/* ---- `find` for heterozygous insertions (include/mtg_fill.h: mtg_index_find_het_sequences; the rule and the word-level logic: mtg_find_het.h).
 * k_profile<true> writes the planes.  k_het_count / k_profile_seq_scan / k_het_list: the candidate positions in scan order by the two counted
 * passes of the runs (popcounts per plane word).  k_het_judge: one wave per candidate, the observer as if `recent` were 0.  k_het_chain: the
 * head of every chain of raw sites accepts or drops its sites.  k_het_final: the other outcomes look back at the accepted sites; mark[c] = the
 * candidate is a call.  k_mark_* list the calls in order, k_het_emit writes their records.
 * counters (CNT_HET_*): candidates (a qualifying i exists), raw sites, refused by the branching filter, suppressed by `recent`, clean sites,
 * fuzzy sites, insertions of 1-2 nt */
__global__ void __launch_bounds__(RUNS_BLOCK) k_het_count(const uint64_t* __restrict__ vbits, const uint64_t* __restrict__ in2, const uint64_t* __restrict__ out2,
                                                          const uint64_t* __restrict__ rep, const uint64_t* __restrict__ word_off, const uint32_t* __restrict__ len, size_t nseq,
                                                          int k, int max_repeat, uint32_t* seq_cnt)
{
    __shared__ uint32_t s_w[RUNS_BLOCK / 64];
    for (size_t s = blockIdx.x; s < nseq; s += gridDim.x) {
        const uint32_t L = len[s], npos = L < (uint32_t)k ? 0u : L - (uint32_t)k + 1u, nw = run_words(npos);
        const uint64_t o = word_off[s];
        uint32_t mine = 0;
        for (uint32_t w = threadIdx.x; w < nw; w += RUNS_BLOCK) mine += run_popc(het_cand_word(vbits + o, in2 + o, out2 + o, rep ? rep + o : nullptr, w, npos, k, max_repeat));
        uint32_t excl;
        const uint32_t total = runs_block_sum(mine, s_w, excl);
        if (threadIdx.x == 0) seq_cnt[s] = total;
    }
}
__global__ void __launch_bounds__(RUNS_BLOCK) k_het_list(const uint64_t* __restrict__ vbits, const uint64_t* __restrict__ in2, const uint64_t* __restrict__ out2,
                                                         const uint64_t* __restrict__ rep, const uint64_t* __restrict__ word_off, const uint32_t* __restrict__ len, size_t nseq,
                                                         int k, int max_repeat, const uint64_t* __restrict__ seq_before, HetEntry* e, uint64_t cap)
{
    __shared__ uint32_t s_w[RUNS_BLOCK / 64];
    for (size_t s = blockIdx.x; s < nseq; s += gridDim.x) {
        const uint32_t L = len[s], npos = L < (uint32_t)k ? 0u : L - (uint32_t)k + 1u, nw = run_words(npos);
        const uint64_t o = word_off[s];
        uint64_t before = seq_before[s];
        for (uint32_t w0 = 0; w0 < nw; w0 += RUNS_BLOCK) {
            const uint32_t w = w0 + threadIdx.x;
            const uint64_t m = w < nw ? het_cand_word(vbits + o, in2 + o, out2 + o, rep ? rep + o : nullptr, w, npos, k, max_repeat) : 0ull;
            uint32_t excl;
            const uint32_t total = runs_block_sum(run_popc(m), s_w, excl);
            uint64_t at = before + excl;
            for (uint64_t x = m; x && at < cap; x &= x - 1ull, at++) { e[at].seq = (uint32_t)s; e[at].p = w * 64u + run_ctz(x); }
            before += total;
        }
    }
}
__global__ void __launch_bounds__(FIND_WAVES * 64) k_het_judge(Index ix, const uint64_t* __restrict__ words, const uint64_t* __restrict__ word_off, const uint32_t* __restrict__ len,
                                                               const uint64_t* __restrict__ bad, const uint64_t* __restrict__ vbits, const uint64_t* __restrict__ out2,
                                                               const uint64_t* __restrict__ br, const uint64_t* __restrict__ rep, HetEntry* e, uint64_t n, int max_repeat,
                                                               int branching_filter, unsigned long long* counters)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t c = (uint64_t)blockIdx.x * FIND_WAVES + (threadIdx.x >> 6);
    if (c >= n) return; /* (uniform in the wave; the kernel has no workgroup barrier) */
    const uint32_t s = e[c].seq, p = e[c].p;
    const int k = ix.k;
    const uint64_t mk = kmask(k), o = word_off[s];
    const uint64_t *w = words + o, *vp = vbits + o, *op = out2 + o, *bp = br + o, *rp = rep ? rep + o : nullptr;
    /* the first i whose history slot holds a k-mer of out-degree 2 with a suffix that is not repeated */
    int64_t hq = -1;
    bool ok = false;
    if (lane <= (uint32_t)max_repeat) {
        hq = het_history_pos(vp, (int64_t)p - k + (int64_t)lane);
        ok = hq >= 0 && het_bit(op, (uint32_t)hq) && !(rp && het_bit(rp, (uint32_t)hq + 1u));
    }
    const unsigned long long bal = __ballot(ok);
    uint32_t out = HET_NONE, i = 0, left = 0;
    int found = -1;
    if (bal) {
        i = (uint32_t)__ffsll(bal) - 1u;
        left = (uint32_t)__shfl((int)(uint32_t)hq, (int)i, 64);
        const uint32_t L = len[s], right = p + i;
        bool right_ok = (uint64_t)right + (uint32_t)k <= L;
        if (right_ok && bad) right_ok = !covers_bad(bad + o, right, k);
        if (right_ok) {
            uint32_t lines = 0;
            found = find_micro_assembly(ix, le_kmer(w, left, mk), le_kmer(w, right, mk), lane, lines);
            if (found >= 0) out = HET_INS;
            else { /* the branching k-mers among the 100 history slots before the window */
                uint32_t nb = 0;
                for (uint32_t j0 = 1; j0 <= 100u; j0 += 64u) {
                    const uint32_t j = j0 + lane;
                    bool b = false;
                    if (j <= 100u) {
                        const int64_t h = het_history_pos(vp, (int64_t)p - k - (int64_t)j);
                        b = h >= 0 && het_bit(bp, (uint32_t)h);
                    }
                    nb += (uint32_t)__popcll(__ballot(b));
                }
                out = (branching_filter < 0 || nb <= (uint32_t)branching_filter) ? HET_SITE : HET_FILTERED;
            }
        }
    }
    if (lane == 0) {
        e[c].out = out; e[c].rep = i; e[c].left = left; e[c].ins = found >= 0 ? (uint32_t)found : 0u;
        if (bal) atomicAdd(&counters[CNT_HET_CANDIDATES], 1ull);
        if (out == HET_SITE) atomicAdd(&counters[CNT_HET_RAW_SITES], 1ull);
    }
}
__global__ void __launch_bounds__(RUNS_BLOCK) k_het_chain(HetEntry* e, uint64_t n, const uint64_t* __restrict__ vbits, const uint64_t* __restrict__ word_off, int max_repeat)
{
    const uint64_t c = (uint64_t)blockIdx.x * RUNS_BLOCK + threadIdx.x;
    if (c >= n || e[c].out != HET_SITE) return;
    if (het_is_head(e, vbits, word_off, c, (uint32_t)max_repeat)) het_walk_chain(e, n, vbits, word_off, c, (uint32_t)max_repeat);
}
__global__ void __launch_bounds__(RUNS_BLOCK) k_het_final(const HetEntry* __restrict__ e, uint64_t n, const uint64_t* __restrict__ vbits, const uint64_t* __restrict__ word_off,
                                                          int max_repeat, uint32_t* mark, unsigned long long* counters)
{
    const uint64_t c = (uint64_t)blockIdx.x * RUNS_BLOCK + threadIdx.x;
    if (c >= n) return;
    const uint32_t out = e[c].out;
    uint32_t keep = 0;
    if (out == HET_SITE) {
        keep = e[c].state == HET_ACCEPTED;
        atomicAdd(&counters[keep ? (e[c].rep ? CNT_HET_FUZZY : CNT_HET_CLEAN) : CNT_HET_SUPPRESSED], 1ull);
    } else if (out != HET_NONE) {
        const bool quiet = het_suppressed(e, vbits, word_off, c, (uint32_t)max_repeat);
        keep = out == HET_INS && !quiet;
        if (out == HET_INS) atomicAdd(&counters[quiet ? CNT_HET_SUPPRESSED : CNT_HET_SMALL], 1ull);
        else if (!quiet) atomicAdd(&counters[CNT_HET_FILTERED], 1ull);
    }
    mark[c] = keep;
}
/* the records of the calls: call j is candidate sel[j] */
__global__ void __launch_bounds__(RUNS_BLOCK) k_het_emit(const HetEntry* __restrict__ e, const uint32_t* __restrict__ sel, uint64_t n, mtg_find_call* calls)
{
    const uint64_t j = (uint64_t)blockIdx.x * RUNS_BLOCK + threadIdx.x;
    if (j >= n) return;
    const HetEntry h = e[sel[j]];
    const bool site = h.out == HET_SITE;
    mtg_find_call q;
    q.seq = h.seq; q.pos = site ? h.p - 1u + h.rep : h.p - 1u; q.kind = site ? 2u : 3u; q.repeat = h.rep; q.left = h.left; q.right = h.p + h.rep; q.ins = site ? 0u : h.ins;
    calls[j] = q;
}

/* dependent chains of random line reads: the access pattern of the simple-path walk.  LINE = bytes read per step (16..128) */
template <int LINE>
__global__ void __launch_bounds__(64) k_chase(const uint64_t* __restrict__ table, uint64_t nlines, uint64_t n_chains, uint32_t chain_len, uint64_t* sink)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_chains) return;
    uint64_t x = d_splitmix64(t + 1);
    uint64_t acc = 0;
    for (uint32_t i = 0; i < chain_len; i++) {
        const uint64_t line = x % nlines;
        const U64x2* p = reinterpret_cast<const U64x2*>(table + line * (LINE / 8));
        uint64_t v = 0;
#pragma unroll
        for (int j = 0; j < LINE / 16; j++) { const U64x2 q = p[j]; v ^= q.x ^ q.y; }
        acc += v;
        x = d_splitmix64(x ^ v);
    }
    if (acc == 0x123456789ull) sink[0] = acc;
}

__global__ void k_fill_random(uint64_t* p, uint64_t nwords, uint64_t seed)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (; i < nwords; i += stride) p[i] = d_splitmix64(seed + i);
}

int query_run(const mtg_index* idx, const uint64_t* kmers, size_t n, uint32_t* abund, uint8_t* succ, uint8_t* pred, Workspace* ws)
{
    if (int rc = use_device_of(idx)) return rc;
    if (!idx || (n && !kmers)) { set_error("null argument"); return MTG_ERR_ARG; }
    if (n == 0) return MTG_OK;
    hipStream_t stream = ws ? (hipStream_t)ws->stream : nullptr;
    CallBuf d_k, d_a, d_s, d_p;
    HIP_TRY(d_k.alloc(ws, CALL_SLOT0 + 0, n * 8));
    HIP_TRY(hipMemcpyAsync(d_k.p, kmers, n * 8, hipMemcpyHostToDevice, stream));
    if (abund) HIP_TRY(d_a.alloc(ws, CALL_SLOT0 + 1, n * 4));
    if (succ) HIP_TRY(d_s.alloc(ws, CALL_SLOT0 + 2, n));
    if (pred) HIP_TRY(d_p.alloc(ws, CALL_SLOT0 + 3, n));
    const int blocks = (int)std::min<size_t>((n + 255) / 256, 256 * 16);
    hipLaunchKernelGGL(k_query, dim3(blocks), dim3(256), 0, stream, idx->dev, d_k.as<uint64_t>(), n, abund ? d_a.as<uint32_t>() : nullptr, succ ? d_s.as<uint8_t>() : nullptr,
                       pred ? d_p.as<uint8_t>() : nullptr);
    HIP_TRY(hipGetLastError());
    if (abund) HIP_TRY(hipMemcpyAsync(abund, d_a.p, n * 4, hipMemcpyDeviceToHost, stream));
    if (succ) HIP_TRY(hipMemcpyAsync(succ, d_s.p, n, hipMemcpyDeviceToHost, stream));
    if (pred) HIP_TRY(hipMemcpyAsync(pred, d_p.p, n, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return MTG_OK;
}

void* staging_host(Workspace* wsp, int slot, size_t bytes)
{
    if (!wsp || slot < 0 || slot >= Workspace::NHOST) return nullptr;
    Workspace& ws = *wsp;
    if (ws.hcap[slot] < bytes) {
        if (ws.hptr[slot]) (void)hipHostFree(ws.hptr[slot]);
        ws.hptr[slot] = nullptr;
        ws.hcap[slot] = 0;
        const size_t want = bytes + bytes / 4 + 4096;
        if (hipHostMalloc(&ws.hptr[slot], want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); ws.hptr[slot] = nullptr; return nullptr; }
        ws.hcap[slot] = want;
    }
    return ws.hptr[slot];
}


void* pinned_alloc(size_t bytes)
{
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 8, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
void pinned_free(void* p) { if (p) (void)hipHostFree(p); }
int host_register(void* p, size_t bytes)
{
    if (hipHostRegister(p, bytes, hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); set_error("cannot page-lock %zu bytes at %p", bytes, p); return MTG_ERR_ARG; }
    return MTG_OK;
}
int host_unregister(void* p) { if (hipHostUnregister(p) != hipSuccess) { (void)hipGetLastError(); set_error("%p is not page-locked", p); return MTG_ERR_ARG; } return MTG_OK; }
int device_download(const mtg_index* idx, void* host_dst, const void* dev_src, size_t bytes)
{
    if (int rc = use_device_of(idx)) return rc;
    if (bytes) HIP_TRY(hipMemcpy(host_dst, dev_src, bytes, hipMemcpyDeviceToHost));
    return MTG_OK;
}
int device_upload(const mtg_index* idx, void* dev_dst, const void* host_src, size_t bytes)
{
    if (int rc = use_device_of(idx)) return rc;
    if (bytes) HIP_TRY(hipMemcpy(dev_dst, host_src, bytes, hipMemcpyHostToDevice));
    return MTG_OK;
}

/* the text of a batch's simple sites, formatted on the device and brought to page-locked host memory (mtg_internal.h: FormatIn / FormatOut) */
int format_run(const mtg_index* idx, const FormatIn& fi, FormatOut& out)
{
    if (int rc = use_device_of(idx)) return rc;
    if (!fi.ws || !fi.ws->stream) { set_error("format_run: no batch has run on this workspace"); return MTG_ERR_ARG; }
    Workspace& ws = *fi.ws;
    const hipStream_t stream = (hipStream_t)ws.stream;
    const uint32_t n = (uint32_t)fi.n;
    out.n = n; out.n_simple = 0;
    out.bytes[0] = out.bytes[1] = out.bytes[2] = 0;
    out.complex_sites.clear();
    for (int s2 = 0; s2 < FMT_STREAMS; s2++) out.complex_off[s2].clear();
    if (n == 0) return MTG_OK;
    int slot = Workspace::SLOT_FMT0;
    auto wsbuf = [&]() { WsBuf b; b.ws = &ws; b.slot = slot++; return b; };
    WsBuf d_names = wsbuf(), d_rec = wsbuf(), d_cplx = wsbuf(), d_tot = wsbuf(), d_o0 = wsbuf(), d_o1 = wsbuf(), d_o2 = wsbuf(), d_recs_up = wsbuf();
    HIP_TRY(d_names.alloc((size_t)n * 12));
    HIP_TRY(d_rec.alloc((size_t)n * sizeof(FmtRec)));
    HIP_TRY(d_cplx.alloc((size_t)n * 28 + 64));
    HIP_TRY(d_tot.alloc(64));
    HIP_TRY(hipMemcpyAsync(d_names.p, fi.name_off, (size_t)n * 8, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync((uint8_t*)d_names.p + (size_t)n * 8, fi.name_len, (size_t)n * 4, hipMemcpyHostToDevice, stream));
    FmtArgs A;
    if (fi.device_records_whole && ws.ptr[Workspace::SLOT_RES] && ws.ptr[Workspace::SLOT_FIL]) {
        A.res = (const mtg_gap_result*)ws.ptr[Workspace::SLOT_RES];
        A.fil = (const mtg_filled*)ws.ptr[Workspace::SLOT_FIL];
    } else { /* several launches, re-run gaps, gaps the host finished: the records as the host has them go up */
        HIP_TRY(d_recs_up.alloc((size_t)n * (sizeof(mtg_gap_result) + sizeof(mtg_filled))));
        HIP_TRY(hipMemcpyAsync(d_recs_up.p, fi.res, (size_t)n * sizeof(mtg_gap_result), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync((uint8_t*)d_recs_up.p + (size_t)n * sizeof(mtg_gap_result), fi.fil, (size_t)n * sizeof(mtg_filled), hipMemcpyHostToDevice, stream));
        A.res = (const mtg_gap_result*)d_recs_up.p;
        A.fil = (const mtg_filled*)((uint8_t*)d_recs_up.p + (size_t)n * sizeof(mtg_gap_result));
    }
    const uint8_t* c = (const uint8_t*)ws.ptr[Workspace::SLOT_TEXT_BLOCK];
    A.text = (const char*)(c + FillInput::text_block_off(fi.n, fi.nt, 5));
    A.source_off = (const uint64_t*)(c + FillInput::text_block_off(fi.n, fi.nt, 0));
    A.source_len = (const uint32_t*)(c + FillInput::text_block_off(fi.n, fi.nt, 3));
    A.name_off = (const uint64_t*)d_names.p;
    A.name_len = (const uint32_t*)((uint8_t*)d_names.p + (size_t)n * 8);
    A.d_seq = (const char*)ws.ptr[Workspace::SLOT_SEQ];
    A.host_seq = (uint64_t)(uintptr_t)fi.host_seq;
    A.seq_used = fi.seq_used;
    A.host_fil = (uint64_t)(uintptr_t)fi.fil;
    A.rec = d_rec.as<FmtRec>();
    A.out[0] = A.out[1] = A.out[2] = nullptr;
    A.n = n;
    EventSet events;
    hipEvent_t e0, e1;
    HIP_TRY(events.make(e0));
    HIP_TRY(events.make(e1));
    HIP_TRY(hipEventRecord(e0, stream));
    hipLaunchKernelGGL(k_fmt_size, dim3(n), dim3(64), 0, stream, A);
    hipLaunchKernelGGL(k_fmt_scan, dim3(1), dim3(1024), 0, stream, d_rec.as<FmtRec>(), n, d_cplx.as<uint32_t>(), (uint64_t*)((uint8_t*)d_cplx.p + (((size_t)n * 4 + 7) & ~(size_t)7)), d_tot.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    unsigned long long* h_tot = (unsigned long long*)staging_host(&ws, Workspace::NHOST - 2, 64);
    if (!h_tot) { set_error("no page-locked memory"); return MTG_ERR_NOMEM; }
    HIP_TRY(hipMemcpyAsync(h_tot, d_tot.p, 40, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    WsBuf* d_o[3] = {&d_o0, &d_o1, &d_o2};
    for (int s2 = 0; s2 < FMT_STREAMS; s2++) {
        out.bytes[s2] = h_tot[s2];
        HIP_TRY(d_o[s2]->alloc((size_t)h_tot[s2] + 64));
        A.out[s2] = d_o[s2]->as<char>();
        if (out.cap[s2] < h_tot[s2] + 64) {
            pinned_free(out.text[s2]);
            out.cap[s2] = (size_t)h_tot[s2] + (size_t)h_tot[s2] / 4 + 4096;
            out.text[s2] = (char*)pinned_alloc(out.cap[s2]);
            if (!out.text[s2]) { out.cap[s2] = 0; set_error("no page-locked memory for %llu bytes of text", h_tot[s2]); return MTG_ERR_NOMEM; }
        }
    }
    out.n_simple = h_tot[3];
    const size_t nc = (size_t)h_tot[4];
    hipLaunchKernelGGL(k_fmt_write, dim3(n), dim3(64), 0, stream, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e1, stream));
    {
        CopyTurn copy_turn(idx->device);
        for (int s2 = 0; s2 < FMT_STREAMS; s2++)
            if (out.bytes[s2]) HIP_TRY(hipMemcpyAsync(out.text[s2], A.out[s2], out.bytes[s2], hipMemcpyDeviceToHost, stream));
        std::vector<uint64_t> co(3 * nc);
        out.complex_sites.resize(nc);
        if (nc) {
            HIP_TRY(hipMemcpyAsync(out.complex_sites.data(), d_cplx.p, nc * 4, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipMemcpyAsync(co.data(), (uint8_t*)d_cplx.p + (((size_t)n * 4 + 7) & ~(size_t)7), nc * 24, hipMemcpyDeviceToHost, stream));
        }
        HIP_TRY(hipStreamSynchronize(stream));
        for (int s2 = 0; s2 < FMT_STREAMS; s2++) { out.complex_off[s2].resize(nc); for (size_t i = 0; i < nc; i++) out.complex_off[s2][i] = co[3 * i + s2]; }
    }
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    out.kernel_ms = ms;
    return MTG_OK;
}

int nw_run(const mtg_index* idx, const std::vector<NwPair>& pairs, std::vector<uint32_t>& matches, Workspace* ws)
{
    (void)idx;
    if (int rc = use_device_of(idx)) return rc;
    const size_t np = pairs.size();
    matches.assign(np, 0);
    if (np == 0) return MTG_OK;
    std::vector<uint64_t> oa(np), ob(np), bo(np);
    std::vector<uint32_t> la(np), lb(np);
    uint64_t nt = 0, nbnd = 0;
    for (size_t i = 0; i < np; i++) { oa[i] = nt; nt += pairs[i].na; ob[i] = nt; nt += pairs[i].nb; la[i] = pairs[i].na; lb[i] = pairs[i].nb; bo[i] = nbnd; nbnd += (uint64_t)pairs[i].na + 1; }
    std::vector<uint8_t> text(nt + 1);
    for (size_t i = 0; i < np; i++) { memcpy(text.data() + oa[i], pairs[i].a, pairs[i].na); memcpy(text.data() + ob[i], pairs[i].b, pairs[i].nb); }
    hipStream_t stream = ws ? (hipStream_t)ws->stream : nullptr;
    CallBuf d_text, d_oa, d_ob, d_la, d_lb, d_bo, d_bnd, d_out;
    const auto up = [&](CallBuf& b, int slot, const void* src, size_t bytes) -> hipError_t {
        const hipError_t e = b.alloc(ws, CALL_SLOT0 + slot, bytes);
        if (e != hipSuccess || bytes == 0) return e;
        return hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, stream);
    };
    HIP_TRY(up(d_text, 0, text.data(), text.size())); HIP_TRY(up(d_oa, 1, oa.data(), np * 8)); HIP_TRY(up(d_ob, 2, ob.data(), np * 8)); HIP_TRY(up(d_la, 3, la.data(), np * 4));
    HIP_TRY(up(d_lb, 4, lb.data(), np * 4)); HIP_TRY(up(d_bo, 5, bo.data(), np * 8));
    HIP_TRY(d_bnd.alloc(ws, CALL_SLOT0 + 6, nbnd * sizeof(int2)));
    HIP_TRY(d_out.alloc(ws, CALL_SLOT0 + 7, np * 4));
    hipLaunchKernelGGL(k_nw, dim3((unsigned)np), dim3(64), 0, stream, d_text.as<uint8_t>(), d_oa.as<uint64_t>(), d_la.as<uint32_t>(), d_ob.as<uint64_t>(), d_lb.as<uint32_t>(),
                       d_bnd.as<int2>(), d_bo.as<uint64_t>(), d_out.as<uint32_t>(), (uint32_t)np);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(matches.data(), d_out.p, np * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return MTG_OK;
}

namespace {
/* The packed sequences of scan_run / profile_run / find_run as their kernels read them: words, word_off and len, and where
 * the run has them the bad plane, the rep plane (both of nwords words) and pos_off (one per sequence).  upload: the caller's arrays are host
 * memory and go to buffers of our own; take: they are device memory and are used as they are */
struct SeqInput {
    const uint64_t *words = nullptr, *word_off = nullptr, *bad = nullptr, *rep = nullptr, *pos_off = nullptr;
    const uint32_t* len = nullptr;
    size_t nwords = 0, nseq = 0;
    bool on_device = false;
    DevBuf d_words, d_word_off, d_len, d_bad, d_rep, d_pos_off;

    void take(const uint64_t* w, const uint64_t* off, const uint32_t* l, size_t n, const uint64_t* b = nullptr, const uint64_t* r = nullptr, const uint64_t* po = nullptr)
    {
        words = w; word_off = off; len = l; nseq = n; bad = b; rep = r; pos_off = po;
        on_device = true;
    }
    int upload(const uint64_t* w, size_t nw, const uint64_t* off, const uint32_t* l, size_t n, const uint64_t* b = nullptr, const uint64_t* r = nullptr, const uint64_t* po = nullptr)
    {
        nwords = nw; nseq = n;
        if (int rc = up(d_words, w, nw, words)) return rc;
        if (int rc = up(d_word_off, off, n, word_off)) return rc;
        if (int rc = up(d_len, l, n, len)) return rc;
        if (b) { if (int rc = up(d_bad, b, nw, bad)) return rc; }
        if (r) { if (int rc = up(d_rep, r, nw, rep)) return rc; }
        if (po) { if (int rc = up(d_pos_off, po, n, pos_off)) return rc; }
        return MTG_OK;
    }
    /* the planes take a word per 64 positions at the sequence's word offset: how many words they span.  Of device arrays the offsets and
     * lengths come to the host for that (two copies that wait for the device) */
    int plane_words(size_t* n) const
    {
        *n = nwords;
        if (!on_device) return MTG_OK;
        std::vector<uint64_t> ho(nseq);
        std::vector<uint32_t> hl(nseq);
        HIP_TRY(hipMemcpy(ho.data(), word_off, nseq * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(hl.data(), len, nseq * 4, hipMemcpyDeviceToHost));
        size_t reach = 0;
        for (size_t s = 0; s < nseq; s++) reach = std::max<size_t>(reach, (size_t)ho[s] + hl[s] / 64 + 1);
        *n = reach;
        return MTG_OK;
    }

private:
    template <typename T> static int up(DevBuf& d, const T* src, size_t count, const T*& dev)
    {
        HIP_TRY(d.alloc(count * sizeof(T)));
        HIP_TRY(hipMemcpy(d.p, src, count * sizeof(T), hipMemcpyHostToDevice));
        dev = d.as<T>();
        return MTG_OK;
    }
};

/* What the find runs (find_gap_run, find_het_run) set up and end with alike: the input, the planes (HET: five of them), the per-sequence counts,
 * the counter block and its host image c, the events of the two spans every run has, the scratch of compact() and the kernel time.  All device
 * work goes to the null stream; DESIGN.md lists it per operation */
struct FindStage {
    SeqInput in;
    DevBuf d_v, d_p, d_in2, d_out2, d_br, d_cnt, d_before, d_c, d_blk_cnt, d_blk_before, d_sel, d_calls;
    unsigned long long c[CNT_FIND_SLOTS] = {};
    EventSet events;
    hipEvent_t e_planes[2], e_tail[2];
    const mtg_index* idx = nullptr;
    size_t nseq = 0;
    int k = 0, max_repeat = 0, device_ptrs = 0;
    float ms = 0;

    unsigned long long* cnt() { return d_c.as<unsigned long long>(); }
    dim3 grid() const { return dim3((unsigned)std::min<size_t>(nseq, 256 * 16)); }
    int add_span(hipEvent_t from, hipEvent_t to) { float part = 0; HIP_TRY(hipEventElapsedTime(&part, from, to)); ms += part; return MTG_OK; }
    int read_counters() { HIP_TRY(hipMemcpy(c, d_c.p, sizeof c, hipMemcpyDeviceToHost)); return MTG_OK; }

    /* The checks, *n_calls and the statistics zeroed; then, unless there is no sequence (the caller returns), the input taken or uploaded, the
     * planes and counts allocated, the counters zeroed.  The arrays of a: FindArgs (mtg_internal.h) */
    template <typename Stats> int begin(const mtg_index* index, const FindArgs& a, bool het, Stats* st)
    {
        if (int rc = use_device_of(index)) return rc;
        if (!index || !index->dev.bloom.bits) { set_error("the index has no Bloom filter (MTG_BLOOM_BITS=0)"); return MTG_ERR_ARG; }
        *a.n_calls = 0;
        if (st) *st = Stats{};
        if (a.nseq == 0) return MTG_OK;
        idx = index; nseq = a.nseq; k = idx->dev.k; device_ptrs = a.device_ptrs;
        max_repeat = a.max_repeat > k - 2 ? k - 2 : a.max_repeat;
        if (device_ptrs) in.take(a.words, a.word_off, a.len, nseq, a.bad, a.rep);
        else if (int rc = in.upload(a.words, a.nwords, a.word_off, a.len, nseq, a.bad, a.rep)) return rc;
        size_t nwords = 0;
        if (int rc = in.plane_words(&nwords)) return rc;
        HIP_TRY(d_v.alloc(nwords * 8)); HIP_TRY(d_p.alloc(nwords * 8));
        if (het) { HIP_TRY(d_in2.alloc(nwords * 8)); HIP_TRY(d_out2.alloc(nwords * 8)); HIP_TRY(d_br.alloc(nwords * 8)); }
        HIP_TRY(d_cnt.alloc(nseq * 4)); HIP_TRY(d_before.alloc(nseq * 8));
        HIP_TRY(d_c.alloc(sizeof c));
        HIP_TRY(hipMemset(d_c.p, 0, sizeof c));
        for (hipEvent_t* e : {&e_planes[0], &e_planes[1], &e_tail[0], &e_tail[1]}) HIP_TRY(events.make(*e));
        return MTG_OK;
    }
    /* k_profile<HET>, the caller's count kernel (per sequence, into d_cnt) and their prefix sums, the total in slot `slot`: one span.  The
     * counters come back (the one wait); *total is refused from 2^32 on */
    template <bool HET, typename Count> int planes(Count launch_count, int slot, const char* what, uint64_t* total)
    {
        HIP_TRY(hipEventRecord(e_planes[0], 0));
        hipLaunchKernelGGL(k_profile<HET>, grid(), dim3(SCAN_TILE), 0, 0, idx->dev, in.words, in.word_off, in.len, nseq, in.bad, (const uint64_t*)nullptr, (uint32_t*)nullptr, d_v.as<uint64_t>(), d_p.as<uint64_t>(), cnt(),
                           d_in2.as<uint64_t>(), d_out2.as<uint64_t>(), d_br.as<uint64_t>()); /* (null unless HET) */
        launch_count();
        hipLaunchKernelGGL(k_profile_seq_scan, dim3(1), dim3(1024), 0, 0, d_cnt.as<uint32_t>(), nseq, d_before.as<uint64_t>(), cnt() + slot);
        HIP_TRY(hipEventRecord(e_planes[1], 0));
        HIP_TRY(hipGetLastError());
        if (int rc = read_counters()) return rc;
        if (int rc = add_span(e_planes[0], e_planes[1])) return rc;
        *total = c[slot];
        if (*total > 0xFFFFFFFFull) { set_error("more than 2^32 - 1 %s", what); return MTG_ERR_ARG; }
        return MTG_OK;
    }
    /* the n gaps written in (seq, start) order, the longest into CNT_GAPS_LONGEST; `from` is recorded ahead of the two kernels, the span is the caller's to end */
    int gaps(uint64_t n, DevBuf& d_gaps, hipEvent_t from)
    {
        HIP_TRY(d_gaps.alloc((size_t)n * sizeof(mtg_run)));
        HIP_TRY(hipMemset(d_gaps.p, 0, (size_t)n * sizeof(mtg_run)));
        HIP_TRY(hipEventRecord(from, 0));
        hipLaunchKernelGGL(k_profile_write<true>, grid(), dim3(RUNS_BLOCK), 0, 0, d_v.as<uint64_t>(), d_p.as<uint64_t>(), in.word_off, in.len, nseq, k, d_before.as<uint64_t>(), d_gaps.as<mtg_run>(), n);
        hipLaunchKernelGGL(k_profile_finish, dim3((unsigned)std::min<uint64_t>((n + RUNS_BLOCK - 1) / RUNS_BLOCK, 256 * 16)), dim3(RUNS_BLOCK), 0, 0, d_gaps.as<mtg_run>(), n, cnt() + CNT_GAPS);
        return MTG_OK;
    }
    /* the indices of the non-zero marks in ascending order (k_mark_count, k_profile_seq_scan, k_mark_index): *total = how many, written to
     * slot `slot` as well; index receives min(*total, cap) of them (allocated here).  Synchronises once, to read the total */
    int compact(const uint32_t* mark, uint64_t n, int slot, DevBuf& index, uint64_t cap, uint64_t* total)
    {
        const unsigned nb = (unsigned)((n + RUNS_BLOCK - 1) / RUNS_BLOCK);
        HIP_TRY(d_blk_cnt.alloc((size_t)nb * 4)); HIP_TRY(d_blk_before.alloc((size_t)nb * 8));
        hipLaunchKernelGGL(k_mark_count, dim3(nb), dim3(RUNS_BLOCK), 0, 0, mark, n, d_blk_cnt.as<uint32_t>());
        hipLaunchKernelGGL(k_profile_seq_scan, dim3(1), dim3(1024), 0, 0, d_blk_cnt.as<uint32_t>(), (size_t)nb, d_blk_before.as<uint64_t>(), cnt() + slot);
        HIP_TRY(hipGetLastError());
        unsigned long long t = 0;
        HIP_TRY(hipMemcpy(&t, cnt() + slot, 8, hipMemcpyDeviceToHost));
        *total = t;
        const uint64_t keep = std::min<uint64_t>(t, cap);
        HIP_TRY(index.alloc((size_t)keep * 4));
        if (keep) hipLaunchKernelGGL(k_mark_index, dim3(nb), dim3(RUNS_BLOCK), 0, 0, mark, n, d_blk_before.as<uint64_t>(), index.as<uint32_t>(), keep);
        HIP_TRY(hipGetLastError());
        return MTG_OK;
    }
    /* What every run ends with, the caller having recorded e_tail[0] ahead of its judging: the non-zero entries of mark[0 : n] are the calls,
     * counted into slot `slot`; emit(sel, keep, out) launches the kernel that writes the first keep = min(*total, cap) records, call j from
     * entry sel[j], into device memory; they reach `calls` (the caller's device array, or host memory by one copy).  Ends the span (end_tail) */
    template <typename Emit> int calls_tail(const uint32_t* mark, uint64_t n, int slot, mtg_find_call* calls, size_t cap, uint64_t* total, Emit emit)
    {
        if (int rc = compact(mark, n, slot, d_sel, cap, total)) return rc;
        const uint64_t keep = std::min<uint64_t>(*total, cap);
        mtg_find_call* pc = calls;
        if (keep) {
            if (!device_ptrs) { HIP_TRY(d_calls.alloc((size_t)keep * sizeof(mtg_find_call))); pc = d_calls.as<mtg_find_call>(); }
            emit(d_sel.as<uint32_t>(), keep, pc);
        }
        if (int rc = end_tail()) return rc;
        if (keep && !device_ptrs) HIP_TRY(hipMemcpy(calls, pc, (size_t)keep * sizeof(mtg_find_call), hipMemcpyDeviceToHost));
        return MTG_OK;
    }
    /* the end of the span that the caller began at e_tail[0], waited for: calls_tail's, and by itself the tail of a run that has nothing to list */
    int end_tail()
    {
        HIP_TRY(hipEventRecord(e_tail[1], 0));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventSynchronize(e_tail[1]));
        return add_span(e_tail[0], e_tail[1]);
    }
};
} // namespace

int scan_run(const mtg_index* idx, const uint64_t* words, size_t nwords, const uint64_t* word_off, const uint32_t* len, size_t nseq, int mode, uint64_t* out_bits,
             int device_ptrs, mtg_scan_stats* st)
{
    if (int rc = use_device_of(idx)) return rc;
    if (!idx || !idx->dev.bloom.bits) { set_error("the index has no Bloom filter (MTG_BLOOM_BITS=0)"); return MTG_ERR_ARG; }
    if (nseq == 0) return MTG_OK;
    SeqInput in;
    DevBuf d_b, d_c;
    uint64_t* pb = out_bits;
    if (device_ptrs) in.take(words, word_off, len, nseq); /* (no plane_words here: the device entry makes no copy and does not wait) */
    else {
        if (int rc = in.upload(words, nwords, word_off, len, nseq)) return rc;
        HIP_TRY(d_b.alloc(nwords * 8));
        HIP_TRY(hipMemset(d_b.p, 0, nwords * 8));
        pb = d_b.as<uint64_t>();
    }
    HIP_TRY(d_c.alloc(SCAN_COUNTERS * 8));
    HIP_TRY(hipMemset(d_c.p, 0, SCAN_COUNTERS * 8));
    EventSet events;
    hipEvent_t e0, e1;
    HIP_TRY(events.make(e0)); HIP_TRY(events.make(e1));
    HIP_TRY(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(k_scan, dim3((unsigned)std::min<size_t>(nseq, 256 * 16)), dim3(SCAN_TILE), 0, 0, idx->dev, in.words, in.word_off, in.len, nseq, mode, pb, d_c.as<unsigned long long>());
    HIP_TRY(hipEventRecord(e1, 0));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    unsigned long long c[SCAN_COUNTERS];
    HIP_TRY(hipMemcpy(c, d_c.p, SCAN_COUNTERS * 8, hipMemcpyDeviceToHost));
    if (!device_ptrs) HIP_TRY(hipMemcpy(out_bits, pb, nwords * 8, hipMemcpyDeviceToHost));
    if (st) { st->n_kmers = c[SCAN_KMERS]; st->bloom_positive = c[SCAN_BLOOM_POSITIVE]; st->confirmed = c[SCAN_CONFIRMED]; st->blocks_staged = c[SCAN_BLOCKS_STAGED]; st->kernel_ms = ms; }
    return MTG_OK;
}

/* profile over packed sequences (mtg_index_profile_sequences / _packed_device).  device_ptrs = 0: words / word_off / len / bad / pos_off are
 * host arrays, out (npos_total words, or nullptr) and runs host memory; 1: all of them device memory (nwords, npos_total unused) */
int profile_run(const mtg_index* idx, const uint64_t* words, size_t nwords, const uint64_t* word_off, const uint32_t* len, size_t nseq, const uint64_t* bad,
                const uint64_t* pos_off, uint64_t npos_total, uint32_t* out, mtg_run* runs, size_t runs_cap, size_t* n_runs, int device_ptrs, mtg_profile_stats* st)
{
    if (int rc = use_device_of(idx)) return rc;
    if (!idx || !idx->dev.bloom.bits) { set_error("the index has no Bloom filter (MTG_BLOOM_BITS=0)"); return MTG_ERR_ARG; }
    *n_runs = 0;
    if (st) *st = mtg_profile_stats{};
    if (nseq == 0) return MTG_OK;
    const int k = idx->dev.k;
    SeqInput in;
    DevBuf d_out, d_v, d_p, d_cnt, d_before, d_c, d_runs;
    uint32_t* pout = out;
    if (device_ptrs) in.take(words, word_off, len, nseq, bad, nullptr, pos_off);
    else {
        if (int rc = in.upload(words, nwords, word_off, len, nseq, bad, nullptr, out ? pos_off : nullptr)) return rc;
        if (out) { HIP_TRY(d_out.alloc(npos_total * 4)); pout = d_out.as<uint32_t>(); }
    }
    if (int rc = in.plane_words(&nwords)) return rc;
    HIP_TRY(d_v.alloc(nwords * 8)); HIP_TRY(d_p.alloc(nwords * 8));
    HIP_TRY(d_cnt.alloc(nseq * 4)); HIP_TRY(d_before.alloc(nseq * 8));
    HIP_TRY(d_c.alloc(CNT_PROFILE_SLOTS * 8));
    HIP_TRY(hipMemset(d_c.p, 0, CNT_PROFILE_SLOTS * 8));
    unsigned long long* cnt = d_c.as<unsigned long long>();
    EventSet events;
    hipEvent_t e0, e1, e2, e3;
    HIP_TRY(events.make(e0)); HIP_TRY(events.make(e1)); HIP_TRY(events.make(e2)); HIP_TRY(events.make(e3));
    const dim3 grid((unsigned)std::min<size_t>(nseq, 256 * 16));
    HIP_TRY(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(k_profile<false>, grid, dim3(SCAN_TILE), 0, 0, idx->dev, in.words, in.word_off, in.len, nseq, in.bad, in.pos_off, pout, d_v.as<uint64_t>(), d_p.as<uint64_t>(), cnt, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr);
    hipLaunchKernelGGL(k_profile_count<false>, grid, dim3(RUNS_BLOCK), 0, 0, d_v.as<uint64_t>(), d_p.as<uint64_t>(), in.word_off, in.len, nseq, k, d_cnt.as<uint32_t>());
    hipLaunchKernelGGL(k_profile_seq_scan, dim3(1), dim3(1024), 0, 0, d_cnt.as<uint32_t>(), nseq, d_before.as<uint64_t>(), cnt + CNT_RUNS);
    HIP_TRY(hipEventRecord(e1, 0));
    HIP_TRY(hipGetLastError());
    unsigned long long c[CNT_PROFILE_SLOTS];
    HIP_TRY(hipMemcpy(c, d_c.p, sizeof c, hipMemcpyDeviceToHost));
    const uint64_t total = c[CNT_RUNS];
    /* every run is written (the longest one may lie past runs_cap): into the caller's device array when it holds them all, else into one of our own */
    mtg_run* pr = runs;
    if (!device_ptrs || total > runs_cap) { HIP_TRY(d_runs.alloc((size_t)total * sizeof(mtg_run))); pr = d_runs.as<mtg_run>(); }
    float ms0 = 0, ms1 = 0;
    if (total) {
        HIP_TRY(hipMemset(pr, 0, (size_t)total * sizeof(mtg_run)));
        HIP_TRY(hipEventRecord(e2, 0));
        hipLaunchKernelGGL(k_profile_write<false>, grid, dim3(RUNS_BLOCK), 0, 0, d_v.as<uint64_t>(), d_p.as<uint64_t>(), in.word_off, in.len, nseq, k, d_before.as<uint64_t>(), pr, total);
        hipLaunchKernelGGL(k_profile_finish, dim3((unsigned)std::min<uint64_t>((total + RUNS_BLOCK - 1) / RUNS_BLOCK, 256 * 16)), dim3(RUNS_BLOCK), 0, 0, pr, total, cnt + CNT_RUNS);
        HIP_TRY(hipEventRecord(e3, 0));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventSynchronize(e3));
        HIP_TRY(hipEventElapsedTime(&ms1, e2, e3));
        HIP_TRY(hipMemcpy(c, d_c.p, sizeof c, hipMemcpyDeviceToHost));
        const size_t ncopy = (size_t)std::min<uint64_t>(total, runs_cap);
        if (ncopy && pr != runs) HIP_TRY(hipMemcpy(runs, pr, ncopy * sizeof(mtg_run), device_ptrs ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    }
    HIP_TRY(hipEventElapsedTime(&ms0, e0, e1));
    if (!device_ptrs && out) HIP_TRY(hipMemcpy(out, pout, npos_total * 4, hipMemcpyDeviceToHost));
    *n_runs = (size_t)total;
    if (st) { st->n_positions = c[CNT_POSITIONS]; st->n_valid = c[CNT_VALID]; st->n_present = c[CNT_PRESENT]; st->n_runs = total; st->longest_run = total ? c[CNT_RUNS_LONGEST] : 0; st->kernel_ms = (double)ms0 + (double)ms1; }
    return MTG_OK;
}

/* The calls of the observers that make at most one call per gap (HomoObserver, DelObserver, SoloObserver): a result word per candidate, the
 * observer's judge kernel, one wave per candidate, and the calls -- the non-zero results -- listed in order and written by k_gap_emit */
template <typename Observer>
int OneCallPerGap<Observer>::calls(FindStage& S, const FindArgs& a, const mtg_run* gaps, const uint32_t* cand, uint64_t n_cand, uint64_t* total)
{
    const SeqInput& in = S.in;
    DevBuf d_res;
    HIP_TRY(d_res.alloc((size_t)n_cand * 4));
    HIP_TRY(hipEventRecord(S.e_tail[0], 0));
    Observer::judge(S.idx->dev, in.words, in.word_off, in.len, in.bad, gaps, cand, n_cand, S.max_repeat, d_res.as<uint32_t>(), S.cnt());
    return S.calls_tail(d_res.as<uint32_t>(), n_cand, CNT_GAP_CALLS, a.calls, a.cap, total, [&](const uint32_t* sel, uint64_t keep, mtg_find_call* out) {
        hipLaunchKernelGGL(k_gap_emit<Observer>, dim3((unsigned)((keep + RUNS_BLOCK - 1) / RUNS_BLOCK)), dim3(RUNS_BLOCK), 0, 0, gaps, cand, d_res.as<uint32_t>(), sel, keep, S.k, out);
    });
}

/* The multi-SNP observer's calls, several per gap: a slab of L / m entries per candidate; the chain, one wave per candidate; the per-candidate
 * records (the first a.gap_cap of them, where a.gap_recs is given); the calls listed from the slabs and written.  Without a slab -- every
 * candidate unjudged -- there is nothing to list, and the span ends by end_tail.  REV: the entries with the reverse pass -- k_msnp_rev_judge
 * on a.passes, four result words per candidate, records of mtg_find_msnp_rev_gap */
template <bool REV>
static int msnp_calls(FindStage& S, const FindArgs& a, const mtg_run* gaps, const uint32_t* cand, uint64_t n_cand, uint64_t* total)
{
    using Rec = typename std::conditional<REV, mtg_find_msnp_rev_gap, mtg_find_msnp_gap>::type;
    const SeqInput& in = S.in;
    DevBuf d_bound, d_slab_off, d_slab, d_out, d_recs;
    const unsigned nb = (unsigned)((n_cand + RUNS_BLOCK - 1) / RUNS_BLOCK), judge_blocks = (unsigned)((n_cand + FIND_WAVES - 1) / FIND_WAVES);
    HIP_TRY(d_bound.alloc((size_t)n_cand * 4)); HIP_TRY(d_slab_off.alloc((size_t)n_cand * 8)); HIP_TRY(d_out.alloc((size_t)n_cand * (REV ? 16 : 8)));
    HIP_TRY(hipEventRecord(S.e_tail[0], 0));
    hipLaunchKernelGGL(k_msnp_bound, dim3(nb), dim3(RUNS_BLOCK), 0, 0, gaps, cand, n_cand, a.snp_min_val, d_bound.as<uint32_t>());
    hipLaunchKernelGGL(k_profile_seq_scan, dim3(1), dim3(1024), 0, 0, d_bound.as<uint32_t>(), (size_t)n_cand, d_slab_off.as<uint64_t>(), S.cnt() + CNT_GAP_CALLS);
    HIP_TRY(hipGetLastError());
    unsigned long long n_slab = 0;
    HIP_TRY(hipMemcpy(&n_slab, S.cnt() + CNT_GAP_CALLS, 8, hipMemcpyDeviceToHost));
    if (n_slab > 0xFFFFFFFFull) { set_error("more than 2^32 - 1 possible SNPs in the candidate gaps"); return MTG_ERR_ARG; }
    HIP_TRY(d_slab.alloc((size_t)n_slab * 4));
    if (n_slab) HIP_TRY(hipMemsetAsync(d_slab.p, 0, (size_t)n_slab * 4, 0));
    if constexpr (REV)
        hipLaunchKernelGGL(k_msnp_rev_judge, dim3(judge_blocks), dim3(FIND_WAVES * 64), 0, 0, S.idx->dev, in.words, in.word_off, gaps, cand, n_cand, a.snp_min_val, a.passes,
                           d_slab_off.as<uint64_t>(), d_slab.as<uint32_t>(), d_out.as<uint32_t>(), S.cnt());
    else
        hipLaunchKernelGGL(k_msnp_judge, dim3(judge_blocks), dim3(FIND_WAVES * 64), 0, 0, S.idx->dev, in.words, in.word_off, gaps, cand, n_cand, a.snp_min_val,
                           d_slab_off.as<uint64_t>(), d_slab.as<uint32_t>(), d_out.as<uint32_t>(), S.cnt());
    const uint64_t keep_recs = a.gap_recs ? std::min<uint64_t>(n_cand, a.gap_cap) : 0;
    Rec* pr = static_cast<Rec*>(a.gap_recs);
    if (keep_recs) {
        if (!a.device_ptrs) { HIP_TRY(d_recs.alloc((size_t)keep_recs * sizeof(Rec))); pr = d_recs.as<Rec>(); }
        const dim3 rec_blocks((unsigned)((keep_recs + RUNS_BLOCK - 1) / RUNS_BLOCK));
        if constexpr (REV) hipLaunchKernelGGL(k_msnp_rev_gaps, rec_blocks, dim3(RUNS_BLOCK), 0, 0, gaps, cand, d_out.as<uint32_t>(), keep_recs, pr);
        else hipLaunchKernelGGL(k_msnp_gaps, rec_blocks, dim3(RUNS_BLOCK), 0, 0, gaps, cand, d_out.as<uint32_t>(), keep_recs, pr);
    }
    if (n_slab) {
        if (int rc = S.calls_tail(d_slab.as<uint32_t>(), n_slab, CNT_GAP_CALLS, a.calls, a.cap, total, [&](const uint32_t* sel, uint64_t keep, mtg_find_call* out) {
                const dim3 emit_blocks((unsigned)((keep + RUNS_BLOCK - 1) / RUNS_BLOCK));
                if constexpr (REV)
                    hipLaunchKernelGGL(k_msnp_rev_emit, emit_blocks, dim3(RUNS_BLOCK), 0, 0, gaps, cand, n_cand, d_slab_off.as<uint64_t>(), d_slab.as<uint32_t>(), d_out.as<uint32_t>(), sel, keep,
                                       S.k, out);
                else
                    hipLaunchKernelGGL(k_msnp_emit, emit_blocks, dim3(RUNS_BLOCK), 0, 0, gaps, cand, n_cand, d_slab_off.as<uint64_t>(), d_slab.as<uint32_t>(), sel, keep, S.k, out);
            })) return rc;
    } else if (int rc = S.end_tail()) return rc;
    if (keep_recs && !a.device_ptrs) HIP_TRY(hipMemcpy(a.gap_recs, pr, (size_t)keep_recs * sizeof(Rec), hipMemcpyDeviceToHost));
    return MTG_OK;
}
int MultiObserver::calls(FindStage& S, const FindArgs& a, const mtg_run* gaps, const uint32_t* cand, uint64_t n_cand, uint64_t* total) { return msnp_calls<false>(S, a, gaps, cand, n_cand, total); }
int MultiRevObserver::calls(FindStage& S, const FindArgs& a, const mtg_run* gaps, const uint32_t* cand, uint64_t n_cand, uint64_t* total) { return msnp_calls<true>(S, a, gaps, cand, n_cand, total); }

/* `find` by a gap observer over packed sequences: what all of them share.  Between "there are candidates" and "the calls are written" the
 * observer is on its own (Observer::calls) */
template <typename Observer>
static int find_gap_run(const mtg_index* idx, const FindArgs& a, typename Observer::Stats* st)
{
    FindStage S;
    if (a.n_gap_recs) *a.n_gap_recs = 0;
    if (int rc = S.begin(idx, a, false, st); rc || a.nseq == 0) return rc;
    const int k = S.k;
    const SeqInput& in = S.in;
    DevBuf d_gaps, d_mark, d_cand;
    hipEvent_t e_gaps[2];
    HIP_TRY(S.events.make(e_gaps[0])); HIP_TRY(S.events.make(e_gaps[1]));
    uint64_t n_gaps_all = 0, n_cand = 0, total = 0;
    /* 1. the planes, the gaps counted */
    if (int rc = S.planes<false>([&] { hipLaunchKernelGGL(k_profile_count<true>, S.grid(), dim3(RUNS_BLOCK), 0, 0, S.d_v.as<uint64_t>(), S.d_p.as<uint64_t>(), in.word_off, in.len, S.nseq, k, S.d_cnt.as<uint32_t>()); },
                                 CNT_GAPS, "gaps", &n_gaps_all)) return rc;
    if (n_gaps_all) {
        /* 2. the gaps written, the candidates marked and listed in order */
        HIP_TRY(d_mark.alloc((size_t)n_gaps_all * 4));
        if (int rc = S.gaps(n_gaps_all, d_gaps, e_gaps[0])) return rc;
        hipLaunchKernelGGL(k_gap_mark<Observer>, dim3((unsigned)((n_gaps_all + RUNS_BLOCK - 1) / RUNS_BLOCK)), dim3(RUNS_BLOCK), 0, 0, d_gaps.as<mtg_run>(), n_gaps_all, k,
                           Observer::candidate_param(S.max_repeat, a.snp_min_val), d_mark.as<uint32_t>(), S.cnt());
        if (int rc = S.compact(d_mark.as<uint32_t>(), n_gaps_all, CNT_GAP_CANDIDATES, d_cand, ~0ull, &n_cand)) return rc;
        HIP_TRY(hipEventRecord(e_gaps[1], 0));
    }
    /* 3. the observer on the candidates: the calls listed in order and written */
    if (n_cand) { if (int rc = Observer::calls(S, a, d_gaps.as<mtg_run>(), d_cand.as<uint32_t>(), n_cand, &total)) return rc; }
    if (n_gaps_all) {
        HIP_TRY(hipEventSynchronize(e_gaps[1]));
        if (int rc = S.add_span(e_gaps[0], e_gaps[1])) return rc;
    }
    if (int rc = S.read_counters()) return rc;
    *a.n_calls = (size_t)total;
    if (a.n_gap_recs) *a.n_gap_recs = (size_t)n_cand;
    if (st) { Observer::fill(*st, S.c, n_cand, total); st->kernel_ms = (double)S.ms; }
    return MTG_OK;
}

/* `find` for heterozygous insertions over packed sequences (mtg_index_find_het_sequences / _packed_device): no gaps, a run of its own on the
 * stage.  Beyond the input: six planes of a bit per position and one HetEntry per candidate */
static int find_het_run(const mtg_index* idx, const FindArgs& a, mtg_find_het_stats* st)
{
    FindStage S;
    if (int rc = S.begin(idx, a, true, st); rc || a.nseq == 0) return rc;
    const int k = S.k, max_repeat = S.max_repeat;
    const size_t nseq = S.nseq;
    const SeqInput& in = S.in;
    DevBuf d_e, d_mark;
    const dim3 grid = S.grid();
    unsigned long long* cnt = S.cnt();
    uint64_t *const d_v = S.d_v.as<uint64_t>(), *const d_in2 = S.d_in2.as<uint64_t>(), *const d_out2 = S.d_out2.as<uint64_t>(), *const d_br = S.d_br.as<uint64_t>();
    uint64_t n_cand = 0, total = 0;
    /* 1. the planes, the candidates counted */
    if (int rc = S.planes<true>([&] { hipLaunchKernelGGL(k_het_count, grid, dim3(RUNS_BLOCK), 0, 0, d_v, d_in2, d_out2, in.rep, in.word_off, in.len, nseq, k, max_repeat, S.d_cnt.as<uint32_t>()); },
                                CNT_HET_LISTED, "candidates", &n_cand)) return rc;
    if (n_cand) {
        /* 2. the candidates listed and judged, the chains resolved, the calls listed in order and written */
        HIP_TRY(d_e.alloc((size_t)n_cand * sizeof(HetEntry)));
        HIP_TRY(hipMemset(d_e.p, 0, (size_t)n_cand * sizeof(HetEntry)));
        HIP_TRY(d_mark.alloc((size_t)n_cand * 4));
        const unsigned cb = (unsigned)((n_cand + RUNS_BLOCK - 1) / RUNS_BLOCK);
        HIP_TRY(hipEventRecord(S.e_tail[0], 0));
        hipLaunchKernelGGL(k_het_list, grid, dim3(RUNS_BLOCK), 0, 0, d_v, d_in2, d_out2, in.rep, in.word_off, in.len, nseq, k, max_repeat, S.d_before.as<uint64_t>(), d_e.as<HetEntry>(), n_cand);
        hipLaunchKernelGGL(k_het_judge, dim3((unsigned)((n_cand + FIND_WAVES - 1) / FIND_WAVES)), dim3(FIND_WAVES * 64), 0, 0, idx->dev, in.words, in.word_off, in.len, in.bad, d_v, d_out2, d_br, in.rep,
                           d_e.as<HetEntry>(), n_cand, max_repeat, a.branching_filter, cnt);
        hipLaunchKernelGGL(k_het_chain, dim3(cb), dim3(RUNS_BLOCK), 0, 0, d_e.as<HetEntry>(), n_cand, d_v, in.word_off, max_repeat);
        hipLaunchKernelGGL(k_het_final, dim3(cb), dim3(RUNS_BLOCK), 0, 0, d_e.as<HetEntry>(), n_cand, d_v, in.word_off, max_repeat, d_mark.as<uint32_t>(), cnt);
        if (int rc = S.calls_tail(d_mark.as<uint32_t>(), n_cand, CNT_HET_CALLS, a.calls, a.cap, &total, [&](const uint32_t* sel, uint64_t keep, mtg_find_call* out) {
                hipLaunchKernelGGL(k_het_emit, dim3((unsigned)((keep + RUNS_BLOCK - 1) / RUNS_BLOCK)), dim3(RUNS_BLOCK), 0, 0, d_e.as<HetEntry>(), sel, keep, out);
            })) return rc;
        if (int rc = S.read_counters()) return rc;
    }
    *a.n_calls = (size_t)total;
    if (st) {
        const unsigned long long* c = S.c;
        st->n_positions = c[CNT_POSITIONS]; st->n_candidates = c[CNT_HET_CANDIDATES]; st->n_raw_sites = c[CNT_HET_RAW_SITES]; st->n_filtered = c[CNT_HET_FILTERED]; st->n_suppressed = c[CNT_HET_SUPPRESSED];
        st->n_het_clean = c[CNT_HET_CLEAN]; st->n_het_fuzzy = c[CNT_HET_FUZZY]; st->n_het_small = c[CNT_HET_SMALL];
        st->kernel_ms = (double)S.ms;
    }
    return MTG_OK;
}

/* The one run entry behind the twelve find entries of the ABI; the only place where the statistics pointer gets its type back: the layer's run
 * says which */
template <typename Stats>
static int find_run_as(int (*run)(const mtg_index*, const FindArgs&, Stats*), const mtg_index* idx, const FindArgs& a, void* stats)
{
    return run(idx, a, static_cast<Stats*>(stats));
}
int find_run(const mtg_index* idx, FindLayer layer, const FindArgs& args, void* stats)
{
    switch (layer) {
        case FIND_HOMO: return find_run_as(find_gap_run<HomoObserver>, idx, args, stats);
        case FIND_DEL: return find_run_as(find_gap_run<DelObserver>, idx, args, stats);
        case FIND_SNP: return find_run_as(find_gap_run<SoloObserver>, idx, args, stats);
        case FIND_MSNP: return find_run_as(find_gap_run<MultiObserver>, idx, args, stats);
        case FIND_MSNP_REV: return find_run_as(find_gap_run<MultiRevObserver>, idx, args, stats);
        case FIND_HET: return find_run_as(find_het_run, idx, args, stats);
    }
    set_error("invalid argument");
    return MTG_ERR_ARG;
}

int bench_random_lines(uint64_t table_bytes, uint64_t n_chains, uint32_t chain_len, uint32_t line_bytes, double* ms_out, double* gbps)
{
    if (int rc = ensure_device()) return rc;
    if (line_bytes != 16 && line_bytes != 32 && line_bytes != 64 && line_bytes != 128) { set_error("line_bytes must be 16, 32, 64 or 128"); return MTG_ERR_ARG; }
    const uint64_t nlines = table_bytes / line_bytes;
    if (nlines == 0 || n_chains == 0 || chain_len == 0) { set_error("invalid argument"); return MTG_ERR_ARG; }
    DevBuf tab, sink;
    HIP_TRY(tab.alloc(nlines * line_bytes));
    HIP_TRY(sink.alloc(8));
    hipLaunchKernelGGL(k_fill_random, dim3(256 * 16), dim3(256), 0, 0, tab.as<uint64_t>(), nlines * (line_bytes / 8), 12345ull);
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    const uint32_t blocks = (uint32_t)((n_chains + 63) / 64);
    auto launch = [&](uint32_t len) {
        switch (line_bytes) {
            case 16: hipLaunchKernelGGL(k_chase<16>, dim3(blocks), dim3(64), 0, 0, tab.as<uint64_t>(), nlines, n_chains, len, sink.as<uint64_t>()); break;
            case 32: hipLaunchKernelGGL(k_chase<32>, dim3(blocks), dim3(64), 0, 0, tab.as<uint64_t>(), nlines, n_chains, len, sink.as<uint64_t>()); break;
            case 64: hipLaunchKernelGGL(k_chase<64>, dim3(blocks), dim3(64), 0, 0, tab.as<uint64_t>(), nlines, n_chains, len, sink.as<uint64_t>()); break;
            default: hipLaunchKernelGGL(k_chase<128>, dim3(blocks), dim3(64), 0, 0, tab.as<uint64_t>(), nlines, n_chains, len, sink.as<uint64_t>()); break;
        }
    };
    launch(std::min<uint32_t>(chain_len, 64));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipEventRecord(e0, 0));
    launch(chain_len);
    HIP_TRY(hipEventRecord(e1, 0));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (ms_out) *ms_out = ms;
    if (gbps) *gbps = (double)n_chains * chain_len * (double)line_bytes / (ms * 1e-3) / 1e9;
    return MTG_OK;
}

} // namespace mtgi

/* ------------------------------------------------------------------------------------------------ C ABI (device side) */
namespace mtgi {
int index_from_kmers(const uint64_t*, const uint32_t*, size_t, int, mtg_index**);
int index_from_packed_device(const uint64_t*, const uint64_t*, const uint32_t*, size_t, uint64_t, int, uint32_t, uint32_t, mtg_index**);
int index_replicate(const mtg_index*, int, mtg_index**);
void index_release(mtg_index*);
int bench_random_lines(uint64_t, uint64_t, uint32_t, uint32_t, double*, double*);
}

extern "C" {

const char* mtg_last_error(void) { return mtgi::g_err; }
int mtg_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
int mtg_set_device(int device)
{
    if (hipSetDevice(device) != hipSuccess) { mtgi::set_error("hipSetDevice(%d) failed", device); return MTG_ERR_NO_DEVICE; }
    return MTG_OK;
}
int mtg_index_create_from_kmers(const uint64_t* canon_kmers, const uint32_t* abundance, size_t n, int k, mtg_index** out)
{
    return mtgi::index_from_kmers(canon_kmers, abundance, n, k, out);
}
int mtg_index_create_from_packed_device(const uint64_t* d_words, const uint64_t* d_word_off, const uint32_t* d_len, size_t nseq, uint64_t ub, int k,
                                        uint32_t abund_lo, uint32_t abund_span, mtg_index** out)
{
    return mtgi::index_from_packed_device(d_words, d_word_off, d_len, nseq, ub, k, abund_lo, abund_span, out);
}
void mtg_index_free(mtg_index* idx) { mtgi::index_release(idx); }
int mtg_index_replicate(const mtg_index* idx, int device, mtg_index** out) { return mtgi::index_replicate(idx, device, out); }
int mtg_index_get_info(const mtg_index* idx, mtg_index_info* info)
{
    if (!idx || !info) { mtgi::set_error("null argument"); return MTG_ERR_ARG; }
    *info = idx->info;
    return MTG_OK;
}
int mtg_index_contains(const mtg_index* idx, const uint64_t* kmers, size_t n, uint8_t* out)
{
    std::vector<uint32_t> ab(n);
    int rc = mtgi::query_run(idx, kmers, n, ab.data(), nullptr, nullptr);
    if (rc) return rc;
    for (size_t i = 0; i < n; i++) out[i] = ab[i] != 0;
    return MTG_OK;
}
int mtg_index_abundance(const mtg_index* idx, const uint64_t* kmers, size_t n, uint32_t* out) { return mtgi::query_run(idx, kmers, n, out, nullptr, nullptr); }
int mtg_index_neighbors(const mtg_index* idx, const uint64_t* kmers, size_t n, uint8_t* succ, uint8_t* pred)
{
    return mtgi::query_run(idx, kmers, n, nullptr, succ, pred);
}
int mtg_index_scan_packed_device(const mtg_index* idx, const uint64_t* d_words, const uint64_t* d_word_off, const uint32_t* d_len, size_t nseq, int mode,
                                 uint64_t* d_out_bits, mtg_scan_stats* st)
{
    if (!d_words || !d_word_off || !d_len || !d_out_bits) { mtgi::set_error("null argument"); return MTG_ERR_ARG; }
    return mtgi::scan_run(idx, d_words, 0, d_word_off, d_len, nseq, mode, d_out_bits, 1, st);
}
int mtg_last_batch_stats(mtg_batch_stats* s)
{
    if (!s) return MTG_ERR_ARG;
    *s = mtgi::g_stats;
    return MTG_OK;
}
int mtg_bench_random_lines(uint64_t table_bytes, uint64_t n_chains, uint32_t chain_len, uint32_t line_bytes, double* ms, double* gbps)
{
    return mtgi::bench_random_lines(table_bytes, n_chains, chain_len, line_bytes, ms, gbps);
}
}

